"""CPU: the host side of long-form conversion -- facppg.longform.plan_segments (the worked example, its edge cases, a seeded
property loop), the grouping rule, every refusal of the planner and of synthesize_long / synthesize_long_wavs / the stream
jobs before any device work, and the three new symbols in header and binding (test_abi_cpu.py holds the library to them)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def _flags(T, runs):
    f = np.zeros(T, dtype=np.uint8)
    for a, b in runs:
        f[a:b] = 1
    return f


def _covers(plan, T):
    s = 0
    for start, frames in plan:
        assert start == s and frames >= 1
        s += frames
    assert s == T


def test_worked_example():
    from facppg.longform import pause_runs, plan_segments
    f = _flags(97, [(20, 23), (30, 37), (60, 62), (70, 75)])
    assert pause_runs(f, 3) == [(20, 23), (30, 37), (70, 75)]
    assert plan_segments(f, 40, 10, 3) == [(0, 33), (33, 39), (72, 25)]
    assert plan_segments(torch.from_numpy(f), 40, 10, 3) == [(0, 33), (33, 39), (72, 25)]


def test_short_recording_is_one_segment():
    from facppg.longform import plan_segments
    assert plan_segments(_flags(40, [(10, 20)]), 40, 10, 3) == [(0, 40)]
    assert plan_segments(_flags(1, []), 40, 10, 3) == [(0, 1)]
    assert plan_segments(_flags(0, []), 40, 10, 3) == []


def test_forced_cuts_without_pauses():
    from facppg.longform import plan_segments
    # s + max_frames each time; at s = 80 (45 frames left) the window ends at T - min_frames = 115, not at s + max_frames = 120
    assert plan_segments(_flags(125, []), 40, 10, 3) == [(0, 40), (40, 40), (80, 35), (115, 10)]
    assert plan_segments(_flags(85, []), 40, 10, 3) == [(0, 40), (40, 35), (75, 10)]


def test_short_run_is_ignored():
    from facppg.longform import plan_segments
    assert plan_segments(_flags(60, [(24, 26)]), 40, 10, 3) == [(0, 40), (40, 20)]       # forced
    assert plan_segments(_flags(60, [(24, 27)]), 40, 10, 3) == [(0, 25), (25, 35)]       # long enough: cut at (24 + 27) // 2


def test_tie_goes_to_the_later_run():
    from facppg.longform import plan_segments
    assert plan_segments(_flags(60, [(12, 16), (30, 34)]), 40, 10, 3) == [(0, 32), (32, 28)]
    # (the longer run wins over the later one)
    assert plan_segments(_flags(60, [(12, 17), (30, 34)]), 40, 10, 3)[0] == (0, 14)
    # a run whose cut lies outside the window does not count, however long
    assert plan_segments(_flags(60, [(0, 12), (30, 34)]), 40, 10, 3)[0] == (0, 32)


def test_planner_properties():
    from facppg.longform import plan_segments
    g = np.random.Generator(np.random.PCG64(5))
    for _ in range(3000):
        T = int(g.integers(0, 400))
        mn = int(g.integers(1, 30))
        mx = int(g.integers(2 * mn, 2 * mn + 60))
        mp = int(g.integers(1, 8))
        p = float(g.choice([0.0, 0.05, 0.3, 0.7, 1.0]))
        f = np.repeat(g.random(T // 3 + 1) < p, 3)[:T].astype(np.uint8) if g.random() < 0.5 else (g.random(T) < p).astype(np.uint8)
        plan = plan_segments(f, mx, mn, mp)
        _covers(plan, T)
        assert all(n <= mx for _, n in plan), (T, mx, mn, mp, plan)
        if len(plan) > 1:
            assert all(n >= mn for _, n in plan), (T, mx, mn, mp, plan)


def test_planner_refusals():
    from facppg.lib import FacppgError
    from facppg.longform import plan_segments
    f = _flags(97, [])
    with pytest.raises(FacppgError, match="min_frames must be at least 1"):
        plan_segments(f, 40, 0, 3)
    with pytest.raises(FacppgError, match="max_frames must be at least 2 \\* min_frames"):
        plan_segments(f, 19, 10, 3)
    with pytest.raises(FacppgError, match="min_pause must be at least 1"):
        plan_segments(f, 40, 10, 0)
    assert plan_segments(f, 20, 10, 1)[0] == (0, 20)


def test_grouping():
    from facppg.longform import group_segments
    assert group_segments([33, 39, 25], 640) == [(0, 3)]
    assert group_segments([33, 39, 25], 40) == [(0, 1), (1, 2), (2, 3)]
    assert group_segments([33, 39, 25], 78) == [(0, 2), (2, 3)]         # 2 * 39 = 78 fits, 3 * 39 does not
    assert group_segments([33, 39, 25], 1) == [(0, 1), (1, 2), (2, 3)]  # at least one each
    assert group_segments([10, 10, 50, 10], 100) == [(0, 2), (2, 4)]    # the third would make it 3 * 50
    assert group_segments([], 100) == []


# ---- the pipeline's refusals come before any device work

class _Decoder(object):
    max_decoder_steps = 1000


class _Taco(object):
    """As much of Tacotron2 as the argument checks read; asking for its parameters is a step towards the device."""
    _hp = {"n_symbols": 40}
    decoder = _Decoder()

    def parameters(self):
        raise AssertionError("device work was reached")


class _Deps(object):
    nnet = lda = monophone_trans = None


def _never(*a, **kw):
    raise AssertionError("device work was reached")


@pytest.fixture
def no_device(monkeypatch):
    from facppg import pipeline
    from ppg import compute_ppg
    for name in ("_synthesize_long", "pad_ppgs", "pause_flags", "_synthesize", "_acoustic", "_acoustic_stream"):
        monkeypatch.setattr(pipeline, name, _never)
    monkeypatch.setattr(compute_ppg, "compute_ppg_padded", _never)
    monkeypatch.setattr(compute_ppg, "_feat_for_nnet_flat", _never)


def test_synthesize_long_argument_errors_come_first(no_device):
    from facppg import pipeline
    from facppg.lib import FacppgError
    ppg40 = [np.zeros((97, 40), dtype=np.float32)]
    batch40 = (torch.zeros(1, 40, 97), [97])               # a CPU tensor in the device batch's place
    for p in (ppg40, batch40):
        for fade in (48, -1, 8192, 3, 1.5, "64"):
            with pytest.raises(FacppgError, match="seam_fade"):
                pipeline.synthesize_long(p, _Taco(), None, seam_fade=fade)
        for thr in (0.0, 1.0, -0.2, 1.5, float("nan")):
            with pytest.raises(FacppgError, match="pause_threshold"):
                pipeline.synthesize_long(p, _Taco(), None, pause_threshold=thr)
        with pytest.raises(FacppgError, match="max_frames must be at least 2 \\* min_frames"):
            pipeline.synthesize_long(p, _Taco(), None, max_frames=299, min_frames=150)
        with pytest.raises(FacppgError, match="min_frames must be at least 1"):
            pipeline.synthesize_long(p, _Taco(), None, min_frames=0)
        with pytest.raises(FacppgError, match="min_pause must be at least 1"):
            pipeline.synthesize_long(p, _Taco(), None, min_pause=0)
        with pytest.raises(FacppgError, match="max_frames=1001 is above the model's max_decoder_steps \\(1000\\)"):
            pipeline.synthesize_long(p, _Taco(), None, max_frames=1001)
        with pytest.raises(FacppgError, match="vocoder_arithmetic"):
            pipeline.synthesize_long(p, _Taco(), None, vocoder_arithmetic="fp8")
        with pytest.raises(FacppgError, match="pause_rows must be at least one row in \\[0, 40\\)"):
            pipeline.synthesize_long(p, _Taco(), None, pause_rows=[40])
        with pytest.raises(FacppgError, match="pause_rows must be at least one row"):
            pipeline.synthesize_long(p, _Taco(), None, pause_rows=[])
    # a threshold of 1.5 is inside (0, 2) for two rows: the call gets past its checks (and would touch the device next)
    with pytest.raises(AssertionError, match="device work was reached"):
        pipeline.synthesize_long(ppg40, _Taco(), None, pause_rows=[38, 39], pause_threshold=1.5)
    for p in ([np.zeros((97, 5816), dtype=np.float32)], (torch.zeros(1, 5816, 9), [9])):
        with pytest.raises(FacppgError, match="pause_rows is needed for PPGs of 5816 symbols"):
            pipeline.synthesize_long(p, _Taco(), None)
    for p in ([], None, (torch.zeros(1, 40, 9), [10]), (torch.zeros(1, 40, 9), [9, 9]), (torch.zeros(40, 9), [9])):
        with pytest.raises(FacppgError, match="non-empty list|a device batch is"):
            pipeline.synthesize_long(p, _Taco(), None)
    with pytest.raises(TypeError):
        pipeline.synthesize_long(ppg40, _Taco(), None, None, [39])         # the settings are keyword-only


def test_synthesize_long_wavs_argument_errors_come_first(no_device):
    from facppg import pipeline
    from facppg.lib import FacppgError
    wav = object()
    with pytest.raises(FacppgError, match="non-empty list"):
        pipeline.synthesize_long_wavs([], _Deps(), _Taco(), None)
    with pytest.raises(FacppgError, match="no PPG dependencies"):
        pipeline.synthesize_long_wavs([wav], None, _Taco(), None)
    with pytest.raises(FacppgError, match="no acoustic model"):
        pipeline.synthesize_long_wavs([wav], _Deps(), _Taco(), None)
    s = pipeline.Synthesizer.__new__(pipeline.Synthesizer)        # (the constructor loads checkpoints onto the GPU)
    s.tacotron, s.waveglow, s.denoiser, s.vocoder_arithmetic, s.vocoder_stream = _Taco(), None, None, None, None
    with pytest.raises(FacppgError, match="non-empty list"):
        s.convert_long([], _Deps())
    with pytest.raises(FacppgError, match="no acoustic model"):
        s.convert_long([wav], _Deps(), seam_fade=48)


def test_long_wavs_checks_behind_the_dependencies(no_device, monkeypatch):
    """With dependencies that pass _checked_wavs: the senone default of pause_rows and the shared checks."""
    from facppg import pipeline
    from facppg.lib import FacppgError

    class Taco(_Taco):
        _hp = {"n_symbols": 5816}
    seen = {}

    def checked(wavs, deps, tacotron, is_full_ppg, what, ppgs=None):
        return seen["full"]
    monkeypatch.setattr(pipeline, "_checked_wavs", checked)
    deps = _Deps()
    seen["full"] = True
    with pytest.raises(FacppgError, match="pause_rows is needed for senone PPGs"):
        pipeline.synthesize_long_wavs([object()], deps, Taco(), None)
    with pytest.raises(FacppgError, match="seam_fade"):
        pipeline.synthesize_long_wavs([object()], deps, Taco(), None, pause_rows=[3, 5], seam_fade=48)
    trans = torch.zeros(40, 5816)
    trans[39, [17, 4000, 5]] = 1.0
    trans[38, 9] = 1.0
    deps.monophone_trans = trans
    got = {}
    monkeypatch.setattr(pipeline, "_checked_long", lambda taco, D, what, rows, *a: got.update(rows=rows, D=D) or _never())
    with pytest.raises(AssertionError):
        pipeline.synthesize_long_wavs([object()], deps, Taco(), None)
    assert got == {"rows": [5, 17, 4000], "D": 5816}
    seen["full"] = False
    with pytest.raises(AssertionError):
        pipeline.synthesize_long_wavs([object()], deps, _Taco(), None)
    assert got == {"rows": [39], "D": 40}


def test_the_fixture_maps_ten_senones_to_sil():
    """What synthesize_long_wavs reads its senone pause rows from: row 39 (``sil``) of the reference's pdf -> monophone matrix
    has ten unit weights."""
    from common import feat
    from test_feat_cpu import KF
    trans = feat.read_sparse_mat(os.path.join(KF, "reduce_dim.mat"))
    row = trans[39]
    cols = torch.nonzero(row).flatten()
    assert trans.shape == (40, 5816) and cols.numel() == 10 and bool((row[cols] == 1.0).all())


def test_stream_job_with_two_sources_is_refused(no_device):
    from facppg import pipeline
    from facppg.lib import FacppgError
    x = (torch.zeros(1, 40, 9), [9])
    ppgs = [np.zeros((9, 40), dtype=np.float32)]
    for job, names in ((dict(ppgs=ppgs, prepared=x), "ppgs and prepared"), (dict(wavs=[object()], prepared=x), "wavs and prepared"),
                       (dict(ppgs=ppgs, wavs=[object()]), "ppgs and wavs"), (dict(ppgs=ppgs, wavs=[object()], prepared=x), "ppgs and wavs and prepared")):
        with pytest.raises(FacppgError, match="both %s given" % names):
            list(pipeline.synthesize_stream([job], _Taco(), None))
    assert list(pipeline.synthesize_stream([], _Taco(), None)) == []


def test_header_and_binding_know_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "facppg.h")).read()
    want = {
        "facppg_ppg_pause_flags": ["x_dev", "lengths_dev", "B", "K", "Tmax", "rows_dev", "rows_host", "n_rows", "threshold", "flags_dev", "stream"],
        "facppg_ppg_gather_segments": ["x_dev", "B", "K", "Tmax", "table_dev", "table_host", "S", "Lmax", "y_dev", "stream"],
        "facppg_join_segments": ["audio_dev", "Nmax", "n_dev", "n_host", "S", "fade", "out_dev", "stream"],
    }
    from facppg import lib as flib
    L = flib.load()
    for name, names in want.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "include/facppg.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
        assert name in flib.exported_symbols() and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(names)
    assert "Reached max decoder steps" in src and "NO counterpart" in src
    assert L.facppg_version() == 103


def test_abi_refusals_need_no_device():
    """The three entry points validate before they launch: with host memory in the pointers' places a refusal comes back as an
    error code and nothing runs."""
    import ctypes
    from facppg import lib as flib
    L = flib.load()
    buf = (ctypes.c_float * 16)()
    i3 = flib.offsets_array
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.facppg_ppg_pause_flags(p, p, 1, 4, 4, p, i3([0]), 0, 0.5, p, None) == -1 and b"n_rows" in L.facppg_last_error()
    assert L.facppg_ppg_pause_flags(p, p, 1, 4, 4, p, i3([4]), 1, 0.5, p, None) == -1 and b"outside [0, 4)" in L.facppg_last_error()
    assert L.facppg_ppg_pause_flags(p, p, 1, 4, 4, p, i3([0, -1]), 2, 0.5, p, None) == -1
    for thr in (0.0, 2.0, -1.0, float("nan")):
        assert L.facppg_ppg_pause_flags(p, p, 1, 4, 4, p, i3([0, 3]), 2, thr, p, None) == -1 and b"threshold" in L.facppg_last_error()
    for seg in ((0, 2, 3), (0, 0, 0), (0, 0, 4), (1, 0, 1), (-1, 0, 1), (0, -1, 2)):      # Tmax 4, Lmax 3, B 1
        assert L.facppg_ppg_gather_segments(p, 1, 2, 4, p, i3(seg), 1, 3, p, None) == -1, seg
    assert L.facppg_ppg_gather_segments(p, 1, 2, 4, p, None, 1, 3, p, None) == -1
    for fade in (48, -2, 8192, 3):
        assert L.facppg_join_segments(p, 4, p, i3([4, 4]), 2, fade, p, None) == -1 and b"power of two" in L.facppg_last_error()
    assert L.facppg_join_segments(p, 4, p, i3([4, 5]), 2, 64, p, None) == -1
    assert L.facppg_join_segments(p, 4, p, i3([4, 4]), 0, 64, p, None) == -1
