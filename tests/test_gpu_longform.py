"""GPU: long recordings end to end (facppg.pipeline.synthesize_long / synthesize_long_wavs, Synthesizer.convert_long_file, the
``prepared`` jobs of synthesize_stream) against what a caller had to write by hand: the same cuts on host copies of the PPG,
synthesize_stream over ``ppgs`` jobs, a NumPy join.

Everything is an equality of samples.  A group of segments reaches the acoustic model as the batch pad_ppgs would have built
from its host slices (facppg_ppg_gather_segments copies), with the same seeds, step limits and keywords, through the same
pipelined path; the join's gains are exact.  Two GROUPINGS of the same segments need not agree bit for bit (other launch
shapes): their difference is measured and printed, not bounded (measured on an MI355X: relative RMS 0.0, the two agree).  Models, acoustic model and wavs are those of
test_gpu_wav2wav.py / test_gpu_ppg_batch.py; every call runs under test_gpu_wav2wav.py's co-tenancy environment, and
limit_to_input=True with the never-stopping gate bias makes every length that of the input."""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

from longform_helpers import join, pause_flags
from stream_helpers import acoustic, make_vocoder
from test_gpu_ppg_batch import FRAMES, WAVS, _wave_data, world  # noqa: F401  (the module fixture, built once for this file)
from test_gpu_wav2wav import _cotenancy, _host_rows, mono  # noqa: F401

pytestmark = pytest.mark.gpu

RUNS = [(20, 23), (30, 37), (60, 62), (70, 75)]          # the planner's worked example: T = 97, (max, min, pause) = (40, 10, 3)
PLAN = dict(max_frames=40, min_frames=10, min_pause=3)
TABLE_97 = [(0, 33, 33), (33, 39, 39), (72, 25, 25)]
SEED = 31


def _ppg(T, runs, seed):
    """[T, 40] rows that sum to one: ``sil`` (column 39) 0.9 on the runs and 0.02 elsewhere, the rest spread at random."""
    g = np.random.Generator(np.random.PCG64(seed))
    sil = np.full(T, 0.02, dtype=np.float32)
    for a, b in runs:
        sil[a:b] = 0.9
    rest = g.random((T, 39)).astype(np.float32) + np.float32(0.05)
    rest = rest / rest.sum(axis=1, keepdims=True) * (1.0 - sil)[:, None]
    return np.concatenate([rest, sil[:, None]], axis=1).astype(np.float32)


def _by_hand(s, ppg, groups, first_seed):
    """The parent commit's way: host slices of every group as ``ppgs`` jobs of synthesize_stream, seeds first_seed + 2 j in
    pooled order, step limits the frame counts -> the segments' samples in order."""
    jobs, j = [], 0
    for group in groups:
        jobs.append(dict(ppgs=[ppg[a:a + n] for a, n in group], utterance_seeds=[first_seed + 2 * (j + i) for i in range(len(group))],
                         step_limits=[n for _, n in group]))
        j += len(group)
    out = []
    for wavs, tout in s.stream(jobs, return_device=False):
        out += wavs
    return out


@pytest.fixture(scope="module")
def alone(mono):
    """The 97-frame recording (default grouping: its three segments in one batch) and the 37-frame one (one segment, the seed it
    gets as pooled segment 3), each converted on its own: shared by the tests below, never written to."""
    from facppg import pipeline
    s = mono["synthesizer"]
    p97, p37 = _ppg(97, RUNS, 1), _ppg(37, [(5, 9)], 2)
    mp = pytest.MonkeyPatch()
    _cotenancy(mp)
    try:
        w97, t97 = pipeline.synthesize_long([p97], s.tacotron, s.waveglow, s.denoiser, seed=SEED, limit_to_input=True, **PLAN)
        w37, t37 = pipeline.synthesize_long([p37], s.tacotron, s.waveglow, s.denoiser, seed=SEED + 6, limit_to_input=True, **PLAN)
    finally:
        mp.undo()
    for w in (w97[0], w37[0]):
        w.setflags(write=False)
    return dict(p97=p97, p37=p37, w97=w97[0], t97=t97[0], w37=w37[0], t37=t37[0])


@pytest.mark.parametrize("batch_frames", [None, 40])
def test_monophone_recording_equals_the_hand_written_conversion(mono, alone, monkeypatch, batch_frames):
    from facppg import pipeline
    _cotenancy(monkeypatch)
    s, ppg = mono["synthesizer"], alone["p97"]
    segs = [(a, n) for a, n, _ in TABLE_97]
    if batch_frames is None:
        out, table, groups = alone["w97"], alone["t97"], [segs]                 # one group of three
    else:
        (out,), (table,) = pipeline.synthesize_long([ppg], s.tacotron, s.waveglow, s.denoiser, seed=SEED, limit_to_input=True,
                                                    batch_frames=batch_frames, **PLAN)
        groups = [[g] for g in segs]                                            # three groups of one
    assert table == TABLE_97
    assert out.dtype == np.float32 and out.shape == (97 * 160,) and np.isfinite(out).all()
    ref = join(_by_hand(s, ppg, groups, SEED), 64)
    assert ref.shape == out.shape and np.array_equal(out, ref)
    if batch_frames is not None:
        other = alone["w97"]
        assert other.shape == out.shape and np.isfinite(other).all()
        d = out.astype(np.float64) - other
        print("grouping 3x1 against 1x3: relative RMS difference %.3e, max abs %.3e" % (
            np.sqrt((d * d).mean() / (other.astype(np.float64) ** 2).mean()), np.abs(d).max()))


def test_short_recording_is_one_segment(mono, alone, monkeypatch):
    _cotenancy(monkeypatch)
    s = mono["synthesizer"]
    assert alone["t37"] == [(0, 37, 37)] and alone["w37"].shape == (37 * 160,)
    (ref,) = _by_hand(s, alone["p37"], [[(0, 37)]], SEED + 6)
    assert np.array_equal(alone["w37"], ref)                 # (one segment has no seam: the join is a copy)


def test_two_recordings_are_pooled(mono, alone, monkeypatch):
    """97 and 37 frames in one call: pooled segments 0-2 and 3, seeds SEED + 2 j.  batch_frames = 3 * 39 keeps the groups of the
    recordings converted alone -- (33, 39, 25) and (37) -- so each waveform must be the one it was there."""
    from facppg import pipeline
    _cotenancy(monkeypatch)
    s = mono["synthesizer"]
    kw = dict(seed=SEED, limit_to_input=True, batch_frames=117, **PLAN)
    out, tables = pipeline.synthesize_long([alone["p97"], alone["p37"]], s.tacotron, s.waveglow, s.denoiser, **kw)
    assert tables == [TABLE_97, [(0, 37, 37)]]
    assert np.array_equal(out[0], alone["w97"]) and np.array_equal(out[1], alone["w37"])
    # the same as ONE device batch, waveforms left on the device
    x, lens = pipeline.pad_ppgs([alone["p97"], alone["p37"]], device="cuda")
    dev, tables_d = pipeline.synthesize_long((x, lens), s.tacotron, s.waveglow, s.denoiser, return_device=True, **kw)
    assert tables_d == tables and all(w.is_cuda for w in dev)
    assert np.array_equal(dev[0].cpu().numpy(), alone["w97"]) and np.array_equal(dev[1].cpu().numpy(), alone["w37"])


def test_senone_wavs_equal_long_over_the_padded_posteriors(world, monkeypatch):
    """The 150-frame wav at hop 256 with (max, min, pause) = (60, 20, 2): pause rows from the fixture's reduce_dim.mat, the
    threshold the median of their mass on this (random) acoustic model, so that both flag values occur."""
    import ppg
    from facppg import pipeline
    _cotenancy(monkeypatch)
    deps = world["deps"]
    _, wg, den = make_vocoder()
    _, taco = acoustic(150, -10.0)
    wd = _wave_data(world["wavs"])[3:]
    rows = [int(c) for c in torch.nonzero(deps.monophone_trans[39]).flatten()]
    assert len(rows) == 10
    x, lens = ppg.compute_ppg_padded(wd, deps)
    assert lens == [150] and tuple(x.shape) == (1, 5816, 150)
    xh = x.cpu().numpy()
    mass = xh[0, rows, :].astype(np.float64).sum(axis=0)
    thr = float(np.float32(np.median(mass)))
    flags = pipeline.pause_flags(x, lens, rows, thr).cpu().numpy()
    want = pause_flags(xh, lens, rows, thr)
    print("pause mass: median %.3e, %d of 150 frames flagged" % (thr, int(want.sum())))
    assert np.array_equal(flags, want) and 0 < want.sum() < 150
    # (groups of at most three segments: the co-tenancy decoder shape holds a bounded number of utterances)
    kw = dict(max_frames=60, min_frames=20, min_pause=2, pause_threshold=thr, seed=SEED, limit_to_input=True, batch_frames=60)
    ref, tables_ref = pipeline.synthesize_long(_host_rows(x, lens), taco, wg, den, pause_rows=rows, **kw)
    out, tables = pipeline.synthesize_long_wavs(wd, deps, taco, wg, den, **kw)           # pause_rows from deps, senone by n_symbols
    from facppg.longform import plan_segments
    assert [(a, n) for a, n, _ in tables[0]] == plan_segments(want[0], 60, 20, 2)
    assert tables == tables_ref and len(tables[0]) >= 3 and sum(n for _, n, _ in tables[0]) == 150
    assert all(t == n for _, n, t in tables[0])
    assert out[0].shape == ref[0].shape == (150 * 256,) and np.isfinite(out[0]).all() and np.array_equal(out[0], ref[0])
    with pytest.raises(pipeline_error(), match="pause_rows is needed for PPGs of 5816 symbols"):
        pipeline.synthesize_long(_host_rows(x, lens), taco, wg, den, **kw)
    with pytest.raises(pipeline_error(), match="max_frames=151 is above the model's max_decoder_steps \\(150\\)"):
        pipeline.synthesize_long_wavs(wd, deps, taco, wg, den, max_frames=151, min_frames=20)


def pipeline_error():
    from facppg.lib import FacppgError
    return FacppgError


def test_convert_long_file_and_convert_file_still_truncates(world, mono, monkeypatch, capsys):
    _cotenancy(monkeypatch)
    monkeypatch.setenv("FACPPG_STREAM", "0")
    s, deps, tmp = mono["synthesizer"], world["deps"], world["tmp"]
    plan = dict(max_frames=60, min_frames=20, min_pause=2, batch_frames=60)
    src = world["paths"][3]                                   # 24 000 samples at 16 kHz: 150 frames
    table = s.convert_long_file(src, str(tmp / "long.wav"), 16000, ppg_deps=deps, seed=SEED, limit_to_input=True, **plan)
    assert len(table) >= 3 and [a for a, _, _ in table] == list(np.cumsum([0] + [n for _, n, _ in table[:-1]]))
    assert sum(n for _, n, _ in table) == 150 and all(t == n for _, n, t in table)
    fs, a = wavfile.read(str(tmp / "long.wav"))
    assert fs == 16000 and a.dtype == np.float32 and a.shape == (sum(t for _, _, t in table) * 160,) and np.isfinite(a).all()     # ([N, 1] was written: one channel)
    # the same call through convert_long: the same samples
    (again,), (table2,) = s.convert_long(_wave_data(world["wavs"])[3:], deps, seed=SEED, limit_to_input=True, **plan)
    assert table2 == table and np.array_equal(again, a)
    # convert_file keeps cutting a recording off at max_decoder_steps, as the reference does
    monkeypatch.setattr(s.tacotron.decoder, "max_decoder_steps", 100)
    capsys.readouterr()
    tout = s.convert_file(src, str(tmp / "cut.wav"), 16000, ppg_deps=deps)
    assert tout == 100 and "Reached max decoder steps" in capsys.readouterr().out
    fs, cut = wavfile.read(str(tmp / "cut.wav"))
    assert fs == 16000 and cut.shape == (100 * 160,)
