"""CPU: round-trip scoring without a device -- the two facppg_ppg_dtw symbols in header and library, every host-side refusal of
the entry point (nothing is launched: no device is needed), the float64 reference of score_helpers.py against its float32
restatement over the whole GPU matrix (every case must be decidable: the three integers agree), and the corpus script's
refusal of --score_file with --ppg_list."""
import ctypes
import os
import re

import numpy as np
import pytest

import score_helpers as sh
from conftest import ROOT
from facppg import lib as flib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def test_header_declares_and_library_exports_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facppg.h")).read(), flags=re.S)
    L = flib.load()
    for name in ("facppg_ppg_dtw_workspace_bytes", "facppg_ppg_dtw"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in flib.exported_symbols()
    assert L.facppg_version() == 103


def _call(L, B=2, D=40, Ta_max=8, Tb_max=9, band=0, la=(8, 3), lb=(9, 1), ws_bytes=None, null=None):
    """facppg_ppg_dtw with made-up device addresses: every refusal comes before the first launch, so none is touched."""
    fake = lambda k: ctypes.c_void_p(0 if null == k else 0x1000 * (k + 1))    # noqa: E731
    la_h, lb_h = flib.offsets_array(la), flib.offsets_array(lb)
    if ws_bytes is None:
        ws_bytes = L.facppg_ppg_dtw_workspace_bytes(max(B, 1), max(D, 1), max(Ta_max, 1), max(Tb_max, 1), band) or 1 << 20
    rc = L.facppg_ppg_dtw(fake(0), fake(1), None if null == "la_host" else la_h, Ta_max, fake(2), fake(3), None if null == "lb_host" else lb_h,
                          Tb_max, B, D, band, fake(4), fake(5), fake(6), fake(7), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def test_host_side_refusals():
    L = flib.load()
    for null in list(range(8)) + ["la_host", "lb_host"]:
        rc, msg = _call(L, null=null)
        assert rc == EINVAL and "NULL argument" in msg, (null, rc, msg)
    for kw, value in ((dict(B=0, la=(), lb=()), "got 0, 40, 8, 9"), (dict(D=0), "got 2, 0, 8, 9"), (dict(Ta_max=0), "got 2, 40, 0, 9"),
                      (dict(Tb_max=-3), "got 2, 40, 8, -3")):
        rc, msg = _call(L, **kw)
        assert rc == EINVAL and "must be positive" in msg and value in msg, (kw, rc, msg)
    for band in (1, -1, -40):
        rc, msg = _call(L, band=band)
        assert rc == EINVAL and "band must be 0" in msg and "got %d" % band in msg, (band, rc, msg)
    for kw, value in ((dict(la=(8, 0)), "pair 1: a has 0 frames"), (dict(la=(9, 3)), "pair 0: a has 9 frames"), (dict(lb=(9, 10)), "pair 1: b has 10 frames"),
                      (dict(lb=(-2, 1)), "pair 0: b has -2 frames")):
        rc, msg = _call(L, **kw)
        assert rc == EINVAL and value in msg, (kw, rc, msg)
    rc, msg = _call(L, D=257)
    assert rc == EUNSUPPORTED and "got 257" in msg and "monophone" in msg, (rc, msg)
    many = 65536
    rc, msg = _call(L, B=many, la=(1,) * many, lb=(1,) * many, Ta_max=1, Tb_max=1)
    assert rc == EUNSUPPORTED and "65535" in msg and "got 65536" in msg, (rc, msg)
    need = L.facppg_ppg_dtw_workspace_bytes(2, 40, 8, 9, 0)
    assert need > 0
    rc, msg = _call(L, ws_bytes=need - 1)
    assert rc == EWORKSPACE and str(need - 1) in msg and str(need) in msg, (rc, msg)
    # the workspace holds at least the square roots and the admissible distances
    assert need >= 4 * 2 * (40 * (8 + 9) + 8 * 9)
    assert L.facppg_ppg_dtw_workspace_bytes(0, 40, 8, 9, 0) == 0 and "got 0, 40, 8, 9" in L.facppg_last_error().decode()


def test_python_refusals_need_no_device():
    import torch
    from facppg import score
    from facppg.lib import FacppgError
    with pytest.raises(FacppgError, match="must be a GPU tensor"):
        score.ppg_dtw(torch.zeros(1, 4, 3), [3], torch.zeros(1, 4, 3), [3])

    class Deps(object):
        nnet, lda, monophone_trans = object(), object(), None
    with pytest.raises(FacppgError, match="monophone_trans"):
        score.roundtrip([object()], [np.zeros(160, np.float32)], 16000, Deps())
    with pytest.raises(FacppgError, match="no PPG dependencies"):
        score.roundtrip([object()], [np.zeros(160, np.float32)], 16000, None)


def test_reference_hand_example():
    """Two frames each, three classes: checked by hand.  a's frames are classes 0, 1; b's are 0, 0 -> the path (0,0), (1,1) by the
    diagonal-first rule only if it is cheapest; here C(1,1) = d(1,1) + min(d(0,0), C(0,1), C(1,0))."""
    a = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], dtype=np.float32)
    b = np.array([[1.0, 1.0], [0.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    # d = [[0, 0], [1, 1]]: C(0,0) = 0, C(0,1) = 0, C(1,0) = 1, C(1,1) = 1 + min(0 (diag), 0 (up, a tie: the diagonal stays), 1) = 1
    assert sh.reference(a, b) == (1.0, 2, 1)
    # identical sequences: the diagonal, every cell agrees
    assert sh.reference(a, a) == (0.0, 2, 2)
    # all ties (D = 1): the diagonal first, then whatever is left along the edge
    one = np.ones((1, 3), dtype=np.float32)
    assert sh.reference(one, np.ones((1, 5), dtype=np.float32)) == (0.0, 5, 5)
    assert sh.reference(one, one, band=2) == (0.0, 3, 3)


def test_band_corners_and_paths():
    for Ta, Tb in sh.SHAPES:
        for band in (2, 40):
            ok = sh.admissible(Ta, Tb, band)
            assert ok[0, 0] and ok[Ta - 1, Tb - 1], (Ta, Tb, band)
    assert not sh.admissible(64, 64, 2)[0, 3] and sh.admissible(64, 64, 2)[0, 2]


def test_every_case_of_the_matrix_is_decidable():
    """The float64 reference and its float32 restatement (d and every sum in NumPy float32, k in increasing order) agree on steps
    and agree for all 72 cases; D = 1 costs exactly 0 in both; the restatement's worst deviation per path cell is what the GPU
    test's tolerance is 4 x of."""
    assert len(sh.MATRIX) == 72
    undecidable, worst = [], (0.0, None)
    for c in sh.MATRIX:
        r64, r32 = sh.case(*c)
        if r64[1:] != r32[1:]:
            undecidable.append((c, r64, r32))
        if c[2] == 1:
            assert r64[0] == 0.0 and r32[0] == 0.0, c
        dev = abs(r32[0] - r64[0]) / r64[1]
        if dev > worst[0]:
            worst = (dev, c)
        Ta, Tb = c[:2]
        assert max(Ta, Tb) <= r64[1] <= Ta + Tb - 1 and 0 <= r64[2] <= r64[1], (c, r64)
    print("float32 restatement: worst |cost32 - cost64| / steps = %.3e at (Ta, Tb, D, band) = %s; tolerance %.3e per cell" % (
        worst[0], worst[1], sh.cost_tolerance()))
    assert not undecidable, undecidable          # cap: no case of the matrix may be undecidable
    assert worst[0] == sh.emulation_deviation() > 0.0


def test_score_file_with_ppg_list_is_refused_at_parse_time(capsys):
    from script import synthesize_corpus
    base = ["--ppg2mel_model", "t.pt", "--waveglow_model", "w.pt", "--output_dir", "out"]
    with pytest.raises(SystemExit) as e:
        synthesize_corpus.parse(base + ["--ppg_list", "ppgs.txt", "--score_file", "scores.tsv"])
    assert e.value.code == 2 and "no teacher audio" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(base + ["--wav_list", "wavs.txt", "--score_file", "scores.tsv", "--score_band", "1"])
    args = synthesize_corpus.parse(base + ["--wav_list", "wavs.txt", "--score_file", "scores.tsv", "--score_band", "60"])
    assert args.score_file == "scores.tsv" and args.score_band == 60
    plain = synthesize_corpus.parse(base + ["--wav_list", "wavs.txt"])
    assert plain.score_file is None and plain.score_band == 0
