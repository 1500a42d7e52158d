"""CPU: free-running validation without a device -- the four symbols of csrc/facppg_mcd.hip in header, library and binding, every
host-side refusal of the two entry points (nothing is launched: no device is needed), cepstral_basis, the float64 reference of
mcd_helpers.py against its float32 restatement over the whole GPU matrix (every case must be decidable: the steps agree), the
reference's own properties, and the argument refusals of validate_free_running, finetune(free_running=True) and
script.validate_ppg2mel.

Measured here: the float32 restatement's worst |cost32 - cost64| / steps over the 72 cases is 8.952e-6 (at Ta, Tb, M, K, band =
257, 300, 80, 64, 2; a cell costs about 2.4 there), so the GPU tests' tolerance is 4 x that = 3.581e-5 per path cell
(mcd_helpers.cost_tolerance; the test prints both).  Most of it is the projection: 80 products of about 0.16 x -5 each, rounded
one by one in NumPy, where the device's fma chain rounds once per term."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mcd_helpers as mh
from conftest import ROOT
from facppg import lib as flib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
SYMBOLS = ("facppg_mel_dtw_workspace_bytes", "facppg_mel_dtw", "facppg_attention_path_workspace_bytes", "facppg_attention_path")


def test_header_library_and_binding_know_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facppg.h")).read(), flags=re.S)
    L = flib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in flib.exported_symbols()
    assert L.facppg_version() == 103


def _fake(k, null):
    return ctypes.c_void_p(0 if null == k else 0x1000 * (k + 1))


def _dtw(L, B=2, M=80, K=13, Ta_max=8, Tb_max=9, band=0, la=(8, 3), lb=(9, 1), ws_bytes=None, null=None):
    """facppg_mel_dtw with made-up device addresses: every refusal comes before the first launch, so none is touched."""
    la_h, lb_h = flib.offsets_array(la), flib.offsets_array(lb)
    if ws_bytes is None:
        ws_bytes = L.facppg_mel_dtw_workspace_bytes(max(B, 1), max(M, 1), max(K, 1), max(Ta_max, 1), max(Tb_max, 1), band) or 1 << 20
    rc = L.facppg_mel_dtw(_fake(0, null), _fake(1, null), None if null == "la_host" else la_h, Ta_max, _fake(2, null), _fake(3, null),
                          None if null == "lb_host" else lb_h, Tb_max, B, M, _fake(4, null), K, band, _fake(5, null), _fake(6, null), _fake(7, null),
                          ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def test_mel_dtw_host_side_refusals():
    L = flib.load()
    names = {0: "a_dev", 1: "la_dev", "la_host": "la_host", 2: "b_dev", 3: "lb_dev", "lb_host": "lb_host", 4: "basis_dev", 5: "cost_dev",
             6: "steps_dev", 7: "ws_dev"}
    for null, name in names.items():
        rc, msg = _dtw(L, null=null)
        assert rc == EINVAL and "NULL argument: %s" % name in msg, (null, rc, msg)
    for kw, value in ((dict(B=0, la=(), lb=()), "got 0, 80, 13, 8, 9"), (dict(M=0), "got 2, 0, 13, 8, 9"), (dict(K=0), "got 2, 80, 0, 8, 9"),
                      (dict(Ta_max=0), "got 2, 80, 13, 0, 9"), (dict(Tb_max=-3), "got 2, 80, 13, 8, -3")):
        rc, msg = _dtw(L, **kw)
        assert rc == EINVAL and "B, M, K, Ta_max, Tb_max must be positive" in msg and value in msg, (kw, rc, msg)
    for band in (1, -1, -40):
        rc, msg = _dtw(L, band=band)
        assert rc == EINVAL and "band must be 0" in msg and "got %d" % band in msg, (band, rc, msg)
    for kw, value in ((dict(la=(8, 0)), "pair 1: a has 0 frames (1 <= la"), (dict(la=(9, 3)), "pair 0: a has 9 frames (1 <= la"),
                      (dict(lb=(9, 10)), "pair 1: b has 10 frames (1 <= lb"), (dict(lb=(-2, 1)), "pair 0: b has -2 frames (1 <= lb")):
        rc, msg = _dtw(L, **kw)
        assert rc == EINVAL and value in msg, (kw, rc, msg)
    rc, msg = _dtw(L, M=257)
    assert rc == EUNSUPPORTED and "mel channels M" in msg and "got 257" in msg, (rc, msg)
    rc, msg = _dtw(L, K=65)
    assert rc == EUNSUPPORTED and "coefficients K" in msg and "got 65" in msg, (rc, msg)
    many = 65536
    rc, msg = _dtw(L, B=many, la=(1,) * many, lb=(1,) * many, Ta_max=1, Tb_max=1)
    assert rc == EUNSUPPORTED and "pairs B" in msg and "got 65536" in msg, (rc, msg)
    need = L.facppg_mel_dtw_workspace_bytes(2, 80, 13, 8, 9, 0)
    assert need > 0
    rc, msg = _dtw(L, ws_bytes=need - 1)
    assert rc == EWORKSPACE and "ws_bytes" in msg and str(need - 1) in msg and str(need) in msg, (rc, msg)
    # the workspace holds at least the cepstra and the admissible distances
    assert need >= 4 * 2 * (13 * (8 + 9) + 8 * 9)
    assert L.facppg_mel_dtw_workspace_bytes(0, 80, 13, 8, 9, 0) == 0 and "got 0, 80, 13, 8, 9" in L.facppg_last_error().decode()


def _path(L, B=2, Tout_max=8, Tin_max=9, tout=(8, 3), tin=(9, 1), ws_bytes=None, null=None):
    if ws_bytes is None:
        ws_bytes = L.facppg_attention_path_workspace_bytes(max(B, 1), max(Tout_max, 1), max(Tin_max, 1)) or 1 << 20
    rc = L.facppg_attention_path(_fake(0, null), _fake(1, null), None if null == "tout_host" else flib.offsets_array(tout), Tout_max,
                                 _fake(2, null), None if null == "tin_host" else flib.offsets_array(tin), Tin_max, B, _fake(3, null),
                                 _fake(4, null), _fake(5, null), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def test_attention_path_host_side_refusals():
    L = flib.load()
    names = {0: "align_dev", 1: "tout_dev", "tout_host": "tout_host", 2: "tin_dev", "tin_host": "tin_host", 3: "stats_dev", 4: "focus_dev",
             5: "ws_dev"}
    for null, name in names.items():
        rc, msg = _path(L, null=null)
        assert rc == EINVAL and "NULL argument: %s" % name in msg, (null, rc, msg)
    for kw, value in ((dict(B=0, tout=(), tin=()), "got 0, 8, 9"), (dict(Tout_max=0), "got 2, 0, 9"), (dict(Tin_max=-1), "got 2, 8, -1")):
        rc, msg = _path(L, **kw)
        assert rc == EINVAL and "B, Tout_max, Tin_max must be positive" in msg and value in msg, (kw, rc, msg)
    for kw, value in ((dict(tout=(8, 0)), "utterance 1: 0 decoder steps (1 <= tout"), (dict(tout=(9, 3)), "utterance 0: 9 decoder steps (1 <= tout"),
                      (dict(tin=(9, 10)), "utterance 1: 10 input frames (1 <= tin"), (dict(tin=(-2, 1)), "utterance 0: -2 input frames (1 <= tin")):
        rc, msg = _path(L, **kw)
        assert rc == EINVAL and value in msg, (kw, rc, msg)
    many = 65536
    rc, msg = _path(L, B=many, tout=(1,) * many, tin=(1,) * many, Tout_max=1, Tin_max=1)
    assert rc == EUNSUPPORTED and "utterances B" in msg and "got 65536" in msg, (rc, msg)
    need = L.facppg_attention_path_workspace_bytes(2, 8, 9)
    assert need >= 2 * (8 * 8 + 9)
    rc, msg = _path(L, ws_bytes=need - 1)
    assert rc == EWORKSPACE and "ws_bytes" in msg and str(need - 1) in msg and str(need) in msg, (rc, msg)
    assert L.facppg_attention_path_workspace_bytes(2, 0, 9) == 0 and "got 2, 0, 9" in L.facppg_last_error().decode()


def test_cepstral_basis():
    from facppg import score
    from facppg.lib import FacppgError
    for M, K in mh.DIMS + ((14, 13), (65, 64)):
        bas = score.cepstral_basis(M, K)
        assert bas.dtype == torch.float32 and tuple(bas.shape) == (K, M)
        assert np.array_equal(bas.numpy(), mh.basis(M, K))
        gram = bas.double().numpy() @ bas.double().numpy().T
        assert np.abs(gram - np.eye(K)).max() <= 1e-6, (M, K)
        assert np.abs(bas.double().numpy().sum(1)).max() <= 1e-6           # no row sees the level (c0 is left out)
    for M, K in ((80, 0), (80, 80), (80, -1), (200, 65), (2, 2), (1, 1)):
        with pytest.raises(FacppgError, match=r"n_cep must lie in \[1, min\(M - 1, 64\)\].*n_cep = %d for M = %d" % (K, M)):
            score.cepstral_basis(M, K)
    assert score.MCD_DB == mh.MCD_DB and abs(score.MCD_DB - 6.141851463713754) < 1e-12


def test_python_refusals_need_no_device():
    from facppg import score
    from facppg.lib import FacppgError
    with pytest.raises(FacppgError, match="mel_dtw: a must be a GPU tensor"):
        score.mel_dtw(torch.zeros(1, 80, 3), [3], torch.zeros(1, 80, 3), [3])
    with pytest.raises(FacppgError, match="attention_path: alignments must be a GPU tensor"):
        score.attention_path(torch.zeros(1, 4, 3), [4], [3])


def test_every_case_of_the_matrix_is_decidable():
    """The float64 reference and its float32 restatement (projection, differences and every sum in NumPy float32, m and k in
    increasing order) agree on steps for all 72 cases -- no case was dropped --, and the restatement's worst deviation per path cell
    is what the GPU tests' tolerance is 4 x of."""
    assert len(mh.MATRIX) == 72 and len(set(mh.MATRIX)) == 72
    assert set(c[:2] for c in mh.MATRIX) == set(mh.SHAPES) and set(c[2:4] for c in mh.MATRIX) == set(mh.DIMS)
    assert set(c[4] for c in mh.MATRIX) == set(mh.BANDS)
    undecidable, worst = [], (0.0, None)
    for c in mh.MATRIX:
        r64, r32 = mh.case(*c)
        if r64[1] != r32[1]:
            undecidable.append((c, r64, r32))
        dev = abs(r32[0] - r64[0]) / r64[1]
        if dev > worst[0]:
            worst = (dev, c)
        Ta, Tb = c[:2]
        assert max(Ta, Tb) <= r64[1] <= Ta + Tb - 1 and r64[0] > 0.0, (c, r64)
    print("float32 restatement: worst |cost32 - cost64| / steps = %.3e at (Ta, Tb, M, K, band) = %s; tolerance %.3e per cell" % (
        worst[0], worst[1], mh.cost_tolerance()))
    assert not undecidable, undecidable          # cap: no case of the matrix may be undecidable
    assert worst[0] == mh.emulation_deviation() > 0.0


def test_reference_properties():
    """Identical sequences cost exactly 0 in T steps; a gain change (a constant added to every log-mel channel of b) moves mcd by
    less than the tolerance, since c0 is left out."""
    tol = mh.cost_tolerance()
    for Ta, M, K in ((65, 80, 13), (7, 2, 1), (64, 80, 64)):
        a, _ = mh.inputs(Ta, Ta if Ta != 65 else 130, M)
        assert mh.reference(a, a, mh.basis(M, K)) == (0.0, Ta)
        assert mh.reference(a, a, mh.basis(M, K), band=2, dtype=np.float32) == (0.0, Ta)
    for Ta, Tb, M, K in ((63, 65, 80, 13), (65, 130, 80, 64), (7, 1, 2, 1)):
        a, b = mh.inputs(Ta, Tb, M)
        bas = mh.basis(M, K)
        c0, n0 = mh.reference(a, b, bas)
        c1, n1 = mh.reference(a, (b.astype(np.float64) + 0.5), bas)
        print("(%d, %d, %d, %d): mcd %.6f dB -> %.6f dB with +0.5 on every channel of b" % (Ta, Tb, M, K, mh.MCD_DB * c0 / n0, mh.MCD_DB * c1 / n1))
        assert abs(mh.MCD_DB * c1 / n1 - mh.MCD_DB * c0 / n0) < mh.MCD_DB * tol, (Ta, Tb, M, K, c0, n0, c1, n1)
    # a hand example, M = 2, K = 1: the one coefficient is (x0 - x1) / sqrt(2)
    bas = mh.basis(2, 1)
    a = np.array([[2.0, 0.0], [0.0, 0.0]], dtype=np.float32)          # c = sqrt(2), 0
    b = np.array([[2.0, 2.0], [0.0, 0.0]], dtype=np.float32)          # c = sqrt(2), sqrt(2)
    # d = [[0, 0], [r, r]], r = sqrt(2): C(0,1) = 0, C(1,0) = r, C(1,1) = r + min(0 (diag), 0 (up, a tie: the diagonal stays), r) = r
    cost, steps = mh.reference(a, b, bas)
    assert steps == 2 and abs(cost - float(np.sqrt(2.0))) < 1e-6


def test_attention_reference_hand_examples():
    eye = np.eye(5)
    assert mh.attention_reference(eye, 5, 5) == ([0, 4, 0, 1, 1, 5], np.float32(1.0))
    A = np.zeros((4, 6))
    for t, j in enumerate((2, 2, 1, 5)):
        A[t, j] = 0.5
    A[3, 3] = 0.5                                     # a tie at t = 3: the lower j
    assert mh.attention_reference(A, 4, 6) == ([2, 3, 1, 2, 2, 3], np.float32(0.5))
    assert mh.attention_reference(A, 4, 1)[0] == [0, 0, 0, 0, 4, 1]


class _Hp(object):
    fp16_run = False


def test_free_running_argument_refusals(capsys):
    from script import train_ppg2mel, validate_ppg2mel
    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="free_running=True scores the checkpoints on a valset"):
        train_ppg2mel.finetune(model, _Hp(), [], None, 1, free_running=True)
    with pytest.raises(ValueError, match="batch_size must be at least 1"):
        train_ppg2mel.validate_free_running(model, [(None, None)], 0)
    with pytest.raises(ValueError, match="step_factor must be positive"):
        train_ppg2mel.validate_free_running(model, [(None, None)], 2, step_factor=0.0)
    with pytest.raises(ValueError, match="validation set is empty"):
        train_ppg2mel.validate_free_running(model, [], 2)
    base = ["--ppg2mel_model", "ckpt", "--wav_list", "val.txt", "--out", "scores.tsv"]
    args = validate_ppg2mel.parse(base)
    assert (args.batch_size, args.seed, args.step_factor, args.hparams) == (None, 0, None, "")
    args = validate_ppg2mel.parse(base + ["--batch_size", "4", "--seed", "7", "--step_factor", "1.5", "--hparams", "n_symbols=40"])
    assert (args.batch_size, args.seed, args.step_factor, args.hparams) == (4, 7, 1.5, "n_symbols=40")
    for extra, text in ((["--batch_size", "0"], "--batch_size must be at least 1"), (["--step_factor", "0"], "--step_factor must be positive"),
                        (["--step_factor", "-2"], "--step_factor must be positive")):
        with pytest.raises(SystemExit) as e:
            validate_ppg2mel.parse(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err
    with pytest.raises(SystemExit):
        validate_ppg2mel.parse(base[:4])              # --out is required
    line = validate_ppg2mel.score_line("a.wav", {c: np.asarray([1.25 if c in ("mcd", "stretch", "coverage", "focus") else 3])
                                                 for c in validate_ppg2mel.SCORE_COLUMNS}, 0)
    assert line == "a.wav\t3\t3\t3\t1.25\t1.25\t3\t3\t3\t1.25\t3\t1.25"
