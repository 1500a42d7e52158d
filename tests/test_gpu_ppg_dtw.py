"""GPU: facppg_ppg_dtw (facppg.score.ppg_dtw) against the float64 reference of its definition (score_helpers.py).

The matrix: (Ta, Tb) in {(1,1), (1,7), (7,1), (2,2), (63,65), (64,64), (65,130), (257,300)} x D in {1, 40, 256} x band
in {0, 2, 40} -- a single cell, both orientations of unequal lengths, a wave boundary, a 32 x 32 tile boundary, more than one
256-frame block.  steps and agree are exact; |cost - ref| <= tol * steps with tol = 4 x the float32 restatement's own worst
deviation per path cell (score_helpers.cost_tolerance, measured in test_ppg_dtw_cpu.py: 4 x 4.39e-7 = 1.75e-6); D = 1 costs exactly 0.
Two more shapes for the paths the matrix does not reach: the sweep in strips (more rows than a workgroup has threads -- forced at
257 rows with FACPPG_DTW_ROWS=64, and for real at 1030 rows).

Measured on the MI355X: the device's worst |cost - ref| / steps over the matrix is 4.39e-7 (257 x 300, D = 40, band 2; the single cell
at D = 256: 3.29e-7); the matrix test prints it per shape."""
import ctypes

import numpy as np
import pytest
import torch

import score_helpers as sh

pytestmark = pytest.mark.gpu


def _padded(mats, Tmax, fill):
    """[D, T_p] arrays -> [B, D, Tmax] on the GPU with ``fill`` behind every length."""
    x = np.full((len(mats), mats[0].shape[0], Tmax), fill, dtype=np.float32)
    for p, m in enumerate(mats):
        x[p, :, :m.shape[1]] = m
    return torch.from_numpy(x).cuda()


def _dtw(pairs, band, Ta_max=None, Tb_max=None, fill=np.nan):
    from facppg import score
    la, lb = [a.shape[1] for a, _ in pairs], [b.shape[1] for _, b in pairs]
    a = _padded([a for a, _ in pairs], Ta_max or max(la), fill)
    b = _padded([b for _, b in pairs], Tb_max or max(lb), fill)
    return score.ppg_dtw(a, la, b, lb, band=band)


def _check(out, p, ref, tol, what):
    cost, steps, agree = float(out["cost"][p]), int(out["steps"][p]), int(out["agree"][p])
    assert np.isfinite(cost), what
    assert (steps, agree) == ref[1:], (what, (cost, steps, agree), ref)
    assert abs(cost - ref[0]) <= tol * steps, (what, cost, ref[0], abs(cost - ref[0]) / steps, tol)
    return abs(cost - ref[0]) / steps


@pytest.mark.parametrize("Ta,Tb", sh.SHAPES)
def test_matrix_against_the_float64_reference(Ta, Tb):
    tol = sh.cost_tolerance()
    worst = 0.0
    for D in sh.DIMS:
        a, b = sh.inputs(Ta, Tb, D)
        for band in sh.BANDS:
            ref = sh.case(Ta, Tb, D, band)[0]
            out = _dtw([(a, b)], band)
            dev = _check(out, 0, ref, tol, (Ta, Tb, D, band))
            if D == 1:
                assert float(out["cost"][0]) == 0.0, (Ta, Tb, band, out["cost"])
            # the derived figures
            assert out["distance"][0] == float(out["cost"][0]) / ref[1] and out["agreement"][0] == ref[2] / ref[1]
            assert out["stretch"][0] == ref[1] / max(Ta, Tb)
            worst = max(worst, dev)
    print("(%d, %d): device worst |cost - ref| / steps = %.3e (tolerance %.3e)" % (Ta, Tb, worst, tol))


def test_ragged_batch_equals_each_pair_alone_and_ignores_the_padding():
    """B = 3 pairs of different lengths in one padded batch, NaN behind every length in a and b."""
    shapes = ((63, 65), (7, 1), (65, 130))
    pairs = [sh.inputs(Ta, Tb, 40) for Ta, Tb in shapes]
    for band in (0, 2):
        batch = _dtw(pairs, band)
        assert all(np.isfinite(batch[k]).all() for k in ("cost", "distance", "agreement", "stretch"))
        for p, (Ta, Tb) in enumerate(shapes):
            alone = _dtw([pairs[p]], band)
            for k in ("cost", "steps", "agree"):
                assert batch[k][p].tobytes() == alone[k][0].tobytes(), (band, p, k, batch[k][p], alone[k][0])
            _check(batch, p, sh.case(Ta, Tb, 40, band)[0], sh.cost_tolerance(), (band, p))
    # the same batch in wider buffers (Ta_max, Tb_max beyond every length), +inf instead of NaN behind the lengths
    wide = _dtw(pairs, 0, Ta_max=100, Tb_max=131, fill=np.inf)
    ref = _dtw(pairs, 0)
    assert all(wide[k].tobytes() == ref[k].tobytes() for k in ("cost", "steps", "agree"))


def test_identity():
    a, _ = sh.inputs(65, 130, 40)
    out = _dtw([(a, a)], 0)
    assert int(out["steps"][0]) == int(out["agree"][0]) == 65
    assert 0.0 <= float(out["cost"][0]) <= sh.cost_tolerance() * 65
    assert out["agreement"][0] == 1.0 and out["stretch"][0] == 1.0


def test_the_band_is_honoured():
    """b = a shifted by 10 frames at T = 64: the free alignment follows the shift, band = 2 cannot."""
    a, _ = sh.inputs(64, 64, 40)
    b = a[:, np.minimum(np.arange(64) + 10, 63)].copy()
    tol = sh.cost_tolerance()
    free, narrow = _dtw([(a, b)], 0), _dtw([(a, b)], 2)
    ref_free, ref_narrow = sh.reference(a, b, 0), sh.reference(a, b, 2)
    _check(free, 0, ref_free, tol, "band 0")
    _check(narrow, 0, ref_narrow, tol, "band 2")
    print("shift 10: band 0 cost %.6f (%d steps), band 2 cost %.6f (%d steps)" % (free["cost"][0], free["steps"][0], narrow["cost"][0],
                                                                                 narrow["steps"][0]))
    assert ref_narrow[0] > ref_free[0] + 1.0 and float(narrow["cost"][0]) != float(free["cost"][0])


def test_the_sweep_in_strips(monkeypatch):
    """More rows than one strip: 257 rows in strips of 64 (the same bits as in one strip), and 1030 rows in the real strips of 1024."""
    tol = sh.cost_tolerance()
    a, b = sh.inputs(257, 300, 40)
    whole = {band: _dtw([(a, b)], band) for band in (0, 40)}
    monkeypatch.setenv("FACPPG_DTW_ROWS", "64")
    for band in (0, 40):
        strips = _dtw([(a, b)], band)
        assert all(strips[k].tobytes() == whole[band][k].tobytes() for k in ("cost", "steps", "agree")), band
    # a ragged batch in strips: the short pairs leave the later launches at once
    shapes = ((63, 65), (7, 1), (65, 130))
    pairs = [sh.inputs(Ta, Tb, 40) for Ta, Tb in shapes]
    out = _dtw(pairs, 0, Ta_max=70)
    for p, (Ta, Tb) in enumerate(shapes):
        _check(out, p, sh.case(Ta, Tb, 40, 0)[0], tol, ("strips", p))
    monkeypatch.delenv("FACPPG_DTW_ROWS")
    a, b = sh.make(1030, 40, 40, sh.seed_of(1030, 40, 40))
    for band in (0, 2):
        _check(_dtw([(a, b)], band), 0, sh.reference(a, b, band), tol, ("1030 rows", band))


def test_twice_on_one_workspace_of_the_stated_size():
    """The raw entry point twice back to back on one workspace of exactly facppg_ppg_dtw_workspace_bytes, a canary behind it: the
    same results, the stream still usable, nothing written past the stated size."""
    from facppg import lib as flib
    L = flib.load()
    shapes = ((63, 65), (257, 300), (65, 130))
    pairs = [sh.inputs(Ta, Tb, 40) for Ta, Tb in shapes]
    la, lb = [s[0] for s in shapes], [s[1] for s in shapes]
    a, b = _padded([p[0] for p in pairs], 257, np.nan), _padded([p[1] for p in pairs], 300, np.nan)
    need = L.facppg_ppg_dtw_workspace_bytes(3, 40, 257, 300, 40)
    assert need > 0
    guard = 4096
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.tensor(la + lb, dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((3, 3), -1, dtype=torch.int32, device="cuda")
        flib.check(L.facppg_ppg_dtw(flib.ptr(a), flib.ptr(lens[:3]), flib.offsets_array(la), 257, flib.ptr(b), flib.ptr(lens[3:]),
                                    flib.offsets_array(lb), 300, 3, 40, 40, flib.ptr(out[0]), flib.ptr(out[1]), flib.ptr(out[2]), flib.ptr(ws),
                                    ctypes.c_size_t(need), flib.current_stream(a.device)))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((ws[need:] == 0xA5).all())
    host = outs[0].cpu().numpy()
    for p, (Ta, Tb) in enumerate(shapes):
        ref = sh.case(Ta, Tb, 40, 40)[0]
        assert (int(host[1, p]), int(host[2, p])) == ref[1:]
        assert abs(float(host[0, p:p + 1].view(np.float32)[0]) - ref[0]) <= sh.cost_tolerance() * ref[1]
    assert float((torch.ones(8, device="cuda") * 2).sum()) == 16.0      # the stream goes on
