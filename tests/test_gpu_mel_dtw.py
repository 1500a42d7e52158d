"""GPU: facppg_mel_dtw (facppg.score.mel_dtw) and facppg_attention_path (facppg.score.attention_path) against the float64
references of their definitions (mcd_helpers.py).

mel_dtw's matrix: (Ta, Tb) in {(1,1), (1,7), (7,1), (2,2), (63,65), (64,64), (65,130), (257,300)} x (M, K) in {(80,13), (80,64),
(2,1)} x band in {0, 2, 40} -- a single cell, both orientations of unequal lengths, a wave boundary, the 64 x 64 tile boundary of
the distance kernel, more than one 256-frame block of the projection, the largest K a tile stages.  steps is exact;
|cost - ref| <= tol * steps with tol = 4 x the float32 restatement's own worst deviation per path cell
(mcd_helpers.cost_tolerance, measured in test_mel_dtw_cpu.py: 4 x 8.952e-6 = 3.581e-5).  Two more shapes for the sweep in strips (more
rows than a workgroup has threads -- forced at 257 rows with FACPPG_DTW_ROWS=64, and for real at 1030 rows).

Measured on the MI355X: the device's worst |cost - ref| / steps over the matrix is 5.71e-6 (257 x 300; the single cell: 2.39e-6) --
the 80-term fp32 projection dominates it on the device as in NumPy; the matrix test prints it per shape.

attention_path: hand-built alignments (a monotone diagonal, one backward jump, a skip of 9, a stall of 5, a tie, T = 1, L = 1) and
random row-stochastic matrices in a ragged batch with NaN behind T and L: the six integers exact, focus within one fp32 ulp."""
import ctypes

import numpy as np
import pytest
import torch

import mcd_helpers as mh

pytestmark = pytest.mark.gpu


def _padded(mats, Tmax, fill):
    """[M, T_p] arrays -> [B, M, Tmax] on the GPU with ``fill`` behind every length."""
    x = np.full((len(mats), mats[0].shape[0], Tmax), fill, dtype=np.float32)
    for p, m in enumerate(mats):
        x[p, :, :m.shape[1]] = m
    return torch.from_numpy(x).cuda()


def _dtw(pairs, K, band, Ta_max=None, Tb_max=None, fill=np.nan):
    from facppg import score
    la, lb = [a.shape[1] for a, _ in pairs], [b.shape[1] for _, b in pairs]
    a = _padded([a for a, _ in pairs], Ta_max or max(la), fill)
    b = _padded([b for _, b in pairs], Tb_max or max(lb), fill)
    return score.mel_dtw(a, la, b, lb, n_cep=K, band=band)


def _check(out, p, ref, tol, what):
    cost, steps = float(out["cost"][p]), int(out["steps"][p])
    assert np.isfinite(cost), what
    assert steps == ref[1], (what, (cost, steps), ref)
    assert abs(cost - ref[0]) <= tol * steps, (what, cost, ref[0], abs(cost - ref[0]) / steps, tol)
    return abs(cost - ref[0]) / steps


@pytest.mark.parametrize("Ta,Tb", mh.SHAPES)
def test_matrix_against_the_float64_reference(Ta, Tb):
    tol = mh.cost_tolerance()
    worst = 0.0
    for M, K in mh.DIMS:
        a, b = mh.inputs(Ta, Tb, M)
        for band in mh.BANDS:
            ref = mh.case(Ta, Tb, M, K, band)[0]
            out = _dtw([(a, b)], K, band)
            worst = max(worst, _check(out, 0, ref, tol, (Ta, Tb, M, K, band)))
            # the derived figures
            assert out["mcd"][0] == mh.MCD_DB * float(out["cost"][0]) / ref[1]
            assert out["stretch"][0] == ref[1] / max(Ta, Tb)
    print("(%d, %d): device worst |cost - ref| / steps = %.3e (tolerance %.3e)" % (Ta, Tb, worst, tol))


def test_ragged_batch_equals_each_pair_alone_and_ignores_the_padding():
    """B = 3 pairs of different lengths in one padded batch, NaN behind every length in a and b."""
    shapes = ((63, 65), (7, 1), (65, 130))
    pairs = [mh.inputs(Ta, Tb, 80) for Ta, Tb in shapes]
    for band in (0, 2):
        batch = _dtw(pairs, 13, band)
        assert all(np.isfinite(batch[k]).all() for k in ("cost", "mcd", "stretch"))
        for p, (Ta, Tb) in enumerate(shapes):
            alone = _dtw([pairs[p]], 13, band)
            for k in ("cost", "steps"):
                assert batch[k][p].tobytes() == alone[k][0].tobytes(), (band, p, k, batch[k][p], alone[k][0])
            _check(batch, p, mh.case(Ta, Tb, 80, 13, band)[0], mh.cost_tolerance(), (band, p))
    # the same batch in wider buffers (Ta_max, Tb_max beyond every length), +inf instead of NaN behind the lengths
    wide = _dtw(pairs, 13, 0, Ta_max=100, Tb_max=131, fill=np.inf)
    ref = _dtw(pairs, 13, 0)
    assert all(wide[k].tobytes() == ref[k].tobytes() for k in ("cost", "steps"))


def test_identity():
    a, _ = mh.inputs(65, 130, 80)
    out = _dtw([(a, a)], 13, 0)
    assert int(out["steps"][0]) == 65
    assert 0.0 <= float(out["cost"][0]) <= mh.cost_tolerance() * 65
    assert out["stretch"][0] == 1.0


def test_the_band_is_honoured():
    """b = a shifted by 10 frames at T = 64: the free alignment follows the shift, band = 2 cannot."""
    a, _ = mh.inputs(64, 64, 80)
    b = a[:, np.minimum(np.arange(64) + 10, 63)].copy()
    tol, bas = mh.cost_tolerance(), mh.basis(80, 13)
    free, narrow = _dtw([(a, b)], 13, 0), _dtw([(a, b)], 13, 2)
    ref_free, ref_narrow = mh.reference(a, b, bas, 0), mh.reference(a, b, bas, 2)
    _check(free, 0, ref_free, tol, "band 0")
    _check(narrow, 0, ref_narrow, tol, "band 2")
    print("shift 10: band 0 cost %.6f (%d steps), band 2 cost %.6f (%d steps)" % (free["cost"][0], free["steps"][0], narrow["cost"][0],
                                                                                 narrow["steps"][0]))
    assert ref_narrow[0] > ref_free[0] + 1.0 and float(narrow["cost"][0]) != float(free["cost"][0])


def test_the_sweep_in_strips(monkeypatch):
    """More rows than one strip: 257 rows in strips of 64 (the same bits as in one strip), and 1030 rows in the real strips of 1024."""
    tol = mh.cost_tolerance()
    a, b = mh.inputs(257, 300, 80)
    whole = {band: _dtw([(a, b)], 13, band) for band in (0, 40)}
    monkeypatch.setenv("FACPPG_DTW_ROWS", "64")
    for band in (0, 40):
        strips = _dtw([(a, b)], 13, band)
        assert all(strips[k].tobytes() == whole[band][k].tobytes() for k in ("cost", "steps")), band
    # a ragged batch in strips: the short pairs leave the later launches at once
    shapes = ((63, 65), (7, 1), (65, 130))
    pairs = [mh.inputs(Ta, Tb, 80) for Ta, Tb in shapes]
    out = _dtw(pairs, 13, 0, Ta_max=70)
    for p, (Ta, Tb) in enumerate(shapes):
        _check(out, p, mh.case(Ta, Tb, 80, 13, 0)[0], tol, ("strips", p))
    monkeypatch.delenv("FACPPG_DTW_ROWS")
    a, b = mh.make(1030, 40, 80, mh.seed_of(1030, 40, 80))
    for band in (0, 2):
        _check(_dtw([(a, b)], 13, band), 0, mh.reference(a, b, mh.basis(80, 13), band), tol, ("1030 rows", band))


def test_twice_on_one_workspace_of_the_stated_size():
    """The raw entry point twice back to back on one workspace of exactly facppg_mel_dtw_workspace_bytes, a canary behind it: the
    same results, the stream still usable, nothing written past the stated size."""
    from facppg import lib as flib
    L = flib.load()
    shapes = ((63, 65), (257, 300), (65, 130))
    pairs = [mh.inputs(Ta, Tb, 80) for Ta, Tb in shapes]
    la, lb = [s[0] for s in shapes], [s[1] for s in shapes]
    a, b = _padded([p[0] for p in pairs], 257, np.nan), _padded([p[1] for p in pairs], 300, np.nan)
    bas = torch.from_numpy(mh.basis(80, 64)).cuda()
    need = L.facppg_mel_dtw_workspace_bytes(3, 80, 64, 257, 300, 40)
    assert need > 0
    guard = 4096
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.tensor(la + lb, dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(2):
        out = torch.full((2, 3), -1, dtype=torch.int32, device="cuda")
        flib.check(L.facppg_mel_dtw(flib.ptr(a), flib.ptr(lens[:3]), flib.offsets_array(la), 257, flib.ptr(b), flib.ptr(lens[3:]),
                                    flib.offsets_array(lb), 300, 3, 80, flib.ptr(bas), 64, 40, flib.ptr(out[0]), flib.ptr(out[1]), flib.ptr(ws),
                                    ctypes.c_size_t(need), flib.current_stream(a.device)))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((ws[need:] == 0xA5).all())
    host = outs[0].cpu().numpy()
    for p, (Ta, Tb) in enumerate(shapes):
        ref = mh.case(Ta, Tb, 80, 64, 40)[0]
        assert int(host[1, p]) == ref[1]
        assert abs(float(host[0, p:p + 1].view(np.float32)[0]) - ref[0]) <= mh.cost_tolerance() * ref[1]
    assert float((torch.ones(8, device="cuda") * 2).sum()) == 16.0      # the stream goes on


# ------------------------------------------------------------------------------------ attention_path

def _path_of(pos, L, weight=0.75):
    """An alignment [T, L] whose row t peaks at pos[t] (the rest of the row spread evenly below the peak)."""
    A = np.full((len(pos), L), (1.0 - weight) / max(L - 1, 1), dtype=np.float32)
    for t, j in enumerate(pos):
        A[t, j] = weight if L > 1 else 1.0
    return A


def _attention(mats, fill=np.nan, Tout_max=None, Tin_max=None):
    from facppg import score
    T, L = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    x = np.full((len(mats), Tout_max or max(T), Tin_max or max(L)), fill, dtype=np.float32)
    for p, m in enumerate(mats):
        x[p, :m.shape[0], :m.shape[1]] = m
    return score.attention_path(torch.from_numpy(x).cuda(), T, L), T, L


def _check_path(out, mats, T, L):
    from facppg import score
    for p, m in enumerate(mats):
        stats, focus = mh.attention_reference(m, T[p], L[p])
        got = [int(out[name][p]) for name in score.ATTENTION_FIELDS]
        assert got == stats, (p, got, stats)
        assert abs(float(out["focus"][p]) - float(focus)) <= 2.0 ** -23 * abs(float(focus)), (p, out["focus"][p], focus)
        assert out["coverage"][p] == stats[5] / L[p] and int(out["end_gap"][p]) == L[p] - 1 - stats[1]


def test_attention_path_hand_built():
    diagonal = _path_of(list(range(12)), 12)
    backward = _path_of([0, 1, 2, 3, 2, 3, 4, 5], 6)
    skip = _path_of([0, 1, 2, 11, 12, 13], 14)
    stall = _path_of([0, 1, 2, 2, 2, 2, 2, 3, 4], 7)
    tie = _path_of([1, 2, 4], 6)
    tie[1, 5] = tie[1, 2]                            # two equal maxima in row 1: j = 2 wins
    tie[2, 0] = tie[2, 4]                            # and in row 2: j = 0 wins, a backward jump
    one_step = _path_of([3], 5)
    one_input = _path_of([0, 0, 0], 1)
    mats = [diagonal, backward, skip, stall, tie, one_step, one_input]
    out, T, L = _attention(mats)
    _check_path(out, mats, T, L)
    want = {"first": [0, 0, 0, 0, 1, 3, 0], "last": [11, 5, 13, 4, 0, 3, 0], "back": [0, 1, 0, 0, 1, 0, 0], "max_jump": [1, 1, 9, 1, 1, 0, 0],
            "longest_stall": [1, 1, 1, 5, 1, 1, 3], "visited": [12, 6, 6, 5, 3, 1, 1]}
    for name, values in want.items():
        assert out[name].tolist() == values, (name, out[name], values)
    assert out["end_gap"].tolist() == [0, 0, 0, 2, 5, 1, 0] and out["coverage"][2] == 6 / 14
    # each utterance alone, in a buffer of its own size: the same bits
    for p, m in enumerate(mats):
        alone, _, _ = _attention([m])
        assert all(alone[k][0].tobytes() == out[k][p].tobytes() for k in out), p


def test_attention_path_random_ragged_batch():
    r = np.random.RandomState(5)
    mats = []
    for T, L in ((1, 1), (7, 300), (65, 64), (300, 257)):
        m = r.rand(T, L) ** 8                          # peaky rows
        mats.append((m / m.sum(1, keepdims=True)).astype(np.float32))
    # long runs and many chunks: 2048 steps that dwell, jump back and forth over 40 inputs
    pos = np.repeat(r.randint(0, 40, size=128), 16)
    mats.append(_path_of(pos.tolist(), 40, weight=0.6))
    out, T, L = _attention(mats)
    _check_path(out, mats, T, L)
    wide, _, _ = _attention(mats, fill=np.inf, Tout_max=2100, Tin_max=333)
    assert all(wide[k].tobytes() == out[k].tobytes() for k in out)
