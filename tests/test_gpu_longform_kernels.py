"""GPU: the three long-form kernels through the C ABI (facppg_ppg_pause_flags, facppg_ppg_gather_segments,
facppg_join_segments) on seeded random data, each against a NumPy restatement with EXACT equality -- the flag sum adds float32
rows in the order given, the gather copies, the join's gains are fp32 numbers -- and each output between guard bytes that
must come back unchanged.

Shapes.  B = 2, Tmax = 53 (odd: rows of the source start on any 4-byte boundary; 53 = 13 whole groups of four frames and one
frame, so the flag kernel takes both of its paths), lengths (53, 17); K = 40 (monophone) and K = 5816 (senone: 11 632 source
rows, several thousand workgroups).  Lmax = 13 (scalar destination rows) and 16 (16-byte stores; once more into a destination
that is NOT 16-byte aligned, which must take the scalar path)."""
import numpy as np
import pytest
import torch

from longform_helpers import flag_sums, join, seam_fades

pytestmark = pytest.mark.gpu

B, TMAX, LENGTHS = 2, 53, (53, 17)
GUARD, FILL = 64, 0xA5
SEGMENTS = ((0, 0, 13), (0, 1, 1), (0, 3, 7), (1, 40, 13), (1, 5, 12))


@pytest.fixture(scope="module")
def posteriors():
    """{K: softmax rows [B, K, Tmax] float32 on the host} -- computed once, never written to."""
    out = {}
    for K in (40, 5816):
        g = np.random.Generator(np.random.PCG64(100 + K))
        z = (3.0 * g.standard_normal((B, K, TMAX))).astype(np.float32)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        out[K] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        out[K].setflags(write=False)
    return out


def _guarded(nbytes, shift=0):
    """A device buffer of ``nbytes`` between two guards -> (whole allocation, the view in the middle, ``shift`` bytes further on)."""
    buf = torch.full((GUARD + shift + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + nbytes]


def _guards_intact(buf, nbytes, shift=0):
    host = buf.cpu().numpy()
    return bool((host[:GUARD + shift] == FILL).all() and (host[GUARD + shift + nbytes:] == FILL).all())


def _lib():
    from facppg import lib as flib
    return flib, flib.load()


def _i32(values):
    flib, _ = _lib()
    flat = [int(v) for v in np.asarray(values).reshape(-1)]
    return flib.offsets_array(flat), torch.tensor(flat, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("K, rows", [(40, [39]), (5816, [5815, 17, 0, 4001, 233, 5000, 1024])])
def test_pause_flags(posteriors, K, rows):
    flib, L = _lib()
    x = posteriors[K]
    sums = flag_sums(x, rows)
    thr = np.float32(np.median(np.concatenate([sums[b, :n] for b, n in enumerate(LENGTHS)])))
    t = np.arange(TMAX)[None, :]
    want = ((t < np.asarray(LENGTHS)[:, None]) & (sums > thr)).astype(np.uint8)
    assert 0.0 < thr < len(rows) and 0 < want[0].sum() < TMAX and 0 < want[1, :17].sum() < 17      # both values occur
    xd = torch.from_numpy(x.copy()).cuda()
    rows_host, rows_dev = _i32(rows)
    _, lens_dev = _i32(LENGTHS)
    buf, flags = _guarded(B * TMAX)
    st = flib.current_stream(xd.device)
    flib.check(L.facppg_ppg_pause_flags(flib.ptr(xd), flib.ptr(lens_dev), B, K, TMAX, flib.ptr(rows_dev), rows_host, len(rows), float(thr),
                                        flib.ptr(flags), st))
    got = flags.cpu().numpy().reshape(B, TMAX)
    assert np.array_equal(got, want)
    assert not got[1, 17:].any() and _guards_intact(buf, B * TMAX)
    # refusals: error code, nothing written
    before = buf.clone()
    assert L.facppg_ppg_pause_flags(flib.ptr(xd), flib.ptr(lens_dev), B, K, TMAX, flib.ptr(rows_dev), rows_host, 0, float(thr), flib.ptr(flags), st) == -1
    bad_host, bad_dev = _i32(rows[:-1] + [K])
    assert L.facppg_ppg_pause_flags(flib.ptr(xd), flib.ptr(lens_dev), B, K, TMAX, flib.ptr(bad_dev), bad_host, len(rows), float(thr), flib.ptr(flags), st) == -1
    for bad in (0.0, float(len(rows))):
        assert L.facppg_ppg_pause_flags(flib.ptr(xd), flib.ptr(lens_dev), B, K, TMAX, flib.ptr(rows_dev), rows_host, len(rows), bad, flib.ptr(flags), st) == -1
    assert torch.equal(buf, before)


@pytest.mark.parametrize("K", [40, 5816])
@pytest.mark.parametrize("Lmax, shift", [(13, 0), (16, 0), (16, 4)])
def test_gather_segments(posteriors, K, Lmax, shift):
    flib, L = _lib()
    x = posteriors[K]
    S = len(SEGMENTS)
    want = np.zeros((S, K, Lmax), dtype=np.float32)
    for s, (b, start, frames) in enumerate(SEGMENTS):
        want[s, :, :frames] = x[b, :, start:start + frames]
    xd = torch.from_numpy(x.copy()).cuda()
    nbytes = S * K * Lmax * 4
    buf, raw = _guarded(nbytes, shift)
    y = raw.view(torch.float32)
    y.fill_(float("nan"))
    assert y.data_ptr() % 16 == shift
    t_host, t_dev = _i32(SEGMENTS)
    st = flib.current_stream(xd.device)
    flib.check(L.facppg_ppg_gather_segments(flib.ptr(xd), B, K, TMAX, flib.ptr(t_dev), t_host, S, Lmax, flib.ptr(y), st))
    got = y.cpu().numpy().reshape(S, K, Lmax)
    assert np.array_equal(got, want)                     # (no NaN is left: every element was written)
    assert _guards_intact(buf, nbytes, shift)
    # a table that leaves the source or the destination is refused with an error code and launches nothing
    y.fill_(float("nan"))
    for bad in ((1, 41, 13), (0, 3, 0), (0, 0, Lmax + 1), (2, 0, 1), (0, -1, 4)):
        t_host, t_dev = _i32(SEGMENTS[:2] + (bad,) + SEGMENTS[3:])
        assert L.facppg_ppg_gather_segments(flib.ptr(xd), B, K, TMAX, flib.ptr(t_dev), t_host, S, Lmax, flib.ptr(y), st) == -1, bad
        assert b"segment 2" in L.facppg_last_error()
    assert bool(torch.isnan(y).all()) and _guards_intact(buf, nbytes, shift)


@pytest.mark.parametrize("n, fade", [((5, 400, 1, 130), 64), ((400,), 64), ((5, 400, 1, 130), 0), ((130, 257), 4096), ((7, 0, 9), 2)])
def test_join_segments(n, fade):
    flib, L = _lib()
    NMAX, S = 400, len(n)
    if n == (5, 400, 1, 130) and fade == 64:
        assert seam_fades(n, fade) == [2, 64, 0, 64]
    g = np.random.Generator(np.random.PCG64(7 + S + fade))
    audio = g.standard_normal((S, NMAX)).astype(np.float32)
    want = join([audio[s, :n[s]] for s in range(S)], fade)
    if S == 1 or fade == 0:
        assert np.array_equal(want, np.concatenate([audio[s, :n[s]] for s in range(S)]))      # a plain copy
    ad = torch.from_numpy(audio).cuda()
    n_host, n_dev = _i32(n)
    total = sum(n)
    buf, raw = _guarded(total * 4)
    st = flib.current_stream(ad.device)
    flib.check(L.facppg_join_segments(flib.ptr(ad), NMAX, flib.ptr(n_dev), n_host, S, fade, flib.ptr(raw), st))
    got = raw.view(torch.float32).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert _guards_intact(buf, total * 4)
    before = buf.clone()
    assert L.facppg_join_segments(flib.ptr(ad), NMAX, flib.ptr(n_dev), n_host, S, 48, flib.ptr(raw), st) == -1
    assert b"power of two" in L.facppg_last_error() and torch.equal(buf, before)
