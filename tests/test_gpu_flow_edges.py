"""GPU: the small fp32 kernels at the edges of a WaveGlow flow in the training direction (csrc/facppg_train.hip), each called
directly and held to a float64 reference element by element: facppg_conv1x1 (k_conv1x1), facppg_conv1x1_wgrad
(k_conv1x1_wgrad_part, k_sum_parts), facppg_affine_forward / backward, facppg_weight_norm_forward / backward and
facppg_segment_sums.  The runner of tests/wn_train_helpers.py throughout: every output starts as NaN with a sentinel tail,
every workspace as 0xFF bytes, every operand is followed by NaN.

Ternary operands (every sum an integer below 2^24): np.array_equal.  Random operands: allowances derived from the number of
roundings -- conv1x1 c u S; its weight gradient (B L + 2) 2u S; the affine coupling (4 + 2 |log_s|) u of the magnitudes (2 |x| u
from exp2(x log2 e) with a rounded constant and a rounded product, 2 u = 1 ulp from the hardware exp2, one u per following
multiply or add); weight norm from its summation order (below); the segment sums, formed in double, 1 ulp of float32."""
import ctypes
import math

import numpy as np
import pytest
import torch

import wn_train_helpers as wh
from wn_train_helpers import U, dev_input, dev_output, dev_workspace, guard_intact, host

pytestmark = pytest.mark.gpu


def _lib():
    return wh._lib()


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _data(g, shape, kind):
    if kind == "int":
        return g.integers(-1, 2, shape).astype(np.float32)
    return g.standard_normal(shape, dtype=np.float32)


def _worst(err, tol):
    live = tol > 0
    assert not err[~live].any()
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


def _stream():
    return _lib()[0].current_stream(torch.device("cuda"))


# --------------------------------------------------------------------------------------------------------- facppg_conv1x1
CONV_L = (1, 3, 4, 5, 1023, 1024, 1025, 1028)      # the float4 path (L % 4 == 0), the scalar tail, the grid edge at 1024


@pytest.mark.parametrize("kind", ["int", "random"])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("c", [2, 4, 6, 8])
def test_conv1x1(c, trans, kind):
    lib, L = _lib()
    worst = 0.0
    for B in (1, 3):
        for n in CONV_L:
            g = _rng(c, trans, B, n)
            W, z = _data(g, (c, c), kind), _data(g, (B, c, n), kind)
            Wd, zd, out = dev_input(W), dev_input(z), dev_output(B * c * n)
            rc = L.facppg_conv1x1(lib.ptr(Wd), lib.ptr(zd), lib.ptr(out), B, c, n, trans, _stream())
            torch.cuda.synchronize()
            assert rc == wh.OK, (rc, wh.last_error())
            assert guard_intact(out, B * c * n), (B, n)
            got = host(out, (B, c, n))
            Wm = W.astype(np.float64).T if trans else W.astype(np.float64)
            ref = np.einsum("ij,bjl->bil", Wm, z.astype(np.float64))
            if kind == "int":
                assert np.array_equal(got, ref), (B, n)
            else:
                tol = c * U * np.einsum("ij,bjl->bil", np.abs(Wm), np.abs(z.astype(np.float64)))
                err = np.abs(got - ref)
                worst = max(worst, _worst(err, tol))
                assert (err <= tol).all(), (B, n)
    if kind == "random":
        print("conv1x1 c %d trans %d: worst err/tol %.3f" % (c, trans, worst))


def test_conv1x1_rejects_what_it_does_not_build():
    lib, L = _lib()
    z, out = dev_input(np.zeros((1, 10, 4), np.float32)), dev_output(40)
    W = dev_input(np.zeros(100, np.float32))
    for c in (3, 10):
        assert L.facppg_conv1x1(lib.ptr(W), lib.ptr(z), lib.ptr(out), 1, c, 4, 0, _stream()) == wh.EUNSUPPORTED
    assert L.facppg_conv1x1(lib.ptr(W), lib.ptr(z), lib.ptr(z), 1, 4, 4, 0, _stream()) == wh.EINVAL
    assert "not in-place" in wh.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:40]).all()) and guard_intact(out, 40)


# --------------------------------------------------------------------------------------------------- facppg_conv1x1_wgrad
# B L = 1 (one partial), 255 / 256 / 257 (one or two workgroups: fewer partials than k_sum_parts' 16 groups), 3000 (12
# partials), 140 000 (547 workgroups' worth: past the 512-workgroup cap, the grid-stride loop runs)
WGRAD_BL = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 1000), (4, 35000))


@pytest.mark.parametrize("kind", ["int", "random"])
@pytest.mark.parametrize("c", [2, 4, 6, 8])
def test_conv1x1_wgrad(c, kind):
    lib, L = _lib()
    nbytes = L.facppg_conv1x1_wgrad_workspace_bytes(c)
    assert nbytes == 512 * c * c * 4
    worst = 0.0
    for B, n in WGRAD_BL:
        g = _rng(c, B, n, 7)
        dout, z = _data(g, (B, c, n), kind), _data(g, (B, c, n), kind)
        dd, zd, dw, ws = dev_input(dout), dev_input(z), dev_output(c * c), dev_workspace(nbytes)
        rc = L.facppg_conv1x1_wgrad(lib.ptr(dd), lib.ptr(zd), lib.ptr(dw), B, c, n, lib.ptr(ws), nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == wh.OK, (rc, wh.last_error())
        assert guard_intact(dw, c * c) and guard_intact(ws, nbytes), (B, n)
        got = host(dw, (c, c))
        d64, z64 = dout.astype(np.float64), z.astype(np.float64)
        ref = np.einsum("bil,bjl->ij", d64, z64)
        if kind == "int":
            assert np.array_equal(got, ref), (B, n, got, ref)
        else:
            tol = (B * n + 2) * 2 * U * np.einsum("bil,bjl->ij", np.abs(d64), np.abs(z64))
            err = np.abs(got - ref)
            worst = max(worst, _worst(err, tol))
            assert (err <= tol).all(), (B, n)
    if kind == "random":
        print("conv1x1_wgrad c %d: worst err/tol %.4f" % (c, worst))


def test_conv1x1_wgrad_rejects_a_short_workspace_and_other_channel_counts():
    lib, L = _lib()
    x, dw = dev_input(np.zeros((1, 10, 8), np.float32)), dev_output(100)
    nbytes = L.facppg_conv1x1_wgrad_workspace_bytes(4)
    ws = dev_workspace(nbytes)
    assert L.facppg_conv1x1_wgrad(lib.ptr(x), lib.ptr(x), lib.ptr(dw), 1, 4, 8, lib.ptr(ws), nbytes - 1, _stream()) == wh.EWORKSPACE
    big = dev_workspace(L.facppg_conv1x1_wgrad_workspace_bytes(10))
    for c in (3, 10):
        assert L.facppg_conv1x1_wgrad(lib.ptr(x), lib.ptr(x), lib.ptr(dw), 1, c, 8, lib.ptr(big), big.numel(), _stream()) == wh.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw[:100]).all()) and guard_intact(dw, 100) and bool((ws[:nbytes] == 0xFF).all())


# ------------------------------------------------------------------------------------------------- the affine coupling
@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_affine_forward_and_backward(h):
    """y = [x0 | exp(log_s) x1 + b], wn = [b | log_s];  dx = [dy0 | dy1 e],  dwn = [dy1 | dy1 e x1]"""
    lib, L = _lib()
    worst = {"y": 0.0, "dx": 0.0, "dwn": 0.0}
    for B in (1, 3):
        for n in (1, 3, 4, 5, 1024, 1025):
            g = _rng(h, B, n, 11)
            x, dy = _data(g, (B, 2 * h, n), "random"), _data(g, (B, 2 * h, n), "random")
            wn = np.concatenate([_data(g, (B, h, n), "random"), g.uniform(-6, 6, (B, h, n)).astype(np.float32)], axis=1)
            N = B * 2 * h * n
            xd, wd, dyd, y, dx, dwn = dev_input(x), dev_input(wn), dev_input(dy), dev_output(N), dev_output(N), dev_output(N)
            rc = L.facppg_affine_forward(lib.ptr(xd), lib.ptr(wd), lib.ptr(y), B, h, n, _stream())
            assert rc == wh.OK, (rc, wh.last_error())
            rc = L.facppg_affine_backward(lib.ptr(xd), lib.ptr(wd), lib.ptr(dyd), lib.ptr(dx), lib.ptr(dwn), B, h, n, _stream())
            assert rc == wh.OK, (rc, wh.last_error())
            torch.cuda.synchronize()
            assert guard_intact(y, N) and guard_intact(dx, N) and guard_intact(dwn, N), (B, n)
            yh, dxh, dwnh = (host(t, (B, 2 * h, n)) for t in (y, dx, dwn))
            # the pass-through halves: equal bits
            assert np.array_equal(yh[:, :h].view(np.uint32), x[:, :h].view(np.uint32))
            assert np.array_equal(dxh[:, :h].view(np.uint32), dy[:, :h].view(np.uint32))
            assert np.array_equal(dwnh[:, :h].view(np.uint32), dy[:, h:].view(np.uint32))
            ls, b, x1, d1 = (a.astype(np.float64) for a in (wn[:, h:], wn[:, :h], x[:, h:], dy[:, h:]))
            e = np.exp(ls)
            k = (4 + 2 * np.abs(ls)) * U
            for name, got, ref, mag in (("y", yh[:, h:], e * x1 + b, np.abs(e * x1) + np.abs(b)), ("dx", dxh[:, h:], d1 * e, np.abs(d1 * e)),
                                        ("dwn", dwnh[:, h:], d1 * e * x1, np.abs(d1 * e * x1))):
                err, tol = np.abs(got - ref), k * mag
                worst[name] = max(worst[name], _worst(err, tol))
                assert (err <= tol).all(), (name, B, n)
    print("affine h %d: worst err/tol %s" % (h, " ".join("%s %.3f" % kv for kv in worst.items())))


def test_affine_rejects_bad_arguments():
    lib, L = _lib()
    x = dev_input(np.zeros(8, np.float32))
    assert L.facppg_affine_forward(lib.ptr(x), lib.ptr(x), lib.ptr(x), 1, 0, 4, _stream()) == wh.EINVAL
    assert L.facppg_affine_backward(lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(x), None, 1, 1, 4, _stream()) == wh.EINVAL


# ---------------------------------------------------------------------------------------------------------- weight norm
# (rows, row length, floats skipped in front of the tensor in every flat buffer).  2 / 3 / 4: the start convs (4: the vector
# path with one live lane); 256 / 640 / 768 / 1024: the vector path; 1023 / 1028: the scalar path; (3, 640, 1): a row length
# that is a multiple of 4 at a base one float off a 16-byte boundary -- wn_vec_row must fall back; (4, 256, 3): off a boundary
# in the forward, in the backward only its dv is.  27 rows: not a multiple of 4.
WN_TENSORS = ((1, 2, 0), (5, 3, 0), (2, 4, 0), (1, 256, 0), (3, 640, 0), (2, 768, 0), (1, 1024, 0), (3, 1023, 0), (2, 1028, 0), (3, 640, 1),
              (4, 256, 3))


def _wn_layout(skip_of):
    """-> (offsets of the tensors in a flat float buffer whose base is 16-byte aligned, total floats): every tensor starts on
    a 16-byte boundary plus its skip"""
    offs, o = [], 0
    for t, (rows, ln, _) in enumerate(WN_TENSORS):
        o = wh.round_up(o, 4) + skip_of(t)
        offs.append(o)
        o += rows * ln
    return offs, o


def _wn_table(entries):
    """as waveglow/glow.py packs it: six 8-byte words per tensor, {v, g, w, norm, first row, rows | len << 32}"""
    t = np.zeros((len(entries), 6), dtype=np.int64)
    row0 = 0
    for i, (v, g, w, norm, rows, ln) in enumerate(entries):
        t[i] = (v, g, w, norm, row0, rows | (ln << 32))
        row0 += rows
    return torch.from_numpy(t).cuda(), row0


def _wn_flat(g, offs, total, what):
    a = np.full(total, np.nan, dtype=np.float32)
    for o, (rows, ln, _) in zip(offs, WN_TENSORS):
        a[o:o + rows * ln] = g.standard_normal(rows * ln, dtype=np.float32) * (0.1 if what == "v" else 1.0)
    return a


def _n_sum(ln):
    """roundings a row sum can meet on any path: a chain of at most ceil(len / 64) FMAs per lane, then a 6-level tree"""
    return math.ceil(ln / 64) + 6


def test_weight_norm_forward_and_backward():
    lib, L = _lib()
    g = _rng(2024)
    skips = [s for _, _, s in WN_TENSORS]
    offs, total = _wn_layout(lambda t: skips[t])
    roffs, rtotal = [], 0
    for rows, _, _ in WN_TENSORS:                     # g, norm, dg: one float per row, tensors two floats apart
        roffs.append(rtotal)
        rtotal += rows + 2
    v, dw = _wn_flat(g, offs, total, "v"), _wn_flat(g, offs, total, "dw")
    gv = np.full(rtotal, np.nan, dtype=np.float32)
    for o, (rows, _, _) in zip(roffs, WN_TENSORS):
        gv[o:o + rows] = g.standard_normal(rows, dtype=np.float32)
    vd, gd, wout, nout = dev_input(v), dev_input(gv), dev_output(total), dev_output(rtotal)
    assert vd.data_ptr() % 16 == 0 and wout.data_ptr() % 16 == 0
    at = lambda t, o: t.data_ptr() + 4 * o
    table, rows_total = _wn_table([(at(vd, o), at(gd, r), at(wout, o), at(nout, r), rows, ln) for o, r, (rows, ln, _) in zip(offs, roffs, WN_TENSORS)])
    assert rows_total % 4 != 0
    rc = L.facppg_weight_norm_forward(lib.ptr(table), len(WN_TENSORS), rows_total, _stream())
    torch.cuda.synchronize()
    assert rc == wh.OK, (rc, wh.last_error())
    assert guard_intact(wout, total) and guard_intact(nout, rtotal)
    wh_, nh = host(wout, (total,)), host(nout, (rtotal,))
    covered, rcovered = np.zeros(total, bool), np.zeros(rtotal, bool)
    worst = {"w": 0.0, "norm": 0.0, "dv": 0.0, "dg": 0.0}
    norms = np.full(rtotal, np.nan, dtype=np.float32)
    for o, r, (rows, ln, _) in zip(offs, roffs, WN_TENSORS):
        covered[o:o + rows * ln], rcovered[r:r + rows] = True, True
        v64, g64 = v[o:o + rows * ln].reshape(rows, ln).astype(np.float64), gv[r:r + rows].astype(np.float64)
        norm = np.sqrt((v64 * v64).sum(1))
        w = g64[:, None] * v64 / norm[:, None]
        n = _n_sum(ln)
        # sum of squares: relative n u (every term positive); sqrt halves it and rounds once; g / norm, v * sc: one u each;
        # one more u for the second-order terms
        e_n, t_n = np.abs(nh[r:r + rows] - norm), (n / 2 + 2) * U * norm
        e_w, t_w = np.abs(wh_[o:o + rows * ln].reshape(rows, ln) - w), (n / 2 + 4) * U * np.abs(w)
        worst["norm"], worst["w"] = max(worst["norm"], _worst(e_n, t_n)), max(worst["w"], _worst(e_w, t_w))
        assert (e_n <= t_n).all() and (e_w <= t_w).all(), (rows, ln)
        norms[r:r + rows] = norm.astype(np.float32)
    assert np.isnan(wh_[~covered]).all() and np.isnan(nh[~rcovered]).all(), "rows that no table entry covers must stay untouched"

    # backward: dg = <dw, v> / norm, dv = (g / norm) dw - (g <dw, v> / norm^3) v, with the norm the forward kept.  dv sits at
    # its own offsets: the last tensor's v and dw are 16-byte aligned there and only its dv is not.
    doffs, dtotal = _wn_layout(lambda t: 1 if t == len(WN_TENSORS) - 1 else skips[t])
    offs_b, total_b = _wn_layout(lambda t: 0 if t == len(WN_TENSORS) - 1 else skips[t])
    vb, dwb = np.full(total_b, np.nan, dtype=np.float32), np.full(total_b, np.nan, dtype=np.float32)
    for o, ob, (rows, ln, _) in zip(offs, offs_b, WN_TENSORS):
        vb[ob:ob + rows * ln], dwb[ob:ob + rows * ln] = v[o:o + rows * ln], dw[o:o + rows * ln]
    vbd, dwd, nd, dv, dg = dev_input(vb), dev_input(dwb), dev_input(norms), dev_output(dtotal), dev_output(rtotal)
    tin, _ = _wn_table([(at(vbd, o), at(gd, r), at(dwd, o), at(nd, r), rows, ln) for o, r, (rows, ln, _) in zip(offs_b, roffs, WN_TENSORS)])
    tout, _ = _wn_table([(at(dv, o), at(dg, r), 0, 0, rows, ln) for o, r, (rows, ln, _) in zip(doffs, roffs, WN_TENSORS)])
    rc = L.facppg_weight_norm_backward(lib.ptr(tin), lib.ptr(tout), len(WN_TENSORS), rows_total, _stream())
    torch.cuda.synchronize()
    assert rc == wh.OK, (rc, wh.last_error())
    assert guard_intact(dv, dtotal) and guard_intact(dg, rtotal)
    dvh, dgh = host(dv, (dtotal,)), host(dg, (rtotal,))
    dcovered = np.zeros(dtotal, bool)
    for o, do, r, (rows, ln, _) in zip(offs, doffs, roffs, WN_TENSORS):
        dcovered[do:do + rows * ln] = True
        v64, d64 = (a[o:o + rows * ln].reshape(rows, ln).astype(np.float64) for a in (v, dw))
        g64, nm = gv[r:r + rows].astype(np.float64)[:, None], norms[r:r + rows].astype(np.float64)[:, None]
        dot, S = (d64 * v64).sum(1, keepdims=True), np.abs(d64 * v64).sum(1, keepdims=True)
        E = _n_sum(ln) * U * S                                       # the dot product, whatever the order
        a, bq = g64 / nm, g64 * dot / nm ** 3
        ref_dg, ref_dv = dot / nm, a * d64 - bq * v64
        # dg: the dot's error over norm, one division.  dv: a (1 u) times dw (1 u); bq = g dot (1 u) / norm^3 (2 u, 1 u for the
        # division) times v (1 u), its dot carrying E; the subtraction (1 u); one more u on each product for second-order terms
        t_dg = E / nm + 2 * U * np.abs(ref_dg)
        t_dv = 3 * U * np.abs(a * d64) + 6 * U * np.abs(bq * v64) + np.abs(v64) * np.abs(g64) * E / nm ** 3 + U * np.abs(ref_dv)
        e_dg, e_dv = np.abs(dgh[r:r + rows][:, None] - ref_dg), np.abs(dvh[do:do + rows * ln].reshape(rows, ln) - ref_dv)
        worst["dg"], worst["dv"] = max(worst["dg"], _worst(e_dg, t_dg)), max(worst["dv"], _worst(e_dv, t_dv))
        assert (e_dg <= t_dg).all() and (e_dv <= t_dv).all(), (rows, ln)
    assert np.isnan(dvh[~dcovered]).all() and np.isnan(dgh[~rcovered]).all()
    print("weight norm: worst err/tol %s" % " ".join("%s %.3f" % kv for kv in worst.items()))


def test_weight_norm_rejects_empty_tables():
    lib, L = _lib()
    t = torch.zeros(6, dtype=torch.int64, device="cuda")
    assert L.facppg_weight_norm_forward(lib.ptr(t), 0, 4, _stream()) == wh.EINVAL
    assert L.facppg_weight_norm_backward(lib.ptr(t), None, 1, 4, _stream()) == wh.EINVAL


# --------------------------------------------------------------------------------------------------------- segment sums
# (outer, inner, outer_stride): totals of 1, 5, 63, 64, 65 and 100 003 elements -- fewer elements than the 64 slices, uneven
# slices; outer_stride > inner is the log_s layout (the upper half of a flow's WN output), NaN in the gaps
SEGMENTS = ((1, 1, 1), (5, 1, 3), (1, 5, 5), (7, 9, 12), (8, 8, 11), (5, 13, 20), (100003, 1, 2), (1, 100003, 100003))


def _segments(n, g):
    lib, _ = _lib()
    segs, keep, want = (lib.SumSegment * max(n, 1))(), [], []
    for e in range(n):
        outer, inner, stride = SEGMENTS[e % len(SEGMENTS)]
        square = (e // len(SEGMENTS) + e) % 2
        a = np.full((outer, stride), np.nan, dtype=np.float32)
        a[:, :inner] = g.standard_normal((outer, inner), dtype=np.float32) + np.float32(0.25)
        t = dev_input(a)
        keep.append(t)
        segs[e].data_dev, segs[e].outer_stride, segs[e].outer, segs[e].inner, segs[e].square = t.data_ptr(), stride, outer, inner, square
        live = a[:, :inner].astype(np.float64)
        want.append((live * live).sum() if square else live.sum())
    return segs, keep, np.array(want)


@pytest.mark.parametrize("n", [1, 8, 16])
def test_segment_sums(n):
    lib, L = _lib()
    segs, keep, want = _segments(n, _rng(n, 5))
    nbytes = n * 64 * 8
    ws, out = dev_workspace(nbytes), dev_output(n)
    rc = L.facppg_segment_sums(segs, n, lib.ptr(ws), nbytes, lib.ptr(out), _stream())
    torch.cuda.synchronize()
    assert rc == wh.OK, (rc, wh.last_error())
    assert guard_intact(ws, nbytes) and guard_intact(out, n)
    got = host(out, (n,))
    want32 = want.astype(np.float32)
    ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
    print("segment sums, %d segments: worst distance from the rounded float64 sum %.1f ulp" % (n, ulps.max()))
    assert (ulps <= 1).all(), (got, want)


def test_segment_sums_rejects_17_segments_and_a_short_workspace():
    lib, L = _lib()
    segs, keep, _ = _segments(16, _rng(3))
    more = (lib.SumSegment * 17)(*list(segs), segs[0])
    ws, out = dev_workspace(17 * 64 * 8), dev_output(17)
    assert L.facppg_segment_sums(more, 17, lib.ptr(ws), 17 * 64 * 8, lib.ptr(out), _stream()) == wh.EINVAL
    assert L.facppg_segment_sums(segs, 16, lib.ptr(ws), 16 * 64 * 8 - 1, lib.ptr(out), _stream()) == wh.EINVAL
    assert "workspace" in wh.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:17]).all()) and bool((ws[:17 * 64 * 8] == 0xFF).all())
