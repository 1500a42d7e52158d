"""k_gemm, k_gemm_lat, k_gemm_reduce and k_pack_a (csrc/facppg_gemm.hip) held directly to a float64 reference of
facppg_gemm.h's contract, through the test-only probe library (tests/native/gemm_probe.hip; gemm_helpers.py has the
binding, the reference, the case lists and the runner that poisons everything around the operands).

Exact class: small integer operands make every fp32 sum exact in any order (test_gemm_reference_cpu.py computes the
condition per case), so indexing, windows, padding, split-K and the epilogue are compared with np.array_equal -- no
tolerance.  Rounding class: standard normal operands against the textbook bound (K + 2) * 2u * sum|w||x| plus one u per
affine epilogue step, u = 2^-24.  Every launch of at most 256 columns runs as k_gemm_lat and again as k_gemm
(FACPPG_GEMM_SHAPE=legacy): each is compared to float64 on its own, and the two buffers must be equal bit for bit.

Not tested: the dispatch guard Cin * ldx + N >= 2^31 (sends a launch to k_gemm whatever its width); reaching it takes an
operand of more than 8 GB."""
import dataclasses

import numpy as np
import pytest

import gemm_helpers as gh
from gemm_helpers import Case, U

pytestmark = pytest.mark.gpu

# Allowance for the device's tanhf / logf in the activation tests, in float32 ulps of the result: twice the largest distance
# from float64 that test_device_tanh_and_log_against_float64 measures (identity product, 4096 inputs each: the output is the
# device function of the input itself).  Measured on gfx950: tanhf 0.970 ulp over [-9, 9]; logf 2.104 ulp over [1e-6, 1e3]
# (1.641 ulp at the clamp, log(1e-5f)).  Rounded up to two digits.
TANH_ALLOW_ULPS = 2.0
LOG_ALLOW_ULPS = 4.3


def expected_out(cs, r):
    """the float64 reference as the runner's out array: SENTINEL where the launch may not write"""
    win = np.concatenate([r.win, r.win], 1) if cs.gate else r.win
    e = np.full(win.shape, gh.SENTINEL, np.float32)
    e[win] = r.v[win].astype(np.float32)
    return e, win


@pytest.mark.parametrize("cs", gh.EXACT_CASES, ids=lambda cs: cs.id)
def test_exact(cs):
    r = gh.reference(cs)
    want, win = expected_out(cs, r)
    if cs.skip:
        assert not win.any()
    for name, run in gh.run_shapes(cs).items():
        bad = np.flatnonzero(run.out != want)
        assert bad.size == 0, "%s: %d of %d elements differ from float64, first %s: got %r, want %r" % (
            name, bad.size, int(win.sum()), np.unravel_index(bad[0], want.shape), run.out.flat[bad[0]], want.flat[bad[0]])


@pytest.mark.parametrize("cs", gh.PACK_CASES, ids=lambda cs: cs.id)
def test_packed_image(cs):
    """pack_a / pack_a_strided against facppg_gemm.h's index formula, the zero padding of k >= K, of rows >= M and of the extra
    k-group included; the trailing 3 * 64 float4 are unspecified."""
    run = gh.run_case(cs)
    want = gh.packed_image(gh.make_data(cs).W).reshape(-1)
    assert want.size == run.packed_floats - 3 * 64 * 4
    assert np.array_equal(run.packed[:want.size], want)


def _single(cs, d, b):
    """batch entry b of (cs, d) as a launch of its own"""
    one = dataclasses.replace(cs, B=1, n_valid=None if cs.n_valid is None else (cs.n_valid[b],), x_shared=False, tag=cs.tag + "row%d" % b)
    sl = lambda a: None if a is None else a[b:b + 1]
    return one, gh.Data(W=d.W, X=d.X[0:1] if cs.x_shared else d.X[b:b + 1], bias=d.bias, scale=d.scale, shift=d.shift,
                        mask=sl(d.mask), res=sl(d.res), gate=sl(d.gate))


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("data", ["int", "normal"])
@pytest.mark.parametrize("kind", ["ragged", "muladd", "shared"])
def test_batch_row_equals_single_run(kind, data, split):
    """facppg_gemm.h: a padded batch equals independent batch-1 runs -- bit for bit, rounding included (the split factor
    depends on K alone)."""
    kw = dict(Cin=128, taps=5, pad=2, N=65, B=3, split=split, data=data, bias=True, affine=True, mask=True, res=True, tag="rows")
    cs = {"ragged": Case(n_valid=(65, 0, 17), **kw),
          "muladd": Case(n_valid=(40, 2, 9), mul=2, add=-1, src_hi=72, **kw),
          "shared": Case(n_valid=(65, 31, 33), x_shared=True, **kw)}[kind]
    d = gh.make_data(cs)
    batch = gh.run_shapes(cs, d)
    for b in range(cs.B):
        one, d1 = _single(cs, d, b)
        for name, run in gh.run_shapes(one, d1).items():
            assert np.array_equal(run.out[0], batch[name].out[b]), (name, b)


@pytest.mark.parametrize("cs", gh.ROUNDING_CASES, ids=lambda cs: cs.id)
def test_rounding(cs):
    r = gh.reference(cs)
    win = r.win
    live = win & (r.S_out > 0)
    assert live.any()
    for name, run in gh.run_shapes(cs).items():
        err = np.abs(run.out.astype(np.float64) - r.v)
        over = win & (err > r.tol)
        ratio = err[live] / (U * r.S_out[live])
        rms = float(np.sqrt(np.mean(ratio * ratio)))
        print("%s %s: max err/tol %.3g, rms err/(u S) %.3g (sqrt K = %.3g), median err %.3g" % (
            cs.id, name, float((err[win] / np.maximum(r.tol[win], 1e-300)).max()), rms, cs.K ** 0.5, float(np.median(err[live]))))
        assert not over.any(), "%s: %d elements beyond the bound, worst err / tol = %.3g" % (
            name, int(over.sum()), float((err[over] / r.tol[over]).max()))
        assert rms < cs.K ** 0.5           # the bound is not being leaned on
        if cs.K >= 512:
            assert np.median(err[live]) > 0   # ... and the comparison is not vacuous


def _act_f(act, v):
    return np.tanh(v) if act == gh.ACT_TANH else np.log(np.maximum(v, gh.LOG_FLOOR))


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("K", [40, 640])
@pytest.mark.parametrize("act", [gh.ACT_TANH, gh.ACT_LOG_CLAMP], ids=["tanh", "logclamp"])
def test_activation(act, K, split):
    """f over [v - tol, v + tol] in float64 (both are monotone), widened by the device function's own allowance.  The
    arguments spread over (-20, 20) at K = 40: tanh through its whole range, the log half below its clamp, between the clamp and 1 and above 1.  The argument
    exactly AT the clamp (and its two float32 neighbours) is in test_device_tanh_and_log_against_float64, whose identity
    product hands the kernel the exact value."""
    cs = Case(Cin=K // 5, taps=5, pad=2, split=split, data="normal", bias=True, affine=K == 640, act=act, tag="act")
    r = gh.reference(cs)
    lo, hi = _act_f(act, r.v_act - r.tol_act), _act_f(act, r.v_act + r.tol_act)
    allow = TANH_ALLOW_ULPS if act == gh.ACT_TANH else LOG_ALLOW_ULPS
    A = allow * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    if act == gh.ACT_LOG_CLAMP:
        assert (r.v_act < gh.LOG_FLOOR).any() and (r.v_act > 1.0).any() and ((r.v_act > gh.LOG_FLOOR) & (r.v_act < 1.0)).any()
    for name, run in gh.run_shapes(cs).items():
        out = run.out.astype(np.float64)
        assert ((out >= lo - A) & (out <= hi + A))[r.win].all(), name


def _identity_run(act, x):
    """W = I_32, K = 32: exact, the output is the device's f(x) itself"""
    assert x.size == 4096 and x.dtype == np.float32
    cs = Case(M=32, Cin=32, taps=1, N=128, act=act, tag="identity")
    d = gh.Data(W=np.eye(32, dtype=np.float32).reshape(32, 32, 1), X=x.reshape(1, 32, 128))
    runs = gh.run_shapes(cs, d)
    return runs["default"].out.reshape(-1)


def test_device_tanh_and_log_against_float64():
    """The measurement behind TANH_ALLOW_ULPS / LOG_ALLOW_ULPS (math library against float64, not the GEMM against itself):
    the allowances are twice what is seen here, so the largest distance must stay within half of them."""
    x = np.linspace(-9.0, 9.0, 4096).astype(np.float32)
    t = gh.ulp_distance(_identity_run(gh.ACT_TANH, x), np.tanh(x.astype(np.float64)))
    x = np.geomspace(1e-6, 1e3, 4096).astype(np.float32)
    floor = np.float32(1e-5)
    i = int(np.searchsorted(x, floor))
    x[i - 1:i + 2] = [np.nextafter(floor, np.float32(0)), floor, np.nextafter(floor, np.float32(1))]   # below, at, above the clamp
    out = _identity_run(gh.ACT_LOG_CLAMP, x)
    ref = np.log(np.maximum(x.astype(np.float64), gh.LOG_FLOOR))
    lg = gh.ulp_distance(out, ref)
    below = x <= floor
    assert below.sum() > 100 and np.unique(out[below]).size == 1
    print("tanhf: max %.3f ulp; logf: max %.3f ulp (clamped inputs: %.3f)" % (t.max(), lg.max(), lg[below].max()))
    assert 2 * t.max() <= TANH_ALLOW_ULPS
    assert 2 * lg.max() <= LOG_ALLOW_ULPS
