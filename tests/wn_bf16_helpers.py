"""The bf16 training direction of one WaveGlow WN stack (csrc/facppg_train_bf16.hip: facppg_wn_forward_bf16,
facppg_wn_backward_bf16) held to a float64 reference STAGE BY STAGE: the case list, the bf16 tools, the staged reference, the
acceptance functions and a runner that surrounds every buffer with poison -- shared by test_wn_bf16_reference_cpu.py and
test_gpu_wn_bf16.py.  Operands, weight shapes, the autograd reference and the poisoned device buffers are wn_train_helpers'.

Why staged.  A last-bit difference flips a bf16 rounding and travels through eight layers, so a whole-stack comparison needs a
tolerance (2e-2 of a tensor's maximum, test_gpu_train_bf16.py) under which one wrong row, chunk or slice disappears.  Here every
stage's float64 reference starts from the bits the KERNEL stored for the stage before (read out of `state` and `scratch` at the
offsets facppg_wn_bf16_layout reports), so the only admissible deviation is one bf16 rounding of a value that is within the fp32
summation bound of the reference.

Stages, position-major ([B, L, channels]; n + s outside [0, L) reads zero), as the kernels compute them (k_t_start, k_bgemm's
epilogues bgemm_store4, k_wn_fwd, k_wn_bwd, k_dspect, k_wgrad, k_colsum_*, k_t_end, k_t_end_bwd, k_t_start_bwd, k_small_*):
    h.0      = bf16(a0 Ws^T + bs)                                                     fp32 weights
    pre.i    = (b_in + b_cond) + sum_tap h.i[n + (tap - 1) 2^i] Win_i[:, :, tap]^T + spect Wc_i^T      bf16 weights
    ts.i     = bf16(T | S),  T = tanh(clamp(pre_t, +-15)), S = sigmoid(pre_s);   acts.i = bf16(T S)    (T, S unrounded)
    h.(i+1)  = bf16(h.i + acts.i Wrs_i[:256]^T + b)          skip = sum_i (acts.i Wrs_i[skip rows]^T + b)  fp32
    out      = skip We^T + be                                                          fp32 weights
    dskip    = bf16(dout We)
    dpre.i   = bf16(gate'(ts.i) * ([dh.(i+1) | dskip] Wrs_i)),  gate' = (S (1 - T^2) | T S (1 - S))   (last layer: dskip alone)
    dh.i     = bf16(dh.(i+1) + sum_tap dpre.i[n - (tap - 1) 2^i] Win_i[:, :, tap])
    dspect   = (previous +) sum_i dpre.i Wc_i              da0 = dh.0 Ws
    g.*      = the NT products over (b, n) and the column sums of the same buffers (in_b and cond_b share one sum; the skip
               half of every rs_b is the column sum of dskip)
Acceptance of a bf16 output g with reference r and fp32 error bound d: bf16(r - d) <= g <= bf16(r + d), i.e. g is the rounding
of SOME value within d of r; of an fp32 output: |g - r| <= d.  d = (K + 2) 2 U S for K terms with S = sum |a| |x| + the
epilogue's |addends|, carried through the gate with |dT/dx| <= 1, |dS/dy| <= 1/4 plus MARGIN x the error the gate's own
formula has in float32 (GATE_ERR_T, GATE_ERR_S: measured on the CPU, see measure_gate_error).  On top, per stage, the share of
elements whose bits differ from bf16(r) may be MARGIN x the number the same stage has when evaluated in float32 on the CPU,
plus MISMATCH_FLOOR = 8 elements (mismatch_allowance)."""
import collections
import dataclasses
import functools
import hashlib

import numpy as np
import pytest

import wn_train_helpers as wt
from upsample_helpers import bf16_bits, bf16_to_f64
from wn_train_helpers import CH, NC, HALO, U, MARGIN, GUARD, OK, EWORKSPACE, weight_shapes

K1 = 3 * CH + NC
SWITCHES = ("FACPPG_TRAIN_FUSED_FWD", "FACPPG_TRAIN_FUSED_BWD", "FACPPG_TRAIN_TILE", "FACPPG_WGRAD_TILE", "FACPPG_TRAIN_DSPECT_BGEMM",
            "FACPPG_WGRAD_NO_XCD_MAP", "FACPPG_TRAIN_PACK", "FACPPG_WN_FWD_STAMPS", "FACPPG_WN_BWD_STAMPS", "FACPPG_WGRAD_STAMPS")
STRUCTURES = collections.OrderedDict([
    ("two", {"FACPPG_TRAIN_FUSED_FWD": "0", "FACPPG_TRAIN_FUSED_BWD": "0", "FACPPG_TRAIN_DSPECT_BGEMM": "1", "FACPPG_WGRAD_TILE": "128",
             "FACPPG_WGRAD_NO_XCD_MAP": "1"}),
    ("fused64", {"FACPPG_TRAIN_FUSED_FWD": "1", "FACPPG_TRAIN_FUSED_BWD": "1", "FACPPG_TRAIN_TILE": "64", "FACPPG_WGRAD_TILE": "256",
                 "FACPPG_TRAIN_DSPECT_BGEMM": "0"}),
    ("fused32", {"FACPPG_TRAIN_FUSED_FWD": "1", "FACPPG_TRAIN_FUSED_BWD": "1", "FACPPG_TRAIN_TILE": "32", "FACPPG_WGRAD_TILE": "128"}),
    ("default", {}),
])

# G: the absolute error of gate_ts's formula evaluated in float32 (NumPy's exp2 and division) against float64, worst over the
# pre-activations of every case's reference, the wide case included: 2.29 U for T, 1.59 U for S, pinned at that, rounded up to a
# tenth of U (measure_gate_error; test_wn_bf16_reference_cpu.py re-measures all of these cases and holds them under the
# constants).  The hardware's v_exp_f32 and v_rcp_f32 are about an ulp worse each: the kernels get MARGIN times this.
GATE_ERR_T = 2.3 * U
GATE_ERR_S = 1.6 * U


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    n_in: int
    n_layers: int
    B: int
    L: int
    accumulate: bool = False      # accumulate_dspect = 1 onto a random previous buffer

    @property
    def id(self):
        return "in%d-nl%d-B%d-L%d%s" % (self.n_in, self.n_layers, self.B, self.L, "-acc" if self.accumulate else "")

    @property
    def operands_key(self):
        return wt.Case(self.n_in, self.n_layers, self.B, self.L, "random")


_ONE = ((1, 1, 1, 1), (2, 1, 2, 31), (3, 1, 1, 32), (4, 1, 3, 33), (1, 1, 2, 63), (2, 1, 1, 64), (3, 1, 2, 65), (4, 1, 1, 127), (1, 1, 1, 128),
        (2, 1, 3, 129), (4, 1, 2, 240))
_FEW = ((3, 2, 2, 1), (4, 2, 1, 63), (1, 2, 3, 129), (2, 2, 2, 150), (2, 3, 1, 65))
_EIGHT = ((2, 8, 1, 1), (1, 8, 1, 63), (3, 8, 2, 65), (4, 8, 1, 127), (4, 8, 2, 128), (2, 8, 1, 129), (4, 8, 2, 257))
_ACCUMULATE = ((4, 1, 3, 33), (1, 2, 3, 129), (2, 3, 1, 65), (3, 8, 2, 65), (2, 8, 1, 1))      # one per layer count, and L = 1
CASES = tuple(Case(*c) for c in _ONE + _FEW + _EIGHT) + tuple(Case(*c, accumulate=True) for c in _ACCUMULATE)
SMALL_CPU_CASES = (Case(3, 1, 2, 5), Case(2, 2, 1, 37), Case(4, 8, 1, 70))      # the last: 8 layers, L < 128


def wide_case():
    """The smallest L at B = 12, n_layers = 2 at which EVERY k_bgemm launch of the two-launch structure takes 128-column tiles,
    found in the plan itself (facppg_train_bf16_launch_plan under the `two` switches).  plan_bgemm: ceil(L / 128) nm B >= 384 with
    nm = 2 row tiles for the 256-row products, i.e. ceil(L / 128) >= 16."""
    from facppg import lib
    B, nl = 12, 2
    with pytest.MonkeyPatch.context() as mp:
        set_structure(mp, "two")
        r = lib.TrainLaunchReport()

        def all_wide(L):
            assert lib.load().facppg_train_bf16_launch_plan(nl, B, L, r) == 0
            return all(c == 128 for c in r.gemm_cols) and r.dspect_bgemm == 1 and r.dspect_cols == 128
        L = next(L for L in range(1, 1 << 14) if all_wide(L))
        assert not all_wide(L - 1)
    return Case(4, nl, B, L)


def set_structure(mp, name):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in STRUCTURES[name].items():
        mp.setenv(k, v)


# ----------------------------------------------------------------------------------------------------------- bf16 tools
BF16_MAX = 3.3895313892515355e38          # (2 - 2^-7) 2^127


def _bf16_round_any(x):
    """the general form: frexp, rint (ties to even) at 8 significant bits, fixed spacing 2^-133 in the subnormal range"""
    _, e = np.frexp(x)                                    # x = m 2^e, 0.5 <= |m| < 1
    e = np.maximum(e, -125)
    r = np.ldexp(np.rint(np.ldexp(x, 8 - e)), e - 8)
    r = np.where(np.abs(r) > BF16_MAX, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def bf16_round(x):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even, subnormals below 2^-126, infinity beyond the largest
    finite value), as float64.  One rounding: no detour through float32.  Normal range: round-to-nearest-even on the bit pattern
    (bf16 keeps 7 of the 52 fraction bits; the exponent ranges nest, a carry into the exponent is the right binade); everything
    else -- zeros, the subnormal range, overflow, infinities, NaN -- takes the general form."""
    x = np.asarray(x, dtype=np.float64)
    flat = np.ascontiguousarray(x).reshape(-1)
    b = flat.view(np.uint64)
    r = ((b + np.uint64(0x0FFFFFFFFFFF) + ((b >> np.uint64(45)) & np.uint64(1))) & np.uint64(0xFFFFE00000000000)).view(np.float64)
    with np.errstate(invalid="ignore"):
        special = ~((np.abs(flat) >= 2.0 ** -126) & (np.abs(r) <= BF16_MAX))
    if special.any():
        r[special] = _bf16_round_any(flat[special])
    return r.reshape(x.shape)


def identity(x):
    return np.asarray(x, dtype=np.float64)


# -------------------------------------------------------------------------------------------------------- the gate
def gate_f64(pre):
    return np.concatenate([np.tanh(np.clip(pre[..., :CH], -15.0, 15.0)), 1.0 / (1.0 + np.exp(-pre[..., CH:]))], axis=-1)


def gate_f32(pre):
    """gate_ts of the kernels in NumPy float32: the same clamp, the same constants, (1 - e) / (1 + e) and 1 / (1 + e)"""
    pre = np.asarray(pre, dtype=np.float32)
    one = np.float32(1.0)
    ea = np.exp2(np.clip(pre[..., :CH], np.float32(-15.0), np.float32(15.0)) * np.float32(-2.8853900817779268))
    T = (one - ea) * (one / (one + ea))
    S = one / (one + np.exp2(pre[..., CH:] * np.float32(-1.4426950408889634)))
    return np.concatenate([T, S], axis=-1)


def measure_gate_error(pre):
    """-> (worst |T32 - T64|, worst |S32 - S64|) of gate_f32 over float64 pre-activations (rounded to float32 first: the kernel's
    accumulator is a float32, whose distance from the float64 sum the summation bound already covers)"""
    p32 = np.asarray(pre, dtype=np.float32)
    d = np.abs(gate_f32(p32).astype(np.float64) - gate_f64(p32.astype(np.float64)))
    return float(d[..., :CH].max()), float(d[..., CH:].max())


# ------------------------------------------------------------------------------------------------------------ reference
Ref = collections.namedtuple("Ref", "r delta emu kind")      # float64 reference, bound, the stage in float32 on the CPU, "bf16" | "f32"


def _shift(x, s):
    """y[:, n] = x[:, n + s], zero outside"""
    if s == 0:
        return x
    y = np.zeros_like(x)
    L = x.shape[1]
    if abs(s) < L:
        if s > 0:
            y[:, :L - s] = x[:, s:]
        else:
            y[:, -s:] = x[:, :L + s]
    return y


def _bound(K, S):
    return (K + 2) * 2 * U * np.asarray(S, dtype=np.float64) * (1 + 2.0 ** -10)     # (S itself is summed in float32)


class _Arith:
    """One arithmetic for the linear parts: float64 (the reference), float32 (the CPU's fp32 evaluation) or float32 on absolute
    values (the S of the bounds)."""

    def __init__(self, dt, absolute=False):
        self.dt, self.absolute = dt, absolute

    def __call__(self, x):
        x = np.asarray(x, dtype=self.dt)
        return np.abs(x) if self.absolute else x

    def mm(self, x, w):          # [B, L, K] x [K, M] -> [B, L, M]
        x, w = np.ascontiguousarray(self(x)), np.ascontiguousarray(self(w))      # (strided views would leave BLAS)
        return (x.reshape(-1, x.shape[-1]) @ w).reshape(x.shape[:-1] + (w.shape[-1],))

    def nt(self, y, x):          # [B, L, M], [B, L, K] -> [M, K]: sum over (b, n)
        y, x = np.ascontiguousarray(self(y)), np.ascontiguousarray(self(x))
        return y.reshape(-1, y.shape[-1]).T @ x.reshape(-1, x.shape[-1])

    def colsum(self, y):
        y = self(y)
        return y.reshape(-1, y.shape[-1]).sum(axis=0)


F64, F32, ABS = _Arith(np.float64), _Arith(np.float32), _Arith(np.float32, absolute=True)


def staged_reference(case, weights, a0, spect_pm, dout, kernel=None, rnd=bf16_round, dspect_prev=None, forward_only=False):
    """-> OrderedDict stage name -> Ref.  weights: name -> float32 array (chain_operands); a0 [B, n_in, L], dout [B, 2 n_in, L];
    spect_pm [B, L, 640] float64 as the kernels read it (bf16 values).  kernel: name -> float64 array [B, L, channels] of what the
    kernel STORED for h.i, ts.i, acts.i, skip, dskip, dpre.i, dh.i -- every stage starts from these; None: every stage starts from
    this function's own outputs, rounded with `rnd` (rnd = identity: the plain mathematics, which must equal stack_reference).
    rnd also rounds in_w, cond_w, rs_w, where k_pack_bf16 / k_pack_rows_bf16 round them."""
    c = case
    nl, B, L, n_in = c.n_layers, c.B, c.L, c.n_in
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    for k in list(w):
        if k.split(".")[0] in ("in_w", "cond_w", "rs_w"):
            w[k] = rnd(w[k])
    a0_pm, dout_pm = np.asarray(a0, np.float64).transpose(0, 2, 1), np.asarray(dout, np.float64).transpose(0, 2, 1)
    out = collections.OrderedDict()
    own = {}

    def src(name):
        return kernel[name] if kernel is not None else own[name]

    def put(name, f, K, kind="bf16", post=None):
        """f(arith) -> the linear form in that arithmetic; post(value, arith) -> the stage's output"""
        r, e, S = f(F64), f(F32), f(ABS)
        d = _bound(K, S)
        if post:
            r, e, d = post(r, e, d)
        out[name] = Ref(r, d, e, kind)
        own[name] = rnd(r) if kind == "bf16" else r
        return out[name]

    # ---- forward
    put("h.0", lambda A: A.mm(a0_pm, w["start_w"].T) + A(w["start_b"]), n_in)
    skip_terms = []
    for i in range(nl):
        last, d = i == nl - 1, 1 << i
        h, win, wc, wrs = src("h.%d" % i), w["in_w.%d" % i], w["cond_w.%d" % i], w["rs_w.%d" % i]

        def pre(A, h=h, win=win, wc=wc, i=i, d=d):
            v = A.mm(spect_pm, wc.T) + (A(w["in_b.%d" % i]) + A(w["cond_b.%d" % i]))
            for tap in range(3):
                v = v + A.mm(_shift(h, (tap - 1) * d), win[:, :, tap].T)
            return v
        p64, p32, Sp = pre(F64), pre(F32), pre(ABS)
        dp = _bound(K1, Sp)
        ts64, ts32 = gate_f64(p64), gate_f32(p32)
        dts = np.concatenate([dp[..., :CH] + MARGIN * GATE_ERR_T, dp[..., CH:] / 4 + MARGIN * GATE_ERR_S], axis=-1)
        out["pre.%d" % i] = Ref(p64, dp, p32, "none")
        out["ts.%d" % i] = Ref(ts64, dts, ts32, "bf16")
        T, S, dT, dS = ts64[..., :CH], ts64[..., CH:], dts[..., :CH], dts[..., CH:]
        out["acts.%d" % i] = Ref(T * S, dT * np.abs(S) + dS * np.abs(T) + dT * dS + 2 * U * np.abs(T * S), ts32[..., :CH] * ts32[..., CH:], "bf16")
        own["ts.%d" % i], own["acts.%d" % i] = rnd(ts64), rnd(T * S)
        acts = src("acts.%d" % i)
        if not last:
            put("h.%d" % (i + 1), lambda A, h=h, acts=acts, wrs=wrs, i=i: A(h) + (A.mm(acts, wrs[:CH].T) + A(w["rs_b.%d" % i][:CH])), CH + 1)
        rows = slice(0, CH) if last else slice(CH, 2 * CH)
        skip_terms.append((acts, wrs[rows], w["rs_b.%d" % i][rows]))

    def skip_f(A):
        v = 0
        for acts, wr, b in skip_terms:
            v = v + (A.mm(acts, wr.T) + A(b))
        return v
    put("skip", skip_f, (CH + 1) * nl, "f32")
    skip = src("skip")
    put("out", lambda A: A.mm(skip, w["end_w"].T) + A(w["end_b"]), CH, "f32")

    if forward_only:
        return out

    # ---- backward, data
    put("dskip", lambda A: A.mm(dout_pm, w["end_w"]), 2 * n_in)
    dskip = src("dskip")
    for i in range(nl - 1, -1, -1):
        last, d = i == nl - 1, 1 << i
        ts, wrs, win = src("ts.%d" % i), w["rs_w.%d" % i], w["in_w.%d" % i]
        up = dskip if last else np.concatenate([src("dh.%d" % (i + 1)), dskip], axis=-1)

        def gate_bwd(v, e, dv, ts=ts):
            T, S = ts[..., :CH], ts[..., CH:]
            ft, fs = S * (1 - T * T), T * S * (1 - S)
            # the factors are formed in fp32 from the stored T, S: 1 - T T and 1 - S carry an absolute error <= 2 U, each product
            # a relative one <= U
            dt = dv * np.abs(ft) + np.abs(v) * np.abs(S) * 2 * U + 4 * U * np.abs(v * ft)
            ds = dv * np.abs(fs) + np.abs(v) * np.abs(T * S) * 2 * U + 4 * U * np.abs(v * fs)
            T32, S32 = np.float32(T), np.float32(S)
            one = np.float32(1)
            e = np.concatenate([e * S32 * (one - T32 * T32), e * T32 * S32 * (one - S32)], axis=-1)
            return np.concatenate([v * ft, v * fs], axis=-1), e, np.concatenate([dt, ds], axis=-1)
        put("dpre.%d" % i, lambda A, up=up, wrs=wrs: A.mm(up, wrs), up.shape[-1], post=gate_bwd)
        dpre = src("dpre.%d" % i)

        def dh_f(A, dpre=dpre, win=win, last=last, i=i, d=d):
            v = 0 if last else A(src("dh.%d" % (i + 1)))
            g = 0
            for tap in range(3):
                g = g + A.mm(_shift(dpre, -(tap - 1) * d), win[:, :, tap])
            return v + g
        put("dh.%d" % i, dh_f, 3 * 2 * CH + 1)

    def dspect_f(A):
        v = 0 if dspect_prev is None else A(dspect_prev)
        g = 0
        for i in range(nl):
            g = g + A.mm(src("dpre.%d" % i), w["cond_w.%d" % i])
        return v + g
    put("dspect", dspect_f, nl * 2 * CH + 1, "f32")
    dh0 = src("dh.0")
    put("da0", lambda A: A.mm(dh0, w["start_w"]).transpose(0, 2, 1), CH, "f32")

    # ---- backward, weights: NT products over (b, n) and column sums
    R = B * L
    put("g.start_w", lambda A: A.nt(dh0, a0_pm), R, "f32")
    put("g.start_b", lambda A: A.colsum(dh0), R, "f32")
    for i in range(nl):
        last, d = i == nl - 1, 1 << i
        dpre, h, acts = src("dpre.%d" % i), src("h.%d" % i), src("acts.%d" % i)
        put("g.in_w.%d" % i, lambda A, dpre=dpre, h=h, d=d: np.stack([A.nt(dpre, _shift(h, (tap - 1) * d)) for tap in range(3)], axis=-1), R, "f32")
        put("g.in_b.%d" % i, lambda A, dpre=dpre: A.colsum(dpre), R, "f32")
        put("g.cond_w.%d" % i, lambda A, dpre=dpre: A.nt(dpre, spect_pm), R, "f32")
        out["g.cond_b.%d" % i] = out["g.in_b.%d" % i]
        up = dskip if last else np.concatenate([src("dh.%d" % (i + 1)), dskip], axis=-1)
        put("g.rs_w.%d" % i, lambda A, up=up, acts=acts: A.nt(up, acts), R, "f32")
        put("g.rs_b.%d" % i, lambda A, up=up: A.colsum(up), R, "f32")
    put("g.end_w", lambda A: A.nt(dout_pm, skip), R, "f32")
    put("g.end_b", lambda A: A.colsum(dout_pm), R, "f32")
    return out


# ----------------------------------------------------------------------------------------------------------- acceptance
def violations(got, ref):
    """-> boolean array: elements of the stored values `got` (float64; bf16 outputs as their exact values) outside the window."""
    if ref.kind == "bf16":
        return ~((got >= bf16_round(ref.r - ref.delta)) & (got <= bf16_round(ref.r + ref.delta)))
    return ~(np.abs(got - ref.r) <= ref.delta)


def err_over_delta(got, ref):
    """the worst |got - r| / delta, a reported figure; for a bf16 output half a bf16 ulp of r, the one admissible rounding, is
    taken off the distance first"""
    err = np.abs(got - ref.r)
    if ref.kind == "bf16":
        _, e = np.frexp(ref.r)
        err = np.maximum(err - np.ldexp(1.0, np.maximum(e, -125) - 9), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0, err / ref.delta, 0.0)
    q = np.where(np.isnan(got), np.inf, q)
    return float(q.max()) if q.size else 0.0


def mismatch_counts(got, ref):
    """-> (elements of `got` that are not bf16(r), elements of the CPU's float32 evaluation rounded to bf16 that are not)"""
    want = bf16_round(ref.r)
    return int((got != want).sum()), int((bf16_round(np.asarray(ref.emu, dtype=np.float64)) != want).sum())


MISMATCH_FLOOR = 8


def mismatch_allowance(cpu_count):
    """How many elements of a stage may differ from bf16(r): MARGIN times the count of the same stage evaluated in float32 on the
    CPU, plus a floor of MISMATCH_FLOOR elements.  An element differs when r lies closer to a rounding boundary than the stage's
    fp32 error, so the expected count is proportional to that error, of which the kernels get MARGIN times the CPU's; the floor
    is for the stages whose CPU count is zero or a handful, where the two counts are small-number statistics of their own."""
    return int(MARGIN * cpu_count) + MISMATCH_FLOOR


def describe(name, got, ref, bad, limit=4):
    """the first few offending elements: stage, (b, n, channel) or the weight's index, got, want, delta"""
    idx = np.argwhere(bad)[:limit]
    items = ["%s%s got %.9g want %.9g delta %.3g" % (name, tuple(int(v) for v in ix), got[tuple(ix)], ref.r[tuple(ix)], ref.delta[tuple(ix)])
             for ix in idx]
    return "%d of %d elements outside the window: %s" % (int(bad.sum()), bad.size, "; ".join(items))


# --------------------------------------------------------------------------------------------------------------- runner
def _lib():
    from facppg import lib
    return lib, lib.load()


def layout(case):
    lib, L = _lib()
    o = lib.WnBf16Offsets()
    rc = L.facppg_wn_bf16_layout(case.n_layers, case.B, case.L, o)
    assert rc == OK, (rc, wt.last_error())
    return o


@functools.lru_cache(maxsize=2)
def operands(case):
    """-> (weights, a0, spect bits uint16 [B, Lr, 640] with zero rows [L, Lr), dout, dspect_prev [B, L, 640] float32 or None)"""
    w, a0, spect, dout = wt.chain_operands(case.operands_key)
    Lr = _lib()[1].facppg_wn_bf16_padded_len(case.L)
    bits = np.zeros((case.B, Lr, NC), dtype=np.uint16)
    bits[:, :case.L] = bf16_bits(spect.transpose(0, 2, 1).astype(np.float64))
    prev = None
    if case.accumulate:
        prev = wt._rng(case.operands_key, "dspect_prev").standard_normal((case.B, case.L, NC), dtype=np.float32)
    return w, a0, wt._frozen(bits), dout, prev


DSPECT_PAD = float(np.float32(7.25))      # what rows [L, Lr) of dspect hold before the call (and must hold after it)


def _views(case, o, state, scratch):
    """the stage buffers inside state / scratch as int16 (bf16 bits) or float32 device views, full padded shapes"""
    import torch
    nl, B, Lr, Lp = case.n_layers, case.B, o.Lr, o.Lp

    def view(buf, off, shape, dt):
        nbytes = int(np.prod(shape)) * (2 if dt is torch.int16 else 4)
        return buf[off:off + nbytes].view(dt).view(shape)
    v = {"h": view(state, o.h, (nl + 1, B, Lp, CH), torch.int16), "ts": view(state, o.ts, (nl, B, Lr, 2 * CH), torch.int16),
         "acts": view(state, o.acts, (nl, B, Lr, CH), torch.int16), "skip": view(state, o.skip, (B, Lr, CH), torch.float32),
         "dpre": view(scratch, o.dpre, (nl, B, Lp, 2 * CH), torch.int16), "dh": view(scratch, o.dh, (nl + 1, B, Lr, CH), torch.int16),
         "dskip": view(scratch, o.dskip, (B, Lr, CH), torch.int16)}
    assert o.h_stride == B * Lp * CH * 2 and o.ts_stride == B * Lr * 2 * CH * 2 and o.acts_stride == B * Lr * CH * 2
    assert o.dpre_stride == B * Lp * 2 * CH * 2 and o.dh_stride == B * Lr * CH * 2
    return v


def _nonzero(t):
    return int(t.count_nonzero()) if hasattr(t, "count_nonzero") else int(np.count_nonzero(t))


def check_padding(v, nl, L):
    """v: the padded buffers h, dpre [.., B, Lp, ch], ts, acts, dh [.., B, Lr, ch], dskip [B, Lr, ch] as int16 bit patterns (device
    or host).  Every margin row and every row of [L, Lr) must be exactly zero -- of the spare images h[n_layers] and dh[n_layers]
    too, which the zeroing jobs cover; what their live rows hold is nobody's contract (no layer writes or reads them)."""
    zero = lambda t: not _nonzero(t)
    for name in ("h", "dpre"):                                  # [.., Lp, ..]: margins and rows [HALO + L, Lp)
        assert zero(v[name][:, :, :HALO]), name + ": the left margin is not exactly zero"
        assert zero(v[name][:, :, HALO + L:]), name + ": rows [128 + L, Lp) are not exactly zero"
    for name in ("ts", "acts", "dh"):
        assert zero(v[name][:, :, L:]), name + ": rows [L, Lr) are not exactly zero"
    assert zero(v["dskip"][:, L:]), "dskip: rows [L, Lr) are not exactly zero"


def _f64(t):
    """device view of bf16 bits (int16) or float32 -> float64 NumPy"""
    import torch
    if t.dtype is torch.int16:
        return bf16_to_f64(t.cpu().numpy().view(np.uint16))
    return t.cpu().numpy().astype(np.float64)


def run_stack(case, structure):
    """facppg_wn_forward_bf16 then facppg_wn_backward_bf16 on operands(case) under `structure`.  State and scratch start as 0xFF
    bytes, outputs and gradients as NaN, every buffer is followed by poison.  Asserted here: the return codes; every guard; exact
    zeros in every row of [L, Lr) and every margin row of h, ts, acts, dpre, dh, dskip; rows [L, Lr) of skip and dspect
    untouched (no kernel writes them: they keep what the caller left).  -> name -> float64 array of the live rows, named as staged_reference names them."""
    import torch
    lib, Lh = _lib()
    c = case
    nl, B, L, n_in = c.n_layers, c.B, c.L, c.n_in
    w, a0, spect_bits, dout, prev = operands(c)
    o = layout(c)
    Lr, Lp = o.Lr, o.Lp
    wdev = collections.OrderedDict((k, wt.dev_input(v)) for k, v in w.items())
    wst = wt._struct(lib.WnWeights, wdev)
    grads = wt._grad_buffers(c.operands_key)
    gst = wt._struct(lib.WnGrads, grads)
    a0_d, dout_d = wt.dev_input(a0), wt.dev_input(dout)
    sp = torch.full((spect_bits.size + GUARD,), 0x7FC0, dtype=torch.int16, device="cuda")       # bf16 NaN behind the operand
    sp[:spect_bits.size] = torch.from_numpy(spect_bits.view(np.int16).reshape(-1)).cuda()
    out_d, da0_d = wt.dev_output(B * 2 * n_in * L), wt.dev_output(B * n_in * L)
    dspect_d = wt.dev_output(B * Lr * NC)
    dsv = dspect_d[:B * Lr * NC].view(B, Lr, NC)
    dsv[:, L:] = DSPECT_PAD
    if prev is not None:
        dsv[:, :L] = torch.from_numpy(prev).cuda()
    state_bytes, scratch_bytes = Lh.facppg_wn_bf16_state_bytes(nl, B, L), Lh.facppg_wn_bf16_scratch_bytes(nl, B, L)
    assert state_bytes == o.state_end
    state, scratch = wt.dev_workspace(state_bytes), wt.dev_workspace(scratch_bytes)
    stream = lib.current_stream(a0_d.device)
    with pytest.MonkeyPatch.context() as mp:
        set_structure(mp, structure)
        rc = Lh.facppg_wn_forward_bf16(wst, n_in, nl, lib.ptr(a0_d), lib.ptr(sp), B, L, lib.ptr(out_d), lib.ptr(state), state_bytes,
                                       lib.ptr(scratch), scratch_bytes, stream)
        torch.cuda.synchronize()
        assert rc == OK, (rc, wt.last_error())
        assert wt.guard_intact(state, state_bytes) and wt.guard_intact(scratch, scratch_bytes), "the forward wrote behind state / scratch"
        # the backward gets a fresh scratch, as production hands it one (torch.empty): nothing of the forward's may be needed
        scratch.fill_(0xFF)
        scratch[scratch_bytes:] = 0xA5
        rc = Lh.facppg_wn_backward_bf16(wst, gst, n_in, nl, lib.ptr(a0_d), lib.ptr(sp), lib.ptr(dout_d), B, L, lib.ptr(state), state_bytes,
                                        lib.ptr(da0_d), lib.ptr(dspect_d), 1 if c.accumulate else 0, lib.ptr(scratch), scratch_bytes, stream)
        torch.cuda.synchronize()
        assert rc == OK, (rc, wt.last_error())
    assert wt.guard_intact(state, state_bytes) and wt.guard_intact(scratch, scratch_bytes), "the backward wrote behind state / scratch"
    for name, t, n in (("out", out_d, B * 2 * n_in * L), ("da0", da0_d, B * n_in * L), ("dspect", dspect_d, B * Lr * NC)):
        assert wt.guard_intact(t, n), "a kernel wrote behind " + name
    assert bool((sp[spect_bits.size:] == 0x7FC0).all())
    v = _views(c, o, state, scratch)
    check_padding(v, nl, L)
    assert bool((v["skip"][:, L:].contiguous().view(torch.int32) == -1).all()), "skip: rows [L, Lr) were written"
    assert bool((dsv[:, L:] == DSPECT_PAD).all()), "dspect: rows [L, Lr) were written"
    # facppg_posmajor_to_f32 carries the live rows alone into the channel-major gradient (ld = L + 3: the gaps stay as they were)
    ld = L + 3
    cm = wt.dev_output(B * NC * ld)
    rc = Lh.facppg_posmajor_to_f32(lib.ptr(dspect_d), B, NC, L, lib.ptr(cm), ld, stream)
    torch.cuda.synchronize()
    assert rc == OK and wt.guard_intact(cm, B * NC * ld)
    cmv = cm[:B * NC * ld].view(B, NC, ld)
    assert bool(torch.isnan(cmv[:, :, L:]).all()), "facppg_posmajor_to_f32 wrote columns >= L"
    assert torch.equal(cmv[:, :, :L], dsv[:, :L].transpose(1, 2)), "facppg_posmajor_to_f32 is not the transpose of the live rows"

    r = {"out": wt.host(out_d, (B, 2 * n_in, L)).astype(np.float64).transpose(0, 2, 1),
         "da0": wt.host(da0_d, (B, n_in, L)).astype(np.float64),
         "skip": _f64(v["skip"][:, :L]), "dskip": _f64(v["dskip"][:, :L]), "dspect": _f64(dsv[:, :L])}
    for i in range(nl):
        r["h.%d" % i] = _f64(v["h"][i, :, HALO:HALO + L])
        r["ts.%d" % i] = _f64(v["ts"][i, :, :L])
        r["acts.%d" % i] = _f64(v["acts"][i, :, :L])
        r["dpre.%d" % i] = _f64(v["dpre"][i, :, HALO:HALO + L])
        r["dh.%d" % i] = _f64(v["dh"][i, :, :L])
    for k, s in weight_shapes(n_in, nl).items():
        assert wt.guard_intact(grads[k], int(np.prod(s))), "a kernel wrote behind the gradient of " + k
        r["g." + k] = wt.host(grads[k], s).astype(np.float64)
    return r


KERNEL_STAGES = ("h", "ts", "acts", "dpre", "dh")


def kernel_operands(case, r):
    """what the stages read of a run's results: the stored h.i, ts.i, acts.i, skip, dskip, dpre.i, dh.i"""
    return {k: v for k, v in r.items() if k.split(".")[0] in KERNEL_STAGES + ("skip", "dskip")}


def operands_digest(k):
    h = hashlib.sha1()
    for name in sorted(k):
        h.update(name.encode())
        h.update(np.ascontiguousarray(k[name]).tobytes())
    return h.hexdigest()


_references = collections.OrderedDict()      # (case, digest of the kernel-stored operands) -> staged reference


def reference_for(case, r):
    """The staged reference on a run's stored operands, cached on their digest: the structures store the same bits (the fused and
    two-launch paths are bit-equal, test_gpu_train_bf16.py), so a case's four runs share one reference."""
    k = kernel_operands(case, r)
    key = (case, operands_digest(k))
    if key not in _references:
        w, a0, spect_bits, dout, prev = operands(case)
        spect_pm = bf16_to_f64(spect_bits[:, :case.L])
        _references[key] = staged_reference(case, w, a0, spect_pm, dout, kernel=k, dspect_prev=prev)
        while len(_references) > 2:
            _references.popitem(last=False)
    return _references[key]


FORWARD = ("h", "ts", "acts", "skip", "out")
BACKWARD = ("dskip", "dpre", "dh", "dspect", "da0")
WEIGHTS = ("g",)
Verdict = collections.namedtuple("Verdict", "stage failures worst mismatches cpu_mismatches elements")
_verdicts = {}


def judge(ref, r):
    """every element of every stage of the results `r` against the staged reference `ref`.  -> stage name -> Verdict"""
    res = collections.OrderedDict()
    for name, rf in ref.items():
        if rf.kind == "none":
            continue
        got = r[name]
        assert got.shape == rf.r.shape, (name, got.shape, rf.r.shape)
        bad = violations(got, rf)
        fail = describe(name, got, rf, bad) if bad.any() else None
        mm = mismatch_counts(got, rf) if rf.kind == "bf16" else (0, 0)
        res[name] = Verdict(name, fail, err_over_delta(got, rf), mm[0], mm[1], got.size)
    return res


def assert_accepted(res):
    failures = [v.failures for v in res.values() if v.failures]
    assert not failures, "\n".join(failures)
    for v in res.values():
        assert v.mismatches <= mismatch_allowance(v.cpu_mismatches), (
            "%s: %d of %d elements are not bf16(reference); the stage in float32 on the CPU has %d, which allows %d"
            % (v.stage, v.mismatches, v.elements, v.cpu_mismatches, mismatch_allowance(v.cpu_mismatches)))


def verdicts(case, structure):
    """Run (once per case and structure, whether it succeeds or not) and judge every stage.  -> stage name -> Verdict"""
    key = (case, structure)
    if key not in _verdicts:
        try:
            r = run_stack(case, structure)
            _verdicts[key] = judge(reference_for(case, r), r)
        except Exception as e:      # kept and raised again: what failed or faulted once is not launched again by the case's other tests
            _verdicts[key] = e
    if isinstance(_verdicts[key], Exception):
        raise _verdicts[key]
    return _verdicts[key]


def check(case, structure, groups):
    """assert the verdicts of the stages whose family (the name before the first dot) is in `groups`; prints what was measured"""
    res = {k: v for k, v in verdicts(case, structure).items() if k.split(".")[0] in groups}
    assert res
    worst = max(res.values(), key=lambda v: v.worst)
    mm = [v for v in res.values() if v.mismatches or v.cpu_mismatches]
    print("%s [%s] %s: worst err/delta %.3g (%s); bits != bf16(r): kernel %d, CPU fp32 %d of %d" % (
        case.id, structure, "/".join(groups), worst.worst, worst.stage, sum(v.mismatches for v in mm), sum(v.cpu_mismatches for v in mm),
        sum(v.elements for v in res.values() if v.stage.split(".")[0] in ("h", "ts", "acts", "dskip", "dpre", "dh"))))
    assert_accepted(res)
    return res
