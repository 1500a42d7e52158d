"""Direct tests of the TDNN acoustic-model kernels (csrc/facppg_tdnn.hip) through the public C ABI: hand-made
facppg_tdnn_layer tables and weight blobs (`Plan`), a float64 reference written from include/facppg.h's contract ON THE FRAME
AXIS, the case lists that test_tdnn_reference_cpu.py and test_gpu_tdnn_plans.py share, and a runner that fills workspace
and output with NaN and puts sentinel guard bands behind them.

Contract (include/facppg.h):  y_l[:, t] = act(W_l . [y_{l-1}[:, t + first_l + j * dil_l], j = 0..taps_l-1] + b_l), followed by
NormalizeComponent where renorm > 0 (y * (max(sum y^2 / (C rms^2), 2^-66))^-1/2); y_0[:, u] = feats[clamp(u, 0, T-1)]; the
output is final_op (copy | softmax | log-softmax) of the last layer's frames 0..T-1; every utterance of a batch on its own.
The reference evaluates layer l on exactly the frames [lo_l, hi_l] the last layer's frames 0..T-1 need, by gathering frames
-- it knows nothing of Tp, of shifted columns, of segments or of the zero fill the kernels rely on.

The running error bound (rounding class).  u = 2^-24.  e_0 = 0 (the features are float32), and per layer, elementwise,

    e_l = |W_l| e_{l-1} + g_l (|W_l| (|y_{l-1}| + e_{l-1}) + |b_l|),      g_l = (K_l + 2) * 2u  (+ u with rounded weights)

the first term carries the input's error through the exact product, the second is the textbook bound of a K_l-term fp32 sum in
any order, doubled for an unfused product's rounding, as in gemm_helpers.py, applied to the magnitudes the device may see
(|y| + e).  ReLU is 1-Lipschitz: the bound carries over.  Plans whose weights are float64 (the folded file path) hand the
device the weights rounded to float32: |dW| <= u |W|, one more u in g_l.

Renorm, y = x * s(x), s = r sqrt(C) / ||x||.  The device holds x^ = x + d with |d_c| <= e_c; write n = ||x||, eps = ||e||_2,
n^ = ||x^|| >= n - eps.  Then per channel

    |x^_c / n^ - x_c / n| <= |d_c| / n^ + |x_c| |1/n^ - 1/n| <= (e_c + |x_c| eps / n) / (n - eps),

the first-order perturbation of x / ||x|| with its denominator kept (no term is dropped: the inequality is exact).  The CPU
test checks eps <= 0.01 n on every frame a plan evaluates, so n - eps >= 0.99 n.  On top comes the kernel's own arithmetic,
relative to the result: C sequential fmaf of non-negative terms (C u on the sum), (float)C * rms * rms (2u) and the divide (u),
all halved by the square root; sqrtf and the reciprocal at 2u each (one ulp: neither is assumed correctly rounded), the final
multiply u:  RENORM_REL(C) = ((C + 3) / 2 + 5) u, first order, inflated by 1 / (1 - that) for the higher orders.  A frame whose
sum of squares is below the 2^-66 floor is scaled by 2^33; the cases reach the floor only with x = 0 exactly, where the result
is 0 whatever the scale."""
import contextlib
import ctypes
import dataclasses
import functools
import math
import zlib

import numpy as np

from gemm_helpers import SENTINEL, U, shape_env, ulp_distance  # noqa: F401  (re-exported to the test modules)

OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
GUARD = 256                 # floats of sentinel behind every output and workspace
NORM_FLOOR = 2.0 ** -66
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- plans
@dataclasses.dataclass(frozen=True)
class Layer:
    out_dim: int
    in_dim: int
    taps: int
    dil: int
    first: int
    relu: bool
    renorm: float           # target rms, 0 = no NormalizeComponent

    @property
    def K(self):
        return self.in_dim * self.taps

    @property
    def last(self):
        return self.first + (self.taps - 1) * self.dil


@dataclasses.dataclass(eq=False)
class Plan:
    """A layer table, final_op, and per layer W [out][taps * in] (tap-major) and b [out]: float32, or float64 where the device
    gets the rounded values (w_round)."""
    name: str
    layers: tuple
    final_op: int
    W: tuple
    b: tuple
    w_round: bool = False

    @property
    def in_dim(self):
        return self.layers[0].in_dim

    @property
    def out_dim(self):
        return self.layers[-1].out_dim

    @property
    def left(self):
        return sum(max(-l.first, 0) for l in self.layers)

    @property
    def right(self):
        return sum(max(l.last, 0) for l in self.layers)

    def with_final(self, final_op):
        return dataclasses.replace(self, final_op=final_op, name="%s-op%d" % (self.name, final_op))

    def table(self):
        from facppg import lib
        t = (lib.TdnnLayer * len(self.layers))()
        for i, l in enumerate(self.layers):
            t[i].out_dim, t[i].in_dim, t[i].taps, t[i].dil, t[i].first, t[i].relu = l.out_dim, l.in_dim, l.taps, l.dil, l.first, int(l.relu)
            t[i].renorm_target_rms = float(l.renorm)
        return t

    def blob(self):
        """include/facppg.h: per layer W [out_dim][taps * in_dim], then b [out_dim]"""
        return np.concatenate([a.reshape(-1).astype(F32) for Wb in zip(self.W, self.b) for a in Wb])

    @contextlib.contextmanager
    def handle(self):
        """facppg_tdnn_create ... facppg_tdnn_destroy on the current device"""
        h = create(self)
        try:
            yield h
        finally:
            from facppg import lib
            lib.load().facppg_tdnn_destroy(h)


def create(plan):
    import torch
    from facppg import lib
    L = lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    flat = torch.from_numpy(plan.blob()).to(dev)
    h = ctypes.c_void_p()
    rc = L.facppg_tdnn_create(plan.table(), len(plan.layers), plan.final_op, lib.ptr(flat), flat.numel(), dev.index,
                              lib.current_stream(dev), ctypes.byref(h))
    assert rc == OK, (plan.name, rc, L.facppg_last_error().decode())
    left, right = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.facppg_tdnn_context(h, ctypes.byref(left), ctypes.byref(right)) == OK
    assert (left.value, right.value) == (plan.left, plan.right), (plan.name, left.value, right.value)
    return h


def grid(offsets):
    """Append offsets -> (first, dil, taps, live taps): the uniform grid first + j * dil that holds them all"""
    offs = sorted(offsets)
    dil = int(np.gcd.reduce(np.diff(offs))) if len(offs) > 1 else 1
    return offs[0], dil, (offs[-1] - offs[0]) // dil + 1, [(o - offs[0]) // dil for o in offs]


def _int_weights(g, out_dim, in_dim, taps, live, nnz, wmax):
    """Small integers, about nnz non-zeros per row, none on a gap tap, every live column non-zero in at least one row: the
    rows' positions are cut from random permutations of the live columns laid end to end."""
    cols = np.concatenate([np.arange(in_dim) + t * in_dim for t in live])
    per = max(nnz, -(-cols.size // out_dim))
    need = out_dim * per
    pos = np.concatenate([g.permutation(cols) for _ in range(-(-need // cols.size))])[:need].reshape(out_dim, per)
    val = g.integers(1, wmax + 1, pos.shape) * g.choice([-1, 1], pos.shape)
    W = np.zeros((out_dim, taps * in_dim), F32)
    np.put_along_axis(W, pos, val.astype(F32), axis=1)
    return W


def make_plan(name, in_dim, specs, data="int", final_op=0, nnz=6, wmax=2, bmax=2, last_scale=1.0, bias_sign=0):
    """specs: per layer (out_dim, Append offsets, relu, renorm).  data 'int': the exact class; 'normal': N(0, 1 / K_live)
    weights and 0.1 N(0, 1) biases.  last_scale: a power of two on the last layer's W and b."""
    g = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))
    layers, Ws, bs = [], [], []
    cin = in_dim
    for i, (out_dim, offsets, relu, renorm) in enumerate(specs):
        first, dil, taps, live = grid(offsets)
        layers.append(Layer(out_dim, cin, taps, dil, first, bool(relu), float(renorm)))
        if data == "int":
            W = _int_weights(g, out_dim, cin, taps, live, nnz, wmax)
            b = g.integers(-bmax, bmax + 1, out_dim).astype(F32)
            if bias_sign:
                b = np.abs(b) * F32(bias_sign)
        else:
            W = np.zeros((out_dim, taps, cin), F32)
            W[:, live, :] = g.standard_normal((out_dim, len(live), cin), dtype=F32) / F32(math.sqrt(len(live) * cin))
            W = W.reshape(out_dim, -1)
            b = F32(0.1) * g.standard_normal(out_dim, dtype=F32)
        if i == len(specs) - 1:
            W, b = W * F32(last_scale), b * F32(last_scale)
        Ws.append(W)
        bs.append(b)
        cin = out_dim
    for a in Ws + bs:
        a.flags.writeable = False
    return Plan(name, tuple(layers), final_op, tuple(Ws), tuple(bs))


def hidden_chain(hidden, out_dim, splices, renorm=0.0):
    """splices -> specs: hidden ReLU layers per splice, then a 1-tap output layer"""
    return [(hidden, s, True, renorm) for s in splices] + [(out_dim, (0,), False, 0.0)]


DEFAULT_SPLICES = ((-2, -1, 0, 1, 2), (-1, 2), (-3, 3), (0,))


def _plan_specs():
    """name -> (in_dim, specs, keywords): the smallest plans at which the code can still go wrong"""
    seven = [(24, s, i % 2 == 0, 0.0) for i, s in enumerate(((-1, 0), (0, 1), (0,), (-2, 0), (0, 2), (-1, 1)))] + [(20, (0,), False, 0.0)]
    return {
        "a_default": (40, hidden_chain(64, 41, DEFAULT_SPLICES), {}),                              # L 6, R 7
        "b_left": (13, hidden_chain(50, 41, ((-1, 0), (-3, 0), (-6, -3, 0))), {}),                 # L 10, R 0
        "c_right": (13, hidden_chain(50, 41, ((0, 1), (0, 3))), {}),                               # L 0, R 4
        "d_point": (13, [(41, (0,), False, 0.0)], {}),                                             # L = R = 0, Tp = T
        "e_gaps": (8, hidden_chain(50, 41, ((-4, -1, 0, 2),)), {}),                                # 7 taps, 3 of them zero
        "f_dil9": (13, hidden_chain(50, 41, ((-7, 2),)), {}),                                      # dilation 9
        "g_k500": (100, hidden_chain(50, 41, ((-2, -1, 0, 1, 2),)), {}),                           # K = 500: split-K 2
        "h_k4096": (1024, hidden_chain(32, 41, ((-1, 0, 1, 2),)), dict(wmax=1)),                   # K = 4096: split-K 16
        "i_seven": (16, seven, dict(wmax=1)),                                                      # the chain ends in x[1]
        "i_two": (13, hidden_chain(50, 41, ((-1, 0, 1),)), {}),                                    # ... and in x[0]
    }


@functools.lru_cache(maxsize=None)
def exact_plan(name):
    in_dim, specs, kw = _plan_specs()[name]
    return make_plan(name, in_dim, specs, **kw)


@functools.lru_cache(maxsize=None)
def rounding_plan(name, renorm=0.0):
    """plans (a), (b), (e), (g) with standard-normal weights / sqrt(K); renorm > 0: relu-renorm hidden layers"""
    in_dim, specs, _ = _plan_specs()[name]
    specs = [(o, s, r, renorm if r else 0.0) for o, s, r, _ in specs]
    return make_plan("r%s%s" % (name, "-rn%g" % renorm if renorm else ""), in_dim, specs, data="normal")


@functools.lru_cache(maxsize=None)
def layer_plan(name, i):
    """Layer i of a rounding plan as a plan of its own, fed with features: the same GEMM (M, Cin, taps, dil) under the bound
    of ONE layer, g_l sum |w| |x|.  Down a chain the worst-case recursion multiplies the bound by ||W_l||_1 per layer (about
    0.8 sqrt(K)) where random rounding errors grow far slower, so by the last layer of plan (a) the chain's bound could no
    longer tell fp32 from a reduced-precision product; one layer's bound can, at every layer shape."""
    p = rounding_plan(name)
    return Plan("%s-L%d" % (p.name, i), (p.layers[i],), 0, (p.W[i],), (p.b[i],))


SOFTMAX_M = (8, 41, 256, 257, 600)
SOFTMAX_SCALE = 2.0 ** -2


@functools.lru_cache(maxsize=None)
def softmax_plan(M, final_op=1):
    """13 -> 24 (-1, 0, 1) ReLU -> M, integer operands, the last layer times a power of two: exactly known logits"""
    p = make_plan("s%d" % M, 13, hidden_chain(24, M, ((-1, 0, 1),)), last_scale=SOFTMAX_SCALE, nnz=4, wmax=1)
    return p.with_final(final_op)


@functools.lru_cache(maxsize=None)
def renorm_plan(C, rms):
    """one exact layer 13 -> C (ReLU, biases <= 0: a zero feature frame gives a zero column) followed by k_tdnn_renorm"""
    return make_plan("n%d-%g" % (C, rms), 13, [(C, (0,), True, rms)], bias_sign=-1)


def identity_plan(final_op):
    """two classes, W = I: the logits are the features"""
    return Plan("id2-op%d" % final_op, (Layer(2, 2, 1, 1, 0, False, 0.0),), final_op, (np.eye(2, dtype=F32),), (np.zeros(2, F32),))


# ----------------------------------------------------------------------------------------------------------------- data
SINGLE_T = (1, 2, 5, 37)
BATCHES = ((1, 5, 37, 150), (1, 5, 37, 150, 2))       # 252 columns with the default context; above the 256-column dispatch
POINT_BATCH = (1, 1, 2)                               # plan (d): three segments inside one 32-column tile


@functools.lru_cache(maxsize=None)
def features(in_dim, T, data="int", seed=0):
    g = np.random.Generator(np.random.PCG64([in_dim, T, seed, data == "int"]))
    x = g.integers(-3, 4, (T, in_dim)).astype(F32) if data == "int" else (2.0 * g.standard_normal((T, in_dim))).astype(F32)
    x.flags.writeable = False
    return x


def utterances(plan, lengths, data="int"):
    """utterance i of a batch has its own seed: equal lengths do not mean equal data"""
    return [features(plan.in_dim, T, data, seed=i) for i, T in enumerate(lengths)]


@dataclasses.dataclass(frozen=True)
class Case:
    plan: str
    lengths: tuple
    entry: str              # single | batch

    @property
    def id(self):
        return "%s-%s-%s" % (self.plan, self.entry, "_".join(map(str, self.lengths)))


def _exact_cases():
    out = []
    for name in _plan_specs():
        out += [Case(name, (T,), "single") for T in SINGLE_T]
        out += [Case(name, b, "batch") for b in BATCHES]
    out.append(Case("d_point", POINT_BATCH, "batch"))
    return out


EXACT_CASES = _exact_cases()
ROUNDING_PLANS = [("a_default", 0.0), ("b_left", 0.0), ("e_gaps", 0.0), ("g_k500", 0.0), ("e_gaps", 1.0), ("g_k500", 0.5)]
# (the renorm plans are the two-layer ones: down plans (a) and (b) the worst-case recursion, which a renorm layer doubles, leaves
# the ||e|| <= 0.01 ||x|| the renorm bound is derived under -- 3.5 and 0.016 at their last renorm layer)
ROUNDING_LAYERS = [(n, i) for n, rn in ROUNDING_PLANS if not rn for i in range(len(_plan_specs()[n][1]))]
ROUNDING_SHAPES = [((37,), "single"), (BATCHES[1], "batch")]
RENORM_CASES = [(C, rms) for C in (16, 50, 256) for rms in (1.0, 0.5)]
RENORM_T, RENORM_ZERO_FRAME = 37, 11
MONO_MD = (1, 40, 64)
FILE_MODEL = dict(splices=((-1, 0, 1), (-3, 0, 3), (-6, -3, 0)), lda=True, norm="batchnorm", hidden=50, output_dim=41)


def renorm_features(C, rms):
    x = np.array(features(13, RENORM_T))
    x[RENORM_ZERO_FRAME] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def transform(M, Md):
    """a non-negative [M][Md] transform (transposed reduce_ppg_dim matrix), a fifth of it zero"""
    g = np.random.Generator(np.random.PCG64([M, Md]))
    Rt = (g.random((M, Md)) * (g.random((M, Md)) > 0.2)).astype(F32)
    Rt.flags.writeable = False
    return Rt


# ------------------------------------------------------------------------------------------------------------ reference
@dataclasses.dataclass
class Ref:
    y: np.ndarray            # [T][out_dim] float64: the last layer, before final_op
    e: np.ndarray            # [T][out_dim]: the running error bound of y
    out: np.ndarray          # final_op applied, float64
    acts: list               # per layer: its activations on the frames it was evaluated on, [frames][C]
    renorm_ratio: float      # max over renorm layers and frames of ||e|| / ||x||
    sum_abs: float           # max over layers of sum |w| |x| + |b|: every partial sum, in any order, stays below it
    S: np.ndarray            # [T][out_dim]: sum |w| (|x| + e) + |b| of the last layer
    zero_frames: int         # frames of a renorm layer whose activations are all exactly zero (the 2^-66 floor)


def frame_ranges(plan, T):
    """[lo_l, hi_l] per layer output l = 0 (features) .. n: what the last layer's frames 0..T-1 need"""
    rng = [(0, T - 1)]
    for l in reversed(plan.layers):
        lo, hi = rng[0]
        rng.insert(0, (lo + l.first, hi + l.last))
    return rng


def final_f64(y, final_op):
    if final_op == 0:
        return y
    z = y - y.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1, keepdims=True))
    return np.exp(z - lse) if final_op == 1 else z - lse


def reference(plan, feats, exact_gemm=False):
    """One utterance, float64, on the frame axis (module docstring) -> Ref.  exact_gemm: the products are known to be exact
    (integer operands below 2^24, which the CPU test proves per plan): g_l = 0, the bound holds what comes after them."""
    feats = np.asarray(feats)
    assert feats.dtype == F32 and feats.shape[1] == plan.in_dim
    T = feats.shape[0]
    rng = frame_ranges(plan, T)
    lo, hi = rng[0]
    x = feats[np.clip(np.arange(lo, hi + 1), 0, T - 1)].astype(np.float64)      # y_0[u] = feats[clamp(u)]
    e = np.zeros_like(x)
    acts, ratio, sum_abs, zero_frames = [], 0.0, 0.0, 0
    for l, W, b, (lo1, hi1) in zip(plan.layers, plan.W, plan.b, rng[1:]):
        t = np.arange(lo1, hi1 + 1)
        idx = [t + l.first + j * l.dil - lo for j in range(l.taps)]
        assert min(i.min() for i in idx) == 0 and max(i.max() for i in idx) == x.shape[0] - 1
        xin = np.concatenate([x[i] for i in idx], axis=1)                        # [frames][taps * in]: Append order
        ein = np.concatenate([e[i] for i in idx], axis=1)
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        aW = np.abs(W64)
        gl = 0.0 if exact_gemm else (l.K + 2) * 2 * U + (U if plan.w_round else 0.0)
        S = (np.abs(xin) + ein) @ aW.T + np.abs(b64)
        sum_abs = max(sum_abs, float(S.max()))
        y = xin @ W64.T + b64
        e = ein @ aW.T + gl * S
        if l.relu:
            y = np.maximum(y, 0.0)
        if l.renorm > 0:
            C = l.out_dim
            n = np.sqrt((y * y).sum(axis=1, keepdims=True))
            eps = np.sqrt((e * e).sum(axis=1, keepdims=True))
            floor = n * n / (C * l.renorm ** 2) < NORM_FLOOR
            assert not (floor & (n > 0)).any(), "a non-zero frame below the 2^-66 floor: outside what the bound is derived for"
            zero_frames += int((n == 0).sum())
            ns = np.where(n > 0, n, 1.0)
            ratio = max(ratio, float((eps / ns).max()))
            k = l.renorm * math.sqrt(C)
            yn = y * (k / ns)
            g = ((C + 3) / 2 + 5) * U
            e = k * (e + np.abs(y) * eps / ns) / np.maximum(ns - eps, 1e-300) + g / (1 - g) * np.abs(yn)
            y, e = np.where(n > 0, yn, 0.0), np.where(n > 0, e, 0.0)
        acts.append(y)
        x, lo = y, lo1
    assert x.shape[0] == T
    return Ref(y=x, e=e, out=final_f64(x, plan.final_op), acts=acts, renorm_ratio=ratio, sum_abs=sum_abs, S=S, zero_frames=zero_frames)


def exact_bound(plan, xmax=3.0):
    """prod_l max_row ||W_l||_1 * max |x| + biases: the worst-case magnitude of any partial sum of the chain, in units of
    the plan's quantum"""
    q = min(float(np.abs(a[a != 0]).min()) for a in plan.W + plan.b if (a != 0).any())
    q = min(q, 1.0)
    bound = xmax
    for W, b in zip(plan.W, plan.b):
        bound = float(np.abs(W.astype(np.float64)).sum(axis=1).max()) * bound + float(np.abs(b).max())
    return bound / q


# the output kernels' bounds, given the allowances E1 (ulps of a posterior) and E2 (units of u max(1, |log-posterior|)) that
# test_gpu_tdnn_plans.py measures.  The logits are z (exact in class 3; spread = the largest |z - max z| of the frame, which
# matters only where z - max is itself rounded: the rounding class).
def softmax_rel_bound(M, E1, spread=0.0):
    """sum of M non-negative terms in any order: M u; the expf, add and divide of one element: E1 ulps = 2 E1 u; a rounded
    difference z - max moves the exponent by at most u spread, numerator and denominator: 2 u spread"""
    return (M + 2 * E1 + 2 * spread) * U


def logsoftmax_abs_bound(M, E1, E2, result, rounded=False):
    """log of the sum: its relative error (M + 2 E1) u as an absolute one; logf and the two subtractions: E2 u max(1, |result|);
    a rounded z - max: u |z - max| <= u |result|"""
    r = np.abs(result)
    return (M + 2 * E1) * U + E2 * U * np.maximum(1.0, r) + (U * r if rounded else 0.0)


def mono_rel_bound(M, E1):
    """softmax sum M u, the M-term fmaf chain of non-negative products M u, one element's expf / divide 2 E1 u"""
    return (2 * M + 2 * E1) * U


# --------------------------------------------------------------------------------------------------------------- runner
@dataclasses.dataclass
class Run:
    rc: int
    out: np.ndarray          # single / batch: [sum T][K]; padded / strided: [B][K][Tmax]
    guards: np.ndarray       # every sentinel element behind the output (strided: the guard rows of each utterance too)
    ws_guard: np.ndarray
    raw: np.ndarray          # the whole output buffer
    error: str

    def check(self):
        assert self.rc == OK, (self.rc, self.error)
        assert (self.guards == SENTINEL).all(), "%d guard elements behind the output were overwritten" % int((self.guards != SENTINEL).sum())
        assert (self.ws_guard == SENTINEL).all(), "the workspace was overrun"
        assert not np.isnan(self.out).any(), "%d elements of the output still hold the NaN pre-fill" % int(np.isnan(self.out).sum())
        return self.out


def launch(h, plan, entry, utts, shape=None, Rt=None, Tmax=None, guard_rows=0, ws_bytes=None, T=None):
    """One call of one entry point (single | batch | reduced | padded | strided) under one GEMM shape (None | 'legacy').
    Workspace and output hold NaN before the call, SENTINEL behind their declared sizes (and in the guard_rows rows behind each
    utterance's K rows of the strided call).  ws_bytes / T override what the call is told (the refusals)."""
    import torch
    from facppg import lib
    L = lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    frames = [int(u.shape[0]) for u in utts]
    B, G = len(frames), sum(frames)
    feats = torch.from_numpy(np.concatenate(utts, 0)).to(dev)
    off = lib.host_offsets(frames)
    off_dev = torch.tensor(list(off), dtype=torch.int32, device=dev)
    need = L.facppg_tdnn_workspace_bytes(h, frames[0]) if entry == "single" else L.facppg_tdnn_batch_workspace_bytes(h, off, B)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), float("nan"), device=dev)
    ws[need // 4:] = float(SENTINEL)
    K = plan.out_dim if Rt is None else Rt.shape[1]
    rt_dev = None if Rt is None else torch.from_numpy(np.array(Rt)).to(dev)
    if entry in ("padded", "strided"):
        Tmax = max(frames) if Tmax is None else Tmax
        stride = (K + guard_rows) * Tmax
        host = np.full((B, K + guard_rows, Tmax), np.nan, F32)
        host[:, K:, :] = SENTINEL
        n_out = B * stride
    else:
        n_out = G * K
        host = np.full(n_out, np.nan, F32)
    buf = torch.from_numpy(np.concatenate([host.reshape(-1), np.full(GUARD, SENTINEL, F32)])).to(dev)
    s = lib.current_stream(dev)
    wsb = need if ws_bytes is None else ws_bytes
    with shape_env(shape):
        if entry == "single":
            assert B == 1 and Rt is None
            rc = L.facppg_tdnn_forward(h, lib.ptr(feats), frames[0] if T is None else T, lib.ptr(buf), lib.ptr(ws), wsb, s)
        elif entry == "batch":
            rc = L.facppg_tdnn_forward_batch(h, lib.ptr(feats), lib.ptr(off_dev), off, B, lib.ptr(buf), lib.ptr(ws), wsb, s)
        elif entry == "reduced":
            rc = L.facppg_tdnn_forward_batch_reduced(h, lib.ptr(feats), lib.ptr(off_dev), off, B, lib.ptr(rt_dev), K, lib.ptr(buf), lib.ptr(ws), wsb, s)
        elif entry == "padded":
            assert guard_rows == 0
            rc = L.facppg_tdnn_forward_batch_padded(h, lib.ptr(feats), lib.ptr(off_dev), off, B, lib.ptr(rt_dev), K if Rt is not None else 0,
                                                    Tmax, lib.ptr(buf), lib.ptr(ws), wsb, s)
        elif entry == "strided":
            rc = L.facppg_tdnn_forward_batch_padded_strided(h, lib.ptr(feats), lib.ptr(off_dev), off, B, lib.ptr(rt_dev), K if Rt is not None else 0,
                                                            Tmax, stride, lib.ptr(buf), lib.ptr(ws), wsb, s)
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    err = L.facppg_last_error().decode() if rc != OK else ""
    ws_guard = ws[need // 4:].cpu().numpy()
    if entry in ("padded", "strided"):
        body = raw[:n_out].reshape(B, K + guard_rows, Tmax)
        out, guards = body[:, :K, :], np.concatenate([body[:, K:, :].reshape(-1), raw[n_out:]])
    else:
        out, guards = raw[:n_out].reshape(G, K), raw[n_out:]
    return Run(rc=rc, out=out, guards=guards, ws_guard=ws_guard, raw=raw, error=err)


def run_shapes(h, plan, entry, utts, **kw):
    """-> {'default': out, 'legacy': out}: every launch under both GEMM shapes, each checked (return code, guards, no NaN)"""
    return {name: launch(h, plan, entry, utts, shape=shape, **kw).check() for name, shape in (("default", None), ("legacy", "legacy"))}


def split_rows(out, lengths):
    """[sum T][K] -> the utterances' [T_b][K]"""
    at = np.concatenate([[0], np.cumsum(lengths)])
    return [out[at[i]:at[i + 1]] for i in range(len(lengths))]


# ---------------------------------------------------------------------------------------------------------- file path
def file_model():
    from common import nnet3
    kw = dict(FILE_MODEL)
    return nnet3.synthetic_tdnn(**kw)


def fold_file_model(net):
    """The synthetic_tdnn graph (lda -> [affine -> ReLU -> BatchNorm] x n -> affine -> softmax) folded in float64 as
    nnet3::CollapseModel would: test-mode BatchNorm y = (x - mean) s, s = rms / sqrt(var + eps), goes into the NEXT affine
    (W <- W diag(s) per tap, b <- b - W (mean s)), the fixed 'lda' affine on the spliced input is multiplied into tdnn1.
    Written from the graph, not from plan_layers -> Plan with float64 weights (w_round)."""
    c = net.components
    f64 = lambda a: np.asarray(a, np.float64)
    splices = FILE_MODEL["splices"]
    hidden, layers, Ws, bs = FILE_MODEL["hidden"], [], [], []
    scale = shift = None
    cin = net.input_dim()
    for i, offs in enumerate(splices):
        first, dil, taps, live = grid(offs)
        assert live == list(range(taps))
        A = c["tdnn%d.affine" % (i + 1)]
        W, b = f64(A.linear), f64(A.bias)
        if i == 0:                                   # tdnn1 reads lda, lda reads the splice: W (Wl x + bl) + b
            Wl, bl = f64(c["lda"].linear), f64(c["lda"].bias)
            W, b = W @ Wl, W @ bl + b
        else:                                        # the input is BatchNorm(prev): x s - mean s, per tap
            W3 = W.reshape(hidden, taps, cin)
            b = b + np.einsum("otc,c->o", W3, shift)
            W = (W3 * scale[None, None, :]).reshape(hidden, -1)
        layers.append(Layer(hidden, cin, taps, dil, first, True, 0.0))
        Ws.append(W)
        bs.append(b)
        bn = c["tdnn%d.batchnorm" % (i + 1)].fields
        scale = float(bn["TargetRms"]) / np.sqrt(f64(bn["StatsVar"]) + float(bn["Epsilon"]))
        shift = -f64(bn["StatsMean"]) * scale
        cin = hidden
    A = c["output.affine"]
    W, b = f64(A.linear), f64(A.bias)
    layers.append(Layer(W.shape[0], cin, 1, 1, 0, False, 0.0))
    Ws.append(W * scale[None, :])
    bs.append(b + W @ shift)
    return Plan("file", tuple(layers), 1, tuple(Ws), tuple(bs), w_round=True)
