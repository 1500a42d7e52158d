"""Direct tests of the tapped GEMM (csrc/facppg_gemm.h): a ctypes binding of the test-only probe library
(tests/native/gemm_probe.hip), a float64 NumPy reference written from the header's contract, the case lists that
test_gemm_reference_cpu.py and test_gpu_gemm.py share, and a runner that surrounds every operand with poison.

Contract (facppg_gemm.h):  C[b][m][n] = epilogue(sum_{tap, c} W[m][c][tap] * X[b][c][n + (tap - pad) * dil]) for
n in [col0, Nb), m in [0, M); Nb = min(N, n_valid[b] * mul + add) (N without n_valid); a source column outside [0, Ns)
reads as zero, Ns = src_hi > 0 ? min(src_hi, n_valid[b] * mul + add) : Nb; epilogue = bias, scale / shift, activation,
keep-mask * 2, residual, then the store (plain, transposed, or the gate backward's two row ranges)."""
import ctypes as c
import dataclasses
import functools
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "tests", "native", "libfacppg_gemm_probe.so")

OK, EINVAL, EWORKSPACE = 0, -1, -4
ACT_NONE, ACT_RELU, ACT_TANH, ACT_LOG_CLAMP = 0, 1, 2, 3
LOG_FLOOR = float(np.float32(1e-5))   # the kernel's clamp is the float32 constant
U = 2.0 ** -24                        # unit roundoff of float32
SENTINEL = np.float32(-1.2345e30)
LAT_MAX_N = 256                       # launches of at most this many columns take the latency shape


class Args(c.Structure):
    """probe_gemm_args of gemm_probe.hip: every field of GemmArgs, in its order."""
    _fields_ = [("A", c.c_void_p), ("M", c.c_int), ("Cin", c.c_int), ("taps", c.c_int), ("dil", c.c_int), ("pad", c.c_int),
                ("X", c.c_void_p), ("x_bs", c.c_long), ("ldx", c.c_int), ("N", c.c_int), ("col0", c.c_int), ("src_hi", c.c_int),
                ("skip", c.c_void_p), ("n_valid", c.c_void_p), ("n_valid_mul", c.c_int), ("n_valid_add", c.c_int),
                ("bias", c.c_void_p), ("scale", c.c_void_p), ("shift", c.c_void_p), ("act", c.c_int),
                ("mask", c.c_void_p), ("mask_bs", c.c_long), ("ldmask", c.c_int),
                ("res", c.c_void_p), ("res_bs", c.c_long), ("ldres", c.c_int),
                ("C", c.c_void_p), ("c_bs", c.c_long), ("ldc", c.c_int), ("c_transposed", c.c_int),
                ("gate_ts", c.c_void_p), ("gate_bs", c.c_long), ("ldgate", c.c_int), ("B", c.c_int),
                ("splitk_ws", c.c_void_p), ("splitk_ws_bytes", c.c_size_t)]


@functools.lru_cache(maxsize=None)
def probe():
    """-> (probe library, product library).  A missing probe is an error, never a skip."""
    from facppg import lib
    L = lib.load()   # first: the probe resolves facppg:: against the library the package itself uses
    if not os.path.isfile(PROBE_PATH):
        raise RuntimeError("%s is missing: run build() of __graft_entry__.py (or `make -C fac-via-ppg_amd/csrc`), "
                           "which builds the GEMM probe next to the product library" % PROBE_PATH)
    P = c.CDLL(PROBE_PATH)
    P.probe_args_size.restype = c.c_size_t
    P.probe_args_size.argtypes = []
    P.probe_packed_a_bytes.restype = c.c_size_t
    P.probe_packed_a_bytes.argtypes = [c.c_int, c.c_int]
    P.probe_pack_a.restype = c.c_int
    P.probe_pack_a.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    P.probe_pack_a_strided.restype = c.c_int
    P.probe_pack_a_strided.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, c.c_long, c.c_long, c.c_void_p,
                                       c.c_void_p]
    P.probe_gemm.restype = c.c_int
    P.probe_gemm.argtypes = [c.POINTER(Args), c.c_void_p]
    return P, L


def last_error():
    return probe()[1].facppg_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    M: int = 33
    Cin: int = 64
    taps: int = 1
    dil: int = 1
    pad: int = 0
    N: int = 65
    B: int = 1
    col0: int = 0
    src_hi: int = 0
    n_valid: tuple = None     # per batch entry
    mul: int = 1
    add: int = 0
    skip: int = None          # None: no flag; 0 / 1: the flag's value
    bias: bool = False
    affine: bool = False      # scale and shift
    act: int = ACT_NONE
    mask: bool = False
    res: bool = False
    ct: bool = False          # c_transposed
    gate: bool = False
    split: bool = False       # lend a split-K buffer
    x_shared: bool = False    # x_bs = 0
    wview: str = "plain"      # how the weights lie in memory for pack_a_strided: plain | transposed | reversed | wn_bwd
    data: str = "int"         # int: the exact class; normal: standard normal float32
    tag: str = ""

    @property
    def K(self):
        return self.Cin * self.taps

    @property
    def id(self):
        d = Case()
        parts = []
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if v != getattr(d, f.name):
                if isinstance(v, bool):
                    parts.append(f.name)
                elif isinstance(v, tuple):
                    parts.append(f.name + "_".join(map(str, v)))
                elif f.name == "tag":
                    parts.append(v)
                else:
                    parts.append("%s%s" % (f.name, v))
        return "-".join(parts) or "default"

    def both_shapes(self):
        return self.N - self.col0 <= LAT_MAX_N

    def bounds(self, b):
        """-> (Nb, Ns) of batch entry b."""
        nv = None if self.n_valid is None else self.n_valid[b] * self.mul + self.add
        Nb = self.N if nv is None else min(self.N, nv)
        Ns = (self.src_hi if nv is None else min(self.src_hi, nv)) if self.src_hi > 0 else Nb
        return Nb, Ns

    def x_cols(self):
        """columns the logical X carries: every column some batch entry may legally read"""
        return max(self.N, self.src_hi)


EPI = dict(bias=True, affine=True, act=ACT_RELU, mask=True, res=True)


def _pad(taps, dil, N, which):
    return {0: 0, 1: (taps - 1) // 2}.get(which, N // dil + 1)


def _grid_cases():
    """row-block and column-tile edges: every M with every N, whole epilogue"""
    return [Case(M=M, N=N, Cin=5, taps=5, pad=2, **EPI)
            for M in (1, 31, 32, 33, 127, 128, 129) for N in (1, 31, 32, 33, 63, 64, 65, 256, 257, 300)]


# (K, [(Cin, taps), ...]): one entry per Cin regime the factorisation of K allows -- Cin < 8 (several tap wraps inside one
# thread's 8 k), 64 % Cin != 0 (the r64 carry), Cin >= 64.  K = 40 has no Cin >= 64; every Cin with Cin * taps = 64 or 512
# divides 64 or is >= 64; every divisor of 8128 = 2^6 * 127 below 64 divides 64 (127 stands in).
K_PATHS = [(40, [(1, 40), (5, 8), (40, 1)]),
           (64, [(4, 16), (64, 1)]),
           (65, [(5, 13), (13, 5), (65, 1)]),
           (448, [(1, 448), (7, 64), (56, 8), (64, 7), (448, 1)]),
           (512, [(4, 128), (128, 4), (512, 1)]),
           (832, [(4, 208), (13, 64), (64, 13), (832, 1)]),
           (2560, [(5, 512), (40, 64), (512, 5)]),
           (8128, [(4, 2032), (127, 64), (8128, 1)])]


def _k_cases(data="int", N=65, col0=0):
    out = []
    for K, facts in K_PATHS:
        for i, (Cin, taps) in enumerate(facts):
            for split in (False, True):
                # long tap rows at few columns leave most chunks all zero: move the live taps to the front (pad 0), the
                # middle and the back (causal, pad = taps - 1) so that the first and the last chunk carry data somewhere
                pad = (0, (taps - 1) // 2, taps - 1)[(i + split) % 3] if taps > 5 else (taps - 1) // 2
                out.append(Case(Cin=Cin, taps=taps, pad=pad, N=N, col0=col0, split=split, data=data, bias=data == "int",
                                res=data == "int"))
    return out


def _cin_cases():
    out = []
    i = 0
    for Cin in (3, 5, 64, 80, 600):
        for taps in (1, 3, 5):
            for dil in (1, 2, 128):
                which = i % 3
                i += 1
                # dil = 128 reaches other columns only in a long row: N = 300 (window from 60: both shapes)
                N, col0 = (300, 60) if dil == 128 else (65, 0)
                out.append(Case(Cin=Cin, taps=taps, dil=dil, pad=_pad(taps, dil, N, which), N=N, col0=col0, split=Cin == 600,
                                bias=True, act=ACT_RELU if i % 2 else ACT_NONE))
    # each pad option with each dil at taps = 5 (the rotation above gives each (Cin, taps) only one pad per dil)
    for dil in (1, 2, 128):
        for which in (0, 1, 2):
            N, col0 = (300, 60) if dil == 128 else (65, 0)
            out.append(Case(Cin=80, taps=5, dil=dil, pad=_pad(5, dil, N, which), N=N, col0=col0, tag="padgrid"))
    return out


def _window_cases():
    """K = 640: split in two with a buffer, ten chunks (one refill round) without"""
    out = []
    for N, col0 in ((65, 1), (65, 31), (65, 32), (65, 45), (300, 60), (300, 10)):
        for src_hi in (0, N - 3, N, N + 7):
            for nv in (None, (N - 5,), (N + 4,)):
                for split in (False, True):
                    out.append(Case(Cin=128, taps=5, pad=2, N=N, col0=col0, src_hi=src_hi, n_valid=nv, split=split, bias=True))
    for skip in (0, 1):
        for split in (False, True):
            for N, col0 in ((65, 0), (300, 10)):
                out.append(Case(Cin=128, taps=5, pad=2, N=N, col0=col0, skip=skip, split=split, res=True))
    return out


def _batch_cases():
    out = []
    N = 65
    for split in (False, True):
        for src_hi in (0, N + 7):
            kw = dict(Cin=128, taps=5, pad=2, N=N, B=3, split=split, src_hi=src_hi, mask=True, res=True)
            out.append(Case(n_valid=(N, 0, 17), **kw))
            out.append(Case(n_valid=(33, 0, 9), mul=2, add=-1, **kw))            # 65, -1, 17
            out.append(Case(n_valid=(40, 2, 36), mul=2, add=-1, **kw))           # 79 (clips), 3, 71 (clips)
            out.append(Case(n_valid=(N, 0, 17), x_shared=True, **kw))
            out.append(Case(x_shared=True, **kw))
    return out


def _store_cases():
    out = []
    for M in (33, 129):
        for split in (False, True):
            out.append(Case(M=M, Cin=128, taps=5, pad=2, ct=True, split=split, bias=True, res=True))
            out.append(Case(M=M, Cin=128, taps=5, pad=2, ct=True, split=split, col0=31, n_valid=(60,)))
            out.append(Case(M=M, Cin=128, taps=5, pad=2, gate=True, split=split))
            out.append(Case(M=M, Cin=128, taps=3, dil=128, pad=1, N=300, col0=60, gate=True, split=split))
    return out


def _pack_cases():
    out = []
    for view in ("transposed", "reversed", "wn_bwd"):
        out.append(Case(M=33, Cin=10, taps=3, pad=1, wview=view))
        out.append(Case(M=5, Cin=80, taps=3, pad=1, dil=2, wview=view, bias=True))
        out.append(Case(M=129, Cin=200, taps=3, pad=1, wview=view, split=True))
    out.append(Case(M=33, Cin=10, taps=3, pad=1, tag="packplain"))
    return out


GRID_CASES = _grid_cases()
EXACT_K_CASES = _k_cases()
CIN_CASES = _cin_cases()
WINDOW_CASES = _window_cases()
BATCH_CASES = _batch_cases()
STORE_CASES = _store_cases()
PACK_CASES = _pack_cases()
EXACT_CASES = GRID_CASES + EXACT_K_CASES + CIN_CASES + WINDOW_CASES + BATCH_CASES + STORE_CASES + PACK_CASES
# rounding class: the K paths at M = 33, N = 65 and again at N = 300 (the long row once per kernel: window from 60 for the
# latency shape, from 0 for the 64-column kernel)
ROUNDING_CASES = (_k_cases("normal") + _k_cases("normal", N=300, col0=60) + _k_cases("normal", N=300)
                  + [Case(Cin=512, taps=5, pad=2, split=s, data="normal", bias=True, affine=True, mask=True, res=True, tag="epi")
                     for s in (False, True)])


# ----------------------------------------------------------------------------------------------------------------- data
@dataclasses.dataclass
class Data:
    W: np.ndarray            # [M][Cin][taps]
    X: np.ndarray            # [B or 1][Cin][x_cols]
    bias: np.ndarray = None
    scale: np.ndarray = None
    shift: np.ndarray = None
    mask: np.ndarray = None  # [B][M][N] uint8
    res: np.ndarray = None   # [B][M][N]
    gate: np.ndarray = None  # [B][2M][N]: T rows, then S rows


def _freeze(d):
    for f in dataclasses.fields(d):
        v = getattr(d, f.name)
        if v is not None:
            v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def make_data(cs):
    g = np.random.Generator(np.random.PCG64(zlib.crc32(cs.id.encode())))
    Bx = 1 if cs.x_shared else cs.B
    shp_w, shp_x, shp_c = (cs.M, cs.Cin, cs.taps), (Bx, cs.Cin, cs.x_cols()), (cs.B, cs.M, cs.N)
    f32 = np.float32
    if cs.data == "int":
        ints = lambda lo, hi, shp: g.integers(lo, hi + 1, shp).astype(f32)
        d = Data(W=ints(-2, 2, shp_w), X=ints(-3, 3, shp_x))
        if cs.bias:
            d.bias = ints(-4, 4, (cs.M,))
        if cs.affine:
            d.scale = (2.0 ** g.integers(-2, 3, (cs.M,))).astype(f32)
            d.shift = ints(-4, 4, (cs.M,))
        if cs.res:
            d.res = ints(-5, 5, shp_c)
        if cs.gate:   # dyadic T in (-1, 1) and S in (0, 1): every product of the gate backward stays exact
            d.gate = np.concatenate([ints(-3, 3, shp_c) / f32(4), ints(1, 3, shp_c) / f32(4)], axis=1)
    else:
        nrm = lambda shp: g.standard_normal(shp, dtype=f32)
        d = Data(W=nrm(shp_w), X=nrm(shp_x))
        if cs.bias:
            d.bias = nrm((cs.M,))
        if cs.affine:
            d.scale, d.shift = nrm((cs.M,)), nrm((cs.M,))
        if cs.res:
            d.res = nrm(shp_c)
        assert not cs.gate
    if cs.mask:
        d.mask = (g.random(shp_c) < 0.5).astype(np.uint8)
    return _freeze(d)


# ------------------------------------------------------------------------------------------------------------ reference
@dataclasses.dataclass
class Ref:
    win: np.ndarray      # [B][M][N] bool: the elements the launch writes
    pre: np.ndarray      # [B][M][N] float64: the sum
    S: np.ndarray        # sum |w| |x|
    v: np.ndarray        # after the epilogue, before the store ([B][M][N]); with gate: [B][2M][N]
    tol: np.ndarray      # rounding-class tolerance of v (same shape as v; not defined for gate)
    S_out: np.ndarray    # S carried through the epilogue's multiplications (what err / (u S) is measured against)
    v_act: np.ndarray    # the activation's argument, tol_act its tolerance (tanh / log-clamp cases)
    tol_act: np.ndarray
    f32_exact: bool      # every intermediate of the epilogue is a float32 number (exact class)


def conv_sum(cs, W, X):
    """-> (sum, sum of magnitudes), float64 [B][M][N], by the header's formula."""
    W64 = W.astype(np.float64)
    aW = np.abs(W64)
    pre = np.zeros((cs.B, cs.M, cs.N))
    S = np.zeros_like(pre)
    n = np.arange(cs.N)
    for b in range(cs.B):
        Nb, Ns = cs.bounds(b)
        Xb = X[0 if cs.x_shared else b].astype(np.float64)
        for tap in range(cs.taps):
            src = n + (tap - cs.pad) * cs.dil
            ok = (src >= 0) & (src < Ns)
            if not ok.any():
                continue
            Xs = np.zeros((cs.Cin, cs.N))
            Xs[:, ok] = Xb[:, src[ok]]
            pre[b] += W64[:, :, tap] @ Xs
            S[b] += aW[:, :, tap] @ np.abs(Xs)
    return pre, S


def _is_f32(v):
    return bool(np.array_equal(v.astype(np.float32).astype(np.float64), v))


def _reference(cs, d):
    pre, S = conv_sum(cs, d.W, d.X)
    win = np.zeros((cs.B, cs.M, cs.N), bool)
    for b in range(cs.B):
        Nb, _ = cs.bounds(b)
        if not cs.skip and Nb > cs.col0:
            win[b, :, cs.col0:Nb] = True
    col = lambda a: a.astype(np.float64)[None, :, None]
    v, S_out = pre.copy(), S.copy()
    tol = (cs.K + 2) * 2 * U * S   # first-order summation bound K u S, doubled for an unfused product's rounding
    exact = _is_f32(v)
    if cs.bias:
        v = v + col(d.bias)
        tol = tol + U * np.abs(v)
        exact &= _is_f32(v)
    if cs.affine:
        v = v * col(d.scale) + col(d.shift)
        tol = tol * np.abs(col(d.scale)) + U * np.abs(v)
        S_out = S_out * np.abs(col(d.scale))
        exact &= _is_f32(v)
    v_act, tol_act = v, tol
    if cs.act == ACT_RELU:
        v = np.maximum(v, 0.0)   # 1-Lipschitz: the tolerance carries over
    elif cs.act == ACT_TANH:
        v = np.tanh(v)
    elif cs.act == ACT_LOG_CLAMP:
        v = np.log(np.maximum(v, LOG_FLOOR))
    if cs.mask:
        k = 2.0 * d.mask.astype(np.float64)
        v, tol, S_out = v * k, tol * k, S_out * k
    if cs.res:
        v = v + d.res.astype(np.float64)
        tol = tol + U * np.abs(v)
        exact &= _is_f32(v)
    if cs.gate:
        T, Sg = d.gate[:, :cs.M].astype(np.float64), d.gate[:, cs.M:].astype(np.float64)
        v = np.concatenate([v * Sg * (1.0 - T * T), v * T * Sg * (1.0 - Sg)], axis=1)
        exact &= _is_f32(v)
        tol = None
    return Ref(win=win, pre=pre, S=S, v=v, tol=tol, S_out=S_out, v_act=v_act, tol_act=tol_act, f32_exact=bool(exact))


@functools.lru_cache(maxsize=None)
def reference(cs):
    """float64 reference of a case on its own data; computed once, shared, read-only"""
    r = _reference(cs, make_data(cs))
    for f in dataclasses.fields(r):
        a = getattr(r, f.name)
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return r


# --------------------------------------------------------------------------------------------------------- weight views
def weight_view(cs, W):
    """-> (flat float32 storage, sm, sc, st, off): element (m, c, tap) of W at storage[off + m*sm + c*sc + tap*st]"""
    M, Cin, taps = W.shape
    if cs.wview == "plain":
        return W.reshape(-1).copy(), Cin * taps, taps, 1, 0
    if cs.wview == "transposed":      # stored [Cin][M][taps]
        return W.transpose(1, 0, 2).reshape(-1).copy(), taps, M * taps, 1, 0
    if cs.wview == "reversed":        # stored [M][Cin][taps] with the taps back to front
        return W[:, :, ::-1].reshape(-1).copy(), Cin * taps, taps, -1, taps - 1
    if cs.wview == "wn_bwd":          # the WN backward's: stored [Cin][M][taps] (a forward weight [cout][cin][k]), taps reversed
        return W[:, :, ::-1].transpose(1, 0, 2).reshape(-1).copy(), taps, M * taps, -1, taps - 1
    raise ValueError(cs.wview)


def packed_image(W):
    """The A-operand image by facppg_gemm.h's index formula -> float32 [MB * (KG + 1) * 64][4] (without the unspecified tail)."""
    M, Cin, taps = W.shape
    K = Cin * taps
    KG = (K + 63) // 64 * 8
    MB = (M + 31) // 32
    idx = np.arange(MB * (KG + 1) * 64)
    lane, g, mb = idx & 63, (idx >> 6) % (KG + 1), (idx >> 6) // (KG + 1)
    m = mb * 32 + (lane & 31)
    out = np.zeros((idx.size, 4), np.float32)
    for s in range(4):
        k = 8 * g + 4 * (lane >> 5) + s
        ok = (m < M) & (k < K) & (g < KG)
        tap, ch = k[ok] // Cin, k[ok] % Cin
        out[ok, s] = W[m[ok], ch, tap]
    return out


# --------------------------------------------------------------------------------------------------------------- runner
class shape_env:
    """FACPPG_GEMM_SHAPE for the calls inside (gemm_launch reads it per call)"""

    def __init__(self, shape):
        self.shape = shape

    def __enter__(self):
        self.old = os.environ.get("FACPPG_GEMM_SHAPE")
        if self.shape == "legacy":
            os.environ["FACPPG_GEMM_SHAPE"] = "legacy"
        else:
            os.environ.pop("FACPPG_GEMM_SHAPE", None)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("FACPPG_GEMM_SHAPE", None)
        else:
            os.environ["FACPPG_GEMM_SHAPE"] = self.old


@dataclasses.dataclass
class Run:
    out: np.ndarray      # [B][rows][N] float32, rows = 2M with gate: SENTINEL wherever the launch may not write
    raw: np.ndarray      # the whole C buffer
    packed: np.ndarray   # the whole packed-weight buffer, float32
    packed_floats: int   # probe_packed_a_bytes / 4


def _poisoned(shape_bld, valid, value, dtype, poison):
    """array [B][rows][ld] holding value[b] in [:, :N] where valid, poison elsewhere"""
    B, rows, ld = shape_bld
    a = np.full(shape_bld, poison, dtype)
    N = value.shape[2]
    a[:, :, :N] = np.where(valid, value, np.array(poison, dtype))
    return a


def run_case(cs, d=None, shape=None):
    """One pack_a + gemm_launch on the GPU with every buffer larger than needed: leading dimensions above N, NaN in the packed
    buffer before pack_a, in X outside each batch entry's valid source (a shared X, x_bs = 0, can only be poisoned behind the
    LONGEST entry's source: a shorter entry that read past its own would see live data, which the exact comparison with
    the reference -- zero there -- still catches) and in res / gate_ts outside the output window (255 in the byte mask there), NaN in the split-K buffer, SENTINEL in C.  Checks on the way out: return codes, C outside the window
    still SENTINEL, C inside finite, the packed buffer untouched behind its declared size."""
    import torch
    P, _ = probe()
    d = d or make_data(cs)
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    keep = []

    def up(a):
        t = torch.from_numpy(np.array(a)).to(dev)   # (a copy: the shared data is read-only)
        keep.append(t)
        return t

    M, Cin, taps, N, B = cs.M, cs.Cin, cs.taps, cs.N, cs.B
    ref_win = np.zeros((B, M, N), bool)
    for b in range(B):
        Nb, _ = cs.bounds(b)
        if not cs.skip and Nb > cs.col0:
            ref_win[b, :, cs.col0:Nb] = True

    a = Args()
    # weights
    pbytes = P.probe_packed_a_bytes(M, cs.K)
    assert pbytes % 16 == 0
    slack = 64
    tA = up(np.full(pbytes // 4 + slack, np.nan, np.float32))
    store, sm, sc, st, off = weight_view(cs, d.W)
    tW = up(store)
    if cs.wview == "plain":
        rc = P.probe_pack_a(tW.data_ptr(), M, Cin, taps, tA.data_ptr(), stream)
    else:
        rc = P.probe_pack_a_strided(tW.data_ptr(), M, Cin, taps, sm, sc, st, off, tA.data_ptr(), stream)
    assert rc == OK, last_error()
    a.A, a.M, a.Cin, a.taps, a.dil, a.pad = tA.data_ptr(), M, Cin, taps, cs.dil, cs.pad
    # activations: NaN outside [0, Ns) of each batch entry (of the longest entry for a shared X)
    Bx = 1 if cs.x_shared else B
    ldx = cs.x_cols() + 5
    xs = np.full((Bx, Cin, ldx), np.nan, np.float32)
    for b in range(Bx):
        Ns = max(cs.bounds(bb)[1] for bb in range(B)) if cs.x_shared else cs.bounds(b)[1]
        Ns = max(0, min(Ns, cs.x_cols()))
        xs[b, :, :Ns] = d.X[b, :, :Ns]
    x_bs = Cin * ldx + 11
    xflat = np.full(Bx * x_bs, np.nan, np.float32)
    for b in range(Bx):
        xflat[b * x_bs:b * x_bs + Cin * ldx] = xs[b].reshape(-1)
    tX = up(xflat)
    a.X, a.x_bs, a.ldx, a.N, a.col0, a.src_hi = tX.data_ptr(), 0 if cs.x_shared else x_bs, ldx, N, cs.col0, cs.src_hi
    if cs.skip is not None:
        a.skip = up(np.array([cs.skip], np.int32)).data_ptr()
    if cs.n_valid is not None:
        a.n_valid = up(np.array(cs.n_valid, np.int32)).data_ptr()
    a.n_valid_mul, a.n_valid_add = cs.mul, cs.add
    if cs.bias:
        a.bias = up(d.bias).data_ptr()
    if cs.affine:
        a.scale, a.shift = up(d.scale).data_ptr(), up(d.shift).data_ptr()
    a.act = cs.act
    if cs.mask:
        a.ldmask = N + 2
        a.mask_bs = M * a.ldmask
        a.mask = up(_poisoned((B, M, a.ldmask), ref_win, d.mask, np.uint8, 255)).data_ptr()
    if cs.res:
        a.ldres = N + 4
        a.res_bs = M * a.ldres
        a.res = up(_poisoned((B, M, a.ldres), ref_win, d.res, np.float32, np.nan)).data_ptr()
    rows = 2 * M if cs.gate else M
    if cs.gate:
        a.ldgate = N + 1
        a.gate_bs = 2 * M * a.ldgate
        a.gate_ts = up(_poisoned((B, 2 * M, a.ldgate), np.concatenate([ref_win, ref_win], 1), d.gate, np.float32, np.nan)).data_ptr()
    # C: two spare rows (columns when transposed) and a spare tail per batch entry
    if cs.ct:
        crows, ldc = N + 2, M + 3
    else:
        crows, ldc = rows + 2, N + 3
    c_bs = crows * ldc + 13
    tC = up(np.full(B * c_bs, SENTINEL, np.float32))
    a.C, a.c_bs, a.ldc, a.c_transposed, a.B = tC.data_ptr(), c_bs, ldc, int(cs.ct), B
    if cs.split:
        nws = 16 * B * M * N   # the most gemm_launch asks for (16 splits)
        tWs = up(np.full(nws + 32, np.nan, np.float32))
        a.splitk_ws, a.splitk_ws_bytes = tWs.data_ptr(), nws * 4
    with shape_env(shape):
        rc = P.probe_gemm(c.byref(a), stream)
    assert rc == OK, last_error()
    torch.cuda.synchronize()
    raw = tC.cpu().numpy()
    packed = tA.cpu().numpy()
    assert np.isnan(packed[pbytes // 4:]).all(), "pack_a wrote behind packed_a_float4s"
    # the window in C's layout
    win = np.concatenate([ref_win, ref_win], 1) if cs.gate else ref_win
    out = np.full((B, rows, N), SENTINEL, np.float32)
    inside = np.zeros(raw.shape, bool)
    for b in range(B):
        slab = raw[b * c_bs:b * c_bs + crows * ldc].reshape(crows, ldc)
        ins = inside[b * c_bs:b * c_bs + crows * ldc].reshape(crows, ldc)
        if cs.ct:
            ins[:N, :rows] = win[b].T
            vals = slab[:N, :rows].T
        else:
            ins[:rows, :N] = win[b]
            vals = slab[:rows, :N]
        out[b][win[b]] = vals[win[b]]
    stray = np.flatnonzero(~inside & (raw != SENTINEL))
    assert stray.size == 0, "%d stores outside the output window, first at C + %d" % (stray.size, stray[0])
    assert np.isfinite(raw[inside]).all(), "non-finite output inside the window: padding that should read as zero was used"
    return Run(out=out, raw=raw, packed=packed, packed_floats=pbytes // 4)


def run_shapes(cs, d=None):
    """-> {shape name: Run}: the default shape, and the 64-column kernel too where the default is the latency shape; the
    two must agree bit for bit."""
    runs = {"default": run_case(cs, d)}
    if cs.both_shapes():
        runs["legacy"] = run_case(cs, d, "legacy")
        assert np.array_equal(runs["default"].raw, runs["legacy"].raw), "latency shape and 64-column kernel differ"
    return runs


def ulp_distance(x, ref):
    """|x - ref| in units of float32's spacing at ref (ref float64)"""
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(x.astype(np.float64) - ref) / sp
