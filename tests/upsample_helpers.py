"""Direct tests of the bf16 training upsampler (csrc/facppg_train_bf16.hip: facppg_upsample_regroup_bf16 and
facppg_upsample_regroup_backward): the case list that test_upsample_reference_cpu.py and test_gpu_upsample.py share, a float64
NumPy reference written from the reference's formula (glow.py:184-186, 214-222), and a runner that surrounds every buffer
with poison.

Contract.  y = ConvTranspose1d(80, 80, ksize, stride hop)(mel), i.e.
    y[b][m][q hop + k] = bias[m] + sum_{m'} mel[b][m'][q] W[m'][m][k]         (0 <= q < T, 0 <= k < ksize),
cropped to 8 L samples (every call with (T - 1) hop + ksize >= 8 L is accepted) and regrouped into the position-major bf16
operand spect[b][l][8 m + g] = y[b][m][8 l + g] of Lr = facppg_wn_bf16_padded_len(L) rows, rows [L, Lr) zero.  Backward, from
the fp32 position-major gradient dspect of Lr rows (dup[b][m][n] = dspect[b][n / 8][8 m + n % 8] for n < 8 L, 0 beyond):
    dW[m'][m][k] = sum_{b, q} mel[b][m'][q] dup[b][m][q hop + k],        db[m] = sum_{b, n} dup[b][m][n]."""
import collections
import ctypes
import dataclasses
import functools
import zlib

import numpy as np
import pytest

NM = 80                                  # the entry points require 80 mel channels
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
U = 2.0 ** -24                           # unit roundoff of float32
UMAXJ = 8                                # kernel taps per hop the forward supports (ceil(ksize / hop) <= UMAXJ)
GUARD = 4096                             # bytes of poison behind every buffer the kernels write
NAN_BF16 = 0x7FC0


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    hop: int
    ksize: int
    B: int
    T: int
    L: int
    data: str = "int"        # int: ternary operands, every sum an integer bf16 holds | random: standard normal
    path: str = "gemm"       # gemm | scalar (FACPPG_UPSAMPLE_GEMM=0) | no_ws (forward without a workspace)

    @property
    def id(self):
        return "h%d-k%d-B%d-T%d-L%d-%s-%s" % (self.hop, self.ksize, self.B, self.T, self.L, self.data, self.path)

    @property
    def shape(self):
        """what the reference depends on: everything but the path"""
        return dataclasses.replace(self, path="gemm")

    @property
    def nj(self):
        return -(-self.ksize // self.hop)

    @property
    def accepted(self):
        return (self.T - 1) * self.hop + self.ksize >= 8 * self.L

    @property
    def forward_supported(self):
        return self.nj <= UMAXJ

    @property
    def tail(self):
        """samples at or past T hop: formed by the kernel tails of earlier frames alone"""
        return 8 * self.L > self.T * self.hop


def _shapes():
    out = []
    for hop, ks in ((160, 1024), (256, 1024)):
        B, T = 2, 6
        for L in ((T - 1) * hop // 8,                     # the training relation
                  83,                                     # crop inside a frame, fewer output frames than mel frames
                  128, 129,                               # Lr boundary
                  {160: 150, 256: 224}[hop],              # tail: 8 L > T hop
                  ((T - 1) * hop + ks) // 8):             # longest accepted tail
            out.append((hop, ks, B, T, L))
        out += [(hop, ks, 1, 1, 1), (hop, ks, 1, 1, 128)]  # one frame; L = 128 is almost all tail
    out += [(160, 1024, 3, 23, 440),                      # 66 GEMM rows: K of the backward product > 64, batch stride
            (160, 1024, 3, 23, 450),                      # 69 GEMM rows: > 64 and odd
            (160, 800, 2, 6, 100),                        # nj = 5 exactly
            (256, 1000, 2, 6, 160),                       # last tap group partly beyond the kernel
            (256, 200, 2, 6, 160),                        # ksize < hop: phases pp >= 200 are bias only
            (8, 64, 2, 40, 39),                           # nj = UMAXJ, one 8-sample piece per frame
            (8, 72, 2, 40, 39)]                           # nj = 9: forward unsupported, backward on the scalar kernel
    return out


SHAPES = tuple(_shapes())
CASES = tuple(Case(*s, data=d, path=p) for s in SHAPES for d in ("int", "random") for p in ("gemm", "scalar"))
NO_WS_CASES = (Case(160, 1024, 2, 6, 150, "int", "no_ws"), Case(256, 1024, 2, 6, 224, "int", "no_ws"),
               Case(8, 64, 2, 40, 39, "int", "no_ws"))
REJECTED = Case(160, 1024, 2, 6, 229)                     # (T - 1) hop + ksize = 1824 < 8 L = 1832
SMALL_CPU_CASES = (Case(8, 40, 2, 6, 8), Case(8, 40, 2, 6, 10, "random"), Case(16, 8, 1, 3, 5, "random"))


# ----------------------------------------------------------------------------------------------------------------- data
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=2)
def _weights(ksize, data, hop):
    """-> (W float32, W float64, |W| float64), [80, 80, ksize]: drawn once per kernel size and kind of data (80 x 80 x 1024
    values cost more than everything else in a case), shared by the cases that use it; a short cache, 130 MB an entry."""
    g = np.random.Generator(np.random.PCG64([ksize, zlib.crc32(data.encode())]))
    shp = (NM, NM, ksize)
    if data == "int":
        W = (g.integers(-1, 2, shp, dtype=np.int8) * (g.random(shp, dtype=np.float32) < 0.375)).astype(np.float32)
    else:
        # synth.waveglow_state_dict: ~1024 / hop taps x 80 channels meet in every sample
        W = g.standard_normal(shp, dtype=np.float32) * np.float32(0.2 / np.sqrt(NM * 1024.0 / hop))
    W64 = W.astype(np.float64)
    return _frozen(W), _frozen(W64), _frozen(np.abs(W64))


def weights(shape):
    return _weights(shape.ksize, shape.data, shape.hop if shape.data == "random" else 0)


@functools.lru_cache(maxsize=4)
def operands(shape):
    """-> dict of float32 arrays mel [B, 80, T], W [80, 80, ksize], bias [80], dspect [B, L, 640] (read-only)."""
    c = shape
    g = np.random.Generator(np.random.PCG64(zlib.crc32(c.id.encode())))
    if c.data == "int":
        mel = (g.integers(-1, 2, (c.B, NM, c.T)) * (g.random((c.B, NM, c.T)) < 0.375)).astype(np.float32)
        bias = g.integers(-2, 3, NM).astype(np.float32)
        dspect = g.integers(-1, 2, (c.B, c.L, NM * 8)).astype(np.float32)
    else:
        mel = g.standard_normal((c.B, NM, c.T), dtype=np.float32)
        bias = g.standard_normal(NM, dtype=np.float32) * np.float32(0.01)
        dspect = g.standard_normal((c.B, c.L, NM * 8), dtype=np.float32)
    return {k: _frozen(v) for k, v in dict(mel=mel, W=weights(c)[0], bias=bias, dspect=dspect).items()}


# ------------------------------------------------------------------------------------------------------------ reference
def conv_transpose(mel, W, bias, hop):
    """float64 ConvTranspose1d, stride hop: every frame adds its kernel at q hop.  -> [B, 80, (T - 1) hop + ksize]"""
    B, nm, T = mel.shape
    ks = W.shape[2]
    cols = (mel.transpose(0, 2, 1).reshape(B * T, nm) @ W.reshape(nm, -1)).reshape(B, T, W.shape[1], ks)
    y = np.tile(bias[None, :, None], (B, 1, (T - 1) * hop + ks))
    for q in range(T):
        y[:, :, q * hop:q * hop + ks] += cols[:, q]
    return y


def regroup(y, L, Lr):
    """[B, 80, >= 8 L] -> [B, Lr, 640]: spect[b][l][8 m + g] = y[b][m][8 l + g], rows [L, Lr) zero"""
    B, nm = y.shape[:2]
    out = np.zeros((B, Lr, nm * 8))
    out[:, :L] = y[:, :, :8 * L].reshape(B, nm, L, 8).transpose(0, 2, 1, 3).reshape(B, L, nm * 8)
    return out


def ungroup(dspect, n_total):
    """[B, L, 640] -> dup [B, 80, n_total]: the inverse of regroup, zero from sample 8 L on"""
    B, L, _ = dspect.shape
    dup = np.zeros((B, NM, n_total))
    dup[:, :, :8 * L] = dspect.reshape(B, L, NM, 8).transpose(0, 2, 1, 3).reshape(B, NM, 8 * L)
    return dup


def weight_grad(mel, dup, hop, ks):
    """dW[m'][m][k] = sum_{b, q} mel[b][m'][q] dup[b][m][q hop + k]"""
    B, nm, T = mel.shape
    win = np.stack([dup[:, :, q * hop:q * hop + ks] for q in range(T)], axis=1)          # [B, T, 80, ks]
    return (mel.transpose(1, 0, 2).reshape(nm, B * T) @ win.reshape(B * T, -1)).reshape(nm, dup.shape[1], ks)


@dataclasses.dataclass(frozen=True, eq=False)
class ForwardReference:
    spect: np.ndarray     # [B, Lr, 640] float64
    S_fwd: np.ndarray     # the same sums of absolute values


@dataclasses.dataclass(frozen=True, eq=False)
class BackwardReference:
    dW: np.ndarray        # [80, 80, ksize] float64
    db: np.ndarray        # [80]
    S_dW: np.ndarray      # the same sums of absolute values
    S_db: np.ndarray


def padded_len(L):
    from facppg import lib
    return lib.load().facppg_wn_bf16_padded_len(L)


# Both references are computed once per shape and shared by the paths, whose cases follow each other in CASES; the caches are
# short because a weight gradient in float64 is 52 MB.
@functools.lru_cache(maxsize=2)
def forward_reference(shape):
    c = shape
    assert c.accepted
    o = operands(c)
    _, W, absW = weights(c)
    mel, bias = o["mel"].astype(np.float64), o["bias"].astype(np.float64)
    Lr = padded_len(c.L)
    return ForwardReference(_frozen(regroup(conv_transpose(mel, W, bias, c.hop), c.L, Lr)),
                            _frozen(regroup(conv_transpose(np.abs(mel), absW, np.abs(bias), c.hop), c.L, Lr)))


@functools.lru_cache(maxsize=2)
def backward_reference(shape):
    c = shape
    assert c.accepted
    o = operands(c)
    mel = o["mel"].astype(np.float64)
    dup = ungroup(o["dspect"].astype(np.float64), (c.T - 1) * c.hop + c.ksize)
    return BackwardReference(*map(_frozen, (weight_grad(mel, dup, c.hop, c.ksize), dup.sum(axis=(0, 2)),
                                            weight_grad(np.abs(mel), np.abs(dup), c.hop, c.ksize), np.abs(dup).sum(axis=(0, 2)))))


def forward_tolerance(case, ref):
    """|out - y| <= 2^-8 (|y| + E) + E, E = (K + 3) 2 U S_fwd, K = 80 ceil(ksize / hop): one bf16 rounding of an fp32 sum of K
    products and the bias, whatever the order (the GEMM tests' summation bound, tests/gemm_helpers.py)."""
    E = (NM * case.nj + 3) * 2 * U * ref.S_fwd
    return 2.0 ** -8 * (np.abs(ref.spect) + E) + E


def dW_tolerance(case, ref):
    return (case.B * case.T + 2) * 2 * U * ref.S_dW


def db_tolerance(case, ref):
    return (case.B * 8 * case.L + 2) * U * ref.S_db


def bf16_bits(x64):
    """float64 array -> the uint16 patterns of its round-to-nearest-even bf16 values (torch's conversion)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def bf16_to_f64(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- runner
def _lib():
    from facppg import lib
    return lib, lib.load()


def _guarded(nbytes, fill_byte):
    """uint8 device buffer of nbytes + GUARD bytes, all fill_byte"""
    import torch
    return torch.full((nbytes + GUARD,), fill_byte, dtype=torch.uint8, device="cuda")


def _guard_intact(buf, nbytes, fill_byte):
    return bool((buf[nbytes:] == fill_byte).all())


def _input(a, tail=GUARD // 4):
    """float32 array -> flat device tensor followed by `tail` NaNs: a read past an operand's end shows as NaN in the result"""
    import torch
    t = torch.full((a.size + tail,), float("nan"), device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)
    return t


def _path_env(mp, path):
    if path == "scalar":
        mp.setenv("FACPPG_UPSAMPLE_GEMM", "0")
    else:
        mp.delenv("FACPPG_UPSAMPLE_GEMM", raising=False)


def last_error():
    return _lib()[1].facppg_last_error().decode()


_results = collections.OrderedDict()     # the last few results: a case's two paths are compared without a second run


def _cached(key, run):
    if key not in _results:
        _results[key] = run()
        while len(_results) > 4:
            _results.popitem(last=False)
    return _results[key]


def run_forward(case):
    """-> (rc, spect bits uint16 [B, Lr, 640] or None).  The output starts as bf16 NaN, the workspace as 0xFF bytes of exactly
    facppg_upsample_forward_workspace_bytes; the guard tails behind both must come back untouched."""
    return _cached(("fwd", case), lambda: _run_forward(case))


def _run_forward(case):
    import torch
    lib, L = _lib()
    c = case
    o = operands(c.shape)
    mel, W, bias = (_input(o[k]) for k in ("mel", "W", "bias"))
    Lr = padded_len(c.L)
    out_bytes = c.B * Lr * NM * 8 * 2
    out = _guarded(out_bytes, 0)
    out.view(torch.int16).fill_(NAN_BF16)
    ws_bytes = L.facppg_upsample_forward_workspace_bytes(c.B, c.T, NM, c.hop, c.ksize, c.L)
    ws = _guarded(ws_bytes, 0xFF)
    with pytest.MonkeyPatch.context() as mp:
        _path_env(mp, c.path)
        no_ws = c.path == "no_ws"
        rc = L.facppg_upsample_regroup_bf16(lib.ptr(mel), lib.ptr(W), lib.ptr(bias), c.B, c.T, NM, c.hop, c.ksize, c.L, lib.ptr(out),
                                            ctypes.c_void_p(0) if no_ws else lib.ptr(ws), 0 if no_ws else ws_bytes,
                                            lib.current_stream(mel.device))
        torch.cuda.synchronize()
    assert _guard_intact(ws, ws_bytes, 0xFF), "forward wrote behind its workspace"
    assert bool((out[out_bytes:].view(torch.int16) == NAN_BF16).all()), "forward wrote behind spect_pm"
    if rc != OK:
        return rc, None
    return rc, out[:out_bytes].view(torch.int16).cpu().numpy().view(np.uint16).reshape(c.B, Lr, NM * 8)


def run_backward(case):
    """-> (rc, dW [80, 80, ksize], db [80]) float32.  dspect rows [L, Lr) are NaN (the kernels must not read them), dW and db
    start as NaN with NaN guard tails, the workspace as 0xFF bytes of exactly facppg_upsample_backward_workspace_bytes plus a
    guard tail."""
    return _cached(("bwd", case), lambda: _run_backward(case))


def _run_backward(case):
    import torch
    lib, L = _lib()
    c = case
    o = operands(c.shape)
    mel = _input(o["mel"])
    Lr = padded_len(c.L)
    padded = np.full((c.B, Lr, NM * 8), np.nan, dtype=np.float32)
    padded[:, :c.L] = o["dspect"]
    dspect = _input(padded, tail=32 * NM * 8)           # (a frame of hop <= 256 samples spans at most 32 rows)
    n_dw, n_db, n_guard = NM * NM * c.ksize, NM, GUARD // 4
    dW = torch.full((n_dw + n_guard,), float("nan"), device="cuda")
    db = torch.full((n_db + n_guard,), float("nan"), device="cuda")
    ws_bytes = L.facppg_upsample_backward_workspace_bytes(c.B, c.T, NM, c.hop, c.ksize, c.L)
    ws = _guarded(ws_bytes, 0xFF)
    with pytest.MonkeyPatch.context() as mp:
        _path_env(mp, c.path)
        rc = L.facppg_upsample_regroup_backward(lib.ptr(mel), lib.ptr(dspect), c.B, c.T, NM, c.hop, c.ksize, c.L, lib.ptr(dW), lib.ptr(db),
                                                lib.ptr(ws), ws_bytes, lib.current_stream(mel.device))
        torch.cuda.synchronize()
    assert _guard_intact(ws, ws_bytes, 0xFF), "backward wrote behind its workspace"
    assert bool(torch.isnan(dW[n_dw:]).all()) and bool(torch.isnan(db[n_db:]).all()), "backward wrote behind dW / db"
    after = dspect[:padded.size].cpu().numpy().reshape(padded.shape)
    assert np.isnan(after[:, c.L:]).all() and np.array_equal(after[:, :c.L], o["dspect"]), "backward changed dspect"
    return rc, dW[:n_dw].cpu().numpy().reshape(NM, NM, c.ksize), db[:n_db].cpu().numpy()
