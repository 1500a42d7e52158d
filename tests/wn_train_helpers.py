"""Direct tests of the fp32 training direction of one WaveGlow WN stack (csrc/facppg_wg.hip: facppg_wn_forward_save,
facppg_wn_backward_data; csrc/facppg_train.hip: facppg_wn_weight_grads): the case lists that test_wn_train_reference_cpu.py and
test_gpu_wn_train.py share, two float64 references, and a runner that surrounds every buffer with poison.

Reference 1, stack_reference: WN.forward of the reference (glow.py:154-175) written out as matrix products in torch, in float64
(or float32, to measure what fp32 arithmetic costs on a case), with everything the kernels keep and, through autograd, every
gradient and every intermediate gradient:
    h_0 = Ws a0 + bs
    pre_i = sum_tap Win_i[:, :, tap] h_i[n + (tap - 1) 2^i] + Wc_i spect + bin_i + bc_i        (h_i zero outside [0, L))
    T_i, S_i = tanh(pre_i[:256]), sigmoid(pre_i[256:])
    rs_i = Wrs_i (T_i S_i) + brs_i;   h_{i+1} = h_i + rs_i[:256], skip += rs_i[256:]   (last layer: skip += rs_i, 256 rows)
    out = We skip + be
Reference 2, weight_grad_reference: the NT products and row sums of facppg_wn_weight_grads in float64 NumPy on the KERNEL'S
buffers (padded rows, margins, NaN past L), written from the comment above k_wgrad_f32 and from k_wn_grad_tables.

Buffers (Lr = round_up(L, 64), Lp = 128 + Lr + 128):
    a0 [B][n_in][L]   spect_pad [B][640][Lr]   out, dout [B][2 n_in][L]   da0 [B][n_in][L]
    h_all [n_layers + 1][B][256][Lp]     layer inputs at columns [128, 128 + L), EXACT ZERO everywhere else (the weight
                                         gradient's taps and the next layer's taps read the margins)
    ts_all, dpre_all [n_layers][B][512][Lr]   skip, dskip [B][256][Lr]   dh_all [n_layers + 1][B][256][Lr], dh_all[n_layers] = 0
    dspect [B][640][Lr]
Columns [L, Lr) of spect_pad, ts_all, skip, dpre_all, dskip are never written and may hold anything, NaN included: every kernel
masks them."""
import collections
import ctypes
import dataclasses
import functools
import zlib

import numpy as np

CH, NC, HALO, TN = 256, 640, 128, 64
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -4
U = 2.0 ** -24                           # unit roundoff of float32
GUARD = 1024                             # floats of poison behind every buffer a kernel writes
SENTINEL = float(np.float32(-1.2345e30))
FLOOR = 16 * U                           # the chained comparison's floor on max|err| / max|ref|
MARGIN = 4.0                             # ... and how many times the CPU's own fp32 error the kernels may take


def round_up(x, m):
    return -(-x // m) * m


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    n_in: int
    n_layers: int
    B: int
    L: int
    data: str = "int"        # int: ternary operands | random: standard normal operands, weights scaled as synth.waveglow_state_dict

    @property
    def id(self):
        return "in%d-nl%d-B%d-L%d-%s" % (self.n_in, self.n_layers, self.B, self.L, self.data)

    @property
    def Lr(self):
        return round_up(self.L, TN)

    @property
    def Lp(self):
        return HALO + self.Lr + HALO

    @property
    def wide(self):
        """facppg_wn_forward_save's plan: 64-wide tiles (k_wn_layer<*, 2, true>) from 768 tiles on"""
        return (self.Lr // TN) * self.B >= 768


WG_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 129, 240)


def _wg_cases():
    """facppg_wn_weight_grads called directly on ternary operands: every L with both batch sizes and all n_in; L below the
    dilation (L <= 5 against 2^i up to 128, and every L < 128 with 8 layers); odd L (rows of a0 / dout start at any 4-byte
    address); one layer (the only layer is the last: skip-only rs_w), two (res and skip rows), eight."""
    out = []
    for k, L in enumerate(WG_LENGTHS):
        out.append(Case(1 + k % 4, 2, 1, L))
        out.append(Case(1 + (k + 1) % 4, 1, 3, L))
        out.append(Case(1 + (k + 2) % 4, 2 if k % 2 else 1, 3 if k % 2 else 1, L))
    for n_in in (1, 2, 3, 4):
        out += [Case(n_in, 2, 3, 3), Case(n_in, 1, 1, 5), Case(n_in, 2, 1, 65)]
    for k, L in enumerate((1, 5, 33, 64, 65, 127, 129, 240)):
        out.append(Case(1 + k % 4, 8, 1 + 2 * (k % 2), L))
    return tuple(dict.fromkeys(out))


WG_CASES = _wg_cases()
WG_RANDOM_CASES = (Case(3, 2, 3, 129, "random"), Case(1, 8, 1, 65, "random"), Case(4, 1, 3, 240, "random"))

# forward, backward and weight gradients chained: every n_in, n_layers 1 / 3 / 8, both batch sizes, every L
CHAIN_CASES = (Case(1, 1, 1, 1, "random"), Case(2, 1, 2, 63, "random"), Case(3, 1, 1, 150, "random"), Case(4, 1, 2, 240, "random"),
               Case(1, 3, 2, 64, "random"), Case(2, 3, 1, 65, "random"), Case(3, 3, 2, 1, "random"), Case(4, 3, 1, 63, "random"),
               Case(1, 3, 1, 240, "random"), Case(1, 8, 2, 150, "random"), Case(2, 8, 1, 240, "random"), Case(3, 8, 2, 65, "random"),
               Case(4, 8, 1, 64, "random"), Case(4, 8, 2, 240, "random"), Case(2, 8, 1, 1, "random"), Case(1, 8, 1, 63, "random"))
WIDE_CASE = Case(4, 1, 12, 4090, "random")            # Lr = 4096: 64 tiles x 12 = 768, the first shape of the wide plan
WIDE_CASE_2 = Case(4, 2, 12, 4090, "random")          # ... and k_wn_layer<false, 2, true>


def weight_shapes(n_in, n_layers):
    """name -> shape, in the order of facppg_wn_weights (and of _WNFunction's inputs)"""
    s = collections.OrderedDict()
    s["start_w"], s["start_b"] = (CH, n_in), (CH,)
    for i in range(n_layers):
        rs = CH if i == n_layers - 1 else 2 * CH
        s["in_w.%d" % i], s["in_b.%d" % i] = (2 * CH, CH, 3), (2 * CH,)
        s["cond_w.%d" % i], s["cond_b.%d" % i] = (2 * CH, NC), (2 * CH,)
        s["rs_w.%d" % i], s["rs_b.%d" % i] = (rs, CH), (rs,)
    s["end_w"], s["end_b"] = (2 * n_in, CH), (2 * n_in,)
    return s


# ----------------------------------------------------------------------------------------------------------------- data
def _frozen(a):
    a.setflags(write=False)
    return a


def _rng(case, what):
    return np.random.Generator(np.random.PCG64([zlib.crc32(case.id.encode()), zlib.crc32(what.encode())]))


def _ternary(g, shape, density=0.5):
    return (g.integers(-1, 2, shape) * (g.random(shape) < density)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def wg_operands(case):
    """The nine saved tensors of facppg_wn_weight_grads in the kernel's layout, float32, read-only.  Live columns: ternary
    values (random cases: standard normal; the gate halves in (-1, 1) and (0, 1)).  h_all: exact zeros in [0, 128) and
    [128 + L, 256 + L), the columns the taps can reach; NaN in [256 + L, Lp) and in the whole of h_all[n_layers], which nothing
    reads.  NaN in [L, Lr) of everything else and in the whole of dh_all[n_layers] (the last layer has no res rows)."""
    c = case
    B, L, Lr, Lp, nl = c.B, c.L, c.Lr, c.Lp, c.n_layers
    g = _rng(c, "wg")

    def live(shape, kind=None):
        if c.data == "int":
            return _ternary(g, shape)
        x = g.standard_normal(shape, dtype=np.float32)
        return np.tanh(x) if kind == "t" else (1 / (1 + np.exp(-x))).astype(np.float32) if kind == "s" else x

    def padded(shape_live, ld):
        a = np.full(shape_live[:-1] + (ld,), np.nan, dtype=np.float32)
        a[..., :L] = live(shape_live)
        return a

    o = {"a0": live((B, c.n_in, L)), "dout": live((B, 2 * c.n_in, L)), "spect": padded((B, NC, L), Lr), "skip": padded((B, CH, L), Lr),
         "dskip": padded((B, CH, L), Lr), "dpre_all": padded((nl, B, 2 * CH, L), Lr), "dh_all": padded((nl + 1, B, CH, L), Lr)}
    o["dh_all"][nl] = np.nan
    ts = np.full((nl, B, 2 * CH, Lr), np.nan, dtype=np.float32)
    ts[:, :, :CH, :L], ts[:, :, CH:, :L] = live((nl, B, CH, L), "t"), live((nl, B, CH, L), "s")
    o["ts_all"] = ts
    h = np.full((nl + 1, B, CH, Lp), np.nan, dtype=np.float32)
    h[:nl, :, :, :HALO + L + HALO] = 0.0
    h[:nl, :, :, HALO:HALO + L] = live((nl, B, CH, L))
    o["h_all"] = h
    return {k: _frozen(v) for k, v in o.items()}


def _normal(g, shape, std):
    return (g.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)


@functools.lru_cache(maxsize=2)
def chain_operands(case):
    """-> (weights: name -> float32 array, scaled as synth.waveglow_state_dict scales them; a0, spect [B, 640, L], dout)"""
    c = case
    g = _rng(c, "chain")
    std = {"start_w": 1.0 / np.sqrt(c.n_in), "in_w": 1.0 / np.sqrt(CH * 3), "cond_w": 1.0 / np.sqrt(NC), "rs_w": 1.0 / np.sqrt(CH),
           "end_w": 0.01, "end_b": 0.02}
    w = collections.OrderedDict((k, _frozen(_normal(g, s, std.get(k.split(".")[0], 0.01)))) for k, s in weight_shapes(c.n_in, c.n_layers).items())
    a0, spect, dout = (_frozen(g.standard_normal(s, dtype=np.float32)) for s in ((c.B, c.n_in, c.L), (c.B, NC, c.L), (c.B, 2 * c.n_in, c.L)))
    return w, a0, spect, dout


# ------------------------------------------------------------------------------------------------------------ reference
def _stack_forward(w, a0, spect, n_layers, keep):
    """torch, any float dtype; `keep` receives every tensor the kernels keep (and, under autograd, retains its gradient)"""
    import torch
    L = a0.shape[2]
    h = keep("h.0", torch.einsum("mc,bcn->bmn", w["start_w"], a0) + w["start_b"][None, :, None])
    skip = None
    for i in range(n_layers):
        d = 2 ** i
        hp = torch.nn.functional.pad(h, (d, d))
        pre = torch.einsum("mc,bcn->bmn", w["cond_w.%d" % i], spect) + (w["in_b.%d" % i] + w["cond_b.%d" % i])[None, :, None]
        for tap in range(3):
            pre = pre + torch.einsum("mc,bcn->bmn", w["in_w.%d" % i][:, :, tap], hp[:, :, tap * d:tap * d + L])
        pre = keep("pre.%d" % i, pre)
        t, s = torch.tanh(pre[:, :CH]), torch.sigmoid(pre[:, CH:])
        keep("ts.%d" % i, torch.cat([t, s], 1))
        rs = torch.einsum("mc,bcn->bmn", w["rs_w.%d" % i], t * s) + w["rs_b.%d" % i][None, :, None]
        if i < n_layers - 1:
            h = keep("h.%d" % (i + 1), h + rs[:, :CH])
            sk = rs[:, CH:]
        else:
            sk = rs
        skip = sk if skip is None else skip + sk
    skip = keep("skip", skip)
    return keep("out", torch.einsum("mc,bcn->bmn", w["end_w"], skip) + w["end_b"][None, :, None])


def stack_reference(weights, a0, spect, dout, dtype="float64"):
    """-> name -> float64 NumPy array: out, h.i, ts.i ([B, 512, L]: tanh rows then sigmoid rows), skip; the gradients of
    sum(out * dout): da0, dspect, g.<weight name>, and of the kept tensors dpre.i, dh.i, dskip.  Computed in `dtype`."""
    import torch
    dt = getattr(torch, dtype)
    n_layers = (len(weights) - 4) // 6
    leaf = lambda x: torch.from_numpy(np.array(x)).to(dt).requires_grad_(True)
    w = {k: leaf(v) for k, v in weights.items()}
    a0_t, spect_t = leaf(a0), leaf(spect)
    kept = {}

    def keep(name, x):
        x.retain_grad()
        kept[name] = x
        return x

    out = _stack_forward(w, a0_t, spect_t, n_layers, keep)
    (out * torch.from_numpy(np.array(dout)).to(dt)).sum().backward()
    f64 = lambda x: x.detach().double().numpy()
    r = {"da0": f64(a0_t.grad), "dspect": f64(spect_t.grad)}
    for k, x in kept.items():
        if not k.startswith("pre."):
            r[k] = f64(x)
        if k.startswith(("pre.", "h.")) or k == "skip":
            r["d" + k] = f64(x.grad)
    for k, x in w.items():
        r["g." + k] = f64(x.grad)
    return r


@functools.lru_cache(maxsize=2)
def chain_reference(case):
    """-> (float64 reference, the same reference evaluated in float32 on the CPU)"""
    w, a0, spect, dout = chain_operands(case)
    return stack_reference(w, a0, spect, dout, "float64"), stack_reference(w, a0, spect, dout, "float32")


def ratio(got, ref):
    """max|got - ref| / max|ref| (the absolute error where the reference is all zero)"""
    scale = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (scale if scale > 0 else 1.0)


def to_kernel_layout(r, case, a0, spect, dout, fill=np.nan):
    """The nine saved tensors of facppg_wn_weight_grads, float64, from a stack_reference result: what facppg_wn_forward_save
    and facppg_wn_backward_data leave, with `fill` wherever they write nothing."""
    c = case
    B, L, Lr, Lp, nl = c.B, c.L, c.Lr, c.Lp, c.n_layers

    def padded(x, ld):
        a = np.full(x.shape[:-1] + (ld,), fill, dtype=np.float64)
        a[..., :L] = x
        return a

    h = np.zeros((nl + 1, B, CH, Lp))
    dh = np.zeros((nl + 1, B, CH, Lr))
    for i in range(nl):
        h[i, :, :, HALO:HALO + L] = r["h.%d" % i]
        dh[i, :, :, :L] = r["dh.%d" % i]
    return {"a0": a0.astype(np.float64), "dout": dout.astype(np.float64), "spect": padded(spect.astype(np.float64), Lr), "h_all": h,
            "ts_all": np.stack([padded(r["ts.%d" % i], Lr) for i in range(nl)]), "skip": padded(r["skip"], Lr),
            "dpre_all": np.stack([padded(r["dpre.%d" % i], Lr) for i in range(nl)]), "dh_all": dh, "dskip": padded(r["dskip"], Lr)}


def weight_grad_reference(o, n_in, n_layers, B, L, absolute=False):
    """float64 NumPy restatement of facppg_wn_weight_grads on the kernel's buffers `o` (wg_operands' layout).
    Every product is out[m * so_m + k * so_k] = sum_b sum_{n < L} A[b][m][n] X[b][k][n] (X optionally times X2), every bias
    gradient a row sum over b and n < L; columns >= L are never touched.  absolute: the same sums of absolute values.
    -> name -> array of weight_shapes."""
    Lr = round_up(L, TN)
    shapes = weight_shapes(n_in, n_layers)
    out = {k: np.full(int(np.prod(s)), np.nan) for k, s in shapes.items()}
    f = (lambda x: np.abs(x.astype(np.float64))) if absolute else (lambda x: x.astype(np.float64))

    def prob(A, M, X, X2, K, dst, off, so_m, so_k):
        a = f(A[:, :M, :L]).transpose(1, 0, 2).reshape(M, B * L)
        x = f(X[:, :K, :L])
        if X2 is not None:
            x = x * f(X2[:, :K, :L])
        p = a @ x.transpose(1, 0, 2).reshape(K, B * L).T
        idx = off + np.arange(M)[:, None] * so_m + np.arange(K)[None, :] * so_k
        out[dst][idx] = p

    def rowsum(src, n, dst, off=0, dst2=None):
        s = f(src[:, :n, :L]).sum(axis=(0, 2))
        out[dst][off:off + n] = s
        if dst2:
            out[dst2][off:off + n] = s

    dh, dpre_all, ts_all, h_all = o["dh_all"], o["dpre_all"], o["ts_all"], o["h_all"]
    prob(dh[0], CH, o["a0"], None, n_in, "start_w", 0, n_in, 1)
    rowsum(dh[0], CH, "start_b")
    for i in range(n_layers):
        last = i == n_layers - 1
        dpre, ts, h, d = dpre_all[i], ts_all[i], h_all[i], 1 << i
        for tap in range(3):     # in.w[m][c][tap] = sum dpre[m][n] h_i[c][n + (tap - 1) d]: the row starts at HALO + (tap - 1) d
            s0 = HALO + (tap - 1) * d
            prob(dpre, 2 * CH, h[:, :, s0:s0 + Lr], None, CH, "in_w.%d" % i, tap, 3 * CH, 3)
        prob(dpre, 2 * CH, o["spect"], None, NC, "cond_w.%d" % i, 0, NC, 1)
        rowsum(dpre, 2 * CH, "in_b.%d" % i, 0, "cond_b.%d" % i)
        if not last:             # res rows take dh_{i+1}, skip rows dskip; the last layer's rs_w is [256][256], skip only
            prob(dh[i + 1], CH, ts, ts[:, CH:], CH, "rs_w.%d" % i, 0, CH, 1)
            rowsum(dh[i + 1], CH, "rs_b.%d" % i)
        prob(o["dskip"], CH, ts, ts[:, CH:], CH, "rs_w.%d" % i, 0 if last else CH * CH, CH, 1)
        rowsum(o["dskip"], CH, "rs_b.%d" % i, 0 if last else CH)
    prob(o["dout"], 2 * n_in, o["skip"], None, CH, "end_w", 0, CH, 1)
    rowsum(o["dout"], 2 * n_in, "end_b")
    assert Lr >= L
    return {k: v.reshape(shapes[k]) for k, v in out.items()}


@functools.lru_cache(maxsize=2)
def wg_reference(case):
    """-> (gradients, the same sums of absolute values), float64, for wg_operands(case)"""
    o = wg_operands(case)
    return (weight_grad_reference(o, case.n_in, case.n_layers, case.B, case.L),
            weight_grad_reference(o, case.n_in, case.n_layers, case.B, case.L, absolute=True))


# --------------------------------------------------------------------------------------------------------------- runner
def _lib():
    from facppg import lib
    return lib, lib.load()


def last_error():
    return _lib()[1].facppg_last_error().decode()


def dev_input(a, tail=GUARD):
    """float32 array -> flat device tensor followed by `tail` NaNs: a read past an operand's end shows as NaN in the result"""
    import torch
    t = torch.full((a.size + tail,), float("nan"), device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().reshape(-1)
    return t


def dev_output(n):
    """n NaNs (production hands the kernels torch.empty) followed by GUARD sentinels"""
    import torch
    t = torch.full((n + GUARD,), float("nan"), device="cuda")
    t[n:] = SENTINEL
    return t


def dev_workspace(nbytes):
    """nbytes of 0xFF (NaN as float, -1 as an index) followed by 4 GUARD bytes of 0xA5"""
    import torch
    t = torch.full((nbytes + 4 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    t[nbytes:] = 0xA5
    return t


def guard_intact(t, n):
    if t.dtype.is_floating_point:
        return bool((t[n:] == SENTINEL).all())
    return bool((t[n:] == 0xA5).all())


def host(t, shape):
    n = int(np.prod(shape))
    return t[:n].cpu().numpy().reshape(shape)


def _struct(cls, tensors):
    st = cls()
    for k, t in tensors.items():
        name, _, i = k.partition(".")
        if i:
            getattr(st, name)[int(i)] = t.data_ptr()
        else:
            setattr(st, name, t.data_ptr())
    return st


def _grad_buffers(case):
    return collections.OrderedDict((k, dev_output(int(np.prod(s)))) for k, s in weight_shapes(case.n_in, case.n_layers).items())


def _call_weight_grads(case, dev, grads):
    """dev: the nine saved tensors on the device.  -> rc; asserts the workspace's guard"""
    import torch
    lib, L = _lib()
    c = case
    nbytes = L.facppg_wn_weight_grads_workspace_bytes(c.n_layers)
    ws = dev_workspace(nbytes)
    gs = _struct(lib.WnGrads, grads)
    rc = L.facppg_wn_weight_grads(c.n_in, c.n_layers, *(lib.ptr(dev[k]) for k in ("a0", "spect", "h_all", "ts_all", "skip", "dout", "dpre_all",
                                                                                  "dh_all", "dskip")),
                                  c.B, c.L, gs, lib.ptr(ws), nbytes, lib.current_stream(ws.device))
    torch.cuda.synchronize()
    assert guard_intact(ws, nbytes), "facppg_wn_weight_grads wrote behind its workspace"
    return rc


def _read_grads(case, grads):
    out = {}
    for k, s in weight_shapes(case.n_in, case.n_layers).items():
        assert guard_intact(grads[k], int(np.prod(s))), "a kernel wrote behind the gradient of " + k
        out[k] = host(grads[k], s)
        assert not np.isnan(out[k]).any(), "NaN (an element never written, or a masked column read) in the gradient of " + k
    return out


def run_weight_grads(case):
    """facppg_wn_weight_grads on wg_operands(case).  -> (rc, name -> float32 gradient)"""
    o = wg_operands(case)
    dev = {k: dev_input(v) for k, v in o.items()}
    grads = _grad_buffers(case)
    rc = _call_weight_grads(case, dev, grads)
    if rc != OK:
        return rc, None
    return rc, _read_grads(case, grads)


def run_chain(case):
    """facppg_wn_forward_save, facppg_wn_backward_data and facppg_wn_weight_grads on chain_operands(case), each handed what the
    one before left.  Every output and kept buffer starts as NaN with a sentinel tail, every workspace as 0xFF bytes, spect_pad
    holds NaN in [L, Lr), every operand is followed by NaN.  Asserted here: the tails are untouched; no output holds NaN in
    a column < L; h_all is exactly zero in [0, 128) and [128 + L, Lp) of every row of every layer; dh_all[n_layers] is exactly
    zero.  -> name -> float32 array cropped to the L live columns, named as stack_reference names them."""
    import torch
    lib, L = _lib()
    c = case
    B, Lg, Lr, Lp, nl, n_in = c.B, c.L, c.Lr, c.Lp, c.n_layers, c.n_in
    w, a0, spect, dout = chain_operands(c)
    wdev = collections.OrderedDict((k, dev_input(v)) for k, v in w.items())
    st = _struct(lib.WnWeights, wdev)
    spect_pad = np.full((B, NC, Lr), np.nan, dtype=np.float32)
    spect_pad[:, :, :Lg] = spect
    dev = {"a0": dev_input(a0), "spect": dev_input(spect_pad), "dout": dev_input(dout)}
    shapes = {"out": (B, 2 * n_in, Lg), "h_all": (nl + 1, B, CH, Lp), "ts_all": (nl, B, 2 * CH, Lr), "skip": (B, CH, Lr),
              "dpre_all": (nl, B, 2 * CH, Lr), "dh_all": (nl + 1, B, CH, Lr), "dskip": (B, CH, Lr), "dspect": (B, NC, Lr),
              "da0": (B, n_in, Lg)}
    for k, s in shapes.items():
        dev[k] = dev_output(int(np.prod(s)))
    nbytes = L.facppg_wn_train_workspace_bytes(nl, B, Lg)
    stream = lib.current_stream(dev["a0"].device)

    ws = dev_workspace(nbytes)
    rc = L.facppg_wn_forward_save(st, n_in, nl, lib.ptr(dev["a0"]), lib.ptr(dev["spect"]), B, Lg, lib.ptr(dev["out"]), lib.ptr(dev["h_all"]),
                                  lib.ptr(dev["ts_all"]), lib.ptr(dev["skip"]), lib.ptr(ws), nbytes, stream)
    torch.cuda.synchronize()
    assert rc == OK, (rc, last_error())
    assert guard_intact(ws, nbytes), "facppg_wn_forward_save wrote behind its workspace"
    ws.fill_(0xFF)
    ws[nbytes:] = 0xA5
    rc = L.facppg_wn_backward_data(st, n_in, nl, lib.ptr(dev["dout"]), lib.ptr(dev["ts_all"]), B, Lg, lib.ptr(dev["dpre_all"]),
                                   lib.ptr(dev["dh_all"]), lib.ptr(dev["dskip"]), lib.ptr(dev["dspect"]), lib.ptr(dev["da0"]), lib.ptr(ws),
                                   nbytes, stream)
    torch.cuda.synchronize()
    assert rc == OK, (rc, last_error())
    assert guard_intact(ws, nbytes), "facppg_wn_backward_data wrote behind its workspace"
    del ws
    grads = _grad_buffers(c)
    rc = _call_weight_grads(c, dev, grads)
    assert rc == OK, (rc, last_error())

    for k, s in shapes.items():
        assert guard_intact(dev[k], int(np.prod(s))), "a kernel wrote behind " + k
    # the margins and the zero slab, on the device (the wide case's h_all is 100 MB)
    h_all = dev["h_all"][:int(np.prod(shapes["h_all"]))].view(shapes["h_all"])
    assert not bool(h_all[..., :HALO].count_nonzero()), "h_all: the left margin is not exactly zero"
    assert not bool(h_all[..., HALO + Lg:].count_nonzero()), "h_all: columns [128 + L, Lp) are not exactly zero"
    assert not bool(h_all[nl].count_nonzero()), "h_all[n_layers] is written by no layer and must stay zero"
    dh_all = dev["dh_all"][:int(np.prod(shapes["dh_all"]))].view(shapes["dh_all"])
    assert not bool(dh_all[nl].count_nonzero()), "dh_all[n_layers] must be exactly zero"
    r = {"out": host(dev["out"], shapes["out"]), "da0": host(dev["da0"], shapes["da0"])}
    full = {k: host(dev[k], shapes[k]) for k in ("ts_all", "skip", "dpre_all", "dskip", "dspect")}
    for i in range(nl):
        r["h.%d" % i] = h_all[i, :, :, HALO:HALO + Lg].cpu().numpy()
        r["dh.%d" % i] = dh_all[i, :, :, :Lg].cpu().numpy()
        r["ts.%d" % i] = full["ts_all"][i, :, :, :Lg]
        r["dpre.%d" % i] = full["dpre_all"][i, :, :, :Lg]
    for k in ("skip", "dskip", "dspect"):
        r[k] = full[k][:, :, :Lg]
    for k, v in _read_grads(c, grads).items():
        r["g." + k] = v
    for k, v in r.items():
        assert not np.isnan(v).any(), "NaN in a column < L of " + k
    return r
