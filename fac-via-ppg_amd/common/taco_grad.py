"""Backward pass of the teacher-forced ``Tacotron2.forward`` (eval mode): gradients of all 61 parameter tensors.

``Tacotron2.forward(..., differentiable=True)`` keeps a ``ForcedState`` -- its inputs, the dropout masks it used, the encoder
output, the unmasked mel frames, the alignments and the hidden states of the two decoder LSTMCells of every frame -- and
returns its outputs through ``ForcedGraph``, whose backward is ``backward`` below.

How the work is divided ("The backward pass"):

* What is sequential runs on the HIP kernels of csrc/facppg_taco_bwd.hip (``HipRecurrences``): the cell-state scans, the
  decoder LSTM's backward chain, the attention chain (attention LSTMCell, softmax, location layer, query layer) and the two
  directions of the encoder's BiLSTM.  They leave the ADJOINTS OF THE PRE-ACTIVATIONS of every frame: dgates of the three
  LSTMs, d(tanh argument) and d(energies) of the attention, d(context).
* With the hidden states and alignments of the forward pass as constants, each of those pre-activations is a dense function of
  the parameters over all frames at once (``decoder_local``, ``bilstm_local``, ``encoder_front``, ``postnet``): torch matmuls
  on the saved activations.  ``torch.autograd.grad`` of those local functions against the kernels' adjoints gives every
  weight gradient and the data gradients between the stages (convolutions as unfold + matmul: rocBLAS, nothing else).

Padded-batch semantics hold as in the forward pass: the encoder's convolutions and the postnet see the zero-padded batch, so
bias and BatchNorm gradients include the padding columns.  One reference behaviour is reproduced on purpose: parse_output
masks ``mel`` through ``.data`` (model.py:573), IN PLACE on the tensor the postnet's first convolution saved for its weight
gradient, so that gradient (and only it) sees the masked frames while the forward value saw the unmasked ones.
"""
import torch
import torch.nn.functional as F

from facppg import lib as _lib


# ---------------------------------------------------------------------------------------- dense local functions
def conv1d_mm(x, w, b=None):
    """Conv1d (stride 1, 'same' padding, odd kernel) of x [B, C, T] with w [O, C, k] as unfold + one matmul."""
    k = w.shape[2]
    cols = F.pad(x, ((k - 1) // 2, (k - 1) // 2)).unfold(2, k, 1)            # [B, C, T, k]
    B, C, T, _ = cols.shape
    y = (cols.permute(0, 2, 1, 3).reshape(B * T, C * k) @ w.reshape(w.shape[0], C * k).t()).view(B, T, -1).transpose(1, 2)
    return y if b is None else y + b[None, :, None]


def bn_eval(x, bn):
    """BatchNorm1d on its running statistics: a per-channel affine map of x [B, C, T]."""
    scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return (x - bn.running_mean[None, :, None]) * scale[None, :, None] + bn.bias[None, :, None]


def shift(x):
    """x [B, T, ...] -> the previous frame's value at every frame (zeros at frame 0: the zero initial states)."""
    return torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)


def prenet(layers, x, masks):
    """Prenet.forward (model.py:132-135) on x [B, T, in] with keep-masks [2][B, T, out]: relu, mask, times 2."""
    for lin, m in zip(layers, masks):
        x = F.relu(x @ lin.linear_layer.weight.t()) * (m.to(x.dtype) * 2.0)
    return x


def postnet(model, mel, mel_masked):
    """Postnet.forward (model.py:178-184), eval mode, on mel [B, NF, T].  The first convolution's WEIGHT gradient is taken on
    ``mel_masked`` (see the module docstring); values and every other gradient are those of ``mel``."""
    x = mel
    n = len(model.postnet.convolutions)
    for j, (cv, bn) in enumerate(model.postnet.convolutions):
        if j == 0 and mel_masked is not None:
            seen = conv1d_mm(mel_masked, cv.conv.weight)
            x = conv1d_mm(x, cv.conv.weight.detach(), cv.conv.bias) + (seen - seen.detach())
        else:
            x = conv1d_mm(x, cv.conv.weight, cv.conv.bias)
        x = bn_eval(x, bn)
        if j < n - 1:
            x = torch.tanh(x)
    return x


def encoder_front(model, ppg, enc_masks):
    """Encoder.forward up to the BiLSTM (model.py:217-222), eval mode, over the padded batch: ppg [B, S, Tin], enc_masks
    [2, B, E, Tin] -> [B, Tin, E]."""
    x = prenet(model.encoder.prenet.layers, ppg.transpose(1, 2), [enc_masks[0].transpose(1, 2), enc_masks[1].transpose(1, 2)])
    x = x.transpose(1, 2)
    for cv, bn in model.encoder.convolutions:
        x = F.relu(bn_eval(conv1d_mm(x, cv.conv.weight, cv.conv.bias), bn))
    return x.transpose(1, 2)


def reverse_index(lengths, T, device):
    """[B, T] time indices that reverse each utterance's own valid frames (an involution; frames beyond the length stay)."""
    t = torch.arange(T, device=device)[None, :]
    ln = lengths.to(device).long()[:, None]
    return torch.where(t < ln, ln - 1 - t, t)


def bilstm_local(lstm, x, h, sfx):
    """Gate pre-activations of one direction of the encoder's LSTM for all frames, from its inputs x [B, T, E] and its saved
    hidden states h [B, T, H] (both in the direction's own time order): [B, T, 4H]."""
    w_ih, w_hh = getattr(lstm, "weight_ih_l0" + sfx), getattr(lstm, "weight_hh_l0" + sfx)
    return x @ w_ih.t() + shift(h) @ w_hh.t() + (getattr(lstm, "bias_ih_l0" + sfx) + getattr(lstm, "bias_hh_l0" + sfx))


def decoder_local(model, memory, targets, dec_masks, ah, dh, align):
    """The decoder's pre-activations of all frames as dense functions of the parameters and ``memory``, given the saved hidden
    states ah [B, T, A], dh [B, T, D] and alignments [B, T, Tin] (constants).  -> dict of
    gates_a [B, T, 4A], gates_d [B, T, 4D], out [B, T, NF + 1], ctx [B, T, E], s [B, T, Tin, AD], energies [B, T, Tin]."""
    d, att = model.decoder, model.decoder.attention_layer
    x0 = shift(targets.transpose(1, 2))                                       # go frame, then the targets (model.py:459-461)
    p = prenet(d.prenet.layers, x0, [dec_masks[0].transpose(1, 2), dec_masks[1].transpose(1, 2)])
    ctx = align @ memory
    ctx_c = ctx.detach()
    rnn_a, rnn_d = d.attention_rnn, d.decoder_rnn
    gates_a = torch.cat([p, shift(ctx_c)], 2) @ rnn_a.weight_ih.t() + shift(ah) @ rnn_a.weight_hh.t() + (rnn_a.bias_ih + rnn_a.bias_hh)
    gates_d = torch.cat([ah, ctx_c], 2) @ rnn_d.weight_ih.t() + shift(dh) @ rnn_d.weight_hh.t() + (rnn_d.bias_ih + rnn_d.bias_hh)
    w_out = torch.cat([d.linear_projection.linear_layer.weight, d.gate_layer.linear_layer.weight], 0)
    b_out = torch.cat([d.linear_projection.linear_layer.bias, d.gate_layer.linear_layer.bias], 0)
    out = torch.cat([dh, ctx_c], 2) @ w_out.t() + b_out
    B, T, Tin = align.shape
    loc_in = torch.stack([shift(align), shift(torch.cumsum(align, 1))], 2).reshape(B * T, 2, Tin)
    feat = conv1d_mm(loc_in, att.location_layer.location_conv.conv.weight)    # [B T, NFIL, Tin]
    loc = (feat.transpose(1, 2) @ att.location_layer.location_dense.linear_layer.weight.t()).view(B, T, Tin, -1)
    pm = memory @ att.memory_layer.linear_layer.weight.t()                    # [B, Tin, AD]
    s = (ah @ att.query_layer.linear_layer.weight.t())[:, :, None, :] + loc + pm[:, None]
    tanh_s = torch.tanh(s.detach())
    energies = (tanh_s * att.v.linear_layer.weight.reshape(-1)).sum(-1)       # (as a matrix-vector product: 2.9 ms in rocBLAS's gemv)
    return dict(gates_a=gates_a, gates_d=gates_d, out=out, ctx=ctx, s=s, energies=energies, tanh_s=tanh_s, w_out=w_out)


# ---------------------------------------------------------------------------------------- the recurrences, on HIP
class HipRecurrences(object):
    """The sequential parts, through the C ABI (csrc/facppg_taco_bwd.hip).  A missing symbol is an error of ``lib.load``."""

    def __init__(self, config, device):
        self.cfg, self.dev, self.L = config, device, _lib.load()
        self.launches = []          # (kernel family, N, T, H) of every call: the launch report of this backward pass

    def _f(self, t):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise _lib.FacppgError("the backward kernels take fp32 GPU tensors")
        return t.contiguous()

    def cell_scan(self, pre, lengths=None):
        act = self._f(pre.detach()).clone()
        N, T, H4 = act.shape
        c = torch.empty(N, T, H4 // 4, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.L.facppg_lstm_cell_scan(_lib.ptr(act), _lib.ptr(c), _lib.ptr(lengths), N, T, H4 // 4,
                                                    _lib.current_stream(self.dev)))
        return act, c

    def lstm_backward(self, w_hh, act, c, seed, lengths=None):
        w_hh, seed = self._f(w_hh.detach()), self._f(seed)
        N, T, H = c.shape
        dg = torch.empty_like(act)
        ws = torch.empty(self.L.facppg_lstm_backward_workspace_bytes(N, H), dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.L.facppg_lstm_backward(_lib.ptr(w_hh), _lib.ptr(act), _lib.ptr(c), _lib.ptr(seed), _lib.ptr(lengths), N, T, H,
                                                   _lib.ptr(dg), _lib.ptr(ws), ws.numel(), _lib.current_stream(self.dev)))
        self.launches.append(("lstm_backward", N, T, H))
        return dg

    def attention_backward(self, w_cat, w_query, v, w_loc_dense, w_loc_conv, memory, align, tanh_s, act_a, c_a, base_ctx, base_ah):
        ins = [self._f(t.detach()) for t in (w_cat, w_query, v, w_loc_dense, w_loc_conv, memory, align, tanh_s, act_a, c_a, base_ctx,
                                             base_ah)]
        B, T, Tin = align.shape
        A, E, AD = c_a.shape[2], memory.shape[2], tanh_s.shape[3]
        outs = [torch.empty(B, T, 4 * A, dtype=torch.float32, device=self.dev), torch.empty(B, T, E, dtype=torch.float32, device=self.dev),
                torch.empty(B, T, Tin, AD, dtype=torch.float32, device=self.dev), torch.empty(B, T, Tin, dtype=torch.float32, device=self.dev)]
        args = _lib.TacoAttentionBackwardArgs(*[t.data_ptr() for t in ins + outs])
        ws = torch.empty(self.L.facppg_taco_attention_backward_workspace_bytes(self.cfg, B, Tin), dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.L.facppg_taco_attention_backward(self.cfg, _lib.ctypes.byref(args), B, Tin, T, _lib.ptr(ws), ws.numel(),
                                                             _lib.current_stream(self.dev)))
        self.launches.append(("attention_backward", B, T, A))
        return outs


# ---------------------------------------------------------------------------------------- the backward pass
class ForcedState(object):
    """What one differentiable forward call keeps for its backward pass."""
    __slots__ = ("ppg", "lengths", "lengths_dev", "targets", "pad", "enc_masks", "dec_masks", "memory", "mel", "align", "ah", "dh",
                 "identity", "outputs", "launches")


def backward(model, st, g_mel, g_post, g_gate, rec=None):
    """Gradients of ``model.parameters()`` (in that order) for the output gradients g_mel, g_post [B, NF, T], g_gate [B, T]
    of the UNMASKED outputs (any may be None).  Also returns d loss / d memory."""
    if rec is None:
        rec = HipRecurrences(model._config(), st.memory.device)
    params = list(model.parameters())
    grads = {id(p): None for p in params}

    def take(ps, gs):
        for p, g in zip(ps, gs):
            if g is not None:
                grads[id(p)] = g if grads[id(p)] is None else grads[id(p)] + g

    zeros = lambda ref: torch.zeros_like(ref)                                 # noqa: E731
    g_mel = zeros(st.mel) if g_mel is None else g_mel
    g_gate = zeros(st.mel[:, 0]) if g_gate is None else g_gate
    d_mel = g_mel
    if g_post is not None:
        with torch.enable_grad():
            mel_in = st.mel.detach().requires_grad_(True)
            masked = st.mel.masked_fill(st.pad.unsqueeze(1), 0.0) if st.pad is not None else None
            y = postnet(model, mel_in, masked)
        ps = list(model.postnet.parameters())
        gs = torch.autograd.grad(y, [mel_in] + ps, g_post)
        d_mel = g_mel + g_post + gs[0]
        take(ps, gs[1:])
    d_out = torch.cat([d_mel.transpose(1, 2), g_gate.unsqueeze(2)], 2).contiguous()          # [B, T, NF + 1]

    # ---- decoder
    d = model.decoder
    with torch.enable_grad():
        memory = st.memory.detach().requires_grad_(True)
        loc = decoder_local(model, memory, st.targets, st.dec_masks, st.ah, st.dh, st.align)
    with torch.no_grad():
        D, A, P = d.decoder_rnn_dim, d.attention_rnn_dim, d.prenet_dim
        act_d, c_d = rec.cell_scan(loc["gates_d"])
        act_a, c_a = rec.cell_scan(loc["gates_a"])
        w_out = loc["w_out"].detach()
        dg_d = rec.lstm_backward(d.decoder_rnn.weight_hh, act_d, c_d, d_out @ w_out[:, :D])
        w_ih_d = d.decoder_rnn.weight_ih.detach()
        base_ah = dg_d @ w_ih_d[:, :A]
        base_ctx = d_out @ w_out[:, D:] + dg_d @ w_ih_d[:, A:]
        att = d.attention_layer
        w_cat = torch.cat([d.attention_rnn.weight_ih.detach()[:, P:], d.attention_rnn.weight_hh.detach()], 1)
        dg_a, d_ctx, d_s, d_e = rec.attention_backward(
            w_cat, att.query_layer.linear_layer.weight, att.v.linear_layer.weight.reshape(-1),
            att.location_layer.location_dense.linear_layer.weight, att.location_layer.location_conv.conv.weight,
            st.memory, st.align, loc["tanh_s"], act_a, c_a, base_ctx, base_ah)
    ps = list(d.parameters())
    gs = torch.autograd.grad([loc["gates_a"], loc["gates_d"], loc["out"], loc["ctx"], loc["s"], loc["energies"]], [memory] + ps,
                             [dg_a, dg_d, d_out, d_ctx, d_s, d_e], allow_unused=True)
    d_memory = gs[0]
    take(ps, gs[1:])
    del loc

    # ---- encoder: the BiLSTM's two chains, then the convolutions and the prenet over the padded batch
    enc = model.encoder
    H = enc.lstm.hidden_size
    with torch.enable_grad():
        x = encoder_front(model, st.ppg, st.enc_masks)
    B, Tin, _ = x.shape
    rev = reverse_index(st.lengths, Tin, x.device)
    d_x = torch.zeros_like(x)
    for k, sfx in enumerate(("", "_reverse")):
        idx = None if k == 0 else rev[:, :, None]
        order = (lambda t: t) if k == 0 else (lambda t: t.gather(1, idx.expand(-1, -1, t.shape[2])))
        with torch.enable_grad():
            x_k = order(x.detach()).requires_grad_(True)
            pre = bilstm_local(enc.lstm, x_k, order(st.memory[:, :, k * H:(k + 1) * H]), sfx)
        with torch.no_grad():
            act, c = rec.cell_scan(pre, st.lengths_dev)
            dg = rec.lstm_backward(getattr(enc.lstm, "weight_hh_l0" + sfx), act, c, order(d_memory[:, :, k * H:(k + 1) * H]).contiguous(),
                                   st.lengths_dev)
        ps = [getattr(enc.lstm, n + "_l0" + sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        gs = torch.autograd.grad(pre, [x_k] + ps, dg)
        d_x = d_x + order(gs[0])
        take(ps, gs[1:])
    ps = list(enc.prenet.parameters()) + list(enc.convolutions.parameters())
    take(ps, torch.autograd.grad(x, ps, d_x))
    st.launches = list(rec.launches) if hasattr(rec, "launches") else None
    missing = [n for n, p in model.named_parameters() if grads[id(p)] is None]
    if missing:
        raise _lib.FacppgError("backward pass produced no gradient for %s" % ", ".join(missing))
    return [grads[id(p)] for p in params], d_memory


class ForcedGraph(torch.autograd.Function):
    """The teacher-forced pass as one node: forward hands out what the HIP stages computed, backward is ``backward``."""

    @staticmethod
    def forward(ctx, model, st, *params):
        ctx.model, ctx.st = model, st
        mel, mel_post, gate, align = st.outputs
        ctx.mark_non_differentiable(align)
        return mel, mel_post, gate, align

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mel, g_post, g_gate, _g_align):
        model, st = ctx.model, ctx.st
        if not st.identity.unchanged():
            raise _lib.FacppgError("Tacotron2.forward(differentiable=True): the parameters changed between this forward call and "
                                   "its backward pass")
        grads, d_memory = backward(model, st, g_mel, g_post, g_gate)
        model.last_memory_grad = d_memory          # (for single-threaded callers: tests, tools)
        model.last_backward_launches = st.launches
        return (None, None) + tuple(g if p.requires_grad else None for g, p in zip(grads, model.parameters()))
