"""Tacotron2-style PPG -> mel model -- drop-in for src/common/model.py.

The module tree (names, parameter shapes, state-dict keys: SURVEY.md Appendix B) equals the
reference's so ``load_state_dict(torch.load(ckpt)['state_dict'])`` works unchanged
(generate_synthesis.py:82).  The modules hold parameters only; ``Tacotron2.inference`` packs
them once into a ``facppg_taco`` handle and runs the encoder GEMMs, the BiLSTM kernel, the
persistent decoder kernel and the postnet GEMMs of csrc/facppg_taco.hip through the C ABI;
``Tacotron2.forward`` is the teacher-forced pass (eval mode) on the padded-batch encoder, the
teacher-forced recurrent kernel and the same postnet; ``forward(..., differentiable=True)`` attaches that pass to the autograd
graph, its backward pass being common/taco_grad.py on the recurrent kernels of csrc/facppg_taco_bwd.hip.  There is no CPU
path, and training-mode semantics (batch-statistics BatchNorm, the training-mode dropouts) are not built.

Extensions over the reference signature (defaults reproduce it):
  ``inference(inputs, lengths=None, dropout_masks=None, seed=None)``
    lengths        valid PPG frames per utterance for a padded batch; every utterance is decoded
                   exactly as its own batch-1 run (the reference only supports batch 1,
                   model.py:524-528)
    dropout_masks  (enc [2, B, Tin, E], dec [steps, 2, B, prenet_dim]) keep-masks in {0,1} for the
                   prenets' always-on dropout (model.py:132-135); None -> drawn on the device
    utterance_seeds  B integers: the dropout draws of utterance b depend on utterance_seeds[b] alone, so the
                   batch reproduces B independent batch-1 calls with the same seeds (facppg_taco_draw_dropout)
    step_limits    B integers: utterance b stops after min(step_limits[b], max_decoder_steps) frames at the
                   latest (per-utterance max_decoder_steps of a padded batch)
"""
import collections

import torch
from torch import nn

from common.layers import ConvNorm, LinearNorm
from common.utils import get_mask_from_lengths, to_gpu
from facppg import lib as _lib

# One decoder launch as facppg_taco_decode reports it: mode 'single', 'coop' or 'split', its workgroups, and whether it published
# its frames to the call's frame consumer.
DecoderLaunch = collections.namedtuple("DecoderLaunch", "mode workgroups streamed step", defaults=(0,))


class InferenceOutputs(list):
    """What Tacotron2.inference returns: the reference's [mel, mel_post, gate, alignments], carrying what THIS call did --
    out_lengths (Tout per utterance, long, on the host) and launch (DecoderLaunch) -- so that calls on a shared model do not
    read each other's results."""

    def __init__(self, outputs, out_lengths, launch):
        super(InferenceOutputs, self).__init__(outputs)
        self.out_lengths, self.launch = out_lengths, launch


class LocationLayer(nn.Module):
    """model.py:44-60"""

    def __init__(self, attention_n_filters, attention_kernel_size, attention_dim):
        super(LocationLayer, self).__init__()
        self.location_conv = ConvNorm(2, attention_n_filters, kernel_size=attention_kernel_size,
                                      padding=(attention_kernel_size - 1) // 2, bias=False, stride=1, dilation=1)
        self.location_dense = LinearNorm(attention_n_filters, attention_dim, bias=False, w_init_gain='tanh')


class Attention(nn.Module):
    """model.py:63-121 (location-sensitive attention); evaluated inside k_decoder."""

    def __init__(self, attention_rnn_dim, embedding_dim, attention_dim, attention_location_n_filters,
                 attention_location_kernel_size):
        super(Attention, self).__init__()
        self.query_layer = LinearNorm(attention_rnn_dim, attention_dim, bias=False, w_init_gain='tanh')
        self.memory_layer = LinearNorm(embedding_dim, attention_dim, bias=False, w_init_gain='tanh')
        self.v = LinearNorm(attention_dim, 1, bias=False)
        self.location_layer = LocationLayer(attention_location_n_filters, attention_location_kernel_size, attention_dim)
        self.score_mask_value = -float("inf")
        self.not_so_small_mask = -1000


class Prenet(nn.Module):
    """model.py:124-135: bias-free Linear + ReLU + dropout(p=0.5, ALWAYS on) per layer."""

    def __init__(self, in_dim, sizes):
        super(Prenet, self).__init__()
        in_sizes = [in_dim] + sizes[:-1]
        self.layers = nn.ModuleList([LinearNorm(i, o, bias=False) for i, o in zip(in_sizes, sizes)])


class Postnet(nn.Module):
    """model.py:138-184: five 1-D convolutions (k=5) with BatchNorm, tanh on all but the last."""

    def __init__(self, hparams):
        super(Postnet, self).__init__()
        nf, pe, pk = hparams.n_acoustic_feat_dims, hparams.postnet_embedding_dim, hparams.postnet_kernel_size
        dims = [nf] + [pe] * (hparams.postnet_n_convolutions - 1) + [nf]
        self.convolutions = nn.ModuleList()
        for j in range(hparams.postnet_n_convolutions):
            last = j == hparams.postnet_n_convolutions - 1
            self.convolutions.append(nn.Sequential(
                ConvNorm(dims[j], dims[j + 1], kernel_size=pk, stride=1, padding=(pk - 1) // 2, dilation=1,
                         w_init_gain='linear' if last else 'tanh'),
                nn.BatchNorm1d(dims[j + 1])))


class Encoder(nn.Module):
    """model.py:187-249: prenet, conv bank (conv+BN+ReLU), bidirectional LSTM."""

    def __init__(self, hparams):
        super(Encoder, self).__init__()
        E = hparams.encoder_embedding_dim
        self.prenet = Prenet(hparams.n_symbols, [hparams.symbols_embedding_dim, hparams.symbols_embedding_dim])
        ks = hparams.encoder_kernel_size
        self.convolutions = nn.ModuleList([
            nn.Sequential(ConvNorm(E, E, kernel_size=ks, stride=1, padding=(ks - 1) // 2, dilation=1, w_init_gain='relu'),
                          nn.BatchNorm1d(E))
            for _ in range(hparams.encoder_n_convolutions)])
        self.lstm = nn.LSTM(E, E // 2, 1, batch_first=True, bidirectional=True)


class Decoder(nn.Module):
    """model.py:252-535"""

    def __init__(self, hparams):
        super(Decoder, self).__init__()
        self.n_acoustic_feat_dims = hparams.n_acoustic_feat_dims
        self.encoder_embedding_dim = hparams.encoder_embedding_dim
        self.attention_rnn_dim = hparams.attention_rnn_dim
        self.decoder_rnn_dim = hparams.decoder_rnn_dim
        self.prenet_dim = hparams.prenet_dim
        self.max_decoder_steps = hparams.max_decoder_steps
        self.gate_threshold = hparams.gate_threshold
        self.p_attention_dropout = hparams.p_attention_dropout
        self.p_decoder_dropout = hparams.p_decoder_dropout
        self.attention_window_size = hparams.attention_window_size
        self.prenet = Prenet(hparams.n_acoustic_feat_dims, [hparams.prenet_dim, hparams.prenet_dim])
        self.attention_rnn = nn.LSTMCell(hparams.prenet_dim + hparams.encoder_embedding_dim, hparams.attention_rnn_dim)
        self.attention_layer = Attention(hparams.attention_rnn_dim, hparams.encoder_embedding_dim, hparams.attention_dim,
                                         hparams.attention_location_n_filters, hparams.attention_location_kernel_size)
        self.decoder_rnn = nn.LSTMCell(hparams.attention_rnn_dim + hparams.encoder_embedding_dim, hparams.decoder_rnn_dim, 1)
        self.linear_projection = LinearNorm(hparams.decoder_rnn_dim + hparams.encoder_embedding_dim,
                                            hparams.n_acoustic_feat_dims)
        self.gate_layer = LinearNorm(hparams.decoder_rnn_dim + hparams.encoder_embedding_dim, 1, bias=True,
                                     w_init_gain='sigmoid')


class Tacotron2(nn.Module):
    """model.py:538-610"""

    def __init__(self, hparams):
        super(Tacotron2, self).__init__()
        self.mask_padding = hparams.mask_padding
        self.fp16_run = hparams.fp16_run
        self.n_acoustic_feat_dims = hparams.n_acoustic_feat_dims
        self.encoder = Encoder(hparams)
        self.decoder = Decoder(hparams)
        self.postnet = Postnet(hparams)
        self._hp = {k: getattr(hparams, k) for k in (
            "n_symbols", "symbols_embedding_dim", "encoder_kernel_size", "encoder_n_convolutions", "encoder_embedding_dim",
            "n_acoustic_feat_dims", "prenet_dim", "attention_rnn_dim", "decoder_rnn_dim", "attention_dim",
            "attention_location_n_filters", "attention_location_kernel_size", "attention_window_size",
            "postnet_embedding_dim", "postnet_kernel_size", "postnet_n_convolutions", "gate_threshold")}

    # ---------------------------------------------------------------- HIP handle
    def _config(self):
        c = _lib.TacoConfig()
        for k, v in self._hp.items():
            if k == "attention_window_size":
                v = -1 if v is None else int(v)
            setattr(c, k, v)
        c.gate_threshold = float(self.decoder.gate_threshold)
        c.bn_eps = float(self.postnet.convolutions[0][1].eps)
        return c

    def _flat_weights(self):
        """Plain weight blob in the order include/facppg.h documents."""
        sd = self.state_dict()
        keys = ["encoder.prenet.layers.0.linear_layer.weight", "encoder.prenet.layers.1.linear_layer.weight"]
        for j in range(len(self.encoder.convolutions)):
            p = "encoder.convolutions.%d." % j
            keys += [p + "0.conv.weight", p + "0.conv.bias", p + "1.weight", p + "1.bias", p + "1.running_mean", p + "1.running_var"]
        for sfx in ("", "_reverse"):
            keys += ["encoder.lstm.%s_l0%s" % (n, sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        keys += ["decoder.prenet.layers.0.linear_layer.weight", "decoder.prenet.layers.1.linear_layer.weight"]
        keys += ["decoder.attention_rnn." + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        a = "decoder.attention_layer."
        keys += [a + "query_layer.linear_layer.weight", a + "memory_layer.linear_layer.weight", a + "v.linear_layer.weight",
                 a + "location_layer.location_conv.conv.weight", a + "location_layer.location_dense.linear_layer.weight"]
        keys += ["decoder.decoder_rnn." + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        keys += ["decoder.linear_projection.linear_layer.weight", "decoder.linear_projection.linear_layer.bias",
                 "decoder.gate_layer.linear_layer.weight", "decoder.gate_layer.linear_layer.bias"]
        for j in range(len(self.postnet.convolutions)):
            p = "postnet.convolutions.%d." % j
            keys += [p + "0.conv.weight", p + "0.conv.bias", p + "1.weight", p + "1.bias", p + "1.running_mean", p + "1.running_var"]
        return torch.cat([sd[k].detach().float().reshape(-1) for k in keys])

    def _release(self):
        h = self.__dict__.pop("_facppg_handle", None)
        if h is not None:
            _lib.load().facppg_taco_destroy(h[0])

    def invalidate_packed_weights(self):
        self._release()

    def train(self, mode=True):
        self._release()
        return super(Tacotron2, self).train(mode)

    # CUs the decoder may occupy (facppg_taco_decode_opts.max_workgroups) unless a call says otherwise; 0 = the whole device.
    # facppg.pipeline.synthesize_stream bounds its own calls while the decoder runs under the previous batch's vocoder.
    decoder_workgroups = 0

    def _handle(self, dev):
        h = self.__dict__.get("_facppg_handle")
        if h is not None and h[1] == dev and h[2].unchanged():
            return h[0]
        self._release()
        L = _lib.load()
        cfg = self._config()
        blob = self._flat_weights().to(dev).contiguous()
        if blob.numel() != L.facppg_taco_weight_count(cfg):
            raise _lib.FacppgError("weight blob has %d values, library expects %d: %s" % (
                blob.numel(), L.facppg_taco_weight_count(cfg), L.facppg_last_error().decode()))
        out = _lib.ctypes.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(L.facppg_taco_create(cfg, _lib.ptr(blob), blob.numel(), dev.index, _lib.current_stream(dev),
                                            _lib.ctypes.byref(out)))
        self.__dict__["_facppg_handle"] = (out, dev, _lib.WeightIdentity(self))
        return out

    def last_decoder_launch(self):
        """(mode, workgroups) of the most recent decoder launch on this model: mode is 'single', 'coop' or 'split'.  For
        single-threaded callers (tests, tools); a caller that shares the model reads the ``launch`` of inference's result."""
        launch = self.__dict__.get("_last_launch")
        if launch is None:
            raise _lib.FacppgError("last_decoder_launch: no inference has run on this model yet")
        return launch.mode, launch.workgroups

    def _apply(self, fn, *a, **k):
        self._release()
        return super(Tacotron2, self)._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._release()
        return super(Tacotron2, self).load_state_dict(*a, **k)

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_facppg_handle", None)
        return d

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---------------------------------------------------------------- reference surface
    def parse_input(self, inputs):
        if self.fp16_run:
            raise _lib.FacppgError("fp16_run is not built (the reference's README.md:53 says FP16 does not work either)")
        return inputs

    def parse_batch(self, batch):
        """A collated batch (common.data_utils.ppg_acoustics_collate: ppg, input lengths, acoustic targets, gate targets, output
        lengths) -> (forward's inputs, the loss's targets), on the GPU: the features as float, the lengths as long
        (the reference's model.py:548-560).  forward's inputs carry the longest PPG length as a host integer in slot 3."""
        if len(batch) != 5:
            raise ValueError("parse_batch: a batch is (ppg, input_lengths, acoustic, gate, output_lengths), got %d items" % len(batch))
        ppg, in_lens, acoustic, gate, out_lens = (to_gpu(t).float() if k in (0, 2, 3) else to_gpu(t).long()
                                                  for k, t in enumerate(batch))
        return (ppg, in_lens, acoustic, int(in_lens.max()), out_lens), (acoustic, gate)

    def parse_output(self, outputs, output_lengths=None):
        """model.py:566-578: beyond each utterance's output length mel and mel_post become 0 and the gate energies 1e3 (when
        ``mask_padding``); the alignments stay as they are.  ``inference`` calls it without lengths."""
        if self.mask_padding and output_lengths is not None:
            pad = ~get_mask_from_lengths(output_lengths)                 # [B, T_out], True = padding
            outputs[0].masked_fill_(pad.unsqueeze(1), 0.0)
            outputs[1].masked_fill_(pad.unsqueeze(1), 0.0)
            outputs[2].masked_fill_(pad, 1e3)
        return outputs

    def forward(self, inputs, dropout_masks=None, seed=None, utterance_seeds=None, differentiable=False):
        """The teacher-forced pass (model.py:580-595) in eval mode, on the HIP kernels of csrc/facppg_taco.hip.
        inputs = (ppg_padded [B, n_symbols, Tin], input_lengths [B] descending, acoustic_padded [B, n_feat, T_out], max_len,
        output_lengths [B]) as ``parse_batch`` returns them -> [mel, mel_post, gate [B, T_out], alignments [B, T_out, Tin]].
        It reproduces the reference's PADDED-BATCH computation (facppg_taco_encode_padded, facppg_taco_postnet without lengths):
        the encoder's conv bank and the postnet run over the zero-padded batch, so an utterance's result depends on how far
        its batch is padded -- what the checkpoints were trained with and what makes a validation loss comparable.
        dropout_masks  (enc [2, B, Tin, E], dec [2, T_out + 1, B, prenet_dim]) keep-masks in the reference's draw order (it draws
                       T_out + 1 decoder frames and uses the first T_out); None -> drawn on the device from ``seed``
        utterance_seeds  B integers, as in ``inference``: utterance b's dropout draws depend on utterance_seeds[b] alone
        differentiable   per call, not model state.  False: the outputs are detached and nothing is kept, whatever the grad mode.
                       True (eval mode, gradients enabled, at least one parameter requiring a gradient -- anything else
                       raises): the same values, bit for bit, attached to the autograd graph; ``backward()`` leaves the
                       gradients of this eval-mode function -- running-statistics BatchNorm, the prenet dropouts under the
                       masks of this call, padded-batch semantics -- in all 61 parameter tensors.  ``alignments`` is not
                       differentiable, and no gradient is produced for the PPG or the targets.
        B = 1 works (the reference's own forward fails there on a squeeze(), model.py:481).  Training mode raises: the backward
        pass is not built for ITS semantics (batch-statistics BatchNorm, the 0.5 / 0.1 training-mode dropouts)."""
        if self.training:
            raise _lib.FacppgError("Tacotron2.forward in training mode: the backward pass is not built for training-mode semantics "
                                   "(batch-statistics BatchNorm, the training-mode dropouts) -- call model.eval(); "
                                   "forward(..., differentiable=True) gives the gradients of the eval-mode pass")
        if differentiable:
            if not torch.is_grad_enabled():
                raise _lib.FacppgError("Tacotron2.forward(differentiable=True) under torch.no_grad(): nothing could be attached to a graph")
            if not any(p.requires_grad for p in self.parameters()):
                raise _lib.FacppgError("Tacotron2.forward(differentiable=True): no parameter requires a gradient")
        ppg, input_lengths, targets, _max_len, output_lengths = self.parse_input(inputs)
        _lib.require_cuda(ppg, "Tacotron2.forward: inputs")
        _lib.require_cuda(targets, "Tacotron2.forward: targets")
        L = _lib.load()
        dev = ppg.device
        hp = self._hp
        x = ppg.float().contiguous()
        tgt = targets.to(dev).float().contiguous()
        B, S, Tin = x.shape
        E, P, NF, AD = hp["encoder_embedding_dim"], hp["prenet_dim"], hp["n_acoustic_feat_dims"], hp["attention_dim"]
        if S != hp["n_symbols"]:
            raise _lib.FacppgError("inputs have %d symbols, model was built for %d" % (S, hp["n_symbols"]))
        if tgt.dim() != 3 or tgt.shape[0] != B or tgt.shape[1] != NF or tgt.shape[2] < 1:
            raise _lib.FacppgError("targets must be [B, %d, T_out], got %s" % (NF, tuple(tgt.shape)))
        T = tgt.shape[2]
        lens_host = torch.as_tensor(input_lengths).detach().to("cpu", torch.int32).contiguous()
        out_lens = torch.as_tensor(output_lengths).to(dev).long()
        if lens_host.numel() != B or out_lens.numel() != B:
            raise _lib.FacppgError("input_lengths and output_lengths must hold B values")
        if int(lens_host.max()) != Tin:
            raise _lib.FacppgError("the longest utterance has %d frames, the padded batch %d (model.py:232-233 pads to the longest)"
                                   % (int(lens_host.max()), Tin))
        if int(out_lens.max()) != T:
            raise _lib.FacppgError("the longest target has %d frames, the padded targets %d" % (int(out_lens.max()), T))
        lt = lens_host.to(dev)
        h = self._handle(dev)
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        seed &= 0xFFFFFFFFFFFFFFFF
        enc_m = dec_m = None
        st = _lib.current_stream(dev)
        if dropout_masks is not None:
            if utterance_seeds is not None:
                raise _lib.FacppgError("utterance_seeds: B integers, and not together with dropout_masks")
            em, dm = dropout_masks
            enc_m = torch.as_tensor(em).to(dev).to(torch.uint8).reshape(2, B, Tin, E).permute(0, 1, 3, 2).contiguous()
            dm = torch.as_tensor(dm).to(dev).to(torch.uint8)
            if tuple(dm.shape) != (2, T + 1, B, P):
                raise _lib.FacppgError("decoder masks must be [2, T_out + 1, B, prenet_dim]")
            dec_m = dm[:, :T].permute(0, 2, 3, 1).contiguous()               # [2, B, P, T_out]
        elif utterance_seeds is not None:
            if len(utterance_seeds) != B:
                raise _lib.FacppgError("utterance_seeds: B integers, and not together with dropout_masks")
            enc_m, _ = self.draw_dropout_masks(utterance_seeds, Tin, dev, 1)
            sd = torch.tensor([int(v) & 0x7FFFFFFFFFFFFFFF for v in utterance_seeds], dtype=torch.int64, device=dev)
            dec_m = torch.empty(2, B, P, T, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L.facppg_taco_draw_dropout_forced(h, _lib.ptr(sd), B, T, _lib.ptr(dec_m), st))
        ws = torch.empty(max(L.facppg_taco_workspace_bytes(h, B, Tin), L.facppg_taco_decode_forced_workspace_bytes(h, B, T),
                             L.facppg_taco_postnet_workspace_bytes(h, B, T)), dtype=torch.uint8, device=dev)
        memory = torch.empty(B, Tin, E, dtype=torch.float32, device=dev)
        pm = torch.empty(B, AD, Tin, dtype=torch.float32, device=dev)
        mel = torch.empty(B, NF, T, dtype=torch.float32, device=dev)
        mel_post = torch.empty_like(mel)
        gate = torch.empty(B, T, dtype=torch.float32, device=dev)
        align = torch.empty(B, T, Tin, dtype=torch.float32, device=dev)
        opts = _lib.TacoDecodeOpts(max_workgroups=int(self.decoder_workgroups))
        with torch.cuda.device(dev):
            _lib.check(L.facppg_taco_encode_padded(h, _lib.ptr(x), _lib.ptr(lt), _lib.ctypes.c_void_p(lens_host.data_ptr()),
                                                   _lib.ptr(enc_m), seed, B, Tin, _lib.ptr(memory), _lib.ptr(pm), _lib.ptr(ws),
                                                   ws.numel(), st))
            if differentiable and enc_m is None:      # the masks the encoder drew from the seed, before its workspace is reused
                enc_m = torch.empty(2, B, hp["symbols_embedding_dim"], Tin, dtype=torch.uint8, device=dev)
                _lib.check(L.facppg_taco_encode_state(h, _lib.ptr(ws), ws.numel(), B, Tin, _lib.ptr(enc_m), st))
            _lib.check(L.facppg_taco_decode_forced(h, _lib.ptr(memory), _lib.ptr(pm), _lib.ptr(lt), _lib.ptr(tgt), _lib.ptr(dec_m),
                                                   seed, B, Tin, T, _lib.ptr(mel), _lib.ptr(gate), _lib.ptr(align), _lib.ptr(ws),
                                                   ws.numel(), _lib.ctypes.byref(opts), st))
            if differentiable:                        # the LSTMCells' hidden states of every frame, out of the exchange words
                ah = torch.empty(B, T, hp["attention_rnn_dim"], dtype=torch.float32, device=dev)
                dh = torch.empty(B, T, hp["decoder_rnn_dim"], dtype=torch.float32, device=dev)
                drawn = torch.empty(2, B, P, T, dtype=torch.uint8, device=dev) if dec_m is None else None
                _lib.check(L.facppg_taco_decode_forced_state(h, _lib.ptr(ws), ws.numel(), B, T, _lib.ptr(ah), _lib.ptr(dh),
                                                             _lib.ptr(drawn), st))
                dec_m = drawn if dec_m is None else dec_m
            _lib.check(L.facppg_taco_postnet(h, _lib.ptr(mel), None, B, T, T, _lib.ptr(mel_post), _lib.ptr(ws), ws.numel(), st))
        # (for single-threaded callers: tests, tools)
        self.last_memory, self._last_launch = memory, DecoderLaunch("coop", opts.workgroups, False)
        if not differentiable:
            return self.parse_output([mel, mel_post, gate, align], out_lens)
        from common import taco_grad
        s = taco_grad.ForcedState()
        s.ppg, s.lengths, s.lengths_dev, s.targets, s.enc_masks, s.dec_masks = x, lens_host, lt, tgt, enc_m, dec_m
        s.memory, s.mel, s.align, s.ah, s.dh = memory, mel, align, ah, dh
        masking = self.mask_padding and out_lens is not None
        s.pad = ~get_mask_from_lengths(out_lens) if masking else None
        s.identity = self.__dict__["_facppg_handle"][2]
        s.outputs, s.launches = (mel.clone(), mel_post, gate, align.clone()), None
        outs = list(taco_grad.ForcedGraph.apply(self, s, *self.parameters()))
        s.outputs = None
        if masking:                                   # parse_output's masking as graph operations: the same values
            outs = [outs[0].masked_fill(s.pad.unsqueeze(1), 0.0), outs[1].masked_fill(s.pad.unsqueeze(1), 0.0),
                    outs[2].masked_fill(s.pad, 1e3), outs[3]]
        return outs

    def draw_dropout_masks(self, utterance_seeds, Tin, device=None, steps=None):
        """Per-utterance dropout keep-masks (facppg_taco_draw_dropout) in the DEVICE layouts the kernels read:
        (enc uint8 [2, B, symbols_embedding_dim, Tin], dec uint8 [max_decoder_steps, 2, B, prenet_dim]).  Mask bits of
        utterance b depend on utterance_seeds[b] only (not on B or Tin).  For ``inference(dropout_masks=...)``,
        which takes the reference-shaped [2, B, Tin, E] encoder masks, pass ``enc.permute(0, 1, 3, 2)``."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        L = _lib.load()
        h = self._handle(dev)
        B, steps = len(utterance_seeds), int(self.decoder.max_decoder_steps if steps is None else steps)
        sd = torch.tensor([int(v) & 0x7FFFFFFFFFFFFFFF for v in utterance_seeds], dtype=torch.int64, device=dev)
        enc_m = torch.empty(2, B, self._hp["symbols_embedding_dim"], Tin, dtype=torch.uint8, device=dev)
        dec_m = torch.empty(steps, 2, B, self._hp["prenet_dim"], dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.facppg_taco_draw_dropout(h, _lib.ptr(sd), B, Tin, steps, _lib.ptr(enc_m), _lib.ptr(dec_m),
                                                  _lib.current_stream(dev)))
        return enc_m, dec_m

    def inference(self, inputs, lengths=None, dropout_masks=None, seed=None, utterance_seeds=None, step_limits=None, timer=None,
                  while_decoding=None, frame_consumer=None, decoder_workgroups=None, frame_consumer_arithmetic=None):
        """inputs [B, n_symbols, Tin] (GPU fp32) -> [mel, mel_post, gate, alignments]
        = [B,80,Tout], [B,80,Tout], [B,Tout,1], [B,Tout,Tin]  (model.py:597-610).  For B > 1 the
        outputs are zero beyond each utterance's own Tout, kept in the result's ``out_lengths`` (InferenceOutputs).
        Everything the call needs goes in as an argument and what it did comes back with the result: concurrent calls on one
        model do not see each other's settings or results.
        decoder_workgroups: the CUs the decoder may occupy (None: the model's ``decoder_workgroups``).
        while_decoding: optional callable run on the host after the decoder has been enqueued and before its output lengths
        are read back (facppg.pipeline checks the vocoder's packed weights there: ~0.4 ms that would otherwise sit between the
        acoustic model and the vocoder with the GPU idle).
        frame_consumer: optional (B = 1; facppg.pipeline.ConditioningStream): the split decoder publishes every mel frame the
        moment it exists and the consumer runs the postnet -- and whatever else it wants of the frames -- on a second stream
        WHILE the decoder is still running; mel_post is then the consumer's (the same values bit for bit).
        frame_consumer_arithmetic: handed to the consumer's begin() when not None (the vocoder arithmetic of this utterance)."""
        inputs = self.parse_input(inputs)
        _lib.require_cuda(inputs, "Tacotron2.inference: inputs")
        L = _lib.load()
        dev = inputs.device
        x = inputs.float().contiguous()
        B, D, Tin = x.shape
        hp = self._hp
        if D != hp["n_symbols"]:
            raise _lib.FacppgError("inputs have %d symbols, model was built for %d" % (D, hp["n_symbols"]))
        h = self._handle(dev)
        lt = None
        if lengths is not None:
            lt = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
            if lt.numel() != B or int(lt.max()) > Tin or int(lt.min()) < 1:
                raise _lib.FacppgError("lengths must be B values in [1, Tin]")
        if seed is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        seed &= 0xFFFFFFFFFFFFFFFF
        enc_m = dec_m = None
        steps = int(self.decoder.max_decoder_steps)
        sl = None
        if step_limits is not None:
            sl = torch.as_tensor(step_limits).to(dtype=torch.int32)
            if sl.numel() != B or int(sl.min()) < 1:
                raise _lib.FacppgError("step_limits must be B values >= 1")
            steps = min(steps, int(sl.max()))          # no utterance can run longer: size the outputs for that
            sl = sl.to(dev).contiguous()
        E, P, NF, AD = hp["encoder_embedding_dim"], hp["prenet_dim"], hp["n_acoustic_feat_dims"], hp["attention_dim"]
        if dropout_masks is not None:
            em, dm = dropout_masks
            enc_m = torch.as_tensor(em).to(dev).to(torch.uint8).reshape(2, B, Tin, E).permute(0, 1, 3, 2).contiguous()
            dec_m = torch.as_tensor(dm).to(dev).to(torch.uint8).contiguous()
            if dec_m.numel() != steps * 2 * B * P:
                raise _lib.FacppgError("decoder masks must be [max_decoder_steps, 2, B, prenet_dim]")
        st = _lib.current_stream(dev)
        if utterance_seeds is not None:
            if dropout_masks is not None or len(utterance_seeds) != B:
                raise _lib.FacppgError("utterance_seeds: B integers, and not together with dropout_masks")
            enc_m, dec_m = self.draw_dropout_masks(utterance_seeds, Tin, dev, steps)
        ws = torch.empty(max(L.facppg_taco_workspace_bytes(h, B, Tin), L.facppg_taco_decode_workspace_bytes(h, B, steps)),
                         dtype=torch.uint8, device=dev)
        # the six zero-initialised outputs as views of ONE zeroed allocation: one fill launch instead of six (each tiny launch
        # costs the stream ~8 us of kernel boundary, and they sit in front of the encoder on the latency path)
        sizes = (B * Tin * E, B * Tin * AD, B * NF * steps, B * steps, B * steps * Tin, B)
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 63) // 64 * 64                      # 256-byte aligned pieces
        arena = torch.zeros(tot, dtype=torch.float32, device=dev)
        memory = arena[offs[0]:offs[0] + sizes[0]].view(B, Tin, E)
        pm = arena[offs[1]:offs[1] + sizes[1]].view(B, Tin, AD)
        mel = arena[offs[2]:offs[2] + sizes[2]].view(B, NF, steps)
        gate = arena[offs[3]:offs[3] + sizes[3]].view(B, steps)
        align = arena[offs[4]:offs[4] + sizes[4]].view(B, steps, Tin)
        out_len = arena[offs[5]:offs[5] + sizes[5]].view(torch.int32)
        opts = _lib.TacoDecodeOpts(max_workgroups=int(self.decoder_workgroups if decoder_workgroups is None else decoder_workgroups))
        if frame_consumer is not None and B == 1:
            kind = {} if frame_consumer_arithmetic is None else {"arithmetic": frame_consumer_arithmetic}
            words = frame_consumer.begin(self, h, dev, steps, Tin, **kind)   # (zeroed on this stream, ahead of the decoder launch)
            if words is not None:
                opts.frame_words_dev, opts.frame_words_frames = words.data_ptr(), steps
        with torch.cuda.device(dev):
            _lib.check(L.facppg_taco_encode(h, _lib.ptr(x), _lib.ptr(lt), _lib.ptr(enc_m), seed, B, Tin, _lib.ptr(memory),
                                            _lib.ptr(pm), _lib.ptr(ws), ws.numel(), st))
            if timer is not None:
                timer.mark("encoder")
            _lib.check(L.facppg_taco_decode(h, _lib.ptr(memory), _lib.ptr(pm), _lib.ptr(lt), _lib.ptr(sl), _lib.ptr(dec_m), seed, B, Tin,
                                            steps, _lib.ptr(mel), _lib.ptr(gate), _lib.ptr(align), _lib.ptr(out_len),
                                            _lib.ptr(ws), ws.numel(), _lib.ctypes.byref(opts), st))
            launch = DecoderLaunch(("single", "coop", "split")[opts.mode], opts.workgroups, bool(opts.streamed), int(opts.step))
            if frame_consumer is not None and B == 1:
                if launch.streamed:
                    frame_consumer.enqueue(out_len, launch.workgroups)   # its launches, gated on the frames, on its own stream
                else:
                    frame_consumer.cancel()
            if while_decoding is not None:                     # host work that needs no result of the decoder: the GPU is busy for
                while_decoding()                               # milliseconds, the host would only sit in the read below
            out_len_host = out_len.cpu()                       # the path's single device->host sync
            if timer is not None:
                timer.mark("decoder")
            Tout = int(out_len_host.max())
            if Tout == int(self.decoder.max_decoder_steps):
                print("Warning! Reached max decoder steps")     # model.py:527
            mel_post = frame_consumer.finish(Tout, out_len) if launch.streamed else None   # [1, NF, >= Tout] view: what is left of the postnet
            if mel_post is None:
                mel_post = torch.zeros_like(mel)
                ws2 = torch.empty(L.facppg_taco_postnet_workspace_bytes(h, B, Tout), dtype=torch.uint8, device=dev)
                _lib.check(L.facppg_taco_postnet(h, _lib.ptr(mel), _lib.ptr(out_len), B, Tout, steps, _lib.ptr(mel_post),
                                                 _lib.ptr(ws2), ws2.numel(), st))
            if timer is not None:
                timer.mark("postnet")
        out_lengths = out_len_host.to(torch.long)
        # (for single-threaded callers: tests, tools)
        self.last_output_lengths, self.last_memory, self._last_launch = out_lengths, memory, launch
        return InferenceOutputs(self.parse_output([mel[:, :, :Tout], mel_post[:, :, :Tout], gate[:, :Tout].unsqueeze(-1),
                                                   align[:, :Tout]]), out_lengths, launch)
