"""PPG extraction -- the part of src/ppg/compute_ppg.py that needs no acoustic-model blob, on libfacppg_hip:

  DependenciesPPG          loads the LDA matrix (data/feats/final.mat), the pdf -> monophone reduction
                           (data/feats/reduce_dim.mat) and the splice options; the nnet3 model (data/am/final.raw) is NOT
                           shipped by the reference: ``nnet`` is None when the file is absent
  compute_feat_for_nnet[_internal]   wav -> MFCC -> CMN -> splice -> LDA, the acoustic model's input (compute_ppg.py:97-158)
  reduce_ppg_dim           full (senone) PPG [T, 5816] -> monophone PPG [T, 40] (compute_ppg.py:73-94)
  compute_full_ppg         nnet3 TDNN inference on the exact-fp32 MFMA GEMM (csrc/facppg_tdnn.hip): acoustic-model input
                           features [T, 40] -> senone posteriors [T, K] (compute_ppg.py:42-70).  The model is read by
                           common.decode.read_nnet3_model / common.nnet3 -- PARITY UNPINNED: the reference ships neither
                           the model (data/am/final.raw) nor anything Kaldi computed from it
  compute_feat_for_nnet_batch, compute_full_ppg_batch, compute_ppg_batch
                           the same chain for a LIST of utterances in one pass: the utterances are laid end to end, every
                           TDNN layer is one GEMM over all of them (facppg_tdnn_forward_batch), and the monophone
                           reduction is fused into the output kernel (facppg_tdnn_forward_batch_reduced)
  compute_ppg_padded       the batch chain again, the posteriors left on the device as the padded channel-major batch
                           [B, D, Tmax] that Tacotron2.inference reads (facppg_tdnn_forward_batch_padded): wav in, wav out
                           without the PPGs visiting the host (facppg.pipeline.synthesize_wavs); with ``append_f0`` the log F0
                           of ppg.compute_f0's track and its two deltas in three more rows (hparams.is_append_f0)

Matrices are float32 GPU tensors; file paths default to ``<repo data dir>/...`` like the reference's module constants and
can be overridden (FACPPG_DATA_DIR, or the constructor arguments)."""
import logging
import os
import re

import numpy as np
import torch

from common import decode, feat, kaldi_io, nnet3
from facppg import lib as _lib
from ppg.compute_f0 import F0Options, f0_flat, lf0_rows_padded

DATA_DIR = os.environ.get("FACPPG_DATA_DIR", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "data"))
NNET_PATH = os.path.join(DATA_DIR, 'am', 'final.raw')
LDA_PATH = os.path.join(DATA_DIR, 'feats', 'final.mat')
REDUCE_DIM_PATH = os.path.join(DATA_DIR, 'feats', 'reduce_dim.mat')
SPLICE_OPTS_PATH = os.path.join(DATA_DIR, 'feats', 'splice_opts')


class _TdnnHandle(object):
    """The packed HIP form of one nnet3 model on one device (kept on the Nnet object)."""

    def __init__(self, nnet, dev):
        L = _lib.load()
        layers, final = nnet3.plan_layers(nnet)
        table = (_lib.TdnnLayer * len(layers))()
        blob = []
        for i, l in enumerate(layers):
            out_dim, k = l["W"].shape
            table[i].out_dim, table[i].in_dim, table[i].taps = out_dim, k // l["taps"], l["taps"]
            table[i].dil, table[i].first, table[i].relu = l["dil"], l["first"], int(l["act"] == "relu")
            table[i].renorm_target_rms = float(l["renorm"] or 0.0)
            blob += [l["W"].reshape(-1), l["b"].reshape(-1)]
        flat = torch.from_numpy(np.concatenate(blob).astype(np.float32)).to(dev)
        self.handle = _lib.ctypes.c_void_p()
        self.dev, self.out_dim, self.in_dim = dev, layers[-1]["W"].shape[0], layers[0]["W"].shape[1] // layers[0]["taps"]
        with torch.cuda.device(dev):
            _lib.check(L.facppg_tdnn_create(table, len(layers), {"none": 0, "softmax": 1, "log-softmax": 2}[final], _lib.ptr(flat),
                                            flat.numel(), dev.index, _lib.current_stream(dev), _lib.ctypes.byref(self.handle)))

    def __del__(self):
        try:
            _lib.load().facppg_tdnn_destroy(self.handle)
        except Exception:
            pass


def compute_full_ppg(nnet, feats):
    """compute_ppg.py:42-70: nnet (common.nnet3.Nnet) x feats [T, D] (GPU tensor or numpy) -> raw PPGs [T, K] on the GPU,
    K = number of senones.  Batch-norm in test mode, frames beyond the utterance = the edge frames repeated, acoustic
    scale 1, no priors -- what the reference configures on DecodableNnetSimple."""
    if nnet is None:
        raise _lib.FacppgError("compute_full_ppg: no acoustic model -- the reference does not ship data/am/final.raw; pass a model read "
                               "with common.decode.read_nnet3_model, or use precomputed PPGs (common.data_utils.get_ppg)")
    L = _lib.load()
    feats = torch.as_tensor(feats)
    if not feats.is_cuda:
        feats = feats.cuda()
    feats = feats.float().contiguous()
    dev = feats.device
    h = getattr(nnet, "_facppg_tdnn", None)
    if h is None or h.dev != dev:
        h = nnet._facppg_tdnn = _TdnnHandle(nnet, dev)
    T, D = feats.shape
    if D != h.in_dim:
        raise _lib.FacppgError("compute_full_ppg: features have %d dims, the model's input node has %d" % (D, h.in_dim))
    out = torch.empty(T, h.out_dim, device=dev)
    ws = torch.empty(L.facppg_tdnn_workspace_bytes(h.handle, T), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_tdnn_forward(h.handle, _lib.ptr(feats), T, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    return out


def _require_model(nnet, what):
    if nnet is None:
        raise _lib.FacppgError("%s: no acoustic model -- the reference does not ship data/am/final.raw; pass a model read "
                               "with common.decode.read_nnet3_model, or use precomputed PPGs (common.data_utils.get_ppg)" % what)


def _tdnn_handle(nnet, dev, what):
    _require_model(nnet, what)
    h = getattr(nnet, "_facppg_tdnn", None)
    if h is None or h.dev != dev:
        h = nnet._facppg_tdnn = _TdnnHandle(nnet, dev)
    return h


def _full_ppg_flat(nnet, feats, frames, transform=None):
    """feats [sum T, D] (GPU, the utterances laid end to end) x frame counts -> [sum T, K] posteriors, or with ``transform``
    ([d, K], read_sparse_mat) the [sum T, d] monophone PPGs from the fused output kernel."""
    L = _lib.load()
    dev = feats.device
    h = _tdnn_handle(nnet, dev, "compute_full_ppg_batch")
    T, D = feats.shape
    if D != h.in_dim:
        raise _lib.FacppgError("compute_full_ppg_batch: features have %d dims, the model's input node has %d" % (D, h.in_dim))
    off = _lib.host_offsets(frames)
    if off[-1] != T:
        raise ValueError("compute_full_ppg_batch: the frame counts add up to %d, the matrix has %d rows" % (off[-1], T))
    B = len(frames)
    nbytes = L.facppg_tdnn_batch_workspace_bytes(h.handle, off, B)
    if nbytes == 0:
        _lib.check(-1)
    off_dev = _lib.upload(list(off), torch.int32, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        if transform is None:
            out = torch.empty(T, h.out_dim, device=dev)
            _lib.check(L.facppg_tdnn_forward_batch(h.handle, _lib.ptr(feats), _lib.ptr(off_dev), off, B, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                   _lib.current_stream(dev)))
        else:
            tr_t = torch.as_tensor(transform).to(dev).float().t().contiguous()            # [K, d]
            if tr_t.shape[0] != h.out_dim:
                raise _lib.FacppgError("reduce_ppg_dim: PPG has %d dims, the transform expects %d" % (h.out_dim, tr_t.shape[0]))
            out = torch.empty(T, tr_t.shape[1], device=dev)
            _lib.check(L.facppg_tdnn_forward_batch_reduced(h.handle, _lib.ptr(feats), _lib.ptr(off_dev), off, B, _lib.ptr(tr_t), tr_t.shape[1],
                                                           _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    return out


def _split(flat, frames):
    """[sum T, K] -> the B utterances' [T_b, K] (views of the one buffer)."""
    out, at = [], 0
    for n in frames:
        out.append(flat[at:at + n])
        at += n
    return out


def compute_full_ppg_batch(nnet, feats_list, transform=None):
    """compute_full_ppg (compute_ppg.py:42-70) for a list of feature matrices [T_b, D] (GPU tensors or numpy) in ONE pass ->
    list of [T_b, K] GPU tensors.  With ``transform`` (the pdf -> monophone matrix [d, K]) the list holds the [T_b, d]
    monophone PPGs instead, reduced inside the output kernel (the model's output must be a softmax)."""
    _require_model(nnet, "compute_full_ppg_batch")
    if not len(feats_list):
        raise ValueError("compute_full_ppg_batch: no utterance")
    mats = []
    for f in feats_list:
        f = torch.as_tensor(f)
        mats.append((f if f.is_cuda else f.cuda()).float())
    frames = [int(m.shape[0]) for m in mats]
    flat = mats[0].contiguous() if len(mats) == 1 else torch.cat(mats, 0)
    return _split(_full_ppg_flat(nnet, flat, frames, transform), frames)


def reduce_ppg_dim(ppgs, transform):
    """ppgs [T, D] (GPU tensor or numpy) x transform [d, D] (dense; read_sparse_mat) -> [T, d] on the GPU."""
    L = _lib.load()
    ppgs = torch.as_tensor(ppgs)
    if not ppgs.is_cuda:
        ppgs = ppgs.cuda()
    ppgs = ppgs.float().contiguous()
    dev = ppgs.device
    tr_t = torch.as_tensor(transform).to(dev).float().t().contiguous()            # [D, d]
    T, D = ppgs.shape
    if tr_t.shape[0] != D:
        raise _lib.FacppgError("reduce_ppg_dim: PPG has %d dims, the transform expects %d" % (D, tr_t.shape[0]))
    out = torch.empty(T, tr_t.shape[1], device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_reduce_ppg(_lib.ptr(ppgs), _lib.ptr(tr_t), T, D, tr_t.shape[1], _lib.ptr(out), _lib.current_stream(dev)))
    return out


def compute_feat_for_nnet_internal(wav, lda, **kwargs):
    """compute_ppg.py:97-134, same options and defaults."""
    options = {"is_use_energy": False, "is_downsample": True, "frame_shift": 10, "is_snip_edges": False, "left_context": 3,
               "right_context": 3}
    for key, val in kwargs.items():
        if key in options:
            options[key] = val
        else:
            logging.error("Option %s not allowed!" % (key))
    mfcc_opts = feat.MfccOptions()
    mfcc_opts.use_energy = options["is_use_energy"]
    mfcc_opts.frame_opts.allow_downsample = options["is_downsample"]
    mfcc_opts.frame_opts.frame_shift_ms = options["frame_shift"]
    mfcc_opts.frame_opts.snip_edges = options["is_snip_edges"]
    mfccs = feat.compute_mfcc_feats(wav, mfcc_opts)
    return feat.cmn_splice_transform(mfccs, options["left_context"], options["right_context"], lda)


def _mfcc_options(options):
    mfcc_opts = feat.MfccOptions()
    mfcc_opts.use_energy = options["is_use_energy"]
    mfcc_opts.frame_opts.allow_downsample = options["is_downsample"]
    mfcc_opts.frame_opts.frame_shift_ms = options["frame_shift"]
    mfcc_opts.frame_opts.snip_edges = options["is_snip_edges"]
    return mfcc_opts


def _feat_for_nnet_flat(wavs, lda, keep_tables=False, samples=None, **kwargs):
    options = {"is_use_energy": False, "is_downsample": True, "frame_shift": 10, "is_snip_edges": False, "left_context": 3,
               "right_context": 3}
    for key, val in kwargs.items():
        if key in options:
            options[key] = val
        else:
            logging.error("Option %s not allowed!" % (key))
    mfccs, frames = feat.compute_mfcc_feats_batch(wavs, _mfcc_options(options), keep_tables=keep_tables, samples=samples)
    return feat.cmn_splice_transform_batch(mfccs, frames, options["left_context"], options["right_context"], lda), frames


def compute_feat_for_nnet_batch(wavs, lda, **options):
    """compute_feat_for_nnet_internal (compute_ppg.py:97-134, same options and defaults) for a list of WaveData in one pass
    -> list of [T_b, 40] GPU tensors, each equal to the single call's bit for bit."""
    flat, frames = _feat_for_nnet_flat(wavs, lda, **options)
    return _split(flat, frames)


def compute_ppg_batch(wavs, deps, is_full_ppg=True, shift=10):
    """compute_full_ppg_wrapper / compute_monophone_ppg (compute_ppg.py:161-202) for a list of WaveData in one pass: wav ->
    features -> acoustic model -> list of GPU tensors [T_b, K]: the senone posteriors, or with ``is_full_ppg=False`` the
    monophone PPGs through ``deps.monophone_trans``."""
    _require_model(deps.nnet, "compute_ppg_batch")
    flat, frames = _feat_for_nnet_flat(wavs, deps.lda, frame_shift=shift)
    if is_full_ppg:
        return _split(_full_ppg_flat(deps.nnet, flat, frames), frames)
    if deps.monophone_trans is None:
        raise _lib.FacppgError("compute_ppg_batch: monophone PPGs need the pdf -> monophone matrix (data/feats/reduce_dim.mat)")
    if nnet3.plan_layers(deps.nnet)[1] != "softmax":      # the fused kernel reduces posteriors: other outputs go the long way
        return [reduce_ppg_dim(p, deps.monophone_trans) for p in _split(_full_ppg_flat(deps.nnet, flat, frames), frames)]
    return _split(_full_ppg_flat(deps.nnet, flat, frames, deps.monophone_trans), frames)


def padded_ppg_dim(deps, is_full_ppg):
    """Channels of compute_ppg_padded's result: the model's senones, or the rows of the pdf -> monophone matrix.  Raises
    compute_ppg_padded's refusals (host work only)."""
    _require_model(deps.nnet, "compute_ppg_padded")
    kept = getattr(deps.nnet, "_facppg_output", None)      # (planning the layers folds every weight matrix: milliseconds of host time)
    if kept is None:
        layers, final = nnet3.plan_layers(deps.nnet)
        kept = deps.nnet._facppg_output = (final, int(layers[-1]["W"].shape[0]))
    final, out_dim = kept
    if not is_full_ppg and deps.monophone_trans is None:
        raise _lib.FacppgError("compute_ppg_padded: monophone PPGs need the pdf -> monophone matrix (data/feats/reduce_dim.mat)")
    if final != "softmax":
        raise _lib.FacppgError("compute_ppg_padded: the padded layout holds posteriors: the model's output must be a softmax (it is %s)" % final)
    return out_dim if is_full_ppg else int(deps.monophone_trans.shape[0])


def _on_device(deps, name, dev, transposed=False):
    """deps.<name> as a float32 matrix on ``dev`` (transposed: [K, d], what the output kernel reads), kept with the dependencies:
    an upload from pageable memory waits for the stream."""
    cache = deps.__dict__.setdefault("_facppg_on_device", {})
    src = getattr(deps, name)
    hit = cache.get((name, dev))
    if hit is None or hit[0] is not src:
        t = torch.as_tensor(src).to(dev).float()
        hit = cache[(name, dev)] = (src, t.t().contiguous() if transposed else t.contiguous())
    return hit[1]


def compute_ppg_padded(wavs, deps, is_full_ppg=True, shift=10, append_f0=False, f0_options=None):
    """compute_ppg_batch for a consumer on the device: list of WaveData -> (x [B, D, Tmax] float32 on the GPU, lengths [B] on
    the host), the batch Tacotron2.inference reads -- channel-major, frames contiguous, exactly 0 behind each utterance's
    T_b frames (facppg_tdnn_forward_batch_padded writes every element: nothing is zeroed here).  D = the model's senones, or
    with ``is_full_ppg=False`` the monophone classes of ``deps.monophone_trans`` (bit for bit compute_ppg_batch's values).  The
    feature pass is compute_ppg_batch's; the frame counts come from the sample counts on the host: the call copies nothing
    back from the device and does not wait for it (from the second call on a device on: the first one packs the model and
    uploads the feature tables and matrices, which stay).  The model's output must be a softmax.

    Kept between calls, tables and never results: the model's output kind and width (``nnet._facppg_output``, next to its packed
    handle and like it for the life of the model object), the device copies of ``deps.lda`` / ``deps.monophone_trans``
    (``deps._facppg_on_device``, replaced when the attribute is bound to another object) and one Mfcc per set of option values
    (common.feat._KEPT_MFCC, for the life of the process: a few hundred KB each).  A model or matrix is a loaded file here; one
    that is changed IN PLACE after the first call is not seen -- bind a new object, or delete the attribute named above.

    append_f0: x is [B, D + 3, Tmax], the input of a model trained with ``is_append_f0`` (append_ppg, data_utils.py:142-160):
    rows [:D] are the posteriors above, bit for bit (written in place through a batch stride: no copy), rows [D:] the log F0,
    its delta and its delta-delta of ppg.compute_f0's track over the very samples the features were cut from
    (facppg_f0_batch, facppg_lf0_rows_padded), exactly 0 behind T_b as well.  ``f0_options``: an F0Options whose sample rate and
    frame shift are the front end's.  Still nothing is copied back and nothing waits."""
    K = padded_ppg_dim(deps, is_full_ppg)
    if not len(wavs):
        raise ValueError("compute_ppg_padded: no utterance")
    if append_f0:
        f0_options = f0_options or F0Options()
        if int(f0_options.sample_rate) != 16000 or int(f0_options.frame_shift) * 1000 != int(shift) * int(f0_options.sample_rate):
            raise _lib.FacppgError("compute_ppg_padded: F0 frames of %d samples at %d Hz are not the front end's %d ms frames at 16000 Hz"
                                   % (f0_options.frame_shift, f0_options.sample_rate, shift))
    L = _lib.load()
    dev = wavs[0].data().device
    samples = [] if append_f0 else None
    flat, frames = _feat_for_nnet_flat(wavs, _on_device(deps, "lda", dev) if dev.type == "cuda" else deps.lda, keep_tables=True, samples=samples,
                                       frame_shift=shift)
    h = _tdnn_handle(deps.nnet, dev, "compute_ppg_padded")
    if flat.shape[1] != h.in_dim:
        raise _lib.FacppgError("compute_ppg_padded: features have %d dims, the model's input node has %d" % (flat.shape[1], h.in_dim))
    tr_t = None
    if not is_full_ppg:
        tr_t = _on_device(deps, "monophone_trans", dev, transposed=True)
        if tr_t.shape[0] != h.out_dim:
            raise _lib.FacppgError("reduce_ppg_dim: PPG has %d dims, the transform expects %d" % (h.out_dim, tr_t.shape[0]))
    B, Tmax = len(frames), max(frames)
    off = _lib.host_offsets(frames)
    nbytes = L.facppg_tdnn_batch_workspace_bytes(h.handle, off, B)
    if nbytes == 0:
        _lib.check(-1)
    off_dev = _lib.upload(list(off), torch.int32, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if not append_f0:
        x = torch.empty(B, K, Tmax, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.facppg_tdnn_forward_batch_padded(h.handle, _lib.ptr(flat), _lib.ptr(off_dev), off, B, _lib.ptr(tr_t),
                                                          K if tr_t is not None else 0, Tmax, _lib.ptr(x), _lib.ptr(ws), ws.numel(),
                                                          _lib.current_stream(dev)))
        return x, [int(n) for n in frames]
    x = torch.empty(B, K + 3, Tmax, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_tdnn_forward_batch_padded_strided(h.handle, _lib.ptr(flat), _lib.ptr(off_dev), off, B, _lib.ptr(tr_t),
                                                              K if tr_t is not None else 0, Tmax, (K + 3) * Tmax, _lib.ptr(x), _lib.ptr(ws),
                                                              ws.numel(), _lib.current_stream(dev)))
    lf0_rows_padded(f0_flat(samples[0], f0_options), samples[0], x, K)
    return x, [int(n) for n in frames]


def compute_feat_for_nnet(wav_path, lda_path):
    """compute_ppg.py:137-158"""
    if not os.path.exists(wav_path):
        logging.error("File %s does not exist." % (wav_path))
    if not os.path.exists(lda_path):
        logging.error("Transform file %s does not exist." % (lda_path))
    return compute_feat_for_nnet_internal(feat.read_wav_kaldi(wav_path), torch.from_numpy(kaldi_io.read_matrix(lda_path)))


def compute_monophone_ppg(wav, nnet, lda, transform, shift=10):
    """compute_ppg.py:161-181: wav -> features -> full PPG -> monophone PPG, as a numpy array."""
    feats = compute_feat_for_nnet_internal(wav, lda, frame_shift=shift)
    return reduce_ppg_dim(compute_full_ppg(nnet, feats), transform).cpu().numpy()


def compute_full_ppg_wrapper(wav, nnet, lda, shift=10):
    """compute_ppg.py:184-202"""
    feats = compute_feat_for_nnet_internal(wav, lda, frame_shift=shift)
    return compute_full_ppg(nnet, feats).cpu().numpy()


class DependenciesPPG(object):
    """compute_ppg.py:205-256.  The reference does not ship the acoustic model: ``nnet`` is None (and ``precomputed_only``
    True) when ``nnet_path`` does not exist, else the model read by common.decode.read_nnet3_model."""

    def __init__(self, nnet_path=NNET_PATH, lda_path=LDA_PATH, reduce_dim_path=REDUCE_DIM_PATH, splice_opts_path=SPLICE_OPTS_PATH):
        self.nnet_path, self.lda_path, self.reduce_dim_path, self.splice_opts_path = nnet_path, lda_path, reduce_dim_path, splice_opts_path
        self.precomputed_only = not os.path.isfile(nnet_path)
        self.nnet = None if self.precomputed_only else decode.read_nnet3_model(nnet_path)
        self.context_parser = re.compile(r"--left-context=(\d+) --right-context=(\d+)")
        self.lda = self.monophone_trans = None
        self.splice_opts, self.left_context, self.right_context = "", None, None
        if os.path.isfile(lda_path):
            self.lda = torch.from_numpy(kaldi_io.read_matrix(lda_path))
        if os.path.isfile(reduce_dim_path):
            self.monophone_trans = feat.read_sparse_mat(reduce_dim_path)
        if os.path.isfile(splice_opts_path):
            with open(splice_opts_path, 'r') as reader:
                self.splice_opts = reader.readline()
            context = self.context_parser.match(self.splice_opts) if self.splice_opts else None
            if context:
                self.left_context, self.right_context = context.groups()
            else:
                logging.warning("Splice options are empty.")
