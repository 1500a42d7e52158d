"""Score a conversion by its PPG round trip: does the synthesized speech still say the teacher's phones?

The reference has no counterpart (generate_synthesis.py:86-98 writes the wav and never compares it with anything).  The decoder
is autoregressive and its prenet dropouts are on at inference, so an utterance can skip, repeat or babble up to its step limit;
the teacher-forced loss of validate() never sees that.  Here the converted audio goes back through the wav -> PPG front end, and
its monophone posteriors are aligned with the teacher's by dynamic time warping on the device (facppg_ppg_dtw, include/facppg.h
states the definition): local distance the squared Hellinger distance of two posteriors, and along the chosen path its length and
the number of cells whose top classes agree.

  distance   cost / steps: the mean squared Hellinger distance along the path; 0 = the same phones
  agreement  agree / steps: the share of path cells whose top class matches
  stretch    steps / max(la, lb): 1.0 = a path with no stalls beyond the length difference

Three numbers per utterance do not say WHICH phones were lost: ``roundtrip(..., phones=True)`` adds facppg.align.phone_report's
per-phone records from the same padded batch.

The round trip needs a vocoder, a second front-end pass and an acoustic model, and it scores phones.  ``mel_dtw`` and
``attention_path`` score the free-running decoder on what its loss is defined over, with nothing but its own outputs
(script.train_ppg2mel.validate_free_running): the mel-cepstral distortion along a DTW path between the decoded and the target
mels, and a summary of the attention path that says why a score is bad -- skipped input, backward jumps, stalls, stopping short.
"""
import math

import numpy as np
import torch

from facppg import lib as _lib
from facppg.lib import FacppgError


def _lengths(values, B, what, who="ppg_dtw"):
    vals = [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]
    if len(vals) != B:
        raise FacppgError("%s: %d lengths for the %d utterances of %s" % (who, len(vals), B, what))
    return vals


def ppg_dtw(a, la, b, lb, band=0):
    """a [B, D, Ta_max], b [B, D, Tb_max]: fp32 GPU tensors in the front end's layout (channel-major, frames contiguous); la, lb:
    their B lengths on the host.  Pair p is a[p, :, :la[p]] against b[p, :, :lb[p]]; what lies behind a length is not read.
    band: 0, or the half-width (>= 2) of the slanted band of include/facppg.h in frames of the longer side.
    Returns a dict of host arrays [B]: cost (float32), steps, agree (int32), distance, agreement, stretch (float64).
    One launch sequence on the current stream and one small device -> host copy at the end."""
    _lib.require_cuda(a, "ppg_dtw: a")
    _lib.require_cuda(b, "ppg_dtw: b")
    if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != b.shape[:2]:
        raise FacppgError("ppg_dtw: a and b must be [B, D, T] with equal B and D (got %s and %s)" % (tuple(a.shape), tuple(b.shape)))
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device:
        raise FacppgError("ppg_dtw: a and b must be float32 tensors on one device")
    L = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    B, D, Ta_max = (int(v) for v in a.shape)
    Tb_max = int(b.shape[2])
    la, lb = _lengths(la, B, "a"), _lengths(lb, B, "b")
    dev = a.device
    la_host, lb_host = _lib.offsets_array(la), _lib.offsets_array(lb)
    nbytes = L.facppg_ppg_dtw_workspace_bytes(B, D, Ta_max, Tb_max, int(band))
    if nbytes == 0:
        _lib.check(-1)
    lens = _lib.upload(la + lb, torch.int32, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(3, B, dtype=torch.int32, device=dev)          # cost (fp32 bits), steps, agree: one copy back
    with torch.cuda.device(dev):
        _lib.check(L.facppg_ppg_dtw(_lib.ptr(a), _lib.ptr(lens[:B]), la_host, Ta_max, _lib.ptr(b), _lib.ptr(lens[B:]), lb_host, Tb_max, B, D,
                                    int(band), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(ws), ws.numel(),
                                    _lib.current_stream(dev)))
    host = out.cpu().numpy()
    cost, steps, agree = host[0].view(np.float32).copy(), host[1].copy(), host[2].copy()
    longest = np.maximum(np.asarray(la, dtype=np.float64), np.asarray(lb, dtype=np.float64))
    return {"cost": cost, "steps": steps, "agree": agree, "distance": cost.astype(np.float64) / steps, "agreement": agree / steps.astype(np.float64),
            "stretch": steps / longest}


MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)      # dB per unit of Euclidean distance between natural-log cepstra
MAX_CEP = 64                                         # facppg_mel_dtw stages at most 64 coefficients of a tile of frames


def cepstral_basis(M, n_cep):
    """fp32 [n_cep, M]: rows k = 1 .. n_cep of the orthonormal DCT-II over M channels, sqrt(2 / M) cos(pi k (m + 0.5) / M), computed
    in float64 and rounded once.  Row 0 (c0, the level) is left out, so a gain change does not score.  1 <= n_cep <= min(M - 1, 64)."""
    M, n_cep = int(M), int(n_cep)
    if M < 2 or not 1 <= n_cep <= min(M - 1, MAX_CEP):
        raise FacppgError("cepstral_basis: n_cep must lie in [1, min(M - 1, %d)] (got n_cep = %d for M = %d channels)" % (MAX_CEP, n_cep, M))
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return torch.from_numpy((math.sqrt(2.0 / M) * np.cos(math.pi * k * (m + 0.5) / M)).astype(np.float32))


def mel_dtw(a, la, b, lb, n_cep=13, band=0, basis=None):
    """a [B, M, Ta_max], b [B, M, Tb_max]: fp32 GPU tensors of NATURAL-log mels, channel-major with the frames contiguous
    (Tacotron2.inference's mel_post, the padded targets); la, lb: their B lengths on the host.  Pair p is a[p, :, :la[p]] against
    b[p, :, :lb[p]]; what lies behind a length is not read.  basis: None -- cepstral_basis(M, n_cep) -- or an fp32 [K, M] matrix
    (n_cep is then ignored).  band: 0, or the half-width (>= 2) of the slanted band of include/facppg.h.
    Returns a dict of host arrays [B]: cost (float32), steps (int32), mcd, stretch (float64), where
      mcd      MCD_DB * cost / steps: the mean mel-cepstral distortion along the path in dB, MCD_DB = 10 sqrt(2) / ln 10
      stretch  steps / max(la, lb), as ppg_dtw's
    THIS IS THIS BUILD'S OWN DEFINITION (facppg_mel_dtw, include/facppg.h): a DTW over an orthonormal DCT of log-mels without c0,
    not over WORLD or SPTK cepstra.  Its values compare within this build only.
    One launch sequence on the current stream and one small device -> host copy at the end."""
    _lib.require_cuda(a, "mel_dtw: a")
    _lib.require_cuda(b, "mel_dtw: b")
    if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != b.shape[:2]:
        raise FacppgError("mel_dtw: a and b must be [B, M, T] with equal B and M (got %s and %s)" % (tuple(a.shape), tuple(b.shape)))
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device:
        raise FacppgError("mel_dtw: a and b must be float32 tensors on one device")
    L = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    B, M, Ta_max = (int(v) for v in a.shape)
    Tb_max = int(b.shape[2])
    dev = a.device
    if basis is None:
        basis = cepstral_basis(M, n_cep)
    if not torch.is_tensor(basis) or basis.dim() != 2 or int(basis.shape[1]) != M or basis.dtype != torch.float32:
        raise FacppgError("mel_dtw: basis must be a float32 [K, M = %d] tensor (cepstral_basis)" % M)
    basis = basis.to(dev).contiguous()
    K = int(basis.shape[0])
    la, lb = _lengths(la, B, "a", "mel_dtw"), _lengths(lb, B, "b", "mel_dtw")
    la_host, lb_host = _lib.offsets_array(la), _lib.offsets_array(lb)
    nbytes = L.facppg_mel_dtw_workspace_bytes(B, M, K, Ta_max, Tb_max, int(band))
    if nbytes == 0:
        _lib.check(-1)
    lens = _lib.upload(la + lb, torch.int32, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(2, B, dtype=torch.int32, device=dev)          # cost (fp32 bits), steps: one copy back
    with torch.cuda.device(dev):
        _lib.check(L.facppg_mel_dtw(_lib.ptr(a), _lib.ptr(lens[:B]), la_host, Ta_max, _lib.ptr(b), _lib.ptr(lens[B:]), lb_host, Tb_max, B, M,
                                    _lib.ptr(basis), K, int(band), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws), ws.numel(),
                                    _lib.current_stream(dev)))
    host = out.cpu().numpy()
    cost, steps = host[0].view(np.float32).copy(), host[1].copy()
    longest = np.maximum(np.asarray(la, dtype=np.float64), np.asarray(lb, dtype=np.float64))
    return {"cost": cost, "steps": steps, "mcd": MCD_DB * cost.astype(np.float64) / steps, "stretch": steps / longest}


ATTENTION_FIELDS = ("first", "last", "back", "max_jump", "longest_stall", "visited")


def attention_path(alignments, out_lengths, in_lengths):
    """alignments [B, Tout_max, Tin_max]: fp32 GPU tensor, finite (Tacotron2.inference's fourth output); out_lengths, in_lengths: the
    B decoder-step and input-frame counts on the host.  With pos[t] the arg max of row t over the utterance's own input frames
    (the lowest on a tie) -- facppg_attention_path, include/facppg.h -- returns a dict of host arrays [B]:
      first, last     pos[0], pos[T-1]
      back            the steps on which pos moved backwards
      max_jump        the largest forward move of pos in one step (0: it never moved forward)
      longest_stall   the longest run of steps on one input frame
      visited         the distinct input frames pos was on               (int32 each)
      focus           the mean attention weight at pos (float32)
      coverage        visited / L;   end_gap   L - 1 - last: the input frames behind the last one attended to
    One launch sequence on the current stream and one small device -> host copy at the end."""
    _lib.require_cuda(alignments, "attention_path: alignments")
    if alignments.dim() != 3 or alignments.dtype != torch.float32:
        raise FacppgError("attention_path: alignments must be a float32 [B, Tout, Tin] tensor (got %s %s)" % (alignments.dtype, tuple(alignments.shape)))
    L = _lib.load()
    x = alignments.contiguous()
    B, Tout_max, Tin_max = (int(v) for v in x.shape)
    tout = _lengths(out_lengths, B, "the alignments (out_lengths)", "attention_path")
    tin = _lengths(in_lengths, B, "the alignments (in_lengths)", "attention_path")
    dev = x.device
    nbytes = L.facppg_attention_path_workspace_bytes(B, Tout_max, Tin_max)
    if nbytes == 0:
        _lib.check(-1)
    lens = _lib.upload(tout + tin, torch.int32, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(7 * B, dtype=torch.int32, device=dev)         # stats [B][6], then focus [B] (fp32 bits): one copy back
    with torch.cuda.device(dev):
        _lib.check(L.facppg_attention_path(_lib.ptr(x), _lib.ptr(lens[:B]), _lib.offsets_array(tout), Tout_max, _lib.ptr(lens[B:]),
                                           _lib.offsets_array(tin), Tin_max, B, _lib.ptr(out), _lib.ptr(out[6 * B:]), _lib.ptr(ws), ws.numel(),
                                           _lib.current_stream(dev)))
    host = out.cpu().numpy()
    res = {name: host[:6 * B].reshape(B, 6)[:, k].copy() for k, name in enumerate(ATTENTION_FIELDS)}
    res["focus"] = host[6 * B:].copy().view(np.float32)
    n_in = np.asarray(tin, dtype=np.float64)
    res["coverage"] = res["visited"] / n_in
    res["end_gap"] = np.asarray(tin, dtype=np.int32) - 1 - res["last"]
    return res


def _rates(sampling_rate, B):
    rates = list(sampling_rate) if hasattr(sampling_rate, "__len__") else [sampling_rate] * B
    if len(rates) != B or any(float(r) <= 0 for r in rates):
        raise FacppgError("roundtrip: sampling_rate must be one positive rate, or one per utterance (got %r for %d utterances)" % (sampling_rate, B))
    return [float(r) for r in rates]


def check_roundtrip_deps(deps, what="roundtrip"):
    """roundtrip's refusals that need no audio: host work only."""
    if deps is None:
        raise FacppgError("%s: no PPG dependencies (ppg.DependenciesPPG) -- the converted audio goes back through the acoustic model" % what)
    if getattr(deps, "monophone_trans", None) is None:
        raise FacppgError("%s: scores are over monophone classes: the dependencies have no monophone_trans, the pdf -> monophone "
                          "matrix (data/feats/reduce_dim.mat)" % what)


def roundtrip(wavs, audio, sampling_rate, deps, band=0, phones=False):
    """wavs: the B teacher WaveData (common.feat.read_wav_kaldi), on the GPU.  audio: the conversion's samples per utterance --
    device tensors or host arrays [N_b], floats in [-1, 1] at ``sampling_rate`` (one rate, or one per utterance).  The audio is
    wrapped as WaveData in Kaldi's int16 range, teacher and converted audio go through ONE ppg.compute_ppg_padded pass of 2 B
    utterances (monophone classes; the front end downsamples as it does for any wav), and rows [:B] of that padded batch are
    scored against rows [B:].  Returns ppg_dtw's dict plus teacher_frames and roundtrip_frames.
    phones: the scores gain "phones" (facppg.align.phone_report: per utterance one record per teacher phone -- where it landed in
    the conversion and how well it is supported) and "phones_kept" [B], from the same padded batch: there is no further front-end
    pass.
    Without ``deps.monophone_trans`` the call is refused on the host, before any device work."""
    from common.feat import WaveData
    from ppg.compute_ppg import compute_ppg_padded
    check_roundtrip_deps(deps)
    if wavs is None or not hasattr(wavs, "__len__") or len(wavs) == 0:
        raise FacppgError("roundtrip: wavs must be a non-empty list of WaveData (common.feat.read_wav_kaldi)")
    B = len(wavs)
    if audio is None or not hasattr(audio, "__len__") or len(audio) != B:
        raise FacppgError("roundtrip: one converted waveform per teacher wav (%d wavs, %s waveforms)" % (B, "no" if audio is None else len(audio)))
    rates = _rates(sampling_rate, B)
    dev = wavs[0].data().device
    back = []
    for x, fs in zip(audio, rates):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        back.append(WaveData(fs, (x.detach().to(dev, non_blocking=True).float().reshape(1, -1) * 32768.0)))
    with torch.no_grad():
        x, frames = compute_ppg_padded(list(wavs) + back, deps, is_full_ppg=False)
        scores = ppg_dtw(x[:B], frames[:B], x[B:], frames[B:], band=band)
        if phones:
            from facppg import align
            scores["phones"], scores["phones_kept"] = align.phone_report(x[:B], frames[:B], x[B:], frames[B:])
    scores["teacher_frames"] = np.asarray(frames[:B], dtype=np.int32)
    scores["roundtrip_frames"] = np.asarray(frames[B:], dtype=np.int32)
    return scores


SCORE_COLUMNS = ("teacher_frames", "roundtrip_frames", "distance", "agreement", "stretch")


def score_line(path, scores, b):
    """One line of synthesize_corpus --score_file: path, teacher_frames, roundtrip_frames, distance, agreement, stretch (tabs;
    floats as %.6g)."""
    return "%s\t%d\t%d\t%.6g\t%.6g\t%.6g" % (path, int(scores["teacher_frames"][b]), int(scores["roundtrip_frames"][b]),
                                             float(scores["distance"][b]), float(scores["agreement"][b]), float(scores["stretch"][b]))
