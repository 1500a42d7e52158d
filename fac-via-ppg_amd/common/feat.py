"""Acoustic-feature helpers of the PPG front-end -- drop-in for the blob-free part of src/common/feat.py (:29-170), on
libfacppg_hip instead of pykaldi.  Kaldi objects become plain tensors: a "Matrix" is a float32 GPU tensor [T, D].

  read_wav_kaldi / read_wav_kaldi_internal   wav file / array -> WaveData (first channel, int16-range floats, on the GPU)
  MfccOptions, compute_mfcc_feats            Kaldi MFCC with the reference's options (facppg_mfcc_*)
  apply_cepstral_mean_norm, splice_frames, apply_feat_transform          (facppg_cmn_splice_transform)
  read_sparse_mat                            Kaldi sparse matrix -> dense float32 GPU tensor
  compute_mfcc_feats_batch, cmn_splice_transform_batch   the same chain for a list of utterances in one pass
                                             (facppg_mfcc_compute_batch, facppg_cmn_splice_transform_batch)

Dither is not applied (Kaldi's default adds random +-1 LSB noise; this path is deterministic); inputs above 16 kHz are
downsampled with Kaldi's LinearResample when allow_downsample is set (facppg_resample), as the reference does."""
import copy
import logging

import numpy as np
import torch
from scipy.io import wavfile

from common import kaldi_io
from facppg import lib as _lib


class WaveData(object):
    """What the reference gets from kaldi.feat.wave.WaveData: ``data()`` [channels = 1, N] and ``samp_freq``."""

    def __init__(self, samp_freq, data):
        self.samp_freq = float(samp_freq)
        self._data = data

    def data(self):
        return self._data

    @property
    def duration(self):
        return self._data.shape[1] / self.samp_freq


def read_wav_kaldi_internal(wav, fs):
    """feat.py:29-56: numpy samples [N] or [N, channels] (int16 range) -> WaveData holding the first channel only."""
    wav = np.asarray(wav)
    if wav.ndim == 2:
        wav = wav[:, 0]
    if wav.ndim != 1:
        raise ValueError("wav must be [samples] or [samples, channels]")
    data = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))[None]
    return WaveData(fs, data.cuda() if torch.cuda.is_available() else data)


def read_wav_kaldi(wav_file_path):
    """feat.py:59-71"""
    fs, wav = wavfile.read(wav_file_path, False)
    return read_wav_kaldi_internal(wav, fs)


class FrameExtractionOptions(object):
    """kaldi.feat.window.FrameExtractionOptions defaults (feature-window.h)."""

    def __init__(self):
        self.samp_freq = 16000.0
        self.frame_shift_ms = 10.0
        self.frame_length_ms = 25.0
        self.dither = 1.0
        self.preemph_coeff = 0.97
        self.remove_dc_offset = True
        self.window_type = "povey"
        self.round_to_power_of_two = True
        self.snip_edges = True
        self.allow_downsample = False


class MelBanksOptions(object):
    def __init__(self):
        self.num_bins = 23
        self.low_freq = 20.0
        self.high_freq = 0.0


class MfccOptions(object):
    """kaldi.feat.mfcc.MfccOptions defaults (feature-mfcc.h)."""

    def __init__(self):
        self.frame_opts = FrameExtractionOptions()
        self.mel_opts = MelBanksOptions()
        self.num_ceps = 13
        self.use_energy = True
        self.cepstral_lifter = 22.0


class SampleBatch(object):
    """B utterances at the features' rate laid end to end: ``flat`` [sum n] on the GPU, sample counts and frame counts, and
    the offset tables of both as C arrays on the host (s_off, f_off) and int32 tensors on the device (s_dev, f_dev)."""

    def __init__(self, flat, counts, frames, s_off, f_off, s_dev, f_dev):
        self.flat, self.counts, self.frames = flat, counts, frames
        self.s_off, self.f_off, self.s_dev, self.f_dev = s_off, f_off, s_dev, f_dev


class Mfcc(object):
    """kaldi.feat.mfcc.Mfcc: folds DC removal, pre-emphasis, povey window, zero padding and the DFT into one matrix on the
    host (float64), and hands it with the mel bank and the liftered DCT to facppg_mfcc_create."""

    def __init__(self, opts):
        fo = opts.frame_opts
        if fo.snip_edges:
            raise _lib.FacppgError("Mfcc: only snip_edges=False is built (what the reference uses, compute_ppg.py:106-121)")
        if fo.window_type != "povey" or not fo.remove_dc_offset or not fo.round_to_power_of_two:
            raise _lib.FacppgError("Mfcc: only Kaldi's default povey window / DC removal / power-of-two padding are built")
        if fo.dither != 0.0 and not getattr(Mfcc, "_dither_noted", False):
            logging.info("Mfcc: dither is not applied (deterministic features)")
            Mfcc._dither_noted = True
        self.opts = opts
        fs = fo.samp_freq
        self.length, self.shift = int(fs * 0.001 * fo.frame_length_ms), int(fs * 0.001 * fo.frame_shift_ms)
        n_fft = 1 << (self.length - 1).bit_length()
        self.nbins = n_fft // 2 + 1
        n = self.length
        i = np.arange(n)
        window = (0.5 - 0.5 * np.cos(2 * np.pi * i / (n - 1))) ** 0.85
        dc = np.eye(n) - np.full((n, n), 1.0 / n)                              # x - mean(x)
        pre = np.eye(n) - fo.preemph_coeff * np.eye(n, k=-1)
        pre[0, 0] -= fo.preemph_coeff                                          # w[0] -= c * w[0]
        lin = (window[:, None] * pre) @ dc                                     # [n, n]: frame -> windowed, pre-emphasised frame
        k = np.arange(self.nbins)
        ang = -2.0 * np.pi * np.outer(k, i) / n_fft
        basis = np.concatenate([np.cos(ang) @ lin, np.sin(ang) @ lin], 0)      # [2*nbins, n]
        mo = opts.mel_opts
        nyq = 0.5 * fs
        hi_f = mo.high_freq if mo.high_freq > 0 else nyq + mo.high_freq
        ms = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
        lo, hi = ms(mo.low_freq), ms(hi_f)
        delta = (hi - lo) / (mo.num_bins + 1)
        mel_f = ms(fs / n_fft * np.arange(n_fft // 2))
        mel = np.zeros((mo.num_bins, self.nbins))                              # the Nyquist column stays zero (Kaldi skips it)
        for b in range(mo.num_bins):
            left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
            up, dn = (mel_f > left) & (mel_f <= center), (mel_f > center) & (mel_f < right)
            mel[b, :n_fft // 2][up] = (mel_f[up] - left) / (center - left)
            mel[b, :n_fft // 2][dn] = (right - mel_f[dn]) / (right - center)
        dct = np.zeros((opts.num_ceps, mo.num_bins))
        dct[0] = np.sqrt(1.0 / mo.num_bins)
        nn = np.arange(mo.num_bins)
        for c in range(1, opts.num_ceps):
            dct[c] = np.sqrt(2.0 / mo.num_bins) * np.cos(np.pi / mo.num_bins * (nn + 0.5) * c)
        if opts.cepstral_lifter != 0.0:
            dct *= (1.0 + 0.5 * opts.cepstral_lifter * np.sin(np.pi * np.arange(opts.num_ceps) / opts.cepstral_lifter))[:, None]
        self._tables = [torch.from_numpy(a.astype(np.float32)).contiguous() for a in (basis, mel, dct)]
        self._handle = None

    def _get(self, dev):
        if self._handle is None or self._handle[1] != dev:
            self._release()
            L = _lib.load()
            basis, mel, dct = [t.to(dev) for t in self._tables]
            out = _lib.ctypes.c_void_p()
            with torch.cuda.device(dev):
                _lib.check(L.facppg_mfcc_create(self.length, self.shift, self.nbins, _lib.ptr(basis), _lib.ptr(mel), mel.shape[0], _lib.ptr(dct),
                                                dct.shape[0], dev.index, _lib.current_stream(dev), _lib.ctypes.byref(out)))
            self._handle = (out, dev)
        return self._handle[0]

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _lib.load().facppg_mfcc_destroy(self._handle[0])
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _at_model_rate(self, wave, samp_freq, out=None):
        """wave [N] at samp_freq -> the samples at the features' rate, downsampled through facppg_resample when the input
        rate is higher (feature-common-inl.h ComputeFeatures); written into ``out`` when given (a slice of a batch's buffer)."""
        L = _lib.load()
        dev = wave.device
        target = self.opts.frame_opts.samp_freq
        if float(samp_freq) == float(target):
            return wave if out is None else out.copy_(wave)
        # a higher input rate is downsampled when allow_downsample, anything else is an error
        if float(samp_freq) < float(target) or not self.opts.frame_opts.allow_downsample:
            raise _lib.FacppgError("Mfcc: waveform sampled at %g Hz, features need %g Hz (set frame_opts.allow_downsample for higher rates)"
                                   % (samp_freq, target))
        n_out = L.facppg_resample_num_samples(wave.numel(), int(samp_freq), int(target))
        res = torch.empty(n_out, device=dev) if out is None else out
        with torch.cuda.device(dev):
            _lib.check(L.facppg_resample(_lib.ptr(wave), wave.numel(), int(samp_freq), int(target), _lib.ptr(res), _lib.current_stream(dev)))
        return res

    def num_samples_at_model_rate(self, n, samp_freq):
        target = self.opts.frame_opts.samp_freq
        return n if float(samp_freq) == float(target) else _lib.load().facppg_resample_num_samples(n, int(samp_freq), int(target))

    def compute_features(self, wave, samp_freq, vtln_warp=1.0):
        """wave: [N] samples (GPU tensor, int16 range) -> [T, num_ceps] (GPU)."""
        _lib.require_cuda(wave, "Mfcc.compute_features: wave")
        if vtln_warp != 1.0:
            raise _lib.FacppgError("VTLN warping is not built (the reference always passes 1.0, feat.py:95)")
        L = _lib.load()
        dev = wave.device
        wave = self._at_model_rate(wave.float().contiguous().reshape(-1), samp_freq)
        h = self._get(dev)
        n = wave.numel()
        T = L.facppg_mfcc_num_frames(h, n)
        out = torch.empty(T, self.opts.num_ceps, device=dev)
        ws = torch.empty(L.facppg_mfcc_workspace_bytes(h, n), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.facppg_mfcc_compute(h, _lib.ptr(wave), n, 1 if self.opts.use_energy else 0, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                             _lib.current_stream(dev)))
        return out


    def samples_end_to_end(self, waves, samp_freqs):
        """waves: B tensors [N_b] (GPU, int16 range) sampled at samp_freqs[b] -> a SampleBatch: the utterances at the features'
        rate laid end to end in one buffer (each downsampled on its own where needed, straight into its place), their sample
        and frame counts, and both offset tables on the host and on the device -- what the batch entry points read."""
        if not len(waves):
            raise ValueError("compute_features_batch: no utterance")
        for w in waves:
            _lib.require_cuda(w, "Mfcc.compute_features_batch: wave")
        L = _lib.load()
        dev = waves[0].device
        h = self._get(dev)
        waves = [w.float().contiguous().reshape(-1) for w in waves]
        counts = [self.num_samples_at_model_rate(w.numel(), fs) for w, fs in zip(waves, samp_freqs)]
        frames = [L.facppg_mfcc_num_frames(h, n) for n in counts]
        for w, fs, T in zip(waves, samp_freqs, frames):
            if T <= 0:
                self.compute_features(w, fs)          # too short for one frame: the single call's refusal, word for word
        s_off, f_off = _lib.host_offsets(counts), _lib.host_offsets(frames)
        flat = torch.empty(s_off[-1], device=dev)
        for b, (w, fs) in enumerate(zip(waves, samp_freqs)):
            self._at_model_rate(w, fs, out=flat[s_off[b]:s_off[b + 1]])
        s_dev, f_dev = _lib.upload(list(s_off), torch.int32, dev), _lib.upload(list(f_off), torch.int32, dev)
        return SampleBatch(flat, counts, frames, s_off, f_off, s_dev, f_dev)

    def compute_features_batch(self, waves, samp_freqs, samples=None):
        """waves: B tensors [N_b] (GPU, int16 range) sampled at samp_freqs[b] -> (mfcc [sum T, num_ceps], frame counts [B]).
        Each utterance is downsampled on its own where needed, straight into its place in one buffer; framing, spectrum and
        cepstra then run once over all frames (facppg_mfcc_compute_batch).  Every row equals compute_features' bit for bit.
        samples: a list that receives the SampleBatch the features were cut from (the F0 tracker reads the same samples)."""
        sb = self.samples_end_to_end(waves, samp_freqs)
        if samples is not None:
            samples.append(sb)
        L = _lib.load()
        flat, frames, s_off, f_off, s_dev, f_dev = sb.flat, sb.frames, sb.s_off, sb.f_off, sb.s_dev, sb.f_dev
        dev = flat.device
        h = self._get(dev)
        out = torch.empty(f_off[-1], self.opts.num_ceps, device=dev)
        ws = torch.empty(L.facppg_mfcc_batch_workspace_bytes(h, f_off[-1]), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.facppg_mfcc_compute_batch(h, _lib.ptr(flat), _lib.ptr(s_dev), s_off, _lib.ptr(f_dev), f_off, len(frames),
                                                   1 if self.opts.use_energy else 0, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                   _lib.current_stream(dev)))
        return out, frames


_KEPT_MFCC = {}


def _kept_mfcc(opts):
    """One Mfcc per set of option values, kept with its device tables: building one costs the host a float64 DFT basis, an
    upload, and -- when it is dropped -- a hipFree, which waits for the device.  The key is the option VALUES and the kept
    Mfcc holds a copy of them, so options changed afterwards find or make another entry; entries live as long as the process
    (``_KEPT_MFCC.clear()`` releases them)."""
    key = tuple(sorted(vars(opts.frame_opts).items())) + tuple(sorted(vars(opts.mel_opts).items())) + \
        (opts.num_ceps, opts.use_energy, opts.cepstral_lifter)
    if key not in _KEPT_MFCC:
        _KEPT_MFCC[key] = Mfcc(copy.deepcopy(opts))
    return _KEPT_MFCC[key]


def compute_mfcc_feats_batch(wavs, mfcc_opts, keep_tables=False, samples=None):
    """compute_mfcc_feats for a list of WaveData: (mfcc [sum T, D] of the first channels laid end to end, frame counts).
    keep_tables: compute with the Mfcc kept for these option values (same values; no table upload or hipFree in the call).
    samples: a list that receives the SampleBatch (Mfcc.compute_features_batch)."""
    mfcc = _kept_mfcc(mfcc_opts) if keep_tables else Mfcc(mfcc_opts)
    return mfcc.compute_features_batch([w.data()[0] for w in wavs], [w.samp_freq for w in wavs], samples=samples)


def compute_mfcc_feats(wav, mfcc_opts):
    """feat.py:74-100: T*D MFCCs of the first channel."""
    return Mfcc(mfcc_opts).compute_features(wav.data()[0], wav.samp_freq, 1.0)


def _cst(feats, do_cmn, left, right, transform):
    _lib.require_cuda(feats, "feature matrix")
    L = _lib.load()
    dev = feats.device
    feats = feats.float().contiguous()
    T, D = feats.shape
    W = (left + right + 1) * D
    tr = None if transform is None else transform.to(dev).float().contiguous()
    if tr is not None and tr.shape[1] not in (W, W + 1):
        logging.error("Transform matrix has bad dimension %dx%d versus feat dim %d" % (tr.shape[0], tr.shape[1], W))   # feat.py:154-155
        raise _lib.FacppgError("Transform matrix has bad dimension %dx%d versus feat dim %d" % (tr.shape[0], tr.shape[1], W))
    out = torch.empty(T, W if tr is None else tr.shape[0], device=dev)
    mean = torch.empty(D, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_cmn_splice_transform(_lib.ptr(feats), T, D, 1 if do_cmn else 0, left, right, _lib.ptr(tr), 0 if tr is None else tr.shape[0],
                                                 0 if tr is None else tr.shape[1], _lib.ptr(out), _lib.ptr(mean), _lib.current_stream(dev)))
    return out


def apply_cepstral_mean_norm(feats):
    """feat.py:103-118 (mean only)."""
    return _cst(feats, True, 0, 0, None)


def splice_frames(feats, left_context, right_context):
    """kaldi.feat.functions.splice_frames (compute_ppg.py:128): edge frames are replicated."""
    return _cst(feats, False, int(left_context), int(right_context), None)


def apply_feat_transform(feats, transform):
    """feat.py:121-156: linear (D' x D) or affine (D' x (D+1)) transform."""
    return _cst(feats, False, 0, 0, torch.as_tensor(transform))


def cmn_splice_transform(feats, left_context, right_context, transform):
    """The three steps of compute_ppg.py:124-132 in one pass."""
    return _cst(feats, True, int(left_context), int(right_context), torch.as_tensor(transform))


def cmn_splice_transform_batch(feats, frames, left_context, right_context, transform, do_cmn=True):
    """cmn_splice_transform per utterance in one pass: feats [sum T, D] (utterances laid end to end), frames = their frame
    counts -> [sum T, M] (or the spliced width when transform is None).  Mean, splice and clamp stay inside each utterance."""
    _lib.require_cuda(feats, "feature matrix")
    L = _lib.load()
    dev = feats.device
    feats = feats.float().contiguous()
    left, right = int(left_context), int(right_context)
    f_off = _lib.host_offsets(frames)
    T, D = feats.shape
    if f_off[-1] != T:
        raise ValueError("cmn_splice_transform_batch: the frame counts add up to %d, the matrix has %d rows" % (f_off[-1], T))
    W = (left + right + 1) * D
    tr = None if transform is None else torch.as_tensor(transform).to(dev).float().contiguous()
    if tr is not None and tr.shape[1] not in (W, W + 1):
        logging.error("Transform matrix has bad dimension %dx%d versus feat dim %d" % (tr.shape[0], tr.shape[1], W))   # feat.py:154-155
        raise _lib.FacppgError("Transform matrix has bad dimension %dx%d versus feat dim %d" % (tr.shape[0], tr.shape[1], W))
    out = torch.empty(T, W if tr is None else tr.shape[0], device=dev)
    mean = torch.empty(len(frames), D, device=dev)
    f_dev = _lib.upload(list(f_off), torch.int32, dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_cmn_splice_transform_batch(_lib.ptr(feats), _lib.ptr(f_dev), f_off, len(frames), D, 1 if do_cmn else 0, left, right,
                                                       _lib.ptr(tr), 0 if tr is None else tr.shape[0], 0 if tr is None else tr.shape[1],
                                                       _lib.ptr(out), _lib.ptr(mean), _lib.current_stream(dev)))
    return out


def read_sparse_mat(sparse_mat_dir):
    """feat.py:159-170; returned densified (float32 tensor [rows, cols]), which is how the reference uses it."""
    return torch.from_numpy(kaldi_io.read_sparse_matrix(sparse_mat_dir))
