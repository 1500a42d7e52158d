"""F0 track on the device (csrc/facppg_f0.hip; include/facppg.h states the definition) -- what the reference takes from WORLD
through pyworld (utterance.py:33-38), which this tracker does not reproduce: PARITY UNPINNED at the WORLD boundary.

  F0Options            the fields of facppg_f0_config with their defaults, and the two host tables the tracker reads
  compute_nccf_batch   list of WaveData -> list of [T_b, L + 2] GPU tensors: the normalised cross-correlation, lags
                       lag_min - 1 .. lag_max + 1
  compute_f0_batch     list of WaveData -> list of [T_b] GPU tensors in Hz, 0 = unvoiced; the same resampling and the same
                       frames as ppg.compute_ppg_batch: one F0 frame meets one PPG frame
  compute_f0           one WaveData -> [T]

A user who wants WORLD tracks brings them as ``<wav>.f0.npy`` files (common.data_utils.get_f0_batch)."""
import numpy as np
import torch

from common import feat
from facppg import lib as _lib


class F0Options(object):
    """facppg_f0_config (include/facppg.h), same names and defaults."""

    def __init__(self, **kwargs):
        self.sample_rate = 16000
        self.frame_shift = 160
        self.window = 320
        self.lag_min = 40                # floor(16000 / 400)
        self.lag_max = 334               # ceil(16000 / 48)
        self.ballast = 50.0
        self.voicing_cost = 0.2
        self.freq_weight = 2.0
        for key, val in kwargs.items():
            if not hasattr(self, key):
                raise TypeError("F0Options: no option %r" % key)
            setattr(self, key, val)

    def config(self):
        return _lib.F0Config(int(self.sample_rate), int(self.frame_shift), int(self.window), int(self.lag_min), int(self.lag_max),
                             float(self.ballast), float(self.voicing_cost), float(self.freq_weight))

    @property
    def num_lags(self):
        return int(self.lag_max) - int(self.lag_min) + 1

    def tables(self):
        """float32 [2, L]: wl[l] = 1 - 0.3 l / lag_max and g[l] = log2 l for l = lag_min .. lag_max, computed in float64 and
        rounded once."""
        lags = np.arange(int(self.lag_min), int(self.lag_max) + 1, dtype=np.float64)
        return np.stack([1.0 - 0.3 * lags / float(self.lag_max), np.log2(lags)]).astype(np.float32)

    def _key(self):
        return tuple(sorted(vars(self).items()))


_KEPT_TABLES = {}


def _tables_on(options, dev):
    """The two tables on ``dev``, kept per option values and device (a few KB; an upload from pageable memory waits for the
    stream)."""
    key = (options._key(), dev)
    if key not in _KEPT_TABLES:
        _KEPT_TABLES[key] = torch.from_numpy(options.tables()).to(dev).contiguous()
    return _KEPT_TABLES[key]


def _front_end_mfcc(options):
    """The Mfcc of ppg.compute_ppg_batch's front end (kept: common.feat._kept_mfcc): its resampling and its frame count."""
    shift_ms = 1000.0 * int(options.frame_shift) / int(options.sample_rate)
    opts = feat.MfccOptions()
    opts.use_energy = False
    opts.frame_opts.allow_downsample = True
    opts.frame_opts.frame_shift_ms = int(shift_ms) if shift_ms == int(shift_ms) else shift_ms
    opts.frame_opts.snip_edges = False
    opts.frame_opts.samp_freq = float(options.sample_rate)
    mfcc = feat._kept_mfcc(opts)
    if mfcc.shift != int(options.frame_shift):
        raise _lib.FacppgError("F0Options: a frame shift of %d samples at %d Hz is no whole number of the front end's units" %
                               (options.frame_shift, options.sample_rate))
    return mfcc


def _samples(wavs, options):
    if not len(wavs):
        raise ValueError("compute_f0_batch: no utterance")
    return _front_end_mfcc(options).samples_end_to_end([w.data()[0] for w in wavs], [w.samp_freq for w in wavs])


def _check_samples(sb, options):
    for n, T in zip(sb.counts, sb.frames):
        if (n + int(options.frame_shift) // 2) // int(options.frame_shift) != T:
            raise _lib.FacppgError("F0Options: frame_shift %d does not cut %d samples into the front end's %d frames" % (options.frame_shift, n, T))


def f0_flat(sb, options=None):
    """A SampleBatch (common.feat) -> f0 [sum T] on the GPU (Hz, 0 = unvoiced), the utterances' frames laid end to end.  Queues
    work on the current stream and returns: nothing is copied back."""
    options = options or F0Options()
    _check_samples(sb, options)
    L = _lib.load()
    dev = sb.flat.device
    cfg = options.config()
    total = sb.f_off[len(sb.frames)]
    nbytes = L.facppg_f0_workspace_bytes(cfg, total)
    if nbytes == 0:
        _lib.check(-1)
    tables = _tables_on(options, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lag = torch.empty(total, dtype=torch.int32, device=dev)
    f0 = torch.empty(total, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_f0_batch(cfg, _lib.ptr(sb.flat), _lib.ptr(sb.s_dev), sb.s_off, _lib.ptr(sb.f_dev), sb.f_off, len(sb.frames),
                                     _lib.ptr(tables), _lib.ptr(lag), _lib.ptr(f0), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    return f0


def lf0_rows_padded(f0, sb, x, K):
    """Writes log F0, delta and delta-delta of f0 [sum T] into rows [K : K + 3] of the padded batch x [B, K + 3, Tmax]
    (facppg_lf0_rows_padded): zeros behind each utterance, every element of the three rows written."""
    L = _lib.load()
    dev = x.device
    B, rows, Tmax = x.shape
    with torch.cuda.device(dev):
        _lib.check(L.facppg_lf0_rows_padded(_lib.ptr(f0), _lib.ptr(sb.f_dev), sb.f_off, B, Tmax, rows * Tmax, _lib.ptr(x[0, K:]),
                                            _lib.current_stream(dev)))


def _split(flat, frames):
    out, at = [], 0
    for n in frames:
        out.append(flat[at:at + n])
        at += n
    return out


def compute_nccf_batch(wavs, options=None):
    """List of WaveData -> list of [T_b, L + 2] GPU tensors: phi(t, l) for l = lag_min - 1 .. lag_max + 1 (include/facppg.h).
    A row has the same bits whatever else is in the batch."""
    options = options or F0Options()
    sb = _samples(wavs, options)
    _check_samples(sb, options)
    L = _lib.load()
    dev = sb.flat.device
    out = torch.empty(sb.f_off[len(sb.frames)], options.num_lags + 2, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_f0_nccf_batch(options.config(), _lib.ptr(sb.flat), _lib.ptr(sb.s_dev), sb.s_off, _lib.ptr(sb.f_dev), sb.f_off,
                                          len(sb.frames), _lib.ptr(out), _lib.current_stream(dev)))
    return _split(out, sb.frames)


def compute_f0_batch(wavs, options=None):
    """List of WaveData -> list of [T_b] GPU tensors: F0 in Hz per PPG frame, 0 = unvoiced.  Inputs above the model's rate are
    downsampled as ppg.compute_ppg_batch downsamples them, and T_b is its frame count."""
    options = options or F0Options()
    sb = _samples(wavs, options)
    return _split(f0_flat(sb, options), sb.frames)


def compute_f0(wav, options=None):
    """One WaveData -> [T] GPU tensor (Hz, 0 = unvoiced)."""
    return compute_f0_batch([wav], options)[0]
