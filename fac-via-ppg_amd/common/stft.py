"""STFT / inverse STFT -- drop-in for src/common/stft.py, computed by libfacppg_hip.so.

Same constructor, buffers (``forward_basis``/``inverse_basis`` [n_fft+2, 1, n_fft]) and method
signatures as the reference's ``STFT`` module.  The bases are built analytically on the host
(the reference takes ``fft(eye)`` and a numerical ``pinv``, stft.py:55-63; for the real DFT the
pseudo-inverse is the inverse-rFFT weighting w_c/n with w_c = 1 for DC/Nyquist and 2 otherwise,
tests check the two agree), then handed to ``facppg_stft_create`` once per device.  ``transform`` /
``inverse`` / ``forward`` run the framing gather, MFMA GEMMs and overlap-add kernels of
csrc/facppg_dsp.hip; there is no CPU path.
"""
import numpy as np
import torch
from scipy.signal import get_window

from common.audio_processing import _center_pad, squared_window
from facppg import lib as _lib


def dft_bases(filter_length, hop_length, win_length, window):
    """(forward [n+2, n], inverse [n+2, n]) float32, windowed as stft.py:65-74."""
    n = filter_length
    cutoff = n // 2 + 1
    ang = 2.0 * np.pi * np.outer(np.arange(cutoff), np.arange(n)) / n
    fwd = np.vstack([np.cos(ang), -np.sin(ang)])
    wc = np.full(cutoff, 2.0)
    wc[0] = 1.0
    if n % 2 == 0:
        wc[-1] = 1.0
    scale = n / hop_length
    inv = np.vstack([np.cos(ang) * wc[:, None], -np.sin(ang) * wc[:, None]]) / (n * scale)
    fwd32, inv32 = fwd.astype(np.float32), inv.astype(np.float32)
    if window is not None:
        assert filter_length >= win_length
        win = _center_pad(get_window(window, win_length, fftbins=True), n).astype(np.float32)
        fwd32, inv32 = fwd32 * win, inv32 * win
    return fwd32, inv32


class STFT(torch.nn.Module):
    """stft.py:44-143"""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window='hann', mel_basis=None):
        super(STFT, self).__init__()
        self.filter_length = filter_length
        self.hop_length = hop_length
        self.win_length = win_length
        self.window = window
        self.forward_transform = None
        fwd, inv = dft_bases(filter_length, hop_length, win_length, window)
        self.register_buffer('forward_basis', torch.from_numpy(fwd[:, None, :]).float())
        self.register_buffer('inverse_basis', torch.from_numpy(inv[:, None, :]).float())
        wsq = squared_window(window, win_length, filter_length) if window is not None else \
            np.zeros(filter_length)   # window=None: no normalisation (stft.py:118)
        self.register_buffer('_win_sq', torch.from_numpy(wsq.astype(np.float32)), persistent=False)
        self._mel_basis_np = mel_basis

    # ------------------------------------------------------------ handle / workspace
    def _handle(self, dev):
        h = self.__dict__.get("_facppg_handle")
        if h is not None and h[1] == dev:
            return h[0]
        self._release()
        L = _lib.load()
        fwd = self.forward_basis.squeeze(1).to(dev).contiguous()
        inv_t = self.inverse_basis.squeeze(1).t().to(dev).contiguous()
        wsq = self._win_sq.to(dev).contiguous()
        mel = None if self._mel_basis_np is None else torch.as_tensor(self._mel_basis_np, dtype=torch.float32).to(dev).contiguous()
        out = _lib.ctypes.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(L.facppg_stft_create(self.filter_length, self.hop_length, _lib.ptr(fwd), _lib.ptr(inv_t), _lib.ptr(wsq),
                                            _lib.ptr(mel), 0 if mel is None else mel.shape[0], dev.index,
                                            _lib.current_stream(dev), _lib.ctypes.byref(out)))
        self.__dict__["_facppg_handle"] = (out, dev)
        return out

    def _release(self):
        h = self.__dict__.pop("_facppg_handle", None)
        if h is not None:
            _lib.load().facppg_stft_destroy(h[0])
        self.__dict__.pop("_facppg_ws", None)
        self.__dict__.pop("_facppg_pinv", None)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_facppg_handle", None)
        d.pop("_facppg_ws", None)
        d.pop("_facppg_pinv", None)
        return d

    def _workspace(self, h, dev, B, N):
        nbytes = _lib.load().facppg_stft_workspace_bytes(h, B, N)
        ws = self.__dict__.get("_facppg_ws")
        if ws is None or ws.numel() < nbytes or ws.device != dev:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.__dict__["_facppg_ws"] = ws
        return ws

    @staticmethod
    def _lengths(lengths, B, N, dev):
        if lengths is None:
            return None
        if torch.is_tensor(lengths):
            lt = lengths.to(device=dev, dtype=torch.int32).contiguous()
            if lt.numel() != B or int(lt.max()) > N:
                raise _lib.FacppgError("lengths must be B sample counts <= N")
            return lt
        if len(lengths) != B or max(int(n) for n in lengths) > N:       # host list: checked here, uploaded without a host stall
            raise _lib.FacppgError("lengths must be B sample counts <= N")
        return _lib.upload([int(n) for n in lengths], torch.int32, dev)

    # ------------------------------------------------------------ reference API
    def transform(self, input_data, lengths=None):
        """[B, N] -> magnitude, phase [B, n_fft/2+1, N//hop+1]  (stft.py:79-107)"""
        _lib.require_cuda(input_data, "STFT.transform: input_data")
        x = input_data.float().contiguous()
        B, N = x.shape
        self.num_samples = N
        dev = x.device
        h = self._handle(dev)
        ws = self._workspace(h, dev, B, N)
        F = N // self.hop_length + 1
        cutoff = self.filter_length // 2 + 1
        mag = torch.zeros(B, cutoff, F, device=dev) if lengths is not None else torch.empty(B, cutoff, F, device=dev)
        phase = torch.zeros_like(mag) if lengths is not None else torch.empty_like(mag)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_stft_transform(h, _lib.ptr(x), _lib.ptr(self._lengths(lengths, B, N, dev)), B, N,
                                                         _lib.ptr(mag), _lib.ptr(phase), _lib.ptr(ws), ws.numel(),
                                                         _lib.current_stream(dev)))
        return mag, phase

    def inverse(self, magnitude, phase):
        """[B, cutoff, F] x2 -> [B, 1, hop*(F-1)]  (stft.py:109-138)"""
        _lib.require_cuda(magnitude, "STFT.inverse: magnitude")
        mag = magnitude.float().contiguous()
        ph = phase.to(mag.device).float().contiguous()
        B, _, F = mag.shape
        dev = mag.device
        h = self._handle(dev)
        ws = self._workspace(h, dev, B, (F - 1) * self.hop_length)
        out = torch.empty(B, 1, self.hop_length * (F - 1), device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_stft_inverse(h, _lib.ptr(mag), _lib.ptr(ph), B, F, _lib.ptr(out), _lib.ptr(ws),
                                                       ws.numel(), _lib.current_stream(dev)))
        return out

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    # ------------------------------------------------------------ fused entry points
    def mel(self, y, lengths=None):
        """log-mel of y [B, N] in one pass (used by TacotronSTFT.mel_spectrogram)."""
        _lib.require_cuda(y, "mel_spectrogram: y")
        x = y.float().contiguous()
        B, N = x.shape
        dev = x.device
        h = self._handle(dev)
        ws = self._workspace(h, dev, B, N)
        n_mel = self._mel_basis_np.shape[0]
        F = N // self.hop_length + 1
        out = torch.zeros(B, n_mel, F, device=dev) if lengths is not None else torch.empty(B, n_mel, F, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_stft_mel(h, _lib.ptr(x), _lib.ptr(self._lengths(lengths, B, N, dev)), B, N,
                                                   _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
        return out

    # ------------------------------------------------------------ vocoder-free preview
    def _frame_lengths(self, lengths, B, F, dev, what):
        """``lengths`` as frame counts: None, a host list (checked here: B values in [2, F], each longer than the reflect
        padding) or a tensor (trusted beyond its size, as _lengths trusts sample counts) -> int32 [B] on the device or None."""
        if lengths is None:
            return None
        if torch.is_tensor(lengths):
            if lengths.numel() != B:
                raise _lib.FacppgError("%s: lengths must be B frame counts <= F" % what)
            return lengths.to(device=dev, dtype=torch.int32).contiguous()
        fb = [int(n) for n in lengths]
        if len(fb) != B or max(fb) > F:
            raise _lib.FacppgError("%s: lengths must be B frame counts <= F" % what)
        for n in fb:
            if n < 2 or self.hop_length * (n - 1) <= self.filter_length // 2:
                raise _lib.FacppgError("%s: an utterance of %d frames has hop * (frames - 1) = %d samples, reflect padding needs more "
                                       "than filter_length / 2 = %d" % (what, n, self.hop_length * (n - 1), self.filter_length // 2))
        return _lib.upload(fb, torch.int32, dev)

    @staticmethod
    def derive_seeds(seed, B):
        """B per-utterance phase seeds from one integer: SplitMix64 of seed + b (host arithmetic, 64 bits)."""
        out, m = [], 0xFFFFFFFFFFFFFFFF
        for b in range(B):
            z = (int(seed) + (b + 1) * 0x9E3779B97F4A7C15) & m
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
            out.append(z ^ (z >> 31))
        return out

    def _phase_seeds(self, B, dev, init_phase, seed, utterance_seeds, what):
        """The rule of Tacotron2.inference: ``utterance_seeds`` (B integers; utterance b's draws depend on its own alone) or one
        ``seed`` (B seeds derived on the host; None: drawn), never both, and neither next to ``init_phase``."""
        if seed is not None and utterance_seeds is not None:
            raise _lib.FacppgError("%s: seed and utterance_seeds are two ways to say the same thing -- give one" % what)
        if init_phase is not None:
            if seed is not None or utterance_seeds is not None:
                raise _lib.FacppgError("%s: init_phase leaves nothing to draw -- give it without seed / utterance_seeds" % what)
            return None
        if utterance_seeds is not None:
            if len(utterance_seeds) != B:
                raise _lib.FacppgError("%s: utterance_seeds must be B integers" % what)
            vals = [int(v) & 0xFFFFFFFFFFFFFFFF for v in utterance_seeds]
        else:
            if seed is None:
                seed = int(torch.empty((), dtype=torch.int64).random_().item())
            vals = self.derive_seeds(int(seed) & 0xFFFFFFFFFFFFFFFF, B)
        # (uint64 bit patterns through int64: the kernels read them as uint64_t)
        return _lib.upload([v - (1 << 64) if v >= (1 << 63) else v for v in vals], torch.int64, dev)

    def _gl_workspace(self, h, dev, B, F):
        nbytes = _lib.load().facppg_griffin_lim_workspace_bytes(h, B, max(F, 2))   # (mel_to_magnitude takes one frame too)
        ws = self.__dict__.get("_facppg_ws")
        if ws is None or ws.numel() < nbytes or ws.device != dev:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.__dict__["_facppg_ws"] = ws
        return ws

    def griffin_lim(self, magnitudes, n_iters=30, momentum=0.0, lengths=None, init_phase=None, seed=None, utterance_seeds=None,
                    return_convergence=False):
        """Griffin-Lim with optional momentum as one device loop (facppg_griffin_lim, defined in include/facppg.h):
        magnitudes [B, cutoff, F] -> [B, 1, hop * (F - 1)] (zeros behind hop * (lengths[b] - 1)), plus sc [B] with
        ``return_convergence`` (|| |t_n| - M || / || M || at the last iteration; 1 for n_iters = 0).  momentum = 0 is the loop
        of audio_processing.griffin_lim.  lengths: frame counts per utterance (list or tensor).  The starting phases are
        ``init_phase`` [B, cutoff, F] or drawn on the device from ``utterance_seeds`` / ``seed`` (this build's own Philox
        stream, not NumPy's: pass init_phase for the reference's draws); utterance b of a batch under utterance_seeds equals
        its own batch-1 call."""
        what = "STFT.griffin_lim"
        _lib.require_cuda(magnitudes, what + ": magnitudes")
        mag = magnitudes.float().contiguous()
        if mag.dim() != 3 or mag.shape[1] != self.filter_length // 2 + 1:
            raise _lib.FacppgError("%s: magnitudes must be [B, %d, F]" % (what, self.filter_length // 2 + 1))
        B, cutoff, F = mag.shape
        dev = mag.device
        if B < 1 or F < 2:
            raise _lib.FacppgError("%s: need at least one utterance of at least 2 frames, got B=%d F=%d" % (what, B, F))
        seeds = self._phase_seeds(B, dev, init_phase, seed, utterance_seeds, what)
        phi = None
        if init_phase is not None:
            phi = init_phase.to(dev).float().contiguous()
            if phi.shape != mag.shape:
                raise _lib.FacppgError("%s: init_phase must have the magnitudes' shape" % what)
        if lengths is None and self.hop_length * (F - 1) <= self.filter_length // 2:
            lengths = [F] * B               # (refused below with the reason)
        lt = self._frame_lengths(lengths, B, F, dev, what)
        h = self._handle(dev)
        ws = self._gl_workspace(h, dev, B, F)
        out = torch.empty(B, 1, self.hop_length * (F - 1), device=dev)
        sc = torch.empty(B, device=dev) if return_convergence else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_griffin_lim(h, _lib.ptr(mag), _lib.ptr(lt), _lib.ptr(phi), _lib.ptr(seeds), int(n_iters),
                                                      float(momentum), B, F, _lib.ptr(out), _lib.ptr(sc), _lib.ptr(ws), ws.numel(),
                                                      _lib.current_stream(dev)))
        return (out, sc) if return_convergence else out

    def draw_phase(self, utterance_seeds, F, device):
        """The phases griffin_lim(utterance_seeds=...) starts from, [B, cutoff, F] (facppg_griffin_lim_draw_phase)."""
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        B = len(utterance_seeds)
        seeds = self._phase_seeds(B, dev, None, None, utterance_seeds, "STFT.draw_phase")
        out = torch.empty(B, self.filter_length // 2 + 1, F, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_griffin_lim_draw_phase(self._handle(dev), _lib.ptr(seeds), B, F, _lib.ptr(out),
                                                                 _lib.current_stream(dev)))
        return out

    def _mel_pinv(self, h, dev):
        """pinv(mel_basis) [cutoff, n_mel]: float64 on the host, rounded to float32, handed to the handle once per device."""
        if self._mel_basis_np is None:
            raise _lib.FacppgError("mel_to_magnitude: this STFT was built without a mel basis")
        cur = self.__dict__.get("_facppg_pinv")
        if cur is None or cur[1] != dev or cur[2] is not h:
            P = np.linalg.pinv(np.asarray(self._mel_basis_np, dtype=np.float64)).astype(np.float32)
            t = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().facppg_stft_set_mel_pinv(h, _lib.ptr(t), _lib.current_stream(dev)))
            self.__dict__["_facppg_pinv"] = (t, dev, h)

    def mel_to_magnitude(self, mel, lengths=None):
        """log-mel [B, n_mel, F] (what ``mel`` makes) -> max(pinv(mel_basis) . exp(mel), 0) [B, cutoff, F], zeros at and behind
        lengths[b] frames: this build's own mel inversion (include/facppg.h)."""
        what = "mel_to_magnitude"
        _lib.require_cuda(mel, what + ": mel")
        if self._mel_basis_np is None:
            raise _lib.FacppgError("mel_to_magnitude: this STFT was built without a mel basis")
        x = mel.float().contiguous()
        if x.dim() != 3 or x.shape[1] != self._mel_basis_np.shape[0]:
            raise _lib.FacppgError("%s: mel must be [B, %d, F]" % (what, self._mel_basis_np.shape[0]))
        B, n_mel, F = x.shape
        dev = x.device
        lt = None
        if lengths is not None:
            if torch.is_tensor(lengths):
                lt = lengths.to(device=dev, dtype=torch.int32).contiguous()
                ok = lt.numel() == B
            else:
                ok = len(lengths) == B and 0 <= min(int(n) for n in lengths) and max(int(n) for n in lengths) <= F
                lt = _lib.upload([int(n) for n in lengths], torch.int32, dev) if ok else None
            if not ok:
                raise _lib.FacppgError("%s: lengths must be B frame counts <= F" % what)
        h = self._handle(dev)
        self._mel_pinv(h, dev)
        ws = self._gl_workspace(h, dev, B, F)
        out = torch.empty(B, self.filter_length // 2 + 1, F, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_mel_to_magnitude(h, _lib.ptr(x), _lib.ptr(lt), B, F, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                           _lib.current_stream(dev)))
        return out

    def denoise(self, audio, bias_spec, strength, lengths=None):
        """Spectral subtraction (Denoiser.forward) fused: [B, N] -> [B, 1, hop*(N//hop)]."""
        _lib.require_cuda(audio, "Denoiser: audio")
        x = audio.float().contiguous()
        B, N = x.shape
        dev = x.device
        h = self._handle(dev)
        ws = self._workspace(h, dev, B, N)
        bias = bias_spec.to(dev).float().reshape(-1).contiguous()
        n_out = self.hop_length * (N // self.hop_length)
        out = torch.zeros(B, 1, n_out, device=dev) if lengths is not None else torch.empty(B, 1, n_out, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().facppg_denoise(h, _lib.ptr(x), _lib.ptr(self._lengths(lengths, B, N, dev)), _lib.ptr(bias),
                                                  float(strength), B, N, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                  _lib.current_stream(dev)))
        return out
