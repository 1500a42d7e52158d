"""NumPy restatement of the two definitions of the vocoder-free preview (include/facppg.h): the mel inversion
mag = max(P . exp(mel), 0) and Griffin-Lim with optional momentum over this build's own STFT / inverse STFT (reflect padding,
the windowed bases of common.stft.dft_bases, overlap-add with the window sum-square envelope, trim).  Every function takes the
dtype it computes in, so the same text runs in float64 (the yardstick) and in float32 (whose deviation from float64 sets the
tolerances of the device tests: a bound comes from the two restatements, never from the device).

The float32 run uses the float32 tables the library is given; the float64 run evaluates the same formulas in float64 (Tables).
The pseudo-inverse of the mel basis is the float32 table in both (the definition rounds it: include/facppg.h)."""
import functools

import numpy as np
from scipy.signal import get_window

from common.audio_processing import squared_window
from common.stft import dft_bases

TINY = 1.17549435e-38          # float32 tiny: the envelope threshold of k_overlap_add / stft.py:126

# (filter_length, hop, F)
SHAPES = ((64, 16, 3), (64, 16, 12), (64, 16, 40), (64, 32, 5), (1024, 256, 9), (1024, 160, 20))
SEEDS = (0, 1, 2)
# ragged batches: every utterance keeps hop * (F_b - 1) > filter_length / 2
RAGGED = ((64, 16, (40, 3, 17)), (1024, 256, (12, 9, 4)))


class Tables(object):
    """The transform's constants for (filter_length, hop) with a full-length hann window.  float32: the tables the library is
    given (dft_bases' float32 bases, the float32 squared window).  float64: the same formulas (common.stft.dft_bases) evaluated
    in float64 throughout, so that the float64 run is the definition itself and the float32 run carries the tables' rounding."""

    def __init__(self, fl, hop, dtype):
        self.fl, self.hop, self.cutoff, self.dtype = fl, hop, fl // 2 + 1, dtype
        if dtype == np.float32:
            self.fwd, self.inv = dft_bases(fl, hop, fl, 'hann')       # [fl + 2, fl] each
            self.win_sq = squared_window('hann', fl, fl).astype(np.float32)
            return
        ang = 2.0 * np.pi * np.outer(np.arange(self.cutoff), np.arange(fl)) / fl
        wc = np.full(self.cutoff, 2.0)
        wc[0] = wc[-1] = 1.0
        win = get_window('hann', fl, fftbins=True)
        self.fwd = np.vstack([np.cos(ang), -np.sin(ang)]) * win
        self.inv = np.vstack([np.cos(ang) * wc[:, None], -np.sin(ang) * wc[:, None]]) / (fl * (fl / hop)) * win
        self.win_sq = squared_window('hann', fl, fl).astype(np.float64)


@functools.lru_cache(maxsize=None)
def tables(fl, hop, dtype):
    return Tables(fl, hop, np.dtype(dtype).type)


def frames(t, y):
    """y [N] -> X [fl, N // hop + 1], reflect padding of fl / 2 at both ends.  Reflect padding proper needs N > fl / 2; the
    shape set's (64, 16, 3) has N = fl / 2 exactly, where the C entry point documents the framing kernel's clamped reflection:
    one reflection off each end, then a clamp into the utterance.  For N > fl / 2 the clamp never acts."""
    N = y.shape[0]
    F = N // t.hop + 1
    j = np.arange(t.fl)[:, None] + t.hop * np.arange(F)[None, :] - t.fl // 2
    j = np.abs(j)
    j = np.where(j >= N, 2 * (N - 1) - j, j)
    return y[np.clip(j, 0, N - 1)]


def stft(t, y):
    """y [N] -> S [2 * cutoff, F]: re rows, then im rows."""
    return t.fwd @ frames(t, y.astype(t.dtype))


def istft(t, S):
    """S [2 * cutoff, F] -> y [hop * (F - 1)]: overlap-add, sum-square normalisation where > tiny, * fl / hop, trim."""
    F = S.shape[1]
    Z = t.inv.T @ S.astype(t.dtype)                                   # [fl, F]
    total = t.fl + t.hop * (F - 1)
    acc = np.zeros(total, t.dtype)
    env = np.zeros(total, t.dtype)
    for f in range(F):
        acc[f * t.hop:f * t.hop + t.fl] += Z[:, f]
        env[f * t.hop:f * t.hop + t.fl] += t.win_sq
    nz = env > TINY
    acc[nz] /= env[nz]
    acc *= t.dtype(t.fl) / t.dtype(t.hop)
    return acc[t.fl // 2:t.fl // 2 + t.hop * (F - 1)]


def magnitude(S):
    c = S.shape[0] // 2
    return np.sqrt(S[:c] ** 2 + S[c:] ** 2)


def project(M, Y):
    """Pm(Y) = M . Y / |Y|; a bin with |Y| = 0 gives (M, 0)."""
    c = Y.shape[0] // 2
    mag = magnitude(Y)
    pos = mag > 0
    scale = np.where(pos, M / np.where(pos, mag, 1), 0).astype(Y.dtype)
    out = np.concatenate([Y[:c] * scale, Y[c:] * scale])
    out[:c][~pos] = M[~pos]
    return out


def convergence(M, T):
    """sc = || |T| - M ||_2 / || M ||_2 (0 where M = 0); T None: |T| := 0 (a call without iterations).  Always summed in float64."""
    M = M.astype(np.float64)
    d = M if T is None else magnitude(T.astype(np.float64)) - M
    den = float(np.sum(M * M))
    return float(np.sqrt(np.sum(d * d) / den)) if den > 0 else 0.0


def griffin_lim(fl, hop, M, phi0, n_iters, alpha, dtype):
    """One utterance: M, phi0 [cutoff, F] -> (signal [hop * (F - 1)], sc).  The loop of include/facppg.h, in ``dtype``."""
    t = tables(fl, hop, dtype)
    dt = t.dtype
    M = M.astype(dt)
    phi0 = phi0.astype(dt)
    c = np.concatenate([M * np.cos(phi0), M * np.sin(phi0)])
    prev = last = None
    for n in range(1, n_iters + 1):
        last = stft(t, istft(t, c))
        y = last if prev is None else last + dt(alpha) * (last - prev)
        c = project(M, y)
        prev = last
    return istft(t, c), convergence(M, last)


def signal_convergence(fl, hop, M, y):
    """float64 sc of a signal: || |STFT(y)| - M || / || M ||."""
    t = tables(fl, hop, np.float64)
    return convergence(M, stft(t, y.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def case(fl, hop, F, seed):
    """(signal [hop * (F - 1)] float64, M [cutoff, F] its float64 magnitudes, phi0 [cutoff, F] uniform in [-pi, pi), true phases):
    5 to 8 tones plus noise at 0.02 to 0.05."""
    g = np.random.Generator(np.random.PCG64(1000003 * fl + 1009 * hop + 17 * F + seed))
    N = hop * (F - 1)
    n = np.arange(N)
    y = np.zeros(N)
    for _ in range(int(g.integers(5, 9))):
        y += g.uniform(0.05, 0.2) * np.cos(2 * np.pi * g.uniform(0.01, 0.45) * n + g.uniform(0, 2 * np.pi))
    y += g.uniform(0.02, 0.05) * g.standard_normal(N)
    t = tables(fl, hop, np.float64)
    S = stft(t, y)
    c = fl // 2 + 1
    M = magnitude(S)
    phi0 = g.uniform(-np.pi, np.pi, size=M.shape)
    return y, M, phi0, np.arctan2(S[c:], S[:c])


def rel_err(a, ref):
    """max |a - ref| over the utterance's RMS."""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref)) / np.sqrt(np.mean(ref * ref)))


STEP_ITERS = (0, 1, 2)
ALPHAS = (0.0, 0.99)


@functools.lru_cache(maxsize=None)
def step_reference(fl, hop, F, seed, n_iters, alpha):
    """The float64 run of a steps case: (signal, sc)."""
    _, M, phi0, _ = case(fl, hop, F, seed)
    return griffin_lim(fl, hop, M, phi0, n_iters, alpha, np.float64)


@functools.lru_cache(maxsize=None)
def steps_tolerance():
    """4 x the largest deviation of the float32 restatement from the float64 one over the steps cases (every shape, seed,
    n_iters in {0, 1, 2}, alpha in {0, 0.99}), as max |f32 - f64| over the RMS of the float64 signal."""
    worst = 0.0
    for fl, hop, F in SHAPES:
        for seed in SEEDS:
            _, M, phi0, _ = case(fl, hop, F, seed)
            for n in STEP_ITERS:
                for a in ALPHAS:
                    if n < 2 and a != 0.0:          # (momentum enters at the second iteration: the same runs)
                        continue
                    y32, _ = griffin_lim(fl, hop, M, phi0, n, a, np.float32)
                    worst = max(worst, rel_err(y32, step_reference(fl, hop, F, seed, n, a)[0]))
    return 4.0 * worst


# ------------------------------------------------------------------ mel inversion
def mel_pinv(mel_basis):
    """P = pinv(mel_basis) [cutoff, n_mel] in float64."""
    return np.linalg.pinv(np.asarray(mel_basis, np.float64))


def mel_to_magnitude(P, mel, dtype):
    """max(P . exp(mel), 0) in ``dtype``; P is the float32 table the library holds, widened."""
    dt = np.dtype(dtype).type
    P = np.asarray(P, np.float64).astype(np.float32).astype(dt)
    return np.maximum(P @ np.exp(mel.astype(dt)), dt(0))


def triangular_basis(n_mel, cutoff):
    """A hand-built filterbank: n_mel overlapping triangles of unit height, evenly spaced over cutoff bins."""
    centres = np.linspace(0, cutoff - 1, n_mel + 2)
    bins = np.arange(cutoff)[None, :]
    up = (bins - centres[:-2, None]) / (centres[1:-1] - centres[:-2])[:, None]
    down = (centres[2:, None] - bins) / (centres[2:] - centres[1:-1])[:, None]
    return np.clip(np.minimum(up, down), 0.0, None)


def mel_case(mel_basis, F, seed):
    """A log-mel [n_mel, F] as TacotronSTFT.mel_spectrogram makes it from a tone-plus-noise magnitude (so about a tenth of the
    bins of its inversion clamp), float32 values."""
    g = np.random.Generator(np.random.PCG64(4242 + seed))
    cutoff = mel_basis.shape[1]
    mag = 0.02 * np.abs(g.standard_normal((cutoff, F)))
    for _ in range(6):
        k = int(g.integers(1, cutoff - 1))
        mag[k] += g.uniform(0.5, 3.0)
        mag[k - 1] += 0.3
        mag[k + 1] += 0.3
    return np.log(np.maximum(np.asarray(mel_basis, np.float64) @ mag, 1e-5)).astype(np.float32)
