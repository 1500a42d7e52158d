"""The F0 tracker of include/facppg.h restated in NumPy, for test_f0_cpu.py and test_gpu_f0.py:

  nccf(x, dtype)        phi [T, L + 2] by the definition, float64 (the reference) or float32 (products and sums in NumPy float32:
                        what an fp32 evaluation in ANOTHER order gives -- its deviation from float64 sets the kernel's tolerance)
  track(phi, dtype)     the Viterbi pass, backtrace and refinement with the stated operation order: float32 is the definition (the
                        kernel's integers must equal it), float64 the same recurrence without rounding questions
  tone, vibrato_burst_silence, white_noise, dc_silence     seeded signals, rounded to integers in the int16 range
  NCCF_CASES, nccf_cases(), nccf_tolerance()               the sample counts of the GPU test, their signals, and 4 x the float32
                        restatement's worst deviation from float64 over exactly those signals (computed, never a constant)
Nothing here touches a device."""
import functools

import numpy as np

FS, S, W, LAG_MIN, LAG_MAX = 16000, 160, 320, 40, 334
L = LAG_MAX - LAG_MIN + 1
BALLAST, VOICING_COST, FREQ_WEIGHT = 50.0, 0.2, 2.0
TONES = (55.0, 60.0, 110.0, 220.0, 380.0)
NCCF_CASES = (80, 81, 240, 653, 654, 1600, 4801)


def num_frames(n):
    return (n + S // 2) // S


def tables():
    """wl [L], g [L] as float32 (computed in float64, rounded once)."""
    lags = np.arange(LAG_MIN, LAG_MAX + 1, dtype=np.float64)
    return (1.0 - 0.3 * lags / LAG_MAX).astype(np.float32), np.log2(lags).astype(np.float32)


def nccf(x, dtype=np.float64):
    """phi(t, l), l = LAG_MIN - 1 .. LAG_MAX + 1, for the T = num_frames(len(x)) frames of x; samples outside [0, n) are 0."""
    x = np.asarray(x, dtype=dtype)
    n = len(x)
    T = num_frames(n)
    half = (W + LAG_MAX + 1) // 2
    reach = W + LAG_MAX + 1                                  # samples a frame reads: a .. a + reach - 1
    front = half                                             # a(0) = S / 2 - half >= -half
    pad = np.zeros(front + max(n, (T - 1) * S + S // 2 - half + reach) + reach, dtype)
    pad[front:front + n] = x
    sq = pad * pad
    ball = dtype((W * BALLAST ** 2) ** 2)
    phi = np.zeros((T, L + 2), dtype)
    lags = np.arange(LAG_MIN - 1, LAG_MAX + 2)
    for t in range(T):
        a = t * S + S // 2 - half + front
        seg = pad[a:a + reach]
        rows = np.lib.stride_tricks.sliding_window_view(seg, W)[lags]          # [L + 2, W]: x[a + l + j]
        dot = rows @ seg[:W]
        e0 = sq[a:a + W].sum(dtype=dtype)
        el = np.lib.stride_tricks.sliding_window_view(sq[a:a + reach], W)[lags].sum(axis=1, dtype=dtype)
        phi[t] = dot / np.sqrt(e0 * el + ball)
    return phi


def track(phi, dtype=np.float32, voicing_cost=VOICING_COST, freq_weight=FREQ_WEIGHT, sample_rate=FS):
    """phi [T, L + 2] -> (lag [T] int, 0 = unvoiced; f0 [T] in ``dtype``).  Every product and sum is one NumPy operation in ``dtype``."""
    dt = dtype
    phi = np.asarray(phi).astype(dt)
    T = phi.shape[0]
    wl, g = (a.astype(dt) for a in tables())
    mid, below, above = phi[:, 1:-1], phi[:, :-2], phi[:, 2:]
    peak = (mid >= below) & (mid > above)
    dv = np.where(peak, dt(1) - mid * wl, dt(np.inf)).astype(dt)            # [T, L]
    du = mid.max(axis=1)
    trans = (dt(freq_weight) * np.abs(g[:, None] - g[None, :])).astype(dt)   # [to l, from l']
    vuv = dt(voicing_cost)
    C = np.concatenate([[du[0]], dv[0]]).astype(dt)
    bp = np.zeros((T, L + 1), np.int64)
    for t in range(1, T):
        into_u = np.concatenate([[C[0]], C[1:] + vuv]).astype(dt)
        b0 = int(np.argmin(into_u))                          # the first minimum: s' increasing, strict <
        into_l = np.concatenate([np.full((L, 1), C[0] + vuv, dt), C[1:][None, :] + trans], axis=1).astype(dt)
        b = np.argmin(into_l, axis=1)
        bp[t, 0], bp[t, 1:] = b0, b
        C = np.concatenate([[into_u[b0] + du[t]], into_l[np.arange(L), b] + dv[t]]).astype(dt)
    s = int(np.argmin(C))
    lag, f0 = np.zeros(T, np.int64), np.zeros(T, dt)
    for t in range(T - 1, -1, -1):
        if s:
            p, q, r = phi[t, s - 1], phi[t, s], phi[t, s + 1]
            den = (p - (q + q)) + r
            delta = dt(0.5) * (p - r) / den if den < 0 else dt(0)
            lag[t] = LAG_MIN + s - 1
            f0[t] = dt(sample_rate) / (dt(lag[t]) + delta)
        s = int(bp[t, s])
    return lag, f0


def reference_f0(x):
    """The float64 reference end to end: (lag, f0) of a signal."""
    return track(nccf(x, np.float64), np.float64)


def _int16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.float64)


def tone(f0, n, seed=0, amplitude=3000.0, noise=20.0):
    """Eight harmonics of f0 with amplitudes 1 / k and a little white noise."""
    r = np.random.RandomState(seed)
    ph = 2.0 * np.pi * f0 * np.arange(n) / FS
    return _int16(amplitude * sum(np.sin(k * ph) / k for k in range(1, 9)) + noise * r.randn(n))


def vibrato_burst_silence(n, seed=0):
    """In every 0.8 s: 0.5 s of a harmonic tone whose F0 swings around 120 Hz + 15 seed, 0.15 s of noise, 0.15 s of near silence."""
    r = np.random.RandomState(seed)
    t = np.arange(n) / FS
    f = 120.0 + 60.0 * np.sin(2.0 * np.pi * 0.7 * t) + 15.0 * seed
    ph = 2.0 * np.pi * np.cumsum(f) / FS
    voiced = (t % 0.8) < 0.5
    burst = ((t % 0.8) >= 0.5) & ((t % 0.8) < 0.65)
    x = np.where(voiced, 3000.0 * sum(np.sin(k * ph) / k for k in range(1, 9)), 0.0)
    return _int16(x + np.where(burst, 1500.0 * r.randn(n), 0.0) + 20.0 * r.randn(n))


def white_noise(n, seed=0, amplitude=2000.0):
    return _int16(amplitude * np.random.RandomState(seed).randn(n))


def dc_silence(n, dc=30.0):
    return np.full(n, float(dc))


def silence(n):
    return np.zeros(n)


@functools.lru_cache(maxsize=None)
def nccf_cases():
    """One signal per sample count of NCCF_CASES (read-only): tones for the shortest, then mixtures and noise."""
    makers = (lambda n: tone(220.0, n, 1), lambda n: tone(110.0, n, 2), lambda n: white_noise(n, 3), lambda n: tone(150.0, n, 4),
              lambda n: vibrato_burst_silence(n, 1)[::-1].copy(), lambda n: white_noise(n, 5, 300.0) + dc_silence(n), vibrato_burst_silence)
    out = []
    for n, make in zip(NCCF_CASES, makers):
        x = make(n)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nccf_references():
    """(float64 phi, float32-restatement phi) per case, computed once."""
    return tuple((nccf(x, np.float64), nccf(x, np.float32)) for x in nccf_cases())


def emulation_deviation():
    return max(float(np.abs(p32.astype(np.float64) - p64).max()) for p64, p32 in nccf_references())


def nccf_tolerance():
    """4 x the float32 restatement's worst deviation from float64 over the cases of the GPU test."""
    return 4.0 * emulation_deviation()


def ulp_distance(a, b):
    """Units in the last place between two float32 arrays of equal sign."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
