"""Shared by test_mel_dtw_cpu.py, test_gpu_mel_dtw.py and test_gpu_free_running.py: the inputs, the float64 reference of
facppg_mel_dtw's and facppg_attention_path's definitions (include/facppg.h) in plain loops, a float32 restatement of mel_dtw, and
the cost tolerance derived from the two.

Every result is computed once per process and kept (the GPU tests read what the CPU test computed when both run in one session)."""
import functools
import math

import numpy as np

from score_helpers import admissible

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 130), (257, 300))
DIMS = ((80, 13), (80, 64), (2, 1))           # (mel channels M, cepstral coefficients K)
BANDS = (0, 2, 40)
MATRIX = tuple((Ta, Tb, M, K, band) for Ta, Tb in SHAPES for M, K in DIMS for band in BANDS)
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)
LOG_FLOOR = math.log(1e-5)

# a case whose float32 restatement takes another path than float64 gets another seed here (never another comparison)
SEED_OVERRIDES = {}


def seed_of(Ta, Tb, M):
    return SEED_OVERRIDES.get((Ta, Tb, M), 2000 + 7 * Ta + Tb + M)


def make(Ta, Tb, M, seed):
    """a [M, Ta]: random natural-log mels in [ln 1e-5, 1], smooth over the channels (a moving average over 5 of them); b [M, Tb]: a
    time-warped copy (score_helpers.make's warp) plus noise, clipped to the same range."""
    r = np.random.RandomState(seed)
    z = r.randn(M + 4, Ta)
    smooth = sum(z[k:k + M] for k in range(5)) / math.sqrt(5.0)
    a = np.clip(-5.0 + 3.0 * smooth + 1.5 * r.randn(1, Ta), LOG_FLOOR, 1.0)
    idx = np.minimum((np.linspace(0, 1, Tb) ** 1.3 * (Ta - 1) + 0.5).astype(int), Ta - 1) if Ta > 1 else np.zeros(Tb, int)
    b = np.clip(a[:, idx] + 0.3 * r.randn(M, Tb), LOG_FLOOR, 1.0)
    return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(Ta, Tb, M):
    return make(Ta, Tb, M, seed_of(Ta, Tb, M))


@functools.lru_cache(maxsize=None)
def basis(M, K):
    """float32 [K, M]: rows k = 1 .. K of the orthonormal DCT-II, in float64 and rounded once (what cepstral_basis must return)."""
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return (math.sqrt(2.0 / M) * np.cos(math.pi * k * (m + 0.5) / M)).astype(np.float32)


def project(x, bas, dtype):
    """c [K, T] in ``dtype``: one accumulator per (k, t), m increasing; products and sums rounded in that type."""
    x, bas = x.astype(dtype), bas.astype(dtype)
    c = np.zeros((bas.shape[0], x.shape[1]), dtype=dtype)
    for m in range(x.shape[0]):
        c = c + bas[:, m][:, None] * x[m][None, :]
    assert c.dtype == dtype
    return c


def local_distance(a, b, bas, dtype):
    """d [Ta, Tb] in ``dtype``: direct differences of the cepstra, squares summed with k increasing (one accumulator), square root."""
    ca, cb = project(a, bas, dtype), project(b, bas, dtype)
    s = np.zeros((a.shape[1], b.shape[1]), dtype=dtype)
    for k in range(bas.shape[0]):
        diff = ca[k][:, None] - cb[k][None, :]
        s = s + diff * diff
    assert s.dtype == dtype
    return np.sqrt(s)


def sweep(d, band, dtype):
    """(cost, steps) over the distances d [Ta, Tb] by facppg_ppg_dtw's recurrence, every sum in ``dtype``."""
    Ta, Tb = d.shape
    ok = admissible(Ta, Tb, band).tolist()
    d = [[dtype(v) for v in row] for row in d]
    C = [[None] * Tb for _ in range(Ta)]
    N = [[0] * Tb for _ in range(Ta)]
    inf = dtype(np.inf)
    for i in range(Ta):
        for j in range(Tb):
            if not ok[i][j]:
                continue
            if i == 0 and j == 0:
                C[0][0], N[0][0] = d[0][0], 1
                continue
            best, pred = inf, None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pi >= 0 and pj >= 0 and ok[pi][pj] and C[pi][pj] is not None and (pred is None or C[pi][pj] < best):
                    best, pred = C[pi][pj], (pi, pj)
            if pred is None:            # an admissible cell no admissible path reaches
                continue
            C[i][j] = d[i][j] + best
            N[i][j] = N[pred[0]][pred[1]] + 1
    assert C[Ta - 1][Tb - 1] is not None, "no admissible path"
    assert type(C[Ta - 1][Tb - 1]) is dtype
    return float(C[Ta - 1][Tb - 1]), N[Ta - 1][Tb - 1]


def reference(a, b, bas, band=0, dtype=np.float64):
    """(cost, steps) of a [M, Ta] against b [M, Tb] by the definition, every product and sum in ``dtype``."""
    return sweep(local_distance(a, b, bas, dtype), band, dtype)


@functools.lru_cache(maxsize=None)
def _distances(Ta, Tb, M, K):
    a, b = inputs(Ta, Tb, M)
    return local_distance(a, b, basis(M, K), np.float64), local_distance(a, b, basis(M, K), np.float32)


@functools.lru_cache(maxsize=None)
def case(Ta, Tb, M, K, band):
    """One case of the matrix -> (float64 reference, float32 restatement), each (cost, steps)."""
    d64, d32 = _distances(Ta, Tb, M, K)
    return sweep(d64, band, np.float64), sweep(d32, band, np.float32)


@functools.lru_cache(maxsize=None)
def emulation_deviation():
    """The float32 restatement's worst deviation from float64 per path cell, over the matrix: max |cost32 - cost64| / steps."""
    return max(abs(r32[0] - r64[0]) / r64[1] for r64, r32 in (case(*c) for c in MATRIX))


def cost_tolerance():
    """Per path cell: 4 x the float32 restatement's own worst deviation -- the device sums with fused multiply-adds, where NumPy
    rounds every product (score_helpers.cost_tolerance's rule)."""
    return 4.0 * emulation_deviation()


def attention_reference(A, T, L):
    """facppg_attention_path's definition in plain loops: A [>= T, >= L] -> ([first, last, back, max_jump, longest_stall, visited],
    focus), focus the float64 mean of the row maxima rounded to float32 once."""
    pos, w = [], []
    for t in range(T):
        best, arg = A[t][0], 0
        for j in range(1, L):
            if A[t][j] > best:
                best, arg = A[t][j], j
        pos.append(arg)
        w.append(float(best))
    back = sum(1 for t in range(1, T) if pos[t] < pos[t - 1])
    jump = max([0] + [pos[t] - pos[t - 1] for t in range(1, T)])
    stall = run = 1
    for t in range(1, T):
        run = run + 1 if pos[t] == pos[t - 1] else 1
        stall = max(stall, run)
    total = 0.0
    for v in w:
        total += v
    return [pos[0], pos[-1], back, jump, stall, len(set(pos))], np.float32(total / T)
