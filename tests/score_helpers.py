"""Shared by test_ppg_dtw_cpu.py and test_gpu_ppg_dtw.py: the inputs, the float64 reference of facppg_ppg_dtw's definition
(include/facppg.h) in plain NumPy loops, its float32 restatement, and the cost tolerance derived from the two.

Every result is computed once per process and kept (the GPU tests read what the CPU test computed when both run in one session)."""
import functools

import numpy as np

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 130), (257, 300))
DIMS = (1, 40, 256)
BANDS = (0, 2, 40)
MATRIX = tuple((Ta, Tb, D, band) for Ta, Tb in SHAPES for D in DIMS for band in BANDS)


def make(Ta, Tb, D, seed):
    r = np.random.RandomState(seed)
    z = 3.0 * r.randn(D, Ta); a = np.exp(z - z.max(0)); a /= a.sum(0)
    idx = np.minimum((np.linspace(0, 1, Tb) ** 1.3 * (Ta - 1) + 0.5).astype(int), Ta - 1) if Ta > 1 else np.zeros(Tb, int)
    zb = np.log(a[:, idx] + 1e-12) + 0.7 * r.randn(D, Tb); b = np.exp(zb - zb.max(0)); b /= b.sum(0)
    return a.astype(np.float32), b.astype(np.float32)     # seed = 1000 + 7*Ta + Tb + D


def seed_of(Ta, Tb, D):
    return 1000 + 7 * Ta + Tb + D


@functools.lru_cache(maxsize=None)
def inputs(Ta, Tb, D):
    return make(Ta, Tb, D, seed_of(Ta, Tb, D))


def admissible(Ta, Tb, band):
    """[Ta, Tb] bool: band == 0 or |i (Tb - 1) - j (Ta - 1)| <= band * max(Ta - 1, Tb - 1, 1), in 64-bit integers."""
    if band == 0:
        return np.ones((Ta, Tb), dtype=bool)
    i = np.arange(Ta, dtype=np.int64)[:, None]
    j = np.arange(Tb, dtype=np.int64)[None, :]
    return np.abs(i * (Tb - 1) - j * (Ta - 1)) <= np.int64(band) * max(Ta - 1, Tb - 1, 1)


def local_distance(a, b, dtype):
    """d [Ta, Tb] in ``dtype``: square roots, products and the sum over k (k increasing, one accumulator) all in that type."""
    ra = np.sqrt(np.maximum(a.astype(dtype), dtype(0)))
    rb = np.sqrt(np.maximum(b.astype(dtype), dtype(0)))
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=dtype)
    for k in range(a.shape[0]):
        acc = acc + ra[k][:, None] * rb[k][None, :]
    assert acc.dtype == dtype
    return np.maximum(dtype(0), dtype(1) - acc)


def reference(a, b, band=0, dtype=np.float64):
    """(cost, steps, agree) of a [D, Ta] against b [D, Tb] by the definition, every sum in ``dtype``."""
    Ta, Tb = a.shape[1], b.shape[1]
    d = local_distance(a, b, dtype)
    ok = admissible(Ta, Tb, band).tolist()
    same = (np.argmax(a, axis=0)[:, None] == np.argmax(b, axis=0)[None, :]).tolist()   # argmax: the lowest k on a tie
    d = [[dtype(v) for v in row] for row in d]
    C = [[None] * Tb for _ in range(Ta)]
    N = [[0] * Tb for _ in range(Ta)]
    M = [[0] * Tb for _ in range(Ta)]
    inf = dtype(np.inf)
    for i in range(Ta):
        for j in range(Tb):
            if not ok[i][j]:
                continue
            if i == 0 and j == 0:
                C[0][0], N[0][0], M[0][0] = d[0][0], 1, int(same[0][0])
                continue
            best, pred = inf, None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pi >= 0 and pj >= 0 and ok[pi][pj] and C[pi][pj] is not None and (pred is None or C[pi][pj] < best):
                    best, pred = C[pi][pj], (pi, pj)
            if pred is None:            # an admissible cell no admissible path reaches
                continue
            C[i][j] = d[i][j] + best
            N[i][j] = N[pred[0]][pred[1]] + 1
            M[i][j] = M[pred[0]][pred[1]] + int(same[i][j])
    assert C[Ta - 1][Tb - 1] is not None, "no admissible path"
    assert type(C[Ta - 1][Tb - 1]) is dtype
    return float(C[Ta - 1][Tb - 1]), N[Ta - 1][Tb - 1], M[Ta - 1][Tb - 1]


@functools.lru_cache(maxsize=None)
def case(Ta, Tb, D, band):
    """One case of the matrix -> (float64 reference, float32 restatement), each (cost, steps, agree)."""
    a, b = inputs(Ta, Tb, D)
    return reference(a, b, band, np.float64), reference(a, b, band, np.float32)


@functools.lru_cache(maxsize=None)
def emulation_deviation():
    """The float32 restatement's worst deviation from float64 per path cell, over the matrix: max |cost32 - cost64| / steps."""
    return max(abs(r32[0] - r64[0]) / r64[1] for r64, r32 in (case(*c) for c in MATRIX))


def cost_tolerance():
    """Per path cell: 4 x the float32 restatement's own worst deviation -- the device sums k with fused multiply-adds and may
    take another order."""
    return 4.0 * emulation_deviation()
