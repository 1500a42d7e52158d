"""Shared by test_align_cpu.py, test_gpu_align.py and test_gpu_phone_report.py: the inputs, the reference of the definition of
facppg_ppg_emissions / facppg_ppg_decode_phones / facppg_ppg_force_align (include/facppg.h) in NumPy -- a loop over the frames,
every operation of a frame elementwise in ONE type, so float64 is the reference and float32 its restatement (every add rounded on
its own, as the kernels round theirs) --, and the tolerances derived from the two.

Every result is computed once per process and kept."""
import functools

import numpy as np

FRAMES = (1, 2, 7, 63, 64, 65, 150, 600)
DIMS_CPU = (3, 40)
DIMS_GPU = (3, 40, 256)                 # the decode on both sides of its single-wave cut
EMIT_DIMS = (1, 3, 40, 256)
EMIT_FRAMES = (1, 63, 64, 65, 257)
SWITCH_COST = 2.0
FLOOR = 1e-10


def seed_of(T, D):
    return 1000 + 7 * T + D


def make(T, D, seed):
    """[D, T] float32 posteriors: runs of 1 - 12 frames of a random class; a frame's logits are randn(D) with +4.0 on the run's
    class, then a softmax, then the cast.  Per run the draws are: its length, its class, its logits as one [D, length] block (x's
    own layout; a run cut by T still draws its whole block).  The self-consistency that test_align_cpu.py asserts -- x aligned
    to its own decoded runs gives the runs back, and the two costs differ by the switches to within 5e-13, a few float64 ulps of
    a cost of several hundred -- is a condition on the inputs: it holds for this draw order and these seeds, and another order
    may round a case an ulp past it."""
    r = np.random.RandomState(seed)
    x = np.empty((D, T), dtype=np.float64)
    t = 0
    while t < T:
        n, k = int(r.randint(1, 13)), int(r.randint(D))
        m = min(n, T - t)
        z = r.randn(D, n)[:, :m].copy()
        z[k] += 4.0
        p = np.exp(z - z.max(axis=0))
        x[:, t:t + m] = p / p.sum(axis=0)
        t += m
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(T, D):
    return make(T, D, seed_of(T, D))


def emissions(x, floor=FLOOR, dtype=np.float64):
    """x [D, T] -> (em [T, D], eb [T], top [T]) in ``dtype``: em = -log(max(x, floor)), its minimum per frame, arg max_k x (the lowest
    k on a tie)."""
    em = -np.log(np.maximum(x.T.astype(dtype), dtype(floor)))
    assert em.dtype == dtype
    return np.ascontiguousarray(em), em.min(axis=1), np.argmax(x, axis=0).astype(np.int32)


def decode(em, switch_cost=SWITCH_COST):
    """The phone loop over em [T, D], in em's type -> (labels int32 [T], cost)."""
    dtype = em.dtype.type
    T, D = em.shape
    sc = dtype(switch_cost)
    own = np.arange(D)
    C = em[0].copy()
    bp = np.zeros((T, D), dtype=np.int64)
    for t in range(1, T):
        j = int(np.argmin(C))                # the first minimum
        sw = C[j] + sc
        leave = sw < C                       # strict: a tie stays
        C = em[t] + np.where(leave, sw, C)
        bp[t] = np.where(leave, j, own)
        assert C.dtype == em.dtype
    at = int(np.argmin(C))
    cost = C[at]
    labels = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        labels[t] = at
        if t > 0:
            at = int(bp[t][at])
    return labels, cost


def runs_of(labels):
    """labels [T] -> [(class, start, frames)]."""
    out = []
    for t, k in enumerate(np.asarray(labels).tolist()):
        if out and out[-1][0] == k:
            out[-1][2] += 1
        else:
            out.append([k, t, 1])
    return [tuple(r) for r in out]


def align(em, eb, top, seq, optional=None):
    """The forced alignment of em [T, D] (with eb, top of its frames) to the states ``seq`` with the flags ``optional``, in em's
    type -> dict(start, frames, hits int32 [S], gop [S], cost, ok)."""
    dtype = em.dtype.type
    T = em.shape[0]
    seq = np.asarray(seq, dtype=np.int64)
    S = len(seq)
    opt = np.zeros(S, dtype=bool) if optional is None else np.asarray(optional) != 0
    inf = dtype(np.inf)
    may_skip = np.zeros(S, dtype=bool)
    may_skip[2:] = opt[1:S - 1]              # state s may be entered from s - 2 when s - 1 is optional
    C = np.full(S, inf, dtype=em.dtype)
    C[0] = em[0][seq[0]]
    if opt[0] and S > 1:
        C[1] = em[0][seq[1]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        c1 = np.concatenate([[inf], C[:-1]]).astype(em.dtype)
        c2 = np.where(may_skip, np.concatenate([[inf, inf], C[:-2]])[:S], inf).astype(em.dtype)
        best, frm = C, np.zeros(S, dtype=np.int8)
        adv = c1 < best                      # stay, advance, skip in that order, strict <
        best, frm = np.where(adv, c1, best), np.where(adv, 1, frm)
        skp = c2 < best
        best, frm = np.where(skp, c2, best), np.where(skp, 2, frm)
        C = best + em[t][seq]
        bp[t] = frm
        assert C.dtype == em.dtype
    at = S - 1
    if S >= 2 and opt[S - 1] and C[S - 2] < C[S - 1]:
        at = S - 2
    cost = C[at]
    start, frames = np.full(S, -1, dtype=np.int32), np.zeros(S, dtype=np.int32)
    hits, gop = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=em.dtype)
    ok = bool(cost < inf)
    if ok:
        for t in range(T - 1, -1, -1):
            start[at] = t
            frames[at] += 1
            if t > 0:
                at -= int(bp[t][at])
        assert at == 0 or (at == 1 and opt[0])
        for s in range(S):
            if frames[s]:
                acc = dtype(0)
                for t in range(start[s], start[s] + frames[s]):      # in frame order
                    acc = acc + (eb[t] - em[t][seq[s]])
                    hits[s] += int(top[t] == seq[s])
                gop[s] = acc / dtype(frames[s])
    return {"start": start, "frames": frames, "hits": hits, "gop": gop, "cost": cost, "ok": ok}


@functools.lru_cache(maxsize=None)
def case(T, D):
    """One case of the matrix, in float64 and float32: the decode of x, and x force-aligned to its own decoded runs (no optional
    state) -> {dtype: (labels, decode cost, alignment)}."""
    x = inputs(T, D)
    out = {}
    for dtype in (np.float64, np.float32):
        em, eb, top = emissions(x, FLOOR, dtype)
        labels, cost = decode(em)
        out[dtype] = (labels, cost, align(em, eb, top, [r[0] for r in runs_of(labels)]))
    return out


@functools.lru_cache(maxsize=None)
def emission_deviation():
    """NumPy's own float32 -log against float64, over the emission matrix: the worst |em32 - em64| / max(1, |em64|)."""
    worst = 0.0
    for D in EMIT_DIMS:
        for T in EMIT_FRAMES:
            e64, e32 = emissions(inputs(T, D))[0], emissions(inputs(T, D), FLOOR, np.float32)[0]
            worst = max(worst, float(np.max(np.abs(e32.astype(np.float64) - e64) / np.maximum(1.0, np.abs(e64)))))
    return worst


def emission_tolerance():
    """4 x the float32 restatement's own deviation: the device's logf may round differently."""
    return 4.0 * emission_deviation()


@functools.lru_cache(maxsize=None)
def cost_deviation_per_frame():
    """The float32 restatement's worst deviation of a cost (decode or alignment) from float64 per frame, over the matrix."""
    worst = 0.0
    for D in DIMS_GPU:
        for T in FRAMES:
            c = case(T, D)
            worst = max(worst, abs(float(c[np.float32][1]) - float(c[np.float64][1])) / T,
                        abs(float(c[np.float32][2]["cost"]) - float(c[np.float64][2]["cost"])) / T)
    return worst


def cost_tolerance(T):
    """A device cost of T frames against the float64 one: the emission tolerance times the frame count plus the restatement's own
    deviation (its worst per frame over the matrix, times T)."""
    return emission_tolerance() * T + cost_deviation_per_frame() * T


# ---- hand cases of the forced alignment: (name, x [D, T], seq, optional, expected) with expected a dict of what must hold ----

def peaked(classes, D, hot=0.9):
    """x [D, T]: frame t has ``hot`` on classes[t] and the rest spread evenly."""
    T = len(classes)
    x = np.full((D, T), (1.0 - hot) / (D - 1), dtype=np.float32)
    x[np.asarray(classes), np.arange(T)] = hot
    return x


def hand_cases():
    cases = []
    # one state takes every frame
    cases.append(("S = 1", peaked([2, 2, 0, 1, 2], 3), [2], [0], dict(start=[0], frames=[5], hits=[3], ok=True)))
    # as many mandatory states as frames: one frame each
    cls = [0, 1, 2, 0, 1, 1, 2]
    cases.append(("S = T", peaked(cls, 3), cls, [0] * 7, dict(start=list(range(7)), frames=[1] * 7, hits=[1] * 7, gop=[0.0] * 7, ok=True)))
    # one more state than frames, one of them optional: it must be skipped
    cases.append(("S = T + 1, one optional", peaked([0, 1, 0, 1], 3), [0, 1, 2, 0, 1], [0, 0, 1, 0, 0],
                  dict(start=[0, 1, -1, 2, 3], frames=[1, 1, 0, 1, 1], hits=[1, 1, 0, 1, 1], ok=True)))
    # more mandatory states than frames: no path
    cases.append(("mandatory = T + 1", peaked([0, 1, 0], 3), [0, 1, 0, 1], [0, 0, 0, 0],
                  dict(start=[-1] * 4, frames=[0] * 4, hits=[0] * 4, gop=[0.0] * 4, ok=False)))
    # optional first and last states: the first and last frames choose by cost -- taken where the frame is silence, skipped where not
    cases.append(("optional ends, both taken", peaked([2, 0, 1, 2], 3), [2, 0, 1, 2], [1, 0, 0, 1],
                  dict(start=[0, 1, 2, 3], frames=[1, 1, 1, 1], ok=True)))
    cases.append(("optional ends, both skipped", peaked([0, 0, 1, 1], 3), [2, 0, 1, 2], [1, 0, 0, 1],
                  dict(start=[-1, 0, 2, -1], frames=[0, 2, 2, 0], ok=True)))
    cases.append(("optional ends, first taken", peaked([2, 0, 1, 1], 3), [2, 0, 1, 2], [1, 0, 0, 1],
                  dict(start=[0, 1, 2, -1], frames=[1, 1, 2, 0], ok=True)))
    # two equal adjacent classes: at the last frame stay and advance tie exactly, and stay is tried first -- the second state
    # keeps the frames from 1 on (advance-before-stay would give frames [2, 1])
    cases.append(("tie: stay before advance", peaked([1, 1, 1], 3), [1, 1], [0, 0], dict(start=[0, 1], frames=[1, 2], ok=True)))
    # a single frame with an optional first state: state 1 may start
    cases.append(("T = 1, optional first", peaked([0], 3), [2, 0], [1, 0], dict(start=[-1, 0], frames=[0, 1], ok=True)))
    return cases


@functools.lru_cache(maxsize=None)
def long_case(S, T=1030, D=40):
    """x of T frames and a sequence of S states for it: the classes of x's decoded runs, repeated or cut to S, every fourth state
    optional (never two in a row)."""
    x = make(T, D, seed_of(T, D))
    classes = [r[0] for r in runs_of(decode(emissions(x)[0])[0])]
    seq = [classes[i % len(classes)] for i in range(S)]
    return x, seq, [1 if i % 4 == 3 else 0 for i in range(S)]


def check_expected(name, got, want):
    for key, value in want.items():
        if key == "ok":
            assert bool(got["ok"]) == value, (name, key, got["ok"])
        elif key == "gop":
            assert np.asarray(got[key], dtype=np.float64).tolist() == value, (name, key, got[key])
        else:
            assert np.asarray(got[key]).tolist() == value, (name, key, np.asarray(got[key]).tolist(), value)
