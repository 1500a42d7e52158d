"""NumPy restatements shared by the long-form tests (tests/test_gpu_longform_kernels.py, tests/test_gpu_longform.py): float32
throughout, the operations of the kernels in their order, so that equality is exact."""
import numpy as np


def flag_sums(x, rows):
    """x [B, K, T] float32 -> the pause mass [B, T]: ONE float32 accumulator, the rows added in the order given."""
    acc = x[:, rows[0], :].copy()
    for r in rows[1:]:
        acc = acc + x[:, r, :]
    assert acc.dtype == np.float32
    return acc


def pause_flags(x, lengths, rows, threshold):
    t = np.arange(x.shape[2])[None, :]
    return ((t < np.asarray(lengths)[:, None]) & (flag_sums(x, rows) > np.float32(threshold))).astype(np.uint8)


def seam_fades(n, fade):
    """f_s = min(fade, n_s // 2) rounded down to a power of two, or 0 (restated here, not imported from the product)."""
    out = []
    for v in n:
        f, p = min(int(fade), int(v) // 2), 1
        while p * 2 <= f:
            p *= 2
        out.append(p if f >= 1 else 0)
    return out


def join(segments, fade):
    """list of float32 [n_s] -> their concatenation with the linear fades on both sides of every interior seam: gain
    (2 i + 1) / (2 f_s) over the first f_s samples of segments s > 0, mirrored over the last f_s of segments s < S - 1."""
    n = [len(a) for a in segments]
    S, parts = len(n), []
    for s, f in enumerate(seam_fades(n, fade)):
        seg = np.array(segments[s], dtype=np.float32, copy=True)
        if f:
            gain = (2 * np.arange(f) + 1).astype(np.float32) / np.float32(2 * f)
            if s > 0:
                seg[:f] = seg[:f] * gain
            if s < S - 1:
                seg[n[s] - f:] = seg[n[s] - f:] * gain[::-1]
        parts.append(seg)
    out = np.concatenate(parts)
    assert out.dtype == np.float32
    return out
