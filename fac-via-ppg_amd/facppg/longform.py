"""Where a long recording is cut (facppg.pipeline.synthesize_long): host work on one byte per frame, integers only.

The reference converts one utterance of at most max_decoder_steps frames and cuts a longer one off (model.py:527,
generate_synthesis.py:90-93); it has nothing to restate here.  The flags come from facppg_ppg_pause_flags: 1 where the
pause classes of the PPG hold more than the threshold.
"""
import numpy as np

from facppg.lib import FacppgError


def check_plan_args(max_frames, min_frames, min_pause, what="plan_segments"):
    """plan_segments' refusals, for callers that want them before they have flags."""
    if int(min_frames) < 1:
        raise FacppgError("%s: min_frames must be at least 1 (got %r)" % (what, min_frames))
    if int(max_frames) < 2 * int(min_frames):
        raise FacppgError("%s: max_frames must be at least 2 * min_frames (got %r, min_frames %r)" % (what, max_frames, min_frames))
    if int(min_pause) < 1:
        raise FacppgError("%s: min_pause must be at least 1 (got %r)" % (what, min_pause))


def pause_runs(flags, min_pause):
    """The maximal runs [a, b) of set flags that are at least ``min_pause`` long, in order."""
    f = np.asarray(flags).reshape(-1) != 0
    edges = np.flatnonzero(np.diff(np.concatenate(([0], f.view(np.int8), [0]))))
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2]) if b - a >= min_pause]


def plan_segments(flags, max_frames, min_frames, min_pause):
    """flags [T] -> [(start, frames), ...]: segments that cover [0, T) in order, nothing dropped, nothing repeated.

    A pause run [a, b) offers the cut (a + b) // 2.  From s = 0, while more than ``max_frames`` are left: among the runs whose cut
    lies in [s + min_frames, min(s + max_frames, T - min_frames)] the longest wins, the later one on a tie; without one the cut is
    the window's upper end (a forced cut).  What is left is the last segment.  Every segment has 1 <= frames <= max_frames, and
    when there is more than one, every one has at least ``min_frames``: the window keeps min_frames on either side of a cut, and it
    is never empty (T - s > max_frames >= 2 * min_frames)."""
    check_plan_args(max_frames, min_frames, min_pause)
    max_frames, min_frames, min_pause = int(max_frames), int(min_frames), int(min_pause)
    T = int(np.asarray(flags).reshape(-1).shape[0])
    cuts = [((a + b) // 2, b - a) for a, b in pause_runs(flags, min_pause)]
    out, s = [], 0
    while T - s > max_frames:
        lo, hi = s + min_frames, min(s + max_frames, T - min_frames)
        cut, best = hi, 0
        for c, n in cuts:
            if lo <= c <= hi and n >= best:
                cut, best = c, n
        out.append((s, cut - s))
        s = cut
    if T > s:
        out.append((s, T - s))
    return out


def group_segments(frames, batch_frames):
    """Frame counts of the pooled segments -> [(first, end), ...]: each group the longest run of consecutive segments with
    count * longest <= batch_frames (the padded batch's columns), and at least one segment."""
    groups, i, n = [], 0, len(frames)
    while i < n:
        j, longest = i + 1, int(frames[i])
        while j < n and (j + 1 - i) * max(longest, int(frames[j])) <= batch_frames:
            longest = max(longest, int(frames[j]))
            j += 1
        groups.append((i, j))
        i = j
    return groups

