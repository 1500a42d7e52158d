"""Per-phone report of a conversion: which of the teacher's phones survived, where they landed and how well they are supported.

The reference has no counterpart on the wav -> wav path: its DataUtterance carries phone tiers and its align.py reads and writes
TextGrids that an external aligner produced from a transcript.  Here there is neither, and none is needed: the teacher is the
native speaker, so the phone sequence decoded from the teacher's own monophone PPG is the canonical one, and the converted
audio's PPG is force-aligned to it.  Both dynamic programs run on the device (include/facppg.h states the definition:
facppg_ppg_emissions, facppg_ppg_decode_phones, facppg_ppg_force_align) over the padded batch the front end wrote.

  decode_phones   the teacher's runs (class, start, frames) by a phone loop with a switch cost
  force_align     per state of a given sequence: start, frames, hits (frames whose top class is the phone) and gop, the mean of
                  log p(phone) - log p(best class) over the segment: 0 = the phone is the top class on every frame
  phone_report    the two together, the teacher's ``sil`` runs optional: per teacher phone where it landed in the conversion
  write_textgrid  runs -> a long-format TextGrid with one interval tier
"""
import collections
import ctypes

import numpy as np
import torch

from facppg import lib as _lib
from facppg.lib import FacppgError

RUN_COLUMNS = ("class", "start", "frames")
REPORT_DTYPE = np.dtype([("phone", np.int32), ("teacher_start", np.int32), ("teacher_frames", np.int32), ("start", np.int32),
                         ("frames", np.int32), ("gop", np.float32), ("share", np.float64), ("kept", np.bool_)])

# em [sum T, D], eb [sum T], top [sum T] on the device; offsets: the B + 1 frame offsets on the host
Emissions = collections.namedtuple("Emissions", "em eb top offsets D")


def _config(floor, switch_cost):
    return _lib.AlignConfig(float(floor), float(switch_cost))


def emissions(x, lengths, floor=1e-10):
    """x [B, D, Tmax]: fp32 GPU tensor in the front end's layout (channel-major, frames contiguous); lengths: its B lengths on
    the host.  One launch: em = -log(max(x, floor)) frame-major, each frame's minimum and top class.  Nothing is copied back."""
    _lib.require_cuda(x, "align: x")
    if x.dim() != 3 or x.dtype != torch.float32:
        raise FacppgError("align: x must be a float32 tensor [B, D, T] (got %s %s)" % (x.dtype, tuple(x.shape)))
    L = _lib.load()
    x = x.contiguous()
    B, D, Tmax = (int(v) for v in x.shape)
    lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lens) != B:
        raise FacppgError("align: %d lengths for %d utterances" % (len(lens), B))
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    dev = x.device
    total = max(off[-1], 1)
    em = torch.empty(total, D, dtype=torch.float32, device=dev)
    eb = torch.empty(total, dtype=torch.float32, device=dev)
    top = torch.empty(total, dtype=torch.int32, device=dev)
    off_dev = _lib.upload(off, torch.int32, dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_ppg_emissions(_config(floor, 0.0), _lib.ptr(x), B, D, Tmax, _lib.ptr(off_dev), _lib.offsets_array(off), _lib.ptr(em),
                                          _lib.ptr(eb), _lib.ptr(top), _lib.current_stream(dev)))
    return Emissions(em, eb, top, off, D)


def _decode_launch(E, switch_cost):
    """The decode of every utterance of E, enqueued: (labels [sum T], cost [B]) as ONE int32 device tensor (cost: fp32 bits)."""
    L = _lib.load()
    dev = E.em.device
    B, total = len(E.offsets) - 1, E.offsets[-1]
    nbytes = L.facppg_ppg_decode_phones_workspace_bytes(total, E.D)
    if nbytes == 0:
        _lib.check(-1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(total + B, dtype=torch.int32, device=dev)
    off_dev = _lib.upload(E.offsets, torch.int32, dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_ppg_decode_phones(_config(1.0, switch_cost), _lib.ptr(E.em), _lib.ptr(off_dev), _lib.offsets_array(E.offsets), B, E.D,
                                              _lib.ptr(out), _lib.ptr(out[total:]), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    return out


def labels_to_runs(labels):
    """Frame labels [T] -> int32 [R, 3]: the runs (class, start, frames)."""
    labels = np.asarray(labels)
    cuts = np.flatnonzero(np.diff(labels)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(labels)]])
    return np.stack([labels[starts], starts, ends - starts], axis=1).astype(np.int32)


def _decode_finish(E, out):
    host = out.cpu().numpy()                 # the one device -> host copy
    total = E.offsets[-1]
    labels = [host[E.offsets[b]:E.offsets[b + 1]].copy() for b in range(len(E.offsets) - 1)]
    return labels, host[total:].view(np.float32).copy()


def decode_labels(E, switch_cost=2.0):
    """Emissions -> (per utterance the frame labels int32 [T_b], cost float32 [B]).  One launch, one device -> host copy."""
    return _decode_finish(E, _decode_launch(E, switch_cost))


def decode_phones(x, lengths, switch_cost=2.0, floor=1e-10):
    """The phone-loop decode of every utterance of the padded batch x (see ``emissions``): per utterance an int32 array [R, 3] of
    runs (class, start, frames).  switch_cost is what one more phone costs, in nats.  Two launches and one device -> host copy
    of the frame labels; the runs are formed on the host."""
    labels, _ = decode_labels(emissions(x, lengths, floor), switch_cost)
    return [labels_to_runs(l) for l in labels]


def _sequences(seqs, optional, B):
    if len(seqs) != B:
        raise FacppgError("force_align: %d sequences for %d utterances" % (len(seqs), B))
    seqs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs]
    if any(len(s) < 1 for s in seqs):
        raise FacppgError("force_align: every utterance needs at least one state")
    if optional is None:
        optional = [np.zeros(len(s), dtype=np.uint8) for s in seqs]
    if len(optional) != B or any(len(o) != len(s) for o, s in zip(optional, seqs)):
        raise FacppgError("force_align: one optional flag per state")
    optional = [(np.asarray(o).reshape(-1) != 0).astype(np.uint8) for o in optional]
    soff = [0]
    for s in seqs:
        soff.append(soff[-1] + len(s))
    return seqs, optional, soff


def align_emissions(E, seqs, optional=None):
    """force_align over emissions that are on the device already."""
    L = _lib.load()
    dev = E.em.device
    B, total = len(E.offsets) - 1, E.offsets[-1]
    seqs, optional, soff = _sequences(seqs, optional, B)
    n = soff[-1]
    seq_host = np.ascontiguousarray(np.concatenate(seqs))
    opt_host = np.ascontiguousarray(np.concatenate(optional))
    S_max = max(len(s) for s in seqs)
    # (classes and flags are refused by the entry point from the host copies, before any launch)
    ints = _lib.upload(seq_host.tolist() + soff + E.offsets, torch.int32, dev)
    opt_dev = _lib.upload(opt_host.tolist(), torch.uint8, dev)
    seq_dev, soff_dev, off_dev = ints[:n], ints[n:n + B + 1], ints[n + B + 1:]
    nbytes = L.facppg_ppg_force_align_workspace_bytes(total, S_max)        # (0, with the reason, beyond 1024 states)
    if nbytes == 0:
        _lib.check(-1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(4 * n + 2 * B, dtype=torch.int32, device=dev)     # start, frames, hits, gop (fp32 bits) [n]; cost (fp32 bits), ok [B]
    with torch.cuda.device(dev):
        _lib.check(L.facppg_ppg_force_align(
            _lib.ptr(E.em), _lib.ptr(E.eb), _lib.ptr(E.top), _lib.ptr(off_dev), _lib.offsets_array(E.offsets), B, E.D,
            _lib.ptr(seq_dev), seq_host.ctypes.data_as(ctypes.c_void_p), _lib.ptr(opt_dev),
            opt_host.ctypes.data_as(ctypes.c_void_p), _lib.ptr(soff_dev), _lib.offsets_array(soff),
            _lib.ptr(out), _lib.ptr(out[n:]), _lib.ptr(out[2 * n:]), _lib.ptr(out[3 * n:]), _lib.ptr(out[4 * n:]), _lib.ptr(out[4 * n + B:]),
            _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    host = out.cpu().numpy()                 # the one device -> host copy
    cut = lambda v: [v[soff[b]:soff[b + 1]].copy() for b in range(B)]    # noqa: E731
    return {"start": cut(host[:n]), "frames": cut(host[n:2 * n]), "hits": cut(host[2 * n:3 * n]), "gop": cut(host[3 * n:4 * n].view(np.float32)),
            "cost": host[4 * n:4 * n + B].view(np.float32).copy(), "ok": host[4 * n + B:] != 0}


def force_align(x, lengths, seqs, optional=None, floor=1e-10):
    """Force-align every utterance of the padded batch x (see ``emissions``) to its own state sequence: seqs[b] the classes of its
    states, optional[b] (None: no state is) the flags of the states a path may skip; two adjacent optional states are refused.
    Returns a dict: per utterance arrays over its states -- start (int32, -1 for a skipped state), frames, hits (int32), gop
    (float32) -- and per batch cost (float32 [B]) and ok (bool [B]: False where the utterance has fewer frames than mandatory
    states; its arrays then read start -1, frames 0).  Two launches and one device -> host copy."""
    return align_emissions(emissions(x, lengths, floor), seqs, optional)


def teacher_sequence(runs, sil_class, T):
    """The teacher's runs -> (classes, optional flags, teacher_start, teacher_frames) of the states the conversion is aligned to:
    the ``sil`` runs are optional, and a sequence that does not begin or end with one gets an optional ``sil`` of no frames there."""
    cls, start, frames = (runs[:, c].tolist() for c in range(3))
    if not cls or cls[0] != sil_class:
        cls, start, frames = [sil_class] + cls, [0] + start, [0] + frames
    if cls[-1] != sil_class:
        cls, start, frames = cls + [sil_class], start + [T], frames + [0]
    cls = np.asarray(cls, dtype=np.int32)
    return cls, (cls == sil_class).astype(np.uint8), np.asarray(start, dtype=np.int32), np.asarray(frames, dtype=np.int32)


def phone_report(x_teacher, len_t, x_conv, len_c, sil_class=None, kept_share=0.5, switch_cost=2.0, floor=1e-10):
    """Teacher PPGs and the conversions' PPGs, two padded batches of B utterances (see ``emissions``; e.g. the two halves of
    score.roundtrip's single front-end pass) -> (reports, phones_kept).  The teacher's phone sequence is decoded from its own PPG,
    its ``sil`` runs (class ``sil_class``, default D - 1 where data/arpa_phonemes puts it) made optional, and the conversion
    force-aligned to it.  reports[b]: one record per teacher phone (REPORT_DTYPE) -- phone, teacher_start, teacher_frames, where it
    landed in the conversion (start, frames; -1, 0: skipped, or nothing could be aligned), gop, share = hits / frames and
    kept = frames > 0 and share >= kept_share.  phones_kept [B]: the share of the teacher's non-sil phones that are kept (1.0
    for an utterance without any).  An optional ``sil`` added at an end has teacher_frames 0."""
    if x_teacher.dim() != 3 or x_conv.dim() != 3 or x_teacher.shape[:2] != x_conv.shape[:2]:
        raise FacppgError("phone_report: teacher and conversion must be [B, D, T] with equal B and D")
    D = int(x_teacher.shape[1])
    sil = D - 1 if sil_class is None else int(sil_class)
    if not 0 <= sil < D:
        raise FacppgError("phone_report: sil_class %d is outside [0, %d)" % (sil, D))
    Et = emissions(x_teacher, len_t, floor)
    pending = _decode_launch(Et, switch_cost)
    Ec = emissions(x_conv, len_c, floor)     # enqueued behind the decode, in front of the copy that waits for it
    labels, _ = _decode_finish(Et, pending)
    states = [teacher_sequence(labels_to_runs(l), sil, len(l)) for l in labels]
    got = align_emissions(Ec, [s[0] for s in states], [s[1] for s in states])
    reports, kept_share_out = [], np.ones(len(states), dtype=np.float64)
    for b, (cls, opt, t_start, t_frames) in enumerate(states):
        r = np.zeros(len(cls), dtype=REPORT_DTYPE)
        r["phone"], r["teacher_start"], r["teacher_frames"] = cls, t_start, t_frames
        r["start"], r["frames"], r["gop"] = got["start"][b], got["frames"][b], got["gop"][b]
        r["share"] = got["hits"][b] / np.maximum(got["frames"][b], 1).astype(np.float64)
        r["kept"] = (r["frames"] > 0) & (r["share"] >= kept_share)
        spoken = cls != sil
        if spoken.any():
            kept_share_out[b] = r["kept"][spoken].sum() / float(spoken.sum())
        reports.append(r)
    return reports, kept_share_out


def phone_lines(path, report, names=None):
    """The lines of synthesize_corpus --phone_file for one utterance, one per teacher phone: path, index, phone, teacher_start,
    teacher_frames, start, frames, gop, share, kept (tabs; floats as %.6g; phone: its name with a table, else its class)."""
    return ["%s\t%d\t%s\t%d\t%d\t%d\t%d\t%.6g\t%.6g\t%d" % (
        path, i, names[int(r["phone"])] if names is not None else int(r["phone"]), int(r["teacher_start"]), int(r["teacher_frames"]), int(r["start"]),
        int(r["frames"]), float(r["gop"]), float(r["share"]), int(r["kept"])) for i, r in enumerate(report)]


def read_phone_table(path):
    """A ``name index`` table, one phone per line (data/arpa_phonemes) -> the names, by index."""
    pairs = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2 or not parts[1].isdigit():
                raise FacppgError("%s:%d: expected `name index`, got %r" % (path, n, line.rstrip("\n")))
            pairs.append((int(parts[1]), parts[0]))
    if sorted(i for i, _ in pairs) != list(range(len(pairs))):
        raise FacppgError("%s: the indices must be 0 .. %d, each once" % (path, len(pairs) - 1))
    return [name for _, name in sorted(pairs)]


def write_textgrid(path, runs, frame_shift_s, names=None, tier="phones"):
    """runs [R, 3] (class, start, frames), in frames, -> a long-format TextGrid with one interval tier.  Runs of no frames (skipped
    states: start -1) are left out; the others must follow each other, and a gap between two becomes an interval without text
    (a TextGrid's intervals are contiguous).  Times are frames x frame_shift_s; names: class -> text (None: the number)."""
    spans = []
    at = 0
    for cls, start, frames in np.asarray(runs).reshape(-1, 3).tolist():
        if frames <= 0:
            continue
        if start < at:
            raise FacppgError("write_textgrid: the run at frame %d starts inside the one before it (which ends at %d)" % (start, at))
        if start > at:
            spans.append((at, start, ""))
        spans.append((start, start + frames, str(names[cls]) if names is not None else str(cls)))
        at = start + frames
    sec = lambda f: repr(round(f * float(frame_shift_s), 9))    # noqa: E731
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %s" % sec(at), "tiers? <exists>", "size = 1", "item []:",
           "    item [1]:", '        class = "IntervalTier"', '        name = "%s"' % tier, "        xmin = 0", "        xmax = %s" % sec(at),
           "        intervals: size = %d" % len(spans)]
    for i, (a, b, text) in enumerate(spans, 1):
        out += ["        intervals [%d]:" % i, "            xmin = %s" % sec(a), "            xmax = %s" % sec(b),
                '            text = "%s"' % text.replace('"', '""')]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
