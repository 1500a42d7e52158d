"""GPU: facppg_ppg_emissions, facppg_ppg_decode_phones and facppg_ppg_force_align (facppg.align) against the reference of their
definition (align_helpers.py).

Emissions: em, eb, top against float64 over D in (1, 3, 40, 256) x T in (1, 63, 64, 65, 257) -- one class, fewer classes than waves
of the workgroup, one pass and four passes over the LDS tile; one frame, a tile of 64 frames less one, full, plus one, and five
tiles.  top is exact (the generator leaves no ties); the bar for em is 4 x what NumPy's own float32 -log deviates from float64
(align_helpers.emission_tolerance), since the device's logf may round differently; both figures are printed.
Measured on the MI355X: NumPy's own deviation 9.08e-8, the bar 3.63e-7, the device's worst 1.85e-7 (D = 256; 1.83e-7 at D = 40,
1.64e-7 at D = 3, exactly 0 at D = 1); the test prints them per D.

Decode and forced alignment are held BIT FOR BIT to the float32 restatement run on the emissions the device wrote: labels,
segments, hits, cost and gop -- each cell is one add and some comparisons, so nothing may differ.  Against the float64 reference the
costs stay within align_helpers.cost_tolerance: the emission tolerance times the frame count plus the restatement's own deviation
(measured on the MI355X: the device's worst is 8.7e-7 per frame, the bar 1.13e-6), and the labels equal the float64 ones.
T in (1, 2, 7, 63, 64, 65, 150, 600) x D in (3, 40, 256): the decode on both sides of its single-wave cut; the state counts are those of the decoded sequences (with and without optional states) plus the hand
cases of align_helpers.hand_cases and S = 64, 65, 1024 at T = 1030 (both sides of the aligner's single-wave cut, and a full
workgroup)."""
import ctypes

import numpy as np
import pytest
import torch

import align_helpers as ah

pytestmark = pytest.mark.gpu


def _padded(mats, Tmax=None, fill=np.nan):
    """[D, T_b] arrays -> [B, D, Tmax] on the GPU with ``fill`` behind every length."""
    Tmax = Tmax or max(m.shape[1] for m in mats)
    x = np.full((len(mats), mats[0].shape[0], Tmax), fill, dtype=np.float32)
    for b, m in enumerate(mats):
        x[b, :, :m.shape[1]] = m
    return torch.from_numpy(x).cuda()


def _emit(mats, floor=ah.FLOOR, **kw):
    from facppg import align
    return align.emissions(_padded(mats, **kw), [m.shape[1] for m in mats], floor)


def _host(E, b=0):
    lo, hi = E.offsets[b], E.offsets[b + 1]
    return E.em[lo:hi].cpu().numpy(), E.eb[lo:hi].cpu().numpy(), E.top[lo:hi].cpu().numpy()


def _bits(v):
    return np.ascontiguousarray(v).tobytes()


def _same_alignment(got, b, ref, what):
    """The device's utterance b against a restatement's dict, bit for bit."""
    for k in ("start", "frames", "hits"):
        assert got[k][b].tolist() == ref[k].tolist(), (what, k, got[k][b].tolist(), ref[k].tolist())
    assert got["gop"][b].dtype == np.float32 and _bits(got["gop"][b]) == _bits(ref["gop"].astype(np.float32)), (what, got["gop"][b], ref["gop"])
    assert _bits(got["cost"][b:b + 1]) == _bits(np.float32(ref["cost"])), (what, got["cost"][b], ref["cost"])
    assert bool(got["ok"][b]) == ref["ok"], what


@pytest.mark.parametrize("D", ah.EMIT_DIMS)
def test_emissions_against_float64(D):
    mats = [ah.inputs(T, D) for T in ah.EMIT_FRAMES]
    E = _emit(mats)                                   # one ragged batch, NaN behind every length
    tol, worst = ah.emission_tolerance(), 0.0
    for b, x in enumerate(mats):
        em, eb, top = _host(E, b)
        e64, b64, t64 = ah.emissions(x)
        assert em.shape == e64.shape and np.isfinite(em).all()
        assert top.tolist() == t64.tolist(), (D, x.shape[1])
        assert _bits(eb) == _bits(em.min(axis=1)), (D, x.shape[1])
        dev = float(np.max(np.abs(em.astype(np.float64) - e64) / np.maximum(1.0, np.abs(e64))))
        worst = max(worst, dev)
        assert dev <= tol, (D, x.shape[1], dev, tol)
    print("D = %d: device worst |em - em64| / max(1, |em64|) = %.3e; NumPy float32 -log: %.3e; bar %.3e" % (D, worst, ah.emission_deviation(), tol))
    # NaN (or anything else) behind the lengths changes nothing; neither do the neighbours in the batch
    other = _emit(mats, fill=0.25, Tmax=300)
    assert all(torch.equal(getattr(E, k), getattr(other, k)) for k in ("em", "eb", "top"))
    alone = _emit([mats[3]])
    assert all(_bits(u) == _bits(v) for u, v in zip(_host(alone), _host(E, 3)))


def test_emissions_floor():
    """Posteriors of exactly 0 -- and anything else below the floor -- give -logf(floor): the bits of a posterior AT the floor."""
    z = np.zeros((40, 70), dtype=np.float32)
    z[7, :] = 1.0
    z[3, 5] = 1e-12
    at = np.where(z < np.float32(1e-10), np.float32(1e-10), z)
    em = _host(_emit([z]))[0]
    assert _bits(em) == _bits(_host(_emit([at]))[0])
    assert abs(float(em[0, 0]) - -np.log(1e-10)) <= ah.emission_tolerance() * -np.log(1e-10) and (em[:, 7] == 0.0).all()
    high = _host(_emit([z], floor=1e-3))
    assert abs(float(high[0][0, 0]) - -np.log(1e-3)) <= ah.emission_tolerance() * -np.log(1e-3)
    assert high[2].tolist() == [7] * 70 and (high[1] == 0.0).all()


@pytest.mark.parametrize("D", ah.DIMS_GPU)
def test_decode_and_alignment_equal_the_float32_restatement_bit_for_bit(D):
    from facppg import align
    worst = 0.0
    for T in ah.FRAMES:
        x = ah.inputs(T, D)
        E = _emit([x])
        em, eb, top = _host(E)
        labels, cost = align.decode_labels(E, ah.SWITCH_COST)
        l32, c32 = ah.decode(em, ah.SWITCH_COST)
        assert labels[0].tolist() == l32.tolist(), (T, D)
        assert _bits(cost) == _bits(np.float32(c32)), (T, D, cost, c32)
        ref64 = ah.case(T, D)[np.float64]
        assert labels[0].tolist() == ref64[0].tolist(), (T, D)      # (so the two alignments below are to one sequence)
        assert abs(float(cost[0]) - float(ref64[1])) <= ah.cost_tolerance(T), (T, D, cost, ref64[1])
        worst = max(worst, abs(float(cost[0]) - float(ref64[1])) / T)
        assert align.decode_phones(_padded([x]), [T])[0].tolist() == [list(r) for r in ah.runs_of(l32)]
        # aligned to its own decoded runs, no optional state: the float64 case of the CPU test
        runs = align.labels_to_runs(labels[0])
        got = align.align_emissions(E, [runs[:, 0]])
        _same_alignment(got, 0, ah.align(em, eb, top, runs[:, 0]), (T, D, "plain"))
        a64 = ref64[2]
        assert abs(float(got["cost"][0]) - float(a64["cost"])) <= ah.cost_tolerance(T), (T, D, got["cost"][0], a64["cost"])
        worst = max(worst, abs(float(got["cost"][0]) - float(a64["cost"])) / T)
        # the last class optional, an optional one added at either end (phone_report's sequence): skips are in play
        seq, opt, _, _ = align.teacher_sequence(runs, D - 1, T)
        got = align.align_emissions(E, [seq], [opt])
        _same_alignment(got, 0, ah.align(em, eb, top, seq, opt), (T, D, "optional"))
    print("D = %d: device worst |cost - cost64| / T = %.3e (the restatement's own: %.3e; bar %.3e)" % (
        D, worst, ah.cost_deviation_per_frame(), ah.cost_tolerance(1)))


def test_hand_cases_of_the_forced_alignment():
    from facppg import align
    for name, x, seq, opt, want in ah.hand_cases():
        E = _emit([x])
        got = align.align_emissions(E, [seq], [opt])
        ah.check_expected(name, {k: v[0] for k, v in got.items()}, want)
        _same_alignment(got, 0, ah.align(*_host(E), seq, opt), name)
        if not want["ok"]:
            assert np.isinf(got["cost"][0])
    for S in (64, 65, 1024):                         # the single-wave form, one state past it, a full workgroup
        x, seq, opt = ah.long_case(S)
        E = _emit([x])
        got = align.align_emissions(E, [seq], [opt])
        ref = ah.align(*_host(E), seq, opt)
        _same_alignment(got, 0, ref, S)
        assert got["ok"][0] and int(got["frames"][0].sum()) == 1030


def test_ragged_batch_equals_single_calls():
    """Five utterances of different lengths and state counts in one padded batch (NaN behind the lengths), one of them without a
    path: the same bits as five calls."""
    from facppg import align
    D = 40
    mats = [ah.inputs(T, D) for T in (7, 150, 2, 65, 64)]
    E = _emit(mats, Tmax=160)
    labels, cost = align.decode_labels(E)
    seqs, opts = [], []
    for b, l in enumerate(labels):
        seq, opt, _, _ = align.teacher_sequence(align.labels_to_runs(l), D - 1, len(l))
        seqs.append(seq)
        opts.append(opt)
    seqs[2], opts[2] = np.asarray([1, 2, 3], dtype=np.int32), np.zeros(3, dtype=np.uint8)      # three mandatory states, two frames
    got = align.align_emissions(E, seqs, opts)
    assert got["ok"].tolist() == [True, True, False, True, True] and got["start"][2].tolist() == [-1, -1, -1]
    for b, x in enumerate(mats):
        E1 = _emit([x])
        l1, c1 = align.decode_labels(E1)
        assert l1[0].tolist() == labels[b].tolist() and _bits(c1) == _bits(cost[b:b + 1]), b
        one = align.align_emissions(E1, [seqs[b]], [opts[b]])
        for k in ("start", "frames", "hits", "gop"):
            assert _bits(one[k][0]) == _bits(got[k][b]), (b, k)
        assert _bits(one["cost"]) == _bits(got["cost"][b:b + 1]) and bool(one["ok"][0]) == bool(got["ok"][b])
    # the public calls over the same batch
    x = _padded(mats, Tmax=160)
    lens = [m.shape[1] for m in mats]
    assert all(r.tolist() == align.labels_to_runs(l).tolist() for r, l in zip(align.decode_phones(x, lens), labels))
    pub = align.force_align(x, lens, seqs, opts)
    assert all(_bits(pub[k][b]) == _bits(got[k][b]) for k in ("start", "frames", "hits", "gop") for b in range(5))


def _raw_align(E, seq, opt, soff, ws=None, ws_bytes=None, null=None):
    """The raw entry point over real buffers, the outputs and the workspace pre-filled: (rc, message, outputs, workspace)."""
    from facppg import lib as flib
    L = flib.load()
    dev = E.em.device
    B, n = len(soff) - 1, len(seq)
    seq_h, opt_h = np.asarray(seq, dtype=np.int32), np.asarray(opt, dtype=np.uint8)
    seq_d, opt_d = torch.from_numpy(seq_h).to(dev), torch.from_numpy(opt_h).to(dev)
    soff_d, off_d = torch.tensor(soff, dtype=torch.int32, device=dev), torch.tensor(E.offsets, dtype=torch.int32, device=dev)
    out = torch.full((4 * n + 2 * B,), -7, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.full((1 << 21,), 0xA5, dtype=torch.uint8, device=dev)
    p = lambda k, t: ctypes.c_void_p(0) if null == k else flib.ptr(t)    # noqa: E731
    rc = L.facppg_ppg_force_align(p("em", E.em), flib.ptr(E.eb), flib.ptr(E.top), flib.ptr(off_d), flib.offsets_array(E.offsets), B, E.D,
                                  flib.ptr(seq_d), seq_h.ctypes.data_as(ctypes.c_void_p), flib.ptr(opt_d), opt_h.ctypes.data_as(ctypes.c_void_p),
                                  flib.ptr(soff_d), flib.offsets_array(soff), flib.ptr(out), flib.ptr(out[n:]), flib.ptr(out[2 * n:]),
                                  flib.ptr(out[3 * n:]), flib.ptr(out[4 * n:]), p("ok", out[4 * n + B:]), flib.ptr(ws),
                                  ctypes.c_size_t(ws.numel() if ws_bytes is None else ws_bytes), flib.current_stream(dev))
    torch.cuda.synchronize()
    return rc, L.facppg_last_error().decode(), out, ws


def test_refusals_launch_nothing():
    from facppg import align
    from facppg import lib as flib
    L = flib.load()
    x = ah.inputs(150, 40)
    E = _emit([x])
    untouched = lambda out, ws: bool((out == -7).all()) and bool((ws == 0xA5).all())    # noqa: E731
    big = _emit([ah.make(1030, 40, ah.seed_of(1030, 40))])
    for what, (e, seq, opt, soff, kw), code, text in (
            ("S = 1025", (big, [1] * 1025, [0] * 1025, [0, 1025], {}), -2, "1025 states"),
            ("a class equal to D", (E, [1, 40, 2], [0, 0, 0], [0, 3], {}), -1, "class 40 is outside [0, 40)"),
            ("adjacent optional states", (E, [1, 39, 39, 2], [0, 1, 1, 0], [0, 4], {}), -1, "both optional"),
            ("a short workspace", (E, [1, 39, 2], [0, 1, 0], [0, 3], dict(ws_bytes=150 * 3 - 1)), -4, "asks for"),
            ("NULL emissions", (E, [1, 39, 2], [0, 1, 0], [0, 3], dict(null="em")), -1, "NULL argument"),
            ("NULL ok", (E, [1, 39, 2], [0, 1, 0], [0, 3], dict(null="ok")), -1, "NULL argument")):
        rc, msg, out, ws = _raw_align(e, seq, opt, soff, **kw)
        assert rc == code and text in msg, (what, rc, msg)
        assert untouched(out, ws), what
    # through the Python surface: FacppgError with the library's message
    with pytest.raises(flib.FacppgError, match="class 40 is outside"):
        align.align_emissions(E, [[1, 40, 2]])
    with pytest.raises(flib.FacppgError, match="both optional"):
        align.force_align(_padded([x]), [150], [[1, 39, 39, 2]], [[0, 1, 1, 0]])
    with pytest.raises(flib.FacppgError, match=r"S_max in \[1, 1024\] \(got 1030, 1025\)"):
        align.align_emissions(big, [[1] * 1025])
    with pytest.raises(flib.FacppgError, match="at most 256 classes"):
        align.emissions(torch.zeros(1, 257, 4, device="cuda"), [4])
    # the decode's workspace and NULL
    lab = torch.full((151,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.tensor(E.offsets, dtype=torch.int32, device="cuda")
    cfg = flib.AlignConfig(1e-10, 2.0)
    need = L.facppg_ppg_decode_phones_workspace_bytes(150, 40)
    for kw, code in ((dict(ws_bytes=need - 1), -4), (dict(em=None), -1)):
        rc = L.facppg_ppg_decode_phones(cfg, flib.ptr(kw.get("em", E.em)), flib.ptr(off), flib.offsets_array(E.offsets), 1, 40, flib.ptr(lab),
                                        flib.ptr(lab[150:]), flib.ptr(ws), ctypes.c_size_t(kw.get("ws_bytes", need)), flib.current_stream(lab.device))
        torch.cuda.synchronize()
        assert rc == code and L.facppg_last_error(), kw
        assert untouched(lab, ws), kw


def test_twice_on_one_workspace_of_the_stated_size():
    """The aligner twice back to back on a workspace of exactly facppg_ppg_force_align_workspace_bytes, a canary behind it and
    behind the outputs: the same results, nothing written past the stated size, the stream still usable."""
    from facppg import align
    from facppg import lib as flib
    L = flib.load()
    mats = [ah.inputs(T, 40) for T in (65, 150, 7)]
    E = _emit(mats)
    labels, _ = align.decode_labels(E)
    seqs = [align.labels_to_runs(l)[:, 0] for l in labels]
    soff = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).tolist()
    need = L.facppg_ppg_force_align_workspace_bytes(E.offsets[-1], max(len(s) for s in seqs))
    assert need > 0
    outs = []
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        rc, msg, out, ws = _raw_align(E, np.concatenate(seqs), np.zeros(soff[-1], np.uint8), soff, ws=ws, ws_bytes=need)
        assert rc == 0, msg
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool((ws[need:] == 0xA5).all())
    ref = align.align_emissions(E, seqs)
    n = soff[-1]
    assert outs[0][:n].cpu().numpy().tolist() == np.concatenate(ref["start"]).tolist()
    assert outs[0][4 * n + 3:].cpu().numpy().tolist() == [1, 1, 1]
    assert float((torch.ones(8, device="cuda") * 2).sum()) == 16.0      # the stream goes on
