"""The TDNN acoustic-model kernels (csrc/facppg_tdnn.hip: k_tdnn_input[_batch], k_tdnn_colstart, k_tdnn_renorm,
k_tdnn_output[_batch], k_tdnn_mono<false/true>, k_tdnn_zero_padding, k_tdnn_post_padded) and the chain of k_gemm layers they
surround, held to a float64 reference across layer plans, through the public C ABI alone (tdnn_helpers.py has the plans, the
reference written on the frame axis, the bounds' derivations and the runner; test_tdnn_reference_cpu.py proves the
conditions each class rests on).  Every launch runs under the default GEMM shape and under FACPPG_GEMM_SHAPE=legacy, over a
NaN-filled workspace and output with sentinel guard bands behind them.

Exact class: integer operands, every fp32 sum exact in any order -> np.array_equal with float64, no tolerance: left-only,
right-only and context-free plans, splices with zero-weight gap taps, a dilation longer than the utterance, widths that are
no multiple of 16, split-K 2 and 16, both parities of the ping-pong buffers, T = 1, batches below and above the 256-column
dispatch, every utterance of a batch against its own reference.
Output kernels: exactly known logits (a power of two on the last layer), float64 softmax of those as the reference.
Renorm: one exact layer, then k_tdnn_renorm against float64 under ((C + 3) / 2 + 5) u; the 2^-66 floor on a zero frame.
Rounding class: standard-normal operands against the running bound of tdnn_helpers.py, chain by chain and layer by layer.

Allowances for the device's expf / logf / divide in the output kernels, measured by test_device_softmax_allowances on a
two-class identity plan over 4096 arguments (logits (x, 0), x in [-40, 40]) against float64 -- never against another device
path.  E1: a posterior's distance in float32 ulps; E2: a log-posterior's distance in units of u * max(1, |log-posterior|).
Each allowance is twice the measured value, rounded up to two digits (the other cases use other arguments).
Measured on gfx950: E1 = 1.833 ulp, E2 = 1.929; allowances 3.7 and 3.9."""
import ctypes

import numpy as np
import pytest
import torch

import tdnn_helpers as th
from tdnn_helpers import U

pytestmark = pytest.mark.gpu

E1_ALLOW_ULPS = 3.7
E2_ALLOW = 3.9


@pytest.fixture(scope="module")
def handle():
    """plan -> its device handle, created once per plan for this module, destroyed at the end"""
    from facppg import lib
    made = {}

    def get(plan):
        if plan.name not in made:
            made[plan.name] = (plan, th.create(plan))
        return made[plan.name][1]

    yield get
    for _, h in made.values():
        lib.load().facppg_tdnn_destroy(h)


def _first_bad(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d elements differ from float64, first %s: got %r, want %r" % (
        len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------- exact class
@pytest.mark.parametrize("cs", th.EXACT_CASES, ids=lambda cs: cs.id)
def test_exact(handle, cs):
    plan = th.exact_plan(cs.plan)
    utts = th.utterances(plan, cs.lengths)
    want = [th.reference(plan, u).y.astype(np.float32) for u in utts]
    for name, out in th.run_shapes(handle(plan), plan, cs.entry, utts).items():
        for b, (got, w) in enumerate(zip(th.split_rows(out, cs.lengths), want)):
            assert np.array_equal(got, w), "%s, utterance %d (T = %d): %s" % (name, b, cs.lengths[b], _first_bad(got, w))


@pytest.mark.parametrize("name,renorm,data", [("a_default", 0.0, "normal"), ("g_k500", 0.0, "normal"), ("e_gaps", 1.0, "normal"),
                                              ("h_k4096", 0.0, "int")])
def test_same_bits_alone_and_in_a_batch(handle, name, renorm, data):
    """include/facppg.h: through the GEMM layers the sums are k_gemm's, whose order does not depend on the column count; renorm
    and the output are the single call's arithmetic per frame -- an utterance alone (single call, batch of one) and among
    neighbours (one of them a hundred times larger) gives the same bits, rounding included: standard-normal operands at
    split-K 1 and 2, with a renorm layer, and the integer plan at split-K 16."""
    plan = th.exact_plan(name) if data == "int" else th.rounding_plan(name, renorm)
    h = handle(plan)
    u = th.features(plan.in_dim, 37, data, seed=2)
    lengths = th.BATCHES[1]
    utts = [u if i == 2 else th.features(plan.in_dim, T, data, seed=10 + i) * np.float32(100.0 if i == 3 else 1.0) for i, T in enumerate(lengths)]
    alone = th.run_shapes(h, plan, "single", [u])
    one = th.run_shapes(h, plan, "batch", [u])
    many = th.run_shapes(h, plan, "batch", utts)
    for shape in alone:
        assert np.array_equal(alone[shape], one[shape]) and np.array_equal(alone[shape], th.split_rows(many[shape], lengths)[2]), shape
    assert np.array_equal(alone["default"], alone["legacy"])


# ------------------------------------------------------------------------------------------------------- output kernels
def _check_softmax(got, ref, M, op, what, spread=0.0, extra=0.0):
    """got float32 [T][M] against the float64 (log-)softmax ref.  Exactly known logits: spread = extra = 0.  Rounding class, per
    frame ([T][1]): spread = the largest |z - max z| the device may see, extra = 2 max_c e, the logits' own error bound as it
    reaches a log-posterior (a posterior: exp(extra) - 1, relative)"""
    got = got.astype(np.float64)
    rounded = np.any(spread > 0)
    if op == 1:
        rel = (1 + th.softmax_rel_bound(M, E1_ALLOW_ULPS, spread)) * np.exp(extra) - 1
        err = np.abs(got - ref) / ref
        print("%s: softmax M=%d: max rel err %.3g u, max err / bound %.3g" % (what, M, err.max() / U, (err / rel).max()))
        assert (err <= rel).all(), "%s: worst err / bound %.4g" % (what, (err / rel).max())
    else:
        tol = th.logsoftmax_abs_bound(M, E1_ALLOW_ULPS, E2_ALLOW, ref, rounded=rounded) + extra
        err = np.abs(got - ref)
        print("%s: log-softmax M=%d: max err %.3g u, max err / bound %.3g" % (what, M, err.max() / U, (err / tol).max()))
        assert (err <= tol).all(), "%s: worst err / bound %.4g" % (what, (err / tol).max())


def test_device_softmax_allowances(handle):
    """The measurement behind E1_ALLOW_ULPS / E2_ALLOW: W = I_2, so the logits are the features themselves, (x, 0) for 4096 x
    in [-40, 40]; the two posteriors are expf(-|x|) / (1 + expf(-|x|)) and 1 / (1 + expf(-|x|)) as the device computes them."""
    x = np.zeros((4096, 2), np.float32)
    x[:, 0] = np.linspace(-40.0, 40.0, 4096)
    seen = {}
    for op in (1, 2):
        plan = th.identity_plan(op)
        ref = th.final_f64(x.astype(np.float64), op)
        for name, out in th.run_shapes(handle(plan), plan, "single", [x]).items():
            d = th.ulp_distance(out, ref) if op == 1 else np.abs(out.astype(np.float64) - ref) / (U * np.maximum(1.0, np.abs(ref)))
            seen[op] = max(seen.get(op, 0.0), float(d.max()))
    print("softmax: max %.3f ulp (E1); log-softmax: max %.3f u max(1, |r|) (E2)" % (seen[1], seen[2]))
    assert 2 * seen[1] <= E1_ALLOW_ULPS
    assert 2 * seen[2] <= E2_ALLOW


@pytest.mark.parametrize("op", [1, 2], ids=["softmax", "logsoftmax"])
@pytest.mark.parametrize("M", th.SOFTMAX_M)
def test_output_kernels(handle, M, op):
    """k_tdnn_output (single call) and k_tdnn_output_batch"""
    plan = th.softmax_plan(M, op)
    h = handle(plan)
    lengths = th.BATCHES[1]
    utts = th.utterances(plan, lengths)
    refs = [th.reference(plan, u).out for u in utts]
    for name, out in th.run_shapes(h, plan, "batch", utts).items():
        for b, (got, ref) in enumerate(zip(th.split_rows(out, lengths), refs)):
            _check_softmax(got, ref, M, op, "%s batch[%d]" % (name, b))
    for name, out in th.run_shapes(h, plan, "single", [utts[2]]).items():
        _check_softmax(out, refs[2], M, op, "%s single" % name)


@pytest.mark.parametrize("Md", th.MONO_MD)
@pytest.mark.parametrize("M", th.SOFTMAX_M)
def test_mono(handle, M, Md):
    """k_tdnn_mono<false> against float64 softmax . Rt; k_tdnn_mono<true> + k_tdnn_zero_padding: the same bits in [B][Md][Tmax],
    exactly 0.0f behind each utterance over the NaN pre-fill, with Tmax equal to and above the longest utterance; the strided
    form leaves the guard rows behind each utterance's Md rows alone."""
    plan = th.softmax_plan(M, 1)
    h = handle(plan)
    Rt = th.transform(M, Md)
    lengths = th.BATCHES[1]
    utts = th.utterances(plan, lengths)
    want = [th.reference(plan, u).out @ Rt.astype(np.float64) for u in utts]
    bound = th.mono_rel_bound(M, E1_ALLOW_ULPS)
    flat = th.run_shapes(h, plan, "reduced", utts, Rt=Rt)
    for name, out in flat.items():
        worst = 0.0
        for got, w in zip(th.split_rows(out, lengths), want):
            assert (w > 0).all()
            err = np.abs(got.astype(np.float64) - w) / w
            worst = max(worst, float(err.max()))
            assert (err <= bound).all(), (name, err.max() / U, bound / U)
        print("%s mono M=%d Md=%d: max rel err %.3g u, bound %.3g u" % (name, M, Md, worst / U, bound / U))
    for entry, Tmax, rows in (("padded", 150, 0), ("padded", 157, 0), ("strided", 153, 3)):
        for name, out in th.run_shapes(h, plan, entry, utts, Rt=Rt, Tmax=Tmax, guard_rows=rows).items():
            assert out.shape == (len(lengths), Md, Tmax)
            for b, (T, rows_b) in enumerate(zip(lengths, th.split_rows(flat[name], lengths))):
                assert np.array_equal(out[b, :, :T].T, rows_b), (entry, Tmax, name, b)
                assert not out[b, :, T:].any() and not np.signbit(out[b, :, T:]).any()


POST_LENGTHS = tuple(37 if i == 5 else (1, 2, 5, 9, 16, 3, 12)[i % 7] for i in range(32))


@pytest.mark.parametrize("M", [41, 257, 600])
def test_post_padded(handle, M):
    """k_tdnn_post_padded against float64; padding exactly zero; one utterance alone (widest channel split) and inside a batch
    with tiles * B >= 2 * multi_processor_count (split 1: one workgroup stores all M rows) give equal bits -- the max and the
    sum run over all M rows whatever rows a workgroup stores; the strided form keeps its guard rows."""
    plan = th.softmax_plan(M, 1)
    h = handle(plan)
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    utts = th.utterances(plan, POST_LENGTHS)
    refs = [th.reference(plan, u).out for u in utts]

    def check(out, lengths, refs, what):
        for b, (T, ref) in enumerate(zip(lengths, refs)):
            _check_softmax(out[b, :, :T].T, ref, M, 1, "%s[%d]" % (what, b))
            assert not out[b, :, T:].any() and not np.signbit(out[b, :, T:]).any()

    alone = {}
    for Tmax in (37, 40, 64):                                      # 3, 3 and 4 tiles of one utterance: split 16 ways
        assert 2 * n_cu // ((Tmax + 15) // 16) >= 16
        alone[Tmax] = th.run_shapes(h, plan, "padded", [utts[5]], Tmax=Tmax)
        for name, out in alone[Tmax].items():
            check(out, (37,), [refs[5]], "%s alone Tmax=%d" % (name, Tmax))
            assert np.array_equal(out[0, :, :37], alone[37][name][0])
    if M <= 257:                                                    # (M = 600 at Tmax = 256 x 32 utterances is 20 MB of output)
        Tmax = 256
        assert (Tmax // 16) * len(utts) >= 2 * n_cu, "the batch no longer reaches split 1 on this device: lengthen it"
        for entry, rows in (("padded", 0), ("strided", 3)):
            for name, out in th.run_shapes(h, plan, entry, utts, Tmax=Tmax, guard_rows=rows).items():
                check(out, POST_LENGTHS, refs, "%s %s batch of 32" % (name, entry))
                assert np.array_equal(out[5, :, :37], alone[37][name][0]), "the channel split changed a posterior"
    for name, out in th.run_shapes(h, plan, "strided", utts[:6], Tmax=41, guard_rows=3).items():
        check(out, POST_LENGTHS[:6], refs[:6], "%s strided" % name)
        assert np.array_equal(out[5, :, :37], alone[37][name][0])


# --------------------------------------------------------------------------------------------------------------- renorm
@pytest.mark.parametrize("C,rms", th.RENORM_CASES)
def test_renorm(handle, C, rms):
    """one exact layer, then k_tdnn_renorm: relative bound ((C + 3) / 2 + 5) u (tdnn_helpers.py); the all-zero frame reaches the
    2^-66 floor: exactly 0.0f there, finite everywhere"""
    plan = th.renorm_plan(C, rms)
    x = th.renorm_features(C, rms)
    r = th.reference(plan, x, exact_gemm=True)
    others = [th.features(13, T, seed=30 + T) for T in (5, 2)]
    runs = {"single": th.run_shapes(handle(plan), plan, "single", [x]), "batch": th.run_shapes(handle(plan), plan, "batch", [others[0], x, others[1]])}
    for entry, shapes in runs.items():
        for name, out in shapes.items():
            got = out if entry == "single" else out[5:5 + th.RENORM_T]
            assert np.isfinite(out).all()
            assert not got[th.RENORM_ZERO_FRAME].any()
            err = np.abs(got.astype(np.float64) - r.y)
            live = r.y > 0
            print("%s %s renorm C=%d rms=%g: max rel err %.3g u, bound %.3g u" % (
                entry, name, C, rms, (err[live] / r.y[live]).max() / U, (r.e[live] / r.y[live]).max() / U))
            assert (err <= r.e).all() and (got[~live] == 0).all()
        assert np.array_equal(shapes["default"], shapes["legacy"])
    assert np.array_equal(runs["single"]["default"], runs["batch"]["default"][5:5 + th.RENORM_T])


# ------------------------------------------------------------------------------------------------------- rounding class
def _report(what, err, e):
    print("%s: max err %.3g, bound there %.3g, max err / bound %.3g" % (what, err.max(), e.flat[err.argmax()], (err / e).max()))


@pytest.mark.parametrize("lengths,entry", th.ROUNDING_SHAPES, ids=["single", "batch"])
@pytest.mark.parametrize("name,renorm", th.ROUNDING_PLANS)
def test_rounding(handle, name, renorm, lengths, entry):
    """the last layer (final_op 0) within the running bound e; the posteriors (final_op 1) within exp(2 max_c e) - 1 on top of
    the output kernel's own bound"""
    base = th.rounding_plan(name, renorm)
    utts = th.utterances(base, lengths, "normal")
    refs = [th.reference(base, u) for u in utts]
    for name_, out in th.run_shapes(handle(base), base, entry, utts).items():
        for b, (got, r) in enumerate(zip(th.split_rows(out, lengths), refs)):
            err = np.abs(got.astype(np.float64) - r.y)
            _report("%s %s[%d] logits" % (base.name, name_, b), err, r.e)
            assert (err <= r.e).all()
    post = base.with_final(1)
    M = post.out_dim
    for name_, out in th.run_shapes(handle(post), post, entry, utts).items():
        for b, (got, r) in enumerate(zip(th.split_rows(out, lengths), refs)):
            emax = r.e.max(axis=1, keepdims=True)
            spread = r.y.max(axis=1, keepdims=True) - r.y.min(axis=1, keepdims=True) + 2 * emax
            _check_softmax(got, th.final_f64(r.y, 1), M, 1, "%s %s[%d]" % (post.name, name_, b), spread=spread, extra=2 * emax)


@pytest.mark.parametrize("name,i", th.ROUNDING_LAYERS)
def test_rounding_layer(handle, name, i):
    """every layer shape of the rounding plans on its own: the bound of one layer, (K + 2) 2u sum |w| |x|, and -- as
    test_gpu_gemm.py asks of k_gemm -- the bound is not being leaned on: rms of err / (u S) below sqrt(K)"""
    plan = th.layer_plan(name, i)
    K = plan.layers[0].K
    for lengths, entry in th.ROUNDING_SHAPES:
        utts = th.utterances(plan, lengths, "normal")
        refs = [th.reference(plan, u) for u in utts]
        for name_, out in th.run_shapes(handle(plan), plan, entry, utts).items():
            ratios, live = [], []
            for b, (got, r) in enumerate(zip(th.split_rows(out, lengths), refs)):
                err = np.abs(got.astype(np.float64) - r.y)
                assert (err <= r.e).all(), (name_, b, (err / r.e).max())
                ratios.append((err / (U * r.S)).reshape(-1))
                live.append((r.y != 0).reshape(-1))
            ratio, live = np.concatenate(ratios), np.concatenate(live)
            rms = float(np.sqrt(np.mean(ratio * ratio)))
            print("%s %s %s: max err / bound %.3g, rms err / (u S) %.3g (sqrt K = %.3g)" % (
                plan.name, entry, name_, float(ratio.max() / ((K + 2) * 2)), rms, K ** 0.5))
            assert rms < K ** 0.5
            assert K < 128 or np.median(ratio[live]) > 0               # ... and the comparison is not vacuous (a ReLU's zeros apart)


def test_file_path(handle, tmp_path):
    """write_nnet3 -> read_nnet3_model -> compute_full_ppg / compute_full_ppg_batch on a non-default plan (lda, batchnorm,
    splices (-1, 0, 1), (-3, 0, 3), (-6, -3, 0), 40 -> 50 -> 41): plan_layers' folding and _TdnnHandle's blob order against
    the float64 fold of tdnn_helpers.fold_file_model"""
    import ppg
    from common import decode, nnet3
    path = str(tmp_path / "final.raw")
    nnet3.write_nnet3(path, th.file_model())
    model = decode.read_nnet3_model(path)
    plan = th.fold_file_model(model)
    lengths = th.BATCHES[1]
    utts = th.utterances(plan, lengths, "normal")
    refs = [th.reference(plan, u) for u in utts]
    single = [ppg.compute_full_ppg(model, torch.from_numpy(np.array(u)).cuda()).cpu().numpy() for u in utts]
    batch = [t.cpu().numpy() for t in ppg.compute_full_ppg_batch(model, [torch.from_numpy(np.array(u)).cuda() for u in utts])]
    for what, outs in (("compute_full_ppg", single), ("compute_full_ppg_batch", batch)):
        for b, (got, r) in enumerate(zip(outs, refs)):
            assert got.shape == r.out.shape
            emax = r.e.max(axis=1, keepdims=True)
            spread = r.y.max(axis=1, keepdims=True) - r.y.min(axis=1, keepdims=True) + 2 * emax
            _check_softmax(got, r.out, 41, 1, "%s[%d]" % (what, b), spread=spread, extra=2 * emax)
    for a, b in zip(single, batch):
        assert np.array_equal(a, b)
    # the same chain through the C ABI with the folded weights of this file: the logits within the running bound
    logits = plan.with_final(0)
    for name, out in th.run_shapes(handle(logits), logits, "batch", utts).items():
        for b, (got, r) in enumerate(zip(th.split_rows(out, lengths), refs)):
            err = np.abs(got.astype(np.float64) - r.y)
            _report("file plan %s[%d] logits" % (name, b), err, r.e)
            assert (err <= r.e).all()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_create_refusals():
    """each returns its code, names the cause in facppg_last_error and leaves *out alone"""
    from facppg import lib
    L = lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    good = th.exact_plan("i_two")
    n = good.blob().size

    def attempt(edit=None, final_op=0, n_weights=None):
        table = good.table()
        if edit:
            edit(table)
        count = L.facppg_tdnn_weight_count(table, len(good.layers))                          # (0 for a table it cannot size)
        flat = torch.zeros(max(count, n) + 1, device=dev)
        flat[:n] = torch.from_numpy(good.blob()).to(dev)
        out = ctypes.c_void_p(0xD15EA5E)
        rc = L.facppg_tdnn_create(table, len(good.layers), final_op, lib.ptr(flat), count if n_weights is None else n_weights, dev.index,
                                  lib.current_stream(dev), ctypes.byref(out))
        assert out.value == 0xD15EA5E, "a refused facppg_tdnn_create wrote its out pointer"
        return rc, L.facppg_last_error().decode()

    def setf(i, **kw):
        def edit(t):
            for k, v in kw.items():
                setattr(t[i], k, v)
        return edit

    cases = [
        ("first > 0", th.EUNSUPPORTED, "splice", dict(edit=setf(1, first=1))),
        ("last tap < 0", th.EUNSUPPORTED, "splice", dict(edit=setf(0, first=-3))),              # taps 3, dil 1: last tap at -1
        ("in_dim != previous out_dim", th.EINVAL, "layer 1 reads", dict(edit=setf(1, in_dim=49))),
        ("blob too short", th.EINVAL, "weight blob", dict(n_weights=n - 1)),
        ("blob too long", th.EINVAL, "weight blob", dict(n_weights=n + 1)),
        ("final_op 3", th.EINVAL, "final_op", dict(final_op=3)),
        ("final_op -1", th.EINVAL, "final_op", dict(final_op=-1)),
        ("taps 0", th.EINVAL, "weight blob", dict(edit=setf(0, taps=0))),
        ("dil 0", th.EINVAL, "weight blob", dict(edit=setf(0, dil=0))),
    ]
    for what, code, needle, kw in cases:
        rc, msg = attempt(**kw)
        assert rc == code and needle in msg, (what, rc, msg)


def test_forward_refusals(handle):
    plan = th.exact_plan("i_two")
    h = handle(plan)
    u = th.features(plan.in_dim, 5)
    for what, code, needle, kw in (("T = 0", th.EINVAL, "T must be positive", dict(T=0)), ("T < 0", th.EINVAL, "T must be positive", dict(T=-3)),
                                   ("short workspace", th.EWORKSPACE, "workspace", dict(ws_bytes=256))):
        run = th.launch(h, plan, "single", [u], **kw)
        assert run.rc == code and needle in run.error, (what, run.rc, run.error)
        assert np.isnan(run.out).all() and (run.guards == th.SENTINEL).all(), what            # nothing was launched
    run = th.launch(h, plan, "batch", [u, u], ws_bytes=256)
    assert run.rc == th.EWORKSPACE and "workspace" in run.error and np.isnan(run.out).all()
