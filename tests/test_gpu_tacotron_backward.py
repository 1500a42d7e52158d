"""GPU: the backward pass of the teacher-forced Tacotron2.forward (eval mode) against the imported reference's float64
loss.backward() (tests/golden/make_golden_forced_grad.py), and finetune() against 8 reference Adam steps.

Tolerance (backward_helpers): C * E32 with E32 = 6.7e-6, the reference's own float32-vs-float64 deviation; every one of the
61 tensors is held to it, on its norm and on its sub-sample, in every case.

Measured on an MI355X (worst over the 61 tensors, norm and sub-sample):
    ragged 8.5e-6 (location_dense), dup 5.9e-6, mono40 6.7e-6; d loss / d memory of ragged 5.6e-6; B = 1 against the dup batch
    3.2e-6; under the forward pass's forced launch shapes 6.1e-6 - 8.5e-6.  The worst, 8.5e-6 = 1.27 E32, with a factor 2 of
    headroom needs 1.7e-5: C = 4 (2.7e-5) is the smallest power of two that gives it (C = 2: 1.3e-5).
    finetune: the 8 losses follow the float64 trajectory to 3.7e-7 relative; the fixture's float32 run deviates by 1.2e-6, so by
    the same rule C_LOSS = 1 (1.2e-6, a factor 3.3 of headroom).  Pre-clip gradient norms: 7.9e-6, held to C * E32 like every
    other gradient norm.
"""
import os

import numpy as np
import pytest
import torch

import backward_helpers as bh
from forced_helpers import forced_case, forced_utterances
from helpers import golden, masks_from_seed

pytestmark = pytest.mark.gpu


def build(hp, sd):
    from script.train_ppg2mel import load_model
    m = load_model(hp)
    m.load_state_dict(sd, strict=True)
    return m.eval()


def inputs_of(d, ppg, tgt):
    il, ol = torch.tensor(d["input_lengths"]).long().cuda(), torch.tensor(d["output_lengths"]).long().cuda()
    return (ppg.cuda(), il, tgt.cuda(), int(il.max()), ol)


def loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec):
    from common.loss_function import Tacotron2Loss
    m.zero_grad()
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec), differentiable=True)
    loss = Tacotron2Loss()(out, (tgt.cuda(), gate_t.cuda()))
    loss.backward()
    return loss, {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}


def hold(fix, grads, tag):
    dev = bh.deviations(fix, grads)
    assert len(dev) == 61
    tol = bh.tolerance()
    worst = max(dev, key=lambda r: max(r[1], r[2]))
    print(tag, "worst %s norm %.2e sub %.2e | tolerance %.2e" % (worst + (tol,)))
    bad = [r for r in dev if not (r[1] <= tol and r[2] <= tol)]
    assert not bad, bad


def expected_launches(hp, B, Tin, T):
    H = hp.encoder_embedding_dim // 2
    return [("lstm_backward", B, T, hp.decoder_rnn_dim), ("attention_backward", B, T, hp.attention_rnn_dim),
            ("lstm_backward", B, Tin, H), ("lstm_backward", B, Tin, H)]


@pytest.mark.parametrize("tag", bh.TAGS)
def test_gradients_match_the_float64_reference(tag):
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case(tag)
    fix = bh.grad_fixture(tag)
    m = build(hp, sd)
    loss, grads = loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec)
    print(tag, "loss %.7f reference %.7f" % (float(loss), float(fix["loss"])))
    assert m.last_backward_launches == expected_launches(hp, ppg.shape[0], ppg.shape[2], tgt.shape[2])
    if tag == "ragged":                                   # the decoder alone: d loss / d (encoder output)
        got, ref = m.last_memory_grad.cpu().numpy().astype(np.float64), fix["dmemory"].astype(np.float64)
        dev = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print(tag, "d memory %.2e" % dev)
        assert dev <= bh.tolerance()
        for b, n in enumerate(d["input_lengths"]):        # beyond an utterance's length: exactly zero in the encoder's input
            assert np.all(ref[b, int(n):] == 0)
    hold(fix, grads, tag)


def test_differentiable_call_returns_the_same_bits_and_a_plain_call_stays_detached():
    from facppg import lib as flib
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    x = inputs_of(d, ppg, tgt)
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    plain = m(x, dropout_masks=(enc, dec))
    assert all(t.grad_fn is None and not t.requires_grad for t in plain)
    with torch.no_grad():
        quiet = m(x, dropout_masks=(enc, dec))
    diff = m(x, dropout_masks=(enc, dec), differentiable=True)
    assert all(t.grad_fn is not None for t in diff[:3]) and not diff[3].requires_grad
    for a, b, c in zip(plain, quiet, diff):
        assert torch.equal(a, b) and torch.equal(a, c.detach())
    # the masks the kernels draw from a seed are the ones the backward pass sees
    s1, s2 = m(x, seed=5), m(x, seed=5, differentiable=True)
    assert all(torch.equal(a, b.detach()) for a, b in zip(s1, s2))
    with torch.no_grad():
        with pytest.raises(flib.FacppgError, match="no_grad"):
            m(x, dropout_masks=(enc, dec), differentiable=True)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(flib.FacppgError, match="no parameter requires a gradient"):
        m(x, dropout_masks=(enc, dec), differentiable=True)


def test_seeded_draws_reach_the_backward_pass():
    """seed= and utterance_seeds= (no masks given): the gradient equals the one under the same masks passed explicitly."""
    from common.loss_function import Tacotron2Loss
    d, hp, sd, ppg, tgt, gate_t, _, _ = forced_case("dup")
    m = build(hp, sd)
    x, y = inputs_of(d, ppg, tgt), (tgt.cuda(), gate_t.cuda())
    B, Tin, T = ppg.shape[0], ppg.shape[2], tgt.shape[2]
    enc_m, _ = m.draw_dropout_masks([5, 6], Tin, steps=1)
    dec_m = torch.empty(2, B, hp.prenet_dim, T, dtype=torch.uint8, device="cuda")
    from facppg import lib as flib
    sd_t = torch.tensor([5, 6], dtype=torch.int64, device="cuda")
    flib.check(flib.load().facppg_taco_draw_dropout_forced(m._handle(torch.device("cuda", 0)), flib.ptr(sd_t), B, T, flib.ptr(dec_m),
                                                           flib.current_stream(torch.device("cuda", 0))))
    masks = (enc_m.permute(0, 1, 3, 2), torch.cat([dec_m.permute(0, 3, 1, 2), dec_m.new_zeros(2, 1, B, hp.prenet_dim)], 1))
    grads = []
    for kw in ({"utterance_seeds": [5, 6]}, {"dropout_masks": masks}):
        m.zero_grad()
        Tacotron2Loss()(m(x, differentiable=True, **kw), y).backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_inference_is_untouched_by_a_differentiable_forward_and_backward():
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    xi = ppg[:1].cuda()
    before = m.inference(xi, seed=3, step_limits=[25])
    loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec)
    after = m.inference(xi, seed=3, step_limits=[25])
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    assert torch.equal(before.out_lengths, after.out_lengths)


def test_two_backward_passes_give_the_same_bits():
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    _, g1 = loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec)
    _, g2 = loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec)
    diff = [n for n in g1 if not np.array_equal(g1[n], g2[n])]
    assert not diff, diff


@pytest.mark.parametrize("shape", ["U=150", "U=8", "chunks", "no_regw"])
def test_every_forward_launch_shape_feeds_the_same_backward(shape, monkeypatch):
    """The backward kernels have ONE launch shape each (16 columns x 64 K-parts per workgroup, one launch per frame; the
    launch report lists them); what varies is the forward pass that saves their state: forced slice widths, a batch in chunks
    of co-resident utterances, streamed instead of register-resident chain slices.  Each is held to the same fixture."""
    tag = "dup" if shape == "no_regw" else "ragged"
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case(tag)
    m = build(hp, sd)
    B = ppg.shape[0]
    if shape.startswith("U="):
        monkeypatch.setenv("FACPPG_DECODER_COOP_U", shape[2:])
        want = B * 2 * ((hp.attention_rnn_dim + int(shape[2:]) - 1) // int(shape[2:]))
    elif shape == "chunks":
        m.decoder_workgroups, want = 4, 4
    else:
        monkeypatch.setenv("FACPPG_FORCED_NO_REGW", "1")
        want = 2 * (38 + 38)
    _, grads = loss_and_grads(m, d, ppg, tgt, gate_t, enc, dec)
    assert m.last_decoder_launch() == ("coop", want)
    assert m.last_backward_launches == expected_launches(hp, B, ppg.shape[2], tgt.shape[2])
    hold(bh.grad_fixture(tag), grads, shape)


def test_batch_of_one_equals_its_row_of_the_dup_batch():
    """B = 1 (the reference's own forward fails there): torch.autograd.grad of utterance 0 alone, under row 0's masks, for
    seeded output gradients, against the dup batch given the same output gradients on row 0 and zeros on row 1.  Equal
    lengths and eval-mode BatchNorm: the rows do not interact.  Whole tensors, relative L2, the tolerance of the fixtures."""
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("dup")
    m = build(hp, sd)
    g = torch.Generator().manual_seed(5)
    seeds = [torch.randn(1, 80, 30, generator=g).cuda(), torch.randn(1, 80, 30, generator=g).cuda(), torch.randn(1, 30, generator=g).cuda()]
    params = list(m.parameters())
    x1 = (ppg[:1].cuda(), torch.tensor([24]).cuda(), tgt[:1].cuda(), 24, torch.tensor([30]).cuda())
    o1 = m(x1, dropout_masks=(enc[:, :1], dec[:, :, :1]), differentiable=True)
    g1 = torch.autograd.grad(o1[:3], params, seeds)
    o2 = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec), differentiable=True)
    g2 = torch.autograd.grad(o2[:3], params, [torch.cat([s, torch.zeros_like(s)], 0) for s in seeds])
    dev = [float((a - b).double().norm() / b.double().norm()) for a, b in zip(g1, g2)]
    print("B=1 vs dup row 0: worst %.2e" % max(dev))
    assert len(dev) == 61 and max(dev) <= bh.tolerance()


class Utterances(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def ragged_run(steps, first=0, **kw):
    """finetune on the ragged batch with the fixture's per-step mask seeds (1000 + s / 2000 + s at step s)."""
    from common.data_utils import ppg_acoustics_collate
    from script.train_ppg2mel import finetune
    d, hp, sd, ppg, tgt, _, _, _ = forced_case("ragged")
    B, Tin, T = ppg.shape[0], ppg.shape[2], tgt.shape[2]
    m = kw.pop("model", None) or build(hp, sd)

    def masks(s):
        return (masks_from_seed(1000 + first + s, (2, B, Tin, hp.symbols_embedding_dim)),
                masks_from_seed(2000 + first + s, (2, T + 1, B, hp.prenet_dim)))
    hp.batch_size = 3
    res = finetune(m, hp, Utterances(forced_utterances(d)), ppg_acoustics_collate, steps, step_masks=masks, log=None, **kw)
    return m, hp, res


def test_finetune_follows_the_reference_trajectory(tmp_path):
    fix = golden("tacotron_finetune_ragged.npz")
    assert float(fix["learning_rate"]) == 1e-4 and int(fix["steps"]) == 8
    m, hp, res = ragged_run(8)
    assert hp.learning_rate == 1e-4 and hp.weight_decay == 1e-6 and hp.grad_clip_thresh == 1.0
    loss_dev = np.abs(np.array(res["losses"]) - fix["loss"]) / fix["loss"]
    norm_dev = np.abs(np.array(res["grad_norms"]) - fix["grad_norm"]) / fix["grad_norm"]
    tol = bh.C_LOSS * float(fix["loss_dev32"])
    print("finetune losses", " ".join("%.4f" % v for v in res["losses"]))
    print("finetune: loss deviation %.2e (fixture's float32 run %.2e, tolerance %.2e), grad-norm deviation %.2e"
          % (loss_dev.max(), float(fix["loss_dev32"]), tol, norm_dev.max()))
    assert tol <= bh.CAP and loss_dev.max() <= tol
    assert norm_dev.max() <= bh.tolerance()
    opt = res["optimizer"]
    assert not opt._hip_off and opt._hip                      # every step was the HIP launch: all 61 tensors had a gradient
    assert all(p.grad is not None for p in m.parameters()) and len(list(m.parameters())) == 61
    # the packed-weight handle followed the weights: inference equals that of a fresh model loaded from the state dict
    xi = forced_case("ragged")[3][:1].cuda()
    fresh = build(hp, {k: v.clone() for k, v in m.state_dict().items()})
    a, b = m.inference(xi, seed=3, step_limits=[20]), fresh.inference(xi, seed=3, step_limits=[20])
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_checkpoint_round_trip_resumes_bit_for_bit(tmp_path):
    from script.train_ppg2mel import load_checkpoint, save_checkpoint
    from waveglow.optim import Adam
    m, hp, res = ragged_run(3)
    path = os.path.join(str(tmp_path), "checkpoint_2")
    save_checkpoint(m, res["optimizer"], res["learning_rate"], res["iteration"] - 1, path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["iteration", "learning_rate", "optimizer", "state_dict"] and ck["iteration"] == 2
    _, _, straight = ragged_run(1, first=3, model=m, optimizer=res["optimizer"])
    d, hp2, sd, _, _, _, _, _ = forced_case("ragged")
    m2 = build(hp2, sd)
    opt2 = Adam(m2.parameters(), lr=hp2.learning_rate, weight_decay=hp2.weight_decay)
    m2b, opt2b, lr, it = load_checkpoint(path, m2, opt2)
    assert it == 2 and lr == res["learning_rate"]
    _, _, resumed = ragged_run(1, first=3, model=m2, checkpoint_path=path, optimizer=opt2)
    assert resumed["iteration"] == 4
    print("resumed loss %.8f uninterrupted %.8f" % (resumed["losses"][0], straight["losses"][0]))
    assert resumed["losses"][0] == straight["losses"][0]
    assert resumed["grad_norms"][0] == straight["grad_norms"][0]
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), m2.parameters()))
