"""GPU parity: the teacher-forced Tacotron2.forward (padded-batch encoder, hoisted prenet / projection GEMMs, the
teacher-forced recurrent kernel, padded-batch postnet, parse_output masking) against the imported reference's forward
with the same injected dropout masks (tests/golden/make_golden_forced.py).  Tolerance: 1e-4 absolute, what every Tacotron
golden test of this repository holds (test_gpu_tacotron.py).  A per-utterance implementation (the inference path's
semantics) misses the ragged fixture by 0.5 or more."""
import numpy as np
import pytest
import torch

from forced_helpers import forced_case, forced_utterances, loss_tolerance

pytestmark = pytest.mark.gpu
EPS = 1e-4


def build(hp, sd):
    from script.train_ppg2mel import load_model
    m = load_model(hp)
    m.load_state_dict(sd, strict=True)
    return m.eval()


def inputs_of(d, ppg, tgt):
    il, ol = torch.tensor(d["input_lengths"]).long().cuda(), torch.tensor(d["output_lengths"]).long().cuda()
    return (ppg.cuda(), il, tgt.cuda(), int(il.max()), ol)


def check_against(d, m, out, rows=None, tag=""):
    """mel, mel_post, gate, alignments and the encoder memory within EPS of the fixture (rows: the fixture rows the batch
    holds); masked part exactly 0 / exactly 1e3; the alignments' zero pattern equal to the reference's."""
    rows = list(range(d["mel"].shape[0])) if rows is None else rows
    mel, mel_post, gate, align = [t.cpu().numpy() for t in out]
    ref = {k: d[k][rows] for k in ("mel", "mel_post", "gate", "align", "memory")}
    assert mel.shape == ref["mel"].shape and mel_post.shape == ref["mel_post"].shape
    assert gate.shape == ref["gate"].shape and align.shape == ref["align"].shape
    err = {"memory": np.abs(m.last_memory.cpu().numpy() - ref["memory"]).max(), "mel": np.abs(mel - ref["mel"]).max(),
           "mel_post": np.abs(mel_post - ref["mel_post"]).max(), "align": np.abs(align - ref["align"]).max()}
    valid = np.arange(gate.shape[1])[None, :] < np.asarray(d["output_lengths"])[rows][:, None]
    err["gate"] = np.abs(gate - ref["gate"])[valid].max()
    print(tag, " ".join("%s %.2e" % kv for kv in sorted(err.items())))
    assert all(e <= EPS for e in err.values()), err
    pad3 = np.broadcast_to(~valid[:, None, :], mel.shape)
    assert np.all(mel[pad3] == 0.0) and np.all(mel_post[pad3] == 0.0)
    assert np.all(gate[~valid] == np.float32(1e3))
    assert np.array_equal(align == 0, ref["align"] == 0)


@pytest.mark.parametrize("tag", ["ragged", "dup", "mono40"])
def test_forward_matches_reference_golden(tag):
    from common.loss_function import Tacotron2Loss
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case(tag)
    m = build(hp, sd)
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    check_against(d, m, out, tag=tag)
    # the loss on the product's outputs: the bound follows from EPS and the fixture (forced_helpers.loss_tolerance)
    loss = float(Tacotron2Loss()(out, (tgt.cuda(), gate_t.cuda())).double())
    tol = loss_tolerance(d, tgt, EPS)
    print(tag, "loss %.7f reference %.7f |diff| %.2e tol %.2e" % (loss, float(d["loss"]), abs(loss - float(d["loss"])), tol))
    assert abs(loss - float(d["loss"])) <= tol


@pytest.mark.parametrize("U", [8, 20, 40, 75, 150])
def test_every_slice_width_matches_the_ragged_fixture(U, monkeypatch):
    """The recurrent kernel at every LSTM slice width it is launched with: 38 / 15 / 8 / 4 / 2 attention-chain workgroups per
    utterance and, under the forced width, as many decoder-LSTM workgroups."""
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", str(U))
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    assert m.last_decoder_launch() == ("coop", 3 * 2 * ((hp.attention_rnn_dim + U - 1) // U))
    check_against(d, m, out, tag="U=%d" % U)


def test_batch_in_chunks_of_co_resident_utterances():
    """A bound of 4 workgroups holds one utterance (2 attention-chain + 2 decoder-LSTM workgroups): three launches, one after
    the other."""
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    m.decoder_workgroups = 4
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    assert m.last_decoder_launch() == ("coop", 4)
    check_against(d, m, out, tag="chunks")


def test_mixed_slice_widths():
    """What the automatic choice gives at the reference's batch sizes: chain slices of one width, decoder-LSTM slices of the
    next (here 38 workgroups of 8 units + 15 of 20 per utterance, under a bound of 3 * 53 workgroups)."""
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    m.decoder_workgroups = 3 * (38 + 15)
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    assert m.last_decoder_launch() == ("coop", 3 * (38 + 15))
    check_against(d, m, out, tag="38+15")


def test_short_last_chunk_takes_narrower_slices():
    """A bound of 8 workgroups: two utterances at 2 + 2 workgroups each, then the third alone at 4 + 4."""
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    m.decoder_workgroups = 8
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    assert m.last_decoder_launch() == ("coop", 8)
    check_against(d, m, out, tag="chunks 2+1")


@pytest.mark.parametrize("regw", [True, False])
def test_register_resident_chain_and_its_switch(regw, monkeypatch):
    """B <= 2: 75 chain workgroups per utterance with their attention-LSTM slice in registers (+ 38 decoder-LSTM workgroups);
    FACPPG_FORCED_NO_REGW=1 keeps the streamed slices (38 + 38)."""
    if not regw:
        monkeypatch.setenv("FACPPG_FORCED_NO_REGW", "1")
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("dup")
    m = build(hp, sd)
    out = m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    assert m.last_decoder_launch() == ("coop", 2 * (75 + 38) if regw else 2 * (38 + 38))
    check_against(d, m, out, tag="regw=%s" % regw)


def test_batch_of_one():
    """B = 1 (the reference's own forward fails there, model.py:481): row 0 of the dup fixture under row 0's draws."""
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("dup")
    m = build(hp, sd)
    x = (ppg[:1].cuda(), torch.tensor([24]).cuda(), tgt[:1].cuda(), 24, torch.tensor([30]).cuda())
    out = m(x, dropout_masks=(enc[:, :1], dec[:, :, :1]))
    assert out[0].shape == (1, 80, 30) and out[2].shape == (1, 30) and out[3].shape == (1, 30, 24)
    check_against(d, m, out, rows=[0], tag="B=1")


def test_forward_through_collate_and_parse_batch():
    """Unsorted (ppg, acoustic) pairs: the collate sorts them into the ragged fixture's order."""
    from common.data_utils import ppg_acoustics_collate
    d, hp, sd, _, _, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    u = forced_utterances(d)
    x, y = m.parse_batch(ppg_acoustics_collate([u[1], u[2], u[0]]))
    assert x[0].is_cuda and x[3] == 30 and y[0].is_cuda and y[1].shape == (3, 48)
    out = m(x, dropout_masks=(enc, dec))
    check_against(d, m, out, tag="collate")


def test_lengths_must_be_descending():
    from facppg import lib as flib
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    x = (ppg.cuda(), torch.tensor([30, 9, 22]).cuda(), tgt.cuda(), 30, torch.tensor([37, 48, 12]).cuda())
    with pytest.raises(flib.FacppgError, match="descending"):
        m(x, dropout_masks=(enc, dec))


def test_validate_returns_the_mean_fixture_loss(capsys):
    """validate() over a list data set of two batches (the ragged fixture's three utterances, then the dup fixture's two):
    the mean of the two fixture losses; the model is left in train() mode, as the reference leaves it, where forward
    raises.  The dropout draws are injected per batch, as the fixture generator injects them into the reference."""
    from common.data_utils import ppg_acoustics_collate
    from common.loss_function import Tacotron2Loss
    from facppg import lib as flib
    from script.train_ppg2mel import validate
    dr, hp, sd, _, tgt_r, _, enc_r, dec_r = forced_case("ragged")
    dd, _, _, _, tgt_d, _, enc_d, dec_d = forced_case("dup")
    m = build(hp, sd)
    masks = {30: (enc_r, dec_r), 24: (enc_d, dec_d)}                # by padded PPG length
    plain = m.forward
    m.forward = lambda x: plain(x, dropout_masks=masks[x[0].shape[2]])
    valset = forced_utterances(dr) + forced_utterances(dd)
    loss = validate(m, Tacotron2Loss(), valset, 7, 3, 1, ppg_acoustics_collate, None, False, 0)
    want = 0.5 * (float(dr["loss"]) + float(dd["loss"]))
    tol = 0.5 * (loss_tolerance(dr, tgt_r, EPS) + loss_tolerance(dd, tgt_d, EPS))
    print("validate %.7f want %.7f |diff| %.2e tol %.2e" % (loss, want, abs(loss - want), tol))
    assert abs(loss - want) <= tol
    assert "Validation loss 7: %9f" % loss in capsys.readouterr().out
    assert m.training
    del m.forward
    with pytest.raises(flib.FacppgError, match="backward pass is not built"):
        m((None,) * 5)


def test_seeds():
    """Same seed -> identical outputs; under utterance_seeds utterance b's result does not depend on its neighbours' seeds."""
    d, hp, sd, ppg, tgt, _, _, _ = forced_case("ragged")
    m = build(hp, sd)
    x = inputs_of(d, ppg, tgt)
    a, b, c = m(x, seed=11), m(x, seed=11), m(x, seed=12)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(a[0], c[0])
    u1, u2, u3 = m(x, utterance_seeds=[5, 6, 7]), m(x, utterance_seeds=[5, 6, 7]), m(x, utterance_seeds=[5, 9, 7])
    assert all(torch.equal(p, q) for p, q in zip(u1, u2))
    for p, q in zip(u1, u3):
        assert torch.equal(p[0], q[0]) and torch.equal(p[2], q[2])
    assert not torch.equal(u1[0][1], u3[0][1])


def test_inference_is_untouched_by_a_forward_on_the_same_model():
    d, hp, sd, ppg, tgt, _, enc, dec = forced_case("ragged")
    m = build(hp, sd)
    xi = ppg[:1].cuda()
    before = m.inference(xi, seed=3, step_limits=[25])
    m(inputs_of(d, ppg, tgt), dropout_masks=(enc, dec))
    after = m.inference(xi, seed=3, step_limits=[25])
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    assert torch.equal(before.out_lengths, after.out_lengths)
