"""The one-barrier worker stages of k_decoder_split (a row's K parts meet inside a half-wave, operand vectors in a padded K-part
layout read as float4, a pause between publishing and polling) and the main workgroup's LDS-resident query-weight rows, against
the stages they replaced (FACPPG_DECODER_STEP=legacy: stat_mv16n's two barriers per matvec, every query-weight row requested per
frame).  Every sum keeps its operands and its order, so mel, gate, alignments and output lengths are equal BIT FOR BIT.  Seeded
synthetic weights at the reference's layer widths (the split shape needs them)."""
import numpy as np
import pytest
import torch

from facppg import synth
from helpers import masks_from_seed
from stream_helpers import HOP, acoustic, make_vocoder, run, utterance

pytestmark = pytest.mark.gpu

NS = 5816
_models = {}


def model(steps, gate_bias):
    if (steps, gate_bias) not in _models:
        _models[(steps, gate_bias)] = acoustic(steps, gate_bias)
    return _models[(steps, gate_bias)]


def batch(lens, seed0):
    x = torch.zeros(len(lens), NS, max(lens))
    for b, n in enumerate(lens):
        x[b, :, :n] = torch.from_numpy(synth.synthetic_ppg(n, NS, seed=seed0 + b, alpha=0.002)).t()
    return x.cuda()


def both_steps(taco, monkeypatch, x, **kw):
    """One inference with the default stages and one with the legacy ones -> the two results, checked to be the split decoder's."""
    monkeypatch.setenv("FACPPG_DECODER_MODE", "split")
    res = []
    for step in (None, "legacy"):
        if step:
            monkeypatch.setenv("FACPPG_DECODER_STEP", step)
        else:
            monkeypatch.delenv("FACPPG_DECODER_STEP", raising=False)
        out = taco.inference(x, **kw)
        mel, mel_post, gate, align = out
        assert out.launch.mode == "split" and out.launch.step == (2 if step else 1)      # the kernel the setting names really ran
        res.append((mel.clone(), gate.clone(), align.clone(), taco.last_output_lengths.clone(), taco.last_decoder_launch()[1]))
    return res


def assert_same(new, old):
    assert new[4] == old[4]                                      # the same launch shape (workgroups)
    assert torch.equal(new[3], old[3]), (new[3], old[3])         # output lengths
    assert torch.count_nonzero(new[0]) > 0
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])


@pytest.mark.parametrize("Tin", [1, 2, 3, 17, 45])
def test_one_utterance_equals_legacy(Tin, monkeypatch):
    """B = 1: the first frames (all operands zero, nothing gathered), and at Tin = 45 with 60 steps a window (41 wide) that
    slides over the memory and past its end."""
    steps = 60 if Tin == 45 else 12
    hp, taco = model(steps, -10.0)
    em, dm = masks_from_seed(41, (2, 1, Tin, hp.symbols_embedding_dim)), masks_from_seed(42, (steps, 2, 1, hp.prenet_dim))
    new, old = both_steps(taco, monkeypatch, batch([Tin], 60 + Tin), dropout_masks=(em, dm))
    assert new[0].shape[2] == steps and new[4] == 76
    assert_same(new, old)


@pytest.mark.parametrize("lens,wgs,nu", [([19, 11], None, 1), ([19, 11], 80, 2), ([13, 19, 7], None, 1), ([13, 19, 7], 80, 3)])
def test_ragged_batch_equals_legacy(lens, wgs, nu, monkeypatch):
    """B = 2 and 3 with unequal lengths, one worker set per utterance (NU = 1) and, with the decoder held to 80 workgroups,
    one set for all of them (NU = 2, 3: 75 workers + NU mains)."""
    steps, B = 14, len(lens)
    hp, taco = model(steps, -10.0)
    em, dm = masks_from_seed(43, (2, B, max(lens), hp.symbols_embedding_dim)), masks_from_seed(44, (steps, 2, B, hp.prenet_dim))
    new, old = both_steps(taco, monkeypatch, batch(lens, 80), lengths=lens, dropout_masks=(em, dm), decoder_workgroups=wgs)
    assert new[4] == (75 + nu) * (B // nu)
    assert_same(new, old)


def test_utterances_of_one_group_stop_at_different_frames(monkeypatch):
    """A gate bias at which the gate fires on its own: three utterances share one worker set (NU = 3) and stop at different
    frames -- the `alive` mask, and workers that go on for the survivors."""
    steps, lens = 48, [24, 9, 17]
    hp, taco = model(steps, -0.02)
    em, dm = masks_from_seed(45, (2, 3, max(lens), hp.symbols_embedding_dim)), masks_from_seed(46, (steps, 2, 3, hp.prenet_dim))
    new, old = both_steps(taco, monkeypatch, batch(lens, 90), lengths=lens, dropout_masks=(em, dm), decoder_workgroups=80)
    out_lens = new[3].tolist()
    print("stop frames", out_lens)
    assert new[4] == 78 and len(set(out_lens)) > 1 and min(out_lens) < steps      # the case is what it claims to be
    assert_same(new, old)


def test_step_limits_end_utterances_of_one_group_apart(monkeypatch):
    """The same through per-utterance step limits (the stop no gate decides), the last utterance running to max_decoder_steps:
    the extra pass with t = max_steps that forms a prenet row nobody reads."""
    steps, lens, limits = 16, [12, 20, 8], [5, 11, 16]
    hp, taco = model(steps, -10.0)
    em, dm = masks_from_seed(47, (2, 3, max(lens), hp.symbols_embedding_dim)), masks_from_seed(48, (steps, 2, 3, hp.prenet_dim))
    new, old = both_steps(taco, monkeypatch, batch(lens, 100), lengths=lens, dropout_masks=(em, dm), step_limits=limits,
                          decoder_workgroups=80)
    assert new[3].tolist() == limits and new[4] == 78
    assert_same(new, old)


def test_max_decoder_steps_is_reached(monkeypatch):
    """An utterance whose gate never fires: max_decoder_steps frames, then the pass with t = max_steps that only stops."""
    steps, Tin = 9, 30
    hp, taco = model(steps, -10.0)
    em, dm = masks_from_seed(49, (2, 1, Tin, hp.symbols_embedding_dim)), masks_from_seed(50, (steps, 2, 1, hp.prenet_dim))
    new, old = both_steps(taco, monkeypatch, batch([Tin], 110), dropout_masks=(em, dm))
    assert new[3].tolist() == [steps]
    assert_same(new, old)


@pytest.mark.parametrize("how", ["seed", "utterance_seeds"])
def test_device_drawn_masks_equal_legacy(how, monkeypatch):
    """The masks the library draws itself: one seed for the call, and one seed per utterance."""
    steps, lens = 14, [15, 22]
    hp, taco = model(steps, -10.0)
    kw = dict(seed=1234) if how == "seed" else dict(utterance_seeds=[77, 78])
    new, old = both_steps(taco, monkeypatch, batch(lens, 120), lengths=lens, **kw)
    assert_same(new, old)


def test_streamed_utterance_equals_legacy(monkeypatch):
    """One streamed utterance of 130 frames through pipeline.synthesize: the tagged frame words still arrive (the call is
    streamed and published) and the samples are equal under both settings."""
    monkeypatch.setenv("FACPPG_DECODER_MODE", "split")
    cfg, wg, den = make_vocoder()
    steps = Tin = 130
    hp, taco = model(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=23)
    outs = []
    for step in (None, "legacy"):
        if step:
            monkeypatch.setenv("FACPPG_DECODER_STEP", step)
        else:
            monkeypatch.delenv("FACPPG_DECODER_STEP", raising=False)
        out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
        assert seen["streamed"] and seen["published"] and t_out == steps
        launch = taco.__dict__["_last_launch"]
        assert launch.mode == "split" and launch.step == (2 if step else 1)
        outs.append((out, seen["mel_post"]))
    assert outs[0][0].shape == (steps * HOP,) and np.abs(outs[0][0]).max() > 0
    assert np.array_equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
