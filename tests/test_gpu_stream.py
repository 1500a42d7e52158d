"""GPU: the streamed batch-1 path (facppg.pipeline.ConditioningStream: the postnet and the conditioning part of every WaveNet
layer's gate GEMM run on a second stream WHILE the split decoder is still producing frames) against the path it replaces --
the same utterance with FACPPG_STREAM=0 -- bit for bit, at lengths that end on and off block boundaries, with the decoder
running to its step limit and stopping early on its gate (blocks that never become final are void)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from facppg import synth
from helpers import masks_from_seed
from stream_helpers import HOP, acoustic, late_encode, make_vocoder, run, utterance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocoder():
    return make_vocoder()


@pytest.mark.parametrize("Tin,steps,gate_bias", [(200, 200, -10.0), (170, 170, -10.0), (96, 96, -10.0), (75, 75, -10.0),
                                                 (130, 400, -10.0), (150, 200, -10.0), (150, 1000, -0.02), (64, 64, -10.0)])
def test_streamed_utterance_equals_the_unstreamed_path_bit_for_bit(vocoder, Tin, steps, gate_bias, monkeypatch):
    from facppg.pipeline import ConditioningStream
    cfg, wg, den = vocoder
    if Tin == 96:                  # (the optional mode of the stream: unbounded seed passes)
        monkeypatch.setenv("FACPPG_STREAM_SPARE_CUS", "-1")
    hp, taco = acoustic(steps, gate_bias)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    ref, t_ref, seen_ref = run(taco, wg, den, ppg, em, dm, None, False, monkeypatch)
    zs = synth.synthetic_z(1, t_ref * HOP // 8, cfg, seed=23)
    ref, t_ref, seen_ref = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    # the buffers are laid out for the PPG's length + SLACK frames: an utterance the decoder takes further (130 frames in, 400 out)
    # is finished by the one-shot postnet and the ordinary vocoder
    cap = min(steps, -(-(Tin + ConditioningStream.SLACK) // 32) * 32)
    assert not seen_ref["streamed"] and seen["streamed"] == (min(steps, Tin) >= 64 and t_ref <= cap)
    assert not seen_ref["published"] and seen["published"] == (min(steps, Tin) >= 64)
    assert taco.last_decoder_launch()[0] == "split"
    assert t_out == t_ref and (gate_bias > -1 or t_ref == steps)
    cs = wg.__dict__["_facppg_cond_stream"]
    print("Tin %d steps %d: Tout %d, streamed %s, blocks %s, %.2f GB held" % (Tin, steps, t_out, seen["streamed"],
                                                                             cs.cuts if seen["streamed"] else None, cs.footprint_bytes() / 1e9))
    assert torch.equal(seen["mel_post"], seen_ref["mel_post"])                     # the streaming postnet: same bits
    assert out.shape == ref.shape == (t_ref * HOP,) and np.array_equal(out, ref)    # ... and so the samples


def test_fp32_tail_by_one_more_pass_or_inside_the_layer_launches_same_bits(vocoder, monkeypatch):
    """75 frames: 64 seeded under the decoder and an 11-frame, half-filled tail tile -- the shortest utterance with both a
    seeded part and a ragged tail.  The tail gets its seeds from one more pass in front of the vocoder (FACPPG_STREAM_TAIL=seed:
    frames [64, 96), every layer launch all-seeded 32-frame tiles) or runs unseeded inside the layer launches (the default at
    this length: k_wn_layer_mixed, two seeded 32-frame tiles and one 16-frame tile per phase); both equal the unstreamed path bit
    for bit.  (At 75 frames both launches have 3 tiles per phase, so last_launch_shape() reads the same for either; which side
    ran is read off the calls the stream made on the vocoder.)"""
    cfg, wg, den = vocoder
    Tin = steps = 75
    P = HOP // 8
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=23)
    ref, t_ref, seen_ref = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    assert not seen_ref["streamed"] and t_ref == steps
    calls = []
    cond_seed, infer_seeded = wg.cond_seed, wg.infer_seeded

    def spy_seed(melp, T, frame0, nframes, seeds, block_tiles=1, layers_per_workgroup=4, max_workgroups=0, **kw):
        calls.append(("seed", frame0, nframes, block_tiles, layers_per_workgroup, max_workgroups > 0))
        return cond_seed(melp, T, frame0, nframes, seeds, block_tiles=block_tiles, layers_per_workgroup=layers_per_workgroup,
                         max_workgroups=max_workgroups, **kw)

    def spy_infer(melp, T, seeds, seeded_frames, **kw):
        calls.append(("infer", T, seeded_frames))
        return infer_seeded(melp, T, seeds, seeded_frames, **kw)
    wg.cond_seed, wg.infer_seeded = spy_seed, spy_infer
    outs = {}
    try:
        for tail in ("seed", None):
            if tail is None:
                monkeypatch.delenv("FACPPG_STREAM_TAIL", raising=False)
            else:
                monkeypatch.setenv("FACPPG_STREAM_TAIL", tail)
            del calls[:]
            out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
            cs = wg.__dict__["_facppg_cond_stream"]
            print("tail %s: seeded %d, blocks %s, calls %s, launch shape %s" % (tail, cs.seeded, cs.cuts, calls, wg.last_launch_shape()))
            assert seen["streamed"] and t_out == t_ref and not cs.half and cs.void_blocks == 0
            assert cs.seeded == 64                               # frames seeded under the decoder, before any tail pass
            outs[tail] = (out, list(calls), wg.last_launch_shape())
    finally:
        del wg.cond_seed, wg.infer_seeded
    under_decoder = [("seed", 0, 32, 1, 1, True), ("seed", 32, 32, 1, 1, True)]      # two bounded passes, one per planned block
    # the default: nothing more in front of the vocoder, whose launches carry the tail as a 16-frame tile behind two seeded ones
    assert outs[None][1] == under_decoder + [("infer", 75, 64)]
    assert outs[None][2] == (32, 8, P * (64 // 32 + -(-(75 - 64) // 16)))
    # seed: one more, unbounded pass over the tail tile, then all 32-frame tiles
    assert outs["seed"][1] == under_decoder + [("seed", 64, 32, 1, 2, False), ("infer", 75, 96)]
    assert outs["seed"][2] == (32, 8, 3 * 32)
    assert np.array_equal(outs["seed"][0], ref) and np.array_equal(outs[None][0], ref) and np.array_equal(outs["seed"][0], outs[None][0])


def test_blocks_that_time_out_are_redone_behind_the_decoder(vocoder, monkeypatch):
    """k_collect_frames gives a block up when its frames do not arrive within FACPPG_STREAM_WAIT_MS (a profiler that serialises
    kernels, a cooperative launch queued behind another process): the block and every block behind it is void -- no postnet
    columns, no seeds.  The host reads the flags back with the length and redoes those frames behind the decoder: late, not wrong.
    With a 1 us limit every block times out; the samples must still equal the unstreamed path's bit for bit."""
    cfg, wg, den = vocoder
    Tin = steps = 200
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 5, mask_seeds=(61, 62))
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=63)
    ref, t_ref, _ = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    cs = wg.__dict__["_facppg_cond_stream"]
    assert seen["streamed"] and cs.void_blocks == 0 and np.array_equal(out, ref)
    monkeypatch.setenv("FACPPG_STREAM_WAIT_MS", "0.001")
    late_encode(monkeypatch)     # (the frames must really be late)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    print("blocks", cs.cuts, "void", cs.void_blocks, "seeded frames", cs.seeded)
    assert seen["streamed"] and cs.void_blocks > 0 and cs.seeded < 160
    assert t_out == t_ref and np.array_equal(out, ref)


def test_a_decode_inside_a_streamed_call_publishes_nothing_into_it(vocoder, monkeypatch):
    """The frame words and the launch report travel with each facppg_taco_decode call, not on the shared handle.  A second,
    unstreamed B = 1 call on the same model inside a streamed call's window -- frame words zeroed, decoder not launched yet: what a
    second thread on the same models may do -- leaves those words alone, and each utterance equals its own serial, unstreamed
    result bit for bit.  The nested call runs from the streamed call's encode, where the window is open."""
    cfg, wg, den = vocoder
    Tin = steps = 200
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 8, mask_seeds=(81, 82))
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=83)
    x2 = torch.from_numpy(synth.synthetic_ppg(Tin, 5816, seed=9, alpha=0.002).T.copy()).unsqueeze(0).cuda()
    em2 = masks_from_seed(84, (2, 1, Tin, hp.symbols_embedding_dim))
    dm2 = masks_from_seed(85, (steps, 2, 1, hp.prenet_dim))
    inference = taco.inference

    def second_utterance():
        with contextlib.redirect_stdout(io.StringIO()):
            out = inference(x2, dropout_masks=(em2, dm2))
        return [o.cpu().numpy() for o in out], out.launch
    serial, _ = second_utterance()
    ref, t_ref, _ = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    from facppg import lib as flib
    L = flib.load()
    encode = L.facppg_taco_encode
    nested = {}

    def encode_then_second_utterance(*a):
        rc = encode(*a)
        if not nested:                                   # (the nested call's own encode is the real one)
            nested["running"] = True
            words = wg.__dict__["_facppg_cond_stream"].words
            nested["outputs"], nested["launch"] = second_utterance()
            nested["words_untouched"] = not bool((words != 0).any())
        return rc
    monkeypatch.setattr(L, "facppg_taco_encode", encode_then_second_utterance)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    assert seen["streamed"] and "launch" in nested
    assert nested["words_untouched"]                     # the nested decode published nothing into the streamed call's words
    assert nested["launch"].mode == "split" and not nested["launch"].streamed
    assert t_out == t_ref and np.array_equal(out, ref)
    assert all(np.array_equal(a, b) for a, b in zip(nested["outputs"], serial))


def test_stream_footprint_follows_the_utterance_not_the_step_limit(vocoder, monkeypatch):
    """The default max_decoder_steps is 1000: the stream must not hold 6.4 GB of seeds for a 2 s utterance.  Its buffers are laid
    out for the PPG's length + 64 frames, grow only, and the side streams are created once."""
    cfg, wg, den = vocoder
    hp, taco = acoustic(1000, -10.0)
    wg.__dict__.pop("_facppg_cond_stream", None)
    held = []
    for Tin in (136, 200, 150):
        ppg, em, dm = utterance(hp, Tin, Tin, Tin, mask_seeds=(71, 72))
        from facppg import pipeline
        monkeypatch.setenv("FACPPG_STREAM", "1")
        with contextlib.redirect_stdout(io.StringIO()):
            wavs, tout = pipeline.synthesize([ppg], taco, wg, den, sigma=0.6, strength=0.005, dropout_masks=(em, dm), step_limits=[Tin], seed=3)
        cs = wg.__dict__["_facppg_cond_stream"]
        held.append((cs.footprint_bytes(), cs.side, cs.cap))
        assert tout[0] == Tin and cs.cap == Tin                      # (step_limits bounds the layout too)
    print("held GB:", ["%.2f" % (h[0] / 1e9) for h in held])
    assert held[1][0] <= 2.0e9 and held[2][0] == held[1][0] and held[2][1] is held[0][1]


def test_stream_buffers_are_reused_across_utterances(vocoder, monkeypatch):
    """The stream's buffers (frame words, void flags, work counters, mel buffer, seeds) live with the models and are reused by
    every utterance of the same step limit: three different utterances in a row, each streamed and unstreamed, and the first one
    again at the end -- every streamed result equals its unstreamed one bit for bit (nothing of an earlier utterance leaks)."""
    cfg, wg, den = vocoder
    steps = 136
    hp, taco = acoustic(steps, -10.0)
    cases = []
    for i, Tin in enumerate((136, 90, 120)):
        ppg, em, dm = utterance(hp, Tin, steps, 70 + i, mask_seeds=(31 + i, 41 + i))
        zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=51 + i)
        cases.append((ppg, em, dm, zs))
    refs = [run(taco, wg, den, *c, False, monkeypatch)[0] for c in cases]
    stream_obj = None
    for i in (0, 1, 2, 0):
        out, t_out, seen = run(taco, wg, den, *cases[i], True, monkeypatch)
        assert seen["streamed"] and t_out == steps
        cs = wg.__dict__["_facppg_cond_stream"]
        assert stream_obj is None or cs is stream_obj            # the same object, the same buffers
        stream_obj = cs
        assert np.array_equal(out, refs[i]), i
