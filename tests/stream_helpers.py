"""The harness of the streamed batch-1 tests (tests/test_gpu_stream.py, tests/test_gpu_stream_f16.py): the synthetic hop-256
vocoder in either precision, the acoustic model with a chosen step limit and gate bias, one utterance's inputs, one
pipeline.synthesize call with the stream on or off, and the patch that makes the decoder's first frames late."""
import contextlib
import io

import torch

from helpers import masks_from_seed
from facppg import synth

HOP = 256


def halve(m):
    """The reference's recipe (inference.py:40-43): .half(), convinv kept in float."""
    m.half()
    for k in m.convinv:
        k.float()
    return m


def make_vocoder(half=False):
    """-> (config, WaveGlow on the GPU, its Denoiser)."""
    from waveglow.denoiser import Denoiser
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=HOP)
    wg = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    wg.load_state_dict(synth.waveglow_state_dict(cfg))
    wg = wg.cuda().eval()
    if half:
        halve(wg)
    return cfg, wg, Denoiser(wg, hop_length=HOP, mode="zeros")


def acoustic(steps, gate_bias):
    from common.hparams import create_hparams_stage
    from script.train_ppg2mel import load_model
    hp = create_hparams_stage(max_decoder_steps=steps)
    with contextlib.redirect_stdout(io.StringIO()):
        taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=gate_bias))
    taco.eval()
    return hp, taco


def utterance(hp, Tin, steps, seed, mask_seeds=(21, 22)):
    """-> (ppg, encoder dropout masks, decoder dropout masks) of one utterance of Tin PPG frames."""
    ppg = synth.synthetic_ppg(Tin, 5816, seed=seed, alpha=0.002)
    em = masks_from_seed(mask_seeds[0], (2, 1, Tin, hp.symbols_embedding_dim))
    dm = masks_from_seed(mask_seeds[1], (steps, 2, 1, hp.prenet_dim))
    return ppg, em, dm


def run(taco, wg, den, ppg, em, dm, zs, stream, monkeypatch):
    """One pipeline.synthesize call of the utterance, streamed or not -> (samples, Tout, what Tacotron2.inference saw)."""
    from facppg import pipeline
    monkeypatch.setenv("FACPPG_STREAM", "1" if stream else "0")
    monkeypatch.setenv("FACPPG_STREAM_MIN_FRAMES", "64")     # (short utterances are not streamed by default: they do not gain)
    seen = {}
    inference = taco.inference

    def spy(*a, **kw):
        out = inference(*a, **kw)
        seen["mel_post"] = out[1].detach().clone()
        seen["streamed"] = kw.get("frame_consumer") is not None and kw["frame_consumer"].active
        seen["published"] = out.launch.streamed
        return out
    taco.inference = spy
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            wavs, tout = pipeline.synthesize([ppg], taco, wg, den, sigma=0.6, strength=0.005, dropout_masks=(em, dm), z=zs)
    finally:
        del taco.inference
    return wavs[0], tout[0], seen


def late_encode(monkeypatch):
    """The frames must really be late for a block to time out.  The collectors start with the encoder and test the limit only
    every few hundred polls, and the first frame follows about a millisecond later: a fast encoder wins that race and no block
    times out.  A spin kernel behind the encoder, on the stream the decoder is launched on, holds the frames back for
    milliseconds."""
    from facppg import lib as flib
    L = flib.load()
    encode = L.facppg_taco_encode

    def encode_then_spin(*a):
        rc = encode(*a)
        torch.cuda._sleep(20_000_000)
        return rc
    monkeypatch.setattr(L, "facppg_taco_encode", encode_then_spin)
