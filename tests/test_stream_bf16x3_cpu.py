"""CPU: what the split-bf16 streamed path (pipeline.synthesize(vocoder_arithmetic="bf16x3", vocoder_stream=True)) decides on the
host: the keyword's values, the arithmetic names of WaveGlow's seeded methods, the tail rule of the new kind, the binding."""
import ctypes

import numpy as np
import pytest
import torch

from facppg import lib as flib
from facppg import pipeline
from facppg.pipeline import ConditioningStream


def test_vocoder_stream_is_checked_before_any_model_is_touched():
    ppgs = [np.zeros((4, 8), np.float32)]
    for bad in ("yes", False, 1, "bf16x3"):
        with pytest.raises(flib.FacppgError, match="vocoder_stream"):
            pipeline.synthesize(ppgs, object(), object(), vocoder_stream=bad)
        with pytest.raises(flib.FacppgError, match="vocoder_stream"):
            pipeline.synthesize(ppgs, object(), object(), vocoder_arithmetic="bf16x3", vocoder_stream=bad)
    with pytest.raises(flib.FacppgError, match="vocoder_arithmetic"):      # (the older check still comes first)
        pipeline.synthesize(ppgs, object(), object(), vocoder_arithmetic="fp8", vocoder_stream=True)
    # None and True pass the check: the call then fails on the placeholder models, not on the keyword
    for ok in (None, True):
        with pytest.raises(AttributeError):
            pipeline.synthesize(ppgs, object(), object(), vocoder_stream=ok)


def test_seeded_methods_refuse_an_unknown_arithmetic_without_a_device():
    from facppg import synth
    from waveglow.glow import WaveGlow
    m = WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=1))
    mel = torch.zeros(1, 80, 4)
    melp = torch.zeros(8, 80)
    seeds = torch.zeros(4)
    for call in (lambda: m.seed_layout(4, torch.device("cpu"), arithmetic="bf16"),
                 lambda: m.mel_pad(mel, arithmetic="bf16"),
                 lambda: m.mel_convert(mel[0], 4, 0, 4, melp, arithmetic="bf16"),
                 lambda: m.cond_seed(melp, 4, 0, 4, seeds, arithmetic="bf16"),
                 lambda: m.infer_seeded(melp, 4, seeds, 0, arithmetic="bf16")):
        with pytest.raises(flib.FacppgError, match="arithmetic='bf16'"):
            call()
    assert "_facppg_handle" not in m.__dict__ and "_facppg_split_handle" not in m.__dict__
    # the split path's buffer and input kinds are named before a device is needed, too
    with pytest.raises(flib.FacppgError, match="fp32 mel buffer"):
        m.cond_seed(melp.half(), 4, 0, 4, seeds, arithmetic="bf16x3")
    with pytest.raises(flib.FacppgError, match="fp32 mel"):
        m.mel_pad(mel.half(), arithmetic="bf16x3")


def test_tail_pass_of_the_split_kind():
    kind = ConditioningStream.SPLIT
    assert kind == "bf16x3"
    # nothing left behind the blocks
    assert ConditioningStream.tail_pass(kind, 200, 224, 32, 256) is None
    assert ConditioningStream.tail_pass(kind, 64, 64, 32, 256) is None
    # one more bounded pass over whole tiles, from a tile's first frame, whatever the length
    for T, seeded in ((200, 160), (75, 32), (96, 0), (1000, 960), (33, 32)):
        frame0, nframes, block_tiles, lpw, bounded = ConditioningStream.tail_pass(kind, T, seeded, 32, 256)
        assert frame0 == seeded and frame0 % 32 == 0 and nframes % 32 == 0 and frame0 + nframes == -(-T // 32) * 32
        assert 1 <= block_tiles <= nframes // 32 and lpw == 1 and bounded
        assert ConditioningStream.tail_pass(kind, T, seeded, 32, 256, tail="seed") == (frame0, nframes, block_tiles, lpw, bounded)
        assert ConditioningStream.tail_pass(kind, T, seeded, 32, 256, tail="mixed") is None
    # the other kinds keep their rules
    assert ConditioningStream.tail_pass(torch.float16, 200, 160, 32, 256) == ConditioningStream.tail_pass(kind, 200, 160, 32, 256)
    assert ConditioningStream.tail_pass(torch.float32, 200, 160, 32, 256) is None
    assert ConditioningStream.MIN_FRAMES_SPLIT >= 32 and set(ConditioningStream.MIN_FRAMES) == {torch.float32, torch.float16}


def test_binding_declares_the_seeded_split_entry_points():
    names = flib.exported_symbols()
    for n in ("facppg_wg_split_seed_layout", "facppg_wg_split_mel_pad", "facppg_wg_split_cond_seed", "facppg_wg_split_infer_seeded"):
        assert n in names
    L = flib.load()
    null = ctypes.c_void_p(0)
    i, sz = ctypes.c_int(), ctypes.c_size_t()
    assert L.facppg_wg_split_seed_layout(null, 4, ctypes.byref(i), ctypes.byref(i), ctypes.byref(sz), ctypes.byref(i)) == -1
    assert b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_split_mel_pad(null, null, 4, 4, 0, 4, null, null, null) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_split_cond_seed(null, null, 4, 0, 4, 1, 1, 0, 0, null, 0, null, 0, null, null) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_split_infer_seeded(null, null, 4, 4, null, 0, null, 0, 1.0, null, null, 0, null, null) == -1
    assert b"NULL" in L.facppg_last_error()
    assert L.facppg_version() == 103
