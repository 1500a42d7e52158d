"""CPU: what the half-precision streamed path (facppg.pipeline.ConditioningStream with a .half() vocoder) decides on the host:
which vocoders it accepts, and the argument validation of its entry points that needs no device."""
import ctypes
import types

import pytest
import torch

from facppg import lib as flib
from facppg.pipeline import ConditioningStream


def _namespace(dtype, wn_dtype=None):
    conv = lambda dt: types.SimpleNamespace(weight=torch.empty(1, dtype=dt), parameters=lambda: [torch.empty(1, dtype=dt)])
    wn = types.SimpleNamespace(n_layers=8, parameters=lambda: [torch.empty(1, dtype=wn_dtype or dtype)])
    return types.SimpleNamespace(WN=[wn], n_group=8, upsample=conv(dtype))


def test_usable_accepts_all_fp16_and_refuses_bf16_and_mixed(monkeypatch):
    for var in ("FACPPG_STREAM", "FACPPG_WG_UNFOLDED", "FACPPG_WG_EDGE_FOLD"):
        monkeypatch.delenv(var, raising=False)
    taco = types.SimpleNamespace(decoder_workgroups=0)
    assert ConditioningStream.usable(taco, _namespace(torch.float32))
    assert ConditioningStream.usable(taco, _namespace(torch.float16))
    assert ConditioningStream.precision(_namespace(torch.float16)) == torch.float16
    assert not ConditioningStream.usable(taco, _namespace(torch.bfloat16))
    assert not ConditioningStream.usable(taco, _namespace(torch.float16, wn_dtype=torch.float32))
    # a namespace without an upsampler (tests/test_stream_plan_cpu.py) stays usable
    assert ConditioningStream.usable(taco, types.SimpleNamespace(WN=[types.SimpleNamespace(n_layers=8)], n_group=8))
    # the existing switches hold for a half vocoder too
    half = _namespace(torch.float16)
    monkeypatch.setenv("FACPPG_STREAM", "0")
    assert not ConditioningStream.usable(taco, half)
    monkeypatch.delenv("FACPPG_STREAM")
    monkeypatch.setenv("FACPPG_WG_EDGE_FOLD", "0")
    assert not ConditioningStream.usable(taco, half)
    monkeypatch.delenv("FACPPG_WG_EDGE_FOLD")
    monkeypatch.setenv("FACPPG_WG_UNFOLDED", "1")
    assert not ConditioningStream.usable(taco, half)
    monkeypatch.delenv("FACPPG_WG_UNFOLDED")
    taco.decoder_workgroups = 32
    assert not ConditioningStream.usable(taco, half)


def test_usable_on_real_modules():
    from facppg import synth
    from waveglow.glow import WaveGlow
    taco = types.SimpleNamespace(decoder_workgroups=0)
    m = WaveGlow.remove_weightnorm(WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=2)))
    assert ConditioningStream.precision(m) == torch.float32
    m.half()
    for k in m.convinv:          # the reference's recipe: convinv kept in float
        k.float()
    assert ConditioningStream.precision(m) == torch.float16 and ConditioningStream.usable(taco, m)
    m.WN[1].end.float()
    assert ConditioningStream.precision(m) is None and not ConditioningStream.usable(taco, m)
    m.to(torch.bfloat16)
    assert not ConditioningStream.usable(taco, m)


def test_a_minimum_length_exists_for_both_precisions():
    assert set(ConditioningStream.MIN_FRAMES) == {torch.float32, torch.float16}
    assert ConditioningStream.MIN_FRAMES[torch.float32] == 128          # (measured for the fp32 path; unchanged)
    assert ConditioningStream.MIN_FRAMES[torch.float16] == 64           # (the half sweep: streamed wins from its shortest length on)


def test_new_entry_points_validate_without_device():
    L = flib.load()
    null = ctypes.c_void_p(0)
    i, sz = ctypes.c_int(), ctypes.c_size_t()
    assert L.facppg_wg_seed_layout_f16(null, 4, ctypes.byref(i), ctypes.byref(i), ctypes.byref(sz)) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_mel_pad_f16(null, null, 4, 4, 0, 4, null, null, null) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_cond_seed_f16(null, null, 4, 0, 4, 1, 1, 0, 0, null, 0, null, 0, null, null) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_infer_seeded_f16(null, null, 4, 4, null, 0, null, 0, 1.0, null, null, 0, null, null) == -1
    assert b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_infer_f16_order(null, null, null, null, 0, 1.0, 1, 4, 1, null, null, 0, null) == -1 and b"NULL" in L.facppg_last_error()


def test_cond_first_is_refused_without_a_gpu_as_any_infer_is():
    from facppg import synth
    from waveglow.glow import WaveGlow
    m = WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=1))
    with pytest.raises(flib.FacppgError, match="no CPU path"):
        m.infer(torch.zeros(1, 80, 4), cond_first=True)
