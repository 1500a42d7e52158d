"""CPU: argument validation of the half-precision WaveGlow entry points (facppg_wg_create_f16 / facppg_wg_infer_f16)
that needs no device, and the module-level precision rules of WaveGlow (which parameters decide the path)."""
import ctypes

import pytest
import torch

from facppg import lib as flib


def test_f16_entry_points_validate_without_device():
    L = flib.load()
    null = ctypes.c_void_p(0)
    rc = L.facppg_wg_infer_f16(null, null, null, null, 0, 1.0, 1, 4, null, null, 0, null)
    assert rc == -1 and b"NULL" in L.facppg_last_error()
    out = ctypes.c_void_p()
    assert L.facppg_wg_create_f16(None, null, 0, 0, null, ctypes.byref(out)) == -1
    cfg = flib.WgConfig(80, 160, 12, 8, 4, 2, 8, 256, 3, 1024)
    assert L.facppg_wg_create_f16(ctypes.byref(cfg), null, 0, 0, null, None) == -1
    assert L.facppg_wg_create_f16(ctypes.byref(cfg), null, 5, 0, null, ctypes.byref(out)) == -1
    assert L.facppg_wg_workspace_bytes(null, 1, 4) == 0


def _module():
    from facppg import synth
    from waveglow.glow import WaveGlow
    m = WaveGlow.remove_weightnorm(WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=4)))
    return m


def test_module_precision_rules():
    m = _module()
    assert m._precision() == torch.float32
    m.half()
    assert m._precision() == torch.float16
    for k in m.convinv:          # the reference's recipe: convinv kept in float
        k.float()
    assert m._precision() == torch.float16
    m.WN[1].end.float()           # any other mix is refused
    with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
        m._precision()
    m.float()
    assert m._precision() == torch.float32
    m.to(torch.bfloat16)
    with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
        m._precision()
