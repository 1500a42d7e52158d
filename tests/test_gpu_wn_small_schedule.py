"""GPU: the small-launch schedule of the 8-wave 32-frame WaveNet layer tiles (second-GEMM operands requested ahead of the
gate, write-through epilogue stores) against the schedule before it (FACPPG_WN_SMALL=legacy).  The schedule changes when
operands are requested and how stores leave the CU, never an operand, an MFMA or the order of a sum: every case compares
the two with np.array_equal, asserts through facppg_wg_last_layer_schedule that each schedule ran and through
last_launch_shape() the tile kind, and anchors the default to the CPU oracle with the tolerance of test_gpu_waveglow.py.
All cases use the standard 12-flow config."""
import numpy as np
import pytest
import torch

from helpers import rms
from test_gpu_waveglow import RMS_TOL, make_model
from facppg import synth

pytestmark = pytest.mark.gpu

SIGMA = 0.6
_MODELS = {}


def model(hop):
    if hop not in _MODELS:
        _MODELS[hop] = make_model(hop)
    return _MODELS[hop]


def inputs(cfg, T, hop, seed):
    mel = synth.synthetic_mel(1, T, seed=seed)
    zs = synth.synthetic_z(1, T * hop // 8, cfg, seed=seed + 1)
    return mel, zs


def oracle(cfg, mel, zs):
    from oracle import waveglow as owg
    with torch.no_grad():
        return owg.infer(synth.waveglow_state_dict(cfg), cfg, mel, SIGMA, zs).numpy()


def both(monkeypatch, m, fn):
    """fn() under the default schedule and under FACPPG_WN_SMALL=legacy: (outputs, launch shapes), each schedule asserted."""
    outs, shapes = [], []
    for env, name in ((None, "small"), ("legacy", "legacy")):
        if env is None:
            monkeypatch.delenv("FACPPG_WN_SMALL", raising=False)
        else:
            monkeypatch.setenv("FACPPG_WN_SMALL", env)
        outs.append(fn())
        assert m.last_layer_schedule() == name
        shapes.append(m.last_launch_shape())
    monkeypatch.delenv("FACPPG_WN_SMALL")
    return outs, shapes


def check(tag, cfg, mel, zs, outs, shapes, shape, hop):
    small, legacy = outs
    assert shapes[0] == shapes[1] == shape
    assert small.shape == (1, mel.shape[2] * hop) and np.array_equal(small, legacy)
    e = rms(small - oracle(cfg, mel, zs))
    print("%s: small schedule vs oracle rms err %.3e" % (tag, e))
    assert e <= RMS_TOL


def seeded_run(m, mel, zs, T, seeded):
    melp = m.mel_pad(mel.cuda())
    _, _, nbytes = m.seed_layout(T, melp.device)
    seeds = torch.empty(nbytes, dtype=torch.uint8, device=melp.device)
    m.cond_seed(melp, T, 0, seeded, seeds)
    return lambda: m.infer_seeded(melp, T, seeds, seeded, sigma=SIGMA, z=zs).cpu().numpy()


def test_unseeded_tiles_with_a_ragged_last_tile(monkeypatch):
    """Unstreamed T = 131 = 4 x 32 + 3 at hop 256, per-layer kernels: 8-wave 32-frame unseeded tiles, the last one with
    3 live frames -- less than one lane group, so its rows leave through the 4-byte tail stores."""
    hop, T = 256, 131
    m, cfg = model(hop)
    monkeypatch.setenv("FACPPG_WG_PERSIST", "0")
    mel, zs = inputs(cfg, T, hop, seed=500 + T)
    outs, shapes = both(monkeypatch, m, lambda: m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy())
    check("unseeded T %d" % T, cfg, mel, zs, outs, shapes, (32, 8, 32 * 5), hop)


def test_mixed_launch_seeded_tiles_next_to_unseeded_ones(monkeypatch):
    """infer_seeded at T = 150 with 128 frames seeded: four seeded 32-frame tiles and two unseeded 16-frame tiles per phase
    (k_wn_layer_mixed): both kinds of tile store write-through, the seeded ones request ahead of the gate."""
    hop, T, seeded = 256, 150, 128
    m, cfg = model(hop)
    mel, zs = inputs(cfg, T, hop, seed=177)
    outs, shapes = both(monkeypatch, m, seeded_run(m, mel, zs, T, seeded))
    check("mixed T %d" % T, cfg, mel, zs, outs, shapes, (32, 8, 32 * (seeded // 32 + 2)), hop)


def test_every_frame_seeded(monkeypatch):
    """infer_seeded at T = 64 with all 64 frames seeded: no unseeded tail, the single-kind launch k_wn_layer8<..., SEED>."""
    hop, T = 256, 64
    m, cfg = model(hop)
    mel, zs = inputs(cfg, T, hop, seed=264)
    outs, shapes = both(monkeypatch, m, seeded_run(m, mel, zs, T, T))
    check("all seeded T %d" % T, cfg, mel, zs, outs, shapes, (32, 8, 32 * 2), hop)


def test_hop_160_forced_32_frame_tiles(monkeypatch):
    """hop 160: 20 phases (no XCD map), another conditioning chunk count; T = 40 with FACPPG_WN_TILE=32 (two tiles per
    phase, the second with 8 live frames)."""
    hop, T = 160, 40
    m, cfg = model(hop)
    monkeypatch.setenv("FACPPG_WN_TILE", "32")
    mel, zs = inputs(cfg, T, hop, seed=340)
    outs, shapes = both(monkeypatch, m, lambda: m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy())
    check("hop 160 T %d" % T, cfg, mel, zs, outs, shapes, (32, 8, 20 * 2), hop)


def test_consecutive_calls_on_one_handle_are_equal(monkeypatch):
    """Two calls on one handle and workspace, mixed launch: an operand requested before its producer was done, or a
    write-through row that reached memory behind a later plain one, shows up as a difference between the calls."""
    hop, T, seeded = 256, 150, 128
    m, cfg = model(hop)
    mel, zs = inputs(cfg, T, hop, seed=177)
    run = seeded_run(m, mel, zs, T, seeded)
    outs, shapes = both(monkeypatch, m, lambda: (run(), run()))
    assert shapes[0] == shapes[1] == (32, 8, 32 * (seeded // 32 + 2))
    (a0, a1), (b0, b1) = outs
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1) and np.array_equal(a0, b0)
    e = rms(a0 - oracle(cfg, mel, zs))
    print("consecutive calls: small schedule vs oracle rms err %.3e" % e)
    assert e <= RMS_TOL
