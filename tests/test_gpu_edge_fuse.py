"""GPU: the inner flow edges run inside the LAST WaveNet layer's tiles on the small-launch path (one short utterance:
16-frame tiles, 8-wave 32-frame tiles, seeded and mixed launches) instead of a k_flow_end launch each.  The fused tiles run
the same operations in the same order, so every case compares the default against FACPPG_WG_EDGE_FUSE=0 (the separate
launches) bit for bit, checks the tile kind that ran, and anchors the fused result to the CPU oracle with the tolerance of
test_gpu_waveglow.py.  All cases use the standard 12-flow config (early-z flows, n_half 2, 3 and 4)."""
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


def oracle(cfg, mel, zs, alternate=False):
    from oracle import waveglow as owg
    with torch.no_grad():
        return owg.infer(synth.waveglow_state_dict(cfg), cfg, mel, SIGMA, zs, alternate=alternate).numpy()


def both(monkeypatch, fn):
    """fn() with the fused edges (default) and with the separate edge launches."""
    monkeypatch.delenv("FACPPG_WG_EDGE_FUSE", raising=False)
    fused = fn()
    monkeypatch.setenv("FACPPG_WG_EDGE_FUSE", "0")
    split = fn()
    monkeypatch.delenv("FACPPG_WG_EDGE_FUSE")
    return fused, split


@pytest.mark.parametrize("hop,T,tile", [(256, 21, 16), (256, 50, 16), (256, 131, 32), (160, 40, 16)])
def test_unstreamed_infer_fused_edges_equal_the_separate_launches(hop, T, tile, monkeypatch):
    """16-frame tiles at T = 21 and 50 (ragged last tile, a lane group with fewer than 4 live frames), 8-wave 32-frame
    unseeded tiles at T = 131 = 4 x 32 + 3 (the per-layer kernels: the persistent launch is switched off for both runs),
    and hop 160 (20 phases: no XCD map)."""
    m, cfg = model(hop)
    if T == 131:
        monkeypatch.setenv("FACPPG_WG_PERSIST", "0")
    mel, zs = inputs(cfg, T, hop, seed=300 + T)
    shapes = []

    def run():
        out = m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy()
        shapes.append(m.last_launch_shape())
        return out
    fused, split = both(monkeypatch, run)
    P = hop // 8
    assert shapes[0] == shapes[1] == (tile, 8, P * -(-T // tile))
    assert fused.shape == (1, T * hop) and np.array_equal(fused, split)
    e = rms(fused - oracle(cfg, mel, zs))
    print("hop %d T %d: fused vs oracle rms err %.3e" % (hop, T, e))
    assert e <= RMS_TOL


def test_seeded_and_mixed_tiles_fused_edges_equal_the_separate_launches(monkeypatch):
    """facppg_wg_infer_seeded with the first 128 of 150 frames seeded by k_cond_seed: four seeded 32-frame tiles and two
    unseeded 16-frame tiles (the second with 6 live frames) per phase in every launch (k_wn_layer_mixed)."""
    hop, T, seeded = 256, 150, 128
    m, cfg = model(hop)
    mel, zs = inputs(cfg, T, hop, seed=77)
    melp = m.mel_pad(mel.cuda())
    dev = melp.device
    _, _, nbytes = m.seed_layout(T, dev)
    seeds = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    m.cond_seed(melp, T, 0, seeded, seeds)
    shapes = []

    def run():
        out = m.infer_seeded(melp, T, seeds, seeded, sigma=SIGMA, z=zs).cpu().numpy()
        shapes.append(m.last_launch_shape())
        return out
    fused, split = both(monkeypatch, run)
    assert shapes[0] == shapes[1] == (32, 8, 32 * (seeded // 32 + 2))
    assert fused.shape == (1, T * hop) and np.array_equal(fused, split)
    e = rms(fused - oracle(cfg, mel, zs))
    print("seeded + mixed T %d: fused vs oracle rms err %.3e" % (T, e))
    assert e <= RMS_TOL


def test_legacy_layout_fused_edges_equal_the_separate_launches(monkeypatch):
    """waveglow.glow_old (odd flows condition on the second half: swap / swap_next in the edge)."""
    from waveglow import glow_old
    hop, T = 256, 40
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop)
    m = glow_old.WaveGlow(**{k: v for k, v in cfg.items() if k != "hop_length"})
    m = glow_old.WaveGlow.remove_weightnorm(m)
    m.load_state_dict(synth.waveglow_state_dict(cfg), strict=True)
    m = m.cuda().eval()
    mel, zs = inputs(cfg, T, hop, seed=91)
    shapes = []

    def run():
        out = m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy()
        shapes.append(m.last_launch_shape())
        return out
    fused, split = both(monkeypatch, run)
    assert shapes[0] == shapes[1] == (16, 8, 32 * 3)
    assert np.array_equal(fused, split)
    e = rms(fused - oracle(cfg, mel, zs, alternate=True))
    print("glow_old T %d: fused vs oracle rms err %.3e" % (T, e))
    assert e <= RMS_TOL


def test_consecutive_calls_on_one_handle_are_equal(monkeypatch):
    """The fused tiles write the next flow's start-conv rows while neighbouring tiles of the same launch still read h_in
    through their dilated taps: the rows go to the other h buffer.  A stale or overwritten h_in -- or a margin of that
    buffer that did not stay zero -- shows up as a difference between two calls on the same handle and workspace."""
    hop, T = 256, 131
    m, cfg = model(hop)
    monkeypatch.setenv("FACPPG_WG_PERSIST", "0")
    monkeypatch.delenv("FACPPG_WG_EDGE_FUSE", raising=False)
    mel, zs = inputs(cfg, T, hop, seed=300 + T)
    first = m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy()
    assert m.last_launch_shape()[:2] == (32, 8)
    second = m.infer(mel.cuda(), sigma=SIGMA, z=zs).cpu().numpy()
    assert np.array_equal(first, second)
