"""The latency shape of k_gemm (launches of at most 256 columns: 32-column tiles, every activation chunk of a split requested
before the K loop) against the 64-column kernel it stands in for (FACPPG_GEMM_SHAPE=legacy).  Every output element is the
same MFMA sequence, so everything downstream is equal BIT FOR BIT: the acoustic model's outputs, a ragged batch, the streamed
utterance's samples (column windows, src_hi, the skip flag) and the denoiser (1026 rows: a partial last row block)."""
import numpy as np
import pytest
import torch

from facppg import synth
from helpers import masks_from_seed, tacotron_case
from stream_helpers import HOP, acoustic, make_vocoder, run, utterance

pytestmark = pytest.mark.gpu


def build(hp, sd):
    from script.train_ppg2mel import load_model
    m = load_model(hp)
    m.load_state_dict(sd, strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def stop_model():
    d, hp, sd, ppg, em, dm = tacotron_case("stop")
    return d, hp, build(hp, sd)


@pytest.fixture(scope="module")
def vocoder():
    return make_vocoder()


def both_shapes(monkeypatch, fn):
    """-> (fn() under the default shape, fn() under FACPPG_GEMM_SHAPE=legacy)."""
    monkeypatch.delenv("FACPPG_GEMM_SHAPE", raising=False)
    new = fn()
    monkeypatch.setenv("FACPPG_GEMM_SHAPE", "legacy")
    return new, fn()


def inference_outputs(m, x, lens, masks):
    mel, mel_post, gate, align = m.inference(x.cuda(), lengths=lens, dropout_masks=masks)
    return [t.clone() for t in (m.last_memory, mel, mel_post, gate, align)]


@pytest.mark.parametrize("Tin", [1, 31, 33, 65])
def test_inference_equals_legacy_shape(stop_model, Tin, monkeypatch):
    """One column, a partial 32-column tile, one column past a tile edge, one past the old shape's 64-column tile."""
    d, hp, m = stop_model
    ns, ms = int(d["n_symbols"]), int(d["max_steps"])
    x = torch.from_numpy(synth.synthetic_ppg(Tin, ns, seed=80 + Tin, alpha=0.002 if ns > 100 else 0.1)).t().unsqueeze(0).contiguous()
    masks = (masks_from_seed(41, (2, 1, Tin, hp.symbols_embedding_dim)), masks_from_seed(42, (ms, 2, 1, hp.prenet_dim)))
    new, old = both_shapes(monkeypatch, lambda: inference_outputs(m, x, None, masks))
    assert new[0].shape == (1, Tin, hp.encoder_embedding_dim) and new[1].shape[2] >= 1
    for name, a, b in zip(("memory", "mel", "mel_post", "gate", "align"), new, old):
        assert torch.count_nonzero(a) > 0, name
        assert torch.equal(a, b), name


def test_ragged_batch_equals_legacy_shape(stop_model, monkeypatch):
    """Per-utterance column counts (n_valid): the batch of test_bilstm_shapes_agree."""
    d, hp, m = stop_model
    ns, ms = int(d["n_symbols"]), int(d["max_steps"])
    lens = [24, 9, 17]
    x = torch.zeros(len(lens), ns, max(lens))
    for b, n in enumerate(lens):
        x[b, :, :n] = torch.from_numpy(synth.synthetic_ppg(n, ns, seed=40 + b)).t()
    g = np.random.Generator(np.random.PCG64(5))
    emb = (g.random((2, len(lens), max(lens), hp.symbols_embedding_dim)) < 0.5).astype(np.uint8)
    dmb = (g.random((ms, 2, len(lens), hp.prenet_dim)) < 0.5).astype(np.uint8)
    new, old = both_shapes(monkeypatch, lambda: inference_outputs(m, x, lens, (emb, dmb)))
    for name, a, b in zip(("memory", "mel", "mel_post", "gate", "align"), new, old):
        assert torch.count_nonzero(a) > 0, name
        assert torch.equal(a, b), name
    for b, n in enumerate(lens):
        assert torch.count_nonzero(new[0][b, n:]) == 0


def test_streamed_utterance_equals_legacy_shape(vocoder, monkeypatch):
    """75 frames through the streamed batch-1 path: facppg_taco_postnet_range extends every postnet layer by column windows
    (col0 > 0, src_hi, the skip flag of blocks that are not final yet)."""
    cfg, wg, den = vocoder
    Tin = steps = 75
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=23)

    def once():
        out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
        assert seen["streamed"] and t_out == steps
        return out, seen["mel_post"]
    (new, new_post), (old, old_post) = both_shapes(monkeypatch, once)
    assert new.shape == (steps * HOP,) and np.count_nonzero(new) > 0
    assert torch.equal(new_post, old_post)
    assert np.array_equal(new, old)


def test_denoiser_equals_legacy_shape(vocoder, monkeypatch):
    """20 frames through the denoiser: its STFT products have M = 1026 rows = 32 row blocks and 2 rows."""
    cfg, wg, den = vocoder
    g = np.random.Generator(np.random.PCG64(9))
    x = torch.from_numpy(g.standard_normal((1, 19 * HOP), dtype=np.float32) * 0.2).cuda()
    new, old = both_shapes(monkeypatch, lambda: den(x, strength=0.1).clone())
    assert new.shape[-1] == 19 * HOP and torch.count_nonzero(new) > 0
    assert torch.equal(new, old)
