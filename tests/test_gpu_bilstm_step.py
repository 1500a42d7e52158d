"""The one-barrier step of k_bilstm_coop (K parts and gates of a unit meet inside a wave, hv double buffered) against the
three-barrier step it replaced (FACPPG_BILSTM_STEP=legacy): every sum keeps its order, so the encoder memory is equal BIT FOR
BIT, for both slice widths (FACPPG_BILSTM_MODE coop = 32 units per workgroup, wide = 64)."""
import numpy as np
import pytest
import torch

from helpers import masks_from_seed, tacotron_case

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


def memory_of(m, x, lens, masks, monkeypatch, mode, step):
    monkeypatch.setenv("FACPPG_BILSTM_MODE", mode)
    if step:
        monkeypatch.setenv("FACPPG_BILSTM_STEP", step)
    else:
        monkeypatch.delenv("FACPPG_BILSTM_STEP", raising=False)
    m.inference(x.cuda(), lengths=lens, dropout_masks=masks)
    return m.last_memory.clone()


@pytest.mark.parametrize("mode", ["coop", "wide"])
@pytest.mark.parametrize("Tin", [1, 2, 3])
def test_first_steps_equal_legacy(stop_model, Tin, mode, monkeypatch):
    """B = 1 at Tin = 1, 2, 3: the first step (h = 0, nothing gathered) and both parities of the exchange / hv buffers."""
    from facppg import synth
    d, hp, m = stop_model
    ns, ms = int(d["n_symbols"]), int(d["max_steps"])
    x = torch.from_numpy(synth.synthetic_ppg(Tin, ns, seed=70 + Tin, alpha=0.002 if ns > 100 else 0.1)).t().unsqueeze(0).contiguous()
    masks = (masks_from_seed(31, (2, 1, Tin, hp.symbols_embedding_dim)), masks_from_seed(32, (ms, 2, 1, hp.prenet_dim)))
    new = memory_of(m, x, None, masks, monkeypatch, mode, None)
    old = memory_of(m, x, None, masks, monkeypatch, mode, "legacy")
    assert new.shape == (1, Tin, hp.encoder_embedding_dim)
    assert torch.count_nonzero(new) > 0
    assert torch.equal(new, old)


@pytest.mark.parametrize("mode", ["coop", "wide"])
def test_ragged_batch_equals_legacy(stop_model, mode, monkeypatch):
    """The ragged batch of test_bilstm_shapes_agree: per-utterance lengths, the backward direction starting at len - 1, and
    H = 300 = 9 * 32 + 12: the last workgroup of a direction holds 12 live units of 32 (44 of 64 in the wide shape)."""
    from facppg import synth
    d, hp, m = stop_model
    ns, ms = int(d["n_symbols"]), int(d["max_steps"])
    lens = [24, 9, 17]
    x = torch.zeros(len(lens), ns, max(lens))
    for b, n in enumerate(lens):
        x[b, :, :n] = torch.from_numpy(synth.synthetic_ppg(n, ns, seed=40 + b)).t()
    g = np.random.Generator(np.random.PCG64(5))
    emb = (g.random((2, len(lens), max(lens), hp.symbols_embedding_dim)) < 0.5).astype(np.uint8)
    dmb = (g.random((ms, 2, len(lens), hp.prenet_dim)) < 0.5).astype(np.uint8)
    new = memory_of(m, x, lens, (emb, dmb), monkeypatch, mode, None)
    old = memory_of(m, x, lens, (emb, dmb), monkeypatch, mode, "legacy")
    assert torch.equal(new, old)
    for b, n in enumerate(lens):
        assert torch.count_nonzero(new[b, :n]) > 0
        assert torch.count_nonzero(new[b, n:]) == 0


@pytest.mark.parametrize("mode", ["coop", "wide"])
def test_small_hidden_size_equals_legacy(mode, monkeypatch):
    """H = 36 at Tin = 5: a second workgroup with 4 live units of 32 (coop), one workgroup with 36 of 64 (wide), and a dot
    product of 9 (18) live columns = 3 (5) groups of 4 with a partly padded last group.  The encoder alone, through the C ABI
    (the decoder's shapes are not what this is about)."""
    from common.hparams import create_hparams_stage
    from facppg import lib as flib
    from facppg import synth
    ns, Tin, E = 40, 5, 72
    hp = create_hparams_stage(n_symbols=ns, symbols_embedding_dim=E, encoder_embedding_dim=E, max_decoder_steps=4)
    m = build(hp, synth.tacotron_state_dict(hp, seed=16807))
    L = flib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(synth.synthetic_ppg(Tin, ns, seed=77, alpha=0.1)).t().unsqueeze(0).contiguous().to(dev)
    enc_m = torch.from_numpy(masks_from_seed(33, (2, 1, Tin, E))).to(dev).to(torch.uint8).permute(0, 1, 3, 2).contiguous()
    h = m._handle(dev)
    ws = torch.empty(L.facppg_taco_workspace_bytes(h, 1, Tin), dtype=torch.uint8, device=dev)
    st = flib.current_stream(dev)
    monkeypatch.setenv("FACPPG_BILSTM_MODE", mode)
    mems = []
    for step in (None, "legacy"):
        if step:
            monkeypatch.setenv("FACPPG_BILSTM_STEP", step)
        else:
            monkeypatch.delenv("FACPPG_BILSTM_STEP", raising=False)
        memory = torch.zeros(1, Tin, E, device=dev)
        pm = torch.zeros(1, Tin, hp.attention_dim, device=dev)
        flib.check(L.facppg_taco_encode(h, flib.ptr(x), None, flib.ptr(enc_m), 0, 1, Tin, flib.ptr(memory), flib.ptr(pm),
                                        flib.ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        mems.append(memory.cpu())
    assert torch.count_nonzero(mems[0]) > 0
    assert torch.equal(mems[0], mems[1])
