"""CPU: the argument normaliser WaveGlow.infer and WaveGlow.infer_seeded share (WaveGlow._infer_args): what it refuses and what
it hands on, for both precisions, on CPU tensors (every check comes before anything moves to a device)."""
import pytest
import torch

from facppg import lib as flib
from facppg import synth

B, T = 3, 5


@pytest.fixture(scope="module")
def model():
    from waveglow.glow import WaveGlow
    return WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=1))


def n_values(m, b=B, t=T):
    return b * m.n_group * (t * m.upsample.stride[0] // m.n_group)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_refusals(model, dtype):
    args = lambda **kw: model._infer_args(B, T, dtype, kw.get("z"), kw.get("lengths"), kw.get("seed"), kw.get("utterance_seeds"))
    for lengths in ([5, 4], [5, 4, 3, 2], [5, 6, 1], [5, 0, 1], torch.tensor([5, 4]), torch.tensor([5, 6, 1]), torch.tensor([5, 0, 1])):
        with pytest.raises(flib.FacppgError, match="lengths must be B values"):
            args(lengths=lengths)
    n = n_values(model)
    with pytest.raises(flib.FacppgError, match="not together with z"):
        args(z=torch.zeros(n), utterance_seeds=[1, 2, 3])
    for seeds in ([1, 2], [1, 2, 3, 4]):
        with pytest.raises(flib.FacppgError, match="utterance_seeds: B integers"):
            args(utterance_seeds=seeds)
    for z in (torch.zeros(n - 1), torch.zeros(B, n // B + 1), [torch.zeros(n // 2), torch.zeros(n // 2 - 1)], [torch.zeros(n), torch.zeros(1)]):
        with pytest.raises(flib.FacppgError, match="z has %d values, expected B\\*n_group\\*L = %d" % (sum(t.numel() for t in (z if isinstance(z, list) else [z])), n)):
            args(z=z)
    with pytest.raises(flib.FacppgError, match="z has"):
        model._infer_args(1, T, dtype, torch.zeros(n), None, None, None)        # (infer_seeded: B = 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_what_it_hands_on(model, dtype):
    n = n_values(model)
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn(B, 2, n // B // 8, generator=g, dtype=torch.float64), torch.randn(B, 6, n // B // 8, generator=g)]
    flat = torch.cat([p.to(dtype).reshape(-1) for p in parts])
    for z in (parts, tuple(parts), flat.double().view(B, -1), flat.view(-1)[:, None].expand(n, 2)[:, 0]):
        zt, lengths, seed, us = model._infer_args(B, T, dtype, z, [5, 3, 1], 7, None)
        assert zt.dtype == dtype and zt.dim() == 1 and zt.is_contiguous() and torch.equal(zt, flat)
        assert lengths == [5, 3, 1] and seed == 7 and us is None           # (injected z: no derived streams)
    zt, lengths, seed, us = model._infer_args(B, T, dtype, None, torch.tensor([5, 3, 1]), None, [11, 12, 13])
    assert zt is None and lengths.dtype == torch.int32 and lengths.tolist() == [5, 3, 1] and us == [11, 12, 13]
    assert isinstance(seed, int)                                            # (drawn from torch's generator)
    assert model._infer_args(B, T, dtype, None, None, 7, None) == (None, None, 7, None)
    assert model._infer_args(1, T, dtype, None, [5], 7, None) == (None, [5], 7, None)          # one utterance: nothing to derive
    assert model._infer_args(B, T, dtype, None, torch.tensor([5, 3, 1]), 7, None)[3] is None     # lengths on the device: no host plan


def test_derived_utterance_seeds_are_the_same_for_both_precisions(model):
    """`seed` alone on a ragged batch with host-side lengths: utterance b draws from (seed * 0x9E3779B97F4A7C15 + (b + 1) *
    0xBF58476D1CE4E5B9) mod 2^63, whatever the precision."""
    seed = 0x123456789ABCDEF
    want = [(seed * 0x9E3779B97F4A7C15 + (b + 1) * 0xBF58476D1CE4E5B9) & 0x7FFFFFFFFFFFFFFF for b in range(B)]
    assert want == [0x4BEBEF24B7D28E54, 0x0B443691D4B7740D, 0x4A9C7DFEF19C59C6]
    got = [model._infer_args(B, T, dt, None, [5, 3, 1], seed, None) for dt in (torch.float32, torch.float16)]
    assert got[0] == got[1] == (None, [5, 3, 1], seed, want)
