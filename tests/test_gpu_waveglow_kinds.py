"""GPU: what a WaveGlow inference call costs in packed-weight validity checks, for each of the three vocoder kinds (fp32, fp16,
bf16x3).  A check (WeightIdentity.unchanged) walks ~1000 tensors, 0.2 - 0.4 ms of host time between the two models of the batch-1
path, so the number per call is part of the contract: a steady-state infer() validates its handle ONCE, none at all after
prepare() (whose token the call consumes), and the seeded methods validate nothing when they are handed the handle.  The counts
are read off the code paths (one _handle / _split_handle per infer(); draw_noise, which a ragged batch with host-side lengths and
no z goes through, validates the fp32 / fp16 handle it draws with once more), not measured.  4 flows at hop 160, the WN stack
of the standard config (8 layers x 256 channels); one utterance of 40 frames and a ragged batch of three."""
import pytest
import torch

from facppg import lib as flib
from facppg import synth
from stream_helpers import halve

pytestmark = pytest.mark.gpu

HOP, T, LENGTHS = 160, 40, [40, 33, 17]
CFG = dict(synth.WAVEGLOW_CONFIG, hop_length=HOP, n_flows=4)
KINDS = {"fp32": (False, None), "fp16": (True, None), "bf16x3": (False, "bf16x3")}
_MODELS = {}


def model(half):
    from waveglow.glow import WaveGlow
    if half not in _MODELS:
        m = WaveGlow.remove_weightnorm(WaveGlow(**CFG))
        m.load_state_dict(synth.waveglow_state_dict(CFG))
        m = m.cuda().eval()
        _MODELS[half] = halve(m) if half else m
    return _MODELS[half]


@pytest.fixture
def walks(monkeypatch):
    """[number of WeightIdentity.unchanged calls so far]"""
    n = [0]
    unchanged = flib.WeightIdentity.unchanged

    def counted(self):
        n[0] += 1
        return unchanged(self)
    monkeypatch.setattr(flib.WeightIdentity, "unchanged", counted)
    return n


def counted(walks, fn):
    walks[0] = 0
    out = fn()
    return out, walks[0]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_validity_walks_per_call(kind, walks):
    half, arith = KINDS[kind]
    m = model(half)
    dev = torch.device("cuda", 0)
    kw = {} if arith is None else {"arithmetic": arith}
    dtype = torch.float16 if half else torch.float32
    mel1 = synth.synthetic_mel(1, T, seed=91).cuda().to(dtype)
    mel3 = synth.synthetic_mel(3, T, seed=93).cuda().to(dtype)
    z1 = synth.synthetic_z(1, T * HOP // 8, CFG, seed=92)
    z3 = synth.synthetic_z(3, T * HOP // 8, CFG, seed=94)
    first = m.infer(mel1, sigma=0.6, seed=7, **kw)              # builds the handle(s): not steady state yet
    m.infer(mel3, sigma=0.6, seed=7, lengths=LENGTHS, **kw)     # (and, through draw_noise, the fp32 one next to the split one)
    # a steady-state plain infer(): exactly one
    again, n = counted(walks, lambda: m.infer(mel1, sigma=0.6, seed=7, **kw))
    assert n == 1 and again.dtype == dtype and again.shape == (1, T * HOP) and torch.equal(again, first)
    ragged, n = counted(walks, lambda: m.infer(mel3, sigma=0.6, z=z3, lengths=LENGTHS, **kw))
    assert n == 1 and ragged.shape == (3, T * HOP)
    for b, Tb in enumerate(LENGTHS):
        assert not ragged[b, Tb * HOP:].any() and torch.isfinite(ragged[b].float()).all()
    # seed alone on a ragged batch with host-side lengths: per-utterance streams, drawn on the fp32 / fp16 handle (one more check)
    _, n = counted(walks, lambda: m.infer(mel3, sigma=0.6, seed=7, lengths=LENGTHS, **kw))
    assert n == 2
    # after prepare(): none, and the token is gone
    _, n = counted(walks, lambda: m.prepare(dev, arith))
    assert n == 1 and "_facppg_prepared" in m.__dict__
    prepared, n = counted(walks, lambda: m.infer(mel1, sigma=0.6, seed=7, **kw))
    assert n == 0 and "_facppg_prepared" not in m.__dict__ and torch.equal(prepared, first)
    _, n = counted(walks, lambda: m.infer(mel1, sigma=0.6, seed=7, **kw))
    assert n == 1                                               # single use
    m.prepare(dev, arith)
    _, n = counted(walks, lambda: m.infer(mel3, sigma=0.6, z=z3, lengths=LENGTHS, **kw))
    assert n == 0 and "_facppg_prepared" not in m.__dict__
    # the seeded methods with the handle passed in: none
    h = m._split_handle(dev) if arith else m._handle(dev)
    seeds = torch.empty(m.seed_layout(T, dev, **kw)[2], dtype=torch.uint8, device=dev)

    def seeded():
        melp = m.mel_pad(mel1.float(), handle=h, **kw)
        m.cond_seed(melp, T, 0, 64, seeds, handle=h, **kw)
        return m.infer_seeded(melp, T, seeds, 64, sigma=0.6, z=z1, handle=h, **kw)
    out, n = counted(walks, seeded)
    assert n == 0 and out.dtype == dtype and out.shape == (1, T * HOP) and torch.isfinite(out.float()).all()
    if kind == "fp32":                                          # (conditioning-first already: the seeded samples are infer()'s)
        assert torch.equal(out, m.infer(mel1, sigma=0.6, z=z1))
    torch.cuda.synchronize()
