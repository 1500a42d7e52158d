"""facppg_taco_launch_plan against the launches themselves: for a handle's own co-residency bound (facppg_taco_coop_limit) the
query names the mode, the workgroups and the worker stages that facppg_taco_decode / facppg_taco_decode_forced then report in
their opts.  Seeded synthetic weights at the reference's layer widths (the split shape needs them), tiny batches."""
import ctypes

import pytest
import torch

from facppg import lib as flib
from facppg import synth
from stream_helpers import acoustic

pytestmark = pytest.mark.gpu

NS = 5816
DECODE, FORCED = 1, 2
_model = []


def model():
    if not _model:
        _model.append(acoustic(4, -10.0))
    return _model[0]


def query(taco, what, B, Tin, steps, wgs):
    dev = torch.device("cuda", torch.cuda.current_device())
    L = flib.load()
    limit = L.facppg_taco_coop_limit(taco._handle(dev))
    assert limit > 0
    r = flib.TacoLaunchReport()
    flib.check(L.facppg_taco_launch_plan(taco._config(), limit, what, B, Tin, steps, wgs, r))
    return r


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("lens,steps,wgs,mode", [([3], 4, 0, 2), ([5, 3, 4], 4, 80, 2), ([3] * 10, 2, 0, 1)])
def test_decode_launches_what_the_query_says(lens, steps, wgs, mode, legacy, monkeypatch):
    hp, taco = model()
    monkeypatch.setattr(taco.decoder, "max_decoder_steps", steps)
    if legacy:
        monkeypatch.setenv("FACPPG_DECODER_STEP", "legacy")
    else:
        monkeypatch.delenv("FACPPG_DECODER_STEP", raising=False)
    B, Tin = len(lens), max(lens)
    r = query(taco, DECODE, B, Tin, steps, wgs)
    x = torch.zeros(B, NS, Tin)
    for b, n in enumerate(lens):
        x[b, :, :n] = torch.from_numpy(synth.synthetic_ppg(n, NS, seed=300 + b, alpha=0.002)).t()
    out = taco.inference(x.cuda(), lengths=lens, seed=77, decoder_workgroups=wgs)
    launch = out.launch                                     # mode, workgroups and step of the call's opts
    print("query", r.mode, r.workgroups, r.step, "launch", launch)
    assert r.mode == mode                                   # the case is the shape it is meant to be
    assert (("single", "coop", "split")[r.mode], r.workgroups, r.step) == (launch.mode, launch.workgroups, launch.step)
    assert out[0].shape == (B, hp.n_acoustic_feat_dims, steps) and bool(torch.isfinite(out[0]).all())


@pytest.mark.parametrize("B", [2, 3])
def test_forced_launches_what_the_query_says(B):
    hp, taco = model()
    Tin = T = 3
    r = query(taco, FORCED, B, Tin, T, 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    L, h = flib.load(), taco._handle(dev)
    g = torch.Generator().manual_seed(11)
    # the recurrence runs T frames whatever the values: any finite memory / processed memory / targets do
    mem = torch.randn(B, Tin, hp.encoder_embedding_dim, generator=g).to(dev)
    pm = torch.randn(B, hp.attention_dim, Tin, generator=g).to(dev)
    tgt = torch.randn(B, hp.n_acoustic_feat_dims, T, generator=g).to(dev)
    lens = torch.full((B,), Tin, dtype=torch.int32, device=dev)
    mel = torch.empty(B, hp.n_acoustic_feat_dims, T, device=dev)
    gate, align = torch.empty(B, T, device=dev), torch.empty(B, T, Tin, device=dev)
    ws = torch.empty(L.facppg_taco_decode_forced_workspace_bytes(h, B, T), dtype=torch.uint8, device=dev)
    opts = flib.TacoDecodeOpts()
    flib.check(L.facppg_taco_decode_forced(h, flib.ptr(mem), flib.ptr(pm), flib.ptr(lens), flib.ptr(tgt), None, 5, B, Tin, T,
                                           flib.ptr(mel), flib.ptr(gate), flib.ptr(align), flib.ptr(ws), ws.numel(),
                                           ctypes.byref(opts), flib.current_stream(dev)))
    torch.cuda.synchronize()
    print("query", r.mode, r.workgroups, r.step, r.regw, "opts", opts.mode, opts.workgroups, opts.step)
    assert r.regw == (1 if B == 2 else 0)
    assert (r.mode, r.workgroups, r.step) == (opts.mode, opts.workgroups, opts.step)
    assert bool(torch.isfinite(mel).all())
