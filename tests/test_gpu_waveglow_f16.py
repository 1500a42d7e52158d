"""GPU: half-precision WaveGlow.infer (the reference's HalfTensor branch, glow.py:261-290, via inference.py --is_fp16) on
the fp16 MFMA kernels (facppg_wg_create_f16 / facppg_wg_infer_f16): accuracy against the reference's own half branch,
ragged batches, determinism, switching a module between precisions, Denoiser / pipeline with a half vocoder, refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, rms
from facppg import lib as flib
from facppg import synth

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3


def _model(hop, half=False, n_flows=12):
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=n_flows)
    m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    sd = synth.waveglow_state_dict(cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    if half:
        _halve(m)
    return m, cfg, sd


def _halve(m):
    m.half()
    for k in m.convinv:     # the reference's recipe (inference.py:40-43): convinv stays in float
        k.float()
    return m


def _ref_half(sd, cfg, mel, sigma, zs):
    """The reference's half branch restated on the CPU: half weights, mel and noise; W_inverse formed in fp32 from the
    float convinv weight and then .half() (glow.py:88-95)."""
    from oracle import waveglow as owg
    sdh = {k: v.half() for k, v in sd.items()}
    hop = cfg["hop_length"]
    T = mel.size(2)
    ksz = sd["upsample.weight"].size(2)
    sp = owg.upsample_regroup(sdh, cfg, mel.half(), (T - 1) * hop + ksz - (ksz - hop))
    zs = [z.half() for z in zs]
    audio = sigma * zs.pop(0)
    for k in reversed(range(cfg["n_flows"])):
        n_half = audio.size(1) // 2
        a0, a1 = audio[:, :n_half], audio[:, n_half:]
        out = owg.wn_forward(sdh, k, cfg, a0, sp)
        s, b = out[:, n_half:], out[:, :n_half]
        a1 = (a1 - b) / torch.exp(s)
        audio = torch.cat([a0, a1], 1)
        winv = sd["convinv.%d.conv.weight" % k].squeeze(-1).float().inverse().half()
        audio = F.conv1d(audio, winv[..., None])
        if k % cfg["n_early_every"] == 0 and k > 0:
            audio = torch.cat((sigma * zs.pop(0), audio), 1)
    return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def _relerr(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return rms(x - ref) / rms(ref)


@pytest.mark.parametrize("hop", [256, 160])
def test_half_infer_at_least_as_accurate_as_reference_half_branch(hop):
    from oracle import waveglow as owg
    m, cfg, sd = _model(hop, half=True)
    lengths, sigma = [24, 17], 0.6
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=31)
    zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=32)
    out = m.infer(mel.half().cuda(), sigma=sigma, z=[z.half() for z in zs], lengths=lengths)
    assert out.shape == (B, T * hop) and out.dtype == torch.float16
    out = out.float().cpu()
    a32, aref, ahip = [], [], []
    with torch.no_grad():
        for b, Tb in enumerate(lengths):
            Lb = Tb * hop // 8
            zb = [z[b:b + 1, :, :Lb] for z in zs]
            a32.append(owg.infer(sd, cfg, mel[b:b + 1, :, :Tb], sigma, zb)[0])
            aref.append(_ref_half(sd, cfg, mel[b:b + 1, :, :Tb], sigma, zb)[0].float())
            ahip.append(out[b, :Tb * hop])
            assert torch.all(out[b, Tb * hop:] == 0)
    a32, aref, ahip = (torch.cat(v).numpy() for v in (a32, aref, ahip))
    e_ref, e_hip = _relerr(aref, a32), _relerr(ahip, a32)
    print("hop %d: err(aref16) %.3e  err(ahip16) %.3e" % (hop, e_ref, e_hip))
    assert np.isfinite(ahip).all()
    assert e_hip <= 1.5 * e_ref


def test_half_ragged_batch_equals_single_runs():
    m, cfg, _ = _model(160, half=True)
    lengths = [24, 5, 17, 1]
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=41).half().cuda()
    zs = synth.synthetic_z(B, T * 20, cfg, seed=42)
    seeds = [11, 22, 33, 44]
    got_z = m.infer(mel, sigma=0.6, z=zs, lengths=lengths)
    got_s = m.infer(mel, sigma=0.6, utterance_seeds=seeds, lengths=lengths)
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    assert torch.equal(m.infer(mel, sigma=0.6, utterance_seeds=seeds, lengths=lt), got_s)   # device-side lengths
    for b, Tb in enumerate(lengths):
        Lb = Tb * 20
        one_z = m.infer(mel[b:b + 1, :, :Tb].contiguous(), sigma=0.6, z=[z[b:b + 1, :, :Lb] for z in zs])
        one_s = m.infer(mel[b:b + 1, :, :Tb].contiguous(), sigma=0.6, utterance_seeds=[seeds[b]])
        assert torch.equal(got_z[b, :Tb * 160], one_z[0]), b
        assert torch.equal(got_s[b, :Tb * 160], one_s[0]), b
        assert torch.all(got_z[b, Tb * 160:] == 0) and torch.all(got_s[b, Tb * 160:] == 0)


def test_half_deterministic_and_seed_free_at_sigma_zero():
    m, cfg, _ = _model(256, half=True)
    mel = synth.synthetic_mel(2, 40, seed=51).half().cuda()
    a = m.infer(mel, sigma=0.6, seed=1234)
    b = m.infer(mel, sigma=0.6, seed=1234)
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    assert not torch.equal(a, m.infer(mel, sigma=0.6, seed=4321))
    assert torch.equal(m.infer(mel, sigma=0.0, seed=1), m.infer(mel, sigma=0.0, seed=2))


def test_switching_precision_back_and_forth():
    m, cfg, sd = _model(256)
    d = golden("waveglow_hop256.npz")
    B, T = int(d["B"]), int(d["T"])
    mel = synth.synthetic_mel(B, T, seed=int(d["mel_seed"])).cuda()
    zs = synth.synthetic_z(B, T * 256 // 8, cfg, seed=int(d["z_seed"]))
    sigma = float(d["sigma"])
    never_halved, _, _ = _model(256)
    fresh = never_halved.infer(mel, sigma=sigma, z=zs)
    _halve(m)
    h16 = m.infer(mel.half(), sigma=sigma, z=zs)
    assert h16.dtype == torch.float16 and h16.shape == (B, T * 256)
    m.float()
    m.load_state_dict(sd)      # .half() rounded the weights: reload them
    back = m.infer(mel, sigma=sigma, z=zs)
    assert back.dtype == torch.float32
    assert torch.equal(back, fresh)
    assert rms(back.cpu().numpy() - d["audio"]) <= RMS_TOL
    assert _relerr(h16.float().cpu().numpy(), d["audio"]) < 2e-2


def test_denoiser_and_pipeline_with_half_vocoder():
    from common.hparams import create_hparams_stage
    from facppg import pipeline
    from script.train_ppg2mel import load_model
    from waveglow.denoiser import Denoiser
    m32, cfg, _ = _model(160)
    m16, _, _ = _model(160, half=True)
    d32, d16 = Denoiser(m32, mode="zeros"), Denoiser(m16, mode="zeros")
    e = _relerr(d16.bias_spec.cpu().numpy(), d32.bias_spec.cpu().numpy())
    print("denoiser bias_spec rel rms", e)
    assert e <= 1e-2
    steps = 40
    hp = create_hparams_stage(max_decoder_steps=steps)
    taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    taco.eval()
    lens = [40, 29]
    ppgs = [synth.synthetic_ppg(n, 5816, seed=500 + i, alpha=0.002) for i, n in enumerate(lens)]
    seeds = [71, 72]
    w32, t32 = pipeline.synthesize(ppgs, taco, m32, None, sigma=0.6, utterance_seeds=seeds, step_limits=lens)
    w16, t16 = pipeline.synthesize(ppgs, taco, m16, None, sigma=0.6, utterance_seeds=seeds, step_limits=lens)
    w32b, _ = pipeline.synthesize(ppgs, taco, m32, None, sigma=0.6, utterance_seeds=seeds, step_limits=lens)
    assert t16 == t32 and [len(w) for w in w16] == [len(w) for w in w32]
    for a, b, c in zip(w32, w16, w32b):
        assert b.dtype == np.float32 and np.array_equal(a, c)
        eb = _relerr(b, a)
        print("pipeline rel rms", eb)
        assert eb <= 1e-2


def test_refusals():
    m, cfg, _ = _model(160, half=True)
    mel = synth.synthetic_mel(1, 8, seed=61).cuda()
    with pytest.raises(flib.FacppgError, match="must be fp16"):
        m.infer(mel)                                    # half module, fp32 mel
    with pytest.raises(flib.FacppgError, match="groups"):
        m.infer(torch.cat([mel, mel]).half(), lengths=[8, 6], groups=2)
    m32, _, _ = _model(160)
    with pytest.raises(flib.FacppgError, match="fp32 only"):
        m32.infer(mel.half())
    bf, _, _ = _model(160)
    bf.to(torch.bfloat16)
    with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
        bf.infer(mel.to(torch.bfloat16))
    mixed, _, _ = _model(160, half=True)
    mixed.WN[3].in_layers[2].float()
    with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
        mixed.infer(mel.half())
    # raw ABI: each kind of handle into the other kind's entry point
    L = flib.load()
    dev = torch.device("cuda", 0)
    h16, h32 = m._handle(dev), m32._handle(dev)
    B, T = 1, 8
    ws = torch.empty(max(L.facppg_wg_workspace_bytes(h16, B, T), L.facppg_wg_workspace_bytes(h32, B, T)), dtype=torch.uint8,
                     device=dev)
    a32 = torch.empty(B, T * 160, device=dev)
    a16 = torch.empty(B, T * 160, dtype=torch.float16, device=dev)
    mel16 = mel.half()
    null = ctypes.c_void_p(0)
    st = flib.current_stream(dev)
    rc = L.facppg_wg_infer(h16, flib.ptr(mel), null, null, 1, 0.6, B, T, flib.ptr(a32), flib.ptr(ws), ws.numel(), st)
    assert rc == -1 and b"fp16" in L.facppg_last_error()
    rc = L.facppg_wg_infer_f16(h32, flib.ptr(mel16), null, null, 1, 0.6, B, T, flib.ptr(a16), flib.ptr(ws), ws.numel(), st)
    assert rc == -1 and b"fp32" in L.facppg_last_error()
    torch.cuda.synchronize()


@pytest.mark.skipif(os.environ.get("FACPPG_PERF_TESTS") != "1", reason="performance check: FACPPG_PERF_TESTS=1")
def test_half_throughput_at_least_twice_fp32():
    m32, cfg, _ = _model(256)
    m16, _, _ = _model(256, half=True)
    B, T = 8, 1000
    mel = synth.synthetic_mel(B, T, seed=71).cuda()
    mel16 = mel.half()

    def best(f):
        f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        return min(ts)
    t32 = best(lambda: m32.infer(mel, sigma=0.6, seed=1))
    t16 = best(lambda: m16.infer(mel16, sigma=0.6, seed=1))
    print("B=8 x 1000 hop 256: fp32 %.2f ms, fp16 %.2f ms (%.2fx)" % (t32, t16, t32 / t16))
    assert t32 >= 2.0 * t16
