"""GPU: WaveGlow.infer(arithmetic="bf16x3") (glow.py:252-293) on split-bf16 operands (facppg_wg_split_*): accuracy against the
emulated arithmetic, the project's tolerance on the reference's outputs, ragged batches, every tile width, determinism,
weights following the module, the pipeline, refusals.

Every fp32 operand x of a WaveNet contraction is hi + lo with hi = RNE_bf16(x), lo = RNE_bf16(x - hi); a product is
A_hi.B_hi + A_hi.B_lo + A_lo.B_hi in fp32.  The emulation replaces the CPU oracle's conv1d by that product with exact (float64)
accumulation for every convolution with >= 16 input channels."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, rms
from facppg import lib as flib
from facppg import synth

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3          # the tolerance the fp32 path is held to (tests/test_gpu_waveglow.py)
ARITH = "bf16x3"


def _model(hop, n_flows=12, seed=16807):
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=n_flows)
    m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    sd = synth.waveglow_state_dict(cfg, seed=seed)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), cfg, sd


def _relerr(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return rms(x - ref) / rms(ref)


def _split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


class _SplitF(object):
    """torch.nn.functional with conv1d replaced by the split product: three partial convolutions in float64, summed, cast to fp32,
    bias added in fp32; convolutions with fewer than 16 input channels stay fp32."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def conv1d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if x.shape[1] < 16:
            return F.conv1d(x, w, bias, stride, padding, dilation, groups)
        (xh, xl), (wh, wl) = _split(x.float()), _split(w.float())

        def conv(a, c):
            return F.conv1d(a.double(), c.double(), None, stride, padding, dilation, groups)
        y = (conv(xh, wh) + conv(xh, wl) + conv(xl, wh)).float()
        return y if bias is None else y + bias.view(1, -1, 1)


@functools.lru_cache(maxsize=None)
def _references(hop):
    """(a32, aemu, e_emu) of the accuracy case, per utterance on the CPU and concatenated: the oracle, and the oracle with its
    conv1d replaced by the split product (the oracle module's F is patched for the call and restored)."""
    from oracle import waveglow as owg
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=12)
    sd = synth.waveglow_state_dict(cfg)
    lengths, sigma = [24, 17], 0.6
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=31)
    zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=32)
    a32, aemu = [], []
    with torch.no_grad():
        for b, Tb in enumerate(lengths):
            Lb = Tb * hop // 8
            zb = [z[b:b + 1, :, :Lb] for z in zs]
            a32.append(owg.infer(sd, cfg, mel[b:b + 1, :, :Tb], sigma, zb)[0])
            real = owg.F
            owg.F = _SplitF()
            try:
                aemu.append(owg.infer(sd, cfg, mel[b:b + 1, :, :Tb], sigma, zb)[0])
            finally:
                owg.F = real
    a32, aemu = torch.cat(a32).numpy(), torch.cat(aemu).numpy()
    return a32, aemu, _relerr(aemu, a32)


@pytest.mark.parametrize("hop", [256, 160])
def test_accuracy_against_the_emulated_split_arithmetic(hop):
    """Requirement: e_hip <= 3 * e_emu (relative RMS against the fp32 oracle), finite, zeros past each utterance's end."""
    m, cfg, sd = _model(hop)
    lengths, sigma = [24, 17], 0.6
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=31)
    zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=32)
    out = m.infer(mel.cuda(), sigma=sigma, z=zs, lengths=lengths, arithmetic=ARITH)
    assert out.shape == (B, T * hop) and out.dtype == torch.float32
    out = out.cpu()
    a32, aemu, e_emu = _references(hop)
    ahip = []
    for b, Tb in enumerate(lengths):
        ahip.append(out[b, :Tb * hop])
        assert torch.all(out[b, Tb * hop:] == 0)
    ahip = torch.cat(ahip).numpy()
    e_hip = _relerr(ahip, a32)
    print("hop %d: e_emu %.3e  e_hip %.3e  (hip against the emulation %.3e)" % (hop, e_emu, e_hip, _relerr(ahip, aemu)))
    assert np.isfinite(ahip).all()
    assert e_hip <= 3.0 * e_emu


@pytest.mark.parametrize("hop", [256, 160])
def test_project_tolerance_and_untouched_fp32_path(hop):
    d = golden("waveglow_hop%d.npz" % hop)
    B, T = int(d["B"]), int(d["T"])
    m, cfg, _ = _model(hop)
    mel = synth.synthetic_mel(B, T, seed=int(d["mel_seed"])).cuda()
    zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=int(d["z_seed"]))
    sigma = float(d["sigma"])
    untouched, _, _ = _model(hop)
    fresh = untouched.infer(mel, sigma=sigma, z=zs)
    before = m.infer(mel, sigma=sigma, z=zs)
    split = m.infer(mel, sigma=sigma, z=zs, arithmetic=ARITH)
    after = m.infer(mel, sigma=sigma, z=zs, arithmetic="fp32")
    assert "_facppg_handle" in m.__dict__ and "_facppg_split_handle" in m.__dict__      # both handles at once
    assert torch.equal(before, fresh) and torch.equal(after, fresh)
    assert split.dtype == torch.float32 and split.shape == fresh.shape
    assert not torch.equal(split, fresh)                                                # the new kernels ran
    e = rms(split.cpu().numpy() - d["audio"])
    print("hop %d: rms against the golden audio: bf16x3 %.3e, fp32 %.3e" % (hop, e, rms(fresh.cpu().numpy() - d["audio"])))
    assert e <= RMS_TOL


def test_ragged_batch_equals_single_runs():
    m, cfg, _ = _model(160)
    lengths = [24, 5, 17, 1]
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=41).cuda()
    zs = synth.synthetic_z(B, T * 20, cfg, seed=42)
    seeds = [11, 22, 33, 44]
    got_z = m.infer(mel, sigma=0.6, z=zs, lengths=lengths, arithmetic=ARITH)
    got_s = m.infer(mel, sigma=0.6, utterance_seeds=seeds, lengths=lengths, arithmetic=ARITH)
    lt = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    assert torch.equal(m.infer(mel, sigma=0.6, utterance_seeds=seeds, lengths=lt, arithmetic=ARITH), got_s)   # device-side lengths
    assert torch.equal(m.infer(mel, sigma=0.6, z=zs, lengths=lt, arithmetic=ARITH), got_z)
    for b, Tb in enumerate(lengths):
        Lb = Tb * 20
        one = mel[b:b + 1, :, :Tb].contiguous()
        one_z = m.infer(one, sigma=0.6, z=[z[b:b + 1, :, :Lb] for z in zs], arithmetic=ARITH)
        one_s = m.infer(one, sigma=0.6, utterance_seeds=[seeds[b]], arithmetic=ARITH)
        assert torch.equal(got_z[b, :Tb * 160], one_z[0]), b
        assert torch.equal(got_s[b, :Tb * 160], one_s[0]), b
        assert torch.all(got_z[b, Tb * 160:] == 0) and torch.all(got_s[b, Tb * 160:] == 0)


def test_every_tile_width_runs_and_agrees(monkeypatch):
    m, cfg, _ = _model(256)
    T = 70                      # a full 64-frame tile plus a remainder, taps crossing the tile edge
    mel = synth.synthetic_mel(1, T, seed=45).cuda()
    zs = synth.synthetic_z(1, T * 32, cfg, seed=46)
    outs = {}
    for tw in (32, 64):
        monkeypatch.setenv("FACPPG_WG_SPLIT_TILE", str(tw))
        outs[tw] = m.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)
        assert m.last_launch_shape(ARITH) == (tw, 8, 32 * -(-T // tw))
    assert torch.equal(outs[32], outs[64])
    assert torch.isfinite(outs[32]).all()
    monkeypatch.delenv("FACPPG_WG_SPLIT_TILE")
    free = m.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)
    tile, waves, tiles = m.last_launch_shape(ARITH)
    assert tile in (32, 64) and waves == 8 and tiles == 32 * -(-T // tile)
    assert torch.equal(free, outs[32])
    monkeypatch.setenv("FACPPG_WG_SPLIT_TILE", "128")      # no 128-frame tile: 104 KiB of LDS at 64 frames already
    with pytest.raises(flib.FacppgError, match="FACPPG_WG_SPLIT_TILE"):
        m.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)


def test_deterministic_and_seed_free_at_sigma_zero():
    m, cfg, _ = _model(256)
    mel = synth.synthetic_mel(2, 40, seed=51).cuda()
    a = m.infer(mel, sigma=0.6, seed=1234, arithmetic=ARITH)
    b = m.infer(mel, sigma=0.6, seed=1234, arithmetic=ARITH)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(a, m.infer(mel, sigma=0.6, seed=4321, arithmetic=ARITH))
    assert torch.equal(m.infer(mel, sigma=0.0, seed=1, arithmetic=ARITH), m.infer(mel, sigma=0.0, seed=2, arithmetic=ARITH))


def test_weights_follow_the_module():
    m, cfg, sd = _model(160)
    mel = synth.synthetic_mel(2, 20, seed=55).cuda()
    zs = synth.synthetic_z(2, 20 * 20, cfg, seed=56)
    first = m.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)
    other = synth.waveglow_state_dict(cfg, seed=4242)
    m.load_state_dict(other)
    assert "_facppg_split_handle" not in m.__dict__
    second = m.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)
    fresh, _, _ = _model(160, seed=4242)
    assert torch.equal(second, fresh.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH))
    assert not torch.equal(second, first)


def _acoustic(steps):
    from common.hparams import create_hparams_stage
    from script.train_ppg2mel import load_model
    hp = create_hparams_stage(max_decoder_steps=steps)
    taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    taco.eval()
    return taco


def _spy(taco, seen):
    inference = taco.inference

    def spy(*a, **kw):
        out = inference(*a, **kw)
        consumer = kw.get("frame_consumer")
        seen.append((consumer is not None and consumer.active, bool(out.launch.streamed), out[1].detach().clone()))
        return out
    taco.inference = spy


def test_pipeline_passes_the_arithmetic_through_and_never_streams(monkeypatch):
    from facppg import pipeline
    m, cfg, _ = _model(160)
    taco = _acoustic(40)
    lens = [40, 29]
    ppgs = [synth.synthetic_ppg(n, 5816, seed=500 + i, alpha=0.002) for i, n in enumerate(lens)]
    seeds = [71, 72]
    w32, t32 = pipeline.synthesize(ppgs, taco, m, None, sigma=0.6, utterance_seeds=seeds, step_limits=lens)
    wsp, tsp = pipeline.synthesize(ppgs, taco, m, None, sigma=0.6, utterance_seeds=seeds, step_limits=lens, vocoder_arithmetic=ARITH)
    assert tsp == t32 and [len(w) for w in wsp] == [len(w) for w in w32]
    e_emu = _references(160)[2]
    for a, b in zip(w32, wsp):
        assert b.dtype == np.float32 and not np.array_equal(a, b)
        e = _relerr(b, a)
        print("pipeline rel rms %.3e (3 e_emu = %.3e)" % (e, 3 * e_emu))
        assert e <= 3.0 * e_emu
    with pytest.raises(flib.FacppgError, match="vocoder_arithmetic"):
        pipeline.synthesize(ppgs, taco, m, None, vocoder_arithmetic="fp8")
    # one utterance of 70 frames: a length the fp32 path streams (given the chance) -- the bf16x3 call must not
    monkeypatch.setenv("FACPPG_STREAM", "1")
    monkeypatch.setenv("FACPPG_STREAM_MIN_FRAMES", "64")
    m256, cfg256, _ = _model(256)
    taco70 = _acoustic(70)
    ppg = synth.synthetic_ppg(70, 5816, seed=510, alpha=0.002)
    zs = synth.synthetic_z(1, 70 * 32, cfg256, seed=57)
    seen = []
    _spy(taco70, seen)
    try:
        wavs, tout = pipeline.synthesize([ppg], taco70, m256, None, sigma=0.6, seed=5, z=zs, vocoder_arithmetic=ARITH)
    finally:
        del taco70.inference
    assert tout == [70] and len(seen) == 1
    consumer_active, published, mel_post = seen[0]
    assert not consumer_active and not published          # last_streamed: the call did not stream
    assert "_facppg_cond_stream" not in m256.__dict__
    direct = m256.infer(mel_post.contiguous(), sigma=0.6, z=zs, arithmetic=ARITH)
    assert np.array_equal(wavs[0], direct[0].cpu().numpy())


def test_refusals():
    m, cfg, _ = _model(160)
    mel = synth.synthetic_mel(2, 8, seed=61).cuda()
    with pytest.raises(flib.FacppgError, match="arithmetic"):
        m.infer(mel, arithmetic="bf16")
    with pytest.raises(flib.FacppgError, match="groups"):
        m.infer(mel, lengths=[8, 6], groups=2, arithmetic=ARITH)
    with pytest.raises(flib.FacppgError, match="groups"):
        m.infer(mel, groups=1, arithmetic=ARITH)
    with pytest.raises(flib.FacppgError, match="cond_first"):
        m.infer(mel, cond_first=True, arithmetic=ARITH)
    with pytest.raises(flib.FacppgError, match="fp32 mel"):
        m.infer(mel.half(), arithmetic=ARITH)
    half, _, _ = _model(160)
    half.half()
    for k in half.convinv:
        k.float()
    with pytest.raises(flib.FacppgError, match="all-fp32 module"):
        half.infer(mel.half(), arithmetic=ARITH)
    with pytest.raises(flib.FacppgError, match="all-fp32 module"):
        half.infer(mel, arithmetic=ARITH)
    # raw ABI
    L = flib.load()
    dev = torch.device("cuda", 0)
    hs = m._split_handle(dev)
    B, T = 1, 8
    one = mel[:1].contiguous()
    need = L.facppg_wg_split_workspace_bytes(hs, B, T)
    assert need > 0 and L.facppg_wg_split_workspace_bytes(None, B, T) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    audio = torch.empty(B, T * 160, device=dev)
    null = ctypes.c_void_p(0)
    st = flib.current_stream(dev)
    args = lambda h, mp, ap, wp, n: (h, mp, null, null, 1, 0.6, B, T, ap, wp, n, st)     # noqa: E731
    assert L.facppg_wg_split_infer(*args(null, flib.ptr(one), flib.ptr(audio), flib.ptr(ws), ws.numel())) == -1
    assert L.facppg_wg_split_infer(*args(hs, null, flib.ptr(audio), flib.ptr(ws), ws.numel())) == -1
    assert L.facppg_wg_split_infer(*args(hs, flib.ptr(one), null, flib.ptr(ws), ws.numel())) == -1
    assert L.facppg_wg_split_infer(*args(hs, flib.ptr(one), flib.ptr(audio), null, ws.numel())) == -1
    assert b"NULL" in L.facppg_last_error()
    rc = L.facppg_wg_split_infer(*args(hs, flib.ptr(one), flib.ptr(audio), flib.ptr(ws), need - 1))
    assert rc == -4 and b"workspace" in L.facppg_last_error()
    i0 = ctypes.c_int(0)
    assert L.facppg_wg_split_last_launch_shape(null, ctypes.byref(i0), ctypes.byref(i0), ctypes.byref(i0)) == -1
    blob = m._flat_weights().to(dev).contiguous()
    out = ctypes.c_void_p()
    assert L.facppg_wg_split_create(m._config(), flib.ptr(blob), blob.numel(), 0, st, None) == -1
    bad = m._config()
    bad.wn_channels = 128
    rc = L.facppg_wg_split_create(bad, flib.ptr(blob), blob.numel(), 0, st, ctypes.byref(out))
    assert rc == -2 and not out.value and b"n_channels=256" in L.facppg_last_error()
    L.facppg_wg_split_destroy(null)
    assert L.facppg_wg_split_infer(*args(hs, flib.ptr(one), flib.ptr(audio), flib.ptr(ws), ws.numel())) == 0   # and the handle still works
    torch.cuda.synchronize()
    assert torch.isfinite(audio).all()


@pytest.mark.skipif(os.environ.get("FACPPG_PERF_TESTS") != "1", reason="performance check: FACPPG_PERF_TESTS=1")
def test_split_infer_faster_than_fp32():
    m, cfg, _ = _model(256)

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
    for B, T in ((8, 1000), (1, 200)):
        mel = synth.synthetic_mel(B, T, seed=71).cuda()
        t32 = best(lambda: m.infer(mel, sigma=0.6, seed=1))
        tsp = best(lambda: m.infer(mel, sigma=0.6, seed=1, arithmetic=ARITH))
        print("B=%d x %d hop 256: fp32 %.2f ms, bf16x3 %.2f ms (%.2fx)" % (B, T, t32, tsp, t32 / tsp))
        assert tsp < t32
