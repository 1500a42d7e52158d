"""GPU: the bf16 training step's upsampler -- ConvTranspose1d(80, 80, K, stride hop) + crop + 8-sample regroup into the bf16
position-major conditioning operand, and its backward (csrc/facppg_train_bf16.hip: k_up_fold / k_up_pack_mel / k_gemm /
k_up_regroup / k_up_ungroup / k_up_unfold on the GEMM path, k_up_fwd / k_up_wgrad on the scalar path, the bias column sums) --
called directly and held to the float64 reference of tests/upsample_helpers.py, case by case, at both hops, with and without
samples past T hop, under both paths.

Integer operands (every sum an integer bf16 and fp32 hold exactly, test_upsample_reference_cpu.py): equal bits.  Random
operands: one bf16 rounding on top of the fp32 summation bound (upsample_helpers.forward_tolerance), (R + 2) 2u S for the
weight gradient over R = B T frames, (8 B L + 2) u S for the bias gradient.  Every output starts as NaN, the workspace as 0xFF
bytes (production passes torch.empty), every operand and buffer is followed by poison.

Measured on the MI355X: worst err / tol of the random cases 0.985 forward (round to nearest sits just below 1: u = 2^-8 is
bf16's unit roundoff), 0.20 dW, 0.13 db; the whole file takes 13 s: the three module-level steps 5.5 s (float64 oracle
backward on the CPU), the 253 direct cases 7.5 s, most of it start-up and the float64 references.

The conversions facppg_spect_to_bf16 / facppg_posmajor_to_f32 and three whole bf16 training steps (hop 256; samples past T hop
at both hops) against float64 autograd of the oracle follow."""
import numpy as np
import pytest
import torch

import upsample_helpers as uh
from facppg import synth

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda c: c.id)
INT_SHAPES = tuple(c.shape for c in uh.CASES if c.data == "int" and c.path == "gemm")


def _worst(err, tol):
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("c", uh.CASES + uh.NO_WS_CASES, **_ids)
def test_forward_vs_float64_reference(c):
    rc, bits = uh.run_forward(c)
    if not c.forward_supported:
        assert rc == uh.EUNSUPPORTED, (rc, uh.last_error())
        return
    assert rc == uh.OK, (rc, uh.last_error())
    ref = uh.forward_reference(c.shape)
    assert bits.shape == ref.spect.shape
    assert not bits[:, c.L:].any(), "rows [L, Lr) must be zero"
    if c.data == "int":
        want = uh.bf16_bits(ref.spect + 0.0)
        bad = np.argwhere(bits != want)
        assert bad.size == 0, "%d of %d values differ, first at (b, l, 8m+g) = %s: got %g, want %g" % (
            len(bad), bits.size, tuple(bad[0]), uh.bf16_to_f64(bits)[tuple(bad[0])], ref.spect[tuple(bad[0])])
    else:
        out = uh.bf16_to_f64(bits)
        assert np.isfinite(out).all()
        err, tol = np.abs(out - ref.spect), uh.forward_tolerance(c, ref)
        print("%s: forward worst err/tol %.3f" % (c.id, _worst(err, tol)))
        assert (err <= tol).all()


@pytest.mark.parametrize("c", uh.CASES, **_ids)
def test_backward_vs_float64_reference(c):
    rc, dW, db = uh.run_backward(c)
    assert rc == uh.OK, (rc, uh.last_error())
    ref = uh.backward_reference(c.shape)
    assert np.isfinite(dW).all() and np.isfinite(db).all()
    if c.data == "int":
        bad = np.argwhere(dW != ref.dW)
        assert bad.size == 0, "dW: %d of %d values differ, first at (m', m, k) = %s: got %g, want %g" % (
            len(bad), dW.size, tuple(bad[0]), dW[tuple(bad[0])], ref.dW[tuple(bad[0])])
        assert np.array_equal(db, ref.db), (db, ref.db)
        # and bit for bit (no negative zero: every sum starts from +0)
        assert np.array_equal(dW.view(np.uint32), (ref.dW + 0.0).astype(np.float32).view(np.uint32))
        assert np.array_equal(db.view(np.uint32), (ref.db + 0.0).astype(np.float32).view(np.uint32))
    else:
        eW, tW = np.abs(dW - ref.dW), uh.dW_tolerance(c, ref)
        eb, tb = np.abs(db - ref.db), uh.db_tolerance(c, ref)
        print("%s: dW worst err/tol %.4f, db %.4f" % (c.id, _worst(eW, tW), _worst(eb, tb)))
        assert (eW <= tW).all() and (eb <= tb).all()


@pytest.mark.parametrize("shape", INT_SHAPES, **_ids)
def test_gemm_path_and_scalar_path_give_the_same_bits(shape):
    import dataclasses
    g, s = dataclasses.replace(shape, path="gemm"), dataclasses.replace(shape, path="scalar")
    (rg, fg), (rs, fs) = uh.run_forward(g), uh.run_forward(s)
    assert rg == rs
    if shape.forward_supported:
        assert rg == uh.OK and np.array_equal(fg, fs)
    (rg, wg, bg), (rs, ws, bs) = uh.run_backward(g), uh.run_backward(s)
    assert rg == rs == uh.OK
    assert np.array_equal(wg.view(np.uint32), ws.view(np.uint32)) and np.array_equal(bg.view(np.uint32), bs.view(np.uint32))


@pytest.mark.parametrize("path", ["gemm", "scalar", "no_ws"])
def test_mel_shorter_than_the_audio_is_rejected(path):
    import dataclasses
    rc, bits = uh.run_forward(dataclasses.replace(uh.REJECTED, path=path))
    assert rc == uh.EINVAL and bits is None
    assert "shorter than the audio" in uh.last_error()


# ------------------------------------------------------------------------------------------ the layout conversions
CONV_SHAPES = [(ch, L, pad) for ch in (640, 33) for L in (1, 31, 33, 128, 129) for pad in (0, 5)]


def _normal(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32))


@pytest.mark.parametrize("ch,L,pad", CONV_SHAPES)
def test_spect_to_bf16(ch, L, pad):
    """fp32 channel-major [B, ch, ld] (first L columns) -> bf16 position-major [B, Lr, ch], rows [L, Lr) zero; the columns
    [L, ld) of the source are NaN and must never appear."""
    from facppg import lib
    Lh = lib.load()
    B, ld, Lr = 2, L + pad, uh.padded_len(L)
    src = _normal((B, ch, ld), 1000 * ch + 10 * L + pad)
    src[:, :, L:] = float("nan")
    n_out = B * Lr * ch
    out = torch.full((n_out + uh.GUARD // 2,), uh.NAN_BF16, dtype=torch.int16, device="cuda")
    dev = src.cuda()
    rc = Lh.facppg_spect_to_bf16(lib.ptr(dev), B, ch, L, ld, lib.ptr(out), lib.current_stream(dev.device))
    torch.cuda.synchronize()
    assert rc == uh.OK, uh.last_error()
    assert bool((out[n_out:] == uh.NAN_BF16).all()), "wrote behind the output"
    want = torch.zeros(B, Lr, ch, dtype=torch.bfloat16)
    want[:, :L] = src[:, :, :L].transpose(1, 2).bfloat16()
    assert torch.equal(out[:n_out].cpu().view(B, Lr, ch), want.view(torch.int16))


@pytest.mark.parametrize("ch,L,pad", CONV_SHAPES)
def test_posmajor_to_f32(ch, L, pad):
    """fp32 position-major [B, Lr, ch] -> fp32 channel-major [B, ch, ld], first L columns: the rows [L, Lr) of the source (NaN
    here) are not read, the columns [L, ld) of the output keep what they held."""
    from facppg import lib
    Lh = lib.load()
    B, ld, Lr = 2, L + pad, uh.padded_len(L)
    src = _normal((B, Lr, ch), 2000 * ch + 10 * L + pad)
    src[:, L:] = float("nan")
    marker = -1.2345e30
    n_out = B * ch * ld
    out = torch.full((n_out + uh.GUARD // 4,), marker, device="cuda")
    dev = src.cuda()
    rc = Lh.facppg_posmajor_to_f32(lib.ptr(dev), B, ch, L, lib.ptr(out), ld, lib.current_stream(dev.device))
    torch.cuda.synchronize()
    assert rc == uh.OK, uh.last_error()
    assert bool((out[n_out:] == marker).all()), "wrote behind the output"
    got = out[:n_out].cpu().view(B, ch, ld)
    assert torch.equal(got[:, :, :L], src[:, :L].transpose(1, 2))
    assert bool((got[:, :, L:] == marker).all())


# ------------------------------------------------------------------------------------------ whole training steps
@pytest.mark.parametrize("hop,T,n_audio", [(256, 5, 1024), (256, 4, 1280), (160, 6, 1200)],
                         ids=["hop256", "hop256-tail", "hop160-tail"])
def test_training_step_bf16_vs_float64_oracle(hop, T, n_audio):
    """WaveGlow.forward + WaveGlowLoss + backward under train_precision = "bf16" against float64 autograd of the oracle, at hop 256
    and with audio longer than T hop (the upsampled samples past T hop are kernel tails and bias, not zero).  Tolerances of
    test_gpu_train_bf16.py: loss 2e-3 relative, every gradient norm 2e-2 relative, cosine of every full gradient >= 0.995."""
    from oracle import waveglow as owg
    from test_gpu_e2e import weightnorm_state_dict
    from waveglow.glow import WaveGlow, WaveGlowLoss
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop)
    assert (T - 1) * hop + 1024 >= n_audio
    m = WaveGlow(**cfg)
    m.load_state_dict(weightnorm_state_dict(synth.waveglow_state_dict(cfg)), strict=True)
    mel = synth.synthetic_mel(1, T, seed=hop + T)
    g = np.random.Generator(np.random.PCG64(n_audio))
    wav = torch.from_numpy(np.clip(0.1 * g.standard_normal((1, n_audio), dtype=np.float32), -1, 1))

    # float64 oracle on the CPU: effective weights w = g v / ||v|| of the weight-normed convolutions, as torch forms them
    leaves = {k: p.detach().double().requires_grad_(True) for k, p in m.named_parameters()}
    sd = {}
    for k, v in leaves.items():
        if k.endswith(".weight_v"):
            gk = leaves[k[:-1] + "g"]
            sd[k[:-2]] = v * (gk / v.flatten(1).norm(dim=1).view(-1, 1, 1))
        elif not k.endswith(".weight_g"):
            sd[k] = v
    ref_loss = owg.loss(*owg.forward(sd, cfg, mel.double(), wav.double()), sigma=0.7071)
    ref_loss.backward()

    m = m.cuda().train()
    m.train_precision = "bf16"
    m.zero_grad()
    loss = WaveGlowLoss(0.7071)(m((mel.cuda(), wav.cuda())))
    loss.backward()
    rel_loss = abs(float(loss) - float(ref_loss)) / max(1.0, abs(float(ref_loss)))
    rel, cos = {}, {}
    for k, p in m.named_parameters():
        a, b = p.grad.detach().cpu().double().reshape(-1), leaves[k].grad.reshape(-1)
        assert torch.isfinite(a).all(), k
        rel[k] = abs(float(a.norm()) - float(b.norm())) / max(float(b.norm()), 1e-6)
        cos[k] = float(a @ b) / max(1e-30, float(a.norm()) * float(b.norm()))
    wr, wc = max(rel, key=rel.get), min(cos, key=cos.get)
    print("bf16 step hop %d, T %d, audio %d: loss %.6f (float64 oracle %.6f, rel %.1e); grad-norm rel err max %.1e (%s); cosine min %.5f "
          "(%s); upsample.weight: norm rel %.1e cosine %.6f" % (hop, T, n_audio, float(loss), float(ref_loss), rel_loss, rel[wr], wr, cos[wc],
                                                                 wc, rel["upsample.weight"], cos["upsample.weight"]))
    assert rel_loss <= 2e-3
    assert rel[wr] <= 2e-2, (wr, rel[wr])
    assert cos[wc] >= 0.995, (wc, cos[wc])
