"""GPU: the streamed batch-1 path with a .half() vocoder (facppg.pipeline.ConditioningStream on the fp16 kernels: k16_cond_seed's
seed passes and the fp32 -> fp16 mel conversion under the decoder, seeded 32-frame tiles of k16_wn_layer behind it) against the
same utterance unstreamed -- bit for bit --, the seed kernel and the seeded tiles directly on WaveGlow, the accuracy of the
conditioning-first K order, and the refusals.  Hop 256, the synthetic 12-flow vocoder halved by the reference's recipe
(inference.py:40-43: convinv kept in float), injected dropout masks and z; the harness of tests/stream_helpers.py."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import golden, rms
from facppg import lib as flib
from facppg import synth
from stream_helpers import HOP, acoustic, halve, late_encode, make_vocoder, run, utterance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocoder():
    return make_vocoder(half=True)


@pytest.mark.parametrize("Tin,steps,gate_bias", [(64, 64, -10.0), (75, 75, -10.0), (96, 96, -10.0), (150, 1000, -0.02), (130, 400, -10.0)])
def test_streamed_half_utterance_equals_the_unstreamed_one_bit_for_bit(vocoder, Tin, steps, gate_bias, monkeypatch):
    from facppg.pipeline import ConditioningStream
    cfg, wg, den = vocoder
    hp, taco = acoustic(steps, gate_bias)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    t_ref = steps
    if gate_bias > -1:             # (the gate decides the length: one run to learn it)
        _, t_ref, _ = run(taco, wg, den, ppg, em, dm, None, False, monkeypatch)
    zs = synth.synthetic_z(1, t_ref * HOP // 8, cfg, seed=23)
    ref, t_ref, seen_ref = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    cap = min(steps, -(-(Tin + ConditioningStream.SLACK) // 32) * 32)
    assert not seen_ref["streamed"] and seen["streamed"] == (t_ref <= cap)          # the stream really ran (or the decoder outran cap)
    assert not seen_ref["published"] and seen["published"]
    assert t_out == t_ref and (gate_bias > -1 or t_ref == steps)
    cs = wg.__dict__["_facppg_cond_stream"]
    tile, waves, tiles = wg.last_launch_shape()
    print("Tin %d steps %d: Tout %d, streamed %s, blocks %s, seeded %s, tile %d x %d" % (
        Tin, steps, t_out, seen["streamed"], cs.cuts if seen["streamed"] else None, cs.seeded if seen["streamed"] else None, tile, tiles))
    if seen["streamed"]:
        assert cs.half and (tile, waves, tiles) == (32, 8, -(-t_out // 32) * (HOP // 8))
        assert cs.seeded % 32 == 0 and (cs.seeded > 0 or t_out - cs.lag < 32)
    assert seen["mel_post"].dtype == torch.float32 and torch.equal(seen["mel_post"], seen_ref["mel_post"])
    assert out.dtype == np.float32 and out.shape == ref.shape == (t_ref * HOP,) and np.array_equal(out, ref)
    assert np.isfinite(out).all() and rms(out) > 0
    # the tail tiles (the half-filled last one included): seeded by one more pass behind the decoder (the default, above), or
    # unseeded inside the layer launches -- the same bits
    monkeypatch.setenv("FACPPG_STREAM_TAIL", "mixed")
    out_m, t_m, seen_m = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    assert seen_m["streamed"] == seen["streamed"] and t_m == t_ref and np.array_equal(out_m, ref)
    if seen["streamed"]:
        assert wg.last_launch_shape() == (tile, waves, tiles)


def test_void_blocks_change_no_bit(vocoder, monkeypatch):
    """The fp32 suite's timed-out-blocks scenario with the half vocoder: the collectors give up after 1 us while a spin kernel
    holds the first frames back, the blocks are void, their frames are converted and run unseeded behind the decoder."""
    cfg, wg, den = vocoder
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 5)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=63)
    ref, t_ref, _ = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    cs = wg.__dict__["_facppg_cond_stream"]
    seeded_all = cs.seeded
    assert seen["streamed"] and cs.void_blocks == 0 and seeded_all == 64 and np.array_equal(out, ref)
    monkeypatch.setenv("FACPPG_STREAM_WAIT_MS", "0.001")
    late_encode(monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    print("blocks", cs.cuts, "void", cs.void_blocks, "seeded frames", cs.seeded)
    assert seen["streamed"] and cs.void_blocks > 0 and cs.seeded < seeded_all
    assert t_out == t_ref and np.array_equal(out, ref)


def test_seeds_and_seeded_tiles_directly(vocoder):
    cfg, wg, _ = vocoder
    dev = torch.device("cuda", 0)
    T = 75
    mel = synth.synthetic_mel(1, T, seed=91).cuda()
    zs = synth.synthetic_z(1, T * HOP // 8, cfg, seed=92)
    tqp, margin, nbytes = wg.seed_layout(T, dev)
    melp = wg.mel_pad(mel)
    assert melp.dtype == torch.float16 and melp.shape == (tqp, 80)
    assert torch.equal(melp[margin:margin + T], mel[0].t().half()) and not melp[:margin].any() and not melp[margin + T:].any()
    n_tiles = (tqp - 2 * margin) // 32
    assert nbytes == cfg["n_flows"] * 8 * (HOP // 8) * n_tiles * 65536
    SENT = -7.0

    def buf():
        return torch.full((nbytes // 4,), SENT, dtype=torch.float32, device=dev)
    a, b, c, d = buf(), buf(), buf(), buf()
    wg.cond_seed(melp, T, 0, 64, a, block_tiles=2, layers_per_workgroup=1)
    wg.cond_seed(melp, T, 0, 32, b, block_tiles=1, layers_per_workgroup=1)
    wg.cond_seed(melp, T, 32, 32, b, block_tiles=1, layers_per_workgroup=1)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    wg.cond_seed(melp, T, 0, 64, c, block_tiles=1, layers_per_workgroup=2, max_workgroups=64, counter=counter)
    wg.cond_seed(melp, T, 0, 64, d, block_tiles=2, skip=torch.ones(1, dtype=torch.int32, device=dev))
    tiles = a.view(-1, n_tiles, 16384)
    assert not (tiles[:, :2] == SENT).any() and torch.isfinite(tiles[:, :2]).all()      # every seeded register was written
    assert (tiles[:, 2:] == SENT).all()                                               # and nothing else
    assert int(counter) > 0                                                           # the bounded launch took items from the counter
    assert torch.equal(a, b) and torch.equal(a, c)
    assert (d == SENT).all()                                                          # a raised skip flag: untouched
    del b, c, d
    ref = wg.infer(mel.half(), sigma=0.6, z=zs, cond_first=True)
    assert ref.dtype == torch.float16 and torch.isfinite(ref.float()).all()
    for s in (0, 32, 64):
        got = wg.infer_seeded(melp, T, a, s, sigma=0.6, z=zs)
        assert wg.last_launch_shape() == (32, 8, 3 * (HOP // 8))
        assert got.dtype == torch.float16 and torch.equal(got, ref), s
    wg.cond_seed(melp, T, 64, 32, a)                   # the half-filled last tile seeded too (frames past T are zero mel)
    assert torch.equal(wg.infer_seeded(melp, T, a, 96, sigma=0.6, z=zs), ref)
    # a layout for more frames than the utterance has (the stream's cap)
    tqp2, _, nbytes2 = wg.seed_layout(200, dev)
    melp2 = torch.zeros(tqp2, 80, dtype=torch.float16, device=dev)
    wg.mel_convert(mel[0], 200, 0, T, melp2)
    a2 = torch.full((nbytes2 // 4,), SENT, dtype=torch.float32, device=dev)
    wg.cond_seed(melp2, 200, 0, 64, a2, block_tiles=2)
    assert torch.equal(wg.infer_seeded(melp2, T, a2, 64, sigma=0.6, z=zs, T_layout=200), ref)
    # seeded_frames: whole tiles, at most T rounded up
    for bad in (16, 128, -32):
        with pytest.raises(flib.FacppgError, match="seeded_frames"):
            wg.infer_seeded(melp, T, a, bad, sigma=0.6, z=zs)
    with pytest.raises(flib.FacppgError, match="multiple of 32"):
        wg.cond_seed(melp, T, 16, 32, a)
    torch.cuda.synchronize()


@pytest.mark.parametrize("hop", [256, 160])
def test_conditioning_first_order_at_least_as_accurate_as_reference_half_branch(hop):
    """The yardstick of test_half_infer_at_least_as_accurate_as_reference_half_branch -- same shapes and inputs, same fp32 oracle,
    same restated reference half branch, same 1.5 x bound -- applied to the conditioning-first K order.  The two CPU references
    take a minute to compute; they are read from tests/golden/waveglow_half_yardstick_hop*.npz (written from exactly that
    test's code by tests/golden/make_half_yardstick.py)."""
    from test_gpu_waveglow_f16 import _model, _relerr
    d = golden("waveglow_half_yardstick_hop%d.npz" % hop)
    m, cfg, sd = _model(hop, half=True)
    lengths, sigma = [int(v) for v in d["lengths"]], float(d["sigma"])
    assert lengths == [24, 17] and sigma == 0.6
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=int(d["mel_seed"]))
    zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=int(d["z_seed"]))
    z16 = [z.half() for z in zs]
    plain = m.infer(mel.half().cuda(), sigma=sigma, z=z16, lengths=lengths)
    assert torch.equal(m.infer(mel.half().cuda(), sigma=sigma, z=z16, lengths=lengths, cond_first=False), plain)
    out = m.infer(mel.half().cuda(), sigma=sigma, z=z16, lengths=lengths, cond_first=True)
    assert out.shape == (B, T * hop) and out.dtype == torch.float16
    out = out.float().cpu()
    for b, Tb in enumerate(lengths):
        assert torch.all(out[b, Tb * hop:] == 0)
    ahip, aplain = (torch.cat([v[b, :Tb * hop] for b, Tb in enumerate(lengths)]).numpy() for v in (out, plain.float().cpu()))
    a32, aref = d["a32"], d["aref"]
    assert a32.shape == aref.shape == ahip.shape
    e_ref, e_hip, e_plain = _relerr(aref, a32), _relerr(ahip, a32), _relerr(aplain, a32)
    print("hop %d: err(aref16) %.3e  err(ahip16, cond_first) %.3e  err(ahip16, tap-first) %.3e  same bits: %s" % (
        hop, e_ref, e_hip, e_plain, np.array_equal(ahip, aplain)))
    assert np.isfinite(ahip).all()
    assert e_hip <= 1.5 * e_ref


def test_streamed_half_against_the_fp32_pipeline(vocoder, monkeypatch):
    cfg, wg, den = vocoder
    _, wg32, den32 = make_vocoder()
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=23)
    a16, t16, seen16 = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    a32, t32, seen32 = run(taco, wg32, den32, ppg, em, dm, zs, True, monkeypatch)
    assert seen16["streamed"] and seen32["streamed"] and t16 == t32 == steps
    e = rms(a16.astype(np.float64) - a32.astype(np.float64)) / rms(a32.astype(np.float64))
    print("streamed half vs fp32 pipeline: rel rms %.3e" % e)
    assert e <= 1e-2


def test_refusals(vocoder):
    cfg, wg, _ = vocoder
    from test_gpu_waveglow_f16 import _model
    m32, _, _ = _model(HOP)
    m16, _, _ = _model(HOP, half=True)
    dev = torch.device("cuda", 0)
    T = 40
    mel = synth.synthetic_mel(1, T, seed=61).cuda()
    with pytest.raises(flib.FacppgError, match="cond_first"):
        m32.infer(mel, cond_first=True)
    assert m32.infer(mel, sigma=0.0, cond_first=False).dtype == torch.float32
    L = flib.load()
    h16, h32 = m16._handle(dev), m32._handle(dev)
    null = ctypes.c_void_p(0)
    st = flib.current_stream(dev)
    i1, i2, sz = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    # an fp32 handle into every new entry point
    assert L.facppg_wg_seed_layout_f16(h32, T, ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(sz)) == -1 and b"fp32" in L.facppg_last_error()
    assert L.facppg_wg_seed_layout_f16(h16, T, ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(sz)) == 0
    tqp, nbytes = i1.value, sz.value
    melp16 = torch.zeros(tqp, 80, dtype=torch.float16, device=dev)
    melp32 = torch.zeros(80, tqp + 64, device=dev)
    seeds = torch.zeros(nbytes // 4, device=dev)
    ws = torch.empty(max(L.facppg_wg_workspace_bytes(h16, 1, T), L.facppg_wg_workspace_bytes(h32, 1, T)), dtype=torch.uint8, device=dev)
    a16 = torch.empty(1, T * HOP, dtype=torch.float16, device=dev)
    a32 = torch.empty(1, T * HOP, device=dev)
    P = flib.ptr
    assert L.facppg_wg_mel_pad_f16(h32, P(mel), T, T, 0, T, P(melp16), null, st) == -1 and b"fp32" in L.facppg_last_error()
    assert L.facppg_wg_cond_seed_f16(h32, P(melp16), T, 0, 32, 1, 1, 0, 0, P(seeds), nbytes, null, 0, null, st) == -1
    assert b"fp32" in L.facppg_last_error()
    assert L.facppg_wg_infer_seeded_f16(h32, P(melp16), T, T, P(seeds), 32, null, 1, 0.6, P(a16), P(ws), ws.numel(), null, st) == -1
    assert b"fp32" in L.facppg_last_error()
    assert L.facppg_wg_infer_f16_order(h32, P(mel.half()), null, null, 1, 0.6, 1, T, 1, P(a16), P(ws), ws.numel(), st) == -1
    assert b"fp32" in L.facppg_last_error()
    # an fp16 handle into the fp32 seeded entry points
    assert L.facppg_wg_seed_layout(h16, T, ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(sz)) == -1 and b"fp16" in L.facppg_last_error()
    assert L.facppg_wg_mel_pad(h16, P(mel), T, T, P(melp32), st) == -1 and b"fp16" in L.facppg_last_error()
    assert L.facppg_wg_cond_seed(h16, P(melp32), T, 0, 32, 1, 1, 0, 0, P(seeds), nbytes, null, 0, null, st) == -1 and b"fp16" in L.facppg_last_error()
    assert L.facppg_wg_infer_seeded(h16, P(melp32), T, T, P(seeds), 32, null, 1, 0.6, P(a32), P(ws), ws.numel(), null, st) == -1
    assert b"fp16" in L.facppg_last_error()
    # seeded_frames: whole tiles, at most T rounded up; K order 0 or 1; the frame range of the conversion inside the layout
    for bad in (8, 96):
        assert L.facppg_wg_infer_seeded_f16(h16, P(melp16), T, T, P(seeds), bad, null, 1, 0.6, P(a16), P(ws), ws.numel(), null, st) == -1
        assert b"seeded_frames" in L.facppg_last_error()
    assert L.facppg_wg_infer_f16_order(h16, P(mel.half()), null, null, 1, 0.6, 1, T, 2, P(a16), P(ws), ws.numel(), st) == -1
    assert L.facppg_wg_mel_pad_f16(h16, P(mel), T, T, 0, T + 1, P(melp16), null, st) == -1
    assert L.facppg_wg_cond_seed_f16(h16, P(melp16), T, 0, 32, 1, 1, 0, 0, P(seeds), nbytes - 1, null, 0, null, st) == -4   # EWORKSPACE
    # the Python layer names a mel buffer of the wrong kind before any launch
    with pytest.raises(flib.FacppgError, match="fp16"):
        m16.cond_seed(melp32, T, 0, 32, seeds)
    torch.cuda.synchronize()


def test_precision_switch_between_streamed_utterances(monkeypatch):
    """.float() + reload, then .half() again, between streamed utterances on the same model pair: the handle, the stream and its
    layouts are rebuilt for the precision at hand, and every utterance still equals its unstreamed run."""
    cfg, wg, den = make_vocoder(half=True)
    sd = synth.waveglow_state_dict(cfg)
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    zs = synth.synthetic_z(1, steps * HOP // 8, cfg, seed=23)
    results, streams = [], []
    for i, half in enumerate((True, False, True)):
        if i == 1:
            wg.float()
            wg.load_state_dict(sd)
        elif i == 2:
            halve(wg)
        ppg, em, dm = utterance(hp, Tin, steps, 300 + i)
        ref, _, seen_ref = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
        out, _, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
        cs = wg.__dict__["_facppg_cond_stream"]
        assert seen["streamed"] and not seen_ref["streamed"] and cs.half == half
        assert cs.seeds.dtype == torch.float32 and (cs.melp16 is not None) == half
        assert np.array_equal(out, ref), i
        results.append(out)
        streams.append(cs)
    assert streams[0] is not streams[1] and streams[1] is not streams[2]
