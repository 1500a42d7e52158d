"""GPU: the streamed batch-1 path on split-bf16 operands (pipeline.synthesize(vocoder_arithmetic="bf16x3", vocoder_stream=True):
ks_cond_seed's seed passes and the mel copy under the decoder, seeded 32-frame tiles of ks_wn_layer<.., SEED> behind it) against the
same utterance unstreamed -- bit for bit --, the seed kernel and the seeded tiles directly on WaveGlow, the accuracy of the
conditioning-first K order, the untouched plain "bf16x3" call, the kind switch on one model pair, and the refusals.  The synthetic
12-flow fp32 vocoder, injected dropout masks and z; the models and inputs of tests/stream_helpers.py with a runner that passes the
two keywords."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from helpers import golden, rms
from facppg import lib as flib
from facppg import synth
from stream_helpers import HOP, acoustic, halve, late_encode, make_vocoder, utterance
from test_gpu_waveglow_bf16x3 import RMS_TOL, _model, _references, _relerr

pytestmark = pytest.mark.gpu

ARITH = "bf16x3"
P = HOP // 8


@pytest.fixture(scope="module")
def vocoder():
    return make_vocoder()


def run(taco, wg, den, ppg, em, dm, zs, stream, monkeypatch, arithmetic=ARITH, opt_in=True):
    """One pipeline.synthesize call of the utterance with FACPPG_STREAM on or off -> (samples, Tout, what Tacotron2.inference saw)."""
    from facppg import pipeline
    monkeypatch.setenv("FACPPG_STREAM", "1" if stream else "0")
    monkeypatch.setenv("FACPPG_STREAM_MIN_FRAMES", "64")
    seen = {}
    inference = taco.inference

    def spy(*a, **kw):
        out = inference(*a, **kw)
        consumer = kw.get("frame_consumer")
        seen["mel_post"] = out[1].detach().clone()
        seen["streamed"] = consumer is not None and consumer.active
        seen["published"] = bool(out.launch.streamed)
        seen["kind"] = kw.get("frame_consumer_arithmetic")
        return out
    taco.inference = spy
    kw = {}
    if arithmetic is not None:
        kw["vocoder_arithmetic"] = arithmetic
    if opt_in:
        kw["vocoder_stream"] = True
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            wavs, tout = pipeline.synthesize([ppg], taco, wg, den, sigma=0.6, strength=0.005, dropout_masks=(em, dm), z=zs, **kw)
    finally:
        del taco.inference
    return wavs[0], tout[0], seen


@pytest.mark.parametrize("hop,T", [(256, 75), (160, 40)])
def test_seeds_and_seeded_tiles_directly(vocoder, hop, T):
    """T = 75 at hop 256: three tiles, the last half-filled; T = 40 at hop 160: kc = 560 is no multiple of 64 (the last chunk is
    zero-padded) and one tile's window is all the LDS holds (max_block_tiles == 1)."""
    if hop == HOP:
        cfg, wg, _ = vocoder
    else:
        wg, cfg, _ = _model(hop)
    dev = torch.device("cuda", 0)
    ph = hop // 8
    mel = synth.synthetic_mel(1, T, seed=91).cuda()
    zs = synth.synthetic_z(1, T * ph, cfg, seed=92)
    tqp, margin, nbytes, bt_max = wg.seed_layout(T, dev, arithmetic=ARITH)
    assert bt_max == (3 if hop == 256 else 1)
    melp = wg.mel_pad(mel, arithmetic=ARITH)
    assert melp.dtype == torch.float32 and melp.shape == (tqp, 80)
    assert torch.equal(melp[margin:margin + T], mel[0].t()) and not melp[:margin].any() and not melp[margin + T:].any()
    n_tiles = (tqp - 2 * margin) // 32
    assert nbytes == cfg["n_flows"] * 8 * ph * n_tiles * 65536
    used = -(-T // 32)                    # tiles the utterance touches
    full = 32 * (used - 1)                # frames of all but the last of them
    SENT = -7.0

    def buf():
        return torch.full((nbytes // 4,), SENT, dtype=torch.float32, device=dev)
    a, b, c, d = buf(), buf(), buf(), buf()
    wg.cond_seed(melp, T, 0, full, a, block_tiles=1, layers_per_workgroup=1, arithmetic=ARITH)
    for t in range(used - 1):             # tile by tile, two layers per work item
        wg.cond_seed(melp, T, 32 * t, 32, b, block_tiles=1, layers_per_workgroup=2, arithmetic=ARITH)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    wg.cond_seed(melp, T, 0, full, c, block_tiles=bt_max, layers_per_workgroup=2, max_workgroups=64, counter=counter, arithmetic=ARITH)
    wg.cond_seed(melp, T, 0, full, d, block_tiles=bt_max, skip=torch.ones(1, dtype=torch.int32, device=dev), arithmetic=ARITH)
    tiles = a.view(-1, n_tiles, 16384)
    assert not (tiles[:, :used - 1] == SENT).any() and torch.isfinite(tiles[:, :used - 1]).all()   # every seeded register was written
    assert (tiles[:, used - 1:] == SENT).all()                                                   # and nothing else
    assert int(counter) > 0                                                                      # the bounded launch took items from the counter
    assert torch.equal(a, b) and torch.equal(a, c)
    assert (d == SENT).all()                                                                     # a raised skip flag: untouched
    for bt in range(2, bt_max + 1):       # every block width up to the largest
        d.fill_(SENT)
        wg.cond_seed(melp, T, 0, full, d, block_tiles=bt, layers_per_workgroup=1, arithmetic=ARITH)
        assert torch.equal(a, d), bt
    with pytest.raises(flib.FacppgError, match="maximum is %d" % bt_max):
        wg.cond_seed(melp, T, 0, full, d, block_tiles=bt_max + 1, arithmetic=ARITH)
    del b, c, d
    ref = wg.infer_seeded(melp, T, None, 0, sigma=0.6, z=zs, arithmetic=ARITH)
    assert wg.last_launch_shape(ARITH) == (32, 8, used * ph)
    assert ref.dtype == torch.float32 and ref.shape == (1, T * hop) and torch.isfinite(ref).all()
    for s in range(0, full + 1, 32):
        got = wg.infer_seeded(melp, T, a, s, sigma=0.6, z=zs, arithmetic=ARITH)
        assert wg.last_launch_shape(ARITH) == (32, 8, used * ph)
        assert got.dtype == torch.float32 and torch.equal(got, ref), s
    wg.cond_seed(melp, T, full, 32, a, arithmetic=ARITH)      # the half-filled last tile seeded too (frames past T are zero mel)
    assert torch.equal(wg.infer_seeded(melp, T, a, 32 * used, sigma=0.6, z=zs, arithmetic=ARITH), ref)
    # the new K order really ran: not the bits of the tap-first call
    plain = wg.infer(mel, sigma=0.6, z=zs, arithmetic=ARITH)
    assert plain.shape == ref.shape and not torch.equal(plain, ref)
    # a layout for more frames than the utterance has (the stream's cap)
    tqp2, _, nbytes2, _ = wg.seed_layout(200, dev, arithmetic=ARITH)
    melp2 = torch.zeros(tqp2, 80, dtype=torch.float32, device=dev)
    wg.mel_convert(mel[0], 200, 0, T, melp2, arithmetic=ARITH)
    a2 = torch.full((nbytes2 // 4,), SENT, dtype=torch.float32, device=dev)
    wg.cond_seed(melp2, 200, 0, full, a2, block_tiles=bt_max, arithmetic=ARITH)
    assert torch.equal(wg.infer_seeded(melp2, T, a2, full, sigma=0.6, z=zs, T_layout=200, arithmetic=ARITH), ref)
    del a2
    # refusals: seeded_frames whole tiles, at most T rounded up; the first seeded frame a tile's; the kinds of buffer and module
    for bad in (16, 128, -32):
        with pytest.raises(flib.FacppgError, match="seeded_frames"):
            wg.infer_seeded(melp, T, a, bad, sigma=0.6, z=zs, arithmetic=ARITH)
    with pytest.raises(flib.FacppgError, match="multiple of 32"):
        wg.cond_seed(melp, T, 16, 32, a, arithmetic=ARITH)
    for call in (lambda: wg.cond_seed(melp.half(), T, 0, 32, a, arithmetic=ARITH),
                 lambda: wg.infer_seeded(melp.half(), T, a, 0, sigma=0.6, z=zs, arithmetic=ARITH),
                 lambda: wg.mel_convert(mel[0], T, 0, T, melp.half(), arithmetic=ARITH)):
        with pytest.raises(flib.FacppgError, match="fp32 mel buffer"):
            call()
    half, _, _ = _model(hop)
    halve(half)
    for call in (lambda: half.seed_layout(T, dev, arithmetic=ARITH), lambda: half.mel_pad(mel, arithmetic=ARITH),
                 lambda: half.cond_seed(melp, T, 0, 32, a, arithmetic=ARITH),
                 lambda: half.infer_seeded(melp, T, a, 0, sigma=0.6, z=zs, arithmetic=ARITH)):
        with pytest.raises(flib.FacppgError, match="all-fp32 module"):
            call()
    # the raw ABI
    L = flib.load()
    hs = wg._split_handle(dev)
    null = ctypes.c_void_p(0)
    st = flib.current_stream(dev)
    ptr = flib.ptr
    need = L.facppg_wg_split_workspace_bytes(hs, 1, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    audio = torch.empty(1, T * hop, device=dev)
    i1, i2, i3, sz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert L.facppg_wg_split_seed_layout(null, T, ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(sz), ctypes.byref(i3)) == -1
    assert L.facppg_wg_split_seed_layout(hs, T, ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(sz), ctypes.byref(i3)) == 0
    assert (i1.value, i2.value, sz.value, i3.value) == (tqp, margin, nbytes, bt_max)
    args = lambda h, mp, sp, ap, wp, n: (h, mp, T, T, sp, 32, null, 1, 0.6, ap, wp, n, null, st)     # noqa: E731
    for bad in (args(null, ptr(melp), ptr(a), ptr(audio), ptr(ws), need), args(hs, null, ptr(a), ptr(audio), ptr(ws), need),
                args(hs, ptr(melp), null, ptr(audio), ptr(ws), need), args(hs, ptr(melp), ptr(a), null, ptr(ws), need)):
        assert L.facppg_wg_split_infer_seeded(*bad) == -1 and b"NULL" in L.facppg_last_error()
    assert L.facppg_wg_split_infer_seeded(*args(hs, ptr(melp), ptr(a), ptr(audio), ptr(ws), need - 1)) == -4
    assert b"workspace" in L.facppg_last_error()
    assert L.facppg_wg_split_mel_pad(null, ptr(mel), T, T, 0, T, ptr(melp), null, st) == -1
    assert L.facppg_wg_split_mel_pad(hs, ptr(mel), T, T, 0, T + 1, ptr(melp), null, st) == -1
    assert L.facppg_wg_split_cond_seed(null, ptr(melp), T, 0, 32, 1, 1, 0, 0, ptr(a), nbytes, null, 0, null, st) == -1
    assert L.facppg_wg_split_cond_seed(hs, ptr(melp), T, 0, 32, 1, 1, 0, 0, ptr(a), nbytes - 1, null, 0, null, st) == -4   # EWORKSPACE
    assert L.facppg_wg_split_infer_seeded(*args(hs, ptr(melp), ptr(a), ptr(audio), ptr(ws), need)) == 0   # and the handle still works
    torch.cuda.synchronize()
    assert torch.isfinite(audio).all()


def _streamed_against_unstreamed(vocoder, Tin, steps, gate_bias, monkeypatch):
    from facppg.pipeline import ConditioningStream
    cfg, wg, den = vocoder
    hp, taco = acoustic(steps, gate_bias)
    ppg, em, dm = utterance(hp, Tin, steps, Tin)
    t_ref = steps
    if gate_bias > -1:             # (the gate decides the length: one run to learn it)
        _, t_ref, _ = run(taco, wg, den, ppg, em, dm, None, False, monkeypatch)
    zs = synth.synthetic_z(1, t_ref * P, cfg, seed=23)
    ref, t_ref, seen_ref = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    shape_ref = wg.last_launch_shape(ARITH)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    cap = min(steps, -(-(Tin + ConditioningStream.SLACK) // 32) * 32)
    assert not seen_ref["streamed"] and seen["streamed"] == (t_ref <= cap)          # the stream really ran (or the decoder outran cap)
    assert not seen_ref["published"] and seen["published"] and seen["kind"] == ARITH
    assert t_out == t_ref and (gate_bias > -1 or t_ref == steps)
    cs = wg.__dict__["_facppg_cond_stream"]
    tile, waves, tiles = wg.last_launch_shape(ARITH)
    print("Tin %d steps %d: Tout %d, streamed %s, blocks %s, seeded %s, tile %d x %d" % (
        Tin, steps, t_out, seen["streamed"], cs.cuts if seen["streamed"] else None, cs.seeded if seen["streamed"] else None, tile, tiles))
    assert (tile, waves, tiles) == shape_ref == (32, 8, -(-t_out // 32) * P)        # streamed or not: the seeded launches
    if seen["streamed"]:
        assert cs.split and not cs.half and cs.melp_split is not None and cs.melp16 is None
        assert cs.seeded % 32 == 0 and (cs.seeded > 0 or t_out - cs.lag < 32)
    assert seen["mel_post"].dtype == torch.float32 and torch.equal(seen["mel_post"], seen_ref["mel_post"])
    assert out.dtype == np.float32 and out.shape == ref.shape == (t_ref * HOP,) and np.array_equal(out, ref)
    assert np.isfinite(out).all() and rms(out) > 0
    # the tail tiles (the half-filled last one included): seeded by one more pass behind the decoder (the default, above), or
    # unseeded inside the layer launches -- the same bits
    monkeypatch.setenv("FACPPG_STREAM_TAIL", "mixed")
    out_m, t_m, seen_m = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    assert seen_m["streamed"] == seen["streamed"] and t_m == t_ref and np.array_equal(out_m, ref)
    assert wg.last_launch_shape(ARITH) == (tile, waves, tiles)
    # and the unstreamed call is mel_pad + infer_seeded with no seeded frame, on the same mel_post
    mel_post = seen_ref["mel_post"][:, :, :t_ref].contiguous()
    direct = wg.infer_seeded(wg.mel_pad(mel_post, arithmetic=ARITH), t_ref, None, 0, sigma=0.6, z=zs, arithmetic=ARITH)
    direct = den(direct, strength=0.005)[:, 0]
    assert np.array_equal(direct[0].cpu().numpy(), ref)


@pytest.mark.parametrize("Tin,steps,gate_bias", [(64, 64, -10.0), (75, 75, -10.0), (96, 96, -10.0), (150, 1000, -0.02), (130, 400, -10.0)])
def test_streamed_split_utterance_equals_the_unstreamed_one_bit_for_bit(vocoder, Tin, steps, gate_bias, monkeypatch):
    _streamed_against_unstreamed(vocoder, Tin, steps, gate_bias, monkeypatch)


def test_void_blocks_change_no_bit(vocoder, monkeypatch):
    """The fp16 suite's timed-out-blocks scenario: the collectors give up after 1 us while a spin kernel holds the first frames
    back, the blocks are void, their frames are copied and run unseeded (or seeded by the tail pass) behind the decoder."""
    cfg, wg, den = vocoder
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 5)
    zs = synth.synthetic_z(1, steps * P, cfg, seed=63)
    ref, t_ref, _ = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    cs = wg.__dict__["_facppg_cond_stream"]
    seeded_all = cs.seeded
    assert seen["streamed"] and cs.split and cs.void_blocks == 0 and seeded_all == 64 and np.array_equal(out, ref)
    monkeypatch.setenv("FACPPG_STREAM_WAIT_MS", "0.001")
    late_encode(monkeypatch)
    out, t_out, seen = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    print("blocks", cs.cuts, "void", cs.void_blocks, "seeded frames", cs.seeded)
    assert seen["streamed"] and cs.void_blocks > 0 and cs.seeded < seeded_all
    assert t_out == t_ref and np.array_equal(out, ref)


def test_the_plain_bf16x3_call_is_untouched(vocoder, monkeypatch):
    """Without the keyword a "bf16x3" call keeps its K order, its bits and its unstreamed path, before and after opt-in calls on
    the same models; the opt-in samples differ from it in some bit (the other order ran) and by no more than the arithmetic's own
    error, 3 e_emu (the bar of tests/test_gpu_waveglow_bf16x3.py; e_emu accumulates in float64 and favours neither order)."""
    cfg, wg, den = vocoder
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 7)
    zs = synth.synthetic_z(1, steps * P, cfg, seed=29)
    before, t0, seen0 = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch, opt_in=False)
    assert not seen0["streamed"] and not seen0["published"] and seen0["kind"] is None
    assert wg.last_launch_shape(ARITH)[2] == P * -(-steps // wg.last_launch_shape(ARITH)[0])
    opt, t1, seen1 = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    assert seen1["streamed"] and seen1["published"]
    after, t2, seen2 = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch, opt_in=False)
    assert not seen2["streamed"] and not seen2["published"]
    assert t0 == t1 == t2 == steps and np.array_equal(before, after)
    mel_post = seen0["mel_post"][:, :, :steps].contiguous()
    direct = den(wg.infer(mel_post, sigma=0.6, z=zs, arithmetic=ARITH), strength=0.005)[:, 0]
    assert np.array_equal(direct[0].cpu().numpy(), before)
    e_emu = _references(HOP)[2]
    e = _relerr(opt, before)
    print("opt-in against plain bf16x3: rel rms %.3e (3 e_emu = %.3e)" % (e, 3 * e_emu))
    assert not np.array_equal(opt, before)
    assert e <= 3.0 * e_emu


@pytest.mark.parametrize("hop", [256, 160])
def test_accuracy_of_the_conditioning_first_order(hop):
    """The case of test_accuracy_against_the_emulated_split_arithmetic, each utterance as B = 1 through mel_pad + cond_seed (all
    tiles) + infer_seeded.  Requirement: relative RMS against the fp32 CPU oracle <= 3 e_emu, and RMS <= 1e-3 against the golden
    audio of the reference's outputs, utterance by utterance."""
    m, cfg, _ = _model(hop)
    dev = torch.device("cuda", 0)
    ph = hop // 8
    lengths, sigma = [24, 17], 0.6
    B, T = len(lengths), max(lengths)
    mel = synth.synthetic_mel(B, T, seed=31).cuda()
    zs = synth.synthetic_z(B, T * ph, cfg, seed=32)

    def seeded_infer(mel_b, z_b, Tb):
        melp = m.mel_pad(mel_b, arithmetic=ARITH)
        nbytes, bt_max = m.seed_layout(Tb, dev, arithmetic=ARITH)[2:]
        seeds = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        m.cond_seed(melp, Tb, 0, Tb, seeds, block_tiles=bt_max, arithmetic=ARITH)
        out = m.infer_seeded(melp, Tb, seeds, -(-Tb // 32) * 32, sigma=sigma, z=z_b, arithmetic=ARITH)
        assert out.shape == (1, Tb * hop) and out.dtype == torch.float32
        return out[0].cpu()
    ahip = torch.cat([seeded_infer(mel[b:b + 1, :, :Tb].contiguous(), [z[b:b + 1, :, :Tb * ph] for z in zs], Tb)
                      for b, Tb in enumerate(lengths)]).numpy()
    a32, aemu, e_emu = _references(hop)
    e_hip = _relerr(ahip, a32)
    print("hop %d: e_emu %.3e  e_hip (conditioning first, seeded) %.3e  (hip against the emulation %.3e)" % (
        hop, e_emu, e_hip, _relerr(ahip, aemu)))
    assert np.isfinite(ahip).all()
    assert e_hip <= 3.0 * e_emu
    d = golden("waveglow_hop%d.npz" % hop)
    Bg, Tg = int(d["B"]), int(d["T"])
    melg = synth.synthetic_mel(Bg, Tg, seed=int(d["mel_seed"])).cuda()
    zg = synth.synthetic_z(Bg, Tg * ph, cfg, seed=int(d["z_seed"]))
    sigma = float(d["sigma"])
    for b in range(Bg):
        out = seeded_infer(melg[b:b + 1].contiguous(), [z[b:b + 1] for z in zg], Tg).numpy()
        e = rms(out - d["audio"][b])
        print("hop %d utterance %d: rms against the golden audio %.3e" % (hop, b, e))
        assert e <= RMS_TOL


def test_kind_switch_on_one_model_pair(vocoder, monkeypatch):
    """fp32 streamed -> bf16x3 streamed (opt-in) -> fp32 streamed through one ConditioningStream: the buffers are re-laid-out per
    kind and every utterance equals its unstreamed run."""
    cfg, wg, den = vocoder
    Tin = steps = 96
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 311)
    zs = synth.synthetic_z(1, steps * P, cfg, seed=23)
    ref32, _, s0 = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch, arithmetic=None, opt_in=False)
    refsp, _, s1 = run(taco, wg, den, ppg, em, dm, zs, False, monkeypatch)
    assert not s0["streamed"] and not s1["streamed"]
    first, _, sa = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch, arithmetic=None, opt_in=False)
    cs = wg.__dict__["_facppg_cond_stream"]
    assert sa["streamed"] and not cs.split and cs.melp_split is None
    second, _, sb = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch)
    assert wg.__dict__["_facppg_cond_stream"] is cs and sb["streamed"] and cs.split and cs.melp_split is not None
    third, _, sc = run(taco, wg, den, ppg, em, dm, zs, True, monkeypatch, arithmetic=None, opt_in=False)
    assert wg.__dict__["_facppg_cond_stream"] is cs and sc["streamed"] and not cs.split
    assert np.array_equal(first, ref32) and np.array_equal(third, ref32)
    assert np.array_equal(second, refsp) and not np.array_equal(refsp, ref32)


def test_refusals_at_the_pipeline(monkeypatch):
    from facppg import pipeline
    cfg, wg16, den16 = make_vocoder(half=True)
    Tin = steps = 64
    hp, taco = acoustic(steps, -10.0)
    ppg, em, dm = utterance(hp, Tin, steps, 17)
    zs = synth.synthetic_z(1, steps * P, cfg, seed=23)
    calls = []
    inference = taco.inference
    taco.inference = lambda *a, **kw: calls.append(1) or inference(*a, **kw)
    try:
        with pytest.raises(flib.FacppgError, match="vocoder_stream"):
            pipeline.synthesize([ppg], taco, wg16, den16, vocoder_stream="yes")
        with pytest.raises(flib.FacppgError, match="vocoder_stream"):
            pipeline.synthesize([ppg], taco, wg16, den16, vocoder_arithmetic=ARITH, vocoder_stream=False)
    finally:
        del taco.inference
    assert not calls                                         # refused before any model ran
    # the keyword with an arithmetic that streams by its own rules: nothing changes
    plain, t0, s0 = run(taco, wg16, den16, ppg, em, dm, zs, True, monkeypatch, arithmetic=None, opt_in=False)
    keyed, t1, s1 = run(taco, wg16, den16, ppg, em, dm, zs, True, monkeypatch, arithmetic=None, opt_in=True)
    assert s0["streamed"] and s1["streamed"] and s1["kind"] is None and t0 == t1 == steps
    assert wg16.__dict__["_facppg_cond_stream"].half and not wg16.__dict__["_facppg_cond_stream"].split
    assert np.array_equal(plain, keyed)
    # and a half vocoder asked for split operands is refused by the vocoder stage: the plain call as it always was, the opt-in
    # call by the seeded methods
    with pytest.raises(flib.FacppgError, match="arithmetic='bf16x3'"):
        run(taco, wg16, den16, ppg, em, dm, zs, True, monkeypatch, opt_in=False)
    with pytest.raises(flib.FacppgError, match="all-fp32 module"):
        run(taco, wg16, den16, ppg, em, dm, zs, True, monkeypatch, opt_in=True)
