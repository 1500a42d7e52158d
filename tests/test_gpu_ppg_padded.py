"""GPU: the acoustic model's posteriors in the layout the encoder reads (facppg_tdnn_forward_batch_padded,
ppg.compute_ppg_padded): out [B][K][Tmax], channel-major with the frames contiguous, exactly 0 behind each utterance.

The recipe is test_gpu_ppg_batch.py's: its synthetic nnet3 TDNN (hidden 128, 5816 senones, renorm layers, left context 6 !=
right context 7), the reference's final.mat / reduce_dim.mat, frames (1, 5, 37, 150) from its four wavs -- an utterance
shorter than either context, one shorter than the 16-frame tile of the output kernel, one that is no multiple of it, segment
starts 0 / 16 / 36 / 88 (multiples of 4 only) and Tmax = 150 (rows that do not start on 16 bytes) -- plus a lone (37,) batch
(odd Tmax) and a (150, 150) batch (328 columns: the 64-column GEMM kernel).

Bounds.  Against oracle.nnet3.forward: those the row-major output kernel is held to (test_gpu_ppg_batch.py /
test_gpu_tdnn.py): posteriors 2e-6 from features, 5e-5 from wavs, row sums within 1e-4 of 1, equal argmax.  Against
compute_full_ppg_batch's transposed output (same logits, the sum of exp in another order): 4e-6, the sum of the two oracle
bounds.  The monophone case promises bits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nnet3 as onnet3
from test_gpu_ppg_batch import FRAMES, _wave_data, world  # noqa: F401  (world: the module fixture, built once for this file)

pytestmark = pytest.mark.gpu

K = 5816
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def _padded_call(model, feats, Tmax=None, transform_t=None, M=0, fill=float("nan"), **override):
    """facppg_tdnn_forward_batch_padded through the C ABI over features [T_b, 40] (numpy) -> (rc, out [B, K or M, Tmax] pre-filled
    with ``fill``).  override: arguments replaced by the refusal cases (feats_dev / off_dev / off_host / out_dev / ws_dev: None =
    NULL; B, ws_bytes, handle)."""
    from facppg import lib as _lib
    from ppg import compute_ppg
    L = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = compute_ppg._tdnn_handle(model, dev, "test")
    frames = [int(f.shape[0]) for f in feats]
    flat = torch.from_numpy(np.concatenate(feats, 0)).to(dev).contiguous()
    off = _lib.host_offsets(frames)
    B = len(frames)
    Tmax = max(frames) if Tmax is None else Tmax
    off_dev = torch.tensor(list(off), dtype=torch.int32, device=dev)
    ws = torch.empty(L.facppg_tdnn_batch_workspace_bytes(h.handle, off, B), dtype=torch.uint8, device=dev)
    out = torch.full((B, max(M, 1) if transform_t is not None else K, max(Tmax, 1)), fill, device=dev)
    a = dict(handle=h.handle, feats_dev=flat, off_dev=off_dev, off_host=off, B=B, out_dev=out, ws_dev=ws, ws_bytes=ws.numel())
    a.update(override)
    rc = L.facppg_tdnn_forward_batch_padded(a["handle"], _lib.ptr(a["feats_dev"]), _lib.ptr(a["off_dev"]), a["off_host"], a["B"],
                                            _lib.ptr(transform_t), M, Tmax, _lib.ptr(a["out_dev"]), _lib.ptr(a["ws_dev"]), a["ws_bytes"],
                                            _lib.current_stream(dev))
    torch.cuda.synchronize()
    return rc, out


def _padded(model, feats, Tmax=None):
    rc, out = _padded_call(model, feats, Tmax)
    assert rc == 0, rc
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def extra(world):
    """The second utterance of the (150, 150) batch and its oracle answer."""
    g = np.random.Generator(np.random.PCG64(22))
    second = (2.0 * g.standard_normal((150, 40))).astype(np.float32)
    return dict(second=second, ref=onnet3.forward(world["model"], second))


def _check_padded(out, frames, refs, bound):
    """Valid frames against the oracle, the padding exactly zero, no NaN of the pre-fill left."""
    B, Tmax = len(frames), out.shape[2]
    assert out.shape == (B, K, Tmax) and not np.isnan(out).any()
    for b, (T, ref) in enumerate(zip(frames, refs)):
        got = out[b, :, :T].T
        err, row = np.abs(got - ref).max(), np.abs(got.sum(1) - 1.0).max()
        print("  T=%d of %s, Tmax=%d: posterior max err %.2e, row-sum err %.1e" % (T, tuple(frames), Tmax, err, row))
        assert err <= bound and row <= 1e-4
        assert np.array_equal(got.argmax(1), ref.argmax(1))
        assert not out[b, :, T:].any()                     # exactly 0.0f behind the utterance


def test_senone_posteriors_against_the_oracle(world, extra):
    """Test 1.  Measured on an MI355X (this test's print-out): against compute_full_ppg_batch's transposed output the largest
    deviation is 1.5e-8 at frames (1, 5, 37, 150), 1.0e-8 at (37,), 1.8e-8 at (150, 150) and 2.5e-8 from the wavs (bound 4e-6);
    against the oracle 1.5e-8 from features (bound 2e-6) and 1.2e-7 from wavs (bound 5e-5)."""
    import ppg
    model, deps, feats = world["model"], world["deps"], world["feats"]
    sets = {"(1, 5, 37, 150)": (feats, world["ref_post"]), "(37,)": ([feats[2]], [world["ref_post"][2]]),
            "(150, 150)": ([feats[3], extra["second"]], [world["ref_post"][3], extra["ref"]])}
    for name, (fs, refs) in sets.items():
        frames = [f.shape[0] for f in fs]
        out = _padded(model, fs)
        _check_padded(out, frames, refs, 2e-6)
        rows = ppg.compute_full_ppg_batch(model, [torch.from_numpy(f).cuda() for f in fs])
        dev = max(float(np.abs(out[b, :, :T].T - r.cpu().numpy()).max()) for b, (T, r) in enumerate(zip(frames, rows)))
        print("frames %s: padded vs compute_full_ppg_batch transposed: max deviation %.3e" % (name, dev))
        assert dev <= 4e-6
    # from wavs, through ppg.compute_ppg_padded
    wd = _wave_data(world["wavs"])
    x, lens = ppg.compute_ppg_padded(wd, deps)
    assert lens == list(FRAMES) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (4, K, 150)
    _check_padded(x.cpu().numpy(), FRAMES, world["ref_wav_post"], 5e-5)
    rows = ppg.compute_ppg_batch(wd, deps)
    dev = max(float((x[b, :, :T].t() - r).abs().max()) for b, (T, r) in enumerate(zip(FRAMES, rows)))
    print("wavs: padded vs compute_ppg_batch transposed: max deviation %.3e" % dev)
    assert dev <= 4e-6


def test_determinism_and_independence(world):
    """Test 2: the same bits twice; utterances 1 and 2 with other neighbours (one of them 1e4 times larger); the same frame
    under another Tmax."""
    model, feats, other = world["model"], world["feats"], world["other"]
    a, again = _padded(model, feats), _padded(model, feats)
    assert np.array_equal(a, again)
    b = _padded(model, [other[0], feats[1], feats[2], other[3] * np.float32(1e4)])
    for k in (1, 2):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a[3], b[3]) and np.isfinite(b).all()
    t37, t64 = _padded(model, [feats[2]], Tmax=37), _padded(model, [feats[2]], Tmax=64)
    assert t37.shape == (1, K, 37) and t64.shape == (1, K, 64)
    assert np.array_equal(t37[0], t64[0, :, :37]) and not t64[0, :, 37:].any()
    # (the same utterance alone and inside the batch of four: not bits -- the layers of a wider batch may run another k_gemm
    #  shape -- but both are within 2e-6 of the oracle)
    assert np.abs(t37[0] - a[2, :, :37]).max() <= 4e-6


def test_monophone_output_is_the_reduced_batch_call(world):
    """Test 3: bits of compute_ppg_batch(..., is_full_ppg=False), transposed and zero-padded."""
    import ppg
    deps = world["deps"]
    wd, od = _wave_data(world["wavs"]), _wave_data(world["other_wavs"])
    for name, wavs in (("(1, 5, 37, 150)", wd), ("(37,)", [wd[2]]), ("(150, 150)", [wd[3], od[3]])):
        x, lens = ppg.compute_ppg_padded(wavs, deps, is_full_ppg=False)
        rows = ppg.compute_ppg_batch(wavs, deps, is_full_ppg=False)
        assert lens == [int(r.shape[0]) for r in rows] and tuple(x.shape) == (len(wavs), 40, max(lens)) and x.is_contiguous()
        want = torch.zeros_like(x)
        for b, r in enumerate(rows):
            want[b, :, :lens[b]] = r.t()
        assert torch.equal(x, want), name
    # through the C ABI over a NaN pre-fill: the padding is written by the call
    red_t = torch.as_tensor(deps.monophone_trans).cuda().float().t().contiguous()
    rc, out = _padded_call(world["model"], world["feats"], Tmax=151, transform_t=red_t, M=40)
    assert rc == 0 and not bool(torch.isnan(out).any())
    for b, T in enumerate(FRAMES):
        assert not bool(out[b, :, T:].any())
        assert float((out[b, :, :T].sum(0) - 1).abs().max()) <= 1e-4


def test_the_call_does_not_wait_for_the_device(world):
    """compute_ppg_padded behind 40 M cycles of spinning on its stream (some tens of milliseconds): once warm, it returns with
    the spin still running -- no copy back to the host and no synchronisation is inside it -- for both kinds of PPG."""
    import ppg
    deps = world["deps"]
    wd = _wave_data(world["wavs"])
    for full in (True, False):
        ppg.compute_ppg_padded(wd, deps, is_full_ppg=full)            # (the first call packs the model and uploads the tables)
        torch.cuda.synchronize()
        torch.cuda._sleep(40_000_000)
        spun = torch.cuda.Event()
        spun.record()
        x, lens = ppg.compute_ppg_padded(wd, deps, is_full_ppg=full)
        still_spinning = not spun.query()
        torch.cuda.synchronize()
        assert still_spinning, "is_full_ppg=%s: the call waited for the device" % full
        assert lens == list(FRAMES) and bool(torch.isfinite(x).all())


def test_refusals(world):
    """Test 4: every refusal returns its code, names itself in facppg_last_error, and leaves the output untouched."""
    from facppg import lib as _lib
    L = _lib.load()
    model, f37 = world["model"], [world["feats"][2]]
    red_t = torch.as_tensor(world["deps"].monophone_trans).cuda().float().t().contiguous()
    cases = [
        ("not a softmax", EUNSUPPORTED, "softmax", dict(model=world["model_log"])),
        ("Tmax short", EINVAL, "Tmax", dict(Tmax=36)),
        ("B = 0", EINVAL, "B must be at least 1", dict(B=0)),
        ("B < 0", EINVAL, "B must be at least 1", dict(B=-1)),
        ("M = 0", EINVAL, "bad M", dict(transform_t=red_t, M=0)),
        ("M = 65", EINVAL, "bad M", dict(transform_t=red_t, M=65)),
        ("NULL handle", EINVAL, "NULL", dict(handle=ctypes.c_void_p(0))),
        ("NULL feats", EINVAL, "NULL", dict(feats_dev=None)),
        ("NULL device offsets", EINVAL, "NULL", dict(off_dev=None)),
        ("NULL host offsets", EINVAL, "NULL", dict(off_host=None)),
        ("NULL out", EINVAL, "NULL", dict(out_dev=None)),
        ("NULL workspace", EINVAL, "NULL", dict(ws_dev=None)),
        ("short workspace", EWORKSPACE, "workspace", dict(ws_bytes=1024)),
    ]
    for name, code, word, kw in cases:
        kw = dict(kw)
        m = kw.pop("model", model)
        rc, out = _padded_call(m, f37, **kw)
        msg = L.facppg_last_error().decode()
        print("%s: rc %d, %s" % (name, rc, msg))
        assert rc == code, name
        assert word in msg, (name, msg)
        assert bool(torch.isnan(out).all()), name            # nothing was launched
    # the Python surface: no model, no monophone map (compute_ppg_batch's messages), a log-softmax model
    import ppg

    class Deps(object):
        pass
    d = Deps()
    d.nnet, d.lda, d.monophone_trans = None, world["deps"].lda, None
    wd = _wave_data(world["wavs"])[2:3]
    with pytest.raises(_lib.FacppgError, match="no acoustic model"):
        ppg.compute_ppg_padded(wd, d)
    d.nnet = model
    with pytest.raises(_lib.FacppgError, match="monophone PPGs need the pdf -> monophone matrix"):
        ppg.compute_ppg_padded(wd, d, is_full_ppg=False)
    d.nnet = world["model_log"]
    with pytest.raises(_lib.FacppgError, match="softmax"):
        ppg.compute_ppg_padded(wd, d)
