"""GPU: STFT.griffin_lim / STFT.mel_to_magnitude (facppg_griffin_lim, facppg_mel_to_magnitude) against the float64 restatement of
tests/griffin_lim_helpers.py.  Every tolerance is computed from the float32 and float64 restatements, never from the device.

The shape set's smallest shape (64, 16, 3) has hop * (F - 1) = filter_length / 2 exactly, which the Python layer refuses when the
lengths are on the host (reflect padding proper needs more); its cases pass their lengths as device tensors, which are trusted,
and take the C entry point's documented clamped reflection -- the helper's frames() restates it.  The drawn phases are read
through the seed kernel's debug path (STFT.draw_phase, facppg_griffin_lim_draw_phase)."""
import ctypes

import numpy as np
import pytest
import torch

import griffin_lim_helpers as glh

pytestmark = pytest.mark.gpu


def _stft(fl, hop, mel_basis=None):
    from common.stft import STFT
    return STFT(fl, hop, fl, mel_basis=mel_basis).cuda()


def _batch(fl, hop, F):
    """The three seeds of a shape as one batch: M, phi0 [3, cutoff, F] on the device."""
    cs = [glh.case(fl, hop, F, s) for s in glh.SEEDS]
    M = torch.from_numpy(np.stack([c[1] for c in cs]).astype(np.float32)).cuda()
    phi = torch.from_numpy(np.stack([c[2] for c in cs]).astype(np.float32)).cuda()
    return M, phi


def _dev_lengths(F, B):
    return torch.full((B,), F, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def tol():
    t = glh.steps_tolerance()
    print("steps tolerance %.3e" % t)
    assert 1e-6 < t < 1e-3
    return t


@pytest.mark.parametrize("fl,hop,F", glh.SHAPES)
def test_steps_against_float64(fl, hop, F, tol):
    """n_iters in {0, 1, 2}, alpha in {0, 0.99}, given phi0: max |device - float64| over the utterance's RMS within the tolerance
    (4 x the float32 restatement's worst deviation over the same cases); sc within the same tolerance.
    Measured on an MI355X: the device's worst is 5.4e-5 (at (1024, 256, 9); 2.3e-6 to 7.0e-6 on the other shapes) under a tolerance
    of 5.09e-4, sc within 5.6e-8; the README row carries the same figures."""
    stft = _stft(fl, hop)
    M, phi = _batch(fl, hop, F)
    worst = worst_sc = 0.0
    for n in glh.STEP_ITERS:
        for alpha in glh.ALPHAS:
            out, sc = stft.griffin_lim(M, n_iters=n, momentum=alpha, lengths=_dev_lengths(F, 3), init_phase=phi, return_convergence=True)
            assert out.shape == (3, 1, hop * (F - 1)) and sc.shape == (3,)
            out, sc = out.cpu().numpy(), sc.cpu().numpy()
            for b, seed in enumerate(glh.SEEDS):
                ref, sc_ref = glh.step_reference(fl, hop, F, seed, n, alpha)
                worst = max(worst, glh.rel_err(out[b, 0], ref))
                worst_sc = max(worst_sc, abs(float(sc[b]) - sc_ref))
    print("shape", (fl, hop, F), "device worst %.3e, sc worst %.3e, tolerance %.3e" % (worst, worst_sc, tol))
    assert worst <= tol and worst_sc <= tol


def _depth_margin():
    """10 x the largest gap between the float32 and float64 restatements' sc (returned, and of the output signal) at 32
    iterations over the depth cases."""
    gap = 0.0
    for fl, hop, F in DEPTH_SHAPES:
        _, M, phi0, _ = glh.case(fl, hop, F, 0)
        for alpha in glh.ALPHAS:
            y64, s64 = glh.griffin_lim(fl, hop, M, phi0, 32, alpha, np.float64)
            y32, s32 = glh.griffin_lim(fl, hop, M, phi0, 32, alpha, np.float32)
            gap = max(gap, abs(s32 - s64), abs(glh.signal_convergence(fl, hop, M, y32) - glh.signal_convergence(fl, hop, M, y64)))
    return 10.0 * gap


DEPTH_SHAPES = ((64, 16, 40), (64, 32, 5), (1024, 160, 20))


def test_depth(tol):
    """32 iterations, both alphas: samples are not compared (float32 and float64 runs drift apart).  Instead
    (1) the device's returned sc, and the float64 sc of the device's output signal, agree with the float64 run's (its returned sc,
        resp. the sc of its output signal) within 10 x the largest float32-to-float64 gap of the restatements;
    (2) the device's sc is strictly decreasing over 0, 4 and 32 iterations;
    (3) the device's sc at 32 equals the host float64 sc of t_32 within the steps tolerance, t_32 being the float64 transform of
        the device's own 31-iteration output (out = ISTFT(c_31), t_32 = STFT of it)."""
    margin = _depth_margin()
    print("depth margin %.3e" % margin)
    assert margin < 0.05
    for fl, hop, F in DEPTH_SHAPES:
        stft = _stft(fl, hop)
        _, M, phi0, _ = glh.case(fl, hop, F, 0)
        Md = torch.from_numpy(M.astype(np.float32)[None]).cuda()
        pd = torch.from_numpy(phi0.astype(np.float32)[None]).cuda()
        M32 = M.astype(np.float32).astype(np.float64)
        for alpha in glh.ALPHAS:
            run = {n: stft.griffin_lim(Md, n_iters=n, momentum=alpha, init_phase=pd, return_convergence=True) for n in (0, 4, 31, 32)}
            sc = {n: float(v[1][0]) for n, v in run.items()}
            y64, s64 = glh.griffin_lim(fl, hop, M, phi0, 32, alpha, np.float64)
            out32 = run[32][0][0, 0].cpu().numpy()
            s_out_dev, s_out_64 = glh.signal_convergence(fl, hop, M, out32), glh.signal_convergence(fl, hop, M, y64)
            t32 = glh.signal_convergence(fl, hop, M32, run[31][0][0, 0].cpu().numpy())
            print((fl, hop, F), alpha, "sc dev %.5f f64 %.5f | of output dev %.5f f64 %.5f | of t_32 %.6f" % (sc[32], s64, s_out_dev, s_out_64, t32))
            assert abs(sc[32] - s64) <= margin and abs(s_out_dev - s_out_64) <= margin
            assert sc[0] == 1.0 and sc[0] > sc[4] > sc[32]
            assert abs(sc[32] - t32) <= tol


def test_against_the_existing_loop(tol):
    """audio_processing.griffin_lim under np.random.seed, its angles recovered by re-seeding and passed as init_phase, agrees
    with STFT.griffin_lim(alpha = 0, n_iters = 3) within the steps tolerance."""
    from common.audio_processing import griffin_lim
    fl, hop, F = 1024, 256, 9
    stft = _stft(fl, hop)
    M, _ = _batch(fl, hop, F)
    np.random.seed(77)
    loop = griffin_lim(M, stft, n_iters=3)
    np.random.seed(77)
    angles = np.angle(np.exp(2j * np.pi * np.random.rand(*M.size()))).astype(np.float32)
    out = stft.griffin_lim(M, n_iters=3, momentum=0.0, init_phase=torch.from_numpy(angles).cuda())
    for b in range(3):
        err = glh.rel_err(out[b, 0].cpu().numpy(), loop[b].cpu().numpy())
        print("loop vs device loop, utterance %d: %.3e" % (b, err))
        assert err <= tol


@pytest.mark.parametrize("fl,hop,Fb", glh.RAGGED)
def test_ragged_batches(fl, hop, Fb):
    """Utterance b of a ragged batch under utterance_seeds equals its own batch-1 call bit for bit, samples and sc (with drawn
    phases and with given ones); everything behind hop * (F_b - 1) is exactly zero."""
    stft = _stft(fl, hop)
    F, B = max(Fb), len(Fb)
    cutoff = fl // 2 + 1
    M = torch.full((B, cutoff, F), 7.0, device="cuda")             # (whatever lies behind an utterance's frames does not matter)
    for b, f in enumerate(Fb):
        M[b, :, :f] = torch.from_numpy(glh.case(fl, hop, f, 1)[1].astype(np.float32)).cuda()
    lens = torch.tensor(Fb, dtype=torch.int32, device="cuda")
    seeds = [11, 2 ** 63 + 5, 13]
    for n, alpha in ((0, 0.0), (3, 0.0), (5, 0.99)):
        out, sc = stft.griffin_lim(M, n_iters=n, momentum=alpha, lengths=lens, utterance_seeds=seeds, return_convergence=True)
        assert out.shape == (B, 1, hop * (F - 1)) and bool(torch.isfinite(out).all())
        for b, f in enumerate(Fb):
            one, sc1 = stft.griffin_lim(M[b:b + 1, :, :f].contiguous(), n_iters=n, momentum=alpha, lengths=lens[b:b + 1],
                                        utterance_seeds=seeds[b:b + 1], return_convergence=True)
            nb = hop * (f - 1)
            assert torch.equal(out[b, 0, :nb], one[0, 0]) and torch.equal(sc[b], sc1[0]), (n, alpha, b)
            assert bool(out[b, 0, :nb].any()) and not bool(out[b, 0, nb:].any())
        # the drawn phases as init_phase: the same call
        phi = stft.draw_phase(seeds, F, "cuda")
        again, sc2 = stft.griffin_lim(M, n_iters=n, momentum=alpha, lengths=lens, init_phase=phi, return_convergence=True)
        assert torch.equal(again, out) and torch.equal(sc2, sc)


def test_drawn_phases():
    """Same seed, same result; different seeds differ; the phases (read through the seed kernel's debug path, STFT.draw_phase) lie
    in [-pi, pi) and are uniform: the mean resultant length over 513 x 40 bins is below 4 / sqrt(n)."""
    stft = _stft(1024, 256)
    _, M, _, _ = glh.case(1024, 256, 9, 0)
    Md = torch.from_numpy(M.astype(np.float32)[None]).cuda()
    a = stft.griffin_lim(Md, n_iters=2, seed=5)
    assert torch.equal(a, stft.griffin_lim(Md, n_iters=2, seed=5))
    assert not torch.equal(a, stft.griffin_lim(Md, n_iters=2, seed=6))
    assert torch.equal(a, stft.griffin_lim(Md, n_iters=2, utterance_seeds=stft.derive_seeds(5, 1)))
    phi = stft.draw_phase([123, 124], 40, "cuda").cpu().numpy().astype(np.float64)
    assert phi.shape == (2, 513, 40)
    assert phi.min() >= -np.pi and phi.max() < np.pi
    assert not np.array_equal(phi[0], phi[1])
    # utterance b's phases depend on its seed alone, not on the batch or the padded length
    assert np.array_equal(stft.draw_phase([124], 17, "cuda").cpu().numpy()[0], phi[1][:, :17].astype(np.float32))
    for b in range(2):
        n = phi[b].size
        r = abs(np.mean(np.exp(1j * phi[b])))
        print("mean resultant length %.2e (bound %.2e)" % (r, 4 / np.sqrt(n)))
        assert r < 4 / np.sqrt(n)
        assert abs(np.mean(phi[b] < 0) - 0.5) < 4 * 0.5 / np.sqrt(n)


def _mel_bases():
    from common.layers import slaney_mel_basis
    return {(80, 513): slaney_mel_basis(16000, 1024, 80, 0.0, 8000.0).astype(np.float32), (20, 33): glh.triangular_basis(20, 33).astype(np.float32)}


@pytest.mark.parametrize("n_mel,cutoff,F", [(80, 513, 1), (80, 513, 37), (20, 33, 5)])
def test_mel_to_magnitude(n_mel, cutoff, F):
    """Against float64 with the tolerance 4 x the float32 restatement's deviation (relative to the largest magnitude); the inputs
    include bins that clamp.  Rows at and behind F_b are zero and an utterance equals its batch-1 call."""
    basis = _mel_bases()[(n_mel, cutoff)]
    fl = 2 * (cutoff - 1)
    stft = _stft(fl, fl // 4, mel_basis=basis)
    P = glh.mel_pinv(basis)
    mels = np.stack([glh.mel_case(basis, F, s) for s in range(3)])
    out = stft.mel_to_magnitude(torch.from_numpy(mels).cuda())
    assert out.shape == (3, cutoff, F)
    bar = dev = 0.0
    for b in range(3):
        ref = glh.mel_to_magnitude(P, mels[b], np.float64)
        f32 = glh.mel_to_magnitude(P, mels[b], np.float32)
        assert 0.0 < np.mean(ref == 0.0) < 0.5
        bar = max(bar, 4.0 * np.max(np.abs(f32 - ref)) / ref.max())
        dev = max(dev, np.max(np.abs(out[b].cpu().numpy() - ref)) / ref.max())
    print("mel_to_magnitude", (n_mel, cutoff, F), "device %.3e, bar %.3e" % (dev, bar))
    assert dev <= bar
    if F > 2:
        Fb = [F, 2, F - 1]
        rag = stft.mel_to_magnitude(torch.from_numpy(mels).cuda(), lengths=Fb)
        for b, f in enumerate(Fb):
            assert torch.equal(rag[b, :, :f], stft.mel_to_magnitude(torch.from_numpy(mels[b:b + 1, :, :f].copy()).cuda())[0])
            assert torch.equal(rag[b, :, :f], out[b, :, :f]) and not bool(rag[b, :, f:].any())


def test_tacotron_stft_griffin_lim_is_the_two_steps():
    from common.layers import TacotronSTFT
    t = TacotronSTFT(1024, 160, 1024, 80, 16000, 0.0, 8000.0).cuda()
    basis = t.mel_basis.cpu().numpy()
    mel = torch.from_numpy(np.stack([glh.mel_case(basis, 30, s) for s in range(2)])).cuda()
    lens = [30, 12]
    mag = t.mel_to_magnitude(mel, lens)
    a = t.griffin_lim(mel, lengths=lens, n_iters=4, momentum=0.99, utterance_seeds=[3, 4])
    assert torch.equal(a, t.stft_fn.griffin_lim(mag, n_iters=4, momentum=0.99, lengths=lens, utterance_seeds=[3, 4]))
    assert a.shape == (2, 1, 160 * 29) and bool(torch.isfinite(a).all()) and not bool(a[1, 0, 160 * 11:].any())


def test_refusals_leave_the_stream_usable():
    from common.stft import STFT
    from facppg import lib as flib
    from facppg.lib import FacppgError
    fl, hop, F = 64, 16, 12
    basis = glh.triangular_basis(20, 33).astype(np.float32)
    stft = _stft(fl, hop, mel_basis=basis)
    M, phi = _batch(fl, hop, F)
    good = stft.griffin_lim(M, n_iters=2, init_phase=phi)
    mel = torch.from_numpy(glh.mel_case(basis, F, 0)[None]).cuda()
    good_mag = stft.mel_to_magnitude(mel)

    def still_fine():
        assert torch.equal(stft.griffin_lim(M, n_iters=2, init_phase=phi), good)
        assert torch.equal(stft.mel_to_magnitude(mel), good_mag)
    with pytest.raises(FacppgError, match="alpha"):
        stft.griffin_lim(M, n_iters=2, momentum=1.0, init_phase=phi)
    still_fine()
    with pytest.raises(FacppgError, match="n_iters"):
        stft.griffin_lim(M, n_iters=-1, init_phase=phi)
    still_fine()
    with pytest.raises(FacppgError, match="at least 2 frames"):
        stft.griffin_lim(M[:, :, :1].contiguous(), n_iters=2, init_phase=phi[:, :, :1].contiguous(), lengths=_dev_lengths(1, 3))
    still_fine()
    for kw in (dict(seed=1), dict(utterance_seeds=[1, 2, 3])):
        with pytest.raises(FacppgError, match="init_phase"):
            stft.griffin_lim(M, n_iters=2, init_phase=phi, **kw)
    with pytest.raises(FacppgError, match="seed and utterance_seeds"):
        stft.griffin_lim(M, n_iters=2, seed=1, utterance_seeds=[1, 2, 3])
    with pytest.raises(FacppgError, match="reflect padding"):
        stft.griffin_lim(M, n_iters=2, init_phase=phi, lengths=[12, 3, 12])       # host lengths: 16 * 2 = 32 samples <= 32
    still_fine()
    # a handle without a mel basis
    plain = _stft(fl, hop)
    with pytest.raises(FacppgError, match="without a mel basis"):
        plain.mel_to_magnitude(mel)
    L = flib.load()
    h = plain._handle(torch.device("cuda", torch.cuda.current_device()))
    table = torch.zeros(33, 20, device="cuda")
    st = flib.current_stream(torch.device("cuda"))
    assert L.facppg_stft_set_mel_pinv(h, flib.ptr(table), st) != 0 and b"without a mel basis" in L.facppg_last_error()
    # a short workspace, at the C entry points
    h = stft._handle(torch.device("cuda", torch.cuda.current_device()))
    need = L.facppg_griffin_lim_workspace_bytes(h, 3, F)
    assert need > 0 and L.facppg_griffin_lim_workspace_bytes(h, 3, 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(3, hop * (F - 1), device="cuda")
    args = (h, flib.ptr(M), ctypes.c_void_p(0), flib.ptr(phi), ctypes.c_void_p(0), 2, 0.0, 3, F, flib.ptr(out), ctypes.c_void_p(0), flib.ptr(ws))
    assert L.facppg_griffin_lim(*args, need - 1, st) != 0 and b"workspace" in L.facppg_last_error()
    assert L.facppg_griffin_lim(*args, need, st) == 0
    assert torch.equal(out, good[:, 0])
    assert L.facppg_griffin_lim(h, flib.ptr(M), ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0), 2, 0.0, 3, F, flib.ptr(out),
                                ctypes.c_void_p(0), flib.ptr(ws), need, st) != 0            # neither phases nor seeds
    mag = torch.empty(1, 33, F, device="cuda")
    assert L.facppg_mel_to_magnitude(h, flib.ptr(mel), ctypes.c_void_p(0), 1, F, flib.ptr(mag), flib.ptr(ws), 20 * F * 4 - 1, st) != 0
    assert b"workspace" in L.facppg_last_error()
    still_fine()
