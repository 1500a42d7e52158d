"""GPU: the F0 tracker (csrc/facppg_f0.hip, ppg.compute_f0) and the log-F0 input rows (hparams.is_append_f0) through every layer.

  NCCF       against the float64 definition (f0_helpers.nccf), every sample count alone and all in one batch -- the batch rows equal
             the single calls bit for bit --, within 4 x the float32 restatement's own deviation over the same signals
  tracker    over the DEVICE's matrix: the lags equal the float32 restatement's integers, F0 within 4 fp32 ulp (the division may
             round differently); crafted matrices handed to facppg_f0_track_batch (T = 1, no peak, two equal peaks, a peak at
             lag_min and one at lag_max, a weak frame too short for voicing_cost to switch)
  end to end five steady tones within 0.5 % on interior frames, all voiced; silence and DC 30 all unvoiced
  padded     ppg.compute_ppg_padded(append_f0=True): rows [:K] bits of the plain call, rows [K:] within 1.5e-5 of the host
             append_ppg over compute_f0_batch (4 fp32 ulp at |-36.04|: one float32 rounding of the float64 result plus the device
             logf), exactly 0 behind T_b
  wav in, wav out, long recordings and the loader at n_symbols = 43
Acoustic model and wavs are test_gpu_ppg_batch.py's (imported, not edited)."""
import numpy as np
import pytest
import torch
from scipy.io import wavfile

import f0_helpers as fh
from test_gpu_ppg_batch import FRAMES, _wave_data, world  # noqa: F401  (world: the module fixture, built once for this file)
from test_gpu_wav2wav import SEEDS, _cotenancy, _host_rows

pytestmark = pytest.mark.gpu

K_SENONE, K_MONO = 5816, 40
NS = fh.L + 2


def _wd(x, fs=16000):
    from common import feat
    return feat.read_wav_kaldi_internal(np.asarray(x, dtype=np.float32), fs)


@pytest.fixture(scope="module")
def device_nccf():
    """The device's matrix of every case, alone and in one batch (host copies), computed once."""
    import ppg
    cases = fh.nccf_cases()
    alone = [ppg.compute_nccf_batch([_wd(x)])[0].cpu().numpy() for x in cases]
    batch = [p.cpu().numpy() for p in ppg.compute_nccf_batch([_wd(x) for x in cases])]
    return alone, batch


def _track_abi(phis, **options):
    """facppg_f0_track_batch over host matrices [T_b, L + 2] -> (lags, f0s) per utterance."""
    from facppg import lib as _lib
    from ppg import F0Options
    Lb = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    opt = F0Options(**options)
    frames = [int(p.shape[0]) for p in phis]
    off = _lib.host_offsets(frames)
    total = off[len(frames)]
    flat = torch.from_numpy(np.ascontiguousarray(np.concatenate(phis, 0), dtype=np.float32)).to(dev)
    assert flat.shape == (total, opt.num_lags + 2)
    off_dev = torch.tensor(list(off), dtype=torch.int32, device=dev)
    tables = torch.from_numpy(opt.tables()).to(dev).contiguous()
    ws = torch.empty(Lb.facppg_f0_workspace_bytes(opt.config(), total), dtype=torch.uint8, device=dev)
    lag = torch.full((total,), -7, dtype=torch.int32, device=dev)
    f0 = torch.full((total,), float("nan"), device=dev)
    _lib.check(Lb.facppg_f0_track_batch(opt.config(), _lib.ptr(flat), _lib.ptr(off_dev), off, len(frames), _lib.ptr(tables), _lib.ptr(lag),
                                        _lib.ptr(f0), _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)))
    torch.cuda.synchronize()
    lag, f0 = lag.cpu().numpy(), f0.cpu().numpy()
    return [lag[off[b]:off[b + 1]] for b in range(len(frames))], [f0[off[b]:off[b + 1]] for b in range(len(frames))]


def _check_track(phis, lags, f0s, tag):
    """Device (lags, f0s) over ``phis`` against the float32 restatement: integers exact, Hz within 4 ulp."""
    for b, (p, lag, f0) in enumerate(zip(phis, lags, f0s)):
        want_lag, want_f0 = fh.track(p, np.float32)
        assert np.array_equal(lag, want_lag), (tag, b, lag, want_lag)
        assert not f0[lag == 0].any() and np.isfinite(f0).all()
        ulp = int(fh.ulp_distance(f0, want_f0).max()) if len(f0) else 0
        print("  %s[%d]: %d frames, %d voiced, F0 within %d ulp" % (tag, b, len(lag), int((lag > 0).sum()), ulp))
        assert ulp <= 4, (tag, b, ulp)


def test_nccf_against_float64(device_nccf):
    """Measured on an MI355X (this test's print-out): worst deviation 2.54e-7 (the 4801-sample case); the float32 restatement's own
    is 2.43e-7, the tolerance 9.73e-7."""
    alone, batch = device_nccf
    tol = fh.nccf_tolerance()
    worst = 0.0
    for x, (p64, _), a, b in zip(fh.nccf_cases(), fh.nccf_references(), alone, batch):
        assert a.shape == b.shape == p64.shape == (fh.num_frames(len(x)), NS) and a.dtype == np.float32
        assert np.array_equal(a, b), len(x)                    # the batch row is the single call's, bit for bit
        err = float(np.abs(a.astype(np.float64) - p64).max())
        worst = max(worst, err)
        print("  n=%d (%d frames): max |phi - phi64| = %.3e (tolerance %.3e)" % (len(x), a.shape[0], err, tol))
        assert np.isfinite(a).all() and err <= tol, (len(x), err, tol)
    print("NCCF worst deviation %.3e, float32 restatement %.3e" % (worst, fh.emulation_deviation()))


def test_tracker_is_exact_on_the_device_matrix(device_nccf):
    import ppg
    _, batch = device_nccf
    lags, f0s = _track_abi(batch)
    _check_track(batch, lags, f0s, "cases")
    one_lags, one_f0s = _track_abi(batch[-1:])
    assert np.array_equal(one_lags[0], lags[-1]) and np.array_equal(one_f0s[0], f0s[-1])
    assert any((l > 0).any() for l in lags) and any((l == 0).all() for l in lags)
    # compute_f0_batch is the two kernels back to back: the same bits
    got = ppg.compute_f0_batch([_wd(x) for x in fh.nccf_cases()])
    for g, f in zip(got, f0s):
        assert g.is_cuda and g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), f)
    assert np.array_equal(ppg.compute_f0(_wd(fh.nccf_cases()[3])).cpu().numpy(), f0s[3])


def _row(peaks, base=0.0):
    r = np.full(NS, base, np.float32)
    for col, v in peaks.items():
        r[col] = v
    return r


def _equal_cost_peaks(a, b, va=0.8):
    """Values at columns a < b whose voiced costs 1 - phi * wl are the same float32."""
    wl, _ = fh.tables()
    target = np.float32(va) * wl[a - 1]
    vb = np.float32(target / wl[b - 1])
    for _ in range(64):
        prod = vb * wl[b - 1]
        if prod == target:
            return np.float32(va), vb
        vb = np.nextafter(vb, np.float32(2.0 if prod < target else -2.0))
    raise AssertionError("no float32 value gives the same product")


def test_tracker_on_crafted_matrices():
    wl, _ = fh.tables()
    # T = 1: a single peak at lag 89 (column 50) wins over unvoiced (1 - 0.9 wl < 0.9)
    single = np.stack([_row({50: 0.9})])
    # constant rows: q > r never holds, no peak, all unvoiced
    const = np.full((6, NS), 0.5, np.float32)
    # two peaks of equal cost in one frame, then the same frame again: the lower state wins both at the end and as predecessor
    va, vb = _equal_cost_peaks(60, 200)
    tie = _row({60: va, 200: vb})
    assert np.float32(1) - va * wl[59] == np.float32(1) - vb * wl[199]
    ties = [np.stack([tie]), np.stack([tie, tie, tie])]
    # a peak at lag_min (column 1) and one at lag_max (column L): the refinement reads the guard columns 0 and L + 1
    lo = np.stack([_row({0: 0.7, 1: 0.9, 2: 0.3})] * 3)
    hi = np.stack([_row({fh.L - 1: 0.2, fh.L: 0.95, fh.L + 1: 0.6})] * 3)
    # voiced, one weak frame, voiced: the switch costs 2 x 0.2 and does not pay; five weaker frames do
    strong, weak, weaker = _row({61: 0.95}), _row({61: 0.45}), _row({61: 0.1})
    short_gap = np.stack([strong] * 5 + [weak] + [strong] * 5)
    long_gap = np.stack([strong] * 5 + [weaker] * 5 + [strong] * 5)
    phis = [single, const] + ties + [lo, hi, short_gap, long_gap]
    lags, f0s = _track_abi(phis)
    _check_track(phis, lags, f0s, "crafted")
    assert list(lags[0]) == [89] and fh.ulp_distance(f0s[0][:1], np.float32(16000.0) / np.float32(89.0))[0] <= 4
    assert not lags[1].any() and not f0s[1].any()
    assert list(lags[2]) == [fh.LAG_MIN + 59] and list(lags[3]) == [fh.LAG_MIN + 59] * 3
    assert list(lags[4]) == [fh.LAG_MIN] * 3 and list(lags[5]) == [fh.LAG_MAX] * 3
    assert abs(float(f0s[4][0]) - 16000.0 / 39.75) < 1e-2 and f0s[4][0] != np.float32(400.0)        # delta = 0.5 (0.7 - 0.3) / -0.8
    den = (0.2 - 1.9) + 0.6
    assert abs(float(f0s[5][0]) - 16000.0 / (334 + 0.5 * (0.2 - 0.6) / den)) < 1e-2 and f0s[5][0] != np.float32(16000.0) / np.float32(334.0)
    assert list(lags[6]) == [100] * 11
    assert list(lags[7]) == [100] * 5 + [0] * 5 + [100] * 5
    # each alone: the same integers and bits as in the batch
    for k in (3, 7):
        l1, f1 = _track_abi([phis[k]])
        assert np.array_equal(l1[0], lags[k]) and np.array_equal(f1[0], f0s[k])


def test_end_to_end_tones_and_silence():
    import ppg
    signals = [fh.tone(f, 8000, seed=int(f)) for f in fh.TONES] + [fh.silence(3200), fh.dc_silence(3200), fh.silence(80)]
    got = [g.cpu().numpy() for g in ppg.compute_f0_batch([_wd(x) for x in signals])]
    for f, f0 in zip(fh.TONES, got):
        inner = f0[4:-4]
        rel = float(np.abs(inner - f).max() / f)
        print("  tone %5.1f Hz: %d frames, worst relative error %.2e on the interior" % (f, len(f0), rel))
        assert len(f0) == 50 and (inner > 0).all() and rel <= 5e-3, (f, rel)
    for f0, n in zip(got[5:], (20, 20, 1)):
        assert f0.shape == (n,) and not f0.any()
    # a 44.1 kHz input is downsampled as the PPG front end downsamples it: one value per PPG frame
    t = np.arange(44100) / 44100.0
    x = np.round(3000.0 * sum(np.sin(2 * np.pi * 150.0 * k * t) / k for k in range(1, 6)))
    f0 = ppg.compute_f0(_wd(x, 44100)).cpu().numpy()
    assert f0.shape == (100,) and (f0[4:-4] > 0).all() and float(np.abs(f0[4:-4] - 150.0).max()) <= 0.75


def _lf0_host(f0):
    from common.data_utils import append_ppg
    return append_ppg(np.zeros((len(f0), 0)), f0)             # [T, 3] float64


@pytest.mark.parametrize("is_full", [True, False], ids=["senone", "monophone"])
def test_padded_batch_with_f0_rows(world, is_full):
    import ppg
    deps = world["deps"]
    wd = _wave_data(world["wavs"])
    K = K_SENONE if is_full else K_MONO
    plain, lens = ppg.compute_ppg_padded(wd, deps, is_full_ppg=is_full)
    x, lens_f0 = ppg.compute_ppg_padded(wd, deps, is_full_ppg=is_full, append_f0=True)
    assert lens == lens_f0 == list(FRAMES) and tuple(x.shape) == (4, K + 3, 150) and x.is_contiguous() and x.dtype == torch.float32
    assert torch.equal(x[:, :K], plain)                      # bit for bit today's posteriors
    f0s = ppg.compute_f0_batch(wd)
    xh = x.cpu().numpy()
    worst = 0.0
    for b, T in enumerate(FRAMES):
        f0 = f0s[b].cpu().numpy()
        assert f0.shape == (T,)
        err = float(np.abs(xh[b, K:, :T].T.astype(np.float64) - _lf0_host(f0)).max())
        worst = max(worst, err)
        assert err <= 1.5e-5, (b, err)
        assert not xh[b, :, T:].any()                          # exactly 0 behind T_b, the three new rows included
    voiced = sum(int((f.cpu().numpy() > 0).sum()) for f in f0s)
    print("  %s: lf0 rows within %.2e of the host append_ppg (bound 1.5e-5); %d of %d frames voiced" % ("senone" if is_full else "monophone", worst,
                                                                                                          voiced, sum(FRAMES)))
    assert 0 < voiced
    # a lone utterance, odd Tmax
    x1, _ = ppg.compute_ppg_padded(wd[2:3], deps, is_full_ppg=is_full, append_f0=True)
    assert tuple(x1.shape) == (1, K + 3, 37) and torch.equal(x1[0, K:], x[2, K:, :37])


@pytest.fixture(scope="module")
def mono43(world):
    """The monophone + F0 (n_symbols = 43) pair of synthetic checkpoints and their Synthesizer."""
    from common.hparams import create_hparams_stage
    from facppg import synth
    from facppg.pipeline import Synthesizer
    from waveglow.glow import WaveGlow
    from test_gpu_e2e import weightnorm_state_dict
    tmp = world["tmp"]
    cfg = dict(synth.WAVEGLOW_CONFIG)
    wg = WaveGlow(**cfg)
    wg.load_state_dict(weightnorm_state_dict(synth.waveglow_state_dict(cfg)), strict=True)
    torch.save({"model": wg, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, tmp / "f0_waveglow.pt")
    hp = create_hparams_stage(n_symbols=43, is_full_ppg=False, is_append_f0=True, max_decoder_steps=150)
    torch.save({"state_dict": synth.tacotron_state_dict(hp, gate_bias=-10.0), "iteration": 0}, tmp / "f0_tacotron.pt")
    return dict(hp=hp, synthesizer=Synthesizer(str(tmp / "f0_tacotron.pt"), str(tmp / "f0_waveglow.pt"), hparams=hp))


def test_wavs_through_a_model_with_f0_inputs(world, mono43, monkeypatch):
    import ppg
    from facppg import pipeline
    from facppg.lib import FacppgError
    _cotenancy(monkeypatch)
    s, deps = mono43["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])
    kw = dict(utterance_seeds=SEEDS, step_limits=list(FRAMES))
    x, lens = ppg.compute_ppg_padded(wd, deps, is_full_ppg=False, append_f0=True)
    ref, tout_ref = pipeline.synthesize(_host_rows(x, lens), s.tacotron, s.waveglow, s.denoiser, **kw)
    out, tout = pipeline.synthesize_wavs(wd, deps, s.tacotron, s.waveglow, s.denoiser, **kw)          # append_f0=None: by n_symbols
    assert tout == tout_ref == list(FRAMES)
    for b in range(4):
        assert out[b].shape == (FRAMES[b] * 160,) and np.isfinite(out[b]).all() and np.array_equal(out[b], ref[b]), b
    conv, tout_c = s.convert(wd, deps, **kw)
    assert tout_c == tout and all(np.array_equal(a, r) for a, r in zip(conv, ref))
    # the F0 rows are inputs: without them the model hears something else (here: refused, the width says so)
    with pytest.raises(FacppgError, match="append_f0=False gives 40 input rows"):
        pipeline.synthesize_wavs(wd, deps, s.tacotron, s.waveglow, s.denoiser, append_f0=False, **kw)

    class Wide(object):
        _hp = {"n_symbols": 44}
    with pytest.raises(FacppgError, match="40 symbols, the PPG -> mel model was built for 44"):
        pipeline.synthesize_wavs(wd, deps, Wide(), None)
    with pytest.raises(FacppgError, match="40 symbols, the PPG -> mel model was built for 44"):
        pipeline.synthesize_long_wavs(wd, deps, Wide(), None)


def test_convert_long_carries_the_whole_recordings_rows(world, mono43, monkeypatch):
    """A 150-frame recording of three tones around two pauses: the segments' rows [K:] are slices of the whole recording's rows
    (the deltas at a cut are the recording's, not a segment's edge replication)."""
    import ppg
    from facppg import pipeline
    _cotenancy(monkeypatch)
    monkeypatch.setenv("FACPPG_STREAM", "0")
    s, deps = mono43["synthesizer"], world["deps"]
    rec = np.concatenate([fh.tone(120.0, 6400, 1), fh.silence(3200), fh.tone(180.0, 4800, 2), fh.silence(3200), fh.tone(140.0, 6400, 3)])
    wd = [_wd(rec)]
    x, lens = ppg.compute_ppg_padded(wd, deps, is_full_ppg=False, append_f0=True)
    assert lens == [150] and tuple(x.shape) == (1, 43, 150)
    thr = float(np.float32(np.median(x[0, 39].cpu().numpy())))
    seen = []
    stream = pipeline.synthesize_stream

    def spy(jobs, *a, **kw):
        jobs = list(jobs)
        seen.extend((j["prepared"][0].clone(), list(j["prepared"][1])) for j in jobs)
        return stream(jobs, *a, **kw)
    monkeypatch.setattr(pipeline, "synthesize_stream", spy)
    (audio,), (table,) = s.convert_long(wd, deps, seed=41, limit_to_input=True, max_frames=60, min_frames=20, min_pause=2, batch_frames=60,
                                        pause_threshold=thr)
    assert len(table) >= 3 and sum(n for _, n, _ in table) == 150 and all(t == n for _, n, t in table)
    assert audio.shape == (150 * 160,) and np.isfinite(audio).all()
    segments = [(y[k], n) for y, frames in seen for k, n in enumerate(frames)]
    assert [n for _, n in segments] == [n for _, n, _ in table]
    cut_slopes = 0
    for (y, n), (start, _, _) in zip(segments, table):
        assert tuple(y.shape)[0] == 43 and torch.equal(y[:, :n], x[0, :, start:start + n]) and not y[:, n:].any()
        cut_slopes += int(start > 0 and bool(y[41, 0] != 0))
    f0 = ppg.compute_f0(wd[0]).cpu().numpy()
    print("  %d segments %s, %d of 150 frames voiced, %d cuts with a non-zero slope in their first frame" % (
        len(table), [(a, n) for a, n, _ in table], int((f0 > 0).sum()), cut_slopes))
    assert (f0[5:35] > 0).all() and not f0[45:55].any()       # the tones are voiced, the pauses are not


def test_loader_appends_f0(world, monkeypatch):
    from common import data_utils
    from common.hparams import create_hparams_stage
    from facppg import synth
    from script.train_ppg2mel import load_model
    import ppg
    deps, tmp = world["deps"], world["tmp"]
    paths = []
    for i, (n, f) in enumerate(((4000, 110.0), (5920, 220.0), (3200, 150.0))):
        paths.append(str(tmp / ("f0_train%d.wav" % i)))
        wavfile.write(paths[-1], 16000, fh.tone(f, n, seed=i).astype(np.int16))
    listing = tmp / "f0_train.txt"
    listing.write_text("\n".join(paths) + "\n")
    hp = create_hparams_stage(n_symbols=43, is_full_ppg=False, is_append_f0=True, load_feats_from_disk=False)
    loader = data_utils.PPGMelLoader(str(listing), hp, ppg_deps=deps, batch_utterances=2)            # chunks of 2 + 1
    assert len(loader) == 3
    from common import feat
    for i, path in enumerate(loader.data_utterance_paths):
        x, y = loader[i]
        mono = data_utils.get_ppg_batch([path], deps, is_full_ppg=False)[0]
        f0 = ppg.compute_f0(feat.read_wav_kaldi(path)).cpu().numpy()
        want = data_utils.append_ppg(mono, f0)
        T = (wavfile.read(path)[1].shape[0] + 80) // 160
        assert x.dtype == torch.float32 and tuple(x.shape) == want.shape == (T, 43) and (f0[4:-4] > 0).all()
        assert float(np.abs(x.numpy()[:, :40] - want[:, :40]).max()) <= 2e-6
        assert np.array_equal(x.numpy()[:, 40:], want[:, 40:].astype(np.float32))
        assert np.array_equal(data_utils.get_f0_batch([path])[0], f0)
    # a precomputed track next to one wav wins over the tracker (how WORLD tracks get in); append_ppg cuts it to the PPG's frames
    np.save(paths[1] + ".f0.npy", np.full(40, 123.0))
    again = data_utils.PPGMelLoader(str(listing), hp, ppg_deps=deps)
    k = again.data_utterance_paths.index(paths[1])
    x, _ = again[k]
    assert tuple(x.shape) == (37, 43) and np.array_equal(x.numpy()[:, 40], np.full(37, np.float32(np.log(123.0 + np.finfo(float).eps))))
    assert not x.numpy()[:, 41:].any()
    other = again.data_utterance_paths.index(paths[0])
    assert torch.equal(again[other][0], loader[loader.data_utterance_paths.index(paths[0])][0])
    # the collate and the teacher-forced pass take the batch
    model = load_model(hp)
    model.load_state_dict(synth.tacotron_state_dict(hp))
    model.eval()
    xb, yb = model.parse_batch(data_utils.ppg_acoustics_collate([loader[i] for i in range(3)]))
    assert tuple(xb[0].shape) == (3, 43, 37)
    out = model(xb, seed=7)
    assert out[0].shape[:2] == (3, hp.n_acoustic_feat_dims) and all(torch.isfinite(o).all() for o in out[:3])
