"""CPU: the F0 tracker without a device -- the new symbols in header, library and binding, every host-side refusal of the new entry
points (nothing is launched: the device addresses are made up), the host append_ppg family against the reference's own outputs
(tests/golden/f0_append.npz, written by make_golden_f0_append.py), the DEFINITION of the tracker on steady tones and silence
(f0_helpers.py in float64: a condition on the definition, not on a kernel), and PPGMelLoader accepting is_append_f0."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import f0_helpers as fh
from conftest import ROOT
from facppg import lib as flib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
NEW = ("facppg_f0_workspace_bytes", "facppg_f0_nccf_batch", "facppg_f0_track_batch", "facppg_f0_batch", "facppg_lf0_rows_padded",
       "facppg_tdnn_forward_batch_padded_strided")


def test_header_library_and_binding_know_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facppg.h")).read(), flags=re.S)
    L = flib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in flib.exported_symbols()
    assert "facppg_f0_config" in src and L.facppg_version() == 103
    m = re.search(r"typedef struct facppg_f0_config \{(.*?)\}", src, flags=re.S)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == [n for n, _ in flib.F0Config._fields_]
    from ppg import F0Options
    cfg = F0Options().config()
    assert [getattr(cfg, n) for n, _ in flib.F0Config._fields_] == [16000, 160, 320, 40, 334, 50.0, pytest.approx(0.2), 2.0]
    wl, g = F0Options().tables()
    rwl, rg = fh.tables()
    assert wl.dtype == np.float32 and wl.shape == (295,) and np.array_equal(wl, rwl) and np.array_equal(g, rg)


def _cfg(**kw):
    from ppg import F0Options
    return F0Options(**kw).config()


def _fake(k, null=None):
    return ctypes.c_void_p(0 if null == k else 0x1000 * (k + 1))


S_OFF, F_OFF = (0, 400, 2000), (0, 3, 13)        # 400 samples = 3 frames, 1600 = 10


def _nccf(L, cfg=None, s_off=S_OFF, f_off=F_OFF, B=2, null=None):
    rc = L.facppg_f0_nccf_batch(_cfg() if cfg is None else cfg, _fake(0, null), _fake(1, null), None if null == "s" else flib.offsets_array(s_off),
                                _fake(2, null), None if null == "f" else flib.offsets_array(f_off), B, _fake(3, null), None)
    return rc, L.facppg_last_error().decode()


def _track(L, cfg=None, f_off=F_OFF, B=2, ws_bytes=1 << 30, null=None):
    rc = L.facppg_f0_track_batch(_cfg() if cfg is None else cfg, _fake(0, null), _fake(1, null), None if null == "f" else flib.offsets_array(f_off), B,
                                 _fake(2, null), _fake(3, null), _fake(4, null), _fake(5, null), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def _batch(L, cfg=None, s_off=S_OFF, f_off=F_OFF, B=2, ws_bytes=1 << 30, null=None):
    rc = L.facppg_f0_batch(_cfg() if cfg is None else cfg, _fake(0, null), _fake(1, null), None if null == "s" else flib.offsets_array(s_off),
                           _fake(2, null), None if null == "f" else flib.offsets_array(f_off), B, _fake(3, null), _fake(4, null), _fake(5, null),
                           _fake(6, null), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def _rows(L, f_off=F_OFF, B=2, Tmax=10, stride=30, null=None):
    rc = L.facppg_lf0_rows_padded(_fake(0, null), _fake(1, null), None if null == "f" else flib.offsets_array(f_off), B, Tmax, stride, _fake(2, null), None)
    return rc, L.facppg_last_error().decode()


def test_host_side_refusals():
    L = flib.load()
    need = L.facppg_f0_workspace_bytes(_cfg(), 13)
    # back-pointers uint16 [T][L + 1], the local costs and the matrix of facppg_f0_batch
    assert need >= 13 * (296 * 2 + 296 * 4 + 297 * 4)
    for call, nulls in ((_nccf, [0, 1, 2, 3, "s", "f"]), (_track, [0, 1, 2, 3, 4, 5, "f"]), (_batch, [0, 1, 2, 3, 4, 5, 6, "s", "f"]),
                        (_rows, [0, 1, 2, "f"])):
        for null in nulls:
            rc, msg = call(L, null=null)
            assert rc == EINVAL and "NULL" in msg, (call.__name__, null, rc, msg)
        rc, msg = call(L, B=0)
        assert rc == EINVAL and "B must be at least 1 (got 0)" in msg, (call.__name__, rc, msg)
        rc, msg = call(L, f_off=(0, 3, 3))
        assert rc == EINVAL and "offsets must increase" in msg, (call.__name__, rc, msg)
        rc, msg = call(L, f_off=(1, 3, 13))
        assert rc == EINVAL and "offsets must start at 0" in msg, (call.__name__, rc, msg)
    for call in (_nccf, _batch):
        rc, msg = call(L, s_off=(0, 400, 400))
        assert rc == EINVAL and "offsets must increase" in msg, (call.__name__, rc, msg)
        rc, msg = call(L, s_off=(0, 79, 1679), f_off=(0, 1, 11))           # 79 samples: (79 + 80) / 160 = 0 frames
        assert rc == EINVAL and "no frames in 79 samples" in msg, (call.__name__, rc, msg)
        rc, msg = call(L, f_off=(0, 4, 14))
        assert rc == EINVAL and "400 samples are 3 frames, the frame offsets say 4" in msg, (call.__name__, rc, msg)
    for call in (_nccf, _track, _batch):
        for kw, text in ((dict(lag_min=1), "lag_min must be at least 2 (got 1)"), (dict(lag_max=2048), "lag_max must be below 2048 (got 2048)"),
                         (dict(window=0), "window must be at least 1 (got 0)"), (dict(lag_min=50, lag_max=49), "lag_max 49 is below lag_min 50"),
                         (dict(voicing_cost=-0.5), "not negative"), (dict(frame_shift=0), "must be positive")):
            rc, msg = call(L, cfg=_cfg(**kw))
            assert rc == EINVAL and text in msg, (call.__name__, kw, rc, msg)
            assert L.facppg_f0_workspace_bytes(_cfg(**kw), 13) == 0 and text in L.facppg_last_error().decode()
        rc, msg = call(L, cfg=_cfg(lag_min=2, lag_max=2047))
        assert rc == EUNSUPPORTED and "at most 1023 candidate lags" in msg, (call.__name__, rc, msg)
        rc, msg = call(L, cfg=_cfg(window=20000))
        assert rc == EUNSUPPORTED and "a workgroup stages" in msg, (call.__name__, rc, msg)
        many = 65536
        off = tuple(range(many + 1))
        rc, msg = call(L, **(dict(f_off=off, B=many) if call is _track else dict(s_off=tuple(160 * v for v in off), f_off=off, B=many)))
        assert rc == EUNSUPPORTED and "got 65536" in msg, (call.__name__, rc, msg)
    for call in (_track, _batch):
        rc, msg = call(L, ws_bytes=need - 1)
        assert rc == EWORKSPACE and str(need - 1) in msg and str(need) in msg, (call.__name__, rc, msg)
    assert L.facppg_f0_workspace_bytes(_cfg(), 0) == 0 and "total_frames must be positive (got 0)" in L.facppg_last_error().decode()
    assert L.facppg_f0_workspace_bytes(None, 13) == 0 and "NULL" in L.facppg_last_error().decode()
    rc, msg = _rows(L, Tmax=9)
    assert rc == EINVAL and "Tmax 9 is shorter than the longest utterance (10 frames)" in msg, (rc, msg)
    rc, msg = _rows(L, stride=29)
    assert rc == EINVAL and "batch stride of 29 floats" in msg, (rc, msg)
    # the strided posteriors: a stride shorter than the K rows of one utterance
    junk, off = ctypes.c_void_p(0x1000), flib.offsets_array((0, 3, 13))
    assert L.facppg_tdnn_forward_batch_padded_strided(None, junk, junk, off, 2, None, 0, 10, 0, junk, junk, 1 << 20, None) == EINVAL


def test_python_refusals_need_no_device():
    from common import feat
    from ppg import F0Options, compute_f0_batch
    with pytest.raises(TypeError, match="no option"):
        F0Options(lag_mim=3)
    with pytest.raises(ValueError, match="no utterance"):
        compute_f0_batch([])
    with pytest.raises(flib.FacppgError, match="must be a GPU tensor"):
        compute_f0_batch([feat.WaveData(16000, torch.zeros(1, 1600))])


def test_host_append_ppg_family_equals_the_reference():
    from common import data_utils as du
    gold = np.load(os.path.join(ROOT, "tests", "golden", "f0_append.npz"))
    assert np.array_equal(gold["delta_win"], du.DELTA_WIN) and np.array_equal(gold["acc_win"], du.ACC_WIN)
    for key in ("1_1", "2_3", "5_4", "37_40"):
        feats, f0 = gold["feats_" + key], gold["f0_" + key]
        assert (f0 == 0).any() or key == "1_1"
        got = du.append_ppg(feats, f0)
        want = gold["append_" + key]
        assert got.shape == want.shape == (min(len(feats), len(f0)), 8) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-12, key
        assert np.abs(du.compute_delta_acc_feat(feats, True, True) - gold["delta_acc_" + key]).max() <= 1e-12, key
        assert np.abs(du.compute_dynamic_matrix(feats, du.DELTA_WIN) - gold["delta_" + key]).max() <= 1e-12, key
        vec = du.compute_dynamic_vector(feats[:, 0], du.ACC_WIN, len(feats))
        assert vec.shape == gold["vector_" + key].shape == (len(feats), 1) and np.abs(vec - gold["vector_" + key]).max() <= 1e-12, key
        # a float32 track (what the device tracker returns) is widened first: the same rows to float32 rounding of the track
        assert np.abs(du.append_ppg(feats, f0.astype(np.float32)) - want).max() <= 1e-6
    assert du.compute_delta_acc_feat(feats, False, False) is feats
    with pytest.raises(ValueError, match="delta-delta"):
        du.compute_delta_acc_feat(feats, False, True)


def test_the_definition_finds_steady_tones_and_rejects_silence():
    """The float64 reference, no device.  Measured: worst relative error 2.0e-4 (220 Hz) on frames at least 4 from either end."""
    for f in fh.TONES:
        lag, f0 = fh.reference_f0(fh.tone(f, 8000, seed=int(f)))
        inner = slice(4, len(f0) - 4)
        assert len(f0) == 50 and (lag[inner] > 0).all(), f
        rel = float(np.abs(f0[inner] - f).max() / f)
        print("tone %5.1f Hz: worst relative error %.2e on %d interior frames" % (f, rel, len(f0) - 8))
        assert rel <= 5e-3, (f, rel)
    for x in (fh.silence(3200), fh.dc_silence(3200), fh.silence(80), fh.silence(800)):
        lag, f0 = fh.reference_f0(x)
        assert len(lag) == fh.num_frames(len(x)) and not lag.any() and not f0.any()


def test_float32_restatement_agrees_with_float64_on_the_gpu_cases():
    """Every case of the GPU test is decidable: the float32 tracker over the float32 NCCF makes the float64 decisions."""
    dev = fh.emulation_deviation()
    print("float32 NCCF restatement: worst |phi32 - phi64| = %.3e, kernel tolerance %.3e" % (dev, fh.nccf_tolerance()))
    assert 0.0 < dev < 1e-5 and fh.nccf_tolerance() == 4.0 * dev
    for x, (p64, p32) in zip(fh.nccf_cases(), fh.nccf_references()):
        assert p64.shape == (fh.num_frames(len(x)), fh.L + 2) and np.abs(p64).max() <= 1.0
        l64, f64 = fh.track(p64, np.float64)
        l32, f32 = fh.track(p32, np.float32)
        assert np.array_equal(l64, l32), len(x)
        assert np.abs(f32 - f64).max() <= 1e-3 * max(1.0, f64.max())


class _Hp(object):
    def __init__(self, **kw):
        from common.hparams import create_hparams_stage
        hp = create_hparams_stage(n_symbols=43, is_full_ppg=False, is_append_f0=True)
        self.__dict__.update({k: getattr(hp, k) for k in (
            "max_wav_value", "sampling_rate", "is_full_ppg", "is_append_f0", "is_cache_feats", "load_feats_from_disk",
            "feats_cache_path", "ppg_subsampling_factor", "seed", "filter_length", "hop_length", "win_length", "n_acoustic_feat_dims",
            "mel_fmin", "mel_fmax")})
        self.__dict__.update(kw)


def test_loader_accepts_is_append_f0(tmp_path):
    """With features from the disk the loader needs no device: is_append_f0 no longer raises, and the items are the cached ones."""
    from common.data_utils import PPGMelLoader, append_ppg
    listing = str(tmp_path / "list.txt")
    open(listing, "w").write("a.wav\nb.wav\n")
    g = np.random.Generator(np.random.PCG64(5))
    ppgs = [append_ppg(g.random((T, 40)), 100.0 * (g.random(T) > 0.4)).astype(np.float32) for T in (7, 4)]
    mels = [torch.zeros(9, 80), torch.zeros(5, 80)]
    cache = str(tmp_path / "feats.pkl")
    with open(cache, "wb") as f:
        pickle.dump([ppgs, mels], f)

    class Deps(object):
        nnet = lda = monophone_trans = None
    loader = PPGMelLoader(listing, _Hp(load_feats_from_disk=True, feats_cache_path=cache), ppg_deps=Deps())
    assert loader.is_append_f0 and len(loader) == 2
    x, y = loader[0]
    assert tuple(x.shape) == (7, 43) and x.dtype == torch.float32 and np.array_equal(x.numpy(), ppgs[0])
    assert np.allclose(x.numpy()[:, 40][ppgs[0][:, 40] < 0], np.log(np.finfo(float).eps))          # unvoiced frames: log(eps) = -36.04


def test_loader_wants_an_f0_source_per_utterance(tmp_path):
    """Without an acoustic model the PPG is a file, and then the F0 has to be one as well; with both files the check passes and
    the loader's next check (the sampling rate) speaks."""
    from scipy.io import wavfile
    from common.data_utils import PPGMelLoader
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, 22050, np.zeros(4000, np.int16))
    listing = str(tmp_path / "list.txt")
    open(listing, "w").write(wav + "\n")

    class Deps(object):
        nnet = lda = monophone_trans = None
    hp = _Hp(load_feats_from_disk=False)
    with pytest.raises(NotImplementedError, match="is_append_f0.*no precomputed F0 track.*no acoustic model"):
        PPGMelLoader(listing, hp, ppg_deps=Deps())
    np.save(wav + ".ppg.npy", np.zeros((25, 40), np.float32))
    with pytest.raises(NotImplementedError, match="a precomputed PPG file"):
        PPGMelLoader(listing, hp, ppg_deps=Deps())
    np.save(str(tmp_path / "a.f0.npy"), np.zeros(25))
    with pytest.raises(ValueError, match="22050 SR doesn't match target 16000 SR"):
        PPGMelLoader(listing, hp, ppg_deps=Deps())


def test_corpus_script_follows_the_hparam():
    from script import synthesize_corpus
    hp = synthesize_corpus.parse_hparams("is_append_f0=True,n_symbols=43,is_full_ppg=False")
    assert hp.is_append_f0 is True and hp.n_symbols == 43
    seen = {}

    class S(object):
        def stream(self, jobs, **kw):
            seen.update(kw)
            return iter(())
    args = synthesize_corpus.parse(["--ppg2mel_model", "t.pt", "--waveglow_model", "w.pt", "--output_dir", "o", "--wav_list", "w.txt", "--device_ppgs"])
    synthesize_corpus.synthesize_shard(S(), None, [3, 4], 0, 1, args, wav_paths=["a", "b"], ppg_deps=object(), is_full_ppg=False, append_f0=True)
    assert seen["append_f0"] is True and seen["is_full_ppg"] is False
    seen.clear()
    synthesize_corpus.synthesize_shard(S(), None, [3, 4], 0, 1, args, wav_paths=["a", "b"], ppg_deps=object(), is_full_ppg=False)
    assert "append_f0" not in seen
