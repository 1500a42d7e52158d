"""CPU: what the batched PPG front end checks without a device -- the new C symbols, the offsets of a batch, the options
of PPGMelLoader and of script.synthesize_corpus, and get_ppg_batch on precomputed PPG files."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.io import wavfile

from conftest import ROOT
from facppg import lib as flib

NEW = ("facppg_tdnn_batch_workspace_bytes", "facppg_tdnn_forward_batch", "facppg_tdnn_forward_batch_reduced",
       "facppg_mfcc_batch_workspace_bytes", "facppg_mfcc_compute_batch", "facppg_cmn_splice_transform_batch")


def test_new_symbols_are_declared_bound_and_exported():
    L = flib.load()
    header = open(os.path.join(ROOT, "include", "facppg.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in flib.exported_symbols() and hasattr(L, name), name


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_offsets_are_checked_before_anything_else():
    """Offsets that do not start at 0, or that do not increase, are refused on the host: no handle is read, no launch made
    (the pointers handed over here are not device pointers)."""
    L = flib.load()
    junk = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    good = _i32(0, 3, 8)
    for bad, what in ((_i32(1, 3, 8), "start at 0"), (_i32(0, 5, 4), "must increase"), (_i32(0, 3, 3), "must increase")):
        assert L.facppg_tdnn_forward_batch(junk, junk, junk, bad, 2, junk, junk, 1 << 20, None) == -1
        assert what in L.facppg_last_error().decode()
        assert L.facppg_tdnn_forward_batch_reduced(junk, junk, junk, bad, 2, junk, 40, junk, junk, 1 << 20, None) == -1
        assert what in L.facppg_last_error().decode()
        assert L.facppg_tdnn_batch_workspace_bytes(junk, bad, 2) == 0
        assert L.facppg_mfcc_compute_batch(junk, junk, junk, bad, junk, good, 2, 0, junk, junk, 1 << 20, None) == -1
        assert what in L.facppg_last_error().decode()
        assert L.facppg_cmn_splice_transform_batch(junk, junk, bad, 2, 13, 1, 3, 3, None, 0, 0, junk, junk, None) == -1
        assert what in L.facppg_last_error().decode()
    assert L.facppg_tdnn_forward_batch(junk, junk, junk, good, 0, junk, junk, 1 << 20, None) == -1
    assert L.facppg_tdnn_forward_batch(junk, junk, junk, None, 2, junk, junk, 1 << 20, None) == -1
    assert list(flib.host_offsets([3, 5])) == [0, 3, 8]


class _Hp(object):
    def __init__(self, **kw):
        from common.hparams import create_hparams_stage
        hp = create_hparams_stage(n_symbols=40, is_full_ppg=False, load_feats_from_disk=False)
        self.__dict__.update({k: getattr(hp, k) for k in (
            "max_wav_value", "sampling_rate", "is_full_ppg", "is_append_f0", "is_cache_feats", "load_feats_from_disk",
            "feats_cache_path", "ppg_subsampling_factor", "seed", "filter_length", "hop_length", "win_length", "n_acoustic_feat_dims",
            "mel_fmin", "mel_fmax")})
        self.__dict__.update(kw)


class _Deps(object):
    nnet = lda = monophone_trans = None


def test_loader_refusals(tmp_path):
    from common.data_utils import PPGMelLoader
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, 22050, np.zeros(4000, np.int16))
    listing = str(tmp_path / "list.txt")
    open(listing, "w").write(wav + "\n")
    with pytest.raises(ValueError, match="do not rewrite"):
        PPGMelLoader(listing, _Hp(is_cache_feats=True, load_feats_from_disk=True), ppg_deps=_Deps())
    with pytest.raises(NotImplementedError, match="is_append_f0"):
        PPGMelLoader(listing, _Hp(is_append_f0=True), ppg_deps=_Deps())
    with pytest.raises(ValueError, match="22050 SR doesn't match target 16000 SR"):
        PPGMelLoader(listing, _Hp(), ppg_deps=_Deps())
    with pytest.raises(ValueError, match="batch_utterances"):
        PPGMelLoader(listing, _Hp(), ppg_deps=_Deps(), batch_utterances=0)


def test_corpus_script_takes_one_source_of_ppgs(capsys):
    from script import synthesize_corpus
    common = ["--ppg2mel_model", "t.pt", "--waveglow_model", "w.pt", "--output_dir", "out"]
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(common + ["--ppg_list", "a.txt", "--wav_list", "b.txt"])
    assert "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(common)
    assert "one of the arguments --ppg_list --wav_list is required" in capsys.readouterr().err
    args = synthesize_corpus.parse(common + ["--wav_list", "b.txt"])
    assert args.wav_list == "b.txt" and args.ppg_list is None and args.nnet_path is None
    assert synthesize_corpus.parse(common + ["--ppg_list", "a.txt"]).wav_list is None


def test_wav_ppg_lengths_from_headers(tmp_path):
    from script import synthesize_corpus
    paths = []
    for i, (n, fs) in enumerate(((160, 16000), (5920, 16000), (16317, 44100), (24000, 16000))):
        paths.append(str(tmp_path / ("u%d.wav" % i)))
        wavfile.write(paths[-1], fs, np.zeros(n, np.int16))
    assert synthesize_corpus.wav_ppg_lengths(paths) == [1, 37, 37, 150]


def test_get_ppg_batch_reads_precomputed_files_without_a_device(tmp_path, monkeypatch):
    import torch
    from common import data_utils
    monkeypatch.setattr(torch.Tensor, "cuda", lambda *a, **k: pytest.fail("touched the GPU"))
    g = np.random.Generator(np.random.PCG64(1))
    a, b = g.random((7, 40)).astype(np.float32), g.random((3, 40)).astype(np.float64)
    np.save(str(tmp_path / "a.npy"), a)
    np.save(str(tmp_path / "b.ppg.npy"), b)
    got = data_utils.get_ppg_batch([str(tmp_path / "a.npy"), str(tmp_path / "b.wav")], None)
    assert len(got) == 2 and np.array_equal(got[0], a) and np.array_equal(got[1], b.astype(np.float32)) and got[1].dtype == np.float32
    for p, single in zip([str(tmp_path / "a.npy"), str(tmp_path / "b.wav")], got):
        assert np.array_equal(data_utils.get_ppg(p), single)
    assert data_utils.get_ppg_batch([], None) == []
    with pytest.raises(NotImplementedError, match="acoustic model"):                      # get_ppg's error: neither a file nor a model
        data_utils.get_ppg_batch([str(tmp_path / "a.npy"), str(tmp_path / "c.wav")], _Deps())
    with pytest.raises(NotImplementedError, match="acoustic model"):
        data_utils.get_ppg(str(tmp_path / "c.wav"), _Deps())


def test_batch_front_end_needs_a_model():
    import ppg
    with pytest.raises(flib.FacppgError, match="acoustic model"):
        ppg.compute_full_ppg_batch(None, [np.zeros((3, 40), np.float32)])
    with pytest.raises(flib.FacppgError, match="acoustic model"):
        ppg.compute_ppg_batch([], _Deps())


def test_product_still_never_imports_the_oracle():
    pat = re.compile(r"^\s*(from\s+oracle\b|import\s+oracle\b)", re.M)
    root = os.path.join(ROOT, "fac-via-ppg_amd")
    offenders = [os.path.join(d, f) for d, _, files in os.walk(root) for f in files
                 if f.endswith(".py") and pat.search(open(os.path.join(d, f)).read())]
    assert not offenders, offenders
