"""GPU: the layers above facppg_ppg_dtw -- facppg.score.roundtrip, Synthesizer.convert_scored and
script.synthesize_corpus --wav_list --score_file.

Acoustic model, wavs (frames 1, 5, 37, 150; the 37-frame one sampled at 44.1 kHz) and corpus are test_gpu_ppg_batch.py's, the
monophone checkpoints and their Synthesizer test_gpu_wav2wav.py's, under the co-tenancy environment those tests set; seeds are
fixed per utterance and every step limit is the utterance's input length."""
import copy
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from test_feat_cpu import KF
from test_gpu_ppg_batch import FRAMES, WAVS, _wave_data, corpus, world  # noqa: F401  (the module fixtures, built once for this file)
from test_gpu_wav2wav import SEEDS, _cotenancy, mono  # noqa: F401

pytestmark = pytest.mark.gpu

KEYS = ("cost", "steps", "agree", "distance", "agreement", "stretch", "teacher_frames", "roundtrip_frames")


def _same(x, y):
    return sorted(x) == sorted(y) == sorted(KEYS) and all(x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes() for k in KEYS)


def test_teacher_audio_as_the_conversion_scores_perfectly(world):
    """The teacher wavs' own samples, scaled to [-1, 1], as the "converted" audio: one front-end pass of 2 B utterances, rows [:B]
    against rows [B:] -- equal frames, the diagonal path, every top class agreeing."""
    from facppg import score
    wd = _wave_data(world["wavs"])
    rates = [fs for _, fs in WAVS]
    audio = [w.astype(np.float32) / 32768.0 for w in world["wavs"]]
    out = score.roundtrip(wd, audio, rates, world["deps"])
    print({k: out[k].tolist() for k in KEYS})
    assert sorted(out) == sorted(KEYS)
    assert out["teacher_frames"].tolist() == out["roundtrip_frames"].tolist() == out["steps"].tolist() == list(FRAMES)
    assert out["agreement"].tolist() == [1.0] * 4 and out["stretch"].tolist() == [1.0] * 4
    # d(i, i) = max(0, 1 - sum_k a[k][i]): a posterior's mass is 1 to within the 1e-4 test_gpu_ppg_batch.py holds it to
    assert np.isfinite(out["cost"]).all() and (out["distance"] >= 0).all() and (out["distance"] <= 2e-4).all()
    # device tensors instead of host arrays, a band: the same alignment
    dev = score.roundtrip(wd, [torch.from_numpy(a).cuda() for a in audio], rates, world["deps"], band=2)
    assert _same(dev, out)


def test_convert_scored_is_convert_plus_roundtrip(world, mono, monkeypatch):
    from facppg import score
    _cotenancy(monkeypatch)
    s, deps = mono["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])
    kw = dict(utterance_seeds=SEEDS, step_limits=list(FRAMES))
    ref, tout_ref = s.convert(wd, deps, **kw)
    audio, tout, scores = s.convert_scored(wd, deps, **kw)
    assert tout == tout_ref == list(FRAMES) and len(audio) == 4
    for b in range(4):
        assert audio[b].dtype == np.float32 and np.array_equal(audio[b], ref[b]), b
    by_hand = score.roundtrip(wd, ref, s.hparams.sampling_rate, deps)
    print({k: scores[k].tolist() for k in KEYS})
    assert _same(scores, by_hand)
    assert scores["teacher_frames"].tolist() == list(FRAMES) and scores["roundtrip_frames"].tolist() == list(FRAMES)   # hop 160 at 16 kHz
    for k in ("cost", "distance", "agreement", "stretch"):
        assert np.isfinite(scores[k]).all(), k
    assert (scores["agreement"] >= 0).all() and (scores["agreement"] <= 1).all() and (scores["stretch"] >= 1).all()
    assert (scores["distance"] >= 0).all() and (scores["distance"] <= 1).all()
    # on the device, with a band
    dev_audio, _, banded = s.convert_scored(wd, deps, score_band=8, return_device=True, **kw)
    assert all(a.is_cuda and np.array_equal(a.cpu().numpy(), r) for a, r in zip(dev_audio, ref))
    assert _same(banded, score.roundtrip(wd, ref, 16000, deps, band=8))


def test_dependencies_without_the_monophone_matrix_are_refused_before_any_launch(world, mono):
    from facppg import score
    from facppg.lib import FacppgError
    bare = copy.copy(world["deps"])
    bare.monophone_trans = None

    class Untouchable(object):
        def data(self):
            raise AssertionError("device work was reached")
    with pytest.raises(FacppgError, match="monophone_trans"):
        score.roundtrip([Untouchable()], [np.zeros(160, dtype=np.float32)], 16000, bare)
    with pytest.raises(FacppgError, match="monophone_trans"):
        mono["synthesizer"].convert_scored([Untouchable()], bare)


def test_synthesize_corpus_score_file(world, corpus, mono, monkeypatch):
    """--wav_list --score_file at world size 1: one line per wav in list order, the numbers convert_scored gives for the batches
    the script forms, and the wavs of a run without the flag, byte for byte."""
    from common.feat import read_wav_kaldi
    from facppg import score, shard
    from script import synthesize_corpus
    _cotenancy(monkeypatch)
    tmp = world["tmp"]
    paths, listing = corpus
    common = ["--ppg2mel_model", mono["taco_path"], "--waveglow_model", mono["wg_path"], "--seed", "31", "--limit_steps_to_input",
              "--hparams", "n_symbols=40,is_full_ppg=False", "--batch_size", "3", "--wav_list", listing, "--nnet_path", world["nnet_path"],
              "--feats_dir", KF]
    names = ["train%d.wav" % i for i in range(4)]
    score_file = str(tmp / "scores.tsv")
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "rt_plain")]) == names
    assert not os.path.exists(score_file)
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "rt_scored"), "--score_file", score_file, "--score_band", "12"]) == names
    for n in names:
        assert open(os.path.join(str(tmp), "rt_scored", n), "rb").read() == open(os.path.join(str(tmp), "rt_plain", n), "rb").read(), n
    lines = open(score_file).read().splitlines()
    assert len(lines) == 4 and [l.split("\t")[0] for l in lines] == paths
    lengths = synthesize_corpus.wav_ppg_lengths(paths)
    expected = {}
    for batch in shard.batches(shard.partition(lengths, 1)[0], lengths, 3):
        audio, tout, scores = mono["synthesizer"].convert_scored([read_wav_kaldi(paths[i]) for i in batch], world["deps"], score_band=12,
                                                                 utterance_seeds=[31 + 2 * i for i in batch], step_limits=[lengths[i] for i in batch])
        for b, i in enumerate(batch):
            assert np.array_equal(audio[b], wavfile.read(os.path.join(str(tmp), "rt_scored", names[i]))[1]), i
            expected[i] = score.score_line(paths[i], scores, b)
    print("\n".join(lines))
    assert lines == [expected[i] for i in range(4)]
    for l, T in zip(lines, lengths):
        f = l.split("\t")
        assert len(f) == 6 and int(f[1]) == int(f[2]) == T and 0.0 <= float(f[3]) <= 1.0 and 0.0 <= float(f[4]) <= 1.0 and float(f[5]) >= 1.0
