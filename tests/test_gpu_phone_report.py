"""GPU: the layers above the aligner -- facppg.align.phone_report, score.roundtrip(phones=True),
Synthesizer.convert_scored(phones=True) and script.synthesize_corpus --phone_file.

Acoustic model, wavs (frames 1, 5, 37, 150; the 37-frame one sampled at 44.1 kHz), corpus and the monophone synthesizer are
test_gpu_roundtrip.py's own fixtures, under the co-tenancy environment those tests set; seeds are fixed per utterance and every
step limit is the utterance's input length."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import ROOT
from test_feat_cpu import KF
from test_gpu_roundtrip import FRAMES, KEYS, SEEDS, WAVS, _cotenancy, _same, _wave_data, corpus, mono, world  # noqa: F401  (the module fixtures)

pytestmark = pytest.mark.gpu

PHONES = os.path.join(ROOT, "tests", "golden", "arpa_phonemes")
SIL = 39


def _same_report(x, y):
    return len(x) == len(y) and all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y))


def test_teacher_audio_as_the_conversion_keeps_every_phone(world):
    """The teacher wavs' own samples as the "converted" audio: both halves of the front end's batch hold the same posteriors, so
    every teacher phone lands where the teacher has it, with the teacher's own segment score."""
    from common.feat import WaveData
    from facppg import align, score
    from ppg.compute_ppg import compute_ppg_padded
    wd = _wave_data(world["wavs"])
    rates = [fs for _, fs in WAVS]
    audio = [w.astype(np.float32) / 32768.0 for w in world["wavs"]]
    out = score.roundtrip(wd, audio, rates, world["deps"], phones=True)
    assert sorted(out) == sorted(KEYS + ("phones", "phones_kept"))
    plain = score.roundtrip(wd, audio, rates, world["deps"])
    assert _same({k: out[k] for k in KEYS}, plain)
    # the teacher's own: its rows of the same front-end pass decoded, and force-aligned to their own sequence
    back = [WaveData(float(fs), torch.from_numpy(a).cuda().reshape(1, -1) * 32768.0) for a, fs in zip(audio, rates)]
    x, frames = compute_ppg_padded(list(wd) + back, world["deps"], is_full_ppg=False)
    x, frames = x[:4], frames[:4]
    runs = align.decode_phones(x, frames)
    states = [align.teacher_sequence(r, SIL, T) for r, T in zip(runs, frames)]
    own = align.force_align(x, frames, [s[0] for s in states], [s[1] for s in states])
    for b, rep in enumerate(out["phones"]):
        cls, opt, t_start, t_frames = states[b]
        print(b, [(int(r["phone"]), int(r["start"]), int(r["frames"]), round(float(r["gop"]), 3), round(float(r["share"]), 2)) for r in rep])
        assert rep.dtype == align.REPORT_DTYPE and rep["phone"].tolist() == cls.tolist()
        assert rep["teacher_start"].tolist() == t_start.tolist() and rep["teacher_frames"].tolist() == t_frames.tolist()
        assert int(rep["frames"].sum()) == FRAMES[b]
        spoken = cls != SIL
        assert rep["start"][spoken].tolist() == t_start[spoken].tolist() and rep["frames"][spoken].tolist() == t_frames[spoken].tolist(), b
        assert rep["gop"].tobytes() == own["gop"][b].tobytes(), b
        assert (rep["gop"] <= 0).all() and rep["kept"][spoken].all(), b
    assert out["phones_kept"].tolist() == [1.0] * 4


def test_a_zeroed_run_through_the_front_end_is_aligned_to_the_teachers_sequence(world):
    """The 150-frame teacher with the samples of one decoded non-sil run zeroed, as the conversion, through roundtrip's own
    front-end pass: the report's teacher columns are the teacher's decode, every frame of the conversion is given to a state, and
    whatever phone lies before or after the zeroed one and its two neighbours keeps its frames to within the front end's context.
    With this fixture's random acoustic model that last clause has nothing to hold: the model puts one class on top of all 150
    frames, the teacher decodes to sil? - ah - sil?, and the zeroed run is the whole utterance (the test prints how many phones
    it held to the bound: 0).  test_a_damaged_phone_on_synthetic_posteriors asks it of posteriors that have phones."""
    from facppg import align, score
    from ppg.compute_ppg import compute_ppg_padded
    deps = world["deps"]
    # what a PPG frame sees of the audio: the acoustic model's own context plus the feature splice in front of it, on either side
    left, right = deps.nnet.context()
    context = (left + int(deps.left_context)) + (right + int(deps.right_context))
    assert context == (6 + 3) + (7 + 3)
    wd = _wave_data(world["wavs"])[3:]
    # (twice: as many columns as roundtrip's own pass below, so the same GEMM kernel and the same bits)
    x, frames = compute_ppg_padded(wd * 2, deps, is_full_ppg=False)
    runs = align.decode_phones(x[:1], frames[:1])[0]
    seq, opt, t_start, t_frames = align.teacher_sequence(runs, SIL, 150)
    inner = [i for i in range(len(seq)) if seq[i] != SIL and t_frames[i] > 0]
    assert inner, runs.tolist()
    hit = max(inner, key=lambda i: (t_frames[i], -i))             # the longest non-sil run
    samples = world["wavs"][3].astype(np.float32) / 32768.0
    samples[160 * t_start[hit]:160 * (t_start[hit] + t_frames[hit])] = 0.0
    out = score.roundtrip(wd, [samples], 16000, deps, phones=True)
    rep = out["phones"][0]
    print("zeroed state %d of %d (class %d, frames %d + %d)" % (hit, len(seq), seq[hit], t_start[hit], t_frames[hit]))
    print([(int(r["phone"]), int(r["teacher_start"]), int(r["teacher_frames"]), int(r["start"]), int(r["frames"]), int(r["kept"])) for r in rep])
    assert rep["phone"].tolist() == seq.tolist() and rep["teacher_start"].tolist() == t_start.tolist()
    assert rep["teacher_frames"].tolist() == t_frames.tolist() and int(rep["frames"].sum()) == 150
    assert (rep["gop"] <= 0).all() and 0.0 <= out["phones_kept"][0] <= 1.0
    held = [i for i in range(len(seq)) if abs(i - hit) > 1 and not (seq[i] == SIL and t_frames[i] == 0)]
    for i in held:
        assert abs(int(rep["start"][i]) - int(t_start[i])) <= context and abs(int(rep["frames"][i]) - int(t_frames[i])) <= context, (i, rep[i])
    print("phones held to the context of %d frames: %d" % (context, len(held)))


def test_a_damaged_phone_on_synthetic_posteriors():
    """The fixtures' acoustic model is a random network: the teacher wavs decode to a single phone, which leaves the test above
    little to say.  The same property on posteriors that have phones (align_helpers' generator, 150 frames, 22 states): the
    frames of one inner run replaced by another class in the "conversion" -- that phone is lost (it keeps the one frame a
    mandatory state must take, without a hit), at most its two neighbours move, and every other phone has the record it has when
    the teacher is aligned to itself, bit for bit."""
    import align_helpers as ah
    from facppg import align
    T, D = 150, 40
    x = ah.inputs(T, D)
    xt = torch.from_numpy(x).cuda()[None]
    own, own_kept = align.phone_report(xt, [T], xt, [T])
    own = own[0]
    spoken = (own["phone"] != D - 1) & (own["teacher_frames"] > 0)
    assert len(own) >= 10 and own_kept.tolist() == [1.0] and own["kept"][spoken].all()
    assert own["start"][spoken].tolist() == own["teacher_start"][spoken].tolist()
    assert own["frames"][spoken].tolist() == own["teacher_frames"][spoken].tolist()
    inner = [i for i in range(1, len(own) - 1) if spoken[i] and own["teacher_frames"][i] >= 3]
    hit = max(inner, key=lambda i: (own["teacher_frames"][i], -i))
    other = [k for k in range(D - 1) if k not in own["phone"][hit - 1:hit + 2].tolist()][0]
    y = x.copy()
    lo, n = int(own["teacher_start"][hit]), int(own["teacher_frames"][hit])
    y[:, lo:lo + n] = ah.peaked([other] * n, D)
    rep, kept = align.phone_report(xt, [T], torch.from_numpy(y).cuda()[None], [T])
    rep = rep[0]
    print([(int(r["phone"]), int(r["teacher_start"]), int(r["teacher_frames"]), int(r["start"]), int(r["frames"]), int(r["kept"])) for r in rep])
    assert not rep["kept"][hit] and rep["share"][hit] == 0.0 and rep["gop"][hit] < -1.0 and int(rep["frames"].sum()) == T
    assert kept[0] == (spoken.sum() - 1 - sum(1 for i in (hit - 1, hit + 1) if spoken[i] and not rep["kept"][i])) / float(spoken.sum())
    far = np.abs(np.arange(len(rep)) - hit) > 1
    assert rep[far].tobytes() == own[far].tobytes()


def test_convert_scored_with_phones(world, mono, monkeypatch):
    from common.feat import WaveData
    from facppg import align
    from ppg.compute_ppg import compute_ppg_padded
    _cotenancy(monkeypatch)
    s, deps = mono["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])
    kw = dict(utterance_seeds=SEEDS, step_limits=list(FRAMES))
    audio, tout, plain = s.convert_scored(wd, deps, **kw)
    audio_p, tout_p, scores = s.convert_scored(wd, deps, phones=True, **kw)
    assert tout == tout_p and all(np.array_equal(a, b) for a, b in zip(audio, audio_p))
    assert sorted(plain) == sorted(KEYS) and sorted(scores) == sorted(KEYS + ("phones", "phones_kept"))
    assert _same({k: scores[k] for k in KEYS}, plain)
    # by hand: the front end's pass over the 2 B utterances, then phone_report over its two halves
    back = [WaveData(16000.0, torch.from_numpy(a).cuda().reshape(1, -1) * 32768.0) for a in audio]
    x, frames = compute_ppg_padded(list(wd) + back, deps, is_full_ppg=False)
    reports, kept = align.phone_report(x[:4], frames[:4], x[4:], frames[4:])
    assert _same_report(scores["phones"], reports) and scores["phones_kept"].tobytes() == kept.tobytes()
    assert ((kept >= 0) & (kept <= 1)).all()
    for rep, T in zip(reports, FRAMES):
        assert int(rep["frames"].sum()) in (0, T) and (rep["gop"] <= 0).all() and ((rep["share"] >= 0) & (rep["share"] <= 1)).all()
    # the report's own keywords: kept_share = 0 keeps whatever has a frame
    tuned, _ = align.phone_report(x[:4], frames[:4], x[4:], frames[4:], kept_share=0.0, switch_cost=0.5)
    assert all((t["kept"] == (t["frames"] > 0)).all() and int(t["frames"].sum()) in (0, T) for t, T in zip(tuned, FRAMES))


def test_synthesize_corpus_phone_file(world, corpus, mono, monkeypatch):
    """--wav_list --phone_file at world size 1: one line per teacher phone, the utterances in list order; the wavs and the
    --score_file of a run without the flag, byte for byte."""
    from common.feat import read_wav_kaldi
    from facppg import align, shard
    from script import synthesize_corpus
    _cotenancy(monkeypatch)
    tmp = world["tmp"]
    paths, listing = corpus
    common = ["--ppg2mel_model", mono["taco_path"], "--waveglow_model", mono["wg_path"], "--seed", "31", "--limit_steps_to_input",
              "--hparams", "n_symbols=40,is_full_ppg=False", "--batch_size", "3", "--wav_list", listing, "--nnet_path", world["nnet_path"],
              "--feats_dir", KF]
    names = ["train%d.wav" % i for i in range(4)]
    plain_scores, scores, phones = str(tmp / "ph_plain.tsv"), str(tmp / "ph_scores.tsv"), str(tmp / "ph_phones.tsv")
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "ph_plain"), "--score_file", plain_scores]) == names
    assert not os.path.exists(phones)
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "ph_phones"), "--score_file", scores, "--phone_file", phones,
                                            "--phone_table", PHONES]) == names
    for n in names:
        assert open(os.path.join(str(tmp), "ph_phones", n), "rb").read() == open(os.path.join(str(tmp), "ph_plain", n), "rb").read(), n
    assert open(scores, "rb").read() == open(plain_scores, "rb").read()
    table = align.read_phone_table(PHONES)
    lengths = synthesize_corpus.wav_ppg_lengths(paths)
    expected = {}
    for batch in shard.batches(shard.partition(lengths, 1)[0], lengths, 3):
        audio, _, sc = mono["synthesizer"].convert_scored([read_wav_kaldi(paths[i]) for i in batch], world["deps"], phones=True,
                                                          utterance_seeds=[31 + 2 * i for i in batch], step_limits=[lengths[i] for i in batch])
        for b, i in enumerate(batch):
            assert np.array_equal(audio[b], wavfile.read(os.path.join(str(tmp), "ph_phones", names[i]))[1]), i
            expected[i] = align.phone_lines(paths[i], sc["phones"][b], table)
    lines = open(phones).read().splitlines()
    print("\n".join(lines[:12]))
    assert lines == [l for i in range(4) for l in expected[i]]
    assert [l.split("\t")[0] for l in lines] == [paths[i] for i in range(4) for _ in expected[i]]       # list order
    for l in lines:
        f = l.split("\t")
        assert len(f) == 10 and f[2] in table and int(f[9]) in (0, 1) and float(f[7]) <= 0.0 and 0.0 <= float(f[8]) <= 1.0
