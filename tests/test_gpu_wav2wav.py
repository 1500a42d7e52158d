"""GPU: wav in, wav out with the PPGs kept on the device (facppg.pipeline.synthesize_wavs, Synthesizer.convert, the ``wavs`` jobs
of synthesize_stream, script.synthesize_corpus --wav_list --device_ppgs) against the same calls over host copies of the PPGs.

Everything here is an equality of samples: the front end's posteriors reach the encoder where ppg.compute_ppg_padded left
them, and the stages behind are synthesize()'s.  The monophone PPGs are compute_ppg_batch's bit for bit (test_gpu_ppg_padded.py),
so the monophone tests compare with synthesize() over compute_ppg_batch's host copies; the senone posteriors sum their softmax in
another order, so the senone tests compare with synthesize() over host copies of the padded call's own values (what is under
test there is the plumbing).  Acoustic model, wavs (frames 1, 5, 37, 150) and corpus are test_gpu_ppg_batch.py's; the
checkpoints are the small synthetic ones of its test_synthesize_corpus_from_wavs, the streamed utterance runs on the models of
test_gpu_stream.py.  Seeds are fixed per utterance and every step limit is the utterance's input length."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from stream_helpers import acoustic, make_vocoder
from test_feat_cpu import KF
from test_gpu_ppg_batch import FRAMES, WAVS, _wave_data, corpus, world  # noqa: F401  (the module fixtures, built once for this file)

pytestmark = pytest.mark.gpu

SEEDS = [31, 33, 35, 37]


def _cotenancy(monkeypatch):
    """The decoder / BiLSTM modes test_synthesize_corpus_from_wavs runs its batches under (cooperative launches sized to run next
    to whatever else the pytest process holds on the GPU)."""
    monkeypatch.setenv("FACPPG_DECODER_MODE", "coop")
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "150")
    monkeypatch.setenv("FACPPG_BILSTM_MODE", "single")


def _host_rows(x, lens):
    """compute_ppg_padded's batch -> the host PPGs synthesize() takes: [T_b, D] each."""
    return [x[b, :, :T].t().contiguous().cpu().numpy() for b, T in enumerate(lens)]


@pytest.fixture(scope="module")
def mono(world):
    """Checkpoints of the monophone (n_symbols = 40) pair, as test_synthesize_corpus_from_wavs writes them, and their Synthesizer."""
    from common.hparams import create_hparams_stage
    from facppg import synth
    from facppg.pipeline import Synthesizer
    from waveglow.glow import WaveGlow
    from test_gpu_e2e import weightnorm_state_dict
    tmp = world["tmp"]
    cfg = dict(synth.WAVEGLOW_CONFIG)
    wg = WaveGlow(**cfg)
    wg.load_state_dict(weightnorm_state_dict(synth.waveglow_state_dict(cfg)), strict=True)
    torch.save({"model": wg, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, tmp / "w2w_waveglow.pt")
    hp = create_hparams_stage(n_symbols=40, is_full_ppg=False)
    torch.save({"state_dict": synth.tacotron_state_dict(hp, gate_bias=-10.0), "iteration": 0}, tmp / "w2w_tacotron.pt")
    return dict(taco_path=str(tmp / "w2w_tacotron.pt"), wg_path=str(tmp / "w2w_waveglow.pt"),
                synthesizer=Synthesizer(str(tmp / "w2w_tacotron.pt"), str(tmp / "w2w_waveglow.pt"), hparams=hp))


@pytest.fixture(scope="module")
def senone(world):
    """The senone (n_symbols = 5816) models of the streamed tests, the 150-frame utterance's padded posteriors on the host, and
    its unstreamed samples from synthesize() over them (FACPPG_STREAM=0): the reference of tests 6 and 7."""
    import ppg
    from facppg import pipeline
    cfg, wg, den = make_vocoder()
    hp, taco = acoustic(150, -10.0)
    wd = _wave_data(world["wavs"])
    x, lens = ppg.compute_ppg_padded(wd[3:], world["deps"])
    rows = _host_rows(x, lens)
    mp = pytest.MonkeyPatch()
    mp.setenv("FACPPG_STREAM", "0")
    try:
        ref, tout = pipeline.synthesize(rows, taco, wg, den, utterance_seeds=SEEDS[3:], step_limits=[150])
    finally:
        mp.undo()
    assert tout == [150]
    return dict(taco=taco, wg=wg, den=den, wd=wd, lone_rows=rows, lone_ref=ref[0])


def _spied(taco, call):
    """``call()`` with Tacotron2.inference watched, as stream_helpers.run watches it -> (result, what inference saw)."""
    seen = {}
    inference = taco.inference

    def spy(*a, **kw):
        out = inference(*a, **kw)
        consumer = kw.get("frame_consumer")
        seen["streamed"] = consumer is not None and consumer.active
        seen["published"] = bool(out.launch.streamed)
        seen["kind"] = kw.get("frame_consumer_arithmetic")
        return out
    taco.inference = spy
    try:
        return call(), seen
    finally:
        del taco.inference


def test_monophone_wavs_equal_synthesize_over_host_ppgs(world, mono, monkeypatch):
    """Test 5."""
    import ppg
    from facppg import pipeline
    _cotenancy(monkeypatch)
    s, deps = mono["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])
    kw = dict(utterance_seeds=SEEDS, step_limits=list(FRAMES))
    host = [p.cpu().numpy() for p in ppg.compute_ppg_batch(wd, deps, is_full_ppg=False)]
    ref, tout_ref = pipeline.synthesize(host, s.tacotron, s.waveglow, s.denoiser, **kw)
    out, tout = pipeline.synthesize_wavs(wd, deps, s.tacotron, s.waveglow, s.denoiser, **kw)       # is_full_ppg=None: by n_symbols
    assert tout == tout_ref == list(FRAMES) and len(out) == 4
    for b in range(4):
        assert out[b].dtype == np.float32 and out[b].shape == ref[b].shape == (FRAMES[b] * 160,) and np.isfinite(out[b]).all()
        assert np.array_equal(out[b], ref[b]), b
    conv, tout_c = s.convert(wd, deps, **kw)
    assert tout_c == tout and all(np.array_equal(a, r) for a, r in zip(conv, ref))
    # a width the model was not built for is refused before the front end runs
    with pytest.raises(pipeline_error(), match="5816 symbols, the PPG -> mel model was built for 40"):
        pipeline.synthesize_wavs(wd, deps, s.tacotron, s.waveglow, s.denoiser, is_full_ppg=True, **kw)


def pipeline_error():
    from facppg.lib import FacppgError
    return FacppgError


def test_senone_wavs_equal_synthesize_over_the_padded_posteriors(world, senone, monkeypatch):
    """Test 6: the batch of four, and the 150-frame utterance alone with the stream off."""
    import ppg
    from facppg import pipeline
    taco, wg, den, wd, deps = senone["taco"], senone["wg"], senone["den"], senone["wd"], world["deps"]
    monkeypatch.setenv("FACPPG_STREAM", "0")
    (lone,), tout = pipeline.synthesize_wavs(wd[3:], deps, taco, wg, den, is_full_ppg=True, utterance_seeds=SEEDS[3:], step_limits=[150])
    assert tout == [150] and lone.shape == (150 * 256,) and np.array_equal(lone, senone["lone_ref"])
    _cotenancy(monkeypatch)
    kw = dict(utterance_seeds=SEEDS, step_limits=list(FRAMES))
    x, lens = ppg.compute_ppg_padded(wd, deps)
    ref, tout_ref = pipeline.synthesize(_host_rows(x, lens), taco, wg, den, **kw)
    out, tout = pipeline.synthesize_wavs(wd, deps, taco, wg, den, **kw)
    assert tout == tout_ref == list(FRAMES)
    for b in range(4):
        assert out[b].shape == (FRAMES[b] * 256,) and np.isfinite(out[b]).all() and np.array_equal(out[b], ref[b]), b


def test_one_utterance_takes_the_streamed_paths(world, senone, monkeypatch):
    """Test 7: 150 frames through synthesize_wavs with the stream on -- streamed, and the samples of the unstreamed call (the
    equality test_gpu_stream.py establishes for synthesize()); then the split-bf16 opt-in call against itself on host PPGs."""
    from facppg import pipeline
    from facppg.pipeline import ConditioningStream
    taco, wg, den, wd, deps = senone["taco"], senone["wg"], senone["den"], senone["wd"], world["deps"]
    monkeypatch.setenv("FACPPG_STREAM", "1")
    monkeypatch.setenv("FACPPG_STREAM_MIN_FRAMES", "64")
    kw = dict(utterance_seeds=SEEDS[3:], step_limits=[150])
    (out, tout), seen = _spied(taco, lambda: pipeline.synthesize_wavs(wd[3:], deps, taco, wg, den, **kw))
    cs = wg.__dict__["_facppg_cond_stream"]
    print("fp32: streamed %s, published %s, blocks %s, seeded %d" % (seen["streamed"], seen["published"], cs.cuts, cs.seeded))
    assert seen["streamed"] and seen["published"] and seen["kind"] is None and not cs.split and cs.void_blocks == 0
    assert taco.last_decoder_launch()[0] == "split"
    assert tout == [150] and np.array_equal(out[0], senone["lone_ref"])
    split = dict(kw, vocoder_arithmetic="bf16x3", vocoder_stream=True)
    (ref, tout_ref), seen_ref = _spied(taco, lambda: pipeline.synthesize(senone["lone_rows"], taco, wg, den, **split))
    (out, tout), seen = _spied(taco, lambda: pipeline.synthesize_wavs(wd[3:], deps, taco, wg, den, **split))
    print("bf16x3: streamed %s / %s, seeded %d" % (seen_ref["streamed"], seen["streamed"], cs.seeded))
    assert seen_ref["streamed"] and seen["streamed"] and seen["kind"] == ConditioningStream.SPLIT and cs.split
    assert tout == tout_ref == [150] and np.array_equal(out[0], ref[0])
    assert not np.array_equal(out[0], senone["lone_ref"])            # (another arithmetic: the call really took it)


def test_stream_jobs_may_carry_wavs(world, mono, monkeypatch):
    """Test 8: two batches as ``wavs`` jobs against the same batches as ``ppgs`` jobs."""
    import ppg
    _cotenancy(monkeypatch)
    s, deps = mono["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])
    batches = [[0, 3], [1, 2]]
    meta = [dict(utterance_seeds=[SEEDS[i] for i in b], step_limits=[FRAMES[i] for i in b]) for b in batches]
    ppg_jobs = [dict(m, ppgs=[p.cpu().numpy() for p in ppg.compute_ppg_batch([wd[i] for i in b], deps, is_full_ppg=False)])
                for b, m in zip(batches, meta)]
    wav_jobs = [dict(m, wavs=[wd[i] for i in b]) for b, m in zip(batches, meta)]
    ref = list(s.stream(ppg_jobs))
    out = list(s.stream(wav_jobs, ppg_deps=deps))
    assert len(out) == len(ref) == 2
    for b, (o, t), (r, tr) in zip(batches, out, ref):
        assert t == tr == [FRAMES[i] for i in b]
        for a, c in zip(o, r):
            assert a.is_cuda and a.numel() > 0 and torch.equal(a, c)
    with pytest.raises(pipeline_error(), match="both ppgs and wavs"):
        list(s.stream([dict(wav_jobs[0], ppgs=ppg_jobs[0]["ppgs"])], ppg_deps=deps))
    # ``wavs`` as a callable (how synthesize_corpus --device_ppgs reads its batches): called once per job, with the stream of the
    # acoustic models current and not the caller's, on which the vocoder in front runs
    from common.feat import read_wav_kaldi_internal
    main, seen = torch.cuda.current_stream(), []

    def reader(b):
        def read():
            seen.append(torch.cuda.current_stream() != main)
            return [read_wav_kaldi_internal(world["wavs"][i].astype(np.float32), WAVS[i][1]) for i in b]
        return read
    lazy = list(s.stream([dict(m, wavs=reader(b)) for b, m in zip(batches, meta)], ppg_deps=deps))
    assert seen == [True, True]
    for (o, t), (r, tr) in zip(lazy, ref):
        assert t == tr and all(torch.equal(a, c) for a, c in zip(o, r))


def test_synthesize_corpus_device_ppgs(world, corpus, mono, monkeypatch):
    """Test 9: --wav_list --device_ppgs at world size 1 writes the files --wav_list writes."""
    from script import synthesize_corpus
    _cotenancy(monkeypatch)
    tmp = world["tmp"]
    paths, listing = corpus
    common = ["--ppg2mel_model", mono["taco_path"], "--waveglow_model", mono["wg_path"], "--seed", "31", "--limit_steps_to_input",
              "--hparams", "n_symbols=40,is_full_ppg=False", "--batch_size", "3", "--wav_list", listing, "--nnet_path", world["nnet_path"],
              "--feats_dir", KF]
    names = ["train%d.wav" % i for i in range(4)]
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "w2w_host")]) == names
    assert synthesize_corpus.main(common + ["--output_dir", str(tmp / "w2w_device"), "--device_ppgs"]) == names
    for i, p in enumerate(paths):
        n = wavfile.read(p)[1].shape[0]
        sr, a = wavfile.read(os.path.join(str(tmp), "w2w_device", names[i]))
        assert sr == 16000 and a.shape == (((n + 80) // 160) * 160,) and np.isfinite(a).all()
        assert np.array_equal(a, wavfile.read(os.path.join(str(tmp), "w2w_host", names[i]))[1]), i
