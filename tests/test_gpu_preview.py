"""GPU: the vocoder-free preview above STFT.griffin_lim -- facppg.pipeline.preview, Synthesizer(ppg2mel, None).preview and
script.preview_ppg2mel -- on synthetic seeded weights (facppg.synth, monophone PPGs) and two ragged utterances of 30 and 50
input frames; preview_wavs / preview_scored on the front end's test wavs (test_gpu_ppg_batch.py) and the monophone Synthesizer
of test_gpu_wav2wav.py.  Everything is an equality of samples; the numerics are test_gpu_griffin_lim.py's."""
import contextlib
import io

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from facppg import synth
from test_gpu_ppg_batch import FRAMES, _wave_data, world  # noqa: F401  (the front end's module fixtures: acoustic model, wavs)
from test_gpu_wav2wav import SEEDS as WAV_SEEDS, mono  # noqa: F401  (the monophone checkpoints and their Synthesizer, vocoder loaded)

pytestmark = pytest.mark.gpu

TIN = (30, 50)
SEEDS = [41, 44]
KW = dict(n_iters=6, momentum=0.99)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from common.hparams import create_hparams_stage
    from common.layers import TacotronSTFT
    from script.train_ppg2mel import load_model
    tmp = tmp_path_factory.mktemp("preview")
    hp = create_hparams_stage(n_symbols=40, is_full_ppg=False)
    sd = synth.tacotron_state_dict(hp, gate_bias=-10.0)
    torch.save({"state_dict": sd, "iteration": 0}, tmp / "taco.pt")
    with contextlib.redirect_stdout(io.StringIO()):
        taco = load_model(hp)
    taco.load_state_dict(sd)
    taco.eval()
    stft = TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_acoustic_feat_dims, hp.sampling_rate, hp.mel_fmin,
                        hp.mel_fmax).cuda()
    ppgs = [synth.synthetic_ppg(t, 40, seed=60 + t, alpha=0.05) for t in TIN]
    return dict(tmp=tmp, hp=hp, taco=taco, stft=stft, ppgs=ppgs, path=str(tmp / "taco.pt"))


def _cotenancy(monkeypatch):
    """The decoder / BiLSTM modes the batched pipeline tests run under (cooperative launches sized to run next to whatever else
    the pytest process holds on the GPU)."""
    monkeypatch.setenv("FACPPG_DECODER_MODE", "coop")
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "150")
    monkeypatch.setenv("FACPPG_BILSTM_MODE", "single")


def test_preview_is_acoustic_plus_griffin_lim(models, monkeypatch):
    """pipeline.preview equals _acoustic followed by TacotronSTFT.griffin_lim written out here, bit for bit; each utterance
    equals its own batch-1 preview under utterance_seeds."""
    from facppg import pipeline
    _cotenancy(monkeypatch)
    taco, stft, ppgs, hop = models["taco"], models["stft"], models["ppgs"], models["hp"].hop_length
    kw = dict(KW, utterance_seeds=SEEDS, step_limits=list(TIN))
    out, tout = pipeline.preview(ppgs, taco, stft, **kw)
    assert tout == list(TIN) and len(out) == 2
    with torch.no_grad():
        mel, tout2 = pipeline._acoustic(ppgs, taco, None, None, SEEDS, list(TIN))
        ref = stft.griffin_lim(mel, lengths=tout2, utterance_seeds=[s + 2 for s in SEEDS], **KW)
    assert tout2 == tout
    for b, t in enumerate(tout):
        assert out[b].dtype == np.float32 and out[b].shape == ((t - 1) * hop,) and np.isfinite(out[b]).all() and out[b].any()
        assert np.array_equal(out[b], ref[b, 0, :(t - 1) * hop].cpu().numpy()), b
        (one,), t1 = pipeline.preview(ppgs[b:b + 1], taco, stft, **dict(KW, utterance_seeds=SEEDS[b:b + 1], step_limits=[TIN[b]]))
        assert t1 == [t] and np.array_equal(one, out[b]), b
    dev, _ = pipeline.preview(ppgs, taco, stft, return_device=True, **kw)
    assert all(d.is_cuda and np.array_equal(d.cpu().numpy(), o) for d, o in zip(dev, out))
    # one seed for the batch: reproducible, and another seed gives other phases
    a, _ = pipeline.preview(ppgs, taco, stft, seed=9, step_limits=list(TIN), **KW)
    b_, _ = pipeline.preview(ppgs, taco, stft, seed=9, step_limits=list(TIN), **KW)
    c, _ = pipeline.preview(ppgs, taco, stft, seed=10, step_limits=list(TIN), **KW)
    assert np.array_equal(a[0], b_[0]) and not np.array_equal(a[0], c[0])


def test_vocoderless_synthesizer_and_script(models, monkeypatch):
    """Synthesizer(ppg2mel, None).preview returns what preview returns on the same model; script.preview_ppg2mel writes the
    expected files with the expected lengths; the vocoder methods are refused."""
    from facppg import pipeline
    from facppg.lib import FacppgError
    from script import preview_ppg2mel
    _cotenancy(monkeypatch)
    hp, ppgs, tmp = models["hp"], models["ppgs"], models["tmp"]
    with contextlib.redirect_stdout(io.StringIO()):
        s = pipeline.Synthesizer(models["path"], None, hparams=hp)
    assert s.waveglow is None and s.denoiser is None
    kw = dict(KW, utterance_seeds=SEEDS, step_limits=list(TIN))
    ref, tout = pipeline.preview(ppgs, models["taco"], models["stft"], **kw)
    out, tout_s = s.preview(ppgs, **kw)
    assert tout_s == tout and all(np.array_equal(a, b) for a, b in zip(out, ref))
    with pytest.raises(FacppgError, match="preview"):
        s(ppgs)
    # the script: utterance i keyed by seed + 3 * i, step limit max_decoder_steps (the gate never closes on these weights)
    names = []
    for i, p in enumerate(ppgs):
        np.save(tmp / ("utt%d.npy" % i), p)
        names.append(str(tmp / ("utt%d.npy" % i)))
    (tmp / "ppgs.txt").write_text("\n".join(names) + "\n")
    steps = 40
    argv = ["--ppg2mel_model", models["path"], "--ppg_list", str(tmp / "ppgs.txt"), "--output_dir", str(tmp / "out"),
            "--hparams", "n_symbols=40,is_full_ppg=false,max_decoder_steps=%d" % steps, "--n_iters", "6", "--seed", "7", "--batch_size", "2"]
    with contextlib.redirect_stdout(io.StringIO()):
        written = preview_ppg2mel.main(argv)
    assert written == ["utt0.wav", "utt1.wav"]
    for name in written:
        fs, w = wavfile.read(tmp / "out" / name)
        # (written as [N, 1]; scipy reads a one-channel file back as [N])
        assert fs == hp.sampling_rate and w.dtype == np.float32 and w.reshape(-1).shape == ((steps - 1) * hp.hop_length,)
        assert np.isfinite(w).all() and w.any()


def test_preview_from_wavs_and_scored(world, mono, monkeypatch):
    """preview_wavs (PPGs kept on the device) equals preview over compute_ppg_batch's host copies of the same monophone PPGs, on a
    synthesizer that has its vocoder loaded; preview_scored is preview_wavs plus score.roundtrip; an utterance too short for
    reflect padding (hop * (frames - 1) <= filter_length / 2) is refused."""
    import ppg
    from facppg import pipeline, score
    from facppg.lib import FacppgError
    _cotenancy(monkeypatch)
    s, deps = mono["synthesizer"], world["deps"]
    wd = _wave_data(world["wavs"])[1:]                    # 5, 37 and 150 frames (the one-frame wav cannot be previewed)
    frames, seeds = list(FRAMES[1:]), WAV_SEEDS[1:]
    kw = dict(KW, utterance_seeds=seeds, step_limits=frames)
    host = [p.cpu().numpy() for p in ppg.compute_ppg_batch(wd, deps, is_full_ppg=False)]
    ref, tout_ref = pipeline.preview(host, s.tacotron, s.stft, **kw)
    out, tout = s.preview_wavs(wd, deps, **kw)
    assert tout == tout_ref == frames
    hop = s.hparams.hop_length
    for b, t in enumerate(frames):
        assert out[b].shape == ((t - 1) * hop,) and np.isfinite(out[b]).all() and np.array_equal(out[b], ref[b]), b
    audio, tout_s, scores = s.preview_scored(wd, deps, **kw)
    assert tout_s == frames and all(np.array_equal(a, r) for a, r in zip(audio, ref))
    by_hand = score.roundtrip(wd, ref, s.hparams.sampling_rate, deps)
    assert sorted(scores) == sorted(by_hand)
    for k in scores:
        assert np.array_equal(np.asarray(scores[k]), np.asarray(by_hand[k])), k
    assert scores["teacher_frames"].tolist() == frames
    with pytest.raises(FacppgError, match="2 frames|reflect padding"):
        s.preview_wavs(_wave_data(world["wavs"])[:1], deps, n_iters=2, utterance_seeds=[1], step_limits=[1])
