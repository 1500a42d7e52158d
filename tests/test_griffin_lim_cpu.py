"""CPU: the yardstick of the vocoder-free preview (tests/griffin_lim_helpers.py) held to the reference's own griffin_lim and to
the properties the device tests rely on, the pseudo-inverse of the mel basis, and the argument checks that need no device."""
import os

import numpy as np
import pytest

import griffin_lim_helpers as glh
from conftest import ROOT


def test_float64_restatement_reproduces_the_reference():
    """tests/golden/griffin_lim.npz holds what the reference's griffin_lim (audio_processing.py:91-107, float32 torch on its own
    STFT) made of M and the angles it drew.  The float64 restatement with alpha = 0 and those angles reproduces the signal within
    the float32 reference's own rounding: 4 x the float32 restatement's deviation from the float64 one on this case."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "griffin_lim.npz"))
    fl, hop, n = int(g["filter_length"]), int(g["hop_length"]), int(g["n_iters"])
    M, phi = g["M"].astype(np.float64), g["angles"].astype(np.float64)
    y64, _ = glh.griffin_lim(fl, hop, M, phi, n, 0.0, np.float64)
    y32, _ = glh.griffin_lim(fl, hop, M, phi, n, 0.0, np.float32)
    bar = 4.0 * glh.rel_err(y32, y64)
    err = glh.rel_err(g["signal"], y64)
    print("reference vs float64 restatement: %.3e (bar %.3e)" % (err, bar))
    assert g["signal"].shape == y64.shape == (hop * (M.shape[1] - 1),)
    assert err <= bar


@pytest.mark.parametrize("fl,hop,F", glh.SHAPES)
def test_fixed_point(fl, hop, F):
    """A consistent M with its true phases is a fixed point: the float64 restatement returns the signal after 3 iterations."""
    for seed in glh.SEEDS:
        y, M, _, phase = glh.case(fl, hop, F, seed)
        for alpha in glh.ALPHAS:
            out, sc = glh.griffin_lim(fl, hop, M, phase, 3, alpha, np.float64)
            assert np.max(np.abs(out - y)) <= 1e-12 and sc <= 1e-12, (seed, alpha, np.max(np.abs(out - y)), sc)


@pytest.mark.parametrize("fl,hop,F", glh.SHAPES)
def test_yardstick_converges(fl, hop, F):
    """float64 sc after 0, 4 and 32 iterations is strictly decreasing, for alpha = 0 and alpha = 0.99, on every case."""
    for seed in glh.SEEDS:
        _, M, phi0, _ = glh.case(fl, hop, F, seed)
        for alpha in glh.ALPHAS:
            sc = [glh.griffin_lim(fl, hop, M, phi0, n, alpha, np.float64)[1] for n in (0, 4, 32)]
            print(fl, hop, F, seed, alpha, ["%.4f" % v for v in sc])
            assert sc[0] == 1.0 and sc[0] > sc[1] > sc[2], (seed, alpha, sc)


def _bases():
    from common.layers import slaney_mel_basis
    return [slaney_mel_basis(16000, 1024, 80, 0.0, 8000.0), slaney_mel_basis(22050, 1024, 80, 0.0, 8000.0), glh.triangular_basis(20, 33)]


def test_pinv_of_the_mel_basis():
    """P . mel_basis . P = P to float64 rounding, and the inversion of a mel made from a magnitude reproduces that mel within
    1e-9 wherever nothing clamps: mel_basis . (P . E) = E."""
    for basis in _bases():
        P = glh.mel_pinv(basis)
        assert P.shape == basis.shape[::-1]
        assert np.max(np.abs(P @ basis @ P - P)) <= 1e-10 * np.max(np.abs(P))
        E = np.exp(glh.mel_case(basis, 7, 0).astype(np.float64))
        assert np.max(np.abs(basis @ (P @ E) - E)) <= 1e-9 * np.max(E)
        mag = glh.mel_to_magnitude(P, np.log(E), np.float64)
        clamped = float(np.mean(mag == 0.0))
        print("clamped share %.3f" % clamped)
        assert mag.min() >= 0.0 and 0.0 < clamped < 0.5


class _Taco(object):
    _hp = {"n_symbols": 40}

    def parameters(self):
        raise AssertionError("device work was reached")


def _vocoderless(monkeypatch, tmp_path):
    """Synthesizer(path, None) with the checkpoint loaders replaced: nothing touches a device."""
    import torch
    from common.hparams import create_hparams_stage
    from facppg import pipeline
    from script import train_ppg2mel

    class Model(torch.nn.Module):
        _hp = {"n_symbols": 40}

        def __init__(self):
            super(Model, self).__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    monkeypatch.setattr(train_ppg2mel, "load_model", lambda hp: Model())
    monkeypatch.setattr(torch, "load", lambda *a, **kw: {"state_dict": {"w": torch.zeros(1)}})
    return pipeline.Synthesizer(str(tmp_path / "taco.pt"), None, hparams=create_hparams_stage(n_symbols=40, is_full_ppg=False))


def test_synthesizer_without_a_vocoder(monkeypatch, tmp_path):
    """Synthesizer(path, None) is legal: no vocoder, no denoiser, a TacotronSTFT from its hparams; every method that needs the
    vocoder raises FacppgError naming preview, before any device work."""
    from common.layers import TacotronSTFT
    from facppg import pipeline
    from facppg.lib import FacppgError
    s = _vocoderless(monkeypatch, tmp_path)
    assert s.waveglow is None and s.denoiser is None and isinstance(s.stft, TacotronSTFT)
    assert s.stft.stft_fn.hop_length == s.hparams.hop_length and s.stft.n_mel_channels == s.hparams.n_acoustic_feat_dims

    def never(*a, **kw):
        raise AssertionError("device work was reached")
    for name in ("synthesize", "synthesize_wavs", "synthesize_stream", "synthesize_long_wavs", "_synthesize", "_acoustic"):
        monkeypatch.setattr(pipeline, name, never)
    wav = object()
    calls = {"__call__": lambda: s([np.zeros((4, 40), np.float32)]), "stream": lambda: s.stream([{"ppgs": []}]),
             "convert": lambda: s.convert([wav]), "convert_scored": lambda: s.convert_scored([wav]),
             "convert_file": lambda: s.convert_file("a.wav", "b.wav", 16000), "convert_long": lambda: s.convert_long([wav]),
             "convert_long_file": lambda: s.convert_long_file("a.wav", "b.wav", 16000),
             "synthesize_file": lambda: s.synthesize_file("a.npy", "b.wav", 16000)}
    for name, call in calls.items():
        with pytest.raises(FacppgError, match="preview"):
            call()
    # the preview methods check their arguments before any device work too
    with pytest.raises(FacppgError, match="non-empty list"):
        s.preview_wavs([])
    with pytest.raises(FacppgError, match="non-empty list"):
        s.preview_scored([])
    with pytest.raises(FacppgError, match="seed and utterance_seeds"):
        s.preview([np.zeros((4, 40), np.float32)], seed=1, utterance_seeds=[2])


def test_preview_ppg2mel_parse_errors(capsys):
    from script import preview_ppg2mel
    base = ["--ppg2mel_model", "t.pt", "--output_dir", "out"]
    for extra, msg in ((["--ppg_list", "p.txt", "--score_file", "s.tsv"], "--score_file goes with --wav_list"),
                       (["--ppg_list", "p.txt", "--n_iters", "-1"], "--n_iters must not be negative"),
                       (["--ppg_list", "p.txt", "--momentum", "1.0"], "--momentum must be in [0, 1)"),
                       (["--ppg_list", "p.txt", "--batch_size", "0"], "--batch_size must be positive"),
                       (["--ppg_list", "p.txt", "--wav_list", "w.txt"], "not allowed with"),
                       ([], "one of the arguments")):
        with pytest.raises(SystemExit):
            preview_ppg2mel.parse(base + extra)
        assert msg in capsys.readouterr().err
    args = preview_ppg2mel.parse(base + ["--wav_list", "w.txt", "--score_file", "s.tsv", "--seed", "5"])
    assert args.n_iters == 60 and args.momentum == 0.99 and args.seed == 5 and args.batch_size == 16 and args.score_file == "s.tsv"
