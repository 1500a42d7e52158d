"""CPU: the wav -> wav surface that needs no device -- the header declares the padded entry point (test_abi_cpu.py then holds
the library to it), the argument errors of synthesize_wavs / Synthesizer.convert / the ``wavs`` jobs come before any device
work, and synthesize_corpus's parser knows where --device_ppgs belongs."""
import os
import re

import pytest

from conftest import ROOT


class _Taco(object):
    """As much of Tacotron2 as the argument checks read."""
    _hp = {"n_symbols": 40}


class _Deps(object):
    nnet = lda = monophone_trans = None


def _never(*a, **kw):
    raise AssertionError("device work was reached")


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the front end, the PPG upload, the models' parameters."""
    from facppg import pipeline
    from ppg import compute_ppg
    monkeypatch.setattr(compute_ppg, "compute_ppg_padded", _never)
    monkeypatch.setattr(compute_ppg, "_feat_for_nnet_flat", _never)
    monkeypatch.setattr(pipeline, "_synthesize", _never)
    monkeypatch.setattr(pipeline, "_acoustic", _never)


def test_header_declares_the_padded_entry_point():
    src = open(os.path.join(ROOT, "include", "facppg.h")).read()
    m = re.search(r"int\s+facppg_tdnn_forward_batch_padded\s*\(([^;]*)\)\s*;", src)
    assert m, "include/facppg.h does not declare facppg_tdnn_forward_batch_padded"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "feats_dev", "offsets_dev", "offsets_host", "B", "transform_t_dev", "M", "Tmax",
                                                         "out_dev", "workspace_dev", "ws_bytes", "stream"]
    from facppg import lib as flib
    assert "facppg_tdnn_forward_batch_padded" in flib.exported_symbols()
    assert flib.load().facppg_version() == 103


def test_synthesize_wavs_argument_errors_come_first(no_device):
    from facppg import pipeline
    from facppg.lib import FacppgError
    wav = object()
    with pytest.raises(FacppgError, match="both ppgs and wavs"):
        pipeline.synthesize_wavs([wav], _Deps(), _Taco(), None, ppgs=[object()])
    for empty in ([], (), None):
        with pytest.raises(FacppgError, match="non-empty list"):
            pipeline.synthesize_wavs(empty, _Deps(), _Taco(), None)
    with pytest.raises(FacppgError, match="no acoustic model"):
        pipeline.synthesize_wavs([wav], _Deps(), _Taco(), None)
    with pytest.raises(FacppgError, match="no PPG dependencies"):
        pipeline.synthesize_wavs([wav], None, _Taco(), None)
    with pytest.raises(TypeError, match="nonsense"):
        pipeline.synthesize_wavs([wav], _Deps(), _Taco(), None, nonsense=1)


def test_convert_argument_errors_come_first(no_device):
    from facppg import pipeline
    from facppg.lib import FacppgError
    s = pipeline.Synthesizer.__new__(pipeline.Synthesizer)        # (the constructor loads checkpoints onto the GPU)
    s.tacotron, s.waveglow, s.denoiser, s.vocoder_arithmetic, s.vocoder_stream = _Taco(), None, None, None, None
    wav = object()
    with pytest.raises(FacppgError, match="both ppgs and wavs"):
        s.convert([wav], _Deps(), ppgs=[object()])
    with pytest.raises(FacppgError, match="non-empty list"):
        s.convert([], _Deps())
    with pytest.raises(FacppgError, match="no acoustic model"):
        s.convert([wav], _Deps())


def test_device_ppgs_goes_with_wav_list(capsys):
    from script import synthesize_corpus
    base = ["--ppg2mel_model", "t.pt", "--waveglow_model", "w.pt", "--output_dir", "out"]
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(base + ["--ppg_list", "p.txt", "--device_ppgs"])
    assert "--device_ppgs goes with --wav_list" in capsys.readouterr().err
    args = synthesize_corpus.parse(base + ["--wav_list", "w.txt", "--device_ppgs"])
    assert args.device_ppgs and args.wav_list == "w.txt" and args.ppg_list is None
    assert not synthesize_corpus.parse(base + ["--wav_list", "w.txt"]).device_ppgs
    assert not synthesize_corpus.parse(base + ["--ppg_list", "p.txt"]).device_ppgs
