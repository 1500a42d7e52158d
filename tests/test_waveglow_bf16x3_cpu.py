"""CPU: the host-side checks of WaveGlow.infer(arithmetic=...) (glow.py:252-293) -- the value is checked before any device work, the
combinations it does not go with are refused, the CLI flags parse, the binding declares the split entry points."""
import pytest
import torch

from facppg import lib as flib
from facppg import synth


def _cpu_model(hop=160):
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=4)
    return WaveGlow.remove_weightnorm(WaveGlow(**cfg)).eval(), cfg


def test_arithmetic_value_is_checked_before_any_device_work():
    m, _ = _cpu_model()
    mel = torch.zeros(1, 80, 4)           # a CPU tensor: a call that got as far as the device check would name it
    for bad in ("bf16", "BF16X3", "fp16", 3, ""):
        with pytest.raises(flib.FacppgError, match="arithmetic"):
            m.infer(mel, arithmetic=bad)
        with pytest.raises(flib.FacppgError, match="arithmetic"):
            m.last_launch_shape(bad)
        with pytest.raises(flib.FacppgError, match="arithmetic"):
            m.prepare(torch.device("cpu"), bad)
    for ok in (None, "fp32", "bf16x3"):   # accepted values reach the device check
        with pytest.raises(flib.FacppgError, match="must be a GPU tensor"):
            m.infer(mel, arithmetic=ok)
    assert "_facppg_handle" not in m.__dict__ and "_facppg_split_handle" not in m.__dict__


def test_bf16x3_refuses_groups_cond_first_and_half():
    m, _ = _cpu_model()
    mel = torch.zeros(2, 80, 4)
    with pytest.raises(flib.FacppgError, match="groups"):
        m.infer(mel, lengths=[4, 3], groups=2, arithmetic="bf16x3")
    with pytest.raises(flib.FacppgError, match="groups"):
        m.infer(mel, groups=1, arithmetic="bf16x3")
    with pytest.raises(flib.FacppgError, match="cond_first"):
        m.infer(mel, cond_first=True, arithmetic="bf16x3")
    with pytest.raises(flib.FacppgError, match="fp32 mel"):
        m.infer(mel.half(), arithmetic="bf16x3")
    m.half()
    for k in m.convinv:
        k.float()
    with pytest.raises(flib.FacppgError, match="all-fp32 module"):
        m.infer(mel.half(), arithmetic="bf16x3")
    with pytest.raises(flib.FacppgError, match="all-fp32 module"):
        m.infer(mel, arithmetic="bf16x3")


def test_handles_are_dropped_together_and_never_pickled():
    import pickle
    m, _ = _cpu_model()
    destroyed = []

    class _Lib(object):
        def facppg_wg_destroy(self, h):
            destroyed.append(("fp32", h))

        def facppg_wg_split_destroy(self, h):
            destroyed.append(("split", h))
    real = flib.load
    flib.load = lambda: _Lib()
    try:
        for drop in (m._release, lambda: m.load_state_dict(m.state_dict()), lambda: m.float(), lambda: m.train(False)):
            destroyed.clear()
            m.__dict__["_facppg_handle"] = ("H", None, None, torch.float32)
            m.__dict__["_facppg_split_handle"] = ("S", None, None)
            drop()
            assert sorted(destroyed) == [("fp32", "H"), ("split", "S")]
            assert "_facppg_handle" not in m.__dict__ and "_facppg_split_handle" not in m.__dict__
        m.__dict__["_facppg_split_handle"] = ("S", None, None)
        m._release(keep_split=True)
        assert m.__dict__["_facppg_split_handle"][0] == "S"
        state = m.__getstate__()
        assert "_facppg_split_handle" not in state and "_facppg_handle" not in state
        m.__dict__.pop("_facppg_split_handle")
        pickle.dumps(m)
    finally:
        flib.load = real


def test_pipeline_checks_vocoder_arithmetic_before_any_model_runs():
    from facppg import pipeline
    with pytest.raises(flib.FacppgError, match="vocoder_arithmetic"):
        pipeline.synthesize([], None, None, vocoder_arithmetic="bf16")
    with pytest.raises(flib.FacppgError, match="vocoder_arithmetic"):
        next(pipeline.synthesize_stream([], None, None, vocoder_arithmetic="half"))
    assert pipeline._checked_arithmetic("fp32") is None and pipeline._checked_arithmetic(None) is None
    assert pipeline._checked_arithmetic("bf16x3") == "bf16x3"


def test_cli_flags_parse():
    from script import synthesize_corpus
    from waveglow import inference
    base = ["-f", "list.txt", "-w", "wg.pt", "-o", "out"]
    assert inference.parse(base).arithmetic is None and not inference.parse(base).is_fp16
    assert inference.parse(base + ["--arithmetic", "bf16x3"]).arithmetic == "bf16x3"
    assert inference.parse(base + ["--arithmetic", "fp32"]).arithmetic == "fp32"
    assert inference.parse(base + ["--is_fp16"]).is_fp16
    with pytest.raises(SystemExit):
        inference.parse(base + ["--arithmetic", "bf16x3", "--is_fp16"])
    with pytest.raises(SystemExit):
        inference.parse(base + ["--arithmetic", "fp16"])
    with pytest.raises(ValueError, match="is_fp16"):
        inference.main("list.txt", "wg.pt", 1.0, "out", 22050, True, arithmetic="bf16x3")
    corpus = ["--ppg2mel_model", "a", "--waveglow_model", "b", "--ppg_list", "c", "--output_dir", "d"]
    assert synthesize_corpus.parse(corpus).vocoder_arithmetic is None
    assert synthesize_corpus.parse(corpus + ["--vocoder_arithmetic", "bf16x3"]).vocoder_arithmetic == "bf16x3"
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(corpus + ["--vocoder_arithmetic", "fp16"])


def test_generate_synthesis_keeps_the_reference_flags():
    import inspect
    from script import generate_synthesis
    src = inspect.getsource(generate_synthesis)
    assert "arithmetic" not in src


def test_binding_declares_the_split_entry_points():
    names = flib.exported_symbols()
    for n in ("facppg_wg_split_create", "facppg_wg_split_destroy", "facppg_wg_split_workspace_bytes", "facppg_wg_split_infer",
              "facppg_wg_split_last_launch_shape"):
        assert n in names
    L = flib.load()
    assert L.facppg_wg_split_workspace_bytes(None, 1, 1) == 0
    assert L.facppg_version() == 103
