"""CPU: the kind table of WaveGlow's inference host side (waveglow.glow._KINDS: fp32, fp16, bf16x3) -- every entry point a row names
exists in the binding with the argument count its shared call site passes (a typo in a row otherwise shows only when that path
first runs on a device), the selector maps (arithmetic, module) to the kind or to the refusal, and seed_layout's public arity."""
import pytest
import torch

from facppg import lib as flib
from facppg import synth
from waveglow import glow

# arguments the ONE call site of each entry passes (WaveGlow._build, _release, _workspace, _infer_launch, _seed_layout, mel_pad /
# mel_convert, cond_seed, infer_seeded, last_launch_shape), written out from include/facppg.h
ARGS = {"create": 6, "destroy": 1, "workspace_bytes": 3, "infer": 12, "seed_layout": 5, "mel_pad": 9, "cond_seed": 15,
        "infer_seeded": 14, "last_launch_shape": 4}


def _model(n_flows=1):
    return glow.WaveGlow.remove_weightnorm(glow.WaveGlow(**dict(synth.WAVEGLOW_CONFIG, n_flows=n_flows))).eval()


def test_every_row_names_declared_entry_points_with_the_call_sites_argument_counts():
    assert [k.name for k in glow._KINDS.values()] == ["fp32", "fp16", "bf16x3"]
    assert glow._KINDS[torch.float32].name == "fp32" and glow._KINDS[torch.float16].name == "fp16" and glow._SPLIT.name == "bf16x3"
    sigs = flib._declare(flib.load())
    assert set(sigs) == set(flib.exported_symbols())
    for kind in glow._KINDS.values():
        want = dict(ARGS)
        want["infer"] += 1 if kind.takes_order else 0                      # the K order
        want["seed_layout"] += 1 if kind.max_block_tiles is None else 0    # max_block_tiles reported
        if not kind.mel_rows:
            want["mel_pad"] = 6                                            # the whole utterance, channel-major: no frame range, no skip flag
        for entry, n in want.items():
            name = getattr(kind, entry)
            assert name in sigs, (kind.name, entry, name)
            assert len(sigs[name][1]) == n, (kind.name, entry, name)
            assert kind.fn(entry) is not None
    # what the rows say about the kinds
    f32, f16, split = (glow._KINDS[k] for k in (torch.float32, torch.float16, "bf16x3"))
    assert f32.slot == f16.slot == "_facppg_handle" and split.slot == "_facppg_split_handle"
    assert (f32.ws_slot, f16.ws_slot, split.ws_slot) == (0, 0, "bf16x3")
    assert (f32.dtype, f16.dtype, split.dtype) == (torch.float32, torch.float16, torch.float32)
    assert (f32.mel_dtype, f16.mel_dtype, split.mel_dtype) == (torch.float32, torch.float16, torch.float32)
    assert (f32.mel_rows, f16.mel_rows, split.mel_rows) == (False, True, True) and f32.mel_pad == "facppg_wg_mel_pad"
    assert (f32.takes_order, f16.takes_order, split.takes_order) == (False, True, False)
    assert (f32.max_block_tiles, f16.max_block_tiles, split.max_block_tiles) == (4, 4, None)
    with pytest.raises(AttributeError):
        f32.name = "other"


def test_selector_maps_arithmetic_and_module_to_the_kind_or_the_refusal():
    fp32, half, mixed = _model(), _model().half(), _model().half()
    for k in half.convinv:
        k.float()                                   # the reference's recipe: convinv stays in float
    mixed.WN[0].in_layers[2].float()
    for arith in (None, "fp32"):
        assert fp32._kind("infer", arith) == (glow._KINDS[torch.float32], False)
        assert half._kind("infer", arith) == (glow._KINDS[torch.float16], False)
        with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
            mixed._kind("infer", arith)
    assert fp32._kind("infer", "bf16x3") == (glow._SPLIT, True)
    with pytest.raises(flib.FacppgError, match=r"WaveGlow\.cond_seed: arithmetic='bf16x3' splits fp32 operands: an all-fp32 module"):
        half._kind("cond_seed", "bf16x3")
    with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
        mixed._kind("infer", "bf16x3")
    for m in (fp32, half, mixed):
        for bad in ("bf16", "fp16", "BF16X3", 3, ""):
            with pytest.raises(flib.FacppgError, match="arithmetic=%r: expected None, 'fp32' or 'bf16x3'" % (bad,)):
                m._kind("infer", bad)
    # a handle passed in was built from an all-fp32 module: the split kind without a look at the parameters; the module's own kind
    # is the one its handle was built for (no walk), while that still is the upsampler's precision
    assert half._kind("cond_seed", "bf16x3", handle="H") == (glow._SPLIT, True)
    mixed.__dict__["_facppg_handle"] = ("H", None, None, torch.float16)
    try:
        assert mixed._kind("infer", None) == (glow._KINDS[torch.float16], False)
        mixed.upsample.float()
        with pytest.raises(flib.FacppgError, match="all fp32 or all fp16"):
            mixed._kind("infer", None)
    finally:
        mixed.__dict__.pop("_facppg_handle")
    # the resolver refuses a handle that is not the module's current one of the kind, in the kind's words
    with pytest.raises(flib.FacppgError, match="not this module's current one"):
        fp32._resolve("infer_seeded", None, "H", glow._KINDS[torch.float32])
    with pytest.raises(flib.FacppgError, match="not this module's current split-bf16 one"):
        fp32._resolve("infer_seeded", None, "H", glow._SPLIT)
    for m in (fp32, half, mixed):
        assert "_facppg_handle" not in m.__dict__ and "_facppg_split_handle" not in m.__dict__


def test_seed_layout_public_arity_per_kind():
    calls = []

    def layout(n_out):
        def fn(h, T, *out):
            assert len(out) == n_out
            calls.append((h, T, n_out))
            for o, v in zip(out, (96, 16, 4096, 3)):
                o._obj.value = v
            return 0
        return fn

    class _Lib(object):
        facppg_wg_seed_layout = staticmethod(layout(3))
        facppg_wg_seed_layout_f16 = staticmethod(layout(3))
        facppg_wg_split_seed_layout = staticmethod(layout(4))

        def facppg_wg_destroy(self, h):
            pass

        def facppg_wg_split_destroy(self, h):
            pass
    fp32, half = _model(), _model().half()
    ident = type("Same", (), {"unchanged": lambda self: True})()
    dev = torch.device("cpu")
    real = flib.load
    flib.load = lambda: _Lib()
    try:
        fp32.__dict__["_facppg_handle"] = ("H32", dev, ident, torch.float32)
        fp32.__dict__["_facppg_split_handle"] = ("HS", dev, ident)
        half.__dict__["_facppg_handle"] = ("H16", dev, ident, torch.float16)
        assert fp32.seed_layout(40, dev) == fp32.seed_layout(40, dev, arithmetic="fp32") == (96, 16, 4096)
        assert half.seed_layout(40, dev) == (96, 16, 4096)
        assert fp32.seed_layout(40, dev, arithmetic="bf16x3") == (96, 16, 4096, 3)
        # four values for every kind on request: the table's 4 where the query does not report the widest block
        assert fp32.seed_layout(40, dev, block_tiles=True) == half.seed_layout(40, dev, block_tiles=True) == (96, 16, 4096, 4)
        assert fp32.seed_layout(40, dev, arithmetic="bf16x3", block_tiles=True) == (96, 16, 4096, 3)
        assert [c[0] for c in calls] == ["H32", "H32", "H16", "HS", "H32", "H16", "HS"] and {c[1] for c in calls} == {40}
        with pytest.raises(flib.FacppgError, match="all-fp32 module"):
            half.seed_layout(40, dev, arithmetic="bf16x3")
        for m in (fp32, half):
            m._release()
    finally:
        flib.load = real
