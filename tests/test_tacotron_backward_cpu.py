"""CPU: what the backward pass of the teacher-forced Tacotron2.forward can show without a device -- the gradient fixtures
are self-consistent, the C ABI's new symbols exist, the refusals are in place, and the dense half of the backward pass
(common/taco_grad.py), run in float64 on torch stand-ins for the recurrent kernels, reproduces the reference's float64
gradients."""
import os
import re

import numpy as np
import pytest
import torch

import backward_helpers as bh
from conftest import ROOT
from forced_helpers import forced_case
from helpers import golden

NEW_SYMBOLS = ("facppg_taco_decode_forced_state", "facppg_taco_encode_state", "facppg_lstm_cell_scan", "facppg_lstm_backward",
               "facppg_lstm_backward_workspace_bytes", "facppg_taco_attention_backward",
               "facppg_taco_attention_backward_workspace_bytes")


@pytest.mark.parametrize("tag", bh.TAGS)
def test_gradient_fixture_is_self_consistent(tag):
    """61 tensors named as the model names them, non-zero sub-samples, and the reference's own float32 run passes the tests'
    comparison at C = 1."""
    from common.model import Tacotron2
    d, hp, _, _, _, _, _, _ = forced_case(tag)
    fix = bh.grad_fixture(tag)
    names = [n for n, _ in Tacotron2(hp).named_parameters()]
    assert [str(n) for n in fix["names"]] == names and len(names) == 61
    assert fix["sub"].shape == (61, bh.N_SUB) and np.all(fix["norm"] > 0)
    for i, (n, p) in enumerate(Tacotron2(hp).named_parameters()):
        k = bh.sub_index(p.numel()).size
        assert np.linalg.norm(fix["sub"][i][:k]) > 0 and np.all(fix["sub"][i][k:] == 0), n
    e32 = float(fix["e32"])
    assert e32 == max(fix["dev32_full"].max(), fix["dev32_sub"].max())
    assert fix["dev32_norm"].max() <= e32 and fix["dev32_sub"].max() <= e32            # C = 1
    assert 1e-7 < e32 < 1e-5
    assert abs(float(fix["loss"]) - float(d["loss"])) <= 1e-5 * float(d["loss"])        # the forward fixture's (float32) loss
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tacotron_forced_grad_%s.npz" % tag)) < 431 * 1024
    if tag == "ragged":
        assert fix["dmemory"].shape == d["memory"].shape and float(fix["dmemory_dev32"]) <= e32


def test_tolerance_is_capped():
    assert bh.C & (bh.C - 1) == 0 and bh.C_LOSS & (bh.C_LOSS - 1) == 0 and bh.tolerance() <= 1e-3


def test_finetune_fixture():
    fix = golden("tacotron_finetune_ragged.npz")
    assert fix["loss"].shape == (8,) and fix["grad_norm"].shape == (8,)
    assert np.all(np.diff(fix["loss"]) < 0)                                             # 39.98 -> 17.77
    assert float(fix["loss_dev32"]) == np.max(np.abs(fix["loss32"] - fix["loss"]) / fix["loss"]) < 1e-5
    assert bh.C_LOSS * float(fix["loss_dev32"]) <= bh.CAP


def test_header_declares_and_library_exports_the_backward_symbols():
    from facppg import lib as flib
    src = open(os.path.join(ROOT, "include", "facppg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(facppg_[a-z0-9_]+)\s*\(", src))
    L = flib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert hasattr(L, n), n
        assert n in flib.exported_symbols(), n
    assert L.facppg_version() == 103
    assert L.facppg_taco_attention_backward_workspace_bytes(None, 1, 1) == 0
    assert L.facppg_lstm_backward_workspace_bytes(0, 0) == 0
    from common.hparams import create_hparams_stage
    from common.model import Tacotron2
    cfg = Tacotron2(create_hparams_stage())._config()
    assert L.facppg_taco_attention_backward_workspace_bytes(cfg, 6, 200) >= 6 * 200 * (3 + 32) * 4
    assert L.facppg_lstm_backward_workspace_bytes(6, 1024) == 6 * 1024 * 4


def test_refusals():
    from common.hparams import create_hparams_stage
    from common.model import Tacotron2
    from facppg import lib as flib
    from script import train_ppg2mel
    hp = create_hparams_stage(n_symbols=40)
    m = Tacotron2(hp)
    x = (torch.zeros(1, 40, 4), torch.tensor([4]), torch.zeros(1, 80, 3), 4, torch.tensor([3]))
    with pytest.raises(flib.FacppgError, match="backward pass is not built"):       # training mode, whatever the keyword
        m(x, differentiable=True)
    with pytest.raises(flib.FacppgError, match="training mode"):
        m((None,) * 5)
    m.eval()
    with pytest.raises(flib.FacppgError, match="no CPU path"):
        m(x, differentiable=True)
    with torch.no_grad():
        with pytest.raises(flib.FacppgError, match="no_grad"):
            m(x, differentiable=True)
    with pytest.raises(NotImplementedError, match="not built"):
        train_ppg2mel.train("out", "log", None, False, 1, 0, "g", None)
    with pytest.raises(ValueError, match="must be on the GPU"):
        train_ppg2mel.finetune(m, hp, [], None, 1)
    hp.fp16_run = True
    with pytest.raises(NotImplementedError, match="fp16_run"):
        train_ppg2mel.finetune(m, hp, [], None, 1)


def test_dense_half_of_the_backward_pass_in_float64():
    """common.taco_grad.backward on the mono40 case, entirely on the CPU in float64: the recurrences as torch loops
    (backward_emulation.EmuRec: the recurrences the kernels of csrc/facppg_taco_bwd.hip compute, frame by frame), the states from a
    torch forward pass.  Every one of the 61 gradients then equals the reference's float64 gradient to 1e-9 -- far inside E32:
    the division of the backward pass into recurrences and dense local functions loses nothing."""
    from backward_emulation import EmuRec, torch_forward
    from common import taco_grad as tg
    from common.loss_function import Tacotron2Loss
    from common.model import Tacotron2
    d, hp, sd, ppg, tgt, gate_t, enc, dec = forced_case("mono40")
    fix = bh.grad_fixture("mono40")
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m = Tacotron2(hp)
        m.load_state_dict(sd)
        m.double().eval()
        ppg, tgt, gate_t = ppg.double(), tgt.double(), gate_t.double()
        B, _, Tin = ppg.shape
        T = tgt.shape[2]
        lens, olens = torch.tensor(d["input_lengths"]).long(), torch.tensor(d["output_lengths"]).long()
        st = tg.ForcedState()
        st.enc_masks = torch.from_numpy(enc).reshape(2, B, Tin, -1).permute(0, 1, 3, 2).contiguous()
        st.dec_masks = torch.from_numpy(dec)[:, :T].permute(0, 2, 3, 1).contiguous()
        st.memory, st.mel, gate, st.align, st.ah, st.dh = torch_forward(m, ppg, lens, tgt, st.enc_masks, st.dec_masks)
        st.ppg, st.lengths, st.lengths_dev, st.targets = ppg, lens, lens.int(), tgt
        st.pad = ~(torch.arange(T)[None] < olens[:, None])
        assert float((st.align - torch.from_numpy(d["align"])).abs().max()) < 1e-4
        with torch.no_grad():
            post = st.mel + tg.postnet(m, st.mel, None)
        leaves = [t.clone().requires_grad_(True) for t in (st.mel, post, gate)]
        outs = [leaves[0].masked_fill(st.pad.unsqueeze(1), 0.0), leaves[1].masked_fill(st.pad.unsqueeze(1), 0.0),
                leaves[2].masked_fill(st.pad, 1e3), st.align]
        loss = Tacotron2Loss()(outs, (tgt, gate_t))
        assert abs(float(loss.detach()) - float(fix["loss"])) <= 1e-9 * float(fix["loss"])
        loss.backward()
        grads, _ = tg.backward(m, st, leaves[0].grad, leaves[1].grad, leaves[2].grad, rec=EmuRec())
        dev = bh.deviations(fix, {n: g.numpy() for (n, _), g in zip(m.named_parameters(), grads)})
    finally:
        torch.set_default_dtype(old)
    worst = max(dev, key=lambda r: max(r[1], r[2]))
    print("float64 emulation: worst %s norm %.2e sub %.2e" % worst)
    assert len(dev) == 61 and max(worst[1], worst[2]) <= 1e-9
