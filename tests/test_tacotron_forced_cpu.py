"""CPU: the parts of the teacher-forced pass that need no device -- Tacotron2Loss against the reference's stored loss,
ppg_acoustics_collate, the parse_output masking, the refusal to run on CPU tensors, and the C ABI's new symbols."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from forced_helpers import forced_case, forced_utterances
from helpers import golden

NEW_SYMBOLS = ("facppg_taco_encode_padded", "facppg_taco_decode_forced", "facppg_taco_decode_forced_workspace_bytes",
               "facppg_taco_draw_dropout_forced")


@pytest.mark.parametrize("tag", ["ragged", "dup", "mono40"])
def test_loss_reproduces_the_reference_loss(tag):
    from common.loss_function import Tacotron2Loss
    d, _, _, _, tgt, gate_t, _, _ = forced_case(tag)
    out = [torch.from_numpy(d[k]) for k in ("mel", "mel_post", "gate", "align")]
    loss = float(Tacotron2Loss()(out, (tgt, gate_t)).double())
    ref = float(d["loss"])
    print(tag, "loss %.8f reference %.8f" % (loss, ref))
    assert abs(loss - ref) <= 1e-6 * abs(ref)
    # the weights are the constructor's
    l2 = float(Tacotron2Loss(mel_weight=2, gate_weight=0)(out, (tgt, gate_t)).double())
    mse = float(((out[0] - tgt) ** 2).double().mean() + ((out[1] - tgt) ** 2).double().mean())
    assert abs(l2 - 2 * mse) <= 1e-5 * abs(l2)


def test_collate_sorts_pads_and_marks_the_gate():
    from common.data_utils import ppg_acoustics_collate
    d = golden("tacotron_forced_ragged.npz")
    utts = forced_utterances(d)                     # lengths 30/22/9 -> 37/48/12
    shuffled = [utts[2], utts[0], utts[1]]
    ppg, il, ac, gate, ol = ppg_acoustics_collate(shuffled)
    assert ppg.shape == (3, 5816, 30) and ac.shape == (3, 80, 48) and gate.shape == (3, 48)
    assert il.tolist() == [30, 22, 9] and ol.tolist() == [37, 48, 12] and il.dtype == torch.long and ol.dtype == torch.long
    _, _, _, ppg_ref, tgt_ref, gate_ref, _, _ = forced_case("ragged")
    assert torch.equal(ppg, ppg_ref) and torch.equal(ac, tgt_ref) and torch.equal(gate, gate_ref)
    for b, n in enumerate([37, 48, 12]):
        assert gate[b, :n - 1].sum() == 0 and bool((gate[b, n - 1:] == 1).all())
        assert float(ac[b, :, n:].abs().sum()) == 0.0


def test_parse_output_masks_as_the_reference():
    from common.hparams import create_hparams_stage
    from common.model import Tacotron2
    m = Tacotron2(create_hparams_stage(n_symbols=40))
    ol = torch.tensor([5, 3, 1])
    mk = lambda *s: torch.full(s, 2.5)
    mel, post, gate, al = m.parse_output([mk(3, 80, 5), mk(3, 80, 5), mk(3, 5), mk(3, 5, 7)], ol)
    for b, n in enumerate(ol.tolist()):
        assert bool((mel[b, :, :n] == 2.5).all()) and bool((mel[b, :, n:] == 0).all())
        assert bool((post[b, :, :n] == 2.5).all()) and bool((post[b, :, n:] == 0).all())
        assert bool((gate[b, :n] == 2.5).all()) and bool((gate[b, n:] == 1e3).all())
    assert bool((al == 2.5).all())                                   # alignments are returned unmasked
    out = m.parse_output([mk(3, 80, 5), mk(3, 80, 5), mk(3, 5), mk(3, 5, 7)])
    assert all(bool((t == 2.5).all()) for t in out)                  # no lengths (inference): untouched
    m.mask_padding = False
    out = m.parse_output([mk(3, 80, 5), mk(3, 80, 5), mk(3, 5), mk(3, 5, 7)], ol)
    assert all(bool((t == 2.5).all()) for t in out)


def test_forward_refuses_cpu_tensors_and_training_mode():
    from common.hparams import create_hparams_stage
    from common.model import Tacotron2
    from facppg import lib as flib
    m = Tacotron2(create_hparams_stage(n_symbols=40))
    x = (torch.zeros(1, 40, 4), torch.tensor([4]), torch.zeros(1, 80, 3), 4, torch.tensor([3]))
    with pytest.raises(flib.FacppgError, match="backward pass is not built"):
        m(x)                                          # a fresh module is in training mode
    m.eval()
    with pytest.raises(flib.FacppgError, match="no CPU path"):
        m(x)


def test_train_says_it_is_not_built():
    from script import train_ppg2mel
    with pytest.raises(NotImplementedError, match="not built"):
        train_ppg2mel.train("out", "log", None, False, 1, 0, "g", None)


def test_header_declares_and_library_exports_the_new_symbols():
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
    assert L.facppg_taco_decode_forced_workspace_bytes(None, 1, 1) == 0


def test_fixtures_pin_what_they_claim():
    """The ragged fixture reaches the 'last frame stays unmasked' quirk for its 9-frame utterance (decoder step 48 > 9 + 20)
    and carries masked padding; the dup fixture's two rows are the same utterance under different dropout draws."""
    d = golden("tacotron_forced_ragged.npz")
    al = d["align"]                                                  # [3, 48, 30]
    assert np.array_equal(al[2, 40] != 0, np.arange(30) == 8)        # only frame len - 1 = 8 keeps weight
    assert float(np.abs(d["mel"][2, :, 12:]).max()) == 0.0 and float(d["gate"][2, 12:].min()) == 1e3
    assert float(np.abs(d["mel"][0, :, 37:]).max()) == 0.0
    assert float(np.abs(d["mel"][1, :, 47]).max()) > 0.0         # the longest utterance is not masked anywhere
    d2 = golden("tacotron_forced_dup.npz")
    assert float(np.abs(d2["mel"][0] - d2["mel"][1]).max()) > 1e-3
