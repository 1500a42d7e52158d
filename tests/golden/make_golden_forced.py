#!/usr/bin/env python3
"""Generate the teacher-forced Tacotron fixtures (tests/golden/tacotron_forced_*.npz) by IMPORTING THE REFERENCE.

Runs only where the reference checkout exists (see make_golden.py, whose shims this script installs).  One more shim, its
own: the reference's ``get_mask_from_lengths`` (utils.py:39-43) returns a byte mask and ``Tacotron2.forward`` /
``parse_output`` apply ``~`` to it, a BITWISE not under today's torch; ``common.model.get_mask_from_lengths`` is replaced
by a bool version.  The reference's forward runs in eval mode with the prenets' always-on dropouts fed from the
``InjectDropout`` queue [enc0, enc1, dec0, dec1] (model.py:217, 462).

The files hold seeds, lengths, the reference's outputs and its loss only: weights and inputs are rebuilt from facppg.synth
(tests/forced_helpers.py::forced_case).

Usage:  python tests/golden/make_golden_forced.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from facppg import synth  # noqa: E402

CASES = (  # tag, n_symbols, input lengths (descending), target lengths, gate_bias
    ("ragged", 5816, (30, 22, 9), (37, 48, 12), -0.08),
    ("dup", 5816, (24, 24), (30, 30), -0.08),
    ("mono40", 40, (16, 16), (20, 20), -10.0),
)
ENC_MASK_SEED, DEC_MASK_SEED = 777, 778


def forced_inputs(n_sym, in_lens, out_lens, dup):
    """PPG of utterance b: synthetic_ppg(len, n_sym, seed=b), targets synthetic_mel(1, len, seed=100 + b), both zero-padded;
    gate targets 1 from the last frame on (data_utils.py:327).  ``dup``: every row is utterance 0 (row 0, under row 0's mask
    draws, is what a B = 1 call must return)."""
    B, Tin, T = len(in_lens), max(in_lens), max(out_lens)
    ppg = torch.zeros(B, n_sym, Tin)
    tgt = torch.zeros(B, 80, T)
    gate = torch.zeros(B, T)
    for b in range(B):
        s = 0 if dup else b
        ppg[b, :, :in_lens[b]] = torch.from_numpy(synth.synthetic_ppg(in_lens[b], n_sym, seed=s, alpha=0.002 if n_sym > 100 else 0.1)).float().t()
        tgt[b, :, :out_lens[b]] = synth.synthetic_mel(1, out_lens[b], seed=100 + s)[0]
        gate[b, out_lens[b] - 1:] = 1
    return ppg, tgt, gate


def gen_forced():
    from common import hparams as rh
    from common import model as rmodel
    from common.loss_function import Tacotron2Loss

    def bool_mask(lengths):
        max_len = int(torch.max(lengths).item())
        return torch.arange(0, max_len) < lengths.unsqueeze(1)
    rmodel.get_mask_from_lengths = bool_mask
    for tag, n_sym, in_lens, out_lens, gate_bias in CASES:
        hp = rh.create_hparams_stage(n_symbols=n_sym)
        m = rmodel.Tacotron2(hp)
        m.load_state_dict(synth.tacotron_state_dict(hp, seed=16807, gate_bias=gate_bias), strict=True)
        m.eval()
        B, Tin, T = len(in_lens), max(in_lens), max(out_lens)
        ppg, tgt, gate_t = forced_inputs(n_sym, in_lens, out_lens, tag == "dup")
        enc = mg.masks_from_seed(ENC_MASK_SEED, (2, B, Tin, hp.symbols_embedding_dim))
        dec = mg.masks_from_seed(DEC_MASK_SEED, (2, T + 1, B, hp.prenet_dim))
        il, ol = torch.LongTensor(in_lens), torch.LongTensor(out_lens)
        with torch.no_grad(), mg.InjectDropout(rmodel, [enc[0], enc[1], dec[0], dec[1]]) as inj:
            mel, mel_post, gate, align = m((ppg, il, tgt, Tin, ol))
            assert inj.i == 4
        with torch.no_grad(), mg.InjectDropout(rmodel, [enc[0], enc[1]]):
            memory = m.encoder(ppg, il)
        loss = Tacotron2Loss()([mel, mel_post, gate, align], (tgt.clone(), gate_t.clone()))
        print(tag, "loss %.6f" % float(loss), "mel", tuple(mel.shape), "align", tuple(align.shape))
        mg.save("tacotron_forced_%s.npz" % tag, n_symbols=n_sym, input_lengths=np.array(in_lens), output_lengths=np.array(out_lens),
                gate_bias=gate_bias, enc_mask_seed=ENC_MASK_SEED, dec_mask_seed=DEC_MASK_SEED, dup=int(tag == "dup"),
                ppg_sha=np.frombuffer(mg.sha(ppg.numpy()).encode(), dtype=np.uint8),
                memory=memory, mel=mel, mel_post=mel_post, gate=gate, align=align, loss=loss.double())


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mg.install_shims()
    gen_forced()
