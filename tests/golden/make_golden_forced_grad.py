#!/usr/bin/env python3
"""Generate the gradient fixtures of the teacher-forced pass (tests/golden/tacotron_forced_grad_<tag>.npz,
tests/golden/tacotron_finetune_ragged.npz) by IMPORTING THE REFERENCE.

Runs only where the reference checkout exists (see make_golden.py / make_golden_forced.py, whose shims and cases this script
uses).  For each case the reference's Tacotron2 runs in eval() with the prenet dropouts fed from ``InjectDropout``,
Tacotron2Loss, loss.backward() -- once in float64 and once in float32.  Full gradients are 76 MB, so per parameter tensor
(61) a file holds: the float64 gradient's norm, a strided sub-sample of it, and the float32 run's relative L2 deviation from
the float64 run on the whole tensor and on the sub-sample.  ``e32`` is the largest of those deviations: the unit every
tolerance of tests/test_gpu_tacotron_backward.py is expressed in.  The script asserts that the float32 reference itself
passes the comparison the tests make, with c = 1.

Usage:  python tests/golden/make_golden_forced_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_forced as mf  # noqa: E402
from facppg import synth  # noqa: E402

N_SUB = 256
FT_STEPS, FT_LR, FT_WD, FT_CLIP = 8, 1e-4, 1e-6, 1.0


def sub_index(n):
    """The strided sub-sample of a tensor of n values: at most N_SUB indices, the same rule in the tests."""
    return np.arange(0, n, max(1, n // N_SUB))[:N_SUB]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def build(rmodel, rh, tag, n_sym, gate_bias, dtype):
    hp = rh.create_hparams_stage(n_symbols=n_sym)
    m = rmodel.Tacotron2(hp)
    m.load_state_dict(synth.tacotron_state_dict(hp, seed=16807, gate_bias=gate_bias), strict=True)
    return hp, m.to(dtype).eval()


def run(rmodel, m, hp, ppg, tgt, gate_t, in_lens, out_lens, enc_seed, dec_seed, dtype):
    from common.loss_function import Tacotron2Loss
    B, Tin, T = len(in_lens), max(in_lens), max(out_lens)
    enc = mg.masks_from_seed(enc_seed, (2, B, Tin, hp.symbols_embedding_dim))
    dec = mg.masks_from_seed(dec_seed, (2, T + 1, B, hp.prenet_dim))
    il, ol = torch.LongTensor(in_lens), torch.LongTensor(out_lens)
    kept = {}

    def keep(_mod, _inp, out):
        out.retain_grad()
        kept["memory"] = out
    hook = m.encoder.register_forward_hook(keep)
    with mg.InjectDropout(rmodel, [enc[0], enc[1], dec[0], dec[1]]) as inj:
        out = m((ppg.to(dtype), il, tgt.to(dtype), Tin, ol))
        assert inj.i == 4
    hook.remove()
    loss = Tacotron2Loss()(out, (tgt.to(dtype).clone(), gate_t.to(dtype).clone()))
    loss.backward()
    return loss.detach().double(), kept["memory"].grad.double().numpy()


def gen_grad(rmodel, rh):
    e32_all = 0.0
    for tag, n_sym, in_lens, out_lens, gate_bias in mf.CASES:
        ppg, tgt, gate_t = mf.forced_inputs(n_sym, in_lens, out_lens, tag == "dup")
        res = {}
        for dtype in (torch.float64, torch.float32):
            hp, m = build(rmodel, rh, tag, n_sym, gate_bias, dtype)
            loss, dmem = run(rmodel, m, hp, ppg, tgt, gate_t, in_lens, out_lens, mf.ENC_MASK_SEED, mf.DEC_MASK_SEED, dtype)
            res[dtype] = (loss, dmem, [(n, p.grad.double().numpy().reshape(-1)) for n, p in m.named_parameters()])
        (l64, dm64, g64), (l32, dm32, g32) = res[torch.float64], res[torch.float32]
        assert len(g64) == 61
        names, norms, subs, dev_full, dev_sub, dev_norm = [], [], [], [], [], []
        for (n, a), (_, b) in zip(g64, g32):
            idx = sub_index(a.size)
            assert np.linalg.norm(a[idx]) > 0, n
            names.append(n)
            norms.append(np.linalg.norm(a))
            subs.append(np.pad(a[idx], (0, N_SUB - idx.size)))
            dev_full.append(rel(b, a))
            dev_sub.append(rel(b[idx], a[idx]))
            dev_norm.append(abs(np.linalg.norm(b) - np.linalg.norm(a)) / np.linalg.norm(a))
        e32 = max(max(dev_full), max(dev_sub))
        # the comparison of the tests, c = 1: norm and sub-sample of every tensor within e32
        assert max(dev_norm) <= e32 and max(dev_sub) <= e32
        e32_all = max(e32_all, e32)
        total = float(np.sqrt(sum(v * v for v in norms)))
        print(tag, "loss %.6f" % float(l64), "total norm %.3f" % total, "e32 %.2e" % e32, "median %.1e" % float(np.median(dev_full)),
              "worst", names[int(np.argmax(dev_full))])
        extra = {}
        if tag == "ragged":
            extra = dict(dmemory=dm64.astype(np.float32), dmemory_dev32=rel(dm32, dm64))
        mg.save("tacotron_forced_grad_%s.npz" % tag, names=np.array(names), norm=np.array(norms), sub=np.stack(subs),
                dev32_full=np.array(dev_full), dev32_sub=np.array(dev_sub), dev32_norm=np.array(dev_norm), e32=e32,
                loss=l64, loss32=l32, **extra)
    print("e32 over all cases %.2e" % e32_all)


def gen_finetune(rmodel, rh):
    tag, n_sym, in_lens, out_lens, gate_bias = mf.CASES[0]
    ppg, tgt, gate_t = mf.forced_inputs(n_sym, in_lens, out_lens, False)
    out = {}
    for dtype in (torch.float64, torch.float32):
        hp, m = build(rmodel, rh, tag, n_sym, gate_bias, dtype)
        opt = torch.optim.Adam(m.parameters(), lr=FT_LR, weight_decay=FT_WD)
        losses, norms = [], []
        for s in range(FT_STEPS):
            opt.zero_grad()
            loss, _ = run(rmodel, m, hp, ppg, tgt, gate_t, in_lens, out_lens, 1000 + s, 2000 + s, dtype)
            norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), FT_CLIP)))
            opt.step()
            losses.append(float(loss))
        out[dtype] = (np.array(losses), np.array(norms))
    (l64, n64), (l32, n32) = out[torch.float64], out[torch.float32]
    print("finetune losses", " ".join("%.2f" % v for v in l64), "fp32 vs fp64 %.2e" % float(np.max(np.abs(l32 - l64) / l64)))
    mg.save("tacotron_finetune_ragged.npz", loss=l64, loss32=l32, grad_norm=n64, grad_norm32=n32, steps=FT_STEPS,
            learning_rate=FT_LR, weight_decay=FT_WD, grad_clip_thresh=FT_CLIP, enc_seed0=1000, dec_seed0=2000,
            loss_dev32=float(np.max(np.abs(l32 - l64) / l64)))


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mg.install_shims()
    from common import hparams as rh
    from common import model as rmodel

    def bool_mask(lengths):
        max_len = int(torch.max(lengths).item())
        return torch.arange(0, max_len) < lengths.unsqueeze(1)
    rmodel.get_mask_from_lengths = bool_mask
    gen_grad(rmodel, rh)
    gen_finetune(rmodel, rh)
