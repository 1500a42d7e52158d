"""Inputs of the tests/golden/tacotron_forced_<tag>.npz fixtures, rebuilt exactly as tests/golden/make_golden_forced.py
builds them (the files hold seeds, lengths and the reference's outputs only)."""
import torch

from helpers import golden, masks_from_seed


def forced_case(tag):
    """-> (fixture, hparams, state dict, ppg [B, n_sym, Tin], targets [B, 80, T], gate targets [B, T], enc masks
    [2, B, Tin, E], dec masks [2, T + 1, B, P]); lengths are the fixture's input_lengths / output_lengths."""
    from common.hparams import create_hparams_stage
    from facppg import synth
    d = golden("tacotron_forced_%s.npz" % tag)
    n_sym = int(d["n_symbols"])
    in_lens, out_lens = [int(v) for v in d["input_lengths"]], [int(v) for v in d["output_lengths"]]
    hp = create_hparams_stage(n_symbols=n_sym)
    sd = synth.tacotron_state_dict(hp, seed=16807, gate_bias=float(d["gate_bias"]))
    B, Tin, T = len(in_lens), max(in_lens), max(out_lens)
    ppg, tgt, gate = torch.zeros(B, n_sym, Tin), torch.zeros(B, 80, T), torch.zeros(B, T)
    for b, (ppg_b, tgt_b) in enumerate(forced_utterances(d)):
        ppg[b, :, :in_lens[b]] = ppg_b.t()
        tgt[b, :, :out_lens[b]] = tgt_b.t()
        gate[b, out_lens[b] - 1:] = 1
    enc = masks_from_seed(int(d["enc_mask_seed"]), (2, B, Tin, hp.symbols_embedding_dim))
    dec = masks_from_seed(int(d["dec_mask_seed"]), (2, T + 1, B, hp.prenet_dim))
    return d, hp, sd, ppg, tgt, gate, enc, dec


def forced_utterances(d):
    """The fixture's utterances as a data set yields them: (PPG [L_in, n_sym], acoustic [L_out, 80]) pairs, in the
    fixture's (length-sorted) order."""
    from facppg import synth
    n_sym = int(d["n_symbols"])
    out = []
    for b, (li, lo) in enumerate(zip(d["input_lengths"], d["output_lengths"])):
        s = 0 if int(d["dup"]) else b
        ppg = torch.from_numpy(synth.synthetic_ppg(int(li), n_sym, seed=s, alpha=0.002 if n_sym > 100 else 0.1)).float()
        out.append((ppg, synth.synthetic_mel(1, int(lo), seed=100 + s)[0].t().contiguous()))
    return out


def loss_tolerance(d, tgt, eps=1e-4, w_mel=1.0, w_gate=0.005):
    """How far Tacotron2Loss may move when mel, mel_post and the gate logits each move by at most eps from the fixture's:
    |dMSE| <= eps (2 mean|ref - target| + eps) per MSE term, and BCE-with-logits is 1-Lipschitz in the logits."""
    t = tgt.numpy()
    a = float(abs(d["mel"] - t).mean()) + float(abs(d["mel_post"] - t).mean())
    return w_mel * eps * (2 * a + 2 * eps) + w_gate * eps
