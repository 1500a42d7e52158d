"""``get_ppg`` hook of the reference's src/common/data_utils.py:55-59.

The reference computes the PPG of a wav with PyKaldi: features (ppg.compute_feat_for_nnet, built here on HIP kernels) ->
nnet3 acoustic model (data/am/final.raw, a blob the reference does not ship) -> posteriors.  With a model file present
(``deps.nnet``) the same chain runs here on the HIP kernels (ppg.compute_full_ppg_wrapper); without it this build reads a
precomputed PPG ([Tin, n_symbols] float array, 10 ms frame shift, rows = posteriors): either the
given path itself is a ``.npy`` file or a sibling ``<wav>.ppg.npy`` exists next to the wav.

``ppg_acoustics_collate`` is the reference's mini-batch collation (data_utils.py:281-334), what ``Tacotron2.parse_batch``
takes.  ``PPGMelLoader`` (data_utils.py:62-278) is out of scope: it extracts its PPGs with Kaldi.
"""
import os

import numpy as np
import torch


def ppg_candidates(wav_path):
    """Where the precomputed PPG of ``wav_path`` may live."""
    if wav_path.endswith(".npy"):
        return [wav_path]
    return [wav_path + ".ppg.npy", os.path.splitext(wav_path)[0] + ".ppg.npy"]


def get_ppg(wav_path, deps=None, is_fmllr=False):
    candidates = ppg_candidates(wav_path)
    for c in candidates:
        if os.path.isfile(c):
            ppg = np.load(c)
            if ppg.ndim != 2:
                raise ValueError("PPG file %s must hold a [Tin, n_symbols] array, got shape %s" % (c, ppg.shape))
            return ppg.astype(np.float32)
    if deps is not None and getattr(deps, "nnet", None) is not None and os.path.isfile(wav_path):
        # data_utils.py:55-59: wav -> features -> acoustic model -> full PPG, all on the HIP kernels
        from common import feat
        from ppg import compute_full_ppg_wrapper
        return compute_full_ppg_wrapper(feat.read_wav_kaldi(wav_path), deps.nnet, deps.lda, 10)
    raise NotImplementedError(
        "PPG extraction from audio needs the Kaldi nnet3 acoustic model (data/am/final.raw), which the reference does not ship; "
        "provide a precomputed PPG as %s (the model's input features are available: ppg.compute_feat_for_nnet)" % " or ".join(candidates))


def ppg_acoustics_collate(batch):
    """data_utils.py:281-334.  ``batch``: B pairs (PPG [L_in, n_symbols], acoustic [L_out, n_feat]) of tensors.  The
    utterances are sorted by PPG length, descending (pack_padded_sequence's order, which ``Tacotron2.forward`` demands),
    both sequences are right zero-padded to the longest and the gate target is 1 from each utterance's last frame on.
    Returns ppg_padded [B, n_symbols, max L_in], input_lengths [B], acoustic_padded [B, n_feat, max L_out],
    gate_padded [B, max L_out], output_lengths [B]."""
    input_lengths, order = torch.sort(torch.LongTensor([x[0].shape[0] for x in batch]), dim=0, descending=True)
    B = len(batch)
    ppg_padded = torch.zeros(B, int(input_lengths[0]), batch[0][0].shape[1])
    acoustic_padded = torch.zeros(B, max(x[1].shape[0] for x in batch), batch[0][1].shape[1])
    gate_padded = torch.zeros(B, acoustic_padded.shape[1])
    output_lengths = torch.zeros(B, dtype=torch.long)
    for i, j in enumerate(order.tolist()):
        ppg, acoustic = torch.as_tensor(batch[j][0]), torch.as_tensor(batch[j][1])
        ppg_padded[i, :ppg.shape[0]] = ppg
        acoustic_padded[i, :acoustic.shape[0]] = acoustic
        gate_padded[i, acoustic.shape[0] - 1:] = 1
        output_lengths[i] = acoustic.shape[0]
    return ppg_padded.transpose(1, 2), input_lengths, acoustic_padded.transpose(1, 2), gate_padded, output_lengths
