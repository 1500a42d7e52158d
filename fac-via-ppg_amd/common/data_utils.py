"""``get_ppg`` hook of the reference's src/common/data_utils.py:55-59.

The reference computes the PPG of a wav with PyKaldi: features (ppg.compute_feat_for_nnet, built here on HIP kernels) ->
nnet3 acoustic model (data/am/final.raw, a blob the reference does not ship) -> posteriors.  With a model file present
(``deps.nnet``) the same chain runs here on the HIP kernels (ppg.compute_full_ppg_wrapper); without it this build reads a
precomputed PPG ([Tin, n_symbols] float array, 10 ms frame shift, rows = posteriors): either the
given path itself is a ``.npy`` file or a sibling ``<wav>.ppg.npy`` exists next to the wav.

``ppg_acoustics_collate`` is the reference's mini-batch collation (data_utils.py:281-334), what ``Tacotron2.parse_batch``
takes.

``get_ppg_batch`` is ``get_ppg`` for a list of paths: the precomputed-file rule per path, and ONE pass of the batch front
end (ppg.compute_ppg_batch: the utterances laid end to end through the MFCC, CMN / splice / LDA and TDNN kernels) for the
paths that have no precomputed file.  ``PPGMelLoader`` (data_utils.py:163-278) is the reference's (PPG, mel) data set on top
of it, what ``script.train_ppg2mel.finetune`` trains from.

``append_ppg`` with ``compute_delta_acc_feat``, ``compute_dynamic_matrix``, ``compute_dynamic_vector`` (data_utils.py:62-160) are
the reference's F0 input columns in float64 NumPy; ``get_f0_batch`` supplies the track (``hparams.is_append_f0``).
"""
import os
import pickle
import random

import numpy as np
import torch
import torch.utils.data
from scipy.io import wavfile

from common.utils import load_filepaths


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


def _precomputed(wav_path):
    for c in ppg_candidates(wav_path):
        if os.path.isfile(c):
            return True
    return False


def get_ppg_batch(wav_paths, deps=None, is_full_ppg=True):
    """``get_ppg`` for a list of paths -> list of [Tin, n_symbols] float32 arrays, in the order given.  A path with a
    precomputed PPG file is read as ``get_ppg`` reads it; the others go through the batch front end together
    (ppg.compute_ppg_batch, one pass over all of them); a path with neither a file nor a model raises ``get_ppg``'s error.
    ``is_full_ppg=False`` returns monophone PPGs: computed ones come reduced out of the acoustic model's output kernel,
    precomputed senone PPGs go through ppg.reduce_ppg_dim."""
    wav_paths = list(wav_paths)
    out = [None] * len(wav_paths)
    todo = []
    for i, path in enumerate(wav_paths):
        if _precomputed(path) or deps is None or getattr(deps, "nnet", None) is None or not os.path.isfile(path):
            out[i] = get_ppg(path, deps)                 # the file, or get_ppg's error
        else:
            todo.append(i)
    trans = getattr(deps, "monophone_trans", None)
    if not is_full_ppg:
        if trans is None:
            raise ValueError("get_ppg_batch: monophone PPGs need deps.monophone_trans (data/feats/reduce_dim.mat)")
        for i, p in enumerate(out):
            if p is not None and p.shape[1] == trans.shape[1]:
                from ppg import reduce_ppg_dim
                out[i] = reduce_ppg_dim(p, trans).cpu().numpy()
    if todo:
        from common import feat
        from ppg import compute_ppg_batch
        ppgs = compute_ppg_batch([feat.read_wav_kaldi(wav_paths[i]) for i in todo], deps, is_full_ppg=is_full_ppg, shift=10)
        for i, p in zip(todo, ppgs):
            out[i] = p.cpu().numpy()
    return out


DELTA_WIN = [0, -0.5, 0.0, 0.5, 0]        # data_utils.py:48-52: dx(t) = 0.5 (x(t+1) - x(t-1)), five taps wide
ACC_WIN = [0.25, 0, -0.5, 0, 0.25]        # ddx(t) = 0.25 (x(t+2) - 2 x(t) + x(t-2))


def compute_dynamic_vector(vector, dynamic_win, frame_number):
    """data_utils.py:62-91: a [T] vector x a window of odd length -> [T, 1] float64, out[i] = sum_w win[w] * x[i + w - half]
    with the first / last value repeated beyond the ends; the products are added in the order of the window."""
    vector = np.asarray(vector, dtype=np.float64).reshape(frame_number)
    half = len(dynamic_win) // 2
    padded = np.concatenate([np.full(half, vector[0]), vector, np.full(half, vector[frame_number - 1])]) if frame_number else vector
    out = np.zeros(frame_number)
    for w, coeff in enumerate(dynamic_win):
        out += padded[w:w + frame_number] * coeff
    return out.reshape(frame_number, 1)


def compute_dynamic_matrix(data_matrix, dynamic_win):
    """data_utils.py:94-114: compute_dynamic_vector for every column of a [T, D] matrix -> [T, D] float64."""
    data_matrix = np.asarray(data_matrix, dtype=np.float64)
    frame_number, dimension = data_matrix.shape
    half = len(dynamic_win) // 2
    if frame_number == 0:
        return np.zeros((0, dimension))
    padded = np.concatenate([np.repeat(data_matrix[:1], half, 0), data_matrix, np.repeat(data_matrix[-1:], half, 0)], 0)
    out = np.zeros((frame_number, dimension))
    for w, coeff in enumerate(dynamic_win):
        out += padded[w:w + frame_number] * coeff
    return out


def compute_delta_acc_feat(matrix, is_delta=False, is_acc=False):
    """data_utils.py:117-139: [T, D] -> [T, D], [T, 2 D] (with the deltas) or [T, 3 D] (and the delta-deltas)."""
    if not is_delta and is_acc:
        raise ValueError('To use delta-delta feats you have to also use delta feats.')
    parts = [matrix]
    if is_delta:
        parts.append(compute_dynamic_matrix(matrix, DELTA_WIN))
    if is_acc:
        parts.append(compute_dynamic_matrix(matrix, ACC_WIN))
    return np.concatenate(parts, axis=1) if len(parts) > 1 else matrix


def append_ppg(feats, f0):
    """data_utils.py:142-160: feats [T1, D] and an F0 track [T2] (Hz, 0 = unvoiced) -> [min(T1, T2), D + 3]: the features, then
    log(f0 + eps) with its delta and delta-delta in float64 (WORLD's tracks are float64; a float32 track is widened first)."""
    frames = min(feats.shape[0], f0.shape[0])
    lf0 = np.log(np.asarray(f0[:frames], dtype=np.float64) + np.finfo(float).eps).reshape(frames, 1)
    return np.concatenate((feats[:frames, :], compute_delta_acc_feat(lf0, True, True)), axis=1)


def f0_candidates(wav_path):
    """Where the precomputed F0 track of ``wav_path`` may live."""
    return [wav_path + ".f0.npy", os.path.splitext(wav_path)[0] + ".f0.npy"]


def get_f0_batch(wav_paths, deps=None):
    """F0 tracks for a list of wav paths -> list of [T] float32 arrays in Hz, 0 = unvoiced, in the order given.  A precomputed
    ``<wav>.f0.npy`` / ``<stem>.f0.npy`` wins, as the ``.ppg.npy`` rule does -- that is how WORLD tracks (utterance.py:33-38) get
    in; the other paths go through ONE pass of the device tracker (ppg.compute_f0_batch), one value per PPG frame.  ``deps`` is
    accepted for symmetry with get_ppg_batch: the tracker needs no model."""
    wav_paths = list(wav_paths)
    out = [None] * len(wav_paths)
    todo = []
    for i, path in enumerate(wav_paths):
        for c in f0_candidates(path):
            if os.path.isfile(c):
                f0 = np.load(c)
                if f0.ndim != 1:
                    raise ValueError("F0 file %s must hold a [T] array in Hz, got shape %s" % (c, f0.shape))
                out[i] = f0.astype(np.float32)
                break
        else:
            todo.append(i)
    if todo:
        from common import feat
        from ppg import compute_f0_batch
        for i in todo:
            if not os.path.isfile(wav_paths[i]):
                raise FileNotFoundError("get_f0_batch: neither %s nor a precomputed track (%s)" % (wav_paths[i], " or ".join(f0_candidates(wav_paths[i]))))
        tracks = compute_f0_batch([feat.read_wav_kaldi(wav_paths[i]) for i in todo])
        for i, f in zip(todo, tracks):
            out[i] = f.cpu().numpy()
    return out


class PPGMelLoader(torch.utils.data.Dataset):
    """Loads [ppg, mel] pairs: the reference's data_utils.py:163-278.

    data_utterance_paths   a text file with one wav path per line (``load_filepaths``); the list is shuffled under
                           ``random.seed(hparams.seed)`` as the reference does, and the stored order is the shuffled one
    hparams                max_wav_value, sampling_rate, is_full_ppg, is_append_f0, is_cache_feats, load_feats_from_disk,
                           feats_cache_path, ppg_subsampling_factor, seed and the STFT's parameters
    ppg_deps               None builds ``DependenciesPPG()`` as the reference does
    batch_utterances       utterances extracted per pass of the batch front end (``get_ppg_batch``) and of the ragged
                           ``TacotronSTFT.mel_spectrogram``; within a pass they are sorted by length (the padding of the
                           mel batch stays small); the features do not depend on it beyond fp32 round-off

    The PPG side is the senone PPG (``is_full_ppg``) or the monophone PPG, reduced inside the acoustic model's output
    kernel; the acoustic side is the log-mel of ``audio / max_wav_value``, [T, n_mel].  With ``is_append_f0`` every PPG becomes
    ``append_ppg(ppg, f0)`` ([T, n_symbols + 3], data_utils.py:248-256) for either ``is_full_ppg`` setting; the reference reads
    ``utt.f0`` (WORLD), here the track is ``get_f0_batch``'s: a ``.f0.npy`` file next to the wav, else the device tracker -- the
    latter only for an utterance whose PPG the front end computes too (``_check_f0_sources``: otherwise NotImplementedError)."""

    def __init__(self, data_utterance_paths, hparams, ppg_deps=None, batch_utterances=32):
        self.data_utterance_paths = load_filepaths(data_utterance_paths)
        self.max_wav_value = hparams.max_wav_value
        self.sampling_rate = hparams.sampling_rate
        self.is_full_ppg = hparams.is_full_ppg
        self.is_append_f0 = hparams.is_append_f0
        self.is_cache_feats = hparams.is_cache_feats
        self.load_feats_from_disk = hparams.load_feats_from_disk
        self.feats_cache_path = hparams.feats_cache_path
        self.ppg_subsampling_factor = hparams.ppg_subsampling_factor
        self.batch_utterances = int(batch_utterances)
        if self.is_cache_feats and self.load_feats_from_disk:
            raise ValueError('If you are loading feats from the disk, do not rewrite them back!')
        if self.batch_utterances < 1:
            raise ValueError("PPGMelLoader: batch_utterances must be at least 1")
        if ppg_deps is None:
            from ppg import DependenciesPPG
            ppg_deps = DependenciesPPG()
        self.ppg_deps = ppg_deps
        if self.is_append_f0 and not self.load_feats_from_disk:
            self._check_f0_sources()

        from common import layers
        self.stft = layers.TacotronSTFT(hparams.filter_length, hparams.hop_length, hparams.win_length, hparams.n_acoustic_feat_dims,
                                        hparams.sampling_rate, hparams.mel_fmin, hparams.mel_fmax)
        random.seed(hparams.seed)
        random.shuffle(self.data_utterance_paths)

        self.ppg_sequences = []
        self.acoustic_sequences = []
        if self.load_feats_from_disk:
            print('Loading data from %s.' % self.feats_cache_path)
            with open(self.feats_cache_path, 'rb') as f:
                data = pickle.load(f)
            self.ppg_sequences = data[0]
            self.acoustic_sequences = data[1]
        else:
            for at in range(0, len(self.data_utterance_paths), self.batch_utterances):
                ppgs, mels = self.extract_batch_feats(self.data_utterance_paths[at:at + self.batch_utterances], self.is_full_ppg)
                self.ppg_sequences += [p.astype(np.float32) for p in ppgs]
                self.acoustic_sequences += mels
        if self.is_cache_feats:
            print('Caching data to %s.' % self.feats_cache_path)
            with open(self.feats_cache_path, 'wb') as f:
                pickle.dump([self.ppg_sequences, self.acoustic_sequences], f)

    def _check_f0_sources(self):
        """Host work, before any extraction.  The device tracker's frames are the front end's frames (one F0 frame meets one PPG
        frame), so its track is appended only to a PPG the front end computes in the same pass.  An utterance whose PPG comes from a
        file -- or all of them, when the dependencies hold no acoustic model -- carries a frame clock of its own, and needs its F0
        as a file as well (``<wav>.f0.npy``: a WORLD track next to a Kaldi PPG, as the reference pairs them)."""
        has_model = getattr(self.ppg_deps, "nnet", None) is not None
        for path in self.data_utterance_paths:
            if any(os.path.isfile(c) for c in f0_candidates(path)):
                continue
            if not has_model or _precomputed(path):
                raise NotImplementedError(
                    "PPGMelLoader: is_append_f0: %s has no precomputed F0 track (%s) and its PPG does not come from the front end "
                    "(%s); the device tracker's F0 is built only for PPGs the front end computes in the same pass"
                    % (path, " or ".join(f0_candidates(path)), "a precomputed PPG file" if _precomputed(path) else "no acoustic model"))

    def extract_batch_feats(self, paths, is_full_ppg=False):
        """extract_utterance_feats (data_utils.py:215-258) for a chunk of utterances: (PPGs, mels) in the order of ``paths``;
        PPG [Tin, n_symbols] numpy, mel [N // hop + 1, n_mel] CPU tensor."""
        audio = []
        for path in paths:
            fs, wav = wavfile.read(path)
            if fs != self.stft.sampling_rate:
                raise ValueError("{} SR doesn't match target {} SR".format(fs, self.stft.sampling_rate))
            audio.append((wav[:, 0] if wav.ndim == 2 else wav).astype(np.float32))
        order = sorted(range(len(paths)), key=lambda i: len(audio[i]))
        got = get_ppg_batch([paths[i] for i in order], self.ppg_deps, is_full_ppg=is_full_ppg)
        if self.is_append_f0:
            got = [append_ppg(p, f) for p, f in zip(got, get_f0_batch([paths[i] for i in order], self.ppg_deps))]
        hop = self.stft.stft_fn.hop_length
        padded = np.zeros((len(order), len(audio[order[-1]])), np.float32)
        for row, i in enumerate(order):
            padded[row, :len(audio[i])] = audio[i] / self.max_wav_value
        lengths = [len(audio[i]) for i in order]
        mel = self.stft.mel_spectrogram(torch.from_numpy(padded).cuda(), lengths)          # [B, n_mel, max N // hop + 1]
        ppgs, mels = [None] * len(paths), [None] * len(paths)
        for row, i in enumerate(order):
            ppgs[i] = got[row]
            mels[i] = mel[row, :, :lengths[row] // hop + 1].transpose(0, 1).contiguous().cpu()
        return ppgs, mels

    def extract_utterance_feats(self, data_utterance_path, is_full_ppg=False):
        """data_utils.py:215-258: [ppg, mel] of one utterance."""
        ppgs, mels = self.extract_batch_feats([data_utterance_path], is_full_ppg)
        return [ppgs[0], mels[0]]

    def __getitem__(self, index):
        """data_utils.py:260-275: (T*D1 PPG sequence, T*D2 mels) as float32 tensors."""
        if self.ppg_subsampling_factor == 1:
            curr_ppg = self.ppg_sequences[index]
        else:
            curr_ppg = self.ppg_sequences[index][0::self.ppg_subsampling_factor, :]
        return torch.from_numpy(curr_ppg), self.acoustic_sequences[index]

    def __len__(self):
        return len(self.ppg_sequences)


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
