"""Listen to a PPG -> mel checkpoint without a vocoder: PPGs (or teacher wavs) -> mel -> Griffin-Lim on the device.

No counterpart in the reference.  The vocoder is trained per speaker and takes days, the PPG -> mel model minutes; until the
vocoder exists this writes waveforms for a checkpoint through facppg.pipeline.Synthesizer(ckpt, None).preview -- the mel
inverted to a linear magnitude by the pseudo-inverse of the mel basis, then Griffin-Lim with momentum as one device loop -- and,
with ``--score_file``, scores each of them by its PPG round trip (facppg.score.roundtrip), as synthesize_corpus does.

  python -m script.preview_ppg2mel --ppg2mel_model taco.pt --wav_list wavs.txt --output_dir out/ --score_file scores.tsv

The wavs are float32 [N, 1] at hparams.sampling_rate, named as script.synthesize_corpus names them (<stem>.wav).  Utterance i's
dropout and phase streams are keyed by seed + 3 * i alone, so its wav does not depend on the batch size or its place in a batch.
"""
import argparse
import os

import numpy as np
from scipy.io import wavfile

from common.utils import load_filepaths
from script.synthesize_corpus import parse_hparams, ppg_dependencies


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ppg2mel_model', required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--ppg_list', help='text file, one precomputed PPG .npy path per line')
    src.add_argument('--wav_list', help='text file, one teacher wav per line: the PPGs are extracted on the device (acoustic model: '
                                        '--nnet_path and the files of --feats_dir)')
    ap.add_argument('--nnet_path', default=None, help='nnet3 acoustic model for --wav_list (default: data/am/final.raw)')
    ap.add_argument('--feats_dir', default=None, help='directory of final.mat, reduce_dim.mat and splice_opts for --wav_list')
    ap.add_argument('--output_dir', required=True)
    ap.add_argument('--hparams', default='', help='comma separated "name=value" overrides of create_hparams_stage')
    ap.add_argument('--n_iters', type=int, default=60, help='Griffin-Lim iterations')
    ap.add_argument('--momentum', type=float, default=0.99, help='Griffin-Lim momentum, 0 <= momentum < 1 (0: the plain iteration)')
    ap.add_argument('--seed', type=int, default=0, help='base seed: utterance i is keyed by seed + 3*i alone')
    ap.add_argument('--batch_size', type=int, default=16, help='utterances per batch; the waveforms do not depend on it')
    ap.add_argument('--score_file', default=None,
                    help='with --wav_list: score every preview by its PPG round trip and write one line per utterance, in list order '
                         '(the columns of script.synthesize_corpus --score_file)')
    args = ap.parse_args(argv)
    if args.score_file and not args.wav_list:
        ap.error("--score_file goes with --wav_list: with --ppg_list there is no teacher audio to compare the preview with")
    if args.n_iters < 0:
        ap.error("--n_iters must not be negative (got %d)" % args.n_iters)
    if not 0.0 <= args.momentum < 1.0:
        ap.error("--momentum must be in [0, 1) (got %g)" % args.momentum)
    if args.batch_size < 1:
        ap.error("--batch_size must be positive (got %d)" % args.batch_size)
    return args


def main(argv=None, synthesizer=None):
    """``synthesizer``: a facppg.pipeline.Synthesizer (built from the checkpoint, without a vocoder, when None).  Returns the
    names of the files written."""
    args = parse(argv)
    hparams = parse_hparams(args.hparams)
    if synthesizer is None:
        from facppg.pipeline import Synthesizer
        synthesizer = Synthesizer(args.ppg2mel_model, None, hparams=hparams)
    paths = load_filepaths(args.wav_list or args.ppg_list)
    deps = ppg_dependencies(args) if args.wav_list else None
    os.makedirs(args.output_dir, exist_ok=True)
    written, lines = [], []
    for lo in range(0, len(paths), args.batch_size):
        ids = list(range(lo, min(lo + args.batch_size, len(paths))))
        kw = dict(n_iters=args.n_iters, momentum=args.momentum, utterance_seeds=[args.seed + 3 * i for i in ids])
        if args.wav_list:
            from common.feat import read_wav_kaldi
            wavs = [read_wav_kaldi(paths[i]) for i in ids]
            if args.score_file:
                from facppg import score
                audio, _, scores = synthesizer.preview_scored(wavs, deps, **kw)
                lines += [score.score_line(paths[i], scores, b) for b, i in enumerate(ids)]
            else:
                audio, _ = synthesizer.preview_wavs(wavs, deps, **kw)
        else:
            audio, _ = synthesizer.preview([np.load(paths[i]) for i in ids], **kw)
        for i, w in zip(ids, audio):
            name = os.path.splitext(os.path.basename(paths[i]))[0] + ".wav"
            wavfile.write(os.path.join(args.output_dir, name), hparams.sampling_rate, np.asarray(w, dtype=np.float32)[:, None])
            written.append(name)
    if args.score_file:
        with open(args.score_file, "w") as f:
            for line in lines:
                f.write(line + "\n")
    return written


if __name__ == '__main__':
    main()
