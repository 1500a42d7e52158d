"""Score a PPG-to-Mel checkpoint on a list of utterances, teacher-forced AND the way it converts.

No counterpart in the reference, whose ``validate`` (train_ppg2mel.py:152-177) runs inside training only and is teacher-forced
only.  The decoder is used differently when it converts: it runs free, its prenet dropouts are on, and it can skip, repeat or
babble up to its step limit.  This prints the teacher-forced ``validate`` loss next to the free-running aggregates of
``script.train_ppg2mel.validate_free_running`` -- the mel-cepstral DTW distortion of the decoded mels against the targets
(facppg.score.mel_dtw: this build's own definition, values compare within this build only), the share of utterances the gate
stopped, the attention's coverage of the input -- and writes one line per utterance:

  python -m script.validate_ppg2mel --ppg2mel_model ckpt --wav_list val.txt [--hparams k=v,...] [--batch_size N] [--seed S]
      [--step_factor F] --out scores.tsv

The utterances come from ``common.data_utils.PPGMelLoader``: with ``--hparams load_feats_from_disk=True,feats_cache_path=FILE`` the
features are read from a cache file and no acoustic model is needed.  The lines are in the data set's order (the loader shuffles
the list under ``hparams.seed``, as the reference does): path, target_frames, frames, stopped, mcd, stretch, back, max_jump,
longest_stall, coverage, end_gap, focus (tab separated, floats as %.6g).
"""
import argparse

import torch

from script.synthesize_corpus import parse_hparams

SCORE_COLUMNS = ("target_frames", "frames", "stopped", "mcd", "stretch", "back", "max_jump", "longest_stall", "coverage", "end_gap", "focus")
_FLOATS = ("mcd", "stretch", "coverage", "focus")


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Teacher-forced and free-running validation of a PPG-to-Mel checkpoint.")
    ap.add_argument('--ppg2mel_model', required=True, help="a checkpoint of train_ppg2mel.save_checkpoint (its 'state_dict' is read)")
    ap.add_argument('--wav_list', required=True, help='text file, one wav path per line (PPGMelLoader)')
    ap.add_argument('--hparams', default='', help='comma separated "name=value" overrides of create_hparams_stage, e.g. '
                                                  'load_feats_from_disk=True,feats_cache_path=feats.pkl: no acoustic model is needed then')
    ap.add_argument('--batch_size', type=int, default=None, help='utterances per batch (default: hparams.batch_size)')
    ap.add_argument('--seed', type=int, default=0, help='utterance k is decoded with the dropout seed seed + k')
    ap.add_argument('--step_factor', type=float, default=None,
                    help='stop utterance k after ceil(step_factor * its target frames) frames at the latest (default: max_decoder_steps alone)')
    ap.add_argument('--out', required=True, help='the score file, one line per utterance')
    args = ap.parse_args(argv)
    if args.batch_size is not None and args.batch_size < 1:
        ap.error("--batch_size must be at least 1 (got %d)" % args.batch_size)
    if args.step_factor is not None and not args.step_factor > 0.0:
        ap.error("--step_factor must be positive (got %r)" % args.step_factor)
    return args


def score_line(path, result, k):
    """One line of --out: path, then SCORE_COLUMNS of utterance k (tabs; floats as %.6g, stopped as 0 / 1)."""
    return "\t".join([path] + ["%.6g" % float(result[c][k]) if c in _FLOATS else "%d" % int(result[c][k]) for c in SCORE_COLUMNS])


def main(argv=None):
    from common.data_utils import PPGMelLoader, ppg_acoustics_collate
    from common.loss_function import Tacotron2Loss
    from script.train_ppg2mel import load_model, validate, validate_free_running, warm_start_model
    args = parse(argv)
    hparams = parse_hparams(args.hparams)
    batch_size = hparams.batch_size if args.batch_size is None else args.batch_size
    valset = PPGMelLoader(args.wav_list, hparams)
    model = warm_start_model(args.ppg2mel_model, load_model(hparams)).eval()
    criterion = Tacotron2Loss(hparams.mel_weight, hparams.gate_weight)
    loss = validate(model, criterion, valset, 0, batch_size, 1, ppg_acoustics_collate, None, False, 0)
    model.eval()                                              # (validate leaves train() mode, as the reference does)
    result = validate_free_running(model, valset, batch_size, seed=args.seed, step_factor=args.step_factor)
    with open(args.out, "w") as f:
        for k in range(len(valset)):
            f.write(score_line(valset.data_utterance_paths[k], result, k) + "\n")
    print("Wrote %d lines to %s" % (len(valset), args.out))
    torch.cuda.synchronize()
    return loss, result


if __name__ == "__main__":
    main()
