"""Offline corpus synthesis sharded data-parallel over the GPUs of one node (BASELINE config 4).

No counterpart in the reference (its only multi-GPU code is WaveGlow training, distributed.py:145-170, whose
one-process-per-GPU launch pattern this follows); it is the utterance-batch scaling path named by
BASELINE.json's north_star.  Utterances are independent, so each rank synthesises a length-balanced shard
(facppg.shard.partition) with its own copy of the weights; the only exchanges are an all_gather of
(id, length) and one padded gather of the audio to rank 0, which writes the wavs.

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
      -m script.synthesize_corpus --ppg2mel_model taco.pt --waveglow_model wg.pt \
      --ppg_list ppgs.txt --output_dir out/ --batch_size 64

With ``--wav_list`` instead of ``--ppg_list`` the corpus is a list of teacher wavs (the reference's purpose: wav in,
converted wav out, generate_synthesis.py:60-98): each rank extracts the PPGs of its own shard through the batch front end
(common.data_utils.get_ppg_batch, ``--batch_size`` utterances per pass) and then synthesises as above.  With ``--device_ppgs``
as well, each batch's wavs are read, converted and dropped in turn: the front end runs in front of the batch's acoustic model
and hands its PPGs to the encoder on the device, so no PPG is ever held on the host.

With ``--score_file scores.tsv`` (and ``--wav_list``) every conversion is scored by its PPG round trip (facppg.score.roundtrip:
the converted audio back through the front end, aligned with the teacher's PPG on the device): each rank scores its own batches
and rank 0 writes one line per utterance, in list order.  The wavs do not depend on the flag.

With ``--phone_file phones.tsv`` (and ``--wav_list``) the same round trip also says, per phone of the teacher, where it landed in
the conversion (facppg.align.phone_report: the teacher's phone sequence decoded from its own PPG, the conversion force-aligned to
it): one line per teacher phone, the utterances in list order; ``--phone_table FILE`` (``name index`` lines, data/arpa_phonemes)
names the phones.  Neither the wavs nor the score file depend on the flag.
"""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist
from scipy.io import wavfile

from common.utils import load_filepaths
from facppg import shard

FS = 16000   # generate_synthesis.py:56


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ppg2mel_model', required=True)
    ap.add_argument('--waveglow_model', required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--ppg_list', help='text file, one precomputed PPG .npy path per line')
    src.add_argument('--wav_list', help='text file, one teacher wav per line: the PPGs are extracted here (acoustic model: --nnet_path '
                                        'and the files of --feats_dir; senone or monophone PPGs by the hparam is_full_ppg, with the three log-F0 columns by '
                                        'the hparam is_append_f0 -- set n_symbols to the PPG width + 3 with it)')
    ap.add_argument('--nnet_path', default=None, help='nnet3 acoustic model for --wav_list (default: data/am/final.raw)')
    ap.add_argument('--feats_dir', default=None, help='directory of final.mat, reduce_dim.mat and splice_opts for --wav_list '
                                                      '(default: data/feats)')
    ap.add_argument('--device_ppgs', action='store_true',
                    help="with --wav_list: read, convert and drop each batch's wavs in turn -- the front end of a batch runs in front of "
                         "its acoustic model and its PPGs go to the encoder on the device (facppg.pipeline.synthesize_stream's wavs "
                         "jobs): no PPG is ever held on the host (without the flag: all of a rank's shard, 4.6 MB per 2 s of senone PPG)")
    ap.add_argument('--output_dir', required=True)
    ap.add_argument('--batch_size', type=int, default=64,
                    help='utterances per synthesis batch; the latency-bound decoder costs the same for 16 or 96 utterances, so larger '
                         'batches are faster (one MI355X, 384 utterances: 7.8 / 8.2 / 8.7 / 8.9 M samples/s at 16 / 32 / 64 / 96); the '
                         'waveforms do not depend on it')
    ap.add_argument('--sigma', type=float, default=0.6)
    ap.add_argument('--denoiser_strength', type=float, default=0.005)
    ap.add_argument('--seed', type=int, default=0,
                    help='base seed: the dropout / noise streams of utterance i are keyed by seed + 2*i alone, so its wav '
                         'does not depend on the batch size, its place in a batch, or the number of GPUs')
    ap.add_argument('--limit_steps_to_input', action='store_true',
                    help='stop each utterance after as many mel frames as it has PPG frames at the latest '
                         '(per-utterance max_decoder_steps; both run at a 10 ms frame shift)')
    ap.add_argument('--no_overlap', action='store_true',
                    help='run the batches strictly one after the other instead of starting the acoustic model of the next batch '
                         'under the vocoder of the current one (same waveforms, slower)')
    ap.add_argument('--dist_backend', default='nccl', help='nccl = RCCL over xGMI (default); gloo for CPU tests')
    ap.add_argument('--vocoder_arithmetic', choices=('fp32', 'bf16x3'), default=None,
                    help="arithmetic of the vocoder's WaveGlow.infer: fp32 (exact, the default) or bf16x3 (fp32 operands split into two "
                         "bf16 terms on the bf16 MFMA: fp32-class accuracy, fp32 samples out)")
    ap.add_argument('--score_file', default=None,
                    help='with --wav_list: score every conversion by its PPG round trip (facppg.score.roundtrip) and write one line per '
                         'utterance, in list order: path, teacher_frames, roundtrip_frames, distance, agreement, stretch (tab separated, '
                         'floats as %%.6g)')
    ap.add_argument('--score_band', type=int, default=0,
                    help="--score_file: half-width of the alignment's slanted band in frames of the longer side (0: no band; otherwise "
                         "at least 2)")
    ap.add_argument('--phone_file', default=None,
                    help='with --wav_list: run the PPG round trip and write one line per phone of the teacher, utterances in list order: '
                         'path, index, phone, teacher_start, teacher_frames, start, frames, gop, share, kept (tab separated, frames of 10 ms, '
                         'start -1: the phone was skipped; facppg.align.phone_report)')
    ap.add_argument('--phone_table', default=None,
                    help='--phone_file: a table of `name index` lines (data/arpa_phonemes) that names the phones; without it their class numbers '
                         'are written')
    ap.add_argument('--hparams', default='',
                    help='comma separated "name=value" overrides of create_hparams_stage (train_ppg2mel.py:291-292), '
                         'e.g. n_symbols=40 for monophone PPGs (data_utils.py:253-258)')
    args = ap.parse_args(argv)
    if args.device_ppgs and not args.wav_list:
        ap.error("--device_ppgs goes with --wav_list: PPGs read with --ppg_list are on the host already")
    if args.score_file and not args.wav_list:
        ap.error("--score_file goes with --wav_list: with --ppg_list there is no teacher audio to compare the conversion with")
    if args.phone_file and not args.wav_list:
        ap.error("--phone_file goes with --wav_list: with --ppg_list there is no teacher audio to compare the conversion with")
    if args.phone_table and not args.phone_file:
        ap.error("--phone_table names the phones of --phone_file")
    if args.score_band < 0 or args.score_band == 1:
        ap.error("--score_band must be 0 (no band) or at least 2 (got %d)" % args.score_band)
    return args


def parse_hparams(text):
    """"a=1,b=x" -> create_hparams_stage(a=1, b='x'); values are cast to the type of the default they override."""
    from common.hparams import create_hparams_stage
    base = create_hparams_stage()
    kw = {}
    for item in filter(None, (t.strip() for t in text.split(','))):
        name, _, value = item.partition('=')
        if not hasattr(base, name):
            raise ValueError("unknown hparam %r" % name)          # same failure as hparams.py:233-237
        default = getattr(base, name)
        kw[name] = (value.lower() in ('1', 'true')) if isinstance(default, bool) else type(default)(value)
    return create_hparams_stage(**kw)


def wav_ppg_lengths(paths):
    """PPG frames each teacher wav will yield (10 ms shift at 16 kHz, Kaldi snip_edges = false), from the wav headers alone:
    what the shards are balanced by before any PPG exists."""
    from facppg import lib as _lib
    L = _lib.load()
    lengths = []
    for p in paths:
        fs, wav = wavfile.read(p, mmap=True)
        n = wav.shape[0] if fs == FS else L.facppg_resample_num_samples(wav.shape[0], int(fs), FS)
        lengths.append((n + FS // 200) // (FS // 100))
    return lengths


def ppg_dependencies(args):
    """The acoustic model and feature files of --wav_list (--nnet_path, --feats_dir)."""
    from ppg import compute_ppg
    feats_dir = args.feats_dir or os.path.dirname(compute_ppg.LDA_PATH)
    return compute_ppg.DependenciesPPG(nnet_path=args.nnet_path or compute_ppg.NNET_PATH, lda_path=os.path.join(feats_dir, "final.mat"),
                                       reduce_dim_path=os.path.join(feats_dir, "reduce_dim.mat"),
                                       splice_opts_path=os.path.join(feats_dir, "splice_opts"))


def extract_shard_ppgs(paths, mine, lengths, args, hparams):
    """{global id: PPG} of this rank's utterances, extracted ``args.batch_size`` at a time in batches of similar length.  With the
    hparam ``is_append_f0`` every PPG carries the three log-F0 columns (common.data_utils.append_ppg over get_f0_batch's track: a
    ``.f0.npy`` file next to the wav, else the device tracker)."""
    from common.data_utils import append_ppg, get_f0_batch, get_ppg_batch
    deps = ppg_dependencies(args)
    ppgs = {}
    for batch in shard.batches(mine, lengths, args.batch_size):
        got = get_ppg_batch([paths[i] for i in batch], deps, is_full_ppg=hparams.is_full_ppg)
        if hparams.is_append_f0:
            got = [append_ppg(p, f).astype(np.float32) for p, f in zip(got, get_f0_batch([paths[i] for i in batch], deps))]
        for i, p in zip(batch, got):
            ppgs[i] = p
    return ppgs


def synthesize_shard(synthesizer, ppgs, lengths, rank, world, args, wav_paths=None, ppg_deps=None, is_full_ppg=None, append_f0=False):
    """This rank's utterances, longest first, in batches of similar length.  Returns (waveforms, global ids).
    wav_paths (--device_ppgs) in place of ``ppgs``: every job carries the wavs of its batch, read when its acoustic model is
    enqueued -- the same batches extract_shard_ppgs forms, so the front end sees the same column space with and without the flag.
    append_f0 (the hparam is_append_f0): the front end appends the log-F0 rows of its own track on the device."""
    mine = shard.partition(lengths, world)[rank]
    batches = list(shard.batches(mine, lengths, args.batch_size))

    def source(batch):
        if wav_paths is None:
            return {"ppgs": [np.asarray(ppgs[i]) for i in batch]}
        from common.feat import read_wav_kaldi
        # a callable: the stream reads the batch on its acoustic stream, where the upload does not wait for the vocoder in front
        return {"wavs": lambda: [read_wav_kaldi(wav_paths[i]) for i in batch]}
    jobs = (dict(source(batch), utterance_seeds=[args.seed + 2 * i for i in batch],
                 step_limits=[lengths[i] for i in batch] if args.limit_steps_to_input else None) for batch in batches)
    wavs, ids = [], []
    if wav_paths is not None:
        if not hasattr(synthesizer, "stream"):
            raise ValueError("--device_ppgs needs a synthesizer with stream() (facppg.pipeline.Synthesizer)")
        results = synthesizer.stream(jobs, sigma=args.sigma, strength=args.denoiser_strength, return_device=True,
                                     overlap=not getattr(args, "no_overlap", False), ppg_deps=ppg_deps, is_full_ppg=is_full_ppg,
                                     **({"append_f0": True} if append_f0 else {}))
    elif hasattr(synthesizer, "stream"):      # software-pipelined: batch i+1's acoustic model runs under batch i's vocoder
        results = synthesizer.stream(jobs, sigma=args.sigma, strength=args.denoiser_strength, return_device=True,
                                     overlap=not getattr(args, "no_overlap", False))
    else:
        results = (synthesizer(return_device=True, sigma=args.sigma, strength=args.denoiser_strength, **job) for job in jobs)
    for batch, (out, _) in zip(batches, results):
        wavs += out
        ids += batch
    return wavs, ids


def score_shard(wavs, ids, paths, lengths, rank, world, args, deps):
    """({global id: one line of the score file}, {global id: the lines of the phone file}) for this rank's utterances: the teacher
    wavs of every batch synthesize_shard formed, read again, against that batch's converted audio (still on the device).  The
    second dict is empty without --phone_file."""
    from common.feat import read_wav_kaldi
    from facppg import align, score
    made = dict(zip(ids, wavs))
    names = align.read_phone_table(args.phone_table) if args.phone_table else None
    lines, phone_lines = {}, {}
    for batch in shard.batches(shard.partition(lengths, world)[rank], lengths, args.batch_size):
        scores = score.roundtrip([read_wav_kaldi(paths[i]) for i in batch], [made[i] for i in batch], FS, deps, band=args.score_band,
                                 phones=bool(args.phone_file))
        for b, i in enumerate(batch):
            lines[i] = score.score_line(paths[i], scores, b)
            if args.phone_file:
                phone_lines[i] = "\n".join(align.phone_lines(paths[i], scores["phones"][b], names))
    return lines, phone_lines


def collect_scores(lines, world):
    """Rank 0: {global id: line} of every rank; other ranks: None."""
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, lines)
        lines = {i: l for part in every for i, l in part.items()}
    return lines if int(os.environ.get("RANK", "0")) == 0 else None


def write_scores(score_file, n, lines):
    assert sorted(lines) == list(range(n)), "an utterance's score was lost or duplicated in the gather"
    with open(score_file, "w") as f:
        for i in range(n):
            f.write(lines[i] + "\n")


def collect(wavs, ids, world):
    """Rank 0: {global id: CPU waveform}; other ranks: None."""
    if world > 1:
        return shard.gather_ragged(wavs, ids, dst=0)
    return {i: w.detach().cpu() for i, w in zip(ids, wavs)}


def write_wavs(output_dir, paths, gathered):
    """<output_dir>/<ppg file stem>.wav, float32 [N, 1] at 16 kHz like the CLI's ac.wav (generate_synthesis.py:97-98)."""
    os.makedirs(output_dir, exist_ok=True)
    written = []
    for i, w in sorted(gathered.items()):
        name = os.path.splitext(os.path.basename(paths[i]))[0] + ".wav"
        wavfile.write(os.path.join(output_dir, name), FS, w.numpy().astype(np.float32)[:, None])
        written.append(name)
    return written


def main(argv=None, synthesizer=None):
    """``synthesizer``: a facppg.pipeline.Synthesizer-like callable; built from the two checkpoints when None
    (the CPU tests of the N>1 data path pass a stand-in, since the HIP path needs a GPU)."""
    args = parse(argv)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    on_gpu = args.dist_backend == "nccl"
    if on_gpu:
        torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if on_gpu:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    try:
        hparams = parse_hparams(args.hparams)
        if args.wav_list:
            paths = load_filepaths(args.wav_list)
            lengths = wav_ppg_lengths(paths)
            ppgs = None if args.device_ppgs else extract_shard_ppgs(paths, shard.partition(lengths, world)[rank], lengths, args, hparams)
        else:
            paths = load_filepaths(args.ppg_list)
            ppgs = [np.load(p, mmap_mode="r") for p in paths]
            lengths = [p.shape[0] for p in ppgs]
        if synthesizer is None:
            from facppg.pipeline import Synthesizer
            synthesizer = Synthesizer(args.ppg2mel_model, args.waveglow_model, hparams=hparams,
                                      vocoder_arithmetic=args.vocoder_arithmetic)
        if args.device_ppgs:
            wavs, ids = synthesize_shard(synthesizer, None, lengths, rank, world, args, wav_paths=paths, ppg_deps=ppg_dependencies(args),
                                         is_full_ppg=hparams.is_full_ppg, append_f0=bool(hparams.is_append_f0))
        else:
            wavs, ids = synthesize_shard(synthesizer, ppgs, lengths, rank, world, args)
        if args.score_file or args.phone_file:
            lines, phone_lines = score_shard(wavs, ids, paths, lengths, rank, world, args, ppg_dependencies(args))
            if args.score_file:            # (one gather per file that was asked for: a --score_file run exchanges what it always did)
                lines = collect_scores(lines, world)
            if args.phone_file:
                phone_lines = collect_scores(phone_lines, world)
        gathered = collect(wavs, ids, world)
        if rank == 0:
            assert sorted(gathered) == list(range(len(paths))), "an utterance was lost or duplicated in the gather"
            if args.score_file:
                write_scores(args.score_file, len(paths), lines)
            if args.phone_file:
                write_scores(args.phone_file, len(paths), phone_lines)
            return write_wavs(args.output_dir, paths, gathered)
        return None
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == '__main__':
    main()
