"""One long teacher recording -> converted wav: pipeline.synthesize_long_wavs against the conversion written by hand.

  long   common.feat.read_wav_kaldi(path) followed by pipeline.synthesize_long_wavs: the posteriors stay on the device, are cut
         there (flags, gather), converted as padded batches under synthesize_stream and joined there; one byte per frame and
         the samples visit the host
  hand   what a caller had to write before: common.data_utils.get_ppg_batch to the host, the same flags, cuts and groups with
         NumPy, pipeline.synthesize_stream over ``ppgs`` jobs of host slices, np.concatenate

The recording is --seconds (60) of seeded synthetic audio, 100 frames a second; --ppg senone | monophone picks the PPG -> mel
model (5816 or 40 symbols); the acoustic model (synthetic nnet3 TDNN, --hidden), the LDA, the pdf -> monophone map and the hop-256
vocoder are those of tools/time_wav2wav.py.  The stop gate is closed and limit_to_input is on: every segment runs to its input
length.  Both paths are called ALTERNATELY in one process, --reps (10) times each after --warmup (2) rounds; the time is the host
clock around one call, wav file to samples on the host.  Run it several times: a process is one sample of the clocks and
co-tenants it met.  Prints one JSON line; --out FILE appends it there.  --trace: three calls of ``long`` and nothing else (for a
kernel trace in a run of its own).

  python tools/time_longform.py --ppg senone [--seconds 60] [--hidden 512] [--reps 10] [--out FILE]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def synthetic_wav(np, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 16000.0
    x = 6000 * np.sin(2 * np.pi * 220 * t) + 2500 * np.sin(2 * np.pi * 1370 * t + 1.0) + 300 * g.standard_normal(n)
    return np.round(x).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ppg", choices=("senone", "monophone"), required=True)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path[:0] = [HERE, os.path.join(HERE, "fac-via-ppg_amd")]
    import numpy as np
    import torch
    from scipy.io import wavfile
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    import ppg
    from common import data_utils, feat, nnet3
    from common.hparams import create_hparams_stage
    from facppg import longform, pipeline, synth
    from script.train_ppg2mel import load_model
    from waveglow.denoiser import Denoiser
    from waveglow.glow import WaveGlow
    kf = os.path.join(HERE, "tests", "golden", "kaldi_feats")
    full = args.ppg == "senone"
    frames = 100 * args.seconds
    tmp = tempfile.TemporaryDirectory()
    net = nnet3.synthetic_tdnn(input_dim=40, hidden=args.hidden, output_dim=5816, norm="renorm", seed=3, lda=False)
    nnet3.write_nnet3(os.path.join(tmp.name, "final.raw"), net)
    deps = ppg.DependenciesPPG(nnet_path=os.path.join(tmp.name, "final.raw"), lda_path=os.path.join(kf, "final.mat"),
                               reduce_dim_path=os.path.join(kf, "reduce_dim.mat"), splice_opts_path=os.path.join(kf, "splice_opts"))
    path = os.path.join(tmp.name, "long.wav")
    wavfile.write(path, 16000, synthetic_wav(np, 160 * frames, 900))
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=256)
    wg = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    wg.load_state_dict(synth.waveglow_state_dict(cfg))
    wg = wg.cuda().eval()
    den = Denoiser(wg, hop_length=256, mode="zeros")
    hp = create_hparams_stage() if full else create_hparams_stage(n_symbols=40, is_full_ppg=False)
    with contextlib.redirect_stdout(io.StringIO()):
        taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    taco.eval()
    rows = [int(c) for c in torch.nonzero(deps.monophone_trans[39]).flatten()] if full else [39]
    plan = dict(max_frames=600, min_frames=150, min_pause=8)
    seed, threshold, batch_frames = 11, 0.5, 16 * 600

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def long():
        (wav,), (table,) = pipeline.synthesize_long_wavs([feat.read_wav_kaldi(path)], deps, taco, wg, den, seed=seed, limit_to_input=True,
                                                         pause_threshold=threshold, **plan)
        return wav, table

    def hand():
        (p,) = data_utils.get_ppg_batch([path], deps, is_full_ppg=full)
        mass = p[:, rows[0]].copy()
        for r in rows[1:]:
            mass = mass + p[:, r]
        segs = longform.plan_segments(mass > np.float32(threshold), **plan)
        jobs = [dict(ppgs=[p[a:a + n] for a, n in segs[i:j]], utterance_seeds=[seed + 2 * k for k in range(i, j)],
                     step_limits=[n for _, n in segs[i:j]]) for i, j in longform.group_segments([n for _, n in segs], batch_frames)]
        parts, tout = [], []
        for wavs, t in pipeline.synthesize_stream(jobs, taco, wg, den, return_device=False):
            parts += wavs
            tout += t
        return np.concatenate(parts), [(a, n, t) for (a, n), t in zip(segs, tout)]

    if args.trace:
        for _ in range(3):
            ms, (wav, table) = timed(long)
        print(json.dumps({"trace": args.ppg, "frames": frames, "segments": len(table), "last_call_ms": ms}))
        return
    for _ in range(args.warmup):
        _, (a, ta) = timed(long)
        _, (b, tb) = timed(hand)
    assert ta == tb and sum(t for _, _, t in ta) == frames and a.shape == b.shape == (256 * frames,) and np.isfinite(a).all()
    d = a.astype(np.float64) - b
    seam_free = float(np.sqrt((d * d).mean() / (b.astype(np.float64) ** 2).mean()))     # (the fades are all that differs)
    t_long, t_hand = [], []
    for _ in range(args.reps):
        t_long.append(timed(long)[0])
        t_hand.append(timed(hand)[0])
    res = {"workload": "one %d s recording (%d frames) -> wav, %s PPGs, %d segments %s, TDNN hidden %d, hop 256" % (
               args.seconds, frames, args.ppg, len(ta), [n for _, n, _ in ta], args.hidden),
           "device": torch.cuda.get_device_name(0), "pid": os.getpid(), "reps": args.reps, "alternating": True,
           "long": stats(t_long), "hand": stats(t_hand), "long_over_hand": statistics.median(t_long) / statistics.median(t_hand),
           "relative_rms_long_vs_hand": seam_free}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
