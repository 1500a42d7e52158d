"""wav -> monophone PPG for a corpus chunk: the batch front end (ppg.compute_ppg_batch, one pass over all utterances)
against the same utterances through the single-utterance calls, one after the other.

64 utterances (--utterances) of 1-4 s with the length law of config 3 (100 + PCG64(seed).integers(0, 301) frames of 10 ms),
synthetic 16 kHz wavs already on the GPU, a synthetic nnet3 TDNN of the reference's interface (40 -> hidden -> 5816 senones,
splices (-2..2), (-1, 2), (-3, 3), (0), renorm, softmax), the reference's LDA and pdf -> monophone map.  Both ways end in
[T, 40] monophone PPGs on the device; the time is the host clock around the calls and a device synchronise.  After a warm-up
of both, the two are timed in alternation, --reps rounds.  The outputs are compared (max abs difference over all frames).
Prints one JSON line; --out FILE also writes it there.  --once batch|single: one warmed pass of that path and nothing else
(for a kernel trace in a run of its own).

  python tools/time_ppg_batch.py [--utterances 64] [--hidden 512] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

KF = os.path.join(ROOT, "tests", "golden", "kaldi_feats")


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def synthetic_wav(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 16000.0
    x = 6000 * np.sin(2 * np.pi * 220 * t) + 2500 * np.sin(2 * np.pi * 1370 * t + 1.0) + 300 * g.standard_normal(n)
    return np.round(x).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", choices=("batch", "single"))
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    import ppg
    from common import feat, nnet3
    net = nnet3.synthetic_tdnn(input_dim=40, hidden=args.hidden, output_dim=5816, norm="renorm", seed=3, lda=False)
    with tempfile.TemporaryDirectory() as tmp:
        nnet3.write_nnet3(os.path.join(tmp, "final.raw"), net)
        deps = ppg.DependenciesPPG(nnet_path=os.path.join(tmp, "final.raw"), lda_path=os.path.join(KF, "final.mat"),
                                   reduce_dim_path=os.path.join(KF, "reduce_dim.mat"), splice_opts_path=os.path.join(KF, "splice_opts"))
    g = np.random.Generator(np.random.PCG64(args.seed))
    frames = (100 + g.integers(0, 301, size=args.utterances)).tolist()
    wavs = [feat.read_wav_kaldi_internal(synthetic_wav(160 * n, 900 + i), 16000) for i, n in enumerate(frames)]

    def batch():
        return ppg.compute_ppg_batch(wavs, deps, is_full_ppg=False)

    def single():
        return [ppg.reduce_ppg_dim(ppg.compute_full_ppg(deps.nnet, ppg.compute_feat_for_nnet_internal(w, deps.lda)), deps.monophone_trans)
                for w in wavs]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if args.once:
        fn = batch if args.once == "batch" else single
        timed(fn)
        print(json.dumps({"once": args.once, "ms": timed(fn)[0]}))
        return
    for _ in range(2):
        _, a = timed(batch)
        _, b = timed(single)
    diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
    assert [tuple(x.shape) for x in a] == [(n, 40) for n in frames]
    tb, ts = [], []
    for _ in range(args.reps):
        tb.append(timed(batch)[0])
        ts.append(timed(single)[0])
    res = {"workload": "wav -> monophone PPG, %d utterances of 1-4 s (%d frames, %.1f s of audio), TDNN hidden %d, 5816 senones" % (
               args.utterances, sum(frames), sum(frames) / 100.0, args.hidden),
           "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "batch": stats(tb), "single_calls": stats(ts), "speedup_median": statistics.median(ts) / statistics.median(tb),
           "max_abs_difference": diff}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
