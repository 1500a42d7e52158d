"""What the F0 pass costs next to the front end it joins: ppg.compute_ppg_padded with and without ``append_f0``, and
ppg.compute_f0_batch alone, over the 64 utterances of 1-4 s of tools/time_ppg_batch.py (same length law, wavs, synthetic TDNN,
monophone PPGs).  The time is the host clock around a call and a device synchronise; inside one process the variants are timed
in alternation after a warm-up of each, and the driver runs --processes fresh processes.  With --parent DIR (a built checkout of
the parent commit) its compute_ppg_padded is timed in processes of its own, alternating with this tree's: the plain call must not
have become slower.

  python tools/time_f0.py [--processes 3] [--reps 20] [--parent DIR] [--out profiles/r22_f0_timing.json]
  python tools/time_f0.py --once f0|padded|padded_f0      one warmed pass and nothing else (for a kernel trace)
"""
import argparse
import inspect
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def worker(args):
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "fac-via-ppg_amd")]
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    import ppg
    from common import feat, nnet3
    kf = os.path.join(root, "tests", "golden", "kaldi_feats")

    def synthetic_wav(n, seed):
        g = np.random.Generator(np.random.PCG64(seed))
        t = np.arange(n) / 16000.0
        x = 6000 * np.sin(2 * np.pi * 220 * t) + 2500 * np.sin(2 * np.pi * 1370 * t + 1.0) + 300 * g.standard_normal(n)
        return np.round(x).astype(np.float32)
    net = nnet3.synthetic_tdnn(input_dim=40, hidden=args.hidden, output_dim=5816, norm="renorm", seed=3, lda=False)
    with tempfile.TemporaryDirectory() as tmp:
        nnet3.write_nnet3(os.path.join(tmp, "final.raw"), net)
        deps = ppg.DependenciesPPG(nnet_path=os.path.join(tmp, "final.raw"), lda_path=os.path.join(kf, "final.mat"),
                                   reduce_dim_path=os.path.join(kf, "reduce_dim.mat"), splice_opts_path=os.path.join(kf, "splice_opts"))
    g = np.random.Generator(np.random.PCG64(args.seed))
    frames = (100 + g.integers(0, 301, size=args.utterances)).tolist()
    wavs = [feat.read_wav_kaldi_internal(synthetic_wav(160 * n, 900 + i), 16000) for i, n in enumerate(frames)]
    has_f0 = "append_f0" in inspect.signature(ppg.compute_ppg_padded).parameters
    calls = {"padded": lambda: ppg.compute_ppg_padded(wavs, deps, is_full_ppg=False)}
    if has_f0:
        calls["padded_f0"] = lambda: ppg.compute_ppg_padded(wavs, deps, is_full_ppg=False, append_f0=True)
        calls["f0"] = lambda: ppg.compute_f0_batch(wavs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    if args.once:
        timed(calls[args.once])
        print(json.dumps({"once": args.once, "ms": timed(calls[args.once])[0]}))
        return
    for _ in range(3):
        for fn in calls.values():
            timed(fn)
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(timed(fn)[0])
    res = {k: stats(v) for k, v in times.items()}
    if has_f0:
        f0 = calls["f0"]()
        res["voiced_frames"] = int(sum(int((f > 0).sum()) for f in f0))
    res.update(frames=sum(frames), device=torch.cuda.get_device_name(0))
    print("RESULT " + json.dumps(res))


def run_worker(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--reps", str(args.reps), "--utterances", str(args.utterances),
           "--hidden", str(args.hidden), "--seed", str(args.seed)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent", help="a built checkout of the parent commit: its compute_ppg_padded is timed alternately")
    ap.add_argument("--once", choices=("f0", "padded", "padded_f0"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker or args.once:
        return worker(args)
    here, parent = [], []
    for _ in range(args.processes):
        here.append(run_worker(HERE, args))
        if args.parent:
            parent.append(run_worker(args.parent, args))
    med = lambda runs, k: statistics.median(r[k]["median_ms"] for r in runs)      # noqa: E731
    res = {"workload": "wav -> padded monophone PPG batch, %d utterances of 1-4 s (%d frames), TDNN hidden %d; %d processes x %d alternating reps"
                       % (args.utterances, here[0]["frames"], args.hidden, args.processes, args.reps),
           "device": here[0]["device"], "processes": here,
           "padded_median_ms": med(here, "padded"), "padded_f0_median_ms": med(here, "padded_f0"), "f0_alone_median_ms": med(here, "f0"),
           "f0_cost_ms": med(here, "padded_f0") - med(here, "padded"),
           "f0_cost_over_front_end": (med(here, "padded_f0") - med(here, "padded")) / med(here, "padded")}
    if parent:
        res.update(parent_processes=parent, parent_padded_median_ms=med(parent, "padded"),
                   padded_over_parent=med(here, "padded") / med(parent, "padded"))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
