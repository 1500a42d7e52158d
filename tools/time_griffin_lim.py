"""What Griffin-Lim costs as one device loop (STFT.griffin_lim, momentum 0) next to the Python loop over STFT.transform /
STFT.inverse that the package has always had (common.audio_processing.griffin_lim, unchanged: a fair yardstick).

No models.  STFT(1024, 256, 1024), n_iters = 32, two shapes:
  one     1 utterance of 200 frames
  ragged  16 utterances of 100 to 400 frames; the Python loop has no lengths and runs them padded to 400
The two ALTERNATE in one process, three warm-up and --reps timed calls each, the host clock around every call (synchronised).
Run it in three processes; the bar is that the device loop's median is below the Python loop's in every process at both shapes.
Under ``rocprofv3 --kernel-trace --stats`` (--only device / --only loop: one of the two alone) this is the run the per-kernel
times come from.

Prints one JSON line per shape; --out FILE appends them there.

  python tools/time_griffin_lim.py [--reps 20] [--n_iters 32] [--only device|loop] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n_iters", type=int, default=32)
    ap.add_argument("--only", choices=("device", "loop"), default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path[:0] = [HERE, os.path.join(HERE, "fac-via-ppg_amd")]
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    from common.audio_processing import griffin_lim
    from common.stft import STFT

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    stft = STFT(1024, 256, 1024).cuda()
    g = np.random.Generator(np.random.PCG64(args.seed))
    shapes = {"one": [200], "ragged": [int(v) for v in g.integers(100, 401, size=16)]}
    shapes["ragged"][0], shapes["ragged"][1] = 400, 100
    for name, frames in shapes.items():
        B, F = len(frames), max(frames)
        audio = torch.from_numpy(0.1 * g.standard_normal((B, 256 * (F - 1))).astype(np.float32)).cuda()
        mag, _ = stft.transform(audio)                   # [B, 513, F]
        lengths = frames if B > 1 else None
        np.random.seed(args.seed)

        def device():
            return stft.griffin_lim(mag, n_iters=args.n_iters, momentum=0.0, lengths=lengths, utterance_seeds=list(range(B)))

        def loop():
            return griffin_lim(mag, stft, n_iters=args.n_iters)
        runs = [(n, f) for n, f in (("device", device), ("loop", loop)) if args.only in (None, n)]
        for _ in range(3):
            for _, f in runs:
                timed(f)
        t = {n: [] for n, _ in runs}
        for _ in range(args.reps):
            for n, f in runs:
                t[n].append(timed(f)[0])
        res = {"shape": name, "frames": frames, "n_iters": args.n_iters, "device_name": torch.cuda.get_device_name(0), "reps": args.reps}
        for n in t:
            res[n] = stats(t[n])
            res[n]["per_iteration_us"] = 1e3 * statistics.median(t[n]) / max(args.n_iters, 1)
        if len(t) == 2:
            res["loop_over_device"] = statistics.median(t["loop"]) / statistics.median(t["device"])
            res["device_below_loop"] = statistics.median(t["device"]) < statistics.median(t["loop"])
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
