#!/usr/bin/env python3
"""The .half() vocoder alone on one utterance (hop 256, synthetic weights, 12 flows): WaveGlow.infer in both K orders against
infer_seeded with no, some and all tiles seeded, and one k16_cond_seed pass per block width.  hipEvents around each call, best
and median of --reps after a warm-up; per-launch figures are differences over the 96 layer launches.  Prints one JSON line.

  python tools/time_wg16_seeded.py [--frames 200] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]

import torch  # noqa: E402

from facppg import synth  # noqa: E402
from time_wg16 import model  # noqa: E402


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        f()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    T, hop = args.frames, 256
    dev = torch.device("cuda", 0)
    out = {"frames": T, "hop": hop}
    with torch.no_grad():
        m = model(hop, True)
        mel = synth.synthetic_mel(1, T, seed=5).cuda()
        mel16 = mel.half()
        melp = m.mel_pad(mel)
        _, _, nbytes = m.seed_layout(T, dev)
        seeds = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        s_all = -(-T // 32) * 32
        m.cond_seed(melp, T, 0, s_all, seeds, block_tiles=1)
        out["infer_tap_first"] = timed(lambda: m.infer(mel16, sigma=0.6, seed=1), args.reps)
        out["infer_cond_first"] = timed(lambda: m.infer(mel16, sigma=0.6, seed=1, cond_first=True), args.reps)
        out["launch_shape_unseeded"] = list(m.last_launch_shape())
        for name, s in (("seeded_none", 0), ("seeded_all_but_last_tile", s_all - 32), ("seeded_all", s_all)):
            out["infer_" + name] = timed(lambda: m.infer_seeded(melp, T, seeds, s, sigma=0.6, seed=1), args.reps)
        out["launch_shape_seeded"] = list(m.last_launch_shape())
        for bt in (1, 2, 4):
            r = timed(lambda: m.cond_seed(melp, T, 0, 32 * bt, seeds, block_tiles=bt), args.reps)
            r["TB_per_s_of_weight_images"] = round(1.0066 / r["min_ms"], 3)     # 96 layers x 32 phases x 320 KiB = 1.0066 GB per pass
            out["cond_seed_%d_frames" % (32 * bt)] = r
    d = out["infer_seeded_none"]["min_ms"] - out["infer_seeded_all"]["min_ms"]
    out["per_launch_saving_us"] = round(d * 1e3 / 96, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
