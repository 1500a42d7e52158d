#!/usr/bin/env python3
"""fp32 vs fp16 WaveGlow.infer throughput (synthetic weights, hop 256, 12 flows): samples/s at B = 8 x 1000 frames (BASELINE
config 2's shape) and the vocoder time of one 200-frame utterance (B = 1).  Best of N timed calls after a warm-up, by hipEvents
around the whole infer() (host launch overhead included).  Prints one JSON line.

  python tools/time_wg16.py [--reps N] [--tile 32|64|128]   (--tile forces FACPPG_WG16_TILE)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]

import torch  # noqa: E402

from facppg import synth  # noqa: E402
from waveglow.glow import WaveGlow  # noqa: E402


def model(hop, half):
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop)
    m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    m.load_state_dict(synth.waveglow_state_dict(cfg))
    m = m.cuda().eval()
    if half:
        m.half()
        for k in m.convinv:
            k.float()
    return m


def best_ms(f, reps):
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
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tile", type=int, default=0)
    args = ap.parse_args()
    if args.tile:
        os.environ["FACPPG_WG16_TILE"] = str(args.tile)
    hop = 256
    out = {"hop": hop}
    with torch.no_grad():
        for half in (False, True):
            m = model(hop, half)
            tag = "fp16" if half else "fp32"
            for B, T in ((8, 1000), (1, 200)):
                mel = synth.synthetic_mel(B, T, seed=5).cuda()
                if half:
                    mel = mel.half()
                ms = best_ms(lambda: m.infer(mel, sigma=0.6, seed=1), args.reps)
                out["%s_B%d_T%d_ms" % (tag, B, T)] = round(ms, 3)
                out["%s_B%d_T%d_Msamples_per_s" % (tag, B, T)] = round(B * T * hop / ms / 1e3, 2)
                out["%s_B%d_T%d_launch_shape" % (tag, B, T)] = list(m.last_launch_shape())
            del m
            torch.cuda.empty_cache()
    out["speedup_B8_T1000"] = round(out["fp32_B8_T1000_ms"] / out["fp16_B8_T1000_ms"], 3)
    out["speedup_B1_T200"] = round(out["fp32_B1_T200_ms"] / out["fp16_B1_T200_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
