#!/usr/bin/env python3
"""fp32 vs fp16 vs bf16x3 WaveGlow.infer (synthetic weights, hop 256, 12 flows): B = 8 x 1000 frames (BASELINE config 2's shape)
and one 200-frame utterance (B = 1).  Every measurement is a process of its own -- best of N timed calls after a warm-up, by
hipEvents around the whole infer() (host launch overhead included) -- and the processes of the three arithmetics ALTERNATE
(fp32, fp16, bf16x3, fp32, ...), one at a time, so that clock and thermal drift of the box hits all three alike.  The driver
prints, and with --out writes, the median and the range per arithmetic and shape, the ratios, and whether EVERY bf16x3 run was
faster than EVERY fp32 run at both shapes (the bar the mode is held to).

  python tools/time_wg_split.py [--rounds R] [--reps N] [--out profiles/NAME.json]       the alternation
  python tools/time_wg_split.py --one fp32|fp16|bf16x3 [--reps N] [--tile 32|64]         one process' measurement (one JSON line;
                                                                                         --tile forces FACPPG_WG_SPLIT_TILE)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]

HOP = 256
SHAPES = ((8, 1000), (1, 200))
ARITHMETICS = ("fp32", "fp16", "bf16x3")


def one(arith, reps):
    import torch
    from facppg import synth
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=HOP)
    m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    m.load_state_dict(synth.waveglow_state_dict(cfg))
    m = m.cuda().eval()
    if arith == "fp16":
        m.half()
        for k in m.convinv:
            k.float()
    kw = {"arithmetic": "bf16x3"} if arith == "bf16x3" else {}
    out = {"arithmetic": arith}
    with torch.no_grad():
        for B, T in SHAPES:
            mel = synth.synthetic_mel(B, T, seed=5).cuda()
            if arith == "fp16":
                mel = mel.half()

            def f():
                return m.infer(mel, sigma=0.6, seed=1, **kw)
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
            out["B%d_T%d_ms" % (B, T)] = round(min(ts), 3)
            out["B%d_T%d_launch_shape" % (B, T)] = list(m.last_launch_shape(*([arith] if kw else [])))
    print(json.dumps(out))


def drive(rounds, reps, out_path):
    runs = {a: {"B%d_T%d_ms" % s: [] for s in SHAPES} for a in ARITHMETICS}
    shapes = {}
    for r in range(rounds):
        for a in ARITHMETICS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", a, "--reps", str(reps)], stdout=subprocess.PIPE,
                               timeout=300)
            if p.returncode != 0:            # a failed measurement ends the alternation: nothing more is started on the GPU
                sys.exit("round %d, %s: exit status %d" % (r, a, p.returncode))
            d = json.loads(p.stdout.decode().strip().splitlines()[-1])
            for k in runs[a]:
                runs[a][k].append(d[k])
            shapes[a] = {k: v for k, v in d.items() if k.endswith("launch_shape")}
            print("round %d %s" % (r, json.dumps(d)), flush=True)
    res = {"hop": HOP, "rounds": rounds, "reps_per_process": reps, "launch_shapes": shapes, "ms": {}, "ratio_of_medians": {}, "bar": {}}
    for a in ARITHMETICS:
        res["ms"][a] = {k: {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v), "runs": v} for k, v in runs[a].items()}
    ok = True
    for B, T in SHAPES:
        k = "B%d_T%d_ms" % (B, T)
        f32, sp, f16 = res["ms"]["fp32"][k], res["ms"]["bf16x3"][k], res["ms"]["fp16"][k]
        res["ratio_of_medians"][k] = {"fp32_over_bf16x3": round(f32["median"] / sp["median"], 3),
                                      "fp32_over_fp16": round(f32["median"] / f16["median"], 3),
                                      "bf16x3_over_fp16": round(sp["median"] / f16["median"], 3)}
        res["bar"][k] = sp["max"] < f32["min"]         # every bf16x3 run faster than every fp32 run
        ok = ok and res["bar"][k]
    res["bar"]["met"] = ok
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=ARITHMETICS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.tile:
        os.environ["FACPPG_WG_SPLIT_TILE"] = str(args.tile)
    if args.one:
        one(args.one, args.reps)
    else:
        drive(args.rounds, args.reps, args.out)


if __name__ == "__main__":
    main()
