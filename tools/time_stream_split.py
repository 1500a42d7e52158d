#!/usr/bin/env python3
"""End-to-end time of ONE utterance (PPG -> wav: pipeline.synthesize with denoiser, hop 256, synthetic weights, 12 flows) per
vocoder path and utterance length: host clock around the call, ending in a device synchronise (upload, encoder, decoder, postnet,
vocoder, denoiser; the audio stays on the device).  The decoder runs to its step limit (= the PPG's length); one model pair serves
every length.  --mode picks the path:
  plain    vocoder_arithmetic="bf16x3"                       (tap-first split kernels, never streamed)
  stream   vocoder_arithmetic="bf16x3", vocoder_stream=True  (conditioning-first split kernels; streamed when FACPPG_STREAM allows)
  fp32     the fp32 vocoder's own path                       (streamed by its own rules)
  fp16     a .half() vocoder                                 (streamed by its own rules)
FACPPG_STREAM=0|1 in the environment decides whether the utterance may stream; FACPPG_STREAM_MIN_FRAMES=0 makes every length
stream; FACPPG_STREAM_TAIL=seed|mixed picks the tail variant.  --root imports the package from another checkout (an A/B against
the parent commit's tree on the same box: --mode plain needs nothing newer).  --passes adds one profiled call per length and the
durations of its seed passes (ConditioningStream.pass_ms).
Prints one JSON line: per length the median, min and max ms over --reps timed calls after --warmup untimed ones.

  python tools/time_stream_split.py --mode stream [--frames 64,100,130,200,400,1000] [--reps 20] [--warmup 3] [--passes] [--root DIR]"""
import argparse
import contextlib
import gc
import io
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("plain", "stream", "fp32", "fp16"), default="stream")
    ap.add_argument("--frames", default="200")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", action="store_true", help="one more call per length with the seed passes timed")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "fac-via-ppg_amd")]
    import torch
    from common.hparams import create_hparams_stage
    from facppg import pipeline, synth
    from script.train_ppg2mel import load_model
    from waveglow.denoiser import Denoiser
    from waveglow.glow import WaveGlow
    hop = 256
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop)
    wg = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    wg.load_state_dict(synth.waveglow_state_dict(cfg))
    wg = wg.cuda().eval()
    if args.mode == "fp16":
        wg.half()
        for k in wg.convinv:      # the reference's recipe: convinv kept in float
            k.float()
    den = Denoiser(wg, hop_length=hop, mode="zeros")
    kw = {"plain": {"vocoder_arithmetic": "bf16x3"}, "stream": {"vocoder_arithmetic": "bf16x3", "vocoder_stream": True}}.get(args.mode, {})
    split = args.mode in ("plain", "stream")
    out = {"root": root, "mode": args.mode, "FACPPG_STREAM": os.environ.get("FACPPG_STREAM", "1"),
           "FACPPG_STREAM_MIN_FRAMES": os.environ.get("FACPPG_STREAM_MIN_FRAMES"), "FACPPG_STREAM_TAIL": os.environ.get("FACPPG_STREAM_TAIL"),
           "reps": args.reps}
    frames = [int(v) for v in args.frames.split(",")]
    # ONE acoustic model for every length (its step limit per call): the stream, its side streams and buffers belong to the model pair
    hp = create_hparams_stage(max_decoder_steps=max(frames))
    with contextlib.redirect_stdout(io.StringIO()):
        taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    taco.eval()
    cs = None
    for T in frames:
        ppgs = [synth.synthetic_ppg(T, 5816, seed=T, alpha=0.002)]
        limits = None if T == max(frames) else [T]

        def call():
            with contextlib.redirect_stdout(io.StringIO()):
                wavs, tout = pipeline.synthesize(ppgs, taco, wg, den, sigma=0.6, strength=0.005, seed=3, return_device=True, step_limits=limits, **kw)
            torch.cuda.synchronize()
            return tout[0]
        for _ in range(args.warmup):
            tout = call()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        cs = wg.__dict__.get("_facppg_cond_stream")
        streamed = cs is not None and getattr(cs, "Tout", None) == tout and (args.mode != "plain")
        rec = {"frames_out": tout, "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
               "launch_shape": list(wg.last_launch_shape("bf16x3") if split else wg.last_launch_shape()),
               "seeded_frames": cs.seeded if streamed else None}
        if args.passes and streamed:
            cs.profile = True
            call()
            rec["blocks"] = [list(c) for c in cs.cuts]
            rec["pass_ms"] = [[n, round(ms, 3)] for n, _, ms in cs.pass_ms()]
            cs.profile = False
        out["T%d" % T] = rec
    print(json.dumps(out), flush=True)
    # release the side streams, events and handles while the runtime is still up (not from interpreter teardown)
    wg._release()
    del den, taco, wg, cs
    gc.collect()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
