"""Teacher-forced Tacotron2.forward against the free-running Tacotron2.inference on the same shapes.

For each batch size: B utterances of Tin frames, T_out target frames (inference: step_limits = T_out and gate_bias = -10, so
the free-running decoder never stops early).  Timed, alternating, after a warm-up of both:
  call     the whole Python call, host clock around a device synchronise
  decoder  the decoder entry point alone (facppg_taco_decode_forced: prenet / input-product GEMMs + the recurrent launch +
           projection GEMM; facppg_taco_decode: the free-running loop, which holds all of that), device events
Prints one JSON line; --out FILE also writes it there.

  python tools/time_taco_forward.py [--batches 2 6 16] [--tin 200] [--tout 200] [--reps 20] [--out FILE]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]
import torch  # noqa: E402
from common.hparams import create_hparams_stage  # noqa: E402
from facppg import lib as flib, synth  # noqa: E402
from script.train_ppg2mel import load_model  # noqa: E402


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 6, 16])
    ap.add_argument("--tin", type=int, default=200)
    ap.add_argument("--tout", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one warmed forward per batch size and nothing else (profiler runs)")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    Tin, T = a.tin, a.tout
    hp = create_hparams_stage(max_decoder_steps=T)
    m = load_model(hp)
    m.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    m.eval()
    L = flib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = flib.current_stream(dev)
    E, P, NF, AD = hp.encoder_embedding_dim, hp.prenet_dim, hp.n_acoustic_feat_dims, hp.attention_dim
    rows = []
    for B in a.batches:
        x = torch.stack([torch.from_numpy(synth.synthetic_ppg(Tin, seed=i)).float().t() for i in range(B)]).cuda()
        tgt = synth.synthetic_mel(B, T, seed=100).cuda()
        lens = torch.full((B,), Tin, dtype=torch.long, device=dev)
        olens = torch.full((B,), T, dtype=torch.long, device=dev)
        fwd_in = (x, lens, tgt, Tin, olens)

        def run_forward():
            return m(fwd_in, seed=1)

        def run_inference():
            with contextlib.redirect_stdout(io.StringIO()):     # ("Reached max decoder steps")
                return m.inference(x, lengths=lens if B > 1 else None, seed=1, step_limits=[T] * B)

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(3):
            run_forward()
            if not a.once:
                run_inference()
        if a.once:
            torch.cuda.synchronize()
            run_forward()
            torch.cuda.synchronize()
            continue
        t_fwd, t_inf = [], []
        for _ in range(a.reps):
            t_fwd.append(clock(run_forward))
            t_inf.append(clock(run_inference))
        # the decoder entry points alone, on the encoder outputs of this batch
        h = m._handle(dev)
        memory, lt = m.last_memory, lens.to(torch.int32)
        pm = torch.zeros(B, AD, Tin, device=dev)
        ws = torch.empty(max(L.facppg_taco_workspace_bytes(h, B, Tin), L.facppg_taco_decode_forced_workspace_bytes(h, B, T),
                             L.facppg_taco_decode_workspace_bytes(h, B, T)), dtype=torch.uint8, device=dev)
        mem2 = torch.zeros_like(memory)
        flib.check(L.facppg_taco_encode(h, flib.ptr(x), flib.ptr(lt), None, 1, B, Tin, flib.ptr(mem2), flib.ptr(pm), flib.ptr(ws),
                                        ws.numel(), st))
        mel, gate = torch.zeros(B, NF, T, device=dev), torch.zeros(B, T, device=dev)
        align, out_len = torch.zeros(B, T, Tin, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        sl = torch.full((B,), T, dtype=torch.int32, device=dev)
        of, oi = flib.TacoDecodeOpts(), flib.TacoDecodeOpts()

        def dec_forced():
            flib.check(L.facppg_taco_decode_forced(h, flib.ptr(mem2), flib.ptr(pm), flib.ptr(lt), flib.ptr(tgt), None, 1, B, Tin, T,
                                                   flib.ptr(mel), flib.ptr(gate), flib.ptr(align), flib.ptr(ws), ws.numel(),
                                                   flib.ctypes.byref(of), st))

        def dec_free():
            flib.check(L.facppg_taco_decode(h, flib.ptr(mem2), flib.ptr(pm), flib.ptr(lt), flib.ptr(sl), None, 1, B, Tin, T,
                                            flib.ptr(mel), flib.ptr(gate), flib.ptr(align), flib.ptr(out_len), flib.ptr(ws),
                                            ws.numel(), flib.ctypes.byref(oi), st))

        def events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(3):
            dec_forced()
            dec_free()
        d_fwd, d_inf = [], []
        for _ in range(a.reps):
            d_fwd.append(events(dec_forced))
            d_inf.append(events(dec_free))
        assert int(out_len.min()) == T, out_len
        row = {"B": B, "Tin": Tin, "T_out": T, "reps": a.reps,
               "forward_call": stats(t_fwd), "inference_call": stats(t_inf),
               "forward_decoder": dict(stats(d_fwd), workgroups=of.workgroups),
               "inference_decoder": dict(stats(d_inf), mode=("single", "coop", "split")[oi.mode], workgroups=oi.workgroups)}
        row["forward_decoder_us_per_frame"] = row["forward_decoder"]["median_ms"] * 1e3 / T
        row["inference_decoder_us_per_frame"] = row["inference_decoder"]["median_ms"] * 1e3 / T
        rows.append(row)
        print("B=%d: forward %.2f ms (decoder %.2f ms, %.1f us/frame, %d workgroups) | inference %.2f ms (decoder %.2f ms, %.1f us/frame, "
              "%s, %d workgroups)" % (B, row["forward_call"]["median_ms"], row["forward_decoder"]["median_ms"],
                                      row["forward_decoder_us_per_frame"], of.workgroups, row["inference_call"]["median_ms"],
                                      row["inference_decoder"]["median_ms"], row["inference_decoder_us_per_frame"],
                                      row["inference_decoder"]["mode"], oi.workgroups), file=sys.stderr)
    if a.once:
        return
    line = json.dumps({"tool": "time_taco_forward", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
