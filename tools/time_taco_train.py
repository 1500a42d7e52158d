"""One fine-tuning step of the PPG->mel model, phase by phase, next to the no-grad Tacotron2.forward call.

For each batch size: B utterances of Tin frames, T_out target frames.  Timed in turn within every repetition, after a warm-up:
  forward        the plain call under torch.no_grad() (nothing kept), host clock around a device synchronise
  forward_diff   forward(..., differentiable=True) + Tacotron2Loss
  backward       loss.backward(): common.taco_grad.backward
  recurrences    of it, the calls into csrc/facppg_taco_bwd.hip (cell scans, LSTM chains, attention chain), device events;
                 also per decoder frame for the two decoder chains
  clip_adam      clip_grad_norm_ + waveglow.optim.Adam.step
  rebuild        dropping and re-creating the packed-weight handle, which every optimiser step costs
Prints one JSON line; --out FILE also writes it there.  --once: one warmed step per batch size and nothing else (profilers).

  python tools/time_taco_train.py [--batches 2 6 16] [--tin 200] [--tout 200] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]
import torch  # noqa: E402
from common import taco_grad  # noqa: E402
from common.hparams import create_hparams_stage  # noqa: E402
from common.loss_function import Tacotron2Loss  # noqa: E402
from facppg import synth  # noqa: E402
from script.train_ppg2mel import load_model  # noqa: E402
from waveglow.optim import Adam  # noqa: E402


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


class TimedRecurrences(taco_grad.HipRecurrences):
    """HipRecurrences with a pair of device events around every call."""
    spans = None

    def _timed(self, name, fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a)
        e1.record()
        TimedRecurrences.spans.append((name, e0, e1))
        return out

    def cell_scan(self, *a):
        return self._timed("cell_scan", super().cell_scan, *a)

    def lstm_backward(self, *a):
        return self._timed("lstm_backward_H%d" % a[2].shape[2], super().lstm_backward, *a)

    def attention_backward(self, *a):
        return self._timed("attention_backward", super().attention_backward, *a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 6, 16])
    ap.add_argument("--tin", type=int, default=200)
    ap.add_argument("--tout", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    Tin, T = a.tin, a.tout
    hp = create_hparams_stage(max_decoder_steps=T)
    m = load_model(hp)
    m.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    m.eval()
    dev = torch.device("cuda", torch.cuda.current_device())
    crit = Tacotron2Loss(hp.mel_weight, hp.gate_weight)
    opt = Adam(m.parameters(), lr=hp.learning_rate, weight_decay=hp.weight_decay)
    taco_grad.HipRecurrences = TimedRecurrences
    rows = []

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for B in a.batches:
        x = torch.stack([torch.from_numpy(synth.synthetic_ppg(Tin, seed=i)).float().t() for i in range(B)]).cuda()
        tgt = synth.synthetic_mel(B, T, seed=100).cuda()
        gate_t = torch.zeros(B, T, device=dev)
        gate_t[:, -1] = 1
        lens = torch.full((B,), Tin, dtype=torch.long, device=dev)
        olens = torch.full((B,), T, dtype=torch.long, device=dev)
        fwd_in = (x, lens, tgt, Tin, olens)

        def plain():
            with torch.no_grad():
                return m(fwd_in, seed=1)

        def diff():
            return crit(m(fwd_in, seed=1, differentiable=True), (tgt, gate_t))

        def step():
            torch.nn.utils.clip_grad_norm_(m.parameters(), hp.grad_clip_thresh)
            opt.step()

        def rebuild():
            m.invalidate_packed_weights()
            m._handle(dev)

        keys = ("forward", "forward_diff", "backward", "clip_adam", "rebuild")
        t = {k: [] for k in keys}
        rec = {}
        for r in range(-3, 1 if a.once else a.reps):
            TimedRecurrences.spans = []
            m.zero_grad()
            v = [clock(plain)[0]]
            ms, loss = clock(diff)
            v += [ms, clock(loss.backward)[0], clock(step)[0], clock(rebuild)[0]]
            if r < 0:
                continue
            for k, ms in zip(keys, v):
                t[k].append(ms)
            per = {}
            for name, e0, e1 in TimedRecurrences.spans:
                per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
            for name, ms in per.items():
                rec.setdefault(name, []).append(ms)
        if a.once:
            continue
        row = {"B": B, "Tin": Tin, "T_out": T, "reps": a.reps}
        row.update({k: stats(v) for k, v in t.items()})
        row["recurrences"] = {k: statistics.median(v) for k, v in rec.items()}
        row["recurrences_total_ms"] = sum(row["recurrences"].values())
        row["decoder_chains_us_per_frame"] = (row["recurrences"]["attention_backward"] +
                                              row["recurrences"]["lstm_backward_H%d" % hp.decoder_rnn_dim]) * 1e3 / T
        fb = row["forward_diff"]["median_ms"] + row["backward"]["median_ms"]
        row["forward_plus_backward_over_forward"] = fb / row["forward"]["median_ms"]
        rows.append(row)
        print("B=%d: forward %.2f ms | differentiable forward + loss %.2f ms, backward %.2f ms (recurrences %.2f ms, decoder chains "
              "%.1f us/frame) = %.2f x forward | clip + Adam %.2f ms, handle rebuild %.2f ms"
              % (B, row["forward"]["median_ms"], row["forward_diff"]["median_ms"], row["backward"]["median_ms"],
                 row["recurrences_total_ms"], row["decoder_chains_us_per_frame"], row["forward_plus_backward_over_forward"],
                 row["clip_adam"]["median_ms"], row["rebuild"]["median_ms"]), file=sys.stderr)
    if a.once:
        return
    line = json.dumps({"tool": "time_taco_train", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
