"""Phase profile of the batch-1 vocoder's layer launches (library built with -DFACPPG_WN8_PROF, see tools/prof_wn8.sh):

  python tools/prof_wn8.py [T] [seeded_frames]

The headline's shape by default: one 200-frame utterance, the first 160 frames seeded (k_wn_layer_mixed: seeded 32-frame tiles
and unseeded 16-frame tiles in one launch).  seeded_frames = 0 runs the unseeded WaveGlow.infer of T frames instead.  Prints, per
tile kind and per place of the layer in its flow (first / middle / last), the time one workgroup spends in each phase, in
microseconds (the constant 100 MHz clock), next to the launch-to-launch interval of the same launches from the handle's events."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]
import torch  # noqa: E402
from facppg import synth, lib as flib  # noqa: E402
from waveglow.glow import WaveGlow  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seeded = int(sys.argv[2]) if len(sys.argv) > 2 else 160
cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=256)
m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
m.load_state_dict(synth.waveglow_state_dict(cfg))
m = m.cuda().eval()
mel = synth.synthetic_mel(1, T, seed=5).cuda()
L = flib.load()
out = (ctypes.c_ulonglong * 48)()
if seeded:
    melp = m.mel_pad(mel)
    _, _, nb = m.seed_layout(T, mel.device)
    seeds = torch.empty(nb // 4, dtype=torch.float32, device=mel.device)
    m.cond_seed(melp, T, 0, seeded, seeds)


def step(i):
    if seeded:
        m.infer_seeded(melp, T, seeds, seeded, sigma=0.6, seed=i)
    else:
        m.infer(mel, sigma=0.6, seed=i)


for i in range(3):
    step(i)
torch.cuda.synchronize()
L.facppg_debug_wn_prof(out, 1)
N = 20
for i in range(N):
    step(i)
torch.cuda.synchronize()
L.facppg_debug_wn_prof(out, 1)
names = ["prologue", "K loop", "gate", "2nd GEMM", "end rows", "skip+edge", "epilogue"]
order = [0, 1, 2, 3, 4, 6, 5]
print("T = %d, %d seeded frames, launch shape %s, fused edges %s; us per launch in one workgroup" % (
    T, seeded, m.last_launch_shape(), os.environ.get("FACPPG_WG_EDGE_FUSE", "1") != "0"))
print("%-22s %8s " % ("tile / layer", "launches") + " ".join("%9s" % n for n in names) + " %9s" % "sum")
for tk, tname in enumerate(("32-frame", "16-frame")):
    for kind, kname in enumerate(("first", "middle", "last")):
        v = out[(tk * 3 + kind) * 8:(tk * 3 + kind) * 8 + 8]
        n = v[7]
        if not n:
            continue
        us = [v[i] / n / 100.0 for i in order]
        print("%-22s %8d " % (tname + " " + kname, n) + " ".join("%9.2f" % u for u in us) + " %9.2f" % sum(us))
