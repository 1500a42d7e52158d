"""Writes tests/golden/waveglow_half_yardstick_hop{256,160}.npz: the two CPU references of the half-precision accuracy criterion
(tests/test_gpu_waveglow_f16.py::test_half_infer_at_least_as_accurate_as_reference_half_branch) at its shapes -- the fp32
oracle's audio `a32` and the reference's half branch restated on the CPU `aref` (that test's _ref_half), utterances of 24 and 17
frames concatenated.  Both take a minute on the CPU; tests/test_gpu_stream_f16.py reads them instead of recomputing them.
Run from the repository root:  python tests/golden/make_half_yardstick.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "fac-via-ppg_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from facppg import synth                      # noqa: E402
from oracle import waveglow as owg            # noqa: E402
from test_gpu_waveglow_f16 import _ref_half   # noqa: E402

LENGTHS, SIGMA, MEL_SEED, Z_SEED = [24, 17], 0.6, 31, 32


def main():
    for hop in (256, 160):
        cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=12)
        sd = synth.waveglow_state_dict(cfg)
        B, T = len(LENGTHS), max(LENGTHS)
        mel = synth.synthetic_mel(B, T, seed=MEL_SEED)
        zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=Z_SEED)
        a32, aref = [], []
        with torch.no_grad():
            for b, Tb in enumerate(LENGTHS):
                Lb = Tb * hop // 8
                zb = [z[b:b + 1, :, :Lb] for z in zs]
                a32.append(owg.infer(sd, cfg, mel[b:b + 1, :, :Tb], SIGMA, zb)[0])
                aref.append(_ref_half(sd, cfg, mel[b:b + 1, :, :Tb], SIGMA, zb)[0].float())
        out = os.path.join(HERE, "waveglow_half_yardstick_hop%d.npz" % hop)
        np.savez_compressed(out, a32=torch.cat(a32).numpy(), aref=torch.cat(aref).numpy(), lengths=np.array(LENGTHS), sigma=SIGMA,
                            mel_seed=MEL_SEED, z_seed=Z_SEED)
        print(out, os.path.getsize(out))


if __name__ == "__main__":
    main()
