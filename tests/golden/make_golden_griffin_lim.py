#!/usr/bin/env python3
"""Generate tests/golden/griffin_lim.npz by IMPORTING THE REFERENCE's own griffin_lim (src/common/audio_processing.py:91-107)
over its own STFT (src/common/stft.py), through the shims of make_golden.py.

Runs only in the dev container (needs /root/reference).  One case: STFT(1024, 256, 1024), 12 frames, n_iters = 2, magnitudes of a
tone-plus-noise signal (tests/griffin_lim_helpers.case), phases drawn by the reference itself under np.random.seed(SEED) and
recovered here by re-seeding.  The file holds M [513, 12], the drawn angles [513, 12] and the signal [2816]: a few tens of kB.

Usage:  python tests/golden/make_golden_griffin_lim.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "fac-via-ppg_amd"))
sys.path.insert(0, ROOT)

SEED = 20240
FL, HOP, F, N_ITERS = 1024, 256, 12, 2


def main():
    import griffin_lim_helpers as glh
    _, M, _, _ = glh.case(FL, HOP, F, 0)              # (before the shims replace ``common``)
    M32 = M.astype(np.float32)
    import make_golden
    make_golden.install_shims()
    from common.audio_processing import griffin_lim
    from common.stft import STFT
    stft = STFT(FL, HOP, FL)
    mags = torch.from_numpy(M32[None])
    np.random.seed(SEED)
    with torch.no_grad():
        signal = griffin_lim(mags, stft, n_iters=N_ITERS)
    np.random.seed(SEED)
    angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mags.size()))).astype(np.float32)
    out = os.path.join(HERE, "griffin_lim.npz")
    np.savez_compressed(out, M=M32, angles=angles[0], signal=signal[0].numpy().astype(np.float32),
                        filter_length=FL, hop_length=HOP, n_iters=N_ITERS, seed=SEED)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
