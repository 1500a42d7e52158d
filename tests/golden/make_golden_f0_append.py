#!/usr/bin/env python3
"""Generate tests/golden/f0_append.npz by IMPORTING THE REFERENCE's own append_ppg / compute_delta_acc_feat
(src/common/data_utils.py:62-160) -- the only thing this feature takes from it: a few KB of inputs and outputs.

Runs only in the dev container (needs /root/reference).  The shim is make_golden.py's: a synthetic ``common`` package pointing at
src/common; the modules data_utils.py imports at its top and that need Kaldi, pyworld or librosa (common.utterance, common.layers,
common.feat, common.ppg, ppg) are replaced by empty stand-ins, since the four functions called here use NumPy alone.

Inputs: (T_ppg, T_f0) in {(1, 1), (2, 3), (5, 4), (37, 40)}, five feature columns from a seeded generator, F0 tracks in Hz
that contain zeros (unvoiced frames).  Per case the file holds feats, f0, append_ppg(feats, f0), and
compute_delta_acc_feat(feats, True, True).

Usage:  python tests/golden/make_golden_f0_append.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"
CASES = ((1, 1), (2, 3), (5, 4), (37, 40))


def install_shims():
    for name in [m for m in sys.modules if m == "common" or m.startswith("common.") or m == "ppg" or m.startswith("ppg.")]:
        del sys.modules[name]
    pkg = types.ModuleType("common")
    pkg.__path__ = [os.path.join(REF, "common")]
    sys.modules["common"] = pkg
    for name, attrs in (("common.utterance", ("Utterance",)), ("common.layers", ()), ("common.feat", ()), ("common.ppg", ()),
                        ("ppg", ("DependenciesPPG",))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, type(a, (object,), {}))
        sys.modules[name] = mod
        if name.startswith("common."):
            setattr(pkg, name.split(".")[1], mod)


def inputs(t_ppg, t_f0):
    g = np.random.Generator(np.random.PCG64(1000 * t_ppg + t_f0))
    feats = g.random((t_ppg, 5))
    f0 = 80.0 + 200.0 * g.random(t_f0)
    f0[g.random(t_f0) < 0.35] = 0.0
    if t_f0 > 2:
        f0[0] = 0.0                    # an unvoiced edge: the replicated value is log(eps)
    return feats, f0


def main():
    install_shims()
    from common import data_utils as ref
    out = {"delta_win": np.asarray(ref.DELTA_WIN, np.float64), "acc_win": np.asarray(ref.ACC_WIN, np.float64)}
    for t_ppg, t_f0 in CASES:
        feats, f0 = inputs(t_ppg, t_f0)
        key = "%d_%d" % (t_ppg, t_f0)
        out["feats_" + key], out["f0_" + key] = feats, f0
        out["append_" + key] = ref.append_ppg(feats, f0)
        out["delta_acc_" + key] = ref.compute_delta_acc_feat(feats, True, True)
        out["delta_" + key] = ref.compute_dynamic_matrix(feats, ref.DELTA_WIN)
        out["vector_" + key] = ref.compute_dynamic_vector(feats[:, 0], ref.ACC_WIN, t_ppg)
    path = os.path.join(HERE, "f0_append.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
