"""Shared by the backward-pass tests: the gradient fixtures (tests/golden/make_golden_forced_grad.py) and the comparison
they are held to.

The unit of every tolerance is E32: the largest relative L2 deviation of the reference's OWN float32 backward pass from its
float64 one, over the three cases, all 61 tensors, whole tensor and sub-sample (6.7e-6).  A gradient is compared with the
FLOAT64 reference: the relative error of its norm and the relative L2 deviation on the strided sub-sample must both be within
C * E32, one C for all tensors and cases."""
import numpy as np

from helpers import golden

TAGS = ("ragged", "dup", "mono40")
N_SUB = 256
# C: the smallest power of two that leaves the worst deviation measured on the GPU a factor 2 of headroom (the figures are in
# DESIGN.md section 4 and in tests/test_gpu_tacotron_backward.py); C * E32 may not exceed CAP, the relative tolerance
# test_oracle_golden.py::test_training_step_at_config5_shape holds WaveGlow gradient norms to.
C = 4
C_LOSS = 1          # the same rule for finetune's 8 losses against the fixture's float32-vs-float64 loss deviation (1.2e-6)
CAP = 1e-3


def sub_index(n):
    """The strided sub-sample of a tensor of n values: the generator's rule."""
    return np.arange(0, n, max(1, n // N_SUB))[:N_SUB]


def grad_fixture(tag):
    return golden("tacotron_forced_grad_%s.npz" % tag)


def e32():
    return max(float(grad_fixture(t)["e32"]) for t in TAGS)


def tolerance():
    tol = C * e32()
    assert tol <= CAP, (C, e32())
    return tol


def deviations(fix, named_grads):
    """-> [(name, relative norm error, relative L2 deviation on the sub-sample)] of every tensor of the fixture, in its order;
    ``named_grads``: name -> gradient (numpy, any shape).  A missing tensor is an error: none is skipped."""
    out = []
    for i, name in enumerate(fix["names"]):
        a = np.asarray(named_grads[str(name)], dtype=np.float64).reshape(-1)
        idx = sub_index(a.size)
        ref = fix["sub"][i][:idx.size]
        out.append((str(name), abs(np.linalg.norm(a) - fix["norm"][i]) / fix["norm"][i],
                    np.linalg.norm(a[idx] - ref) / np.linalg.norm(ref)))
    return out
