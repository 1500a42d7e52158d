"""No GPU: the float64 reference of tests/upsample_helpers.py is held to float64 autograd of conv_transpose1d + crop + regroup, and
the integer cases of test_gpu_upsample.py are shown to be exact: every forward value and partial sum is an integer of magnitude
<= max S_fwd <= 256, which bf16 (8 significant bits) and fp32 hold exactly in any summation order; every backward sum stays
below 2^24, the integers fp32 holds exactly."""
import numpy as np
import pytest
import torch

import upsample_helpers as uh


def _autograd(c):
    o = {k: torch.from_numpy(v.astype(np.float64)) for k, v in uh.operands(c.shape).items()}
    W, bias = o["W"].clone().requires_grad_(True), o["bias"].clone().requires_grad_(True)
    y = torch.nn.functional.conv_transpose1d(o["mel"], W, bias, stride=c.hop)[:, :, :8 * c.L]
    s = y.unfold(2, 8, 8).permute(0, 2, 1, 3)                          # the reference's regrouping (glow.py:218-222)
    s = s.contiguous().view(s.size(0), s.size(1), -1)                  # [B, L, 640], position-major
    (s * o["dspect"]).sum().backward()
    return s.detach().numpy(), W.grad.numpy(), bias.grad.numpy()


@pytest.mark.parametrize("c", uh.SMALL_CPU_CASES + (uh.Case(160, 1024, 2, 6, 150), uh.Case(256, 200, 2, 6, 160, "random")), ids=lambda c: c.id)
def test_reference_equals_float64_autograd(c):
    ref, bwd = uh.forward_reference(c.shape), uh.backward_reference(c.shape)
    spect, dW, db = _autograd(c)
    Lr = uh.padded_len(c.L)
    assert ref.spect.shape == (c.B, Lr, 640) and Lr >= c.L and not ref.spect[:, c.L:].any()
    scale = max(1.0, float(np.abs(spect).max()))
    assert np.abs(ref.spect[:, :c.L] - spect).max() <= 1e-12 * scale
    assert np.abs(bwd.dW - dW).max() <= 1e-12 * max(1.0, float(np.abs(dW).max()))
    assert np.abs(bwd.db - db).max() <= 1e-12 * max(1.0, float(np.abs(db).max()))
    # the sums of absolute values bound the sums themselves
    assert (np.abs(ref.spect) <= ref.S_fwd * (1 + 1e-12)).all() and (np.abs(bwd.dW) <= bwd.S_dW * (1 + 1e-12)).all()
    assert (np.abs(bwd.db) <= bwd.S_db * (1 + 1e-12)).all()


def test_case_list_is_what_the_kernels_accept():
    assert len(set(c.id for c in uh.CASES)) == len(uh.CASES)
    for c in uh.CASES + uh.NO_WS_CASES:
        assert c.accepted and c.hop % 8 == 0, c.id
    assert not uh.REJECTED.accepted
    assert [c.id for c in uh.CASES if not c.forward_supported] == [uh.Case(8, 72, 2, 40, 39, d, p).id for d in ("int", "random")
                                                                    for p in ("gemm", "scalar")]
    for hop in (160, 256):                                 # both hops have tail cases and cases without one
        assert {c.tail for c in uh.CASES if c.hop == hop} == {True, False}


@pytest.mark.parametrize("c", [c for c in uh.CASES + uh.NO_WS_CASES if c.data == "int" and c.path != "scalar"]
                         + [uh.Case(8, 40, 2, 6, 10)], ids=lambda c: c.id)
def test_integer_cases_are_exact_in_bf16_and_fp32(c):
    o = uh.operands(c.shape)
    for k in ("mel", "W", "dspect"):
        assert np.isin(o[k], (-1.0, 0.0, 1.0)).all()
    assert np.isin(o["bias"], (-2.0, -1.0, 0.0, 1.0, 2.0)).all()
    ref, bwd = uh.forward_reference(c.shape), uh.backward_reference(c.shape)
    print("%s: max S_fwd %d  S_dW %d  S_db %d" % (c.id, ref.S_fwd.max(), bwd.S_dW.max(), bwd.S_db.max()))
    assert ref.S_fwd.max() <= 256
    assert max(bwd.S_dW.max(), bwd.S_db.max()) < 2 ** 24
    for a in (ref.spect, bwd.dW, bwd.db):
        assert np.array_equal(a, np.rint(a))
    # exact in bf16: the rounded reference IS the reference
    assert np.array_equal(uh.bf16_to_f64(uh.bf16_bits(ref.spect)), ref.spect)
