"""What the direct GEMM tests (test_gpu_gemm.py) stand on, checked without a GPU: the float64 reference of gemm_helpers.py
against torch's conv1d, the probe's argument struct against its ctypes binding, gemm_launch's argument checks (they return
before any HIP call), and the condition under which the exact class IS exact: sum |w||x| < 2^24 for every case."""
import ctypes as c

import numpy as np
import pytest
import torch

import gemm_helpers as gh
from gemm_helpers import Case


@pytest.mark.parametrize("taps", [1, 3, 5])
@pytest.mark.parametrize("dil", [1, 2, 128])
@pytest.mark.parametrize("pad", ["0", "same", "out"])
def test_reference_equals_conv1d(taps, dil, pad):
    """The header's formula is torch's cross-correlation with padding = pad * dil; pad "out" puts every source column of
    the first taps in front of the row (pad * dil > N)."""
    N = 300 if dil == 128 else 37
    cs = Case(M=7, Cin=6, taps=taps, dil=dil, pad={"0": 0, "same": (taps - 1) // 2, "out": N // dil + 1}[pad], N=N, B=2, data="normal")
    d = gh.make_data(cs)
    pre, S = gh.conv_sum(cs, d.W, d.X)
    x = torch.from_numpy(d.X.astype(np.float64))
    x = torch.nn.functional.pad(x, (0, dil * (taps - 1)))   # conv1d's output is as long as the reference's: zeros behind the row
    want = torch.nn.functional.conv1d(x, torch.from_numpy(d.W.astype(np.float64)), padding=cs.pad * dil, dilation=dil)[..., :N]
    assert want.shape == (2, 7, N)
    np.testing.assert_allclose(pre, want.numpy(), rtol=0, atol=1e-12)
    if pad != "out" or taps * dil > N:
        assert np.count_nonzero(pre) > 0
    assert (S >= np.abs(pre) - 1e-12).all()


def test_reference_windows_and_validity():
    """n_valid, src_hi and col0 by hand on a one-tap shift: C[n] = w X[n + 2] where the source is valid."""
    cs = Case(M=1, Cin=1, taps=1, pad=-2, N=10, B=2, col0=3, src_hi=9, n_valid=(4, 6), mul=2, add=-1, data="normal")   # valid 7, 11
    d = gh.make_data(cs)
    assert [cs.bounds(b) for b in range(2)] == [(7, 7), (10, 9)]
    r = gh.reference(cs)
    assert r.win[0, 0].tolist() == [False] * 3 + [True] * 4 + [False] * 3 and r.win[1, 0].tolist() == [False] * 3 + [True] * 7
    x = d.X.astype(np.float64) * float(d.W[0, 0, 0])
    assert np.array_equal(r.pre[0, 0], np.r_[x[0, 0, 2:7], np.zeros(5)])
    assert np.array_equal(r.pre[1, 0], np.r_[x[1, 0, 2:9], np.zeros(3)])


def test_probe_struct_matches_binding():
    P, _ = gh.probe()
    assert P.probe_args_size() == c.sizeof(gh.Args)
    # packed_a_float4s: (M / 32 row blocks) * (K / 8 + 1 k-groups) * 64 lanes + 3 * 64, 16 bytes each
    assert P.probe_packed_a_bytes(33, 65) == (2 * (128 // 8 + 1) * 64 + 192) * 16


def _dummy_args(**kw):
    """arguments that pass every check, with pointers that are never followed (the checks come before any launch)"""
    buf = (c.c_float * 64)()
    p = c.addressof(buf)
    a = gh.Args(A=p, X=p, C=p, M=8, N=16, Cin=512, taps=1, dil=1, pad=0, B=1, ldx=16, ldc=16, n_valid_mul=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a, buf


@pytest.mark.parametrize("bad", [dict(col0=16), dict(col0=17), dict(col0=-1), dict(A=None), dict(X=None), dict(C=None), dict(M=0),
                                 dict(N=0), dict(N=-3), dict(Cin=0), dict(taps=0), dict(B=0), dict(M=-1)],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_gemm_launch_rejects_bad_arguments(bad):
    P, _ = gh.probe()
    a, buf = _dummy_args(**bad)
    assert P.probe_gemm(c.byref(a), None) == gh.EINVAL
    assert "gemm_launch: bad arguments" in gh.last_error()


def test_gemm_launch_rejects_a_short_splitk_buffer():
    """K = 512 is the split threshold: two splits, so 2 * B * M * N floats; one byte less is FACPPG_EWORKSPACE."""
    P, _ = gh.probe()
    need = 2 * 3 * 8 * 16 * 4
    a, buf = _dummy_args(B=3, splitk_ws_bytes=need - 1)
    a.splitk_ws = c.addressof(buf)
    assert P.probe_gemm(c.byref(a), None) == gh.EWORKSPACE
    assert "needs %d" % need in gh.last_error()


def test_case_ids_are_unique():
    for cases in (gh.EXACT_CASES, gh.ROUNDING_CASES):
        ids = [cs.id for cs in cases]
        assert len(set(ids)) == len(ids)


def test_listed_values_are_covered():
    """every value the case lists promise appears in the exact class"""
    E = gh.EXACT_CASES
    have = lambda f: {f(cs) for cs in E}
    assert {1, 31, 32, 33, 127, 128, 129} <= have(lambda cs: cs.M)
    assert {1, 31, 32, 33, 63, 64, 65, 256, 257, 300} <= have(lambda cs: cs.N)
    assert {40, 64, 65, 448, 512, 832, 2560, 8128} <= {cs.K for cs in E if cs.split} & {cs.K for cs in E if not cs.split}
    assert {(1, 40), (1, 448), (3, 5), (5, 5), (80, 5)} <= have(lambda cs: (cs.Cin, cs.taps))
    assert {1, 3, 5, 64, 80, 600} <= have(lambda cs: cs.Cin)
    assert {(t, d) for t in (1, 3, 5) for d in (1, 2, 128)} <= have(lambda cs: (cs.taps, cs.dil))
    assert any(cs.pad * cs.dil > cs.N for cs in E)
    for split in (False, True):
        W = [cs for cs in E if cs.split == split and cs.K >= 512]
        assert {1, 31, 32, 45} <= {cs.col0 for cs in W}
        assert {(300, 60), (300, 10)} <= {(cs.N, cs.col0) for cs in W}
        for nv in (False, True):
            assert {-3, 0, 7} <= {cs.src_hi - cs.N for cs in W if (cs.n_valid is not None) == nv and cs.src_hi}
        assert {0, 1} <= {cs.skip for cs in W}
        assert any(cs.B == 3 and cs.n_valid == (cs.N, 0, 17) for cs in W)
        assert any(cs.mul == 2 and cs.add == -1 for cs in W)
        assert any(cs.n_valid and max(cs.n_valid) * cs.mul + cs.add > cs.N for cs in W)
        assert any(cs.x_shared for cs in W) and any(cs.ct for cs in W) and any(cs.gate for cs in W)
    assert {"transposed", "reversed", "wn_bwd"} <= have(lambda cs: cs.wview)


@pytest.mark.parametrize("cs", gh.EXACT_CASES, ids=lambda cs: cs.id)
def test_exact_class_is_exact(cs):
    """With sum |w||x| < 2^24 every partial sum, in any order, is an integer float32 holds; every later step of the epilogue
    must be a float32 number too.  Computed per case, not assumed."""
    r = gh.reference(cs)
    assert r.S.max() < 2.0 ** 24
    assert r.f32_exact
