"""No GPU: the two float64 references of tests/wn_train_helpers.py are held to float64 autograd of the oracle's WN stack
(oracle.waveglow.wn_forward: conv1d throughout), and the ternary cases of test_gpu_wn_train.py are shown to be exact: every
product and every row sum of facppg_wn_weight_grads has sum |a| |x| < 2^24 there, so every partial sum in any order is an
integer fp32 holds exactly and np.array_equal is the right comparison."""
import numpy as np
import pytest
import torch

import wn_train_helpers as wh
from oracle import waveglow as owg

SHAPES = (wh.Case(3, 3, 2, 37, "random"), wh.Case(1, 2, 1, 5, "random"))


def _oracle(case):
    """float64 autograd of oracle.waveglow.wn_forward -> (out, da0, dspect, name -> weight gradient)"""
    w, a0, spect, dout = wh.chain_operands(case)
    leaf = lambda x: torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    wl = {k: leaf(v) for k, v in w.items()}
    sd = {"WN.0.start.weight": wl["start_w"][:, :, None], "WN.0.start.bias": wl["start_b"],
          "WN.0.end.weight": wl["end_w"][:, :, None], "WN.0.end.bias": wl["end_b"]}
    for i in range(case.n_layers):
        sd["WN.0.in_layers.%d.weight" % i], sd["WN.0.in_layers.%d.bias" % i] = wl["in_w.%d" % i], wl["in_b.%d" % i]
        sd["WN.0.cond_layers.%d.weight" % i], sd["WN.0.cond_layers.%d.bias" % i] = wl["cond_w.%d" % i][:, :, None], wl["cond_b.%d" % i]
        sd["WN.0.res_skip_layers.%d.weight" % i], sd["WN.0.res_skip_layers.%d.bias" % i] = wl["rs_w.%d" % i][:, :, None], wl["rs_b.%d" % i]
    cfg = {"WN_config": {"n_channels": wh.CH, "n_layers": case.n_layers, "kernel_size": 3}}
    a0_t, spect_t = leaf(a0), leaf(spect)
    out = owg.wn_forward(sd, 0, cfg, a0_t, spect_t)
    (out * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    return out.detach().numpy(), a0_t.grad.numpy(), spect_t.grad.numpy(), {k: v.grad.numpy() for k, v in wl.items()}


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(b).max())), what


@pytest.mark.parametrize("c", SHAPES, ids=lambda c: c.id)
def test_stack_reference_equals_float64_autograd_of_the_oracle(c):
    ref, ref32 = wh.chain_reference(c)
    out, da0, dspect, grads = _oracle(c)
    _close(ref["out"], out, "out")
    _close(ref["da0"], da0, "da0")
    _close(ref["dspect"], dspect, "dspect")
    for k, g in grads.items():
        _close(ref["g." + k], g, k)
    assert set(ref) == set(ref32)
    # the float32 evaluation is the same function: close to float64, and not equal to it
    worst = {k: wh.ratio(ref32[k], ref[k]) for k in ref}
    assert 0 < max(worst.values()) < 1e-4, worst
    # what the kernels keep: the layer recursion restated from the kept tensors alone
    for i in range(c.n_layers - 1):
        t, s = ref["ts.%d" % i][:, :wh.CH], ref["ts.%d" % i][:, wh.CH:]
        assert (np.abs(t) < 1).all() and ((0 < s) & (s < 1)).all()
        rs_w = wh.chain_operands(c)[0]["rs_w.%d" % i].astype(np.float64)
        rs_b = wh.chain_operands(c)[0]["rs_b.%d" % i].astype(np.float64)
        res = np.einsum("mc,bcn->bmn", rs_w[:wh.CH], t * s) + rs_b[None, :wh.CH, None]
        _close(ref["h.%d" % (i + 1)], ref["h.%d" % i] + res, "h.%d" % (i + 1))


@pytest.mark.parametrize("c", SHAPES, ids=lambda c: c.id)
def test_weight_grad_reference_equals_float64_autograd_of_conv1d(c):
    """the NT products and row sums, formed on the kernel's padded buffers with NaN wherever the kernels write nothing"""
    ref, _ = wh.chain_reference(c)
    _, a0, spect, dout = wh.chain_operands(c)
    grads = _oracle(c)[3]
    o = wh.to_kernel_layout(ref, c, a0, spect, dout)
    assert np.isnan(o["spect"][:, :, c.L:]).all() and not o["h_all"][..., :wh.HALO].any() and not o["h_all"][..., wh.HALO + c.L:].any()
    got = wh.weight_grad_reference(o, c.n_in, c.n_layers, c.B, c.L)
    assert list(got) == list(wh.weight_shapes(c.n_in, c.n_layers))
    for k, g in grads.items():
        assert not np.isnan(got[k]).any(), k
        _close(got[k], g, k)
    assert got["rs_w.%d" % (c.n_layers - 1)].shape == (wh.CH, wh.CH)


def test_case_lists_cover_what_the_issue_names():
    cases = wh.WG_CASES
    assert len(set(c.id for c in cases)) == len(cases)
    assert {c.L for c in cases} == set(wh.WG_LENGTHS) and {c.B for c in cases} == {1, 3}
    assert {c.n_in for c in cases} == {1, 2, 3, 4} and {c.n_layers for c in cases} == {1, 2, 8}
    assert any(c.L < 2 ** (c.n_layers - 1) for c in cases) and any(c.L % 2 and c.n_in % 2 for c in cases)
    for L in wh.WG_LENGTHS:                                   # every length with both batch sizes
        assert {c.B for c in cases if c.L == L} == {1, 3}, L
    chain = wh.CHAIN_CASES
    assert {c.n_in for c in chain} == {1, 2, 3, 4} and {c.n_layers for c in chain} == {1, 3, 8} and {c.B for c in chain} == {1, 2}
    assert {c.L for c in chain} == {1, 63, 64, 65, 150, 240}
    assert not any(c.wide for c in chain + cases) and wh.WIDE_CASE.wide and wh.WIDE_CASE_2.wide
    assert not wh.Case(4, 1, 12, 4032, "random").wide                    # one tile fewer takes the 32-wide plan


@pytest.mark.parametrize("c", wh.WG_CASES, ids=lambda c: c.id)
def test_integer_cases_are_exact_in_fp32(c):
    o = wh.wg_operands(c)
    for k, v in o.items():
        live = v[~np.isnan(v)]
        assert np.isin(live, (-1.0, 0.0, 1.0)).all(), k
    ref, S = wh.wg_reference(c)
    worst = max(float(s.max()) for s in S.values())
    print("%s: largest sum |a| |x| %d" % (c.id, worst))
    assert worst < 2 ** 24
    for k in ref:
        assert np.array_equal(ref[k], np.rint(ref[k])) and (np.abs(ref[k]) <= S[k]).all(), k
