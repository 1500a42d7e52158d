"""GPU: the bf16 WN training kernels (csrc/facppg_train_bf16.hip: facppg_wn_forward_bf16, facppg_wn_backward_bf16) held to a
float64 reference stage by stage -- every element of h, ts, acts, skip, out, dskip, dpre, dh, dspect, da0 and of every weight and
bias gradient, each stage's reference formed from the bits the kernels stored for the stage before (tests/wn_bf16_helpers.py
states the stages, the window bf16(r - d) <= g <= bf16(r + d) and the bound d).  28 cases -- one layer at every tile edge and the
Lr boundary with 1 to 9 chunks of 64 positions, two and three layers, eight layers with L around the dilation 128, five of them
accumulating dspect onto a previous buffer -- each under four launch structures (two launches per layer with k_bgemm's dspect
and plain-order 128-tiles; fused at 64 positions with k_wgrad2 and k_dspect; fused at 32; whatever the plan selects), and one
wide case, the first length at batch 12 at which every k_bgemm launch takes 128-column tiles.  Every margin row and every row
of [L, Lr) of the bf16 buffers must be exactly zero, rows [L, Lr) of skip and dspect untouched, every guard intact.

Measured on the MI355X (114 runs: 28 cases x 4 structures and the wide case twice; DESIGN.md, "The bf16 WN training kernels held
to a float64 reference"): every stage passes as the kernels stood.  Worst err / delta per stage (err = |g - r| less the half ulp
of the one admissible bf16 rounding) and the share of elements whose bits are not bf16(r), kernels (the stage in float32 on the CPU):
    h 0.12, 3.9e-5 (4.3e-5)      ts 3e-4, 8.3e-5 (7.7e-5)     acts 1e-4, 1.5e-4 (1.4e-4)    skip 0.004     out 0.003
    dskip 0.067, 4.2e-5 (4.2e-5) dpre 0.0012, 7.9e-5 (9.2e-5) dh 5e-4, 1.7e-4 (1.6e-4)      dspect 0.003   da0 0.002
    gradients: start_w 0.18  start_b 0.0015  in_w 0.12  in_b = cond_b 0.0055  cond_w 0.12  rs_w 0.12  rs_b 0.0019  end_w 0.23  end_b 0.085
G, the float32 error of the gate's formula the bound carries (MARGIN times): 2.3 U for tanh, 1.6 U for the sigmoid (measured
2.29 U / 1.59 U on the pre-activations of all these cases).  Per stage at most 4 c + 8 elements may differ from bf16(r), c being
the count of the stage in float32 on the CPU.
Run time: under 20 s for the 339 tests, CPU references included; the wide case 6.8 s (`two`) and 3.8 s (`default`, reference cached),
no other test above 0.6 s: a case's three tests share one run, its four structures one reference."""
import collections

import numpy as np
import pytest
import torch

import wn_bf16_helpers as wb
import wn_train_helpers as wt
from wn_bf16_helpers import NC, OK, EWORKSPACE

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(c, s, id="%s-%s" % (c.id, s)) for c in wb.CASES for s in wb.STRUCTURES]


@pytest.mark.parametrize("case,structure", PARAMS)
def test_forward_stages(case, structure):
    """h.0 .. h.(n_layers - 1), ts.i, acts.i (bf16), skip and out (fp32)"""
    wb.check(case, structure, wb.FORWARD)


@pytest.mark.parametrize("case,structure", PARAMS)
def test_backward_data_stages(case, structure):
    """dskip, dpre.i, dh.i (bf16), dspect (overwritten or accumulated) and da0 (fp32)"""
    wb.check(case, structure, wb.BACKWARD)


@pytest.mark.parametrize("case,structure", PARAMS)
def test_weight_and_bias_gradients(case, structure):
    """start, in, cond, res_skip and end weights and biases: NT products and column sums over the stored bf16 buffers"""
    wb.check(case, structure, wb.WEIGHTS)


@pytest.mark.parametrize("structure", ["two", "default"])
def test_wide_case(structure, monkeypatch):
    """B = 12, two layers, the first L at which plan_bgemm gives every k_bgemm launch 128-column tiles (the plan is asserted, the
    length comes out of it); `default` is what the plan selects for the shape by itself"""
    from facppg import lib
    case = wb.wide_case()
    wb.set_structure(monkeypatch, structure)
    r = lib.TrainLaunchReport()
    assert lib.load().facppg_train_bf16_launch_plan(case.n_layers, case.B, case.L, r) == 0
    if structure == "two":
        assert list(r.gemm_cols) == [128] * 5 and (r.dspect_bgemm, r.dspect_cols) == (1, 128) and (r.fused_fwd, r.fused_bwd) == (0, 0)
        assert lib.load().facppg_train_bf16_launch_plan(case.n_layers, case.B, case.L - 1, r) == 0 and 64 in list(r.gemm_cols)
    else:
        assert (r.fused_fwd, r.fused_bwd, r.tile_positions) == (1, 1, 64)
    wb.check(case, structure, wb.FORWARD + wb.BACKWARD + wb.WEIGHTS)


def test_short_state_or_scratch_is_refused_and_nothing_is_written():
    """state or scratch one byte short: FACPPG_EWORKSPACE from both entry points, and state, scratch, the outputs and every
    gradient still hold their poison.  (The backward needs the scratch without the summed gate biases behind it, which only the
    forward forms: its limit is facppg_wn_bf16_layout's scratch_end.)"""
    from facppg import lib
    Lh = lib.load()
    c = wb.Case(2, 2, 2, 150)
    nl, B, L, n_in = c.n_layers, c.B, c.L, c.n_in
    w, a0, spect_bits, dout, _ = wb.operands(c)
    o = wb.layout(c)
    wdev = collections.OrderedDict((k, wt.dev_input(v)) for k, v in w.items())
    wst = wt._struct(lib.WnWeights, wdev)
    grads = wt._grad_buffers(c.operands_key)
    gst = wt._struct(lib.WnGrads, grads)
    a0_d, dout_d = wt.dev_input(a0), wt.dev_input(dout)
    sp = torch.from_numpy(spect_bits.view(np.int16)).cuda()
    out_d, da0_d, dspect_d = wt.dev_output(B * 2 * n_in * L), wt.dev_output(B * n_in * L), wt.dev_output(B * o.Lr * NC)
    state_bytes, scratch_bytes = Lh.facppg_wn_bf16_state_bytes(nl, B, L), Lh.facppg_wn_bf16_scratch_bytes(nl, B, L)
    state, scratch = wt.dev_workspace(state_bytes), wt.dev_workspace(scratch_bytes)
    stream = lib.current_stream(a0_d.device)

    def untouched():
        torch.cuda.synchronize()
        assert bool((state[:state_bytes] == 0xFF).all()) and bool((scratch[:scratch_bytes] == 0xFF).all())
        assert wt.guard_intact(state, state_bytes) and wt.guard_intact(scratch, scratch_bytes)
        for t, n in ((out_d, B * 2 * n_in * L), (da0_d, B * n_in * L), (dspect_d, B * o.Lr * NC)):
            assert bool(torch.isnan(t[:n]).all()) and wt.guard_intact(t, n)
        for k, s in wt.weight_shapes(n_in, nl).items():
            assert bool(torch.isnan(grads[k][:int(np.prod(s))]).all()), k

    for st_b, sc_b in ((state_bytes - 1, scratch_bytes), (state_bytes, scratch_bytes - 1), (0, scratch_bytes), (state_bytes, 0)):
        rc = Lh.facppg_wn_forward_bf16(wst, n_in, nl, lib.ptr(a0_d), lib.ptr(sp), B, L, lib.ptr(out_d), lib.ptr(state), st_b, lib.ptr(scratch),
                                       sc_b, stream)
        assert rc == EWORKSPACE, (st_b, sc_b, rc)
        assert ("state" if st_b < state_bytes else "scratch") in wt.last_error()
        untouched()
    for st_b, sc_b in ((state_bytes - 1, scratch_bytes), (state_bytes, o.scratch_end - 1), (0, scratch_bytes), (state_bytes, 0)):
        rc = Lh.facppg_wn_backward_bf16(wst, gst, n_in, nl, lib.ptr(a0_d), lib.ptr(sp), lib.ptr(dout_d), B, L, lib.ptr(state), st_b,
                                        lib.ptr(da0_d), lib.ptr(dspect_d), 0, lib.ptr(scratch), sc_b, stream)
        assert rc == EWORKSPACE, (st_b, sc_b, rc)
        untouched()
    # and the exact sizes are accepted
    rc = Lh.facppg_wn_forward_bf16(wst, n_in, nl, lib.ptr(a0_d), lib.ptr(sp), B, L, lib.ptr(out_d), lib.ptr(state), state_bytes, lib.ptr(scratch),
                                   scratch_bytes, stream)
    torch.cuda.synchronize()
    assert rc == OK, wt.last_error()
    assert wt.guard_intact(state, state_bytes) and wt.guard_intact(scratch, scratch_bytes) and not bool(torch.isnan(out_d[:B * 2 * n_in * L]).any())
