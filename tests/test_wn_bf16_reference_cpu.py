"""CPU: the tools test_gpu_wn_bf16.py holds the bf16 WN training kernels with (tests/wn_bf16_helpers.py) -- bf16_round against
torch's conversion; the staged reference, rounding switched off and fed with its own outputs, against the autograd reference of
the fp32 file (so the stage formulas are the stack's mathematics); the acceptance functions against outputs damaged the way
kernels go wrong; the float32 error of the gate's formula under the pinned constants; the case list."""
import numpy as np
import pytest
import torch

import wn_bf16_helpers as wb
import wn_train_helpers as wt
from wn_bf16_helpers import CH, HALO, NC, U


def _torch_bf16(x32):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).bfloat16().double().numpy()


def test_bf16_round_is_torchs_conversion():
    """on float32 inputs (torch converts through float32, so only those are rounded once): random values over the whole exponent
    range, exact ties with even and odd neighbours, the subnormal range and its border, +-0, the largest finite value"""
    g = np.random.Generator(np.random.PCG64(1))
    x = (g.standard_normal(200000) * np.exp2(g.integers(-140, 127, 200000))).astype(np.float32)
    m = np.arange(128, 257, dtype=np.float64)                                  # 8-bit significands and the next binade's first
    ties = np.concatenate([(m + 0.5) * 2.0 ** e for e in (-140, -134, -133, -127, -126, -30, -8, 0, 7, 100, 119)])
    near = np.concatenate([ties * (1 + 2.0 ** -20), ties * (1 - 2.0 ** -20)])
    small = np.array([0.0, -0.0, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -126, 2.0 ** -126 - 2.0 ** -134, 255.5 * 2.0 ** -133,
                      3.3895313892515355e38, 3.3961775292304e38, 3.4e38])
    v = np.concatenate([x.astype(np.float64), ties, -ties, near, -near, small, -small]).astype(np.float32)
    got, want = wb.bf16_round(v.astype(np.float64)), _torch_bf16(v)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # one rounding, not two: a float64 just above a tie must go up although its float32 image is the tie itself
    assert wb.bf16_round(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0 + 2.0 ** -7 and wb.bf16_round(1.0 + 2.0 ** -8) == 1.0
    assert np.array_equal(wb.bf16_to_f64(wb.bf16_bits(v.astype(np.float64))), want)


def _self_fed(case, rnd):
    w, a0, spect, dout = wt.chain_operands(case.operands_key)
    spect_pm = rnd(spect.transpose(0, 2, 1).astype(np.float64))
    return (w, a0, spect, dout), wb.staged_reference(case, w, a0, spect_pm, dout, kernel=None, rnd=rnd)


@pytest.mark.parametrize("case", wb.SMALL_CPU_CASES, ids=lambda c: c.id)
def test_stage_formulas_are_the_stacks_mathematics(case):
    """no rounding, every stage fed with the stage before: forward, every intermediate gradient and every weight gradient equal
    the float64 autograd reference (wn_train_helpers.stack_reference) to 1e-12 of each tensor's largest entry"""
    (w, a0, spect, dout), ref = _self_fed(case, wb.identity)
    auto = wt.stack_reference(w, a0, spect, dout, "float64")
    pm = lambda x: x.transpose(0, 2, 1)
    want = {"out": pm(auto["out"]), "skip": pm(auto["skip"]), "dskip": pm(auto["dskip"]), "dspect": pm(auto["dspect"]), "da0": auto["da0"]}
    for i in range(case.n_layers):
        want["h.%d" % i], want["ts.%d" % i] = pm(auto["h.%d" % i]), pm(auto["ts.%d" % i])
        want["acts.%d" % i] = want["ts.%d" % i][..., :CH] * want["ts.%d" % i][..., CH:]
        want["dpre.%d" % i], want["dh.%d" % i] = pm(auto["dpre.%d" % i]), pm(auto["dh.%d" % i])
    for k in wt.weight_shapes(case.n_in, case.n_layers):
        want["g." + k] = auto["g." + k]
    assert sorted(want) == sorted(k for k, v in ref.items() if v.kind != "none")
    for k, x in want.items():
        assert ref[k].r.shape == x.shape, k
        assert wt.ratio(ref[k].r, x) <= 1e-12, (k, wt.ratio(ref[k].r, x))
        assert (ref[k].delta >= 0).all() and np.isfinite(ref[k].delta).all(), k


def _as_stored(ref):
    """a 'kernel output' made of the reference itself: bf16 stages rounded once, fp32 stages as float32"""
    return {k: (wb.bf16_round(v.r) if v.kind == "bf16" else v.r.astype(np.float32).astype(np.float64)) for k, v in ref.items() if v.kind != "none"}


CONTROL = wb.Case(4, 2, 2, 70)      # two layers (res and skip rows), two items, a partial second chunk of 64 and a partial tile of 32


@pytest.fixture(scope="module")
def control():
    c = CONTROL
    (w, a0, spect, dout), ref = _self_fed(c, wb.bf16_round)
    got = _as_stored(ref)
    spect_pm = wb.bf16_round(spect.transpose(0, 2, 1).astype(np.float64))
    # the reference as the GPU test forms it: every stage from the stored operands
    staged = wb.staged_reference(c, w, a0, spect_pm, dout, kernel=wb.kernel_operands(c, got))
    return c, w, spect_pm, got, staged


def _rejected(staged, got, stage):
    res = wb.judge(staged, got)
    with pytest.raises(AssertionError):
        wb.assert_accepted(res)
    return [k for k, v in res.items() if v.failures] == [stage]


def test_the_undamaged_output_is_accepted(control):
    c, w, spect_pm, got, staged = control
    res = wb.judge(staged, got)
    wb.assert_accepted(res)
    assert max(v.worst for v in res.values()) <= 1.0
    assert set(res) == set(got)


def test_a_tap_one_row_off_at_a_tile_edge_is_rejected(control):
    """layer 1 (dilation 2), tap 0 of position 32 reads row 31 instead of row 30: only ts.1 / acts.1 of that position change"""
    c, w, spect_pm, got, staged = control
    b, n, i, d = 1, 32, 1, 2
    h = got["h.1"]
    win = wb.bf16_round(w["in_w.1"].astype(np.float64))[:, :, 0]
    pre = staged["pre.1"].r[b, n] + win @ (h[b, n - d + 1] - h[b, n - d])
    bad = dict(got)
    bad["ts.1"] = got["ts.1"].copy()
    bad["ts.1"][b, n] = wb.bf16_round(wb.gate_f64(pre))
    assert _rejected(staged, bad, "ts.1")


def test_a_dropped_last_partial_chunk_is_rejected(control):
    """the weight gradient of layer 0's taps without positions [64, 70) of the last item"""
    c, w, spect_pm, got, staged = control
    dpre, h = got["dpre.0"][-1:, 64:], got["h.0"][-1:]
    bad = dict(got)
    bad["g.in_w.0"] = got["g.in_w.0"] - np.stack([wb.F64.nt(dpre, wb._shift(h, tap - 1)[:, 64:]) for tap in range(3)], axis=-1)
    assert _rejected(staged, bad, "g.in_w.0")


def test_a_missing_column_sum_slice_is_rejected(control):
    """in_b / cond_b of layer 1 without one of the 256 row slices of the B L rows (the slice that holds row 70, the first of item 1)"""
    c, w, spect_pm, got, staged = control
    R = c.B * c.L
    r0, r1 = next((R * sl // 256, R * (sl + 1) // 256) for sl in range(256) if R * sl // 256 <= c.L < R * (sl + 1) // 256)
    assert (r0, r1) == (c.L, c.L + 1)
    rows = got["dpre.1"].reshape(R, 2 * CH)[r0:r1].sum(axis=0)
    bad = dict(got)
    bad["g.in_b.1"] = got["g.in_b.1"] - rows
    assert _rejected(staged, bad, "g.in_b.1")
    bad["g.in_b.1"], bad["g.cond_b.1"] = got["g.in_b.1"], got["g.cond_b.1"] - rows      # the second copy of the same sum is held too
    assert _rejected(staged, bad, "g.cond_b.1")


def test_a_missing_layer_in_dspect_is_rejected(control):
    c, w, spect_pm, got, staged = control
    bad = dict(got)
    bad["dspect"] = got["dspect"] - got["dpre.1"] @ wb.bf16_round(w["cond_w.1"].astype(np.float64))
    assert _rejected(staged, bad, "dspect")


def test_a_dirty_padding_row_is_rejected():
    nl, B, L, Lr = 2, 2, 70, 128
    Lp = HALO + Lr + HALO

    def buffers():
        v = {"h": np.zeros((nl + 1, B, Lp, CH), np.int16), "dpre": np.zeros((nl, B, Lp, 2 * CH), np.int16), "ts": np.zeros((nl, B, Lr, 2 * CH), np.int16),
             "acts": np.zeros((nl, B, Lr, CH), np.int16), "dh": np.zeros((nl + 1, B, Lr, CH), np.int16), "dskip": np.zeros((B, Lr, CH), np.int16)}
        for k in ("h", "dpre"):
            v[k][:, :, HALO:HALO + L] = 0x3F80
        for k in ("ts", "acts", "dh"):
            v[k][:, :, :L] = 0x3F80
        v["dskip"][:, :L] = 0x3F80
        v["h"][nl, :, HALO:HALO + L] = -1
        v["dh"][nl, :, :L] = -1
        return v
    wb.check_padding(buffers(), nl, L)
    spots = [("h", (1, 1, HALO - 1, 7)), ("h", (0, 0, HALO + L, 0)), ("h", (2, 1, Lp - 1, 255)), ("dpre", (1, 0, HALO + L, 300)),
             ("dpre", (0, 1, 0, 0)), ("ts", (1, 1, L, 511)), ("acts", (0, 0, Lr - 1, 3)), ("dh", (0, 1, L, 0)), ("dh", (2, 0, L + 1, 9)),
             ("dskip", (1, L, 255))]
    for name, ix in spots:
        v = buffers()
        v[name][ix] = 0x0001                                  # the smallest subnormal counts
        with pytest.raises(AssertionError):
            wb.check_padding(v, nl, L)


def test_window_admits_one_rounding_and_nothing_else():
    """the per-element window: both neighbours of a reference within delta of a tie are admitted, the next value is not; an fp32
    output is held to delta itself; NaN is never admitted"""
    r = np.array([1.0 + 2.0 ** -8 - 1e-9, 1.0 + 2.0 ** -8 + 1e-9, 3.0, 3.0])
    ref = wb.Ref(r, np.array([1e-8, 1e-8, 1e-8, 1e-8]), r.astype(np.float32), "bf16")
    assert not wb.violations(np.array([1.0, 1.0, 3.0, 3.0]), ref).any()
    assert not wb.violations(np.array([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, 3.0, 3.0]), ref).any()
    assert wb.violations(np.array([1.0 - 2.0 ** -8, 1.0 + 2.0 ** -6, 3.0 + 2.0 ** -6, np.nan]), ref).all()
    f = wb.Ref(r, np.full(4, 1e-8), r.astype(np.float32), "f32")
    assert not wb.violations(r + 0.9e-8, f).any() and wb.violations(r + 1.1e-8, f).all() and wb.violations(np.full(4, np.nan), f).all()
    assert wb.mismatch_allowance(0) == 8 and wb.mismatch_allowance(5) == 28 and wb.mismatch_allowance(100) == 408


def test_gate_formula_error_in_float32_is_under_the_pinned_constants():
    """G as the GPU test uses it: gate_ts's formula in NumPy float32 against float64 over the pre-activations of every GPU case's
    reference, the wide case included, is under GATE_ERR_T / GATE_ERR_S (which the bound multiplies by MARGIN) and within a tenth
    of U of them.  A dense sweep of [-20, 20], beyond the clamp on both sides, is printed next to it: the formula is a little
    worse there (2.59 U for tanh) than anywhere the cases go."""
    worst_t, worst_s = 0.0, 0.0
    for case in [c for c in wb.CASES if not c.accumulate] + [wb.wide_case()]:
        w, a0, spect, dout = wt.chain_operands(case.operands_key)
        spect_pm = wb.bf16_round(spect.transpose(0, 2, 1).astype(np.float64))
        ref = wb.staged_reference(case, w, a0, spect_pm, dout, kernel=None, forward_only=True)
        for i in range(case.n_layers):
            t, s = wb.measure_gate_error(ref["pre.%d" % i].r)
            worst_t, worst_s = max(worst_t, t), max(worst_s, s)
    sweep = np.linspace(-20, 20, 400001)
    t, s = wb.measure_gate_error(np.tile(sweep.reshape(-1, 1, 1), (1, 2, CH)).reshape(-1, 2 * CH))
    print("gate formula in float32: worst |dT| %.3g U, |dS| %.3g U on the cases; %.3g U, %.3g U on the sweep" % (worst_t / U, worst_s / U, t / U, s / U))
    assert wb.GATE_ERR_T - 0.1 * U <= worst_t <= wb.GATE_ERR_T and wb.GATE_ERR_S - 0.1 * U <= worst_s <= wb.GATE_ERR_S


def test_case_list():
    ids = [c.id for c in wb.CASES]
    assert len(set(ids)) == len(ids) == 28
    assert {c.n_in for c in wb.CASES} == {1, 2, 3, 4}
    assert {c.n_layers for c in wb.CASES} == {1, 2, 3, 8}
    assert {c.n_layers for c in wb.CASES if c.accumulate} == {1, 2, 3, 8}
    assert list(wb.STRUCTURES) == ["two", "fused64", "fused32", "default"] and wb.STRUCTURES["default"] == {}
    one = [c for c in wb.CASES if c.n_layers == 1 and not c.accumulate]
    assert {1, 2, 3, 4, 8} <= {c.B * -(-c.L // 64) for c in one}                   # chunks of 64 positions below the split limit of 8
    assert {c.L for c in wb.CASES if c.n_layers == 8} >= {1, 63, 65, 127, 128, 129, 257}
    w = wb.wide_case()
    assert (w.n_layers, w.B, w.L) == (2, 12, 15 * 128 + 1)          # ceil(L / 128) = 16: the first length of the 16th tile
