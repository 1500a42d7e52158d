"""GPU: the fp32 training direction of one WaveGlow WN stack -- facppg_wn_forward_save (k_wn_start, k_pack_w1/2, k_add_bias,
k_wn_layer<*, *, true>, k_wn_end), facppg_wn_backward_data (k_wn_end_bwd, three gemm_launch chains with the gate epilogue,
k_wn_start_bwd) and facppg_wn_weight_grads (k_wn_grad_tables, k_wgrad_f32, k_rowsum_f32) -- called directly and held to the
float64 references of tests/wn_train_helpers.py, element by element, with NaN in every buffer before the call, NaN in every
column the kernels are documented to mask, and sentinels behind every buffer.

a) facppg_wn_weight_grads alone on ternary operands (every sum an integer fp32 holds exactly,
   test_wn_train_reference_cpu.py): np.array_equal, 60 shapes.  Random operands: (K + 2) 2u S, K = B L terms, S = sum |a| |x|.
b) forward, backward and weight gradients chained on random operands, 16 shapes: per tensor max|err| / max|ref| against float64,
   allowed 4 x the same figure of the SAME reference evaluated in float32 on the CPU (floor 16 u).
c) the wide plan (64-wide tiles from 768 tiles on), B = 12, L = 4090: one layer (k_wn_layer<true, 2, true>) and two
   (k_wn_layer<false, 2, true>), same checks as b.

Measured on the MI355X: a) random worst err/tol 0.043; b) worst fraction of the allowance 0.98 (dpre), 0.90 (T / S), 0.88 (in_b),
everything else <= 0.72 (per tensor kind in DESIGN.md, "The fp32 WN training kernels held to a float64 reference"); c) <= 0.68.
As the kernels stood before this file, b) failed 11 of 16 shapes (h_i at 8 - 10 x the CPU's float32 error: the res rows' accumulator
chain started at h_in) and c) failed (weight gradients at up to 17 x: one accumulator chain over 49 080 positions); both chains
were changed, DESIGN.md.  The file takes 16 s: the 65 direct cases 4 s, the 16 chained 2 s, the wide cases 3 s and 7 s (both CPU
references included)."""
import time

import numpy as np
import pytest

import wn_train_helpers as wh

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda c: c.id)


@pytest.mark.parametrize("c", wh.WG_CASES, **_ids)
def test_weight_grads_ternary_operands_exact(c):
    rc, got = wh.run_weight_grads(c)
    assert rc == wh.OK, (rc, wh.last_error())
    ref, _ = wh.wg_reference(c)
    for k, want in ref.items():
        bad = np.argwhere(got[k] != want)
        assert bad.size == 0, "%s: %d of %d values differ, first at %s: got %g, want %g" % (
            k, len(bad), want.size, tuple(bad[0]), got[k][tuple(bad[0])], want[tuple(bad[0])])
    # the in and cond biases share one gradient: both copies are written
    for i in range(c.n_layers):
        assert np.array_equal(got["in_b.%d" % i], got["cond_b.%d" % i])


@pytest.mark.parametrize("c", wh.WG_RANDOM_CASES, **_ids)
def test_weight_grads_random_operands(c):
    rc, got = wh.run_weight_grads(c)
    assert rc == wh.OK, (rc, wh.last_error())
    ref, S = wh.wg_reference(c)
    worst = {}
    for k, want in ref.items():
        tol = (c.B * c.L + 2) * 2 * wh.U * S[k]
        err = np.abs(got[k] - want)
        assert (err <= tol).all(), k
        live = tol > 0
        if live.any():
            worst[k.split(".")[0]] = max(worst.get(k.split(".")[0], 0.0), float((err[live] / tol[live]).max()))
    print("%s: worst err/tol %s" % (c.id, " ".join("%s %.3f" % kv for kv in worst.items())))


def test_weight_grads_rejects_a_short_workspace():
    import torch
    lib, L = wh._lib()
    c = wh.Case(2, 2, 1, 5)
    dev = {k: wh.dev_input(v) for k, v in wh.wg_operands(c).items()}
    grads = wh._grad_buffers(c)
    nbytes = L.facppg_wn_weight_grads_workspace_bytes(c.n_layers)
    ws = wh.dev_workspace(nbytes)
    rc = L.facppg_wn_weight_grads(c.n_in, c.n_layers, *(lib.ptr(dev[k]) for k in ("a0", "spect", "h_all", "ts_all", "skip", "dout", "dpre_all",
                                                                                  "dh_all", "dskip")),
                                  c.B, c.L, wh._struct(lib.WnGrads, grads), lib.ptr(ws), nbytes - 1, lib.current_stream(ws.device))
    torch.cuda.synchronize()
    assert rc == wh.EWORKSPACE and bool((ws == 0xFF)[:nbytes].all())
    assert all(bool(torch.isnan(g[:-wh.GUARD]).all()) for g in grads.values())


def _kind(name):
    return name.split(".")[0] + ("." + name.split(".")[1] if name.startswith("g.") else "")


def _compare_chain(c):
    """-> kind of tensor -> (worst max|err| / max|ref| of the kernels, the CPU's in float32 at that tensor, worst kernel / allowance)"""
    ref, ref32 = wh.chain_reference(c)
    got = wh.run_chain(c)
    assert set(got) == set(ref), set(got) ^ set(ref)
    rows, failed = {}, []
    for k in sorted(ref):
        assert got[k].shape == ref[k].shape, k
        r_gpu, r_cpu = wh.ratio(got[k].astype(np.float64), ref[k]), wh.ratio(ref32[k], ref[k])
        allow = max(wh.MARGIN * r_cpu, wh.FLOOR)
        if r_gpu > allow:
            failed.append("%s: %.3g > %.3g (CPU float32 %.3g)" % (k, r_gpu, allow, r_cpu))
        q = rows.setdefault(_kind(k), [0.0, 0.0, 0.0])
        if r_gpu / allow > q[2]:
            q[:] = [r_gpu, r_cpu, r_gpu / allow]
    print("%s: max|err|/max|ref| kernels (CPU float32) [of allowance]: %s" % (
        c.id, "; ".join("%s %.2e (%.2e) [%.2f]" % (k, *v) for k, v in rows.items())))
    assert not failed, failed
    return rows


@pytest.mark.parametrize("c", wh.CHAIN_CASES, **_ids)
def test_chain_vs_float64_reference(c):
    _compare_chain(c)


@pytest.mark.parametrize("c", [wh.WIDE_CASE, wh.WIDE_CASE_2], **_ids)
def test_chain_wide_plan_vs_float64_reference(c):
    """B = 12, L = 4090: 768 tiles of 64 columns, the first shape that takes the wide plan.  One layer: k_wn_layer<true, 2, true>;
    two layers: k_wn_layer<false, 2, true> as well.  Both references (float64 and float32) run on the CPU inside this test."""
    t0 = time.time()
    assert c.wide
    _compare_chain(c)
    print("wide plan, %d layer(s): %.1f s" % (c.n_layers, time.time() - t0))
