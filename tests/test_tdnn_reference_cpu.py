"""CPU: the conditions under which test_gpu_tdnn_plans.py may compare the TDNN kernels (csrc/facppg_tdnn.hip) with the float64
reference of tdnn_helpers.py the way it does -- per case, without a GPU:

  * exact class: the chain's worst-case magnitude prod_l max_row ||W_l||_1 * max|x| + biases stays below 2^24 quanta (so every
    fp32 partial sum, in any order, is an integer number of quanta it can hold), the float64 result is a float32 number, at
    least a quarter of every ReLU layer's activations are non-zero, an output takes at least 16 values, every live column of
    every W is non-zero in some row and every gap tap is all zero;
  * output kernels: the logits are exact, a frame's logits spread over at most 40, the top posterior is below 0.9 in at least
    half the frames;
  * renorm: the zero frame reaches the 2^-66 floor and nothing else does; in the rounding class ||e|| <= 0.01 ||x||;
  * the reference itself against oracle/nnet3.py (the component-by-component float32 oracle) on models that go through the
    nnet3 writer and reader, within the 2e-6 test_nnet3_cpu.py uses; the float64 fold of the file model against plan_layers;
  * the case lists are non-empty and their ids unique."""
import numpy as np
import pytest

import tdnn_helpers as th
from common import decode, nnet3
from oracle import nnet3 as onnet3


def test_case_lists():
    assert len(th.EXACT_CASES) == 6 * len(th._plan_specs()) + 1 and len(th.ROUNDING_PLANS) >= 4 and len(th.RENORM_CASES) == 6
    ids = [cs.id for cs in th.EXACT_CASES]
    assert len(set(ids)) == len(ids)
    for cs in th.EXACT_CASES:
        assert cs.plan in th._plan_specs() and cs.entry in ("single", "batch") and (cs.entry == "batch" or len(cs.lengths) == 1)
    names = [th.rounding_plan(n, rn).name for n, rn in th.ROUNDING_PLANS]
    assert len(set(names)) == len(names)
    # what the plans are there for
    ctx = {n: (th.exact_plan(n).left, th.exact_plan(n).right) for n in th._plan_specs()}
    assert ctx["a_default"] == (6, 7) and ctx["b_left"] == (10, 0) and ctx["c_right"] == (0, 4) and ctx["d_point"] == (0, 0)
    e = th.exact_plan("e_gaps").layers[0]
    assert (e.taps, e.dil, e.first) == (7, 1, -4)
    f = th.exact_plan("f_dil9").layers[0]
    assert (f.taps, f.dil, f.first) == (2, 9, -7) and f.dil > 5
    split = lambda K: (lambda nch: 1 if nch < 8 else min(nch // 4, 16))((K + 63) // 64)         # gemm_split_k of facppg_gemm.h
    assert split(th.exact_plan("g_k500").layers[0].K) == 2 and split(th.exact_plan("h_k4096").layers[0].K) == 16
    assert all(split(l.K) == 1 for n in ("a_default", "b_left", "e_gaps") for l in th.exact_plan(n).layers)
    assert len(th.exact_plan("i_seven").layers) % 2 == 1 and len(th.exact_plan("i_two").layers) % 2 == 0
    cols = lambda p, lengths: sum((p.left + p.right + T + 3) // 4 * 4 for T in lengths)
    a = th.exact_plan("a_default")
    assert cols(a, th.BATCHES[0]) == 252 and cols(a, th.BATCHES[1]) > 256
    assert cols(th.exact_plan("d_point"), th.POINT_BATCH) <= 32
    assert max(cols(th.exact_plan(n), th.BATCHES[1]) for n in th._plan_specs()) <= 600


@pytest.mark.parametrize("name", list(th._plan_specs()))
def test_exact_plan_conditions(name):
    p = th.exact_plan(name)
    bound = th.exact_bound(p)
    print("%s: worst-case magnitude %.3g quanta" % (name, bound))
    assert bound < 2 ** 24
    spec = th._plan_specs()[name][1]
    for l, W, b, (_, offsets, _, _) in zip(p.layers, p.W, p.b, spec):
        assert W.dtype == b.dtype == np.float32 and W.shape == (l.out_dim, l.K)
        assert np.array_equal(W, np.rint(W)) and np.array_equal(b, np.rint(b)) and l.renorm == 0
        live = th.grid(offsets)[3]
        W3 = W.reshape(l.out_dim, l.taps, l.in_dim)
        for t in range(l.taps):
            if t in live:
                assert (W3[:, t, :] != 0).any(axis=0).all(), "a column no row reads would hide a wrong source frame"
            else:
                assert not W3[:, t, :].any()
    for cs in [c for c in th.EXACT_CASES if c.plan == name]:
        for u in th.utterances(p, cs.lengths):
            assert np.abs(u).max() <= 3 and np.array_equal(u, np.rint(u))
            r = th.reference(p, u)
            assert r.sum_abs <= bound
            assert np.array_equal(r.y.astype(np.float32).astype(np.float64), r.y) and np.array_equal(r.y, np.rint(r.y))
            if u.shape[0] >= 5:
                assert np.unique(r.y).size >= 16
            if u.shape[0] >= 37:
                for l, a in zip(p.layers, r.acts):
                    assert not l.relu or (a > 0).mean() >= 0.25


@pytest.mark.parametrize("M", th.SOFTMAX_M)
def test_softmax_plan_conditions(M):
    p = th.softmax_plan(M)
    assert th.exact_bound(p) < 2 ** 24 and p.out_dim == M
    q = th.SOFTMAX_SCALE
    seen = 0
    for lengths in ((37,),) + th.BATCHES[1:]:
        for u in th.utterances(p, lengths):
            r = th.reference(p, u)
            assert np.array_equal(r.y / q, np.rint(r.y / q)) and np.array_equal(r.y.astype(np.float32).astype(np.float64), r.y)
            assert (r.y.max(1) - r.y.min(1)).max() <= 40
            if u.shape[0] >= 37:
                assert (r.out.max(1) < 0.9).mean() >= 0.5 and np.allclose(r.out.sum(1), 1.0, atol=1e-12)
                assert (r.y.max(1) - r.y.min(1)).max() >= 4          # ... and the posteriors are not all alike
                seen += 1
    assert seen


@pytest.mark.parametrize("C,rms", th.RENORM_CASES)
def test_renorm_plan_conditions(C, rms):
    p = th.renorm_plan(C, rms)
    assert th.exact_bound(p) < 2 ** 24 and all((b <= 0).all() for b in p.b)
    x = th.renorm_features(C, rms)
    r = th.reference(p, x, exact_gemm=True)
    assert r.sum_abs < 2 ** 24 and r.zero_frames == 1 and not r.y[th.RENORM_ZERO_FRAME].any()
    live = np.delete(np.arange(th.RENORM_T), th.RENORM_ZERO_FRAME)
    assert np.allclose(np.sqrt((r.y[live] ** 2).mean(1)), rms, rtol=1e-12)             # the contract: rms of a frame = target
    assert (r.y[live] > 0).mean() >= 0.25
    rel = (r.e[live] / np.maximum(r.y[live], 1e-300))[r.y[live] > 0]
    print("C=%d rms=%g: relative bound %.3g u .. %.3g u" % (C, rms, rel.min() / th.U, rel.max() / th.U))
    assert rel.max() <= 1.001 * ((C + 3) / 2 + 5) * th.U                                                   # the bound is a rounding bound


@pytest.mark.parametrize("name,renorm", th.ROUNDING_PLANS)
def test_rounding_plan_conditions(name, renorm):
    p = th.rounding_plan(name, renorm)
    for lengths, _ in th.ROUNDING_SHAPES:
        for u in th.utterances(p, lengths, "normal"):
            r = th.reference(p, u)
            assert r.zero_frames == 0 and r.renorm_ratio <= 0.01
            assert np.isfinite(r.e).all() and np.abs(r.y).max() > 0.5
            if renorm:
                assert r.renorm_ratio > 0
            for l, a in zip(p.layers, r.acts):
                assert not l.relu or (a > 0).mean() >= 0.25


@pytest.mark.parametrize("name,i", th.ROUNDING_LAYERS)
def test_layer_plan_conditions(name, i):
    """one layer's bound is g_l S alone (the GPU test also holds the rms of err / (u S) below sqrt(K), where a bfloat16 product
    would sit near 2^15 / sqrt(K))"""
    p = th.layer_plan(name, i)
    assert len(p.layers) == 1 and p.layers[0] == th.rounding_plan(name).layers[i]
    for lengths, _ in th.ROUNDING_SHAPES:
        for u in th.utterances(p, lengths, "normal"):
            r = th.reference(p, u)
            K = p.layers[0].K
            assert np.allclose(r.e, (K + 2) * 2 * th.U * r.S, rtol=1e-12)
            assert r.e.max() < 5e-3


def _oracle_net(name, **kw):
    in_dim, specs, _ = th._plan_specs()[name]
    splices = tuple(s for _, s, _, _ in specs[:-1])
    hidden = specs[0][0]
    return in_dim, nnet3.synthetic_tdnn(input_dim=in_dim, hidden=hidden, output_dim=specs[-1][0], splices=splices, seed=8, **kw)


def _plan_of(net):
    """plan_layers' fused chain as a Plan (float64 weights)"""
    layers, final = nnet3.plan_layers(net)
    tab, cin = [], layers[0]["W"].shape[1] // layers[0]["taps"]
    for l in layers:
        tab.append(th.Layer(l["W"].shape[0], cin, l["taps"], l["dil"], l["first"], l["act"] == "relu", float(l["renorm"] or 0.0)))
        cin = l["W"].shape[0]
    return th.Plan("planned", tuple(tab), {"none": 0, "softmax": 1, "log-softmax": 2}[final], tuple(l["W"] for l in layers),
                   tuple(l["b"] for l in layers), w_round=True)


@pytest.mark.parametrize("name,kw", [("a_default", dict(norm="batchnorm", lda=True)), ("b_left", dict(norm="renorm", lda=False, output="log-softmax")),
                                     ("c_right", dict(norm="batchnorm", lda=False)), ("e_gaps", dict(norm="renorm", lda=False)),
                                     ("f_dil9", dict(norm="batchnorm", lda=True))])
def test_reference_against_the_oracle(tmp_path, name, kw):
    """The frame-axis reference and the component-by-component oracle are the same function of a model file, edges included
    (utterances shorter than the context, too): 2e-6 on posteriors, as test_nnet3_cpu.py holds plan_layers to the oracle."""
    in_dim, net = _oracle_net(name, **kw)
    path = str(tmp_path / "final.raw")
    nnet3.write_nnet3(path, net)
    model = decode.read_nnet3_model(path)
    p = _plan_of(model)
    assert (p.left, p.right) == model.context()
    for T in (1, 2, 5, 37):
        u = th.features(in_dim, T, "normal")
        want = onnet3.forward(model, u)
        got = th.reference(p, u).out
        if p.final_op == 2:
            got, want = np.exp(got), np.exp(want)
        assert got.shape == want.shape and np.abs(got - want).max() <= 2e-6, (T, np.abs(got - want).max())


def test_file_model_fold(tmp_path):
    """fold_file_model (written from the graph) gives the reference the same function as the oracle (2e-6) and the same
    weights as plan_layers up to float64 rounding -- what the GPU test then holds the blob order and the folding to."""
    net = th.file_model()
    path = str(tmp_path / "final.raw")
    nnet3.write_nnet3(path, net)
    model = decode.read_nnet3_model(path)
    p, q = th.fold_file_model(model), _plan_of(model)
    assert (p.left, p.right) == (10, 4) == model.context() and p.final_op == q.final_op == 1
    assert [dataclasses_tuple(l) for l in p.layers] == [dataclasses_tuple(l) for l in q.layers]
    for a, b in zip(p.W + p.b, q.W + q.b):
        assert a.dtype == np.float64 and np.allclose(a, b, rtol=1e-12, atol=1e-14)
    for T in (1, 5, 37):
        u = th.features(40, T, "normal")
        r = th.reference(p, u)
        assert np.abs(r.out - onnet3.forward(model, u)).max() <= 2e-6
        assert np.isfinite(r.e).all()


def dataclasses_tuple(l):
    return (l.out_dim, l.in_dim, l.taps, l.dil, l.first, l.relu, l.renorm)


def test_bounds_are_rounding_bounds():
    """the output kernels' bounds as functions: monotone in M, a few hundred u at the largest M, and the reference's own float64
    error is far below them"""
    E1, E2 = 4.0, 4.0
    assert th.softmax_rel_bound(8, E1) < th.softmax_rel_bound(600, E1) < 700 * th.U
    assert th.mono_rel_bound(600, E1) < 1300 * th.U
    assert float(th.logsoftmax_abs_bound(600, E1, E2, np.array(-10.0))) < 700 * th.U
    assert 600 * 2.0 ** -53 < 1e-6 * th.softmax_rel_bound(8, E1)
