"""CPU: facppg_wn_bf16_layout, the host-only query of where facppg_wn_forward_bf16 / facppg_wn_backward_bf16 keep each stage inside
the caller's `state` and `scratch` (csrc/facppg_train_plan.h: state_layout, scratch_layout) -- what tests/wn_bf16_helpers.py reads the
kernels' buffers with.  The byte counts themselves are pinned once, by test_buffer_sizes of tests/test_train_plan_cpu.py; here
the offsets are held to the size queries that test pins (facppg_wn_bf16_state_bytes, facppg_wn_bf16_scratch_bytes,
facppg_glow_bf16_layout) and to the images' shapes."""
import pytest

from facppg import lib as flib

EINVAL = -1
# the shapes test_train_plan_cpu.py pins the buffer sizes at; L on and next to the 128 boundary; eight layers of one position
SHAPES = [(1, 1, 1), (2, 2, 65), (8, 3, 1250), (8, 12, 1250), (1, 3, 128), (3, 2, 129), (8, 1, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_stage_offsets_inside_state_and_scratch(shape):
    """facppg_wn_bf16_layout: where the stand-alone WN calls keep h, ts, acts, skip (state) and dpre, dh, dskip (scratch).  Pieces
    are 256-byte aligned, in this order, without overlap; the per-layer strides are the images' sizes; the state ends at
    facppg_wn_bf16_state_bytes, the scratch (whose first pieces are the packed weight images) at facppg_wn_bf16_scratch_bytes minus
    the [8][512] summed gate biases behind it."""
    L = flib.load()
    nl, B, Lg = shape
    o = flib.WnBf16Offsets()
    assert L.facppg_wn_bf16_layout(nl, B, Lg, o) == 0
    Lr = L.facppg_wn_bf16_padded_len(Lg)
    assert (o.Lr, o.Lp, o.halo) == (Lr, Lr + 256, 128)
    assert (o.h_stride, o.ts_stride, o.acts_stride) == (B * o.Lp * 512, B * Lr * 1024, B * Lr * 512)
    assert (o.dpre_stride, o.dh_stride, o.skip_bytes, o.dskip_bytes) == (B * o.Lp * 1024, B * Lr * 512, B * Lr * 1024, B * Lr * 512)
    state = [(o.h, o.h_stride * (nl + 1)), (o.ts, o.ts_stride * nl), (o.acts, o.acts_stride * nl), (o.skip, o.skip_bytes)]
    grads = [(o.dpre, o.dpre_stride * nl), (o.dh, o.dh_stride * (nl + 1)), (o.dskip, o.dskip_bytes)]
    up = lambda n: -(-n // 256) * 256
    for pieces, end in ((state, o.state_end), (grads, o.grads_end)):
        for (off, size), nxt in zip(pieces, [p[0] for p in pieces[1:]] + [end]):
            assert off % 256 == 0 and size > 0 and off + up(size) == nxt, (shape, off, size, nxt)
    assert o.h == 0 and o.state_end == L.facppg_wn_bf16_state_bytes(*shape)
    sz = flib.GlowBf16Sizes()
    assert L.facppg_glow_bf16_layout(nl, B, Lg, sz) == 0
    assert o.dpre == sz.packed_bytes_per_flow - nl * 512 * 4       # behind the packed images (the group calls' packed buffer adds the summed biases)
    assert o.grads_end < o.scratch_end == L.facppg_wn_bf16_scratch_bytes(*shape) - 8 * 512 * 4
    # the reductions' partials behind the gradients: the group calls' work buffer holds the same gradients and column-sum partials
    # and three weight-gradient regions where the scratch has one, plus the scratch's 256 x 9 x 256 floats of <= 8-channel partials
    assert 3 * (o.scratch_end - o.grads_end - 256 * 9 * 256 * 4) - 2 * (256 * 16 * 1024 * 4) == sz.work_bytes - o.grads_end + o.dpre
    for bad in ((0, 1, 1), (9, 1, 1), (8, 0, 1), (8, 1, 0)):
        assert L.facppg_wn_bf16_layout(*bad, o) == EINVAL
    assert L.facppg_wn_bf16_layout(nl, B, Lg, None) == EINVAL
