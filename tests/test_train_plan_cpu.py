"""CPU: which kernels, in what shape, the bf16 training entry points launch and how they carve their buffers --
facppg_train_bf16_launch_plan, the host-side decision of facppg_wn_forward_bf16 / _backward_bf16 and facppg_glow_bf16_*
(csrc/facppg_train_plan.h).  The expected values are worked out by hand from the launch code as it stood before the planning
header existed (C = 256 channels, 640 conditioning channels, segments padded to Lr = 128 ceil(L / 128) with 128-row margins):
  tiles    64 positions once ceil(L / 64) B >= 160, else 32; a fused launch has 8 ceil(ceil(L / tile) B / 8) workgroups
  fused    forward once ceil(L / 32) B >= 160; backward once >= 40 and never for a one-layer stack
  k_bgemm  with nm = M / 128 row tiles: 128-column tiles once ceil(N / 128) nm B >= 384, else 64; 8 nm ceil(ct / 8) workgroups for
           ct = ceil(N / cols) B column tiles.  The product is a multiple of nm, so the last value below 384 is 380 at M = 512
           (ct = 95 | 96) and 382 at M = 256 (ct = 191 | 192): 383 itself is out of reach for both
  k_dspect 2 ceil(L / 64) B tiles, rounded up to 8 workgroups, 64 * 324 * 4 = 82944 bytes of LDS
  wgrad    nall = B ceil(L / 64) position chunks, partial buffer 3 nl * 5 * 512 * 256 * 4 bytes.  256-tiles: t = ceil(K / 256)
           ceil(M / 256) nprob tiles, ns = min(256 // t, 8, nall), taken while t >= 32 and nall // ns >= 24; else 128-tiles:
           t = (K / 128) (M / 128) nprob, ns = min(ceil(256 / t), 8, nall).  ns shrinks until nprob ns M K 4 bytes fit.
           Workgroups: 8 ceil(nprob ns / 8) x tiles per problem, or with FACPPG_WGRAD_NO_XCD_MAP=1 (128-tiles) the plain product
  edges    nchunk = max(1, ceil(B ceil(L / 32) / 512)), gx = ceil(ceil(L / 32) / nchunk), n_parts = B gx
  LDS      k_wn_fwd tile * 516 * 4; k_wn_bwd (2 tile * 136 + tile * 264 + tile * 520) * 2; k_wgrad 2 * 2 * 128 * 72 * 2;
           k_wgrad2 twice that"""
import itertools

import pytest

from facppg import lib as flib

EINVAL = -1
SWITCHES = ("FACPPG_TRAIN_TILE", "FACPPG_TRAIN_FUSED_FWD", "FACPPG_TRAIN_FUSED_BWD", "FACPPG_TRAIN_DSPECT_BGEMM", "FACPPG_TRAIN_PACK",
            "FACPPG_WGRAD_TILE", "FACPPG_WGRAD_NO_XCD_MAP", "FACPPG_EDGE_WGS", "FACPPG_UPSAMPLE_GEMM")
GATE, RESSKIP, RESSKIP_LAST, GATE_BWD, CONV_BWD = range(5)     # gemm_cols / gemm_workgroups
TAPS, COND, RS = range(3)                                      # wgrad_*


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def plan(B, L=1250, nl=8):
    r = flib.TrainLaunchReport()
    got = flib.load().facppg_train_bf16_launch_plan(nl, B, L, r)
    assert got == 0, (got, flib.load().facppg_last_error())
    return r


def gemm(r, i):
    return (r.gemm_cols[i], r.gemm_workgroups[i])


def wgrad(r, i):
    return (r.wgrad_tile[i], r.wgrad_splits[i], r.wgrad_workgroups[i])


def test_fused_forward_starts_at_160_tiles_of_32():
    assert plan(159, L=1).fused_fwd == 0 and plan(160, L=1).fused_fwd == 1
    assert plan(1, L=159 * 32).fused_fwd == 0 and plan(1, L=159 * 32 + 1).fused_fwd == 1
    assert plan(3, L=53 * 32).fused_fwd == 0                   # 3 * 53 = 159
    assert plan(5, L=31 * 32 + 1).fused_fwd == 1               # 5 * 32 = 160


def test_fused_backward_starts_at_40_tiles_of_32_and_needs_two_layers():
    assert plan(39, L=1).fused_bwd == 0 and plan(40, L=1).fused_bwd == 1
    assert plan(1, L=39 * 32).fused_bwd == 0 and plan(1, L=39 * 32 + 1).fused_bwd == 1
    assert plan(3, L=13 * 32).fused_bwd == 0 and plan(3, L=13 * 32 + 1).fused_bwd == 1      # 39 | 42
    assert plan(40, L=1, nl=1).fused_bwd == 0 and plan(12, nl=1).fused_bwd == 0
    assert plan(40, L=1, nl=2).fused_bwd == 1


def test_tiles_of_64_positions_start_at_160_tiles():
    assert plan(159, L=1).tile_positions == 32 and plan(160, L=1).tile_positions == 64
    assert plan(1, L=159 * 64).tile_positions == 32 and plan(1, L=159 * 64 + 1).tile_positions == 64
    # tiles and workgroups of a fused launch; LDS of both fused kernels at the tile size
    r = plan(12)                                                # 20 tiles of 64 per item
    assert (r.tile_positions, r.fused_workgroups, r.fwd_lds_bytes, r.bwd_lds_bytes) == (64, 240, 132096, 135168)
    r = plan(3)                                                 # 40 tiles of 32 per item
    assert (r.tile_positions, r.fused_workgroups, r.fwd_lds_bytes, r.bwd_lds_bytes) == (32, 120, 66048, 67584)
    assert plan(1, L=16).fused_workgroups == 8                  # one tile: a whole round of the XCDs
    assert plan(1, L=159 * 32 + 1).fused_workgroups == 160
    assert plan(3, L=33).fused_workgroups == 8                  # 6 tiles
    assert plan(3, L=97).fused_workgroups == 16                 # 12 tiles
    assert (r.wgrad_lds_bytes, r.wgrad2_lds_bytes) == (73728, 147456)


def test_bgemm_column_tiles_switch_at_384_wide_tiles():
    # M = 512 (gate, res/skip; 4 row tiles): ct = 95 -> 380 wide tiles, ct = 96 -> 384
    r = plan(95, L=1)
    assert gemm(r, GATE) == (64, 8 * 4 * 12) and gemm(r, RESSKIP) == (64, 384)          # 95 tiles of 64 columns
    r = plan(96, L=1)
    assert gemm(r, GATE) == (128, 8 * 4 * 12) and gemm(r, RESSKIP) == (128, 384)
    assert gemm(r, RESSKIP_LAST) == gemm(r, GATE_BWD) == gemm(r, CONV_BWD) == (64, 8 * 2 * 12)   # M = 256: 192 wide tiles
    r = plan(1, L=95 * 128)
    assert gemm(r, GATE) == (64, 8 * 4 * 24)                                            # 190 tiles of 64 columns
    assert gemm(r, CONV_BWD) == (64, 8 * 2 * 24)
    r = plan(1, L=95 * 128 + 1)
    assert gemm(r, GATE) == (128, 8 * 4 * 12)                                           # 96 tiles of 128 columns
    assert gemm(r, CONV_BWD) == (64, 8 * 2 * 24)                                        # 191 tiles of 64 columns
    # M = 256 (last res/skip, gate backward, transposed conv; 2 row tiles): ct = 191 -> 382, ct = 192 -> 384
    r = plan(191, L=1)
    assert gemm(r, RESSKIP_LAST) == gemm(r, GATE_BWD) == gemm(r, CONV_BWD) == (64, 8 * 2 * 24)
    assert gemm(r, GATE) == (128, 8 * 4 * 24)
    r = plan(192, L=1)
    assert gemm(r, RESSKIP_LAST) == gemm(r, GATE_BWD) == gemm(r, CONV_BWD) == (128, 8 * 2 * 24)
    r = plan(1, L=191 * 128)
    assert gemm(r, GATE_BWD) == (64, 8 * 2 * 48) and gemm(r, GATE) == (128, 8 * 4 * 24)  # 382 tiles of 64 columns
    r = plan(1, L=191 * 128 + 1)
    assert gemm(r, GATE_BWD) == (128, 8 * 2 * 24) and gemm(r, GATE) == (128, 8 * 4 * 24)
    # config 5: 10 tiles of 128 columns / 20 of 64 per item
    r = plan(12)
    assert gemm(r, GATE) == gemm(r, RESSKIP) == (128, 480)                              # 480 wide tiles; 8 * 4 * 15
    assert gemm(r, RESSKIP_LAST) == gemm(r, GATE_BWD) == gemm(r, CONV_BWD) == (64, 480)  # 240 wide tiles; 8 * 2 * 30
    r = plan(3)
    assert gemm(r, GATE) == (64, 256) and gemm(r, GATE_BWD) == (64, 128)                # 60 tiles of 64 columns: 8 * 4 * 8, 8 * 2 * 8


def test_conditioning_gradient_kernel(monkeypatch):
    r = plan(12)
    assert (r.dspect_bgemm, r.dspect_cols, r.dspect_workgroups, r.dspect_lds_bytes) == (0, 0, 480, 82944)
    assert plan(3).dspect_workgroups == 120 and plan(1, L=16).dspect_workgroups == 8    # 2 tiles
    monkeypatch.setenv("FACPPG_TRAIN_DSPECT_BGEMM", "1")
    r = plan(12)                                                # M = 640: 5 row tiles, 600 wide tiles; 8 * 5 * 15
    assert (r.dspect_bgemm, r.dspect_cols, r.dspect_workgroups, r.dspect_lds_bytes) == (1, 128, 600, 0)
    r = plan(3)                                                 # 150 wide tiles: 60 tiles of 64 columns; 8 * 5 * 8
    assert (r.dspect_bgemm, r.dspect_cols, r.dspect_workgroups) == (1, 64, 320)
    assert plan(1, L=76 * 128).dspect_cols == 64 and plan(1, L=76 * 128 + 1).dspect_cols == 128      # 380 | 385
    for other in ("0", "2", "", "yes"):
        monkeypatch.setenv("FACPPG_TRAIN_DSPECT_BGEMM", other)
        assert plan(12).dspect_bgemm == 0


def test_weight_gradient_plans_at_config5():
    """nl = 8, L = 1250: 20 position chunks per item, partial buffer 24 * 5 * 512 * 256 * 4 = 62 914 560 bytes.
    B = 12 (nall = 240):
      taps          24 x [512 x 256]: 48 tiles of 256 -> ns = min(5, 8, 240) = 5, exactly the buffer; 48 >= 32, 240 // 5 = 48 >= 24:
                    256-tiles, 120 groups x 2 tiles = 240 workgroups
      conditioning  8 x [512 x 640]: 3 * 2 * 8 = 48 tiles of 256 -> ns = 5; 8 * 5 * 512 * 640 * 4 = 52 428 800 bytes FIT the buffer
                    (the 5 stays); 256-tiles, 40 groups x 6 tiles = 240 workgroups
      res/skip      8 x [512 x 256]: 16 tiles of 256 < 32 -> 128-tiles: 64 tiles, ns = 256 / 64 = 4, 32 groups x 8 = 256 workgroups
    B = 3 (nall = 60): 60 // 5 = 12 < 24 -> 128-tiles throughout: taps 192 tiles, ns = 2, 48 groups x 8 = 384; conditioning 160
    tiles, ns = 2, 16 groups x 20 = 320; res/skip as above.  B = 6 (nall = 120): 120 // 5 = 24 -> 256-tiles for taps and conditioning."""
    r = plan(12)
    assert wgrad(r, TAPS) == (256, 5, 240) and wgrad(r, COND) == (256, 5, 240) and wgrad(r, RS) == (128, 4, 256)
    assert list(r.wgrad_xcd_map) == [1, 1, 1]
    r = plan(3)
    assert wgrad(r, TAPS) == (128, 2, 384) and wgrad(r, COND) == (128, 2, 320) and wgrad(r, RS) == (128, 4, 256)
    r = plan(6)
    assert wgrad(r, TAPS) == (256, 5, 240) and wgrad(r, COND) == (256, 5, 240) and wgrad(r, RS) == (128, 4, 256)


def test_weight_gradient_splits_are_capped_by_chunks_and_by_the_partial_buffer():
    """nall caps: B = 1, L <= 64 is ONE chunk -> one split everywhere (256-tiles would need 24 chunks per workgroup): taps 24 groups
    -> 8 * 3 * 8 tiles = 192 workgroups, conditioning 8 groups x 20 = 160, res/skip 8 groups x 8 = 64.  Two chunks (L = 65): ns = 2
    for taps (2), conditioning (2) and res/skip (min(4, 8, 2)).
    The buffer caps: nl = 2, B = 12, L = 1250: 6 * 5 * 512 * 256 * 4 = 15 728 640 bytes.  Taps: 6 problems, 12 tiles of 256 < 32 ->
    128-tiles, 48 tiles, ns = ceil(256 / 48) = 6 needs 18 874 368 bytes -> 5 (exactly the buffer); 30 groups -> 8 * 4 * 8 = 256.
    Conditioning: 2 problems, 40 tiles of 128, ns = 7 needs 2 * 7 * 512 * 640 * 4 = 18 350 080 -> 6 (15 728 640, exactly);
    12 groups -> 8 * 2 * 20 = 320.  Res/skip: 16 tiles, ns = min(16, 8) = 8 needs 8 388 608: fits; 16 groups x 8 = 128."""
    for L in (1, 64):
        r = plan(1, L=L)
        assert wgrad(r, TAPS) == (128, 1, 192) and wgrad(r, COND) == (128, 1, 160) and wgrad(r, RS) == (128, 1, 64)
    r = plan(1, L=65)
    assert wgrad(r, TAPS) == (128, 2, 384) and wgrad(r, COND) == (128, 2, 320) and wgrad(r, RS) == (128, 2, 128)
    r = plan(12, nl=2)
    assert wgrad(r, TAPS) == (128, 5, 256) and wgrad(r, COND) == (128, 6, 320) and wgrad(r, RS) == (128, 8, 128)


def test_every_switch_forces_what_it_forces(monkeypatch):
    def with_env(name, value, B=12, **kw):
        monkeypatch.setenv(name, value)
        r = plan(B, **kw)
        monkeypatch.delenv(name)
        return r
    # FACPPG_TRAIN_TILE: "32" is 32, everything else 64
    assert with_env("FACPPG_TRAIN_TILE", "32").tile_positions == 32 and with_env("FACPPG_TRAIN_TILE", "32").fused_workgroups == 480
    for v in ("64", "48", "0", "", "x"):
        r = with_env("FACPPG_TRAIN_TILE", v, B=3)
        assert (r.tile_positions, r.fused_workgroups, r.fwd_lds_bytes, r.bwd_lds_bytes) == (64, 64, 132096, 135168)    # 60 tiles
    # FACPPG_TRAIN_FUSED_FWD / _BWD: a leading "0" is off, everything else (the empty string too) on
    for v, on in (("0", 0), ("0x", 0), ("1", 1), ("", 1), ("no", 1)):
        assert with_env("FACPPG_TRAIN_FUSED_FWD", v, B=12).fused_fwd == on and with_env("FACPPG_TRAIN_FUSED_FWD", v, B=1, L=16).fused_fwd == on
        assert with_env("FACPPG_TRAIN_FUSED_BWD", v, B=12).fused_bwd == on and with_env("FACPPG_TRAIN_FUSED_BWD", v, B=1, L=16).fused_bwd == on
    assert with_env("FACPPG_TRAIN_FUSED_BWD", "1", nl=1).fused_bwd == 0
    # FACPPG_WGRAD_TILE: "256" forces k_wgrad2, everything else k_wgrad, for all three products
    for v in ("128", "100", "0", ""):
        r = with_env("FACPPG_WGRAD_TILE", v)
        assert wgrad(r, TAPS) == (128, 2, 384) and wgrad(r, COND) == (128, 2, 320) and wgrad(r, RS) == (128, 4, 256)
    r = with_env("FACPPG_WGRAD_TILE", "256", B=3)
    # res/skip on 256-tiles: 16 tiles, ns = min(16, 8, 60) = 8, 64 groups x 2 tiles
    assert wgrad(r, TAPS) == (256, 5, 240) and wgrad(r, COND) == (256, 5, 240) and wgrad(r, RS) == (256, 8, 128)
    # FACPPG_WGRAD_NO_XCD_MAP=1: k_wgrad's plain grid (2 x 4 tiles x 32 groups); k_wgrad2 has the XCD order alone
    r = with_env("FACPPG_WGRAD_NO_XCD_MAP", "1")
    assert list(r.wgrad_xcd_map) == [1, 1, 0] and wgrad(r, RS) == (128, 4, 256) and wgrad(r, TAPS) == (256, 5, 240)
    r = with_env("FACPPG_WGRAD_NO_XCD_MAP", "1", B=3)       # taps 2 x 4 x 48, conditioning 5 x 4 x 16
    assert list(r.wgrad_xcd_map) == [0, 0, 0] and wgrad(r, TAPS) == (128, 2, 384) and wgrad(r, COND) == (128, 2, 320)
    r = with_env("FACPPG_WGRAD_NO_XCD_MAP", "1", B=1, L=16)  # plain grids: 8 * 24, 20 * 8, 8 * 8 -- no rounding up to 8 groups
    assert wgrad(r, TAPS) == (128, 1, 192) and wgrad(r, COND) == (128, 1, 160) and wgrad(r, RS) == (128, 1, 64)
    r = with_env("FACPPG_WGRAD_NO_XCD_MAP", "1", B=1, L=16, nl=1)   # 3, 1, 1 groups: 24, 20, 8 workgroups (mapped: 64, 160, 64)
    assert [r.wgrad_workgroups[i] for i in range(3)] == [24, 20, 8]
    r = plan(1, L=16, nl=1)
    assert [r.wgrad_workgroups[i] for i in range(3)] == [64, 160, 64]
    for v in ("0", "", "2", "yes"):
        assert list(with_env("FACPPG_WGRAD_NO_XCD_MAP", v).wgrad_xcd_map) == [1, 1, 1]
    # FACPPG_TRAIN_PACK: "step" alone
    assert plan(12).pack_per_step == 0 and with_env("FACPPG_TRAIN_PACK", "step").pack_per_step == 1
    for v in ("Step", "flow", "", "1"):
        assert with_env("FACPPG_TRAIN_PACK", v).pack_per_step == 0
    # FACPPG_EDGE_WGS: 12 * 40 = 480 blocks of 32 positions
    r = plan(12)
    assert (r.edge_nchunk, r.edge_n_parts) == (1, 480)
    r = plan(24)                                                # 960 blocks: two per workgroup, 20 workgroups per item
    assert (r.edge_nchunk, r.edge_n_parts) == (2, 480)
    r = plan(13)                                                # 520 blocks: two per workgroup
    assert (r.edge_nchunk, r.edge_n_parts) == (2, 260)
    for v in ("0", "-3", "", "x"):
        r = with_env("FACPPG_EDGE_WGS", v, B=24)
        assert (r.edge_nchunk, r.edge_n_parts) == (2, 480)
    r = with_env("FACPPG_EDGE_WGS", "100")                      # ceil(480 / 100) = 5 blocks each, 8 workgroups per item
    assert (r.edge_nchunk, r.edge_n_parts) == (5, 96)
    monkeypatch.setenv("FACPPG_EDGE_WGS", "100")
    assert layout(8, 12, 1250).n_parts == 96
    monkeypatch.delenv("FACPPG_EDGE_WGS")
    # FACPPG_UPSAMPLE_GEMM: a leading "0" is off
    assert plan(12).upsample_gemm == 1
    for v, on in (("0", 0), ("00", 0), ("1", 1), ("", 1)):
        assert with_env("FACPPG_UPSAMPLE_GEMM", v).upsample_gemm == on


def test_the_two_queries_agree(monkeypatch):
    """facppg_wn_bf16_launch_plan's bits are the report's fields: bit 0 fused_fwd, bit 1 fused_bwd, bit 2 the taps' 256-tiles,
    bits 8.. tile_positions -- unswitched and under every combination of the four switches the older query names."""
    L = flib.load()
    shapes = [(nl, B, Lg) for nl in (1, 2, 8) for B in (1, 3, 6, 12, 40, 160) for Lg in (1, 16, 65, 1250, 5089)]
    settings = [{}] + [dict(zip(("FACPPG_TRAIN_FUSED_FWD", "FACPPG_TRAIN_FUSED_BWD", "FACPPG_TRAIN_TILE", "FACPPG_WGRAD_TILE"), v))
                       for v in itertools.product(("0", "1"), ("0", "1"), ("32", "64"), ("128", "256"))]
    for env in settings:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for nl, B, Lg in shapes:
            bits, r = L.facppg_wn_bf16_launch_plan(nl, B, Lg), plan(B, L=Lg, nl=nl)
            assert bits == (r.tile_positions << 8) | r.fused_fwd | (r.fused_bwd << 1) | ((r.wgrad_tile[TAPS] == 256) << 2), (env, nl, B, Lg)
    r = flib.TrainLaunchReport()
    for nl, B, Lg in ((0, 3, 1250), (9, 3, 1250), (8, 0, 1250), (8, 3, 0), (8, -1, 5)):
        assert L.facppg_wn_bf16_launch_plan(nl, B, Lg) < 0 and L.facppg_train_bf16_launch_plan(nl, B, Lg, r) == EINVAL
    assert L.facppg_train_bf16_launch_plan(8, 3, 1250, None) == EINVAL


def layout(nl, B, Lg):
    sz = flib.GlowBf16Sizes()
    assert flib.load().facppg_glow_bf16_layout(nl, B, Lg, sz) == 0
    return sz


# (nl, B, L) -> state, scratch, packed per flow, work, n_parts.  Per item and layer: h rows 512 B x (Lr + 256), ts rows 1024 B,
# acts rows 512 B; skip rows 1024 B; every piece is a multiple of 256 bytes.
#   state   B ((nl + 1) (Lr + 256) 512 + nl Lr 1536 + Lr 1024)
#   images  nl (1441792 + 262144 + 262144 + 786432 + 655360) = nl 3407872 (w1 16 x 88 x 1 KB, w2 16 x 16, rst 8 x 32, int 8 x 96,
#           condt 20 x 32 per layer); packed = images + nl 2048 (summed biases)
#   grads   B (nl (Lr + 256) 1024 + (nl + 2) Lr 512)      (dpre, nl + 1 dh, dskip)
#   work    grads + 16777216 (column-sum partials) + 3 nl 7864320 (three weight-gradient regions)
#   scratch images + grads + 2359296 (256 x 9 x 256 floats) + 16777216 + nl 7864320, + 16384 for the summed biases
SIZES = {
    (1, 1, 1): (720896, 30998528 + 16384, 3409920, 40960000, 1),              # Lr = 128: grads 393216 + 196608
    (2, 2, 65): (2228224, 43778048 + 16384, 6819840, 66060288, 6),            # Lr = 128: grads 2 (786432 + 262144)
    (8, 3, 1250): (72351744, 166723584 + 16384, 27279360, 262930432, 120),    # Lr = 1280: 24117248 state, 19136512 grads per item
    (8, 12, 1250): (289406976, 338952192 + 16384, 27279360, 435159040, 480),
}


@pytest.mark.parametrize("shape", sorted(SIZES))
def test_buffer_sizes(shape):
    L = flib.load()
    state, scratch, packed, work, n_parts = SIZES[shape]
    assert L.facppg_wn_bf16_state_bytes(*shape) == state
    assert L.facppg_wn_bf16_scratch_bytes(*shape) == scratch
    sz = layout(*shape)
    assert (sz.packed_bytes_per_flow, sz.state_bytes_per_flow, sz.work_bytes, sz.n_parts, sz.part_floats) == (packed, state, work, n_parts, 3400)


def test_buffer_size_queries_refuse_bad_shapes():
    L = flib.load()
    for bad in ((0, 1, 1), (9, 1, 1), (8, 0, 1), (8, 1, 0)):
        assert L.facppg_wn_bf16_state_bytes(*bad) == 0 and L.facppg_wn_bf16_scratch_bytes(*bad) == 0
        assert L.facppg_glow_bf16_layout(*bad, flib.GlowBf16Sizes()) == EINVAL
    assert L.facppg_glow_bf16_layout(8, 65536, 1, flib.GlowBf16Sizes()) == EINVAL
    assert [L.facppg_wn_bf16_padded_len(n) for n in (0, 1, 128, 129, 1250)] == [0, 128, 128, 256, 1280]


# (B, T, L) at 80 mel channels, hop 256, kernel 1024: nj = 4 taps, K = 320, N = 20480 columns, Tq = ceil(8 L / 256) frames per item.
#   fold   320 x 20480 floats = 26214400
#   image  forward, of [B Tq x 320]: (ceil(rows / 32) x 41 x 64 + 192) x 16 bytes; backward, of [320 x B Tq]: (10 x (ceil(rows /
#          64) x 8 + 1) x 64 + 192) x 16
#   out    B Tq x 20480 floats;   the backward adds the column-sum partials (16777216) in front
UPSAMPLE = {
    (1, 1, 1): (26214400 + 45056 + 81920, 16777216 + 26214400 + 95232 + 81920),                  # 1 row
    (2, 4, 65): (26214400 + 45056 + 491520, 16777216 + 26214400 + 95232 + 491520),                # 6 rows
    (3, 40, 1250): (26214400 + 171008 + 9830400, 16777216 + 26214400 + 177152 + 9830400),         # 120 rows
    (12, 40, 1250): (26214400 + 632832 + 39321600, 16777216 + 26214400 + 668672 + 39321600),      # 480 rows
}


@pytest.mark.parametrize("shape", sorted(UPSAMPLE))
def test_upsample_workspace_sizes(shape):
    L = flib.load()
    B, T, Lg = shape
    fwd, bwd = UPSAMPLE[shape]
    assert L.facppg_upsample_forward_workspace_bytes(B, T, 80, 256, 1024, Lg) == fwd
    assert L.facppg_upsample_backward_workspace_bytes(B, T, 80, 256, 1024, Lg) == bwd
    assert L.facppg_upsample_forward_workspace_bytes(0, T, 80, 256, 1024, Lg) == 0
    assert L.facppg_upsample_backward_workspace_bytes(0, T, 80, 256, 1024, Lg) == 16777216
