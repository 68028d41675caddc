"""The thin GEMMs of the folded cross-attention K | V (ops.KvFold: reductions and outputs over the 128-wide latent)
through the route queries (no launch, no device access: runs on the CPU): at the headline's and fixed_len_80's memory
row counts they stay on the bf16 tile kernels -- the forward with K = 128, the dgrad with N = 128 and accumulate, the
weight gradient whose X operand is 128 wide, the fold product A = W_kv W_z itself -- and the backward is paired where
the planner's model sees a partial round to fill (profiles/r09_kv_fold_lab.log)."""
import pytest

from gct_plus_amd import ops

X6S, X6, BF16_TILES = 0, 5, 3            # GCT_GEMM_ROUTE_X6S, GCT_GEMM_ROUTE_X6, GCT_WGRAD_BF16_TILES
D, LAT, ACCUM = 512, 128, ops.DEPI_ACCUM


@pytest.mark.parametrize("mode", [ops.GEMM_BF16X6, ops.GEMM_BF16X3])
@pytest.mark.parametrize("M", [18432, 40960])
def test_thin_shapes_take_the_bf16_tile_kernels(M, mode):
    assert ops.linear_fwd_route(M, LAT, 2, D, mode=mode)[0] == X6
    assert ops.linear_dgrad_route(M, 2, D, LAT, depi=ACCUM, mode=mode)[0] == X6
    kind, nsplit, rows, bias_fused = ops.wgrad_route(M, 2, D, LAT, 2 * D, LAT, mode=mode)
    assert (kind, bias_fused) == (BF16_TILES, 1) and nsplit * rows >= M
    paired = ops.linear_bwd_route(M, 2, D, LAT, 2 * D, LAT, LAT, LAT, ACCUM, mode=mode)
    assert paired[0] == (1 if M == 18432 else 0)       # 144 dgrad tiles leave half a round; 320 fill theirs


@pytest.mark.parametrize("layers", [1, 6, 16])
def test_fold_product_takes_a_bf16_kernel(layers):
    """A = wstack W_z as gct_kv_fold_fwd computes it: the dgrad form over layers * 2 d rows, 128 outputs, K' = 512"""
    assert ops.linear_dgrad_route(layers * 2 * D, 1, D, LAT, mode=ops.GEMM_BF16X6)[0] in (X6S, X6)
    # the weight-sized gradient dW_z = wstack^T P: rows of the stack against the 128-wide P
    assert ops.wgrad_route(layers * 2 * D, 1, D, LAT, D, LAT, want_bias=False, mode=ops.GEMM_BF16X6)[0] == BF16_TILES
