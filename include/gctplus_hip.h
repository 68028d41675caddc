/*
 * gctplus_hip.h -- C ABI of libgctplus_hip.so (gfx950 / MI355X).
 *
 * The reference (chaoting-sun/GCT-Plus) is pure Python/PyTorch and has NO plugin,
 * operator or FFI interface; the drop-in boundary is the Python
 * nn.Module contract (Model/build_model.py:79-87 get_model, Vaetf/Cvaetf.forward
 * Model/vaetf.py:154-182, Model/cvaetf.py:179-193).  This header is the ABI the
 * build adds UNDERNEATH that contract: one entry point per ATen call site group of
 * SURVEY.md 2.2 (K1..K10).  Each declaration cites the reference call site whose
 * arithmetic it replaces.
 *
 * Conventions
 *  - plain C: raw device pointers, sizes, scalars, a hipStream_t passed as void*.
 *  - all tensors fp32 row-major unless stated; token ids int64; masks uint8.
 *  - the caller owns every buffer (PyTorch caching allocator); the library allocates
 *    nothing and never synchronises; kernels are enqueued on `stream`.
 *  - return 0 on success, <0 on error (GCT_ERR_*); message via gct_last_error()
 *    (thread-local).  Never throws, never exits.
 *  - "segmented" matrices: a logical [R][nseg*nper] matrix whose column block s
 *    (or row block s for weights) lives behind its own pointer p[s].  This is how the
 *    separate q/k/v (and mu/log_var) nn.Linear parameters of the reference are fused
 *    into one GEMM without repacking or renaming any checkpoint tensor.
 *  - dropout: Philox4x32-10, key = (seed, site), counter = element coordinates; the
 *    backward kernels regenerate the mask from (seed, site), nothing is stored.
 *    p == 0 disables it (bit-exact parity mode, SURVEY.md 7 "RNG").
 */
#ifndef GCTPLUS_HIP_H
#define GCTPLUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCT_OK 0
#define GCT_ERR_ARG (-1)  /* bad shape / alignment / null pointer            */
#define GCT_ERR_HIP (-2)  /* a HIP runtime call failed (launch error)        */

#define GCT_ABI_VERSION 33

int gct_version(void);
const char* gct_last_error(void);

/* workspace sizing helpers (bytes); the caller allocates */
int64_t gct_wgrad_ws_bytes(int64_t M, int64_t Ntot, int64_t K);
int64_t gct_rowred_ws_bytes(int64_t rows, int64_t cols);

/* ------------------------------------------------------------------ K2: Norm */
/* Model/modules.py:92-95   y = alpha*(x-mean)/(std_unbiased+eps)+bias.
 * Saves mean[rows] and rstd[rows] = 1/(std+eps) for the backward. d % 4 == 0, d <= 2048. */
int gct_norm_fwd(const float* x, const float* alpha, const float* bias, float* y,
                 float* mean, float* rstd, int64_t rows, int d, float eps, void* stream);
/* dx = dNorm/dx (dy) [+ dres]; dalpha, dbias overwritten. ws >= gct_rowred_ws_bytes(rows, 2*d).
 * quad_map (nullable): dy / dres / dx are QUAD-COMPACTED rows (see gct_live_rows) while x, mean, rstd stay in the
 * forward's row space of src_rows rows: compact row 4i+e reads x row 4*quad_map[i]+e. */
int gct_norm_bwd(const float* dy, const float* x, const float* alpha, const float* mean,
                 const float* rstd, const float* dres, float* dx, float* dalpha, float* dbias,
                 float* ws, int64_t rows, int d, float eps, const int32_t* quad_map, int64_t src_rows,
                 float* drop_out, float p, uint64_t seed, uint32_t site, void* stream);
/* drop_out (nullable, same rows as dx): additionally dropout_bwd(dx) with the mask (seed, site, p) of the dropout the
 * preceding sub-layer applied to its output -- that sub-layer's backward reads it instead of running gct_dropout_bwd. */

/* --------------------------------------------------- K1: embedding + PE (+cond) */
/* Model/modules.py:108-110 (lookup), :134-144 (x*sqrt(d)+pe, dropout),
 * Model/vaetf.py:35-39 (cond rows concatenated in front).  out row (b,l):
 *   l <  n_c : cond[b][l][:]        (cond = embed_cond2enc(econds) viewed [B,n_c,d])
 *   l >= n_c : table[tok[b][l-n_c]][:]
 * then *scale + pe[l][:], dropout(site).  L = n_c + S. */
int gct_embed_pe_fwd(const int64_t* tok, const float* table, const float* cond, const float* pe,
                     float* out, int B, int S, int n_c, int d, int vocab, float scale, float p,
                     uint64_t seed, uint32_t site, void* stream);
/* dtable[vocab][d] overwritten (deterministic two-stage reduction), dcond[B][n_c][d]
 * overwritten (nullable when n_c == 0). ws >= gct_embed_ws_bytes.  The reduction that writes dtable is one of the
 * deferred slab reductions below: while they are being recorded, ws stays intact until the flush.  Token ids outside
 * [0, vocab) are clamped to rows 0 / vocab - 1 in both directions. */
int64_t gct_embed_ws_bytes(int B, int S, int d, int vocab);
int gct_embed_pe_bwd(const float* dout, const int64_t* tok, float* dtable, float* dcond,
                     float* ws, int B, int S, int n_c, int d, int vocab, float scale, float p,
                     uint64_t seed, uint32_t site, void* stream);

/* ------------------------------------------------------------- K3: nn.Linear */
/* Model/sublayers.py:54-59,64-66,70 (q/k/v/out), :81-88 (FFN), :11-12 (fc_mu,
 * fc_log_var), Model/vaetf.py:81 (fc_z), :133/:169 (out).  fp32-input MFMA
 * (v_mfma_f32_32x32x2_f32): results are exact-fp32 fma chains.
 *
 * y_s[m][n] = epi( sum_k x[m][k] * w_s[n][k] + b_s[n] )   s = 0..nseg-1, n < nper
 *   GCT_EPI_BIAS       : plain
 *   GCT_EPI_GELU_DROP  : pre[m][n] = acc+b (saved), y = dropout(gelu_erf(pre))   (FFN-1)
 *   GCT_EPI_DROP_RESID : y = resid[m][n] + dropout(acc+b)                         (out / FFN-2)
 *   GCT_EPI_GELU_DROP_SAVE : y as GCT_EPI_GELU_DROP; pre[m][n] = keep ? gelu'(acc+b) : 0 (saved: the
 *                        factor GCT_DEPI_MUL_SAVED needs, keep = the dropout mask of y)   (FFN-1)
 * pre/resid share y's leading dimension and are only valid with nseg == 1. */
#define GCT_EPI_BIAS 0
#define GCT_EPI_GELU_DROP 1
#define GCT_EPI_DROP_RESID 2
#define GCT_EPI_GELU_DROP_SAVE 3
int gct_linear_fwd(const float* x, int64_t ldx, int64_t M, int K,
                   const float* w0, const float* w1, const float* w2, int64_t ldw,
                   const uint16_t* wp0, int64_t plane_stride,
                   const float* b0, const float* b1, const float* b2,
                   int nseg, int nper, float* y0, float* y1, float* y2, int64_t ldy,
                   int epi, const float* resid, float* pre, float p, uint64_t seed, uint32_t site,
                   float* ws, int64_t ws_bytes, const int32_t* quad_map, void* stream);
/* wp0 (nullable): the weights' bf16 planes (gct_split_planes, below): wp0 = plane 0 of w0; the planes of w1, w2 are
 * addressed as wp0 + (w1 - w0), wp0 + (w2 - w0) (the layout gct_split_planes produces over a common buffer).
 * wp0 == NULL, or mode GCT_GEMM_F32: the fp32 kernels.
 * ws (nullable): caller-provided workspace (>= gct_linear_fwd_ws_bytes), ws_bytes its size.  It lets skinny-M shapes
 * (decode steps, M = batch rows) run split-K with a fused reduce+epilogue pass so all CUs get work, and the bf16x6
 * launches balance their tail (see gct_linear_dgrad); identical results up to fp32 summation order.  A route that
 * needs more slabs than ws holds takes fewer K-splits (same result up to the fp32 summation order) or no workspace
 * route at all; nothing is ever written past ws + ws_bytes.
 * quad_map (nullable): the M rows are a quad compaction of a larger row space (gct_live_rows); the dropout masks of the
 * GCT_EPI_GELU_DROP / GCT_EPI_DROP_RESID epilogues are then drawn at the coordinates of original quad quad_map[q] for
 * compact quad q, i.e. every live row gets exactly the mask it would get in the full row space.  The map holds M / 4
 * entries followed by at least 32 readable ones (any value): a tile's rows beyond M look theirs up. */
int64_t gct_linear_fwd_ws_bytes(int64_t M, int K, int Ntot);

/* dx[m][k] (op)= sum_s sum_n dy_s[m][n] * w_s[n][k]
 *   GCT_DEPI_STORE / GCT_DEPI_ACCUM (dx += ...) /
 *   GCT_DEPI_GELU_BWD : dx = acc * gelu'(pre[m][k]) * dropmask(site)/(1-p)   (through FFN-1 act.)
 *   GCT_DEPI_MUL_SAVED : dx = pre[m][k] == 0 ? 0 : acc * pre[m][k] / (1-p), pre written by
 *                        GCT_EPI_GELU_DROP_SAVE (same p): the GCT_DEPI_GELU_BWD result with the
 *                        same operations in the same order, without Philox / erf / exp */
#define GCT_DEPI_STORE 0
#define GCT_DEPI_ACCUM 1
#define GCT_DEPI_GELU_BWD 2
#define GCT_DEPI_MUL_SAVED 3
int gct_linear_dgrad(const float* dy0, const float* dy1, const float* dy2, int64_t lddy,
                     int64_t M, int nseg, int nper,
                     const float* w0, const float* w1, const float* w2, int64_t ldw,
                     const uint16_t* wp0, int64_t plane_stride, int K,
                     float* dx, int64_t lddx, int depi, const float* pre, float p, uint64_t seed,
                     uint32_t site, float* ws, int64_t ws_bytes, const int32_t* quad_map, int64_t pre_rows,
                     void* stream);
/* wp0 / plane_stride (nullable): the weights' bf16 planes, as for gct_linear_fwd.
 * quad_map (nullable): the M rows are quad-compacted (gct_live_rows); GCT_DEPI_GELU_BWD then regenerates the dropout
 * mask of compact quad q from original quad quad_map[q].  pre_rows == 0: pre is compact like dy / dx; pre_rows > 0:
 * pre keeps the forward's row space (pre_rows rows) and is read through the quad map (no gathered copy needed) --
 * for GCT_DEPI_GELU_BWD and GCT_DEPI_MUL_SAVED alike.
 * ws (nullable): >= gct_linear_dgrad_ws_bytes(M, nseg*nper, K), ws_bytes its size.  With a workspace the
 * bf16x6 forward / dgrad launches balance a partial last round of tiles (the tail rows as a second launch: on 64 x 128
 * tiles when the reduction is <= 1024 long, else K-split into slabs + a fix-up kernel) and split a long reduction over
 * few tiles across the whole chip; gct_linear_fwd_ws_bytes covers the forward (skinny split-K or tail slabs, whichever
 * the launch would use).  Without one every launch is a single kernel. */
int64_t gct_linear_dgrad_ws_bytes(int64_t M, int Ntot, int K);

/* The route gct_linear_fwd / gct_linear_dgrad take for a shape (ABI 30; no launch, no device access; the rule the calls
 * themselves execute, on the calls' own argument builders):
 *   out8[0] kernel(s), a GCT_GEMM_ROUTE_* value (GCT_GEMM_ROUTE_NONE for M == 0: nothing is launched);
 *   out8[1] slabs a K-split route writes (GCT_GEMM_ROUTE_X6_SPLITK_ALL, GCT_GEMM_ROUTE_F32_SMALL), 1 otherwise;
 *   out8[2] tail of a GCT_GEMM_ROUTE_X6 launch: 0 none, 1 the tail rows on 64 x 128 tiles, 2 the tail rows K-split into
 *           slabs + a fix-up kernel.  Reported for a stream that is not being captured: under capture there is no tail;
 *   out8[3] first tail row (a multiple of 128; 0 without a tail);
 *   out8[4] slabs of the tail (1 unless out8[2] == 2);
 *   out8[5] kernel launches of the call, fix-up kernels included;
 *   out8[6] bytes of ws the call writes, from ws on (0: ws is not touched; never above the matching *_ws_bytes query);
 *   out8[7] 0.
 * A tail on 64 x 128 tiles writes no slabs, yet like the slab tail it is taken only where ws_bytes would hold the
 * slabs of the tail rows (one rule for both).
 * aligned16: every buffer of the call (x / dy, w, y / dx, bias, resid, pre, ws) is 16-byte aligned.  Segments are taken
 * to lie where the model keeps them: the weights stacked in one [nseg * nper][ldw] buffer, outputs / dy* and biases side
 * by side (segment s at column s * nper of one [M][ld] buffer).  have_planes: wp0 != NULL, 16-byte aligned, with a
 * plane_stride that is a multiple of 8.  have_bias: b0 != NULL.  resid / pre are present exactly where the epilogue
 * needs them.  mode: a GCT_GEMM_* value (below), passed in rather than read from the process; bf16x6 and bf16x3 plan
 * alike.  ws_bytes: that of the call; 0: ws == NULL.
 * An argument error (unknown mode or epilogue, a negative size, out8 == NULL) returns GCT_ERR_ARG and leaves out8 alone. */
#define GCT_GEMM_ROUTE_NONE (-1)
#define GCT_GEMM_ROUTE_X6S 0           /* gemm_x6s_kernel: 64 x 128 bf16 tiles over the whole problem */
#define GCT_GEMM_ROUTE_X6_SPLITK_ALL 1 /* gemm_x6_kernel, K split into slabs over the whole problem, + fix-up */
#define GCT_GEMM_ROUTE_PANEL_THIN 2    /* gemm_f32_panel_kernel<32, ragged>: N <= 32 (the vocabulary head) */
#define GCT_GEMM_ROUTE_PANEL32 3       /* gemm_f32_panel_kernel<32>: the whole reduction in one workgroup per 32 x 32 tile */
#define GCT_GEMM_ROUTE_F32_SMALL 4     /* gemm_f32_small_kernel: 64 x 64 fp32 tiles; out8[1] > 1: K-split slabs + fix-up */
#define GCT_GEMM_ROUTE_X6 5            /* gemm_x6_kernel: 128 x 256 bf16 tiles, with the tail of out8[2] */
#define GCT_GEMM_ROUTE_F32_FAST 6      /* gemm_f32_fast_kernel */
#define GCT_GEMM_ROUTE_F32_VEC 7       /* gemm_f32_kernel, float4 loads */
#define GCT_GEMM_ROUTE_F32 8           /* gemm_f32_kernel, scalar loads */
int gct_linear_fwd_route(int64_t M, int K, int nseg, int nper, int64_t ldx, int64_t ldw, int64_t ldy, int epi,
                         int aligned16, int have_planes, int have_bias, int mode, int64_t ws_bytes, int64_t* out8);
int gct_linear_dgrad_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldw, int64_t lddx, int depi,
                           int aligned16, int have_planes, int mode, int64_t ws_bytes, int64_t* out8);
/* diagnostics: what the most recent gct_linear_fwd / gct_linear_dgrad call on this thread executed, in the layout above,
 * written by the launcher where it launches (not a second run of the planner); under stream capture out8[2] is 0 and a
 * GCT_GEMM_ROUTE_X6 call is one launch.  Before the first call: GCT_GEMM_ROUTE_NONE. */
int gct_gemm_last_route(int64_t* out8);

/* dw_s[n][k] = sum_m dy_s[m][n] * x[m][k] ; db_s[n] = sum_m dy_s[m][n]  (overwrite).
 * Split over M into fp32 slabs in ws, reduced deterministically (no atomics).
 * ws >= gct_wgrad_ws_bytes(M, nseg*nper, K). db* nullable.
 * tile_list / tile_count (nullable, together): reduce only over the listed 32-row token tiles (gct_nonzero_row_tiles /
 * gct_live_rows, below) -- exact whenever every dy row outside them is zero (the skipped terms are 0 * x).  The list
 * is honoured by the bf16x6 kernel; the fp32 kernels reduce over all rows (same result).
 * Contract:
 *   - the list holds ASCENDING indices of 32-row tiles, each below M / 32; M % 32 == 0 on the route that reads it
 *     (GCT_WGRAD_BF16_TILES is taken only for such M);
 *   - *tile_count == 0, or M == 0, gives dw = 0 and db = 0 exactly (dy0 and x must still be non-null);
 *   - the call writes nothing outside dw*, db* and the first gct_wgrad_ws_bytes(M, nseg*nper, K) bytes of ws;
 *   - what dw*, db* and ws hold on entry does not affect the result. */
int gct_linear_wgrad(const float* dy0, const float* dy1, const float* dy2, int64_t lddy,
                     int64_t M, int nseg, int nper, const float* x, int64_t ldx, int K,
                     float* dw0, float* dw1, float* dw2, int64_t lddw,
                     float* db0, float* db1, float* db2, float* ws,
                     const int32_t* tile_list, const int32_t* tile_count, void* stream);
/* The route gct_linear_wgrad takes for a shape (no launch, no device access; the rule the call itself executes):
 *   out4[0] kernel: GCT_WGRAD_F32_SCALAR (gemm_f32_kernel, scalar loads), GCT_WGRAD_F32_VEC (the same with float4
 *           loads), GCT_WGRAD_F32_FAST (gemm_f32_fast_kernel) or GCT_WGRAD_BF16_TILES (gemm_x6_kernel, bf16x6 / bf16x3);
 *   out4[1] nsplit: slabs written, one per range of rows;
 *   out4[2] rows per split (a multiple of 32; with a tile list split z takes entries [z * per, z * per + per) of the
 *           list instead, per = ceil(*tile_count / nsplit));
 *   out4[3] 1: the GEMM kernel writes the bias slabs behind the weight slabs; 0: gct_colsum, which borrows the head
 *           of ws before the slabs are written (or no bias asked for).
 * aligned16: dy0..2, x and ws are all 16-byte aligned.  want_bias: db0 != NULL.  mode: a GCT_GEMM_* value (below),
 * passed in rather than read from the process. */
#define GCT_WGRAD_F32_SCALAR 0
#define GCT_WGRAD_F32_VEC 1
#define GCT_WGRAD_F32_FAST 2
#define GCT_WGRAD_BF16_TILES 3
int gct_wgrad_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldx, int aligned16, int want_bias,
                    int mode, int64_t* out4);

/* One nn.Linear's backward: gct_linear_wgrad and gct_linear_dgrad of the same dY in one call (ABI 28).  The arguments are
 * those of the two calls (dy*, lddy, M, nseg, nper once); wws / wws_bytes is the weight-gradient workspace
 * (>= gct_linear_bwd_ws_bytes(M, nseg*nper, K)), dws / dws_bytes the dgrad's (nullable, as for gct_linear_dgrad).
 * When both problems take the 128 x 256 bf16 tile kernel on their own, the stream is not being captured, dx overlaps
 * neither dy* nor x, and the planner's model of the shared grid is shorter than that of the two launches, both run as
 * ONE kernel launch (gemm_x6_bwd_pair_kernel: weight-gradient workgroups first, then the dgrad tiles; no dgrad tail
 * launch, no fix-up).  dx and db* are then bit-identical to the separate calls; dw* too whenever the split
 * (gct_linear_bwd_route's out8[1], out8[2]) equals gct_wgrad_route's, and otherwise differs by the fp32 summation order
 * over the slabs only.  In every other case the call IS the two separate calls, in the order wgrad, dgrad.
 * The slab reduction is issued (or deferred, gct_reduce_defer_begin) exactly as by gct_linear_wgrad. */
int gct_linear_bwd(const float* dy0, const float* dy1, const float* dy2, int64_t lddy, int64_t M, int nseg, int nper,
                   const float* x, int64_t ldx, int K,
                   float* dw0, float* dw1, float* dw2, int64_t lddw, float* db0, float* db1, float* db2,
                   float* wws, int64_t wws_bytes, const int32_t* tile_list, const int32_t* tile_count,
                   const float* w0, const float* w1, const float* w2, int64_t ldw,
                   const uint16_t* wp0, int64_t plane_stride,
                   float* dx, int64_t lddx, int depi, const float* pre, float p, uint64_t seed, uint32_t site,
                   float* dws, int64_t dws_bytes, const int32_t* quad_map, int64_t pre_rows, void* stream);
int64_t gct_linear_bwd_ws_bytes(int64_t M, int64_t Ntot, int64_t K);
/* The plan of a gct_linear_bwd call for a shape (no launch, no device access; stream capture and overlapping buffers,
 * which also keep a call from being paired, are not shapes and not reported here):
 *   out8[0] 1: one paired launch; 0: the two separate calls;
 *   out8[1] nsplit, out8[2] rows per split (a multiple of 32) of the weight gradient, as in gct_wgrad_route;
 *   out8[3] bias slabs written by the GEMM kernel;
 *   out8[4], out8[5] weight-gradient and dgrad blocks of the paired grid (0 when not paired);
 *   out8[6], out8[7] modelled duration of the paired launch and of the two separate calls, in 1/1000 of the time of
 *           one 128 x 256 x 32 dgrad K-tile (0: not modelled -- a problem is not on the bf16 tile route).
 * aligned16: every buffer is 16-byte aligned; have_planes: wp0 != NULL; ws_bytes: wws_bytes of the call. */
int gct_linear_bwd_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldx, int64_t ldw, int64_t lddx,
                         int depi, int aligned16, int have_planes, int want_bias, int mode, int64_t ws_bytes,
                         int64_t* out8);

/* ---- GEMM arithmetic mode and pre-split weights ------------------------------------------
 * The nn.Linear GEMMs (Model/sublayers.py:54-59,64-66,70,81-88) run in one of two modes with
 * fp32 operands, fp32 results and fp32-class error:
 *   GCT_GEMM_F32    : v_mfma_f32_32x32x2_f32 (fp32 fma chains);
 *   GCT_GEMM_BF16X6 : every operand element is split EXACTLY into three bf16 values (8+8+8
 *                     significand bits) and the six leading partial products are accumulated in
 *                     fp32 by v_mfma_f32_16x16x32_bf16; launches that do not qualify (odd shapes,
 *                     skinny M, no planes for fwd/dgrad) use the fp32 kernels.
 * and one opt-in lower-precision mode (PyTorch's "high" float32 matmul precision tier):
 *   GCT_GEMM_BF16X3 : the bf16x6 routes and kernels with two pieces per element, x ~ h + m (the
 *                     first two pieces of the same split, so the same weight planes serve), and
 *                     the three leading products am*bh + ah*bm + ah*bh.  Dropped per product:
 *                     <= (3u^2 + 4u^3 + u^4)|a*b| < 3.02 * 2^-16 |a*b| (u = 2^-8), i.e. about 16
 *                     good bits instead of 24, plus the fp32 accumulation error all modes share.
 *                     Launches that take the fp32 kernels in bf16x6 mode take them here too.
 * Process-wide; default from the environment (GCT_GEMM_MODE=f32|x6, x6 when unset); bf16x3 only
 * through gct_gemm_set_mode. */
#define GCT_GEMM_F32 0
#define GCT_GEMM_BF16X6 1
#define GCT_GEMM_BF16X3 2
int gct_gemm_set_mode(int mode);
int gct_gemm_get_mode(void);
/* diagnostics: out2[0] = launches of the fp32-MFMA tile kernels so far, out2[1] = of the bf16x6 kernels
 * (bf16x3 calls are counted by neither) */
int gct_gemm_launch_counts(int64_t* out2);
/* diagnostics: bf16x6 (3-piece) gemm_x6 / gemm_x6s kernel launches so far (a tail-balanced forward / dgrad
 * call launches two) */
int64_t gct_gemm_x6_kernel_launches(void);
/* diagnostics: bf16x3 (2-piece) launches of the same kernels so far, counted the same way */
int64_t gct_gemm_x3_launches(void);

/* planes[p*plane_stride + i] = p-th bf16 piece (p = 0 high, 1 middle, 2 low) of src[i], i < numel.
 * numel % 4 == 0, plane_stride % 4 == 0, plane_stride >= numel; src 16-B aligned.  Run it over the
 * model's flat parameter buffer once per step: the plane of a weight that starts at element offset o
 * of the buffer starts at element offset o of every plane. */
int gct_split_planes(const float* src, int64_t numel, uint16_t* planes, int64_t plane_stride,
                     void* stream);

/* ---- cross-attention K | V straight from the latent (ABI 32) ------------------------------
 * Model/vaetf.py:81: the decoder memory is e = fc_z(z) = z W_z^T + b_z (W_z [dm][lat]).  Where e feeds nothing but the
 * k_linear | v_linear projections of the decoder layers (no cond2lat rows), layer l's K | V are an affine image of z:
 *   kvb_l = z A_l^T + c_l,   A_l = W_kv,l W_z  [2d][lat],   c_l = W_kv,l b_z + b_kv,l,
 * and with P_l = dkv_l^T z, s_l = colsum(dkv_l) (gct_linear_bwd / gct_linear_wgrad over the rows of z against A_l):
 *   dW_kv,l = P_l W_z^T + s_l (x) b_z,  db_kv,l = s_l,  dW_z = sum_l W_kv,l^T P_l,  db_z = sum_l W_kv,l^T s_l.
 * gct_kv_fold_fwd, for all layers of a step (w_addrs / b_addrs: HOST arrays of 2 * layers device addresses, k_linear
 * then v_linear of each layer, weights [d][dm], biases [d]; b_addrs nullable):
 *   wstack [layers * 2d][dm] = the weights stacked (one copy: the products below then are single launches);
 *   c      [layers * 2d]     = wstack b_z + biases (the same launch, exact-fp32 dot products);
 *   a      [layers * 2d][lat] = wstack W_z, as gct_linear_dgrad computes it (bf16x6 with wzp, the planes of W_z);
 *   a_planes (nullable)      = gct_split_planes(a).
 * ws >= gct_kv_fold_ws_bytes.  1 .. GCT_KV_FOLD_MAX_LAYERS layers; d, dm, lat multiples of 4; the weights, wz, bz, wstack
 * and a 16-byte aligned (a_planes: 8, a_plane_stride % 4 == 0 and >= layers * 2d * lat; elements beyond that many of each
 * plane are not written).
 * gct_kv_fold_wgrad, one layer: p [2d][lat] and s [2d] as above -> dw0, dw1 [d][dm] (k_linear, v_linear) and
 * db0, db1 [d], overwritten; fp32 fma chains over lat (no shorter than the bf16x6 kernels' chains: same error class).
 * dm and lat multiples of 4, d any positive number (unlike gct_kv_fold_fwd); p, wz, bz, dw0, dw1 16-byte aligned.
 * gct_kv_fold_dbz: dbz[dm] = wstack^T s over rows = layers * 2d rows (s: the stacked s_l), overwritten, deterministic.
 * Any rows, dm > 0, no alignment asked; ws_bytes >= ceil(rows / 32) * dm * 4 (gct_kv_fold_ws_bytes covers it).
 * Layer count, widths, alignment, the weight table and the dbz workspace are checked before anything is launched: a call
 * refused for one of them leaves its outputs untouched (a_planes' own checks are gct_split_planes', made after a is written).
 * dW_z is gct_linear_wgrad of dY = wstack against X = the stacked P_l. */
#define GCT_KV_FOLD_MAX_LAYERS 16
int64_t gct_kv_fold_ws_bytes(int layers, int d, int dm, int lat);
int gct_kv_fold_fwd(int layers, const int64_t* w_addrs, const int64_t* b_addrs, int d, int dm,
                    const float* wz, const uint16_t* wzp, int64_t wz_plane_stride, const float* bz, int lat,
                    float* wstack, float* a, float* c, uint16_t* a_planes, int64_t a_plane_stride,
                    float* ws, int64_t ws_bytes, void* stream);
int gct_kv_fold_wgrad(const float* p, const float* s, int d, int lat, const float* wz, const float* bz, int dm,
                      float* dw0, float* dw1, float* db0, float* db1, void* stream);
int gct_kv_fold_dbz(const float* wstack, const float* s, int64_t rows, int dm, float* dbz, float* ws,
                    int64_t ws_bytes, void* stream);

/* Zero-gradient rows.  Under an ignore_index loss the rows of padded target positions carry exactly zero
 * gradients through the whole decoder backward.  gct_nonzero_row_tiles lists, in ascending order, the 32-row
 * tiles of x[rows][cols] that hold a non-zero element (list: >= ceil(rows/32) int32; count: device scalar;
 * flags_ws: >= ceil(rows/32) bytes) for gct_linear_wgrad's tile_list / tile_count. */
/* *counter += number of rows of g[rows][cols] with live[row] == 0 that hold a non-zero element: the check a forward
 * that SKIPPED the dead rows (decoder forward over the rows that reach the loss) owes its backward -- a gradient on a
 * skipped row cannot be honoured.  The caller reads the counter at its next host synchronisation. */
int gct_dead_rows_nonzero(const float* g, int64_t ld, int64_t rows, int cols, const uint8_t* live,
                          int32_t* counter, void* stream);
int gct_nonzero_row_tiles(const float* x, int64_t ld, int64_t rows, int cols, int32_t* list,
                          int32_t* count, uint8_t* flags_ws, void* stream);
/* The property above holds only if no live query row attends to a dead (zero-gradient) row: a dead row that is a
 * VISIBLE KEY of a live query receives dK / dV (and a live row that sees NO key attends uniformly to all of them).
 * gct_live_rows derives the live rows of g[B*T][cols] and CHECKS the property on the device against the
 * self-attention mask actually used (mask element (b,i,j) at mask[b*mask_sb + i*mask_sq + j]; NULL = everything
 * visible; mask_sq == 0 = key-padding mask):
 *   live [B*T] u8; n_b [B] live rows per sample;
 *   info [8] i32: [0] live rows, [1] samples that violate the property, [2] samples whose live rows are not the
 *                 prefix 0..n_b-1, [3] listed token tiles, [4] compact rows (multiple of 128), [5] live quads;
 *   tile_list / tile_count / tile_flags_ws (nullable, together): the 32-row token tiles that hold a live row --
 *   EVERY tile when info[1] != 0, so gct_linear_wgrad stays exact without a host round trip;
 *   cstart [B] / quad_list [ceil(B*T/4)+32] / qrank_ws [ceil(B*T/4)] (nullable, together): the COMPACTION MAP of the
 *   decoder backward.  Rows are compacted in aligned groups of 4 ("quads"), the granularity at which every dropout
 *   site draws its Philox values: compact row 4i+e <-> original row 4*quad_list[i]+e (quad_list ascending, padded
 *   with -1 to a multiple of 32 quads); sample b's row t sits at compact row cstart[b]+t for t < n_b[b] (live rows
 *   that are a prefix).  cstart never decreases over the samples: a sample without a live row gets the compact row
 *   where the next live row at or behind its own rows starts (4 * live quads, at most, when there is none).
 * gct_gather_quads / gct_scatter_quads move rows between the two spaces (scatter: dst pre-zeroed by the caller). */
int gct_live_rows(const float* g, int64_t ld, int B, int T, int cols, const uint8_t* mask, int64_t mask_sb,
                  int64_t mask_sq, uint8_t* live, int32_t* n_b, int32_t* info, int32_t* cstart,
                  int32_t* quad_list, int32_t* qrank_ws, int32_t* tile_list, int32_t* tile_count,
                  uint8_t* tile_flags_ws, void* stream);
/* The same compaction map for the KEY side of cross-attention, from a key-padding mask [B][Lk] (element (b,k) at
 * mask[b*mask_sb + k]): padded rows of the encoder memory are masked keys -- their K / V projections are never used
 * and their dK / dV are zero -- so the K / V GEMMs and their backward can run on the visible rows only.  Usable when
 * info[2] == 0 (visible keys are a prefix of every row) and info[6] == 0 (every sample sees a key).
 * info: [0] visible keys, [2] non-prefix samples, [4] compact rows, [5] live quads, [6] samples without a visible key. */
int gct_key_rows(const uint8_t* mask, int64_t mask_sb, int B, int Lk, uint8_t* live, int32_t* n_b, int32_t* info,
                 int32_t* cstart, int32_t* quad_list, int32_t* qrank_ws, void* stream);
int gct_gather_quads(const float* src, int64_t ld, int64_t M, const int32_t* quad_list, int64_t nrows, int cols,
                     float* dst, int64_t ldd, void* stream);
int gct_scatter_quads(const float* src, int64_t ld, const int32_t* quad_list, int64_t nrows, int cols, float* dst,
                      int64_t ldd, int64_t M, void* stream);
/* Zero the rows of a compact [nrows][cols] buffer that belong to no sample: [cstart[b] + n_b[b], cstart[b+1]) for every
 * b and [.., nrows) behind the last one -- what a kernel that writes only rows cstart[b] .. + n_b[b] (attention over
 * compact rows) leaves untouched; no row of a live prefix is written, whatever the order of the two kernels.  cstart
 * must be non-decreasing (gct_live_rows / gct_key_rows emit it so, samples without a live row included).  nrows is the
 * caller's: the compact rows alone, or with the slack rows that follow them in the allocation. */
int gct_zero_gap_rows(float* buf, int64_t ld, int cols, const int32_t* cstart, const int32_t* n_b, int B, int64_t nrows,
                      void* stream);
/* dst rows += the compact rows (gradient of rows that were gathered: the encoder's K | V over its visible rows) */
int gct_scatter_add_quads(const float* src, int64_t ld, const int32_t* quad_list, int64_t nrows, int cols, float* dst,
                          int64_t ldd, int64_t M, void* stream);

/* elementwise dropout backward for the GCT_EPI_DROP_RESID sites: dy = dropmask*dout/(1-p); quad_map (nullable):
 * the rows are quad-compacted, the mask of compact quad q is that of original quad quad_map[q] */
int gct_dropout_bwd(const float* dout, float* dy, int64_t rows, int cols, float p, uint64_t seed,
                    uint32_t site, const int32_t* quad_map, void* stream);

/* ------------------------------------------------------------- K4: attention */
/* Model/sublayers.py:29-41 attention() + head split/merge :64-69.
 * q,k,v are [B][L][H*dk]-shaped views with leading dimension ld* (so the fused QKV
 * buffer is consumed in place); head h uses columns h*dk..h*dk+dk-1.
 * mask: PACKED by gct_attn_mask_pack -- one bit per key, 8 uint32 words per query row (Lk <= 256), bit (k & 31)
 * of word k >> 5 set <=> key k visible; row of (b,q) at mbits + b*mb_sb + q*mb_sq (strides in words, multiples of
 * 4; mb_sq == 0 broadcasts a key-padding mask); a cleared bit => score := -1e9 (masked_fill semantics). nullable.
 * Pack once per forward: the same rows serve every layer, every head and the backward pass.
 * o: [B][Lq][H*dk] (heads merged, ready for the out projection); lse: [B][H][Lq], the log-sum-exp of the row's scaled
 * scores over its visible keys (a masked key's exp(-1e9 - max) is exactly 0 in fp32).  A row WITHOUT a visible key
 * is uniform over its Lk keys; -1e9 + log(Lk) is not representable in fp32, so its lse is log(Lk) and the backward
 * scores its masked keys as 0 instead of -1e9.
 * probs (nullable): pre-dropout probabilities [B][H][Lq][Lk] (get_attn path).
 * dk in {16, 32, 64}; Lq, Lk <= 208 (the reference's positional table ends at 200: Model/modules.py:117; + 3
 * condition tokens).  Lk <= GCT_ATTN_DIRECT_MAX_KEYS runs the barrier-free kernels (one wave per query / key tile),
 * longer rows the LDS kernels. */
#define GCT_ATTN_DIRECT_MAX_KEYS 96
/* mask: uint8, element (b,q,k) at mask[b*mask_sb + q*mask_sq + k] (0 = masked); mask_sq == 0: key-padding mask
 * [B][Lk] -> bits [B][8]; else bits [B][Lq][8]. */
/* tiles (nullable): one word per (batch, 16-row query tile) -- [B][1] for a key-padding mask, [B][ceil(Lq/16)]
 * otherwise -- bit t set <=> key tile t must be visited; passed to gct_attn_fwd / gct_attn_bwd as tbits with the
 * strides (tb_sb, tb_su) = (1, 0) resp. (ceil(Lq/16), 1), it lets a wave request its K rows before its mask rows
 * are back.  The kernels compute the same word themselves when tbits is NULL.
 * The rule, per query tile (rows 16u .. 16u+15 that are below Lq; for a key-padding mask the single row): when every
 * such row sees at least one key, bit t is set <=> one of them sees a key among keys 16t .. 16t+15 (below Lk);
 * when one of them sees no key at all, all ceil(Lk/16) bits are set -- that row is uniform over its Lk keys
 * (masked_fill(-1e9) on the whole row), so every key tile contributes.  Bits at and above ceil(Lk/16) are 0. */
int gct_attn_mask_pack(const uint8_t* mask, int64_t mask_sb, int64_t mask_sq, int B, int Lq, int Lk,
                       uint32_t* bits, uint32_t* tiles, void* stream);
/* The decoder's self-attention mask straight from the token ids: the uint8 form of get_trg_mask(target, pad, False)
 * (Model/modules.py:17-30, 47-58: pad mask & no-peek pattern * pad_idx, so out[b][q][k] = (tokens[b][k] != pad) &
 * (k <= q) & (pad & 1)) in ONE launch instead of the reference's int64 [B][T][T] tensor and its ~10 elementwise
 * launches.  tokens: [B] rows of T ids, leading dimension ld_tok; out: uint8 [B][T][T], 4-byte aligned. */
int gct_trg_mask_tokens(const int64_t* tokens, int64_t ld_tok, int64_t pad, int B, int T, uint8_t* out, void* stream);
int gct_attn_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                 int64_t ldv, const uint32_t* mbits, int64_t mb_sb, int64_t mb_sq,
                 float* o, int64_t ldo, float* lse, float* probs, int B, int H, int Lq, int Lk,
                 int dk, float scale, float p, uint64_t seed, uint32_t site, const int32_t* kstart,
                 const int32_t* klen, const uint32_t* tbits, int64_t tb_sb, int64_t tb_su,
                 const int32_t* qstart, const int32_t* qlen, void* stream);
/* kstart / klen (nullable, together; gct_key_rows): k and v hold only the VISIBLE keys of every sample, quad-compacted:
 * the rows of sample b start at kstart[b] and there are klen[b] of them (keys klen[b]..Lk-1 are masked by mbits).
 * qstart / qlen (nullable, together; gct_live_rows): q and o hold only the first qlen[b] query rows of sample b, at rows
 * qstart[b].. (the decoder forward over the rows that reach the loss); lse keeps its [B][H][Lq] layout, entries of rows
 * that do not exist are not written.  Needs the direct kernels (Lk <= GCT_ATTN_DIRECT_MAX_KEYS, probs == NULL). */
/* dq/dk/dv written (overwrite) with the same layout as q/k/v.
 * cstart / nlive (nullable, together): dout and dq are quad-compacted (gct_live_rows): the rows of sample b start at
 * cstart[b] and only its first nlive[b] query rows exist; kv_compact bit 0 (self-attention, Lq == Lk): dk / dv live
 * in those compact rows too while q, k, v, o stay in the forward's layout; kv_compact bit 1: q and o are compact like
 * dout / dq (the forward ran with qstart / qlen; pass kstart / klen = cstart / nlive for self-attention) -- direct
 * kernels only.  lse keeps the forward's layout. */
int gct_attn_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                 int64_t ldv, const uint32_t* mbits, int64_t mb_sb, int64_t mb_sq,
                 const float* o, const float* dout, int64_t ldo, const float* lse,
                 float* dq, int64_t lddq, float* dk_, int64_t lddk, float* dv, int64_t lddv,
                 int B, int H, int Lq, int Lk, int dk, float scale, float p, uint64_t seed,
                 uint32_t site, const int32_t* cstart, const int32_t* nlive, int kv_compact,
                 const int32_t* kstart, const int32_t* klen, const uint32_t* tbits, int64_t tb_sb, int64_t tb_su,
                 void* ws, int64_t ws_bytes, void* stream);
/* kstart / klen as in gct_attn_fwd: k, v AND dk, dv hold the visible keys only (excludes kv_compact).
 * ws / ws_bytes: caller-owned scratch (16-B aligned, ws_bytes >= gct_attn_bwd_ws_bytes) of the two-launch backward that
 * runs for Lk <= GCT_ATTN_DIRECT_MAX_KEYS (one wave per query tile -> dq, then one wave per key tile -> dk, dv; no LDS).
 * Required whenever gct_attn_bwd_ws_bytes > 0: a null, short or misaligned ws is GCT_ERR_ARG.  Longer rows run the
 * single-launch LDS kernel and need none (gct_attn_bwd_ws_bytes == 0, ws may be NULL). */
int64_t gct_attn_bwd_ws_bytes(int B, int H, int Lq, int Lk);
/* The route gct_attn_fwd (bwd == 0) / gct_attn_bwd (bwd != 0) take for a shape, from the planner they launch by:
 * out4 = {kind (0 direct, 1 LDS 8 tiles, 2 LDS 13 tiles), grid, grid_kv, dynamic LDS bytes}.  grid: workgroups of the
 * launch (direct backward: of the dQ launch, grid_kv of the dK / dV launch; else grid_kv = 0); the LDS kernels are
 * persistent, so npairs > grid means that workgroups walk several (batch, head) pairs.  cus: compute units to plan
 * for; cus <= 0: the device's own count.  No launch, no device memory. */
int gct_attn_route(int bwd, int Lq, int Lk, int dk, int64_t npairs, int cus, int64_t* out4);

/* ------------------------------------------------- K6: reparameterisation + KL */
/* Model/sublayers.py:14-20 / Model/cvaetf.py:63-69: z = eps*exp(0.5*log_var)+mu.
 * eps_in nullable: then eps ~ N(0,1) is generated in-kernel (Philox + Box-Muller,
 * key (seed,site)) and written to eps_out (always written). */
int gct_reparam_fwd(const float* mu, const float* log_var, const float* eps_in, float* eps_out,
                    float* z, int64_t n, uint64_t seed, uint32_t site, void* stream);
/* dmu = dz + dmu_ext ; dlv = 0.5*dz*eps*exp(0.5*lv) + dlv_ext  (ext nullable) */
int gct_reparam_bwd(const float* dz, const float* log_var, const float* eps, const float* dmu_ext,
                    const float* dlv_ext, float* dmu, float* dlv, int64_t n, void* stream);
/* Train/trainer1.py:23  KLD = -0.5*sum(1+lv-mu^2-exp(lv)) over ALL n elements.
 * out[0] overwritten. ws >= 1024 floats. */
int gct_kld_fwd(const float* mu, const float* log_var, float* out, float* ws, int64_t n,
                void* stream);
/* dmu = g*mu ; dlv = g*0.5*(exp(lv)-1), g read from device scalar gout[0] */
int gct_kld_bwd(const float* mu, const float* log_var, const float* gout, float* dmu, float* dlv,
                int64_t n, void* stream);

/* Per-dimension KL with free bits and a row mask (Kingma et al. 2016; engine.kl_dims_reference states the rule in
 * fp64).  mu, log_var fp32 [R][D]; live u8 [R] (nullable: every row counts), nonzero = the row is a real source
 * position or a condition row.  With t(r, j) = 1.0f + l - m*m - expf(l), gct_kld_fwd's fp32 expression:
 *   K_j       = -0.5 * sum over live rows r, in ascending order, of (double) t(r, j)
 *   floor     = (double) free_bits * n_mol           (free_bits: nats per dimension per molecule, batch-averaged form)
 *   gate_j    = K_j > floor                           (strict, in fp64, before any rounding)
 *   objective = sum_j max(floor, K_j);  raw = sum_j K_j;  n_floor = #{j : !gate_j}
 * gct_kld_dims_fwd writes kl_dim[j] = (float) K_j, gate[j] = 1.0f or 0.0f, and out[0..3] = objective, raw, n_floor,
 * live rows, each rounded to fp32 once.  Two launches, no atomics: workgroups of 256 threads, D / 4 lanes per row
 * reading float4, write one fp64 partial per (workgroup, dimension) into ws (>= gct_kld_dims_ws_bytes(D) bytes); one
 * workgroup adds them in a fixed order.  The grid is a function of (R, D) alone (csrc/vae.hip states it), so the same
 * bytes give the same result on every run.  R == 0: K_j = 0, objective = D * floor, every gate 0 when floor > 0.
 * gct_kld_dims_bwd, one launch: d objective / d mu = gate_j * live_r * g * mu and d objective / d log_var =
 * gate_j * live_r * g * 0.5f * (expf(lv) - 1.0f) with g = gout[0] -- gct_kld_bwd's bits where the gate is open and the
 * row is live, exact +0.0f everywhere else.
 * gct_latent_moments, the same two launches with more sums: adds this batch's live rows into the caller's running
 * fp64 state acc [6][D] (zeroed by the caller once): rows 0-5 = sum mu, sum mu^2, sum expf(lv), sum lv, sum -0.5 * t,
 * live rows (the same count in every column).  Values are converted to double before the first product or sum; the
 * same batches in the same order give the same bytes.  R == 0 adds nothing.
 * Limits: D % 4 == 0, 4 <= D <= GCT_LATENT_MAX_DIM, R >= 0, n_mol >= 1, free_bits finite and >= 0; every pointer but
 * live 16-B aligned (gout: 4-B); else GCT_ERR_ARG before a launch.  gct_kld_dims_ws_bytes: 0 for a D outside the limits. */
int64_t gct_kld_dims_ws_bytes(int D);
int gct_kld_dims_fwd(const float* mu, const float* log_var, const uint8_t* live, int64_t R, int D,
                     float free_bits, int n_mol, float* out, float* kl_dim, float* gate, void* ws, void* stream);
int gct_kld_dims_bwd(const float* mu, const float* log_var, const uint8_t* live, const float* gate,
                     const float* gout, float* dmu, float* dlv, int64_t R, int D, void* stream);
int gct_latent_moments(const float* mu, const float* log_var, const uint8_t* live, int64_t R, int D,
                       double* acc, void* ws, void* stream);

/* --------------------------------------------- K12: latents for molecule interpolation */
/* Inference/mol_interpolation.py:124-131 (approximate_z's fit).  mu, log_var fp32 [n][Le][D] contiguous; rows int32 [n]
 * on the device: the first rows[i] latent rows of molecule i are its own (the prefix get_src_mask marks: condition
 * rows, scaffold, <sep>, tokens); rows at or beyond rows[i] are never read.  stats fp32 [n][4][D] = per dimension the
 * mean of mu, the standard deviation of mu, the mean of log_var, the standard deviation of log_var over those rows.
 * The standard deviation is the unbiased one (torch.std, ddof 1) in two passes, rows in ascending order: the mean
 * (sum / rows) first, then sqrt(sum of squared deviations / (rows - 1)).  rows[i] == 1 gives 0 (the reference: NaN).
 * No atomics: bit-reproducible.  Limits: 1 <= D <= GCT_LATENT_MAX_DIM, Le >= 1, 0 <= n <= 65535, else GCT_ERR_ARG before
 * a launch; 1 <= rows[i] <= Le is the caller's to check (ops.latent_stats does, on the host: the library does not read
 * device memory), and the kernel clamps rows[i] into that range instead of reading outside the molecule. */
#define GCT_LATENT_MAX_DIM 1024
int gct_latent_stats(const float* mu, const float* log_var, int n, int Le, int D, const int32_t* rows, float* stats,
                     void* stream);
/* Inference/mol_interpolation.py:124-141, 216-224: output row r interpolates molecule a[r] towards molecule b[r] of
 * stats (gct_latent_stats, n molecules).  z fp32 [R][T][D]; tokens t >= len[r] are written as exact zeros.  a, b, len,
 * item int32 [R], alpha, noise_std fp32 [R], all on the device.  For every t < len[r], one wave per (r, t):
 *   - five vectors of D standard normals n_s, s = 0..4, under the repository's N(0, 1) convention (Philox4x32-10, Box-
 *     Muller on the word pairs (x, y) and (z, w), u01 of csrc/vae.hip) with the key of (seed, site GCT_LATENT_SITE):
 *     element d of n_s is element d & 3 of the call with the counter (item[r], 8 * t + s, d >> 2, GCT_LATENT_C3).
 *     Nothing else enters the counter: a row's latent is a function of (seed, item, a, b, alpha, noise_std, len) and
 *     not of R, T or its position in the batch.  item[r] >= 0 is the row's identity.
 *   - per dimension u = mean_mu[a] + std_mu[a] * n_0, v = mean_mu[b] + std_mu[b] * n_1, and p, q likewise from the
 *     log_var statistics with n_2, n_3.
 *   - m = slerp(u, v, alpha), l = slerp(p, q, alpha) over the D dimensions of the token: c = u.v / (|u| |v|),
 *     w = acos(c), result (sin((1 - alpha) w) u + sin(alpha w) v) / sin(w), not renormalised (as the reference).
 *     Guard: |u| == 0, |v| == 0 or not |c| <= GCT_LATENT_SLERP_MAX_COS (a NaN included) gives the lerp
 *     (1 - alpha) u + alpha v, evaluated as u + alpha (v - u) so that u == v returns u exactly (the reference divides
 *     by zero there).
 *   - z = m + noise_std[r] * n_4 * exp(0.5 * l); noise_std[r] == 0 writes exactly m (and l is not evaluated).
 * The sums over D run in a fixed lane order, independent of the grid.  Limits: 1 <= D <= GCT_LATENT_MAX_DIM, R >= 0
 * (R == 0 writes nothing), T >= 1, n >= 1, R * T <= 2^25 (one wave each: 2^31 work-items in the launch), else GCT_ERR_ARG before a launch.  0 <= len[r] <= T and a[r],
 * b[r] in [0, n) are the caller's to check (ops.latent_interp does, on the host, and raises before a launch); the
 * kernel reads nothing through a bad index: len[r] > T acts as T, and a row whose a or b is outside [0, n) is zeros. */
#define GCT_LATENT_SITE 0x1A7E47u
#define GCT_LATENT_C3 0x082EFA98u
#define GCT_LATENT_SLERP_MAX_COS 0.99999904632568359375f /* 1 - 2^-20 */
int gct_latent_interp(const float* stats, int n, int D, const int32_t* a, const int32_t* b, const float* alpha,
                      const float* noise_std, const int32_t* len, const int32_t* item, int64_t R, int T, float* z,
                      uint64_t seed, void* stream);

/* ------------------------------------ K13: importance-weighted marginal likelihoods */
/* K draws z_k ~ q(z | x) = N(mu, exp(log_var)) per molecule with the prior / posterior part of their log-weights
 * (Burda et al., IWAE): log w_k = log p(x | z_k) + log p(z_k) - log q(z_k | x); the decoder supplies the first term
 * (gct_seq_logp), gct_latent_iw the latents and the other two, gct_iw_combine the bound.
 * mu, log_var fp32 [n][Le][D] contiguous; rows int32 [n] on the device: molecule i owns its first rows[i] latent rows
 * (gct_latent_stats' rule); item int32 [n] on the device: the molecule's stream id, >= 0.  The call makes the draws
 * k = k0 .. k0 + Kc - 1 of every molecule; output row r = i * Kc + (k - k0) (sample-major, the order of
 * decode_unique(return_rows=True)).  z fp32 [n * Kc][Le][D], logw fp32 [n * Kc], eps_out nullable, z's shape.
 * For every t < rows[i] and every d:
 *   - eps: a standard normal under the repository's N(0, 1) convention (Philox4x32-10, Box-Muller on the word pairs
 *     (x, y) and (z, w), u01 of csrc/vae.hip) with the key of (seed, site GCT_IW_SITE): element d & 3 of the call with
 *     the counter (item[i], k, 256 * t + (d >> 2), GCT_IW_C3).  d >> 2 < 256 because D <= GCT_LATENT_MAX_DIM, and
 *     256 * t fits because Le <= 2^24.  Nothing else enters: the draw (item, k, t, d) does not depend on n, Le, k0, Kc,
 *     the order of the molecules or the grid.
 *   - z = fmaf(eps, expf(0.5f * log_var), mu), gct_reparam_fwd's form.
 *   - term = 0.5f * fmaf(eps - z, eps + z, log_var) = log N(z; 0, 1) - log N(z; mu, exp(log_var)): the log 2 pi terms
 *     cancel, and (z - mu)^2 / exp(log_var) is eps^2.
 * Rows t >= rows[i] of z (and of eps_out) are written as exact zeros and add nothing to logw (gct_latent_interp's
 * rule; the decoder never reads them through src_mask).
 * logw[r] = the sum of the row's terms, each widened to fp64 and added in fp64, rounded once to fp32, in a fixed order:
 * with nq = (D + 3) / 4 the quad (t, d >> 2) has the index q = t * nq + (d >> 2); work-item w of 256 adds the quads
 * q = w, w + 256, ... in ascending order, the four elements of a quad in ascending d; the 64 work-items of a wave are
 * summed by a butterfly (xor 32, 16, .. 1), and the four waves as (w0 + w1) + (w2 + w3).  No atomics: bit-reproducible,
 * and independent of the grid (one workgroup per output row).
 * mu == 0 and log_var == 0 give z == eps bit for bit and logw == 0 exactly: that is why the term is written with
 * (eps - z) (eps + z) and not with squares.
 * Limits: 1 <= D <= GCT_LATENT_MAX_DIM, 1 <= Le <= 2^24, n >= 0, Kc >= 0 (a zero writes nothing), k0 >= 0,
 * k0 + Kc <= 2^31 - 1, n * Kc * Le <= 2^25, else GCT_ERR_ARG before a launch with the outputs untouched.
 * 1 <= rows[i] <= Le and item[i] >= 0 are the caller's to check (ops.latent_iw does, on the host); the kernel clamps
 * rows[i] into [1, Le] instead of reading outside the molecule. */
#define GCT_IW_SITE 0x1A7E48u
#define GCT_IW_C3 0x0D95748Fu
int gct_latent_iw(const float* mu, const float* log_var, int n, int Le, int D, const int32_t* rows,
                  const int32_t* item, int k0, int Kc, float* z, float* logw, float* eps_out, uint64_t seed,
                  void* stream);
/* logp (the decoder's log p(x | z_k), row i * K + k), logw (gct_latent_iw's) fp32 [n * K] -> per molecule, fp32 [n]
 * each, with a_k = (double)logp + (double)logw, every step in fp64 and one rounding to fp32 at the end:
 *   iwae  = m + log(sum_k exp(a_k - m)) - log K, m = max_k a_k (two passes: the maximum, then the sum)
 *   elbo  = (sum_k a_k) / K
 *   recon = (sum_k logp_k) / K
 *   ess   = (sum_k w_k)^2 / sum_k w_k^2 with w_k = exp(a_k - m): the effective sample size, in [1, K]
 * One wave per molecule: lane l holds k = l, l + 64, ... in ascending order, and the lanes are combined by a butterfly
 * (xor 32, 16, .. 1).  No atomics: bit-reproducible.  K == 1 gives iwae == elbo bit for bit and ess == 1.
 * Limits: n >= 0 (a zero writes nothing), K >= 1, n * K <= 2^31 - 1, else GCT_ERR_ARG before a launch. */
int gct_iw_combine(const float* logp, const float* logw, int n, int K, float* iwae, float* elbo, float* recon,
                   float* ess, void* stream);

/* ---------------------------------------------------------- K7: cross-entropy */
/* Train/trainer1.py:21-22  F.cross_entropy(logits.view(-1,V), ys, ignore_index=pad,
 * reduction='sum').  out[0] overwritten. ws >= 1024 floats. */
int gct_ce_fwd(const float* logits, const int64_t* target, float* out, float* ws, int64_t rows,
               int V, int64_t pad_id, void* stream);
/* dlogits = g*(softmax - onehot) on non-pad rows, 0 on pad rows; g = gout[0] (device).
 * A target that is neither pad_id nor in [0, V) is not an error: gct_ce_fwd adds nothing for that row and gct_ce_bwd
 * writes g*softmax (no one-hot term) -- F.cross_entropy raises there. */
int gct_ce_bwd(const float* logits, const int64_t* target, const float* gout, float* dlogits,
               int64_t rows, int V, int64_t pad_id, void* stream);
/* Log-likelihoods of token rows (gct_plus_amd/decode.py score_reference states the rule), teacher-forced form.
 * ys [n][ld_ys] int64 holds full rows of W tokens: prefix, tokens, pad.  The logits row of token column c (c >= 1) of
 * sequence r is logits + (r * rows_per_seq + row_shift + c - 1) * ld, V floats (ld >= V: strided views; row_shift: the
 * condition rows a use_cond2dec decoder puts in front).  Column c is SCORED when c >= prefix_lens[r] (int32 [n],
 * 1 .. W; NULL: 1) and ys[r][c] != pad_id; the host validates 0 <= ys < V (an id outside counts as not scored).
 *   token_logp [n][ld_out]: x[t] - m - log(sum exp(x - m)) in fp32 at scored columns (m the row maximum), 0 elsewhere;
 *                           all W columns are written, and the logits rows of columns that are not scored are not read
 *   logp [n]:   the sum of the scored columns in ascending column order
 *   tokens [n]: the number of scored columns;  hits [n]: those whose token is the FIRST maximum of its logits row.
 * One workgroup per sequence, no atomics: bit-reproducible.  1 <= W <= 256, ld_ys >= W, ld_out >= W,
 * rows_per_seq >= row_shift + W - 1; otherwise GCT_ERR_ARG. */
int gct_seq_logp(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift, const int64_t* ys,
                 int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W, float* token_logp,
                 int64_t ld_out, float* logp, int32_t* tokens, int32_t* hits, void* stream);
/* The gradient of gct_seq_logp with respect to the logits (gct_plus_amd/decode.py seq_logp_grad_reference states the
 * rule); same geometry.  Logits row j of sequence r (0 <= j < rows_per_seq) predicts token column c = j - row_shift + 1
 * and is scored exactly when gct_seq_logp scores (r, c): j >= row_shift, 1 <= c < W, c >= prefix_lens[r],
 * ys[r][c] != pad_id and 0 <= ys[r][c] < V.  With g = g_logp[r] + g_token[r][c] (g_logp fp32 [n], g_token fp32
 * [n][ld_g]: the gradients of logp and token_logp; either may be NULL and then counts as 0, not both) a scored row gets
 *   dlogits[v] = (-g) * (softmax(x)[v] - [v == ys[r][c]])
 * in gct_ce_bwd's arithmetic (the same bits for the same row and weight).  A row that is not scored, or whose g is 0,
 * gets V exact zeros, and its logits are not read.  All n * rows_per_seq rows of dlogits (row stride ld_d >= V) are
 * WRITTEN, nothing is accumulated.  One wave per row, no atomics: bit-reproducible.  Shape limits as gct_seq_logp's;
 * otherwise GCT_ERR_ARG before any launch.  n == 0: nothing to do. */
int gct_seq_logp_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift, const int64_t* ys,
                     int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W, const float* g_logp,
                     const float* g_token, int64_t ld_g, float* dlogits, int64_t ld_d, void* stream);
/* Entropy of the next-token distribution and its KL divergence from a second ("prior") model's, per scored token and
 * per sequence (gct_plus_amd/decode.py dist_reference states the rule); gct_seq_logp's geometry and SCORED predicate.
 * prior_logits (nullable) has the agent's row numbering with its own row stride ld_prior >= V; token_kl and kl are
 * null exactly when it is.  With e_v = exp(x_v - m), se = sum e_v over a scored column's agent row x (m its maximum)
 * and m', se' the same of the prior's row y:
 *   token_entropy [n][ld_out]: log(se) - sum e_v (x_v - m) / se
 *   token_kl [n][ld_out]:      sum (e_v / se) ((x_v - m - log se) - (y_v - m' - log se'))
 * in fp32, a term with e_v == 0 (a -inf logit) left out; p_v > 0 where q_v == 0 gives +inf.  Columns that are not
 * scored hold 0 and NEITHER model's logits row of such a column is read; all W columns are written.
 *   entropy [n], kl [n]: the sums of the scored columns in ascending column order.
 * One workgroup per sequence, no atomics: bit-reproducible.  Shape limits as gct_seq_logp's; otherwise, and for kl
 * outputs without a prior (or a prior without them), GCT_ERR_ARG before any launch.  n == 0: nothing is written. */
int gct_seq_dist(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift, const float* prior_logits,
                 int64_t ld_prior, const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                 int W, float* token_entropy, int64_t ld_out, float* entropy, float* token_kl, float* kl, void* stream);
/* The gradient of gct_seq_dist with respect to the AGENT's logits (gct_plus_amd/decode.py dist_grad_reference states
 * the rule); the prior gets none.  Row numbering and predicate as gct_seq_logp_bwd's.  With
 * a = g_entropy[r] + g_token_entropy[r][c] and b = g_kl[r] + g_token_kl[r][c] (fp32 [n] and [n][ld_ge] / [n][ld_gk];
 * each nullable and then 0, not all four; the kl pair only with a prior) a scored row gets
 *   dlogits[v] = a * (-p_v (log p_v + H)) + b * (p_v ((log p_v - log q_v) - KL)),   exactly 0 where p_v == 0,
 * H and KL that row's token_entropy and token_kl.  A row that is not scored, or whose a and b are both 0, gets V exact
 * zeros and neither model's logits row is read.  All n * rows_per_seq rows of dlogits (row stride ld_d >= V) are
 * WRITTEN, nothing is accumulated.  One wave per row, no atomics: bit-reproducible.  Otherwise GCT_ERR_ARG before any
 * launch.  n == 0: nothing to do. */
int gct_seq_dist_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                     const float* prior_logits, int64_t ld_prior, const int64_t* ys, int64_t ld_ys,
                     const int32_t* prefix_lens, int64_t pad_id, int n, int W, const float* g_entropy,
                     const float* g_token_entropy, int64_t ld_ge, const float* g_kl, const float* g_token_kl,
                     int64_t ld_gk, float* dlogits, int64_t ld_d, void* stream);
/* PPO's clipped surrogate, per scored token and per sequence (ABI 29; gct_plus_amd/decode.py ppo_reference states the
 * rule); gct_seq_logp's geometry and SCORED predicate.  old_token_logp fp32 [n][ld_old >= W]: the log-probabilities the
 * tokens were sampled with; advantage fp32 [n]: one number per sequence; 0 <= clip_lo < 1, clip_hi >= 0.  At a scored
 * column, with lp = gct_seq_logp's token_logp (the same bits), A = advantage[r], rho = exp(lp - old): the token is
 * CLIPPED when A > 0 and rho > 1 + clip_hi, or A < 0 and rho < 1 - clip_lo (strict: rho == 1 never is), and
 *   token_surrogate [n][ld_out]: A * (1 + clip_hi) clipped high, A * (1 - clip_lo) clipped low, A * rho otherwise
 *                                (= min(rho A, clamp(rho, 1 - clip_lo, 1 + clip_hi) A) in value);
 *   token_logp [n][ld_out]:      lp.
 * Columns that are not scored hold 0 in both tables, and neither their logits rows nor their old_token_logp are read;
 * all W columns are written.  Per sequence, sums over the scored columns in ascending column order:
 *   logp [n], surrogate [n], approx_kl [n] (the k3 terms (rho - 1) - (lp - old) of KL(old || new)),
 *   tokens [n], hits [n] and clipped [n] (int32 counts; hits as gct_seq_logp's).  logp, tokens and hits are
 *   gct_seq_logp's bits.
 * Non-finite old_token_logp is not an error: IEEE arithmetic decides the result.  One workgroup per sequence, no
 * atomics: bit-reproducible.  Shape limits as gct_seq_logp's, ld_old >= W; otherwise, for a null old_token_logp or
 * advantage and for clips outside their ranges, GCT_ERR_ARG before any launch.  n == 0: nothing is written. */
int gct_seq_ppo(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift, const int64_t* ys,
                int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W, const float* old_token_logp,
                int64_t ld_old, const float* advantage, float clip_lo, float clip_hi, float* token_logp,
                float* token_surrogate, int64_t ld_out, float* logp, float* surrogate, float* approx_kl,
                int32_t* tokens, int32_t* hits, int32_t* clipped, void* stream);
/* The gradient of gct_seq_ppo's surrogate [n] and token_surrogate [n][W] with respect to the logits
 * (gct_plus_amd/decode.py ppo_grad_reference states the rule); row numbering and predicate as gct_seq_logp_bwd's.  With
 * g = g_surrogate[r] + g_token_surrogate[r][c] (fp32 [n] and [n][ld_g]; either may be NULL and then counts as 0, not
 * both) a scored row whose token is not clipped gets
 *   dlogits[v] = -((g * A) * rho) * (softmax(x)[v] - [v == ys[r][c]])
 * in gct_ce_bwd's arithmetic, (g * A) a plain fp32 product: with rho == 1 the bits of gct_seq_logp_bwd for g_logp =
 * g * A.  A row that is not scored, or whose A or g is 0, gets V exact zeros and its logits are not read; a row whose
 * token is clipped gets V exact zeros (its logits are read to decide).  All n * rows_per_seq rows of dlogits (row stride
 * ld_d >= V) are WRITTEN, nothing is accumulated.  One wave per row, no atomics: bit-reproducible.  Refusals as
 * gct_seq_ppo's and gct_seq_logp_bwd's: GCT_ERR_ARG before any launch.  n == 0: nothing to do. */
int gct_seq_ppo_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift, const int64_t* ys,
                    int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W,
                    const float* old_token_logp, int64_t ld_old, const float* advantage, float clip_lo, float clip_hi,
                    const float* g_surrogate, const float* g_token_surrogate, int64_t ld_g, float* dlogits,
                    int64_t ld_d, void* stream);
/* The decode-step form: launched after gct_select_token in the step unit, on the same logits [n][V] and the same
 * device counter.  Row r looks at column p = *pos - row_off[r] + 1 (row_off nullable), the column the selection has
 * just written, takes tok = ys[r][p] and writes out[dst][p] = log-softmax(logits[r])[tok], or 0 when tok == pad_id (a
 * finished row).  The log-probability is always the MODEL's own: it is taken from the raw logits at temperature 1,
 * whatever top-k / nucleus / temperature filter the draw went through.
 * item / prefix_len (both or neither, with row_off; continuous batching as in gct_select_token): dst = item[r], and the
 * row writes nothing when item[r] < 0 (parked) or p < prefix_len[item[r]] (a prefix token is not a generated one) --
 * so the call goes BEFORE gct_stream_refill, which reassigns item[r].  Without them dst = r.  Nothing is written when
 * p is outside [0, ld_out) or dst >= out_rows.  out [out_rows][ld_out]. */
int gct_chosen_logp(const float* logits, int V, const int64_t* ys, int64_t ld_ys, const int32_t* pos,
                    const int32_t* row_off, const int32_t* item, const int32_t* prefix_len, int64_t pad_id, float* out,
                    int64_t ld_out, int out_rows, int n, void* stream);

/* -------------------------------------------------------------- K8: Adam step */
/* torch.optim.Adam semantics (train1.py:116-119; no weight decay, no amsgrad):
 *   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * over one flat buffer of n elements; g is multiplied by gscale first (1/W folds the
 * data-parallel mean). `step` is t (1-based, already incremented). */
int gct_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                  float b2, float eps, int64_t step, float gscale, const int32_t* skip_if_nonzero,
                  const float* clip_state, void* stream);
/* skip_if_nonzero (nullable): a device-side guard: when *skip_if_nonzero != 0 at launch time nothing is updated (p, m,
 * v stay as they are).  The trainer passes the device counter of "gradient rows that fell on decoder rows the forward
 * had skipped" (gct_live_rows / gct_scatter_add_quads_check): a wrong gradient is then never applied, without a host
 * synchronisation in front of the update; the host raises at its next read-back.  NULL: no guard.
 * clip_state (nullable; new in ABI 33): the 8-word state gct_grad_norm (below) wrote for the same g and gscale.  The
 * step then consumes (g * gscale) * coef, in that order, with coef = word 1, and updates nothing when word 2 is set.
 * coef == 1 leaves (g * gscale) exact: a step that did not need to clip is bit-identical to the step without a state.
 * NULL: no clipping -- the kernel of the earlier versions; one kernel template serves both. */

/* Global gradient-norm clipping, torch.nn.utils.clip_grad_norm_'s rule computed on the device:
 *   norm = |gscale| * sqrt(sum g[k]^2)     (the L2 norm of the gradient Adam is about to see)
 *   coef = min(1, max_norm / (norm + 1e-6))
 * gct_grad_norm reads g [n] once (fp64 from the first product on: the result does not depend on n, on magnitudes or
 * on the grid), leaves g as it is and writes `state`, 8 32-bit words on the device:
 *   word 0  float  norm, pre-clip, of the scaled gradient
 *   word 1  float  coef; 0 when the step is to be skipped
 *   word 2  int32  nonfinite: 1 when norm is inf or NaN, else 0, for this step
 *   word 3  int32  steps
 *   word 4  int32  clipped_steps (finite steps with coef < 1)
 *   word 5  int32  nonfinite_steps
 *   word 6  float  the largest finite norm seen
 *   word 7         reserved, written as 0
 * Words 3-6 are running totals since the host last zeroed the state (the host zeroes all 8 words before first use).
 * A norm beyond fp32's range (> 3.4e38) rounds to inf in word 0 and counts as non-finite, as an inf or a NaN in g does.
 * Unlike torch, a non-finite norm skips the step: gct_adam_step, given the state, leaves p, m and v bit-unchanged.
 * Two launches: at most 2048 workgroups write one fp64 partial each into ws (>= gct_grad_norm_ws_bytes(n) bytes, the
 * caller's), one workgroup sums them in a fixed order -- no atomics, so the same bytes give the same state on every
 * run and on every rank of a data-parallel job.  Nothing is read by the host; both launches can be captured.
 * g, state, ws 16-B aligned; n >= 0 (n == 0: norm 0, coef 1; g may be NULL); max_norm finite and > 0. */
int64_t gct_grad_norm_ws_bytes(int64_t n);
int gct_grad_norm(const float* g, int64_t n, float gscale, float max_norm, float* state, void* ws, void* stream);

/* --------------------------------------------------------- K11: KV-cached decode */
/* Inference/sampling_tool.py:140-184 re-runs the whole decoder on ys[:, :i+1] each step; these
 * two kernels (with the GEMM/norm/embedding entry points above) make one step a fixed chain.
 * gct_attn_decode: ONE query row per (sample, head): q [n][H*dk] (ld ldq); keys/values row j of
 * sample b at k + b*kv_batch + j*kv_row (+ h*dk); valid (nullable) uint8 [n][>=Lc], 0 => -1e9;
 * o [n][H*dk].  Lc <= 256.
 * pos (nullable) = DEVICE-side step counter: the caches hold cache_off + *pos keys, and this step's own key / value
 * (row b of knew / vnew, leading dimension ldn) are appended at that row and attended to -- one captured graph then
 * serves every step of the loop (gct_decode_embed / gct_select_token read the same counter, gct_decode_advance
 * increments it at the end of the step).  With pos == NULL the first Lc cached keys are used as they are.
 * klen (nullable, only with pos == NULL): per-sample number of leading keys to look at -- for a key-padding mask
 * whose visible keys are a non-empty prefix, the masked rows behind it weigh exactly 0 and are not read.  The kernel
 * looks at min(klen[b], Lc) keys (as gct_attn_decode_z does): a klen above Lc reads nothing behind the Lc rows.
 * row_off (nullable, only with pos): int32 [n], per-row position offset of a batch of prefixes of different lengths
 * that share one device counter -- row b's position is *pos - row_off[b] (>= 0): the caches of row b hold
 * cache_off + *pos - row_off[b] keys and this step's key is appended there.  gct_decode_embed and gct_select_token
 * take the same offsets (csrc/decode_rows.h is the one statement of where a row of a step sits, for every kernel
 * that takes row_off / item / prefix_len).  NULL: every row is at *pos (the kernel of ABI 16). */
int gct_attn_decode(const float* q, int64_t ldq, float* k, float* v, int64_t kv_row,
                    int64_t kv_batch, const uint8_t* valid, int64_t valid_sb, float* o, int64_t ldo,
                    int n, int H, int Lc, int dk, float scale, const int32_t* pos, int cache_off,
                    const float* knew, const float* vnew, int64_t ldn, const int32_t* klen,
                    const int32_t* row_off, void* stream);
/* gct_attn_decode_z: the cross-attention of a decode step (Model/layers.py:73-76 attn_2 over e_outputs = fc_z(z),
 * Model/vaetf.py:75-95) computed over the LATENT rows themselves.  k_{j,h} = G_h z_j + c_h and v_{j,h} = H_h z_j + d_h
 * with G_h = W_k,h W_z, H_h = W_v,h W_z, so score_{j,h} = (G_h^T q_h) . z_j + (a term equal for all keys of the row)
 * and sum_j p_j v_{j,h} = H_h sum_j p_j z_j + d_h: the caller folds G_h^T into the query projection and H_h into the
 * output projection once per sequence, and a step reads lat floats per key instead of 2 * d_model.
 *   q    [n][ldq]: columns [qoff, qoff + H*lat) hold q'_h = G_h^T q_h; columns [0, H*dk) the plain q (read only if nc > 0)
 *   z    row j of sample b at z + b*z_batch + j*lat, Le rows (lat % 4 == 0, lat <= 128, Le <= 256)
 *   ckv  (nc > 0: cond2lat memory, Model/cvaetf.py:86-96) the nc leading keys that are not functions of z: row j of
 *        sample b at ckv + b*ckv_batch + j*ld_ckv holds k'_j = k_j - c (H*dk floats) then v'_j = v_j - d (H*dk floats)
 *   valid (nullable) uint8 [n][>= nc + Le], 0 => -1e9 (condition rows first); klen (nullable) as in gct_attn_decode
 *   out  [n][ldo]: columns [ooff, ooff + H*lat) = sum_j p_j z_j per head; columns [0, H*dk) = sum_{j < nc} p_j v'_j
 *        (written only if nc > 0). */
int gct_attn_decode_z(const float* q, int64_t ldq, int qoff, const float* z, int64_t z_batch, int lat, int Le,
                      const float* ckv, int64_t ckv_batch, int64_t ld_ckv, int nc, const uint8_t* valid,
                      int64_t valid_sb, const int32_t* klen, float* out, int64_t ldo, int ooff, int n, int H, int dk,
                      float scale, void* stream);
/* x[b] = table[ys[b][p]] * scale + pe[pe_off + p] with p = *pos - (row_off ? row_off[b] : 0) (Embeddings +
 * PositionalEncoding of one position, eval mode; row_off as in gct_attn_decode).  An id outside [0, vocab) is clamped
 * into it (below 0: row 0, vocab and above: row vocab - 1); one multiply and one add (or one fma) per element; out is
 * [n][d] contiguous, d % 4 == 0.  gct_decode_advance: *pos += 1. */
int gct_decode_embed(const int64_t* ys, int64_t ld_ys, const int32_t* pos, int pe_off, const float* table,
                     int vocab, const float* pe, float* out, int n, int d, float scale, const int32_t* row_off,
                     void* stream);
int gct_decode_advance(int32_t* pos, void* stream);
/* softmax(logits[n][V]) then mode 0: argmax (first maximum, torch.max semantics) / mode 1:
 * multinomial (Philox inverse-CDF).  Writes ys[row*ld_ys + pos], valid[row*valid_sb + valid_off + pos] =
 * (token != pad), done[row] |= (token == eos); probs_out (nullable) [n][V].  pos_dev (nullable): pos = *pos_dev + 1;
 * seed_dev (nullable): the multinomial seed is read from device memory (graph replays with a fresh seed).
 * row_off (nullable, only with pos_dev; as in gct_attn_decode): row r writes at pos = *pos_dev - row_off[r] + 1, and
 * its multinomial draw is keyed by (r, that pos).
 * The multinomial draw of row r at token position pos (plain and filtered alike):
 *   x = the FIRST word of Philox4x32-10 at the counter (key, pos, 0x452821E6, 0x38D01377), key = r (or item_base + item,
 *       below), under the key of (seed, site 0xDEC0DE): (seed_lo, seed_hi ^ (0xDEC0DE * 0x9E3779B9 + 0x7F4A7C15));
 *   u = (float32(x >> 8) + 0.5f) * 2^-24, evaluated in fp32.  The addition rounds to even once x >> 8 >= 2^23, so u lies
 *       in (0, 1] -- x >> 8 = 2^24 - 1 gives exactly 1.0 -- not in (0, 1);
 *   the pick is the first token c with w_c > 0 whose inclusive cumulative sum of w / sum w exceeds u (fp32 sums, 64
 *       tokens per wave scan, carried from chunk to chunk); when no sum exceeds u (rounding, or u = 1), the last token
 *       of nonzero weight.  A token of weight 0 (a logit of -inf, or one the nucleus dropped) is never picked.
 * filt (nullable, DEVICE memory, mode 1 only): sampling filter between the softmax and the draw (gct_plus_amd/decode.py
 * sample_filter_reference states the rules), read by the kernel so that one captured graph serves any settings:
 *   p = softmax(x * inv_temp) in fp32;
 *   top-k: token c is in when fewer than k tokens have a strictly larger LOGIT (ties at the k-th value stay in); an out
 *     token gets the weight 1e-6 (the reference's floor); k >= V: no-op;
 *   nucleus: with s = w / sum w, token c is kept when the mass of the tokens with a strictly larger s is < top_p,
 *     otherwise its weight is 0; top_p >= 1: no-op;
 *   the draw picks c with probability w_c / sum w (the same Philox key); probs_out receives w / sum w.  A row the filter
 *   leaves unchanged draws exactly as without filt.  The host validates 1 <= k <= V, 0 < top_p <= 1, 0 < T < inf.
 * V <= GCT_SAMPLE_FILTER_MAX_VOCAB with filt; otherwise (or with mode 0) GCT_ERR_ARG.  NULL: the kernels of ABI 17.
 * item / prefix_len (both or neither; with row_off, valid and done): continuous batching (gct_stream_refill) -- row r
 * decodes pool item item[r] (int32 [n]; < 0: parked, the row writes nothing).  While pos < prefix_len[item] the slot
 * already holds the prefix token the refill laid there and is left alone (done untouched); the multinomial draw is
 * keyed by (item_base + item, pos) instead of (r, pos), in every mode (item_base >= 0: the pool is a slice of a larger
 * one).  NULL: the kernels of ABI 19. */
typedef struct GctSampleFilter {
  int32_t k;        /* top-k (>= V: off) */
  float top_p;      /* nucleus mass (>= 1: off) */
  float inv_temp;   /* 1 / temperature */
  int32_t reserved; /* 0 */
} GctSampleFilter;
#define GCT_SAMPLE_FILTER_MAX_VOCAB 1024
int gct_select_token(const float* logits, int V, int64_t* ys, int64_t ld_ys, int pos, uint8_t* valid,
                     int64_t valid_sb, uint8_t* done, float* probs_out, int n, int mode,
                     int64_t pad_id, int64_t eos_id, uint64_t seed, const int32_t* pos_dev, int valid_off,
                     const uint64_t* seed_dev, const int32_t* row_off, const GctSampleFilter* filt,
                     const int32_t* item, const int32_t* prefix_len, int item_base, void* stream);

/* Grammar-constrained decoding (gct_plus_amd/decode.py SmilesGrammar states the grammar and is the reference): launched in
 * front of gct_select_token in the step unit, on the same device counter.  One wave per row, no state of its own: row r
 * is about to choose column p = *pos + 1 - row_off[r] (row_off nullable); its generated tokens are ys[r][t0_r, p), with
 *   t0_r = gram[1] - row_off[r] and the budget G = gram[0]      (gram: int32 [2] in DEVICE memory, so that a captured
 *                                                                 graph serves any max_strlen and prefix width), or
 *   t0_r = prefix_len[item[r]] and G = limit[item[r]]           with item / prefix_len / limit (all three or none, with
 *                                                                 row_off: continuous batching as in gct_select_token).
 * The wave classifies those g = p - t0_r tokens (at most 255: T <= 256) through table (int32 [V]: class | ring number << 8, GCT_GRAMMAR_*), derives
 * the state -- depth = #OPEN - #CLOSE, open = xor of the ring bits, here = open & (or of the ring bits behind the last
 * ATOM), prev from the last two classes -- and writes masked[r][c] = logits[r][c] (bit for bit) when token c is allowed as
 * the row's g-th token under the budget G, -inf otherwise.  A finished row (prev END) and a row past its budget (g >= G)
 * allow <pad> only.  Nothing is written for a parked row (item < 0), a row inside its prefix (g < 0) or p >= T.
 * logits / masked [n][V] contiguous, distinct; ys [n][ld_ys], T <= 256 columns in use; any V >= 1. */
#define GCT_GRAMMAR_ATOM 0
#define GCT_GRAMMAR_BOND 1
#define GCT_GRAMMAR_OPEN 2
#define GCT_GRAMMAR_CLOSE 3
#define GCT_GRAMMAR_RING 4
#define GCT_GRAMMAR_DOT 5
#define GCT_GRAMMAR_EOS 6
#define GCT_GRAMMAR_PAD 7
#define GCT_GRAMMAR_BANNED 8
#define GCT_GRAMMAR_MAX_RINGS 64
int gct_grammar_mask(const float* logits, float* masked, int V, const int32_t* table, const int64_t* ys, int64_t ld_ys,
                     int T, int n, const int32_t* pos, const int32_t* row_off, const int32_t* gram, const int32_t* item,
                     const int32_t* prefix_len, const int32_t* limit, void* stream);

/* Chemical validity of FINISHED rows (gct_plus_amd/decode.py SmilesChemistry.check states the rules and is the reference):
 * one wave per row, nothing to do with the decode loop.  Row r's span is ys[r][start[r], W) -- its generated tokens, the
 * <eos> and whatever follows it included; nothing outside the span is read.  W - start[r] <= 256 and 0 <= start[r] <= W
 * (a row outside that range is reported as SYNTAX at position 0).  table: the grammar's (int32 [V], as above).
 * chem: int32 [V], one word per token:
 *   bits 0..3    the atom's valence cap, GCT_CHEM_NO_CAP (15) for none and for every token that is no atom
 *   bits 4..7    the atom's explicit hydrogen count
 *   bit  8       the atom is aromatic          bit 9   the atom is carbon-like (its effective element is C)
 *   bits 12..14  the order of a BOND token (1 .. 4), 0 for every other token
 * out [n][4] int32 = (status, position, atoms, ring_bonds), all four written for every row:
 *   SYNTAX     the span is not well formed (an id outside [0, V) and an empty span included); position = the first token
 *              without a transition, or the span's length when no <eos> was reached; atoms = ring_bonds = 0
 *   RING_BOND  a ring closure whose two ends state different orders, or that doubles an existing bond (no bond is added)
 *   VALENCE    an atom whose bond orders + explicit H (+ 1 for an aromatic carbon-like atom without a double bond) exceed
 *              its cap;   AROMATIC  an aromatic atom with fewer than two aromatic neighbours
 *   the finding at the smallest position wins (position = its token's index in the span); OK has position -1.
 *   atoms = ATOM tokens, ring_bonds = closing ring tokens (rejected ones included).
 * n = 0 is a no-op.  No global atomics; the walk's stack and the per-atom sums live in LDS. */
#define GCT_CHEM_OK 0
#define GCT_CHEM_SYNTAX 1
#define GCT_CHEM_VALENCE 2
#define GCT_CHEM_RING_BOND 3
#define GCT_CHEM_AROMATIC 4
#define GCT_CHEM_NO_CAP 15
int gct_smiles_check(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V, const int32_t* table,
                     const int32_t* chem, int32_t* out, void* stream);

/* SMILES randomisation (gct_plus_amd/randomize.py SmilesRandomizer states the rules: `randomize` for one part,
 * randomize_reference for a batch): row r's span ys[r][start[r], W) written out again as a random depth-first spelling
 * of the same molecular graph, one wave per row.  The content is what stands in front of the span's first <eos>; with
 * sep_id >= 0 and a <sep> in it, the scaffold in front of the first <sep> (part 1) and the molecule behind it (part 0)
 * are handled on their own.  A span without <eos>, W - start[r] > 256 or start[r] outside [0, W]: the row's W columns
 * are copied, info = (SYNTAX, -1, span length or 0, 0).
 * table: int32 [V], class | ring number << 8 (as the grammar's) | the order of a BOND token << 16 | unsupported << 20
 * (a / or \ bond, an atom token with @).  ring_ids: int32 [64], the token ids of the n_rings <= 63 ring numbers the
 * spelling may use, lowest first.  key: int64 [n], the row's stream; seed, p: by value, 0 <= p <= 1.
 * out int64 [n][out_width], out_width >= W: columns [0, start) copied, the parts with <sep> between them, <eos>, <pad>.
 * info int32 [n][4] = (status of the molecule, status of the scaffold or -1, new span length with <eos>, atoms).
 * perm int32 [n][out_width] or NULL: the input atom index of the k-th output atom, -1 behind them.
 * A part that is not randomised keeps its tokens; its status says why (OK: it was randomised).
 * n = 0 is a no-op.  No global atomics, no scratch: the graph, the search stack and the new row live in LDS. */
#define GCT_RAND_OK 0
#define GCT_RAND_KEPT 1
#define GCT_RAND_SYNTAX 2
#define GCT_RAND_UNSUPPORTED 3
#define GCT_RAND_NO_RING 4
#define GCT_RAND_TOO_LONG 5
int gct_smiles_randomize(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, const int64_t* key, int V,
                         const int32_t* table, const int32_t* ring_ids, int n_rings, int open_id, int close_id,
                         int pad_id, int eos_id, int sep_id, uint64_t seed, float p, int64_t* out, int32_t* info,
                         int32_t* perm, int out_width, void* stream);

/* Molecule identity keys (gct_plus_amd/molkey.py SmilesKeys states the rules: `key` for one part, key_reference for a
 * batch): a spelling-independent 64-bit key of the labelled graph that gct_smiles_randomize's parse reads from row r's
 * span ys[r][start[r], W), one wave per row.  Spans, <eos>, <sep> and the two parts: as in gct_smiles_randomize.
 * table32: int32 [V], gct_smiles_randomize's word | from bit 21 the key's label of a BOND token (- 1, = 2, # 3, $ 4,
 * : 5, ~ 6) or `aromatic` of an ATOM token.  label64: int64 [V], the FNV-1a hash of every token's string.
 * A part with a graph (status GRAPH): per atom a distance profile over its breadth-first search, GCT_KEY_ROUNDS rounds
 * of bond-labelled refinement, a wrapping sum over the atoms.  A part without one -- it does not parse (STRING_SYNTAX) or
 * the randomiser would report UNSUPPORTED (STRING_UNSUPPORTED) -- gets an order-dependent hash of its tokens' labels.
 * key_out int64 [n][2] = (the molecule's key, the scaffold's or 0); info_out int32 [n][4] = (status of the molecule,
 * status of the scaffold or -1, atoms, bonds of the molecule part).  A span without <eos>, W - start[r] > 256 or
 * start[r] outside [0, W]: keys 0, info (-1, -1, 0, 0).  n = 0 is a no-op.  No global atomics, no scratch. */
#define GCT_KEY_GRAPH 0
#define GCT_KEY_STRING_SYNTAX 1
#define GCT_KEY_STRING_UNSUPPORTED 2
#define GCT_KEY_ROUNDS 3
int gct_smiles_key(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V, const int32_t* table32,
                   const int64_t* label64, int pad_id, int eos_id, int sep_id, int64_t* key_out, int32_t* info_out,
                   void* stream);

/* Murcko scaffolds (gct_plus_amd/scaffold.py SmilesScaffolds states the rules: `scaffold` for one part,
 * scaffold_reference for a batch): the ring systems and linkers of the molecule in row r's span ys[r][start[r], W), with
 * what is double-bonded to them, as a key and as a spelling; one wave per row.  Spans, <eos>, <sep>, table32 and label64:
 * as in gct_smiles_key; ring_ids, n_rings, open_id, close_id: as in gct_smiles_randomize.  The molecule is the part
 * behind the first <sep>, or the whole content; the part in front of the <sep> is the scaffold the row was GIVEN and is
 * keyed by gct_smiles_key's rule.  n_id / nh_id: the ids of the tokens `n` and `[nH]`, -1 for none -- a kept `n` that
 * loses a neighbour is spelled and keyed as `[nH]` (NO_TOKEN without one).
 * tokens_out int64 [n][out_width], out_width >= 1: the spelling (the kept atoms and the bonds between them, written out
 * by the randomiser's walk from the lowest kept atom over the lists in parse order), <eos>, <pad>; a spelling that does
 * not fit min(out_width, 256) - 1 tokens is TOO_LONG.  key_out int64 [n][2] = (key of the extracted scaffold, key of the
 * given part or 0).  info_out int32 [n][4] = (status, GCT_KEY_* status of the given part or -1, atoms kept, length of the
 * spelling).  member_out int32 [n][W]: per atom of the molecule, in order, 0 dropped, 1 core, 2 shell; -1 behind them.
 * ACYCLIC (no ring), SYNTAX and UNSUPPORTED (as the randomiser's): key 0, empty spelling, 0 atoms kept, and for the
 * last two no member entry either.  NO_TOKEN: key 0, empty spelling.  NO_RING, TOO_LONG: empty spelling.  A span without
 * <eos>, W - start[r] > 256 or start[r] outside [0, W]: <pad> tokens, keys 0, info (-1, -1, 0, 0), member -1.
 * n = 0 is a no-op.  No global atomics, no scratch. */
#define GCT_SCA_OK 0
#define GCT_SCA_ACYCLIC 1
#define GCT_SCA_SYNTAX 2
#define GCT_SCA_UNSUPPORTED 3
#define GCT_SCA_NO_TOKEN 4
#define GCT_SCA_NO_RING 5
#define GCT_SCA_TOO_LONG 6
int gct_smiles_scaffold(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                        const int32_t* table32, const int64_t* label64, const int32_t* ring_ids, int n_rings, int open_id,
                        int close_id, int pad_id, int eos_id, int sep_id, int n_id, int nh_id, int64_t* tokens_out,
                        int out_width, int64_t* key_out, int32_t* info_out, int32_t* member_out, void* stream);

/* Circular fingerprints (gct_plus_amd/fingerprint.py SmilesFingerprints states the rules: `fingerprint` for one part,
 * fp_reference for a batch): GCT_FP_BITS bits of the labelled graph that gct_smiles_randomize's parse reads from row r's
 * span ys[r][start[r], W), one wave per row.  Spans, <eos>, <sep>, table32 and label64: as in gct_smiles_key; with a
 * <sep> the molecule behind it is fingerprinted, the part in front of it is not.
 * A part with a graph (status GRAPH): id_0(a) = mix(label(a) ^ mix(0x200 + bonds of a)), GCT_FP_RADIUS rounds of
 * gct_smiles_key's bond-labelled refinement, and for every round 0 .. GCT_FP_RADIUS and atom the bit id mod GCT_FP_BITS.
 * A part without one -- it does not parse (SYNTAX) or the randomiser would report UNSUPPORTED -- has no bit set.
 * bits_out int64 [n][GCT_FP_BITS / 64]: word w holds bits 64 w .. 64 w + 63, bit k at 1 << (k & 63).  info_out int32
 * [n][4] = (status, number of bits set, atoms, bonds).  A span without <eos>, W - start[r] > 256 or start[r] outside
 * [0, W]: no bit, info (-1, 0, 0, 0).  n = 0 is a no-op.  No global atomics, no scratch. */
#define GCT_FP_GRAPH 0
#define GCT_FP_SYNTAX 1
#define GCT_FP_UNSUPPORTED 2
#define GCT_FP_RADIUS 2
#define GCT_FP_BITS 1024
int gct_smiles_fp(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V, const int32_t* table32,
                  const int64_t* label64, int pad_id, int eos_id, int sep_id, int64_t* bits_out, int32_t* info_out,
                  void* stream);

/* Molecular descriptors (gct_plus_amd/descriptor.py SmilesDescriptors states the rules: `describe` for one part,
 * desc_reference for a batch): twelve integers of the labelled graph that gct_smiles_randomize's parse reads from row r's
 * span ys[r][start[r], W), one wave per row.  Spans, <eos>, <sep> and table32: as in gct_smiles_key (the bond symbol's
 * label from bit 21); with a <sep> the molecule behind it is described, the part in front of it is not.
 * desc32: int32 [V], the reading of every ATOM token's string (0 for any other token):
 *   bits 0..3    element index + 1 over B C N O F Si P S Cl Br I; 0: UNKNOWN (another element, `*`, an element H atom, a
 *                stated isotope, an unreadable bracket, a charge outside -3 .. 3)
 *   bit 4        aromatic (a lower-case symbol)
 *   bit 5        bracket atom: its hydrogens are exactly the stated ones; a bare atom gets implicit hydrogens
 *   bits 6..9    stated hydrogens (0 .. 9)
 *   bits 10..12  formal charge + 3
 * Ring perception: one breadth-first search per bond from one end with the bond excluded gives s(e), the smallest ring
 * through the bond (0: no ring bond).  A bond without a symbol between two aromatic atoms is AROMATIC only as a ring bond.
 * values_out int32 [n][GCT_DESC_COLUMNS] = (status, heavy atoms, hydrogens, molecular weight in mDa, formal charge,
 * N/O atoms with a hydrogen, N and O atoms, rotatable bonds, rings = bonds - atoms + 1, aromatic rings, TPSA in 0.01 A^2
 * by Ertl's N and O contributions, ring bonds).  Where the status is not OK, columns 2 .. 11 are 0 and column 1 is the
 * number of atoms of a parsed graph (UNSUPPORTED, UNKNOWN_ATOM), else 0.  A span without <eos>, W - start[r] > 256 or
 * start[r] outside [0, W]: (-1, 0, ..., 0).  Every row's twelve words are written.  n = 0 is a no-op.  No global
 * atomics, no scratch. */
#define GCT_DESC_OK 0
#define GCT_DESC_SYNTAX 1
#define GCT_DESC_UNSUPPORTED 2
#define GCT_DESC_UNKNOWN_ATOM 3
#define GCT_DESC_COLUMNS 12
int gct_smiles_desc(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V, const int32_t* table32,
                    const int32_t* desc32, int pad_id, int eos_id, int sep_id, int32_t* values_out, void* stream);

/* Tanimoto aggregates of every row of a against all rows of b (fingerprint.py tanimoto_reference states the rule).
 * a int64 [n][lda >= 16], b int64 [m][ldb >= 16]: gct_smiles_fp's words; cnt_a int32 [n], cnt_b int32 [m]: their
 * numbers of set bits (0: the row is absent).  For a pair, c = popcount(a_i & b_j), u = cnt_a[i] + cnt_b[j] - c and
 * T = (float)c / (float)u, correctly rounded.  Per row i of a, over the present rows j of b:
 *   best_out float [n]    the largest T, decided by integer cross-multiplication (exact);
 *   arg_out int32 [n]     the LOWEST j that attains it;
 *   total_out double [n]  the sum of T (p = 1) or of the fp64 product T * T (p = 2), every term exact in fp64.
 * An absent row of a, and every row when no row of b is present (m = 0 included): (0, -1, 0).
 * The grid is (tiles of 256 rows of a) x gct_fp_tanimoto_splits(n, m) splits of b in tiles of gct_fp_tanimoto_tile_b()
 * rows; with more than one split, ws (8-byte aligned, ws_bytes >= gct_fp_tanimoto_ws_bytes(n, m); otherwise it may be
 * NULL) takes the partials and a second launch folds them in split order.  The split count is a function of (n, m)
 * alone, so the bits of total_out do not depend on the device.  m <= 2^30.  n = 0 is a no-op.  No atomics. */
int gct_fp_tanimoto_tile_b(void);
int gct_fp_tanimoto_splits(int n, int m);
int64_t gct_fp_tanimoto_ws_bytes(int n, int m);
int gct_fp_tanimoto(const int64_t* a, int64_t lda, const int32_t* cnt_a, int n, const int64_t* b, int64_t ldb,
                    const int32_t* cnt_b, int m, int p, void* ws, int64_t ws_bytes, float* best_out, int32_t* arg_out,
                    double* total_out, void* stream);

/* Per-step sampling statistics (gct_plus_amd/decode.py step_stats_reference states the rules).  Launched behind
 * gct_select_token in the step unit, on the same device counter and with gct_chosen_logp's row rule: row r looks at
 * column p = *pos - row_off[r] + 1, takes tok = ys[r][p] and writes each non-null table at out[dst][p].
 *   pi  the softmax of the RAW logits row (temperature 1), its log-softmax with gct_chosen_logp's arithmetic;
 *   q   the BEHAVIOUR distribution the token was drawn from: the probs row [n][V] gct_select_token wrote to probs_out in
 *       this step, as given; pi itself when probs is null; the one-hot at tok when greedy != 0 (probs is ignored).
 *   model_entropy = -sum pi log pi           behaviour_logp = log q(tok)
 *   behaviour_entropy = -sum_{q>0} q log q    behaviour_kl = sum_{q>0} q (log q - log pi)
 * A term with q == 0 adds exactly 0.  tok == pad_id (a finished row): all four are 0.  probs null and not greedy:
 * behaviour_logp has gct_chosen_logp's bits, behaviour_entropy model_entropy's, behaviour_kl is exactly 0.
 * item / prefix_len / row_off, dst and the cases in which nothing is written: as in gct_chosen_logp (so the call goes
 * BEFORE gct_stream_refill).  The four tables are [out_rows][ld_out], each nullable, at least one given.  One wave per
 * row; any V >= 1.  n == 0 launches nothing. */
int gct_step_stats(const float* logits, const float* probs, int V, const int64_t* ys, int64_t ld_ys, const int32_t* pos,
                   const int32_t* row_off, const int32_t* item, const int32_t* prefix_len, int64_t pad_id, int greedy,
                   float* model_entropy, float* behaviour_logp, float* behaviour_entropy, float* behaviour_kl,
                   int64_t ld_out, int out_rows, int n, void* stream);

/* Continuous batching (gct_plus_amd/decode.py stream_schedule_reference states the schedule).  R decode rows work
 * through a pool of N items behind the shared counter *pos: the step unit is gct_decode_advance, the RAGGED step
 * kernels, gct_select_token(item, prefix_len) and then gct_stream_refill, which, when *enable != 0:
 *   1. finds the rows that FINISHED in the step just run: done[r] set, or the item has produced limit[item] tokens
 *      (generated so far = *pos - row_off[r] + 2 - prefix_len[item]; a row still inside its prefix, generated <= 0, is
 *      not finished, whatever done[r] says); copies ys[r][0, width) to out_ys[item] and the generated length to
 *      out_len[item]; *n_harvested += their number;
 *   2. gives the finished rows and the empty ones (item[r] < 0 or >= items) the items *next_item, *next_item + 1, ...
 *      in ASCENDING ROW ORDER (*next_item stops at items); a row that finds the pool empty gets item -1 (parked).
 *      row_of[item] = r, start_step[item] = *pos + 1;
 *   3. lays out each such row: row_off[r] = *pos + 1 (the next step consumes the row's token 0); with a new item
 *      z3 / src_valid / src_klen / ckv rows from the pools, ys[r][0, T) = the item's prefix then pad, valid[r] = the
 *      prefix's non-pad flags, done[r] = 0.  A parked row gets the offset only, at every call: it stays at position 0.
 * Every item, the first R included, enters through this call (set item[] = -1, *pos = -1 and call it once before the
 * first step).  With *enable == 0 nothing is read or written beyond the word itself (capture warm-ups and timing probes
 * run real steps whose state the host restores).  All fields are 8 bytes wide (pointers and int64_t), in this order. */
#define GCT_STREAM_MAX_ROWS 8192
#define GCT_STREAM_MAX_LAYERS 16
typedef struct GctStreamState {
  /* the decoder's rows */
  int64_t* ys;           /* [rows][ld_ys] */
  uint8_t* valid;        /* [rows][valid_sb], token j at valid_off + j */
  uint8_t* done;         /* [rows] */
  int32_t* row_off;      /* [rows] */
  const int32_t* pos;    /* the shared counter */
  float* z3;             /* [rows][z_row] latent rows */
  uint8_t* src_valid;    /* [rows][Lk] */
  int32_t* src_klen;     /* [rows] */
  float* ckv[GCT_STREAM_MAX_LAYERS];            /* per layer [rows][ckv_row] condition keys | values (ckv_row > 0) */
  int32_t* item;         /* [rows] pool item of the row, -1: none */
  int32_t* harvest;      /* [rows] scratch: item harvested in this call, -1: none */
  uint8_t* fresh;        /* [rows] scratch: the row is laid out again in this call */
  /* the pool */
  const float* z_pool;   /* [items][z_row] */
  const uint8_t* valid_pool;                    /* [items][Lk] */
  const int32_t* klen_pool;                     /* [items] */
  const float* ckv_pool[GCT_STREAM_MAX_LAYERS]; /* per layer [items][ckv_row] */
  const int64_t* prefix_pool;                   /* [items][t0_max], right-padded */
  const int32_t* prefix_len;                    /* [items], 1 .. t0_max */
  const int32_t* limit;                         /* [items] tokens to generate at most, >= 1, prefix_len + limit <= width */
  /* results */
  int64_t* out_ys;       /* [items][width] */
  int32_t* out_len;      /* [items] generated tokens, the <eos> included */
  int32_t* row_of;       /* [items] */
  int32_t* start_step;   /* [items] */
  int32_t* next_item;    /* first item not handed out yet */
  int32_t* n_harvested;  /* items copied out so far */
  const int32_t* enable;
  /* geometry */
  int64_t rows, items, ld_ys, valid_sb, valid_off, T, width, t0_max, z_row, Lk, ckv_row, layers, pad_id;
} GctStreamState;
/* state: HOST memory, read during the call (the kernels get a copy).  1 <= rows <= GCT_STREAM_MAX_ROWS,
 * width <= T <= ld_ys, valid_off + T <= valid_sb, z_row % 4 == 0, ckv_row % 4 == 0, layers <= GCT_STREAM_MAX_LAYERS;
 * otherwise GCT_ERR_ARG.  Two launches: a one-workgroup scan over the rows, then one workgroup per row for the copies. */
int gct_stream_refill(const GctStreamState* state, void* stream);

/* Beam search (gct_plus_amd/decode.py beam_step_reference states the rules).  Sample s owns the k rows
 * s*k .. s*k+k-1 of an n*k-row decode.  The self-attention caches, ys and valid are PHYSICAL slots, each written once:
 * row r writes cache slot cache_off + p in the step that consumes token p, and ys[r][p] / valid[r][cache_off + p] when
 * that token is chosen.  kv_src int32 [n*k][ld_src] maps beam r's logical position j to the physical row kv_src[r][j].
 * gct_attn_decode_beam: the device-position form of gct_attn_decode (pos required, no klen) where key / value j of row
 *   b and valid[.][j] are read from row kv_src[b][j] (clamped to [0, n)); this step's key / value are appended to row b.
 *   T = cache rows (<= 256, <= ld_src).  When the caches are full (cache_off + *pos >= T: no room for this step's key)
 *   the call writes nothing: o and both caches stay as they are.
 * gct_beam_select: one workgroup per sample; p = *pos_dev + 1.  Candidates: live beam b offers scores[b] + logp_b(v)
 *   for every token v (logp = fp32 log-softmax of logits row b, x - m - log sum exp(x - m)); a finished beam offers
 *   itself once, token pad_id, score unchanged; a beam at -inf offers nothing.  The k best by score, ties to the lower
 *   beam * V + token, become the children in order: scores / finished (parent's or token == eos_id) / lengths (parent's
 *   + 1 while the parent was live) / parent (nullable, int32 [n*k]) per row; ys[row][p] = token,
 *   valid[row][valid_off + p] = token != pad_id; kv_src[row][0, T) = the parent's row before this call, with entry
 *   valid_off + p = row; done[s] = all k children finished.  1 <= k <= GCT_BEAM_MAX_K, k <= V <= GCT_BEAM_MAX_VOCAB,
 *   0 <= pad_id < V, T <= 256, ld_src >= T, valid_sb >= T, ld_ys >= T - valid_off; otherwise GCT_ERR_ARG. */
#define GCT_BEAM_MAX_K 16
#define GCT_BEAM_MAX_VOCAB 65536
int gct_attn_decode_beam(const float* q, int64_t ldq, float* k, float* v, int64_t kv_row, int64_t kv_batch,
                         const uint8_t* valid, int64_t valid_sb, float* o, int64_t ldo, int n, int H, int T, int dk,
                         float scale, const int32_t* pos, int cache_off, const float* knew, const float* vnew,
                         int64_t ldn, const int32_t* kv_src, int64_t ld_src, void* stream);
int gct_beam_select(const float* logits, int V, int n, int k, float* scores, uint8_t* finished, int32_t* lengths,
                    int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid, int64_t valid_sb, int valid_off,
                    int32_t* kv_src, int64_t ld_src, int T, uint8_t* done, const int32_t* pos_dev, int64_t pad_id,
                    int64_t eos_id, void* stream);

/* Stochastic beam search (ABI 31; Kool, van Hoof and Welling, ICML 2019; gct_plus_amd/decode.py sbs_step_reference
 * states the rules): beam search over Gumbel-perturbed log-probabilities, whose k beams are a sample WITHOUT replacement
 * from the sequence distribution.  gct_beam_select_gumbel is gct_beam_select -- the same arguments, limits, error checks
 * and write-back, one kernel template -- with one more float of state per row, gumbels [n*k] (in place; after the
 * prefill [0, -inf, ...] like scores), and another ordering value:
 *   a live beam b (finite scores[b]) offers every token v with finite phi_bv = scores[b] + logp_b(v) (gct_beam_select's
 *     fp32 log-softmax); g_bv = phi_bv + noise_bv; Z_b = max_v g_bv over the offered tokens, v*_b its first argmax;
 *   the candidate's value is g~_bv = -log(exp(-G_b) - exp(-Z_b) + exp(-g_bv)), G_b = gumbels[b], evaluated in fp32 as
 *     d = min(g - Z, 0); l = log(1 - exp(d)) (log(-expm1(d)) for d > -ln 2, log1p(-exp(d)) otherwise); w = G - g + l;
 *     g~ = G - max(w, 0) - log1p(exp(-|w|));  token v*_b gets g~ = G_b exactly, BY ITS INDEX;
 *   a token with phi = -inf is not offered; a finished beam offers itself once, token pad_id, score and Gumbel value
 *     unchanged; a beam at -inf offers nothing;
 *   the k candidates of largest g~, ties to the lower beam * V + token, become the children in that order: scores = phi,
 *     gumbels = g~, everything else as gct_beam_select writes it.  A slot c for which no candidate is left (fewer than k
 *     offered) becomes a finished beam at -inf: parent c, token pad_id, scores = gumbels = -inf.
 * The draw: noise_bv of the PHYSICAL row r = s*k + b at token position p = *pos_dev + 1 (a child's noise therefore
 * depends on the slot its parent sits in, which changes no distribution: the variates of distinct (row, p, v) are
 * independent) is word v & 3 of Philox4x32-10 at the counter (r, p, v >> 2, GCT_SBS_C3) -- one call serves four tokens --
 * under the key of (seed, site GCT_SBS_SITE): (seed_lo, seed_hi ^ (GCT_SBS_SITE * 0x9E3779B9 + 0x7F4A7C15));
 *   u = (float32(x >> 9) + 0.5f) * 2^-23: exact in fp32 (23 bits and a half), strictly inside (0, 1);
 *   noise = -logf(-logf(u)).
 * seed_dev (nullable, DEVICE memory) replaces seed, so that one captured graph serves every seed (as gct_select_token).
 * noise_in (nullable, [n*k][V]): these variates are used instead of the draw.  noise_out (nullable, [n*k][V]): receives
 * the variates used for the rows of live beams (all V of them); rows of other beams are not written.
 * gumbels NULL, or anything gct_beam_select refuses: GCT_ERR_ARG. */
#define GCT_SBS_SITE 0x5B5BEAu
#define GCT_SBS_C3 0xBE5466CFu
int gct_beam_select_gumbel(const float* logits, int V, int n, int k, float* scores, uint8_t* finished, int32_t* lengths,
                           int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid, int64_t valid_sb, int valid_off,
                           int32_t* kv_src, int64_t ld_src, int T, uint8_t* done, const int32_t* pos_dev, int64_t pad_id,
                           int64_t eos_id, float* gumbels, uint64_t seed, const uint64_t* seed_dev,
                           const float* noise_in, float* noise_out, void* stream);

/* Sequential Monte Carlo decoding under the grammar (Lew et al. 2023; Loula et al. 2025; gct_plus_amd/decode.py
 * smc_step_reference states the rules).  Sample s owns the k PARTICLE rows s*k .. s*k+k-1 of an n*k-row decode, laid out
 * and written back exactly as the beams of gct_beam_select (physical slots, the ancestry map kv_src).  Why the estimate is
 * unbiased: with gamma_t(x_<=t) = pi(x_<=t) 1[the prefix can still finish inside the budget] and the proposal q_t = the
 * masked, renormalised softmax, gamma_t / (gamma_{t-1} q_t) = A_t, the model's mass on the allowed tokens -- a function
 * of the parent alone, so weighting and resampling come BEFORE the draw (the fully adapted particle filter) and
 * E[exp(log_z) * mean weight] = Z = P(well formed within the budget) for every k and every threshold.
 * gct_grammar_mask_anc: gct_grammar_mask for uniform rows (no row_off, no items; one kernel template with it) whose
 *   history is read through the map: generated token j of row r is ys[kv_src[r][valid_off + t0 + j]][t0 + j], t0 =
 *   gram[1] (map entries clamped to [0, n)).  ld_src >= valid_off + T.  With the identity map: gct_grammar_mask's bits.
 * gct_smc_select: one workgroup per sample, p = *pos_dev + 1; logits the RAW rows [n*k][V], masked the rows
 *   gct_grammar_mask_anc wrote (distinct buffers).  State per row: logw (fp32 log-weight since the last resampling), logp
 *   (fp32 log-probability of its tokens under the model), finished, lengths; per sample log_z (fp64) and resamples.
 *   0. every particle finished on entry: nothing but pad tokens and the map's new slot is written (a_c = c).
 *   1. weight: a live particle b gets logw_b += (my - mx) + (log sy - log sx), (mx, sx) / (my, sy) the row maximum and
 *      sum exp(. - max) of its raw / masked row (gct_select_token's softmax statistics, twice); a finished one keeps
 *      logw_b; a masked row without a finite entry gives logw_b = -inf: the particle is DEAD, is never an ancestor, writes
 *      pad and is finished from then on.
 *   2. resample: M = max_b logw_b; M = -inf (all dead): log_z = -inf, a_c = c.  Otherwise w_b = expf(logw_b - M), S1 =
 *      sum w, S2 = sum w * w (fp32, b ascending, no fused multiply-add), ESS = S1 * S1 / S2; resample iff *tau_dev >= 1 or
 *      ESS < *tau_dev * k.  Systematic, ONE uniform u per (s, p): child c takes the first b whose inclusive fp32 running
 *      sum of w exceeds (u + c) * (S1 / k) and has w_b > 0, else the last b with w_b > 0; log_z += M + log(S1 / k) in
 *      fp64, every child's logw = 0, resamples += 1.  Not resampling: a_c = c and the child keeps logw_c.
 *   3. draw: child c of a live parent a draws from softmax(masked row a) with gct_select_token's multinomial draw, bit
 *      for bit: the uniform is the FIRST word of Philox at (s*k + c, p, 0x452821E6, 0x38D01377) under (seed, site 0xDEC0DE)
 *      -- with no resampling the particles are the rows gct_select_token draws for the same masked rows and seed.
 *      logp_c = logp_a + ((x_a[tok] - mx_a) - log sx_a), finished = tok == eos_id, lengths = lengths_a + 1.  A finished
 *      (or dead) parent hands down pad and its state.  u of step 2: the first word at (s, p, the same two constants)
 *      under (seed, site GCT_SMC_SITE), through the same word-to-uniform map.
 *   4. write-back: gct_beam_select's -- ys[row][p], valid[row][valid_off + p], kv_src[row] = the ancestor's row before
 *      the call with entry valid_off + p = row, parent (nullable), done[s] = all k children finished.
 * tau_dev (float) and seed_dev (nullable; replaces seed) live in DEVICE memory: one captured graph serves every threshold
 * and seed.  u_in (nullable, [n][k + 1]): the k draw uniforms and, last, the resampling uniform, instead of the draws;
 * u_out (nullable, [n][k + 1]) receives the k + 1 uniforms of the step, used or not.
 * 1 <= k <= GCT_BEAM_MAX_K, V >= 1 as in gct_select_token, 0 <= pad_id < V, the map / valid / ys bounds of
 * gct_beam_select; a null state pointer, masked == logits or anything out of range: GCT_ERR_ARG. */
#define GCT_SMC_SITE 0x53C0DEu
int gct_grammar_mask_anc(const float* logits, float* masked, int V, const int32_t* table, const int64_t* ys, int64_t ld_ys,
                         int T, int n, const int32_t* pos, const int32_t* gram, const int32_t* kv_src, int64_t ld_src,
                         int valid_off, void* stream);
int gct_smc_select(const float* logits, const float* masked, int V, int n, int k, float* logw, float* logp,
                   uint8_t* finished, int32_t* lengths, int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid,
                   int64_t valid_sb, int valid_off, int32_t* kv_src, int64_t ld_src, int T, uint8_t* done,
                   const int32_t* pos_dev, int64_t pad_id, int64_t eos_id, double* log_z, int32_t* resamples,
                   const float* tau_dev, uint64_t seed, const uint64_t* seed_dev, const float* u_in, float* u_out,
                   void* stream);

/* ------------------------------------------------ host side: SMILES tokeniser + collate */
/* Utils/field.py:8-33 moltokenize (the atom-wise regex, findall semantics) as a scanner.
 * Returns the number of tokens (may exceed max_tokens: call again with a larger buffer). */
int gct_smiles_tokenize(const char* smi, int with_sep, int32_t* tok_start, int32_t* tok_len,
                        int max_tokens);
/* torchtext Field.process as used by Model/collate_fn.py:5-15,104-124: row r of out[n][width] =
 * [sos] ids(tokens) [eos] pad...; vocab[id] are the token strings, unknown -> unk_id; sos/eos < 0
 * omit them (SRC field).  Returns the longest row length, <0 on error (row does not fit). */
int gct_smiles_encode_batch(const char* const* smiles, int n, int with_sep, const char* const* vocab,
                            int vocab_size, int64_t unk_id, int64_t pad_id, int64_t sos_id,
                            int64_t eos_id, int64_t* out, int64_t width, int32_t* lengths);

/* ------------------------------------------------------------------ utilities */
/* dst[(r / rpb)*dst_rpb + dst_off + r % rpb][:] (op)= src[(r / rpb)*src_rpb + src_off + r % rpb][:]
 * row gather/scatter used for the cond2lat concat (Model/vaetf.py:88-91). accumulate: += */
int gct_copy_rows(const float* src, int64_t src_rpb, int64_t src_off, float* dst, int64_t dst_rpb,
                  int64_t dst_off, int64_t rows, int64_t rpb, int cols, int accumulate,
                  void* stream);
/* tiny dense layer for the property embeddings (Model/vaetf.py:30,75-77; K = n_c <= 8):
 * y[b][n] = sum_k x[b][k]*w[n][k] + b[n]; bwd gives dw, db (overwrite) and no dx. */
int gct_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int rows,
                         int K, int N, void* stream);
int gct_small_linear_bwd(const float* dy, const float* x, float* dw, float* db, int rows, int K,
                         int N, void* stream);
/* dst[i] = sum_s slabs[s*stride + i] (deterministic slab reduction) */
int gct_reduce_slabs(const float* slabs, int nslab, int64_t stride, float* dst, int64_t n,
                     int accumulate, void* stream);
/* Deferred slab reductions: between gct_reduce_defer_begin and gct_reduce_defer_end every float4-shaped slab reduction
 * that the calling THREAD issues through this library (the tails of gct_linear_wgrad, gct_norm_bwd's alpha / bias
 * partials, bias column sums, gct_embed_pe_bwd's dtable) is recorded instead of launched; gct_reduce_defer_flush launches all recorded ones as ONE
 * kernel on `stream` (same summation order per region: results are bit-identical) and keeps recording, _end flushes and
 * stops, _pending returns the number recorded.  Contract: the caller keeps every recorded call's workspace intact until
 * the flush and does not read the destinations before it (a layer's parameter gradients: engine.py flushes at the end of
 * each layer's backward pass, before the data-parallel exchange may start). */
int gct_reduce_defer_begin(void);
int gct_reduce_defer_flush(void* stream);
int gct_reduce_defer_end(void* stream);
int gct_reduce_defer_pending(void);
/* y = a + b (gradient joins of the residual stream) */
int gct_add(const float* a, const float* b, float* y, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCTPLUS_HIP_H */
