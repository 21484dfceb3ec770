/* libavsiam_hip.so - C ABI of the MI355X (gfx950) kernels behind the AVSiam pre-training hot path.
 *
 * The reference (GenjiB/AVSiam) has no native code and no FFI: its hot path is torch.nn calls inside
 * src/models/cav_mae_base.py.  Each entry point below names the reference operation it replaces (file:line
 * relative to /root/reference).  The binding a maintainer adds on the reference side is the ctypes loader of
 * INTEGRATION.md (avsiam_amd/_lib.py is that loader).
 *
 * Conventions
 *  - all pointers are DEVICE pointers; bf16 tensors are raw uint16_t bits; row-major; leading dimensions in elements
 *  - kernels are enqueued on `stream` and never synchronise, allocate or take ownership
 *  - return 0 on success, -1 runtime/launch error, -2 bad argument; avs_last_error() describes the failure
 *  - re-entrant per stream.  Global state: the thread-local error string, and the process-wide TUNING KNOBS below (avs_tuning_set):
 *    plain integers the launchers read; they are written only through this ABI (the host binding sets them once at load from the
 *    AVSIAM_* environment - the library itself never reads the environment and initialises nothing lazily), before kernels are queued
 */
#ifndef AVSIAM_HIP_H
#define AVSIAM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* avs_stream_t;
typedef uint16_t avs_bf16;

const char* avs_last_error(void);
int avs_abi_version(void);
int avs_device_cu_count(void);

/* ---- tuning knobs (no reference counterpart: the reference leaves kernel selection to cuBLAS / cuDNN heuristics).  name:
 *   "gemm_tile" 0 auto | 128 | 256          "gemm_persistent" 0 | 1          "gemm_nt8" 0 | 1 (8-phase 256^2 kernels)
 *   "nt_tile_h" 0 auto | 256 | 224 | 240    "nt_grid" cap of the persistent nt grid, 0 = none
 *   "cu_reserve" compute units EVERY persistent kernel (nt / fp8 nt / tn8 / tn8f grids and split factors) leaves free, a multiple of 8
 *                keeps the XCDs balanced; 0 on one GPU, 8 when a gradient all-reduce overlaps the backward (src/traintest_cavmae_base.py:58-59
 *                is DDP's overlap; RCCL's kernels need CUs WHILE a GEMM runs)
 *   "gemm_ring" 0 | 1 | 2 (default): small forward / input-gradient GEMMs (at most one 128 x 128 workgroup per CU) on the two-buffer kernel | the
 *               4-slot LDS-DMA ring kernel | the ring kernel, and 64 x 128 half-height tiles when even those fill less than half the CUs
 *   "nt_big_min" forward / input-gradient GEMMs with at least this many 256 x 256 output tiles run the persistent 256^2 kernels, smaller ones the
 *               128 x 128 kernels; 0 (default) = half the persistent CU slots
 *   "ln_dma" 0 | 1    "ln_rpw" 0 auto | 4 | 8 | 16    "attn_ring" 0 (default) | 1 (attention forward / dQ with K/V tiles by LDS-DMA ring: same bits, not faster)
 *   "det" 0 (default) | 1: every reduction into a parameter gradient has one writer per element and a fixed order - weight-gradient GEMMs
 *               without a split of their token rows, column sums / vector-matrix product / LayerNorm slab reduce as one block per column group,
 *               atomics-free positional scatter and un-shuffle token sums: two runs of a step give the same bits (a debugging mode, slower;
 *               the reference gets the same from torch.use_deterministic_algorithms).  The host also keeps the step on ONE stream and takes the
 *               fc1 bias gradient by avs_colsum_bf16 instead of the GEMM epilogue's atomics (EngineOptions.deterministic)
 *   "retr_segments" 0 (default) automatic | 1..64: gallery-column segments per query panel of avs_retrieval_rank (every value gives the same
 *               bytes; avs_retrieval_rank_ws_bytes follows the knob, so size the workspace after setting it)
 * avs_persistent_cu_slots(): the CUs a persistent grid fills now (device CUs - cu_reserve). */
int avs_tuning_set(const char* name, int value);
int avs_tuning_get(const char* name, int* value);
int avs_persistent_cu_slots(void);

/* ---- LayerNorm with per-row modality affine (Block.norm1/_a/_v, norm2/_a/_v: src/models/cav_mae_base.py:120-122,
 * 135-137,151-152,169-170,190-191; final norms :492,495,563,566,631).  x fp32 [rows,D] -> y bf16.  row_mod (0/1 per
 * row, may be NULL) picks (g0,b0) or (g1,b1); out_map (may be NULL) redirects output row r to y[out_map[r]]; y is bf16
 * (GEMM operand) or fp32 when y_f32 (final norms that feed the fp32 residual stream / the token mean). */
int avs_layernorm_ws_floats(int rows, int D);
int avs_layernorm_fwd(const float* x, const float* g0, const float* b0, const float* g1, const float* b1,
                      const uint8_t* row_mod, const int* out_map, void* y, int y_f32, float* mean, float* rstd, int rows,
                      int D, float eps, avs_stream_t stream);
/* the same, also writing y8 = e4m3(clamp(y * q8, +-448)) (bf16 output only; y8 may be NULL): the fp8 operand of the forward GEMM that
 * consumes this LayerNorm in the fp8-forward mode, without a quantising pass of its own.  q8_dev (may be NULL): a device
 * quantisation record (see avs_fp8_scale_update) - the scale is then read from q8_dev[0] and max |y| folded into q8_dev[2] */
int avs_layernorm_fwd_q8(const float* x, const float* g0, const float* b0, const float* g1, const float* b1,
                         const uint8_t* row_mod, const int* out_map, void* y, int y_f32, float* mean, float* rstd, int rows,
                         int D, float eps, uint8_t* y8, float q8, float* q8_dev, avs_stream_t stream);
/* dx = dres + LN'(dy) (dres may be NULL; dx may alias dres); dy is bf16, or fp32 when dy_f32; dx_bf16 (may be NULL) gets a
 * bf16 copy of dx; dg/db are accumulated (+=); dcol (may be NULL) accumulates the column sum of dx, i.e. the bias gradient
 * of the Linear that produced this residual branch; ws: avs_layernorm_ws_floats.
 * dres_bf16 != 0: dres is bf16 (the residual-gradient stream kept in bf16 between blocks - the previous call's dx_bf16);
 * dx may then be NULL (only dx_bf16 is written); dx_bf16 must not alias a bf16 dres.
 * dx8 / q8 (fp8 backward; both or neither): also dx8 = e5m2(clamp(dx * q8[0])) - the gradient operand of an fp8 input-gradient GEMM -
 * with max |dx| folded into the device record q8 (avs_fp8_scale_update)
 * D = 1536 / 2048 / 2560: the fusion classification head's LayerNorm over the concatenated audio | video feature (mlp_head_mm[0],
 * src/models/cav_mae_base.py:812-813,1031, and its backward at traintest_ft_base.py:171): few rows, dx / dx_bf16 / dres / row_mod / out_map as
 * above, dg / db reduced in the call in row order (one writer per element; a NULL target skips it), ws unused, no dx8 and no dcol.  These
 * widths came with avs_cls_loss (ABI version unchanged: additions only): a library that exports avs_cls_loss accepts them */
int avs_layernorm_bwd(const void* dy, int dy_f32, const float* x, const float* mean, const float* rstd, const float* g0,
                      const float* g1, const uint8_t* row_mod, const int* out_map, const void* dres, int dres_bf16, float* dx,
                      avs_bf16* dx_bf16, float* dg0, float* db0, float* dg1, float* db1, float* dcol, float* ws, int rows,
                      int D, uint8_t* dx8, float* q8, avs_stream_t stream);
/* Deferred parameter-gradient reduce (a stack's LayerNorm backwards: ONE reduce launch at the end of the stack's backward instead of one per
 * LayerNorm inside it).  avs_layernorm_bwd called with dg0 = db0 = dg1 = db1 = dcol = NULL leaves its per-block partial sums in ws
 * (avs_layernorm_bwd_slabs(rows) slabs of 5 * D floats; a ws of its own per call); avs_layernorm_bwd_reduce_batched adds n such slab sets to their
 * targets: desc (device, 7 * n int64) = {ws, slabs, dg0, db0, dg1, db1, dcol} per set, targets may be 0.  Not in the deterministic mode. */
int avs_layernorm_bwd_slabs(int rows);
int avs_layernorm_bwd_reduce_batched(const long long* desc, int n, int D, avs_stream_t stream);

/* ---- bf16 MFMA GEMMs (nn.Linear / PatchEmbed.proj and their backward: cav_mae_base.py:51,55,60,77,96-99,138-143,
 * 600,634-635).  nt: x = alpha*(A[M,K].B[N,K]^T + bias [*aux] + res[res_idx? res_idx[m] : m]); act 0: out = x;
 * act 1 (timm Mlp fc1 + GELU forward): out = gelu'(x) bf16 - what the backward needs of the pre-activation - and
 * out2 = gelu(x) bf16; act 2 (fc2 input gradient): aux = the saved gelu'(x), out = x.  N%128==0, K%64==0.
 * Columns [0, scale_cols) (a multiple of 64, 0 = none) are multiplied by col_scale in addition: the qkv projection
 * uses it to hand the attention kernels q already multiplied by hd^-0.5 * log2(e), rounded to bf16 once.
 * colsum (bf16 output only, may be NULL): colsum[n] += sum over rows of the output - the bias gradient of the layer
 * whose output gradient this GEMM produces (fc1.bias from the fc2 dgrad), without re-reading the matrix.
 * fp32 output (out_f32 == 1) requires act 0.
 * gelu'(x) as 8-bit fixed-point codes (ABI 2; round((g' + 0.1296875) * 202), g' in [-0.129, 1.129]: a step of 0.005): out_f32 == 2 with act 1 -
 * `out` receives one byte per value, ldo in BYTES; act 3 = act 2 whose `aux` holds those codes (ldaux in bytes) - half the bytes of the one
 * output / operand nothing else reads (as avs_gemm_nt_fp8's out_f32 == 2 / a_e5m2 == 2).  Opt-in (EngineOptions.gelu8). */
int avs_gemm_nt_bf16(const avs_bf16* A, long long lda, const avs_bf16* B, long long ldb, int M, int N, int K,
                     const float* bias, const float* res, long long ldr, const int* res_idx, const avs_bf16* aux,
                     long long ldaux, void* out, long long ldo, int out_f32, avs_bf16* out2, long long ldo2, float alpha,
                     int act, int scale_cols, float col_scale, float* colsum, avs_stream_t stream);
/* ---- fp8 (OCP e4m3) variant of the forward / input-gradient GEMM (BASELINE configs[4]'s "fp8 MFMA path"; not used by the default
 * bf16 path): x = alpha * (A8[M,K] . B8[N,K]^T) + bias (+ res, fp32 output only); act 0: out = x (columns [0, scale_cols) times col_scale);
 * act 1: out = gelu'(x), out2 = gelu(x) (bf16), as in avs_gemm_nt_bf16, and out8 (may be NULL) = e4m3(gelu(x) * out8_scale) for the next fp8 GEMM.
 * fp32 accumulation on v_mfma_f32_16x16x128_f8f6f4,
 * the 8-phase 256x256 kernel of the bf16 GEMM with 128-value K-tiles.  alpha carries 1 / (scale_A * scale_B).  N%256==0, K%128==0,
 * K>=256, leading dimensions multiples of 16.
 * Delayed scaling (no host synchronisation anywhere): a tensor's quantisation state is a DEVICE record of 1024 floats:
 * q[0..3] = {scale, 1 / scale, running max |x| since the last update, saturation events} and 15 shards of the running max at q[64 (1 + k)]
 * (producers add to one shard each, every shard in a 256-byte line of its own: a single address would serialise their atomics).  Where an entry point takes such a record
 * (qa / qw / qw2: operands of the GEMM, de-quantisation factor qa[1] * qw[1]; q8: the e4m3 copy a kernel writes - scale q8[0], amax into
 * q8[2]) it overrides the host float beside it.  avs_fp8_scale_update(q [n][1024], hist [nhist][n], n, nhist, pos, margin, first, count, fmax): per
 * record in [first, first + count), hist[pos] = max(q[2], shards); scale = fmax / (margin * max over hist); q[2] *= 0.9 (the floor the producers filter their atomics against);
 * q[3] += (q[2] * old scale > fmax);
 * fmax = 448 (e4m3 tensors) or 57344 (e5m2: the gradient operands of the input-gradient form).
 * Input-gradient form (a_e5m2 != 0; BASELINE configs[4]'s fp8 path in the backward): A holds e5m2 gradients, B the e4m3 transposed weight;
 * act 0, or act 2 with aux / colsum as in avs_gemm_nt_bf16 (fc2 input gradient); out8 (may be NULL) = e5m2(out * q8[0]) for the next one.
 * gelu'(x) as 8-bit codes (fp8 backward: half the bytes between the two epilogues that write and read it): out_f32 == 2 with act 1 - `out` receives
 * round((gelu'(x) + 0.1296875) * 202) in [0, 255], one byte per element, ldo in bytes; a_e5m2 == 2 with act 2 - `aux` holds such codes, ldaux in bytes.
 * m_split / B2 / bias2 / qw2: a second weight set for rows from m_split (m_split % 256 == 0; needs the records), else m_split = 0.
 * avs_absmax: out = max(out, max |x|) (caller zeroes out; x fp32 or bf16);
 * avs_quantize_fp8: y = e4m3(clamp(x * scale, +-448)) (e5m2 != 0: e5m2, +-57344), n%4==0; with q: scale = q[0], max |x| into q[2]. */
int avs_gemm_nt_fp8(const uint8_t* A, long long lda, const uint8_t* B, long long ldb, int M, int N, int K, const float* bias,
                    const float* res, long long ldr, void* out, long long ldo, int out_f32, avs_bf16* out2, long long ldo2, float alpha,
                    int act, int scale_cols, float col_scale, uint8_t* out8, long long ldo8, float out8_scale, const float* qa,
                    const float* qw, float* q8, int m_split, const uint8_t* B2, const float* bias2, const float* qw2, int a_e5m2,
                    const avs_bf16* aux, long long ldaux, float* colsum, float* colsum2, avs_stream_t stream);
int avs_absmax(const void* x, int is_f32, long long n, float* out, avs_stream_t stream);
int avs_quantize_fp8(const void* x, int is_f32, uint8_t* y, long long n, float scale, float* q, int e5m2, avs_stream_t stream);
/* many bf16 tensors in one launch (all weights of a stack, once per forward): desc [n][4] = {src, dst, numel / 4, record index}, cmap
 * [nchunks][2] = {descriptor, first 4-element group} per chunk of 8192 elements; scales from / amax into the records q [.][1024] */
int avs_quantize_fp8_batched(const long long* desc, const int* cmap, int nchunks, float* q, int e5m2, avs_stream_t stream);
/* many small regions zeroed by one launch: desc [n][2] = {address (16-byte aligned), bytes / 16}, cmap [nchunks][2] = {descriptor, first
 * 16-byte group} per chunk of 64 KB.  No reference counterpart (torch allocates every activation afresh); used for the pad rows of a stack's
 * buffers when the two passes of a step share one activation pool (engine.BufferPool) */
int avs_zero_batched(const long long* desc, const int* cmap, int nchunks, avs_stream_t stream);
int avs_fp8_scale_update(float* q, float* hist, int n, int nhist, int pos, float margin, int first, int count, float fmax, avs_stream_t stream);
/* the same GEMM over TWO weight sets in one launch: rows [0, m_split) of A meet B / bias / colsum, rows [m_split, M) meet
 * B2 / bias2 / colsum2 (same shapes and leading dimension; m_split a multiple of 256).  Replaces the two nn.Linear calls the
 * reference makes per layer for its separate audio and visual towers (cav_mae_base.py:487,489: `blk(v, 'v')` on
 * vit_base.blocks and `blk(a)` on ast_base.blocks), whose row counts alone (8 192 / 31 360 at batch 64) leave the chip
 * partly idle. */
int avs_gemm_nt_bf16_dual(const avs_bf16* A, long long lda, const avs_bf16* B, long long ldb, int M, int N, int K,
                          const float* bias, const float* res, long long ldr, const int* res_idx, const avs_bf16* aux,
                          long long ldaux, void* out, long long ldo, int out_f32, avs_bf16* out2, long long ldo2, float alpha,
                          int act, int scale_cols, float col_scale, float* colsum, int m_split, const avs_bf16* B2,
                          const float* bias2, float* colsum2, avs_stream_t stream);
/* number of kernel dispatches avs_gemm_nt_bf16 has issued so far (a call is one dispatch, or two when the rows left over
 * after the whole rounds of 256x256 tiles go to the half-height-tile kernel): lets bench.py quote a per-DISPATCH average
 * that is directly comparable with rocprofv3's per-kernel statistics */
long long avs_gemm_nt_dispatches(void);
/* tile selection of the nt kernel: 0 = automatic (256x256 when that alone fills the chip, else 128x128), 128, 256 */
int avs_gemm_set_tile(int tile);
/* 1 (default): 256x256 nt tiles run as persistent workgroups (one per CU); 0: one workgroup per tile (A/B measurements) */
int avs_gemm_set_persistent(int on);
/* 1 (default): 256x256 tiles of BOTH GEMMs (nt and tn) run the 8-phase kernels (two wave groups offset by a barrier,
 * 16-KiB staging granules, counted vmcnt); 0: the two-buffer kernels (A/B measurements, the bitwise cross-check of
 * tests/test_kernels_gpu.py).  Environment: AVSIAM_GEMM_NT8=0|1. */
int avs_gemm_set_nt8(int on);
/* tile HEIGHTS of the 8-phase nt kernel.  A persistent workgroup per CU pays whole rounds of tiles, so 0 (default) lets the host mix
 * 256-row and 224-row tiles per GEMM such that the rounds the 256-row tiling needs are filled exactly with cheaper tiles (1122 tiles of
 * 256 rows = 4.4 rounds cost 5 tile-times per CU; 24 + 1254 tiles in two heights cost 4.6); 256 / 224: one height for every tile, 240: half
 * the row tiles of each (A/B measurements, the bitwise cross-check of tests/test_kernels_gpu.py).  With two weight sets the 256-row class
 * covers the first set (the row split is a multiple of 256); the forced one-height modes 224 / 240 apply to one weight set only.
 * Environment: AVSIAM_NT_TILE_H. */
int avs_gemm_set_tile_height(int h);
/* tn (weight gradient): C[N1,N2] += A[M,N1]^T . B[M,N2], fp32 atomics; A and B must be allocated and ZERO up to the
 * next multiple of 64 rows; N1%128==0, N2%128==0; splits<=0 picks a split of the contraction that fills the chip. */
int avs_gemm_tn_bf16(const avs_bf16* A, long long lda, const avs_bf16* B, long long ldb, float* C, long long ldc, int M,
                     int N1, int N2, int splits, avs_stream_t stream);
/* The plan avs_gemm_tn_bf16 takes for (M, N1, N2) with splits <= 0 under the current knobs: output tile size (128 | 256) and the number of
 * splits of the token rows.  Host arithmetic only (no device work, callable without a GPU): pins the split heuristic in the CPU test suite. */
int avs_gemm_tn_plan(int M, int N1, int N2, int* tile, int* splits);
/* The kernel family avs_gemm_nt_bf16 dispatches (M, N, K) to under the current knobs: family 0 two-buffer 128 x 128 tiles | 1 LDS-DMA ring,
 * 128 x 128 | 2 ring, 64 x 128 half-height tiles | 3 two-buffer, 64 x 128 | 4 the 256 x 256 kernels (8-phase or two-buffer).  workgroups: for
 * families 0 - 3 the grid launched; for family 4 the NOMINAL min(256-row tiles, avs_persistent_cu_slots()) - the launch itself may walk more,
 * cheaper 224-row tiles, cap its grid (nt_grid) or start one workgroup per tile (gemm_persistent = 0): avs_gemm_nt_launch_plan gives the real
 * grid.  A coarse view of that plan, kept for the dispatch thresholds it pins.  Host arithmetic only (callable without a GPU). */
int avs_gemm_nt_plan(int M, int N, int K, int* family, int* workgroups);
/* The launch avs_gemm_nt_bf16 (m_split <= 0 or >= M: one weight set) / avs_gemm_nt_bf16_dual (rows from m_split use the second set) makes
 * for (M, N, K) under the current knobs - the plan the launcher itself consumes, for one dispatch (a call whose epilogue streams exceed
 * 4 GiB is two dispatches over halves of its rows, each planned like this).  Writes the first min(n_out, 8) of, in this order:
 *   out[0] kernel   0 two-buffer 128 x 128 | 1 two-buffer, 64 x 128 half-height tiles | 2 ring 128 x 128 | 3 ring, 64 x 128 | 4 two-buffer
 *                   256 x 256 | 5 8-phase, one tile height (256 rows) | 6 8-phase, two tile heights (256 and 224 rows)
 *   out[1] grid     workgroups launched          out[2] block   threads per workgroup          out[3] lds   dynamic LDS bytes
 *   out[4] tb       kernel 6: tiles [0, tb) are 256 rows high, the others 224 (0: every tile 224 rows); 0 for the other kernels
 *   out[5] m_full   kernel 4: rows [0, m_full) in 256-row tiles, the rest in 128-row tiles; kernel 1: 0; M for the other kernels
 *   out[6] tiles    output tiles the grid walks (more than grid when the workgroups are persistent)
 *   out[7] family   as avs_gemm_nt_plan
 * Host arithmetic only (callable without a GPU). */
int avs_gemm_nt_launch_plan(int M, int N, int K, int m_split, int* out, int n_out);
/* up to three weight gradients over the SAME M token rows in one launch: Ci[N1_i, N2_i] (contiguous) += Ai^T . Bi; problem i is absent
 * when Ai is NULL (problem 0 must exist).  A block's fc2 / fc1 / proj gradients (timm Mlp + Attention.proj, cav_mae_base.py:77,138-143)
 * exist at the same time; together they fill the chip with 3 splits of the token rows instead of 7 + 7 + 14, i.e. with 40 % of the fp32
 * atomic traffic.  When every N is a multiple of 256 the 8-phase 256 x 256 kernel takes all tiles; otherwise one launch per problem. */
int avs_gemm_tn_bf16_group3(const avs_bf16* A0, long long lda0, const avs_bf16* B0, long long ldb0, float* C0, int N1_0, int N2_0,
                            const avs_bf16* A1, long long lda1, const avs_bf16* B1, long long ldb1, float* C1, int N1_1, int N2_1,
                            const avs_bf16* A2, long long lda2, const avs_bf16* B2, long long ldb2, float* C2, int N1_2, int N2_2,
                            int M, avs_stream_t stream);

/* the same three-problem launch on fp8 operands (fp8 mode 3): Ai = the e5m2 copy of the output gradient [M, N1_i], Bi = the e4m3 copy of
 * the layer input [M, N2_i] (both ZERO up to the next multiple of 64 rows; leading dimensions in bytes, multiples of 16), qai / qbi the two
 * operands' device records (the product is de-quantised with qa[1] * qb[1]); every N a multiple of 256.  v_mfma_f32_32x32x64_f8f6f4 on
 * fragments read with ds_read_b64_tr_b8; fp32 atomics into the gradient arena like the bf16 form. */
int avs_gemm_tn_fp8_group3(const uint8_t* A0, long long lda0, const uint8_t* B0, long long ldb0, float* C0, int N1_0, int N2_0, const float* qa0, const float* qb0,
                           const uint8_t* A1, long long lda1, const uint8_t* B1, long long ldb1, float* C1, int N1_1, int N2_1, const float* qa1, const float* qb1,
                           const uint8_t* A2, long long lda2, const uint8_t* B2, long long ldb2, float* C2, int N1_2, int N2_2, const float* qa2, const float* qb2,
                           int M, avs_stream_t stream);

/* ---- varlen attention (F.scaled_dot_product_attention in Attention.forward, cav_mae_base.py:60-68) on the packed
 * qkv matrix [rows, 3*D] (q|k|v, head h at columns h*hd); one (tile_start, tile_len, tile_q0) triple per tile of
 * tile_rows (128: 4-wave workgroups; 64: 2-wave workgroups, twice as many resident per CU - for short sequences) rows.
 * Head dims hd = D / H: 64 (ViT-B/L encoder), 32 (decoder), 80 (ViT-H encoder; both tile heights, no ring form).  lse/delta: [H][rows_total] fp32.
 * Rows of qkv, out, dout and dqkv must be 16-byte aligned: ld and ldo multiples of 8 elements (the kernels load fragments and store
 * accumulator blocks 16 bytes per lane), ldo8 / ld8 of the 8-bit copies multiples of 16; other strides are refused (-2). */
int avs_attn_fwd(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                 const int* tile_q0, int ntiles, int tile_rows, avs_bf16* out, long long ldo, float* lse, int rows_total,
                 avs_stream_t stream);
/* the same, also writing out8 = e4m3(clamp(out * q8[0], +-448)) [rows, D] / ldo8 - the fp8 operand of the proj GEMM in the fp8 mode -
 * and folding max |out| into q8[2] (device quantisation record, see avs_fp8_scale_update); out8 and q8 both NULL = avs_attn_fwd */
int avs_attn_fwd_q8(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                    const int* tile_q0, int ntiles, int tile_rows, avs_bf16* out, long long ldo, float* lse, int rows_total,
                    uint8_t* out8, long long ldo8, float* q8, avs_stream_t stream);
int avs_attn_bwd(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                 const int* tile_q0, int ntiles, int tile_rows, const avs_bf16* out, const avs_bf16* dout, long long ldo,
                 const float* lse, float* delta, int rows_total, avs_bf16* dqkv, avs_stream_t stream);
/* the same, also writing dqkv8 = e5m2(clamp(dqkv * qd8[0], +-57344)) [rows, 3*D] / ld8 - the gradient operand of the fp8 qkv input-gradient
 * GEMM (fp8 mode 2: every input-gradient GEMM of a block on e5m2 x e4m3) - and folding max |dqkv| into the device record qd8; both NULL =
 * avs_attn_bwd.  kv_bf16 = 0 (with dqkv8 only; fp8 mode 3): the key / value thirds of the bf16 dqkv are not written - the input- and
 * weight-gradient GEMMs read the e5m2 copy; the query third (column sum = bias gradient) always is */
int avs_attn_bwd_q8(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                    const int* tile_q0, int ntiles, int tile_rows, const avs_bf16* out, const avs_bf16* dout, long long ldo,
                    const float* lse, float* delta, int rows_total, avs_bf16* dqkv, uint8_t* dqkv8, long long ld8, float* qd8,
                    int kv_bf16, avs_stream_t stream);
/* Pruned form for the LAST decoder block (forward_decoder + forward_mae_loss, cav_mae_base.py:629-635,679-682: rows with mask 0 contribute
 * neither loss nor gradient, so in the last block they are needed as keys / values only).  Every sequence of the launch has the same length
 * (tile_len); only its FIRST lq rows are queries, all rows are keys / values; `out` / `dout` are COMPACT [nseq * lq, D]: sequence s
 * (= tile_start / tile_len) owns rows s * lq ..; lse / delta / dqkv keep the packed row numbering.  The backward writes dq for the first lq
 * rows of every sequence only (the caller zeroes the query third of the other rows, avs_expand_rows_bf16) and dk / dv for all rows. */
int avs_attn_fwd_cq(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                    const int* tile_q0, int ntiles, int tile_rows, avs_bf16* out, long long ldo, float* lse, int rows_total,
                    int lq, avs_stream_t stream);
int avs_attn_bwd_cq(const avs_bf16* qkv, long long ld, int D, int H, const int* tile_start, const int* tile_len,
                    const int* tile_q0, int ntiles, int tile_rows, const avs_bf16* out, const avs_bf16* dout, long long ldo,
                    const float* lse, float* delta, int rows_total, avs_bf16* dqkv, int lq, avs_stream_t stream);
/* the same backward for sequences of at most rows_per_wg (64 | 128) tokens, in ONE kernel: a workgroup per (sequence, head) reads q, k,
 * v, dO, o once, evaluates S and its exponentials once and writes dq, dk and dv (hd 32 | 64).  seq_start / seq_len: [nseq] */
int avs_attn_bwd_fused(const avs_bf16* qkv, long long ld, int D, int H, const int* seq_start, const int* seq_len, int nseq,
                       int rows_per_wg, const avs_bf16* out, const avs_bf16* dout, long long ldo, const float* lse, int rows_total,
                       avs_bf16* dqkv, avs_stream_t stream);
int avs_attn_bwd_fused_q8(const avs_bf16* qkv, long long ld, int D, int H, const int* seq_start, const int* seq_len, int nseq,
                          int rows_per_wg, const avs_bf16* out, const avs_bf16* dout, long long ldo, const float* lse, int rows_total,
                          avs_bf16* dqkv, uint8_t* dqkv8, long long ld8, float* qd8, int kv_bf16, avs_stream_t stream);
/* The launches an attention entry point makes under the current knobs (attn_ring) - the plan the launcher itself consumes.
 *   pass   which entry points: the forward (avs_attn_fwd / _q8 / _cq), the two-kernel backward (avs_attn_bwd / _q8 / _cq) or the fused one
 *   hd     head dim 32 | 64 | 80         rows   tile_rows / rows_per_wg          g8   the call also writes the 8-bit copy (out8 / dqkv8)
 *   lq     0, or the _cq forms' query rows per sequence (the fused pass has none: ignored)      items   ntiles / nseq      H   heads
 * Writes out[0] = number of dispatches (1; 2 for the two-kernel backward: dQ, then dK/dV), then per dispatch, in this order:
 *   family   enum avs_attn_family         width   LDS image width 32 | 64 | 96 (head dim 80)        waves   2 | 4 | 7 (32 rows each)
 *   g8       the kernel is the form that writes the 8-bit copy (0 in the forward: its kernels take the copy at run time)
 *   grid     workgroups = items * H       block   threads per workgroup                             lds     dynamic LDS bytes
 * A shorter array receives the leading fields only.  -2 for a combination the entry points refuse: head dim 80 fused above 64 rows, 224 rows
 * with head dim != 64 or with the 8-bit copy or outside the fused pass, any other rows / hd.  Host arithmetic only (callable without a GPU). */
enum avs_attn_pass { AVS_ATTN_PASS_FWD = 0, AVS_ATTN_PASS_BWD = 1, AVS_ATTN_PASS_FUSED = 2 };
enum avs_attn_family { AVS_ATTN_FWD = 0, AVS_ATTN_FWD_RING = 1, AVS_ATTN_DQ = 2, AVS_ATTN_DQ_RING = 3, AVS_ATTN_DKV = 4, AVS_ATTN_FUSED = 5,
                       AVS_ATTN_FUSED224 = 6 };
int avs_attn_launch_plan(int pass, int hd, int rows, int g8, int lq, int items, int H, int* out, int n_out);

/* ---- input normalisation on the device (what the reference dataloader does per sample on the host: dataloader.py:505-513
 * fbank = (fbank - norm_mean) / norm_std [+ rand * amp, roll(shift) when `noise`]; :461-462,152-155 frame / 255 then
 * (x - mean_c) / std_c).  audio: in/out [B, T, F] fp32, out of place, F%4==0; shift/amp per sample or NULL; the noise is a
 * Philox stream keyed by seed.  frames: in [n_images, 3, plane] uint8 -> out fp32, plane = H*W, plane%4==0; mean3/std3
 * are HOST pointers to 3 floats. */
int avs_normalize_audio(const float* in, float* out, int B, int T, int F, float mean, float std, const int* shift,
                        const float* amp, unsigned long long seed, avs_stream_t stream);
int avs_normalize_frames_u8(const uint8_t* in, float* out, int n_images, int plane, const float* mean3, const float* std3,
                            avs_stream_t stream);
/* the frame side of mixup (dataloader_ft.py:441-458): out = weight_b n(in1) + (1 - weight_b) n(in2), n the arithmetic of avs_normalize_frames_u8,
 * b = image / per_sample; weight: DEVICE array, one value per sample (n_images / per_sample of them).  weight_b = 1 gives the bytes of
 * avs_normalize_frames_u8(in1). */
int avs_mix_frames_u8(const uint8_t* in1, const uint8_t* in2, const float* weight, float* out, int n_images, int per_sample, int plane,
                      const float* mean3, const float* std3, avs_stream_t stream);

/* ---- waveform input (dataloader_ft.py:277-340): the Kaldi fbank of torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=16000,
 * use_energy=False, window_type='hanning', num_mel_bins=128, dither=0.0, frame_shift=10) and the waveform mixup in front of it, on the device.
 * The specification is avsiam_amd.preprocess.kaldi_fbank_reference (float64).  Per clip b of n = len[b] samples (NULL: stride), n >= 400 (the
 * caller's check; a shorter clip has no frame and gives pad rows only):
 *   frames   m = 1 + (n - 400) / 160; frame j = samples [160 j, 160 j + 400); subtract the frame mean; y[i] = x[i] - 0.97 x[max(i - 1, 0)];
 *            times 0.5 - 0.5 cos(2 pi i / 399); zero-pad to 512; power spectrum |FFT|^2 of bins 0..255
 *   mel      128 triangles in mel(f) = 1127 ln(1 + f / 700) between 20 Hz and 8 kHz, evaluated at the bins' mel; summed in bin order
 *   out      row j = ln(max(E, FLT_EPSILON)) (an energy at or below FLT_EPSILON gives fp32(ln(FLT_EPSILON)) = -15.942385 exactly);
 *            rows m .. target_length - 1 are 0 (ZeroPad2d), frames beyond target_length are not computed;
 *            use_norm: every row, pad rows included, becomes (value - mean) * (1.0f / std), the product in fp32
 *   samples  plain (no partner, lam NULL or lam[b] < 0): w - mean(w).  Mixed: a = w1 - mean(w1); c = w2 - mean(w2) (its own length), then
 *            zero-padded or cut to n; mix = lam a + (1 - lam) c; the samples are mix - mean(mix).  The means come from `sums`.
 * avs_wave_sums: sums[b] = { sum w1 over n, sum w2 over n2, sum w2 over min(n, n2) } in fp64, one fixed-order reduction per clip (the last
 * two are 0 without a partner).  avs_kaldi_fbank reads them; both run on `stream`, neither synchronises (the first avs_kaldi_fbank call
 * on a device uploads the tables with a blocking copy).  No atomics: two calls give identical bytes.  n_mels other than 128 returns -2.
 * avs_fbank_tables: the host tables (fp64 rounded once to fp32) in the layout of csrc/frontend_math.h, FB_TAB_WORDS = 2960 words. */
int avs_wave_sums(const float* wave, long long stride, const int* len, const float* partner, long long partner_stride,
                  const int* partner_len, int B, double* sums, avs_stream_t stream);
int avs_kaldi_fbank(const float* wave, long long stride, const int* len, const float* partner, long long partner_stride,
                    const int* partner_len, const float* lam, const double* sums, int B, int target_length, int n_mels, float* out,
                    int use_norm, float mean, float std, avs_stream_t stream);
int avs_fbank_tables(float* tab, int words);

/* ---- source-rate audio (dataloader_ft.py:272-277, 298-306): torchaudio.functional.resample(waveform, sr, 16000) - windowed sinc, sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99 - and waveform.mean(dim=0), in one launch.  The specification is avsiam_amd.preprocess.resample_reference
 * (float64).  wave fp32 [B, C, stride], 1 <= C <= 8; len[b] samples per clip (DEVICE, NULL: stride; cut to 0 .. stride); tab_idx[b] (DEVICE):
 * the clip's table, or -1 = pass-through (the clip is at the output rate: only the channel mean is taken).
 *   tables   HOST array of n_tables <= 8 DEVICE pointers, geo HOST int[4 n_tables] = (o, n, width, taps) per table: o = rate / gcd, n = new rate /
 *            gcd, the dense filter bank is [n, L], L = 2 width + o (preprocess.resample_table_reference; it is built in Python, never here).  A table
 *            is COMPACT: int32 first[n], then float w[n][pitch], pitch = taps | 1: phase p's dense row is zero outside first[p] .. first[p] + taps - 1
 *            and first[p] + taps <= L.  n * (pitch + 1) <= 16384 words, and the input span of a 1024-output tile,
 *            (1023 / n + 2) * o + 2 width + 3 words, <= 16384 (avs_resample_plan gives both; -2 otherwise).
 *   out      per channel, output j = q n + p: sum_m w[p][m] x[q o + first[p] + m - width] in fp32, taps in order (samples outside 0 .. len - 1 are
 *            zero); the channels are added in order and divided once by C (C = 1: no division).  out[b, j] for j < out_len[b] =
 *            ceil(n len / o) (64-bit integers), zero from there to out_stride.  Pass-through: out_len = len, out = the channel mean (C = 1: the
 *            input's bytes).  out_stride >= ceil(n stride / o) of every table (-2 otherwise); a pass-through clip is cut to out_stride.
 * One writer per cell, no atomics: two calls give identical bytes.  No synchronisation. */
int avs_resample_plan(int o, int n, int width, int taps, int* table_words, int* span_words);
int avs_resample_wave(const float* wave, int B, int C, long long stride, const int* len, const int* tab_idx, int n_tables,
                      const void* const* tables, const int* geo, float* out, long long out_stride, int* out_len, avs_stream_t stream);

/* ---- PCM decode (dataloader_ft.py:272: torchaudio.load, normalize=True): the payload of a WAV file's data chunk - interleaved sample frames, little
 * endian - to the planar fp32 channels avs_resample_wave reads, in one launch.  The specification is avsiam_amd.preprocess.decode_pcm_reference
 * (numpy, bit for bit).  payload uint8 [B, byte_stride], 16-byte aligned, byte_stride % 16 == 0: row b holds clip b's payload from byte 0 (what lies
 * behind it is never decoded).  desc (DEVICE) int32 [B, 2] = { format, n_frames } per clip; C: the channels of every clip of the call, 1 .. 8.
 *   format   0 U8   (x - 128) * 2^-7            exact          3 S32  (float)x (round to nearest even) * 2^-31      one rounding
 *            1 S16  x * 2^-15                   exact          4 F32  the bits (NaN payloads, -0.0)                 exact
 *            2 S24  3 bytes, sign-extended, x * 2^-23  exact   5 F64  (float)x (a NaN stays a NaN, its payload is not specified)  one rounding
 *   out      fp32 [B, C, stride]: out[b, c, f] = sample c of frame f for f < out_len[b], zero from there to stride
 *   out_len  int32 [B] (DEVICE): n_frames cut to 0 .. min(stride, byte_stride / (C * bytes per sample)); 0 for a format outside 0 .. 5
 * One writer per cell, no atomics: two calls give identical bytes.  No synchronisation. */
int avs_decode_pcm(const uint8_t* payload, long long byte_stride, const int* desc, int B, int C, float* out, long long stride, int* out_len,
                   avs_stream_t stream);

/* ---- decoded-size frames (dataloader_ft.py:136-139, 434-459): frames / 255, Resize([224, 224], BICUBIC, antialias=True), Normalize and the frame
 * mix, from uint8 frames at the video's own size.  The specification is avsiam_amd.preprocess.resize_frames_reference (float64): torch's
 * interpolate(mode='bicubic', align_corners=False, antialias=True), no clamping.  Per axis with input size I and output size O, in float64:
 *   scale = I / O, s = max(scale, 1), support = 2 s; output index i: centre = scale (i + 0.5), start = max(int(centre - support + 0.5), 0),
 *   end = min(int(centre + support + 0.5), I); w_j = cubic((j + start - centre + 0.5) / s), j < end - start, divided by their sum;
 *   cubic(x), a = -0.5: |x| < 1: ((a + 2) |x| - (a + 3)) x^2 + 1; |x| < 2: (((|x| - 5) |x| + 8) |x| - 4) a; else 0.
 * avs_resize_taps (host only, no GPU): start[out_size], count[out_size] and weights[out_size][max_taps] (rounded once to fp32, zero beyond the
 * count) of one axis - the text the kernel runs (csrc/frontend_math.h); -2 when in_size > 10 out_size or max_taps is below what the scale can take.
 * avs_resize_frames_u8: in1 uint8 [n_images, 3, Hs, Ws], a padded buffer: the images of clip b = image / per_sample fill the top-left
 * sizes[2 b] x sizes[2 b + 1] corner (sizes: DEVICE int32 [B, 2], or NULL: Hs x Ws); max_h / max_w: the largest of them (host values; the
 * launch is planned from them and a size beyond them is cut to them).  out fp32 [n_images, 3, out_h, out_w], 16-byte aligned, out_w % 4 == 0:
 *   r = sum_y wy sum_x wx (float)u8 in fp32 in tap order, then n(r) = (r (1/255f) - mean_c) (1 / std_c) as avs_normalize_frames_u8 writes it.
 * in2 (may be NULL, then Hs2 .. max_w2 are 0 and sizes2 / weight NULL): the partner, its own buffer and sizes; out = weight_b n(r1) +
 * (1 - weight_b) n(r2) as avs_mix_frames_u8 (weight: DEVICE, one per clip).  A clip at the output size gives avs_normalize_frames_u8's bytes,
 * weight 1 the plain call's.  1 <= h <= Hs, 1 <= w <= Ws, in / out <= 10 per axis (at most 41 taps: 1080p -> 224 is 8.6); anything else is -2
 * before any launch.  One kernel, the horizontal pass's results stay in LDS; no atomics: two calls give identical bytes.  mean3 / std3: HOST.
 * avs_resize_plan (host only): output rows per workgroup and the LDS bytes (of the call with a partner; without one rows * out_w * 4 fewer)
 * the launch of a batch whose largest clip is max_h x max_w takes. */
int avs_resize_taps(int in_size, int out_size, int* start, int* count, float* weights, int max_taps);
int avs_resize_plan(int max_h, int max_w, int out_h, int out_w, int* rows_per_wg, int* lds_bytes);
int avs_resize_frames_u8(const uint8_t* in1, int Hs, int Ws, const int* sizes, int max_h, int max_w, const uint8_t* in2, int Hs2, int Ws2,
                         const int* sizes2, int max_h2, int max_w2, const float* weight, float* out, int n_images, int per_sample, int out_h,
                         int out_w, const float* mean3, const float* std3, avs_stream_t stream);

/* ---- raw inputs, fused.  The same dataset arithmetic as avs_normalize_* above, applied where the input
 * is READ - the patch gather of the embedding and the target gather of the reconstruction loss - so un-normalised fbank
 * and uint8 frames go straight from the loader's buffers into the model: one read of the raw tensor per consumer instead of
 * read + write + read.  kind 0 / NULL: the tensor is the normalised fp32 tensor of the reference's forward() contract.
 * kind 1 (audio [B, T, F] fp32): value(b,t,f) = (in[b, (t - shift_b) mod T, f] - mean[0]) / std[0] + amp_b * U(b, ts, f); shift / amp
 * are DEVICE arrays per sample or NULL (dataloader.py:510-513: the `noise` augmentation), U is the Philox stream of
 * avs_normalize_audio for the same seed, so both paths agree bit for bit.  kind 2 (frames [n, 3, H, W] uint8):
 * value = (in / 255 - mean[c]) / std[c] (:461-462, 152-155).  The struct itself is read on the HOST at call time. */
typedef struct avs_input_xf {
    int kind;
    float mean[3], std[3];
    const int* shift;
    const float* amp;
    unsigned long long seed;
} avs_input_xf;

/* ---- patch gather of the kept tokens (PatchEmbed input side + random_masking gather: cav_mae_base.py:96-99,
 * 382,431,444-455); the _xf forms take a raw input and its transform */
int avs_im2col_audio(const float* a, const int* row_b, const int* row_tok, avs_bf16* out, int rows, int tlen, int mel,
                     int t_patches, avs_stream_t stream);
int avs_im2col_video(const float* v, const int* row_img, const int* row_tok, avs_bf16* out, int rows, int C, int H, int W,
                     avs_stream_t stream);
int avs_im2col_audio_xf(const float* a, const int* row_b, const int* row_tok, avs_bf16* out, int rows, int tlen, int mel,
                        int t_patches, const avs_input_xf* xf, avs_stream_t stream);
int avs_im2col_video_xf(const void* v, const int* row_img, const int* row_tok, avs_bf16* out, int rows, int C, int H, int W,
                        const avs_input_xf* xf, avs_stream_t stream);
/* random masking on the device (random_masking_unstructured / _structured + the gather index build,
 * cav_mae_base.py:365-439): one workgroup per sequence; seqs = nseq x 16 int32 {L, keep, row_off, src_id, dec_off, enc_base,
 * t_patches, ids_off, mask_off, tmask_x, 0, 0, dec_m_off, dec_k_off, pred_off, pos_base} (the last four: avs_mask_plan_grouped; dec_m_off
 * must be -1 for the two entry points below); L <= 1024.  tmask_lo/hi, fmask (per sequence bit masks of the time columns /
 * frequency rows forced to be removed) are read only where t_patches > 0.  src_row / mask_out / ids_out may be NULL when no
 * sequence uses them. */
int avs_mask_plan(const int* seqs, int nseq, const unsigned* tmask_lo, const unsigned* tmask_hi, const unsigned* fmask,
                  unsigned long long seed, int* row_src, int* row_tok, int* src_row, float* mask_out, int* ids_out,
                  avs_stream_t stream);
/* the same with the Philox key in device memory, read when the kernel runs (a training step replayed from a captured hipGraph
 * freezes kernel arguments; graph_step.GraphedTrainStep advances the key with a node of the graph) */
int avs_mask_plan_dev(const int* seqs, int nseq, const unsigned* tmask_lo, const unsigned* tmask_hi, const unsigned* fmask,
                      const unsigned long long* seed_dev, int* row_src, int* row_tok, int* src_row, float* mask_out, int* ids_out,
                      avs_stream_t stream);
/* GROUPED decoder layout: for the sequences whose descriptor has dec_m_off >= 0 the decoder rows of a sample are ordered [tokens whose
 * prediction is scored (mask 1) | kept tokens] instead of by position (forward_decoder's un-shuffle is a permutation of tokens that the
 * attention blocks are equivariant to, cav_mae_base.py:604-626): src_row[dec row] = encoder row | -1 with dec row = dec_k_off + j (kept) |
 * dec_m_off + j - keep (masked); pos_row[dec row] = pos_base + token (the positional embedding it takes); row_of_pos[dec_off + token] =
 * dec row; pred_id[pred_off + j - keep] = mask_off + token (the (sample, token) a compact prediction row scores).  seed_dev may be NULL. */
int avs_mask_plan_grouped(const int* seqs, int nseq, const unsigned* tmask_lo, const unsigned* tmask_hi, const unsigned* fmask,
                          unsigned long long seed, const unsigned long long* seed_dev, int* row_src, int* row_tok, int* src_row,
                          float* mask_out, int* ids_out, int* pos_row, int* row_of_pos, int* pred_id, avs_stream_t stream);
int avs_cast_scale_bf16(const float* x, avs_bf16* y, long long n, float alpha, avs_stream_t stream);
/* out[r, 0:cols] = src_row[r] >= 0 ? in[src_row[r], 0:cols] : 0 (bf16, cols % 8 == 0, leading dimensions in elements, % 8 == 0).
 * in == NULL: only the rows with src_row[r] < 0 are written (zeroed).  No reference counterpart: bookkeeping of the pruned last decoder block */
int avs_expand_rows_bf16(const avs_bf16* in, long long ld_in, const int* src_row, avs_bf16* out, long long ld_out, int rows, int cols,
                         avs_stream_t stream);
int avs_scatter_add_rows(const avs_bf16* src, const int* idx, float* dst, int rows, int D, float scale, avs_stream_t stream);
/* out[c] += sum over rows of x[r][c], c < C (C % 64 == 0); ld: leading dimension of x (a column range of a wider matrix is allowed) */
int avs_colsum_bf16(const avs_bf16* x, long long ld, float* out, int rows, int C, avs_stream_t stream);
/* y[n] += alpha * sum_k x[k] * W[k][n]  (x fp32 [K], W bf16 [K, N] / ld, N % 256 == 0, K % 32 == 0): the value third of the qkv bias
 * gradient = (proj bias gradient) . W_proj, because softmax rows sum to one (Attention, cav_mae_base.py:51,60-77); the key third is 0 */
int avs_vecmat_bf16(const float* x, const avs_bf16* W, long long ld, float* y, int K, int N, float alpha, avs_stream_t stream);
/* n such products of one shape in one launch: desc (device, int64 [n][3]) = {x, W, y} pointers (a stack's blocks at the end of its backward) */
int avs_vecmat_bf16_batched(const long long* desc, int n, long long ld, int K, int N, float alpha, avs_stream_t stream);

/* ---- decoder un-shuffle (forward_decoder, cav_mae_base.py:604-626) */
int avs_unshuffle_fwd(const float* x, const int* src_row, const int* pos_row, const uint8_t* row_mod,
                      const float* mask_token, const float* pos_a, const float* pos_v, int La, const float* mod_a,
                      const float* mod_v, float* out, int rows, int D, avs_stream_t stream);
int avs_unshuffle_bwd(const float* dout, const int* src_row, int B, int T, int La, int Lv, float* dx, float* dpos_a,
                      float* dpos_v, float* dmask, float* dmod_a, float* dmod_v, int D, avs_stream_t stream);
/* the same when the decoder rows are not in position order (avs_mask_plan_grouped): row_of_pos[b * (La + T * Lv) + position] = decoder row */
int avs_unshuffle_bwd_map(const float* dout, const int* src_row, int B, int T, int La, int Lv, float* dx, float* dpos_a,
                          float* dpos_v, float* dmask, float* dmod_a, float* dmod_v, int D, const int* row_of_pos, avs_stream_t stream);

/* ---- token mean per packed sequence (.mean(dim=1), cav_mae_base.py:563,566).  row_map (may be NULL): segment s is row row_map[s]
 * of reps / dreps - the mixed encoder's inverse permutation (:584-590) folded into the reduction */
int avs_segment_mean_fwd(const float* y, const int* seg_start, float* reps, int nseg, int D, const int* row_map, avs_stream_t stream);
int avs_segment_mean_bwd(const float* dreps, const int* seg_start, float* dy, int nseg, int D, float scale, const int* row_map,
                         avs_stream_t stream);
/* the same with accumulate != 0: dy[r] += ... (the fine-tuned model's pooled heads out_a / out_v, cav_mae_base.py:1011-1012, add their
 * gradient to what the fusion blocks' backward left on the same token rows, :1014-1023).  A segment's rows have one writer: no atomics */
int avs_segment_mean_bwd_acc(const float* dreps, const int* seg_start, float* dy, int nseg, int D, float scale, const int* row_map,
                             int accumulate, avs_stream_t stream);

/* ---- masked-MSE with patchify on the fly (patchify + forward_mae_loss, cav_mae_base.py:343-351,663-683) */
/* loss[0] = masked mean; total (may be NULL): total[0] = (total_init ? 0 : total[0]) + loss[0]  (loss_mae = a + v, :707) */
int avs_mae_loss_fwd(const float* pred, const float* inp, const float* mask, float* row_loss, float* loss, float* total,
                     int total_init, int rows, int audio, int L, int C, int H, int W, float nmask, avs_stream_t stream);
int avs_mae_loss_bwd(const float* pred, const float* inp, const float* mask, const float* gout, avs_bf16* dpred, int rows,
                     int audio, int L, int C, int H, int W, float nmask, avs_stream_t stream);
/* the same with the target read from a raw input (see avs_input_xf) */
int avs_mae_loss_fwd_xf(const float* pred, const void* inp, const float* mask, float* row_loss, float* loss, float* total,
                        int total_init, int rows, int audio, int L, int C, int H, int W, float nmask, const avs_input_xf* xf,
                        avs_stream_t stream);
int avs_mae_loss_bwd_xf(const float* pred, const void* inp, const float* mask, const float* gout, avs_bf16* dpred, int rows,
                        int audio, int L, int C, int H, int W, float nmask, const avs_input_xf* xf, avs_stream_t stream);
/* the same four with a patch STRIDE (1..16) on 16 x 16 patch storage: token (t, f) / (gy, gx) starts at pixel t*stride / gy*stride, only
 * the stride x stride corner of the 256 positions per channel is gathered (the rest of the im2col row is zero) / scored (mean over the
 * scored elements; dpred is zero elsewhere).  stride 16 = the entry points above.  14: the patch grid of ViT-H/14 (config.stride). */
int avs_im2col_audio_s(const float* a, const int* row_b, const int* row_tok, avs_bf16* out, int rows, int tlen, int mel, int t_patches,
                       int stride, const avs_input_xf* xf, avs_stream_t stream);
int avs_im2col_video_s(const void* v, const int* row_img, const int* row_tok, avs_bf16* out, int rows, int C, int H, int W, int stride,
                       const avs_input_xf* xf, avs_stream_t stream);
int avs_mae_loss_fwd_s(const float* pred, const void* inp, const float* mask, float* row_loss, float* loss, float* total,
                       int total_init, int rows, int audio, int L, int C, int H, int W, float nmask, int stride, const avs_input_xf* xf,
                       avs_stream_t stream);
int avs_mae_loss_bwd_s(const float* pred, const void* inp, const float* mask, const float* gout, avs_bf16* dpred, int rows, int audio,
                       int L, int C, int H, int W, float nmask, int stride, const avs_input_xf* xf, avs_stream_t stream);
/* the same two on COMPACT predictions: only the rows whose mask is 1 exist; prediction row r scores (sample, token) row_id[r] - id_base of
 * the [N * L] numbering mask and targets use (row_id: avs_mask_plan_grouped's pred_id; NULL = the two entry points above) */
int avs_mae_loss_fwd_id(const float* pred, const void* inp, const float* mask, float* row_loss, float* loss, float* total,
                        int total_init, int rows, int audio, int L, int C, int H, int W, float nmask, int stride, const avs_input_xf* xf,
                        const int* row_id, int id_base, avs_stream_t stream);
int avs_mae_loss_bwd_id(const float* pred, const void* inp, const float* mask, const float* gout, avs_bf16* dpred, int rows, int audio,
                        int L, int C, int H, int W, float nmask, int stride, const avs_input_xf* xf, const int* row_id, int id_base,
                        avs_stream_t stream);
/* ---- the way back (unpatchify, cav_mae_base.py:353-363): prediction rows -> the picture the model was shown, the inverse of the index
 * arithmetic above.  n pictures of L = (H / stride) * (W / stride) tokens; audio: [n, H = time, W = mel], C = 1, token f * (H / stride) + t;
 * frames: [n, C, H, W], token gy * (W / stride) + gx.  A cell takes pred[pr, e] where mask[n * L + l] == 1 (paste_kept 0: wherever its
 * token has a prediction row), else the input through `xf` - bit for bit what the loss read as its target; cells no patch covers take the
 * input.  pr = n * L + l (row_id NULL; rows == n * L) or the row with row_id[pr] - id_base == n * L + l (compact rows; inv_ws: n * L int32
 * of workspace the call overwrites; a token without a row takes the input).  Outputs, each may be NULL (not all three):
 *   out      fp32, shape of the input, in the model's units
 *   raw_out  the same through the inverse of xf, multiply and add rounded separately: audio fp32 x * std + mean; frames uint8
 *            rint((x * std_c + mean_c) * 255) clamped to 0..255.  Needs xf; refused (-2) when xf carries shift / amp
 *   err      fp32 [n * L]: row_loss[pr] (what avs_mae_loss_fwd_id wrote) where mask == 1, else 0
 * pred must be 16-byte aligned; C <= 3.  One writer per cell, no atomics: the same bytes every call. */
int avs_unpatchify(const float* pred, const void* inp, const float* mask, float* out, void* raw_out, const float* row_loss, float* err,
                   int rows, int audio, int n, int L, int C, int H, int W, int stride, const avs_input_xf* xf, const int* row_id,
                   int id_base, int* inv_ws, int paste_kept, avs_stream_t stream);

/* ---- fine-tuning augmentation where the input is read (dataloader_ft.py:527-548, training set only, per sample, in this order):
 * FrequencyMasking(freqm) and TimeMasking(timem) on the un-normalised fbank (mask value 0.0; each skipped when its parameter is 0), then
 * (fbank - norm_mean) / norm_std, then with `noise`: fbank += rand(T, F) * (rand() / 10) and roll(fbank, randint(-T, T), 0).  Noise lands on
 * masked cells too and the masks roll with the content, so for output cell (b, t, f), ts = (t - shift_b) mod T:
 *     value = (ts in [t0_b, t0_b + tn_b) or f in [f0_b, f0_b + fn_b) ? fill : x) + amp_b * U(ts * F + f, b)     (the last step one fma)
 *     x = (in[b, ts, f] - mean) * (1 / std)   kind 1, un-normalised fp32 fbank (fill is then (0 - mean) * (1 / std) for the reference's result)
 *     x = in[b, ts, f]                        kind 0, the normalised tensor (no normalisation is applied; fill as the caller says)
 * U is the Philox4x32-10 stream of avs_normalize_audio / avs_input_xf kind 1 (24-bit uniforms, counter (ts * F + f, b, 0, 0)), keyed by the plan's
 * noise key: with every mask length 0 the result is avs_input_xf kind 1 with the same shift / amp / seed, bit for bit.  The noise term is skipped
 * where amp_b == 0.  Mixup is NOT here: the reference mixes waveforms before the fbank (dataloader_ft.py:321-325), frames with a second
 * weight (:457-458) and draws the partner from the whole dataset (:400-417) - none of it is a function of a [B, T, F] batch.
 *
 * The AUGMENTATION PLAN of a step lives in device memory: one avs_ft_aug_hdr followed by hdr.n avs_ft_aug_sample records (32 bytes each).
 * A sample index at or beyond hdr.n is read as "no augmentation".  shift may be any int (taken mod T); mask ranges are clipped by the
 * comparisons themselves, so no plan content can make a kernel read out of bounds.
 *
 *  avs_ft_aug_draw       draws the plan of the next step on the device from avs_ft_aug_state {key, counter} and then advances the counter by
 *                        one (a one-thread kernel behind the draw, plain stores).  Everything that changes from step to step is in device
 *                        memory - the launch arguments are the recipe's constants - so a captured step replays.  Uniforms are the top 24
 *                        bits k of Philox words, key = the state's, counter words (b, q, state.counter, 1) for quantity q of sample b:
 *                          q 0, 1 (k1, k2): fn = (k1 * freqm) >> 24;  f0 = (k2 * ((F << 24) - k1 * freqm)) >> 48       [64-bit integers only;
 *                          q 2, 3 (k1, k2): tn = (k1 * timem) >> 24;  t0 = (k2 * ((T << 24) - k1 * timem)) >> 48        torchaudio's mask_along_axis:
 *                                                                     value = u1 * param; min = u2 * (size - value); [floor(min), floor(min) + floor(value))]
 *                          q 4: shift = ((k * 2T) >> 24) - T          q 5: amp = ((float)k / 2^24) / 10.0f  (both 0 unless `noise`)
 *                        The noise key is (Philox(counter, 0, 0, 2), Philox(counter, 1, 0, 2)) under the same key: counter word 3 keeps the
 *                        draws (1), the key derivation (2) and the noise field (0) apart.  0 <= freqm <= F, 0 <= timem <= T, T, F < 32768.
 *  avs_im2col_audio_aug  avs_im2col_audio_s (stride 1..16) with the element read replaced by the formula above
 *  avs_augment_audio     the two-pass form, [B, T, F] -> fp32 [B, T, F] as the model sees it (out of place, F % 4 == 0): what
 *                        avs_normalize_audio is to avs_input_xf; the tests compare the fused read with it
 * Bad arguments (NULL plan, kind other than 0 | 1, std == 0 for kind 1, ...) return -2 before anything is launched. */
typedef struct avs_ft_aug_state {
    unsigned key_lo, key_hi;       /* Philox key of every draw */
    int counter;                   /* draws so far */
    int pad;
} avs_ft_aug_state;
typedef struct avs_ft_aug_hdr {
    unsigned noise_lo, noise_hi;   /* Philox key of this step's noise field */
    int counter;                   /* state.counter the plan was drawn at (information) */
    int n;                         /* sample records that follow */
    int pad[4];
} avs_ft_aug_hdr;
typedef struct avs_ft_aug_sample {
    int f0, fn, t0, tn;            /* masked mel bins [f0, f0 + fn), masked frames [t0, t0 + tn) of the UN-rolled input */
    int shift;                     /* time roll */
    float amp;                     /* noise amplitude */
    int pad[2];
} avs_ft_aug_sample;
int avs_ft_aug_draw(avs_ft_aug_state* state, avs_ft_aug_hdr* plan, int B, int T, int F, int freqm, int timem, int noise, avs_stream_t stream);
int avs_im2col_audio_aug(const float* a, const int* row_b, const int* row_tok, avs_bf16* out, int rows, int tlen, int mel, int t_patches,
                         int stride, const avs_ft_aug_hdr* plan, int kind, float mean, float std, float fill, avs_stream_t stream);
int avs_augment_audio(const float* in, float* out, int B, int T, int F, const avs_ft_aug_hdr* plan, int kind, float mean, float std,
                      float fill, avs_stream_t stream);


/* ---- bidirectional InfoNCE (forward_contrastive, cav_mae_base.py:641-661) */
int avs_l2norm_fwd(const float* x, float* xn, float* norm, int rows, int D, avs_stream_t stream);
int avs_l2norm_bwd(const float* dxn, const float* xn, const float* norm, float* dx, int rows, int D, float scale,
                   avs_stream_t stream);
int avs_gemm_f32_small(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, float* C,
                       long long scm, int M, int N, int K, float alpha, avs_stream_t stream);
/* out = {nce, c_acc, weight * nce} */
int avs_infonce_fwd(const float* total, float* stats, float* out, int N, float weight, avs_stream_t stream);
int avs_infonce_dlogits(const float* total, const float* stats, const float* gout, float weight, float* dtotal, int N,
                        avs_stream_t stream);

/* ---- retrieval evaluation: similarity -> rank of the true match, ties, top-K, in one streaming pass (get_sim_mat + compute_metrics,
 * src/retrieval.py:32-52; there a Python double loop of numpy.dot over an N x N matrix that is then sorted row by row).
 * q [nq, D] / ldq, g [ng, D] / ldg fp32 (L2-normalised or not: the kernel does not care).  s[i][j] = sum_k q[i][k] g[j][k] in fp32 on the
 * f32-input matrix cores, ONE accumulator chain per element with k ascending and no split-K: (i, j) has one value however the grid is cut.
 *   target [nq] (may be NULL = identity, needs nq <= ng): gallery index of each query's true match.  A value outside 0..ng-1 is not read:
 *       that row gets target_sim = NaN, rank = ties = 0
 *   rank[i]  = #{ j != target[i] : s[i][j] >  s[i][target[i]] }   (j == target[i] is excluded by index, never by comparing values)
 *   ties[i]  = #{ j != target[i] : s[i][j] == s[i][target[i]] }   (may be NULL)
 *   target_sim[i] = s[i][target[i]], bitwise the value the tile loop sees for that element (may be NULL)
 *       On tie-free input rank is exactly compute_metrics' `ind`; with ties the reference emits one entry per tied column (len(ind) > N) -
 *       here the optimistic rank and the tie count are reported instead
 *   topk in 0..16: topk_idx / topk_sim [nq, topk] = the best gallery entries of row i ordered by (similarity descending, index ascending);
 *       slots beyond ng hold index -1 / -inf.  Both NULL when topk == 0
 *   sim / ldsim: optional full [nq, ng] output (NULL: the matrix is never materialised)
 *   ws: avs_retrieval_rank_ws_bytes(nq, ng, topk) bytes, O(nq * segments * topk), never O(nq * ng).  Counts are integer atomics and the
 *       top-K order is total: two calls give identical bytes.  Argument errors return -2 before any launch. */
int avs_retrieval_rank(const float* q, long long ldq, int nq, const float* g, long long ldg, int ng, int D, const int* target, int* rank,
                       int* ties, float* target_sim, int topk, int* topk_idx, float* topk_sim, float* sim, long long ldsim, void* ws,
                       size_t ws_bytes, avs_stream_t stream);
size_t avs_retrieval_rank_ws_bytes(int nq, int ng, int topk);

/* ---- classification loss of the fine-tuning loop (src/traintest_ft_base.py:105-110 loss_fn, :156-160 applied to out / out_a / out_v, the
 * backward of :171).  logits x [n, L] (row stride ldx: the head's output buffer is padded), targets y [n, L] (ldy).
 * kind 0: nn.BCEWithLogitsLoss() - mean over n * L of max(x,0) - x y + log1p(exp(-|x|)), d/dx = (sigmoid(x) - y) / (n L)
 * kind 1: nn.CrossEntropyLoss() with probability targets - mean over n of sum_j y_j (logsumexp(x) - x_j), d/dx = (softmax(x) sum_j y_j - y) / n
 * loss[0] = weight * mean loss (device scalar, no host sync): per-row sums into row_loss [n], then ONE ordered single-block sum (no float
 * atomics: the same bits every run).  dx (may be NULL) [n, L] (ldd) = gout[0] * weight * d(mean loss)/dx; gout (device, may be NULL = 1). */
int avs_cls_loss(const float* x, long long ldx, const float* y, long long ldy, int n, int L, int kind, const float* gout, float weight,
                 float* row_loss, float* loss, float* dx, long long ldd, avs_stream_t stream);

/* ---- classification metrics of the fine-tuning loop (src/utilities/stats.py calculate_stats: sklearn's average_precision_score and
 * roc_auc_score per class, top-1 accuracy) by integer counting, without a sort and without leaving the device.
 * scores fp32 [S, N, C]: S prediction sets that share one target (element (s, i, k) at s * set_stride + i * row_stride + k; row_stride >= C,
 * set_stride >= N * C, ignored when S == 1); target fp32 [N, C] (row stride ldt >= C); the positives of class k are target[i][k] > 0.5f.
 * Comparison is IEEE fp32 order / equality (-0 == +0, infinities are ordinary values).  Per (set, class), [S, C]:
 *   n_pos    P, the number of positives (Nn = N - P negatives)
 *   auc_num  the exact integer sum over positives i of 2 #{negatives j: s_j < s_i} + #{negatives j: s_j == s_i};   AUC = auc_num / (2 P Nn)
 *   ap_sum   fp64 sum over positives i of #{positives j: s_j >= s_i} / #{all j: s_j >= s_i};   AP = ap_sum / P - equal scores share one
 *            threshold, which is sklearn's definition.  The terms (one correctly rounded fp64 division each) are added in an order that
 *            depends on nothing but the positives' sample indices: a butterfly over chunks of 64 consecutive positives, the chunks ascending
 * Per set, [S]:
 *   n_correct    rows whose first-index argmax of the scores equals the first-index argmax of the binarised (> 0.5f) target row (numpy.argmax
 *                semantics; a target row without a positive gives class 0)
 *   n_nonfinite  NaN scores of the set.  A NaN compares false against everything: the call does not fault, the set's other outputs mean nothing
 * ws: avs_cls_stats_ws_bytes(S, N, C) bytes - the class-major copy of the scores (4 S N C) plus 5 N C for the labels and the positive
 * lists, plus O(S N C / 64); 0 for a shape the entry refuses.  No floating-point atomics: two calls give identical bytes, S sets in one call the
 * bytes of S calls.  Argument errors (N, C, S < 1, N or C > 2^22, S > 65534, a stride below the dense one, NULL, ws) return -2 before any
 * launch.  Cost: N * sum_k ceil(P_k / 64) * 64 comparisons per set. */
int avs_cls_stats(const float* scores, long long set_stride, long long row_stride, int S, int N, int C, const float* target, long long ldt,
                  int* n_pos, long long* auc_num, double* ap_sum, int* n_correct, int* n_nonfinite, void* ws, size_t ws_bytes,
                  avs_stream_t stream);
size_t avs_cls_stats_ws_bytes(int S, int N, int C);

/* ---- weights: bf16 shadow copies and the fused Adam step (torch.optim.Adam as built at
 * src/traintest_cavmae_base.py:64-66) */
int avs_transpose_bf16(const avs_bf16* in, avs_bf16* out, int R, int C, avs_stream_t stream);
/* one launch for many matrices: desc = nmat x {src, dst, R, C, first_tile, tiles_per_row} (int64), tile_map[b] = matrix of
 * workgroup b, ntiles = sum of ceil(R/64)*ceil(C/64) */
int avs_transpose_batched(const long long* desc, const int* tile_map, int ntiles, avs_stream_t stream);
int avs_cast_bf16(const float* x, avs_bf16* y, long long n, avs_stream_t stream);
int avs_adam(float* p, const float* g, float* m, float* v, avs_bf16* p_bf16, long long n, float lr, float beta1,
             float beta2, float eps, float weight_decay, int step, float grad_scale, avs_stream_t stream);
/* the same update with the step count (>= 1, the count of THIS update) read from device memory when the kernel runs - for a step
 * replayed from a captured hipGraph; bias corrections in double as above */
int avs_adam_dev(float* p, const float* g, float* m, float* v, avs_bf16* p_bf16, long long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, const int* step_dev, float grad_scale, avs_stream_t stream);
/* The same update as ONE launch over a table of arena segments, with everything that changes from step to step in device memory - for
 * data-parallel fine-tuning, where the set of gradient classes that take a step is the union over the ranks and reaches the device as an
 * all-reduced vector the host never sees.
 *   segs[n_segs]  device array; lo: element offset from p / g / m / v / p_bf16 (a multiple of 4), n: elements (a positive multiple of 4),
 *                 group 0..2 selects ctl->lr[], cls 0..15 the step count and liveness.  Segments must not overlap; gaps belong to nobody.
 *                 A segment that breaks these rules is skipped as a whole.  1 <= n_segs <= 4096.
 *   ctl           device block: lr[group]; step[c] = updates class c has HAD; live[c] > 0 = class c takes an update now.
 * For every segment of a live class: t = step[cls] + 1, bias corrections in double, gg = g * grad_scale + weight_decay * p, the bf16 shadow
 * refreshed when p_bf16 is not NULL - the bytes avs_adam(..., lr[group], step = t, ...) leaves on the same slice.  Segments of classes that
 * are not live, and the gaps, are not written.  A second, one-workgroup kernel then does step[c] += (live[c] > 0).
 * NULL p / g / m / v / segs / ctl or n_segs out of range return -2 before any launch.
 *  avs_adam_table_sized      the same with the table's chunk count (sum over the segments of ceil(n / chunk_elems), known to whoever built the
 *                            table): the grid is min(n_chunks, the geometry's grid) workgroups instead of the full grid.  n_chunks < 1: -2
 *  avs_adam_table_set_lr     ctl->lr[] <- the three rates, passed by value (safe while an earlier step is still in flight on the stream)
 *  avs_adam_table_geometry   launch geometry of the update kernel: workgroups, elements per chunk (a workgroup takes chunk blockIdx,
 *                            + grid, ...; a table of more than grid * chunk_elems elements sends workgroups round a second time),
 *                            largest n_segs.  Any pointer may be NULL. */
typedef struct avs_adam_seg {
    long long lo;
    int n, group, cls;
} avs_adam_seg;
typedef struct avs_adam_ctl {
    float lr[3];
    int step[16];
    float live[16];
} avs_adam_ctl;
int avs_adam_table(float* p, const float* g, float* m, float* v, avs_bf16* p_bf16, const avs_adam_seg* segs, int n_segs,
                   avs_adam_ctl* ctl, float beta1, float beta2, float eps, float weight_decay, float grad_scale, avs_stream_t stream);
int avs_adam_table_sized(float* p, const float* g, float* m, float* v, avs_bf16* p_bf16, const avs_adam_seg* segs, int n_segs,
                         long long n_chunks, avs_adam_ctl* ctl, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         avs_stream_t stream);
int avs_adam_table_set_lr(avs_adam_ctl* ctl, float lr_base, float lr_head, float lr_mm, avs_stream_t stream);
int avs_adam_table_geometry(int* grid, int* chunk_elems, int* max_segs);

/* ---- the guard of the fine-tuning step (csrc/grad_guard.hip): gradient norm, clipping coefficient and non-finite skip on the device, between
 * the gradients and Adam.  Semantics: torch.nn.utils.clip_grad_norm_(parameters, max_norm) - total_norm = ||g||_2 over every gradient,
 * clip_coef = clamp(max_norm / (total_norm + 1e-6), max = 1) - and the reference's scaler.step(optimizer), src/traintest_ft_base.py:115,162-165
 * (torch.cuda.amp.GradScaler: the optimizer is not called when a gradient holds inf or NaN).
 *  avs_grad_sumsq   over the table and control block of avs_adam_table, under its rules: malformed segments own nothing, segments of classes
 *                   with live[c] <= 0 and the gaps are not read.  Stage 1, one workgroup per chunk of chunk_elems elements (grid-strided, 16-byte
 *                   loads): the finite elements squared and summed in fp64, the others (!(|x| <= FLT_MAX)) counted and left out; one record per
 *                   chunk in ws, one writer.  Stage 2, one workgroup: the records added in an order fixed by the geometry, then *guard written:
 *                     sumsq[group], sumsq_cls[cls]   sums of squares of the UNSCALED gradients per lr group and per class
 *                     total        sumsq[0] + sumsq[1] + sumsq[2], in that order
 *                     norm         (float)(sqrt(total) * (double)grad_scale): the norm of the gradients Adam applies
 *                     n_nonfinite  elements left out; -1: the table has more chunks than ws holds (nothing was written past ws; skip is set)
 *                     skip         n_nonfinite != 0
 *                     coef         skip ? 0 : fminf(1.0f, max_norm / (norm + 1e-6f)), in fp32; max_norm = +inf gives exactly 1.0f
 *                     n_skipped += skip, n_steps += 1   cumulative: zero the block once, before its first use
 *                   No floating-point atomics: two calls give identical bytes.  ws: avs_grad_sumsq_ws_bytes(n_segs, n_chunks) bytes, n_chunks the
 *                   table's chunk count (avs_adam_table_sized); 16-byte aligned, as g.  The stage-1 grid is min(records ws holds, the geometry's grid).
 *                   NULL g / segs / ctl / guard / ws, n_segs out of range, max_norm not > 0, a non-finite grad_scale, ws_bytes below one record:
 *                   -2 before any launch.  avs_grad_sumsq_ws_bytes: 0 for arguments out of range.
 *  avs_adam_table_guarded   avs_adam_table_sized with the block avs_grad_sumsq wrote: every workgroup reads guard->skip and guard->coef once.
 *                   skip: nothing is written - not p, m, v or p_bf16 - and the step-count kernel leaves ctl->step alone.  Otherwise the update
 *                   with the gradient scale grad_scale * coef (one fp32 multiply): the bytes avs_adam_table_sized leaves when it is given that
 *                   product as its grad_scale.  NULL guard: -2. */
typedef struct avs_grad_guard {
    double sumsq[3];
    double sumsq_cls[16];
    double total;
    float norm, coef;
    int n_nonfinite, skip, n_skipped, n_steps;
} avs_grad_guard;
int avs_grad_sumsq(const float* g, const avs_adam_seg* segs, int n_segs, const avs_adam_ctl* ctl, float grad_scale, float max_norm,
                   avs_grad_guard* guard, void* ws, size_t ws_bytes, avs_stream_t stream);
size_t avs_grad_sumsq_ws_bytes(int n_segs, long long n_chunks);
int avs_adam_table_guarded(float* p, const float* g, float* m, float* v, avs_bf16* p_bf16, const avs_adam_seg* segs, int n_segs,
                           long long n_chunks, avs_adam_ctl* ctl, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                           const avs_grad_guard* guard, avs_stream_t stream);

/* ---- gradient accumulation over micro-batches (csrc/grad_accum.hip): acc (+)= g over the table and control block of avs_adam_table, and the
 * union of the gradient classes the micro-steps of a cycle reached - on the device, where alone that set is known (data parallel: the
 * all-reduced ctl->live; mm_grad: a branch per micro-step).  The table rules are avs_adam_table's, the geometry avs_adam_table_sized's:
 * malformed segments own nothing, gaps belong to nobody, a chunk of a class with ctl->live[c] <= 0 is skipped before any of its memory is
 * touched.  acc and g share the table's element offsets; 16-byte aligned.
 *  kernel 1  for a chunk of a class that is live now:
 *              first != 0, or actl->live[c] <= 0 (the class's first touch in this cycle):  acc = g, a copy - -0.0 and every bit survive, so
 *                        acc never needs a zero-fill and a cycle of one micro-step hands Adam the bytes of g
 *              otherwise:  acc = acc + g, one fp32 add per element; inf and NaN propagate by the add (what lets avs_grad_sumsq skip a whole
 *                        accumulated step)
 *            16-byte loads and stores, one writer per element, no atomics: two call sequences give identical bytes.
 *  kernel 2  one workgroup, behind the first in stream order (the first reads both blocks).  For the 16 classes, with
 *            had = first == 0 && actl->live[c] > 0 and now = ctl->live[c] > 0:  actl->live[c] = (had || now) ? 1 : 0;
 *            n_micro = first ? 1 : n_micro + 1; with publish != 0 additionally ctl->live[c] = actl->live[c] and n_cycles += 1 - the
 *            avs_grad_sumsq / avs_adam_table that follow see the union of the cycle.  ctl->lr and ctl->step are never written.
 * Zero the block once, before its first use.  NULL acc / g / segs / ctl / actl, acc == g, n_segs outside 1..4096, n_chunks < 1 (or a
 * misaligned acc / g): -2 before any launch. */
typedef struct avs_grad_accum_ctl {
    float live[16];
    int n_micro;
    int n_cycles;
} avs_grad_accum_ctl;
int avs_grad_accum(float* acc, const float* g, const avs_adam_seg* segs, int n_segs, long long n_chunks, avs_adam_ctl* ctl,
                   avs_grad_accum_ctl* actl, int first, int publish, avs_stream_t stream);

/* ---- Exact-fp32 forward (csrc/exact.hip; engine_exact.py): the inference forms of the fine-tuned model with fp32 operands on the f32-input
 * MFMA.  No atomics, no split-K, no shape-dependent accumulation order, no fast-math intrinsics: an output row depends on nothing but its own
 * inputs, and two calls give the same bytes.
 *  avs_gemm_nt_f32   out[M,N] = act(alpha * (A[M,K] . B[N,K]^T + bias + res[res_idx])); every operand fp32 with a leading dimension in
 *                    elements (lda, ldb multiples of 4, A and B 16-byte aligned); bias / res / res_idx may be NULL (res_idx needs res);
 *                    act 0 none | 1 exact GELU 0.5 x (1 + erff(x / sqrt 2)); any M, N >= 1; K % 32 == 0 (else -2).  Element (m, n): per
 *                    32-wide K-slab one k-ordered fmaf chain, the slab sums added to one running total in ascending slab order.
 *  avs_attn_fwd_f32  varlen softmax attention over packed fp32 qkv [rows, 3 D] (q UNscaled: hd^-0.5 is applied to the fp32 scores), tile
 *                    tables (start, len, q0) as avs_attn_fwd, tile_rows 64 | 128, head dim 32 | 64 | 80 (else -2), out fp32 [rows, D].
 *                    One workgroup per (tile, head); online softmax over 64-key tiles in ascending order.
 *  avs_im2col_*_f32  the patch gathers of avs_im2col_*_s with fp32 rows out (stride 1..16, the same tables and input transforms) */
int avs_gemm_nt_f32(const float* A, long long lda, const float* B, long long ldb, int M, int N, int K, const float* bias, const float* res,
                    long long ldr, const int* res_idx, float* out, long long ldo, float alpha, int act, avs_stream_t stream);
int avs_attn_fwd_f32(const float* qkv, long long ldq, int D, int H, const int* t_start, const int* t_len, const int* t_q0, int ntiles,
                     int tile_rows, float* out, long long ldo, avs_stream_t stream);
int avs_im2col_audio_f32(const float* a, const int* row_b, const int* row_tok, float* out, int rows, int tlen, int mel, int t_patches,
                         int stride, const avs_input_xf* xf, avs_stream_t stream);
int avs_im2col_video_f32(const void* v, const int* row_img, const int* row_tok, float* out, int rows, int C, int H, int W, int stride,
                         const avs_input_xf* xf, avs_stream_t stream);

/* ---- Collectives of the data-parallel path: thin wrappers over RCCL on a stream of the communicator's own, with event hand-off
 * (SURVEY.md 8(b)).  Replace, on the data path, torch.distributed's all_gather / all_reduce in GatherLayer
 * (src/models/gather_layer.py:21-37) and DistributedDataParallel's bucketed gradient all-reduce
 * (src/traintest_cavmae_base.py:58-59).  RCCL is resolved at run time (the copy PyTorch loaded, else the system's).
 *  avs_comm_unique_id  rank 0: the 128-byte rendezvous id, to be handed to the other ranks over any host channel
 *  avs_comm_init       collective over all ranks (returns when every rank has called it); uses the current device
 *  avs_allreduce       buf[count] <- SUM over ranks, in place          dtype 0 = fp32, 1 = bf16
 *  avs_allgather       out[world * count] <- every rank's in[count], rank-major
 *  avs_reducescatter   out[count] <- SUM over ranks of their in[rank * count ...]
 *     each is ordered behind the work already queued on `after`, runs on the communicator's stream and returns at once
 *  avs_comm_wait       `stream` waits on the device for every collective issued so far */
int avs_comm_unique_id(void* id128);
int avs_comm_init(const void* id128, int rank, int world, void** comm);
int avs_comm_destroy(void* comm);
int avs_comm_rank(void* comm);
int avs_comm_world(void* comm);
int avs_allreduce(void* comm, void* buf, unsigned long long count, int dtype, avs_stream_t after);
int avs_allgather(void* comm, const void* in, void* out, unsigned long long count, int dtype, avs_stream_t after);
int avs_reducescatter(void* comm, const void* in, void* out, unsigned long long count, int dtype, avs_stream_t after);
int avs_comm_wait(void* comm, avs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
