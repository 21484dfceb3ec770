// Retrieval evaluation (the reference's src/retrieval.py:32-52: get_sim_mat + compute_metrics) as ONE streaming pass: the fp32 similarity
// s[i][j] = q_i . g_j is produced tile by tile on v_mfma_f32_32x32x2_f32 and consumed on the spot - per query row the number of gallery
// entries that beat / tie its true match, and its top-K list - so the nq x ng matrix is never stored (unless the caller asks for it).
//
// Numerics: every s[i][j] is ONE accumulator chain, k ascending (an MFMA on f32 inputs is bitwise a k-ordered fmaf chain), over D rounded up
// to the 32-wide K-slab with zeros; there is no split-K, so the value of (i, j) does not depend on how the grid is cut.  The target
// similarity of a row comes from a pre-kernel that runs the SAME chain on (q_i, g_target[i]), hence the same bits the tile loop produces for
// that element (tests compare them); the comparison excludes j == target[i] by index.  Counts are integers (atomics are exact), top-K lists
// are totally ordered by (similarity descending, index ascending): two calls give identical bytes, whatever the segment count.  Inputs are
// expected to be finite: a NaN similarity neither beats nor ties anything and is left out of the top-K lists.
//
// Shape: workgroup = 128 query rows x a SEGMENT of gallery columns walked in 128-column tiles; 4 waves, each 64 x 64 of the tile as 2 x 2
// MFMA blocks (64 accumulator registers).  K-slabs of 32 go global -> registers -> LDS (rows padded to 33 floats: the 32 lanes of an operand
// read hit 32 banks), the next slab's global loads are in flight while the current one is multiplied.  Epilogue per tile: accumulators ->
// LDS, one 64-column half of the tile at a time (row stride 65), where thread t scans 32 values of row t % 128 (columns 32 (t / 128) ... of
// the half, so a thread meets its columns in ascending order): two compares per value, and an insertion
// into its own sorted top-K list (LDS, [k][thread]) only when a value beats the list's K-th.  Not tuned further: single-buffered LDS with two
// barriers per slab, element-wise slab stores (stride 33) and a partly conflicted tile spill; the measured share of the fp32 matrix peak is in
// profiles/r08/retrieval_bench.json (0.73 at N = 65 536 without top-K).
#include "common.h"
#include <math.h>

#define RT_TILE 128
#define RT_BK 32
#define RT_LDS_K 33                                // staged operand row stride (floats)
#define RT_LDS_T 65                                // epilogue half-tile (128 rows x 64 columns) row stride (floats)
#define RT_MAXK 16
#define RT_TILE_BYTES (2 * RT_TILE * RT_LDS_K * 4)  // the two staged operands; the epilogue half-tile (128 * 65 * 4) aliases them
#define RT_MAX_SEG 64

// target similarity with the chain order of the tile loop; also zeroes the counters the tile loop adds to.  One wave per 32 queries: the
// 32 x 32 MFMA block of (q rows) x (their 32 target rows of g), of which only the diagonal is kept - 32 x the necessary FLOP of a
// negligible 2 nq D, in exchange for bitwise the same arithmetic.
__global__ __launch_bounds__(256) void retr_target_kernel(const float* __restrict__ q, long long ldq, int nq, const float* __restrict__ g,
                                                          long long ldg, int ng, int D, const int* __restrict__ target,
                                                          float* __restrict__ tsim, int* __restrict__ rank, int* __restrict__ ties) {
    const int lane = threadIdx.x & 63;
    const int i = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + (lane & 31);
    const int kh = lane >> 5;
    const bool iv = i < nq;
    const int t = iv ? (target ? target[i] : i) : 0;
    const bool tv = iv && t >= 0 && t < ng;
    const float* qi = q + (size_t)(iv ? i : 0) * ldq;
    const float* gt = g + (size_t)(tv ? t : 0) * ldg;
    f32x16 acc = {0};
    const int Dp = (D + RT_BK - 1) / RT_BK * RT_BK;
    for (int k = 0; k < Dp; k += 2) {
        const int kk = k + kh;
        const float a = (iv && kk < D) ? qi[kk] : 0.f;
        const float b = (tv && kk < D) ? gt[kk] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    // element (c, c) of the block, c = lane & 31, lives in the lane whose half holds row c: register (c / 8) * 4 + c % 4
    const int c = lane & 31;
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r == (c >> 3) * 4 + (c & 3)) d = acc[r];
    if (iv && ((c >> 2) & 1) == kh) {
        tsim[i] = tv ? d : NAN;                    // a target outside the gallery: NaN, which no similarity beats or ties
        rank[i] = 0;
        ties[i] = 0;
    }
}

__device__ __forceinline__ void retr_load_slab(const float* __restrict__ base, long long ld, int row0, int nrows, int k0, int D, bool vec,
                                               int tid, f32x4 (&r)[4]) {
    const int kq = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + (tid >> 3) + 32 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows) {
            const float* p = base + (size_t)row * ld + k0 + kq;
            if (vec && k0 + RT_BK <= D) {
                v = *reinterpret_cast<const f32x4*>(p);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (k0 + kq + c < D) v[c] = p[c];
            }
        }
        r[i] = v;
    }
}

__device__ __forceinline__ void retr_store_slab(float* __restrict__ s, int tid, const f32x4 (&r)[4]) {
    const int kq = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* p = s + ((tid >> 3) + 32 * i) * RT_LDS_K + kq;
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = r[i][c];
    }
}

__global__ __launch_bounds__(256) void retr_rank_kernel(const float* __restrict__ q, long long ldq, int nq, const float* __restrict__ g,
                                                        long long ldg, int ng, int D, const int* __restrict__ target,
                                                        const float* __restrict__ tsim, int* __restrict__ rank, int* __restrict__ ties,
                                                        int topk, float* __restrict__ ws_sim, int* __restrict__ ws_idx,
                                                        float* __restrict__ sim, long long ldsim, int tiles_per_seg, int nseg, int vec) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* As = reinterpret_cast<float*>(smem);
    float* Bs = As + RT_TILE * RT_LDS_K;
    float* tile = reinterpret_cast<float*>(smem);                                  // aliases As / Bs (barriers below)
    float* lsim = reinterpret_cast<float*>(smem + RT_TILE_BYTES);                  // [topk][256]
    int* lidx = reinterpret_cast<int*>(lsim + topk * 256);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, kh = lane >> 5;
    const int row0 = blockIdx.x * RT_TILE;
    const int ntiles = (ng + RT_TILE - 1) / RT_TILE;
    const int tile_begin = blockIdx.y * tiles_per_seg;
    const int tile_end = min(ntiles, tile_begin + tiles_per_seg);

    // the scanning role of this thread: row srow of the panel, column half `half` of every tile
    const int srow = tid & 127, half = tid >> 7;
    const int grow = row0 + srow;
    const bool rvalid = grow < nq;
    const int tgt = rvalid ? (target ? target[grow] : grow) : -1;
    const float ts = rvalid ? tsim[grow] : 0.f;
    int cnt_gt = 0, cnt_eq = 0, filled = 0;
    float kth = -INFINITY;

    const int nslab = (D + RT_BK - 1) / RT_BK;
    for (int t = tile_begin; t < tile_end; ++t) {
        const int col0 = t * RT_TILE;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0};
        f32x4 ra[4], rb[4];
        retr_load_slab(q, ldq, row0, nq, 0, D, vec, tid, ra);
        retr_load_slab(g, ldg, col0, ng, 0, D, vec, tid, rb);
        for (int s = 0; s < nslab; ++s) {
            __syncthreads();                                                       // the previous slab (or the previous tile's scan) is consumed
            retr_store_slab(As, tid, ra);
            retr_store_slab(Bs, tid, rb);
            __syncthreads();
            if (s + 1 < nslab) {
                retr_load_slab(q, ldq, row0, nq, (s + 1) * RT_BK, D, vec, tid, ra);
                retr_load_slab(g, ldg, col0, ng, (s + 1) * RT_BK, D, vec, tid, rb);
            }
            const float* ap = As + (wr * 64 + l31) * RT_LDS_K + kh;
            const float* bp = Bs + (wc * 64 + l31) * RT_LDS_K + kh;
#pragma unroll
            for (int kk = 0; kk < RT_BK; kk += 2) {
                const float a0 = ap[kk], a1 = ap[32 * RT_LDS_K + kk];
                const float b0 = bp[kk], b1 = bp[32 * RT_LDS_K + kk];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (sim) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = col0 + wc * 64 + j * 32 + l31;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        if (row < nq && col < ng) sim[(size_t)row * ldsim + col] = acc[i][j][r];
                    }
                }
        }
        // the tile goes through LDS one 64-column half at a time (the waves of column half `ch` spill, everybody scans), so that the spill
        // buffer is no larger than the staged operands it aliases
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            __syncthreads();                                                       // As / Bs (ch 0) or the previous half's scan (ch 1) are done with
            if (wc == ch) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            tile[(wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * RT_LDS_T + j * 32 + l31] = acc[i][j][r];
            }
            __syncthreads();
            if (rvalid) {
                const float* trow = tile + srow * RT_LDS_T + half * 32;
                const int gc0 = col0 + ch * 64 + half * 32;
                const int ncol = min(32, ng - gc0);
                for (int c = 0; c < ncol; ++c) {
                    const float v = trow[c];
                    const int gc = gc0 + c;
                    if (gc != tgt) {
                        cnt_gt += v > ts;
                        cnt_eq += v == ts;
                    }
                    if (topk > 0 && v == v && (filled < topk || v > kth)) {       // (a NaN similarity never enters a list)
                        // sorted insertion; an equal value already in the list has the smaller index and stays ahead
                        int p = filled < topk ? filled : topk - 1;
                        while (p > 0 && lsim[(p - 1) * 256 + tid] < v) {
                            lsim[p * 256 + tid] = lsim[(p - 1) * 256 + tid];
                            lidx[p * 256 + tid] = lidx[(p - 1) * 256 + tid];
                            --p;
                        }
                        lsim[p * 256 + tid] = v;
                        lidx[p * 256 + tid] = gc;
                        if (filled < topk) ++filled;
                        if (filled == topk) kth = lsim[(topk - 1) * 256 + tid];
                    }
                }
            }
        }
    }
    if (!rvalid) return;
    if (cnt_gt) atomicAdd(rank + grow, cnt_gt);
    if (cnt_eq) atomicAdd(ties + grow, cnt_eq);
    if (topk > 0) {
        const size_t base = ((size_t)grow * (2 * nseg) + blockIdx.y * 2 + half) * topk;
        for (int p = 0; p < topk; ++p) {
            ws_sim[base + p] = p < filled ? lsim[p * 256 + tid] : -INFINITY;
            ws_idx[base + p] = p < filled ? lidx[p * 256 + tid] : -1;
        }
    }
}

// (similarity descending, index ascending): is (s1, i1) strictly ahead of (s2, i2)?
__device__ __forceinline__ bool retr_ahead(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// one wave per query row: the top-K of its ncand = 2 * nseg * topk candidates (gallery indices are unique across the lists, so the order is
// total) by K rounds of "best candidate strictly behind the previous pick".  Unfilled slots (index -1) never qualify.
__global__ __launch_bounds__(256) void retr_merge_kernel(const float* __restrict__ ws_sim, const int* __restrict__ ws_idx, int nq, int ncand,
                                                         int topk, int* __restrict__ out_idx, float* __restrict__ out_sim) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    const float* cs = ws_sim + (size_t)row * ncand;
    const int* ci = ws_idx + (size_t)row * ncand;
    float ps = INFINITY;
    int pi = -1;
    for (int r = 0; r < topk; ++r) {
        float bs = -INFINITY;
        int bi = -1;
        for (int c = lane; c < ncand; c += 64) {
            const float s = cs[c];
            const int i = ci[c];
            if (i < 0) continue;
            if (r > 0 && !retr_ahead(ps, pi, s, i)) continue;
            if (bi < 0 || retr_ahead(s, i, bs, bi)) { bs = s; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || retr_ahead(os, oi, bs, bi))) { bs = os; bi = oi; }
        }
        if (lane == 0) {
            out_idx[(size_t)row * topk + r] = bi;
            out_sim[(size_t)row * topk + r] = bi >= 0 ? bs : -INFINITY;
        }
        if (bi < 0) {                                                              // fewer than topk gallery entries: the rest stays empty
            for (int r2 = r + 1; r2 < topk && lane == 0; ++r2) {
                out_idx[(size_t)row * topk + r2] = -1;
                out_sim[(size_t)row * topk + r2] = -INFINITY;
            }
            return;
        }
        ps = bs;
        pi = bi;
    }
}

// column segments per query panel: panels x segments >= 2 x CUs where the gallery has that many tiles, one segment at gallery sizes
// ("retr_segments" knob > 0: that many, for tests).  Returned through tiles_per_seg so that no segment is empty.  Residency: LDS is
// 33 792 B + topk x 2 048 B per workgroup (66 560 B at topk = 16), so two workgroups share a 160 KB CU at every topk and one's epilogue
// and barriers overlap the other's MFMAs (tools/bench_retrieval.py times topk 0 against 16).
static int retr_segments(int nq, int ng, int* tiles_per_seg) {
    const int panels = ceil_div(nq, RT_TILE), ntiles = ceil_div(ng, RT_TILE);
    int s = avs_tuning().retr_segments;
    if (s <= 0) s = ceil_div(2 * avs_persistent_slots(), panels);
    if (s > ntiles) s = ntiles;
    if (s > RT_MAX_SEG) s = RT_MAX_SEG;
    if (s < 1) s = 1;
    const int tps = ceil_div(ntiles, s);
    if (tiles_per_seg) *tiles_per_seg = tps;
    return ceil_div(ntiles, tps);
}

static size_t retr_align(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" size_t avs_retrieval_rank_ws_bytes(int nq, int ng, int topk) {
    if (nq <= 0 || ng <= 0 || topk < 0 || topk > RT_MAXK) return 0;
    const int s = retr_segments(nq, ng, nullptr);
    return 2 * retr_align((size_t)nq * 4) + 2 * retr_align((size_t)nq * 2 * s * topk * 4);
}

extern "C" int avs_retrieval_rank(const float* q, long long ldq, int nq, const float* g, long long ldg, int ng, int D, const int* target,
                                  int* rank, int* ties, float* target_sim, int topk, int* topk_idx, float* topk_sim, float* sim,
                                  long long ldsim, void* ws, size_t ws_bytes, hipStream_t stream) {
    AVS_CHECK_ARG(nq > 0 && ng > 0 && D > 0, "retrieval_rank: nq, ng, D must be positive (nq=%d ng=%d D=%d)", nq, ng, D);
    AVS_CHECK_ARG(q, "retrieval_rank: q is NULL");
    AVS_CHECK_ARG(g, "retrieval_rank: g is NULL");
    AVS_CHECK_ARG(rank, "retrieval_rank: rank is NULL");
    AVS_CHECK_ARG(ldq >= D, "retrieval_rank: ldq = %lld < D = %d", ldq, D);
    AVS_CHECK_ARG(ldg >= D, "retrieval_rank: ldg = %lld < D = %d", ldg, D);
    AVS_CHECK_ARG(topk >= 0 && topk <= RT_MAXK, "retrieval_rank: topk = %d outside 0..%d", topk, RT_MAXK);
    AVS_CHECK_ARG(topk == 0 || (topk_idx && topk_sim), "retrieval_rank: topk = %d needs topk_idx and topk_sim", topk);
    AVS_CHECK_ARG(target || nq <= ng, "retrieval_rank: target is NULL (identity) but nq = %d > ng = %d", nq, ng);
    AVS_CHECK_ARG(!sim || ldsim >= ng, "retrieval_rank: ldsim = %lld < ng = %d", ldsim, ng);
    const size_t need = avs_retrieval_rank_ws_bytes(nq, ng, topk);
    AVS_CHECK_ARG(ws && ws_bytes >= need, "retrieval_rank: ws too small (%zu bytes, avs_retrieval_rank_ws_bytes says %zu)", ws ? ws_bytes : (size_t)0, need);

    int tps = 1;
    const int nseg = retr_segments(nq, ng, &tps);
    char* w = static_cast<char*>(ws);
    float* tsim = target_sim ? target_sim : reinterpret_cast<float*>(w);
    int* tie = ties ? ties : reinterpret_cast<int*>(w + retr_align((size_t)nq * 4));
    float* ws_sim = reinterpret_cast<float*>(w + 2 * retr_align((size_t)nq * 4));
    int* ws_idx = reinterpret_cast<int*>(w + 2 * retr_align((size_t)nq * 4) + retr_align((size_t)nq * 2 * nseg * topk * 4));

    // > 64 KB of dynamic LDS needs the attribute on every device the kernel runs on: set per call (cheap), no per-process flag
    if (hipFuncSetAttribute((const void*)retr_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RT_TILE_BYTES + RT_MAXK * 256 * 8) != hipSuccess) {
        avs_set_error("retrieval_rank: cannot reserve %d bytes of LDS", RT_TILE_BYTES + RT_MAXK * 256 * 8);
        (void)hipGetLastError();
        return -1;
    }
    retr_target_kernel<<<ceil_div(nq, 128), 256, 0, stream>>>(q, ldq, nq, g, ldg, ng, D, target, tsim, rank, tie);
    AVS_LAUNCH_CHECK("retr_target");
    // 16-byte loads of the operands where every row start is aligned; otherwise element loads (ragged leading dimensions)
    const int vec = (ldq % 4 == 0) && (ldg % 4 == 0) && ((uintptr_t)q % 16 == 0) && ((uintptr_t)g % 16 == 0);
    retr_rank_kernel<<<dim3(ceil_div(nq, RT_TILE), nseg), 256, RT_TILE_BYTES + topk * 256 * 8, stream>>>(
        q, ldq, nq, g, ldg, ng, D, target, tsim, rank, tie, topk, ws_sim, ws_idx, sim, ldsim, tps, nseg, vec);
    AVS_LAUNCH_CHECK("retr_rank");
    if (topk > 0) {
        retr_merge_kernel<<<ceil_div(nq, 4), 256, 0, stream>>>(ws_sim, ws_idx, nq, 2 * nseg * topk, topk, topk_idx, topk_sim);
        AVS_LAUNCH_CHECK("retr_merge");
    }
    return 0;
}
