// Classification metrics of the fine-tuning loop (the reference's utilities/stats.py calculate_stats: sklearn's average_precision_score,
// roc_auc_score and the top-1 accuracy) as integer counting, without a sort.  For class k with positives {i : target[i][k] > 0.5}:
//   AP_k  = (1 / P) sum over positives i of TP(s >= s_i) / CNT(s >= s_i)              (equal scores share one threshold, as in sklearn)
//   AUC_k = sum over positives i of (2 #neg(s < s_i) + #neg(s == s_i)) / (2 P Nn)
// Everything under the sums is an integer count of IEEE fp32 comparisons (-0 == +0, infinities are ordinary values), so the counts do not
// depend on any order; the one floating-point sum (the fp64 terms tp / cnt of AP) runs in an order fixed by CS_PPW alone: a butterfly over the
// 64 positives of a chunk, then the chunks of a class in ascending order.  No floating-point atomics; two calls give identical bytes, and
// a call with S sets gives the bytes of S calls with one.
//
// Schedule:
//   cls_transpose_kernel  scores [S][N][C] -> class-major scT [S][C][N], target -> one byte per (class, sample)  (64 x 64 tiles through LDS)
//   cls_argmax_kernel     one wave per sample: first-index argmax of the target row and of every set's score row, NaN count
//   cls_poslist_kernel    one workgroup per class: its positives' sample indices in ascending order (ballot compaction), P_k
//   cls_chunks_kernel     one workgroup: prefix sum of ceil(P_k / CS_PPW) over the classes and the chunk -> class map
//   cls_count_kernel      one workgroup per (set, chunk of CS_PPW positives), grid-strided over the chunks: the class's N scores stream
//                         through LDS in tiles of CS_TILE as pairs {s_j, positive ? s_j : NaN}; lane l of each of the 4 waves holds positive
//                         l's score in a register and counts cnt_ge, tp_ge, cnt_gt, tp_gt over its wave's quarter of the tile (two compares
//                         against s_j, two against the NaN-masked copy - a NaN compares false, so no label logic in the loop); the four
//                         waves' counters meet in LDS.  Every chunk streams the same N entries: no imbalance between a class with one
//                         positive and one with thousands, which only differ in their number of chunks.
//   cls_finish_kernel     one thread per (set, class): chunk partials in ascending order
#include "common.h"
#include <math.h>

#define CS_TILE 2048                               // score tile length (entries of a class staged in LDS at a time)
#define CS_PPW 64                                  // positives per workgroup (one per lane; the 4 waves split the tile)
#define CS_SEG (CS_TILE / 4)                       // tile entries per wave
#define CS_MAX_N (1 << 22)
#define CS_MAX_C (1 << 22)
#define CS_MAX_S 65534

static size_t cs_align(size_t b) { return (b + 255) & ~(size_t)255; }

// upper bound of sum_k ceil(P_k / CS_PPW) over every target: one partly filled chunk per class plus the full ones
static long long cs_max_chunks(int N, int C) { return (long long)C + (long long)N * C / CS_PPW; }

struct CsLayout {
    size_t scT, labT, pos_idx, n_posk, chunk_start, chunk_class, part_ap, part_auc, total;
};

static CsLayout cs_layout(int S, int N, int C) {
    CsLayout L;
    const size_t nc = (size_t)N * C, mc = (size_t)cs_max_chunks(N, C);
    size_t o = 0;
    L.scT = o;         o += cs_align((size_t)S * nc * 4);
    L.labT = o;        o += cs_align(nc);
    L.pos_idx = o;     o += cs_align(nc * 4);
    L.n_posk = o;      o += cs_align((size_t)C * 4);
    L.chunk_start = o; o += cs_align(((size_t)C + 1) * 4);
    L.chunk_class = o; o += cs_align(mc * 4);
    L.part_ap = o;     o += cs_align((size_t)S * mc * 8);
    L.part_auc = o;    o += cs_align((size_t)S * mc * 8);
    L.total = o;
    return L;
}

// z < S: set z of the scores; z == S: the target, as one byte per entry
__global__ __launch_bounds__(256) void cls_transpose_kernel(const float* __restrict__ scores, long long set_stride, long long row_stride, int S,
                                                            int N, int C, const float* __restrict__ target, long long ldt,
                                                            float* __restrict__ scT, unsigned char* __restrict__ labT) {
    __shared__ float tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 64, k0 = blockIdx.y * 64, z = blockIdx.z;
    const bool lab = z == S;
    const float* src = lab ? target : scores + (size_t)z * set_stride;
    const long long ld = lab ? ldt : row_stride;
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) {
        const int i = i0 + r, k = k0 + tx;
        if (i < N && k < C) tile[r][tx] = src[(size_t)i * ld + k];
    }
    __syncthreads();
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, i = i0 + tx;
        if (i < N && k < C) {
            const float v = tile[tx][r];
            if (lab) labT[(size_t)k * N + i] = v > 0.5f ? 1 : 0;
            else scT[((size_t)z * C + k) * N + i] = v;
        }
    }
}

// (value, index) of a first-index argmax: is (v1, i1) ahead of (v2, i2)?
__device__ __forceinline__ bool cs_ahead(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

__device__ __forceinline__ int cs_wave_argmax(float v, int idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (oi >= 0 && (idx < 0 || cs_ahead(ov, oi, v, idx))) { v = ov; idx = oi; }
    }
    return idx;
}

// one wave per sample.  The target row is binarised (> 0.5) first, as calculate_stats does: its argmax is the first positive class, 0 when
// the row has none.  A NaN score is counted and never wins the argmax (a set with any NaN is refused by the host).
__global__ __launch_bounds__(256) void cls_argmax_kernel(const float* __restrict__ scores, long long set_stride, long long row_stride, int S,
                                                         int N, int C, const float* __restrict__ target, long long ldt,
                                                         int* __restrict__ n_correct, int* __restrict__ n_nonfinite) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* trow = target + (size_t)i * ldt;
    float bv = -INFINITY;
    int bi = -1;
    for (int k = lane; k < C; k += 64) {
        const float v = trow[k] > 0.5f ? 1.f : 0.f;
        if (bi < 0 || v > bv) { bv = v; bi = k; }
    }
    const int targ = cs_wave_argmax(bv, bi);
    for (int s = 0; s < S; ++s) {
        const float* row = scores + (size_t)s * set_stride + (size_t)i * row_stride;
        float v0 = -INFINITY;
        int b = -1, nan = 0;
        for (int k = lane; k < C; k += 64) {
            const float v = row[k];
            nan += v != v;
            if (v == v && (b < 0 || v > v0)) { v0 = v; b = k; }
        }
        int am = cs_wave_argmax(v0, b);
        if (am < 0) am = 0;                                                       // an all-NaN row
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nan += __shfl_xor(nan, o, 64);
        if (lane == 0) {
            if (am == targ) atomicAdd(n_correct + s, 1);
            if (nan) atomicAdd(n_nonfinite + s, nan);
        }
    }
}

__global__ __launch_bounds__(256) void cls_poslist_kernel(const unsigned char* __restrict__ labT, int N, int* __restrict__ pos_idx,
                                                          int* __restrict__ n_posk) {
    __shared__ int wcount[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char* lab = labT + (size_t)k * N;
    int* out = pos_idx + (size_t)k * N;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + tid;
        const bool y = i < N && lab[i];
        const unsigned long long m = __ballot(y);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += wcount[w];
        if (y) out[before + __popcll(m & ((1ull << lane) - 1))] = i;               // before + rank < P_k <= N: inside the class's slab
        base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (tid == 0) n_posk[k] = base;
}

__global__ __launch_bounds__(256) void cls_chunks_kernel(const int* __restrict__ n_posk, int C, int* __restrict__ chunk_start,
                                                         int* __restrict__ chunk_class) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const int per = (C + 255) / 256;
    const int k0 = min(C, tid * per), k1 = min(C, k0 + per);
    int sum = 0;
    for (int k = k0; k < k1; ++k) sum += (n_posk[k] + CS_PPW - 1) / CS_PPW;
    part[tid] = sum;
    __syncthreads();
    int start = 0;
    for (int t = 0; t < tid; ++t) start += part[t];
    for (int k = k0; k < k1; ++k) {
        const int n = (n_posk[k] + CS_PPW - 1) / CS_PPW;
        chunk_start[k] = start;
        for (int c = 0; c < n; ++c) chunk_class[start + c] = k;                    // start + c < sum_k ceil(P_k / CS_PPW) <= cs_max_chunks
        start += n;
    }
    if (tid == 255) chunk_start[C] = start;                                        // (thread 255's range ends at C, or is empty behind it)
}

__global__ __launch_bounds__(256) void cls_count_kernel(const float* __restrict__ scT, const unsigned char* __restrict__ labT,
                                                        const int* __restrict__ pos_idx, const int* __restrict__ n_posk,
                                                        const int* __restrict__ chunk_start, const int* __restrict__ chunk_class, int N, int C,
                                                        long long max_chunks, double* __restrict__ part_ap, long long* __restrict__ part_auc) {
    __shared__ __attribute__((aligned(16))) f32x2 tile[CS_TILE];                    // {s_j, positive ? s_j : NaN}
    __shared__ int cnt[4][4][64];                                                  // [counter][wave][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const int total = chunk_start[C];
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int k = chunk_class[w];
        const int P = n_posk[k];
        const int p = (w - chunk_start[k]) * CS_PPW + lane;
        const float* sc = scT + ((size_t)s * C + k) * N;
        const unsigned char* lab = labT + (size_t)k * N;
        const float sp = p < P ? sc[pos_idx[(size_t)k * N + p]] : NAN;             // an idle lane compares false against everything
        int cnt_ge = 0, tp_ge = 0, cnt_gt = 0, tp_gt = 0;
        for (int t0 = 0; t0 < N; t0 += CS_TILE) {
            __syncthreads();                                                       // the previous tile (or chunk) is consumed
#pragma unroll
            for (int e = 0; e < CS_TILE / 256; ++e) {
                const int jl = tid + 256 * e, j = t0 + jl;
                f32x2 v = {NAN, NAN};
                if (j < N) {
                    v[0] = sc[j];
                    if (lab[j]) v[1] = v[0];
                }
                tile[jl] = v;
            }
            __syncthreads();
            int lim = min(CS_SEG, N - t0 - wave * CS_SEG);                         // this wave's entries of the tile (the tail is NaN-padded)
            lim = (lim + 1) & ~1;
            const f32x4* seg = reinterpret_cast<const f32x4*>(tile + wave * CS_SEG);
            for (int j = 0; j < lim; j += 2) {
                const f32x4 v = seg[j >> 1];
                cnt_ge += v[0] >= sp; tp_ge += v[1] >= sp; cnt_gt += v[0] > sp; tp_gt += v[1] > sp;
                cnt_ge += v[2] >= sp; tp_ge += v[3] >= sp; cnt_gt += v[2] > sp; tp_gt += v[3] > sp;
            }
        }
        cnt[0][wave][lane] = cnt_ge;
        cnt[1][wave][lane] = tp_ge;
        cnt[2][wave][lane] = cnt_gt;
        cnt[3][wave][lane] = tp_gt;
        __syncthreads();
        if (wave == 0) {
            int c[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = cnt[q][0][lane] + cnt[q][1][lane] + cnt[q][2][lane] + cnt[q][3][lane];
            const bool live = p < P;
            // neg_ge = cnt_ge - tp_ge, neg_gt = cnt_gt - tp_gt: 2 neg_lt + neg_eq = 2 Nn - neg_ge - neg_gt
            long long auc = live ? 2ll * (N - P) - (c[0] - c[1]) - (c[2] - c[3]) : 0ll;
            double ap = live && c[0] > 0 ? (double)c[1] / (double)c[0] : 0.0;      // (cnt_ge == 0 only for a NaN score)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {                                     // one fixed butterfly: the same bits on every lane, every run
                ap += __shfl_xor(ap, o, 64);
                auc += __shfl_xor(auc, o, 64);
            }
            if (lane == 0) {
                part_ap[(size_t)s * max_chunks + w] = ap;
                part_auc[(size_t)s * max_chunks + w] = auc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void cls_finish_kernel(const int* __restrict__ n_posk, const int* __restrict__ chunk_start, int S, int C,
                                                         long long max_chunks, const double* __restrict__ part_ap,
                                                         const long long* __restrict__ part_auc, int* __restrict__ n_pos,
                                                         long long* __restrict__ auc_num, double* __restrict__ ap_sum) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)S * C) return;
    const int s = (int)(id / C), k = (int)(id % C);
    double ap = 0.0;
    long long auc = 0;
    for (int w = chunk_start[k]; w < chunk_start[k + 1]; ++w) {
        ap += part_ap[(size_t)s * max_chunks + w];
        auc += part_auc[(size_t)s * max_chunks + w];
    }
    n_pos[id] = n_posk[k];
    auc_num[id] = auc;
    ap_sum[id] = ap;
}

static bool cs_shape_ok(int S, int N, int C) {
    return S >= 1 && S <= CS_MAX_S && N >= 1 && N <= CS_MAX_N && C >= 1 && C <= CS_MAX_C && cs_max_chunks(N, C) < (1ll << 31);
}

extern "C" size_t avs_cls_stats_ws_bytes(int S, int N, int C) {
    if (!cs_shape_ok(S, N, C)) return 0;
    return cs_layout(S, N, C).total;
}

extern "C" int avs_cls_stats(const float* scores, long long set_stride, long long row_stride, int S, int N, int C, const float* target,
                             long long ldt, int* n_pos, long long* auc_num, double* ap_sum, int* n_correct, int* n_nonfinite, void* ws,
                             size_t ws_bytes, hipStream_t stream) {
    AVS_CHECK_ARG(S >= 1 && N >= 1 && C >= 1, "cls_stats: S, N, C must be positive (S=%d N=%d C=%d)", S, N, C);
    AVS_CHECK_ARG(N <= CS_MAX_N, "cls_stats: N = %d above %d", N, CS_MAX_N);
    AVS_CHECK_ARG(C <= CS_MAX_C, "cls_stats: C = %d above %d", C, CS_MAX_C);
    AVS_CHECK_ARG(S <= CS_MAX_S, "cls_stats: S = %d above %d", S, CS_MAX_S);
    AVS_CHECK_ARG(cs_max_chunks(N, C) < (1ll << 31), "cls_stats: N x C = %d x %d is too large (more than 2^31 chunks of %d positives)", N, C, CS_PPW);
    AVS_CHECK_ARG(scores, "cls_stats: scores is NULL");
    AVS_CHECK_ARG(target, "cls_stats: target is NULL");
    AVS_CHECK_ARG(n_pos && auc_num && ap_sum && n_correct && n_nonfinite, "cls_stats: an output is NULL");
    AVS_CHECK_ARG(row_stride >= C, "cls_stats: row_stride = %lld < C = %d", row_stride, C);
    AVS_CHECK_ARG(ldt >= C, "cls_stats: ldt = %lld < C = %d", ldt, C);
    AVS_CHECK_ARG(S == 1 || set_stride >= (long long)N * C, "cls_stats: set_stride = %lld < N * C = %lld", set_stride, (long long)N * C);
    const CsLayout L = cs_layout(S, N, C);
    AVS_CHECK_ARG(ws && ws_bytes >= L.total, "cls_stats: ws too small (%zu bytes, avs_cls_stats_ws_bytes says %zu)", ws ? ws_bytes : (size_t)0, L.total);

    char* w = static_cast<char*>(ws);
    float* scT = reinterpret_cast<float*>(w + L.scT);
    unsigned char* labT = reinterpret_cast<unsigned char*>(w + L.labT);
    int* pos_idx = reinterpret_cast<int*>(w + L.pos_idx);
    int* n_posk = reinterpret_cast<int*>(w + L.n_posk);
    int* chunk_start = reinterpret_cast<int*>(w + L.chunk_start);
    int* chunk_class = reinterpret_cast<int*>(w + L.chunk_class);
    double* part_ap = reinterpret_cast<double*>(w + L.part_ap);
    long long* part_auc = reinterpret_cast<long long*>(w + L.part_auc);
    const long long mc = cs_max_chunks(N, C);
    if (S == 1) set_stride = 0;

    if (hipMemsetAsync(n_correct, 0, (size_t)S * 4, stream) != hipSuccess || hipMemsetAsync(n_nonfinite, 0, (size_t)S * 4, stream) != hipSuccess) {
        avs_set_error("cls_stats: cannot clear the counters: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    cls_transpose_kernel<<<dim3(ceil_div(N, 64), ceil_div(C, 64), S + 1), 256, 0, stream>>>(scores, set_stride, row_stride, S, N, C, target, ldt,
                                                                                           scT, labT);
    AVS_LAUNCH_CHECK("cls_transpose");
    cls_argmax_kernel<<<ceil_div(N, 4), 256, 0, stream>>>(scores, set_stride, row_stride, S, N, C, target, ldt, n_correct, n_nonfinite);
    AVS_LAUNCH_CHECK("cls_argmax");
    cls_poslist_kernel<<<C, 256, 0, stream>>>(labT, N, pos_idx, n_posk);
    AVS_LAUNCH_CHECK("cls_poslist");
    cls_chunks_kernel<<<1, 256, 0, stream>>>(n_posk, C, chunk_start, chunk_class);
    AVS_LAUNCH_CHECK("cls_chunks");
    // the chunk count is only known on the device: a grid of up to 8 workgroups per CU strides over the chunks (every chunk costs the same)
    const long long gx = mc < 8ll * avs_persistent_slots() ? mc : 8ll * avs_persistent_slots();
    cls_count_kernel<<<dim3((unsigned)gx, S), 256, 0, stream>>>(scT, labT, pos_idx, n_posk, chunk_start, chunk_class, N, C, mc, part_ap, part_auc);
    AVS_LAUNCH_CHECK("cls_count");
    cls_finish_kernel<<<(unsigned)(((long long)S * C + 255) / 256), 256, 0, stream>>>(n_posk, chunk_start, S, C, mc, part_ap, part_auc, n_pos, auc_num,
                                                                                     ap_sum);
    AVS_LAUNCH_CHECK("cls_finish");
    return 0;
}
