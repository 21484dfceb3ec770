// Exact-fp32 forward kernels: the GEMM with the forward epilogues and the varlen softmax attention on fp32 operands, for the inference forms of
// the fine-tuned model (engine_exact.py).  They are the yardstick the bf16 path is held to, so what they promise is numerics, not speed:
//   * no atomics, no split-K, no shape-dependent accumulation order, no fast-math intrinsic (expf / erff are the device library's, the
//     softmax normaliser is applied by a division);
//   * every product sum runs on v_mfma_f32_32x32x2_f32 - f32 in, f32 accumulate; bit for bit a k-ordered fmaf chain - in an order that
//     depends on nothing but the contraction index: an output row does not depend on the other rows of the call, on the grid, or on the call.
//   * the GEMM's order, per output element: the 32 terms of a K-slab form one k-ordered chain from zero, and the slab sums are added to the
//     element's ONE running total in ascending slab order.  (A single chain over all of K was built first and measured: its rounding error
//     grows with the length of the chain - the logits of the fine-tuned model came out 5.2e-6 from the reference's golden values, three
//     times what a blocked fp32 sum gives, and 3 x that is outside the 1.2e-5 the mode has to hold.  The two-level order is as fixed as the
//     single chain, costs 64 registers and 64 additions per slab, and sits inside the same (K + 3) u bound with room to spare: no term
//     passes through more than 32 + K / 32 roundings.)
// (The fp32 patch gathers of the same path are instantiations of the bf16 path's gather kernels: elementwise.hip, avs_im2col_*_f32.)
//
// avs_gemm_nt_f32: workgroup = 128 x 128 outputs, 4 waves of 64 x 64 as 2 x 2 MFMA blocks (64 accumulator registers); K-slabs of 32 go global
//   -> registers -> LDS (rows padded to 33 floats: the 32 lanes of an operand read hit 32 banks) with the next slab's global loads in flight
//   while the current one is multiplied; rows beyond M / N are zero-filled on load and never stored.
// avs_attn_fwd_f32: workgroup = one (query tile, head); a wave owns 32 queries.  BOTH products run on the f32 MFMA, transposed so that a lane
//   owns ONE query: S^T = K Q^T (a lane's 16 accumulators are 16 keys of its query: the row maximum and sum are in-lane reductions and one
//   exchange between the two half-waves), then O^T += V^T P^T with P^T fed from those registers as they are.  Keys are walked in tiles of 64
//   (two 32-key MFMA blocks) in ascending order with the online softmax; inside a 32-key block the P.V chain takes the keys in the register
//   order 0 4 1 5 2 6 3 7 8 12 ...  (fixed).  Scores are scaled by hd^-0.5 in fp32 after the chain.  Nothing is shared between sequences.
#include "common.h"
#include <math.h>

#define EX_TILE 128
#define EX_BK 32
#define EX_LDS_K 33

__device__ __forceinline__ void ex_load_slab(const float* __restrict__ base, long long ld, int row0, int nrows, int k0, int tid, f32x4 (&r)[4]) {
    const int kq = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + (tid >> 3) + 32 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows) v = *reinterpret_cast<const f32x4*>(base + (size_t)row * ld + k0 + kq);
        r[i] = v;
    }
}

__device__ __forceinline__ void ex_store_slab(float* __restrict__ s, int tid, const f32x4 (&r)[4]) {
    const int kq = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* p = s + ((tid >> 3) + 32 * i) * EX_LDS_K + kq;
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = r[i][c];
    }
}

// nn.GELU() (erf form): 0.5 x (1 + erf(x / sqrt 2)), erff of the device library
__device__ __forceinline__ float ex_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

template <int ACT>
__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ A, long long lda, const float* __restrict__ B, long long ldb,
                                                          int M, int N, int K, const float* __restrict__ bias, const float* __restrict__ res,
                                                          long long ldr, const int* __restrict__ res_idx, float* __restrict__ out, long long ldo,
                                                          float alpha) {
    __shared__ float As[EX_TILE * EX_LDS_K];
    __shared__ float Bs[EX_TILE * EX_LDS_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, kh = lane >> 5;
    const int row0 = blockIdx.y * EX_TILE, col0 = blockIdx.x * EX_TILE;
    f32x16 acc[2][2], part[2][2];                      // running totals; the current slab's chains
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0};
    f32x4 ra[4], rb[4];
    ex_load_slab(A, lda, row0, M, 0, tid, ra);
    ex_load_slab(B, ldb, col0, N, 0, tid, rb);
    const int nslab = K / EX_BK;
    for (int s = 0; s < nslab; ++s) {
        __syncthreads();                                   // the previous slab has been read
        ex_store_slab(As, tid, ra);
        ex_store_slab(Bs, tid, rb);
        __syncthreads();
        if (s + 1 < nslab) {
            ex_load_slab(A, lda, row0, M, (s + 1) * EX_BK, tid, ra);
            ex_load_slab(B, ldb, col0, N, (s + 1) * EX_BK, tid, rb);
        }
        const float* ap = As + (wr * 64 + l31) * EX_LDS_K + kh;
        const float* bp = Bs + (wc * 64 + l31) * EX_LDS_K + kh;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) part[i][j] = f32x16{0};
#pragma unroll
        for (int kk = 0; kk < EX_BK; kk += 2) {
            const float a0 = ap[kk], a1 = ap[32 * EX_LDS_K + kk];
            const float b0 = bp[kk], b1 = bp[32 * EX_LDS_K + kk];
            part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, part[0][0], 0, 0, 0);
            part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, part[0][1], 0, 0, 0);
            part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, part[1][0], 0, 0, 0);
            part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, part[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];       // slab sums in ascending slab order
    }
    // epilogue, per element: ((acc + bias) + res) * alpha, then GELU - three fp32 operations and the activation
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + wc * 64 + j * 32 + l31;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row >= M) continue;
                float x = acc[i][j][r] + bv;
                if (res) x += res[(size_t)(res_idx ? res_idx[row] : row) * ldr + col];
                x *= alpha;
                if (ACT) x = ex_gelu(x);
                out[(size_t)row * ldo + col] = x;
            }
    }
}

extern "C" int avs_gemm_nt_f32(const float* A, long long lda, const float* B, long long ldb, int M, int N, int K, const float* bias,
                               const float* res, long long ldr, const int* res_idx, float* out, long long ldo, float alpha, int act,
                               hipStream_t stream) {
    AVS_CHECK_ARG(A && B && out, "gemm_nt_f32: null operand");
    AVS_CHECK_ARG(M >= 1 && N >= 1 && K >= EX_BK, "gemm_nt_f32: bad shape M=%d N=%d K=%d", M, N, K);
    AVS_CHECK_ARG(K % EX_BK == 0, "gemm_nt_f32: K=%d is not a multiple of %d", K, EX_BK);
    AVS_CHECK_ARG(act == 0 || act == 1, "gemm_nt_f32: act must be 0 or 1, got %d", act);
    AVS_CHECK_ARG(lda >= K && ldb >= K && ldo >= N && (lda % 4) == 0 && (ldb % 4) == 0, "gemm_nt_f32: leading dimensions lda=%lld ldb=%lld ldo=%lld (lda, ldb >= K and multiples of 4; ldo >= N)", lda, ldb, ldo);
    AVS_CHECK_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "gemm_nt_f32: A and B must be 16-byte aligned");
    AVS_CHECK_ARG(!res || ldr >= N, "gemm_nt_f32: ldr=%lld < N", ldr);
    AVS_CHECK_ARG(!res_idx || res, "gemm_nt_f32: res_idx without res");
    dim3 grid(ceil_div(N, EX_TILE), ceil_div(M, EX_TILE)), block(256);
    AVS_CHECK_ARG(grid.y <= 65535, "gemm_nt_f32: M=%d too large", M);
    if (act) gemm_nt_f32_kernel<1><<<grid, block, 0, stream>>>(A, lda, B, ldb, M, N, K, bias, res, ldr, res_idx, out, ldo, alpha);
    else gemm_nt_f32_kernel<0><<<grid, block, 0, stream>>>(A, lda, B, ldb, M, N, K, bias, res, ldr, res_idx, out, ldo, alpha);
    AVS_LAUNCH_CHECK("gemm_nt_f32");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
#define EXA_KT 64                                  // keys per staged tile (two 32-key MFMA blocks)

// HD: head dim; threads = 2 * tile_rows (a wave per 32 queries).  LDS: K tile [64][HD + 1], V tile [64][HDP + 1] with HDP = HD rounded up to
// 32 (the columns beyond HD are zero: whole 32-wide MFMA blocks of O^T, of which only HD rows are stored).
template <int HD>
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ qkv, long long ldq, int D, const int* __restrict__ t_start,
                                                           const int* __restrict__ t_len, const int* __restrict__ t_q0, float* __restrict__ out,
                                                           long long ldo, float scale) {
    constexpr int HDP = (HD + 31) / 32 * 32, ND = HDP / 32, LK = HD + 1, LV = HDP + 1;
    __shared__ float Ks[EXA_KT * LK];
    __shared__ float Vs[EXA_KT * LV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int tile = blockIdx.x, h = blockIdx.y;
    const int start = t_start[tile], L = t_len[tile], q0 = t_q0[tile] + wave * 32;
    const bool wave_live = q0 < L;                     // (a wave without queries still stages keys and meets the barriers)
    const int qi = q0 + l31;
    const bool qv = qi < L;
    const float* kbase = qkv + (size_t)start * ldq + D + h * HD;
    const float* vbase = kbase + D;

    // this lane's query, the k-th pair element: B[k = kh + 2 i][col = l31]
    float qreg[HD / 2];
    {
        const float* qp = qkv + (size_t)(start + (qv ? qi : 0)) * ldq + h * HD + kh;
#pragma unroll
        for (int i = 0; i < HD / 2; ++i) qreg[i] = qv ? qp[2 * i] : 0.f;
    }
    f32x16 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = f32x16{0};
    float m = -INFINITY, l = 0.f;

    for (int j0 = 0; j0 < L; j0 += EXA_KT) {
        __syncthreads();                               // the previous tile has been read
        for (int e = tid; e < EXA_KT * (HD / 4); e += blockDim.x) {
            const int r = e / (HD / 4), c = (e - r * (HD / 4)) * 4;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < L) {
                kv = *reinterpret_cast<const f32x4*>(kbase + (size_t)(j0 + r) * ldq + c);
                vv = *reinterpret_cast<const f32x4*>(vbase + (size_t)(j0 + r) * ldq + c);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Ks[r * LK + c + i] = kv[i];
                Vs[r * LV + c + i] = vv[i];
            }
        }
        if (HDP > HD)
            for (int e = tid; e < EXA_KT * (HDP - HD); e += blockDim.x) {
                const int r = e / (HDP - HD), c = HD + e - r * (HDP - HD);
                Vs[r * LV + c] = 0.f;
            }
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll
        for (int jb = 0; jb < EXA_KT; jb += 32) {
            if (j0 + jb >= L) break;
            // S^T block: rows = 32 keys, column = this lane's query
            f32x16 s = f32x16{0};
            const float* kp = Ks + (jb + l31) * LK + kh;
#pragma unroll
            for (int i = 0; i < HD / 2; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * i], qreg[i], s, 0, 0, 0);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = j0 + jb + (r & 3) + 8 * (r >> 2) + 4 * kh;
                s[r] = key < L ? s[r] * scale : -INFINITY;
                tmax = fmaxf(tmax, s[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mn = fmaxf(m, tmax);           // finite: the first block of a sequence holds key 0
            const float corr = expf(m - mn);           // m = -inf at the first block: 0
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = expf(s[r] - mn);
                psum += s[r];
            }
            psum += __shfl_xor(psum, 32, 64);          // a + b in both halves: the same bits
            l = l * corr + psum;
            m = mn;
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[d][r] *= corr;
            // O^T += V^T P^T: step r contracts keys (r&3) + 8 (r>>2) [half 0] and that + 4 [half 1] - the registers as they are
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* vp = Vs + (jb + (r & 3) + 8 * (r >> 2) + 4 * kh) * LV + l31;
#pragma unroll
                for (int d = 0; d < ND; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * d], s[r], o[d], 0, 0, 0);
            }
        }
    }
    if (!qv) return;
    float* op = out + (size_t)(start + qi) * ldo + h * HD;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = d * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (c < HD) op[c] = o[d][r] / l;
        }
}

extern "C" int avs_attn_fwd_f32(const float* qkv, long long ldq, int D, int H, const int* t_start, const int* t_len, const int* t_q0,
                                int ntiles, int tile_rows, float* out, long long ldo, hipStream_t stream) {
    AVS_CHECK_ARG(qkv && t_start && t_len && t_q0 && out, "attn_fwd_f32: null argument");
    AVS_CHECK_ARG(ntiles > 0 && H > 0 && D > 0 && D % H == 0, "attn_fwd_f32: bad shape ntiles=%d D=%d H=%d", ntiles, D, H);
    AVS_CHECK_ARG(tile_rows == 64 || tile_rows == 128, "attn_fwd_f32: tile_rows must be 64 or 128, got %d", tile_rows);
    const int hd = D / H;
    AVS_CHECK_ARG(hd == 32 || hd == 64 || hd == 80, "attn_fwd_f32: head dim %d not supported (32, 64, 80)", hd);
    AVS_CHECK_ARG(ldq >= 3LL * D && ldo >= D && (ldq % 4) == 0 && ((uintptr_t)qkv % 16) == 0, "attn_fwd_f32: ldq=%lld ldo=%lld (ldq >= 3 D, a multiple of 4, qkv 16-byte aligned; ldo >= D)", ldq, ldo);
    AVS_CHECK_ARG(H <= 65535, "attn_fwd_f32: too many heads");
    dim3 grid(ntiles, H), block(2 * tile_rows);
    const float scale = (float)(1.0 / sqrt((double)hd));         // hd^-0.5 rounded once
    if (hd == 32) attn_fwd_f32_kernel<32><<<grid, block, 0, stream>>>(qkv, ldq, D, t_start, t_len, t_q0, out, ldo, scale);
    else if (hd == 64) attn_fwd_f32_kernel<64><<<grid, block, 0, stream>>>(qkv, ldq, D, t_start, t_len, t_q0, out, ldo, scale);
    else attn_fwd_f32_kernel<80><<<grid, block, 0, stream>>>(qkv, ldq, D, t_start, t_len, t_q0, out, ldo, scale);
    AVS_LAUNCH_CHECK("attn_fwd_f32");
    return 0;
}
