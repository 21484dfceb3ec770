// k10's way back (unpatchify, /root/reference/src/models/cav_mae_base.py:353-363): prediction rows -> the [B, T, F] spectrogram and the
// [N, C, H, W] frames the model was shown, with the kept patches (mask 0) and the cells no patch covers taken from the input.
#include "common.h"

// Inverse of the index arithmetic of mae_target (losses.hip).  Both modalities are one picture problem: a [n][C][H][W] tensor cut into S x S
// patches at (rp, cp) = (row patch, column patch);
//   audio (C = 1, H = time, W = mel):  token l = cp * G + rp (G = time patches),   element e = co * 16 + ro
//   frames:                            token l = rp * G + cp (G = column patches), element e = (ro * 16 + co) * C + c
// with (ro, co) < S the cell's offsets inside the patch.  Prediction rows are contiguous per token and output rows are contiguous along W, so
// for audio this is a 16 x 16 transpose and for frames a stride-C de-interleave: a workgroup owns a BAND - S output rows x up to UNP_TOK
// patches wide, all channels -, reads the prediction rows of the band's scored tokens with 16-byte loads into an LDS tile, fills the rest of
// the tile (kept tokens, uncovered cells) from the input through xf_audio / xf_video - the loss kernel's own target reads - and writes the
// tile out along W, 16 bytes per lane where W and the pointer allow.  One writer per output cell, no atomics: the same bytes every call.
#define UNP_TOK 8
#define UNP_LD (UNP_TOK * 16 + 1)          // odd row pitch: the transposing writes of the audio case walk the banks

// inv[row_id[pr] - id_base] = pr (inv is -1 elsewhere: a token nobody predicted)
__global__ void unpatchify_inv_kernel(const int* __restrict__ row_id, int id_base, int rows, int npos, int* __restrict__ inv) {
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    if (pr >= rows) return;
    const int pos = row_id[pr] - id_base;
    if (pos >= 0 && pos < npos) inv[pos] = pr;
}

// err[pos] = the row loss of a scored token (what mae_loss_fwd left in row_loss), 0 of a kept one
__global__ void unpatchify_err_kernel(const float* __restrict__ row_loss, const float* __restrict__ mask, const int* __restrict__ inv, int rows,
                                      int npos, float* __restrict__ err) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= npos) return;
    const int pr = inv ? inv[pos] : pos;
    err[pos] = (mask[pos] == 1.0f && pr >= 0 && pr < rows) ? row_loss[pr] : 0.f;
}

struct UnpRaw {                    // inverse affine of the input transform (raw outputs)
    float mean[3], std[3];
};

// x * std + mean, the two roundings kept apart (numpy float32 restates it): contraction off - hipcc fuses a * b + c into an fma by default, and
// HIP's __fmul_rn / __fadd_rn are plain operators that do not stop it
__device__ __forceinline__ float unp_raw(float x, float std, float mean) {
#pragma clang fp contract(off)
    const float m = x * std;
    return m + mean;
}

__device__ __forceinline__ uint8_t unp_u8(float x, float std, float mean) {
#pragma clang fp contract(off)
    const float v = rintf(unp_raw(x, std, mean) * 255.0f);
    return (uint8_t)fminf(fmaxf(v, 0.f), 255.f);           // (NaN -> 0: fmaxf returns the other operand)
}

// grid: (column groups, row bands, n).  out: fp32 [n, C, H, W] or NULL; raw_f (audio) / raw_u (frames): the raw output or NULL.
// vec: W % 4 == 0 and every output pointer is aligned for a 4-element store
template <int C>
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ pred, const void* __restrict__ inp, const float* __restrict__ mask,
                                                         float* __restrict__ out, float* __restrict__ raw_f, uint8_t* __restrict__ raw_u,
                                                         const int* __restrict__ inv, int rows, int audio, int L, int H, int W, int S,
                                                         int nrp, int ncp, int paste_kept, int vec, InXf xf, UnpRaw rw) {
    __shared__ float tile[C * 16 * UNP_LD];                // (C = 1: 8 KiB - the LDS does not limit the workgroups per CU; C = 3: 24 KiB)
    __shared__ int tok_pr[UNP_TOK];                        // prediction row of the band's token j, or -1: the token's cells come from the input
    const int cg = blockIdx.x, rp = blockIdx.y, n = blockIdx.z;
    constexpr int P = 256 * C;
    const int c0 = cg * UNP_TOK * S;                       // first column of the band
    const int wid = min(UNP_TOK * S, W - c0);              // its width ...
    const int r0 = rp * S;
    const int hgt = min(S, H - r0);                        // ... and height
    const int G = audio ? nrp : ncp;
    if (threadIdx.x < UNP_TOK) {
        const int cp = cg * UNP_TOK + threadIdx.x;
        int pr = -1;
        if (rp < nrp && cp < ncp) {
            const int pos = n * L + (audio ? cp * G + rp : rp * G + cp);
            const float m = mask[pos];                     // (both loads issued before either is used: one round trip, not two)
            const int r = inv ? inv[pos] : pos;
            if ((!paste_kept || m == 1.0f) && r < rows) pr = r;
        }
        tok_pr[threadIdx.x] = pr;
    }
    __syncthreads();
    // scored tokens: prediction rows, four consecutive elements per lane
    constexpr int NV = UNP_TOK * (P / 4) / 256;             // 16-byte loads per lane: 2 C, issued together, then scattered into the tile
    f32x4 pv[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int i = threadIdx.x + u * 256;
        const int j = i / (P / 4), e0 = (i - j * (P / 4)) * 4;
        const int pr = tok_pr[j];
        if (pr >= 0) pv[u] = *reinterpret_cast<const f32x4*>(pred + (size_t)pr * P + e0);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int i = threadIdx.x + u * 256;
        const int j = i / (P / 4), e0 = (i - j * (P / 4)) * 4;
        if (tok_pr[j] < 0) continue;
        const f32x4 v = pv[u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = e0 + k;
            int c, ro, co;
            if (audio) { c = 0; co = e >> 4; ro = e & 15; }
            else { c = e % C; const int pq = e / C; ro = pq >> 4; co = pq & 15; }
            if (ro < S && co < S) tile[(c * 16 + ro) * UNP_LD + j * S + co] = v[k];
        }
    }
    // everything else: the input as the model saw it.  A lane keeps ONE column of the band (consecutive lanes along W) and walks its rows, so
    // the column's token is looked up once and no index is taken apart by a division (with runtime divisors those cost more than the loads)
    {
        const int col = threadIdx.x & (UNP_TOK * 16 - 1), rs = threadIdx.x >> 7;       // 128 columns x 2 row phases
        if (col < wid && tok_pr[col / S] < 0) {            // (wid <= UNP_TOK * S, so col / S < UNP_TOK; columns past the last patch: tok_pr -1)
#pragma unroll
            for (int c = 0; c < C; ++c)
                for (int ro = rs; ro < hgt; ro += 2) {
                    float v;
                    if (audio) v = xf_audio(reinterpret_cast<const float*>(inp), xf, n, r0 + ro, c0 + col, H, W);
                    else v = xf_video(inp, xf, (((size_t)n * C + c) * H + r0 + ro) * W + c0 + col, c);
                    tile[(c * 16 + ro) * UNP_LD + col] = v;
                }
        }
    }
    __syncthreads();
    if (vec) {                                             // 32 lanes x 16 bytes along W, 8 rows per pass
        const int col = (threadIdx.x & 31) * 4, rs = threadIdx.x >> 5;
        if (col >= wid) return;
#pragma unroll
        for (int c = 0; c < C; ++c)
            for (int ro = rs; ro < hgt; ro += 8) {
                const float* t = tile + (c * 16 + ro) * UNP_LD + col;
                const f32x4 v = {t[0], t[1], t[2], t[3]};
                const size_t o = (((size_t)n * C + c) * H + r0 + ro) * W + c0 + col;
                if (out) *reinterpret_cast<f32x4*>(out + o) = v;
                if (raw_f) {
                    const f32x4 r = {unp_raw(v[0], rw.std[0], rw.mean[0]), unp_raw(v[1], rw.std[0], rw.mean[0]), unp_raw(v[2], rw.std[0], rw.mean[0]),
                                     unp_raw(v[3], rw.std[0], rw.mean[0])};
                    *reinterpret_cast<f32x4*>(raw_f + o) = r;
                }
                if (raw_u) {
                    const uint32_t b = (uint32_t)unp_u8(v[0], rw.std[c], rw.mean[c]) | ((uint32_t)unp_u8(v[1], rw.std[c], rw.mean[c]) << 8) |
                                       ((uint32_t)unp_u8(v[2], rw.std[c], rw.mean[c]) << 16) | ((uint32_t)unp_u8(v[3], rw.std[c], rw.mean[c]) << 24);
                    *reinterpret_cast<uint32_t*>(raw_u + o) = b;
                }
            }
        return;
    }
    const int col = threadIdx.x & (UNP_TOK * 16 - 1), rs = threadIdx.x >> 7;
    if (col >= wid) return;
#pragma unroll
    for (int c = 0; c < C; ++c)
        for (int ro = rs; ro < hgt; ro += 2) {
            const float v = tile[(c * 16 + ro) * UNP_LD + col];
            const size_t o = (((size_t)n * C + c) * H + r0 + ro) * W + c0 + col;
            if (out) out[o] = v;
            if (raw_f) raw_f[o] = unp_raw(v, rw.std[0], rw.mean[0]);
            if (raw_u) raw_u[o] = unp_u8(v, rw.std[c], rw.mean[c]);
        }
}

// ===================================================================================================
int avs_make_xf(const avs_input_xf_t* x, int want_kind, InXf* out, const char* who);     // elementwise.hip

extern "C" int avs_unpatchify(const float* pred, const void* inp, const float* mask, float* out, void* raw_out, const float* row_loss, float* err,
                              int rows, int audio, int n, int L, int C, int H, int W, int stride, const avs_input_xf_t* xf, const int* row_id,
                              int id_base, int* inv_ws, int paste_kept, hipStream_t stream) {
    AVS_CHECK_ARG(rows > 0 && n > 0 && L > 0 && pred && inp && mask && (out || raw_out || err) && stride > 0 && stride <= 16 && H > 0 && W > 0,
                  "unpatchify: bad args (rows %d n %d L %d stride %d)", rows, n, L, stride);
    AVS_CHECK_ARG(C >= 1 && C <= 3 && (!audio || C == 1), "unpatchify: %d channels (1..3; audio: 1)", C);
    AVS_CHECK_ARG((long long)n * L < (1ll << 31) && (long long)rows <= (long long)n * L, "unpatchify: %d rows for %d x %d tokens", rows, n, L);
    const int nrp = H / stride, ncp = W / stride;
    AVS_CHECK_ARG(nrp * ncp == L, "unpatchify: L %d is not (H / stride) * (W / stride) = %d * %d", L, nrp, ncp);
    AVS_CHECK_ARG((reinterpret_cast<uintptr_t>(pred) & 15) == 0, "unpatchify: pred must be 16-byte aligned");
    AVS_CHECK_ARG(!row_id || inv_ws, "unpatchify: compact rows (row_id) need the n * L int32 workspace inv_ws");
    AVS_CHECK_ARG(row_id || rows == n * L, "unpatchify: without row_id every token has a row: rows %d != n * L = %d", rows, n * L);
    AVS_CHECK_ARG(!err || row_loss, "unpatchify: err needs row_loss");
    InXf x;
    if (int rc = avs_make_xf(xf, audio ? 1 : 2, &x, "unpatchify")) return rc;
    AVS_CHECK_ARG(x.kind == 0 || audio || C == 3, "unpatchify: uint8 frames need 3 channels");
    UnpRaw rw{};
    if (raw_out) {
        AVS_CHECK_ARG(x.kind != 0, "unpatchify: raw output needs the input transform it inverts");
        AVS_CHECK_ARG(!x.shift && !x.amp, "unpatchify: raw output is refused with a per-sample shift / amp (a rolled, noised input has no original units)");
        for (int c = 0; c < 3; ++c) { rw.mean[c] = xf->mean[c]; rw.std[c] = xf->std[c]; }
    }
    const int npos = n * L;
    const int* inv = nullptr;
    if (row_id) {
        if (hipMemsetAsync(inv_ws, 0xFF, (size_t)npos * sizeof(int), stream) != hipSuccess) { avs_set_error("unpatchify: memset failed"); return -1; }
        unpatchify_inv_kernel<<<ceil_div(rows, 256), 256, 0, stream>>>(row_id, id_base, rows, npos, inv_ws);
        AVS_LAUNCH_CHECK("unpatchify_inv");
        inv = inv_ws;
    }
    if (out || raw_out) {
        float* raw_f = audio ? reinterpret_cast<float*>(raw_out) : nullptr;
        uint8_t* raw_u = audio ? nullptr : reinterpret_cast<uint8_t*>(raw_out);
        const int vec = (W % 4) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(raw_f) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(raw_u) & 3) == 0;
        const dim3 grid(ceil_div(W, UNP_TOK * stride), ceil_div(H, stride), n);
        AVS_CHECK_ARG(grid.y <= 65535 && grid.z <= 65535, "unpatchify: %d row bands / %d pictures exceed the grid", (int)grid.y, n);
#define UNP_LAUNCH(CH) unpatchify_kernel<CH><<<grid, 256, 0, stream>>>(pred, inp, mask, out, raw_f, raw_u, inv, rows, audio, L, H, W, stride, nrp, ncp, \
                                                                       paste_kept ? 1 : 0, vec, x, rw)
        if (C == 1) UNP_LAUNCH(1); else if (C == 2) UNP_LAUNCH(2); else UNP_LAUNCH(3);
#undef UNP_LAUNCH
        AVS_LAUNCH_CHECK("unpatchify");
    }
    if (err) {
        unpatchify_err_kernel<<<ceil_div(npos, 256), 256, 0, stream>>>(row_loss, mask, inv, rows, npos, err);
        AVS_LAUNCH_CHECK("unpatchify_err");
    }
    return 0;
}
