// k18 - PCM decode on the device: the bytes of a WAV file's data chunk (interleaved sample frames, little endian) to the planar fp32 channels
// that avs_resample_wave reads - what torchaudio.load(normalize=True) hands the reference's loader (dataloader_ft.py:272).  The specification
// is avsiam_amd.preprocess.decode_pcm_reference (numpy, bit for bit); include/avsiam_hip.h states the contract.
//
// A workgroup owns DP_TILE = 1024 consecutive sample frames of one clip.  The tile's first byte, tile * 1024 * C * bytes_per_sample, is a
// multiple of 16 for every format and channel count, so the payload is copied into LDS with aligned 16-byte loads - no byte loads from memory.
// The format is the CLIP's (a device-side descriptor: one call mixes formats), so the LDS cannot be sized by it on the host: the buffer is a
// fixed 16 KiB and a tile whose frames are wider than 16 bytes is walked in 2 or 4 passes of 512 or 256 frames (a pass starts on a multiple
// of 256 frames: still 16-byte aligned).  Out of LDS every work item takes one channel's 4 consecutive frames - samples are cut out of the
// dwords that hold them (24-bit: a 64-bit funnel over two dwords) - and writes the quad to 16 consecutive, 16-byte aligned bytes; adjacent
// lanes own adjacent quads of one channel, so a wave's stores cover whole 1 KiB runs.  (The source asks for one uint4 store; at -O3 the
// compiler merges that path with the scalar fallback and the gfx950 code object holds a 12-byte store plus a 4-byte store per quad, no
// global_store_dwordx4.  The measurements in the README are of that code.)  One writer per cell, no atomics.
#include "common.h"

#define DP_THREADS 256
#define DP_TILE 1024
#define DP_LDS_BYTES 16384
#define DP_MAX_CHANNELS 8

enum { DP_U8 = 0, DP_S16 = 1, DP_S24 = 2, DP_S32 = 3, DP_F32 = 4, DP_F64 = 5, DP_FORMATS = 6 };

static __device__ __forceinline__ int dp_bytes(int fmt) {
    return fmt == DP_U8 ? 1 : fmt == DP_S16 ? 2 : fmt == DP_S24 ? 3 : (fmt == DP_S32 || fmt == DP_F32) ? 4 : fmt == DP_F64 ? 8 : 0;
}

// the fp32 bits of the sample whose first byte is `off` bytes into the LDS copy
template <int FMT>
static __device__ __forceinline__ uint32_t dp_sample(const uint32_t* __restrict__ s, int off) {
    const int w = off >> 2;
    if (FMT == DP_U8) {
        const int x = (int)((s[w] >> ((off & 3) * 8)) & 0xffu);
        return __float_as_uint((float)(x - 128) * 0x1p-7f);
    } else if (FMT == DP_S16) {
        const int x = (int)(short)(s[w] >> ((off & 2) * 8));
        return __float_as_uint((float)x * 0x1p-15f);
    } else if (FMT == DP_S24) {
        const uint64_t two = ((uint64_t)s[w + 1] << 32) | (uint64_t)s[w];       // (the word after the last sample's is inside the array)
        const int x = (int)((uint32_t)(two >> ((off & 3) * 8)) << 8) >> 8;      // sign-extended
        return __float_as_uint((float)x * 0x1p-23f);
    } else if (FMT == DP_S32) {
        return __float_as_uint((float)(int)s[w] * 0x1p-31f);                    // int -> float rounds to nearest even; the scale is exact
    } else if (FMT == DP_F32) {
        return s[w];                                                            // the bits: NaN payloads and -0.0 pass untouched
    } else {
        const double d = __longlong_as_double((long long)(((uint64_t)s[w + 1] << 32) | (uint64_t)s[w]));
        return __float_as_uint((float)d);
    }
}

// frames [g0, g0 + span) of the row, `live` of them the clip's (the rest zero), every channel: LDS -> out
template <int FMT>
static __device__ __forceinline__ void dp_convert(const uint32_t* __restrict__ s, int C, int bps, int live, int span, uint32_t* __restrict__ orow, int stride, int g0,
                                                  int vec_ok) {
    const int nq = (span + 3) >> 2;
    for (int i = threadIdx.x; i < C * nq; i += DP_THREADS) {
        const int c = i / nq, fr = (i - c * nq) * 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fr + k < live ? dp_sample<FMT>(s, ((fr + k) * C + c) * bps) : 0u;
        uint32_t* __restrict__ dst = orow + (size_t)c * stride + g0 + fr;
        if (vec_ok) {                                           // (stride % 4 == 0: a quad that starts inside the row ends inside it)
            *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (fr + k < span) dst[k] = v[k];
        }
    }
}

// grid (ceil(stride / DP_TILE), B), DP_THREADS threads
__global__ __launch_bounds__(DP_THREADS) void decode_pcm_kernel(const uint8_t* __restrict__ payload, long long byte_stride, const int* __restrict__ desc, int C,
                                                                uint32_t* __restrict__ out, int stride, int* __restrict__ out_len, int vec_ok) {
    __shared__ __align__(16) uint32_t s_raw[DP_LDS_BYTES / 4 + 4];
    const int b = blockIdx.y, f0 = blockIdx.x * DP_TILE, tid = threadIdx.x;
    const int fmt = desc[2 * b], bps = dp_bytes(fmt), fb = C * max(bps, 1);
    // the clip's frames, cut to what the two rows hold (an unknown format: none)
    const long long held = byte_stride / fb;
    int n = desc[2 * b + 1];
    n = n < 0 || bps == 0 ? 0 : n;
    n = n > stride ? stride : n;
    n = (long long)n > held ? (int)held : n;
    if (blockIdx.x == 0 && tid == 0) out_len[b] = n;

    const uint8_t* __restrict__ row = payload + (size_t)b * (size_t)byte_stride;
    uint32_t* __restrict__ orow = out + (size_t)b * C * stride;
    const int tile_end = min(f0 + DP_TILE, stride), f_end = min(tile_end, n);
    const int passes = fb <= 16 ? 1 : fb <= 32 ? 2 : 4, sub = DP_TILE / passes;        // sub * fb <= DP_LDS_BYTES

    for (int g0 = f0; g0 < tile_end; g0 += sub) {               // (uniform over the workgroup)
        const int span = min(sub, tile_end - g0), live = min(max(f_end - g0, 0), span);
        if (g0 > f0) __syncthreads();                           // every read of the previous pass is done
        if (live > 0) {
            // live * fb bytes from the pass's first byte, a multiple of 16; the last 16-byte chunk ends at or before ceil16(n * fb) <= byte_stride
            const uint4* __restrict__ src = reinterpret_cast<const uint4*>(row + (size_t)g0 * fb);
            const int chunks = (live * fb + 15) >> 4;
            for (int i = tid; i < chunks; i += DP_THREADS) reinterpret_cast<uint4*>(s_raw)[i] = src[i];
        }
        __syncthreads();
        switch (live > 0 ? fmt : DP_F32) {                      // (no live frame: nothing is read, every cell is zero)
            case DP_U8: dp_convert<DP_U8>(s_raw, C, bps, live, span, orow, stride, g0, vec_ok); break;
            case DP_S16: dp_convert<DP_S16>(s_raw, C, bps, live, span, orow, stride, g0, vec_ok); break;
            case DP_S24: dp_convert<DP_S24>(s_raw, C, bps, live, span, orow, stride, g0, vec_ok); break;
            case DP_S32: dp_convert<DP_S32>(s_raw, C, bps, live, span, orow, stride, g0, vec_ok); break;
            case DP_F64: dp_convert<DP_F64>(s_raw, C, bps, live, span, orow, stride, g0, vec_ok); break;
            default: dp_convert<DP_F32>(s_raw, C, 4, live, span, orow, stride, g0, vec_ok); break;
        }
    }
}

extern "C" int avs_decode_pcm(const uint8_t* payload, long long byte_stride, const int* desc, int B, int C, float* out, long long stride, int* out_len,
                              hipStream_t stream) {
    AVS_CHECK_ARG(payload && desc && out && out_len && B > 0 && B <= 65535 && C >= 1 && C <= DP_MAX_CHANNELS,
                  "decode_pcm: bad arguments (payload, desc, out, out_len; 1 <= B <= 65535; 1 <= C <= %d)", DP_MAX_CHANNELS);
    AVS_CHECK_ARG(byte_stride >= 16 && byte_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(payload) & 15) == 0,
                  "decode_pcm: the payload rows are read with 16-byte loads: byte_stride %lld must be a positive multiple of 16 and the buffer 16-byte aligned", byte_stride);
    AVS_CHECK_ARG(stride >= 1 && stride <= 0x7fffffffLL - DP_TILE, "decode_pcm: stride outside 1 .. 2^31 - %d", DP_TILE + 1);
    AVS_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "decode_pcm: out is not 4-byte aligned");
    const int vec_ok = (stride % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    dim3 grid((unsigned)((stride + DP_TILE - 1) / DP_TILE), B);
    decode_pcm_kernel<<<grid, DP_THREADS, 0, stream>>>(payload, byte_stride, desc, C, reinterpret_cast<uint32_t*>(out), (int)stride, out_len, vec_ok);
    AVS_LAUNCH_CHECK("decode_pcm");
    return 0;
}
