// k13 - waveform input on the device: the Kaldi fbank of the reference's fine-tuning loader (dataloader_ft.py:277-340:
// torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=16000, use_energy=False, window_type='hanning', num_mel_bins=128,
// dither=0.0, frame_shift=10), then ZeroPad2d / cut to target_length) and its waveform mixup (:298-322), waveform in, log-mel out.
// The specification is preprocess.kaldi_fbank_reference (float64); include/avsiam_hip.h states the formulas.
//
//   avs_wave_sums     per clip: sum w1 over n1, sum w2 over n2, sum w2 over min(n1, n2) - what the mean subtraction of the plain path and
//                     the three of the mixed path need.  One workgroup of 1024 threads per clip, fp64 partial sums in a fixed order, no atomics.
//   avs_kaldi_fbank   a workgroup owns FB_TILE consecutive frames of one clip: their sample span (160 (FB_TILE - 1) + 400 samples; frames
//                     overlap 2.5 x) is read ONCE into LDS, and that read is where the clip mean / the mix is applied.  Each of the four
//                     waves then takes a frame at a time: frame mean, pre-emphasis, window, 512-point FFT as three radix-8 Stockham passes
//                     (8 points per lane in registers, LDS between the passes), power, 128 mel sums in bin order (two filters per lane, their
//                     <= 10 weights in registers), log, and one coalesced 512-byte row.  Rows past the clip's frames are pad rows.
//   avs_mix_frames_u8 the frame side of mixup (:441-458): weight_b n(v1) + (1 - weight_b) n(v2), n = avs_normalize_frames_u8's arithmetic.
//   avs_resize_frames_u8  decoded-size uint8 frames, ragged per clip, to the normalised and optionally mixed fp32 frames of the model (:136-139,
//                     434-459): antialiased bicubic resize in one two-pass kernel, the intermediate in LDS (described where it stands, below).
//
// Twiddles, window and mel weights are tables computed on the host in float64, rounded once and uploaded once per device (frontend_math.h);
// no sincosf, no fast-math intrinsic, logf for the log.  No atomics: every output is bit-identical from call to call.
#include <mutex>

#include "common.h"
#include "frontend_math.h"

#define FB_TILE 16                                         // frames per workgroup
#define FB_WAVES 4
#define FB_THREADS (64 * FB_WAVES)
#define FB_SPAN (FB_SHIFT * (FB_TILE - 1) + FB_FRAME)      // 2800 samples, 11.2 KB

__device__ __forceinline__ int fb_clamp_len(const int* __restrict__ len, int b, long long stride) {
    const int n = len ? len[b] : (int)stride;
    return n < 0 ? 0 : (n > stride ? (int)stride : n);
}

// ---- sums -------------------------------------------------------------------------------------------------------------------------------
// grid B, 1024 threads.  Thread t adds the quads t, t + 1024, ... (four consecutive samples each, in order) in fp64, then a tree over the 1024
// partial sums: one fixed order per clip, whatever the alignment (an aligned row is read 16 bytes per lane, any other one sample at a time).
#define WS_THREADS 1024

__device__ __forceinline__ void ws_quad(const float* __restrict__ w, bool vec, int q, int n, int n_cut, double& s, double& s_cut) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int i = 4 * q;
    if (vec && i + 4 <= n) {
        const float4 x = *reinterpret_cast<const float4*>(w + i);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) v[k] = w[i + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i + k < n) s += (double)v[k];
        if (i + k < n_cut) s_cut += (double)v[k];
    }
}

__global__ __launch_bounds__(WS_THREADS) void wave_sums_kernel(const float* __restrict__ wave, long long stride, const int* __restrict__ len,
                                                               const float* __restrict__ wave2, long long stride2, const int* __restrict__ len2,
                                                               double* __restrict__ sums) {
    __shared__ double red[3][WS_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n1 = fb_clamp_len(len, b, stride);
    const int n2 = wave2 ? fb_clamp_len(len2, b, stride2) : 0;
    const int n2c = n2 < n1 ? n2 : n1;
    const float* __restrict__ w1 = wave + (size_t)b * stride;
    const bool vec1 = (reinterpret_cast<uintptr_t>(w1) & 15) == 0;
    double s1 = 0.0, s2 = 0.0, s2c = 0.0, unused = 0.0;
    for (int q = tid; 4 * q < n1; q += WS_THREADS) ws_quad(w1, vec1, q, n1, 0, s1, unused);
    if (wave2) {
        const float* __restrict__ w2 = wave2 + (size_t)b * stride2;
        const bool vec2 = (reinterpret_cast<uintptr_t>(w2) & 15) == 0;
        for (int q = tid; 4 * q < n2; q += WS_THREADS) ws_quad(w2, vec2, q, n2, n2c, s2, s2c);
    }
    red[0][tid] = s1; red[1][tid] = s2; red[2][tid] = s2c;
    __syncthreads();
    for (int h = WS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h];
        }
        __syncthreads();
    }
    if (tid < 3) sums[3 * b + tid] = red[tid][0];
}

// ---- fbank ------------------------------------------------------------------------------------------------------------------------------
// what the framing sees at sample i of clip b (dataloader_ft.py:277-278 plain, :308-322 mixed)
struct FbPrep {
    int mixed, n2c;                  // n2c: samples of the partner that take part, min(n1, n2); beyond them the partner is 0 (padded AFTER its mean left)
    float lam, om, m1, m2, mix_mean;
};

__device__ __forceinline__ FbPrep fb_prep(const double* __restrict__ sums, const float* __restrict__ lam, const int* __restrict__ len2, int b, int n1,
                                          long long stride2, bool have_partner) {
    FbPrep p;
    const double m1 = sums[3 * b] / (double)n1;
    const float l = (have_partner && lam) ? lam[b] : -1.f;
    p.mixed = l >= 0.f ? 1 : 0;
    p.m1 = (float)m1;
    p.n2c = 0; p.lam = 1.f; p.om = 0.f; p.m2 = 0.f; p.mix_mean = 0.f;
    if (p.mixed) {
        const int n2 = fb_clamp_len(len2, b, stride2);
        p.n2c = n2 < n1 ? n2 : n1;
        const double m2 = n2 > 0 ? sums[3 * b + 1] / (double)n2 : 0.0;
        const double om = 1.0 - (double)l;
        // mean over n1 of lam (w1 - m1) + (1 - lam) (w2 - m2 | 0): the w1 part is lam (S1 / n1 - m1) = 0
        p.mix_mean = (float)(om * (sums[3 * b + 2] - (double)p.n2c * m2) / (double)n1);
        p.lam = l; p.om = (float)om; p.m2 = (float)m2;
    }
    return p;
}

// grid (ceil(T / FB_TILE), B), 256 threads
__global__ __launch_bounds__(FB_THREADS) void kaldi_fbank_kernel(const float* __restrict__ wave, long long stride, const int* __restrict__ len,
                                                                 const float* __restrict__ wave2, long long stride2, const int* __restrict__ len2,
                                                                 const float* __restrict__ lam, const double* __restrict__ sums,
                                                                 const float* __restrict__ tab, float* __restrict__ out, int T, int use_norm,
                                                                 float mean, float inv_std) {
    __shared__ float s_span[FB_SPAN];
    __shared__ float s_tw[2 * FB_NFFT];
    __shared__ float s_win[FB_FRAME];
    __shared__ float2 s_z[FB_WAVES][FB_BUF];                            // (re, im) pairs: one 8-byte LDS access per element
    __shared__ float s_pw[FB_WAVES][FB_NBIN];

    const int b = blockIdx.y, t0 = blockIdx.x * FB_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n1 = fb_clamp_len(len, b, stride);
    const int m = n1 >= FB_FRAME ? 1 + (n1 - FB_FRAME) / FB_SHIFT : 0;
    const int rows = min(FB_TILE, T - t0);                              // rows of the output this workgroup writes (>= 1 by the grid)
    const int nf = max(0, min(rows, m - t0));                           // of them, frames of the clip
    const float pad_value = use_norm ? (0.f - mean) * inv_std : 0.f;
    float* __restrict__ orow = out + ((size_t)b * T + t0) * FB_NMEL;

    // pad rows: ZeroPad2d below the clip's frames
    for (int i = nf * FB_NMEL + tid; i < rows * FB_NMEL; i += FB_THREADS) orow[i] = pad_value;
    if (nf == 0) return;                                                // (uniform over the workgroup)

    // tables -> LDS / registers
    for (int i = tid; i < 2 * FB_NFFT; i += FB_THREADS) s_tw[i] = tab[FB_TAB_TW + i];
    for (int i = tid; i < FB_FRAME; i += FB_THREADS) s_win[i] = tab[FB_TAB_WIN + i];
    const int* __restrict__ itab = reinterpret_cast<const int*>(tab);
    float mw[2][FB_MELW];
    int mfirst[2], mcount[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        mfirst[q] = itab[FB_TAB_FIRST + k];
        mcount[q] = itab[FB_TAB_COUNT + k];
#pragma unroll
        for (int i = 0; i < FB_MELW; ++i) mw[q][i] = tab[FB_TAB_MELW + k * FB_MELW + i];
    }

    // the sample span, prepared where it is read.  Every index is below n1: the clip's last frame ends at 160 (m - 1) + 400 <= n1 <= stride
    {
        const FbPrep p = fb_prep(sums, lam, len2, b, n1, stride2, wave2 != nullptr);
        const int s0 = t0 * FB_SHIFT, ns = FB_SHIFT * (nf - 1) + FB_FRAME;
        const float* __restrict__ w1 = wave + (size_t)b * stride + s0;
        if (!p.mixed) {
            for (int i = tid; i < ns; i += FB_THREADS) s_span[i] = w1[i] - p.m1;
        } else {
            const float* __restrict__ w2 = wave2 + (size_t)b * stride2 + s0;
            for (int i = tid; i < ns; i += FB_THREADS) {
                const float a = w1[i] - p.m1;
                const float c = s0 + i < p.n2c ? w2[i] - p.m2 : 0.f;       // (never reads the partner at or beyond min(n1, n2))
                s_span[i] = (p.lam * a + p.om * c) - p.mix_mean;
            }
        }
    }
    __syncthreads();

    float2* __restrict__ z = s_z[wv];
    float* __restrict__ pw = s_pw[wv];
    // every wave runs every round (the barriers are workgroup-wide); a wave without a frame in the last round computes frame nf - 1 again and
    // writes nothing
    for (int f0 = 0; f0 < nf; f0 += FB_WAVES) {
        const int f = f0 + wv;
        const bool live = f < nf;
        const float* __restrict__ x = s_span + FB_SHIFT * (live ? f : nf - 1);
        float vr[8], vi[8];
        // frame mean: lane j adds x[j], x[j + 64], ... (ascending), then the wave's butterfly - one fixed order
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const int i = lane + 64 * r;
            vr[r] = i < FB_FRAME ? x[i] : 0.f;
            s += vr[r];
        }
        const float fmean = wave_sum(s) * (1.0f / FB_FRAME);
        // pre-emphasis on the mean-free frame, window, zero padding to 512: pass 1 reads elements j + 64 r
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = lane + 64 * r;
            float v = 0.f;
            if (r < 7 && i < FB_FRAME) {
                const float cur = vr[r] - fmean, prev = (i > 0 ? x[i - 1] : vr[r]) - fmean;
                v = (cur - 0.97f * prev) * s_win[i];
            }
            vr[r] = v; vi[r] = 0.f;
        }
        int base = fb_pass<1>(lane, vr, vi, s_tw);
#pragma unroll
        for (int r = 0; r < 8; ++r) z[fb_pad(base + r)] = make_float2(vr[r], vi[r]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) { const float2 t = z[fb_pad(lane + 64 * r)]; vr[r] = t.x; vi[r] = t.y; }
        __syncthreads();
        base = fb_pass<8>(lane, vr, vi, s_tw);
#pragma unroll
        for (int r = 0; r < 8; ++r) z[fb_pad(base + 8 * r)] = make_float2(vr[r], vi[r]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) { const float2 t = z[fb_pad(lane + 64 * r)]; vr[r] = t.x; vi[r] = t.y; }
        base = fb_pass<64>(lane, vr, vi, s_tw);                         // base = lane: output r is bin lane + 64 r
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[lane + 64 * r] = vr[r] * vr[r] + vi[r] * vi[r];
        __syncthreads();                                                // (also: every read of z is done before the next round writes it)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float e = 0.f;
#pragma unroll
            for (int i = 0; i < FB_MELW; ++i)
                if (i < mcount[q]) e += mw[q][i] * pw[mfirst[q] + i];   // first + count <= 256 (fb_build_tables)
            float o = e <= FB_EPS ? FB_LOG_EPS : logf(e);
            if (use_norm) o = (o - mean) * inv_std;
            if (live) orow[(size_t)f * FB_NMEL + lane + 64 * q] = o;
        }
    }
}

// ---- tables: built once per process, uploaded once per device ----------------------------------------------------------------------------------
#define FB_MAX_DEVICES 64
static std::mutex fb_mu;
static float fb_host_tab[FB_TAB_WORDS];
static int fb_host_ready = 0;
static float* fb_dev_tab[FB_MAX_DEVICES];

static int fb_host_tables() {
    if (!fb_host_ready) {
        if (fb_build_tables(fb_host_tab) != 0) return -1;
        fb_host_ready = 1;
    }
    return 0;
}

static const float* fb_tables() {
    std::lock_guard<std::mutex> g(fb_mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= FB_MAX_DEVICES) return nullptr;
    if (fb_dev_tab[dev]) return fb_dev_tab[dev];
    if (fb_host_tables() != 0) return nullptr;
    float* d = nullptr;
    if (hipMalloc(&d, sizeof(fb_host_tab)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, fb_host_tab, sizeof(fb_host_tab), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    fb_dev_tab[dev] = d;
    return d;
}

extern "C" int avs_fbank_tables(float* tab, int words) {
    AVS_CHECK_ARG(tab && words == FB_TAB_WORDS, "fbank_tables: need a host buffer of exactly %d words", FB_TAB_WORDS);
    std::lock_guard<std::mutex> g(fb_mu);
    AVS_CHECK_ARG(fb_host_tables() == 0, "fbank_tables: a mel filter is wider than %d bins", FB_MELW);
    for (int i = 0; i < FB_TAB_WORDS; ++i) tab[i] = fb_host_tab[i];
    return 0;
}

static int fb_check_waves(const char* who, const float* wave, long long stride, const float* partner, long long partner_stride,
                          const int* partner_len, int B) {
    AVS_CHECK_ARG(wave && B > 0 && B <= 65535 && stride >= FB_FRAME && stride <= 0x7fffffffLL, "%s: bad arguments (wave, 1 <= B <= 65535, 400 <= stride < 2^31)", who);
    AVS_CHECK_ARG(partner || (!partner_len && partner_stride == 0), "%s: partner lengths / stride without a partner", who);
    AVS_CHECK_ARG(!partner || (partner_stride >= 1 && partner_stride <= 0x7fffffffLL), "%s: partner stride outside 1 .. 2^31 - 1", who);
    return 0;
}

extern "C" int avs_wave_sums(const float* wave, long long stride, const int* len, const float* partner, long long partner_stride,
                             const int* partner_len, int B, double* sums, hipStream_t stream) {
    if (int rc = fb_check_waves("wave_sums", wave, stride, partner, partner_stride, partner_len, B)) return rc;
    AVS_CHECK_ARG(sums, "wave_sums: sums is NULL");
    wave_sums_kernel<<<B, WS_THREADS, 0, stream>>>(wave, stride, len, partner, partner_stride, partner_len, sums);
    AVS_LAUNCH_CHECK("wave_sums");
    return 0;
}

extern "C" int avs_kaldi_fbank(const float* wave, long long stride, const int* len, const float* partner, long long partner_stride,
                               const int* partner_len, const float* lam, const double* sums, int B, int target_length, int n_mels, float* out,
                               int use_norm, float mean, float std, hipStream_t stream) {
    if (int rc = fb_check_waves("kaldi_fbank", wave, stride, partner, partner_stride, partner_len, B)) return rc;
    AVS_CHECK_ARG(n_mels == FB_NMEL, "kaldi_fbank: n_mels = %d: the kernel is built for 128 mel bins over a 512-point FFT at 16 kHz", n_mels);
    AVS_CHECK_ARG(sums && out && target_length > 0 && target_length <= (1 << 20), "kaldi_fbank: bad arguments (sums, out, 1 <= target_length <= 2^20)");
    AVS_CHECK_ARG(!lam || partner, "kaldi_fbank: lam without a partner");
    AVS_CHECK_ARG(!use_norm || std != 0.f, "kaldi_fbank: zero std");
    const float* tab = fb_tables();
    AVS_CHECK_ARG(tab, "kaldi_fbank: could not build / upload the tables");
    dim3 grid(ceil_div(target_length, FB_TILE), B);
    kaldi_fbank_kernel<<<grid, FB_THREADS, 0, stream>>>(wave, stride, len, partner, partner_stride, partner_len, lam, sums, tab, out, target_length,
                                                        use_norm ? 1 : 0, mean, use_norm ? 1.0f / std : 1.0f);
    AVS_LAUNCH_CHECK("kaldi_fbank");
    return 0;
}

// ---- frames -----------------------------------------------------------------------------------------------------------------------------
// out[n, c, :] = w_b n(v1) + (1 - w_b) n(v2), b = n / per_sample, n(x) = (x / 255 - mean_c) / std_c as normalize_frames_kernel; grid (N*3, ceil(plane/4 / 256))
__global__ __launch_bounds__(256) void mix_frames_kernel(const uint8_t* __restrict__ in1, const uint8_t* __restrict__ in2, const float* __restrict__ weight,
                                                         float* __restrict__ out, int plane, int per_sample, float m0, float m1, float m2, float s0,
                                                         float s1, float s2) {
    const int nc = blockIdx.x, c = nc % 3;
    const int i4 = blockIdx.y * 256 + threadIdx.x;
    if (i4 >= plane / 4) return;
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2;
    const float inv = 1.0f / (c == 0 ? s0 : c == 1 ? s1 : s2);
    const float w = weight[(nc / 3) / per_sample], u = 1.0f - w;
    const size_t at = (size_t)nc * plane + (size_t)i4 * 4;
    const uint32_t p = *reinterpret_cast<const uint32_t*>(in1 + at);
    const uint32_t q = *reinterpret_cast<const uint32_t*>(in2 + at);
    float a[4], bq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = ((float)((p >> (8 * k)) & 0xff) * (1.0f / 255.0f) - mean) * inv;
        bq[k] = ((float)((q >> (8 * k)) & 0xff) * (1.0f / 255.0f) - mean) * inv;
    }
    // weight 1: 1 * a + 0 * b = a, the bytes of avs_normalize_frames_u8
    *reinterpret_cast<float4*>(out + at) = make_float4(w * a[0] + u * bq[0], w * a[1] + u * bq[1], w * a[2] + u * bq[2], w * a[3] + u * bq[3]);
}

extern "C" int avs_mix_frames_u8(const uint8_t* in1, const uint8_t* in2, const float* weight, float* out, int n_images, int per_sample, int plane,
                                 const float* mean3, const float* std3, hipStream_t stream) {
    AVS_CHECK_ARG(in1 && in2 && weight && out && n_images > 0 && per_sample > 0 && (n_images % per_sample) == 0 && plane > 0 && (plane % 4) == 0 &&
                      mean3 && std3,
                  "mix_frames: bad arguments (H*W %% 4 == 0; n_images a multiple of the images per sample)");
    AVS_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "mix_frames: zero std");
    AVS_CHECK_ARG((long long)n_images * 3 <= 0x7fffffffLL, "mix_frames: too many images");
    dim3 grid(n_images * 3, ceil_div(plane / 4, 256));
    mix_frames_kernel<<<grid, 256, 0, stream>>>(in1, in2, weight, out, plane, per_sample, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    AVS_LAUNCH_CHECK("mix_frames");
    return 0;
}

// ---- decoded-size frames: antialiased bicubic resize, normalisation, mix ---------------------------------------------------------------------
// dataloader_ft.py:136-139, 434-459: frames / 255, Resize([224, 224], BICUBIC, antialias=True), Normalize, then the frame mix - from the uint8
// frames of a decoder, each clip at its own size inside a padded buffer, to the fp32 tensor the model reads.  The specification is
// preprocess.resize_frames_reference (float64); the taps are frontend_math.h's rz_taps, the same text on host and device.
//
// A workgroup of 8 waves owns `rows` output rows of one image, its three channels in turn.  Per channel and source (the clip, then its partner):
//   taps        one thread per output column / output row evaluates its taps in double into LDS (x weights [tap][column], y weights [row][tap]);
//               without a partner the three channels share them
//   horizontal  the source rows the band needs go through LDS RZ_STAGE at a time, a wave per row, read as aligned dwords; a thread takes one
//               output column of RZ_HB staged rows (each weight is read once for the four) and leaves sum_x wx (float)u8 in the LDS intermediate
//   vertical    a thread takes four output columns of one output row: sum_y wy mid[y] on 16-byte LDS reads, normalised as normalize_frames_kernel
//               does; the clip's result waits in LDS for the partner's, the mix is mix_frames_kernel's, the store one float4
// Sums run in tap order in fp32.  The intermediate never leaves LDS; no atomics.  The host sizes `rows` and the LDS regions from the batch's
// largest clip (rz_plan); sizes read on the device are cut to those maxima, so a wrong size array cannot index outside LDS or the buffer.
#define RZ_THREADS 512
#define RZ_STAGE 8                                         // source rows staged at a time: one per wave
#define RZ_HB 4                                            // staged rows per thread of the horizontal pass
#define RZ_LDS_LIMIT 98304                                 // the largest supported case (2240 x 2240 -> 224 x 224, one row per workgroup) takes 95.3 KB
static_assert(RZ_THREADS == 64 * RZ_STAGE && RZ_STAGE % RZ_HB == 0, "one wave per staged row");

struct RzSrc {
    const uint8_t* p;                // [N, 3, Hs, Ws]
    const int* sizes;                // [B, 2] (h, w) per clip, or NULL: (Hs, Ws)
    int Hs, Ws, max_h, max_w;        // max_*: the largest clip of the batch, <= (Hs, Ws): what the LDS regions were sized for
    size_t bytes;                    // of the whole buffer: the dword reads of a row's ends stay inside it
};

struct RzGeo {
    int out_h, out_w, per_sample;
    int rows, tcx, tcy, row_cap, sw; // output rows per workgroup | tap capacity per axis | rows of the intermediate | bytes per staged row
    int mixed;
};

struct RzPlan {
    int rows, tcx, tcy, row_cap, sw;
    int lds_plain, lds_mixed;
};

// LDS regions, in this order: intermediate [row_cap][out_w] | clip's result [rows][out_w] (mixed only) | wx [tcx][out_w] | wy [rows][tcy] |
// x start, x count [out_w] each | y start, y count [rows] each | staged rows [RZ_STAGE][sw]
static int rz_lds_bytes(int out_w, int rows, int tcx, int tcy, int row_cap, int sw, bool mixed) {
    return 4 * (row_cap * out_w + (mixed ? rows * out_w : 0) + tcx * out_w + rows * tcy + 2 * out_w + 2 * rows) + RZ_STAGE * sw;
}

// the most output rows per workgroup whose regions (the mixed form's) fit RZ_LDS_LIMIT; -> 0, or -1 when not even one row fits
static int rz_plan(int max_h, int max_w, int out_h, int out_w, RzPlan* p) {
    p->tcx = rz_tap_cap(max_w, out_w);
    p->tcy = rz_tap_cap(max_h, out_h);
    p->sw = ((max_w + 6) / 4) * 4;                          // a row keeps its byte offset in its first dword (0..3) and ends on a whole dword
    for (int rows = 32; rows >= 1; rows >>= 1) {
        p->rows = rows;
        p->row_cap = rz_row_cap(max_h, out_h, rows);
        p->lds_plain = rz_lds_bytes(out_w, rows, p->tcx, p->tcy, p->row_cap, p->sw, false);
        p->lds_mixed = rz_lds_bytes(out_w, rows, p->tcx, p->tcy, p->row_cap, p->sw, true);
        if (p->lds_mixed <= RZ_LDS_LIMIT) return 0;
    }
    return -1;
}

// grid (N, ceil(out_h / rows)), 512 threads, dynamic LDS
__global__ __launch_bounds__(RZ_THREADS) void resize_frames_kernel(RzSrc A, RzSrc B, const float* __restrict__ weight, float* __restrict__ out, RzGeo G,
                                                                   float m0, float m1, float m2, float s0, float s1, float s2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rz_lds[];
    float* __restrict__ s_mid = reinterpret_cast<float*>(rz_lds);
    float* __restrict__ s_res = s_mid + G.row_cap * G.out_w;
    float* __restrict__ s_wx = s_res + (G.mixed ? G.rows * G.out_w : 0);
    float* __restrict__ s_wy = s_wx + G.tcx * G.out_w;
    int* __restrict__ s_xs = reinterpret_cast<int*>(s_wy + G.rows * G.tcy);
    int* __restrict__ s_xn = s_xs + G.out_w;
    int* __restrict__ s_ys = s_xn + G.out_w;
    int* __restrict__ s_yn = s_ys + G.rows;
    uint8_t* __restrict__ s_stage = reinterpret_cast<uint8_t*>(s_yn + G.rows);

    const int img = blockIdx.x, b = img / G.per_sample;
    const int y0 = blockIdx.y * G.rows, nrows = min(G.rows, G.out_h - y0);       // >= 1 by the grid
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ow = G.out_w, ow4 = ow >> 2;

    // channel by channel; with a partner the clip, then the partner, of each.  Without one the taps of the first channel serve all three
    for (int cs = 0; cs < 3 * (G.mixed + 1); ++cs) {
        const int c = G.mixed ? cs >> 1 : cs, src = G.mixed ? cs & 1 : 0;
        const RzSrc& S = src ? B : A;
        int h = S.sizes ? S.sizes[2 * b] : S.Hs, w = S.sizes ? S.sizes[2 * b + 1] : S.Ws;
        h = max(1, min(h, S.max_h));
        w = max(1, min(w, S.max_w));

        // taps.  Rows are kept relative to the band's first source row; a count is cut where the intermediate ends (never, by rz_row_cap)
        int unused;
        const int row0 = rz_span(h, G.out_h, y0, &unused);
        for (int i = tid; i < ow + nrows && (G.mixed || c == 0); i += RZ_THREADS) {
            int start;
            if (i < ow) {
                s_xn[i] = rz_taps(w, ow, i, G.tcx, &start, s_wx + i, ow);
                s_xs[i] = start;
            } else {
                const int y = i - ow;
                const int n = rz_taps(h, G.out_h, y0 + y, G.tcy, &start, s_wy + y * G.tcy, 1);
                s_ys[y] = min(start - row0, G.row_cap);
                s_yn[y] = max(0, min(n, row0 + G.row_cap - start));
            }
        }
        __syncthreads();
        const int rows_in = s_ys[nrows - 1] + s_yn[nrows - 1];                  // starts and ends do not decrease with the output row

        const uint8_t* lo = S.p;
        const uint8_t* hi = S.p + S.bytes;
        const int nc = img * 3 + c;
        const float mean = c == 0 ? m0 : c == 1 ? m1 : m2;
        const float inv = 1.0f / (c == 0 ? s0 : c == 1 ? s1 : s2);
        const uint8_t* __restrict__ plane = S.p + (size_t)nc * S.Hs * S.Ws;
        for (int c0 = 0; c0 < rows_in; c0 += RZ_STAGE) {
            // stage: wave wv reads source row row0 + c0 + wv as the aligned dwords that cover its w bytes
            if (c0 + wv < rows_in) {
                const uint8_t* rowp = plane + (size_t)(row0 + c0 + wv) * S.Ws;
                const int off = (int)(reinterpret_cast<uintptr_t>(rowp) & 3);
                const uint8_t* a0 = rowp - off;
                const int ndw = (off + w + 3) >> 2;                             // 4 ndw <= w + 6: within sw
                uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(s_stage + wv * G.sw);
                for (int d = lane; d < ndw; d += 64) {
                    const uint8_t* a = a0 + 4 * d;
                    uint32_t v = 0;
                    if (a >= lo && a + 4 <= hi) {
                        v = *reinterpret_cast<const uint32_t*>(a);
                    } else {                                                    // the buffer's first / last dword when its ends are not aligned
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (a + k >= lo && a + k < hi) v |= (uint32_t)a[k] << (8 * k);
                    }
                    dst[d] = v;
                }
            }
            __syncthreads();
            // horizontal: thread -> (group of RZ_HB staged rows, output column)
            for (int it = tid; it < ow * (RZ_STAGE / RZ_HB); it += RZ_THREADS) {
                const int g = it / ow, x = it - g * ow;
                const int xs = s_xs[x], xn = s_xn[x];
                const uint8_t* sp[RZ_HB];
                float acc[RZ_HB];
#pragma unroll
                for (int q = 0; q < RZ_HB; ++q) {
                    const int k = g * RZ_HB + q;
                    const int off = (int)(reinterpret_cast<uintptr_t>(plane + (size_t)(row0 + c0 + k) * S.Ws) & 3);
                    sp[q] = s_stage + k * G.sw + off + xs;
                    acc[q] = 0.f;
                }
                for (int j = 0; j < xn; ++j) {
                    const float wt = s_wx[j * ow + x];
#pragma unroll
                    for (int q = 0; q < RZ_HB; ++q) acc[q] += wt * (float)sp[q][j];
                }
#pragma unroll
                for (int q = 0; q < RZ_HB; ++q) {
                    const int r = c0 + g * RZ_HB + q;
                    if (r < rows_in) s_mid[r * ow + x] = acc[q];                // (a row past rows_in was computed from stale bytes and is dropped)
                }
            }
            __syncthreads();
        }

        // vertical, normalisation, mix: thread -> (output row, four columns)
        for (int it = tid; it < nrows * ow4; it += RZ_THREADS) {
            const int y = it / ow4, x4 = it - y * ow4;
            const int yn = s_yn[y];
            const float4* __restrict__ mid = reinterpret_cast<const float4*>(s_mid) + s_ys[y] * ow4 + x4;
            const float* __restrict__ wy = s_wy + y * G.tcy;
            float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
            for (int j = 0; j < yn; ++j) {
                const float wt = wy[j];
                const float4 v = mid[j * ow4];
                r0 += wt * v.x; r1 += wt * v.y; r2 += wt * v.z; r3 += wt * v.w;
            }
            // normalize_frames_kernel's (x * (1.0f / 255.0f) - mean) * inv and mix_frames_kernel's w * a + u * b, with the contractions the compiler
            // gives those two kernels spelled out (fma(x, 1 / 255, -mean) * inv; fma(u, b, w * a)): left to the compiler the same expressions
            // come out of this kernel as separate multiplies and adds, and a clip at the output size would differ from them in the last bit
            float4 o;
            o.x = fmaf(r0, 1.0f / 255.0f, -mean) * inv;
            o.y = fmaf(r1, 1.0f / 255.0f, -mean) * inv;
            o.z = fmaf(r2, 1.0f / 255.0f, -mean) * inv;
            o.w = fmaf(r3, 1.0f / 255.0f, -mean) * inv;
            if (G.mixed && src == 0) {
                reinterpret_cast<float4*>(s_res)[it] = o;    // read back by this thread
            } else {
                if (G.mixed) {
                    const float wgt = weight[b], u = 1.0f - wgt;
                    const float4 a = reinterpret_cast<const float4*>(s_res)[it];
                    // weight 1: 1 * a + 0 * b = a, the bytes of the plain path
                    o = make_float4(fmaf(u, o.x, wgt * a.x), fmaf(u, o.y, wgt * a.y), fmaf(u, o.z, wgt * a.z), fmaf(u, o.w, wgt * a.w));
                }
                *reinterpret_cast<float4*>(out + ((size_t)nc * G.out_h + y0 + y) * ow + 4 * x4) = o;
            }
        }
        __syncthreads();                                                        // the next pass's taps and intermediate replace these
    }
}

extern "C" int avs_resize_taps(int in_size, int out_size, int* start, int* count, float* weights, int max_taps) {
    AVS_CHECK_ARG(start && count && weights && in_size >= 1 && out_size >= 1 && max_taps >= 1, "resize_taps: bad arguments");
    AVS_CHECK_ARG((long long)in_size <= (long long)RZ_MAX_SCALE * out_size, "resize_taps: %d -> %d: the scale is limited to %d", in_size, out_size, RZ_MAX_SCALE);
    AVS_CHECK_ARG(max_taps >= rz_tap_cap(in_size, out_size), "resize_taps: %d -> %d can take %d taps per output index, max_taps is %d", in_size, out_size,
                  rz_tap_cap(in_size, out_size), max_taps);
    for (int i = 0; i < out_size; ++i) {
        for (int j = 0; j < max_taps; ++j) weights[(size_t)i * max_taps + j] = 0.f;
        count[i] = rz_taps(in_size, out_size, i, max_taps, start + i, weights + (size_t)i * max_taps, 1);
    }
    return 0;
}

static int rz_check_size(const char* who, int max_h, int max_w, int out_h, int out_w) {
    AVS_CHECK_ARG(out_h >= 1 && out_h <= 65535 && out_w >= 4 && out_w <= 65535 && (out_w % 4) == 0, "%s: output %d x %d: out_w must be a multiple of 4", who, out_h, out_w);
    AVS_CHECK_ARG(max_h >= 1 && max_w >= 1 && (long long)max_h <= (long long)RZ_MAX_SCALE * out_h && (long long)max_w <= (long long)RZ_MAX_SCALE * out_w,
                  "%s: %d x %d -> %d x %d: sizes start at 1 and the scale per axis is limited to %d", who, max_h, max_w, out_h, out_w, RZ_MAX_SCALE);
    return 0;
}

extern "C" int avs_resize_plan(int max_h, int max_w, int out_h, int out_w, int* rows_per_wg, int* lds_bytes) {
    AVS_CHECK_ARG(rows_per_wg && lds_bytes, "resize_plan: NULL result pointers");
    if (int rc = rz_check_size("resize_plan", max_h, max_w, out_h, out_w)) return rc;
    RzPlan p;
    AVS_CHECK_ARG(rz_plan(max_h, max_w, out_h, out_w, &p) == 0, "resize_plan: %d x %d -> %d x %d: one output row takes more than %d bytes of LDS", max_h, max_w,
                  out_h, out_w, RZ_LDS_LIMIT);
    *rows_per_wg = p.rows;
    *lds_bytes = p.lds_mixed;
    return 0;
}

extern "C" int avs_resize_frames_u8(const uint8_t* in1, int Hs, int Ws, const int* sizes, int max_h, int max_w, const uint8_t* in2, int Hs2, int Ws2,
                                    const int* sizes2, int max_h2, int max_w2, const float* weight, float* out, int n_images, int per_sample, int out_h,
                                    int out_w, const float* mean3, const float* std3, hipStream_t stream) {
    AVS_CHECK_ARG(in1 && out && mean3 && std3 && n_images > 0 && per_sample > 0 && (n_images % per_sample) == 0 && (long long)n_images * 3 <= 0x7fffffffLL,
                  "resize_frames: bad arguments (in1, out, mean3, std3; n_images a multiple of the images per sample)");
    AVS_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0, "resize_frames: out must be 16-byte aligned");
    AVS_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "resize_frames: zero std");
    AVS_CHECK_ARG(Hs >= 1 && Ws >= 1 && max_h <= Hs && max_w <= Ws, "resize_frames: the largest clip (%d x %d) must fit the buffer (%d x %d)", max_h, max_w, Hs, Ws);
    if (int rc = rz_check_size("resize_frames", max_h, max_w, out_h, out_w)) return rc;
    if (in2) {
        AVS_CHECK_ARG(weight, "resize_frames: a partner needs a weight per clip");
        AVS_CHECK_ARG(Hs2 >= 1 && Ws2 >= 1 && max_h2 <= Hs2 && max_w2 <= Ws2, "resize_frames: the partner's largest clip (%d x %d) must fit its buffer (%d x %d)",
                      max_h2, max_w2, Hs2, Ws2);
        if (int rc = rz_check_size("resize_frames (partner)", max_h2, max_w2, out_h, out_w)) return rc;
    } else {
        AVS_CHECK_ARG(!sizes2 && !weight && Hs2 == 0 && Ws2 == 0 && max_h2 == 0 && max_w2 == 0, "resize_frames: partner sizes / weight without a partner");
    }
    RzPlan p;
    const int ph = in2 && max_h2 > max_h ? max_h2 : max_h, pw = in2 && max_w2 > max_w ? max_w2 : max_w;
    AVS_CHECK_ARG(rz_plan(ph, pw, out_h, out_w, &p) == 0, "resize_frames: %d x %d -> %d x %d: one output row takes more than %d bytes of LDS", ph, pw, out_h, out_w,
                  RZ_LDS_LIMIT);
    static bool attr_done = false;
    static const KernelEntry kernel{(const void*)resize_frames_kernel, RZ_LDS_LIMIT, RZ_THREADS};      // above the 64 KiB a kernel gets without asking
    if (int rc = kernels_ready("resize_frames", attr_done, {{&kernel, 1}})) return rc;
    const RzSrc A{in1, sizes, Hs, Ws, max_h, max_w, (size_t)n_images * 3 * Hs * Ws};
    const RzSrc B{in2, sizes2, Hs2, Ws2, max_h2, max_w2, in2 ? (size_t)n_images * 3 * Hs2 * Ws2 : 0};
    const RzGeo G{out_h, out_w, per_sample, p.rows, p.tcx, p.tcy, p.row_cap, p.sw, in2 ? 1 : 0};
    dim3 grid(n_images, ceil_div(out_h, p.rows));
    resize_frames_kernel<<<grid, RZ_THREADS, in2 ? p.lds_mixed : p.lds_plain, stream>>>(A, B, weight, out, G, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                                                                                        std3[2]);
    AVS_LAUNCH_CHECK("resize_frames");
    return 0;
}
