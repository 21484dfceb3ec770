// k14 - source-rate audio on the device: what the reference's loader does to decoded PCM ahead of the fbank
// (dataloader_ft.py:272-277, 298-306): torchaudio.functional.resample(waveform, sr, 16000) when the file is not at 16 kHz
// (windowed sinc, sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and waveform.mean(dim=0) over the channels.  The specification is
// avsiam_amd.preprocess.resample_reference (float64) around preprocess.resample_table_reference; include/avsiam_hip.h states the contract.
//
// With o = rate / gcd, n = 16000 / gcd, output j = q n + p (0 <= p < n) of a channel is sum_m table[p, m] x[q o + m - width].  The table
// comes from Python (built with torch so that torch's own sin and type promotion decide its bits) and is COMPACT: in fp32 every phase has one
// contiguous run of non-zero taps (34 of 475 at 44.1 kHz), so a phase is `first` and K weights, K the table's longest run.
//
// A workgroup owns RS_TILE consecutive outputs of one clip.  It copies the clip's table into LDS once, then per channel the tile's input span
// (zero beyond the clip's ends), and every thread accumulates RS_PER outputs RS_THREADS apart - adjacent lanes own adjacent outputs, so the
// stores coalesce, adjacent lanes read table rows one odd pitch apart (conflict-free: ds_read_b32 banks are word mod 32) or one row
// (n = 1, 2: a broadcast), and samples about o / n words apart.  One thread division finds (q, p) of its first output; the others follow by
// adding the host-prepared (RS_THREADS / n, RS_THREADS % n).  The channel sum is kept in registers across the channel loop; one writer per
// cell, no atomics.
#include "common.h"

#define RS_THREADS 256
#define RS_PER 4
#define RS_TILE (RS_THREADS * RS_PER)
#define RS_MAX_TABLES 8
#define RS_MAX_CHANNELS 8
#define RS_MAX_WORDS 16384                                      // compact table: n firsts + n * pitch weights
#define RS_MAX_SPAN 16384                                       // words of one channel's input span
#define RS_LDS_LIMIT ((RS_MAX_WORDS + RS_MAX_SPAN) * 4)

struct RsTab {
    const float* tab;                                           // device: int first[n], then float w[n][pitch]
    int o, n, width, taps, pitch;                               // taps = K; pitch = K | 1
    int dq, dp;                                                 // RS_THREADS / n, RS_THREADS % n
};

struct RsTabs {
    RsTab t[RS_MAX_TABLES];
};

static __device__ __forceinline__ int rs_len(const int* __restrict__ len, int b, int stride) {
    const int l = len ? len[b] : stride;
    return l < 0 ? 0 : l > stride ? stride : l;
}

// grid (ceil(out_stride / RS_TILE), B), RS_THREADS threads, dynamic LDS: the largest table of the call and the largest span
__global__ __launch_bounds__(RS_THREADS) void resample_wave_kernel(const float* __restrict__ wave, int C, int stride, const int* __restrict__ len,
                                                                   const int* __restrict__ tab_idx, RsTabs tabs, float* __restrict__ out,
                                                                   int out_stride, int* __restrict__ out_len, int span_off, int vec_ok) {
    extern __shared__ __align__(16) float s_mem[];
    const int b = blockIdx.y, j0 = blockIdx.x * RS_TILE, tid = threadIdx.x;
    const int n_in = rs_len(len, b, stride);
    const int ti = tab_idx[b];
    const float* __restrict__ x0 = wave + (size_t)b * C * stride;
    float* __restrict__ orow = out + (size_t)b * out_stride;
    const float fc = (float)C;

    if (ti < 0 || ti >= RS_MAX_TABLES) {                        // pass-through: the channel mean (C = 1: the input's bytes)
        const int n_copy = min(n_in, out_stride);
        if (blockIdx.x == 0 && tid == 0) out_len[b] = n_copy;
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) {
            const int j = j0 + tid + RS_THREADS * k;
            if (j >= out_stride) break;
            float s = 0.f;
            if (j < n_copy) {                                   // (n_copy <= stride)
                s = x0[j];
                for (int c = 1; c < C; ++c) s += x0[(size_t)c * stride + j];
                if (C > 1) s = s / fc;
            }
            orow[j] = s;
        }
        return;
    }

    // (selected by a uniform index: the struct lives in scalar registers / the kernel argument segment)
    const RsTab T = tabs.t[ti];
    const int o = T.o, n = T.n;
    // ceil(n len / o): the product reaches 2^31 for long clips at high rates
    long long ol = ((long long)n * (long long)n_in + (long long)(o - 1)) / (long long)o;
    const int n_out = ol > (long long)out_stride ? out_stride : (int)ol;      // (<= out_stride by the host's choice of out_stride)
    if (blockIdx.x == 0 && tid == 0) out_len[b] = n_out;

    const int j_end = min(j0 + RS_TILE, n_out);                 // outputs [j0, j_end) are the clip's; the rest of the tile is zero
    if (j_end <= j0) {
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) {
            const int j = j0 + tid + RS_THREADS * k;
            if (j < out_stride) orow[j] = 0.f;
        }
        return;                                                 // (uniform over the workgroup)
    }

    // the table -> LDS
    const int words = n + n * T.pitch;
    for (int i = tid; i < words; i += RS_THREADS) s_mem[i] = T.tab[i];
    const int* __restrict__ s_first = reinterpret_cast<const int*>(s_mem);
    const float* __restrict__ s_w = s_mem + n;
    float* __restrict__ s_x = s_mem + span_off;

    // the span of the tile: inputs [i0, i0 + ns), i0 = q0 o - width, up to the last output's last tap
    const int q0 = j0 / n, ql = (j_end - 1) / n;                // (uniform)
    const int i0 = q0 * o - T.width;
    const int ns = (ql - q0) * o + 2 * T.width + o;
    // start of the copy: i0 rounded down to a multiple of 4 where the channel rows are 16-byte aligned (stride % 4 == 0, aligned base)
    const int a0 = vec_ok ? (i0 & ~3) : i0;
    const int nc = ns + (i0 - a0);                              // words to fill from a0

    // this thread's outputs: (q, p) of the first, relative sample offset of each
    int q = (j0 + tid) / n, p = (j0 + tid) - q * n;
    int xoff[RS_PER], woff[RS_PER];
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        const bool live = j0 + tid + RS_THREADS * k < j_end;
        const int pp = live ? p : 0, qq = live ? q : q0;        // a dead slot reads a valid place and writes zero
        xoff[k] = (qq - q0) * o + (i0 - a0);                    // (the phase's first tap is added after the barrier)
        woff[k] = pp;
        q += T.dq; p += T.dp;
        if (p >= n) { p -= n; q += 1; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        xoff[k] += min(max(s_first[woff[k]], 0), 2 * T.width + o - T.taps);      // (a well-formed table is inside already)
        woff[k] *= T.pitch;
    }

    float sum[RS_PER];
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ xc = x0 + (size_t)c * stride;
        if (c > 0) __syncthreads();                             // every read of the previous channel's span is done
        if (vec_ok) {
            for (int i = 4 * tid; i < nc; i += 4 * RS_THREADS) {
                const int g = a0 + i;
                float4 v;
                if (g >= 0 && g + 3 < n_in) {
                    v = *reinterpret_cast<const float4*>(xc + g);
                } else {
                    v.x = (g >= 0 && g < n_in) ? xc[g] : 0.f;
                    v.y = (g + 1 >= 0 && g + 1 < n_in) ? xc[g + 1] : 0.f;
                    v.z = (g + 2 >= 0 && g + 2 < n_in) ? xc[g + 2] : 0.f;
                    v.w = (g + 3 >= 0 && g + 3 < n_in) ? xc[g + 3] : 0.f;
                }
                *reinterpret_cast<float4*>(s_x + i) = v;
            }
        } else {
            for (int i = tid; i < nc; i += RS_THREADS) {
                const int g = a0 + i;
                s_x[i] = (g >= 0 && g < n_in) ? xc[g] : 0.f;
            }
        }
        __syncthreads();
        float acc[RS_PER];
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) acc[k] = 0.f;
        for (int m = 0; m < T.taps; ++m) {                      // tap order; the thread's outputs side by side
#pragma unroll
            for (int k = 0; k < RS_PER; ++k) acc[k] += s_w[woff[k] + m] * s_x[xoff[k] + m];
        }
#pragma unroll
        for (int k = 0; k < RS_PER; ++k) sum[k] = c == 0 ? acc[k] : sum[k] + acc[k];
    }
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
        const int j = j0 + tid + RS_THREADS * k;
        if (j < out_stride) orow[j] = j < j_end ? (C > 1 ? sum[k] / fc : sum[k]) : 0.f;
    }
}

static int rs_span_words(int o, int n, int width) {
    // the tile's outputs cover at most (RS_TILE - 1) / n + 1 steps of q after the first; + 3 for the aligned start, rounded up to a float4
    const long long w = ((long long)((RS_TILE - 1) / n + 1)) * o + 2LL * width + o + 3;
    return w > 0x7fffffffLL - 8 ? -1 : (int)((w + 3) & ~3LL);
}

extern "C" int avs_resample_plan(int o, int n, int width, int taps, int* table_words, int* span_words) {
    AVS_CHECK_ARG(table_words && span_words, "resample_plan: NULL result pointers");
    AVS_CHECK_ARG(o >= 1 && n >= 1 && width >= 1 && taps >= 1 && taps <= 2 * width + o, "resample_plan: bad geometry (o %d, n %d, width %d, taps %d)", o, n,
                  width, taps);
    const long long tw = (long long)n * ((taps | 1) + 1);
    *table_words = tw > 0x7fffffffLL ? 0x7fffffff : (int)tw;
    *span_words = rs_span_words(o, n, width);
    return 0;
}

extern "C" int avs_resample_wave(const float* wave, int B, int C, long long stride, const int* len, const int* tab_idx, int n_tables,
                                 const void* const* tables, const int* geo, float* out, long long out_stride, int* out_len, hipStream_t stream) {
    AVS_CHECK_ARG(wave && out && out_len && tab_idx && B > 0 && B <= 65535 && C >= 1 && C <= RS_MAX_CHANNELS && stride >= 1 && stride <= 0x7fffffffLL - 65536,
                  "resample_wave: bad arguments (wave, out, out_len, tab_idx; 1 <= B <= 65535; 1 <= C <= %d; 1 <= stride < 2^31 - 2^16)", RS_MAX_CHANNELS);
    AVS_CHECK_ARG(out_stride >= 1 && out_stride <= 0x7fffffffLL - RS_TILE, "resample_wave: out_stride outside 1 .. 2^31 - %d", RS_TILE + 1);
    AVS_CHECK_ARG(n_tables >= 0 && n_tables <= RS_MAX_TABLES && (n_tables == 0 || (tables && geo)), "resample_wave: 0 .. %d tables, with their geometry",
                  RS_MAX_TABLES);
    RsTabs tabs;
    int max_words = 0, max_span = 0;
    long long need = 1;
    for (int i = 0; i < RS_MAX_TABLES; ++i) {
        RsTab& t = tabs.t[i];
        if (i >= n_tables) {
            t = RsTab{nullptr, 1, 1, 1, 1, 1, RS_THREADS, 0};
            continue;
        }
        const int o = geo[4 * i], n = geo[4 * i + 1], width = geo[4 * i + 2], taps = geo[4 * i + 3];
        AVS_CHECK_ARG(tables[i] && o >= 1 && n >= 1 && width >= 1 && taps >= 1 && taps <= 2 * width + o, "resample_wave: table %d: bad geometry (o %d, n %d, width %d, taps %d)",
                      i, o, n, width, taps);
        const int pitch = taps | 1;
        const long long words = (long long)n * (pitch + 1);
        AVS_CHECK_ARG(words <= RS_MAX_WORDS, "resample_wave: table %d (%d phases x %d taps) takes %lld words: compact tables above %d words are refused", i, n,
                      taps, words, RS_MAX_WORDS);
        const int span = rs_span_words(o, n, width);
        AVS_CHECK_ARG(span > 0 && span <= RS_MAX_SPAN, "resample_wave: table %d (%d -> %d): the input span of %d outputs takes more than %d words", i, o, n, RS_TILE,
                      RS_MAX_SPAN);
        t = RsTab{static_cast<const float*>(tables[i]), o, n, width, taps, pitch, RS_THREADS / n, RS_THREADS % n};
        if ((int)words > max_words) max_words = (int)words;
        if (span > max_span) max_span = span;
        const long long ol = ((long long)n * stride + (o - 1)) / o;
        if (ol > need) need = ol;
    }
    // every resampled clip's outputs fit its row (a pass-through clip is cut to the row by the kernel: the caller sizes the row for it)
    AVS_CHECK_ARG(out_stride >= need, "resample_wave: out_stride %lld is below the %lld outputs a clip of %lld samples can give", out_stride, need, stride);
    const int span_off = (max_words + 3) & ~3;
    const size_t lds = (size_t)(span_off + max_span) * 4;
    static bool attr_done = false;
    static const KernelEntry kernel{(const void*)resample_wave_kernel, RS_LDS_LIMIT, RS_THREADS};      // above the 64 KiB a kernel gets without asking
    if (int rc = kernels_ready("resample_wave", attr_done, {{&kernel, 1}})) return rc;
    const int vec_ok = (stride % 4 == 0) && (reinterpret_cast<uintptr_t>(wave) & 15) == 0;
    dim3 grid((unsigned)((out_stride + RS_TILE - 1) / RS_TILE), B);
    resample_wave_kernel<<<grid, RS_THREADS, lds, stream>>>(wave, C, (int)stride, len, tab_idx, tabs, out, (int)out_stride, out_len, span_off, vec_ok);
    AVS_LAUNCH_CHECK("resample_wave");
    return 0;
}
