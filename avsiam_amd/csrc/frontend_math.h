// Arithmetic of the front end (frontend.hip) that does not depend on where it runs.  Kaldi fbank: the shape constants, the host tables
// (float64, rounded once to fp32) and one lane's share of a radix-8 Stockham pass of the 512-point FFT.  Frame resize: the taps of the
// antialiased bicubic filter (at the end of the file).  Host and device compile the same text, so the index arithmetic of the kernels can be
// walked lane by lane on a CPU.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define FB_NFFT 512                  // round_to_power_of_two(400)
#define FB_FRAME 400                 // 25 ms at 16 kHz
#define FB_SHIFT 160                 // 10 ms
#define FB_NMEL 128
#define FB_NBIN 256                  // bins 0..255 carry mel weight; bin 256 (Nyquist) has weight 0
#define FB_MELW 10                   // widest filter, in bins (checked when the table is built)
#define FB_EPS 1.1920929e-07f        // FLT_EPSILON: the floor of the mel energies
#define FB_LOG_EPS (-15.942385f)     // fp32(ln(double(FLT_EPSILON))): what an energy at or below the floor becomes

// table block, in 4-byte words: twiddles exp(-2 pi i k / 512) as (cos, -sin) pairs | window | mel weights [128][10] | first bin [128] | bins [128]
#define FB_TAB_TW 0
#define FB_TAB_WIN (FB_TAB_TW + 2 * FB_NFFT)
#define FB_TAB_MELW (FB_TAB_WIN + FB_FRAME)
#define FB_TAB_FIRST (FB_TAB_MELW + FB_NMEL * FB_MELW)
#define FB_TAB_COUNT (FB_TAB_FIRST + FB_NMEL)
#define FB_TAB_WORDS (FB_TAB_COUNT + FB_NMEL)

// LDS index of FFT element i: one pad word per 8 keeps the stride-8 and stride-64 accesses of the passes off a single bank
__host__ __device__ inline int fb_pad(int i) { return i + (i >> 3); }
#define FB_BUF (FB_NFFT + FB_NFFT / 8)

// 8-point DFT, forward (exp(-2 pi i n k / 8)), natural order in and out
__host__ __device__ inline void fb_dft8(float* xr, float* xi) {
    const float h = 0.70710678118654752f;
    float ar[4], ai[4], br[4], bi[4];
    for (int n = 0; n < 4; ++n) {
        ar[n] = xr[n] + xr[n + 4]; ai[n] = xi[n] + xi[n + 4];
        br[n] = xr[n] - xr[n + 4]; bi[n] = xi[n] - xi[n + 4];
    }
    // b[n] *= W8^n: 1, (1 - i) / sqrt 2, -i, (-1 - i) / sqrt 2
    float t;
    t = br[1]; br[1] = (t + bi[1]) * h; bi[1] = (bi[1] - t) * h;
    t = br[2]; br[2] = bi[2]; bi[2] = -t;
    t = br[3]; br[3] = (bi[3] - t) * h; bi[3] = -(t + bi[3]) * h;
    // two 4-point DFTs: even outputs from a, odd outputs from b
    for (int half = 0; half < 2; ++half) {
        const float* cr = half ? br : ar;
        const float* ci = half ? bi : ai;
        const float p0r = cr[0] + cr[2], p0i = ci[0] + ci[2], p1r = cr[1] + cr[3], p1i = ci[1] + ci[3];
        const float q0r = cr[0] - cr[2], q0i = ci[0] - ci[2];
        const float q1r = ci[1] - ci[3], q1i = -(cr[1] - cr[3]);          // (c1 - c3) * -i
        xr[0 + half] = p0r + p1r; xi[0 + half] = p0i + p1i;
        xr[4 + half] = p0r - p1r; xi[4 + half] = p0i - p1i;
        xr[2 + half] = q0r + q1r; xi[2 + half] = q0i + q1i;
        xr[6 + half] = q0r - q1r; xi[6 + half] = q0i - q1i;
    }
}

// Stockham radix-8 pass NS (1, 8, 64) of the 512-point transform, lane j of 64: v[r] holds element j + 64 r of the pass's input.
// Multiplies by the pass's twiddles (tw: FB_TAB_TW pairs), transforms, and returns in `base` where output r goes: base + r * NS.
template <int NS>
__host__ __device__ inline int fb_pass(int j, float* vr, float* vi, const float* tw) {
    if (NS > 1) {
        const int k = (j & (NS - 1)) * (FB_NFFT / (NS * 8));
        for (int r = 1; r < 8; ++r) {
            const float c = tw[2 * r * k], s = tw[2 * r * k + 1];
            const float re = vr[r] * c - vi[r] * s;
            vi[r] = vr[r] * s + vi[r] * c;
            vr[r] = re;
        }
    }
    fb_dft8(vr, vi);
    return (j / NS) * NS * 8 + (j & (NS - 1));
}

static inline double fb_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

// the tables, computed in float64 and rounded once.  -> 0, or -1 when a filter is wider than FB_MELW bins (never at this shape)
static inline int fb_build_tables(float* tab) {
    const double pi = 3.14159265358979323846;
    int* itab = reinterpret_cast<int*>(tab);
    for (int k = 0; k < FB_NFFT; ++k) {
        tab[FB_TAB_TW + 2 * k] = (float)cos(2.0 * pi * k / FB_NFFT);
        tab[FB_TAB_TW + 2 * k + 1] = (float)(-sin(2.0 * pi * k / FB_NFFT));
    }
    for (int i = 0; i < FB_FRAME; ++i) tab[FB_TAB_WIN + i] = (float)(0.5 - 0.5 * cos(2.0 * pi * i / (FB_FRAME - 1)));
    const double lo = fb_mel(20.0), hi = fb_mel(8000.0), delta = (hi - lo) / (FB_NMEL + 1);
    for (int k = 0; k < FB_NMEL; ++k) {
        const double left = lo + k * delta, centre = left + delta, right = centre + delta;
        int first = 0, count = 0;
        for (int i = 0; i < FB_MELW; ++i) tab[FB_TAB_MELW + k * FB_MELW + i] = 0.f;
        for (int b = 0; b < FB_NBIN; ++b) {
            const double m = fb_mel(31.25 * b);
            const double up = (m - left) / delta, down = (right - m) / delta;
            const double w = up < down ? up : down;
            if (w > 0.0) {
                if (count == 0) first = b;
                if (b - first >= FB_MELW) return -1;
                tab[FB_TAB_MELW + k * FB_MELW + (b - first)] = (float)w;
                count = b - first + 1;
            }
        }
        itab[FB_TAB_FIRST + k] = first;
        itab[FB_TAB_COUNT + k] = count;
    }
    return 0;
}

// ---- antialiased bicubic resize (torch interpolate(mode='bicubic', align_corners=False, antialias=True), what torchvision's Resize calls) --------
// Per axis, input size I, output size O, all in float64: scale = I / O, s = max(scale, 1), support = 2 s; output index i has its centre at
// scale (i + 0.5), takes the input indices [start, start + n) = [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), I)) with
// weights cubic((j + start - centre + 0.5) / s), a = -0.5, divided by their sum (added in tap order) and rounded once to fp32.
// Every product and sum below is rounded on its own (no fused multiply-add): host, device and numpy give the same bits.
#define RZ_MAX_TAPS 41               // 2 support + 1 at the largest scale
#define RZ_MAX_SCALE 10              // in / out per axis: 1080p -> 224 is 8.6

__host__ __device__ inline double rz_cubic(double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double ax = x < 0.0 ? -x : x;
    if (ax < 1.0) return (1.5 * ax - 2.5) * ax * ax + 1.0;
    if (ax < 2.0) return (((ax - 5.0) * ax + 8.0) * ax - 4.0) * -0.5;
    return 0.0;
}

// first input index and tap count of output index i
__host__ __device__ inline int rz_span(int in_size, int out_size, int i, int* count) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double scale = (double)in_size / (double)out_size, s = scale < 1.0 ? 1.0 : scale, support = 2.0 * s;
    const double centre = scale * ((double)i + 0.5);
    int start = (int)(centre - support + 0.5), end = (int)(centre + support + 0.5);
    if (start < 0) start = 0;
    if (end > in_size) end = in_size;
    *count = end - start;
    return start;
}

// taps of output index i: weight j goes to w[j * wstride], j < the returned count (cut at max_taps: callers size max_taps from the scale, see
// rz_tap_cap, so nothing is cut within the supported range).  No local array: the weights are evaluated twice, once for their sum.
__host__ __device__ inline int rz_taps(int in_size, int out_size, int i, int max_taps, int* start_out, float* w, int wstride) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    int n;
    const int start = rz_span(in_size, out_size, i, &n);
    if (n > max_taps) n = max_taps;
    const double scale = (double)in_size / (double)out_size, s = scale < 1.0 ? 1.0 : scale;
    const double centre = scale * ((double)i + 0.5);
    double total = 0.0;
    for (int j = 0; j < n; ++j) total += rz_cubic(((double)(j + start) - centre + 0.5) / s);
    for (int j = 0; j < n; ++j) w[j * wstride] = (float)(rz_cubic(((double)(j + start) - centre + 0.5) / s) / total);
    *start_out = start;
    return n;
}

// no output index of an axis has more taps than this: end - start <= ceil(2 support) (one more against the rounding of the scale)
static inline int rz_tap_cap(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size, s = scale < 1.0 ? 1.0 : scale;
    const int cap = (int)ceil(4.0 * s) + 1;
    return cap > RZ_MAX_TAPS ? RZ_MAX_TAPS : cap;
}

// input rows that `rows` consecutive output rows span: last end - first start <= scale (rows - 1) + 2 support + 1
static inline int rz_row_cap(int in_size, int out_size, int rows) {
    const double scale = (double)in_size / (double)out_size, s = scale < 1.0 ? 1.0 : scale;
    const int cap = (int)ceil(scale * (rows - 1) + 4.0 * s) + 2;
    return cap > in_size ? in_size : cap;
}
