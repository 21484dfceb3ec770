// The guard of the fine-tuning step: the gradient norm over the segment table of avs_adam_table, the clipping coefficient of
// torch.nn.utils.clip_grad_norm_ and the non-finite skip of torch.cuda.amp.GradScaler.step (the reference's loop,
// src/traintest_ft_base.py:115,162-165), in a device block the guarded Adam reads - no host sync between them.
//   stage 1  one workgroup per chunk of the table (the chunks, the walk and the liveness rule of adam_table.h): the chunk's finite elements
//            squared and summed in fp64, its non-finite ones counted; one 16-byte record per chunk, one writer
//   stage 2  one workgroup: the records added per group and per class, the guard block written
// Every sum has an order fixed by the thread and chunk geometry; there is no atomic anywhere, so two calls give the same bytes.
#include <cfloat>

#include "adam_table.h"

struct GradGuard {
    double sumsq[ADT_NGROUP];
    double sumsq_cls[ADT_NCLS];
    double total;
    float norm, coef;
    int n_nonfinite, skip, n_skipped, n_steps;
};
static_assert(sizeof(GradGuard) == 184, "mirror of avs_grad_guard (include/avsiam_hip.h)");

// one chunk's record.  tag: group << 8 | cls, or -1 for a chunk of a class that is not live (nothing of it was read: sum 0, bad 0)
struct GgPart { double sum; int bad; int tag; };
static_assert(sizeof(GgPart) == 16, "16-byte records");
constexpr int GG_HEAD = 16;                  // bytes in front of the records: int [0] = the table's chunk count, written by workgroup 0
constexpr int GG_BLOCK2 = 1024;              // stage 2's one workgroup
constexpr int GG_TOO_BIG = -1;               // n_nonfinite of a table with more chunks than the workspace holds (the step is skipped)

__device__ __forceinline__ double gg_wave_sum(double x) {         // fixed tree over the 64 lanes; the total lands in lane 0
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    return x;
}
__device__ __forceinline__ int gg_wave_sum(int x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    return x;
}

__global__ __launch_bounds__(ADT_BLOCK) void grad_sumsq_chunks_kernel(const float* __restrict__ g, const AdamSeg* __restrict__ segs, int n_segs,
                                                                      const AdamCtl* __restrict__ ctl, int* __restrict__ head,
                                                                      GgPart* __restrict__ parts, int cap) {
    __shared__ int pre[ADT_MAX_SEGS + 1];
    __shared__ int part[ADT_BLOCK];
    __shared__ int s_live[ADT_NCLS];
    __shared__ double w_sum[ADT_BLOCK / 64];
    __shared__ int w_bad[ADT_BLOCK / 64];
    const int tid = threadIdx.x;
    if (tid < ADT_NCLS) s_live[tid] = ctl->live[tid] > 0.f;
    adt_prefix(segs, n_segs, pre, part);
    const int total = pre[n_segs];
    if (blockIdx.x == 0 && tid == 0) head[0] = total;
    const int end = min(total, cap);                       // (a record past the workspace is never written: stage 2 sees total > cap and skips)
    for (int c = blockIdx.x; c < end; c += gridDim.x) {
        const int lo = adt_find(pre, n_segs, c);
        const AdamSeg sg = segs[lo];
        if (!s_live[sg.cls]) {
            if (tid == 0) parts[c] = GgPart{0.0, 0, -1};
            continue;
        }
        const int first = (c - pre[lo]) * ADT_CHUNK;       // < sg.n
        const int n4 = min(ADT_CHUNK, sg.n - first) / 4;
        const float4* g4 = reinterpret_cast<const float4*>(g + (size_t)sg.lo + (size_t)first);
        float4 x[ADT_CHUNK / 4 / ADT_BLOCK];
#pragma unroll
        for (int k = 0; k < ADT_CHUNK / 4 / ADT_BLOCK; ++k) {
            const int i = tid + k * ADT_BLOCK;
            x[k] = i < n4 ? g4[i] : float4{0.f, 0.f, 0.f, 0.f};
        }
        double acc = 0.0;
        int bad = 0;
#pragma unroll
        for (int k = 0; k < ADT_CHUNK / 4 / ADT_BLOCK; ++k) {
            const float* xp = &x[k].x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool fin = fabsf(xp[j]) <= FLT_MAX;     // false for inf and for NaN
                const double d = fin ? (double)xp[j] : 0.0;
                acc = fma(d, d, acc);
                bad += fin ? 0 : 1;
            }
        }
        acc = gg_wave_sum(acc);
        bad = gg_wave_sum(bad);
        if ((tid & 63) == 0) {
            w_sum[tid >> 6] = acc;
            w_bad[tid >> 6] = bad;
        }
        __syncthreads();
        if (tid == 0) {
            double s = w_sum[0];
            int b = w_bad[0];
#pragma unroll
            for (int w = 1; w < ADT_BLOCK / 64; ++w) {
                s += w_sum[w];
                b += w_bad[w];
            }
            parts[c] = GgPart{s, b, (sg.group << 8) | sg.cls};
        }
        __syncthreads();
    }
}

// Thread t takes the records t, t + GG_BLOCK2, ... in ascending order into one accumulator per group and per class (a record adds its sum to
// its own two and +0.0 to the others, which changes nothing: the sums are >= 0), then the threads are added by a fixed tree: the wave's
// shuffle tree, and the waves' totals in ascending order.
__global__ __launch_bounds__(GG_BLOCK2) void grad_sumsq_finish_kernel(const int* __restrict__ head, const GgPart* __restrict__ parts, int cap,
                                                                      float grad_scale, float max_norm, GradGuard* __restrict__ guard) {
    constexpr int ROWS = ADT_NGROUP + ADT_NCLS, WAVES = GG_BLOCK2 / 64;
    __shared__ double w_sum[ROWS][WAVES];
    __shared__ int w_bad[WAVES];
    __shared__ double row[ROWS];
    const int tid = threadIdx.x;
    const int total = head[0];
    const bool fits = total <= cap;
    double acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.0;
    int bad = 0;
    if (fits) {
        for (int c = tid; c < total; c += GG_BLOCK2) {
            const GgPart q = parts[c];
            const int grp = q.tag >> 8, cls = q.tag & 255;   // tag -1: group -1, no row takes the (zero) sum
#pragma unroll
            for (int r = 0; r < ADT_NGROUP; ++r) acc[r] += (q.tag >= 0 && grp == r) ? q.sum : 0.0;
#pragma unroll
            for (int r = 0; r < ADT_NCLS; ++r) acc[ADT_NGROUP + r] += (q.tag >= 0 && cls == r) ? q.sum : 0.0;
            bad += q.bad;
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const double s = gg_wave_sum(acc[r]);
        if ((tid & 63) == 0) w_sum[r][tid >> 6] = s;
    }
    bad = gg_wave_sum(bad);
    if ((tid & 63) == 0) w_bad[tid >> 6] = bad;
    __syncthreads();
    if (tid < ROWS) {
        double s = w_sum[tid][0];
        for (int w = 1; w < WAVES; ++w) s += w_sum[tid][w];
        row[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int nbad = 0;
        for (int w = 0; w < WAVES; ++w) nbad += w_bad[w];
        if (!fits) nbad = GG_TOO_BIG;
        for (int r = 0; r < ADT_NGROUP; ++r) guard->sumsq[r] = row[r];
        for (int r = 0; r < ADT_NCLS; ++r) guard->sumsq_cls[r] = row[ADT_NGROUP + r];
        const double tot = row[0] + row[1] + row[2];
        const float norm = (float)(sqrt(tot) * (double)grad_scale);
        const int skip = nbad != 0;
        const float coef = skip ? 0.f : fminf(1.0f, max_norm / (norm + 1e-6f));      // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to 1
        guard->total = tot;
        guard->norm = norm;
        guard->coef = coef;
        guard->n_nonfinite = nbad;
        guard->skip = skip;
        guard->n_skipped += skip;
        guard->n_steps += 1;
    }
}

__global__ __launch_bounds__(ADT_BLOCK) void adam_table_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                       float* __restrict__ v, bf16_t* __restrict__ pb,
                                                                       const AdamSeg* __restrict__ segs, int n_segs, const AdamCtl* __restrict__ ctl,
                                                                       float b1, float b2, float eps, float wd, float gscale,
                                                                       const GradGuard* __restrict__ guard) {
    if (guard->skip) return;                                // the same answer in every workgroup: nothing of p, m, v, p_bf16 is written
    adam_table_body(p, g, m, v, pb, segs, n_segs, ctl, b1, b2, eps, wd, gscale * guard->coef);
}

// step[c] += (live[c] > 0) unless the step was skipped: behind the update, as adam_table_advance_kernel is
__global__ void adam_table_guarded_advance_kernel(AdamCtl* ctl, const GradGuard* __restrict__ guard) {
    const int c = threadIdx.x;
    if (guard->skip) return;
    if (c < ADT_NCLS && ctl->live[c] > 0.f) ctl->step[c] += 1;
}

// ===================================================================================================
extern "C" size_t avs_grad_sumsq_ws_bytes(int n_segs, long long n_chunks) {
    if (n_segs < 1 || n_segs > ADT_MAX_SEGS || n_chunks < 1 || n_chunks > (1ll << 30)) return 0;
    return (size_t)GG_HEAD + (size_t)n_chunks * sizeof(GgPart);
}

extern "C" int avs_grad_sumsq(const float* g, const AdamSeg* segs, int n_segs, const AdamCtl* ctl, float grad_scale, float max_norm,
                              GradGuard* guard, void* ws, size_t ws_bytes, hipStream_t stream) {
    AVS_CHECK_ARG(g && segs && ctl && guard && ws && n_segs >= 1 && n_segs <= ADT_MAX_SEGS,
                  "grad_sumsq: g, segs, ctl, guard, ws must not be NULL, n_segs in 1..%d (got %d)", ADT_MAX_SEGS, n_segs);
    AVS_CHECK_ARG(max_norm > 0.f && fabsf(grad_scale) <= FLT_MAX, "grad_sumsq: max_norm must be > 0 (inf: no clipping), grad_scale finite");
    AVS_CHECK_ARG(ws_bytes >= GG_HEAD + sizeof(GgPart) && ((size_t)ws & 15) == 0 && ((size_t)g & 15) == 0 && ((size_t)guard & 7) == 0,
                  "grad_sumsq: ws holds %zu bytes, avs_grad_sumsq_ws_bytes(n_segs, n_chunks) are needed; g and ws 16-byte aligned, guard 8-byte",
                  ws_bytes);
    const size_t room = (ws_bytes - GG_HEAD) / sizeof(GgPart);
    const int cap = (int)(room < (size_t)(1 << 30) ? room : (size_t)(1 << 30));
    int* head = reinterpret_cast<int*>(ws);
    GgPart* parts = reinterpret_cast<GgPart*>(reinterpret_cast<char*>(ws) + GG_HEAD);
    grad_sumsq_chunks_kernel<<<cap < ADT_GRID ? cap : ADT_GRID, ADT_BLOCK, 0, stream>>>(g, segs, n_segs, ctl, head, parts, cap);
    AVS_LAUNCH_CHECK("grad_sumsq");
    grad_sumsq_finish_kernel<<<1, GG_BLOCK2, 0, stream>>>(head, parts, cap, grad_scale, max_norm, guard);
    AVS_LAUNCH_CHECK("grad_sumsq (finish)");
    return 0;
}

extern "C" int avs_adam_table_guarded(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, const AdamSeg* segs, int n_segs,
                                      long long n_chunks, AdamCtl* ctl, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                      const GradGuard* guard, hipStream_t stream) {
    AVS_CHECK_ARG(p && g && m && v && segs && ctl && guard && n_segs >= 1 && n_segs <= ADT_MAX_SEGS && n_chunks >= 1,
                  "adam_table_guarded: p, g, m, v, segs, ctl, guard must not be NULL, n_segs in 1..%d (got %d), n_chunks >= 1", ADT_MAX_SEGS, n_segs);
    const int grid = (int)(n_chunks < ADT_GRID ? n_chunks : ADT_GRID);
    adam_table_guarded_kernel<<<grid, ADT_BLOCK, 0, stream>>>(p, g, m, v, p_bf16, segs, n_segs, ctl, beta1, beta2, eps, weight_decay, grad_scale,
                                                              guard);
    AVS_LAUNCH_CHECK("adam_table_guarded");
    adam_table_guarded_advance_kernel<<<1, 64, 0, stream>>>(ctl, guard);
    AVS_LAUNCH_CHECK("adam_table_guarded (step counts)");
    return 0;
}
