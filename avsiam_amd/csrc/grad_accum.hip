// Gradient accumulation over micro-batches (include/avsiam_hip.h, avs_grad_accum): acc (+)= g over the segment table of avs_adam_table, and the
// bookkeeping of which gradient classes the accumulated step must update - both on the device, because the classes a micro-step reached are
// known only there (data parallel: the all-reduced liveness vector; mm_grad: every micro-step draws its own branch).
//   kernel 1  the chunks, the walk and the liveness rule of adam_table.h.  A chunk of a class that is live NOW is copied (first micro-step of the
//             cycle, or the class's first touch in it: acc never needs a zero-fill, and every bit of g survives) or added, one fp32 add per element.
//             A chunk of a class that is not live now is skipped before any of its memory is touched.
//   kernel 2  one workgroup, behind the first in stream order (the first reads both blocks): the cycle's union, the micro-step count and - with
//             publish - ctl->live <- the union, so that the guard and the Adam that follow walk the classes of the whole cycle.
// One writer per element, no atomics: two call sequences give the same bytes.
#include "adam_table.h"

struct GradAccumCtl { float live[ADT_NCLS]; int n_micro; int n_cycles; };
static_assert(sizeof(GradAccumCtl) == 72, "mirror of avs_grad_accum_ctl (include/avsiam_hip.h)");

constexpr int GA_PER = ADT_CHUNK / 4 / ADT_BLOCK;           // float4 per thread and chunk
static_assert(GA_PER * 4 * ADT_BLOCK == ADT_CHUNK, "a chunk is a whole number of float4 rounds of the workgroup");

__global__ __launch_bounds__(ADT_BLOCK) void grad_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, const AdamSeg* __restrict__ segs,
                                                               int n_segs, const AdamCtl* __restrict__ ctl, const GradAccumCtl* __restrict__ actl,
                                                               int first) {
    // one add per element and nothing to fuse it with; contraction is switched off all the same, as in the table's other kernels
#pragma clang fp contract(off)
    __shared__ int pre[ADT_MAX_SEGS + 1];
    __shared__ int part[ADT_BLOCK];
    __shared__ int s_mode[ADT_NCLS];                        // 0: not live now, 1: copy, 2: add
    const int tid = threadIdx.x;
    if (tid < ADT_NCLS) {
        const bool now = ctl->live[tid] > 0.f;
        const bool had = !first && actl->live[tid] > 0.f;
        s_mode[tid] = now ? (had ? 2 : 1) : 0;
    }
    adt_prefix(segs, n_segs, pre, part);
    const int total = pre[n_segs];
    // The descriptor of the NEXT chunk (binary search in LDS, then a dependent 24-byte read of the table) is fetched behind the loads of this
    // one: the table walk costs a trip no latency of its own.
    int c = blockIdx.x, lo = 0;
    AdamSeg sg{0, 0, 0, 0};
    if (c < total) {
        lo = adt_find(pre, n_segs, c);
        sg = segs[lo];
    }
    while (c < total) {
        const int mode = s_mode[sg.cls];
        const int start = (c - pre[lo]) * ADT_CHUNK;        // < sg.n
        const size_t off = (size_t)sg.lo + (size_t)start;
        const int n4 = mode ? min(ADT_CHUNK, sg.n - start) / 4 : 0;        // a chunk that is not live now: no load, no store
        float4* a4 = reinterpret_cast<float4*>(acc + off);
        const float4* g4 = reinterpret_cast<const float4*>(g + off);
        float4 x[GA_PER], y[GA_PER];
#pragma unroll
        for (int k = 0; k < GA_PER; ++k) {
            const int i = tid + k * ADT_BLOCK;
            if (i < n4) x[k] = g4[i];
        }
        if (mode == 2) {
#pragma unroll
            for (int k = 0; k < GA_PER; ++k) {
                const int i = tid + k * ADT_BLOCK;
                if (i < n4) y[k] = a4[i];
            }
        }
        const int c_next = c + gridDim.x;
        int lo_next = lo;
        AdamSeg sg_next = sg;
        if (c_next < total) {
            lo_next = adt_find(pre, n_segs, c_next);
            sg_next = segs[lo_next];
        }
        if (mode == 2) {
#pragma unroll
            for (int k = 0; k < GA_PER; ++k) {
                const int i = tid + k * ADT_BLOCK;
                if (i < n4) {
                    x[k].x = y[k].x + x[k].x;
                    x[k].y = y[k].y + x[k].y;
                    x[k].z = y[k].z + x[k].z;
                    x[k].w = y[k].w + x[k].w;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < GA_PER; ++k) {
            const int i = tid + k * ADT_BLOCK;
            if (i < n4) a4[i] = x[k];
        }
        c = c_next;
        lo = lo_next;
        sg = sg_next;
    }
}

// the cycle's bookkeeping: every value has one writer (thread c for class c, thread 0 for the counters)
__global__ void grad_accum_finish_kernel(AdamCtl* ctl, GradAccumCtl* actl, int first, int publish) {
    const int c = threadIdx.x;
    if (c < ADT_NCLS) {
        const bool now = ctl->live[c] > 0.f;
        const bool had = !first && actl->live[c] > 0.f;
        const float u = (had || now) ? 1.f : 0.f;
        actl->live[c] = u;
        if (publish) ctl->live[c] = u;
    }
    if (c == 0) {
        actl->n_micro = first ? 1 : actl->n_micro + 1;
        if (publish) actl->n_cycles += 1;
    }
}

// ===================================================================================================
extern "C" int avs_grad_accum(float* acc, const float* g, const AdamSeg* segs, int n_segs, long long n_chunks, AdamCtl* ctl, GradAccumCtl* actl,
                              int first, int publish, hipStream_t stream) {
    AVS_CHECK_ARG(acc && g && segs && ctl && actl && acc != g && n_segs >= 1 && n_segs <= ADT_MAX_SEGS && n_chunks >= 1,
                  "grad_accum: acc, g, segs, ctl, actl must not be NULL, acc != g, n_segs in 1..%d (got %d), n_chunks >= 1", ADT_MAX_SEGS, n_segs);
    AVS_CHECK_ARG(((size_t)acc & 15) == 0 && ((size_t)g & 15) == 0, "grad_accum: acc and g must be 16-byte aligned");
    const int grid = (int)(n_chunks < ADT_GRID ? n_chunks : ADT_GRID);
    grad_accum_kernel<<<grid, ADT_BLOCK, 0, stream>>>(acc, g, segs, n_segs, ctl, actl, first != 0);
    AVS_LAUNCH_CHECK("grad_accum");
    grad_accum_finish_kernel<<<1, 64, 0, stream>>>(ctl, actl, first != 0, publish != 0);
    AVS_LAUNCH_CHECK("grad_accum (bookkeeping)");
    return 0;
}
