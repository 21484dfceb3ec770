// The segment-table Adam update (include/avsiam_hip.h, avs_adam_table): the device mirrors of avs_adam_seg / avs_adam_ctl, the launch
// geometry, and the update itself as ONE piece of code that elementwise.hip (avs_adam_table) and grad_guard.hip (avs_adam_table_guarded)
// both instantiate - what the guarded kernel adds is what it does BEFORE calling in (read the guard block, leave on skip, fold coef into
// the gradient scale), so the two kernels cannot drift apart in their arithmetic.
#pragma once
#include "common.h"

// Work is cut into chunks of ADT_CHUNK elements:
// every workgroup builds the exclusive prefix sum of the segments' chunk counts in LDS (the table is a few KB, read from the L2), then walks
// the chunks blockIdx.x, + gridDim.x, ... and finds each chunk's segment by binary search.  A chunk of a class that is not live is skipped before
// any of its memory is touched; malformed segments (n <= 0, misaligned or negative lo, group / class out of range) own no chunks.
struct AdamSeg { long long lo; int n; int group; int cls; };
struct AdamCtl { float lr[3]; int step[16]; float live[16]; };
static_assert(sizeof(AdamSeg) == 24 && sizeof(AdamCtl) == 140, "mirrors of avs_adam_seg / avs_adam_ctl (include/avsiam_hip.h)");
constexpr int ADT_BLOCK = 256, ADT_CHUNK = 4096, ADT_GRID = 2048, ADT_MAX_SEGS = 4096, ADT_NCLS = 16, ADT_NGROUP = 3;

__device__ __forceinline__ int adt_chunks(const AdamSeg& s) {
    const bool ok = s.n > 0 && (s.n & 3) == 0 && s.lo >= 0 && (s.lo & 3) == 0 && s.group >= 0 && s.group < ADT_NGROUP && s.cls >= 0 && s.cls < ADT_NCLS;
    return ok ? (s.n - 1) / ADT_CHUNK + 1 : 0;
}

// pre[0 .. n_segs] <- exclusive prefix sum of the segments' chunk counts (pre[n_segs] = the table's chunks); part: ADT_BLOCK ints of scratch LDS.
// Called by all ADT_BLOCK threads of a workgroup; ends with a barrier.
__device__ __forceinline__ void adt_prefix(const AdamSeg* __restrict__ segs, int n_segs, int* pre, int* part) {
    const int tid = threadIdx.x;
    const int per = (n_segs + ADT_BLOCK - 1) / ADT_BLOCK;
    const int s0 = min(tid * per, n_segs), s1 = min(s0 + per, n_segs);
    int sum = 0;
    for (int s = s0; s < s1; ++s) sum += adt_chunks(segs[s]);
    part[tid] = sum;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < tid; ++k) base += part[k];
    for (int s = s0; s < s1; ++s) {
        pre[s] = base;
        base += adt_chunks(segs[s]);
    }
    if (tid == ADT_BLOCK - 1) pre[n_segs] = base;         // (its own slice ends the table, or is empty: base is the total)
    __syncthreads();
}

// largest s with pre[s] <= c: pre[s] <= c < pre[s + 1], a segment that owns chunks
__device__ __forceinline__ int adt_find(const int* pre, int n_segs, int c) {
    int lo = 0, hi = n_segs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// The whole of a workgroup's share of the update.  gscale: what the gradient is multiplied by (grad_scale, or grad_scale * coef).
__device__ __forceinline__ void adam_table_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                bf16_t* __restrict__ pb, const AdamSeg* __restrict__ segs, int n_segs,
                                                const AdamCtl* __restrict__ ctl, float b1, float b2, float eps, float wd, float gscale) {
    // The update's roundings are written out - which product of `g * gscale + wd * p`, `b1 * m + (1 - b1) * gg`, `b2 * v + (1 - b2) * gg * gg` is
    // fused into the add - and contraction is off for the rest: left to the compiler, two kernels that inline this body may fuse different
    // products and leave different last bits.  The form is the one adam_kernel (elementwise.hip) compiles to, so a segment gets avs_adam's bytes.
#pragma clang fp contract(off)
    __shared__ int pre[ADT_MAX_SEGS + 1];
    __shared__ int part[ADT_BLOCK];
    __shared__ float s_bc1[ADT_NCLS], s_bc2[ADT_NCLS], s_lr[ADT_NGROUP];
    __shared__ int s_live[ADT_NCLS];
    const int tid = threadIdx.x;
    if (tid < ADT_NCLS) {
        const bool live = ctl->live[tid] > 0.f;
        s_live[tid] = live;
        if (live) {
            const double t = (double)(ctl->step[tid] + 1);
            s_bc1[tid] = (float)(1.0 - pow((double)b1, t));
            s_bc2[tid] = (float)sqrt(1.0 - pow((double)b2, t));
        }
    }
    if (tid < ADT_NGROUP) s_lr[tid] = ctl->lr[tid];
    adt_prefix(segs, n_segs, pre, part);
    const int total = pre[n_segs];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const int lo = adt_find(pre, n_segs, c);
        const AdamSeg sg = segs[lo];
        if (!s_live[sg.cls]) continue;
        const int first = (c - pre[lo]) * ADT_CHUNK;       // < sg.n
        const size_t off = (size_t)sg.lo + (size_t)first;
        const int n4 = min(ADT_CHUNK, sg.n - first) / 4;
        const float lr = s_lr[sg.group], bc1 = s_bc1[sg.cls], bc2_sqrt = s_bc2[sg.cls];
        const float step = lr / bc1;
        float4* p4 = reinterpret_cast<float4*>(p + off);
        const float4* g4 = reinterpret_cast<const float4*>(g + off);
        float4* m4 = reinterpret_cast<float4*>(m + off);
        float4* v4 = reinterpret_cast<float4*>(v + off);
        uint2* pb2 = pb ? reinterpret_cast<uint2*>(pb + off) : nullptr;
        for (int i = tid; i < n4; i += ADT_BLOCK) {
            float4 pv = p4[i];
            const float4 gv = g4[i];
            float4 mv = m4[i];
            float4 vv = v4[i];
            float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gg = fmaf(gp[k], gscale, wd * pp[k]);
                mp[k] = fmaf(b1, mp[k], (1.f - b1) * gg);
                vp[k] = fmaf(b2, vp[k], ((1.f - b2) * gg) * gg);
                pp[k] -= (step * mp[k]) / (sqrtf(vp[k]) / bc2_sqrt + eps);
            }
            p4[i] = pv;
            m4[i] = mv;
            v4[i] = vv;
            if (pb2) {
                uint2 o;
                o.x = pack_bf2(pv.x, pv.y);
                o.y = pack_bf2(pv.z, pv.w);
                pb2[i] = o;
            }
        }
    }
}
