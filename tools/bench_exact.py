#!/usr/bin/env python3
"""The exact-fp32 mode on one MI355X (one JSON file; nothing here is a pass mark):

    python tools/bench_exact.py [--out profiles/r18/exact_bench.json]
    python tools/bench_exact.py --parent DIR [--out ...]          # DIR holds a built checkout of the parent commit; merged into --out

gemm    ops.gemm_nt_f32 at the audioonly batch-64 shapes (M = 32 768; (N, K) = (2304, 768), (768, 768), (3072, 768), (768, 3072); bias) beside
        torch.matmul in fp32 on the same device, interleaved: ROUNDS rounds, in each every variant timed over ITERS calls between device events
        after a warm-up; median and min - max over the rounds; TFLOP/s and the share of the 157.3 TFLOP/s f32 matrix peak.
attn    ops.attn_fwd_f32 at 64 x 512 and 640 x 196 tokens (12 heads of 64), the same way.
model   CAVMAEFT_BASE(527): audioonly and mm_grad(is_eval=True, 10 frames) at batch 16, exact=True beside the bf16 call, interleaved, in ms.
parent  the plain mm fine-tuning step and bench.py on the parent commit against this tree, fresh processes alternating, and the step digest
        (tools/bench_resample.py: against_parent)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, ITERS, MODEL_ROUNDS, MODEL_ITERS = 7, 5, 5, 3
F32_PEAK = 157.3e12
M_GEMM = 32768
GEMM_NK = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
ATTN = {"64x512": [512] * 64, "640x196": [196] * 640}


def stat(v):
    return {"median": sorted(v)[len(v) // 2], "min_max": [min(v), max(v)], "rounds": len(v)}


def time_calls(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(variants, rounds, iters):
    """{name: fn} -> {name: stat of ms per call}; every round times every variant, after one warm-up call of each"""
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(time_calls(fn, iters))
    return {k: stat(v) for k, v in ms.items()}


def bench_gemm():
    import torch
    from avsiam_amd import ops
    out = {}
    g = torch.Generator().manual_seed(0)
    for N, K in GEMM_NK:
        A = torch.randn(M_GEMM, K, generator=g).cuda()
        B = (torch.randn(N, K, generator=g) * 0.05).cuda()
        bias = torch.randn(N, generator=g).cuda()
        C, Ct = torch.empty(M_GEMM, N, device="cuda"), torch.empty(M_GEMM, N, device="cuda")
        r = interleaved({"gemm_nt_f32": lambda: ops.gemm_nt_f32(A, B, C, M_GEMM, bias=bias),
                         "torch_fp32": lambda: torch.addmm(bias, A, B.t(), out=Ct)}, ROUNDS, ITERS)
        flop = 2.0 * M_GEMM * N * K
        for v in r.values():
            v["tflops"] = flop / (v["median"] * 1e-3) / 1e12
            v["share_of_f32_matrix_peak"] = v["tflops"] * 1e12 / F32_PEAK
        r["kernel_over_torch_rate"] = r["gemm_nt_f32"]["tflops"] / r["torch_fp32"]["tflops"]
        r["max_abs_difference"] = float((C - Ct).abs().max())
        out[f"M{M_GEMM}_N{N}_K{K}"] = r
        del A, B, C, Ct
    return out


def bench_attn():
    import torch
    from avsiam_amd import ops
    out = {}
    H, D = 12, 768
    g = torch.Generator().manual_seed(1)
    for name, lens in ATTN.items():
        rows = sum(lens)
        qkv = torch.randn(rows, 3 * D, generator=g).cuda()
        o = torch.empty(rows, D, device="cuda")
        tiles = ops.AttnTiles(lens, "cuda", tile_rows=128)
        r = interleaved({"attn_fwd_f32": lambda: ops.attn_fwd_f32(qkv, tiles, H, o)}, ROUNDS, ITERS)["attn_fwd_f32"]
        r["tflops"] = 4.0 * tiles.sum_sq * D / (r["median"] * 1e-3) / 1e12
        r["share_of_f32_matrix_peak"] = r["tflops"] * 1e12 / F32_PEAK
        out[name] = r
    return out


def bench_model(batch=16):
    import torch
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    cfg = AVSiamConfig()
    m = CAVMAEFT_BASE(527, init_seed=4321, init_mode="random").cuda()
    g = torch.Generator().manual_seed(2)
    a = torch.randn(batch, cfg.audio_len, cfg.n_mels, generator=g).cuda()
    v = torch.randn(batch, 10, 3, cfg.img_size, cfg.img_size, generator=g).cuda()
    out = {"batch": batch}
    with torch.no_grad():
        for name, call in (("audioonly", lambda **kw: m(a, None, "audioonly", **kw)), ("mm_grad_is_eval", lambda **kw: m(a, v, "mm_grad", is_eval=True, **kw))):
            r = interleaved({"exact_ms": lambda: call(exact=True), "bf16_ms": lambda: call()}, MODEL_ROUNDS, MODEL_ITERS)
            r["exact_over_bf16"] = r["exact_ms"]["median"] / r["bf16_ms"]["median"]
            r["max_abs_logit_difference"] = float((call(exact=True) - call()).abs().max())
            out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "exact_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="with --parent: alternations (an even number: each tree runs first equally often)")
    ap.add_argument("--parent", metavar="DIR", help="a built checkout of the parent commit: only the comparison with it is run")
    args = ap.parse_args()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    if args.parent:
        from bench_resample import against_parent
        res["against_parent"] = against_parent(args.parent, args.steps, args.warmup, args.reps)
        print(json.dumps(res["against_parent"]), flush=True)
    else:
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        res["device"] = torch.cuda.get_device_name(0)
        for key, fn in (("gemm", bench_gemm), ("attn", bench_attn), ("model", bench_model)):
            res[key] = fn()
            print(json.dumps({key: res[key]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
