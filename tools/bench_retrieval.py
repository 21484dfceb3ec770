#!/usr/bin/env python3
"""Retrieval evaluation on one MI355X: (a) the streaming similarity -> rank kernel alone at retrieval-set and gallery sizes, beside what a
user would write today on the same box (fp32 torch.matmul with TF32 off + compare + row sum, where N x N fits); (b) feature extraction,
the single-frame path against the existing forward(..., "retrieval") that encodes all ten frames.

    python tools/bench_retrieval.py [--out profiles/r08/retrieval_bench.json] [--sizes 1545,2635,16384,65536] [--skip-extract]

HIP events around repeated launches after a warm-up; every figure is a median of rounds in which the variants alternate.  TFLOP/s counts the
2 N^2 D of the similarity only (the algorithm's work), against the 157.3 TFLOP/s fp32 matrix peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avsiam_amd import ops  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def med(v):
    return sorted(v)[len(v) // 2]


def peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def torch_baseline(q, g):
    s = q @ g.T
    return (s > s.diagonal()[:, None]).sum(1)


def bench_kernel(N, D, rounds=5):
    gen = torch.Generator(device="cuda").manual_seed(0)
    a = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=gen), dim=-1)
    v = torch.nn.functional.normalize(a + 0.3 * torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=gen), dim=-1), dim=-1)
    flop = 2.0 * N * N * D
    iters = max(2, min(50, int(0.25 / (flop / 60e12))))                  # ~ a quarter second per timed window at a guessed 60 TFLOP/s
    variants = {"kernel_topk0": lambda: ops.retrieval_rank(a, v), "kernel_topk16": lambda: ops.retrieval_rank(a, v, topk=16)}
    if N * N * 4 <= 2 << 30:
        variants["torch_matmul_compare"] = lambda: torch_baseline(a, v)
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timeit(fn, iters))
    row = {"N": N, "D": D, "iters": iters, "rounds": rounds}
    for k in variants:
        s = med(t[k])
        row[k] = {"ms": s * 1e3, "tflops": flop / s / 1e12, "fraction_of_f32_matrix_peak": flop / s / PEAK_F32_MATRIX,
                  "spread_ms": [min(t[k]) * 1e3, max(t[k]) * 1e3], "peak_memory_growth_mib": peak_growth(variants[k]) / 2 ** 20}
    if "torch_matmul_compare" in variants:
        row["ranks_equal_torch"] = bool(torch.equal(ops.retrieval_rank(a, v)["rank"].long(), torch_baseline(a, v)))
    else:
        row["torch_matmul_compare"] = f"not run: the {N} x {N} fp32 matrix alone is {N * N * 4 / 2 ** 30:.1f} GiB"
    row["epilogue_share_topk16_vs_topk0"] = row["kernel_topk16"]["ms"] / row["kernel_topk0"]["ms"] - 1.0
    return row


def bench_extract(B=100, T=10, rounds=3, iters=3):
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    cfg = AVSiamConfig()
    m = CAVMAEFT_BASE(527).cuda()
    a = torch.randn(B, cfg.audio_len, cfg.n_mels, device="cuda")
    v = torch.randn(B, T, 3, cfg.img_size, cfg.img_size, device="cuda")
    fa, fv = torch.empty(B, cfg.embed_dim, device="cuda"), torch.empty(B, cfg.embed_dim, device="cuda")

    def full():
        ta, tv = m(a, v, "retrieval")
        return torch.nn.functional.normalize(ta.mean(1), dim=-1), torch.nn.functional.normalize(tv.mean(1), dim=-1)

    variants = {"single_frame_retrieval_features": lambda: m.retrieval_features(a, v, out_a=fa, out_v=fv), "ten_frame_forward_retrieval": full}
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timeit(fn, iters))
    out = {"batch": B, "frames": T}
    for k in variants:
        out[k] = {"ms_per_batch": med(t[k]) * 1e3, "clips_per_s": B / med(t[k]), "spread_ms": [min(t[k]) * 1e3, max(t[k]) * 1e3]}
    out["speedup"] = out["single_frame_retrieval_features"]["clips_per_s"] / out["ten_frame_forward_retrieval"]["clips_per_s"]
    out["encoder_rows_ratio_expected"] = (cfg.audio_tokens + T * cfg.video_tokens) / (cfg.audio_tokens + cfg.video_tokens)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "retrieval_bench.json"))
    ap.add_argument("--sizes", default="1545,2635,16384,65536")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--skip-extract", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    torch.backends.cuda.matmul.allow_tf32 = False
    res = {"device": torch.cuda.get_device_name(0), "f32_matrix_peak_tflops": PEAK_F32_MATRIX / 1e12, "kernel": []}
    for N in (int(s) for s in args.sizes.split(",")):
        row = bench_kernel(N, args.dim)
        res["kernel"].append(row)
        print(json.dumps(row), flush=True)
    if not args.skip_extract:
        res["extraction"] = bench_extract()
        print(json.dumps(res["extraction"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
