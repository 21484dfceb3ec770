"""Fine-tuning throughput of CAVMAEFT_BASE's fused train_step (one JSON line).

    python tools/bench_ft_train.py [--steps 10] [--warmup 3] [--batches 8,64]

The AudioSet recipe (mm_grad, BCE, 527 classes, T = 1, lr 1e-4, head_lr = mm_lr = 100; egs/audioset/run_base_ft.sh): per branch (mm: loss on
out, a: out_a, v: out_v), the reference's 50 / 25 / 25 mix (traintest_ft_base.py:153-160), and freeze_base at the largest batch.  Every
number is ms per step (CUDA events over `steps` steps after `warmup`) and samples/s.  kernel_share: one extra profiled mix step per batch
with every launch timed by HIP events (ops.KernelProfiler): the share of the step in the kernels fine-tuning added (cls_loss,
segment_mean_bwd_acc) and in layernorm_bwd (all widths; the head-width calls are a handful of them).
"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=str, default="8,64")
    args = ap.parse_args(argv)
    from avsiam_amd import ops
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base, draw_branch
    cfg, L = AVSiamConfig(), 527
    res = {"metric": "ft_train", "model": "CAVMAEFT_BASE", "ftmode": "mm_grad", "loss": "BCE", "n_class": L, "frames": 1,
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "results": {}}
    batches = [int(b) for b in args.batches.split(",")]
    for B in batches:
        m = CAVMAEFT_BASE(L).cuda()
        apply_freeze_base(m, False)
        ld = SyntheticFtLoader(cfg, B, 1, L, m.arena.p.device)
        a, v, y = ld.a, ld.v, ld.y
        r = {}
        for br in ("mm", "a", "v"):
            ms = _time(lambda i, br=br: m.train_step(a, v, y, 1e-4, "mm_grad", branch=br, head_lr=100.0, mm_lr=100.0), args.steps, args.warmup)
            r[br] = {"ms_per_step": round(ms, 3), "samples_per_s": round(B * 1e3 / ms, 2)}
        rng = random.Random(0)
        mix = [draw_branch(rng.uniform(0, 1)) for _ in range(args.steps + args.warmup)]
        ms = _time(lambda i: m.train_step(a, v, y, 1e-4, "mm_grad", branch=mix[i], head_lr=100.0, mm_lr=100.0), args.steps, args.warmup)
        r["mix_50_25_25"] = {"ms_per_step": round(ms, 3), "samples_per_s": round(B * 1e3 / ms, 2)}
        if B == max(batches):
            apply_freeze_base(m, True)
            ms = _time(lambda i: m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", head_lr=100.0, mm_lr=100.0), args.steps, args.warmup)
            r["freeze_base_mm"] = {"ms_per_step": round(ms, 3), "samples_per_s": round(B * 1e3 / ms, 2)}
            apply_freeze_base(m, False)
        ops.prof = ops.KernelProfiler()
        for br in ("mm", "a", "v"):
            m.train_step(a, v, y, 1e-4, "mm_grad", branch=br, head_lr=100.0, mm_lr=100.0)
        torch.cuda.synchronize()
        s = ops.prof.summary()
        ops.prof = None
        tot = sum(k["total_ms"] for k in s.values())
        new = sum(s[k]["total_ms"] for k in ("cls_loss", "segment_mean_bwd_acc") if k in s)
        r["kernel_share"] = {"new_kernels": round(new / tot, 5) if tot else None,
                             "layernorm_bwd_all_widths": round(s.get("layernorm_bwd", {}).get("total_ms", 0.0) / tot, 5) if tot else None}
        res["results"][f"batch_{B}"] = r
        del m
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
