#!/usr/bin/env python3
"""Decoded-size frames on one MI355X (one JSON file):

    python tools/bench_frames.py [--out profiles/r14/frames_bench.json] [--batches 8,64] [--no-step]
    python tools/bench_frames.py --parent DIR [--out ...]          # (c) alone: DIR holds a built checkout of the parent commit

kernel  (a) ops.resize_frames at 64 x 10 frames of 360 x 640 -> 224 x 224, plain and mixed, beside the same computation composed from torch
        operations on the same device (interpolate(x.float() / 255, mode='bicubic', antialias=True), normalise, mix: what a user of torch has
        today), interleaved in one process: ROUNDS rounds, in each round every variant timed over ITERS calls between device events after a
        warm-up; median and min - max over the rounds.  Bytes the algorithm must move: the uint8 frames once (442 MB; twice with a partner)
        and the fp32 output once (385 MB); GB/s = those bytes over the median time.  The composition's result is compared with the kernel's.
step    (b) the --wave-input --frame-size 360 640 training step of the launcher beside the --wave-input step (frames already 224 x 224) and
        beside their front ends alone, CAVMAEFT_BASE(527), interleaved, REPS repetitions of `--steps` steps each.
parent  (c) the plain mm fine-tuning step and bench.py on the parent commit against this one, fresh processes alternating (this process never
        opens the GPU); every result beside the parent's own spread.  Merged into the file --out names when it exists.
Nothing here is tuned to the result: shapes and repeat counts are fixed above the measurements."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, ITERS, REPS = 7, 10, 3
B, F, H, W, SIZE = 64, 10, 360, 640, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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


def torch_frames(v, mean, std, partner=None, weight=None, chunk=64):
    """the same frames composed from torch operations, fp32, `chunk` images at a time (the float copy of all 640 frames is 1.8 GB)"""
    import torch

    def one(x):
        out = torch.empty(x.shape[:-2] + (SIZE, SIZE), dtype=torch.float32, device=x.device)
        flat, oflat = x.reshape(-1, 3, x.shape[-2], x.shape[-1]), out.reshape(-1, 3, SIZE, SIZE)
        for i in range(0, flat.shape[0], chunk):
            r = torch.nn.functional.interpolate(flat[i:i + chunk].float() / 255, size=(SIZE, SIZE), mode="bicubic", align_corners=False, antialias=True)
            oflat[i:i + chunk] = (r - mean) / std
        return out
    a = one(v)
    if partner is None:
        return a
    w = weight.reshape(-1, 1, 1, 1, 1)
    return w * a + (1 - w) * one(partner)


def bench_kernel():
    import torch
    from avsiam_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    v = torch.randint(0, 256, (B, F, 3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    p = torch.randint(0, 256, (B, F, 3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    weight = torch.rand(B, device="cuda", generator=g)
    mean, std = (torch.tensor(x, device="cuda").reshape(3, 1, 1) for x in (MEAN, STD))
    out = torch.empty(B, F, 3, SIZE, SIZE, device="cuda")
    ways = {"kernel_plain": lambda: ops.resize_frames(v, size=SIZE, out=out),
            "kernel_mixed": lambda: ops.resize_frames(v, partner=p, weight=weight, size=SIZE, out=out),
            "torch_composition_plain": lambda: torch_frames(v, mean, std),
            "torch_composition_mixed": lambda: torch_frames(v, mean, std, p, weight)}
    nin, nout = float(v.numel()), 4.0 * out.numel()
    nbytes = {"kernel_plain": nin + nout, "kernel_mixed": 2 * nin + nout, "torch_composition_plain": nin + nout, "torch_composition_mixed": 2 * nin + nout}
    for fn in ways.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, fn in ways.items():
            t[k].append(time_calls(fn, ITERS if k.startswith("kernel") else 2))
    rows, lds = ops.resize_plan(H, W, SIZE, SIZE)
    res = {"shape": {"clips": B, "frames": F, "source": [H, W], "output": [SIZE, SIZE], "input_mb": nin / 1e6, "output_mb": nout / 1e6},
           "plan": {"rows_per_workgroup": rows, "lds_bytes_with_partner": lds}, "variants": {}}
    for k in ways:
        s = stat(t[k])
        res["variants"][k] = {"ms": s, "algorithm_bytes": nbytes[k], "gb_per_s_at_median": nbytes[k] / (s["median"] * 1e-3) / 1e9}
    a, b = ops.resize_frames(v[:4], size=SIZE), torch_frames(v[:4], mean, std)
    res["kernel_vs_torch_composition_max_gap"] = float((a - b).abs().max())
    for kind in ("plain", "mixed"):
        res[f"speedup_over_torch_composition_{kind}"] = (res["variants"][f"torch_composition_{kind}"]["ms"]["median"]
                                                         / res["variants"][f"kernel_{kind}"]["ms"]["median"])
    return res


def _model_and_kw(bs):
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import apply_freeze_base
    m = CAVMAEFT_BASE(527).cuda()
    apply_freeze_base(m, False)
    return m, dict(head_lr=100.0, mm_lr=100.0)


def bench_step(batches, steps, warmup):
    import torch
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    cfg, L = AVSiamConfig(), 527
    mean, std = -5.081, 4.4849
    fill = (0.0 - mean) / std
    res = {}
    for bs in batches:
        m, kw = _model_and_kw(bs)
        dev = m.arena.p.device
        wl = SyntheticWaveFtLoader(cfg, bs, 1, L, dev, mixup=0.5, norm=(mean, std))
        fl = SyntheticWaveFtLoader(cfg, bs, 1, L, dev, mixup=0.5, norm=(mean, std), frame_size=(H, W))

        def step_of(loader):
            def run():
                for a, v, y in loader:
                    m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", aug=m.draw_aug(bs, 48, 192, True, fill=fill), **kw)
            return run

        def front_of(loader):
            def run():
                for _ in loader:
                    pass
            return run
        ways = {"wave_input_mm_step": step_of(wl), "wave_input_frame_size_mm_step": step_of(fl), "front_end_only": front_of(wl),
                "front_end_only_frame_size": front_of(fl)}
        t = {k: [] for k in ways}
        for _ in range(REPS):
            for k, fn in ways.items():
                for _ in range(warmup):
                    fn()
                torch.cuda.synchronize()
                t[k].append(time_calls(fn, steps))
        res[f"batch_{bs}"] = {k: {"ms": [round(x, 4) for x in v], "median_ms": round(sorted(v)[len(v) // 2], 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}
                              for k, v in t.items()}
        del m
        torch.cuda.empty_cache()
    return {"recipe": {"mixup": 0.5, "freqm": 48, "timem": 192, "noise": True, "ftmode": "mm_grad", "branch": "mm", "n_class": L, "frame_size": [H, W],
                       "frames_per_clip": 1},
            "steps": steps, "warmup": warmup, "repetitions": REPS, "results": res,
            "note": "both steps include the host draws and their upload; front_end_only* is the loader without the model"}


def plain_step(bs, steps, warmup):
    """the plain mm step on ready-made tensors (no front end), this process's package: one figure"""
    import torch
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader
    m, kw = _model_and_kw(bs)
    ld = SyntheticFtLoader(AVSiamConfig(), bs, 1, 527, m.arena.p.device)
    fn = lambda: m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return time_calls(fn, steps)


def against_parent(parent, steps, warmup, reps=3):
    """fresh processes, parent and this tree alternating; this process never opens the GPU"""
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    out = {"plain_mm_step_batch_64_ms": {k: [] for k in trees}, "bench_py": {k: [] for k in trees}}
    me = os.path.abspath(__file__)
    for _ in range(reps):
        for name, tree in trees.items():
            r = subprocess.run([sys.executable, me, "--plain-only", "--tree", tree, "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                               capture_output=True, text=True, timeout=600, check=True)
            out["plain_mm_step_batch_64_ms"][name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        for name, tree in trees.items():
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree, capture_output=True,
                               text=True, timeout=900, check=True)
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            out["bench_py"][name].append({k: line[k] for k in ("value", "unit", "metric", "ms_per_step") if k in line})
    for key, pick in (("plain_mm_step_batch_64_ms", lambda x: x), ("bench_py", lambda x: x.get("ms_per_step", x.get("value")))):
        vals = {k: [pick(x) for x in v] for k, v in out[key].items()}
        out[key + "_summary"] = {k: {"median": sorted(v)[len(v) // 2], "min_max": [min(v), max(v)]} for k, v in vals.items()}
        lo, hi = out[key + "_summary"]["parent"]["min_max"]
        out[key + "_summary"]["this_median_within_parents_spread"] = bool(lo <= out[key + "_summary"]["this"]["median"] <= hi)
    out["bench_py_args"] = f"--gpus 1 --steps {steps} --warmup {warmup}"
    # one deterministic plain fine-tuning step in both trees: loss, arena hashes and the hash of the list of library calls
    digest = {}
    for name, tree in trees.items():
        r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=tree, capture_output=True, text=True,
                           timeout=600, check=True)
        line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
        digest[name] = {k: line[k] for k in ("losses", "calls_per_step", "p", "g", "adam_m", "adam_v", "trace_calls", "trace")}
    out["step_digest_ft_trace_batch_3"] = {**digest, "equal": digest["parent"] == digest["this"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r14", "frames_bench.json"))
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", dest="no_step", action="store_true")
    ap.add_argument("--reps", type=int, default=3, help="with --parent: alternations")
    ap.add_argument("--parent", metavar="DIR", help="(c) alone: a built checkout of the parent commit")
    ap.add_argument("--plain-only", dest="plain_only", action="store_true", help="print the plain mm step's time of the package under --tree")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.plain_only:
        print(json.dumps({"ms": plain_step(64, args.steps, args.warmup)}))
        return
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    if args.parent:
        res["against_parent"] = against_parent(args.parent, args.steps, args.warmup, args.reps)
        print(json.dumps(res["against_parent"]), flush=True)
    else:
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        res["device"] = torch.cuda.get_device_name(0)
        res["kernel"] = bench_kernel()
        print(json.dumps(res["kernel"]), flush=True)
        if not args.no_step:
            res["step"] = bench_step([int(b) for b in args.batches.split(",")], args.steps, args.warmup)
            print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
