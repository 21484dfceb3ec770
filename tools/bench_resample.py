#!/usr/bin/env python3
"""Source-rate audio on one MI355X (one JSON file):

    python tools/bench_resample.py [--out profiles/r17/resample_bench.json] [--batches 8,64] [--no-step]
    python tools/bench_resample.py --parent DIR [--out ...]        # (c) alone: DIR holds a built checkout of the parent commit

kernel  (a) ops.resample_wave on 64 clips of 10 s at 44.1 kHz stereo -> [64, 160 000] (and, as a second line, 48 kHz mono), beside the same
        computation composed from torch operations on the same device (pad, conv1d with the dense table at stride o, transpose, reshape, cut,
        mean over the channels: what torchaudio's resample and the loader's mean do), interleaved in one process: ROUNDS rounds, in each round
        every variant timed over ITERS calls between device events after a warm-up; median and min - max over the rounds.  Bytes the
        algorithm must move: the fp32 input once (226 MB) and the fp32 output once (41 MB); GB/s = those bytes over the median time, also as a
        fraction of the 6.29 TB/s float4-copy rate measured on this device (README).  The composition's result is compared with the kernel's.
step    (b) the --wave-input --sample-rate 44100 --audio-channels 2 training step of the launcher beside the --wave-input step and beside their
        front ends alone, CAVMAEFT_BASE(527), interleaved, REPS repetitions of `--steps` steps each.
parent  (c) the plain mm fine-tuning step and bench.py on the parent commit against this one, fresh processes alternating (this process never
        opens the GPU), the order of the two swapped from one alternation to the next; every result beside the parent's own spread.  Merged
        into --out.
Nothing here is tuned to the result: shapes and repeat counts are fixed above the measurements."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, ITERS, REPS = 7, 10, 3
B, SECONDS, NEW = 64, 10, 16000
COPY_RATE = 6.29e12                                           # float4 copy on one MI355X, bytes / s (README)
LINES = {"44100_stereo": (44100, 2), "48000_mono": (48000, 1)}


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


def torch_resample(x, table, width, o, n, m):
    """x [B, C, S] -> [B, m]: the dense-table convolution torchaudio runs, then the channel mean"""
    import torch
    Bx, C, S = x.shape
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x.reshape(Bx * C, 1, S), (width, width + o)), table, stride=o)
    y = y.transpose(1, 2).reshape(Bx, C, -1)[..., :m]
    return y.mean(dim=1)


def bench_kernel():
    import torch
    from avsiam_amd import ops, preprocess
    res = {"lines": {}}
    for name, (rate, C) in LINES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        S = rate * SECONDS
        x = torch.randn(B, C, S, device="cuda", generator=g) * 0.1
        table, width = preprocess.resample_table_reference(rate, NEW)
        table = table.cuda()
        o, n = preprocess._resample_ratio(rate, NEW)
        m = preprocess.resample_out_length(S, rate, NEW)
        out = torch.empty(B, m, device="cuda")
        ways = {"kernel": lambda: ops.resample_wave(x, rate, out=out), "torch_composition": lambda: torch_resample(x, table, width, o, n, m)}
        nbytes = 4.0 * (x.numel() + out.numel())
        print(f"{name}: warm-up", flush=True)
        for k in list(ways):
            try:
                for _ in range(2):
                    ways[k]()
                torch.cuda.synchronize()
            except RuntimeError as e:                         # (the library behind conv1d may have no solver for a stride of o)
                if k == "kernel":
                    raise
                res.setdefault("errors", {})[f"{name}.{k}"] = str(e)[:300]
                del ways[k]
        t = {k: [] for k in ways}
        for _ in range(ROUNDS):
            for k, fn in ways.items():
                t[k].append(time_calls(fn, ITERS if k == "kernel" else 2))
        _, geo = ops.resample_table(rate, NEW, x.device)
        line = {"shape": {"clips": B, "channels": C, "rate": rate, "samples": S, "outputs": m, "input_mb": 4.0 * x.numel() / 1e6, "output_mb": 4.0 * out.numel() / 1e6},
                "table": {"o": geo[0], "n": geo[1], "width": geo[2], "taps": geo[3], "compact_words": geo[1] * ((geo[3] | 1) + 1)}, "variants": {}}
        for k in ways:
            s = stat(t[k])
            rate_bs = nbytes / (s["median"] * 1e-3)
            line["variants"][k] = {"ms": s, "algorithm_bytes": nbytes, "gb_per_s_at_median": rate_bs / 1e9, "fraction_of_float4_copy_rate": rate_bs / COPY_RATE}
        if "torch_composition" in ways:
            a, b = ops.resample_wave(x[:4].contiguous(), rate)[0], torch_resample(x[:4], table, width, o, n, m)
            line["kernel_vs_torch_composition_max_gap"] = float((a - b).abs().max())
            line["speedup_over_torch_composition"] = line["variants"]["torch_composition"]["ms"]["median"] / line["variants"]["kernel"]["ms"]["median"]
        # tap products per second: the kernel's inner loop is two LDS reads and one multiply-add per tap, channel and output
        line["kernel_tap_products_per_s"] = float(B) * m * C * geo[3] / (line["variants"]["kernel"]["ms"]["median"] * 1e-3)
        res["lines"][name] = line
        del x, out, table
        torch.cuda.empty_cache()
    return res


def bench_step(batches, steps, warmup):
    import torch
    from bench_frames import _model_and_kw
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
        sl = SyntheticWaveFtLoader(cfg, bs, 1, L, dev, mixup=0.5, norm=(mean, std), sample_rate=44100, channels=2)

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
        ways = {"wave_input_mm_step": step_of(wl), "wave_input_sample_rate_mm_step": step_of(sl), "front_end_only": front_of(wl),
                "front_end_only_sample_rate": front_of(sl)}
        t = {k: [] for k in ways}
        for _ in range(REPS):
            for k, fn in ways.items():
                for _ in range(warmup):
                    fn()
                torch.cuda.synchronize()
                t[k].append(time_calls(fn, steps))
        res[f"batch_{bs}"] = {k: {"ms": [round(x, 4) for x in v], "median_ms": round(sorted(v)[len(v) // 2], 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}
                              for k, v in t.items()}
        del m, wl, sl
        torch.cuda.empty_cache()
    return {"recipe": {"mixup": 0.5, "freqm": 48, "timem": 192, "noise": True, "ftmode": "mm_grad", "branch": "mm", "n_class": L, "sample_rate": 44100,
                       "audio_channels": 2}, "steps": steps, "warmup": warmup, "repetitions": REPS, "results": res,
            "note": "both steps include the host draws and their upload; with mixup the sample-rate step resamples clips and partners (two launches); "
                    "front_end_only* is the loader without the model"}


def against_parent(parent, steps, warmup, reps):
    """tools/bench_frames.py's procedure (fresh processes, this process never opens the GPU) with the order of the two trees swapped from one
    alternation to the next, so that neither tree always runs on the warmer device"""
    import subprocess
    import bench_frames
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    out = {"plain_mm_step_batch_64_ms": {k: [] for k in trees}, "bench_py": {k: [] for k in trees}, "order": []}
    for rep in range(reps):
        order = list(trees) if rep % 2 == 0 else list(trees)[::-1]
        out["order"].append(order)
        for name in order:
            r = subprocess.run([sys.executable, os.path.abspath(bench_frames.__file__), "--plain-only", "--tree", trees[name], "--steps", str(steps), "--warmup",
                                str(warmup)], cwd=trees[name], capture_output=True, text=True, timeout=600, check=True)
            out["plain_mm_step_batch_64_ms"][name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        for name in order:
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=trees[name], capture_output=True,
                               text=True, timeout=900, check=True)
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            out["bench_py"][name].append({k: line[k] for k in ("value", "unit", "metric", "ms_per_step") if k in line})
    for key, pick in (("plain_mm_step_batch_64_ms", lambda x: x), ("bench_py", lambda x: x.get("ms_per_step", x.get("value")))):
        vals = {k: [pick(x) for x in v] for k, v in out[key].items()}
        out[key + "_summary"] = {k: {"median": sorted(v)[len(v) // 2], "min_max": [min(v), max(v)]} for k, v in vals.items()}
        lo, hi = out[key + "_summary"]["parent"]["min_max"]
        out[key + "_summary"]["this_median_within_parents_spread"] = bool(lo <= out[key + "_summary"]["this"]["median"] <= hi)
    out["bench_py_args"] = f"--gpus 1 --steps {steps} --warmup {warmup}"
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
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "resample_bench.json"))
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", dest="no_step", action="store_true")
    ap.add_argument("--reps", type=int, default=4, help="with --parent: alternations (an even number: each tree runs first equally often)")
    ap.add_argument("--parent", metavar="DIR", help="(c) alone: a built checkout of the parent commit")
    args = ap.parse_args()
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
