#!/usr/bin/env python3
"""Fine-tuning metrics on one MI355X: the device path (ops.classification_stats / traintest_ft_base.calculate_stats_device) beside the host
path it can replace - the [N, C] device-to-host copy plus numpy calculate_stats - on the same box, at evaluation-set shapes:

    audioset      20 000 x 527, multi-hot, about 0.5 % positives per class on average with class priors spread log-uniformly over 1e-4 .. 3e-2
    onehot        15 000 x 309, one label per sample
    audioset_x11  the first shape with 11 prediction sets against one target (ten frames and their mean: evaluate_frames)

    python tools/bench_ft_metrics.py [--out profiles/r09/ft_metrics_bench.json] [--full-parent]

Scores are fp32 sigmoids of Gaussian logits shifted on the positives.  Per shape: the kernel call between HIP events (median of rounds of
repeated calls after a warm-up), the whole calculate_stats_device call on the host clock (it ends in the copy of the results, which
synchronises), and the host path on the host clock with 16 threads.  The host path of the 11-set shape is one calculate_stats call per set;
unless --full-parent is given one set is timed and multiplied by 11, and the result says so.  Nothing here is tuned to the result: the
shapes and the repeat counts are fixed above the measurements."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avsiam_amd import ops  # noqa: E402
from avsiam_amd.traintest_ft_base import calculate_stats, calculate_stats_device  # noqa: E402

ROUNDS, ITERS = 5, 10


def med(v):
    return sorted(v)[len(v) // 2]


def make(N, C, S, onehot, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if onehot:
        target = torch.zeros(N, C, device="cuda")
        target[torch.arange(N, device="cuda"), torch.randint(0, C, (N,), device="cuda", generator=g)] = 1.0
    else:
        prior = torch.exp(torch.rand(C, device="cuda", generator=g) * (np.log(3e-2) - np.log(1e-4)) + np.log(1e-4))
        target = (torch.rand(N, C, device="cuda", generator=g) < prior).float()
    logits = 2.0 * torch.randn(S, N, C, device="cuda", generator=g) + 2.0 * target - 3.0
    return torch.sigmoid(logits), target


def bench(name, N, C, S, onehot, full_parent):
    scores, target = make(N, C, S, onehot, 0)
    P = target.sum(0)
    row = {"name": name, "N": N, "C": C, "S": S, "positives_per_class": {"min": int(P.min()), "median": int(P.median()), "max": int(P.max()), "total": int(P.sum())},
           "pair_comparisons_per_set": float(N * P.sum()), "workspace_mib": ops.classification_stats_ws_bytes(S, N, C) / 2 ** 20}
    call = (lambda: ops.classification_stats(scores, target)) if S > 1 else (lambda: ops.classification_stats(scores[0], target))
    call(); torch.cuda.synchronize()
    t = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            call()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / ITERS)
    row["kernel_ms"] = {"median": med(t), "spread": [min(t), max(t)], "rounds": ROUNDS, "calls_per_round": ITERS}

    dev_in = scores if S > 1 else scores[0]
    t = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = calculate_stats_device(dev_in, target)
        t.append((time.perf_counter() - t0) * 1e3)
    row["calculate_stats_device_ms"] = {"median": med(t), "spread": [min(t), max(t)], "rounds": ROUNDS}

    torch.set_num_threads(16)
    nsets = S if full_parent else 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [calculate_stats(scores[s].cpu().numpy(), target.cpu().numpy()) for s in range(nsets)]
    elapsed = (time.perf_counter() - t0) * 1e3
    row["host_path_ms"] = elapsed * S / nsets
    row["host_path_note"] = f"device-to-host copy + numpy calculate_stats, 16 threads, {nsets} of {S} set(s) run" + ("" if nsets == S else f", times {S}")
    row["speedup_whole_call"] = row["host_path_ms"] / row["calculate_stats_device_ms"]["median"]
    # the two paths against each other: auc is one definition; AP differs only where scores tie (the device path groups them, as sklearn)
    dev0 = stats[0] if S > 1 else stats
    row["max_auc_gap_vs_host"] = float(np.nanmax(np.abs(np.array([s["auc"] for s in dev0]) - np.array([s["auc"] for s in host[0]]))))
    row["max_ap_gap_vs_host"] = float(np.nanmax(np.abs(np.array([s["AP"] for s in dev0]) - np.array([s["AP"] for s in host[0]]))))
    sc0 = scores[0]
    row["tied_score_entries_set0"] = int(sum(N - len(torch.unique(sc0[:, k])) for k in range(0, C, max(1, C // 16))))
    row["tied_score_note"] = "entries sharing a value with another of their class, over 16 sampled classes"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "ft_metrics_bench.json"))
    ap.add_argument("--full-parent", action="store_true", help="run the host path on all 11 sets of the last shape (minutes)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "tile": ops.CLS_STATS_TILE, "positives_per_workgroup": ops.CLS_STATS_PPW, "shapes": []}
    for name, N, C, S, onehot in (("audioset", 20000, 527, 1, False), ("onehot", 15000, 309, 1, True), ("audioset_x11", 20000, 527, 11, False)):
        row = bench(name, N, C, S, onehot, args.full_parent)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
