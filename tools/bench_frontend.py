#!/usr/bin/env python3
"""The waveform front end on one MI355X (one JSON file):

    python tools/bench_frontend.py [--out profiles/r12/frontend_bench.json] [--batches 8,64] [--no-step]

fbank   ops.kaldi_fbank (avs_wave_sums + avs_kaldi_fbank) at 64 clips of 160 000 samples -> [64, 1024, 128], plain and mixed, beside the same
        computation composed from torch operations on the same device (unfold, frame mean, pre-emphasis, window, torch.fft.rfft, matmul with
        the mel matrix, log: what a user of torch without torchaudio has today), interleaved in one process: ROUNDS rounds, in each round every
        variant timed over ITERS calls between device events after a warm-up; median and spread over the rounds.  Bytes the algorithm needs:
        the samples the frames cover (4 B each, twice with a partner) plus the output rows; GB/s = those bytes over the median time.  The
        composition's result is compared with the kernel's (largest log-domain gap on cells above 1e-6 of their row's maximum).
step    the --wave-input training step of the launcher (host draws, kaldi_fbank with normalisation and mixup, mix_frames, mixup_labels, one
        augmentation plan, the fused mm step) beside the plain mm step on ready-made tensors, CAVMAEFT_BASE(527), batch 8 and 64, interleaved,
        REPS repetitions of `--steps` steps each.
Nothing here is tuned to the result: shapes and repeat counts are fixed above the measurements."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avsiam_amd import ops, preprocess  # noqa: E402

ROUNDS, ITERS, REPS = 7, 20, 3
B, N, T = 64, 160000, 1024


def stat(v):
    return {"median": sorted(v)[len(v) // 2], "spread": [min(v), max(v)], "rounds": len(v)}


def torch_fbank(wave, window, melw, T):
    """the plain path composed from torch operations, fp32: [B, n] -> [B, T, 128] (clips of one length; the mean of the whole row)"""
    w = wave - wave.mean(dim=1, keepdim=True)
    fr = w.unfold(1, 400, 160)[:, :T]
    fr = fr - fr.mean(dim=2, keepdim=True)
    fr = (fr - 0.97 * torch.cat([fr[..., :1], fr[..., :-1]], dim=2)) * window
    spec = torch.fft.rfft(fr, n=512, dim=2)
    power = spec.real * spec.real + spec.imag * spec.imag
    out = torch.log(torch.clamp(power @ melw, min=1.1920929e-07))
    if out.shape[1] < T:
        out = torch.nn.functional.pad(out, (0, 0, 0, T - out.shape[1]))
    return out


def time_calls(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_fbank():
    g = torch.Generator(device="cuda").manual_seed(0)
    wave = torch.randn(B, N, device="cuda", generator=g) * 0.1
    partner = torch.randn(B, N, device="cuda", generator=g) * 0.1
    lam = torch.full((B,), 0.43, device="cuda")
    window = torch.from_numpy(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)).float().cuda()
    melw = torch.from_numpy(preprocess.fbank_mel_weights().T.copy()).float().cuda()
    out = torch.empty(B, T, 128, device="cuda")
    ways = {"kernel_plain": lambda: ops.kaldi_fbank(wave, target_length=T, out=out),
            "kernel_mixed": lambda: ops.kaldi_fbank(wave, partner=partner, lam=lam, target_length=T, out=out),
            "torch_composition_plain": lambda: torch_fbank(wave, window, melw, T),
            "wave_sums_plain_alone": lambda: ops.wave_sums(wave), "wave_sums_mixed_alone": lambda: ops.wave_sums(wave, None, partner, None)}
    m = min(T, 1 + (N - 400) // 160)
    covered = 160 * (m - 1) + 400
    nbytes = {"kernel_plain": 4.0 * B * (covered + T * 128), "kernel_mixed": 4.0 * B * (2 * covered + T * 128)}
    nbytes["torch_composition_plain"] = nbytes["kernel_plain"]
    nbytes["wave_sums_plain_alone"], nbytes["wave_sums_mixed_alone"] = 4.0 * B * N, 8.0 * B * N      # (the first launch of kernel_*, by itself)
    for fn in ways.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, fn in ways.items():
            t[k].append(time_calls(fn, ITERS))
    res = {"shape": {"clips": B, "samples": N, "rows": T, "frames_per_clip": m}, "calls_per_round": ITERS, "variants": {}}
    for k in ways:
        s = stat(t[k])
        res["variants"][k] = {"ms": s, "algorithm_bytes": nbytes[k], "gb_per_s_at_median": nbytes[k] / (s["median"] * 1e-3) / 1e9}
    res["kernel_launches_note"] = "kernel_* times cover both launches of ops.kaldi_fbank (avs_wave_sums, avs_kaldi_fbank)"
    a = ops.kaldi_fbank(wave, target_length=T).double()
    b = torch_fbank(wave, window, melw, T).double()
    keep = a[:, :m] > (a[:, :m].max(dim=2, keepdim=True).values + np.log(1e-6))
    res["kernel_vs_torch_composition_max_log_gap"] = float((a[:, :m] - b[:, :m]).abs()[keep].max())
    res["speedup_over_torch_composition"] = res["variants"]["torch_composition_plain"]["ms"]["median"] / res["variants"]["kernel_plain"]["ms"]["median"]
    return res


def bench_step(batches, steps, warmup):
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, SyntheticWaveFtLoader, apply_freeze_base
    cfg, L = AVSiamConfig(), 527
    mean, std = -5.081, 4.4849
    fill = (0.0 - mean) / std
    res = {}
    for bs in batches:
        m = CAVMAEFT_BASE(L).cuda()
        apply_freeze_base(m, False)
        ld = SyntheticFtLoader(cfg, bs, 1, L, m.arena.p.device)
        wl = SyntheticWaveFtLoader(cfg, bs, 1, L, m.arena.p.device, mixup=0.5, norm=(mean, std))
        kw = dict(head_lr=100.0, mm_lr=100.0)

        def plain():
            m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw)

        def wave_input():
            for a, v, y in wl:
                m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", aug=m.draw_aug(bs, 48, 192, True, fill=fill), **kw)

        def front_end_only():
            for _ in wl:
                pass
        ways = {"plain_mm_step": plain, "wave_input_mm_step": wave_input, "front_end_only": front_end_only}
        t = {k: [] for k in ways}
        for _ in range(REPS):
            for k, fn in ways.items():
                for _ in range(warmup):
                    fn()
                torch.cuda.synchronize()
                t[k].append(time_calls(fn, steps))
        res[f"batch_{bs}"] = {k: {"ms": [round(x, 4) for x in v], "mean_ms": round(sum(v) / len(v), 4), "spread_ms": round(max(v) - min(v), 4)}
                              for k, v in t.items()}
        del m
        torch.cuda.empty_cache()
    return {"recipe": {"mixup": 0.5, "freqm": 48, "timem": 192, "noise": True, "ftmode": "mm_grad", "branch": "mm", "n_class": L},
            "steps": steps, "warmup": warmup, "repetitions": REPS, "results": res,
            "note": "wave_input_mm_step includes the host draws and their upload; front_end_only is that step without the model"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "frontend_bench.json"))
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", dest="no_step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "fbank": bench_fbank()}
    print(json.dumps(res["fbank"]), flush=True)
    if not args.no_step:
        res["step"] = bench_step([int(b) for b in args.batches.split(",")], args.steps, args.warmup)
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
