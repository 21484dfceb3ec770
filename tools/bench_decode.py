#!/usr/bin/env python3
"""Training from files on one MI355X (one JSON file):

    python tools/bench_decode.py [--out profiles/r21/decode_bench.json] [--no-front]
    python tools/bench_decode.py --parent DIR [--out ...]          # (c) alone: DIR holds a built checkout of the parent commit

kernel  (a) ops.decode_pcm on the payloads of 64 clips of 10 s - stereo PCM16 at 44.1 kHz and, as a second line, mono PCM24 at 48 kHz - beside
        the same decode composed from torch operations on the same device (PCM16: view(int16), convert, scale, permute; PCM24: the byte
        arithmetic), interleaved in one process: ROUNDS rounds, in each round every variant timed over ITERS calls between device events after
        a warm-up; median and min - max over the rounds.  Bytes the algorithm must move: the payload once in, 4 * C * frames out; GB/s =
        those bytes over the median time, also as a fraction of the 6.29 TB/s float4-copy rate measured on this device (README).  The
        composition's result is compared with the kernel's, bit for bit.
front   (b) a dataset of 512 such stereo PCM16 files with one 256 x 340 .npy frame each is written to a temporary directory; per batch of 64:
        the file loader's device side (upload, decode, resample, fbank with mixup, resize) beside the --wave-input --sample-rate 44100
        --audio-channels 2 --frame-size 256 340 front end from device-resident tensors; the loader's host side (read, parse, collate into
        pinned buffers) at 0 and at 8 workers, a host clock around whole epochs (the first, which starts the workers, apart); and the mm training step fed by
        the file loader at 0 and 8 workers beside the step fed by the synthetic loader.
parent  (c) tools/bench_resample.py's procedure: the plain mm fine-tuning step at batch 64 and bench.py on the parent commit against this one,
        fresh processes alternating, the order of the two swapped from one alternation to the next.  Merged into --out.
Nothing here is tuned to the result: shapes and repeat counts are fixed above the measurements."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, ITERS, REPS = 7, 10, 3
B, SECONDS = 64, 10
COPY_RATE = 6.29e12                                           # float4 copy on one MI355X, bytes / s (README)
LINES = {"pcm16_44100_stereo": ("S16", 44100, 2), "pcm24_48000_mono": ("S24", 48000, 1)}
FRAME_H, FRAME_W, CLIPS = 256, 340, 512


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


def torch_decode(payload, fmt, C, n):
    """the decode composed from torch operations: payload uint8 [B, byte_stride] -> fp32 [B, C, n]"""
    import torch
    Bx = payload.shape[0]
    if fmt == "S16":
        x = payload[:, :n * C * 2].contiguous().view(torch.int16).view(Bx, n, C)
        return (x.to(torch.float32) * 2.0 ** -15).permute(0, 2, 1).contiguous()
    b = payload[:, :n * C * 3].reshape(Bx, n, C, 3).to(torch.int32)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    v = (v ^ 0x800000) - 0x800000
    return (v.to(torch.float32) * 2.0 ** -23).permute(0, 2, 1).contiguous()


def bench_kernel():
    import torch
    from avsiam_amd import ops, preprocess
    res = {"lines": {}}
    for name, (fmt, rate, C) in LINES.items():
        code = preprocess.PCM_NAMES.index(fmt)
        n = rate * SECONDS
        nb = n * C * preprocess.PCM_BYTES[code]
        byte_stride = -(-nb // 16) * 16
        g = torch.Generator(device="cuda").manual_seed(0)
        payload = torch.randint(0, 256, (B, byte_stride), device="cuda", generator=g, dtype=torch.uint8)
        desc = torch.tensor([[code, n]] * B, dtype=torch.int32, device="cuda")
        stride = -(-n // 4) * 4
        out, out_l = torch.empty(B, C, stride, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        ways = {"kernel": lambda: ops.decode_pcm(payload, desc, C, stride, out=out, out_lengths=out_l), "torch_composition": lambda: torch_decode(payload, fmt, C, n)}
        nbytes = float(B) * (nb + 4.0 * C * n)
        print(f"{name}: warm-up", flush=True)
        for fn in ways.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ways}
        for _ in range(ROUNDS):
            for k, fn in ways.items():
                t[k].append(time_calls(fn, ITERS))
        line = {"shape": {"clips": B, "channels": C, "rate": rate, "frames": n, "format": fmt, "payload_mb": B * nb / 1e6, "output_mb": 4.0 * B * C * n / 1e6},
                "variants": {}}
        for k in ways:
            s = stat(t[k])
            rate_bs = nbytes / (s["median"] * 1e-3)
            line["variants"][k] = {"ms": s, "algorithm_bytes": nbytes, "gb_per_s_at_median": rate_bs / 1e9, "fraction_of_float4_copy_rate": rate_bs / COPY_RATE}
        a, b = ops.decode_pcm(payload, desc, C, stride)[0][..., :n], torch_decode(payload, fmt, C, n)
        line["kernel_equals_torch_composition_bitwise"] = bool(torch.equal(a.contiguous().view(torch.int32), b.view(torch.int32)))
        line["speedup_over_torch_composition"] = line["variants"]["torch_composition"]["ms"]["median"] / line["variants"]["kernel"]["ms"]["median"]
        res["lines"][name] = line
        del payload, out
        torch.cuda.empty_cache()
    return res


def write_dataset(root):
    """CLIPS files of 10 s stereo PCM16 at 44.1 kHz (64 distinct payloads, each listed 8 times), one .npy frame per clip, 527 classes"""
    import struct
    import numpy as np
    rng = np.random.default_rng(0)
    n = 44100 * SECONDS
    os.makedirs(os.path.join(root, "video", "frame_0"))
    with open(os.path.join(root, "labels.csv"), "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i:03d},c{i}\n" for i in range(527)))
    data = []
    for i in range(CLIPS):
        wav = os.path.join(root, f"clip{i % 64}.wav")
        if i < 64:
            pay = (rng.standard_normal(2 * n) * 3276.8).clip(-32768, 32767).astype("<i2").tobytes()
            head = b"fmt " + struct.pack("<IHHIIHH", 16, 1, 2, 44100, 44100 * 4, 4, 16) + b"data" + struct.pack("<I", len(pay))
            with open(wav, "wb") as f:
                f.write(b"RIFF" + struct.pack("<I", 4 + len(head) + len(pay)) + b"WAVE" + head + pay)
        np.save(os.path.join(root, "video", "frame_0", f"clip{i}.npy"), rng.integers(0, 256, (FRAME_H, FRAME_W, 3), dtype=np.uint8))
        data.append({"wav": wav, "labels": f"/m/{i % 527:03d},/m/{(7 * i + 3) % 527:03d}", "video_id": f"clip{i}", "video_path": os.path.join(root, "video")})
    with open(os.path.join(root, "data.json"), "w") as f:
        json.dump({"data": data}, f)
    return os.path.join(root, "data.json"), os.path.join(root, "labels.csv")


def bench_front(steps, warmup):
    import torch
    from bench_frames import _model_and_kw
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    cfg, L, norm = AVSiamConfig(), 527, (-5.081, 4.4849)
    fill = (0.0 - norm[0]) / norm[1]
    res = {}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.time()
        data_json, label_csv = write_dataset(root)
        res["dataset_written_s"] = round(time.time() - t0, 2)
        m, kw = _model_and_kw(B)
        dev = m.arena.p.device
        ds = FtFileDataset(data_json, label_csv, L)
        loaders = {w: FileFtLoader(ds, cfg, B, dev, mixup=0.5, norm=norm, train=True, total_frame=1, num_workers=w) for w in (0, 8)}
        synth = SyntheticWaveFtLoader(cfg, B, 2, L, dev, mixup=0.5, norm=norm, sample_rate=44100, channels=2, frame_size=(FRAME_H, FRAME_W))
        # host side alone: whole epochs (8 batches of 64) under a host clock
        host = {w: [] for w in loaders}
        for _ in range(REPS + 1):
            for w, ld in loaders.items():
                t0 = time.perf_counter()
                nb = sum(1 for _ in ld.staged(0))
                host[w].append((time.perf_counter() - t0) * 1e3 / nb)
        res["loader_host_side_ms_per_batch"] = {f"workers_{w}": {"ms": [round(x, 2) for x in v[1:]], "median_ms": round(sorted(v[1:])[len(v[1:]) // 2], 2),
                                                                "first_epoch_ms": round(v[0], 2)} for w, v in host.items()}
        # device side of one staged batch beside the synthetic front end
        batch = next(iter(loaders[0].staged(0)))

        def synth_front():
            for _ in synth:
                pass
        ways = {"file_front_end_from_pinned_batch": lambda: loaders[0].front_end(batch), "wave_input_sample_rate_front_end_2_batches": synth_front}
        t = {k: [] for k in ways}
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for k, fn in ways.items():
                t[k].append(time_calls(fn, 3))
        res["front_end_ms_per_batch"] = {"file_loader_device_side": stat(t["file_front_end_from_pinned_batch"]),
                                         "wave_input_sample_rate_device_resident": stat([x / 2.0 for x in t["wave_input_sample_rate_front_end_2_batches"]])}
        # the mm step fed by each loader: a host clock around epochs of 8 batches, ending in a synchronise

        def epoch_of(loader):
            def run():
                t0 = time.perf_counter()
                nb = 0
                for a, v, y in loader:
                    m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", aug=m.draw_aug(B, 48, 192, True, fill=fill), **kw)
                    nb += 1
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / nb
            return run
        runs = {"file_loader_workers_0": epoch_of(loaders[0]), "file_loader_workers_8": epoch_of(loaders[8]), "wave_input_sample_rate_device_resident": epoch_of(synth)}
        st = {k: [] for k in runs}
        for _ in range(warmup):
            for fn in runs.values():
                fn()
        for _ in range(steps):
            for k, fn in runs.items():
                st[k].append(fn())
        res["mm_step_ms_per_batch_host_clock"] = {k: stat(v) for k, v in st.items()}
    res["recipe"] = {"batch": B, "clips": CLIPS, "mixup": 0.5, "freqm": 48, "timem": 192, "noise": True, "branch": "mm", "n_class": L,
                     "audio": "10 s stereo PCM16 at 44.1 kHz", "frames": f"one {FRAME_H} x {FRAME_W} .npy per clip"}
    res["note"] = ("with mixup 0.5 about half of the clips bring a partner: the loader reads, stages and decodes about 1.5 files per clip; the files sit in the "
                   "page cache (they were just written); the workers are started in the first epoch (first_epoch_ms) and kept")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r21", "decode_bench.json"))
    ap.add_argument("--steps", type=int, default=5, help="(b): timed epochs per loader; with --parent: steps per process")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-front", dest="no_front", action="store_true")
    ap.add_argument("--reps", type=int, default=4, help="with --parent: alternations (an even number: each tree runs first equally often)")
    ap.add_argument("--parent", metavar="DIR", help="(c) alone: a built checkout of the parent commit")
    args = ap.parse_args()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    if args.parent:
        from bench_resample import against_parent
        res["untouched_paths_vs_parent"] = against_parent(args.parent, args.steps, args.warmup, args.reps)
    else:
        import torch
        assert torch.cuda.is_available(), "tools/bench_decode.py measures on a GPU"
        res["device"] = torch.cuda.get_device_name(0)
        res["kernel"] = bench_kernel()
        if not args.no_front:
            res["front_end"] = bench_front(args.steps, args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res)[:3000])


if __name__ == "__main__":
    main()
