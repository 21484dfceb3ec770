#!/usr/bin/env python3
"""Attention throughput vs sequence length (random data, one process).  usage: bench_attn.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avsiam_amd import ops  # noqa: E402
from avsiam_amd.engine import attention_plan  # noqa: E402


def timeit(fn, iters=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def run_case(name, H, hd, lens, dev, tile_rows=(128, 64)):
    D = H * hd
    rows = sum(lens)
    rp = ops.pad_rows(rows)
    qkv = torch.zeros(rp, 3 * D, device=dev, dtype=torch.bfloat16)
    qkv[:rows] = torch.randn(rows, 3 * D, device=dev).bfloat16()
    out = torch.zeros(rp, D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=dev)
    dout = torch.zeros(rp, D, device=dev, dtype=torch.bfloat16)
    dout[:rows] = torch.randn(rows, D, device=dev).bfloat16()
    dqkv = torch.zeros_like(qkv)
    delta = torch.zeros_like(lse)
    fl = 4.0 * sum(L * L for L in lens) * D
    msg = f"{name:34s} rows={rows:6d}:"
    for tr in tile_rows:
        tiles = ops.AttnTiles(lens, dev, tile_rows=tr)
        if "--ring-ab" in sys.argv:              # register-staged vs LDS-DMA ring kernels, interleaved rounds in this one process (median)
            from avsiam_amd import _lib
            res = {0: ([], []), 1: ([], [])}
            for _ in range(5):
                for ring in (0, 1):
                    _lib.tuning_set("attn_ring", ring)
                    res[ring][0].append(timeit(lambda: ops.attn_fwd(qkv, tiles, H, out, lse), 10))
                    res[ring][1].append(timeit(lambda: ops.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv), 10))
            _lib.tuning_set("attn_ring", 0)
            med = lambda v: sorted(v)[len(v) // 2]
            msg += (f"  [tile {tr}] fwd staged {med(res[0][0])*1e6:7.1f} ring {med(res[1][0])*1e6:7.1f} us ({fl/med(res[1][0])/1e12:5.0f} TF/s)"
                    f"  bwd staged {med(res[0][1])*1e6:7.1f} ring {med(res[1][1])*1e6:7.1f} us ({2.5*fl/med(res[1][1])/1e12:5.0f} TF/s)")
            continue
        tf = timeit(lambda: ops.attn_fwd(qkv, tiles, H, out, lse), 10)
        tb = timeit(lambda: ops.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv), 10)
        msg += (f"  [tile {tr}] fwd {tf*1e6:7.1f} us {fl/tf/1e12:6.1f} TF/s {rows*8.0*D/tf/1e9:6.0f} GB/s"
                f"  bwd {tb*1e6:7.1f} us {2.5*fl/tb/1e12:6.1f} TF/s {rows*24.0*D/tb/1e9:6.0f} GB/s")
        if "--g8" in sys.argv:          # the fp8 modes' variants: e4m3 copy of the output / e5m2 copy of dqkv written as well (and, lean, no bf16 dK / dV)
            rec = ops.Fp8Records(2, dev, fmax=ops.BF8_MAX)
            rec.q[:, 0], rec.q[:, 1], rec.q[:, 2] = 1000.0, 1e-3, 1e30      # (scale, 1 / scale, amax seen: as in a calibrated step no wave issues the amax atomic)
            o8 = torch.zeros(rp, D, device=dev, dtype=torch.uint8)
            d8 = torch.zeros(rp, 3 * D, device=dev, dtype=torch.uint8)
            tf8 = timeit(lambda: ops.attn_fwd(qkv, tiles, H, out, lse, out8=o8, q8=rec.rec(0)), 10)
            tb8 = timeit(lambda: ops.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv, dqkv8=d8, q8=rec.rec(1)), 10)
            tb8l = timeit(lambda: ops.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv, dqkv8=d8, q8=rec.rec(1), kv_bf16=False), 10)
            msg += f"  [+8-bit copies] fwd {tf8*1e6:7.1f} us  bwd {tb8*1e6:7.1f} us  bwd without bf16 dK/dV {tb8l*1e6:7.1f} us"
    # the backward as the engine runs it (engine.attention_plan: the fused classes, the cut and the tile rows of the two-kernel rest)
    def mixed_bwd(label, lean=False, **kw):
        p = attention_plan(lens, hd, attn_fused=True, inference=False, **kw)
        f = [ops.AttnSeqs(lens, dev, lo, hi) for lo, hi in p.fused]
        tl = ops.AttnTiles(lens, dev, tile_rows=p.bwd_rows, min_len=p.cut)
        g8 = dict(dqkv8=d8, q8=rec.rec(1), kv_bf16=False) if lean else {}

        def mixed():
            if tl.ntiles:
                ops.attn_bwd(qkv, tl, H, out, dout, lse, delta, dqkv, **g8)
            for sq in f:
                ops.attn_bwd_fused(qkv, sq, H, out, dout, lse, dqkv, **g8)
        return label % dict(cut=p.cut, rows=p.bwd_rows, us=timeit(mixed, 10) * 1e6)
    if hd == 80 and min(lens) <= 64:
        # head dim 80: the fused kernel exists for 64-row workgroups only
        for tr in tile_rows:
            msg += mixed_bwd("  [fused<=%(cut)d + tile %(rows)d] bwd %(us)7.1f us", attn_tile=tr, fused224=False)
            if "--g8" in sys.argv:
                msg += mixed_bwd(" (lean e5m2 %(us)7.1f us)", lean=True, attn_tile=tr, fused224=False)
    if hd in (32, 64) and min(lens) <= 128:
        msg += mixed_bwd("  [fused<=%(cut)d] bwd %(us)7.1f us", attn_tile=0, fused224=False)
        if hd == 64 and any(128 < L <= 224 for L in lens):
            # round 6: sequences of 129 .. 224 tokens through the 7-wave fused kernel as well
            msg += mixed_bwd("  [fused<=%(cut)d] bwd %(us)7.1f us", attn_tile=0, fused224=True)
    print(msg, flush=True)


def step_mixes(dev):
    """the sequence mixes of the bench step (batch 64, 10 frames): contrastive pass (five keep ratios), MAE towers, joint layers, decoder"""
    vid = [196] * 130 + [156] * 130 + [117] * 130 + [78] * 130 + [39] * 120
    aud = [512] * 13 + [409] * 13 + [307] * 13 + [204] * 13 + [102] * 12
    if "--decoder-only" in __import__("sys").argv:            # for counter runs (tools/pmc_attn.sh)
        return run_case("decoder (64x2472)", 16, 32, [2472] * 64, dev, tile_rows=(128,))
    run_case("contrastive pass (audio+video)", 12, 64, aud + vid, dev)
    run_case("contrastive pass, video only", 12, 64, vid, dev)
    run_case("contrastive pass, audio only", 12, 64, aud, dev)
    run_case("MAE towers (64x128 + 640x49)", 12, 64, [128] * 64 + [49] * 640, dev)
    run_case("MAE joint layers (64x618)", 12, 64, [618] * 64, dev)
    run_case("decoder (64x2472)", 16, 32, [2472] * 64, dev, tile_rows=(128,))


def huge_mixes(dev):
    """the sequence mixes of the ViT-H/14 step (batch 64, 10 frames; 16 heads of 80): contrastive pass, MAE towers, joint layers, decoder"""
    vid = [256] * 130 + [204] * 130 + [153] * 130 + [102] * 130 + [51] * 120
    aud = [657] * 13 + [525] * 13 + [394] * 13 + [262] * 13 + [131] * 12
    tr = (128, 64) if "--tile64" in sys.argv else (128,)
    run_case("H/14 contrastive pass (audio+video)", 16, 80, aud + vid, dev, tile_rows=tr)
    run_case("H/14 contrastive pass, video only", 16, 80, vid, dev, tile_rows=tr)
    run_case("H/14 MAE towers (64x164 + 640x64)", 16, 80, [164] * 64 + [64] * 640, dev, tile_rows=tr)
    run_case("H/14 MAE joint layers (64x804)", 16, 80, [804] * 64, dev, tile_rows=tr)
    run_case("H/14 decoder (64x3217)", 16, 32, [3217] * 64, dev, tile_rows=(128,))


def main():
    dev = "cuda"
    import sys
    if "--step" in sys.argv:
        return step_mixes(dev)
    if "--huge" in sys.argv:
        return huge_mixes(dev)
    for H, hd, L, rows_target in [(12, 64, 39, 40000), (12, 64, 49, 40000), (12, 64, 78, 40000), (12, 64, 117, 40000), (12, 64, 128, 40000),
                                  (12, 64, 156, 40000), (12, 64, 196, 40000), (12, 64, 307, 40000), (12, 64, 512, 40000), (12, 64, 618, 40000),
                                  (16, 32, 708, 80000), (16, 32, 2472, 160000)]:
        D = H * hd
        nseq = max(1, rows_target // L)
        lens = [L] * nseq
        rows = nseq * L
        rp = ops.pad_rows(rows)
        qkv = torch.zeros(rp, 3 * D, device=dev, dtype=torch.bfloat16)
        qkv[:rows] = torch.randn(rows, 3 * D, device=dev).bfloat16()
        out = torch.zeros(rp, D, device=dev, dtype=torch.bfloat16)
        lse = torch.zeros(H, rp, device=dev)
        dout = torch.zeros(rp, D, device=dev, dtype=torch.bfloat16)
        dout[:rows] = torch.randn(rows, D, device=dev).bfloat16()
        dqkv = torch.zeros_like(qkv)
        delta = torch.zeros_like(lse)
        fl = 4.0 * nseq * L * L * D
        msg = f"H={H} hd={hd} L={L:5d} nseq={nseq:5d}:"
        for tr in (128, 64):
            tiles = ops.AttnTiles(lens, dev, tile_rows=tr)
            tf = timeit(lambda: ops.attn_fwd(qkv, tiles, H, out, lse))
            tb = timeit(lambda: ops.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv))
            msg += f"  [tile {tr}] fwd {tf*1e6:7.1f} us {fl/tf/1e12:6.1f} TF/s bwd {tb*1e6:7.1f} us {2.5*fl/tb/1e12:6.1f} TF/s"
        print(msg, flush=True)


if __name__ == "__main__":
    main()
