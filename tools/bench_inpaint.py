#!/usr/bin/env python3
"""Reconstructions from the MAE pass on one MI355X (two JSON files):

    python tools/bench_inpaint.py [--out profiles/r15/inpaint_bench.json] [--margins profiles/r15/inpaint_margins.json] [--no-margins]

Shape: ViT-B at batch 64 with one frame (audio [64, 1024, 128], frames [64, 3, 224, 224]; 75 % of the tokens masked, compact prediction rows).
kernel   (a) ops.unpatchify alone on the buffers of a finished MAE forward, per modality - called eagerly (what a caller pays: host checks, the
         workspace allocation and three launches included) and replayed from a captured graph of ITERS calls (the device time alone) -, beside the same composition written with torch
         operations on the same device (scatter the compact rows, the reference's einsum, torch.where with the cell mask), interleaved in one
         process: ROUNDS rounds, in each round every variant timed over ITERS calls between device events after a warm-up; median and min - max.
         Bytes the algorithm must move: the masked prediction rows in, the kept input cells in, the output out; GB/s = those bytes over the
         median time, beside the 6.29 TB/s a float4 copy measures on this part (the working set, ~70 MB, fits the 256 MB Infinity Cache, so a
         figure above the HBM rate is possible and says nothing about HBM).
model    (b) CAVMAE_BASE.inpaint() as a whole beside the no_grad MAE forward it contains, the same way.
margins  the worst figures of the checks in tests/test_inpaint_gpu.py (masked-cell relative L2 against the CPU oracle at the parity shapes and
         against the reference golden), measured here so that the margin to the 2e-2 bound is on record.
Nothing here is tuned to the result: shapes and repeat counts are fixed above the measurements."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, ITERS = 7, 20
B = 64
COPY_TBS = 6.29


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


def torch_unpatchify(pred, inp, mask, pid, id_base, audio, L):
    """the same picture from torch operations: compact rows scattered to [n, L, P], unpatchify (cav_mae_base.py:353-363), composed with the input"""
    import torch
    n = mask.numel() // L
    P = pred.shape[1]
    rows = torch.zeros(n * L, P, device=pred.device)
    rows.index_copy_(0, pid.long() - id_base, pred[:pid.numel()])
    if audio:
        T, F = inp.shape[1:]
        x = rows.reshape(n, F // 16, T // 16, 16, 16)
        rec = torch.einsum("nhwpq->nwqhp", x).reshape(n, T, F)
        cm = mask.reshape(n, F // 16, T // 16).transpose(1, 2).repeat_interleave(16, 1).repeat_interleave(16, 2)
    else:
        C, H, W = inp.shape[-3:]
        x = rows.reshape(n, H // 16, W // 16, 16, 16, C)
        rec = torch.einsum("nhwpqc->nchpwq", x).reshape(n, C, H, W)
        cm = mask.reshape(n, 1, H // 16, W // 16).repeat_interleave(16, 2).repeat_interleave(16, 3)
    return torch.where(cm == 1, rec, inp.reshape(rec.shape))


def bench():
    import torch
    from avsiam_amd import ops
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.weights import synth_inputs
    cfg = AVSiamConfig()
    a, v = synth_inputs(cfg, B, 87)
    a, v = a.cuda(), v.cuda()
    m = CAVMAE_BASE(cfg=cfg, verbose=False).cuda()
    res0 = m.inpaint(a, v)
    eng = m._engine("mae", B)
    La, Lv = cfg.audio_tokens, cfg.video_tokens
    out_a, out_v = torch.empty_like(a), torch.empty_like(v)
    sides = {"audio": (eng.p_a, eng.audio, eng.mask_a, eng.pid_a, 0, True, La, out_a), "frames": (eng.p_v, eng.imgs, eng.mask_v, eng.pid_v, B * La, False, Lv, out_v)}
    ways, nbytes, gaps = {}, {}, {}
    for name, (pred, inp, mask, pid, base, audio, L, out) in sides.items():
        ways[f"kernel_{name}"] = (lambda pred=pred, inp=inp, mask=mask, pid=pid, base=base, audio=audio, L=L, out=out:
                                  ops.unpatchify(pred, inp, mask, audio, L, row_id=pid, id_base=base, out=out))
        ways[f"torch_composition_{name}"] = (lambda pred=pred, inp=inp, mask=mask, pid=pid, base=base, audio=audio, L=L:
                                             torch_unpatchify(pred, inp, mask, pid, base, audio, L))
        masked = float(mask.sum().item())
        cells = 4.0 * inp.numel()
        frac = masked / mask.numel()
        nbytes[name] = {"masked_pred_rows_in": masked * pred.shape[1] * 4, "kept_input_cells_in": cells * (1 - frac), "output_out": cells}
        got = ops.unpatchify(pred, inp, mask, audio, L, row_id=pid, id_base=base)[0]
        gaps[name] = bool(torch.equal(got, torch_unpatchify(pred, inp, mask, pid, base, audio, L)))
    # the same calls replayed from a captured graph: ITERS calls per replay, so the host's share of a call (argument checks, the workspace
    # allocation, three launches through ctypes - tens of microseconds, more than the kernel) drops out and the device time is left
    graphs = {}
    for name in sides:
        fn = ways[f"kernel_{name}"]
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(ITERS):
                fn()
        graphs[name] = g
        ways[f"kernel_{name}_graph_replay"] = g.replay
    ways["mae_forward_no_grad"] = lambda: m(a, v, mae_loss_weight=1, contrast_loss_weight=0)
    ways["inpaint"] = lambda: m.inpaint(a, v)

    def guarded(fn):                       # (everything under no_grad: the forward beside inpaint() is the one inpaint() contains)
        def run():
            with torch.no_grad():
                return fn()
        return run
    ways = {k: guarded(fn) for k, fn in ways.items()}
    for fn in ways.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, fn in ways.items():
            if k.endswith("_graph_replay"):
                t[k].append(time_calls(fn, 5) / ITERS)                      # one replay = ITERS calls
            else:
                t[k].append(time_calls(fn, ITERS if k.startswith(("kernel", "torch")) else 5))
    res = {"shape": {"model": "ViT-B", "batch": B, "frames": 1, "audio": list(a.shape), "imgs": list(v.shape), "masked_audio_tokens": int(res0.mask_a.sum().item()),
                     "masked_frame_tokens": int(res0.mask_v.sum().item())},
           "copy_rate_tb_per_s": COPY_TBS, "variants": {}, "kernel_equals_torch_composition": gaps}
    for k in ways:
        s = stat(t[k])
        res["variants"][k] = {"ms": s}
        side = k.replace("_graph_replay", "").split("_")[-1]
        if k.startswith(("kernel", "torch")):
            tot = sum(nbytes[side].values())
            res["variants"][k].update(algorithm_bytes=nbytes[side], gb_per_s_at_median=tot / (s["median"] * 1e-3) / 1e9,
                                      share_of_copy_rate=tot / (s["median"] * 1e-3) / (COPY_TBS * 1e12))
    for side in sides:
        res[f"speedup_over_torch_composition_{side}"] = res["variants"][f"torch_composition_{side}"]["ms"]["median"] / res["variants"][f"kernel_{side}"]["ms"]["median"]
    res["inpaint_minus_forward_ms_at_median"] = res["variants"]["inpaint"]["ms"]["median"] - res["variants"]["mae_forward_no_grad"]["ms"]["median"]
    return res


def margins():
    """the figures tests/test_inpaint_gpu.py asserts on, measured"""
    import numpy as np
    import torch
    from avsiam_amd.config import AVSiamConfig, vit_huge14
    from avsiam_amd.maskplan import make_mae_plan
    from avsiam_amd.models import CAVMAE_BASE, CAVMAE_HUGE
    from avsiam_amd.preprocess import unpatchify_reference
    from avsiam_amd.weights import synth_inputs, synth_state
    from oracle import ref_cpu
    from tests.helpers import golden_plan, load_golden
    torch.set_num_threads(16)
    out = {"bound_relative_l2": 2e-2}

    def cells(mask, shape, audio, S):
        C = 1 if audio else shape[1]
        return unpatchify_reference(np.ones(mask.shape + (256 * C,), dtype=np.float32), np.zeros(shape, dtype=np.float32), audio, S, mask) == 1

    for name, cfg, bs in (("vit_base_B4_T1", AVSiamConfig(audio_tokens=128, frames=1), 4), ("vit_base_B2_T3", AVSiamConfig(audio_tokens=128, frames=3), 2),
                          ("vit_huge14_B2_T2_depth2", vit_huge14(frames=2, depth=2), 2)):
        S, T, La, Lv = cfg.st, cfg.frames, cfg.audio_tokens, cfg.video_tokens
        a, v = synth_inputs(cfg, bs, 99)
        plan = make_mae_plan(cfg, bs, torch.Generator().manual_seed(7))
        m = (CAVMAE_HUGE if cfg.embed_dim == 1280 else CAVMAE_BASE)(cfg=cfg, init_seed=4321, init_mode="random", verbose=False).cuda()
        res = m.inpaint(a.cuda(), v.cuda(), mask_plan=plan)
        ex = {}
        with torch.no_grad():
            ref_cpu.forward(synth_state(cfg, 4321, "random", include_dead=False), cfg, a, v, plan, mae_loss_weight=1, contrast_loss_weight=0, extras=ex)
        fold = lambda x: x.reshape(-1, *x.shape[-3:])                                        # noqa: E731
        ma, mv = plan.mask_a().numpy(), plan.mask_v().reshape(bs * T, Lv).numpy()
        rec = {}
        for k, got, rows, inp, mask, audio in (("audio", res.audio.cpu().numpy(), ex["pred_a"].numpy().reshape(bs, La, -1), a.numpy(), ma, True),
                                               ("frames", fold(res.imgs.cpu().numpy()), ex["pred_v"].numpy().reshape(bs * T, Lv, -1), fold(v.numpy()), mv, False)):
            want = unpatchify_reference(rows, inp, audio, S, mask)
            c = cells(mask, inp.shape, audio, S)
            rec[k + "_masked_rel_l2"] = float(np.linalg.norm(got.astype(np.float64)[c] - want.astype(np.float64)[c]) / np.linalg.norm(want.astype(np.float64)[c]))
            rec[k + "_kept_cells_equal_input"] = bool(np.array_equal(got[~c], inp[~c]))
        out["oracle_" + name] = rec
        del m
    g, base = load_golden("inp_m_w1_b4"), load_golden("m_w1_b4")
    cfg = AVSiamConfig()
    a, v = synth_inputs(cfg, int(base["batch"]), int(base["input_seed"]), None)
    m = CAVMAE_BASE(cfg=cfg, init_seed=int(base["weight_seed"]), init_mode="random", verbose=False).cuda()
    res = m.inpaint(a.cuda(), v.cuda(), mask_plan=golden_plan(base))
    rec = {}
    for k, got, mask, audio in (("recon_a", res.audio.cpu().numpy(), base["mask_a"], True), ("recon_v", res.imgs.cpu().numpy(), base["mask_v"], False)):
        c = cells(mask, got.shape, audio, 16)
        l2 = float(np.linalg.norm(got.astype(np.float64)[c]))
        rec[k] = {"masked_l2": l2, "reference_masked_l2": float(g[k + "_masked_l2"]), "relative_gap": abs(l2 - float(g[k + "_masked_l2"])) / float(g[k + "_masked_l2"])}
    out["golden_m_w1_b4"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r15", "inpaint_bench.json"))
    ap.add_argument("--margins", default=os.path.join("profiles", "r15", "inpaint_margins.json"))
    ap.add_argument("--no-margins", dest="no_margins", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), **bench()}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    if not args.no_margins:
        mg = margins()
        print(json.dumps(mg), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.margins)), exist_ok=True)
        with open(args.margins, "w") as f:
            json.dump(mg, f, indent=1)
        print("wrote", args.margins)


if __name__ == "__main__":
    main()
