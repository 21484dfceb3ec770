"""Fine-tuning throughput of CAVMAEFT_BASE's fused train_step (one JSON line).

    python tools/bench_ft_train.py [--steps 10] [--warmup 3] [--batches 8,64]

The AudioSet recipe (mm_grad, BCE, 527 classes, T = 1, lr 1e-4, head_lr = mm_lr = 100; egs/audioset/run_base_ft.sh): per branch (mm: loss on
out, a: out_a, v: out_v), the reference's 50 / 25 / 25 mix (traintest_ft_base.py:153-160), and freeze_base at the largest batch.  Every
number is ms per step (CUDA events over `steps` steps after `warmup`) and samples/s.  kernel_share: one extra profiled mix step per batch
with every launch timed by HIP events (ops.KernelProfiler): the share of the step in the kernels fine-tuning added (cls_loss,
segment_mean_bwd_acc) and in layernorm_bwd (all widths; the head-width calls are a handful of them).

    python tools/bench_ft_train.py --adam-table [--out profiles/rNN/ft_adam_table.json]
the Adam phase of a mm step (update, shadow transposes, head refresh) per batch: one avs_adam launch per contiguous run of the arena
(adam_step, the single-process path) against the one-launch avs_adam_table, interleaved in one process, three repetitions each.

    python tools/bench_ft_train.py --dp-one-rank [--out profiles/rNN/ft_dp_one_rank.json]
the whole data-parallel step at ONE rank with the collectives forced on (a one-rank RCCL communicator) beside the plain step of a twin
model, interleaved, three repetitions.  A scaling number needs more than one GPU and is not produced here.

    python tools/bench_ft_train.py --aug [--out profiles/rNN/ft_aug_bench.json]
the mm and a steps three ways, interleaved in one process, three repetitions each: "plain" (no augmentation), "fused" (freqm 48, timem 192,
noise: one plan draw per step and the augmentation inside the audio patch gather) and "two_pass" (the same draw, preprocess.augment_fbank
into a second tensor, then the plain step).  All three read a normalised fbank, so the only difference is the augmentation.
    python tools/bench_ft_train.py --aug --plain-only --tree <checkout of another commit, built> [--label parent]
the plain step alone with the package of another tree (the parent commit, which has no augmentation to time): run it alternately with the
line above and compare "plain" with "plain".

    python tools/bench_ft_train.py --guard [--out profiles/rNN/grad_guard_bench.json]
the guarded step (set_grad_guard): avs_grad_sumsq alone on the table of a mm step, as a fraction of the float4-copy rate on its 4 B per
element; the Adam phase guarded (grad_sumsq + adam_table_guarded) against unguarded (adam_table); the whole mm step guarded (max_norm 1.0,
so the coefficient is in play) against plain.  Seven rounds, the ways interleaved inside a round; median and min - max of the rounds.
    python tools/bench_ft_train.py --guard --plain-only --tree <checkout of another commit, built> [--label parent]
the plain step alone with the package of another tree: run it alternately with `--guard --plain-only` of this one.

    python tools/bench_ft_train.py --accum [--out profiles/rNN/grad_accum_bench.json]
gradient accumulation (set_grad_accumulation): avs_grad_accum alone in its copy and add forms, on the table of a mm step and with only the
v branch's classes live, as a fraction of the float4-copy rate on 8 / 12 B per element; beside it one dense acc.add_(g) over the whole
trainable range and the acc.zero_() a cycle would need; k = 4 micro-steps of batch 16 against four plain steps of batch 16 (mm, and the
50 / 25 / 25 mix).  Seven rounds, the ways interleaved inside a round; median and min - max of the rounds.
    python tools/bench_ft_train.py --accum --plain-only [--tree <checkout of another commit, built>] [--label parent]
the plain mm step alone (--batches), with this package or another tree's: run the two alternately.
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


REPS = 3


def _spread(xs):
    return {"ms": [round(x, 4) for x in xs], "mean_ms": round(sum(xs) / len(xs), 4), "spread_ms": round(max(xs) - min(xs), 4)}


def _adam_table(args):
    from avsiam_amd import ops
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.models.cav_mae_ft import CLASSES, grad_class
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base
    cfg, L = AVSiamConfig(), 527
    res = {"metric": "ft_adam_phase", "branch": "mm", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "repetitions": REPS, "geometry": dict(zip(("grid", "chunk_elems", "max_segs"), ops.adam_table_geometry())), "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        m = CAVMAEFT_BASE(L).cuda()
        apply_freeze_base(m, False)
        ld = SyntheticFtLoader(cfg, B, 1, L, m.arena.p.device)
        m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", head_lr=100.0, mm_lr=100.0)       # gradients of a mm step in the arena
        names = [n for n, p in m._params.items() if p.grad is not None]
        a = m.arena
        lo0, hi0 = a.range[1]
        table, ctl = m._adam_table(tuple(m._trainable())), ops.AdamCtl(a.p.device)
        live = {grad_class(n) for n in names}
        ctl.live[:len(CLASSES)] = torch.tensor([1.0 if c in live else 0.0 for c in CLASSES])
        def runs(i):
            m.adam_step(1e-4, 100.0, 100.0, names)

        def one(i):
            ctl.set_lr(1e-4, 1e-2, 1e-2)
            ops.adam_table(a.p[lo0:hi0], a.g[lo0:hi0], m._opt["m"], m._opt["v"], a.pb[lo0:hi0], table, ctl)
            a.refresh_shadows(None, cast=False)
            for e in list(m._engines.values()) + list(m._train_engines.values()):
                e.refresh_heads()

        t_runs, t_one = [], []
        for _ in range(REPS):
            t_runs.append(_time(runs, args.steps, args.warmup))
            t_one.append(_time(one, args.steps, args.warmup))
        res["results"][f"batch_{B}"] = {"per_run_launches": _spread(t_runs), "one_launch_table": _spread(t_one), "table_segments": len(table.segs),
                                        "parameters": int(sum(n for _, n, _, c in table.segs if CLASSES[c] in live))}
        del m
        torch.cuda.empty_cache()
    return res


def _dp_one_rank(args):
    from avsiam_amd import _lib
    from avsiam_amd.comm import RcclComm
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base
    cfg, L = AVSiamConfig(), 527
    comm = RcclComm(rank=0, world=1, always=True)
    res = {"metric": "ft_dp_one_rank", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "repetitions": REPS,
           "comm": "RcclComm(world=1, always=True)", "note": "cu_reserve is 0 for the plain step and 8 for the data-parallel one, as each runs in production", "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        plain, dp = CAVMAEFT_BASE(L).cuda(), CAVMAEFT_BASE(L).cuda()
        for m in (plain, dp):
            apply_freeze_base(m, False)
        dp.set_distributed(1, 0, comm)
        ld = SyntheticFtLoader(cfg, B, 1, L, dp.arena.p.device)
        r = {}
        for br in ("mm", "a", "v"):
            t_p, t_d = [], []
            for _ in range(REPS):
                for m, t in ((plain, t_p), (dp, t_d)):
                    _lib.tuning_set("cu_reserve", 8 if m is dp else 0)
                    t.append(_time(lambda i, m=m: m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch=br, head_lr=100.0, mm_lr=100.0),
                                   args.steps, args.warmup))
            r[br] = {"plain": _spread(t_p), "dp_one_rank": _spread(t_d)}
        res["results"][f"batch_{B}"] = r
        del plain, dp
        torch.cuda.empty_cache()
    return res


def _aug(args):
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base
    import avsiam_amd
    cfg, L = AVSiamConfig(), 527
    res = {"metric": "ft_aug_step", "label": args.label, "package": os.path.dirname(os.path.abspath(avsiam_amd.__file__)),
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "repetitions": REPS,
           "recipe": {"freqm": 48, "timem": 192, "noise": True, "ftmode": "mm_grad", "n_class": L}, "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        m = CAVMAEFT_BASE(L).cuda()
        apply_freeze_base(m, False)
        ld = SyntheticFtLoader(cfg, B, 1, L, m.arena.p.device)
        kw = dict(head_lr=100.0, mm_lr=100.0)
        r = {}
        for br in ("mm", "a"):
            ways = {"plain": lambda i, br=br: m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch=br, **kw)}
            if not args.plain_only:
                from avsiam_amd import preprocess

                def fused(i, br=br):
                    m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch=br, aug=m.draw_aug(B, 48, 192, True, fill=1.133), **kw)

                def two_pass(i, br=br):
                    m.train_step(preprocess.augment_fbank(ld.a, m.draw_aug(B, 48, 192, True, fill=1.133), raw=False), ld.v, ld.y, 1e-4, "mm_grad",
                                 branch=br, **kw)
                ways.update(fused=fused, two_pass=two_pass)
            t = {k: [] for k in ways}
            for _ in range(REPS):
                for k, fn in ways.items():
                    t[k].append(_time(fn, args.steps, args.warmup))
            r[br] = {k: _spread(x) for k, x in t.items()}
        res["results"][f"batch_{B}"] = r
        del m
        torch.cuda.empty_cache()
    return res


GUARD_ROUNDS = 7
COPY_RATE = 6.29e12          # B/s, the float4-copy rate of the README's other HBM-bound kernels (read + write)


def _med(xs):
    ys = sorted(xs)
    return {"median": round(ys[len(ys) // 2], 4), "min": round(ys[0], 4), "max": round(ys[-1], 4), "rounds": [round(x, 4) for x in xs]}


def _guard(args):
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base
    import avsiam_amd
    cfg, L = AVSiamConfig(), 527
    res = {"metric": "ft_grad_guard", "label": args.label, "package": os.path.dirname(os.path.abspath(avsiam_amd.__file__)),
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rounds": GUARD_ROUNDS, "results": {}}
    kw = dict(head_lr=100.0, mm_lr=100.0)
    for B in [int(b) for b in args.batches.split(",")]:
        plain = CAVMAEFT_BASE(L).cuda()
        apply_freeze_base(plain, False)
        ld = SyntheticFtLoader(cfg, B, 1, L, plain.arena.p.device)
        ways = {"plain_ms": lambda i: plain.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw)}
        if not args.plain_only:
            from avsiam_amd import ops
            from avsiam_amd.models.cav_mae_ft import CLASSES
            g = CAVMAEFT_BASE(L).cuda()
            apply_freeze_base(g, False)
            g.set_grad_guard(1.0)
            g.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw)          # builds the table; a mm step's gradients in the arena
            a, st = g.arena, g._dps
            lo0, hi0 = a.range[1]
            table, ctl, guard = st["table"], st["ctl"], g._guard
            mom = (g._opt["m"], g._opt["v"])
            live = ctl.live.cpu().tolist()
            n_live = int(sum(n for _, n, _, c in table.segs if live[c] > 0))

            def refresh():
                a.refresh_shadows(None, cast=False)
                for e in list(g._engines.values()) + list(g._train_engines.values()):
                    e.refresh_heads()

            def adam_plain(i):
                ctl.set_lr(1e-4, 1e-2, 1e-2)
                ops.adam_table(a.p[lo0:hi0], a.g[lo0:hi0], *mom, a.pb[lo0:hi0], table, ctl)
                refresh()

            def adam_guarded(i):
                ctl.set_lr(1e-4, 1e-2, 1e-2)
                ops.grad_sumsq(a.g[lo0:hi0], table, ctl, guard, max_norm=1.0)
                ops.adam_table_guarded(a.p[lo0:hi0], a.g[lo0:hi0], *mom, a.pb[lo0:hi0], table, ctl, guard)
                refresh()

            ways.update(guarded_ms=lambda i: g.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw),
                        grad_sumsq_ms=lambda i: ops.grad_sumsq(a.g[lo0:hi0], table, ctl, guard, max_norm=1.0),
                        adam_phase_plain_ms=adam_plain, adam_phase_guarded_ms=adam_guarded)
        t = {k: [] for k in ways}
        for _ in range(GUARD_ROUNDS):
            for k, fn in ways.items():
                mult = 20 if k == "grad_sumsq_ms" else 1             # (two short launches: a window of 20 x steps calls, not of a millisecond)
                t[k].append(_time(fn, args.steps * mult, args.warmup))
        r = {k: _med(x) for k, x in t.items()}
        if not args.plain_only:
            us = r["grad_sumsq_ms"]["median"] * 1e3
            r["grad_sumsq"] = {"elements_live": n_live, "table_segments": len(table.segs), "chunks": table.chunks, "median_us": round(us, 2),
                               "floor_us_derived": round(4.0 * n_live / COPY_RATE * 1e6, 2),
                               "fraction_of_copy_rate": round(4.0 * n_live / (us * 1e-6) / COPY_RATE, 4),
                               "live_classes": [c for i, c in enumerate(CLASSES) if live[i] > 0]}
            r["guard_stats"] = g.guard_stats()
            del g
        res["results"][f"batch_{B}"] = r
        del plain
        torch.cuda.empty_cache()
    return res


def _accum(args):
    """(a) avs_grad_accum alone, copy form and add form, on the table of the mm step and on the table with only the v branch's classes live,
    against the float4-copy rate on 8 B (copy) / 12 B (add) per element; (b) the composition one would otherwise write: one dense
    acc.add_(g) over the whole trainable range plus the acc.zero_() a cycle needs; (c) k = 4 micro-steps of batch 16 against four plain
    steps of batch 16, mm and the 50/25/25 mix.  --plain-only: the plain mm step alone (batches from --batches), for the parent comparison."""
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, apply_freeze_base, draw_branch
    import avsiam_amd
    cfg, L = AVSiamConfig(), 527
    kw = dict(head_lr=100.0, mm_lr=100.0)
    res = {"metric": "ft_grad_accum", "label": args.label, "package": os.path.dirname(os.path.abspath(avsiam_amd.__file__)),
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rounds": GUARD_ROUNDS, "results": {}}
    if args.plain_only:
        for B in [int(b) for b in args.batches.split(",")]:
            plain = CAVMAEFT_BASE(L).cuda()
            apply_freeze_base(plain, False)
            ld = SyntheticFtLoader(cfg, B, 1, L, plain.arena.p.device)
            t = [_time(lambda i: plain.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw), args.steps, args.warmup)
                 for _ in range(GUARD_ROUNDS)]
            res["results"][f"batch_{B}"] = {"plain_ms": _med(t)}
            del plain
            torch.cuda.empty_cache()
        return res
    from avsiam_amd import ops
    from avsiam_amd.models.cav_mae_ft import CLASSES, live_classes
    from avsiam_amd.ft_train import OUT, OUT_V
    K, B = 4, 16
    m = CAVMAEFT_BASE(L).cuda()
    apply_freeze_base(m, False)
    ld = SyntheticFtLoader(cfg, B, 1, L, m.arena.p.device)
    m.set_grad_accumulation(K)
    m.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch="mm", **kw)                  # builds the table; a mm step's gradients in the arena
    a, st = m.arena, m._dps
    lo0, hi0 = a.range[1]
    table, g = st["table"], a.g[lo0:hi0]
    acc = torch.zeros(hi0 - lo0, device=g.device)
    actl = ops.GradAccumCtl(g.device)
    ctls, n_live = {}, {}
    for name, reach in (("mm", live_classes("mm_grad", OUT)), ("v", live_classes("videoonly", OUT_V))):
        ctls[name] = ops.AdamCtl(g.device)
        ctls[name].live[:len(CLASSES)] = torch.tensor([1.0 if c in reach else 0.0 for c in CLASSES])
        n_live[name] = int(sum(n for _, n, _, c in table.segs if CLASSES[c] in reach))
    for name in ("mm", "v"):                                            # every class touched once, so that the add form adds
        ops.grad_accum(acc, g, table, ctls[name], actl, name == "mm", False)
    ways = {}
    for name in ("mm", "v"):
        ways[f"kernel_copy_{name}"] = lambda i, c=ctls[name]: ops.grad_accum(acc, g, table, c, actl, True, False)
        ways[f"kernel_add_{name}"] = lambda i, c=ctls[name]: ops.grad_accum(acc, g, table, c, actl, False, False)
    ways["dense_add"] = lambda i: acc.add_(g)
    ways["dense_zero"] = lambda i: acc.zero_()
    t = {k: [] for k in ways}
    for _ in range(GUARD_ROUNDS):
        for k, fn in ways.items():
            t[k].append(_time(fn, args.steps * 20, args.warmup))         # (short launches: a window of 20 x steps calls)
    r = {k: _med(x) for k, x in t.items()}
    n_all = hi0 - lo0
    for name in ("mm", "v"):
        for form, nbytes in (("copy", 8.0), ("add", 12.0)):
            us = r[f"kernel_{form}_{name}"]["median"] * 1e3
            r[f"kernel_{form}_{name}"].update(elements_live=n_live[name], median_us=round(us, 2),
                                               floor_us_derived=round(nbytes * n_live[name] / COPY_RATE * 1e6, 2),
                                               fraction_of_copy_rate=round(nbytes * n_live[name] / (us * 1e-6) / COPY_RATE, 4))
    add_us, zero_us = r["dense_add"]["median"] * 1e3, r["dense_zero"]["median"] * 1e3
    r["dense_add"].update(elements=n_all, median_us=round(add_us, 2), fraction_of_copy_rate=round(12.0 * n_all / (add_us * 1e-6) / COPY_RATE, 4))
    r["dense_zero"].update(elements=n_all, median_us=round(zero_us, 2))
    # per micro-step of a cycle of K: the kernel does one copy and K - 1 adds; the composition one zero-fill and K dense adds
    for name in ("mm", "v"):
        kern = (r[f"kernel_copy_{name}"]["median"] + (K - 1) * r[f"kernel_add_{name}"]["median"]) / K * 1e3
        dense = (zero_us + K * add_us) / K
        r[f"per_micro_step_us_{name}"] = {"kernel": round(kern, 2), "dense_add_plus_zero": round(dense, 2), "kernel_over_dense": round(kern / dense, 4)}
    r["table"] = {"segments": len(table.segs), "chunks": table.chunks, "trainable_elements": n_all}
    res["results"]["kernel"] = r
    # (c) whole steps: k = 4 micro-steps of batch 16 against four plain steps of batch 16
    m.apply_accumulated(1e-4, **kw)
    plain = CAVMAEFT_BASE(L).cuda()
    apply_freeze_base(plain, False)
    rng = random.Random(0)
    n_calls = K * (args.steps + args.warmup)
    mix = [draw_branch(rng.uniform(0, 1)) for _ in range(n_calls)]
    step_ways = {}
    for sched, br in (("mm", lambda j: "mm"), ("mix_50_25_25", lambda j: mix[j % n_calls])):
        for label, mod in (("plain", plain), ("accum", m)):
            def cycle(i, mod=mod, br=br):
                for j in range(K):
                    mod.train_step(ld.a, ld.v, ld.y, 1e-4, "mm_grad", branch=br(i * K + j), **kw)
            step_ways[f"{sched}.{label}"] = cycle
    t = {k: [] for k in step_ways}
    for _ in range(GUARD_ROUNDS):
        for k, fn in step_ways.items():
            t[k].append(_time(fn, args.steps, args.warmup) / K)          # ms per (micro-)step
    s = {k: _med(x) for k, x in t.items()}
    for sched in ("mm", "mix_50_25_25"):
        p_ms, a_ms = s[f"{sched}.plain"]["median"], s[f"{sched}.accum"]["median"]
        s[f"{sched}.summary"] = {"plain_ms_per_step": p_ms, "accum_ms_per_micro_step": a_ms, "saved_ms_per_micro_step": round(p_ms - a_ms, 4),
                                 "samples_per_s_plain": round(B * 1e3 / p_ms, 2), "samples_per_s_accum": round(B * 1e3 / a_ms, 2)}
    res["results"][f"k{K}_batch_{B}"] = s
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=str, default="8,64")
    ap.add_argument("--adam-table", dest="adam_table", action="store_true")
    ap.add_argument("--dp-one-rank", dest="dp_one_rank", action="store_true")
    ap.add_argument("--aug", action="store_true", help="the mm / a steps plain, with the fused augmentation and with the two-pass one")
    ap.add_argument("--guard", action="store_true", help="grad_sumsq alone, the Adam phase and the mm step guarded against plain")
    ap.add_argument("--accum", action="store_true", help="avs_grad_accum alone, against a dense add_ + zero_, and k = 4 micro-steps against plain steps")
    ap.add_argument("--plain-only", dest="plain_only", action="store_true", help="with --aug / --guard / --accum: time the plain step only")
    ap.add_argument("--tree", type=str, default=None, help="with --aug / --guard / --accum and --plain-only: import avsiam_amd from this checkout")
    ap.add_argument("--label", type=str, default=None, help="copied into the result")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON result to this file")
    args = ap.parse_args(argv)
    if args.tree:
        if not ((args.aug or args.guard or args.accum) and args.plain_only):
            ap.error("--tree goes with --aug --plain-only, --guard --plain-only or --accum --plain-only")
        sys.path.insert(0, os.path.abspath(args.tree))
    if args.adam_table or args.dp_one_rank or args.aug or args.guard or args.accum:
        res = (_adam_table if args.adam_table else _dp_one_rank if args.dp_one_rank else _aug if args.aug else _guard if args.guard else _accum)(args)
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return res
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
