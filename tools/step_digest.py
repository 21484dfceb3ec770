"""Digest of a few training steps, for checking that a host-side refactor leaves the computation and the launch sequence alone: run it on
the commit before and on the commit after, compare the JSON lines.

    python tools/step_digest.py --opts '{"fp8": "3", "deterministic": true}' --batch 5 --steps 3
    python tools/step_digest.py --opts '{"wgrad_stream": "1"}' --batch 8 --steps 3 --trace
    python tools/step_digest.py --ft --batch 2

CAVMAE_BASE at AVSiamConfig(audio_tokens=128, frames=2), random init, fixed seeds, device-drawn mask plans (the set-up of
tests/test_train_gpu.py::test_deterministic_mode_gives_bit_identical_steps), `--steps` calls of train_step.  One JSON line: the losses of every
step, sha256 of the parameter arena, the gradient arena and the two Adam moments, torch.cuda.max_memory_allocated() and the library calls per step.
Bitwise comparable between two runs only with "deterministic": true.  --trace: also the number and the sha256 of the list of library calls - entry
point, scalar arguments, (dtype, shape) of tensor arguments, whether the side stream is current - which two runs share in every mode.
--ft: one fused mm_grad step of CAVMAEFT_BASE (single frame, deterministic) instead."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from avsiam_amd import _lib  # noqa: E402
from avsiam_amd.config import AVSiamConfig, EngineOptions  # noqa: E402
from avsiam_amd.weights import synth_inputs  # noqa: E402


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def trace_calls(log):
    """wrap _lib.call: every library call is appended to `log` in a form that does not depend on addresses"""
    inner, main = _lib.call, _lib.current_stream()

    def describe(a, stream):
        if hasattr(a, "data_ptr"):
            return [str(a.dtype), list(a.shape)]
        if isinstance(a, bool) or a is None:
            return a
        if isinstance(a, int):
            return "stream" if a == stream and a != 0 else "ptr" if abs(a) >= 1 << 40 else a        # (an address differs from run to run)
        return a if isinstance(a, (float, str)) else type(a).__name__

    def call(name, *args):
        stream = _lib.current_stream()
        log.append([name, stream != main, [describe(a, stream) for a in args]])
        return inner(name, *args)
    _lib.call = call


def pretrain(args, opts):
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.param_spec import P1, P2
    from avsiam_amd.traintest_cavmae_base import train_step
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    a, v = (t.cuda() for t in synth_inputs(cfg, args.batch, 17))
    m = CAVMAE_BASE(cfg=cfg, init_seed=4, init_mode="random", verbose=False, plan_seed=33, options=opts, share_pass_buffers=args.share_pass_buffers).cuda()
    m.publish_grads = False
    losses, per_step = [], []
    for _ in range(args.steps):
        c0 = _lib.calls
        losses.append([float(x.item()) for x in train_step(m, a, v, 2e-4)])
        per_step.append(_lib.calls - c0)
    torch.cuda.synchronize()
    st = [m._opt_state[w] for w in (P1, P2)]
    pool = {"pool_used": m._pool.used(), "pool_nbytes": m._pool.nbytes()} if m._pool is not None else {}
    return {"losses": losses, "calls_per_step": per_step, "p": sha(m.arena.p), "g": sha(m.arena.g), "adam_m": sha(*(s["m"] for s in st)),
            "adam_v": sha(*(s["v"] for s in st)), **pool}


def finetune(args):
    from avsiam_amd.models import CAVMAEFT_BASE
    cfg, L, B = AVSiamConfig(), 527, args.batch
    a, v = synth_inputs(cfg, B, 51)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    hot = (torch.rand(B, L, generator=torch.Generator().manual_seed(11)) < 0.03).float()
    y = (hot * 0.9 + 0.1 / L).cuda()
    m = CAVMAEFT_BASE(L, init_seed=5, init_mode="random").cuda()
    m.requires_grad_(True)
    m._train_engine(B, 1).opts.deterministic = True          # (a runtime option: the engine and its stacks read it on every backward)
    _lib.tuning_set("det", 1)
    c0 = _lib.calls
    loss = float(m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm"))
    torch.cuda.synchronize()
    _lib.tuning_set("det", 0)
    return {"losses": [loss], "calls_per_step": [_lib.calls - c0], "p": sha(m.arena.p), "g": sha(m.arena.g), "adam_m": sha(m._opt["m"]),
            "adam_v": sha(m._opt["v"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--opts", default="{}", help="EngineOptions fields as a JSON object")
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--share-pass-buffers", action="store_true", help="CAVMAE_BASE(share_pass_buffers=True): one activation pool for both passes")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-out", metavar="FILE", help="with --trace: write the list of calls there, one per line (to diff two runs)")
    ap.add_argument("--ft", action="store_true")
    ap.add_argument("--label", default=None, help="copied into the result line")
    args = ap.parse_args()
    spec = json.loads(args.opts)
    _lib.load()
    torch.cuda.init()
    log = []
    if args.trace:
        trace_calls(log)
    res = finetune(args) if args.ft else pretrain(args, EngineOptions(**spec).validated())
    res = {"label": args.label, "what": "ft" if args.ft else "pretrain", "opts": spec, "share_pass_buffers": args.share_pass_buffers, "batch": args.batch, "steps": 1 if args.ft else args.steps, **res,
           "max_memory_allocated": torch.cuda.max_memory_allocated()}
    if args.trace:
        res["trace_calls"] = len(log)
        res["trace"] = hashlib.sha256(json.dumps(log).encode()).hexdigest()
        if args.trace_out:
            with open(args.trace_out, "w") as f:
                f.writelines(json.dumps(c) + "\n" for c in log)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
