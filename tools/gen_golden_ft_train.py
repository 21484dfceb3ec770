"""Golden vectors of the fine-tuned model's TRAINING forms: runs the UNMODIFIED reference ``CAVMAEFT_BASE`` on CPU in fp32 - the
training forward (cav_mae_base.py:827-866,983-1035), the loss of traintest_ft_base.py:105-110,153-160 and ``.backward()``.

    python tools/gen_golden_ft_train.py      # writes tests/golden/ftt_*.npz (needs the reference checkout; oracle/ref_import.py)

Stored (data only): the case, the input seed, the labels, the loss, the logits of every output, and per-parameter gradient statistics
{sum, L2, 8 sampled elements} plus the names of the parameters whose .grad stays None (oracle/gen_golden.py::grad_stats).  Weights are
re-synthesised from (seed, name) by avsiam_amd.weights, as for the inference goldens (oracle/gen_golden_ft.py).
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avsiam_amd.config import AVSiamConfig                      # noqa: E402
from avsiam_amd.param_spec import alias_of, state_dict_keys_ft  # noqa: E402
from avsiam_amd.weights import synth_state_ft                   # noqa: E402
from oracle import ref_import                                   # noqa: E402
from oracle.gen_golden import grad_stats                        # noqa: E402
from oracle.gen_golden_ft import ft_inputs                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 4321
INPUT_SEED = 91

#        name                mode         L    B  T  loss   target          freeze_base
CASES = [("ftt_mm_out",      "mm_grad",   527, 2, 1, "BCE", "out",          False),
         ("ftt_mm_a",        "mm_grad",   527, 2, 1, "BCE", "out_a",        False),
         ("ftt_mm_v",        "mm_grad",   527, 2, 1, "BCE", "out_v",        False),
         ("ftt_mm_sum",      "mm_grad",   527, 2, 1, "BCE", "sum",          False),
         ("ftt_mm_freeze",   "mm_grad",   527, 2, 1, "BCE", "out",          True),
         ("ftt_audio_ce",    "audioonly", 309, 3, 1, "CE",  "out",          False),
         ("ftt_video",       "videoonly", 527, 2, 1, "BCE", "out",          False)]


def labels(B, L, seed):
    """label-smoothed multi-hot targets (the loader's label_smooth 0.1: 0.9 + 0.1 / L on the positives, 0.1 / L elsewhere)"""
    g = torch.Generator().manual_seed(seed)
    hot = (torch.rand(B, L, generator=g) < 0.03).float()
    hot[:, 0] = 1.0
    return hot * 0.9 + 0.1 / L


def loss_of(outs, y, loss, target):
    fn = F.binary_cross_entropy_with_logits if loss == "BCE" else F.cross_entropy
    if target == "sum":
        return sum(fn(o, y) for o in outs.values())
    return fn(outs[target], y)


def is_base(name):
    """traintest_ft_base.py:47-57: neither 'mlp_head' nor 'mm_layer' in the name"""
    return "mlp_head" not in name and "mm_layer" not in name


def main():
    if not ref_import.reference_available():
        print("reference not present - nothing to generate")
        return
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg = AVSiamConfig()
    models = {}
    for name, mode, L, B, T, loss, target, freeze in CASES:
        if L not in models:
            m = ref_import.build_reference_ft_model(L)
            st = synth_state_ft(cfg, L, WEIGHT_SEED, "random")
            m.load_state_dict({k: st[alias_of(k)] for k in state_dict_keys_ft(cfg, L)}, strict=True)
            m.eval()                                               # (dropout layers, if any, off: the oracle has none)
            models[L] = m
        m = models[L]
        for n, p in m.named_parameters():
            p.requires_grad_(not (freeze and is_base(n)))
            p.grad = None
        a, v = ft_inputs(cfg, B, T, INPUT_SEED)
        y = labels(B, L, INPUT_SEED + L)
        if mode == "audioonly":
            v = None
        elif mode == "videoonly":
            a = None
        out = m(a, v, mode)
        outs = dict(zip(("out", "out_a", "out_v"), out)) if isinstance(out, tuple) else {"out": out}
        lo = loss_of(outs, y, loss, target)
        lo.backward()
        d = {"mode": np.array(mode), "label_dim": np.array(L), "batch": np.array(B), "frames": np.array(T), "loss_kind": np.array(loss),
             "target": np.array(target), "freeze_base": np.array(freeze), "input_seed": np.array(INPUT_SEED),
             "weight_seed": np.array(WEIGHT_SEED), "labels": y.numpy().astype(np.float32), "loss": np.array(lo.item())}
        for k, o in outs.items():
            d["logits_" + k] = o.detach().numpy().astype(np.float32)
        d.update(grad_stats([(n, p.grad) for n, p in m.named_parameters()]))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **d)
        print(name, mode, "loss", lo.item(), "live", len(json.loads(str(d["grad_names"]))), "none", len(json.loads(str(d["grad_none"]))), flush=True)


if __name__ == "__main__":
    main()
