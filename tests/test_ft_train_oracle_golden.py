"""The oracle's fine-tuning BACKWARD against the unmodified reference (CPU): autograd through oracle/ref_cpu.ft_forward plus torch's BCE /
CE reproduces every tests/golden/ftt_*.npz (tools/gen_golden_ft_train.py) - the loss, the logits of every output, the set of parameters
that get a gradient, and each gradient's L2 norm and 8 sampled elements.  This pins the oracle the GPU tests compare against."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs, synth_state_ft
from oracle import ref_cpu
from tests.helpers import check_grads_against_golden, load_golden

FTT_CASES = ["ftt_mm_out", "ftt_mm_a", "ftt_mm_v", "ftt_mm_sum", "ftt_mm_freeze", "ftt_audio_ce", "ftt_video"]


def ftt_inputs(d, cfg):
    """inputs of a training golden case (tools/gen_golden_ft_train.py: oracle/gen_golden_ft.py::ft_inputs, then the mode's unused input
    dropped)"""
    B, T = int(d["batch"]), int(d["frames"])
    a, v = synth_inputs(dataclasses.replace(cfg, frames=T), B, int(d["input_seed"]))
    v = v.unsqueeze(1) if T == 1 else v
    mode = str(d["mode"])
    return (None if mode == "videoonly" else a), (None if mode == "audioonly" else v)


def ftt_loss(d, outs, y):
    """outs: {"out", "out_a", "out_v"} -> the case's loss (traintest_ft_base.py:105-110,153-160, or the sum of the three)"""
    fn = F.binary_cross_entropy_with_logits if str(d["loss_kind"]) == "BCE" else F.cross_entropy
    if str(d["target"]) == "sum":
        return sum(fn(o, y) for o in outs.values())
    return fn(outs[str(d["target"])], y)


def is_base(name):
    return "mlp_head" not in name and "mm_layer" not in name


@pytest.mark.parametrize("name", FTT_CASES)
def test_oracle_backward_matches_reference_golden(name):
    torch.set_num_threads(8)
    d = load_golden(name)
    cfg = AVSiamConfig()
    L = int(d["label_dim"])
    a, v = ftt_inputs(d, cfg)
    y = torch.from_numpy(d["labels"])
    freeze = bool(d["freeze_base"])
    P = {k: t.clone().requires_grad_(not (freeze and is_base(k))) for k, t in synth_state_ft(cfg, L, int(d["weight_seed"]), "random").items()}
    out = ref_cpu.ft_forward(P, cfg, a, v, str(d["mode"]))
    outs = dict(zip(("out", "out_a", "out_v"), out)) if isinstance(out, tuple) else {"out": out}
    loss = ftt_loss(d, outs, y)
    loss.backward()
    assert abs(loss.item() - float(d["loss"])) <= 1e-5 * abs(float(d["loss"])) + 1e-6, (loss.item(), float(d["loss"]))
    for k, o in outs.items():
        np.testing.assert_allclose(o.detach().numpy(), d["logits_" + k], rtol=1e-4, atol=1e-4)
    check_grads_against_golden(d, {k: p.grad for k, p in P.items()}, rel_l2=1e-4)
