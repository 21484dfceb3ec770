"""Host-side logic of fine-tuning (no GPU): the reference's branch draw and parameter groups, which tensors can get a gradient, the CLI,
and the C-ABI entries the fine-tuning path adds."""
import ctypes

import pytest
import torch

from avsiam_amd import _lib
from avsiam_amd.config import AVSiamConfig


def test_branch_draw_thresholds():
    """traintest_ft_base.py:153-160: prob > 0.5 -> out, prob < 0.25 -> out_a, otherwise out_v (0.25 and 0.5 themselves -> out_v)"""
    from avsiam_amd.traintest_ft_base import draw_branch
    assert [draw_branch(p) for p in (0.0, 0.2499, 0.25, 0.4, 0.5, 0.5001, 1.0)] == ["a", "a", "v", "v", "v", "mm", "mm"]


def test_parameter_groups_follow_the_reference_name_rule():
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.models.cav_mae_ft import grad_class, live_classes, param_group
    from avsiam_amd.ft_train import OUT, OUT_A, OUT_V
    m = CAVMAEFT_BASE(527)
    groups = {}
    for n, _ in m.named_parameters():
        groups.setdefault(param_group(n), []).append(n)
    assert all("mlp_head" in n for n in groups["head"]) and all("mm_layer" in n for n in groups["mm"])
    assert "mlp_head_mm_v2.1.weight" in groups["head"]
    assert "my_patch_embed.proj.weight" in groups["base"] and "my_patch_embed_a.proj.bias" in groups["base"]
    assert len(groups["head"]) == 16 and len(groups["mm"]) == 2 * 20
    # mm_v2 and my_patch_embed* are read by no mode: no backward can reach them
    spec = m.arena.info
    every = live_classes("mm_grad", OUT | OUT_A | OUT_V) | live_classes("audioonly", 1) | live_classes("videoonly", 1)
    for n in ("mlp_head_mm_v2.1.weight", "my_patch_embed.proj.weight", "my_patch_embed_a.proj.weight", "vit_base.cls_token"):
        assert spec[n].live == 0 or grad_class(n) not in every, n
    # out_a reaches the audio side, the shared blocks and its own head only (cav_mae_base.py:1019)
    cls_a = live_classes("mm_grad", OUT_A)
    assert grad_class("vit_base.blocks.3.norm1_a.weight") in cls_a and grad_class("vit_base.blocks.3.attn.qkv.weight") in cls_a
    assert grad_class("vit_base.blocks.3.norm1_v.weight") not in cls_a and grad_class("vit_base.patch_embed.proj.weight") not in cls_a
    assert grad_class("mlp_head_a.1.weight") in cls_a and grad_class("mlp_head.1.weight") not in cls_a
    assert grad_class("mm_layer_1.attn.qkv.weight") not in cls_a
    assert grad_class("vit_base.norm.weight") == "base_v" and grad_class("vit_base.norm_a.weight") == "base_a"
    assert grad_class("vit_base.pos_embed") == "base_v" and grad_class("vit_base.pos_embed_a") == "base_a"


def test_inference_model_allocates_no_training_buffers():
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(10)
    assert not m.arena.with_grads and m.arena.t_total == 0
    assert all(not p.requires_grad for p in m.parameters())


def test_pretraining_checkpoint_loads_with_the_reference_key_lists():
    """run_cavmae_ft_base.py:243-249: the missing / unexpected lists of a strict=False load equal the difference of the two key schemas"""
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.param_spec import state_dict_keys, state_dict_keys_ft
    cfg = AVSiamConfig()
    m = CAVMAEFT_BASE(527)
    pt_keys = state_dict_keys(cfg)
    ft_keys = state_dict_keys_ft(cfg, 527)
    shapes = {k: v.shape for k, v in m.state_dict().items()}
    from avsiam_amd.weights import synth_state
    src = synth_state(cfg, 3, "random")
    from avsiam_amd.param_spec import alias_of
    sd = {"module." + k: src[alias_of(k)] for k in pt_keys if alias_of(k) in src}
    for k in pt_keys:
        if "module." + k not in sd:
            sd["module." + k] = torch.zeros(shapes.get(k, (1,)))
    miss, unexpected = m.load_state_dict(sd, strict=False)
    assert sorted(miss) == sorted(k for k in ft_keys if k not in set(pt_keys))
    assert sorted(unexpected) == sorted(k for k in pt_keys if k not in set(ft_keys))
    assert "mm_layer_1.attn.qkv.weight" not in miss                     # the fusion blocks come from the checkpoint
    assert torch.equal(m.state_dict()["mm_layer_2.mlp.fc1.weight"], src["mm_layer_2.mlp.fc1.weight"])


def test_cli_parses_the_launcher_flags():
    from avsiam_amd.run_cavmae_ft_base import build_parser
    a = build_parser().parse_args(["--model", "cav-mae-ft", "--ftmode", "mm_grad", "--n_class", "527", "--lr", "1e-4", "--head_lr", "100",
                                   "--mm_lr", "100", "--batch_size", "8", "--freeze_base", "False", "--loss", "BCE", "--wa", "True",
                                   "--lr_adapt", "False", "--lrscheduler_start", "2", "--lrscheduler_decay", "0.75", "--n-print-steps", "100",
                                   "--pretrain_path", "x.pth", "--skip_frame_agg", "False", "--dis_w", "0.0"])
    assert (a.ftmode, a.n_class, a.lr, a.head_lr, a.mm_lr, a.batch_size, a.freeze_base, a.loss) == ("mm_grad", 527, 1e-4, 100.0, 100.0, 8, False, "BCE")
    assert a.lrscheduler_decay == 0.75 and a.n_print_steps == 100 and a.pretrain_path == "x.pth"


def test_cli_refuses_data_parallel():
    from avsiam_amd.run_cavmae_ft_base import main
    with pytest.raises(SystemExit, match="data-parallel"):
        main(["--world_size", "2", "--ftmode", "mm_grad"])


def test_metrics_match_definitions():
    import numpy as np
    from avsiam_amd.traintest_ft_base import calculate_stats
    y = np.array([[1, 0], [0, 1], [1, 0], [0, 1]], dtype=float)
    s = np.array([[0.9, 0.2], [0.8, 0.7], [0.3, 0.1], [0.2, 0.9]])
    st = calculate_stats(s, y)
    assert st[0]["AP"] == pytest.approx((1 + 2 / 3) / 2) and st[0]["auc"] == pytest.approx(0.75)
    assert st[1]["AP"] == pytest.approx(1.0) and st[1]["auc"] == pytest.approx(1.0)
    assert st[0]["acc"] == pytest.approx(0.75)          # argmax hits on rows 0, 2, 3


@pytest.fixture(scope="module")
def lib_path():
    from avsiam_amd.build import build
    return build(verbose=False)


def test_fine_tuning_abi_entries(lib_path):
    """avs_cls_loss and avs_segment_mean_bwd_acc are exported and declared; the additions keep ABI version 2 (nothing existing changed);
    argument validation precedes any launch, so it is testable without a GPU."""
    protos = _lib.parse_header()
    lib = ctypes.CDLL(lib_path)
    for name in ("avs_cls_loss", "avs_segment_mean_bwd_acc"):
        assert name in protos and hasattr(lib, name)
    lib = _lib.load()
    assert lib.avs_abi_version() == 2
    one = ctypes.c_void_p(16)
    assert lib.avs_cls_loss(one, 527, one, 527, 4, 527, 2, None, 1.0, one, one, None, 0, None) == -2          # unknown kind
    assert lib.avs_cls_loss(one, 100, one, 527, 4, 527, 0, None, 1.0, one, one, None, 0, None) == -2          # ldx < L
    assert b"cls_loss" in lib.avs_last_error()
    assert lib.avs_segment_mean_bwd_acc(one, one, one, 3, 770, 1.0, None, 1, None) == -2                      # D % 4
    # layernorm_bwd accepts the head widths now, but not the fp8 copy / column sum there
    rc = lib.avs_layernorm_bwd(one, 1, one, one, one, one, None, None, None, None, 0, one, None, one, one, None, None, one, one, 4, 1536,
                               None, None, None)
    assert rc == -2 and b"classifier head" in lib.avs_last_error()
    rc = lib.avs_layernorm_bwd(one, 1, one, one, one, one, None, None, None, None, 0, one, None, one, one, None, None, None, one, 4, 1792,
                               None, None, None)
    assert rc == -2 and b"unsupported" in lib.avs_last_error()
