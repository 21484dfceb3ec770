"""Fine-tuning CAVMAEFT_BASE on a real MI355X: the classification-loss kernel, LayerNorm backward at the classifier-head widths and the
accumulating token-mean backward against torch in fp64; the hand-scheduled backward of every trainable mode against autograd through the
CPU oracle (oracle/ref_cpu.ft_forward, fp32); the fused train_step against the autograd path; the HIP Adam of the three parameter groups
against torch.optim.Adam; a short training run that must lower the loss; and the inference path left as it was.

Gradient tolerance (bf16 GEMM / attention operands with fp32 accumulation against the fp32 reference): every tensor that gets a gradient
has cosine >= GRAD_COS with the reference gradient and its norm within GRAD_NORM; the measured margins go to parity_margins.json."""
import math

import numpy as np

import pytest
import torch
import torch.nn.functional as F

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs, synth_state_ft
from tests.helpers import gpu_grads_vs_golden, record_margin

pytestmark = pytest.mark.gpu

GRAD_COS, GRAD_NORM, LOSS_TOL = 0.9998, 1e-2, 2e-3      # loss: |error| <= LOSS_TOL * max(1, |loss|) (random weights give CE losses ~60)
FUSED_COS = 0.9999          # fused train_step vs the autograd path of the same model (same kernels, other row packing)


def _lib_ops():
    from avsiam_amd import ops
    return ops


# ---- 1. classification loss kernel -------------------------------------------------------------------------------------
def _cls_inputs(n, L, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, L, generator=g, dtype=torch.float64) * 20
    x[0, 0] = 100.0
    x[-1, -1] = -100.0
    x = x.clamp(-100, 100)
    hot = (torch.rand(n, L, generator=g) < 0.05).double()
    y = hot * 0.9 + 0.1 / L                                     # label-smoothed multi-hot, as the reference's loader (dataloader.py)
    if kind == 1:
        y = y / y.sum(dim=1, keepdim=True) * 1.3                # soft targets that do not sum to one: the sum(y) term is exercised
    return x, y


def _cls_ref(x, y, kind):
    x = x.clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(x, y) if kind == 0 else F.cross_entropy(x, y)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("L", [1, 309, 527])
@pytest.mark.parametrize("n", [1, 7, 64])
def test_cls_loss_kernel_matches_torch_fp64(kind, L, n):
    ops = _lib_ops()
    x, y = _cls_inputs(n, L, kind, 10 * n + L + kind)
    ref_l, ref_g = _cls_ref(x, y, kind)
    npad = ops.pad_rows(L, 128)
    xb = torch.zeros(n, npad, device="cuda")
    xb[:, :L] = x.float().cuda()                               # a column range of a padded buffer, as the head's output
    yd = y.float().cuda().contiguous()
    rows, loss = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    dx = torch.full((n, npad), 7.0, device="cuda")
    gout = torch.tensor([1.0], device="cuda")
    runs = []
    for _ in range(2):
        ops.cls_loss(xb[:, :L], yd, n, L, kind, rows, loss, dx=dx, gout=gout)
        runs.append((loss.clone(), dx.clone()))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    got_l, got_g = runs[0][0].double().cpu()[0], runs[0][1][:, :L].double().cpu()
    assert torch.all(runs[0][1][:, L:] == 7.0), "wrote beyond L"
    scale = max(abs(float(ref_l)), 1e-30)
    assert abs(float(got_l) - float(ref_l)) <= 1e-5 * scale + 1e-7, (float(got_l), float(ref_l))
    gs = float(ref_g.abs().max())
    assert float((got_g - ref_g).abs().max()) <= 1e-5 * gs + 1e-12, float((got_g - ref_g).abs().max() / max(gs, 1e-30))


# ---- 2. LayerNorm backward at the classifier-head widths ---------------------------------------------------------------
@pytest.mark.parametrize("D", [1536, 2048, 2560])
def test_layernorm_bwd_head_widths(D):
    ops = _lib_ops()
    n = 7
    g = torch.Generator().manual_seed(D)
    x = torch.randn(n, D, generator=g, dtype=torch.float64) * 2 + 0.5
    w = 1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    dy = torch.randn(n, D, generator=g, dtype=torch.float64)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xr, (D,), wr, br, eps=1e-6).backward(dy)
    xd, wd, bd = x.float().cuda(), w.float().cuda(), b.float().cuda()
    y, mean, rstd = torch.zeros(n, D, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ops.layernorm_fwd(xd, wd, bd, y, mean, rstd, n, 1e-6)
    dx = torch.zeros(n, D, device="cuda")
    dg, db = torch.full((D,), 0.5, device="cuda"), torch.zeros(D, device="cuda")
    ws = torch.zeros(ops.layernorm_ws(n, D), device="cuda")
    ops.layernorm_bwd(dy.float().cuda(), xd, mean, rstd, wd, dx, dg, db, ws, n)
    torch.cuda.synchronize()
    for got, ref, what in ((dx, xr.grad, "dx"), (dg - 0.5, wr.grad, "dgamma (accumulated)"), (db, br.grad, "dbeta")):
        err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        assert err <= 2e-5, (what, D, err)


def test_segment_mean_bwd_accumulates():
    ops = _lib_ops()
    D, seg = 768, [0, 5, 12, 20]
    dreps = torch.randn(3, D, device="cuda")
    base = torch.randn(20, D, device="cuda")
    out = base.clone()
    rmap = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    s = torch.tensor(seg, dtype=torch.int32, device="cuda")
    ops.segment_mean_bwd_acc(dreps, s, out, 3, 2.0, row_map=rmap, max_row=3)
    ref = base.clone()
    for i in range(3):
        ref[seg[i]:seg[i + 1]] += 2.0 * dreps[int(rmap[i])] / (seg[i + 1] - seg[i])
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)
    ops.segment_mean_bwd_acc(dreps, s, out, 3, 1.0, accumulate=False)
    ref2 = torch.cat([dreps[i:i + 1].expand(seg[i + 1] - seg[i], D) / (seg[i + 1] - seg[i]) for i in range(3)])
    torch.testing.assert_close(out, ref2, rtol=1e-6, atol=1e-6)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _labels(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    hot = (torch.rand(B, L, generator=g) < 0.03).float()
    hot[:, 0] = 1.0
    return hot * 0.9 + 0.1 / L


def _model(L, seed, mode="random"):
    from avsiam_amd.models import CAVMAEFT_BASE
    return CAVMAEFT_BASE(L, init_seed=seed, init_mode=mode).cuda()


def _oracle_grads(P, cfg, a, v, fn):
    """autograd through the CPU oracle: fn(outputs) -> loss; -> (loss, {name: grad or None})"""
    from oracle import ref_cpu
    torch.set_num_threads(16)
    leaf = {k: t.clone().requires_grad_(True) for k, t in P.items()}
    loss = fn(ref_cpu.ft_forward(leaf, cfg, a, v, fn.mode))
    loss.backward()
    return float(loss.detach()), {k: (t.grad if t.grad is not None else None) for k, t in leaf.items()}


def _compare_grads(model, ref, tag):
    got = {n: p.grad for n, p in model.named_parameters() if not n.startswith("my_blocks.")}
    have = {n for n, g in got.items() if g is not None}
    want = {n for n, g in ref.items() if g is not None and n in got}
    assert have == want, (tag, sorted(have - want)[:5], sorted(want - have)[:5])
    worst_cos, worst_norm = 1.0, 0.0
    for n in sorted(want):
        g, r = got[n].double().cpu().reshape(-1), ref[n].double().reshape(-1)
        rn = float(r.norm())
        if rn == 0:
            assert float(g.norm()) == 0, (tag, n)
            continue
        cos = float(g @ r) / (float(g.norm()) * rn + 1e-300)
        nr = abs(float(g.norm()) / rn - 1)
        worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, nr)
        assert cos >= GRAD_COS and nr <= GRAD_NORM, (tag, n, cos, nr)
    return worst_cos, worst_norm


# ---- 4. HIP backward vs autograd through the oracle --------------------------------------------------------------------
def test_mm_grad_all_three_losses_match_oracle_odd_batch():
    """B = 5, mm_grad, loss = BCE(out) + BCE(out_a) + BCE(out_v): every branch of the reverse schedule, the pooled heads' gradient
    accumulated onto the fusion stack's input gradient."""
    cfg, L, B = AVSiamConfig(), 527, 5
    a, v = synth_inputs(cfg, B, 31)
    v = v.unsqueeze(1)
    y = _labels(B, L, 5)
    m = _model(L, 3)
    m.requires_grad_(True)
    out = m(a.cuda(), v.cuda(), "mm_grad")
    yd = y.cuda()
    loss = sum(F.binary_cross_entropy_with_logits(o, yd) for o in out)
    loss.backward()

    def fn(o):
        return sum(F.binary_cross_entropy_with_logits(t, y) for t in o)
    fn.mode = "mm_grad"
    ref_loss, ref = _oracle_grads(synth_state_ft(cfg, L, 3, "random"), cfg, a, v, fn)
    loss = loss.detach()
    assert abs(float(loss) - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    cos, nr = _compare_grads(m, ref, "mm_grad_sum")
    record_margin("ft_train.mm_grad_sum_B5", worst_cos=cos, worst_norm=nr, loss_err=abs(float(loss) - ref_loss))


@pytest.mark.parametrize("case", ["videoonly_T2", "audioonly_CE", "mm_out_freeze_base"])
def test_modes_match_oracle(case):
    cfg = AVSiamConfig()
    if case == "videoonly_T2":
        B, L, mode = 2, 309, "videoonly"
        a, v = synth_inputs(cfg, B * 2, 41)
        a, v = None, v.view(B, 2, *v.shape[1:])
        y = _labels(B * 2, L, 7).view(B, 2, L)
        lossf = lambda o, t: F.binary_cross_entropy_with_logits(o, t)           # noqa: E731
    elif case == "audioonly_CE":
        B, L, mode = 3, 309, "audioonly"
        a, v = synth_inputs(cfg, B, 43)
        v = None
        y = _labels(B, L, 8)
        lossf = lambda o, t: F.cross_entropy(o, t)                                # noqa: E731
    else:
        B, L, mode = 2, 527, "mm_grad"
        a, v = synth_inputs(cfg, B, 45)
        v = v.unsqueeze(1)
        y = _labels(B, L, 9)
        lossf = lambda o, t: F.binary_cross_entropy_with_logits(o[0], t)          # noqa: E731
    m = _model(L, 4)
    from avsiam_amd.models.cav_mae_ft import param_group
    for n, p in m.named_parameters():
        p.requires_grad_(not (case == "mm_out_freeze_base" and param_group(n) == "base"))
    out = m(a.cuda() if a is not None else None, v.cuda() if v is not None else None, mode)
    loss = lossf(out, y.cuda())
    loss.backward()

    def fn(o):
        return lossf(o, y)
    fn.mode = mode
    P = synth_state_ft(cfg, L, 4, "random")
    ref_loss, ref = _oracle_grads(P, cfg, a, v, fn)
    if case == "mm_out_freeze_base":
        ref = {k: (g if param_group(k) != "base" else None) for k, g in ref.items()}
    loss = loss.detach()
    assert abs(float(loss) - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    cos, nr = _compare_grads(m, ref, case)
    record_margin(f"ft_train.{case}", worst_cos=cos, worst_norm=nr, loss_err=abs(float(loss) - ref_loss))
    if case == "mm_out_freeze_base":
        assert all(p.grad is None for n, p in m.named_parameters() if param_group(n) == "base")


# ---- 5. fused train_step vs the autograd path; HIP Adam vs torch.optim.Adam ----------------------------------------------
@pytest.mark.parametrize("branch", ["mm", "a", "v"])
def test_fused_step_matches_autograd_and_torch_adam(branch):
    cfg, L, B = AVSiamConfig(), 527, 2
    a, v = synth_inputs(cfg, B, 51)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    y = _labels(B, L, 11).cuda()
    m = _model(L, 5)
    m.requires_grad_(True)
    # fused step with lr 0: parameters stay, the gradient arena holds the fused gradients
    fl = m.train_step(a, v, y, 0.0, "mm_grad", branch=branch)
    fused = {n: p.grad.clone() for n, p in m._params.items() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    out = m(a, v, "mm_grad")
    o = {"mm": out[0], "a": out[1], "v": out[2]}[branch]
    loss = F.binary_cross_entropy_with_logits(o, y)
    loss.backward()
    auto = {n: p.grad.clone() for n, p in m._params.items() if p.grad is not None}
    assert set(fused) == set(auto), (sorted(set(fused) ^ set(auto))[:5])
    assert abs(float(fl) - float(loss)) <= 1e-4 * abs(float(loss)), (float(fl), float(loss))
    worst = 1.0
    for n in auto:
        g, r = fused[n].double().reshape(-1), auto[n].double().reshape(-1)
        if float(r.norm()) == 0:
            continue
        cos = float(g @ r / (g.norm() * r.norm()))
        worst = min(worst, cos)
        assert cos >= FUSED_COS and abs(float(g.norm() / r.norm()) - 1) <= 1e-3, (branch, n, cos)
    record_margin(f"ft_train.fused_vs_autograd.{branch}", worst_cos=worst)
    # one Adam step of the three groups, HIP vs torch, on the autograd gradients (fresh moments: the lr-0 step above counted as a step)
    m._opt = None
    from avsiam_amd.models.cav_mae_ft import param_group
    lr, head_lr, mm_lr = 1e-4, 100.0, 100.0
    names = [n for n, _ in m.named_parameters()]
    ref_p = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        if p.grad is not None:
            ref_p[n].grad = p.grad.detach().clone()
    groups = {"base": [], "head": [], "mm": []}
    for n in names:
        groups[param_group(n)].append(ref_p[n])
    opt = torch.optim.Adam([{"params": groups["base"], "lr": lr}, {"params": groups["head"], "lr": lr * head_lr},
                            {"params": groups["mm"], "lr": lr * mm_lr}], weight_decay=5e-7, betas=(0.95, 0.999))
    opt.step()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.adam_step(lr, head_lr, mm_lr)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if p.grad is None:
            assert torch.equal(p.detach(), before[n]), f"{n} has no gradient but changed"
        else:
            err = float((p.detach() - ref_p[n].detach()).abs().max() / ref_p[n].detach().abs().max().clamp_min(1e-30))
            assert err <= 1e-6, (n, err)


# ---- 6. training sanity ------------------------------------------------------------------------------------------------
def test_thirty_fused_steps_lower_the_loss():
    cfg, L, B = AVSiamConfig(), 527, 4
    a, v = synth_inputs(cfg, B, 61)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    g = torch.Generator().manual_seed(12)
    y = ((torch.rand(B, L, generator=g) < 0.02).float() * 0.9 + 0.1 / L).cuda()
    m = _model(L, 6, "init")
    m.requires_grad_(True)
    losses = []
    for i in range(30):
        losses.append(m.train_step(a, v, y, 1e-4, "mm_grad", branch=("mm", "a", "v")[i % 3], head_lr=100.0, mm_lr=100.0))
    losses = [float(x) for x in losses]
    record_margin("ft_train.sanity30", first=losses[0], last=losses[-1], tail=losses[-3:])
    assert all(math.isfinite(x) for x in losses), losses
    assert max(losses[-3:]) < 0.35 * losses[0], losses     # measured 0.12 (0.777 -> 0.093 / 0.048 / 0.047)


# ---- 7. inference unchanged --------------------------------------------------------------------------------------------
def test_inference_path_unchanged():
    cfg, L, B = AVSiamConfig(), 527, 2
    a, v = synth_inputs(cfg, B, 71)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    m0 = _model(L, 8)
    ref = m0(a, v, "mm_grad")
    assert all(o.grad_fn is None and not o.requires_grad for o in ref)
    assert m0.arena.g is None and m0.arena.wt.numel() == 0, "an inference-only model allocated training buffers"
    m1 = _model(L, 8)
    m1.requires_grad_(True)
    with torch.no_grad():
        got = m1(a, v, "mm_grad")
    for r, o in zip(ref, got):
        assert torch.equal(r, o)
    t = m1(a, v, "mm_grad")                    # grad mode on: the training node (activations kept), the same kernels
    assert all(o.grad_fn is not None for o in t)
    for r, o in zip(ref, t):
        torch.testing.assert_close(o.detach(), r, rtol=1e-3, atol=1e-3)


def test_second_backward_is_refused():
    cfg, L, B = AVSiamConfig(), 10, 1
    a, _ = synth_inputs(cfg, B, 81)
    m = _model(L, 9)
    m.requires_grad_(True)
    out = m(a.cuda(), None, "audioonly")
    s = out.sum()
    s.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        s.backward()


# ---- 8. command line ---------------------------------------------------------------------------------------------------
def test_cli_two_tiny_epochs_write_checkpoints_and_results(tmp_path):
    """run_cavmae_ft_base.main on synthetic clips, starting from a checkpoint the pre-training train() format writes ('module.' keys)."""
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.param_spec import state_dict_keys, state_dict_keys_ft
    from avsiam_amd.run_cavmae_ft_base import main
    from avsiam_amd.traintest_cavmae_base import _save_checkpoint
    ck = str(tmp_path / "audio_model.1.pth")
    _save_checkpoint(CAVMAE_BASE(), ck)
    exp = tmp_path / "ft"
    out = main(["--ftmode", "mm_grad", "--n_class", "527", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "2",
                "--n_epochs", "2", "--save_model", "True", "--exp_dir", str(exp), "--pretrain_path", ck, "--steps-per-epoch", "3",
                "--val-steps", "1", "--lrscheduler_start", "1", "--n-print-steps", "2"])
    for f in ("models/audio_model.1.pth", "models/audio_model.2.pth", "models/best_audio_model.pth", "result.csv"):
        assert (exp / f).exists(), f
    res = np.loadtxt(exp / "result.csv", delimiter=",")
    assert res.shape == (2, 4) and np.all(np.isfinite(res[:, 3]))
    cfg = AVSiamConfig()
    pt, ft = set(state_dict_keys(cfg)), state_dict_keys_ft(cfg, 527)
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.run_cavmae_ft_base import load_pretrained
    miss, unexpected = load_pretrained(CAVMAEFT_BASE(527), ck)
    assert sorted(miss) == sorted(k for k in ft if k not in pt)
    assert sorted(unexpected) == sorted(k for k in pt if k not in set(ft))
    sd = torch.load(exp / "models" / "best_audio_model.pth")
    assert len(sd) == len(ft) and all(k.startswith("module.") for k in sd)
    assert out["best_epoch"] in (1, 2)


# ---- 3. HIP vs the reference goldens of the training forms (tools/gen_golden_ft_train.py) --------------------------------------
# normalised as tests.helpers.gpu_grads_vs_golden says; the same bounds as the pre-training goldens (tests/test_parity_gpu.py)
GOLD_L2, GOLD_SAMP, GOLD_SUM = 0.01, 0.3, 1.2


@pytest.mark.parametrize("name", ["ftt_mm_out", "ftt_mm_a", "ftt_mm_v", "ftt_mm_sum", "ftt_mm_freeze", "ftt_audio_ce", "ftt_video"])
def test_backward_matches_reference_golden(name):
    from avsiam_amd.models.cav_mae_ft import param_group
    from tests.helpers import golden_grads, load_golden
    from tests.test_ft_train_oracle_golden import ftt_inputs, ftt_loss
    d = load_golden(name)
    cfg = AVSiamConfig()
    m = _model(int(d["label_dim"]), int(d["weight_seed"]))
    freeze = bool(d["freeze_base"])
    for n, p in m.named_parameters():
        p.requires_grad_(not (freeze and param_group(n) == "base"))
    a, v = ftt_inputs(d, cfg)
    out = m(a.cuda() if a is not None else None, v.cuda() if v is not None else None, str(d["mode"]))
    outs = dict(zip(("out", "out_a", "out_v"), out)) if isinstance(out, tuple) else {"out": out}
    loss = ftt_loss(d, outs, torch.from_numpy(d["labels"]).cuda())
    loss.backward()
    ref = float(d["loss"])
    err = abs(float(loss.detach()) - ref) / max(1.0, abs(ref))
    assert err <= LOSS_TOL, (float(loss.detach()), ref)
    names, none, *_ = golden_grads(d)
    have = {n for n, p in m.named_parameters() if p.grad is not None}
    assert have == set(names), (sorted(have ^ set(names))[:6])
    if freeze:
        assert all(p.grad is None for n, p in m.named_parameters() if param_group(n) == "base")
    gpu_grads_vs_golden(d, lambda n: m._params[n].grad, "ft_train.golden_" + name, l2_rel=GOLD_L2, samp_rel=GOLD_SAMP, sum_rel=GOLD_SUM)
    record_margin("ft_train.golden_" + name, loss_err=err)


# ---- gradient accumulation across backwards is refused, not silently wrong ------------------------------------------------
def test_second_backward_without_zeroing_is_refused():
    cfg, L, B = AVSiamConfig(), 527, 2
    a, v = synth_inputs(cfg, B, 91)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    y = _labels(B, L, 13).cuda()
    m = _model(L, 10)
    m.requires_grad_(True)
    F.binary_cross_entropy_with_logits(m(a, v, "mm_grad")[0], y).backward()
    first = {n: p.grad.clone() for n, p in m._params.items() if p.grad is not None}
    # a second forward + backward (micro-batch accumulation) without clearing .grad: an error, and the delivered gradients are intact
    out = m(a[:1], v[:1], "mm_grad")
    with pytest.raises(RuntimeError, match="accumulation"):
        F.binary_cross_entropy_with_logits(out[1], y[:1]).backward()
    for n, g in first.items():
        assert torch.equal(m._params[n].grad, g), n
    # after zero_grad (set_to_none): the same backward as on a fresh forward
    m.zero_grad(set_to_none=True)
    F.binary_cross_entropy_with_logits(m(a, v, "mm_grad")[0], y).backward()
    for n, g in first.items():                     # (equal up to the order of the fp32 atomics in the weight-gradient reductions)
        assert float((m._params[n].grad - g).norm()) <= 1e-4 * float(g.norm()) + 1e-12, n
    # train_step clears the gradients itself (optimizer.zero_grad of the reference loop): consecutive steps never accumulate
    m.train_step(a, v, y, 0.0, "mm_grad", branch="mm")
    m.train_step(a, v, y, 0.0, "mm_grad", branch="a")
    assert m._params["mm_layer_1.attn.qkv.weight"].grad is None and m._params["mlp_head_a.1.weight"].grad is not None


def test_is_eval_forms_stay_inference_only():
    cfg, L, B = AVSiamConfig(), 10, 2
    a, _ = synth_inputs(cfg, B, 93)
    m = _model(L, 11)
    m.requires_grad_(True)
    out = m(a.cuda(), None, "audioonly", is_eval=True)
    assert tuple(out.shape) == (B, 1, L) and out.grad_fn is None
