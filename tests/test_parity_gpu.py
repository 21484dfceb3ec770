"""End-to-end parity on a real MI355X: the HIP path (through CAVMAE_BASE.forward / loss.backward, i.e. through
the C ABI) against the CPU oracle on identical weights, inputs and mask plan, and against the golden vectors
the unmodified reference produced (tests/golden).

Tolerances (bf16 GEMM/attention operands with fp32 accumulation vs an fp32 reference; north_star asks for a
stated tolerance).  They are set at about 3x the worst error MEASURED on an MI355X and logged by these tests into
profiles/r03/parity_margins.json (tests.helpers.record_margin; round 3: with the bf16 residual-gradient stream):
  losses            rel 2e-3 (measured <= 5e-4; the constant-input golden case 1.8e-3 -> 6e-3)
  contrastive logits abs 0.01 (measured 1.7e-3 at tau = 0.05)
  gradients, every live tensor: cosine >= 0.9998 (measured >= 0.99990; ViT-L / ViT-H 0.99985), norm ratio within 1 % (measured <= 0.30 %; ViT-L 0.73 % -> 2 %)
  reference goldens, every live tensor: L2 norm within 1 % (0.29 %), the 8 sampled elements within 0.3 rms (0.10), the
  element sum within 2.0 / 0.25 norms (MAE / contrastive; 0.62 / 0.075 - the sum is a cancelling statistic, kept as a weak check)
  dead parameters get no gradient; masks are bit-exact."""
import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.maskplan import make_contrastive_plan, make_mae_plan
from avsiam_amd.param_spec import build_spec
from avsiam_amd.weights import synth_inputs, synth_state
from tests.helpers import golden_plan, gpu_grads_vs_golden, load_golden, record_margin

pytestmark = pytest.mark.gpu


# Tolerances of the reference-golden gradient checks (normalised as tests.helpers.gpu_grads_vs_golden says).  Measured worst cases
# (profiles/r03/parity_margins.json): l2 0.28 %, samples 0.11 rms, sum 0.66 norms (MAE pass: mm_layer_2.mlp.fc2.weight - the element
# sum is a BIAS detector: 0.66 norms over 2.4 M elements is a common offset of 4e-4 of an element's rms) / 0.066 (contrastive).
# What each tolerance can and cannot reject is pinned on the CPU by tests/test_oracle_golden.py::test_golden_gradient_checker_discriminates.
GOLD_L2, GOLD_SAMP, GOLD_SUM = 0.01, 0.3, 1.2
GOLD_L2_C, GOLD_SAMP_C, GOLD_SUM_C = 0.01, 0.3, 0.25
LOSS_RTOL, LOSS_RTOL_GOLD, LOGITS_ATOL, COS_MIN, RATIO_TOL = 2e-3, 6e-3, 0.01, 0.9998, 0.01


def _model(cfg, seed=1234, mode="random", **kw):
    """kw: per-model options (fp8_mode=, recompute=, grad_stream=, options=) - precision is a property of the model"""
    from avsiam_amd.models import CAVMAE_BASE
    m = CAVMAE_BASE(cfg=cfg, init_seed=seed, init_mode=mode, verbose=False, **kw).cuda()
    return m


def _oracle(cfg, a, v, plan, mae, seed=1234, mode="random"):
    from oracle import ref_cpu
    torch.set_num_threads(16)
    P = {k: t.clone().requires_grad_(True) for k, t in synth_state(cfg, seed, mode, include_dead=False).items()}
    extras = {}
    out = ref_cpu.forward(P, cfg, a, v, plan, mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, extras=extras)
    out[0].backward()
    return out, extras, {k: p.grad for k, p in P.items()}


MATRIX_NUMEL = 1 << 16       # "matrix" tensors (Linear / patch-embedding weights, position tables) vs "vector" tensors (biases, LayerNorm)


def _compare_grads(model, ref_grads, cos_min=0.9998, ratio_tol=0.01, tag=None, whole_cos_min=None, matrix_cos_min=None, matrix_ratio_tol=None,
                   vectors_cos_min=None):
    """Every live tensor against the oracle's: cosine >= cos_min and norm within ratio_tol; the whole live gradient as one vector >=
    whole_cos_min.  matrix_cos_min / matrix_ratio_tol: tighter bounds for the tensors of at least MATRIX_NUMEL elements (the fp8 modes:
    a weight-gradient element sums over every token row and a matrix has 10^5 - 10^7 of them, so its direction and length are far
    better determined than those of a 1280-element bias at batch 2, which set `cos_min` / `ratio_tol`).
    vectors_cos_min: floor for ALL the smaller tensors (biases, LayerNorm vectors) taken together as one vector - a single 1280-element
    bias at batch 2 is mostly noise in the fp8 modes, their union is not.
    All statistics are gathered (and recorded: tests.helpers.record_margin) BEFORE anything is asserted, so a failing run still says
    what the worst tensors were."""
    worst = (1.0, None)
    worst_mat = (1.0, None)
    worst_ratio = (0.0, None)
    worst_mat_ratio = (0.0, None)
    bad = []
    dot = ng = nr = 0.0                    # the whole live gradient as one vector
    vdot = vng = vnr = 0.0                 # the vector tensors as one vector
    for info in build_spec(model.cfg):
        p = model._params[info.name]
        rg = ref_grads.get(info.name)
        if rg is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{info.name}: dead parameter received a gradient"
            continue
        assert p.grad is not None, f"{info.name}: live parameter has no gradient"
        g = p.grad.detach().double().cpu().reshape(-1)
        r = rg.double().reshape(-1)
        if r.norm() == 0:
            assert g.norm() < 1e-6, info.name
            continue
        cos = float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30))
        ratio = float(g.norm() / r.norm())
        dot, ng, nr = dot + float(torch.dot(g, r)), ng + float(g.norm()) ** 2, nr + float(r.norm()) ** 2
        mat = g.numel() >= MATRIX_NUMEL
        if not mat:
            vdot, vng, vnr = vdot + float(torch.dot(g, r)), vng + float(g.norm()) ** 2, vnr + float(r.norm()) ** 2
        if not (cos >= cos_min and abs(ratio - 1) <= ratio_tol):
            bad.append((info.name, cos, ratio))
        if mat:
            if not ((matrix_cos_min is None or cos >= matrix_cos_min) and (matrix_ratio_tol is None or abs(ratio - 1) <= matrix_ratio_tol)):
                bad.append((info.name, cos, ratio, "matrix"))
            if cos < worst_mat[0]:
                worst_mat = (cos, info.name)
            if abs(ratio - 1) > worst_mat_ratio[0]:
                worst_mat_ratio = (abs(ratio - 1), info.name)
        if cos < worst[0]:
            worst = (cos, info.name)
        if abs(ratio - 1) > worst_ratio[0]:
            worst_ratio = (abs(ratio - 1), info.name)
    whole = dot / ((ng * nr) ** 0.5 + 1e-30)
    vwhole = vdot / ((vng * vnr) ** 0.5 + 1e-30)
    if tag:
        record_margin(tag, worst_cos=worst[0], worst_cos_tensor=worst[1], worst_norm_ratio_err=worst_ratio[0], worst_norm_tensor=worst_ratio[1],
                      whole_gradient_cos=whole, worst_matrix_cos=worst_mat[0], worst_matrix_tensor=worst_mat[1],
                      worst_matrix_norm_ratio_err=worst_mat_ratio[0], worst_matrix_norm_tensor=worst_mat_ratio[1], vector_tensors_cos=vwhole)
    assert not bad, (tag, bad[:8], len(bad))
    assert whole_cos_min is None or whole >= whole_cos_min, whole
    assert vectors_cos_min is None or vwhole >= vectors_cos_min, vwhole
    return worst


@pytest.mark.parametrize("name", ["m_w1_b4", "m_w1_b2_const"])
def test_mae_pass_matches_reference_golden(name):
    d = load_golden(name)
    cfg = AVSiamConfig()
    B = int(d["batch"])
    const = float(d["constant"])
    a, v = synth_inputs(cfg, B, int(d["input_seed"]), None if np.isnan(const) else const)
    plan = golden_plan(d)
    m = _model(cfg, int(d["weight_seed"]))
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1, contrast_loss_weight=0, mask_plan=plan)
    out[0].backward()
    got = np.array([out[i].item() for i in (0, 1, 2, 3, 4, 7)])
    np.testing.assert_allclose(got, d["out_scalars"], rtol=LOSS_RTOL_GOLD, atol=1e-6)
    np.testing.assert_array_equal(out[5].cpu().numpy(), d["mask_a"])
    np.testing.assert_array_equal(out[6].cpu().numpy(), d["mask_v"])
    record_margin("golden_" + name, loss_rel=float(np.max(np.abs(got[:4] - d["out_scalars"][:4]) / np.abs(d["out_scalars"][:4]))))
    gpu_grads_vs_golden(d, lambda n: m._params[n].grad, "golden_" + name, l2_rel=GOLD_L2, samp_rel=GOLD_SAMP, sum_rel=GOLD_SUM)


@pytest.mark.parametrize("name", ["c_w1_b4", "c_w1_b5", "c_w1_b10"])
def test_contrastive_pass_matches_reference_golden(name):
    """The three shapes of the 5-way chunk partition (cav_mae_base.py:540-570): B = 4 (one group is empty), B = 5 (five groups of
    one sample) and B = 10 (five groups of two) - outputs, logits and every live gradient against the unmodified reference's."""
    d = load_golden(name)
    cfg = AVSiamConfig()
    B = int(d["batch"])
    a, v = synth_inputs(cfg, B, int(d["input_seed"]))
    plan = golden_plan(d)
    m = _model(cfg, int(d["weight_seed"]))
    out = m(a.cuda(), v.cuda(), mae_loss_weight=0, contrast_loss_weight=1, mask_plan=plan)
    out[0].backward()
    got = np.array([out[i].item() for i in (0, 1, 2, 3, 4, 7)])
    np.testing.assert_allclose(got[[0, 4]], d["out_scalars"][[0, 4]], rtol=LOSS_RTOL)
    assert abs(got[5] - d["out_scalars"][5]) <= 1.0 / B + 1e-6          # c_acc moves in steps of 1/B
    assert out[5] is None and out[6] is None
    eng = m._engine("contrastive", B)
    np.testing.assert_allclose(eng.total.cpu().numpy(), d["logits"], atol=LOGITS_ATOL)
    record_margin("golden_" + name, loss_rel=float(abs(got[0] - d["out_scalars"][0]) / abs(d["out_scalars"][0])),
                  logits_abs=float(np.abs(eng.total.cpu().numpy() - d["logits"]).max()))
    gpu_grads_vs_golden(d, lambda n: m._params[n].grad, "golden_" + name, l2_rel=GOLD_L2_C, samp_rel=GOLD_SAMP_C, sum_rel=GOLD_SUM_C)


@pytest.mark.parametrize("which,B,T,La", [("mae", 4, 1, 128), ("contrastive", 4, 1, 128), ("contrastive", 7, 1, 512),
                                         ("mae", 2, 3, 128), ("contrastive", 5, 2, 128), ("mae-unpruned", 2, 3, 128)])
def test_pass_matches_oracle_full_gradients(which, B, T, La):
    """Every live tensor's gradient vs the oracle (cosine/norm), incl. configs[0] (128 audio tokens) and T > 1.
    "mae-unpruned": the MAE pass with EngineOptions.prune_dead off (position-ordered decoder rows, every row through the last block and the heads)."""
    kw = {}
    if which == "mae-unpruned":
        from avsiam_amd.config import EngineOptions
        which, kw = "mae", {"options": EngineOptions(prune_dead=False)}
    cfg = AVSiamConfig(audio_tokens=La, frames=T)
    a, v = synth_inputs(cfg, B, 99)
    gen = torch.Generator().manual_seed(7)
    import random
    plan = make_mae_plan(cfg, B, gen) if which == "mae" else make_contrastive_plan(cfg, B, gen, random.Random(7))
    mae = which == "mae"
    m = _model(cfg, 4321, **kw)
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
    out[0].backward()
    if mae:
        assert m._engine("mae", B).prune == (not kw)
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 4321)
    for i in (0, 1, 2, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    if mae:
        assert torch.equal(out[5].cpu(), ref[5]) and torch.equal(out[6].cpu(), ref[6])
        eng = m._engine("mae", B)
        # the predictions of the SCORED rows (mask 1): the others are not computed (EngineOptions.prune_dead; the reference computes them for
        # nothing, cav_mae_base.py:679-682) - and every scored row must be there
        pa, pv = eng.predictions()
        sa, sv = ref[5].bool(), ref[6].bool()
        ra_, rv_ = extras["pred_a"].detach().reshape(pa.shape), extras["pred_v"].detach().reshape(pv.shape)
        assert torch.isfinite(pa[sa]).all() and torch.isfinite(pv[sv]).all()
        ea = float((pa[sa] - ra_[sa]).norm() / ra_[sa].norm())
        ev = float((pv[sv] - rv_[sv]).norm() / rv_[sv].norm())
        record_margin(f"oracle_{which}_B{B}_T{T}_La{La}", pred_a_rel_l2=ea, pred_v_rel_l2=ev)
        assert ea < 2e-2 and ev < 2e-2, (ea, ev)
    else:
        eng = m._engine("contrastive", B)
        el = float((eng.total.cpu() - extras["logits"].detach()).abs().max())
        record_margin(f"oracle_{which}_B{B}_T{T}_La{La}", logits_abs=el)
        assert el < LOGITS_ATOL, el
        assert abs(out[7].item() - ref[7].item()) <= 1.0 / B + 1e-6
    record_margin(f"oracle_{which}_B{B}_T{T}_La{La}", loss_rel=max(abs(out[i].item() - ref[i].item()) / max(abs(ref[i].item()), 1e-12) for i in (0, 1, 2, 3, 4)
                                                                   if ref[i].item() != 0))
    _compare_grads(m, rgrads, tag=f"oracle_{which}_B{B}_T{T}_La{La}")


def test_forward_requires_gpu_and_library():
    from avsiam_amd import _lib
    from avsiam_amd.models import CAVMAE_BASE
    cfg = AVSiamConfig(audio_tokens=128)
    m = CAVMAE_BASE(cfg=cfg, verbose=False)
    a, v = synth_inputs(cfg, 2, 1)
    with pytest.raises(_lib.AvsiamHipError):
        m(a, v)


@pytest.mark.parametrize("which,B,T,La", [("mae", 3, 2, 128), ("contrastive", 6, 1, 512)])
def test_device_drawn_plan_matches_oracle(which, B, T, La):
    """Default path: the mask plan is drawn on the device (csrc/maskplan.hip).  Read the plan back, feed it to the
    oracle, and require the same parity as with injected plans - this pins the kernel's index outputs (row gather,
    un-shuffle sources, loss masks) against what the plan says."""
    cfg = AVSiamConfig(audio_tokens=La, frames=T)
    a, v = synth_inputs(cfg, B, 5)
    mae = which == "mae"
    from avsiam_amd.models import CAVMAE_BASE
    m = CAVMAE_BASE(cfg=cfg, init_seed=77, init_mode="random", verbose=False, plan_seed=123).cuda()
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1)
    out[0].backward()
    plan = m.last_plans(B)[which]
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 77)
    for i in (0, 1, 2, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    if mae:
        assert torch.equal(out[5].cpu(), ref[5]) and torch.equal(out[6].cpu(), ref[6])
    _compare_grads(m, rgrads, tag=f"devplan_{which}")
    # a second forward draws a different plan (the Philox key advances)
    m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1)
    plan2 = m.last_plans(B)[which]
    if mae:
        assert not torch.equal(plan.ids_keep_a, plan2.ids_keep_a)
    else:
        assert any(not torch.equal(x, y) for x, y in zip(plan.a_keep, plan2.a_keep) if x.numel() == y.numel() and x.numel() < 512) or \
            not torch.equal(plan.a_group, plan2.a_group)


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_vit_large_matches_oracle(which):
    """BASELINE.json configs[3] family: ViT-L/16 (D=1024, 24 layers, 16 heads), here at a small shape (2 frames, 128 audio
    tokens, batch 2).  No reference source exists for it: the oracle is the pin."""
    from avsiam_amd.config import vit_large
    import random
    cfg = vit_large(audio_tokens=128, frames=2)
    B = 2
    a, v = synth_inputs(cfg, B, 17)
    gen = torch.Generator().manual_seed(3)
    mae = which == "mae"
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(3))
    m = _model(cfg, 99)
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
    out[0].backward()
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 99)
    for i in (0, 1, 2, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    _compare_grads(m, rgrads, cos_min=0.9998, ratio_tol=0.02, tag=f"vit_large_{which}")


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_vit_huge_width_matches_oracle(which):
    """BASELINE.json configs[4]'s encoder width in bf16: 1280 wide, 16 heads of 80 (the hd-80 attention instantiation: a 96-wide LDS
    image, five contraction steps), MLP 5120 - here 4 layers deep at a small shape (2 frames, 128 audio tokens, batch 2) against the
    oracle.  16 x 16 patches (not /14), no fp8."""
    from avsiam_amd.config import vit_huge
    import random
    cfg = vit_huge(audio_tokens=128, frames=2, depth=4)
    B = 2
    a, v = synth_inputs(cfg, B, 19)
    gen = torch.Generator().manual_seed(4)
    mae = which == "mae"
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(4))
    m = _model(cfg, 98)
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
    out[0].backward()
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 98)
    for i in (0, 1, 2, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    _compare_grads(m, rgrads, cos_min=0.9998, ratio_tol=0.02, tag=f"vit_huge_{which}")


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_recompute_matches_saved_activations(which):
    """EngineOptions.recompute (CAVMAE_BASE(recompute=...)): every Stack keeps only its blocks' fp32 inputs and re-runs a block's forward in front of its backward ("1"), or
    does so for the first half of its blocks only and saves the rest ("0.5").  The kernels are deterministic, so the loss is bitwise the
    same and the gradients differ only by the order of the fp32 atomics of the weight-gradient GEMMs."""
    import random
    from avsiam_amd import engine
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    B = 3
    a, v = synth_inputs(cfg, B, 23)
    gen = torch.Generator().manual_seed(6)
    mae = which == "mae"
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(6))
    res = []
    try:
        for rec in ("0", "1", "0.5"):
            m = _model(cfg, 97, recompute=rec)
            comm = None
            if rec == "0.5":           # with the data-parallel reducer attached: every element of the pass's range must be reduced exactly once
                from tests.helpers import _Waited

                class Counting:
                    active, world, rank = True, 1, 0

                    def __init__(self):
                        self.messages = []

                    def all_gather(self, out, inp):
                        out.view(1, -1).copy_(inp.reshape(1, -1))

                    def all_reduce_async(self, t):
                        self.messages.append(t.numel())
                        return _Waited()

                    def all_reduce(self, t):
                        self.messages.append(t.numel())

                comm = Counting()
                m.set_distributed(1, 0, comm)
            out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
            out[0].backward()
            torch.cuda.synchronize()
            res.append((out[0].item(), {k: p.grad.detach().double().cpu() for k, p in m._params.items() if p.grad is not None}))
            if rec == "0.5":           # 12 / 2 / 8-block stacks: 6 / 1 / 4 recomputed, the others with buffers of their own
                from avsiam_amd.param_spec import P1, P2
                lo, hi = m.arena.range[P2 if mae else P1]
                assert len(comm.messages) >= 2 and sum(comm.messages) == hi - lo, (comm.messages, hi - lo)
                eng = m._engine("mae" if mae else "contrastive", B)
                stacks = [v_ for v_ in vars(eng).values() if isinstance(v_, engine.Stack)]
                assert stacks and all(0 < st.nrecomp < st.nblocks for st in stacks), [(st.nrecomp, st.nblocks) for st in stacks]
                assert all(st.act[0] is st.act[st.nrecomp - 1] and st.act[st.nrecomp] is not st.act[0] for st in stacks)
    finally:
        from avsiam_amd import _lib
        _lib.tuning_set("cu_reserve", 0)          # (the counting communicator is "active": set_distributed reserved CUs for collectives, process-wide)
    for r in res[1:]:
        assert res[0][0] == r[0]
        assert res[0][1].keys() == r[1].keys() and len(r[1]) > 100
        worst = 0.0
        for k, g0 in res[0][1].items():
            g1 = r[1][k]
            if float(g0.norm()) > 0:
                worst = max(worst, float((g1 - g0).norm() / g0.norm()))
        assert worst < 1e-5, worst


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_fp8_forward_mode_against_bf16(which):
    """CAVMAE_BASE(fp8_mode=...) (BASELINE configs[4]'s fp8 MFMA path, opt-in): the forward GEMMs of every block on e4m3 operands with per-tensor
    delayed scaling, backward in bf16 (a self-comparison that isolates the quantisation; test_fp8_forward_mode_against_oracle is the pin).  Its own tolerance against the bf16 path (three mantissa bits per operand), at about 3x the measured error:
    losses within 0.3 % (measured 0.08 %), every live gradient tensor's cosine above 0.98 (0.9925) and norm within 6 % (2.2 %)."""
    import random
    from avsiam_amd import engine
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    B = 3
    a, v = synth_inputs(cfg, B, 29)
    gen = torch.Generator().manual_seed(8)
    mae = which == "mae"
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(8))
    res = []
    if True:
        for mode in ("0", "1"):
            m = _model(cfg, 96, fp8_mode=mode)
            out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
            out[0].backward()
            torch.cuda.synchronize()
            res.append((out[0].item(), {k: p.grad.detach().double().cpu() for k, p in m._params.items() if p.grad is not None}))
            if mode == "1":
                # the second forward runs on the calibrated records: LayerNorm, the GELU epilogue and the attention epilogue write the
                # e4m3 operands themselves (rounded from fp32 instead of from bf16) - same weights, same plan, so nearly the same loss
                # (measured 0.4 % on the contrastive loss, whose 3 x 3 logits are divided by tau = 0.05)
                again = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)[0].item()
                record_margin(f"fp8_forward_{which}", second_forward_loss_rel=abs(again - out[0].item()) / abs(out[0].item()))
                assert abs(again - out[0].item()) <= 1.2e-2 * abs(out[0].item()), (again, out[0].item())
    l0, l1 = res[0][0], res[1][0]
    # MAE loss within 0.3 % (measured 0.05 %); the contrastive loss - 3 x 3 logits divided by tau = 0.05 - within 1.2 % (measured 0.34 %)
    assert l0 != l1 and abs(l1 - l0) <= (3e-3 if mae else 1.2e-2) * abs(l0), (l0, l1)
    worst_cos, worst_ratio = 1.0, 0.0
    for k, g0 in res[0][1].items():
        g1 = res[1][1][k]
        if float(g0.norm()) > 0 and g0.numel() >= 512:
            worst_cos = min(worst_cos, float(torch.dot(g0.reshape(-1), g1.reshape(-1)) / (g0.norm() * g1.norm())))
            worst_ratio = max(worst_ratio, abs(float(g1.norm() / g0.norm()) - 1))
    record_margin(f"fp8_forward_{which}", loss_rel=abs(l1 - l0) / abs(l0), grad_cos_min=worst_cos, grad_norm_ratio_err=worst_ratio)
    assert worst_cos > 0.975 and worst_ratio < (0.06 if mae else FP8_RATIO_TOL), (worst_cos, worst_ratio)


# fp8 (e4m3) forward mode against the fp32 CPU oracle: its OWN stated tolerance (three mantissa bits per GEMM operand; the bf16 path's
# margins are ~30x tighter).  Set at about 3x the worst error measured on an MI355X (profiles/r03/parity_margins.json, fp8_oracle_*):
#   losses            rel 5e-3   (measured <= 1.6e-3)
#   contrastive logits abs 0.12  (measured 0.039 at ViT-B, 0.006 at ViT-H/14; tau = 0.05 amplifies 20x)
#   gradients, every live tensor: cosine >= 0.975 (measured >= 0.9919), norm within 25 % (measured <= 8.3 %: at batch 2-3 a small error of
#   the 3 x 3 InfoNCE logits rescales the WHOLE contrastive gradient - direction 0.997, length +8 %; the MAE pass stays within 2.8 %)
FP8_LOSS_RTOL, FP8_LOGITS_ATOL, FP8_COS_MIN, FP8_RATIO_TOL = 5e-3, 0.12, 0.975, 0.25
# mode "2" (e5m2 gradient operands in the fc2 / fc1 / proj input-gradient GEMMs: 2 mantissa bits): losses and logits as above (the forward is
# the same); the whole live gradient as one vector: cosine >= 0.985 (measured 0.993 - 0.996); every tensor: cosine >= 0.70 (measured >= 0.877:
# a 1280-element bias of the batch-2 contrastive pass, it moves between runs; >= 0.956 at ViT-B, >= 0.986 in the MAE pass), norm within 30 %
# (measured <= 11.6 %)  (fp8bwd_oracle_* in the margins file)
FP8B_COS_MIN, FP8B_RATIO_TOL, FP8B_WHOLE_COS = 0.70, 0.30, 0.985
# round 6: the per-tensor bounds of modes "2" / "3" per (shape, pass), at <= 3x the measured gap (parity_margins.json fp8bwd_oracle_* /
# fp8wg_oracle_*); the ViT-H/14 contrastive case runs at batch 5 (one clip per mask-ratio group) instead of 2, where a 1280-element bias was mostly noise
FP8BW_TOL = {("vit_base", "mae"): (0.95, 0.17), ("vit_base", "contrastive"): (0.86, 0.22), ("vit_huge14", "mae"): (0.95, 0.17),
             ("vit_huge14", "contrastive"): (0.90, 0.07)}
# measured worst single tensors: ViT-B MAE 0.984 / 5.6 %, ViT-B contrastive (batch 3) 0.953 / 7.3 %, ViT-H/14 MAE 0.987 / 5.6 %, ViT-H/14 contrastive at batch 5
# 0.967 / 2.1 % (at batch 2: 0.877 / 11.6 % - the reason round 5 had to allow 0.70 / 30 % everywhere)
# mode "3" (round 4: the weight gradients on e5m2 gradient x e4m3 activation operands as well): forward as above; the weight-gradient tensors
# now carry the operands' 2- and 3-bit mantissas directly (each element a sum over the token rows, so the relative error falls with the row
# count: these test shapes have 500 - 1500 rows, the step's 10^5).  Measured (fp8wg_oracle_* in the margins file): the whole gradient's
# cosine 0.9928 - 0.9942 (mode "2": 0.9928 - 0.9959), the worst tensors the same bias vectors as in mode "2" - the same tolerances serve.
FP8W_COS_MIN, FP8W_RATIO_TOL, FP8W_WHOLE_COS = 0.70, 0.30, 0.985
# round 5: the per-tensor floor above is set by 1280-element bias vectors at batch 2; a MATRIX (>= 2^16 elements: every Linear / patch
# weight, the position tables) is held to its own, much tighter floor - a wrong weight-gradient tensor cannot hide behind the bias noise.
FP8W_MATRIX_COS_MIN = 0.90


@pytest.mark.parametrize("which", ["mae", "contrastive"])
@pytest.mark.parametrize("shape", ["vit_base", "vit_huge14"])
@pytest.mark.parametrize("mode", ["1", "2", "3"])
def test_fp8_forward_mode_against_oracle(shape, which, mode):
    """CAVMAE_BASE(fp8_mode=...) (BASELINE.json configs[4]'s "fp8 MFMA path") pinned to oracle/ref_cpu.py (the fp32 restatement of
    /root/reference/src/models/cav_mae_base.py:685-741), not to the HIP bf16 path: losses, contrastive logits, and every live gradient
    tensor's cosine / norm ratio, at ViT-B and at the ViT-H/14 geometry the mode is meant for (2 layers, 2 frames).  Two steps are
    compared: the calibration step (scales from the first batch, activations quantised by a pass) and the step after it (delayed
    scales on the device; LayerNorm / GELU / attention epilogues write the e4m3 operands themselves).
    mode "2": the four input-gradient GEMMs of a block run on e5m2 gradient operands as well (forward unchanged, so losses and logits
    are those of mode "1"; the gradients carry the extra rounding - own stated tolerance); mode "3": the block's weight gradients too."""
    import random
    from avsiam_amd import engine
    from avsiam_amd.config import vit_huge14
    cfg = vit_huge14(frames=2, depth=2) if shape == "vit_huge14" else AVSiamConfig(audio_tokens=128, frames=2)
    mae = which == "mae"
    B = (2 if mae else 5) if shape == "vit_huge14" else 3
    a, v = synth_inputs(cfg, B, 41)
    gen = torch.Generator().manual_seed(9)
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(9))
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 93)
    if True:
        m = _model(cfg, 93, fp8_mode=mode)
        for step in (0, 1):
            out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
            out[0].backward()
            torch.cuda.synchronize()
            tag = f"fp8{ {'1': '', '2': 'bwd', '3': 'wg'}[mode] }_oracle_{shape}_{which}_step{step}"
            worst_loss = 0.0
            for i in (0, 1, 2, 3, 4):
                err = abs(out[i].item() - ref[i].item()) / (abs(ref[i].item()) + 1e-12) if ref[i].item() != 0 else abs(out[i].item())
                worst_loss = max(worst_loss, err)
                assert err <= FP8_LOSS_RTOL, (step, i, out[i].item(), ref[i].item())
            record_margin(tag, loss_rel=worst_loss)
            if not mae:
                eng = m._engine("contrastive", B)
                err = float((eng.total.detach().cpu().double() - extras["logits"].detach().double()).abs().max())
                record_margin(tag, logits_abs=err)
                assert err <= FP8_LOGITS_ATOL, err
            cos_min, ratio_tol, whole = {"1": (FP8_COS_MIN, FP8_RATIO_TOL, None), "2": FP8BW_TOL[(shape, which)] + (FP8B_WHOLE_COS,),
                                         "3": FP8BW_TOL[(shape, which)] + (FP8W_WHOLE_COS,)}[mode]
            _compare_grads(m, rgrads, cos_min=cos_min, ratio_tol=ratio_tol, tag=tag, whole_cos_min=whole,
                           matrix_cos_min=FP8W_MATRIX_COS_MIN if mode in ("2", "3") else None)


PRUNE_REL, PRUNE_WHOLE_REL = 3e-2, 3.5e-3        # measured (six cases): worst tensor 1.05e-2 (the patch embeddings, bottom of the chain), whole gradient 1.1e-3


@pytest.mark.parametrize("frames,batch,recompute", [(1, 4, "0"), (2, 3, "0"), (2, 3, "1")])
def test_pruned_decoder_is_the_same_mae_pass(frames, batch, recompute):
    """EngineOptions.prune_dead (default on): unscored decoder rows (mask 0: zero loss, zero gradient) are dropped where the
    reference computes them for nothing - the last decoder block runs query / proj / LayerNorm-2 / MLP on the scored rows only (keys and values for
    all), decoder_norm, both prediction heads and the loss see the scored rows only, and the decoder rows are laid out [scored | kept] per sample.
    Exact arithmetic removal - but not a bitwise one: the grouped layout permutes the decoder's rows, so every decoder attention sums its keys in
    another order, and one flipped bf16 rounding at the top of a 22-block backward chain grows to the bf16 noise floor at its bottom (docs/rounds/r04.md
    item 1: two runs of the SAME schedule differ as much once an atomics order differs).  Against the same model with prune_dead=False, same
    weights / inputs / plan: masks bitwise, losses to 1e-4 (measured 2.4e-5), every gradient tensor within PRUNE_REL of its norm and the whole gradient within
    PRUNE_WHOLE_REL (~3x measured, parity_margins.json prune_dead_*), dead parameters stay dead - with an injected plan AND with a device-drawn one (the
    plan kernel's grouped layout), also with the recomputed blocks sharing one buffer set.  What pins BOTH forms to the reference are the goldens and
    the oracle (test_pass_matches_oracle_full_gradients runs the unpruned form too)."""
    from avsiam_amd.config import EngineOptions
    from avsiam_amd.models import CAVMAE_BASE
    cfg = AVSiamConfig(audio_tokens=128, frames=frames)
    B = batch
    a, v = synth_inputs(cfg, B, 31)
    plan = make_mae_plan(cfg, B, torch.Generator().manual_seed(12))
    res = {}
    for prune in (False, True):
        m = CAVMAE_BASE(cfg=cfg, init_seed=77, init_mode="random", verbose=False, plan_seed=5, options=EngineOptions(prune_dead=prune, recompute=recompute)).cuda()
        runs = []
        for injected in (True, False):
            for p in m._params.values():
                p.grad = None
            out = m(a.cuda(), v.cuda(), mae_loss_weight=1, contrast_loss_weight=0, mask_plan=plan if injected else None)
            out[0].backward()
            torch.cuda.synchronize()
            drawn = m.last_plans(B)["mae"] if not injected else None
            runs.append(([out[i].item() for i in (0, 1, 2, 3)], out[5].clone(), out[6].clone(),
                         {k: p.grad.detach().double().cpu() for k, p in m._params.items() if p.grad is not None}, drawn))
        eng = m._engine("mae", B)
        assert eng.prune == prune and (eng.st_dec.lq > 0) == prune
        res[prune] = runs
    for injected in (0, 1):
        (l0, ma0, mv0, g0, d0), (l1, ma1, mv1, g1, d1) = res[False][injected], res[True][injected]
        if d0 is not None:                                         # device-drawn: the same Philox key -> the same plan in both layouts
            assert torch.equal(d0.ids_keep_a, d1.ids_keep_a) and torch.equal(d0.ids_restore_v, d1.ids_restore_v)
        assert torch.equal(ma0, ma1) and torch.equal(mv0, mv1)
        for x0, x1 in zip(l0, l1):
            assert abs(x0 - x1) <= 1e-4 * abs(x0), (injected, l0, l1)
        assert g0.keys() == g1.keys() and len(g0) > 100
        worst = (0.0, None)
        num = den = 0.0
        for k in g0:
            n0 = float(g0[k].norm())
            num, den = num + float((g1[k] - g0[k]).norm()) ** 2, den + n0 ** 2
            if n0 > 0:
                e = float((g1[k] - g0[k]).norm()) / n0
                if e > worst[0]:
                    worst = (e, k)
            else:
                assert float(g1[k].norm()) == 0, k
        whole = (num / den) ** 0.5
        record_margin(f"prune_dead_T{frames}_B{batch}_rc{recompute}_{'injected' if injected == 0 else 'device'}", worst_grad_rel=worst[0], worst_tensor=worst[1],
                      whole_grad_rel=whole, loss_rel=max(abs(x0 - x1) / abs(x0) for x0, x1 in zip(l0, l1)))
        assert worst[0] < PRUNE_REL and whole < PRUNE_WHOLE_REL, (worst, whole)


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_batched_reduces_give_the_same_gradients(which):
    """EngineOptions.batch_reduce (round 6, default on): the parameter-gradient reduces of a stack's LayerNorm backwards and the value thirds of its qkv
    bias gradients run as ONE launch each at the end of the stack's backward, from per-call slab workspaces, instead of ~100 small launches inside it.
    The data path is untouched (the same kernels write the same dx), so against the same model with batch_reduce=False - same weights, inputs, plan -
    the losses are bitwise equal and EVERY gradient tensor agrees to the order of its fp32 atomics: 1e-5 of its norm (measured 2.7e-7 / 4.5e-7), including the
    tensors the batches form (LayerNorm affines, proj / fc2 biases from the fused column sums, the qkv bias value thirds).  Two backwards per model: the
    table built by the first one is reused by the second."""
    from avsiam_amd.config import EngineOptions
    from avsiam_amd.engine import Stack
    from avsiam_amd.models import CAVMAE_BASE
    mae = which == "mae"
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    B = 3 if mae else 5
    a, v = synth_inputs(cfg, B, 41)
    gen = torch.Generator().manual_seed(14)
    import random
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(11))
    res = {}
    for batch in (False, True):
        m = CAVMAE_BASE(cfg=cfg, init_seed=78, init_mode="random", verbose=False, plan_seed=5, options=EngineOptions(batch_reduce=batch)).cuda()
        for rep in range(2):
            for p in m._params.values():
                p.grad = None
            out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 0.01, mask_plan=plan)
            out[0].backward()
            torch.cuda.synchronize()
        eng = m._engine(which, B)
        stacks = [st for st in vars(eng).values() if isinstance(st, Stack) and (st._ln_batch is not None or st._vm_batch is not None)]   # (None until a backward builds them)
        assert bool(stacks) == batch, (batch, len(stacks))          # the batches exist exactly when the option is on
        res[batch] = (out[0].item(), {k: p.grad.detach().double().cpu() for k, p in m._params.items() if p.grad is not None})
    (l0, g0), (l1, g1) = res[False], res[True]
    assert l0 == l1
    assert g0.keys() == g1.keys() and len(g0) > 100
    worst = (0.0, None)
    for k in g0:
        n0 = float(g0[k].norm())
        if n0 == 0:
            assert float(g1[k].norm()) == 0, k
            continue
        e = float((g1[k] - g0[k]).norm()) / n0
        if e > worst[0]:
            worst = (e, k)
    record_margin(f"batch_reduce_{which}", worst_grad_rel=worst[0], worst_tensor=worst[1])
    assert worst[0] < 1e-5, worst


@pytest.mark.parametrize("ln_rpw", [16, 4])
def test_batched_reduce_refuses_a_changed_ln_rpw(ln_rpw):
    """The batched LayerNorm reduce of a stack holds the slab count of every workspace as the library's ln_rpw knob gave it at the first backward
    (automatic: 8 rows per wave at these row counts).  Under 16 the kernels write half as many slabs and the one reduce would add stale ones; under 4
    twice as many, more than the workspaces hold.  A backward under a changed knob raises before the stack queues a kernel or claims a gradient
    epoch, and with the knob restored the same model gives the first backward's gradients again: every tensor to 1e-5 of its norm, the order of the
    fp32 atomics (test_batched_reduces_give_the_same_gradients: measured 2.7e-7 / 4.5e-7)."""
    import random
    from avsiam_amd import _lib
    from avsiam_amd.models import CAVMAE_BASE
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    B = 5
    a, v = synth_inputs(cfg, B, 41)
    gen = torch.Generator().manual_seed(14)
    plan = make_contrastive_plan(cfg, B, gen, random.Random(11))
    m = CAVMAE_BASE(cfg=cfg, init_seed=78, init_mode="random", verbose=False, plan_seed=5).cuda()

    def forward():
        for p in m._params.values():
            p.grad = None
        return m(a.cuda(), v.cuda(), mae_loss_weight=0, contrast_loss_weight=0.01, mask_plan=plan)[0]

    def grads():
        torch.cuda.synchronize()
        return {k: p.grad.detach().double().cpu() for k, p in m._params.items() if p.grad is not None}

    forward().backward()
    g0 = grads()
    assert m._engine("contrastive", B).stack._ln_batch is not None and len(g0) > 100
    try:
        _lib.tuning_set("ln_rpw", ln_rpw)
        loss = forward()
        with pytest.raises(RuntimeError, match="ln_rpw"):
            loss.backward()
    finally:
        _lib.tuning_set("ln_rpw", 0)
    forward().backward()
    g1 = grads()
    assert g0.keys() == g1.keys()
    worst = (0.0, None)
    for k in g0:
        n0 = float(g0[k].norm())
        if n0 == 0:
            assert float(g1[k].norm()) == 0, k
            continue
        e = float((g1[k] - g0[k]).norm()) / n0
        if e > worst[0]:
            worst = (e, k)
    print(f"ln_rpw {ln_rpw}: worst gradient tensor after recovery {worst}")
    assert worst[0] < 1e-5, worst


def test_bf16_and_fp8_models_live_side_by_side():
    """Precision is a property of the MODEL (config.EngineOptions): a bf16 model and an fp8 mode-3 model are held alive in one
    process and stepped ALTERNATELY - both forwards, then both backwards - and each keeps its own results: the bf16 model reproduces what it
    computes ALONE (losses bitwise - the forward has no atomics - and every gradient tensor to the order of the fp32 atomics) and its parity against
    the oracle; the fp8 model holds the fp8 tolerances against the oracle on the calibration step and on the step after it.  With the process-wide
    switch of rounds 3 - 5 the mode set last decided the kernels of every model built afterwards."""
    import random
    from avsiam_amd.engine import Stack
    from avsiam_amd.engine_fp8 import Fp8Stack
    from avsiam_amd.models import CAVMAE_BASE
    cfg = AVSiamConfig(audio_tokens=128, frames=2)
    B = 3
    a, v = synth_inputs(cfg, B, 41)
    gen = torch.Generator().manual_seed(9)
    plans = {"mae": make_mae_plan(cfg, B, gen), "contrastive": make_contrastive_plan(cfg, B, gen, random.Random(9))}
    refs = {which: _oracle(cfg, a, v, plan, which == "mae", 93) for which, plan in plans.items()}

    def run(m, which):
        mae = which == "mae"
        for p in m._params.values():
            p.grad = None
        return m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plans[which])

    m16 = CAVMAE_BASE(cfg=cfg, init_seed=93, init_mode="random", verbose=False, fp8_mode="0").cuda()
    solo = {}
    for which in plans:                                              # the bf16 model on its own, before any fp8 model exists
        out = run(m16, which)
        out[0].backward()
        torch.cuda.synchronize()
        solo[which] = ([out[i].item() for i in range(5)], {k: p.grad.detach().double().cpu() for k, p in m16._params.items() if p.grad is not None})
    m8 = CAVMAE_BASE(cfg=cfg, init_seed=93, init_mode="random", verbose=False, fp8_mode="3").cuda()
    assert m16.options is not m8.options and (m16.options.fp8, m8.options.fp8) == ("0", "3")
    for step in (0, 1):
        for which in plans:
            ref, extras, rgrads = refs[which]
            outs = {name: run(m, which) for name, m in (("bf16", m16), ("fp8", m8))}        # both forwards first, then both backwards
            for name in ("fp8", "bf16"):
                outs[name][0].backward()
            torch.cuda.synchronize()
            # the bf16 model is not disturbed by its neighbour
            assert [outs["bf16"][i].item() for i in range(5)] == solo[which][0], (which, step)
            worst = 0.0
            for k, g0 in solo[which][1].items():
                g1 = m16._params[k].grad.detach().double().cpu()
                if float(g0.norm()) > 0:
                    worst = max(worst, float((g1 - g0).norm() / g0.norm()))
            record_margin(f"coexist_bf16_{which}", solo_vs_coexisting_grad_rel=worst)
            assert worst < 1e-5, (which, step, worst)
            for name, ltol in (("bf16", LOSS_RTOL), ("fp8", FP8_LOSS_RTOL)):
                for i in (0, 1, 2, 3, 4):
                    if ref[i].item() != 0:
                        assert abs(outs[name][i].item() - ref[i].item()) <= ltol * abs(ref[i].item()), (name, which, step, i, outs[name][i].item(), ref[i].item())
            # (bf16 against the oracle at this batch of 3: the fc2 bias gradients of the last two blocks measure cosine 0.99954 in the contrastive pass -
            #  3 x 3 logits at tau = 0.05; every other case of this file holds 0.9998)
            _compare_grads(m16, rgrads, cos_min=0.9986, ratio_tol=0.025, tag=f"coexist_bf16_{which}_step{step}")
            _compare_grads(m8, rgrads, cos_min=FP8BW_TOL[("vit_base", which)][0], ratio_tol=FP8BW_TOL[("vit_base", which)][1], tag=f"coexist_fp8m3_{which}_step{step}",
                           whole_cos_min=FP8W_WHOLE_COS, matrix_cos_min=FP8W_MATRIX_COS_MIN)
    eng16, eng8 = m16._engine("contrastive", B), m8._engine("contrastive", B)
    assert not eng16.stack.fp8 and eng8.stack.fp8_wgrad
    # the bf16 model's stacks are the plain engine.Stack - no 8-bit state at all; the fp8 modes live in the subclass
    stacks16 = [eng16.stack] + [st for st in vars(m16._engine("mae", B)).values() if isinstance(st, Stack)]
    assert len(stacks16) >= 4 and all(type(st) is Stack and not hasattr(st, "f8") for st in stacks16)
    assert isinstance(eng8.stack, Fp8Stack) and isinstance(eng8.stack, Stack)
    assert m8.fp8_saturation_events() == 0 and m16.fp8_state() == {}
    # a structural option can be changed on a live model: the engines are rebuilt, the other model is untouched
    m16.set_options(fp8="1")
    out = run(m16, "mae")
    assert m16._engine("mae", B).st_dec.fp8 and not m16._engine("mae", B).st_dec.fp8_bwd and m8.options.fp8 == "3"
    assert isinstance(m16._engine("mae", B).st_dec, Fp8Stack)
    assert abs(out[0].item() - refs["mae"][0][0].item()) <= FP8_LOSS_RTOL * abs(refs["mae"][0][0].item())


@pytest.mark.parametrize("which", ["mae", "contrastive"])
def test_vit_huge14_geometry_matches_oracle(which):
    """BASELINE.json configs[4]'s geometry: 14 x 14 patches (256 tokens per 224 x 224 frame, 9 x 73 = 657 audio tokens from a 1022 x 126
    spectrogram corner) as a patch STRIDE of 14 on 16 x 16 patch storage (config.stride), ViT-H width (heads of 80), 2 layers deep at
    batch 2 x 2 frames, against the oracle - which convolves with the 14 x 14 corner of the stored kernels and scores the 14 x 14 corner of
    every prediction row."""
    from avsiam_amd.config import vit_huge14
    import random
    cfg = vit_huge14(frames=2, depth=2)
    assert (cfg.video_tokens, cfg.audio_tokens, cfg.audio_len, cfg.n_mels) == (256, 657, 1022, 126)
    B = 2
    a, v = synth_inputs(cfg, B, 31)
    gen = torch.Generator().manual_seed(5)
    mae = which == "mae"
    plan = make_mae_plan(cfg, B, gen) if mae else make_contrastive_plan(cfg, B, gen, random.Random(5))
    m = _model(cfg, 95)
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
    out[0].backward()
    ref, extras, rgrads = _oracle(cfg, a, v, plan, mae, 95)
    for i in (0, 1, 2, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    _compare_grads(m, rgrads, cos_min=0.9998, ratio_tol=0.02, tag=f"vit_huge14_{which}")
    # the dead corner of the stored patch kernels never receives a gradient
    g = m._params["vit_base.patch_embed.proj.weight"].grad
    assert g is not None and float(g[..., 14:, :].abs().max()) == 0 and float(g[..., :, 14:].abs().max()) == 0


def test_vit_huge14_device_drawn_plan():
    """The default path (plans drawn on the device) at the 14 x 14 geometry: 657- and 256-token sequences through the mask-plan kernel,
    the contrastive pass's structured time masks over 73 time patches (bits 64.. travel in the sequence descriptor), read back and fed to
    the oracle."""
    from avsiam_amd.config import vit_huge14
    from avsiam_amd.models import CAVMAE_BASE
    cfg = vit_huge14(frames=1, depth=1)
    B = 6
    a, v = synth_inputs(cfg, B, 37)
    m = CAVMAE_BASE(cfg=cfg, init_seed=94, init_mode="random", verbose=False, plan_seed=321).cuda()
    out = m(a.cuda(), v.cuda(), mae_loss_weight=0, contrast_loss_weight=1)
    out[0].backward()
    plan = m.last_plans(B)["contrastive"]
    ref, extras, rgrads = _oracle(cfg, a, v, plan, False, 94)
    for i in (0, 3, 4):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())
    # structured masking removes whole time columns - also columns 64..72
    t = cfg.audio_t
    late = False
    for _ in range(3):
        for keep in m.last_plans(B)["contrastive"].a_keep:
            if keep.numel() < cfg.audio_tokens:
                cols = torch.zeros(t, dtype=torch.bool)
                cols[(keep % t).unique()] = True
                late = late or bool((~cols[64:]).any())
        m(a.cuda(), v.cuda(), mae_loss_weight=0, contrast_loss_weight=1)
    assert late
    out = m(a.cuda(), v.cuda(), mae_loss_weight=1, contrast_loss_weight=0)
    out[0].backward()
    plan = m.last_plans(B)["mae"]
    ref, extras, rgrads = _oracle(cfg, a, v, plan, True, 94)
    for i in (0, 1, 2):
        assert abs(out[i].item() - ref[i].item()) <= LOSS_RTOL * abs(ref[i].item()) + 1e-6, (i, out[i].item(), ref[i].item())


# ViT-H/14 at its FULL DEPTH (32 encoder layers per tower + 2 joint + 8 decoder; 1.33 G parameters), batch 2 x 1 frame, both passes,
# against the oracle - in bf16 and in fp8 mode 3 (round 5).  What depth adds over the 2- and 4-layer cases above: the bf16
# residual-GRADIENT stream rounds 2 x depth times along a stack, and the fp8 operands' rounding accumulates
# over 32 blocks in the forward and again in the backward.  Tolerances at ~3x the measurement (profiles/r05/parity_margins.json,
# vit_huge14_depth32_*): stated next to each assert.
D32_BF16_COS_MIN, D32_BF16_RATIO_TOL = 0.9995, 0.03        # measured: worst tensor 0.99984 (a 1280-element LayerNorm bias), norm 1.1 %
D32_FP8_LOSS_RTOL, D32_FP8_LOGITS_ATOL = 7e-3, 0.14         # measured: 2.2e-3, 0.045
# fp8 mode 3 at depth 32, batch 2 (measured, profiles/r05/parity_margins.json vit_huge14_depth32_*_fp8m3_*):
#   whole gradient            cosine 0.9886 (contrastive, batch 5) / 0.9929 (MAE)             -> >= 0.97
#   every MATRIX              cosine >= 0.974 (contrastive) / 0.979 (MAE), norm within 4 %    -> >= 0.92, within 12 %
#   the vector tensors, taken together as one vector      cosine 0.989 / 0.992                -> >= 0.97
#   a single vector tensor    D32_FP8_VEC below (round 5 ran the contrastive pass at batch 2, where a 1280-element bias of the LAST block was mostly
#                             noise - cosine 0.70, 1.6 x the norm - and could only be held to 0.35 / a factor 2.2)
D32_FP8_MATRIX_COS_MIN, D32_FP8_MATRIX_RATIO_TOL, D32_FP8_WHOLE_COS, D32_FP8_VECTORS_COS = 0.92, 0.12, 0.97, 0.97
# round 6: every single VECTOR tensor (1280-element biases / LayerNorm vectors) gets a bound of its own, per pass, at <= 3x the measured
# gap (parity_margins.json vit_huge14_depth32_*_fp8m3_*): (cosine floor, norm ratio tolerance).  The contrastive pass runs at batch 5 for that.
D32_CONTRASTIVE_BATCH = 5
D32_FP8_VEC = {"mae": (0.93, 0.15), "contrastive": (0.86, 0.18)}         # measured: MAE 0.976 / 4.6 % (blocks.0.norm2_v.weight), contrastive at batch 5: 0.952 / 6.0 %
                                                                         # (blocks.31.mlp.fc1.bias; 0.70 / 62 % at batch 2).  Oracle wall time: 16 s on the box's 16 cores


def test_vit_huge14_depth32_matches_oracle_in_bf16_and_fp8_mode3():
    import gc
    import random
    import time
    from avsiam_amd.config import vit_huge14
    from avsiam_amd.models import CAVMAE_HUGE
    from oracle import ref_cpu
    cfg = vit_huge14(frames=1)
    assert cfg.depth == 32 and cfg.embed_dim == 1280 and cfg.head_dim == 80
    # the MAE pass at batch 2; the contrastive pass at batch D32_CONTRASTIVE_BATCH (one clip per mask-ratio group, 5 x 5 logits): at batch 2 its 2 x 2
    # logits leave a single 1280-element bias gradient mostly noise in fp8 (cosine 0.70 - round 5), which no per-tensor bound can be built on
    batches = {"mae": 2, "contrastive": D32_CONTRASTIVE_BATCH}
    gen = torch.Generator().manual_seed(10)
    data = {w: synth_inputs(cfg, B, 43) for w, B in batches.items()}
    plans = {"mae": make_mae_plan(cfg, batches["mae"], gen), "contrastive": make_contrastive_plan(cfg, batches["contrastive"], gen, random.Random(10))}
    m = CAVMAE_HUGE(cfg=cfg, init_seed=91, init_mode="random", verbose=False).cuda()       # (the 1.3 G-parameter synthesis: once)
    live = [info.name for info in build_spec(cfg) if info.live]
    torch.set_num_threads(16)
    refs = {}
    t0 = time.time()
    for which, plan in plans.items():
        mae = which == "mae"
        a, v = data[which]
        P = {k: m._params[k].detach().cpu().clone().requires_grad_(True) for k in live}
        extras = {}
        out = ref_cpu.forward(P, cfg, a, v, plan, mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, extras=extras)
        out[0].backward()
        refs[which] = ([float(o.item()) for o in out[:5]], extras.get("logits"), {k: p.grad for k, p in P.items()})
        del P, out
        gc.collect()
    record_margin("vit_huge14_depth32_oracle", wall_seconds=time.time() - t0, batches=str(batches))
    try:
        for mode in ("0", "3"):
            m.set_options(fp8=mode)                      # a structural option: the pass engines are rebuilt for the mode
            for which, plan in plans.items():
                mae = which == "mae"
                a, v = data[which]
                B = batches[which]
                ref, logits, rgrads = refs[which]
                for step in ((0,) if mode == "0" else (0, 1)):       # fp8: the calibration step and the step on delayed scales
                    for p in m._params.values():                     # (.grad views of the arena outlive a pass: the other pass's are not this one's)
                        p.grad = None
                    out = m(a.cuda(), v.cuda(), mae_loss_weight=1 if mae else 0, contrast_loss_weight=0 if mae else 1, mask_plan=plan)
                    out[0].backward()
                    torch.cuda.synchronize()
                    tag = f"vit_huge14_depth32_{which}_{'bf16' if mode == '0' else 'fp8m3_step%d' % step}"
                    worst_loss = max(abs(out[i].item() - ref[i]) / abs(ref[i]) for i in (0, 1, 2, 3, 4) if ref[i] != 0)
                    record_margin(tag, loss_rel=worst_loss)
                    assert worst_loss <= (LOSS_RTOL if mode == "0" else D32_FP8_LOSS_RTOL), (tag, [out[i].item() for i in range(5)], ref)
                    if not mae:
                        err = float((m._engine("contrastive", B).total.detach().cpu().double() - logits.detach().double()).abs().max())
                        record_margin(tag, logits_abs=err)
                        assert err <= (LOGITS_ATOL if mode == "0" else D32_FP8_LOGITS_ATOL), (tag, err)
                    if mode == "0":
                        _compare_grads(m, rgrads, cos_min=D32_BF16_COS_MIN, ratio_tol=D32_BF16_RATIO_TOL, tag=tag)
                    else:
                        cmin, rtol = D32_FP8_VEC[which]
                        _compare_grads(m, rgrads, cos_min=cmin, ratio_tol=rtol, tag=tag, whole_cos_min=D32_FP8_WHOLE_COS,
                                       matrix_cos_min=D32_FP8_MATRIX_COS_MIN, matrix_ratio_tol=D32_FP8_MATRIX_RATIO_TOL,
                                       vectors_cos_min=D32_FP8_VECTORS_COS)
            if mode == "3":
                assert m.fp8_saturation_events() == 0
    finally:
        del m
        gc.collect(); torch.cuda.empty_cache()
