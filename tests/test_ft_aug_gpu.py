"""Fine-tuning augmentation where the input is read (SpecAugment masks, noise, time roll: avs_ft_aug_draw, avs_im2col_audio_aug,
avs_augment_audio; dataloader_ft.py:527-548) on a real MI355X: the fused gather against the two-pass form bit for bit, the two-pass form against
a float64 torch restatement in the reference's order (mask on the raw tensor, normalise, add noise, roll), the device draw against its numpy
restatement bit for bit, and the model: train_step / forward with ``aug=`` / ``input_xf=`` against the same calls on separately prepared tensors.

Bounds.  Kernel against kernel: equality of bits.  Two-pass against float64: masked cells exactly fma(amp, u, fill) (evaluated in 80-bit
arithmetic, where the 48-bit product plus the 24-bit fill is exact, then rounded once); unmasked cells within 1e-5 absolute - values reach
|x| ~ 4 (ulp 4.8e-7) and the kernel multiplies by fp32(1 / std) where float64 divides (2 ulp), the bound test_elementwise_gpu.py uses for the
same arithmetic.  Model: the fused and the two-pass step run the same kernels on the same bf16 patch rows; the backward has float atomics, so
gradients are compared with the bounds of tests/test_ft_train_gpu.py (cosine >= 0.9998, norm within 1 %), the forward-only loss with its 1e-4.
Raw inputs in the inference modes: the logit bounds of tests/test_ft_gpu.py (cosine >= 0.9999, |error| <= 0.03).

Library calls of a plain step (aug=None, input_xf=None) must be what they were before this feature existed: see
test_plain_step_issues_the_calls_it_issued_before."""
import types

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
BIG = 1.0e4
MEAN, STD = -5.081, 4.4849
GRAD_COS, GRAD_NORM, LOSS_REL = 0.9998, 1e-2, 1e-4
LOGIT_ABS, LOGIT_COS = 0.03, 0.9999


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def pp():
    from avsiam_amd import preprocess
    return preprocess


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. kernels
B4 = 4
NOISE_SEED = 0x1234ABCD00C0FFEE


def _plan_arrays(S):
    T, F = 3 * S, 2 * S
    #            no aug | masks across a patch boundary, negative odd shift | masks to the ends (all frames), shift >= T | length-1 masks at 0 and last
    return dict(f0=[0, S - 3, F - 5, 0], fn=[0, 7, 5, 1], t0=[0, S - 2, 0, T - 1], tn=[0, S + 5, T, 1], shift=[0, -7, T + 5, 0], amp=[0.0, 0.07, 0.03, 0.0])


@pytest.fixture(scope="module", params=[16, 14])
def kernel_case(request):
    """inputs, plan, row subset and the two-pass outputs of one stride: computed once, shared, never modified"""
    o = ops()
    S = request.param
    T, F = 3 * S, 2 * S
    g = torch.Generator(device=DEV).manual_seed(70 + S)
    buf = torch.randn(B4 + 1, T, F, device=DEV, generator=g) * 4 - 5
    buf[B4] = BIG                                                    # behind the last valid sample: a read past the end shows
    fb = buf[:B4]
    norm = (torch.randn(B4 + 1, T, F, device=DEV, generator=g))
    norm[B4] = BIG
    pa = _plan_arrays(S)
    plan = o.FtAug.from_arrays(pa["f0"], pa["fn"], pa["t0"], pa["tn"], pa["shift"], pa["amp"], seed=NOISE_SEED, device=DEV, fill=1.25)
    L = 6
    pick = torch.randperm(B4 * L, device=DEV, generator=g)[:(B4 * L * 3) // 5]
    # every sample keeps at least one row
    pick = torch.cat([pick, torch.arange(B4, device=DEV) * L + 1]).unique()
    pick = pick[torch.randperm(pick.numel(), device=DEV, generator=g)]
    row_b, row_tok, rows = (pick // L).int(), (pick % L).int(), pick.numel()
    two = {}
    for kind, src in ((1, fb), (0, norm[:B4])):
        out = torch.full((B4 + 1, T, F), SENT, device=DEV)
        o.augment_audio(src, out[:B4], plan, kind, MEAN, STD)
        assert bool((out[B4] == SENT).all()), "augment_audio wrote beyond its B samples"
        two[kind] = out[:B4].clone()
    torch.cuda.synchronize()
    return types.SimpleNamespace(S=S, T=T, F=F, fb=fb, norm=norm[:B4], pa=pa, plan=plan, row_b=row_b, row_tok=row_tok, rows=rows, two=two, tP=3)


def _gather(c, a, **kw):
    o = ops()
    out = torch.full(((c.rows + 2) * 256,), SENT, dtype=torch.bfloat16, device=DEV).reshape(c.rows + 2, 256)
    o.im2col_audio(a, c.row_b, c.row_tok, out, c.rows, c.tP, stride=c.S, **kw)
    assert bool((out[c.rows:] == SENT).all()), "the gather wrote beyond its rows"
    return out[:c.rows]


def test_fused_gather_equals_gather_of_the_two_pass_tensor(kernel_case):
    c, o = kernel_case, ops()
    xa = o.InputXf.audio(MEAN, STD)
    fused1 = _gather(c, c.fb, xf=xa, aug=c.plan)                      # kind 1: raw fbank
    assert same_bits(fused1, _gather(c, c.two[1]))
    fused0 = _gather(c, c.norm, aug=c.plan)                           # kind 0: normalised input, explicit fill
    assert same_bits(fused0, _gather(c, c.two[0]))
    assert not same_bits(fused1, fused0)
    # (b) sample 0 (no masks, no shift, no noise): today's raw-input path, bit for bit
    today = _gather(c, c.fb, xf=xa)
    s0 = c.row_b == 0
    assert int(s0.sum()) > 0 and same_bits(fused1[s0], today[s0])
    assert not same_bits(fused1[~s0], today[~s0])
    # outside the S x S corner the rows are zero, as in the plain gather
    corner = torch.zeros(16, 16, dtype=torch.bool, device=DEV)
    corner[:c.S, :c.S] = True
    assert bool((fused1[:, ~corner.reshape(-1)] == 0).all())


def test_no_masks_is_todays_noise_and_roll_bit_for_bit(kernel_case):
    """every mask length 0: avs_input_xf kind 1 with the same shift / amp / seed - gather and two-pass tensor"""
    c, o = kernel_case, ops()
    z = [0] * B4
    shift, amp = [0, -7, c.T + 5, 3], [0.0, 0.07, 0.03, 0.09]
    plan = o.FtAug.from_arrays(z, z, z, z, shift, amp, seed=NOISE_SEED, device=DEV)
    sh, am = torch.tensor(shift, dtype=torch.int32, device=DEV), torch.tensor(amp, dtype=torch.float32, device=DEV)
    xf = o.InputXf.audio(MEAN, STD, sh, am, seed=NOISE_SEED)
    assert same_bits(_gather(c, c.fb, xf=o.InputXf.audio(MEAN, STD), aug=plan), _gather(c, c.fb, xf=xf))
    two = pp().augment_fbank(c.fb, plan, MEAN, STD)
    assert same_bits(two, pp().normalize_fbank(c.fb, MEAN, STD, noise=True, seed=NOISE_SEED, shift=sh, amp=am))
    # a plan shorter than the batch: the samples beyond it are not augmented
    short = o.FtAug.from_arrays(z[:2], z[:2], z[:2], z[:2], shift[:2], amp[:2], seed=NOISE_SEED, device=DEV)
    got = pp().augment_fbank(c.fb, short, MEAN, STD)
    assert same_bits(got[:2], two[:2]) and same_bits(got[2:], pp().normalize_fbank(c.fb, MEAN, STD)[2:])


@pytest.mark.parametrize("kind", [1, 0])
def test_two_pass_against_float64_restatement(kernel_case, kind):
    """mask on the raw tensor (value 0.0 / the fill), normalise, add noise, torch.roll - in float64"""
    c = kernel_case
    T, F, pa = c.T, c.F, c.pa
    src = (c.fb if kind == 1 else c.norm).double().cpu()
    two = c.two[kind].cpu()
    u = torch.from_numpy(pp().noise_reference(NOISE_SEED, B4, T, F))                        # fp32, un-rolled frame index
    inv_std = np.float32(1.0) / np.float32(STD)
    fill = float((np.float32(0.0) - np.float32(MEAN)) * inv_std) if kind == 1 else c.plan.fill
    worst = 0.0
    for b in range(B4):
        masked = torch.zeros(T, F, dtype=torch.bool)
        masked[pa["t0"][b]:pa["t0"][b] + pa["tn"][b], :] = True
        masked[:, pa["f0"][b]:pa["f0"][b] + pa["fn"][b]] = True
        amp = np.float32(pa["amp"][b])
        if kind == 1:
            x = src[b].clone()
            x[masked] = 0.0                                                                   # FrequencyMasking / TimeMasking, mask value 0
            y = (x - MEAN) / STD
        else:
            y = src[b].clone()
            y[masked] = fill
        y = y + float(amp) * u[b].double()
        y = torch.roll(y, pa["shift"][b], 0)
        rolled_mask = torch.roll(masked, pa["shift"][b], 0)
        # masked cells: fill + noise, exactly (one rounding of the exact sum)
        exact = (np.longdouble(fill) + np.longdouble(amp) * u[b].numpy().astype(np.longdouble)).astype(np.float32)
        exact = torch.roll(torch.from_numpy(exact), pa["shift"][b], 0)
        assert same_bits(two[b][rolled_mask], exact[rolled_mask]), (kind, b)
        if b == 2:
            assert bool(rolled_mask.all())                                                    # t0 = 0, tn = T: everything masked
        if b == 3:
            assert int(masked.sum()) == T + F - 1                                             # one frame and one bin
        d = (two[b].double() - y)[~rolled_mask]
        if d.numel():
            worst = max(worst, float(d.abs().max()))
            assert float(d.abs().max()) <= 1e-5, (kind, b, float(d.abs().max()))
        # the way test_mae_loss_raw_inputs_fused_equals_two_pass bounds it: against the noise-free formula, the noise in [0, amp)
        if kind == 1:
            base = torch.roll((src[b] - MEAN) / STD, pa["shift"][b], 0)
            dn = (two[b].double() - base)[~rolled_mask]
            if dn.numel():
                assert float(dn.min()) >= -1e-5 and float(dn.max()) < float(amp) + 1e-5, (b, float(dn.min()), float(dn.max()))
    print(f"ft_aug two-pass vs float64 (stride {c.S}, kind {kind}): worst |error| on unmasked cells {worst:.3e}")
    from tests.helpers import record_margin
    record_margin(f"ft_aug.two_pass_vs_f64.S{c.S}.kind{kind}", worst_abs=worst)


def test_wrappers_refuse_what_the_kernels_would_refuse(kernel_case):
    c, o = kernel_case, ops()
    from avsiam_amd import _lib
    sh, am = torch.zeros(B4, dtype=torch.int32, device=DEV), torch.zeros(B4, dtype=torch.float32, device=DEV)
    keep = c.two[1].clone()
    for bad in (lambda: _gather(c, c.fb, xf=o.InputXf.audio(MEAN, 0.0), aug=c.plan),                      # zero std
                lambda: _gather(c, c.fb, xf=o.InputXf.frames(), aug=c.plan),                              # a frame transform beside audio
                lambda: _gather(c, c.fb, xf=o.InputXf.audio(MEAN, STD, sh, am), aug=c.plan),              # two sources of shift / amp
                lambda: _gather(c, c.fb, aug=(1, 2)),
                lambda: o.augment_audio(c.fb, c.two[1], c.plan, 2, MEAN, STD),                            # kind 2
                lambda: o.augment_audio(c.fb, c.fb, c.plan, 1, MEAN, STD)):                               # in place
        with pytest.raises(_lib.AvsiamHipError):
            bad()
    torch.cuda.synchronize()
    assert same_bits(keep, c.two[1])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the draw
@pytest.mark.parametrize("B", [1, 5, 300])
def test_device_draw_equals_the_numpy_restatement(B):
    o = ops()
    key = (0x9E3779B9 << 32) | 0x00000007
    T, F, freqm, timem = 1024, 128, 48, 192
    st = o.FtAugState(DEV, key, counter=41)
    buf = torch.full((o.FtAug.HDR + o.FtAug.REC * B + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    plans = []
    for k in range(2):
        plan = o.FtAug.draw(st, B, T, F, freqm, timem, True, out=o.FtAug(buf, B))
        got = plan.arrays()
        assert bool((buf[o.FtAug.HDR + o.FtAug.REC * B:] == 0x5A5A5A5A).all()), "the draw wrote beyond its B records"
        want = pp().draw_plan_reference(key, 41 + k, B, T, F, freqm, timem, True)
        for f in ("f0", "fn", "t0", "tn", "shift"):
            assert np.array_equal(got[f], want[f]), (B, k, f)
        assert np.array_equal(got["amp"].view(np.int32), want["amp"].view(np.int32)), (B, k)
        assert got["noise_key"] == want["noise_key"] and got["counter"] == 41 + k and got["n"] == B
        assert st.counter() == 42 + k                                                  # advanced by exactly one per draw
        plans.append(got)
    assert not np.array_equal(plans[0]["amp"], plans[1]["amp"]) and plans[0]["noise_key"] != plans[1]["noise_key"]
    if B > 1:
        assert not np.array_equal(plans[0]["t0"], plans[1]["t0"])
    # the switches: parameter 0 gives length 0; noise off gives shift 0 and amp 0
    got = o.FtAug.draw(st, B, T, F, 0, timem, False).arrays()
    want = pp().draw_plan_reference(key, 43, B, T, F, 0, timem, False)
    assert not got["fn"].any() and not got["f0"].any() and not got["shift"].any() and not got["amp"].any()
    assert np.array_equal(got["tn"], want["tn"]) and np.array_equal(got["t0"], want["t0"]) and st.counter() == 44


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the model
LBL, MB = 7, 3
CFG = AVSiamConfig(depth=2)


@pytest.fixture(scope="module")
def model_case():
    from avsiam_amd.models import CAVMAEFT_BASE
    o = ops()
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()
    a, v = synth_inputs(CFG, MB, 61)
    fb = (a * STD + MEAN).cuda()
    v8 = (v * 0.25 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8).unsqueeze(1).cuda()
    g = torch.Generator().manual_seed(3)
    hot = (torch.rand(MB, LBL, generator=g) < 0.3).float()
    hot[:, 0] = 1.0
    y = (hot * 0.9 + 0.1 / LBL).cuda()
    T, F = CFG.audio_len, CFG.n_mels
    plan = o.FtAug.from_arrays([0, 13, F - 48], [0, 40, 48], [0, 500, 0], [0, 191, 100], [0, -333, T + 17], [0.0, 0.08, 0.05], seed=NOISE_SEED, device=DEV)
    xf = (o.InputXf.audio(MEAN, STD), o.InputXf.frames())
    two = pp().augment_fbank(fb, plan, MEAN, STD)
    vn = pp().normalize_frames(v8)
    return types.SimpleNamespace(m=m, fb=fb, v8=v8, y=y, plan=plan, xf=xf, two=two, vn=vn, a_norm=a.cuda())


def _step(c, ftmode, branch, a, v, **kw):
    """one train_step at lr 0 (the parameters stay) -> (loss, gradients, audio patch rows, frame patch rows)"""
    m = c.m
    loss = m.train_step(a, v, c.y, 0.0, ftmode, branch=branch, **kw)
    grads = {n: p.grad.clone() for n, p in m._params.items() if p.grad is not None}
    eng = m._train_engines[(MB, 1)]
    kind = {"audioonly": "a", "mm_a": "a", "mm_grad": "av"}[eng.state["mode"]]
    enc = eng._enc[kind]
    cols_a = enc.emb_a.cols[:enc.rows_a].clone()
    cols_v = enc.emb_v.cols[:enc.rows_v].clone() if enc.nv else None
    return float(loss), grads, cols_a, cols_v


@pytest.mark.parametrize("case", ["mm", "mm_a", "audioonly", "mm_freeze_base", "mm_normalised_input"])
def test_train_step_with_aug_equals_the_step_on_the_augmented_tensor(model_case, case):
    from avsiam_amd.traintest_ft_base import apply_freeze_base
    from tests.helpers import record_margin
    c = model_case
    ftmode, branch = ("audioonly", None) if case == "audioonly" else ("mm_grad", "a" if case == "mm_a" else "mm")
    apply_freeze_base(c.m, case == "mm_freeze_base")
    try:
        if case == "mm_normalised_input":                     # aug without input_xf: a normalised input, masked cells take plan.fill
            c.plan.fill = 1.133
            fused = _step(c, ftmode, branch, c.a_norm, c.vn, aug=c.plan)
            plain = _step(c, ftmode, branch, pp().augment_fbank(c.a_norm, c.plan, raw=False), c.vn)
        else:
            fused = _step(c, ftmode, branch, c.fb, c.v8, input_xf=c.xf, aug=c.plan)
            plain = _step(c, ftmode, branch, c.two, c.vn)
    finally:
        c.plan.fill = 0.0
        apply_freeze_base(c.m, False)
    assert same_bits(fused[2], plain[2]), "audio patch rows"
    if fused[3] is not None:
        assert same_bits(fused[3], plain[3]), "frame patch rows"
    unaug = _step(c, ftmode, branch, pp().normalize_fbank(c.fb, MEAN, STD) if case != "mm_normalised_input" else c.a_norm, c.vn)
    assert not same_bits(fused[2], unaug[2]), "the augmentation changed nothing"
    assert abs(fused[0] - plain[0]) <= LOSS_REL * abs(plain[0]), (case, fused[0], plain[0])
    assert set(fused[1]) == set(plain[1]) and len(fused[1]) > 0
    if case == "mm_freeze_base":
        from avsiam_amd.models.cav_mae_ft import param_group
        assert all(param_group(n) != "base" for n in fused[1])
    worst_cos, worst_norm = 1.0, 0.0
    for n, r in plain[1].items():
        g, r = fused[1][n].double().reshape(-1), r.double().reshape(-1)
        if float(r.norm()) == 0:
            assert float(g.norm()) == 0, (case, n)
            continue
        cos = float(g @ r / (g.norm() * r.norm()))
        nr = abs(float(g.norm() / r.norm()) - 1)
        worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, nr)
        assert cos >= GRAD_COS and nr <= GRAD_NORM, (case, n, cos, nr)
    print(f"ft_aug fused vs two-pass step ({case}): loss {fused[0]:.6f} / {plain[0]:.6f}, worst cosine {worst_cos:.8f}, worst norm error {worst_norm:.3e}")
    record_margin(f"ft_aug.fused_vs_two_pass_step.{case}", worst_cos=worst_cos, worst_norm=worst_norm, loss_rel=abs(fused[0] - plain[0]) / abs(plain[0]))


def test_autograd_path_takes_aug_too(model_case):
    """forward(..., aug=) through the autograd node: the same patch rows as the fused step, gradients delivered"""
    c = model_case
    c.m.requires_grad_(True)
    for p in c.m.parameters():
        p.grad = None
    out = c.m(c.fb, c.v8, "audioonly", input_xf=c.xf, aug=c.plan)
    eng = c.m._train_engines[(MB, 1)]
    cols = eng._enc["a"].emb_a.cols[:eng._enc["a"].rows_a].clone()
    torch.nn.functional.binary_cross_entropy_with_logits(out, c.y).backward()
    assert c.m._params["vit_base.patch_embed_a.proj.weight"].grad is not None
    for p in c.m.parameters():
        p.grad = None
    ref = _step(c, "audioonly", None, c.two, c.vn)
    assert same_bits(cols, ref[2])


def test_raw_inputs_in_the_inference_modes(model_case):
    """uint8 frames + un-normalised fbank through input_xf, inference: against the same call on the separately normalised tensors"""
    c = model_case
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()           # inference-only: no parameter requires a gradient
    v10 = torch.randint(0, 256, (MB, 10, 3, CFG.img_size, CFG.img_size), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    an, vn = pp().normalize_fbank(c.fb, MEAN, STD), pp().normalize_frames(v10)
    worst = (1.0, 0.0)
    for mode, kw in (("mm_grad", dict(is_eval=True)), ("videoonly", {}), ("audioonly", {}), ("retrieval", {})):
        with torch.no_grad():
            got = m(c.fb, v10, mode, input_xf=c.xf, **kw)
            ref = m(an, vn, mode, **kw)
        for gt, rf in zip(got if isinstance(got, tuple) else (got,), ref if isinstance(ref, tuple) else (ref,)):
            gt, rf = gt.double().reshape(-1, gt.shape[-1]), rf.double().reshape(-1, rf.shape[-1])
            cos = float(torch.nn.functional.cosine_similarity(gt, rf, dim=1).min())
            err = float((gt - rf).abs().max())
            worst = (min(worst[0], cos), max(worst[1], err))
            assert cos >= LOGIT_COS and err <= LOGIT_ABS, (mode, cos, err)
    print(f"ft_aug raw inputs, inference: worst cosine {worst[0]:.8f}, worst |error| {worst[1]:.3e}")
    from tests.helpers import record_margin
    record_margin("ft_aug.raw_inputs_inference", worst_cos=worst[0], worst_abs=worst[1])
    with pytest.raises(ValueError):
        m(c.fb, v10.float(), "videoonly", input_xf=c.xf)                              # float frames beside a uint8 transform
    # aug is a training augmentation: refused by a model without gradients, and by every is_eval form
    with pytest.raises(ValueError):
        m(c.fb, c.v8, "audioonly", input_xf=c.xf, aug=c.plan)
    c.m.requires_grad_(True)
    with pytest.raises(ValueError):
        c.m(c.fb, v10, "mm_grad", is_eval=True, input_xf=c.xf, aug=c.plan)
    with pytest.raises(ValueError):
        c.m(c.fb, c.v8, "audioonly", is_eval=True, aug=c.plan)
    with torch.no_grad(), pytest.raises(ValueError):
        c.m(c.fb, c.v8, "audioonly", aug=c.plan)
    with pytest.raises(ValueError):
        c.m(c.fb, v10, "retrieval", aug=c.plan)


# library calls of one fused step of a fresh CAVMAEFT_BASE(7, cfg=AVSiamConfig(depth=2)), batch 3, branch mm / a, the second step of the model (the
# first also builds the engine), counted through _lib.calls as tools/step_digest.py does - measured on a checkout of the commit before this feature
PARENT_CALLS = {"mm": 113, "a": 67}


def test_plain_step_issues_the_calls_it_issued_before(model_case):
    """aug=None, input_xf=None: the step's library calls are the parent commit's.  Parent counts (a checkout of the parent commit on the same
    machine, the same model, batch and counting): mm 113, a 67.  tools/step_digest.py --ft --trace --batch 3 (depth 12, deterministic mode)
    gave 301 calls in the step, 303 traced calls with list hash 21a456a12665402b..., loss 0.7534434199333191 and arena hash 2236841a6e97... on
    the parent commit and the very same on this one."""
    from avsiam_amd import _lib
    from avsiam_amd.models import CAVMAEFT_BASE
    c = model_case
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()       # fresh: the count includes the head refresh of every engine the model holds
    m.requires_grad_(True)
    for br in ("mm", "a"):
        m.train_step(c.two, c.vn, c.y, 0.0, "mm_grad", branch=br)
        c0 = _lib.calls
        m.train_step(c.two, c.vn, c.y, 0.0, "mm_grad", branch=br)
        n = _lib.calls - c0
        print(f"ft_aug plain step calls ({br}): {n}")
        assert n == PARENT_CALLS[br], (br, n, PARENT_CALLS[br])
        # the augmented step replaces one gather by another: the same count
        c0 = _lib.calls
        m.train_step(c.fb, c.v8, c.y, 0.0, "mm_grad", branch=br, input_xf=c.xf, aug=c.plan)
        assert _lib.calls - c0 == n, (br, _lib.calls - c0, n)


def test_training_draws_one_plan_per_step_and_validation_none(model_case, tmp_path):
    """train(): the draw counter advances by exactly one per training batch; validate() never touches it"""
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, train, validate
    c = model_case
    m = c.m
    m.set_aug_seed(1234)
    key = (1234 << 32) | 0
    assert m.aug_counter() == 0
    p0 = m.draw_aug(MB, 48, 192, True).arrays()
    p1 = m.draw_aug(MB, 48, 192, True).arrays()
    for k, got in ((0, p0), (1, p1)):
        want = pp().draw_plan_reference(key, k, MB, CFG.audio_len, CFG.n_mels, 48, 192, True)
        assert all(np.array_equal(got[f], want[f]) for f in ("f0", "fn", "t0", "tn", "shift")) and got["noise_key"] == want["noise_key"]
    assert m.aug_counter() == 2
    args = types.SimpleNamespace(ftmode="audioonly", ftmode_test=None, loss="BCE", lr=1e-5, head_lr=10.0, mm_lr=10.0, freeze_base=False, n_epochs=1,
                                 lr_adapt=False, lr_patience=1, lrscheduler_start=2, lrscheduler_step=1, lrscheduler_decay=0.5, metrics="mAP",
                                 exp_dir=str(tmp_path), save_model=False, n_print_steps=100, freqm=48, timem=192, noise=True, raw_input=True,
                                 dataset_mean=MEAN, dataset_std=STD)
    tr = SyntheticFtLoader(CFG, MB, 3, LBL, DEV, seed=5, raw=True)
    va = SyntheticFtLoader(CFG, MB, 2, LBL, DEV, seed=6, raw=True)
    assert tr.a.dtype == torch.float32 and tr.v.dtype == torch.uint8 and float(tr.a.mean()) < -4.0
    validate(m, va, None, args)
    assert m.aug_counter() == 2                                   # validation: no draw
    weights = m.arena.p.clone()
    res = train(m, tr, va, None, args)
    assert m.aug_counter() == 2 + 3                               # three training batches, one validation pass
    assert np.isfinite(res["result"][0, 3]) and not torch.equal(weights, m.arena.p)
    args.freqm, args.timem, args.noise = 0, 0, False
    train(m, tr, va, None, args)
    assert m.aug_counter() == 5                                   # nothing to draw: the plain step
    m.set_aug_seed(1234)
    assert m.aug_counter() == 0
