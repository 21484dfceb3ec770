"""The exact-fp32 forward on a real MI355X: its kernels against fp64 under bounds derived from their arithmetic (tests/exactlib.py), the fp32
patch gathers against a restatement and against the bf16 gathers, the fine-tuned model's inference modes with exact=True against the
reference's golden logits within EXACT_LOGIT_ABS, batch invariance and determinism bit for bit, the ViT-L / ViT-H skeletons against the CPU
oracle, the mode as a yardstick of the bf16 path, and the digest of a plain step (the default path did not move).
Every measured ratio goes through exactlib.record (tools/exact_margins.py writes them to profiles/r18/exact_margins.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_state_ft
from tests import exactlib as X
from tests import rowwise
from tests.helpers import FT_CASES, ft_case_inputs, ft_outputs_as_dict, load_golden, sample_positions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _wide(t, extra=8):
    """the tensor as a row view of a wider buffer (leading dimension = columns + extra), the pad filled with a sentinel"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), 7.0, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _run_gemm(c, M, kw, wide=True):
    from avsiam_amd import ops
    N = c["B"].shape[0]
    A = _wide(c["A"][:M]) if wide else c["A"][:M].to(DEV).contiguous()
    B = c["B"].to(DEV)
    res = kw["res"]
    if res is not None:
        res = _wide(res) if wide else res.to(DEV)
    buf, check = rowwise.guarded(M, N, torch.float32, DEV, extra_rows=130, extra_cols=8 if wide else 0)
    ops.gemm_nt_f32(A, B, buf[:, :N], M, bias=kw["bias"].to(DEV), res=res, res_idx=kw["res_idx"].to(DEV) if kw["res_idx"] is not None else None,
                    alpha=kw["alpha"], act=kw["act"])
    return check()


# ---- 1. GEMM ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_f32_under_bound(shape):
    M, N, K = shape
    c = X.gemm_case(M, N, K)
    for ep in X.GEMM_EPILOGUES:
        kw = X.gemm_args(c, ep)
        got = _run_gemm(c, M, kw).cpu()
        ref, bound = X.gemm_reference(c["A"], c["B"], **kw)
        ratio, at = rowwise.elem_ratio(got, ref, bound)
        print(f"gemm_nt_f32 {shape} {ep}: worst error / bound {ratio:.3f}")
        X.record("gemm_act%d" % kw["act"], ratio)
        assert ratio <= 1.0, (shape, ep, ratio, at)
        again = _run_gemm(c, M, kw).cpu()
        assert rowwise.bitwise_equal(got, again), (shape, ep, "two calls differ")


def test_gemm_nt_f32_rows_do_not_depend_on_the_call():
    """rows 0..32 of an M = 33 call are the first 33 rows of the M = 130 call on the same A, bit for bit; contiguous and wide operands agree"""
    c = X.gemm_case(130, 2304, 768)
    for ep in X.GEMM_EPILOGUES:
        kw = X.gemm_args(c, ep)
        big, small = _run_gemm(c, 130, kw), _run_gemm(c, 33, kw)
        assert rowwise.bitwise_equal(big[:33], small), ep
        assert rowwise.bitwise_equal(small, _run_gemm(c, 33, kw, wide=False)), ep


def test_gemm_nt_f32_refusals_and_erff():
    from avsiam_amd import _lib, ops
    A, B, out = torch.zeros(4, 48, device=DEV), torch.zeros(8, 48, device=DEV), torch.zeros(4, 8, device=DEV)
    with pytest.raises(_lib.AvsiamHipError, match="multiple of 32"):
        ops.gemm_nt_f32(A, B, out, 4)
    lib = _lib.load()                                                    # ... and by the library itself
    rc = lib.avs_gemm_nt_f32(A.data_ptr(), 48, B.data_ptr(), 48, 4, 8, 48, None, None, 0, None, out.data_ptr(), 8, 1.0, 0, None)
    assert rc == -2 and b"multiple of 32" in lib.avs_last_error()
    # erff through the epilogue on EXACT pre-activations: A = one-hot rows, so x = B[n, k] as it is
    g = torch.Generator().manual_seed(18)
    x = (torch.randn(96, 32, generator=g) * 2.0).to(DEV)
    eye = torch.eye(32, device=DEV)
    got = torch.zeros(32, 96, device=DEV)
    ops.gemm_nt_f32(eye, x, got, 32, act=1)
    ulp = X.erff_ulp_estimate(got.t().cpu(), x.cpu())
    print(f"erff: worst error {ulp:.2f} ulp (upper estimate through the GELU epilogue)")
    X.record("erff_ulp_upper", ulp)
    assert ulp <= X.C_ERF + 10            # (+ 10: the epilogue's own three roundings in these units, for erf in [0.38, 1))


# ---- 2. attention -----------------------------------------------------------------------------------------------------------------------------
def _run_attn(qkv, lens, H, extra_rows=40):
    from avsiam_amd import ops
    rows, D = sum(lens), qkv.shape[1] // 3
    tiles = ops.AttnTiles(lens, DEV, tile_rows=128)
    buf, check = rowwise.guarded(rows, D, torch.float32, DEV, extra_rows=extra_rows)
    ops.attn_fwd_f32(qkv.to(DEV).contiguous(), tiles, H, buf)
    return check()


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("lens", X.ATTN_MIXES, ids=lambda l: "-".join(map(str, l)))
def test_attn_fwd_f32_under_bound(lens, hd):
    _attn_check(lens, 2, hd)


def test_attn_fwd_f32_hd32():
    _attn_check([5, 64, 65], 2, 32)


def _attn_check(lens, H, hd):
    qkv = X.attn_case(H, hd, lens)
    got = _run_attn(qkv, lens, H)
    ref, mag, A, Lrow = X.attn_eval(qkv, lens, H)
    r = X.attn_ratio(got.cpu(), ref, mag, A, Lrow, H)
    worst = float(r.max())
    print(f"attn_fwd_f32 hd {hd} {lens}: worst error / bound {worst:.3f}")
    X.record("attn_hd%d" % hd, worst)
    assert worst <= 1.0, (lens, hd, worst)
    assert rowwise.bitwise_equal(got, _run_attn(qkv, lens, H)), "two calls differ"
    r0 = 0
    for L in lens:                                                        # every sequence alone: its rows' bytes
        if len(lens) > 1:
            alone = _run_attn(qkv[r0:r0 + L], [L], H)
            assert rowwise.bitwise_equal(alone, got[r0:r0 + L]), (lens, L)
        r0 += L


def test_attn_fwd_f32_refuses_hd48():
    from avsiam_amd import _lib, ops
    qkv, out = torch.zeros(8, 3 * 96, device=DEV), torch.zeros(8, 96, device=DEV)
    tiles = ops.AttnTiles([8], DEV, tile_rows=128)
    with pytest.raises(_lib.AvsiamHipError, match="head dim"):
        ops.attn_fwd_f32(qkv, tiles, 2, out)
    lib = _lib.load()
    rc = lib.avs_attn_fwd_f32(qkv.data_ptr(), 288, 96, 2, tiles.start.data_ptr(), tiles.len.data_ptr(), tiles.q0.data_ptr(), 1, 128, out.data_ptr(), 96, None)
    assert rc == -2 and b"head dim 48" in lib.avs_last_error()


# ---- 3. the fp32 gathers ----------------------------------------------------------------------------------------------------------------------
def _pad16(x, S):
    return torch.nn.functional.pad(x, (0, 16 - S, 0, 16 - S))


def _audio_rows(a, S):
    """token (f, t) = f * tP + t of sample b; row[p * 16 + q] = a[b, t S + q, f S + p] (p, q < S), zero elsewhere"""
    B = a.shape[0]
    img = a.transpose(1, 2)                                               # [B, mel, time]
    u = img.unfold(1, S, S).unfold(2, S, S)                               # [B, nf, tP, p, q]
    return _pad16(u, S).reshape(B * u.shape[1] * u.shape[2], 256)


def _video_rows(v, S):
    """token (gy, gx) of image n; row[c * 256 + p * 16 + q] = v[n, c, gy S + p, gx S + q]"""
    NF, C = v.shape[:2]
    u = v.unfold(2, S, S).unfold(3, S, S)                                 # [NF, C, Gy, Gx, p, q]
    Gy, Gx = u.shape[2], u.shape[3]
    return _pad16(u, S).permute(0, 2, 3, 1, 4, 5).reshape(NF * Gy * Gx, C * 256)


def _tables(n_src, n_tok):
    return (torch.arange(n_src).repeat_interleave(n_tok).to(torch.int32).to(DEV), torch.arange(n_tok).repeat(n_src).to(torch.int32).to(DEV))


@pytest.mark.parametrize("S", [16, 14])
def test_im2col_f32_plain_inputs_are_the_restatement(S):
    from avsiam_amd import ops
    g = torch.Generator().manual_seed(S)
    tP, nf, G = 5, 3, 2
    a = torch.randn(2, tP * S, nf * S, generator=g)
    src, tok = _tables(2, nf * tP)
    rows = 2 * nf * tP
    buf, check = rowwise.guarded(rows, 256, torch.float32, DEV, extra_rows=8)
    ops.im2col_audio_f32(a.to(DEV), src, tok, buf, rows, tP, stride=S)
    assert rowwise.bitwise_equal(check().cpu(), _audio_rows(a, S))
    v = torch.randn(3, 3, G * S, G * S, generator=g)
    src, tok = _tables(3, G * G)
    rows = 3 * G * G
    buf, check = rowwise.guarded(rows, 768, torch.float32, DEV, extra_rows=8)
    ops.im2col_video_f32(v.to(DEV), src, tok, buf, rows, stride=S)
    assert rowwise.bitwise_equal(check().cpu(), _video_rows(v, S))


@pytest.mark.parametrize("S", [16, 14])
def test_im2col_f32_rounds_to_the_bf16_gather_under_every_transform(S):
    """with each InputXf kind the tested bf16 gather's rows are the bf16 rounding of the fp32 gather's rows, bit for bit"""
    from avsiam_amd import ops
    g = torch.Generator().manual_seed(100 + S)
    tP, nf, G = 5, 3, 2
    a = (torch.randn(2, tP * S, nf * S, generator=g) * 4.4849 - 5.081).to(DEV)
    src, tok = _tables(2, nf * tP)
    rows = 2 * nf * tP
    shift = torch.tensor([3, -7], dtype=torch.int32, device=DEV)
    amp = torch.tensor([0.0, 0.06], dtype=torch.float32, device=DEV)
    for xf in (ops.InputXf.audio(-5.081, 4.4849), ops.InputXf.audio(-5.081, 4.4849, shift=shift, amp=amp, seed=12345)):
        o32, o16 = torch.zeros(rows, 256, device=DEV), torch.zeros(rows, 256, dtype=torch.bfloat16, device=DEV)
        ops.im2col_audio_f32(a, src, tok, o32, rows, tP, xf, stride=S)
        ops.im2col_audio(a, src, tok, o16, rows, tP, xf, stride=S)
        assert float(o32.abs().max()) > 0 and rowwise.bitwise_equal(o32.to(torch.bfloat16), o16)
    v = torch.randint(0, 256, (3, 3, G * S, G * S), generator=g, dtype=torch.uint8).to(DEV)
    src, tok = _tables(3, G * G)
    rows = 3 * G * G
    o32, o16 = torch.zeros(rows, 768, device=DEV), torch.zeros(rows, 768, dtype=torch.bfloat16, device=DEV)
    ops.im2col_video_f32(v, src, tok, o32, rows, ops.InputXf.frames(), stride=S)
    ops.im2col_video(v, src, tok, o16, rows, ops.InputXf.frames(), stride=S)
    assert float(o32.abs().max()) > 0 and rowwise.bitwise_equal(o32.to(torch.bfloat16), o16)


# ---- 4. the reference's goldens ----------------------------------------------------------------------------------------------------------------
_models = {}


def _golden_model(label_dim=527, seed=4321):
    from avsiam_amd.models import CAVMAEFT_BASE
    if (label_dim, seed) not in _models:
        _models[(label_dim, seed)] = CAVMAEFT_BASE(label_dim, init_seed=seed, init_mode="random").cuda()
    return _models[(label_dim, seed)]


@pytest.mark.parametrize("name", FT_CASES)
def test_exact_modes_match_reference_golden(name):
    d = load_golden(name)
    cfg = AVSiamConfig()
    a, v = ft_case_inputs(d, cfg)
    m = _golden_model(int(d["label_dim"]), int(d["weight_seed"]))
    out = m(a.cuda(), v.cuda(), str(d["mode"]), is_eval=bool(d["is_eval"]), exact=True)
    for k, t in ft_outputs_as_dict(d, out).items():
        assert not t.requires_grad
        if k.startswith("tokens"):
            assert tuple(t.shape) == tuple(d[k + "_shape"])
            p = t.double().cpu().reshape(-1)
            l2 = abs(p.norm().item() - d[k + "_l2"]) / d[k + "_l2"]
            s = np.array([p[i].item() for i in sample_positions(k, p.numel(), 256)])
            print(f"{name}.{k}: L2 off by {l2:.2e} relative, samples off by {np.abs(s - d[k + '_samples']).max():.2e}")
            X.record("tokens_l2_rel_over_bound", l2 / X.TOKEN_L2_REL)
            assert l2 <= X.TOKEN_L2_REL, (k, l2)
            np.testing.assert_allclose(s, d[k + "_samples"], rtol=X.TOKEN_RTOL, atol=X.TOKEN_ATOL)
        else:
            err, cos = X.logit_check(t, d[k])
            print(f"{name}.{k}: max |logit error| {err:.3e} (bound {X.EXACT_LOGIT_ABS:.1e}), min row cosine {cos:.9f}")
            X.record("logits_golden_worst", err)
            X.record("logits_golden_over_bound", err / X.EXACT_LOGIT_ABS)
            assert err <= X.EXACT_LOGIT_ABS, (name, k, err)


# ---- 5. batch invariance and determinism -------------------------------------------------------------------------------------------------------
def test_exact_batch_invariance_and_determinism():
    from avsiam_amd.weights import synth_inputs
    cfg = AVSiamConfig()
    m = _golden_model()
    a, v = synth_inputs(cfg, 3, 11)
    a, v = a.cuda(), v.unsqueeze(1).cuda()
    oa = m(a, None, "audioonly", exact=True)
    om = m(a, v, "mm_grad", exact=True)
    assert rowwise.bitwise_equal(oa, m(a, None, "audioonly", exact=True))
    for x, y in zip(om, m(a, v, "mm_grad", exact=True)):
        assert rowwise.bitwise_equal(x, y)
    for b in range(3):
        assert rowwise.bitwise_equal(m(a[b:b + 1], None, "audioonly", exact=True), oa[b:b + 1]), b
        for x, y in zip(m(a[b:b + 1], v[b:b + 1], "mm_grad", exact=True), om):
            assert rowwise.bitwise_equal(x, y[b:b + 1]), b


# ---- 6. ViT-L / ViT-H skeletons ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["large", "huge14"])
def test_exact_large_and_huge_skeletons_match_oracle(family):
    """the inputs and weights of test_ft_gpu.py::test_ft_large_and_huge_skeletons_match_oracle (depth 2; hd 64 / hd 80 and the 14 x 14 stride)"""
    from oracle import ref_cpu
    from avsiam_amd.config import vit_huge14, vit_large
    from avsiam_amd.models import CAVMAEFT_HUGE, CAVMAEFT_LARGE
    from avsiam_amd.weights import synth_inputs
    torch.set_num_threads(16)
    cfg = vit_large(depth=2) if family == "large" else vit_huge14(depth=2)
    cls = CAVMAEFT_LARGE if family == "large" else CAVMAEFT_HUGE
    B, L = 3, 10
    a, v = synth_inputs(cfg, B, 5)
    v = v.unsqueeze(1)
    m = cls(L, cfg=cfg, init_seed=7, init_mode="init").cuda()
    P = synth_state_ft(cfg, L, 7, "init")
    out = m(a.cuda(), v.cuda(), "mm_grad", exact=True)
    oa = m(a.cuda(), None, "audioonly", exact=True)
    with torch.no_grad():
        ref = ref_cpu.ft_forward(P, cfg, a, v, "mm_grad")
        ra = ref_cpu.ft_forward(P, cfg, a, None, "audioonly")
    for g, r, k in list(zip(out, ref, ("out", "out_a", "out_v"))) + [(oa, ra, "audioonly")]:
        err, _ = X.logit_check(g, r)
        tol = X.EXACT_LOGIT_ABS * max(1.0, float(r.abs().max()))
        print(f"{family}.{k}: max |logit error| {err:.3e} (bound {tol:.2e}, max |ref| {float(r.abs().max()):.3f})")
        X.record(f"logits_{family}_over_bound", err / tol)
        assert err <= tol, (family, k, err, tol)


# ---- 7. as a yardstick -------------------------------------------------------------------------------------------------------------------------
def _bf16_close(got, ref, what):
    err, cos = X.logit_check(got, ref.cpu())
    print(f"{what}: bf16 path against the exact one: max |error| {err:.4f}, min row cosine {cos:.6f}")
    assert err <= X.BF16_LOGIT_ABS and cos >= X.BF16_LOGIT_COS, (what, err, cos)


def test_exact_is_a_yardstick_for_the_bf16_path_and_reads_the_masters():
    from avsiam_amd.models import CAVMAEFT_BASE
    cfg = AVSiamConfig()
    L = 527
    m = CAVMAEFT_BASE(L, init_seed=4321, init_mode="random").cuda()
    m.requires_grad_(True)                                                # (exact=True stays an inference output all the same)
    g = torch.Generator().manual_seed(7)
    a = torch.randn(5, cfg.audio_len, cfg.n_mels, generator=g).cuda()
    v = torch.randn(3, 10, 3, cfg.img_size, cfg.img_size, generator=g).cuda()
    with torch.no_grad():
        _bf16_close(m(a[:3], v, "mm_grad", is_eval=True), m(a[:3], v, "mm_grad", is_eval=True, exact=True), "mm_grad is_eval, 3 x 10 frames")
        before = m(a, None, "audioonly", exact=True)
        _bf16_close(m(a, None, "audioonly"), before, "audioonly, B = 5")
    assert not m(a, None, "audioonly", exact=True).requires_grad          # grad mode on, trainable parameters: still no autograd node
    labels = (torch.rand(5, L, generator=g) > 0.9).float().cuda()
    m.train_step(a, None, labels, 1e-3, ftmode="audioonly")
    with torch.no_grad():
        after = m(a, None, "audioonly", exact=True)
        moved = float((after - before).abs().max())
        print(f"one train_step moved the exact logits by up to {moved:.3e}")
        assert moved > 10 * X.EXACT_LOGIT_ABS, moved                      # the masters are read; nothing stale is cached
        _bf16_close(m(a, None, "audioonly"), after, "audioonly after the step")


# ---- 8. the default path is untouched ----------------------------------------------------------------------------------------------------------
# one plain fine-tuning step: tools/step_digest.py --ft --trace --batch 3 (profiles/r14/frames_bench.json; tests/test_resample_gpu.py asserts the same)
PARENT_DIGEST = {"trace_calls": 303, "trace": "21a456a12665402bb61ad36021b881415531210137bfe83da2f626bd146a239a"}


def test_plain_step_is_the_parents():
    r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: got[k] for k in PARENT_DIGEST} == PARENT_DIGEST
