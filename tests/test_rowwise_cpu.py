"""Proof, without a GPU, that the measures of tests/rowwise.py bite: honest emulations of the kernels' arithmetic (fp32 accumulation, bf16
rounding where the kernels round) pass every measure on the case lists of tests/test_rowwise_gpu.py, and every mutant - the subtle damage
a wrong fragment index or tail mask does - fails at least one of them while the suite's whole-tensor norm at its existing tolerance
accepts it.  Run with -s to see the figures."""
import pytest
import torch

from tests import rowwise as rw

BF, F32 = torch.bfloat16, torch.float32


def say(*a):
    print("[rowwise]", *a)


# --- honest emulation of the nt GEMM: an fp32 product of the bf16 operands, the epilogue in fp32, one rounding of the output
def nt_emulate(c, out_dtype=BF, bias=True, res=None, res_idx=None, aux=None, alpha=1.0, scale_cols=0, col_scale=1.0, m_split=0, act=0, codes=False):
    A = c["A"].float()
    M = A.shape[0]
    x = A @ c["B"].float().t()
    if bias:
        x = x + c["bias"]
    if m_split and m_split < M:
        x2 = A[m_split:] @ c["B2"].float().t()
        x = torch.cat([x[:m_split], x2 + c["bias2"] if bias else x2])
    if aux is not None:
        x = x * (rw.gp8_decode(aux).float() if aux.dtype == torch.uint8 else aux.float())
    if res is not None:
        x = x + (res[res_idx.long()] if res_idx is not None else res[:M])
    ac = torch.full((x.shape[1],), rw.f32(alpha))
    ac[:scale_cols] = rw.f32(rw.f32(alpha) * rw.f32(col_scale))
    x = x * ac
    if act == 1:
        g = rw.gelu_grad64(x.double()).float()
        gp = torch.round((g + rw.GP8_BIAS) * rw.GP8_STEPS).clamp(0, 255).to(torch.uint8) if codes else g.to(BF)
        return x, gp, rw.gelu64(x.double()).float().to(BF)
    return x, x.to(out_dtype)


def nt_epilogue_checks(c, K, emu=nt_emulate):
    """every epilogue of the case list at one shape -> {name: worst ratio}"""
    M, N = c["A"].shape[0], c["B"].shape[0]
    qs = rw.attn_q_scale(64)
    worst = {}
    for sc in (64, 192, 320):
        if sc > N:
            continue
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], scale_cols=sc, col_scale=qs)
        m = rw.check_gemm(emu(c, scale_cols=sc, col_scale=qs)[1], ref, S, K)
        worst["bf16_scale%d" % sc] = max(m["elem"], m["row"])
    for name, r, ri in (("f32_res", c["res"], None), ("f32_res_idx", c["res_pool"], c["res_idx"])):
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], res=r, res_idx=ri, alpha=1.5)
        m = rw.check_gemm(emu(c, F32, res=r, res_idx=ri, alpha=1.5)[1], ref, S, K)
        worst[name] = max(m["elem"], m["row"])
    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"])
    dx = rw.gemm_bound(ref, S, K, rw.U_F32)
    gr, ge = rw.gelu_grad64(ref), rw.gelu64(ref)
    for codes in (False, True):
        x, gp, act = emu(c, act=1, codes=codes)
        got = rw.gp8_value(gp) if codes else gp
        worst["act1_codes" if codes else "act1_bf16"] = max(rw.elem_ratio(got, gr, rw.gelu_grad_bound(dx, gr, codes))[0],
                                                           rw.elem_ratio(act, ge, rw.gelu_bound(dx, ge))[0])
    for name, aux in (("act2_bf16", c["aux"]), ("act2_codes", c["aux8"])):
        auxv = rw.gp8_decode(aux) if aux.dtype == torch.uint8 else aux
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], None, aux=auxv)
        x, out = emu(c, bias=False, aux=aux)
        m = rw.check_gemm(out, ref, S, K)
        cs = c["colsum0"] + x.sum(0)
        cr = rw.elem_ratio(cs, c["colsum0"].double() + ref.sum(0), rw.colsum_bound(ref, S, K, c["colsum0"]))[0]
        worst[name] = max(m["elem"], m["row"], cr)
    return worst


def test_honest_gemm_emulations_pass_on_the_case_list():
    worst, at = {}, {}
    for M in rw.NT_M:
        for N in rw.NT_N:
            for K in rw.NT_K:
                w = nt_epilogue_checks(rw.gemm_nt_case(M, N, K), K)
                for k, v in w.items():
                    if v > worst.get(k, 0.0):
                        worst[k], at[k] = v, (M, N, K)
    for k in sorted(worst):
        say(f"nt emulation {k:14s} worst ratio {worst[k]:.3f} at {at[k]}")
        assert worst[k] <= 1.0, (k, worst[k], at[k])
    # two weight sets
    for M in (257, 600):
        c = rw.gemm_nt_case(M, 512, 128)
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], m_split=256, B2=c["B2"], bias2=c["bias2"])
        m = rw.check_gemm(nt_emulate(c, m_split=256)[1], ref, S, 128)
        say(f"nt emulation two weight sets M={M}: elem {m['elem']:.3f} row {m['row']:.3f}")
        assert max(m["elem"], m["row"]) <= 1.0
    # weight gradient: the contraction runs over M, onto a non-zero C
    w = 0.0
    for M in rw.TN_M:
        for N1, N2 in rw.TN_N:
            c = rw.gemm_tn_case(M, N1, N2)
            ref, S = rw.gemm_tn_terms(c["A"], c["B"], c["C0"])
            got = c["C0"] + c["A"].float().t() @ c["B"].float()
            m = rw.check_gemm(got, ref, S, M)
            w = max(w, m["elem"], m["row"])
    say(f"tn emulation worst ratio {w:.3f}")
    assert w <= 1.0


def test_quoted_gemm_figures():
    """an fp32 product against the per-element bound, and the same with one row scaled by 1.01, at 300 x 256 x K"""
    for K in (64, 768, 3072):
        c = rw.gemm_nt_case(300, 256, K, seed=1)
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"])
        out = nt_emulate(c)[1]
        honest = rw.check_gemm(out, ref, S, K)
        mut = out.clone()
        mut[137] = (out[137].float() * 1.01).to(BF)
        bad = rw.check_gemm(mut, ref, S, K)
        say(f"K={K}: honest elem ratio {honest['elem']:.2f}, row x 1.01 elem ratio {bad['elem']:.2f}; whole-tensor norm honest {rw.whole_rel(out, ref):.2e} "
            f"mutant {rw.whole_rel(mut, ref):.2e} (tolerance 4e-3)")
        assert honest["elem"] <= 1.0 and honest["row"] <= 1.0
        assert bad["elem"] > 1.0                                   # the new measure rejects
        assert rw.whole_rel(mut, ref) < 4e-3                       # the existing one accepts
    outf = nt_emulate(c, F32)[1]
    say(f"per-row norm error at 300 x 256 x 3072: bf16 {float(rw.row_rel(out, ref).max()):.2e} (tolerance 4e-3), fp32 {float(rw.row_rel(outf, ref).max()):.2e} (1e-5)")
    assert float(rw.row_rel(out, ref).max()) < 4e-3 and float(rw.row_rel(outf, ref).max()) < 1e-5


def _verdict(name, new_ratio, whole, whole_tol):
    say(f"mutant {name}: new measure ratio {new_ratio:.3g} (rejected above 1); whole-tensor norm {whole:.2e} (accepted below {whole_tol:g})")
    assert new_ratio > 1.0, name
    assert whole < whole_tol, name


def test_gemm_mutants_are_rejected_where_the_whole_tensor_norm_accepts_them():
    # the last valid row replaced by its neighbour (a clamped-row slip).  One row is 1 / M of the tensor: the whole-tensor norm accepts it from the
    # row counts of the workload on (sqrt(2 / M) < 4e-3 from M = 125 000)
    M, N, K = 140001, 128, 64
    c = rw.gemm_nt_case(M, N, K, seed=2)
    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"])
    out = nt_emulate(c)[1]
    assert rw.check_gemm(out, ref, S, K)["elem"] <= 1.0
    mut = out.clone()
    mut[M - 1] = out[M - 2]
    m = rw.check_gemm(mut, ref, S, K)
    _verdict("clamped last row", max(m["elem"], m["row"]), rw.whole_rel(mut, ref), 4e-3)
    assert m["at"][0] == M - 1
    # one 16 x 16 block given another block's bias (biases of a trained layer's size: 0.1)
    M, N, K = 1000, 256, 768
    c = rw.gemm_nt_case(M, N, K, seed=3)
    c["bias"] = c["bias"] * 0.1
    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"])
    x, out = nt_emulate(c)
    mut = out.clone()
    mut[512:528, 64:80] = (x[512:528, 64:80] - c["bias"][64:80] + c["bias"][80:96]).to(BF)
    m = rw.check_gemm(mut, ref, S, K)
    _verdict("16 x 16 block with its neighbour's bias", m["elem"], rw.whole_rel(mut, ref), 4e-3)
    # col_scale applied in 128-column units: a 64-column wave slice is left unscaled whenever scale_cols is an odd multiple of 64.  Every existing
    # test passes a multiple of 128, where this kernel is right - the whole-tensor norm never sees it
    qs = rw.attn_q_scale(64)
    c = rw.gemm_nt_case(300, 384, 256, seed=4)

    def coarse(c, **kw):
        kw["scale_cols"] = kw.get("scale_cols", 0) // 128 * 128
        return nt_emulate(c, **kw)

    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], scale_cols=256, col_scale=qs)
    at128 = rw.whole_rel(coarse(c, scale_cols=256, col_scale=qs)[1], ref)
    new = 0.0
    for sc in (64, 192, 320):
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], scale_cols=sc, col_scale=qs)
        new = max(new, rw.check_gemm(coarse(c, scale_cols=sc, col_scale=qs)[1], ref, S, 256)["elem"])
    _verdict("columns left unscaled at scale_cols 64 / 192 / 320 (existing cases: multiples of 128)", new, at128, 4e-3)
    # a guard row overwritten: the whole-tensor norm looks at rows [0, M) only
    buf, check = rw.guarded(300, 256, BF, "cpu")
    buf[:300] = nt_emulate(rw.gemm_nt_case(300, 256, 64))[1]
    check()
    buf[300, 5] = 0.0
    with pytest.raises(AssertionError):
        check()
    say("mutant guard row overwritten: rejected by the guard band; rows beyond M are outside every norm")


def _attn_measured(H, hd, lens, lq=0):
    c = rw.attn_case(H, hd, lens, lq)
    ref = rw.attention_eval(c["qkv"], lens, H, c["dout"], lq)
    emu = rw.attention_eval(c["qkv"], lens, H, c["dout"], lq, emulate=True)
    return c, ref, emu, rw.attention_measures(emu, ref, H)


def test_honest_attention_emulation_and_quoted_figures():
    worst = {}
    for hd in (32, 64, 80):
        c, ref, emu, m = _attn_measured(2, hd, rw.ATTN_LENS)
        tol = rw.attention_tolerances(m)
        say(f"attention emulation hd {hd}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(m.items())))
        for k, v in m.items():
            assert v <= tol[k], (hd, k)
            if k in rw.ATTN_WHOLE_TOL:
                assert v <= rw.ATTN_WHOLE_TOL[k], (hd, k, v)                     # the honest emulation stays under the cap of its tolerance
            worst[k] = max(worst.get(k, 0.0), v)
        # the plain relative measure collapses where the gradient cancels (dq of a two-token sequence)
        rel = rw.head_row_ratio(emu["dq"], ref["dq"], ref["dq"], 2)
        say(f"  dq relative to ||ref|| instead of the magnitude row: worst {float(rel[1:].max()):.2f} (rows of L = 2: {float(rel[1:3].max()):.2f})")
    for lq in (1, 33):
        c, ref, emu, m = _attn_measured(2, 32, [65, 65, 65], lq)
        say(f"attention emulation compact queries lq {lq}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(m.items())))
        assert all(v <= rw.attention_tolerances(m)[k] for k, v in m.items())
    say("attention emulation worst rows over hd 32 / 64 / 80: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    assert worst["out_rel"] < 6e-3 and max(worst["dq"], worst["dk"], worst["dv"]) < 5e-3


def test_attention_mutants():
    H, hd, lens = 2, 64, rw.ATTN_LENS
    D = H * hd
    c, ref, emu, m = _attn_measured(H, hd, lens)
    tol = rw.attention_tolerances(m)

    def ratio(got):
        mm = rw.attention_measures(got, ref, H, tol=tol)
        return max(mm.values()), mm

    start = {L: sum(lens[:i]) for i, L in enumerate(lens)}
    # one row of one head of the 33-token sequence attends one key beyond L (tail mask off by one): key L is the next sequence's first row
    L, r, h = 33, start[33] + 7, 1
    x = c["qkv"].float()
    q = x[r, h * hd:(h + 1) * hd]
    k = x[start[33]:start[33] + L + 1, D + h * hd:D + (h + 1) * hd]
    v = x[start[33]:start[33] + L + 1, 2 * D + h * hd:2 * D + (h + 1) * hd]
    p = torch.softmax((k @ q) * rw.LN2, 0)
    mut = dict(emu)
    mut["out"] = emu["out"].clone()
    mut["out"][r, h * hd:(h + 1) * hd] = rw.bf16_round(p @ v)
    rr, mm = ratio(mut)
    _verdict("tail mask off by one key (one row, one head, L = 33)", rr, rw.whole_rel(mut["out"], ref["out"]), 6e-3)
    # lse of one row off by 1e-3: never compared with a reference before
    mut = dict(emu)
    mut["lse"] = emu["lse"].clone()
    mut["lse"][1, start[17] + 3] += 1e-3
    rr, mm = ratio(mut)
    _verdict("lse of one row off by 1e-3", rr, rw.whole_rel(mut["lse"], ref["lse"]), 1e-5)


def test_honest_layernorm_emulation_and_the_one_pass_variance_mutant():
    eps = 1e-5
    for D in rw.LN_D + rw.LN_D_HEAD:
        for kind in rw.LN_KINDS:
            c = rw.ln_case(D, kind)
            ref = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], eps, c["mod"], c["g"][1], c["b"][1])
            emu = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], eps, c["mod"], c["g"][1], c["b"][1], emulate=True)
            mean_r = float(((emu["mean"].double() - ref["mean"]).abs() / rw.layernorm_mean_bound(c["x"])).max())
            rstd_e = float(((emu["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]).max())
            y32 = float(rw.row_rel(emu["y"], ref["y"]).max())
            y16 = float(rw.row_rel(emu["y"].to(BF), ref["y"]).max())
            say(f"layernorm emulation D {D} {kind:6s}: mean ratio {mean_r:.3f}, rstd rel {rstd_e:.2e}, y per row fp32 {y32:.2e} bf16 {y16:.2e}")
            assert mean_r <= 1.0 and y16 <= 4e-3
            if kind != "offset":                                   # (offset: 50 / 0.5 = 100 times the usual input's cancellation in x - mean - a plain two-pass fp32 evaluation misses 1e-5; the kernel corrects its mean)
                assert y32 <= 1e-5
            if kind == "const":
                assert abs(float(ref["rstd"][0]) - eps ** -0.5) < 1e-6 * eps ** -0.5
            # backward: the fp32 evaluation against fp64, per row over the magnitude row
            mean, rstd = ref["mean"].float(), ref["rstd"].float()
            br = rw.layernorm_bwd_eval(c["dy"], c["x"], mean, rstd, c["g"][0], c["dres"], c["mod"], c["g"][1])
            be = rw.layernorm_bwd_eval(c["dy"], c["x"], mean, rstd, c["g"][0], c["dres"], c["mod"], c["g"][1], emulate=True)
            dxr = float(rw.mag_row_ratio(be["dx"], br["dx"], br["dx_abs"]).max())
            assert dxr < 1e-6, (D, kind, dxr)
    # rstd from E[x^2] - mean^2 on the offset input: y stays inside the whole-tensor bf16 tolerance, rstd is far outside 3 x the two-pass error
    c = rw.ln_case(768, "offset")
    ref = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], eps)
    emu = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], eps, emulate=True)
    mut = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], eps, emulate=True, one_pass=True)
    tol = 3.0 * max(float(((emu["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]).max()), rw.U_F32)
    err = float(((mut["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]).max())
    _verdict("rstd from E[x^2] - mean^2 on 50 + 0.5 randn", err / tol, rw.whole_rel(mut["y"].to(BF), ref["y"]), 4e-3)
