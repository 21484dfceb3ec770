"""tests/fp8lib.py proved on the CPU: every lattice the GPU tests use is exact (each intermediate representable, the 8-bit copies rounding
with ties over many codes, nothing saturating but the one case meant to), and the checks the GPU tests call reject each kind of damage
a kernel's epilogue could do - shown on a torch emulation of the epilogue (256-row tiles, rows beyond M clamped to row M - 1 by the
loader and kept out by the epilogue's row test)."""
import pytest
import torch

from tests import fp8lib as fl
from tests import rowwise as rw

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def ties_and_codes(x, scale, fmt):
    """how many values of x * scale lie exactly between two neighbouring codes, and how many distinct codes the copy uses"""
    v = x.double() * scale
    down = fl.quant(x, scale, fmt, rne=False)
    lo, hi = fl.decode(down, fmt).abs(), fl.decode(down + 1, fmt).abs()
    return int(((v.abs() - lo) == (hi - v.abs())).sum()), len(torch.unique(fl.quant(x, scale, fmt)))


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(fl.NT_FORMS))
@pytest.mark.parametrize("M,N,K", fl.NT_SHAPES)
def test_nt_lattices_are_exact(M, N, K, form):
    grad, out, _ = fl.NT_FORMS[form]
    c = fl.nt_case(M, N, K, grad)
    opt = fl.nt_form_options(form, c)
    e = fl.nt_expected(c, **opt)                       # (asserts that x and the column sums are exact in fp32)
    x = e["x"]
    assert float(x.abs().max()) < 2 ** 11 and float((fl.decode(c["A8"], c["a_fmt"]).abs() @ fl.decode(c["W8"], fl.E4M3).abs().t()).max()) < 2 ** 11 * c["sa"] * c["sw"]
    rounded = e["bf16"].double() != x
    if opt.get("aux"):
        if M in (17, 257):                   # the lifted last row: 3/4 of integers up to ~170 - bf16 rounding is really exercised, ties among them
            lo, hi = fl.bf16_interval(e["bf16"])
            halfway = (x.float() == lo) | (x.float() == hi)
            assert bool(rounded.any()) and bool((~rounded).any()) and bool((halfway & rounded).any())
        else:
            assert not bool(rounded.any())
    else:
        assert not bool(rounded.any())                                       # integers below 256 (times 1/8 in the scaled columns): exact in bf16
    if "q8_scale" in opt:
        ties, codes = ties_and_codes(x, opt["q8_scale"], fl.E5M2)
        assert float((x.abs() * opt["q8_scale"]).max()) < 57344.0             # nothing saturates
        if M >= 255:
            assert ties > 0 and codes >= 32, (ties, codes)
        assert e["amax"] == (fl.AMAX_ABOVE if M == fl.AMAX_ABOVE_M else float(x.abs().max()))
    if opt.get("colsum"):
        assert float(e["colsum"].abs().max()) < 2 ** 13


@pytest.mark.parametrize("M,N,K", [s for s in fl.NT_SHAPES if s[0] in (17, 257)])
@pytest.mark.parametrize("form", ["fwd_bf16_cols0", "fwd_f32_res", "dgrad_bf16_out8", "dgrad_act2"])
def test_last_row_holds_the_column_wise_and_global_maximum(M, N, K, form):
    c = fl.nt_case(M, N, K, fl.NT_FORMS[form][0])
    x = fl.nt_expected(c, **fl.nt_form_options(form, c))["x"].abs()
    assert bool((x[M - 1] > x[:M - 1].max(0).values).all()) and float(x[M - 1].max()) == float(x.max())


def test_the_one_case_meant_to_saturate():
    M, N, K = fl.SAT_SHAPE
    c = fl.nt_case(M, N, K, True)
    e = fl.nt_expected(c, bias=False, q8_scale=fl.Q8_SCALE_SAT)
    sat = (e["x"].abs() * fl.Q8_SCALE_SAT) > 57344.0
    assert bool(sat[M - 1].all()) and 0 < int(sat.sum()) < sat.numel() // 4
    assert bool(((e["out8"] & 0x7F)[sat] == 0x7B).all())                      # 0x7B: the largest finite e5m2 value, not infinity


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129, 1000])
def test_tn_lattices_are_exact(M):
    for (N1, N2), (sa, sb) in zip(fl.TN_SHAPES, fl.TN_SCALES):
        c = fl.tn_lattice(M, N1, N2, sa, sb)
        C = fl.tn_expected(c)                          # (asserts exactness in fp32)
        Mp = (M + 63) // 64 * 64
        assert c["A8"].shape[0] == Mp and not bool(c["A8"][M:].any()) and not bool(c["B8"][M:].any())
        assert float(C.abs().max()) < 2 ** 12 and float((fl.decode(c["A8"], fl.E5M2).abs().t() @ fl.decode(c["B8"], fl.E4M3).abs()).max()) < 2 ** 11 * sa * sb
        far = fl.tn_lattice(M, N1, N2, sa, sb, extra_rows=64)
        assert torch.equal(far["A8"][:Mp], c["A8"]) and bool(far["A8"][Mp:].all()) and bool(far["B8"][Mp:].all())
        assert torch.equal(fl.tn_expected(far), C)


# ---------------------------------------------------------------------------------------------------
# the epilogue, emulated in fp32 tile by tile, with the damage a kernel could do
def emulate_nt(c, out, damage=None, bias=True, res=False, aux=False, scale_cols=0, col_scale=1.0, m_split=0, colsum=False, q8_scale=None, amax0=0.0, alpha=None):
    M, N = c["M"], c["N"]
    Mt = (M + 255) // 256 * 256
    clamp = torch.arange(Mt).clamp_max(M - 1)                          # the loader: rows beyond M read row M - 1
    A = fl.decode(c["A8"], c["a_fmt"]).float()[clamp]
    pad = lambda t: torch.cat([t.float(), torch.full((Mt + 1 - M, N), 7.0)])      # what lies behind aux / res: not zeros
    auxp, resp = pad(c["aux"]), pad(c["res"])
    dual = 0 < m_split < M
    o16, chk16 = rw.guarded(M, N, BF, "cpu")
    o32, chk32 = rw.guarded(M, N, F32, "cpu")
    o8, chk8 = rw.guarded(M, N, U8, "cpu")
    cs, cs2, amax = c["colsum0"].clone(), c["colsum0_2"].clone(), float(amax0)
    for m0 in range(0, Mt, 256):
        second = dual and m0 >= m_split
        W8, sw, b = (c["W8_2"], c["sw2"], c["bias2"]) if second else (c["W8"], c["sw"], c["bias"])
        if damage == "dq_of_the_other_set" and second:
            sw = c["sw"]
        if damage == "bias_of_the_other_set" and second:
            b = c["bias"]
        dq = rw.f32(alpha) if alpha is not None else 1.0 / (c["sa"] * sw)
        v = (A[m0:m0 + 256] @ fl.decode(W8, fl.E4M3).float().t()) * dq
        if bias:
            v = v + b
        if aux:
            v = v * auxp[m0:m0 + 256]
        if res:
            v = v + resp[m0:m0 + 256]
        ac = torch.ones(N)
        ac[:scale_cols] = col_scale
        if damage == "slice_unscaled":
            ac[64:128] = 1.0
        v = v * ac
        live = torch.arange(m0, m0 + 256) < M
        n = int(live.sum())
        counted = v if damage == "pad_rows_in_colsum" else v[live]
        if colsum:
            if second:
                cs2 = cs2 + counted.sum(0)
            else:
                cs = cs + counted.sum(0)
        if q8_scale is not None:
            seen = v if damage == "pad_rows_in_amax" else v[live]
            amax = max(amax, float(seen.abs().max()))
            w = n + 1 if damage == "out8_row_past_M" and n < 256 else n
            o8[m0:m0 + w] = fl.quant(v[:w], q8_scale, fl.E5M2, rne=damage != "truncated")
        o16[m0:m0 + n], o32[m0:m0 + n] = v[live].to(BF), v[live]
    if damage == "block_from_neighbour" and M >= 48:
        o8[16:32] = o8[32:48]
    got = {}
    if out == "bf16":
        got["bf16"] = chk16()
    if out == "f32":
        got["f32"] = chk32()
    if q8_scale is not None:
        got["out8"], got["amax"] = chk8(), amax
    if colsum:
        got["colsum"] = cs
        if dual:
            got["colsum2"] = cs2
    return got


@pytest.mark.parametrize("form", list(fl.NT_FORMS))
@pytest.mark.parametrize("M,N,K", [(17, 512, 384), (257, 256, 640), (513, 512, 384)])
def test_the_honest_emulation_matches_the_reference(M, N, K, form):
    grad, out, _ = fl.NT_FORMS[form]
    c = fl.nt_case(M, N, K, grad)
    opt = fl.nt_form_options(form, c)
    assert fl.mismatches(emulate_nt(c, out, **opt), fl.nt_expected(c, **opt)) == []


DAMAGE = {   # name -> (M, N, K, form, extra options)
    "pad_rows_in_colsum": (257, 512, 384, "dgrad_bf16", {}),
    "pad_rows_in_amax": (257, 512, 384, "dgrad_act2", {}),
    "slice_unscaled": (257, 512, 384, "fwd_bf16_cols192", {}),
    "dq_of_the_other_set": (600, 512, 384, "fwd_f32_res", {"m_split": 256}),
    "bias_of_the_other_set": (600, 512, 384, "fwd_bf16_cols0", {"m_split": 256}),
    "truncated": (257, 512, 384, "dgrad_bf16_out8", {}),
    "block_from_neighbour": (257, 512, 384, "dgrad_out8_only", {}),
}


@pytest.mark.parametrize("damage", list(DAMAGE))
def test_damage_is_rejected(damage):
    M, N, K, form, extra = DAMAGE[damage]
    grad, out, _ = fl.NT_FORMS[form]
    c = fl.nt_case(M, N, K, grad)
    opt = dict(fl.nt_form_options(form, c), **extra)
    want = fl.nt_expected(c, **opt)
    assert fl.mismatches(emulate_nt(c, out, **opt), want) == []
    bad = fl.mismatches(emulate_nt(c, out, damage=damage, **opt), want)
    hit = {"pad_rows_in_colsum": "colsum", "pad_rows_in_amax": "amax", "slice_unscaled": "bf16", "dq_of_the_other_set": "f32",
           "bias_of_the_other_set": "bf16", "truncated": "out8", "block_from_neighbour": "out8"}[damage]
    assert [b[0] for b in bad] == [hit], bad
    if damage == "slice_unscaled":
        assert bad[0][1] <= M * 64                     # the one slice, nothing else
    if damage in ("dq_of_the_other_set", "bias_of_the_other_set"):
        assert bad[0][2][0] >= 256                     # the first wrong element lies behind m_split


def test_a_row_written_past_M_trips_the_guard_band():
    c = fl.nt_case(257, 512, 384, True)
    opt = fl.nt_form_options("dgrad_bf16_out8", c)
    with pytest.raises(AssertionError, match="rows beyond the output were written"):
        emulate_nt(c, "bf16", damage="out8_row_past_M", **opt)


def test_two_weight_sets_keep_their_column_sums_apart():
    c = fl.nt_case(600, 512, 384, True)
    opt = dict(bias=False, colsum=True, q8_scale=fl.Q8_SCALE, m_split=256)
    e = fl.nt_expected(c, **opt)
    assert torch.equal(e["colsum"].double(), c["colsum0"].double() + e["x"][:256].sum(0))
    assert torch.equal(e["colsum2"].double(), c["colsum0_2"].double() + e["x"][256:].sum(0))
    assert fl.mismatches(emulate_nt(c, "bf16", **opt), e) == []


# ---------------------------------------------------------------------------------------------------
def test_bf16_interval_holds_what_rounds_to_the_value():
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(20000, generator=g) * 3, torch.zeros(4), torch.tensor([1.0, -1.0, 2.0 ** -130, 0.99609375])])
    b = v.to(BF)
    lo, hi = fl.bf16_interval(b)
    assert bool(((lo <= v) & (v <= hi)).all())
    inner = lambda e: torch.nextafter(e, b.float())                    # one fp32 step inside the interval still rounds to b
    assert torch.equal(inner(lo).to(BF), b) and torch.equal(inner(hi).to(BF), b)
    outer = torch.nextafter(hi, torch.full_like(hi, float("inf")))
    assert not bool((outer.to(BF) == b).any())


@pytest.mark.parametrize("fmt", [fl.E4M3, fl.E5M2])
def test_codes_within_accepts_the_honest_double_rounding_and_rejects_one_code_off(fmt):
    g = torch.Generator().manual_seed(11)
    v = torch.randn(200000, generator=g) * 1.7
    b = v.to(BF)
    s = fl.quarter_scale(b.float().abs().max(), fmt)
    code = fl.quant(v, s, fmt)
    bad, share = fl.codes_within(code, b, s, fmt)
    assert bad.numel() == 0
    assert 0.5 * fl.AMBIGUOUS_MAX[fmt] < share <= fl.AMBIGUOUS_MAX[fmt], share          # 6.3 % (e4m3) / 3.3 % (e5m2) here
    # one code off on 0.1 % of the elements
    idx = torch.randperm(v.numel(), generator=g)[:v.numel() // 1000]
    off = code.clone()
    off[idx] = torch.where((code[idx] & 0x7F) == 0, code[idx] + 1, code[idx] - 1)
    bad, _ = fl.codes_within(off, b, s, fmt)
    assert set(bad.tolist()) <= set(idx.tolist()) and bad.numel() >= 0.85 * idx.numel(), (bad.numel(), idx.numel())
    # a copy rounded towards zero, and a copy made from the bf16 value of a neighbouring element
    assert fl.codes_within(fl.quant(v, s, fmt, rne=False), b, s, fmt)[0].numel() > 0.2 * v.numel()
    assert fl.codes_within(code.roll(1), b, s, fmt)[0].numel() > 0.9 * v.numel()


# the producers that are not exact on a lattice: the inputs of the GPU tests must keep the interval check sharp (a condition on the
# inputs, evaluated on the references)
@pytest.mark.parametrize("M,N,K", fl.GELU_SHAPES)
def test_gelu_inputs_keep_the_interval_check_sharp(M, N, K):
    x = fl.nt_expected(fl.gelu_case(M, N, K), alpha=fl.GELU_ALPHA)["x"]
    assert 2.0 < float(x.std()) < 4.0 and len(torch.unique(x)) > 500                  # the grid covers the curved part of GELU finely
    gv = rw.gelu64(x).float()
    b = gv.to(BF)
    s = fl.quarter_scale(b.float().abs().max(), fl.E4M3)
    bad, share = fl.codes_within(fl.quant(gv, s, fl.E4M3), b, s, fl.E4M3)
    assert bad.numel() == 0 and share <= fl.AMBIGUOUS_MAX[fl.E4M3], share


@pytest.mark.parametrize("D", fl.LN_D)
def test_layernorm_inputs_keep_the_interval_check_sharp(D):
    c = fl.ln_case(D)
    for mod in (None, c["mod"]):
        y = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], 1e-5, mod, c["g"][1], c["b"][1])["y"].float()
        b = y.to(BF)
        s = fl.quarter_scale(b.float().abs().max(), fl.E4M3)
        bad, share = fl.codes_within(fl.quant(y, s, fl.E4M3), b, s, fl.E4M3)
        assert bad.numel() == 0 and share <= fl.AMBIGUOUS_MAX[fl.E4M3], share
    if D in fl.LN_BWD_D:
        st = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], 1e-5, c["mod"], c["g"][1], c["b"][1], emulate=True)
        dx = rw.layernorm_bwd_eval(c["dy"], c["x"], st["mean"], st["rstd"], c["g"][0], c["dres"].to(BF), c["mod"], c["g"][1])["dx"].float()
        b = dx.to(BF)
        s = fl.quarter_scale(b.float().abs().max(), fl.E5M2)
        bad, share = fl.codes_within(fl.quant(dx, s, fl.E5M2), b, s, fl.E5M2)
        assert bad.numel() == 0 and share <= fl.AMBIGUOUS_MAX[fl.E5M2], share


@pytest.mark.parametrize("H,hd", fl.ATTN_HEADS)
def test_attention_inputs_keep_the_interval_check_sharp(H, hd):
    c = rw.attn_case(H, hd, fl.ATTN_LENS)
    o = rw.attention_eval(c["qkv"], fl.ATTN_LENS, H, c["dout"])["out"].float()
    b = o.to(BF)
    s = fl.quarter_scale(b.float().abs().max(), fl.E4M3)
    bad, share = fl.codes_within(fl.quant(o, s, fl.E4M3), b, s, fl.E4M3)
    assert bad.numel() == 0 and share <= fl.AMBIGUOUS_MAX[fl.E4M3], share
