"""The fp8 path pinned bit for bit: the fp8 instantiations of the 8-phase GEMM (gemm_nt8_kernel<ACT, 1 | 2>), the fp8 weight-gradient kernel
(gemm_tn8f_kernel) and the 8-bit epilogues of the LayerNorm and attention kernels, under tests/fp8lib.py (proved on the CPU by
tests/test_fp8_exact_cpu.py).

(a) (b) (c) (e): integer lattices - every output byte, column sum and recorded amax must EQUAL an fp64 evaluation; no tolerance.
(d) (f) (g): producers that are not exact on a lattice - the 8-bit copy is checked element by element against the rounding interval of its
bf16 neighbour (fp8lib.codes_within), the bf16 output bitwise against the call without the copy.  The only tolerances are rowwise.gelu_bound /
gelu_grad_bound (bf16 rounding of GELU, what tests/test_rowwise_gpu.py holds the bf16 epilogue to), the 0.0025 + 0.0045 of the 8-bit gelu' codes
(test_gemm_nt_fp8_gelu_grad_as_8_bit_codes) and the bf16 unit roundoff for a recorded amax.

Every output is allocated with guard rows of a non-zero sentinel (rowwise.guarded), operands the epilogue reads per row (aux, res) with
guard rows of 7.0.  ops.gemm_nt_fp8 admits contiguous tensors only, so A8 / out8 cannot be handed over as strided views.
The ambiguous-code shares go to helpers.record_margin ("fp8_exact/...")."""
import pytest
import torch

from tests import fp8lib as fl
from tests import rowwise as rw
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
E4M3, E5M2 = fl.E4M3, fl.E5M2
BF8_MAX = 57344.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """if a test leaves the device in an error state, the session ends there instead of queueing more work on it; and every knob is where
    it was"""
    from avsiam_amd import _lib
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error - nothing more is started on the device: {e}", returncode=3)
    assert all(_lib.tuning_get(k) == v for k, v in fl.KNOB_DEFAULTS.items())


def ops():
    from avsiam_amd import ops as o
    return o


def records(scales, amax=None, fmax=448.0, pow2=True):
    r = ops().Fp8Records(len(scales), DEV, fmax=fmax)
    r.q.copy_(fl.record_rows(scales, amax, pow2))
    return r


def behind(t, fill=7.0):
    """an operand the epilogue reads row by row, with guard rows of a value no lattice holds behind it"""
    buf = torch.full((t.shape[0] + 264, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf


_SHARES = {}


def share(kind, value, bound, numel):
    """the share of elements whose interval admits more than one code: printed, recorded (the worst per kind over tensors of at least 4096
    elements - a single row of 512 scatters by a percent) and, on those, held to the bound that keeps the check sharp.  A condition on the
    inputs: tests/test_fp8_exact_cpu.py asserts it on the references of the same inputs."""
    print(f"[fp8_exact] {kind}: ambiguous share {value:.4f} of {numel}")
    if numel < 4096:
        return
    _SHARES[kind] = max(_SHARES.get(kind, 0.0), value)
    record_margin("fp8_exact/ambiguous_share", **_SHARES)
    assert value <= bound, (kind, value, bound)


def check_codes(kind, code8, bf16_out, scale, fmt):
    bad, amb = fl.codes_within(code8, bf16_out, scale, fmt)
    assert bad.numel() == 0, (kind, bad.numel(), bad[:8].tolist())
    share(kind, amb, fl.AMBIGUOUS_MAX[fmt], code8.numel())


# ===================================================================================================
# (a) (b) (c): avs_gemm_nt_fp8 on lattices
def run_nt(c, grad, out_kind, opt, use_records=False, m_split=0):
    """one call of ops.gemm_nt_fp8 in the form `opt` describes (fp8lib.nt_expected's options) -> what it wrote, under nt_expected's names;
    the guard bands are checked on the way"""
    o = ops()
    M, N = c["M"], c["N"]
    checks, got = {}, {}
    out = None
    if out_kind:
        out, checks[out_kind] = rw.guarded(M, N, BF if out_kind == "bf16" else F32, DEV)
    kw = dict(grad=grad, scale_cols=opt.get("scale_cols", 0), col_scale=opt.get("col_scale", 1.0))
    if opt.get("bias", True):
        kw["bias"] = c["bias"].to(DEV)
    if opt.get("res"):
        kw["res"] = behind(c["res"])
    if opt.get("aux"):
        kw["aux"], kw["act"] = behind(c["aux"]), 2
    cs = cs2 = None
    if opt.get("colsum"):
        cs = kw["colsum"] = c["colsum0"].to(DEV)
    alpha = opt.get("alpha", 1.0 / (c["sa"] * c["sw"]))
    if use_records or m_split:
        ab = records([c["sa"], c["sw"], c["sw2"]], fmax=BF8_MAX if grad else 448.0)
        kw["qa"], kw["qw"], alpha = ab.rec(0), ab.rec(1), 77.0                   # (the host factor is ignored beside records)
    if m_split:
        cs2 = c["colsum0_2"].to(DEV) if cs is not None else None
        kw["dual"] = (m_split, c["W8_2"].to(DEV), c["bias2"].to(DEV) if "bias" in kw else None, ab.rec(2), cs2)
    q8 = None
    if "q8_scale" in opt:
        kw["out8"], checks["out8"] = rw.guarded(M, N, U8, DEV)
        q8 = records([opt["q8_scale"]], [opt["amax0"]], fmax=BF8_MAX)
        kw["q8"] = q8.rec(0)
    o.gemm_nt_fp8(c["A8"].to(DEV), c["W8"].to(DEV), out, M, alpha, **kw)
    torch.cuda.synchronize()
    for k, chk in checks.items():
        got[k] = chk()
    if cs is not None:
        got["colsum"] = cs
    if cs2 is not None:
        got["colsum2"] = cs2
    if q8 is not None:
        got["amax"] = q8.amax(0)
        assert float(q8.q[0, 0]) == opt["q8_scale"] and float(q8.q[0, 3]) == 0.0          # the kernel writes nothing else into the record
    return got


@pytest.mark.parametrize("form", list(fl.NT_FORMS))
@pytest.mark.parametrize("M,N,K", fl.NT_SHAPES)
def test_gemm_nt_fp8_forms_equal_the_lattice_reference(M, N, K, form):
    """(a) every form of the table at M in {1, 17, 255, 256, 257, 513} (N 512, K 384: three K-slabs) and K in {256, 384, 640} (M 257, N 256):
    outputs, e5m2 copy, column sum and recorded amax equal the fp64 evaluation bit for bit.  Row M - 1 holds the column-wise and the global
    maximum at M = 17 / 257 (a duplicate of it counted into a column sum or the amax shows); the record starts above every |x| at M = 255,
    below elsewhere."""
    grad, out_kind, _ = fl.NT_FORMS[form]
    c = fl.nt_case(M, N, K, grad)
    opt = fl.nt_form_options(form, c)
    got = run_nt(c, grad, out_kind, opt, use_records=form.endswith("records"))
    assert fl.mismatches(got, fl.nt_expected(c, **opt)) == []


def test_gemm_nt_fp8_e5m2_copy_saturates_at_the_largest_finite_value():
    """(a) the one case meant to saturate: |x| * 1024 above 57344 in the whole last row"""
    M, N, K = fl.SAT_SHAPE
    c = fl.nt_case(M, N, K, True)
    opt = dict(bias=False, colsum=True, q8_scale=fl.Q8_SCALE_SAT, amax0=fl.AMAX_BELOW)
    assert fl.mismatches(run_nt(c, True, "bf16", opt), fl.nt_expected(c, **opt)) == []


@pytest.mark.parametrize("form", ["fwd_bf16_cols0", "fwd_bf16_cols192", "fwd_f32_res", "dgrad_bf16_out8", "dgrad_act2", "dgrad_act2_out8_only"])
def test_gemm_nt_fp8_two_weight_sets_equal_their_own_references(form):
    """(b) m_split 256, M 600 (three row tiles, the last one partial): rows from 256 meet the second weight set - its de-quantisation factor
    (sw2 = 4 sw), its bias, its column sum.  Each half equals its own reference, each column sum holds only its own rows."""
    grad, out_kind, _ = fl.NT_FORMS[form]
    c = fl.nt_case(600, 512, 384, grad)
    opt = dict(fl.nt_form_options(form, c), m_split=256)
    want = fl.nt_expected(c, **opt)
    got = run_nt(c, grad, out_kind, opt, m_split=256)
    assert fl.mismatches(got, want) == []
    if "colsum" in got:
        assert torch.equal(got["colsum"].cpu().double(), c["colsum0"].double() + want["x"][:256].sum(0))
        assert torch.equal(got["colsum2"].cpu().double(), c["colsum0_2"].double() + want["x"][256:].sum(0))


@pytest.mark.parametrize("form", ["fwd_bf16_cols64", "fwd_f32_res", "dgrad_act2"])
def test_gemm_nt_fp8_tile_walk_with_two_tiles_per_workgroup(form):
    """(c) cu_reserve 128 leaves avs_persistent_cu_slots() workgroups; M is chosen so that there are 6 (or 7) tiles more than that: some
    workgroups run two tiles - with the next tile's first K-slab requested before the epilogue (bf16 output, act 0) or after it (fp32
    output + residual, act 2).  N 512, K 256."""
    from avsiam_amd import _lib
    grad, out_kind, _ = fl.NT_FORMS[form]
    with fl.knobs(cu_reserve=128):
        slots = _lib.load().avs_persistent_cu_slots()
        row_tiles = (slots + 6 + 1) // 2
        M = (row_tiles - 1) * 256 + 17
        assert slots < row_tiles * 2 <= 2 * slots
        c = fl.nt_case(M, 512, 256, grad)
        opt = fl.nt_form_options(form, c)
        got = run_nt(c, grad, out_kind, opt)
    assert _lib.tuning_get("cu_reserve") == 0
    assert fl.mismatches(got, fl.nt_expected(c, **opt)) == []


# ===================================================================================================
# (d) the GELU forms
@pytest.mark.parametrize("M,N,K", fl.GELU_SHAPES)
def test_gemm_nt_fp8_gelu_forms(M, N, K):
    """act 1 on a lattice whose pre-activation x is known exactly (a 1/64 grid over about +-9): gelu(x) and gelu'(x) against fp64 erf-GELU of
    that x within the bf16 rounding (rowwise.gelu_bound / gelu_grad_bound with no error of x), the 8-bit gelu' codes within half a step plus
    the bf16 term of test_gemm_nt_fp8_gelu_grad_as_8_bit_codes, the e4m3 copy element by element inside the rounding interval of out2 (host
    scale and record), the out2=None form identical in its bytes, the recorded amax within 2^-8 of max |out2|."""
    o = ops()
    c = fl.gelu_case(M, N, K)
    x = fl.nt_expected(c, alpha=fl.GELU_ALPHA)["x"]
    g, gp = rw.gelu64(x), rw.gelu_grad64(x)
    A8, W8, bias = c["A8"].to(DEV), c["W8"].to(DEV), c["bias"].to(DEV)

    def run(codes, with_out2, host_scale=None, rec=None):
        out, chk = rw.guarded(M, N, U8 if codes else BF, DEV)
        out2, chk2 = rw.guarded(M, N, BF, DEV) if with_out2 else (None, None)
        kw = {}
        if host_scale is not None or rec is not None:
            kw["out8"], chk8 = rw.guarded(M, N, U8, DEV)
            kw["out8_scale"], kw["q8"] = host_scale if host_scale is not None else 123.0, rec
        o.gemm_nt_fp8(A8, W8, out, M, fl.GELU_ALPHA, bias=bias, out2=out2, act=1, **kw)
        torch.cuda.synchronize()
        return chk().cpu(), chk2().cpu() if with_out2 else None, chk8().cpu() if kw else None

    gp16, act16, _ = run(False, True)
    assert rw.elem_ratio(act16, g, rw.gelu_bound(0.0, g))[0] <= 1.0
    assert rw.elem_ratio(gp16, gp, rw.gelu_grad_bound(0.0, gp))[0] <= 1.0
    s = fl.quarter_scale(act16.float().abs().max(), E4M3)
    gp16b, act16b, a8_host = run(False, True, host_scale=s)
    assert torch.equal(gp16b, gp16) and torch.equal(act16b, act16)
    check_codes("gelu_e4m3", a8_host, act16, s, E4M3)
    rec = records([s], fmax=448.0, pow2=False)
    gp8, act8, a8_rec = run(True, True, rec=rec.rec(0))
    assert torch.equal(act8, act16) and torch.equal(a8_rec, a8_host)
    assert fl.amax_close(rec.amax(0), act16)
    dec = rw.gp8_value(gp8)
    assert float((dec - gp).abs().max()) < 0.0025 + 0.0045
    rec2 = records([s], fmax=448.0, pow2=False)
    gp8b, _, a8_lean = run(True, False, rec=rec2.rec(0))
    assert torch.equal(a8_lean, a8_host) and torch.equal(gp8b, gp8) and rec2.amax(0) == rec.amax(0)


# ===================================================================================================
# (e) avs_gemm_tn_fp8_group3
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("M", fl.TN_M)
def test_gemm_tn_fp8_group_equals_the_lattice_reference(M, det):
    """C_before + A^T . B / (sa sb) with e5m2 A in {-2..2} sa and e4m3 B in {-1, 0, 1} sb: the three-problem group (256 x 512, 512 x 256,
    256 x 256, three scale pairs) and the single 256 x 256 problem, bit for bit; again with 64 rows of non-zero lattice values behind the
    64-row zero pad of the contract - the result must not change: the kernel reads nothing past the pad."""
    o = ops()
    with fl.knobs(det=det):
        for extra in (0, 64):
            cases = [fl.tn_lattice(M, N1, N2, sa, sb, extra_rows=extra) for (N1, N2), (sa, sb) in zip(fl.TN_SHAPES, fl.TN_SCALES)]
            recs = records([s for c in cases for s in (c["sa"], c["sb"])], fmax=BF8_MAX)
            jobs = [(c["A8"].to(DEV), c["B8"].to(DEV), c["C0"].to(DEV).reshape(-1).clone(), recs.rec(2 * i), recs.rec(2 * i + 1)) for i, c in enumerate(cases)]
            o.gemm_tn_fp8_group(jobs, M)
            A8, B8, _, qa, qb = jobs[2]
            alone = cases[2]["C0"].to(DEV).reshape(-1).clone()
            o.gemm_tn_fp8_group([(A8, B8, alone, qa, qb)], M)
            torch.cuda.synchronize()
            for c, job in zip(cases, jobs):
                want = fl.tn_expected(c)
                assert fl.mismatches({"C": job[2].view_as(want)}, {"C": want}) == [], (extra, c["A8"].shape, c["B8"].shape)
            assert fl.mismatches({"C": alone.view(256, 256)}, {"C": fl.tn_expected(cases[2])}) == [], extra


# ===================================================================================================
# (f) LayerNorm
def ln_inputs(D, rows):
    c = fl.ln_case(D)
    d = {k: [t.to(DEV) for t in v] if isinstance(v, list) else v[:rows].to(DEV).contiguous() for k, v in c.items()}
    return d


def ln_forward(d, rows, D, mod, y8=False, y=True, host_scale=None, rec=None):
    o = ops()
    yb, chk = rw.guarded(rows, D, BF, DEV, extra_rows=40) if y else (None, None)
    y8b, chk8 = rw.guarded(rows, D, U8, DEV, extra_rows=40) if y8 else (None, None)
    mean, rstd = torch.full((rows + 8,), 7.0, device=DEV), torch.full((rows + 8,), 7.0, device=DEV)
    kw = dict(g1=d["g"][1], b1=d["b"][1], row_mod=d["mod"]) if mod else {}
    if y8:
        kw.update(y8=y8b, q8=host_scale if host_scale is not None else 123.0, q8_dev=rec)
    o.layernorm_fwd(d["x"], d["g"][0], d["b"][0], yb, mean, rstd, rows, 1e-5, **kw)
    torch.cuda.synchronize()
    assert bool((mean[rows:] == 7.0).all()) and bool((rstd[rows:] == 7.0).all())
    return chk().cpu() if y else None, chk8().cpu() if y8 else None, mean[:rows].cpu(), rstd[:rows].cpu()


@pytest.mark.parametrize("rows", fl.LN_ROWS)
@pytest.mark.parametrize("D", fl.LN_D)
def test_layernorm_fwd_e4m3_copy(D, rows):
    """y8 with a record (ln_fwd_kernel<NV, false, 8>: eight rows per wave, rows of both affine sets among them) and, at D 768 / 1280, with a
    host scale (the four-rows-per-block kernel): mean, rstd and the bf16 y bitwise those of the call without the copy, the copy inside the
    rounding interval of y element by element, the y=None form identical in its bytes, guard rows untouched, the amax within 2^-8."""
    d = ln_inputs(D, rows)
    for mod in (False, True):
        y0, _, mean0, rstd0 = ln_forward(d, rows, D, mod)
        s = fl.quarter_scale(y0.float().abs().max(), E4M3)
        rec = records([s], pow2=False)
        y, y8, mean, rstd = ln_forward(d, rows, D, mod, y8=True, rec=rec.rec(0))
        assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        check_codes("layernorm_y8_e4m3", y8, y0, s, E4M3)
        assert fl.amax_close(rec.amax(0), y0)
        rec2 = records([s], pow2=False)
        _, y8b, mean, rstd = ln_forward(d, rows, D, mod, y8=True, y=False, rec=rec2.rec(0))
        assert torch.equal(y8b, y8) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0) and rec2.amax(0) == rec.amax(0)
        if D in fl.LN_HOST_D:
            y, y8h, mean, rstd = ln_forward(d, rows, D, mod, y8=True, host_scale=s)
            assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0) and torch.equal(y8h, y8)
            _, y8hb, _, _ = ln_forward(d, rows, D, mod, y8=True, y=False, host_scale=s)
            assert torch.equal(y8hb, y8)


def test_layernorm_fwd_e4m3_copy_follows_out_map():
    """The kernel writes the e4m3 copy to the row out_map names, like y.  ops.layernorm_fwd refuses the combination (no caller has it);
    through the C ABI it holds: row out_map[r] of y and y8 is row r of the plain call."""
    from avsiam_amd import _lib
    o = ops()
    D, rows = 768, 33
    d = ln_inputs(D, rows)
    y0, _, mean0, rstd0 = ln_forward(d, rows, D, True)
    s = fl.quarter_scale(y0.float().abs().max(), E4M3)
    rec = records([s], pow2=False)
    _, y8_0, _, _ = ln_forward(d, rows, D, True, y8=True, y=False, rec=rec.rec(0))
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    omap = perm.to(DEV)
    yb, chk = rw.guarded(rows, D, BF, DEV, extra_rows=40)
    y8b, chk8 = rw.guarded(rows, D, U8, DEV, extra_rows=40)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    with pytest.raises(AssertionError):
        o.layernorm_fwd(d["x"], d["g"][0], d["b"][0], yb, mean, rstd, rows, 1e-5, g1=d["g"][1], b1=d["b"][1], row_mod=d["mod"], out_map=omap, y8=y8b, q8_dev=rec.rec(0))
    rec2 = records([s], pow2=False)
    _lib.call("avs_layernorm_fwd_q8", d["x"], d["g"][0], d["b"][0], d["g"][1], d["b"][1], d["mod"], omap, yb, 0, mean, rstd, rows, D, 1e-5, y8b, 1.0,
              rec2.rec(0), _lib.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(chk().cpu()[perm.long()], y0) and torch.equal(chk8().cpu()[perm.long()], y8_0)
    assert torch.equal(mean.cpu(), mean0) and torch.equal(rstd.cpu(), rstd0) and rec2.amax(0) == rec.amax(0)


@pytest.mark.parametrize("rows", fl.LN_BWD_ROWS)
@pytest.mark.parametrize("D", fl.LN_BWD_D)
@pytest.mark.parametrize("path", ["registers", "dma"])
def test_layernorm_bwd_e5m2_copy(path, D, rows):
    """dx8 on the register-load kernel (fp32 residual gradient, fp32 and bf16 dx) and on the LDS-DMA kernel (bf16 dy, bf16 dres, bf16 dx
    only), one and two affine sets: the bf16 dx (and the fp32 one) bitwise those of the call without the copy, the copy inside the rounding
    interval of the bf16 dx element by element, guard rows untouched, the amax within 2^-8."""
    o = ops()
    d = ln_inputs(D, rows)
    dma = path == "dma"
    dres = d["dres"].to(BF) if dma else d["dres"]
    for mod in (False, True):
        _, _, mean, rstd = ln_forward(d, rows, D, mod)
        mean, rstd = mean.to(DEV), rstd.to(DEV)

        def run(rec=None):
            dxb, chk = rw.guarded(rows, D, BF, DEV, extra_rows=40)
            dx, chk32 = (None, None) if dma else rw.guarded(rows, D, F32, DEV, extra_rows=40)
            dx8, chk8 = rw.guarded(rows, D, U8, DEV, extra_rows=40) if rec is not None else (None, None)
            dg = [torch.zeros(D, device=DEV) for _ in range(4)]
            ws = torch.empty(o.layernorm_ws(rows, D), device=DEV)
            kw = dict(g1=d["g"][1], dg1=dg[2], db1=dg[3], row_mod=d["mod"]) if mod else {}
            o.layernorm_bwd(d["dy"], d["x"], mean, rstd, d["g"][0], dx, dg[0], dg[1], ws, rows, dres=dres, dx_bf16=dxb, dx8=dx8, q8=rec, **kw)
            torch.cuda.synchronize()
            return chk().cpu(), None if dma else chk32().cpu(), chk8().cpu() if rec is not None else None

        dxb0, dx0, _ = run()
        s = fl.quarter_scale(dxb0.float().abs().max(), E5M2)
        rec = records([s], fmax=BF8_MAX, pow2=False)
        dxb, dx, dx8 = run(rec.rec(0))
        assert torch.equal(dxb, dxb0) and (dma or torch.equal(dx, dx0))
        check_codes("layernorm_dx8_e5m2", dx8, dxb0, s, E5M2)
        assert fl.amax_close(rec.amax(0), dxb0)


# ===================================================================================================
# (g) attention forward
@pytest.mark.parametrize("tile_rows", [64, 128])
@pytest.mark.parametrize("H,hd", fl.ATTN_HEADS)
def test_attention_fwd_e4m3_copy(H, hd, tile_rows):
    """out8 beside the bf16 output at sequence lengths 1, 39, 64, 65, 200: the bf16 output bitwise that of the plain call, the copy inside
    the rounding interval of it element by element, rows behind the sequences untouched, the amax within 2^-8."""
    o = ops()
    lens, D = fl.ATTN_LENS, H * hd
    rows = sum(lens)
    rp = o.pad_rows(rows, 256)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=BF)
    qkv[:rows] = rw.attn_case(H, hd, lens)["qkv"].to(DEV)
    tiles = o.AttnTiles(lens, DEV, tile_rows=tile_rows)

    def run(rec=None):
        out, chk = rw.guarded(rows, D, BF, DEV)
        out8, chk8 = rw.guarded(rows, D, U8, DEV) if rec is not None else (None, None)
        lse = torch.zeros(H, rp, device=DEV)
        o.attn_fwd(qkv, tiles, H, out, lse, out8=out8, q8=rec)
        torch.cuda.synchronize()
        return chk().cpu(), chk8().cpu() if rec is not None else None, lse[:, :rows].cpu()

    out0, _, lse0 = run()
    s = fl.quarter_scale(out0.float().abs().max(), E4M3)
    rec = records([s], pow2=False)
    out, out8, lse = run(rec.rec(0))
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    check_codes("attention_out8_e4m3", out8, out0, s, E4M3)
    assert fl.amax_close(rec.amax(0), out0)
