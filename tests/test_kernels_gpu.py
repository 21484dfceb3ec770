"""Per-kernel numerics on a real MI355X: every HIP kernel (called through the C ABI) against a plain
PyTorch fp32/fp64 reference of the same op on the same inputs.  bf16-operand kernels are compared against the
reference evaluated on the SAME bf16-rounded operands (so the tolerance covers only accumulation order and the
bf16 rounding of the output)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_rowwise_gpu import A_FUSED, A_FUSED224, PASS_BWD, PASS_FUSED, PASS_FWD, attn_meant, attn_reached

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    torch.manual_seed(0)


def ops():
    from avsiam_amd import ops as o
    return o


def bf(x):
    return x.to(torch.bfloat16)


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


@pytest.mark.parametrize("D,rows", [(768, 1000), (512, 333), (1024, 70)])
def test_layernorm(D, rows):
    o = ops()
    x = torch.randn(rows, D, device=DEV) * 2 + 0.3
    g = [torch.randn(D, device=DEV) * 0.1 + 1 for _ in range(2)]
    b = [torch.randn(D, device=DEV) * 0.1 for _ in range(2)]
    mod = (torch.rand(rows, device=DEV) > 0.5).to(torch.uint8)
    perm = torch.randperm(rows, device=DEV).to(torch.int32)
    y = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    mean = torch.empty(rows, device=DEV); rstd = torch.empty(rows, device=DEV)
    o.layernorm_fwd(x, g[0], b[0], y, mean, rstd, rows, 1e-5, g[1], b[1], mod, perm)
    xr = x.double().requires_grad_(True)
    gr = [t.double().requires_grad_(True) for t in g]
    br = [t.double().requires_grad_(True) for t in b]
    y0 = F.layer_norm(xr, (D,), gr[0], br[0], 1e-5)
    y1 = F.layer_norm(xr, (D,), gr[1], br[1], 1e-5)
    yr = torch.where(mod.bool()[:, None], y1, y0)
    got = y.double()[perm.long()]                     # output row r was redirected to y[out_map[r]]
    assert rel_err(got, yr) < 4e-3
    # backward
    dy_nat = torch.randn(rows, D, device=DEV)
    dy = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    dy[perm.long()] = bf(dy_nat)
    dres = torch.randn(rows, D, device=DEV)
    dx = torch.empty(rows, D, device=DEV)
    dg = [torch.zeros(D, device=DEV) for _ in range(2)]
    db = [torch.zeros(D, device=DEV) for _ in range(2)]
    ws = torch.empty(o.layernorm_ws(rows, D), device=DEV)
    o.layernorm_bwd(dy, x, mean, rstd, g[0], dx, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres)
    (yr * bf(dy_nat).double()).sum().backward()
    assert rel_err(dx, xr.grad + dres.double()) < 1e-4
    for i in range(2):
        assert rel_err(dg[i], gr[i].grad) < 1e-4
        assert rel_err(db[i], br[i].grad) < 1e-4
    # fp32 I/O mode (final norms) + fused bf16 copy of dx
    yf = torch.zeros(rows, D, device=DEV)
    o.layernorm_fwd(x, g[0], b[0], yf, mean, rstd, rows, 1e-6, g[1], b[1], mod, perm)
    y0 = F.layer_norm(x.double(), (D,), g[0].double(), b[0].double(), 1e-6)
    y1 = F.layer_norm(x.double(), (D,), g[1].double(), b[1].double(), 1e-6)
    assert rel_err(yf.double()[perm.long()], torch.where(mod.bool()[:, None], y1, y0)) < 1e-5
    dyf = torch.zeros(rows, D, device=DEV)
    dyf[perm.long()] = bf(dy_nat).float()
    dx2 = torch.empty(rows, D, device=DEV)
    dxb = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    o.layernorm_fwd(x, g[0], b[0], yf, mean, rstd, rows, 1e-5, g[1], b[1], mod, perm)
    dcol = torch.ones(D, device=DEV)
    o.layernorm_bwd(dyf, x, mean, rstd, g[0], dx2, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres, dxb, dcol)
    assert rel_err(dx2, dx) < 1e-6
    assert torch.equal(dxb, bf(dx2))
    assert rel_err(dcol, 1 + dx2.double().sum(0)) < 1e-5           # fused column sum (bias gradient), accumulated
    # bf16 residual-gradient stream (EngineOptions.grad_stream): dres arrives in bf16, only the bf16 copy is written; the sum is formed in
    # fp32 and rounded once, so the result is the bf16 rounding of the fp32-path sum on the rounded dres
    dres_b = bf(dres)
    dxb2 = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    dcol2 = torch.zeros(D, device=DEV)
    o.layernorm_bwd(dyf, x, mean, rstd, g[0], None, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres_b, dxb2, dcol2)
    dx3 = torch.empty(rows, D, device=DEV)
    o.layernorm_bwd(dyf, x, mean, rstd, g[0], dx3, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres_b.float(), None)
    assert torch.equal(dxb2, bf(dx3))
    assert rel_err(dcol2, dx3.double().sum(0)) < 1e-5
    with pytest.raises(AssertionError):                          # in-place on the bf16 stream is refused
        o.layernorm_bwd(dyf, x, mean, rstd, g[0], None, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres_b, dres_b)


@pytest.mark.parametrize("D", [512, 768, 1280])
def test_layernorm_bwd_deferred_reduce(D):
    """avs_layernorm_bwd without gradient targets leaves its per-block partial sums in the call's workspace; avs_layernorm_bwd_reduce_batched adds the
    slabs of MANY such calls to their targets in one launch (engine: one reduce per stack backward instead of one per LayerNorm).  Three calls of
    different row counts (8- and 16-rows-per-wave block counts, a last block with missing rows), with and without a second affine set and a column-sum
    target, accumulating onto what the targets hold: dx BITWISE the direct call's, the parameter gradients equal up to the order of the fp32 atomics."""
    o = ops()
    calls = []
    for rows, two, col in ((1000, True, True), (20001, False, True), (16500, True, False)):
        x = torch.randn(rows, D, device=DEV) * 2 + 0.3
        mean = x.mean(1).contiguous()
        rstd = (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).contiguous()
        calls.append(dict(rows=rows, x=x, mean=mean, rstd=rstd, g=[torch.randn(D, device=DEV) * 0.1 + 1 for _ in range(2)],
                          mod=(torch.rand(rows, device=DEV) > 0.5).to(torch.uint8) if two else None, col=col,
                          dy=bf(torch.randn(rows, D, device=DEV)), dres=bf(torch.randn(rows, D, device=DEV))))

    def targets():
        return [[torch.full((D,), 0.5, device=DEV) for _ in range(5)] for _ in calls]       # dg0, db0, dg1, db1, dcol: accumulated onto

    def run(c, t, ws, defer):
        two = c["mod"] is not None
        dxb = torch.zeros(c["rows"], D, device=DEV, dtype=torch.bfloat16)
        o.layernorm_bwd(c["dy"], c["x"], c["mean"], c["rstd"], c["g"][0], None, t[0], t[1], ws, c["rows"], c["g"][1] if two else None, t[2] if two else None,
                        t[3] if two else None, c["mod"], None, c["dres"], dxb, t[4] if c["col"] else None, defer=defer)
        return dxb

    want_t = targets()
    want_dx = [run(c, t, torch.empty(o.layernorm_ws(c["rows"], D), device=DEV), False) for c, t in zip(calls, want_t)]
    got_t = targets()
    batch = o.LnReduceBatch(D)
    wss = []
    for c, t in zip(calls, got_t):
        two = c["mod"] is not None
        wss.append(torch.full((o.layernorm_bwd_slabs(c["rows"]) * 5 * D,), float("nan"), device=DEV))      # exactly the slabs: every one is written
        batch.add(wss[-1], c["rows"], t[0], t[1], t[2] if two else None, t[3] if two else None, t[4] if c["col"] else None)
    batch.build(DEV)
    for rep in range(2):                                          # the table is reused step after step
        got_dx = [run(c, t, ws, True) for c, t, ws in zip(calls, got_t, wss)]
        for t in got_t:
            assert all(float((v - 0.5).abs().max()) == 0.0 for v in t) or rep == 1      # nothing reduced before run()
        batch.run()
        for a, b_ in zip(got_dx, want_dx):
            assert torch.equal(a, b_)
    for c, gt, wt in zip(calls, got_t, want_t):
        two = c["mod"] is not None
        for k in range(5):
            live = k < 2 or (k < 4 and two) or (k == 4 and c["col"])
            if live:
                assert rel_err(gt[k] - 0.5, 2.0 * (wt[k] - 0.5)) < 2e-5, (c["rows"], k)      # two runs of the batch onto the same targets
            else:
                assert float((gt[k] - 0.5).abs().max()) == 0.0, (c["rows"], k)


@pytest.mark.parametrize("D,rows", [(768, 1000), (768, 20001), (512, 16500), (1024, 777), (1280, 3001), (1280, 17000)])
def test_layernorm_bwd_dma_kernel(D, rows):
    """The step's common LayerNorm backward - bf16 dy, bf16 residual-gradient stream in, bf16 dx out only - runs the LDS-DMA kernel
    (ln_bwd_dma_kernel: next row prefetched into LDS under the current row's reductions, counted waits, DPP row sums).  Against an fp64
    reference of the same formula, and against the register-load kernel (same call with an fp32 dx requested): equal up to the order of
    the two row sums - the bf16 outputs may differ by one rounding in a handful of elements.  Random per-row modality (gamma is
    re-loaded whenever it changes), permuted dy rows (out_map), 8 and 16 rows per wave, a last block with missing rows."""
    o = ops()
    x = torch.randn(rows, D, device=DEV) * 2 + 0.3
    g = [torch.randn(D, device=DEV) * 0.1 + 1 for _ in range(2)]
    mod = (torch.rand(rows, device=DEV) > 0.5).to(torch.uint8)
    mod[: rows // 3] = 0                                           # and a long run of one modality
    perm = torch.randperm(rows, device=DEV).to(torch.int32)
    mean = x.mean(1).contiguous()
    rstd = (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).contiguous()
    dy_nat = bf(torch.randn(rows, D, device=DEV))
    dy = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    dy[perm.long()] = dy_nat
    dres = bf(torch.randn(rows, D, device=DEV))
    ws = torch.empty(o.layernorm_ws(rows, D), device=DEV)

    def run(dx):
        dg = [torch.zeros(D, device=DEV) for _ in range(2)]
        db = [torch.zeros(D, device=DEV) for _ in range(2)]
        dxb = torch.full((rows, D), float("nan"), device=DEV, dtype=torch.bfloat16)
        dcol = torch.zeros(D, device=DEV)
        o.layernorm_bwd(dy, x, mean, rstd, g[0], dx, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres, dxb, dcol)
        return dxb, dg, db, dcol

    dxb, dg, db, dcol = run(None)                                  # -> ln_bwd_dma_kernel
    dx_ref = torch.empty(rows, D, device=DEV)
    dxb_r, dg_r, db_r, dcol_r = run(dx_ref)                        # an fp32 dx is wanted too -> the register-load kernel
    assert torch.isfinite(dxb.float()).all()
    diff = (dxb.float() != dxb_r.float())
    if float(diff.float().mean()) >= 1e-3:                          # say WHERE before failing: which rows, how far
        rowbad = diff.float().mean(1)
        bad_rows = torch.nonzero(rowbad > 0.5).flatten()[:24].tolist()
        per_row = ((dxb.float() - dxb_r.float()).norm(dim=1) / dxb_r.float().norm(dim=1))
        raise AssertionError(f"{float(diff.float().mean()):.4f} of the elements differ; rel err {rel_err(dxb.float(), dxb_r.float()):.3e}; rows mostly different: "
                             f"{int((rowbad > 0.5).sum())} of {rows}, first {bad_rows}; per-row rel err of rows 0..15: {[round(float(v), 4) for v in per_row[:16]]}; "
                             f"mod of rows 0..15: {mod[:16].tolist()}")
    assert rel_err(dxb.float(), dxb_r.float()) < 1e-4
    for a, b_ in zip(dg + db + [dcol], dg_r + db_r + [dcol_r]):
        assert rel_err(a, b_) < 2e-5
    # fp8 backward (round 5): the DMA kernel also writes the e5m2 copy of dx with its device record - same bytes and the same running amax as
    # the register-load kernel's (which the fp32-dx request selects), wherever the two bf16 outputs agree
    def run8(dx):
        rec = o.Fp8Records(1, DEV)
        rec.q[0, 0], rec.q[0, 1] = 64.0, 1.0 / 64.0
        dg = [torch.zeros(D, device=DEV) for _ in range(2)]
        db = [torch.zeros(D, device=DEV) for _ in range(2)]
        dxb8 = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
        d8 = torch.zeros(rows, D, device=DEV, dtype=torch.uint8)
        o.layernorm_bwd(dy, x, mean, rstd, g[0], dx, dg[0], db[0], ws, rows, g[1], dg[1], db[1], mod, perm, dres, dxb8, None, dx8=d8, q8=rec.rec(0))
        return dxb8, d8, rec.amax(0)

    b_dma, d8_dma, q_dma = run8(None)
    b_reg, d8_reg, q_reg = run8(torch.empty(rows, D, device=DEV))
    assert torch.equal(b_dma, dxb)                                                 # the bf16 output does not depend on the extra copy
    same = (b_dma.float() == b_reg.float())
    assert float((d8_dma != d8_reg)[same].float().mean()) < 1e-3                   # (fp32 o differs in its last bits between the kernels: rare e5m2 flips)
    want8 = (b_reg.float() * 64.0).clamp(-57344, 57344).to(torch.float8_e5m2).view(torch.uint8)
    assert float((d8_dma != want8).float().mean()) < 0.02                          # against the quantised bf16 output: e5m2 of the fp32 value, not of its bf16 rounding
    assert abs(q_dma - q_reg) <= 1e-5 * abs(q_reg) and q_dma > 0, (q_dma, q_reg)      # the running amax of the record
    # fp64 reference of the formula
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gam = torch.where(mod.bool()[:, None], g[1].double(), g[0].double())
    gy = dy_nat.double() * gam
    want = rstd.double()[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True)) + dres.double()
    assert rel_err(dxb.float(), want) < 3e-3                       # bf16 rounding of the output
    assert rel_err(dcol, want.sum(0)) < 1e-4
    for i in range(2):
        sel = (mod == i).double()[:, None]
        assert rel_err(dg[i], (dy_nat.double() * xh * sel).sum(0)) < 1e-4
        assert rel_err(db[i], (dy_nat.double() * sel).sum(0)) < 1e-4


@pytest.mark.parametrize("M,N,K", [(333, 256, 768), (1000, 768, 3072), (4099, 2304, 768), (128, 512, 256), (25700, 768, 768)])
def test_gemm_nt_epilogues(M, N, K):
    o = ops()
    A = bf(torch.randn(M, K, device=DEV))
    W = bf(torch.randn(N, K, device=DEV) * 0.05)
    bias = torch.randn(N, device=DEV)
    ref = A.double() @ W.double().t()
    out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    o.gemm_nt(A, W, out, M, bias=bias)
    assert rel_err(out, ref + bias.double()) < 4e-3
    # fp32 out + residual (row-gathered) + alpha
    res = torch.randn(50, N, device=DEV)
    idx = torch.randint(0, 50, (M,), device=DEV, dtype=torch.int32)
    outf = torch.zeros(M, N, device=DEV)
    o.gemm_nt(A, W, outf, M, bias=bias, res=res, res_idx=idx, alpha=2.0)
    assert rel_err(outf, 2 * (ref + bias.double() + res.double()[idx.long()])) < 1e-5
    res2 = torch.randn(M, N, device=DEV)
    o.gemm_nt(A, W, outf, M, bias=bias, res=res2)
    assert rel_err(outf, ref + bias.double() + res2.double()) < 1e-5
    # column-ranged scale (q part of the qkv projection)
    sc = (N // 128) * 64
    o.gemm_nt(A, W, outf, M, bias=bias, scale_cols=sc, col_scale=0.25)
    want = ref + bias.double()
    want[:, :sc] *= 0.25
    assert rel_err(outf, want) < 1e-5
    o.gemm_nt(A, W, out, M, bias=bias, scale_cols=sc, col_scale=0.25)
    assert rel_err(out, want) < 4e-3
    # gelu forward epilogue: out = gelu'(x) (what the backward needs of the pre-activation), out2 = gelu(x)
    dact = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    act = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    o.gemm_nt(A, W, dact, M, bias=bias, out2=act, act=1)
    p = (ref + bias.double()).requires_grad_(True)
    F.gelu(p).sum().backward()
    assert rel_err(dact, p.grad) < 4e-3
    assert float((dact.double() - p.grad).abs().max()) < 8e-3     # gelu' in [-0.13, 1.13]: bf16 rounding + the 5e-5 fit error
    assert rel_err(act, F.gelu(p.detach())) < 5e-3
    # gelu backward epilogue: out = (A W^T) * aux with aux = the saved gelu'(x)
    dpre = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    csum = torch.ones(N, device=DEV)
    o.gemm_nt(A, W, dpre, M, aux=dact, act=2, colsum=csum)
    want = ref * dact.double()
    assert rel_err(dpre, want) < 5e-3
    assert rel_err(csum, 1 + want.sum(0)) < 2e-3                  # fused column sum (bias gradient), accumulated
    # gelu'(x) as 8-bit fixed-point codes in the bf16 GEMMs (EngineOptions.gelu8: a uint8 `out` with act 1, a uint8 `aux` with act 2): the codes
    # decode to the bf16 epilogue's gelu' within half a step (1 / 404) + its bf16 rounding, gelu(x) is bitwise unchanged, and the input gradient
    # formed with the codes equals the one formed with the bf16 operand to the codes' resolution
    codes = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    act8 = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    o.gemm_nt(A, W, codes, M, bias=bias, out2=act8, act=1)
    dec = codes.double() / 202.0 - 0.1296875
    assert torch.equal(act8, act)
    assert float((dec - dact.double()).abs().max()) <= 0.5 / 202 + 4e-3, float((dec - dact.double()).abs().max())
    dpre8 = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    csum8 = torch.ones(N, device=DEV)
    o.gemm_nt(A, W, dpre8, M, aux=codes, act=2, colsum=csum8)
    assert rel_err(dpre8, ref * dec) < 5e-3 and rel_err(dpre8, want) < 8e-3
    assert rel_err(csum8, 1 + (ref * dec).sum(0)) < 2e-3


@pytest.mark.parametrize("M,N,K", [(708, 768, 768), (1979, 2304, 768), (2832, 512, 2048), (333, 256, 256), (2048, 768, 3072), (130, 3072, 768)])
def test_gemm_nt_ring_kernel_for_small_problems_matches_the_two_buffer_kernel(M, N, K):
    """gemm_nt_ring_kernel (round 5: the forward / input-gradient GEMMs of small batches - at most one 128 x 128 workgroup per CU - keep three
    K-slabs in flight in a 4-slot LDS-DMA ring instead of one) against gemm_nt_kernel<., 2, 4>: same tiles, fragments, MFMA order and
    epilogue, so every epilogue variant must be BITWISE equal - bf16 out with column scale, fp32 out + residual, the GELU pair, the GELU'
    input gradient with its fused column sum (to the order of the fp32 atomics), and two weight sets in one launch.  Three repetitions with
    other traffic in between as a race screen of the ring's counted waits.  Shapes: the reference's batch-4 step (708 / 1979 / 2832 rows)."""
    from avsiam_amd import _lib
    o = ops()
    A = bf(torch.randn(M, K, device=DEV))
    W = bf(torch.randn(N, K, device=DEV) * 0.05)
    W2 = bf(torch.randn(N, K, device=DEV) * 0.05)
    bias, bias2 = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    res = torch.randn(M, N, device=DEV)
    split = 256 if M > 512 else 0

    def run():
        out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        o.gemm_nt(A, W, out, M, bias=bias, scale_cols=(N // 128) * 64, col_scale=0.25)
        outf = torch.zeros(M, N, device=DEV)
        o.gemm_nt(A, W, outf, M, bias=bias, res=res)
        pre = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        act = torch.zeros_like(pre)
        o.gemm_nt(A, W, pre, M, bias=bias, out2=act, act=1)
        dpre = torch.zeros_like(pre)
        cs = torch.zeros(N, device=DEV)
        o.gemm_nt(A, W, dpre, M, aux=pre, act=2, colsum=cs)
        outs = [out, outf, pre, act, dpre]
        if split:
            d = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
            o.gemm_nt(A, W, d, M, bias=bias, dual=(split, W2, bias2, None))
            outs.append(d)
        return outs, cs

    try:
        _lib.tuning_set("gemm_ring", 0)
        want, wcs = run()
        for rep in range(4):
            _lib.tuning_set("gemm_ring", 1 if rep < 2 else 2)          # 2: half-height tiles for the shapes under half the CUs, else the ring
            got, gcs = run()
            for i, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), (i, rep, float((g.float() - w.float()).abs().max()))
            assert rel_err(gcs, wcs) < 1e-5
            torch.zeros(32 << 20, device=DEV).add_(1.0)
    finally:
        _lib.tuning_set("gemm_ring", 2)
    ref = A.double() @ W.double().t() + bias.double()
    assert rel_err(want[1], ref + res.double()) < 1e-5


@pytest.mark.parametrize("M,N,K", [(11328, 768, 3072), (16384, 768, 768), (11328, 768, 2304), (9000, 1024, 512)])
def test_gemm_nt_midsize_problems_agree_across_kernel_families(M, N, K):
    """128 ... 224 output tiles of 256^2 (the reference's one-frame shapes at batch 64: 11 328 rows): since round 5 these run the persistent 256^2
    kernel on a part of the chip instead of 128 x 128 tiles in two rounds (knob nt_big_min, default half the CU slots).  Both families accumulate
    K in the same order with the same per-element epilogue arithmetic, so every epilogue variant is BITWISE the same whichever side of the
    threshold a problem falls on (column sums: to the order of the fp32 atomics)."""
    from avsiam_amd import _lib
    o = ops()
    A = bf(torch.randn(M, K, device=DEV))
    W = bf(torch.randn(N, K, device=DEV) * 0.05)
    W2 = bf(torch.randn(N, K, device=DEV) * 0.05)
    bias, bias2 = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    res = torch.randn(M, N, device=DEV)

    def run():
        out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        o.gemm_nt(A, W, out, M, bias=bias, scale_cols=(N // 128) * 64, col_scale=0.25)
        outf = torch.zeros(M, N, device=DEV)
        o.gemm_nt(A, W, outf, M, bias=bias, res=res)
        pre = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        act = torch.zeros_like(pre)
        o.gemm_nt(A, W, pre, M, bias=bias, out2=act, act=1)
        dpre = torch.zeros_like(pre)
        cs = torch.zeros(N, device=DEV)
        o.gemm_nt(A, W, dpre, M, aux=pre, act=2, colsum=cs)
        d = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        o.gemm_nt(A, W, d, M, bias=bias, dual=(4096, W2, bias2, None))
        return [out, outf, pre, act, dpre, d], cs

    try:
        _lib.tuning_set("nt_big_min", 1 << 20)         # 128 x 128 kernels
        want, wcs = run()
        for big_min in (0, 1):                          # the default threshold; the persistent kernel whatever the tile count
            _lib.tuning_set("nt_big_min", big_min)
            got, gcs = run()
            for i, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), (i, big_min, float((g.float() - w.float()).abs().max()))
            assert rel_err(gcs, wcs) < 1e-5
    finally:
        _lib.tuning_set("nt_big_min", 0)
    ref = A.double() @ W.double().t() + bias.double()
    assert rel_err(want[1], ref + res.double()) < 1e-5


@pytest.mark.parametrize("M,N,K", [(33000, 768, 256), (70001, 512, 2048), (95630, 768, 768), (66000, 256, 128), (40001, 512, 192),
                                   (158208, 2048, 512)])
def test_gemm_nt_8phase_matches_two_buffer_kernel(M, N, K):
    """The 8-phase kernel accumulates in the same order as the two-buffer kernel and applies the same per-element arithmetic,
    so every epilogue variant must agree BITWISE (several tiles per workgroup, ragged last row tile, 2 / 3 / many K-tiles per
    tile): a stale or early-read staging granule or a mis-counted wait shows up here as a differing tile."""
    from avsiam_amd import _lib
    o = ops()
    lib = _lib.load()
    A = bf(torch.randn(M, K, device=DEV))
    W = bf(torch.randn(N, K, device=DEV) * 0.05)
    bias = torch.randn(N, device=DEV)
    res = torch.randn(M, N, device=DEV)

    def run():
        out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        o.gemm_nt(A, W, out, M, bias=bias, scale_cols=(N // 128) * 64, col_scale=0.25)
        outf = torch.zeros(M, N, device=DEV)
        o.gemm_nt(A, W, outf, M, bias=bias, res=res)
        pre = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        act = torch.zeros_like(pre)
        o.gemm_nt(A, W, pre, M, bias=bias, out2=act, act=1)
        dpre = torch.zeros_like(pre)
        o.gemm_nt(A, W, dpre, M, aux=pre, act=2)
        return out, outf, pre, act, dpre

    try:
        lib.avs_gemm_set_nt8(0)
        want = run()
        lib.avs_gemm_set_nt8(1)
        # every tile-height layout of the 8-phase kernel (all 256 rows / all 224 / half the row tiles of each / 0 = the host's own mix for
        # this shape): the K loop and the per-element arithmetic do not depend on it, so the results stay bitwise the same
        from avsiam_amd import _lib
        for height, reserve in ((256, 0), (224, 0), (240, 0), (0, 0), (0, 8), (0, 24)):
            # (cu_reserve, round 5: under data parallelism every persistent grid leaves CUs to RCCL's kernels - 248 or 232 workgroups walk
            #  the same tiles, with the host's height mix recomputed for that many slots)
            lib.avs_gemm_set_tile_height(height)
            _lib.tuning_set("cu_reserve", reserve)
            for rep in range(3 if height == 256 else 2):
                got = run()
                for name, g, w in zip(("bf16", "f32+res", "pre", "gelu", "gelu'"), got, want):
                    assert torch.equal(g, w), (height, reserve, name, rep, float((g.float() - w.float()).abs().max()),
                                               torch.nonzero((g != w).any(1))[:4].flatten().tolist(), torch.nonzero((g != w).any(0))[:8].flatten().tolist())
    finally:
        lib.avs_gemm_set_nt8(1)
        lib.avs_gemm_set_tile_height(0)
        __import__("avsiam_amd")._lib.tuning_set("cu_reserve", 0)
    ref = A.double() @ W.double().t() + bias.double()
    assert rel_err(want[1], ref + res.double()) < 1e-5


@pytest.mark.parametrize("M,split,N,K", [(1000, 256, 768, 768), (39552, 8192, 768, 3072), (39552, 8192, 3072, 768), (2560 + 77, 2560, 256, 128)])
def test_gemm_nt_two_weight_sets_in_one_launch(M, split, N, K):
    """avs_gemm_nt_bf16_dual: rows below m_split meet (B, bias, colsum), rows from it (B2, bias2, colsum2).  Must equal the
    two separate GEMMs over the row ranges - bitwise for the outputs (same accumulation order in every kernel variant),
    to fp32-atomic order for the fused column sums."""
    o = ops()
    A = bf(torch.randn(M, K, device=DEV))
    W1, W2 = bf(torch.randn(N, K, device=DEV) * 0.05), bf(torch.randn(N, K, device=DEV) * 0.05)
    b1, b2 = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    res = torch.randn(M, N, device=DEV)
    aux = bf(torch.randn(M, N, device=DEV))

    def both(fn):
        return fn(slice(0, split), split, W1, b1), fn(slice(split, M), M - split, W2, b2)

    # bf16 output with bias and a fused column sum
    out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    cs1, cs2 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    o.gemm_nt(A, W1, out, M, bias=b1, colsum=cs1, dual=(split, W2, b2, cs2))
    want, wcs = torch.zeros_like(out), [torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)]
    both(lambda sl, m, W, b: o.gemm_nt(A[sl], W, want[sl], m, bias=b, colsum=wcs[0] if sl.start == 0 else wcs[1]))
    assert torch.equal(out, want)
    for g, w in ((cs1, wcs[0]), (cs2, wcs[1])):
        assert rel_err(g, w) < 1e-5
    # fp32 output with residual
    outf, wantf = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
    o.gemm_nt(A, W1, outf, M, bias=b1, res=res, dual=(split, W2, b2, None))
    both(lambda sl, m, W, b: o.gemm_nt(A[sl], W, wantf[sl], m, bias=b, res=res[sl]))
    assert torch.equal(outf, wantf)
    # GELU pair and GELU' (no bias on the second: both sets must mirror each other)
    pre, act, wpre, wact = (torch.zeros(M, N, device=DEV, dtype=torch.bfloat16) for _ in range(4))
    o.gemm_nt(A, W1, pre, M, bias=b1, out2=act, act=1, dual=(split, W2, b2, None))
    both(lambda sl, m, W, b: o.gemm_nt(A[sl], W, wpre[sl], m, bias=b, out2=wact[sl], act=1))
    assert torch.equal(pre, wpre) and torch.equal(act, wact)
    d, wd = torch.zeros_like(pre), torch.zeros_like(pre)
    o.gemm_nt(A, W1, d, M, aux=aux, act=2, dual=(split, W2, None, None))
    both(lambda sl, m, W, b: o.gemm_nt(A[sl], W, wd[sl], m, aux=aux[sl], act=2))
    assert torch.equal(d, wd)
    ref = torch.cat([A[:split].double() @ W1.double().t() + b1.double(), A[split:].double() @ W2.double().t() + b2.double()]) + res.double()
    assert rel_err(outf, ref) < 1e-5
    with pytest.raises(AssertionError):                    # the split must sit on a 256-row tile boundary
        o.gemm_nt(A, W1, out, M, bias=b1, dual=(split + 128, W2, b2, None))


@pytest.mark.parametrize("M,N1,N2,splits", [(64, 128, 128, 1), (1000, 256, 768, 0), (4099, 768, 256, 3), (333, 2304, 768, 0),
                                            (20001, 2304, 768, 0), (33333, 768, 3072, 0), (16500, 1536, 1024, 7)])
def test_gemm_tn(M, N1, N2, splits):
    o = ops()
    Mp = o.pad_rows(M, 64)
    A = torch.zeros(Mp, N1, device=DEV, dtype=torch.bfloat16)
    B = torch.zeros(Mp, N2, device=DEV, dtype=torch.bfloat16)
    A[:M] = bf(torch.randn(M, N1, device=DEV))
    B[:M] = bf(torch.randn(M, N2, device=DEV))
    ref = A.double().t() @ B.double() + 1
    for rep in range(3 if M > 16384 else 1):          # the long-contraction shapes run the 8-phase kernel: screen for races
        C = torch.ones(N1, N2, device=DEV)
        o.gemm_tn(A, B, C, M, splits)
        assert rel_err(C, ref) < 1e-5, rep


@pytest.mark.parametrize("M,shapes", [(8192, [(768, 3072), (3072, 768), (768, 768)]), (20001, [(512, 2048), (512, 512)]),
                                      (700, [(768, 768), (256, 512), (1024, 256)]), (5000, [(768, 768), (384, 768)]), (300, [(256, 256), (256, 512)])])
def test_gemm_tn_group(M, shapes):
    """avs_gemm_tn_bf16_group3: up to three weight gradients over the same token rows in one launch of the 8-phase kernel (a block's fc2 /
    fc1 / proj gradients) - every tile of every problem, ragged last stage, accumulation into C; shapes that do not qualify (N not a
    multiple of 256, very short M) fall back to one launch per problem inside the library."""
    o = ops()
    Mp = o.pad_rows(M, 64)
    jobs, refs = [], []
    for N1, N2 in shapes:
        A = torch.zeros(Mp, N1, device=DEV, dtype=torch.bfloat16)
        B = torch.zeros(Mp, N2, device=DEV, dtype=torch.bfloat16)
        A[:M] = bf(torch.randn(M, N1, device=DEV))
        B[:M] = bf(torch.randn(M, N2, device=DEV))
        jobs.append((A, B, torch.ones(N1, N2, device=DEV)))
        refs.append(A.double().t() @ B.double() + 1)
    from avsiam_amd import _lib
    try:
        for rep in range(3):
            _lib.tuning_set("cu_reserve", 8 if rep == 2 else 0)          # (third pass: split factors sized for 248 CUs, as under data parallelism)
            for _, _, C in jobs:
                C.fill_(1.0)
            o.gemm_tn_group(jobs, M)
            for (A, B, C), ref in zip(jobs, refs):
                assert rel_err(C, ref) < 1e-5, (rep, tuple(C.shape))
    finally:
        _lib.tuning_set("cu_reserve", 0)


def _attn_ref(qkv, lens, H):
    D = qkv.shape[1] // 3
    hd = D // H
    outs = []
    row = 0
    for L in lens:
        x = qkv[row:row + L].reshape(L, 3, H, hd).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]
        a = (q @ k.transpose(-1, -2)) * hd ** -0.5
        outs.append((a.softmax(-1) @ v).permute(1, 0, 2).reshape(L, D))
        row += L
    return torch.cat(outs)


@pytest.mark.parametrize("tile_rows", [128, 64])
@pytest.mark.parametrize("H,hd,lens", [(12, 64, [39, 128, 177, 512, 1, 65]), (16, 32, [708, 33, 200]), (2, 64, [300]),
                                       (4, 80, [257, 64, 1, 130, 51, 153])])          # hd 80: ViT-H (1280 / 16 heads)
def test_attention_fwd_bwd(H, hd, lens, tile_rows):
    o = ops()
    D = H * hd
    rows = sum(lens)
    rp = o.pad_rows(rows)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(rows, 3 * D, device=DEV)
    x[:, :D] *= o.attn_q_scale(hd)              # the kernels take q pre-multiplied by hd^-0.5 * log2(e) (qkv GEMM epilogue)
    qkv[:rows] = bf(x)
    tiles = o.AttnTiles(lens, DEV, tile_rows=tile_rows)
    assert (attn_reached(PASS_FWD, tiles, H, hd), attn_reached(PASS_BWD, tiles, H, hd)) == attn_meant(hd, tile_rows)
    out = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=DEV)
    o.attn_fwd(qkv, tiles, H, out, lse)
    qr = qkv[:rows].double()
    qr[:, :D] /= o.attn_q_scale(hd)             # the q the reference formula sees; dqkv is the gradient w.r.t. this q
    qr.requires_grad_(True)
    ref = _attn_ref(qr, lens, H)
    assert rel_err(out[:rows], ref) < 6e-3
    dout = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    dout[:rows] = bf(torch.randn(rows, D, device=DEV))
    dqkv = torch.zeros_like(qkv)
    delta = torch.zeros_like(lse)
    o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv)
    (ref * dout[:rows].double()).sum().backward()
    g = qr.grad
    for i, name in enumerate("qkv"):
        e = rel_err(dqkv[:rows, i * D:(i + 1) * D], g[:, i * D:(i + 1) * D])
        assert e < 1.5e-2, (name, e)
    assert dqkv[rows:].abs().max().item() == 0


@pytest.mark.parametrize("H,hd", [(12, 64), (16, 32)])
@pytest.mark.parametrize("tile_rows", [128, 64])
def test_attention_ring_kernels_match_the_register_staged_ones(H, hd, tile_rows):
    """The LDS-DMA ring kernels (round 5: K / V - Q / dO in the dK,dV kernel - tiles by global_load_lds into a ring of slots, one barrier per
    tile, every LDS read in inline asm) against the register-staged kernels they replace: the same LDS image, the same fragments, the same
    products in the same order - so the outputs must be BITWISE equal (forward output and log-sum-exp, dq / dk / dv, delta), on sequences
    that end inside a tile, fill exactly one, are shorter than one, and run over dozens (the decoder's 2472).  Twice, with the caches in
    another state, as a race screen for the ring's waits; rows outside the sequences stay untouched."""
    from avsiam_amd import _lib
    o = ops()
    D = H * hd
    lens = [2472, 196, 49, 618, 65, 64, 1, 128, 129, 512, 63, 300]
    rows = sum(lens)
    rp = o.pad_rows(rows)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(rows, 3 * D, device=DEV)
    x[:, :D] *= o.attn_q_scale(hd)
    qkv[:rows] = bf(x)
    # head 0 of the long sequence: every query is aligned with key 5 (first tile: it sets the reference point, score ~ 0.05 * 64 * hd in
    # log2 units) and key 1900 is twice key 5 - its score lies 100+ above the reference, the row sum passes 2^40 and the forward's rare
    # "new reference maximum" branch runs in tile 29
    qkv[5, D:D + hd] *= 8.0
    qkv[1900, D:D + hd] = qkv[5, D:D + hd] * 2.0
    qkv[:2472, :hd] = qkv[5:6, D:D + hd] * 0.05
    dout = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    dout[:rows] = bf(torch.randn(rows, D, device=DEV))
    tiles = o.AttnTiles(lens, DEV, tile_rows=tile_rows)

    def run(ring):
        _lib.tuning_set("attn_ring", ring)
        assert (attn_reached(PASS_FWD, tiles, H, hd), attn_reached(PASS_BWD, tiles, H, hd)) == attn_meant(hd, tile_rows, ring)
        out = torch.full((rp, D), 3.0, device=DEV, dtype=torch.bfloat16)
        lse = torch.full((H, rp), 5.0, device=DEV)
        o.attn_fwd(qkv, tiles, H, out, lse)
        dqkv = torch.full_like(qkv, 7.0)
        delta = torch.full_like(lse, 9.0)
        o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv)
        torch.cuda.synchronize()
        return out, lse, dqkv, delta

    try:
        want = run(0)
        for rep in range(2):
            got = run(1)
            for name, g, w in zip(("out", "lse", "dqkv", "delta"), got, want):
                assert torch.equal(g, w), (name, rep, float((g.float() - w.float()).abs().max()))
            torch.zeros(64 << 20, device=DEV).add_(1.0)          # other traffic between the repetitions
        assert torch.isfinite(want[0][:rows].float()).all() and float((want[0][rows:].float() - 3.0).abs().max()) == 0.0
    finally:
        _lib.tuning_set("attn_ring", 0)


@pytest.mark.parametrize("H,hd", [(12, 64), (4, 32), (4, 80)])
def test_attention_bwd_fused_matches_two_kernel_form(H, hd):
    """avs_attn_bwd_fused (sequences of at most 64 / 128 tokens: dq, dk, dv from one read and one S / exp evaluation per (sequence,
    head)) against the fp64 reference AND against the two-kernel backward on the same inputs - the same products in the same order, so
    the two agree to the last bf16 digit or two; rows of the longer sequences are left alone."""
    o = ops()
    D = H * hd
    lens = [39, 200, 49, 64, 65, 1, 128, 300, 33, 100, 117, 78, 127, 2, 129, 224, 196, 156, 204, 225, 160, 193]
    big = {64: 224, 32: 128, 80: 64}[hd]      # (head dim 64: sequences of 129 .. 224 tokens through the 7-wave kernel, round 6; head dim 80 - ViT-H - has the 64-row form only)
    rows = sum(lens)
    rp = o.pad_rows(rows)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(rows, 3 * D, device=DEV)
    x[:, :D] *= o.attn_q_scale(hd)
    qkv[:rows] = bf(x)
    tiles = o.AttnTiles(lens, DEV, tile_rows=64)
    out = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=DEV)
    o.attn_fwd(qkv, tiles, H, out, lse)
    dout = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    dout[:rows] = bf(torch.randn(rows, D, device=DEV))
    want = torch.zeros_like(qkv)
    delta = torch.zeros_like(lse)
    o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, want)
    got = torch.full_like(qkv, 7.0)
    for lo, hi in ((0, 64), (64, 128), (128, 224)):
        if hi > big:
            continue
        sq = o.AttnSeqs(lens, DEV, lo, hi)
        assert sq.nseq == sum(1 for L in lens if lo < L <= hi)
        assert attn_reached(PASS_FUSED, sq, H, hd) == [(A_FUSED224 if hi == 224 else A_FUSED, 96 if hd == 80 else hd, hi // 32, 0)]
        o.attn_bwd_fused(qkv, sq, H, out, dout, lse, got)
    r0 = 0
    for L in lens:
        blk = slice(r0, r0 + L)
        if L <= big:
            for i, name in enumerate("qkv"):
                if L == 1 and name == "q":             # one key: p = 1 and dS = p (dP - delta) = 0 - both forms give rounding noise
                    assert float(got[blk, :D].float().abs().max()) < 2e-2 and float(want[blk, :D].float().abs().max()) < 2e-2
                    continue
                e = rel_err(got[blk, i * D:(i + 1) * D], want[blk, i * D:(i + 1) * D])
                assert e < 2e-3, (L, name, e)
        else:
            assert float((got[blk].float() - 7.0).abs().max()) == 0.0, L          # not this kernel's rows
        r0 += L
    assert float((got[rows:].float() - 7.0).abs().max()) == 0.0
    # and against the fp64 formula, like test_attention_fwd_bwd
    qr = qkv[:rows].double()
    qr[:, :D] /= o.attn_q_scale(hd)
    qr.requires_grad_(True)
    ref = _attn_ref(qr, lens, H)
    (ref * dout[:rows].double()).sum().backward()
    r0 = 0
    for L in lens:
        if 1 < L <= big:
            for i, name in enumerate("qkv"):
                e = rel_err(got[r0:r0 + L, i * D:(i + 1) * D], qr.grad[r0:r0 + L, i * D:(i + 1) * D])
                assert e < 1.5e-2, (L, name, e)
        r0 += L


@pytest.mark.parametrize("M", [640, 1000, 20001])
def test_gemm_tn_fp8_weight_gradients(M):
    """avs_gemm_tn_fp8_group3 (fp8 mode 3): C += A8^T . B8 / (sa sb) with A8 = e5m2 gradient copies and B8 = e4m3 activation copies, up to
    three problems over the same token rows in one launch (v_mfma_f32_32x32x64_f8f6f4 on ds_read_b64_tr_b8 fragments, split over the rows,
    fp32 atomics).  EXACT arithmetic given the operands: against the fp64 product of the de-quantised copies (fp32 accumulation error only),
    accumulating onto what C already holds, rows beyond M (zero by contract) not contributing, and every split configuration of the three
    shapes of a block (fc2 768 x 3072, fc1 3072 x 768, proj 768 x 768) plus the single-problem call (qkv 2304 x 768)."""
    o = ops()
    rp = o.pad_rows(M, 256)
    gen = torch.Generator(device=DEV).manual_seed(M)

    def operand(N, e5m2, scale):
        x = torch.randn(M, N, device=DEV, generator=gen) * (0.02 if e5m2 else 1.0)
        q = torch.zeros(rp, N, device=DEV, dtype=torch.uint8)
        fmt = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
        q[:M] = (x * scale).to(fmt).view(torch.uint8)
        return q, q[:M].view(fmt).double() / scale

    recs = o.Fp8Records(8, DEV)
    jobs, want = [], []
    shapes = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    for k, (N1, N2) in enumerate(shapes):
        sa, sb = 2.0 ** (10 + k), 2.0 ** (4 - k)           # powers of two: the de-quantised values are exact in bf16 (last check)
        recs.q[2 * k, 0], recs.q[2 * k, 1] = sa, 1.0 / sa
        recs.q[2 * k + 1, 0], recs.q[2 * k + 1, 1] = sb, 1.0 / sb
        A8, Ad = operand(N1, True, sa)
        B8, Bd = operand(N2, False, sb)
        C = torch.randn(N1 * N2, device=DEV) * 0.1
        want.append(C.double().view(N1, N2) + Ad.t() @ Bd)
        jobs.append((A8, B8, C, recs.rec(2 * k), recs.rec(2 * k + 1)))
    o.gemm_tn_fp8_group(jobs[:3], M)
    o.gemm_tn_fp8_group(jobs[3:], M)
    for (A8, B8, C, _, _), w, (N1, N2) in zip(jobs, want, shapes):
        e = rel_err(C.view(N1, N2), w)
        assert e < 5e-5, ((N1, N2), e)            # measured ~1e-5: the fp8 MFMA's internal summation (the fp8 nt GEMM shows the same, 1.4e-5)
    # against the bf16 weight-gradient kernel on the same (de-quantised) operands: the same matrix up to bf16 operand rounding
    A8, B8, C, qa, qb = jobs[2]
    Ab = torch.zeros(rp, 768, device=DEV, dtype=torch.bfloat16); Bb = torch.zeros(rp, 768, device=DEV, dtype=torch.bfloat16)
    Ab[:M] = (A8[:M].view(torch.float8_e5m2).float() / float(qa[0])).to(torch.bfloat16)
    Bb[:M] = (B8[:M].view(torch.float8_e4m3fn).float() / float(qb[0])).to(torch.bfloat16)
    C2 = torch.zeros(768 * 768, device=DEV)
    o.gemm_tn(Ab, Bb, C2, M)
    C3 = torch.zeros(768 * 768, device=DEV)
    o.gemm_tn_fp8_group([(A8, B8, C3, qa, qb)], M)
    assert rel_err(C3, C2) < 5e-5          # e5m2 / e4m3 values are exact in bf16: the two kernels multiply the same numbers


@pytest.mark.parametrize("H,hd", [(2, 64), (3, 32), (2, 80)])
def test_attention_bwd_writes_the_e5m2_copy_of_dqkv(H, hd):
    """fp8 backward (fp8 mode 2): avs_attn_bwd_q8 / avs_attn_bwd_fused_q8 also write e5m2(dqkv * scale) - the gradient operand of the
    fp8 qkv input-gradient GEMM - and fold max |dqkv| into the device record.  The bf16 output must be BIT-identical to the plain call,
    the e5m2 copy must be the e5m2 rounding of what the kernels hold in fp32 (checked against the bf16 output: within one e5m2 step, 2^-2
    relative, plus the bf16 rounding), untouched outside the sequences' rows, and the record's amax must equal max |dqkv|."""
    o = ops()
    D = H * hd
    lens = [39, 200, 64, 130, 128, 300, 7]
    rows = sum(lens)
    rp = o.pad_rows(rows, 256)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(rows, 3 * D, device=DEV)
    x[:, :D] *= o.attn_q_scale(hd)
    qkv[:rows] = bf(x)
    tr = 64
    fwd_tiles = o.AttnTiles(lens, DEV, tile_rows=tr)
    out = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=DEV)
    o.attn_fwd(qkv, fwd_tiles, H, out, lse)
    dout = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    dout[:rows] = bf(torch.randn(rows, D, device=DEV))
    cut = 64 if hd == 80 else 128             # (head dim 80: the fused kernel has the 64-row form only)
    tiles = o.AttnTiles(lens, DEV, tile_rows=tr, min_len=cut)
    fused = [sq for sq in (o.AttnSeqs(lens, DEV, 0, 64), o.AttnSeqs(lens, DEV, 64, cut)) if sq.nseq]
    # the copy-writing instantiations: dQ and dK/dV at 64-row tiles, the fused kernel at 64 (and 128) rows
    assert tiles.ntiles and attn_reached(PASS_BWD, tiles, H, hd, g8=1) == attn_meant(hd, tr, g8=1)[1]
    assert [attn_reached(PASS_FUSED, sq, H, hd, g8=1) for sq in fused] == [[(A_FUSED, 96 if hd == 80 else hd, r // 32, 1)] for r in ((64,) if hd == 80 else (64, 128))]

    def run(d8=None, rec=None, kv_bf16=True):
        dq = torch.zeros_like(qkv)
        delta = torch.zeros_like(lse)
        kw = {} if d8 is None else {"dqkv8": d8, "q8": rec, "kv_bf16": kv_bf16}
        o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dq, **kw)
        for sq in fused:
            o.attn_bwd_fused(qkv, sq, H, out, dout, lse, dq, **kw)
        return dq

    plain = run()
    recs = o.Fp8Records(1, DEV, fmax=o.BF8_MAX)
    amax = float(plain[:rows].float().abs().max())
    scale = 0.25 * o.BF8_MAX / amax
    recs.q[0, 0], recs.q[0, 1] = scale, 1.0 / scale
    d8 = torch.full((rp, 3 * D), 0x7B, device=DEV, dtype=torch.uint8)                    # 0x7B = 57344 in e5m2: a value no gradient takes
    got = run(d8, recs.rec(0))
    assert torch.equal(got, plain)
    deq = d8[:rows].view(torch.float8_e5m2).float() / scale
    ref = plain[:rows].float()
    err = (deq - ref).abs()
    assert float((err / (ref.abs() + 1e-3 * amax)).max()) < 0.14, float((err / (ref.abs() + 1e-3 * amax)).max())   # half an e5m2 step (2^-3) + bf16
    assert rel_err(deq, ref) < 0.08
    assert bool((d8[rows:] == 0x7B).all())                                               # pad rows are not this kernel's
    assert abs(recs.amax(0) - amax) <= 2.0 ** -7 * amax                                  # the record saw the fp32 values (bf16-rounded in `plain`)
    # kv_bf16=False (fp8 mode 3): the same e5m2 copy, the query third of the bf16 dqkv as before, its key / value thirds not written
    d8b = torch.full_like(d8, 0x7B)
    lean = run(d8b, recs.rec(0), kv_bf16=False)
    assert torch.equal(d8b, d8) and torch.equal(lean[:, :D], plain[:, :D]) and float(lean[:, D:].float().abs().max()) == 0.0


@pytest.mark.parametrize("H,hd,L,spike", [(2, 64, 200, 8.0), (2, 64, 200, 2.5), (4, 32, 300, 40.0), (4, 32, 300, 4.0)])
def test_attention_spiked_scores(H, hd, L, spike):
    """Large score spread: the forward keeps the first key tile's row max as its reference and moves it only when a later
    tile's row sum reaches 2^40 (or overflows) - spikes below that threshold (large p, no rescale), above it, and beyond
    fp32's exp2 range (inf in the first attempt) must all give the softmax."""
    o = ops()
    D = H * hd
    rp = o.pad_rows(L)
    x = torch.randn(L, 3 * D, device=DEV)
    x[150, D:2 * D] *= spike        # one late key dominates
    x[L - 3, D:2 * D] *= spike      # and one in the partial last key tile (masking + moved reference together)
    x[10, :D] *= 6.0
    x[60:70, :D] *= -4.0            # rows whose first key tile is far BELOW the later maximum and far above others
    x[:, :D] *= o.attn_q_scale(hd)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    qkv[:L] = bf(x)
    tiles = o.AttnTiles([L], DEV)
    out = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=DEV)
    o.attn_fwd(qkv, tiles, H, out, lse)
    qr = qkv[:L].double()
    qr[:, :D] /= o.attn_q_scale(hd)
    ref = _attn_ref(qr, [L], H)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out[:L], ref) < 8e-3
    # the saved log-sum-exp is exact whatever reference max the kernel happened to keep
    q, k = qr[:, :D].reshape(L, H, hd), qr[:, D:2 * D].reshape(L, H, hd)
    lse_ref = torch.logsumexp(torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5, dim=-1)
    assert (lse[:, :L].double() - lse_ref).abs().max().item() < 2e-2


def test_im2col_and_patch_embed_matches_conv():
    o = ops()
    B, Tlen, mel = 3, 256, 128
    a = torch.randn(B, Tlen, mel, device=DEV)
    tP = Tlen // 16
    La = tP * (mel // 16)
    row_b = torch.arange(B, device=DEV).repeat_interleave(La).to(torch.int32)
    row_tok = torch.arange(La, device=DEV).repeat(B).to(torch.int32)
    out = torch.zeros(B * La, 256, device=DEV, dtype=torch.bfloat16)
    o.im2col_audio(a, row_b, row_tok, out, B * La, tP)
    w = torch.randn(64, 1, 16, 16, device=DEV)
    img = bf(a).float().unsqueeze(1).transpose(2, 3)
    ref = F.conv2d(img.double(), w.double(), stride=16).flatten(2).transpose(1, 2).reshape(B * La, 64)
    got = out.double() @ w.double().reshape(64, 256).t()
    assert rel_err(got, ref) < 1e-6
    v = torch.randn(2, 3, 224, 224, device=DEV)
    rows = 2 * 196
    row_img = torch.arange(2, device=DEV).repeat_interleave(196).to(torch.int32)
    row_tok = torch.arange(196, device=DEV).repeat(2).to(torch.int32)
    outv = torch.zeros(rows, 768, device=DEV, dtype=torch.bfloat16)
    o.im2col_video(v, row_img, row_tok, outv, rows)
    wv = torch.randn(32, 3, 16, 16, device=DEV)
    refv = F.conv2d(bf(v).double(), wv.double(), stride=16).flatten(2).transpose(1, 2).reshape(rows, 32)
    gotv = outv.double() @ wv.double().reshape(32, 768).t()
    assert rel_err(gotv, refv) < 1e-6


def test_unshuffle_roundtrip():
    o = ops()
    B, T, La, Lv, D, ka, kv = 3, 2, 32, 16, 512, 8, 4
    Ltot = La + T * Lv
    n_enc = ka + T * kv
    x = torch.randn(B * n_enc, D, device=DEV)
    src = torch.full((B, Ltot), -1, dtype=torch.int32, device=DEV)
    for b in range(B):
        pa = torch.randperm(La, device=DEV)[:ka]
        src[b, pa] = (b * n_enc + torch.arange(ka, device=DEV)).int()
        for t in range(T):
            pv = torch.randperm(Lv, device=DEV)[:kv]
            src[b, La + t * Lv + pv] = (b * n_enc + ka + t * kv + torch.arange(kv, device=DEV)).int()
    pos = torch.cat([torch.arange(La), La + torch.arange(Lv).repeat(T)]).repeat(B).to(torch.int32).to(DEV)
    mod = torch.cat([torch.zeros(La), torch.ones(T * Lv)]).repeat(B).to(torch.uint8).to(DEV)
    mt, pa_, pv_, ma, mv = (torch.randn(n, device=DEV) for n in (D, La * D, Lv * D, D, D))
    out = torch.empty(B * Ltot, D, device=DEV)
    srcf = src.reshape(-1).contiguous()
    o.unshuffle_fwd(x, srcf, pos, mod, mt, pa_, pv_, ma, mv, out, B * Ltot)
    base = torch.where((srcf >= 0)[:, None], x[srcf.clamp(min=0).long()], mt[None])
    posall = torch.cat([pa_.reshape(La, D), pv_.reshape(Lv, D)])
    ref = base + posall[pos.long()] + torch.where(mod.bool()[:, None], mv[None], ma[None])
    assert torch.allclose(out, ref, atol=1e-6)
    dout = torch.randn(B * Ltot, D, device=DEV)
    dx = torch.zeros_like(x)
    dpa, dpv, dm, dma, dmv = (torch.zeros(n, device=DEV) for n in (La * D, Lv * D, D, D, D))
    o.unshuffle_bwd(dout, srcf, B, T, La, Lv, dx, dpa, dpv, dm, dma, dmv)
    kept = srcf >= 0
    dx_ref = torch.zeros_like(x)
    dx_ref[srcf[kept].long()] = dout[kept]
    assert torch.allclose(dx, dx_ref)
    assert rel_err(dm, dout[~kept].sum(0)) < 1e-5
    assert rel_err(dma, dout[~mod.bool()].sum(0)) < 1e-5
    assert rel_err(dmv, dout[mod.bool()].sum(0)) < 1e-5
    dpos_ref = torch.zeros(La + Lv, D, device=DEV).index_add_(0, pos.long(), dout)
    assert rel_err(torch.cat([dpa, dpv]), dpos_ref.reshape(-1)) < 1e-5


def test_segment_mean_colsum_scatter_cast_transpose():
    o = ops()
    D = 768
    lens = [5, 100, 39, 1]
    rows = sum(lens)
    yf = torch.randn(rows, D, device=DEV)
    y = bf(yf)
    seg = torch.tensor([0, 5, 105, 144, 145], dtype=torch.int32, device=DEV)
    reps = torch.empty(4, D, device=DEV)
    o.segment_mean_fwd(yf, seg, reps, 4)
    ref = torch.stack([yf[seg[i]:seg[i + 1]].double().mean(0) for i in range(4)])
    assert rel_err(reps, ref) < 1e-6
    dreps = torch.randn(4, D, device=DEV)
    dy = torch.zeros(rows, D, device=DEV)
    o.segment_mean_bwd(dreps, seg, dy, 4, 3.0)
    refdy = torch.cat([(3 * dreps[i] / lens[i]).expand(lens[i], D) for i in range(4)])
    assert rel_err(dy, refdy) < 1e-6
    cs = torch.zeros(D, device=DEV)
    o.colsum(y, cs, rows)
    assert rel_err(cs, y.double().sum(0)) < 1e-5
    # a column range of a wider matrix (the query third of the qkv gradient), accumulating
    cs3 = torch.ones(256, device=DEV)
    o.colsum(y[:, 256:512], cs3, rows)
    assert rel_err(cs3, 1 + y[:, 256:512].double().sum(0)) < 1e-5
    # y += alpha * x . W (the value third of the qkv bias gradient from the proj bias gradient)
    xk = torch.randn(D, device=DEV)
    Wk = bf(torch.randn(D, 512, device=DEV) * 0.1)
    yk = torch.ones(512, device=DEV)
    o.vecmat(xk, Wk, yk, 0.5)
    assert rel_err(yk, 1 + 0.5 * (xk.double() @ Wk.double())) < 1e-5
    idx = torch.randint(0, 7, (rows,), device=DEV, dtype=torch.int32)
    dst = torch.zeros(7, D, device=DEV)
    o.scatter_add_rows(y, idx, dst, rows, 2.0)
    refd = torch.zeros(7, D, device=DEV, dtype=torch.double).index_add_(0, idx.long(), 2 * y.double())
    assert rel_err(dst, refd) < 1e-5
    w = torch.randn(300, 200, device=DEV)
    wb = torch.empty(300, 200, device=DEV, dtype=torch.bfloat16)
    o.cast_bf16(w, wb, w.numel())
    assert torch.equal(wb, bf(w))
    wt = torch.empty(200, 300, device=DEV, dtype=torch.bfloat16)
    o.transpose_bf16(wb, wt)
    assert torch.equal(wt, wb.t().contiguous())
    xs = torch.randn(1024, device=DEV)
    ys = torch.empty(1024, device=DEV, dtype=torch.bfloat16)
    o.cast_scale(xs, ys, 1024, 2.0)
    assert torch.equal(ys, bf(xs * 2))


@pytest.mark.parametrize("audio", [True, False])
def test_mae_loss(audio):
    o = ops()
    from oracle import ref_cpu
    from avsiam_amd.config import AVSiamConfig
    cfg = AVSiamConfig(audio_tokens=128)
    B = 3
    if audio:
        inp = torch.randn(B, 256, 128, device=DEV)
        L, P = 128, 256
    else:
        inp = torch.randn(B, 3, 224, 224, device=DEV)
        L, P = 196, 768
    pred = torch.randn(B * L, P, device=DEV)
    mask = (torch.rand(B * L, device=DEV) > 0.25).float()
    row_loss = torch.empty(B * L, device=DEV); loss = torch.empty(1, device=DEV)
    nmask = float(mask.sum().item())
    tot = torch.full((1,), 5.0, device=DEV)
    o.mae_loss_fwd(pred, inp, mask, row_loss, loss, audio, L, nmask, total=tot, total_init=False)
    assert abs(tot.item() - 5.0 - loss.item()) < 1e-5
    pr = pred.cpu().reshape(B, L, P).requires_grad_(True)
    ref = ref_cpu.mae_loss(cfg, inp.cpu(), pr, mask.cpu().reshape(B, L), 'a' if audio else 'v')
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    g = torch.tensor([1.7], device=DEV)
    dpred = torch.empty(B * L, P, device=DEV, dtype=torch.bfloat16)
    o.mae_loss_bwd(pred, inp, mask, g, dpred, audio, L, nmask)
    (ref * 1.7).backward()
    assert rel_err(dpred.cpu(), pr.grad.reshape(B * L, P)) < 4e-3


@pytest.mark.parametrize("N", [4, 6, 64, 130, 512])          # 512 = 8 ranks x batch 64: the [WB, WB] logits of BASELINE configs[2]
def test_infonce(N):
    o = ops()
    from oracle import ref_cpu
    D = 768
    a = torch.randn(N, D, device=DEV); v = torch.randn(N, D, device=DEV) + 0.5 * a
    an, vn = torch.empty_like(a), torch.empty_like(v)
    na, nv = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    o.l2norm_fwd(a, an, na); o.l2norm_fwd(v, vn, nv)
    total = torch.empty(N, N, device=DEV)
    o.gemm_f32_small(an, vn, total, N, N, D, (D, 1), (1, D), 1 / 0.05)
    stats = torch.empty(N, 4, device=DEV); out = torch.empty(3, device=DEV)
    o.infonce_fwd(total, stats, out, 0.01)
    assert abs(out[2].item() - 0.01 * out[0].item()) < 1e-7
    ar, vr = a.cpu().double().requires_grad_(True), v.cpu().double().requires_grad_(True)
    nce, acc, tot = ref_cpu.contrastive(ar, vr)
    assert rel_err(total.cpu(), tot.detach()) < 1e-5
    assert abs(out[0].item() - nce.item()) < 1e-5 * abs(nce.item()) + 1e-6
    assert abs(out[1].item() - acc.item()) < 1e-6
    g = torch.tensor([0.9], device=DEV)
    dtotal = torch.empty_like(total)
    o.infonce_dlogits(total, stats, g, 1.0, dtotal)
    dan, dvn = torch.empty_like(a), torch.empty_like(v)
    o.gemm_f32_small(dtotal, vn, dan, N, D, N, (N, 1), (D, 1), 1 / 0.05)
    o.gemm_f32_small(dtotal, an, dvn, N, D, N, (1, N), (D, 1), 1 / 0.05)
    da, dv = torch.empty_like(a), torch.empty_like(v)
    o.l2norm_bwd(dan, an, na, da); o.l2norm_bwd(dvn, vn, nv, dv)
    (nce * 0.9).backward()
    assert rel_err(da.cpu(), ar.grad) < 1e-3      # fp32 exp of +-20 logits vs an fp64 reference
    assert rel_err(dv.cpu(), vr.grad) < 1e-3


def test_adam_matches_torch():
    o = ops()
    n = 4096 + 64
    p = torch.randn(n, device=DEV); g = torch.randn(n, device=DEV)
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([ref_p], 2e-4, weight_decay=5e-7, betas=(0.95, 0.999))
    m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    pb = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    for step in range(1, 4):
        gs = g * step
        ref_p.grad = gs.clone()
        opt.step()
        o.adam(p, gs, m, v, pb, n, 2e-4, step)
        assert torch.allclose(p, ref_p.data, rtol=1e-5, atol=1e-7), step
    assert torch.equal(pb, bf(p))


def test_mask_plan_kernel_properties():
    """Every sequence: ids are a permutation; the first `keep` go to the row arrays; un-shuffle sources / masks agree with
    the permutation; structured sequences never keep a forced-out token while enough free tokens exist; keeps are uniform."""
    import numpy as np
    o = ops()
    nseq, L, keep, t_p = 300, 512, 307, 64
    d = np.zeros((nseq, o.PLAN_FIELDS), dtype=np.int32)
    dec = nseq * L
    for s in range(nseq):
        structured = s % 2 == 0
        d[s] = [L, keep, s * keep, 1000 + s, s * L, s * 77, t_p if structured else 0, s * L, s * L, 0, 0, 0] + o.PLAN_CLASSIC
    rng = np.random.default_rng(0)
    tl = rng.integers(0, 2 ** 31, nseq).astype(np.int32) & 0x0F0F0F0F
    th = rng.integers(0, 2 ** 31, nseq).astype(np.int32) & 0x00FF00FF
    fm = (rng.integers(0, 4, nseq) * 5).astype(np.int32) & 0xFF
    dev = lambda x: torch.from_numpy(x).to(DEV)
    row_src = torch.full((nseq * keep,), -7, dtype=torch.int32, device=DEV)
    row_tok = torch.full((nseq * keep,), -7, dtype=torch.int32, device=DEV)
    src_row = torch.full((dec,), -7, dtype=torch.int32, device=DEV)
    mask = torch.full((dec,), -7.0, device=DEV)
    ids = torch.full((dec,), -7, dtype=torch.int32, device=DEV)
    o.mask_plan(dev(d), d, 0x1234ABCD5678, row_src, row_tok, dev(tl), dev(th), dev(fm), src_row, mask, ids)
    ids_c, tok_c, src_c, mask_c = ids.cpu().view(nseq, L), row_tok.cpu().view(nseq, keep), src_row.cpu().view(nseq, L), mask.cpu().view(nseq, L)
    assert torch.equal(ids_c.sort(dim=1).values, torch.arange(L, dtype=torch.int32).expand(nseq, L))
    assert torch.equal(tok_c, ids_c[:, :keep])
    assert torch.equal(row_src.cpu().view(nseq, keep), (1000 + torch.arange(nseq, dtype=torch.int32))[:, None].expand(nseq, keep))
    for s in range(0, nseq, 37):
        kept = ids_c[s, :keep].long()
        assert torch.equal(src_c[s, kept], (s * 77 + torch.arange(keep)).int())
        assert (mask_c[s, kept] == 0).all() and mask_c[s].sum().item() == L - keep
        assert (src_c[s][mask_c[s] == 1] == -1).all()
    # structured: forced-out tokens are kept only when the free ones run out
    for s in range(0, nseq, 2):
        tbits = (int(tl[s]) & 0xFFFFFFFF) | ((int(th[s]) & 0xFFFFFFFF) << 32)
        forced = torch.tensor([((tbits >> (i % t_p)) & 1) | ((int(fm[s]) >> (i // t_p)) & 1) for i in range(L)], dtype=torch.bool)
        nfree = int((~forced).sum())
        kept = ids_c[s, :keep].long()
        assert int(forced[kept].sum()) == max(0, keep - nfree)
    # unstructured keeps are uniform over positions
    freq = torch.zeros(L)
    for s in range(1, nseq, 2):
        freq[ids_c[s, :keep].long()] += 1
    p = keep / L
    z = (freq - (nseq // 2) * p) / math.sqrt((nseq // 2) * p * (1 - p))
    assert z.abs().max() < 5.0
    # different seed -> different plan; same seed -> same plan
    ids2 = torch.empty_like(ids)
    o.mask_plan(dev(d), d, 0x1234ABCD5678, row_src, row_tok, dev(tl), dev(th), dev(fm), src_row, mask, ids2)
    assert torch.equal(ids2, ids)
    o.mask_plan(dev(d), d, 0x1234ABCD5679, row_src, row_tok, dev(tl), dev(th), dev(fm), src_row, mask, ids2)
    assert not torch.equal(ids2, ids)


def test_mask_plan_grouped_decoder_layout():
    """avs_mask_plan_grouped (round 6, EngineOptions.prune_dead): the decoder rows of a sample are ordered [scored tokens | kept tokens] instead of
    by position.  Same Philox draws as the classic layout (ids equal for the same key); src_row / pos_row / row_of_pos / pred_id are consistent with
    the shuffle: a kept token's row carries its encoder row, a scored token's row -1; row_of_pos inverts pos_row; the compact prediction rows
    enumerate exactly the scored (sample, token) pairs in rank order."""
    import numpy as np
    o = ops()
    B, T, La, Lv, ka, kv = 3, 2, 128, 196, 32, 49
    ma, mv = La - ka, Lv - kv
    Lt, lq, n_enc = La + T * Lv, ma + T * mv, ka + T * kv
    nseq = B + B * T
    d = np.zeros((nseq, o.PLAN_FIELDS), dtype=np.int32)
    for b in range(B):
        d[b] = [La, ka, b * ka, b, b * Lt, b * n_enc, 0, b * La, b * La, 0, 0, 0, b * Lt, b * Lt + lq, b * ma, 0]
        for t in range(T):
            i = b * T + t
            d[B + i] = [Lv, kv, B * ka + i * kv, i, b * Lt + La + t * Lv, b * n_enc + ka + t * kv, 0, B * La + i * Lv, B * La + i * Lv, 0, 0, 0,
                        b * Lt + ma + t * mv, b * Lt + lq + ka + t * kv, B * ma + i * mv, La]       # (every frame takes the one table pos_v: pos_base La)
    dc = d.copy()
    dc[:, 12:] = o.PLAN_CLASSIC
    dev = lambda x: torch.from_numpy(x).to(DEV)
    nrow = B * ka + B * T * kv
    mk = lambda n, v=-7: torch.full((n,), v, dtype=torch.int32, device=DEV)
    row_src, row_tok, src_row, ids = mk(nrow), mk(nrow), mk(B * Lt), mk(B * La + B * T * Lv)
    pos_row, rop, pid = mk(B * Lt), mk(B * Lt), mk(B * ma + B * T * mv)
    mask = torch.full((B * La + B * T * Lv,), -7.0, device=DEV)
    o.mask_plan(dev(d), d, 0xFEED1234, row_src, row_tok, src_row=src_row, mask_out=mask, ids_out=ids, grouped=(pos_row, rop, pid))
    src_c, ids_c, mask_c = mk(B * Lt), mk(B * La + B * T * Lv), torch.full_like(mask, -7.0)
    o.mask_plan(dev(dc), dc, 0xFEED1234, mk(nrow), mk(nrow), src_row=src_c, mask_out=mask_c, ids_out=ids_c)
    assert torch.equal(ids, ids_c) and torch.equal(mask, mask_c)                       # the same draws, the same loss masks
    src_row, pos_row, rop, pid, src_c, mask_c = (x.cpu().long() for x in (src_row, pos_row, rop, pid, src_c, mask_c.int()))
    assert torch.equal(rop.sort().values, torch.arange(B * Lt))                        # a permutation of the decoder rows
    b_of = torch.arange(B * Lt) // Lt
    pos_tab = torch.cat([torch.arange(La), La + torch.arange(Lv).repeat(T)]).repeat(B)  # the positional-table row of every position (frames share pos_v)
    assert torch.equal(pos_row[rop], pos_tab)                                          # the row holding position p takes position p's table row
    assert torch.equal(rop // Lt, b_of)                                                # ... and stays inside the sample
    assert torch.equal(src_row[rop], src_c)                                            # the row holding position p carries what position p carried
    for b in range(B):                                                                 # scored rows first, kept rows after
        blk = src_row[b * Lt:(b + 1) * Lt]
        assert (blk[:lq] == -1).all() and (blk[lq:] >= 0).all()
        assert torch.equal(blk[lq:], b * n_enc + torch.arange(n_enc))                  # kept rows in encoder order: [audio | frame 0 | frame 1]
    # compact prediction rows: audio row b * ma + r <-> the r-th scored token of the audio sequence, as (sample, token) of the mask numbering
    mflat = mask_c
    assert (mflat[pid] == 1).all() and pid.unique().numel() == pid.numel() == int(mflat.sum())
    assert (pid[:B * ma] < B * La).all() and (pid[B * ma:] >= B * La).all()
    # the decoder row of compact row (b, j) holds the same token: its position matches pred_id
    inv = torch.empty_like(rop)
    inv[rop] = torch.arange(B * Lt)                                                    # decoder row -> position b * Lt + l
    for b in range(B):
        pos = inv[b * Lt: b * Lt + lq] - b * Lt
        tok_id = torch.where(pos < La, b * La + pos, B * La + (b * T + (pos - La) // Lv) * Lv + (pos - La) % Lv)
        want = torch.cat([pid[b * ma:(b + 1) * ma]] + [pid[B * ma + (b * T + t) * mv: B * ma + (b * T + t + 1) * mv] for t in range(T)])
        assert torch.equal(tok_id, want)


@pytest.mark.parametrize("H,hd,L,lq", [(16, 32, 300, 203), (16, 32, 2472, 1854), (12, 64, 257, 128), (4, 80, 200, 77)])
def test_attention_with_query_rows_limited_and_compact_output(H, hd, L, lq):
    """avs_attn_fwd_cq / avs_attn_bwd_cq (the decoder's last block in the pruned form): only the first lq rows of every (equal-length) sequence
    are queries, all rows are keys / values, out / dO are compact.  Against the full kernels: the compact output rows are BITWISE the full
    output's rows of the same queries; the backward equals the full backward fed dO = 0 on the rows that are not queries - dq of the query
    rows, dk and dv of every row, bitwise - and leaves the query third of the other rows untouched."""
    o = ops()
    D, nseq = H * hd, 3
    rows = nseq * L
    rp = o.pad_rows(rows)
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(rows, 3 * D, device=DEV)
    x[:, :D] *= o.attn_q_scale(hd)
    qkv[:rows] = bf(x)
    tiles = o.AttnTiles([L] * nseq, DEV, tile_rows=128)
    assert tiles.uniform_len == L
    assert (attn_reached(PASS_FWD, tiles, H, hd, lq=lq), attn_reached(PASS_BWD, tiles, H, hd, lq=lq)) == attn_meant(hd, 128)
    out = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(H, rp, device=DEV)
    o.attn_fwd(qkv, tiles, H, out, lse)
    cp = o.pad_rows(nseq * lq)
    out_c = torch.full((cp, D), 7.0, device=DEV, dtype=torch.bfloat16)
    lse_c = torch.full((H, rp), 7.0, device=DEV)
    o.attn_fwd(qkv, tiles, H, out_c, lse_c, lq=lq)
    isq = torch.zeros(rows, dtype=torch.bool, device=DEV)
    for s in range(nseq):
        assert torch.equal(out_c[s * lq:(s + 1) * lq], out[s * L:s * L + lq])
        assert torch.equal(lse_c[:, s * L:s * L + lq], lse[:, s * L:s * L + lq])
        assert (lse_c[:, s * L + lq:(s + 1) * L] == 7.0).all()                        # rows that are keys / values only: nothing written
        isq[s * L:s * L + lq] = True
    assert (out_c[nseq * lq:] == 7.0).all()
    dout = torch.zeros(rp, D, device=DEV, dtype=torch.bfloat16)
    dout[:rows] = bf(torch.randn(rows, D, device=DEV))
    dout[:rows][~isq] = 0
    dout_c = torch.zeros(cp, D, device=DEV, dtype=torch.bfloat16)
    for s in range(nseq):
        dout_c[s * lq:(s + 1) * lq] = dout[s * L:s * L + lq]
    dqkv, delta = torch.zeros_like(qkv), torch.zeros_like(lse)
    o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv)
    dqkv_c, delta_c = torch.full_like(qkv, 3.0), torch.zeros_like(lse)
    o.attn_bwd(qkv, tiles, H, out_c, dout_c, lse_c, delta_c, dqkv_c, lq=lq)
    assert torch.equal(dqkv_c[:rows, D:], dqkv[:rows, D:])                            # dk, dv: every row
    assert torch.equal(dqkv_c[:rows, :D][isq], dqkv[:rows, :D][isq])                  # dq: the query rows
    assert (dqkv_c[:rows, :D][~isq] == 3.0).all()                                     # ... the others are the caller's to zero
    o.expand_rows(None, torch.where(isq, torch.arange(rows, device=DEV), torch.full((rows,), -1, device=DEV)).int(), dqkv_c, rows, cols=D)
    assert (dqkv_c[:rows, :D][~isq] == 0).all() and torch.equal(dqkv_c[:rows, :D][isq], dqkv[:rows, :D][isq]) and torch.equal(dqkv_c[:rows, D:], dqkv[:rows, D:])
    assert (dqkv[:rows, :D][~isq] == 0).all()                                         # (zero dO -> zero dq: what the pruned form relies on)
    # expand_rows with a source: compact rows back into the packed numbering, zeros elsewhere
    cmap = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    for s in range(nseq):
        cmap[s * L:s * L + lq] = torch.arange(s * lq, (s + 1) * lq, dtype=torch.int32, device=DEV)
    back = torch.full((rp, D), 5.0, device=DEV, dtype=torch.bfloat16)
    o.expand_rows(dout_c, cmap, back, rows)
    assert torch.equal(back[:rows], dout[:rows]) and (back[rows:] == 5.0).all()


def test_input_normalisation_matches_dataloader_formulas():
    """fbank / frame normalisation of the reference dataloader (dataloader.py:505-513, 461-462, 152-155)."""
    import numpy as np
    from avsiam_amd import preprocess as pp
    B, T, Fm = 5, 1024, 128
    fb = torch.randn(B, T, Fm, device=DEV) * 4 - 5
    out = pp.normalize_fbank(fb, -5.081, 4.4849)
    assert torch.allclose(out, (fb - (-5.081)) / 4.4849, rtol=1e-6, atol=1e-6)
    # noise + roll: same amp / shift stream as the wrapper draws, noise within [0, amp), reproducible per seed
    rng = np.random.default_rng(11)
    amp = (rng.random(B) / 10).astype(np.float32)
    shift = rng.integers(-T, T, B)
    o1 = pp.normalize_fbank(fb, -5.081, 4.4849, noise=True, seed=11)
    o2 = pp.normalize_fbank(fb, -5.081, 4.4849, noise=True, seed=11)
    assert torch.equal(o1, o2)
    for b in range(B):
        base = torch.roll((fb[b] - (-5.081)) / 4.4849, int(shift[b]), 0)           # fbank = roll(fbank + noise, shift, 0)  (:511-513)
        d = o1[b] - base
        assert float(d.min()) >= -1e-5 and float(d.max()) < amp[b] + 1e-5, (b, float(d.min()), float(d.max()), amp[b])
        assert abs(float(d.mean()) - amp[b] / 2) < 0.02 * amp[b] + 1e-6
    fr = torch.randint(0, 256, (3, 4, 3, 224, 224), device=DEV, dtype=torch.uint8)
    got = pp.normalize_frames(fr)
    mean = torch.tensor(pp.IMAGENET_DEFAULT_MEAN, device=DEV).view(1, 1, 3, 1, 1)
    std = torch.tensor(pp.IMAGENET_DEFAULT_STD, device=DEV).view(1, 1, 3, 1, 1)
    assert torch.allclose(got, (fr.float() / 255 - mean) / std, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("M,N,K,f32out", [(256, 256, 256, True), (1000, 768, 768, False), (4099, 1280, 5120, True), (70000, 768, 3072, False)])
def test_gemm_nt_fp8(M, N, K, f32out):
    """The fp8 (OCP e4m3) variant of the 8-phase GEMM (BASELINE configs[4]'s fp8 MFMA path).  (1) Layout / arithmetic: against an fp64
    product of the DE-quantised operands the result is exact up to fp32 accumulation.  (2) Its own tolerance against the bf16 GEMM of the
    unquantised operands: e4m3 keeps 3 mantissa bits (relative rounding error up to 2^-4), which on random operands gives ~4 % relative L2."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(M + K)
    A = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) * 0.05
    b = torch.randn(N, device=DEV, generator=g)
    sa, sw = o.FP8_MAX / o.absmax(A), o.FP8_MAX / o.absmax(W)
    assert abs(o.FP8_MAX / sa - A.abs().max().item()) < 1e-6
    Mp = o.pad_rows(M, 256)
    A8 = torch.zeros(Mp, K, device=DEV, dtype=torch.uint8)
    o.quantize_fp8(A, sa, out=A8[:M])
    W8 = o.quantize_fp8(W.to(torch.bfloat16), sw)                       # bf16 source: the weight shadows
    # the encoding is OCP e4m3 (torch.float8_e4m3fn) and the rounding is to nearest
    Ad = A8[:M].view(torch.float8_e4m3fn).double() / sa
    Wd = W8.view(torch.float8_e4m3fn).double() / sw
    assert torch.equal(A8[:M].view(torch.float8_e4m3fn), (A * sa).clamp(-448, 448).to(torch.float8_e4m3fn))
    res = torch.randn(Mp, N, device=DEV, generator=g) if f32out else None
    out = torch.zeros(Mp, N, device=DEV, dtype=torch.float32 if f32out else torch.bfloat16)
    o.gemm_nt_fp8(A8, W8, out, M, 1.0 / (sa * sw), bias=b, res=res)
    ref = Ad @ Wd.t() + b.double() + (res[:M].double() if f32out else 0)
    assert rel_err(out[:M], ref) < (5e-5 if f32out else 3e-3)            # fp32 accumulation over up to 5120 terms (measured 1.4e-5); bf16 output: its own rounding
    assert Mp == M or out[M:].abs().max().item() == 0
    full = A.double() @ W.to(torch.bfloat16).double().t() + b.double() + (res[:M].double() if f32out else 0)
    e = rel_err(out[:M], full)
    assert 5e-3 < e < 8e-2, e


@pytest.mark.parametrize("M,N,K", [(1000, 768, 768), (4099, 3072, 768)])
def test_gemm_nt_fp8_gelu_grad_as_8_bit_codes(M, N, K):
    """fp8 backward (round 5): gelu'(x) travels from the fc1 forward epilogue (act 1) to the fc2 input-gradient epilogue (act 2) as 8-bit
    fixed-point codes - (g' + 0.1296875) * 202 in [0, 255] - instead of bf16: a uint8 `out` / `aux` of ops.gemm_nt_fp8.  The codes decode to the
    bf16 epilogue's gelu'(x) within half a step (0.0025) plus the bf16 rounding; gelu(x) and its e4m3 copy do not change; the input gradient
    computed with the coded operand equals the one computed with the bf16 operand to 2e-3 - far inside the e5m2 rounding of that gradient."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(M)
    Mp = o.pad_rows(M, 256)
    A8 = torch.zeros(Mp, K, device=DEV, dtype=torch.uint8)
    o.quantize_fp8(torch.randn(M, K, device=DEV, generator=g), 64.0, out=A8[:M])
    W8 = o.quantize_fp8((torch.randn(N, K, device=DEV, generator=g) * 0.08).to(torch.bfloat16), 512.0)
    b = torch.randn(N, device=DEV, generator=g)
    alpha = 1.0 / (64.0 * 512.0)
    gp16, act16 = (torch.zeros(Mp, N, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    a8_16, a8_8 = (torch.zeros(Mp, N, device=DEV, dtype=torch.uint8) for _ in range(2))
    o.gemm_nt_fp8(A8, W8, gp16, M, alpha, bias=b, out2=act16, act=1, out8=a8_16, out8_scale=32.0)
    gp8 = torch.full((Mp, N), 255, device=DEV, dtype=torch.uint8)
    act8 = torch.zeros_like(act16)
    o.gemm_nt_fp8(A8, W8, gp8, M, alpha, bias=b, out2=act8, act=1, out8=a8_8, out8_scale=32.0)
    assert torch.equal(act8, act16) and torch.equal(a8_8, a8_16)                 # gelu(x) and its e4m3 copy are untouched
    dec = gp8[:M].float() / 202.0 - 0.1296875
    err = (dec - gp16[:M].float()).abs().max().item()
    assert err < 0.0025 + 0.0045, err                                            # half a code step + the bf16 rounding of the reference near 1
    assert float(dec.min()) > -0.135 and float(dec.max()) < 1.135 and int(gp8[:M].min()) >= 0
    assert Mp == M or bool((gp8[M:] == 255).all())                               # rows beyond M are not written
    # the consumer: fc2 input gradient, e5m2 gradient x e4m3 transposed weight, times gelu'(x), with the fused column sum
    G8 = torch.zeros(Mp, K, device=DEV, dtype=torch.uint8)
    o.quantize_fp8(torch.randn(M, K, device=DEV, generator=g) * 0.01, 4096.0, out=G8[:M], e5m2=True)
    alpha_g = 1.0 / (4096.0 * 512.0)
    d16, d8 = (torch.zeros(Mp, N, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    c16, c8 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    o.gemm_nt_fp8(G8, W8, d16, M, alpha_g, act=2, aux=gp16, colsum=c16, grad=True)
    o.gemm_nt_fp8(G8, W8, d8, M, alpha_g, act=2, aux=gp8, colsum=c8, grad=True)
    assert rel_err(d8[:M].float(), d16[:M].float()) < 6e-3 and rel_err(c8, c16) < 6e-3
    want = (G8[:M].view(torch.float8_e5m2).double() / 4096.0) @ (W8.view(torch.float8_e4m3fn).double() / 512.0).t() * dec.double()
    assert rel_err(d8[:M].float(), want) < 4e-3                                  # bf16 output rounding: the coded operand is applied exactly


def test_fp8_delayed_scaling_records():
    """The fp8 mode's device-side quantisation state (ops.Fp8Records, csrc/common.h AVS_Q_*): calibration (absmax -> scale on the device),
    the producers that write e4m3 operands themselves (quantising pass, LayerNorm, GELU epilogue, attention epilogue) read the scale from the
    record and fold their |max| into it, the GEMM de-quantises with the two records, two weight sets in one launch, the history ring, the
    saturation counter.  No call here synchronises except the test's own reads."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(5)
    M, N, K = 1024, 768, 768
    A = torch.randn(M, K, device=DEV, generator=g) * 1.7
    W = bf(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    W2 = bf(torch.randn(N, K, device=DEV, generator=g) * 0.11)
    b, b2 = torch.randn(N, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    rec = o.Fp8Records(6, DEV, nhist=4, margin=2.0)
    ra, rw, rw2, r8 = rec.rec(0), rec.rec(1), rec.rec(2), rec.rec(3)
    o.absmax_into(A, ra); o.absmax_into(W, rw); o.absmax_into(W2, rw2)
    rec.update(first=0, count=3)
    q = rec.q.cpu()
    for i, t in enumerate((A, W, W2)):
        amax = t.float().abs().max().item()
        assert abs(q[i, 0].item() - 448.0 / (2 * amax)) <= 1e-5 * q[i, 0].item() and abs(q[i, 0].item() * q[i, 1].item() - 1) < 1e-6
        assert abs(q[i, 2].item() - 0.9 * amax) <= 1e-6 * amax                 # the running amax restarts at 0.9 x the recorded one
    assert rec.pos == 0 and q[3:].abs().max().item() == 0 and q[:3, 4:].abs().max().item() == 0                 # a partial update neither advances the ring nor touches other records
    A8 = o.quantize_fp8(A, 123.0, q=ra)                                   # the host scale is ignored beside a record
    W8, W82 = o.quantize_fp8(W, 1.0, q=rw), o.quantize_fp8(W2, 1.0, q=rw2)
    sa, sw, sw2 = (rec.q[i, 0].item() for i in range(3))
    assert torch.equal(A8.view(torch.float8_e4m3fn), (A * sa).clamp(-448, 448).to(torch.float8_e4m3fn))
    assert rec.amax(0) == A.abs().max().item()                            # the pass recorded what it saw
    out = torch.zeros(M, N, device=DEV)
    o.gemm_nt_fp8(A8, W8, out, M, 77.0, bias=b, qa=ra, qw=rw)
    want = torch.zeros(M, N, device=DEV)
    o.gemm_nt_fp8(A8, W8, want, M, 1.0 / (sa * sw), bias=b)
    assert rel_err(out, want) < 1e-6
    # two weight sets in one launch == two launches on the row ranges
    o.gemm_nt_fp8(A8, W8, out, M, bias=b, qa=ra, qw=rw, dual=(512, W82, b2, rw2))
    o.gemm_nt_fp8(A8[512:].contiguous(), W82, want[512:], M - 512, 1.0 / (sa * sw2), bias=b2)
    assert rel_err(out, want) < 1e-6 and rel_err(out[512:], want[512:]) < 1e-6
    # GELU epilogue writing the next GEMM's operand with the record r8 (first calibrated from the bf16 gelu output)
    dact = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16); act = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    o.gemm_nt_fp8(A8, W8, dact, M, bias=b, out2=act, act=1, qa=ra, qw=rw)
    o.absmax_into(act, r8)
    rec.update(first=3, count=1)
    act8 = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    o.gemm_nt_fp8(A8, W8, dact, M, bias=b, out2=act, act=1, qa=ra, qw=rw, out8=act8, q8=r8)
    s8 = rec.q[3, 0].item()
    deq = act8.view(torch.float8_e4m3fn).float() / s8
    assert float((deq - act.float()).abs().max()) <= 2 ** -4 * act.float().abs().max().item() + 1e-3       # e4m3: 3 mantissa bits
    assert rel_err(deq, act) < 0.04
    assert abs(rec.amax(3) - act.float().abs().max().item()) <= 1e-2 * act.float().abs().max().item()
    # 8-bit-only output (fp8 mode 3, EngineOptions.fp8_lean): no bf16 gelu(x) - the e4m3 copy and gelu'(x) are the same bits
    act8b, dact2 = torch.zeros_like(act8), torch.zeros_like(dact)
    o.gemm_nt_fp8(A8, W8, dact2, M, bias=b, out2=None, act=1, qa=ra, qw=rw, out8=act8b, q8=r8)
    assert torch.equal(act8b, act8) and torch.equal(dact2, dact)
    # LayerNorm writing the e4m3 copy with a record
    D, rows = 768, 777
    x = torch.randn(rows, D, device=DEV, generator=g) * 3
    gm, bt = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16); y8 = torch.zeros(rows, D, device=DEV, dtype=torch.uint8)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    rl = rec.rec(4)
    o.layernorm_fwd(x, gm, bt, y, mean, rstd, rows, 1e-5)
    o.absmax_into(y, rl)
    rec.update(first=4, count=1)
    o.layernorm_fwd(x, gm, bt, y, mean, rstd, rows, 1e-5, y8=y8, q8_dev=rl)
    sl = rec.q[4, 0].item()
    assert rel_err(y8.view(torch.float8_e4m3fn).float() / sl, y) < 0.04
    assert abs(rec.amax(4) - y.float().abs().max().item()) <= 1e-2 * y.float().abs().max().item()
    y8b, mean2, rstd2 = torch.zeros_like(y8), torch.empty_like(mean), torch.empty_like(rstd)
    o.layernorm_fwd(x, gm, bt, None, mean2, rstd2, rows, 1e-5, y8=y8b, q8_dev=rl)           # the e4m3 copy as the only output
    assert torch.equal(y8b, y8) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    # attention epilogue writing the proj operand
    Dm, H, L = 768, 12, 200
    qkv = bf(torch.randn(2 * L, 3 * Dm, device=DEV, generator=g) * 0.5)
    tiles = o.AttnTiles([L, L], DEV)
    att = torch.zeros(o.pad_rows(2 * L), Dm, device=DEV, dtype=torch.bfloat16)
    att8 = torch.zeros(o.pad_rows(2 * L), Dm, device=DEV, dtype=torch.uint8)
    lse = torch.zeros(H, o.pad_rows(2 * L), device=DEV)
    rt = rec.rec(5)
    o.attn_fwd(qkv, tiles, H, att, lse)
    ref_att = att.clone()
    o.absmax_into(att, rt)
    rec.update(first=5, count=1)
    o.attn_fwd(qkv, tiles, H, att, lse, out8=att8, q8=rt)
    assert torch.equal(att, ref_att)                                       # the bf16 output does not change
    st_ = rec.q[5, 0].item()
    assert rel_err(att8[:2 * L].view(torch.float8_e4m3fn).float() / st_, att[:2 * L]) < 0.04
    # ---- input-gradient form (fp8 mode 2): e5m2 gradient operand x e4m3 transposed weight, records with fmax 57344
    grec = o.Fp8Records(3, DEV, nhist=4, margin=2.0, fmax=o.BF8_MAX)
    rg, rg2 = grec.rec(0), grec.rec(1)
    dY = torch.randn(M, K, device=DEV, generator=g) * 1e-3                 # gradients are small: the scale moves them into e5m2's range
    dYb = bf(dY)
    o.absmax_into(dYb, rg)
    grec.update(first=0, count=1)
    sg = grec.q[0, 0].item()
    assert abs(sg - 57344.0 / (2 * dYb.float().abs().max().item())) <= 1e-5 * sg
    dY8 = o.quantize_fp8(dYb, 1.0, q=rg, e5m2=True)
    assert torch.equal(dY8.view(torch.float8_e5m2), (dYb.float() * sg).clamp(-57344, 57344).to(torch.float8_e5m2))
    dYd = dY8.view(torch.float8_e5m2).double() / sg
    Wd = W8.view(torch.float8_e4m3fn).double() / sw
    dX = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    o.gemm_nt_fp8(dY8, W8, dX, M, qa=rg, qw=rw, grad=True)
    assert rel_err(dX, dYd @ Wd.t()) < 3e-3                                  # exact product of the de-quantised operands, bf16 output
    assert 5e-3 < rel_err(dX, dYb.double() @ W.double().t()) < 0.12           # e5m2 keeps 2 mantissa bits: ~7 % on random operands
    # act 2: x saved gelu'(x), fused column sum, and the e5m2 copy of the result for the next input-gradient GEMM
    aux = bf(torch.rand(M, N, device=DEV, generator=g))
    cs = torch.ones(N, device=DEV)
    want2 = (dYd @ Wd.t()) * aux.double()
    o.absmax_into(bf(want2.float()), rg2)
    grec.update(first=1, count=1)
    out8g = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    o.gemm_nt_fp8(dY8, W8, dX, M, qa=rg, qw=rw, grad=True, act=2, aux=aux, colsum=cs, out8=out8g, q8=rg2)
    assert rel_err(dX, want2) < 3e-3 and rel_err(cs, 1 + want2.sum(0)) < 2e-3
    s2 = grec.q[1, 0].item()
    assert rel_err(out8g.view(torch.float8_e5m2).float() / s2, want2) < 0.08
    out8h, cs2 = torch.zeros_like(out8g), torch.ones(N, device=DEV)
    o.gemm_nt_fp8(dY8, W8, None, M, qa=rg, qw=rw, grad=True, act=2, aux=aux, colsum=cs2, out8=out8h, q8=rg2)      # the e5m2 copy as the only output
    assert torch.equal(out8h, out8g) and rel_err(cs2, cs) < 1e-5
    # LayerNorm backward writing the e5m2 copy of dx
    dyl = bf(torch.randn(rows, D, device=DEV, generator=g) * 1e-2)
    dxb_ = torch.zeros(rows, D, device=DEV, dtype=torch.bfloat16)
    dx8_ = torch.zeros(rows, D, device=DEV, dtype=torch.uint8)
    wsl = torch.empty(o.layernorm_ws(rows, D), device=DEV)
    dgl, dbl = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    rl8 = grec.rec(2)
    o.layernorm_bwd(dyl, x, mean, rstd, gm, None, dgl, dbl, wsl, rows, dx_bf16=dxb_)
    o.absmax_into(dxb_, rl8)
    grec.update(first=2, count=1)
    o.layernorm_bwd(dyl, x, mean, rstd, gm, None, dgl, dbl, wsl, rows, dx_bf16=dxb_, dx8=dx8_, q8=rl8)
    assert rel_err(dx8_.view(torch.float8_e5m2).float() / grec.q[2, 0].item(), dxb_) < 0.08
    assert abs(grec.amax(2) - dxb_.float().abs().max().item()) <= 1e-2 * dxb_.float().abs().max().item()
    # the ring: a whole-table update stores the amax, restarts it and advances; a 3x larger tensor saturates under the old scale once
    o.quantize_fp8(A * 3, 1.0, q=ra)
    rec.update()
    q = rec.q.cpu()
    assert rec.pos == 1 and q[0, 3].item() == 1.0 and q[1, 3].item() == 0.0 and abs(q[0, 2].item() - 0.9 * 3 * A.abs().max().item()) < 1e-4
    assert abs(q[0, 0].item() - 448.0 / (2 * 3 * A.abs().max().item())) <= 1e-5 * q[0, 0].item()
    assert rec.saturation_events() == 1.0
    st = rec.state()
    rec2 = o.Fp8Records(6, DEV, nhist=4, margin=2.0)
    rec2.load(st)
    assert torch.equal(rec2.q, rec.q) and torch.equal(rec2.hist, rec.hist) and rec2.pos == rec.pos
