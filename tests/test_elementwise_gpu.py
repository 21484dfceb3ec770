"""The data-movement, loss and optimizer kernels (csrc/elementwise.hip, the MAE / InfoNCE half of csrc/losses.hip, csrc/preprocess.hip) at the
shapes where their code branches: the second trip of the grid-stride loops (launches are capped at 4096 blocks), element / row tails, more than
one row block or column pass, the options only whole-model tests reach (row maps, strides, compact predictions, raw-input transforms), the batched
launchers' descriptor and chunk arithmetic, and the one-writer forms of the deterministic mode.

Every test calls the kernel through avsiam_amd.ops and compares with a plain fp64 torch / numpy reference built from the same inputs (on the
bf16-rounded operands where the kernel reads bf16).  Outputs live in buffers larger than needed, pre-filled with a sentinel that must survive
wherever the kernel has no business writing; inputs carry a large value behind their last valid element, so a read past the end shows in the result.
Tolerances are those of the op's test in test_kernels_gpu.py; where an op had none, the bound is derived beside the assert."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5                 # exact in fp32 and bf16
SENT8 = 0xA5
BIG = 1.0e4                   # behind the last valid input element / row: a read past the end wrecks the result
WRAP4 = 4096 * 256 * 4        # elements one trip of a 4-wide grid-stride loop covers at the 4096-block cap


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    torch.manual_seed(0)


def ops():
    from avsiam_amd import ops as o
    return o


def lib():
    from avsiam_amd import _lib
    return _lib


def bf(x):
    return x.to(torch.bfloat16)


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def full(n, dtype=torch.float32, fill=SENT):
    return torch.full((n,), fill, dtype=dtype, device=DEV)


def untouched(buf, n, fill=SENT):
    """elements [n:) of the flat view of buf still hold the sentinel"""
    return bool((buf.reshape(-1)[n:] == fill).all().item())


@contextlib.contextmanager
def det_mode(on):
    """the deterministic knob for the duration of the block, the previous value restored whatever happens"""
    L = lib()
    prev = L.tuning_get("det")
    try:
        L.tuning_set("det", 1 if on else 0)
        yield
    finally:
        L.tuning_set("det", prev)


def refused():
    return pytest.raises((lib().AvsiamHipError, AssertionError))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. Adam
ADAM_N = WRAP4 + 4 * 257          # the second grid-stride trip is partly filled (257 of its float4 groups)
LR, B1, B2, EPS, WD = 2e-4, 0.95, 0.999, 1e-8, 5e-7


def _adam_state(g, n, pad=64, moments=False):
    p, gr = randn(g, n + pad), randn(g, n + pad)
    m = 0.1 * randn(g, n + pad) if moments else torch.zeros(n + pad, device=DEV)
    v = (0.1 * randn(g, n + pad)) ** 2 + 1e-4 if moments else torch.zeros(n + pad, device=DEV)
    pb = full(n + pad, torch.bfloat16)
    for t in (p, gr, m, v):
        t[n:] = SENT
    return p, gr, m, v, pb


@pytest.mark.parametrize("variant", ["plain", "grad_scale", "no_shadow"])
def test_adam_second_grid_trip_against_torch(variant):
    o = ops()
    n = ADAM_N
    p, g, m, v, pb = _adam_state(gen(1), n)
    ref_p = torch.nn.Parameter(p[:n].clone())
    opt = torch.optim.Adam([ref_p], LR, weight_decay=WD, betas=(B1, B2))
    gscale = 0.5 if variant == "grad_scale" else 1.0
    for step in range(1, 4):
        gs = g * step
        gs[n:] = SENT
        ref_p.grad = gscale * gs[:n]
        opt.step()
        o.adam(p, gs, m, v, None if variant == "no_shadow" else pb, n, LR, step, grad_scale=gscale)
        assert torch.allclose(p[:n], ref_p.data, rtol=1e-5, atol=1e-7), (variant, step, float((p[:n] - ref_p.data).abs().max()))
        assert untouched(gs, n)
    if variant == "no_shadow":
        assert untouched(pb, 0)
    else:
        assert torch.equal(pb[:n], bf(p[:n])) and untouched(pb, n)
    for t in (p, g, m, v):
        assert untouched(t, n)


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_step_count_on_the_device(step):
    """avs_adam_dev: one update whose count comes from device memory, against fp64 Adam with the same bias corrections (hyper-parameters rounded to
    fp32, as the kernel receives them)."""
    o = ops()
    n = ADAM_N
    p, g, m, v, pb = _adam_state(gen(2 + step), n, moments=True)
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps, wd = (f32(x) for x in (LR, B1, B2, EPS, WD))
    pd, gd, md, vd = (t[:n].double() for t in (p, g, m, v))
    gg = gd + wd * pd
    m_ref = b1 * md + (1 - b1) * gg
    v_ref = b2 * vd + (1 - b2) * gg * gg
    p_ref = pd - (lr / (1 - b1 ** step)) * m_ref / (v_ref.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    sd = torch.tensor([step, 7], dtype=torch.int32, device=DEV)
    o.adam(p, g, m, v, pb, n, LR, 999, step_dev=sd)                    # the host count is ignored beside step_dev
    for got, want in ((p, p_ref), (m, m_ref), (v, v_ref)):
        assert torch.allclose(got[:n].double(), want, rtol=1e-5, atol=1e-7), (step, float((got[:n].double() - want).abs().max()))
    assert torch.equal(pb[:n], bf(p[:n]))
    for t in (p, g, m, v, pb):
        assert untouched(t, n)
    assert sd.tolist() == [step, 7]


def test_adam_smallest_size_and_refusal():
    o = ops()
    for dev_step in (False, True):
        p, g, m, v, pb = _adam_state(gen(9), 4, pad=12)
        ref_p = torch.nn.Parameter(p[:4].clone())
        ref_p.grad = g[:4].clone()
        torch.optim.Adam([ref_p], LR, weight_decay=WD, betas=(B1, B2)).step()
        sd = torch.tensor([1], dtype=torch.int32, device=DEV) if dev_step else None
        o.adam(p, g, m, v, pb, 4, LR, 1, step_dev=sd)
        assert torch.allclose(p[:4], ref_p.data, rtol=1e-5, atol=1e-7)
        assert torch.equal(pb[:4], bf(p[:4]))
        for t in (p, g, m, v, pb):
            assert untouched(t, 4)
        before = [t.clone() for t in (p, m, v, pb)]
        with refused():
            o.adam(p, g, m, v, pb, 6, LR, 1, step_dev=sd)
        assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, pb)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. casts
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4 * 1000 + 2, WRAP4 + 7])
def test_cast_bf16_tails_and_second_grid_trip(n):
    o = ops()
    x = randn(gen(n % 1000), n + 8)
    x[n:] = BIG
    y = full(n + 8, torch.bfloat16)
    o.cast_bf16(x, y, n)
    assert torch.equal(y[:n], bf(x[:n]))
    assert untouched(y, n)


@pytest.mark.parametrize("n", [4, WRAP4 + 8])
def test_cast_scale_second_grid_trip(n):
    o = ops()
    x = randn(gen(n % 1000), n + 8)
    x[n:] = BIG
    y = full(n + 8, torch.bfloat16)
    o.cast_scale(x, y, n, 0.37)
    assert torch.equal(y[:n], bf(x[:n] * 0.37))
    assert untouched(y, n)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. column sums
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("rows", [1, 31, 33, 511, 512, 513, 1100])
def test_colsum_row_blocks(rows, det):
    """one 32-lane pass (1, 31), a second lap of the row lanes (33), the 512-row block boundary and a third block with a ragged end (1100); det: one
    block walks all the rows.  Accumulates onto what the target holds."""
    o = ops()
    g = gen(100 + rows)
    for C, wide in ((64, False), (768, False), (64, True), (768, True)):
        ld = C + 128 if wide else C
        xfull = bf(randn(g, rows + 3, ld))
        xfull[rows:] = BIG                                      # rows >= `rows` are not to be read
        if wide:
            xfull[:, :64] = BIG; xfull[:, 64 + C:] = BIG        # nor are the neighbouring columns
        x = xfull[:, 64:64 + C] if wide else xfull
        init = randn(g, C)
        ref = init.double() + x[:rows].double().sum(0)
        outs = []
        with det_mode(det):
            for _ in range(2 if det else 1):
                buf = full(C + 64)
                buf[:C] = init
                o.colsum(x, buf[:C], rows)
                outs.append(buf)
        e = rel_err(outs[0][:C], ref)
        print(f"colsum rows={rows} C={C} wide={wide} det={det}: rel_err {e:.3e}")
        assert e < 1e-5, (rows, C, wide, det, e)
        assert untouched(outs[0], C)
        if det:
            assert torch.equal(outs[0], outs[1])
    assert lib().tuning_get("det") == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. scatter-add of rows
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("D", [80, 768])
@pytest.mark.parametrize("rows", [1, 145])
def test_scatter_add_rows(rows, D, det):
    """D = 80: the det kernel's second 64-column block is partly filled.  Every row onto one target row, and onto random ones; scale != 1."""
    o = ops()
    g = gen(rows + D)
    nd = 7
    src = bf(randn(g, rows + 2, D))
    src[rows:] = BIG
    for one_target in (True, False):
        idx = torch.full((rows + 2,), 3, dtype=torch.int32, device=DEV) if one_target else \
            torch.randint(0, nd, (rows + 2,), device=DEV, generator=g).to(torch.int32)
        init = randn(g, nd, D)
        ref = init.double().index_add_(0, idx[:rows].long(), -1.5 * src[:rows].double())
        outs = []
        with det_mode(det):
            for _ in range(2 if det else 1):
                buf = full(nd * D + 64)
                buf[:nd * D] = init.reshape(-1)
                o.scatter_add_rows(src, idx, buf[:nd * D], rows, -1.5)
                outs.append(buf)
        got = outs[0][:nd * D].reshape(nd, D)
        assert rel_err(got, ref) < 1e-5, (rows, D, det, one_target)
        hit = torch.zeros(nd, dtype=torch.bool, device=DEV)
        hit[idx[:rows].long()] = True
        assert torch.equal(got[~hit], init[~hit])               # rows nobody scatters to keep their bits
        assert untouched(outs[0], nd * D)
        if det:
            assert torch.equal(outs[0], outs[1])
    assert lib().tuning_get("det") == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. vector-matrix products
def _vecmat_case(g, K, N, wide):
    ld = N + 256 if wide else N
    Wfull = bf(randn(g, K + 1, ld) * 0.1)
    Wfull[K:] = BIG
    if wide:
        Wfull[:, :128] = BIG; Wfull[:, 128 + N:] = BIG
    W = Wfull[:K, 128:128 + N] if wide else Wfull[:K]
    xbuf = randn(g, K + 8)
    xbuf[K:] = BIG
    init = randn(g, N)
    ref = init.double() - 0.75 * (xbuf[:K].double() @ W.double())
    return xbuf[:K], W, init, ref


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("K,N", [(32, 256), (1280, 256), (768, 512)])
def test_vecmat(K, N, det):
    o = ops()
    g = gen(K + N)
    for wide in (False, True):
        x, W, init, ref = _vecmat_case(g, K, N, wide)
        outs = []
        with det_mode(det):
            for _ in range(2 if det else 1):
                buf = full(N + 64)
                buf[:N] = init
                o.vecmat(x, W, buf[:N], -0.75)
                outs.append(buf)
        assert rel_err(outs[0][:N], ref) < 1e-5, (K, N, det, wide)
        assert untouched(outs[0], N)
        if det:
            assert torch.equal(outs[0], outs[1])
    assert lib().tuning_get("det") == 0


@pytest.mark.parametrize("K,N", [(32, 256), (1280, 256), (768, 512)])
@pytest.mark.parametrize("count", [1, 3])
def test_vecmat_batch_equals_separate_calls(count, K, N):
    o = ops()
    g = gen(count + K + N)
    for wide in (False, True):
        cases = [_vecmat_case(g, K, N, wide) for _ in range(count)]
        bufs, vb = [], o.VecmatBatch()
        for x, W, init, _ in cases:
            buf = full(N + 64)
            buf[:N] = init
            bufs.append(buf)
            vb.add(x, W, buf[:N])
        vb.build(DEV)
        vb.run(-0.75)
        for (x, W, init, ref), buf in zip(cases, bufs):
            sep = init.clone()
            o.vecmat(x, W, sep, -0.75)
            assert rel_err(buf[:N], ref) < 1e-5 and rel_err(buf[:N], sep) < 1e-5, (count, K, N, wide)
            assert untouched(buf, N)
        # the batched launcher has no one-writer form: refused in the deterministic mode, nothing written
        before = [b.clone() for b in bufs]
        with det_mode(1):
            with pytest.raises(lib().AvsiamHipError):
                vb.run(-0.75)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, bufs))
    assert lib().tuning_get("det") == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. decoder un-shuffle
def _unshuffle_layout(g, B, T, La, Lv, permute):
    """positions (b, l) of a [La + T * Lv] decoder sequence -> decoder rows (position order, or a random permutation inside every sample), each kept
    (an encoder row) or masked.  Sample 0 keeps every token, sample 1 none (when they exist), the others about half."""
    Ltot = La + T * Lv
    keep = torch.rand(B, Ltot, device=DEV, generator=g) < 0.5
    keep[0] = True
    if B > 1:
        keep[1] = False
    n_enc = int(keep.sum().item())
    src_by_pos = torch.full((B * Ltot,), -1, dtype=torch.int64, device=DEV)
    src_by_pos[keep.reshape(-1)] = torch.randperm(n_enc, device=DEV, generator=g)
    row_of_pos = torch.arange(B * Ltot, device=DEV)
    if permute:
        row_of_pos = torch.cat([b * Ltot + torch.randperm(Ltot, device=DEV, generator=g) for b in range(B)])
    l = torch.arange(Ltot, device=DEV).repeat(B)
    pos_by_pos = torch.where(l < La, l, La + (l - La) % Lv)              # row of [pos_a ; pos_v]
    src_row = torch.empty_like(src_by_pos); pos_row = torch.empty_like(l); mod = torch.empty_like(l)
    src_row[row_of_pos] = src_by_pos                                      # everything below is indexed by DECODER row
    pos_row[row_of_pos] = pos_by_pos
    mod[row_of_pos] = (l >= La).long()
    return n_enc, src_row, pos_row, mod, row_of_pos


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (5, 1)])
@pytest.mark.parametrize("D", [768, 4])
def test_unshuffle_fwd_bwd(D, B, T, permute, det):
    """D = 768: the backward's second pass over 128 float4 columns is partly filled.  (1, 1): fewer (sample, frame) pairs than the backward's four row
    groups; (3, 2) and (5, 1): not a multiple of four.  The backward ADDS to the positional, mask-token and modality gradients."""
    o = ops()
    g = gen(D + 10 * B + T + 100 * permute)
    La, Lv = 5, 3
    Ltot = La + T * Lv
    rows = B * Ltot
    n_enc, src_row, pos_row, mod, row_of_pos = _unshuffle_layout(g, B, T, La, Lv, permute)
    src32, pos32, mod8, rop32 = src_row.int(), pos_row.int(), mod.to(torch.uint8), row_of_pos.int()
    x = randn(g, n_enc + 2, D)
    x[n_enc:] = BIG
    mt, pa, pv, ma, mv = (randn(g, k) for k in (D, La * D, Lv * D, D, D))
    out = full((rows + 2) * D).reshape(rows + 2, D)
    o.unshuffle_fwd(x, src32, pos32, mod8, mt, pa, pv, ma, mv, out, rows)
    base = torch.where((src_row >= 0)[:, None], x[src_row.clamp(min=0)].double(), mt.double()[None])
    posall = torch.cat([pa.reshape(La, D), pv.reshape(Lv, D)]).double()
    ref = base + posall[pos_row] + torch.where(mod.bool()[:, None], mv.double()[None], ma.double()[None])
    assert torch.allclose(out[:rows].double(), ref, atol=1e-6)
    assert untouched(out, rows * D)
    # backward
    dout = randn(g, rows + 2, D)
    dout[rows:] = BIG
    kept = src_row >= 0
    dd = dout[:rows].double()
    inits = [randn(g, k) for k in (La * D, Lv * D, D, D, D)]             # dpos_a, dpos_v, dmask, dmod_a, dmod_v
    pos_grad = torch.zeros(La + Lv, D, device=DEV, dtype=torch.double).index_add_(0, pos_row, dd)
    refs = [inits[0].double() + pos_grad[:La].reshape(-1), inits[1].double() + pos_grad[La:].reshape(-1),
            inits[2].double() + dd[~kept].sum(0), inits[3].double() + dd[mod == 0].sum(0), inits[4].double() + dd[mod == 1].sum(0)]
    runs = []
    with det_mode(det):
        for _ in range(2 if det else 1):
            dx = full((n_enc + 2) * D).reshape(n_enc + 2, D)
            bufs = []
            for init in inits:
                b_ = full(init.numel() + 64)
                b_[:init.numel()] = init
                bufs.append(b_)
            views = [b_[:init.numel()] for b_, init in zip(bufs, inits)]
            o.unshuffle_bwd(dout, src32, B, T, La, Lv, dx, *views, row_of_pos=rop32 if permute else None)
            runs.append([dx] + bufs)
    dx, bufs = runs[0][0], runs[0][1:]
    dx_ref = torch.full_like(dx, SENT)
    dx_ref[src_row[kept]] = dout[:rows][kept]
    assert torch.equal(dx, dx_ref)                                        # routed rows are copies; nothing else is written
    for name, b_, init, want in zip(("dpos_a", "dpos_v", "dmask", "dmod_a", "dmod_v"), bufs, inits, refs):
        assert rel_err(b_[:init.numel()], want) < 1e-5, (name, D, B, T, permute, det)
        assert untouched(b_, init.numel()), name
    if det:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert lib().tuning_get("det") == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. token means
SEG_LENS = [1, 7, 8, 9, 1960]          # fewer rows than the eight row groups, one short, exact, one over; the longest sequence of the model


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("D", [4, 772, 1280])
def test_segment_mean_fwd_bwd(D, mapped):
    """D = 772: the forward's last block of 32 float4 columns holds one.  row_map sends segment s to row row_map[s] of a table with more rows than
    segments; the rows nobody maps to stay as they were."""
    o = ops()
    g = gen(D + mapped)
    nseg, total = len(SEG_LENS), sum(SEG_LENS)
    max_row = nseg + 3 if mapped else nseg
    bounds = [0]
    for n in SEG_LENS:
        bounds.append(bounds[-1] + n)
    seg = torch.tensor(bounds + [bounds[-1] + 2], dtype=torch.int32, device=DEV)        # a further boundary the kernel must not use
    rmap = torch.randperm(max_row, device=DEV, generator=g)[:nseg] if mapped else torch.arange(nseg, device=DEV)
    rmap32 = rmap.int() if mapped else None
    y = randn(g, total + 2, D)
    y[total:] = BIG
    reps = full((max_row + 1) * D).reshape(max_row + 1, D)
    o.segment_mean_fwd(y, seg, reps, nseg, row_map=rmap32, max_row=max_row if mapped else None)
    ref = torch.full((max_row + 1, D), SENT, device=DEV, dtype=torch.double)
    for s in range(nseg):
        ref[rmap[s]] = y[bounds[s]:bounds[s + 1]].double().mean(0)
    assert rel_err(reps[rmap], ref[rmap]) < 1e-6
    rest = torch.ones(max_row + 1, dtype=torch.bool, device=DEV)
    rest[rmap] = False
    assert bool((reps[rest] == SENT).all())
    # backward: plain, and the accumulating entry point both ways
    dreps = randn(g, max_row, D)
    seglen = torch.tensor(SEG_LENS, device=DEV).double()
    per_seg = -2.5 * dreps[rmap].double() / seglen[:, None]
    ref_dy = per_seg.repeat_interleave(torch.tensor(SEG_LENS, device=DEV), dim=0)
    kw = dict(row_map=rmap32, max_row=max_row if mapped else None)
    for mode in ("plain", "acc_off", "acc_on"):
        dy = randn(g, total + 2, D)
        dy[total:] = SENT
        before = dy[:total].double()
        if mode == "plain":
            o.segment_mean_bwd(dreps, seg, dy, nseg, -2.5, **kw)
        else:
            o.segment_mean_bwd_acc(dreps, seg, dy, nseg, -2.5, accumulate=mode == "acc_on", **kw)
        want = before + ref_dy if mode == "acc_on" else ref_dy
        assert rel_err(dy[:total], want) < 1e-6, (mode, D, mapped)
        assert untouched(dy, total * D), mode


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8. row expansion
def _expand_check(o, g, rows, cols, ld_in, ld_out, n_in, src, with_inp):
    inp = bf(randn(g, n_in, ld_in))
    out = bf(randn(g, rows + 2, ld_out))
    out[rows:] = SENT
    before = out.clone()
    o.expand_rows(inp if with_inp else None, src, out, rows, cols if cols != ld_out else None)
    s = src[:rows].long()
    want = before.clone()
    gathered = torch.where((s >= 0)[:, None], inp[s.clamp(min=0), :cols], torch.zeros((), dtype=torch.bfloat16, device=DEV))
    if with_inp:
        want[:rows, :cols] = gathered
    else:
        want[:rows, :cols][s < 0] = 0                                # rows with a source are left as they are
    assert torch.equal(out, want)


@pytest.mark.parametrize("sources", ["mixed", "all_negative", "none_negative"])
def test_expand_rows_column_range_and_zero_only_form(sources):
    o = ops()
    g = gen(len(sources))
    rows, n_in = 37, 11
    src = torch.randint(0, n_in, (rows + 2,), device=DEV, generator=g).to(torch.int32)
    if sources == "mixed":
        src[torch.rand(rows + 2, device=DEV, generator=g) < 0.4] = -1
    elif sources == "all_negative":
        src[:] = -1
    src[rows:] = 0                                                    # entries behind `rows`: valid, but their output rows must stay untouched
    for with_inp in (True, False):
        _expand_check(o, g, rows, 24, 48, 64, n_in, src, with_inp)    # cols < out.shape[1], ld_in != ld_out
        _expand_check(o, g, rows, 64, 64, 64, n_in, src, with_inp)


def test_expand_rows_second_grid_trip():
    o = ops()
    g = gen(8)
    rows, cols, n_in = 8200, 1024, 300                                # rows * cols / 8 = 1 049 600 16-byte chunks > 4096 * 256
    src = torch.randint(0, n_in, (rows + 2,), device=DEV, generator=g).to(torch.int32)
    src[torch.rand(rows + 2, device=DEV, generator=g) < 0.3] = -1
    src[rows:] = 0
    _expand_check(o, g, rows, cols, cols, cols, n_in, src, True)
    _expand_check(o, g, rows, cols, cols, cols, n_in, src, False)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9. batched transpose
def test_transpose_batched_descriptor_arithmetic():
    """one launch over four matrices whose tile counts are 1, 5 x 4 (ragged both ways), 1 x 3 and 2 x 1; descriptors {src, dst, R, C, first tile,
    tiles per row} as arena.ParamArena writes them"""
    o = ops()
    g = gen(9)
    shapes = [(64, 64), (300, 200), (1, 130), (65, 1)]
    srcs = [bf(randn(g, R, C)) for R, C in shapes]
    gap = 37
    dst = full(sum(R * C + gap for R, C in shapes), torch.bfloat16)
    desc, tmap, t0, off, offs = [], [], 0, gap, []
    for i, ((R, C), s) in enumerate(zip(shapes, srcs)):
        tpr, ntl = (C + 63) // 64, ((C + 63) // 64) * ((R + 63) // 64)
        desc.append([s.data_ptr(), dst[off:].data_ptr(), R, C, t0, tpr])
        tmap += [i] * ntl
        t0 += ntl
        offs.append(off)
        off += R * C + gap
    assert t0 == 1 + 20 + 3 + 2
    o.transpose_batched(torch.tensor(desc, dtype=torch.int64, device=DEV), torch.tensor(tmap, dtype=torch.int32, device=DEV), t0)
    written = torch.zeros(dst.numel(), dtype=torch.bool, device=DEV)
    for (R, C), s, a in zip(shapes, srcs, offs):
        assert torch.equal(dst[a:a + R * C].reshape(C, R), s.t().contiguous()), (R, C)
        written[a:a + R * C] = True
    assert bool((dst[~written] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 10. masked reconstruction loss
def _patchify(inp, audio, S):
    """fp64 targets [N, L, 256 * C] of the S x S corner (zero outside it): layout (p * 16 + q) * C + c; audio: the transposed spectrogram, token f * tP + t"""
    img = inp.double().transpose(1, 2).unsqueeze(1) if audio else inp.double()          # [N, C, H, W]; audio: H = mel, W = time
    N, C, H, W = img.shape
    gh, gw = H // S, W // S
    t = torch.zeros(N, gh * gw, 16, 16, C, device=inp.device, dtype=torch.double)
    for gy in range(gh):
        for gx in range(gw):
            t[:, gy * gw + gx, :S, :S, :] = img[:, :, gy * S:gy * S + S, gx * S:gx * S + S].permute(0, 2, 3, 1)
    return t.reshape(N, gh * gw, 256 * C)


def _mae_ref(pred, tgt, mask, S, C, nmask, gout):
    corner = torch.zeros(16, 16, C, device=pred.device, dtype=torch.double)
    corner[:S, :S] = 1
    d = (pred.double() - tgt.reshape(-1, tgt.shape[-1])) * corner.reshape(-1)
    row = (d * d).sum(1) / (C * S * S) * mask.double()
    dpred = gout * 2 * d * mask.double()[:, None] / (C * S * S * nmask)
    return row, row.sum() / nmask, dpred, corner.reshape(-1).bool()


MAE_CASES = [("a16", True, (1, 48, 48), 16, 9), ("a14", True, (2, 42, 28), 14, 6), ("v14", False, (2, 3, 28, 28), 14, 4),
             ("v16", False, (1, 3, 32, 48), 16, 6)]


def _mae_mask(g, N, L):
    mask = (torch.rand(N * L, device=DEV, generator=g) > 0.3).float()
    mask[N * L - 1] = 1.0
    if N > 1:
        mask[:L] = 0.0                                                # a sample with nothing masked
    return mask


def _mae_run(o, pred, inp, mask, audio, L, stride, gout, rows, xf=None, row_id=None, id_base=0, nmask=None, total=None, total_init=True):
    P = pred.shape[1]
    row_loss, loss = full(rows + 5), full(3)
    dpred = full((rows + 2) * P, torch.bfloat16).reshape(rows + 2, P)
    nmask = float(mask.sum().item()) if nmask is None else nmask
    o.mae_loss_fwd(pred, inp, mask, row_loss, loss, audio, L, nmask, total=total, total_init=total_init, xf=xf, stride=stride, row_id=row_id, id_base=id_base)
    o.mae_loss_bwd(pred, inp, mask, gout, dpred, audio, L, nmask, xf=xf, stride=stride, row_id=row_id, id_base=id_base)
    assert untouched(row_loss, rows) and untouched(loss, 1) and untouched(dpred, rows * P)
    return row_loss[:rows], loss[:1], dpred[:rows]


@pytest.mark.parametrize("name,audio,shape,stride,L", MAE_CASES)
def test_mae_loss_small_shapes_strides_and_compact_rows(name, audio, shape, stride, L):
    """a16: nine rows - the last block of four waves holds one.  Stride 14 scores the 14 x 14 corner of the 16 x 16 storage.  Compact predictions
    (row_id / id_base) give the bits of the corresponding rows of the full call."""
    o = ops()
    g = gen(len(name) + stride + L)
    N, C = shape[0], (1 if audio else 3)
    rows, P = N * L, 256 * C
    inp = randn(g, *shape)
    pred = randn(g, rows + 2, P)
    pred[rows:] = BIG
    mask = _mae_mask(g, N, L)
    nmask = float(mask.sum().item())
    gout = torch.tensor([1.7], device=DEV)
    row_ref, loss_ref, dpred_ref, corner = _mae_ref(pred[:rows], _patchify(inp, audio, stride), mask, stride, C, nmask, 1.7)
    tot = torch.full((2,), 5.0, device=DEV)
    row_loss, loss, dpred = _mae_run(o, pred, inp, mask, audio, L, stride, gout, rows, total=tot, total_init=False)
    assert abs(loss.item() - loss_ref.item()) < 1e-5 * abs(loss_ref.item())
    # a row's loss: at most 768 non-negative fp32 terms, relative error below sqrt(768) * 2^-24 ~ 2e-6: the loss's own bound holds per row
    assert rel_err(row_loss, row_ref) < 1e-5
    assert bool((row_loss[mask == 0] == 0).all())
    assert rel_err(dpred, dpred_ref) < 4e-3
    assert bool((dpred[mask == 0] == 0).all()) and bool((dpred[:, ~corner] == 0).all())       # unscored rows and positions: exactly zero
    assert abs(tot[0].item() - 5.0 - loss.item()) < 1e-5 and tot[1].item() == 5.0               # total += loss
    o.mae_loss_fwd(pred, inp, mask, full(rows), full(1), audio, L, nmask, total=tot, total_init=True, stride=stride)
    assert tot[0].item() == loss.item() and tot[1].item() == 5.0                                # total = loss
    if N > 1:
        # compact: the scored rows of the LAST sample alone, numbered in the whole batch's (sample, token) order
        base = (N - 1) * L
        ids = torch.nonzero(mask[base:]).reshape(-1) + base
        ids = ids[torch.randperm(ids.numel(), device=DEV, generator=g)]
        n_c = ids.numel()
        pred_c = torch.cat([pred[ids], torch.full((2, P), BIG, device=DEV)])
        rl_c, loss_c, dp_c = _mae_run(o, pred_c, inp[N - 1:], mask[base:], audio, L, stride, gout, n_c, row_id=ids.int(), id_base=base, nmask=nmask)
        assert torch.equal(rl_c, row_loss[ids]) and torch.equal(dp_c, dpred[ids])
        assert abs(loss_c.item() - row_ref[ids].sum().item() / nmask) < 1e-5 * abs(loss_ref.item())


@pytest.mark.parametrize("stride", [16, 14])
def test_mae_loss_raw_inputs_fused_equals_two_pass(stride):
    """the input transform applied where the target is read (xf) against the same call on the separately normalised tensor: bit for bit"""
    o = ops()
    from avsiam_amd import preprocess as pp
    g = gen(stride)
    gout = torch.tensor([0.9], device=DEV)
    S = stride
    # audio: [3, T, F] un-normalised fbank, rolled by a negative shift, a shift beyond T and none; one sample without noise
    T, Fm = 3 * S, 2 * S
    L = 6
    fb = randn(g, 3, T, Fm) * 4 - 5
    shift = torch.tensor([-7, T + 5, 0], dtype=torch.int32, device=DEV)
    amp = torch.tensor([0.05, 0.0, 0.09], dtype=torch.float32, device=DEV)
    two = pp.normalize_fbank(fb, -5.081, 4.4849, noise=True, seed=1234567890123, shift=shift, amp=amp)
    xf = o.InputXf.audio(-5.081, 4.4849, shift, amp, seed=1234567890123)
    rows = 3 * L
    pred, mask = randn(g, rows, 256), _mae_mask(g, 3, L)
    a = _mae_run(o, pred, fb, mask, True, L, S, gout, rows, xf=xf)
    b = _mae_run(o, pred, two, mask, True, L, S, gout, rows)
    for x, y, what in zip(a, b, ("row_loss", "loss", "dpred")):
        assert torch.equal(x, y), ("audio", what)
    # the roll really happened: the two-pass tensor is the fp64 formula on the rolled input up to fp32 rounding, noise in [0, amp)
    for i in range(3):
        d = two[i].double() - torch.roll((fb[i].double() + 5.081) / 4.4849, int(shift[i]), 0)
        assert float(d.min()) >= -1e-5 and float(d.max()) < float(amp[i]) + 1e-5
    # frames: uint8 [2, 3, H, W]
    H, W = 2 * S, 3 * S
    fr = torch.randint(0, 256, (2, 3, H, W), device=DEV, generator=g, dtype=torch.uint8)
    rows = 2 * L
    pred, mask = randn(g, rows, 768), _mae_mask(g, 2, L)
    a = _mae_run(o, pred, fr, mask, False, L, S, gout, rows, xf=o.InputXf.frames())
    b = _mae_run(o, pred, pp.normalize_frames(fr), mask, False, L, S, gout, rows)
    for x, y, what in zip(a, b, ("row_loss", "loss", "dpred")):
        assert torch.equal(x, y), ("frames", what)
    with pytest.raises(lib().AvsiamHipError):                           # an audio transform beside frames
        _mae_run(o, pred, fr, mask, False, L, S, gout, rows, xf=xf)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 11. patch gathers
def _subset(g, n_items, L):
    """a random subset of the (item, token) pairs in random order"""
    pick = torch.randperm(n_items * L, device=DEV, generator=g)[:max(1, (n_items * L * 3) // 5)]
    return (pick // L).int(), (pick % L).int(), pick.numel()


def _gather_audio(a, row_b, row_tok, S, tP):
    """out[r, p * 16 + q] = a[b, t * S + q, f * S + p] inside the S x S corner, zero outside"""
    rows = row_b.numel()
    out = torch.zeros(rows, 16, 16, device=a.device, dtype=a.dtype)
    f, t = row_tok.long() // tP, row_tok.long() % tP
    for r in range(rows):
        out[r, :S, :S] = a[row_b[r], t[r] * S:t[r] * S + S, f[r] * S:f[r] * S + S].t()
    return out.reshape(rows, 256)


def _gather_video(v, row_img, row_tok, S, G):
    """out[r, c * 256 + p * 16 + q] = v[img, c, gy * S + p, gx * S + q] inside the corner, zero outside"""
    rows, C = row_img.numel(), v.shape[1]
    out = torch.zeros(rows, C, 16, 16, device=v.device, dtype=v.dtype)
    gy, gx = row_tok.long() // G, row_tok.long() % G
    for r in range(rows):
        out[r, :, :S, :S] = v[row_img[r], :, gy[r] * S:gy[r] * S + S, gx[r] * S:gx[r] * S + S]
    return out.reshape(rows, C * 256)


@pytest.mark.parametrize("stride", [16, 14])
def test_im2col_row_subsets_strides_and_raw_inputs(stride):
    o = ops()
    from avsiam_amd import preprocess as pp
    g = gen(40 + stride)
    S = stride
    # ---- audio [B, time, mel]
    B, tP, fP = 3, 4, 2
    a = randn(g, B, tP * S, fP * S)
    row_b, row_tok, rows = _subset(g, B, tP * fP)
    out = full((rows + 2) * 256, torch.bfloat16).reshape(rows + 2, 256)
    o.im2col_audio(a, row_b, row_tok, out, rows, tP, stride=S)
    want = bf(_gather_audio(a, row_b, row_tok, S, tP))
    assert torch.equal(out[:rows], want) and untouched(out, rows * 256)
    corner = torch.zeros(16, 16, dtype=torch.bool, device=DEV)
    corner[:S, :S] = True
    assert bool((out[:rows][:, ~corner.reshape(-1)] == 0).all())
    # the patch embedding as a convolution with an S x S kernel and stride S; the stored 16 x 16 weights are zero outside the corner
    w = torch.zeros(8, 1, 16, 16, device=DEV, dtype=torch.double)
    w[:, :, :S, :S] = randn(g, 8, 1, S, S).double()
    img = bf(a).double().unsqueeze(1).transpose(2, 3)
    conv = F.conv2d(img, w[:, :, :S, :S].contiguous(), stride=S).flatten(2).transpose(1, 2)              # [B, L, 8], token f * tP + t
    assert rel_err(out[:rows].double() @ w.reshape(8, 256).t(), conv[row_b.long(), row_tok.long()]) < 1e-6
    # raw fbank + transform == gather of the separately normalised tensor
    fb = a * 4 - 5
    shift = torch.tensor([-9, tP * S + 3, 0], dtype=torch.int32, device=DEV)
    amp = torch.tensor([0.07, 0.0, 0.02], dtype=torch.float32, device=DEV)
    xf = o.InputXf.audio(-5.081, 4.4849, shift, amp, seed=99)
    two = pp.normalize_fbank(fb, -5.081, 4.4849, noise=True, seed=99, shift=shift, amp=amp)
    out1 = full((rows + 2) * 256, torch.bfloat16).reshape(rows + 2, 256)
    o.im2col_audio(fb, row_b, row_tok, out1, rows, tP, xf=xf, stride=S)
    assert torch.equal(out1[:rows], bf(_gather_audio(two, row_b, row_tok, S, tP))) and untouched(out1, rows * 256)
    # ---- video [NF, 3, H, W]
    NF, gh, gw = 3, 2, 3
    v = randn(g, NF, 3, gh * S, gw * S)
    row_img, row_tok, rows = _subset(g, NF, gh * gw)
    outv = full((rows + 2) * 768, torch.bfloat16).reshape(rows + 2, 768)
    o.im2col_video(v, row_img, row_tok, outv, rows, stride=S)
    assert torch.equal(outv[:rows], bf(_gather_video(v, row_img, row_tok, S, gw))) and untouched(outv, rows * 768)
    assert bool((outv[:rows].reshape(rows, 3, 256)[:, :, ~corner.reshape(-1)] == 0).all())
    wv = torch.zeros(8, 3, 16, 16, device=DEV, dtype=torch.double)
    wv[:, :, :S, :S] = randn(g, 8, 3, S, S).double()
    convv = F.conv2d(bf(v).double(), wv[:, :, :S, :S].contiguous(), stride=S).flatten(2).transpose(1, 2)
    assert rel_err(outv[:rows].double() @ wv.reshape(8, 768).t(), convv[row_img.long(), row_tok.long()]) < 1e-6
    fr = torch.randint(0, 256, (NF, 3, gh * S, gw * S), device=DEV, generator=g, dtype=torch.uint8)
    out2 = full((rows + 2) * 768, torch.bfloat16).reshape(rows + 2, 768)
    o.im2col_video(fr, row_img, row_tok, out2, rows, xf=o.InputXf.frames(), stride=S)
    assert torch.equal(out2[:rows], bf(_gather_video(pp.normalize_frames(fr), row_img, row_tok, S, gw))) and untouched(out2, rows * 768)
    # refused before anything is launched: a transform of the other kind, a zero std
    for bad_call in (lambda: o.im2col_audio(fb, row_b, row_tok, out1, 1, tP, xf=o.InputXf.frames(), stride=S),
                     lambda: o.im2col_video(fr, row_img, row_tok, out2, 1, xf=xf, stride=S),
                     lambda: o.im2col_audio(fb, row_b, row_tok, out1, 1, tP, xf=o.InputXf.audio(0.0, 0.0), stride=S),
                     lambda: o.im2col_video(fr, row_img, row_tok, out2, 1, xf=o.InputXf.frames(std=(0.2, 0.0, 0.2)), stride=S)):
        k1, k2 = out1.clone(), out2.clone()
        with pytest.raises(lib().AvsiamHipError):
            bad_call()
        torch.cuda.synchronize()
        assert torch.equal(out1, k1) and torch.equal(out2, k2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 12. the noise stream
def philox4x32_10_word0(c0, c1, seed):
    """first output word of Philox4x32-10 for counters (c0, c1, 0, 0) (uint32 arrays) and the 64-bit key `seed`"""
    u = np.uint64
    mask, s32 = u(0xFFFFFFFF), u(32)
    c0, c1 = c0.astype(np.uint64), c1.astype(np.uint64)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = u(seed & 0xFFFFFFFF), u((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + u(0x9E3779B9)) & mask, (k1 + u(0xBB67AE85)) & mask
    return c0


def test_philox_stream_of_the_noise_augmentation():
    """normalize_fbank(noise=True) minus the noiseless result is amp_b * (word >> 8) / 2^24 with word = Philox4x32-10(counter (ts * F + f, b, 0, 0),
    key = seed)[0], ts the SOURCE time frame of the rolled output."""
    from avsiam_amd import preprocess as pp
    # the numpy restatement against the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors; counters with c2 = c3 = 0 only
    # are reachable here, so the all-zero vector is the one that applies)
    assert int(philox4x32_10_word0(np.zeros(1, np.uint32), np.zeros(1, np.uint32), 0)[0]) == 0x6627E8D5
    B, T, Fm, seed = 2, 8, 8, (0xDEADBEEF << 32) | 0x12345678
    g = gen(12)
    fb = randn(g, B, T, Fm) * 4 - 5
    shift = torch.tensor([3, -2], dtype=torch.int32, device=DEV)
    amp = torch.tensor([0.08, 0.031], dtype=torch.float32, device=DEV)
    noisy = pp.normalize_fbank(fb, -5.081, 4.4849, noise=True, seed=seed, shift=shift, amp=amp)
    clean = pp.normalize_fbank(fb, -5.081, 4.4849, shift=shift)
    for b in range(B):
        assert torch.allclose(clean[b], torch.roll((fb[b] + 5.081) / 4.4849, int(shift[b]), 0), rtol=1e-6, atol=1e-6)
    t = np.arange(T)[None, :, None]
    ts = (t - shift.cpu().numpy()[:, None, None]) % T                                        # output frame t shows source frame ts
    c0 = (ts * Fm + np.arange(Fm)[None, None, :]).astype(np.uint32)
    c1 = np.broadcast_to(np.arange(B, dtype=np.uint32)[:, None, None], c0.shape)
    word = philox4x32_10_word0(c0, c1, seed)
    want = amp.cpu().numpy().astype(np.float64)[:, None, None] * ((word >> np.uint64(8)).astype(np.float64) / 2.0 ** 24)
    got = noisy.double().cpu().numpy() - clean.double().cpu().numpy()
    # fp32 rounding: the product amp * u and the sum are rounded once each (half an ulp = 2^-24 relative); allowed: a whole ulp of each
    bound = 2.0 ** -23 * (np.abs(noisy.cpu().numpy().astype(np.float64)) + want)
    assert (np.abs(got - want) <= bound).all(), float(np.abs(got - want).max())
    assert float(want.max()) > 0.05                                                           # the check is not vacuous


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 13. contrastive head
@pytest.mark.parametrize("D", [4, 300, 768])
def test_l2norm_with_a_zero_row(D):
    """F.normalize and its autograd in fp64; an all-zero row has norm eps = 1e-12 and yields no NaN either way.
    Bounds: the sum of D <= 768 squares through 256 lanes, a wave and a block fold is at most ~14 fp32 additions deep: relative error below
    16 * 2^-24 ~ 1e-6 in the squared norm, half of it in the norm, plus the division's half ulp - 1e-6 forward.  The backward adds a D-term dot
    product against vectors of comparable size and three more roundings: 1e-5."""
    o = ops()
    g = gen(D)
    rows = 6
    x = randn(g, rows, D)
    x[2] = 0
    xn = full((rows + 1) * D).reshape(rows + 1, D)
    norm = full(rows + 3)
    o.l2norm_fwd(x, xn[:rows], norm)
    xr = x.double().requires_grad_(True)
    ref = F.normalize(xr, dim=1, eps=1e-12)
    assert bool(torch.isfinite(xn).all()) and bool(torch.isfinite(norm).all())
    assert rel_err(xn[:rows], ref) < 1e-6 and bool((xn[2] == 0).all())
    assert rel_err(norm[:rows], x.double().norm(dim=1).clamp_min(1e-12)) < 1e-6
    assert norm[2].item() == float(np.float32(1e-12))
    assert untouched(xn, rows * D) and untouched(norm, rows)
    dxn = randn(g, rows, D)
    dx = full((rows + 1) * D).reshape(rows + 1, D)
    o.l2norm_bwd(dxn, xn[:rows], norm, dx[:rows], 0.5)
    (ref * dxn.double()).sum().backward()
    assert bool(torch.isfinite(dx).all())
    live = torch.arange(rows, device=DEV) != 2
    assert rel_err(dx[:rows][live], 0.5 * xr.grad[live]) < 1e-5
    assert rel_err(dx[2], 0.5 * xr.grad[2]) < 1e-6                                   # dxn / eps: one division
    assert untouched(dx, rows * D)


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (33, 31, 7), (65, 130, 768)])
def test_gemm_f32_small_stride_forms(M, N, K):
    """the three products of the contrastive loss: A . B^T (logits), A . B and A^T . B (their gradients), each with alpha != 1"""
    o = ops()
    g = gen(M + N + K)

    def run(A, sa, Bm, sb, ref):
        C = full((M + 2) * N).reshape(M + 2, N)
        o.gemm_f32_small(A, Bm, C, M, N, K, sa, sb, -0.3)
        assert rel_err(C[:M], -0.3 * ref) < 1e-5, (M, N, K, sa, sb)
        assert untouched(C, M * N)

    A, Bt = randn(g, M, K), randn(g, N, K)
    run(A, (K, 1), Bt, (1, K), A.double() @ Bt.double().t())
    Bn = randn(g, K, N)
    run(A, (K, 1), Bn, (N, 1), A.double() @ Bn.double())
    At = randn(g, K, M)
    run(At, (1, M), Bn, (N, 1), At.double().t() @ Bn.double())


def _infonce_ref(total, gout, weight):
    t = total.double().cpu().requires_grad_(True)
    n = t.shape[0]
    nce = -0.5 * (torch.diag(F.log_softmax(t, dim=0)).mean() + torch.diag(F.log_softmax(t.t(), dim=0)).mean())
    (gout * weight * nce).backward()
    tn = total.cpu().numpy()
    hits = (np.argmax(tn, axis=0) == np.arange(n)).astype(np.float64) + (np.argmax(tn, axis=1) == np.arange(n))
    return nce.item(), hits, t.grad


@pytest.mark.parametrize("N", [1, 2, 257])
def test_infonce_sizes_and_first_index_ties(N):
    """N = 257: one more than the block's threads.  Equal maxima in a row and in a column: the first index wins, as numpy.argmax has it."""
    o = ops()
    g = gen(N)
    total = randn(g, N, N) * 4
    total.diagonal().add_(6.0)
    if N == 257:
        total[5, 5] = total[5, 200] = 30.0            # row 5: first maximum on the diagonal - a hit
        total[7, 3] = total[7, 7] = 31.0              # row 7: the diagonal is the SECOND maximum - no hit
        total[9, 19] = total[100, 19] = 32.0          # column 19: rows 9 and 100 tie, neither on the diagonal
        total[11, 21] = total[21, 21] = 33.0          # column 21: the diagonal (row 21) is the second maximum - no hit
        total[40, 0] = total[40, 256] = 34.0          # row 40: both maxima belong to the same thread (k = 0, 256)
        total[0, 50] = total[256, 50] = 35.0          # column 50 likewise
        total[60, 60] = total[64, 60] = 36.0          # column 60: the diagonal first, the tie in the next wave - a hit
    stats = full((N + 1) * 4).reshape(N + 1, 4)
    out = full(8)
    o.infonce_fwd(total, stats[:N], out, 0.01)
    nce, hits, dref = _infonce_ref(total, 0.9, 0.01)
    assert abs(out[0].item() - nce) < 1e-5 * abs(nce) + 1e-6
    assert np.array_equal(stats[:N, 3].cpu().numpy().astype(np.float64), hits)
    assert abs(out[1].item() - hits.sum() / (2 * N)) < 1e-6
    assert abs(out[2].item() - 0.01 * out[0].item()) < 1e-7
    assert untouched(stats, N * 4) and untouched(out, 3)
    dtotal = full((N + 1) * N).reshape(N + 1, N)
    o.infonce_dlogits(total, stats[:N], torch.tensor([0.9], device=DEV), 0.01, dtotal[:N])
    assert untouched(dtotal, N * N)
    if N == 1:
        assert out[0].item() == 0.0 and out[1].item() == 1.0 and dtotal[0, 0].item() == 0.0
    else:
        # fp32 exp of t - lse with |t|, |lse| up to ~40: the subtraction and the stored lse carry an absolute error of ~2 * 40 * 2^-24 = 5e-6, which
        # is the relative error of the exponential; 1e-5
        assert rel_err(dtotal[:N].cpu(), dref) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 14. fp8 operand preparation, batched zero-fill
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 7, 9, 2048 * 256 * 8 + 3])
def test_absmax_tail_and_second_grid_trip(n, dtype):
    """the maximum is the LAST element and negative; what lies behind it is larger and must not be read"""
    o = ops()
    buf = (torch.rand(n + 8, device=DEV, generator=gen(n % 1000)) * 2 - 1).to(dtype)
    buf[n - 1] = -3.5
    buf[n:] = BIG
    assert o.absmax(buf[:n]) == 3.5
    if n > 1:
        buf[n - 1] = 0.25
        assert o.absmax(buf[:n]) == buf[:n].float().abs().max().item()


@pytest.mark.parametrize("e5m2", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [4, WRAP4 + 4])
def test_quantize_fp8_saturation_and_second_grid_trip(n, dtype, e5m2):
    o = ops()
    fmax, f8 = (57344.0, torch.float8_e5m2) if e5m2 else (448.0, torch.float8_e4m3fn)
    scale = 0.75
    x = (randn(gen(n % 1000 + e5m2), n + 8) * fmax * 0.6).to(dtype)            # a good part of the values lies beyond +-fmax / scale
    x[0], x[1], x[2], x[n - 1] = 1e6, -1e6, 0.3, -2 * fmax
    x[n:] = 1.0
    y = full(n + 8, torch.uint8, SENT8)
    o.quantize_fp8(x[:n], scale, out=y[:n], e5m2=e5m2)
    want = (x[:n].float() * scale).clamp(-fmax, fmax).to(f8)
    assert torch.equal(y[:n].view(f8), want)
    assert want[0].float().item() == fmax and want[1].float().item() == -fmax and want[n - 1].float().item() == -fmax
    assert untouched(y, n, SENT8)


def test_fp8_batch_chunk_map_and_records():
    """one launch over tensors of 4, 8192 (one full chunk), 8196 (a second chunk of one group) and 3 * 8192 elements with a record each"""
    o = ops()
    g = gen(14)
    sizes = [4, 8192, 8196, 3 * 8192]
    scales = [1.0, 0.5, 2.0, 3.0]
    gap = 16
    srcbuf = bf(randn(g, sum(sizes) + gap * (len(sizes) + 1)) * 100)
    dstbuf = full(srcbuf.numel(), torch.uint8, SENT8)
    rec, rec_sep = o.Fp8Records(4, DEV), o.Fp8Records(4, DEV)
    for r in (rec, rec_sep):
        r.q[:, 0] = torch.tensor(scales, device=DEV)
        r.q[:, 1] = 1.0 / torch.tensor(scales, device=DEV)
    fb8 = o.Fp8Batch(rec)
    off, spans = gap, []
    for i, n in enumerate(sizes):
        src = srcbuf[off:off + n]
        src[n - 1] = -(500.0 + 100 * i)                                  # the largest magnitude sits in the last element
        fb8.add(src, dstbuf[off:off + n], (i + 2) % 4)                   # records in another order than the tensors
        spans.append((off, n, (i + 2) % 4))
        off += n + gap
    fb8.build(DEV)
    assert fb8.nchunks == 1 + 1 + 2 + 3
    fb8.run()
    first = dstbuf.clone()
    written = torch.zeros(dstbuf.numel(), dtype=torch.bool, device=DEV)
    for a, n, r in spans:
        sep = o.quantize_fp8(srcbuf[a:a + n], 123.0, q=rec_sep.rec(r))
        assert torch.equal(dstbuf[a:a + n], sep), n
        assert torch.equal(sep.view(torch.float8_e4m3fn), (srcbuf[a:a + n].float() * scales[r]).clamp(-448, 448).to(torch.float8_e4m3fn))
        assert rec.amax(r) == srcbuf[a:a + n].float().abs().max().item()
        written[a:a + n] = True
    assert bool((dstbuf[~written] == SENT8).all())
    fb8.run()
    assert torch.equal(dstbuf, first)
    rec.update()
    for a, n, r in spans:
        assert rec.hist[0, r].item() == srcbuf[a:a + n].float().abs().max().item()


def test_zero_table_regions_and_their_neighbours():
    """16 B (one thread), 64 KiB (one full chunk), 64 KiB + 16 B (a second chunk of one store) and an empty tensor, zeroed by one launch"""
    o = ops()
    sizes = [16, 65536, 65552, 0]
    gap = 48
    buf = full(sum(sizes) + gap * (len(sizes) + 1), torch.uint8, SENT8)
    zt = o.ZeroTable()
    off, zeroed = gap, torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    for n in sizes:
        zt.add(buf[off:off + n])
        zeroed[off:off + n] = True
        off += n + gap
    zt.build(DEV)
    assert zt.nchunks == 1 + 1 + 2
    zt.run()
    assert bool((buf[zeroed] == 0).all()) and bool((buf[~zeroed] == SENT8).all())
    empty = o.ZeroTable()
    empty.add(buf[0:0])
    empty.build(DEV)
    empty.run()                                                           # nothing to launch
    assert bool((buf[~zeroed] == SENT8).all())
