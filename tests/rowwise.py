"""Row-resolved error measures and plain references for the MFMA GEMM, attention and LayerNorm kernels.

A whole-tensor norm ||got - ref|| / ||ref|| dilutes damage that is local - one row scaled by 1.01, a clamped last row, one
fragment with another fragment's bias - below the tolerance the honest rounding already needs.  The measures here look at
every element (GEMM: a bound derived from fp32 accumulation and the output rounding), every row (LayerNorm) or every
(sequence, head, row) (attention: the row's error over the norm of the same formula with every factor replaced by its
absolute value, so that a row whose gradient cancels is still measured against what went into it).

Pure torch, no call into the library: every function runs on whatever device its inputs live on (the tests evaluate them on the
CPU).  tests/test_rowwise_cpu.py proves on emulations that the measures accept honest rounding and reject subtle damage;
tests/test_rowwise_gpu.py applies them to the kernels.  For attention inputs whose softmax is peaked, tied or shifted (ATTN_PROFILES) the
magnitude rows are the *_full ones (attention_measures_full): tests/test_attn_peaked_cpu.py / tests/test_attn_peaked_gpu.py."""
import math

import torch

U_BF16 = 2.0 ** -8            # unit roundoff of a bf16 result (8 significant bits, round to nearest)
U_F32 = 2.0 ** -24            # ... of an fp32 one
F64 = torch.float64
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
GP8_STEPS, GP8_BIAS = 202.0, 0.1296875          # gelu'(x) as 8-bit codes: round((g' + GP8_BIAS) * GP8_STEPS) (csrc/gemm.hip)
NT_ROW_TOL = {torch.bfloat16: 4e-3, torch.float32: 1e-5}     # the suite's whole-tensor tolerances, applied per row


def f32(v):
    """the value a C float argument carries"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def whole_rel(got, ref):
    """the suite's existing yardstick (tests/test_kernels_gpu.py rel_err)"""
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-30))


def row_rel(got, ref):
    """||got - ref|| / ||ref|| of every row -> [rows]"""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-300)


def elem_ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements (an element whose bound is 0 must be exact) -> (ratio, flat index)"""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    r = torch.nan_to_num(r, nan=float("inf"))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def bitwise_equal(a, b):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ---------------------------------------------------------------------------------------------------
# guard bands
SENTINEL = {torch.bfloat16: 7.0, torch.float32: 7.0, torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}


def guarded(rows, cols, dtype, device, extra_rows=264, extra_cols=0):
    """An output of [rows, cols] allocated with extra rows (more than one 256-row tile) and, for the leading-dimension cases, extra
    columns, everything filled with a sentinel that is not zero.  -> (buf [rows + extra_rows, cols + extra_cols], check): check()
    asserts that the extra rows and columns are bitwise unchanged and returns the valid part."""
    buf = torch.full((rows + extra_rows, cols + extra_cols), SENTINEL[dtype], dtype=dtype, device=device)
    want = buf[:1, :1].clone()

    def check():
        pad_r, pad_c = buf[rows:], buf[:rows, cols:]
        assert bitwise_equal(pad_r, want.expand_as(pad_r)), ("rows beyond the output were written", _first_bad(pad_r, want, rows))
        assert bitwise_equal(pad_c, want.expand_as(pad_c)), "columns beyond the output were written"
        return buf[:rows, :cols]

    return buf, check


def _first_bad(pad, want, base):
    bad = torch.nonzero((pad.float() != want.float()).any(dim=1)).flatten()
    return [base + int(v) for v in bad[:4]]


def untouched(buf, mask):
    """the elements of `buf` under `mask` (bool, broadcastable to buf) still hold the sentinel of the buffer's dtype"""
    sel = buf[mask.expand_as(buf)]
    s = torch.full((1,), SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device)
    return bitwise_equal(sel, s.expand_as(sel))


# ---------------------------------------------------------------------------------------------------
# GEMM: x = a_c * ((A . B^T + bias) * aux + res),  a_c = alpha, times col_scale in columns [0, scale_cols)
def gemm_nt_terms(A, B, bias=None, res=None, res_idx=None, aux=None, alpha=1.0, scale_cols=0, col_scale=1.0, m_split=0, B2=None, bias2=None):
    """fp64 reference x of the epilogue's value on the bf16-rounded operands, and the magnitude S = |a_c| ((|A| |B|^T + |bias|) |aux| + |res|)
    every rounding error of the evaluation is proportional to.  Rows from m_split meet (B2, bias2)."""
    Ad = A.double()
    M = Ad.shape[0]

    def part(rows, Bm, bm):
        Bd = Bm.double()
        x, S = Ad[rows] @ Bd.t(), Ad[rows].abs() @ Bd.abs().t()
        if bm is not None:
            x, S = x + bm.double(), S + bm.double().abs()
        return x, S

    if B2 is not None and 0 < m_split < M:
        (x0, S0), (x1, S1) = part(slice(0, m_split), B, bias), part(slice(m_split, M), B2, bias2)
        x, S = torch.cat([x0, x1]), torch.cat([S0, S1])
    else:
        x, S = part(slice(0, M), B, bias)
    if aux is not None:
        x, S = x * aux.double(), S * aux.double().abs()
    if res is not None:
        r = res.double()
        r = r[res_idx.long()] if res_idx is not None else r[:M]
        x, S = x + r, S + r.abs()
    ac = torch.full((x.shape[1],), f32(alpha), dtype=F64, device=x.device)
    ac[:scale_cols] = f32(f32(alpha) * f32(col_scale))
    return x * ac, S * ac.abs()


def gemm_bound(ref, S, K, u_out):
    """|got - ref| <= u_out |ref| + (K + 3) 2^-24 S (1 + u_out): K products (exact in fp32: bf16 x bf16) summed in fp32 in ANY order
    (splits and atomics included), three more fp32 operations in the epilogue, one rounding of the output"""
    return u_out * ref.abs() + (K + 3) * U_F32 * S * (1 + u_out)


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_grad_bound(dx, g, codes=False):
    """gelu'(x^) against gelu'(x): max |gelu''| = 2 phi(0) = 0.8 times the pre-activation's error, the 5.0e-5 fit error of Phi
    (csrc/common.h), and the rounding of what is stored: bf16, or half a step of the 8-bit code (encoded from the fp32 value)"""
    return 0.8 * dx + 5.0e-5 + (0.5 / GP8_STEPS + 2e-7 if codes else U_BF16 * g.abs())


def gelu_bound(dx, g):
    """gelu(x^) against gelu(x): Lipschitz constant 1.13, fit error 2.5e-5, bf16 rounding"""
    return 1.13 * dx + 2.5e-5 + U_BF16 * g.abs()


def gp8_decode(codes):
    """what the act-2 epilogue multiplies by when `aux` holds codes: fmaf(code, float(1 / 202), -GP8_BIAS), one fp32 rounding"""
    return (codes.double() * f32(1.0 / GP8_STEPS) - GP8_BIAS).float().double()


def gp8_value(codes):
    return codes.double() / GP8_STEPS - GP8_BIAS


def colsum_bound(x, S, K, c0):
    """fp32 column sum of the values BEFORE their bf16 rounding, added to c0: the per-element bounds without the output rounding,
    summed, plus the summation itself - (M + 1) 2^-24 (sum |x| + |c0|)"""
    M = x.shape[0]
    return ((K + 3) * U_F32 * S * (1 + U_BF16)).sum(0) + (M + 1) * U_F32 * (x.abs().sum(0) + c0.double().abs())


def gemm_tn_terms(A, B, C0):
    """C = C0 + A^T . B over the M token rows: reference and magnitude (the contraction runs over M, and C0 is one more term)"""
    Ad, Bd = A.double(), B.double()
    return Ad.t() @ Bd + C0.double(), Ad.abs().t() @ Bd.abs() + C0.double().abs()


def check_gemm(got, ref, S, K, dtype=None):
    """-> {elem: worst ratio to the per-element bound, row: worst per-row norm error over the suite's tolerance}"""
    dtype = dtype or got.dtype
    u = U_BF16 if dtype == torch.bfloat16 else U_F32
    e, i = elem_ratio(got, ref, gemm_bound(ref, S, K, u))
    rr = row_rel(got, ref)
    live = ref.double().norm(dim=-1) > 0
    r = float((rr[live] / NT_ROW_TOL[dtype]).max()) if bool(live.any()) else 0.0
    return {"elem": e, "row": r, "at": (i // ref.shape[1], i % ref.shape[1])}


# ---------------------------------------------------------------------------------------------------
# attention on the packed qkv matrix [rows, 3 D]; the q columns arrive multiplied by hd^-0.5 * log2(e) and rounded to bf16 (the qkv
# GEMM's epilogue), so s = q~ . k is the score in log2 units; the gradients are those with respect to the unscaled q
def attn_q_scale(hd):
    return hd ** -0.5 * LOG2E


def _heads(x, H):
    L, D = x.shape
    return x.reshape(L, H, D // H).permute(1, 0, 2)               # [H, L, hd]


def _rows(x):
    H, L, hd = x.shape
    return x.permute(1, 0, 2).reshape(L, H * hd)


def attention_eval(qkv, lens, H, dout, lq=0, emulate=False, mutant=None):
    """Forward and backward of every sequence, written out as formulas:
        P = softmax(scale q k^T), out = P v, lse = log sum exp (natural log of the scaled scores: what the kernels store),
        dP = dO v^T, delta = sum_d out dO, dS = P o (dP - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T dO.
    emulate=False: fp64 on the bf16 operands, plus the magnitude rows (every factor replaced by its absolute value, every difference by a
    sum): out_abs = P |v|, dS_abs = P o (|dP| + |delta|), dq_abs = scale dS_abs |k|, dk_abs = scale dS_abs^T |q|, dv_abs = P^T |dO|,
    delta_abs = sum_d |out dO|.
    emulate=True: the same in fp32 with bf16 rounding where the kernels round - P before P.v (unnormalised, relative to the row maximum;
    its fp32 row sum divides afterwards), `out`, the P of the backward (recomputed from the stored lse) before P^T.dO, dS before its two
    products, dq / dk / dv - and delta from the ROUNDED out.
    lq > 0: only the first lq rows of every sequence are queries; out / dout are compact (sequence s owns rows s * lq ..), lse / delta and
    the gradients keep the packed numbering (zeros where nothing is defined).
    emulate=False also returns dq_full / dk_full / dv_full, the magnitude rows with every FACTOR made absolute (dS_abs takes |.| of the sums dP
    and delta, which on a peaked row both cancel to far less than the rounding that delta carries from the bf16 out):
    dS_full = P o (|dO| |v|^T + sum_d |out dO|), dq_full = scale dS_full |k|, dk_full = ln 2 dS_full^T |q~|, dv_full = P^T |dO| (= dv_abs).
    mutant (emulate only; the damage of the CPU proofs, tests/test_attn_peaked_cpu.py): ("bwd_tail_key", L, h) - in the sequence of length L, head
    h, the backward of ONE query row (the one whose score of that key is lowest) also sees key L, the following row of the packed matrix.
    -> dict of [rows, D] (out: [nq, D]) and [H, rows] tensors."""
    dt = torch.float32 if emulate else F64
    D = qkv.shape[1] // 3
    hd = D // H
    scale = hd ** -0.5
    rows = sum(lens)
    dev = qkv.device
    nq = sum(min(lq, L) if lq else L for L in lens)
    res = {k: torch.zeros(nq if k.startswith("out") else rows, D, dtype=dt, device=dev) for k in ("out", "dq", "dk", "dv", "out_abs", "dq_abs", "dk_abs", "dv_abs")}
    if not emulate:
        for k in ("dq_full", "dk_full", "dv_full"):
            res[k] = torch.zeros(rows, D, dtype=dt, device=dev)
    for k in ("lse", "delta", "delta_abs"):
        res[k] = torch.zeros(H, rows, dtype=dt, device=dev)
    r0 = o0 = 0
    for L in lens:
        Lq = min(lq, L) if lq else L
        x = qkv[r0:r0 + L].to(dt)
        qt, k, v = _heads(x[:, :D], H)[:, :Lq], _heads(x[:, D:2 * D], H), _heads(x[:, 2 * D:], H)
        dO = _heads(dout[o0:o0 + Lq].to(dt), H)
        s2 = qt @ k.transpose(1, 2)                                 # log2 units
        if emulate:
            m = s2.max(dim=-1, keepdim=True).values
            p = torch.exp2(s2 - m)
            l = p.sum(-1, keepdim=True)
            out = bf16_round((bf16_round(p) @ v) / l)
            lse = ((m + torch.log2(l)) * LN2).squeeze(-1)
            P = torch.exp2(s2 - lse.unsqueeze(-1) * LOG2E)
            Pv = bf16_round(P)
        else:
            sn = s2 * LN2
            lse = torch.logsumexp(sn, dim=-1)
            P = torch.exp(sn - lse.unsqueeze(-1))
            out = P @ v
            Pv = P
        dP = dO @ v.transpose(1, 2)
        delta = (out * dO).sum(-1)
        dS = P * (dP - delta.unsqueeze(-1))
        dSm = bf16_round(dS) if emulate else dS
        dq = (dSm @ k) * scale
        if emulate and mutant is not None and mutant[0] == "bwd_tail_key" and mutant[1] == L and r0 + L < qkv.shape[0]:
            h = mutant[2]
            kx = qkv[r0 + L, D + h * hd:D + (h + 1) * hd].to(dt)
            vx = qkv[r0 + L, 2 * D + h * hd:2 * D + (h + 1) * hd].to(dt)
            sx = qt[h] @ kx
            i = int(sx.argmin())
            px = torch.exp2(sx[i] - lse[h, i] * LOG2E)
            dsx = bf16_round(px * (dO[h, i] @ vx - delta[h, i]))
            dq[h, i] = dq[h, i] + dsx * kx * scale
        dk = (dSm.transpose(1, 2) @ qt) * LN2                      # scale q = q~ ln 2
        dv = Pv.transpose(1, 2) @ dO
        if emulate:
            for name, t, n in (("dq_raw", dq, Lq), ("dk_raw", dk, L), ("dv_raw", dv, L)):      # the fp32 values before their rounding: what an 8-bit copy is taken from
                res.setdefault(name, torch.zeros(rows, D, dtype=dt, device=dev))[r0:r0 + n] = _rows(t)
            dq, dk, dv = bf16_round(dq), bf16_round(dk), bf16_round(dv)
        res["out"][o0:o0 + Lq] = _rows(out)
        res["dq"][r0:r0 + Lq] = _rows(dq)
        res["dk"][r0:r0 + L] = _rows(dk)
        res["dv"][r0:r0 + L] = _rows(dv)
        res["lse"][:, r0:r0 + Lq] = lse
        res["delta"][:, r0:r0 + Lq] = delta
        if not emulate:
            dSa = P * (dP.abs() + delta.abs().unsqueeze(-1))
            res["out_abs"][o0:o0 + Lq] = _rows(P @ v.abs())
            res["dq_abs"][r0:r0 + Lq] = _rows((dSa @ k.abs()) * scale)
            res["dk_abs"][r0:r0 + L] = _rows((dSa.transpose(1, 2) @ qt.abs()) * LN2)
            res["dv_abs"][r0:r0 + L] = _rows(P.transpose(1, 2) @ dO.abs())
            res["delta_abs"][:, r0:r0 + Lq] = (out * dO).abs().sum(-1)
            dSf = P * (dO.abs() @ v.abs().transpose(1, 2) + (out * dO).abs().sum(-1, keepdim=True))
            res["dq_full"][r0:r0 + Lq] = _rows((dSf @ k.abs()) * scale)
            res["dk_full"][r0:r0 + L] = _rows((dSf.transpose(1, 2) @ qt.abs()) * LN2)
            res["dv_full"][r0:r0 + L] = res["dv_abs"][r0:r0 + L]
        r0 += L
        o0 += Lq
    return res


def head_row_ratio(got, ref, mag, H):
    """per (row, head): ||got - ref|| / ||mag|| over the head's columns -> [rows, H] (a unit whose magnitude is 0 must be exact)"""
    rows, D = ref.shape
    e = (got.double() - ref.double()).reshape(rows, H, D // H).norm(dim=-1)
    m = mag.double().reshape(rows, H, D // H).norm(dim=-1)
    return torch.where(e == 0, torch.zeros_like(e), e / m.clamp_min(1e-300))


ATTN_WHOLE_TOL = {"out": 6e-3, "dq": 1.5e-2, "dk": 1.5e-2, "dv": 1.5e-2}     # the suite's whole-tensor tolerances (test_attention_fwd_bwd)


def attention_measures(got, ref, H, rows_mask=None, tol=None):
    """got / ref: dicts as attention_eval returns (got: whatever subset was computed).  tol None -> {name: worst value}: out / dq / dk / dv
    per (row, head) over the magnitude row, out_rel per (row, head) over ||ref||, lse and delta as absolute errors.  With tol (as
    attention_tolerances returns) -> {name: worst value / tolerance}; delta's tolerance grows per row by 2^-8 sum |o dO|, because the
    kernels read the bf16 out.  rows_mask [rows] bool: the packed rows that count (gradients, lse, delta)."""
    res = {}
    for k in ("out", "dq", "dk", "dv"):
        if k in got:
            r = head_row_ratio(got[k], ref[k], ref[k + "_abs"], H)
            if rows_mask is not None and k != "out":
                r = r[rows_mask]
            res[k] = float(r.max())
    if "out" in got:
        res["out_rel"] = float(head_row_ratio(got["out"], ref["out"], ref["out"], H).max())
    for k in ("lse", "delta"):
        if k in got:
            e = (got[k].double() - ref[k].double()).abs()
            if k == "delta" and tol is not None:
                e = e / (tol["delta"] + U_BF16 * ref["delta_abs"].double())
            if rows_mask is not None:
                e = e[:, rows_mask]
            res[k] = float(e.max())
    if tol is not None:
        res = {k: (v if k == "delta" else v / tol[k]) for k, v in res.items()}
    return res


def attention_tolerances(emu):
    """3 x the emulation's worst row on the same inputs (the project's usual margin: accumulation order, fast exp2), never above the suite's
    whole-tensor tolerance of that quantity; lse / delta: 3 x the emulation's worst absolute error"""
    tol = {k: min(3.0 * emu[k], ATTN_WHOLE_TOL[k]) for k in ("out", "dq", "dk", "dv") if k in emu}
    if "out_rel" in emu:
        tol["out_rel"] = min(3.0 * emu["out_rel"], ATTN_WHOLE_TOL["out"])
    for k in ("lse", "delta"):
        if k in emu:
            tol[k] = 3.0 * max(emu[k], U_F32)                       # (never below one fp32 rounding of a value of size 1)
    return tol


def attention_measures_full(got, ref, H, lens, rows_mask=None, tol=None):
    """attention_measures for inputs whose softmax is peaked or shifted: dq / dk / dv per (row, head) as
        ||got - ref|| / max(||full||, 2^-20 max over the rows of the same (sequence, head) of ||full||)
    with the *_full magnitude rows of attention_eval.  The floor is a condition, not a measurement: a key that receives P = 1e-60 has a true gradient
    of that size, any fp32 evaluation returns 0 for it, and against its own magnitude that is a ratio of 1; under the floor the unit is still
    compared - absolutely, against a quantity a million times below the largest gradient row of its own sequence and head.  out, out_rel, lse and delta
    are measured as attention_measures measures them.  A value that is not finite counts as infinite."""
    res = attention_measures({k: v for k, v in got.items() if k in ("out", "lse", "delta")}, ref, H, rows_mask, tol)
    for k in ("dq", "dk", "dv"):
        if k not in got:
            continue
        rows, D = ref[k].shape
        e = (got[k].double() - ref[k].double()).reshape(rows, H, D // H).norm(dim=-1)
        m = ref[k + "_full"].double().reshape(rows, H, D // H).norm(dim=-1)
        floor = torch.zeros_like(m)
        r0 = 0
        for L in lens:
            floor[r0:r0 + L] = m[r0:r0 + L].max(dim=0, keepdim=True).values * 2.0 ** -20
            r0 += L
        r = torch.where(e == 0, torch.zeros_like(e), e / torch.maximum(m, floor).clamp_min(1e-300))
        r = torch.nan_to_num(r, nan=float("inf"))
        if rows_mask is not None:
            r = r[rows_mask]
        res[k] = float(r.max()) / (tol[k] if tol is not None else 1.0)
    return {k: (v if v == v else float("inf")) for k, v in res.items()}


def attention_tolerances_full(emu, ref):
    """attention_tolerances for the full measure: 3 x the emulation's worst value on the same inputs, never above the suite's whole-tensor tolerance;
    lse never below 4 x 2^-24 max |lse| of the case - the rounding of the reference point, of the sum and of the product by ln 2, each at the
    magnitude of lse (the offset profiles: |lse| ~ 250)"""
    tol = attention_tolerances(emu)
    if "lse" in tol:
        tol["lse"] = max(tol["lse"], 4.0 * U_F32 * float(ref["lse"].abs().max()))
    return tol


def attention_forward_lazy(qkv, lens, H, tile=64, lazy_sum=2.0 ** 40, mutant=None):
    """The forward kernels' walk over the key tiles (csrc/attention.hip attn_fwd_kernel / attn_fwd_ring_kernel), restated in torch fp32: the scores
    of a tile start at -m_run; the first tile fixes the reference point m_run at its row maximum; a later tile whose row sum of p = exp2(s - m_run)
    is not below lazy_sum moves it - scores recomputed, tail keys masked AGAIN, d = max(new row maximum, 0), the sum and the accumulated P.V scaled by
    exp2(-d) (which underflows to 0 for d > 149) - for all 32 rows of the wave together; P is rounded to bf16 before P.V; keys beyond L are copies of
    key L - 1 (tile_load clamps the row) and masked to -inf; lse = (m_run + log2 l) ln 2.  (The kernels test the sum of each half of a row's 64
    keys, this the whole row's: a factor of two in a threshold of 2^40.)
    mutant: "no_o_rescale" - the move scales the sum but not the accumulated P.V; "no_remask" - the move leaves the tail keys unmasked;
    "lse_first_ref" - lse is saved from the first tile's reference point.
    -> (out [rows, D] fp32 holding bf16 values, lse [H, rows], moves [H, rows]: how often the row's reference point moved)"""
    D = qkv.shape[1] // 3
    rows = sum(lens)
    f = torch.float32
    out, lse, moves = torch.zeros(rows, D, dtype=f), torch.zeros(H, rows, dtype=f), torch.zeros(H, rows, dtype=torch.int64)
    r0 = 0
    for L in lens:
        x = qkv[r0:r0 + L].to(f)
        q, k, v = _heads(x[:, :D], H), _heads(x[:, D:2 * D], H), _heads(x[:, 2 * D:], H)
        m_run, m_first, l_run = torch.zeros(H, L), torch.zeros(H, L), torch.zeros(H, L)
        o = torch.zeros_like(q)
        nmove = torch.zeros(H, L, dtype=torch.int64)
        wave = torch.arange(L) // 32
        for k0 in range(0, L, tile):
            idx = torch.arange(k0, k0 + tile).clamp_max(L - 1)
            dead = torch.arange(k0, k0 + tile) >= L
            kt, vt = k[:, idx], v[:, idx]
            raw = q @ kt.transpose(1, 2)
            s = (raw - m_run.unsqueeze(-1)).masked_fill(dead, float("-inf"))
            if k0 == 0:
                m_run = s.max(dim=-1).values
                m_first = m_run.clone()
                s = s - m_run.unsqueeze(-1)
            p = torch.exp2(s)
            psum = p.sum(-1)
            if k0 != 0:
                trig = ~(psum < lazy_sum)
                hit = torch.zeros(H, int(wave.max()) + 1, dtype=torch.bool).index_put_((torch.arange(H)[:, None].expand(H, L), wave.expand(H, L)), trig, accumulate=True)
                trig = hit[:, wave]                                 # wave-uniform: the 32 rows of a wave move together
                if bool(trig.any()):
                    s2 = raw - m_run.unsqueeze(-1)
                    if mutant != "no_remask":
                        s2 = s2.masked_fill(dead, float("-inf"))
                    d = s2.max(dim=-1).values.clamp_min(0.0) * trig
                    alpha = torch.exp2(-d)
                    l_run = l_run * alpha
                    if mutant != "no_o_rescale":
                        o = o * alpha.unsqueeze(-1)
                    m_run = m_run + d
                    nmove += (d > 0).long()
                    s2 = s2 - d.unsqueeze(-1)
                    s = torch.where(trig.unsqueeze(-1), s2, s)
                    p = torch.exp2(s)
                    psum = p.sum(-1)
            l_run = l_run + psum
            o = o + bf16_round(p) @ vt
        out[r0:r0 + L] = _rows(bf16_round(o / l_run.unsqueeze(-1)))
        lse[:, r0:r0 + L] = ((m_first if mutant == "lse_first_ref" else m_run) + torch.log2(l_run)) * LN2
        moves[:, r0:r0 + L] = nmove
        r0 += L
    return out, lse, moves


# ---------------------------------------------------------------------------------------------------
# LayerNorm with a per-row choice between two affine sets
def _affine(rows_mod, p0, p1, dt):
    if rows_mod is None or p1 is None:
        return p0.to(dt).unsqueeze(0)
    return torch.where(rows_mod.bool().unsqueeze(1), p1.to(dt), p0.to(dt))


def layernorm_eval(x, g0, b0, eps, mod=None, g1=None, b1=None, emulate=False, one_pass=False):
    """mean, rstd, y of every row: fp64, or (emulate) an fp32 two-pass evaluation - centre, then square, as the kernel does.  one_pass: the
    variance as E[x^2] - mean^2 in fp32 (the mutant of the CPU tests)"""
    dt = torch.float32 if emulate else F64
    xd = x.to(dt)
    mean = xd.mean(1)
    if one_pass:
        var = (xd * xd).mean(1) - mean * mean
    else:
        xc = xd - mean.unsqueeze(1)
        var = (xc * xc).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xd - mean.unsqueeze(1)) * rstd.unsqueeze(1) * _affine(mod, g0, g1, dt) + _affine(mod, b0, b1, dt)
    return {"mean": mean, "rstd": rstd, "y": y}


def layernorm_y_given_stats(x, mean, rstd, g0, b0, mod=None, g1=None, b1=None):
    """fp64 y of the rows for GIVEN statistics: with the mean a kernel stored, what is left of its y error is everything but that mean's
    rounding (which has a bound of its own) - on rows with a large offset the only way to resolve the rest"""
    return (x.double() - mean.double().unsqueeze(1)) * rstd.double().unsqueeze(1) * _affine(mod, g0, g1, F64) + _affine(mod, b0, b1, F64)


def layernorm_mean_bound(x):
    """|mean^ - mean| <= (D + 1) 2^-24 mean |x|: an fp32 sum of D values in any order, one multiplication"""
    return (x.shape[1] + 1) * U_F32 * x.double().abs().mean(1)


def layernorm_bwd_eval(dy, x, mean, rstd, g0, dres=None, mod=None, g1=None, emulate=False):
    """dx = dres + rstd (gy - mean(gy) - xh mean(gy xh)), gy = dy gamma, xh = (x - mean) rstd (tests/test_kernels_gpu.py, the DMA-kernel test), with
    the magnitude form |dres| + rstd (|gy| + mean |gy| + |xh| mean |gy xh|); per-row terms of the parameter gradients: dg = sum dy xh, db = sum dy
    over the rows of each affine set.  mean / rstd are the kernel's INPUTS (fp32).  emulate: fp32."""
    dt = torch.float32 if emulate else F64
    xh = (x.to(dt) - mean.to(dt).unsqueeze(1)) * rstd.to(dt).unsqueeze(1)
    gy = dy.to(dt) * _affine(mod, g0, g1, dt)
    rs = rstd.to(dt).unsqueeze(1)
    dx = rs * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    mag = rs.abs() * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
    if dres is not None:
        dx, mag = dx + dres.to(dt), mag + dres.to(dt).abs()
    return {"dx": dx, "dx_abs": mag, "dy_xh": dy.to(dt) * xh, "dy": dy.to(dt)}


def mag_row_ratio(got, ref, mag):
    """per row: ||got - ref|| / ||mag||"""
    e = (got.double() - ref.double()).norm(dim=-1)
    return torch.where(e == 0, torch.zeros_like(e), e / mag.double().norm(dim=-1).clamp_min(1e-300))


def rowsum_bound(terms, rows_sel, c0, extra=8, mag=None):
    """fp32 sum over the selected rows of per-row terms, added to c0, in any order: reference and bound
    2^-24 |ref| + (rows + extra) 2^-24 (sum |terms| + |c0|) - the GEMM bound over the row sum.  extra: the fp32 roundings a term carries
    itself; mag: the terms' magnitude rows where a term is a difference (the column sum of dx)"""
    sel = rows_sel.double().unsqueeze(1)
    n = int(rows_sel.sum())
    ref = (terms.double() * sel).sum(0) + c0.double()
    tot = ((mag if mag is not None else terms).double().abs() * sel).sum(0) + c0.double().abs()
    return ref, U_F32 * ref.abs() + (n + extra) * U_F32 * tot * (1 + U_F32)


# ---------------------------------------------------------------------------------------------------
# the inputs of the case lists (CPU tensors from a seed: the CPU proofs and the GPU tests see the same numbers)
ATTN_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
NT_M, NT_N, NT_K = (1, 63, 64, 65, 129, 257, 300), (128, 384, 512), (64, 192, 256, 320)
TN_M, TN_N = (1, 63, 64, 65, 129, 513), ((128, 256), (256, 256), (256, 512))
LN_D, LN_D_HEAD, LN_ROWS = (512, 768, 1024, 1280), (1536, 2048, 2560), (1, 7, 8, 9, 17, 33)
LN_KINDS = ("usual", "offset", "const")
LN_CONST = 0.75               # every partial sum of such a row is exact in fp32, so its mean is, in whatever order it is summed: with a constant that is
                              # not (0.7), rstd = eps^-1/2 = 316 turns the last bit of the mean into 4e-4 of the row in ANY fp32 evaluation


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def gemm_nt_case(M, N, K, seed=0):
    """operands of every nt epilogue at one shape: A, two weight sets, biases, residuals (full and row-gathered), gelu' operands (bf16 values
    and 8-bit codes), non-zero column-sum vectors"""
    g = _gen(M, N, K, seed)
    bf = torch.bfloat16
    c = {"A": torch.randn(M, K, generator=g).to(bf), "B": (torch.randn(N, K, generator=g) * 0.05).to(bf), "B2": (torch.randn(N, K, generator=g) * 0.05).to(bf),
         "bias": torch.randn(N, generator=g), "bias2": torch.randn(N, generator=g) + 0.5, "res": torch.randn(M, N, generator=g),
         "res_pool": torch.randn(50, N, generator=g), "res_idx": torch.randint(0, 50, (M,), generator=g, dtype=torch.int32),
         "aux": gelu_grad64(torch.randn(M, N, generator=g).double() * 1.5).to(bf), "aux8": torch.randint(0, 256, (M, N), generator=g, dtype=torch.uint8),
         "colsum0": torch.randn(N, generator=g) * 3.0, "colsum0_2": torch.randn(N, generator=g) * 3.0 - 1.0}
    return c


def gemm_tn_case(M, N1, N2, seed=0):
    """A [Mp, N1], B [Mp, N2] zero from row M to the next multiple of 64, and a non-zero C to accumulate onto"""
    g = _gen(M, N1, N2, seed, 7)
    Mp = (M + 63) // 64 * 64
    A, B = torch.zeros(Mp, N1, dtype=torch.bfloat16), torch.zeros(Mp, N2, dtype=torch.bfloat16)
    A[:M] = torch.randn(M, N1, generator=g).to(torch.bfloat16)
    B[:M] = torch.randn(M, N2, generator=g).to(torch.bfloat16)
    return {"A": A, "B": B, "C0": torch.randn(N1, N2, generator=g) * 2.0}


# score profiles of attn_case: what a trained model's softmax looks like and N(0, 1) draws do not (a spread of ~12 log2 units, a largest
# probability of ~0.05).  Each acts on the unscaled q / k of every (sequence, head); u is a unit vector of that (sequence, head), j the key's
# position in its sequence, offsets are in natural-log score units (q . k hd^-0.5).
#   sharp            q *= 6: the mean largest P is ~0.68
#   late_spike       keys floor(2 L / 3) and L - 3 (L - 1 when L < 3) times 8, every 7th query row times 6: scores ~70 log2 units above the rest, late
#   staircase        q += 4 sqrt(hd) u, k_j += 11.7 floor(j / 64) u: every 64-key tile ~47 nat (68 log2 units) above the one before it
#   offset_pos/_neg  q += 6 sqrt(hd) u, k += +-35 u: every score ~ +-210 nat (303 log2 units), |lse| ~ 210 ... 250
#   ties             every key of a (sequence, head) equals key 0: P is exactly uniform
#   first_tile_high  q += 4 sqrt(hd) u, k_j -= 60 u from key 64 on: everything behind the first tile underflows to p = 0
ATTN_PROFILES = ("sharp", "late_spike", "staircase", "offset_pos", "offset_neg", "ties", "first_tile_high")


def _apply_profile(x, profile, H, hd, lens, g):
    """the profile's change of the unscaled q (columns [0, D)) and k (columns [D, 2 D)) of x, in place; draws come after those of attn_case"""
    D = H * hd
    u = torch.randn(len(lens), H, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    r0 = 0
    for i, L in enumerate(lens):
        q = x[r0:r0 + L, :D].view(L, H, hd)
        k = x[r0:r0 + L, D:2 * D].view(L, H, hd)
        j = torch.arange(L)
        if profile == "sharp":
            q *= 6.0
        elif profile == "late_spike":
            for kj in ((2 * L) // 3, L - 3 if L >= 3 else L - 1):
                k[kj] *= 8.0
            q[::7] *= 6.0
        elif profile == "staircase":
            q += 4.0 * math.sqrt(hd) * u[i]
            k += 11.7 * (j // 64).float()[:, None, None] * u[i]
        elif profile in ("offset_pos", "offset_neg"):
            q += 6.0 * math.sqrt(hd) * u[i]
            k += (35.0 if profile == "offset_pos" else -35.0) * u[i]
        elif profile == "ties":
            k[:] = k[0].clone()
        elif profile == "first_tile_high":
            q += 4.0 * math.sqrt(hd) * u[i]
            k -= 60.0 * (j >= 64).float()[:, None, None] * u[i]
        else:
            raise ValueError(profile)
        r0 += L


def attn_case(H, hd, lens, lq=0, seed=0, profile=None, scaled=True):
    """packed qkv (bf16, q columns pre-multiplied by hd^-0.5 log2 e as the qkv GEMM's epilogue leaves them) and dO (compact when lq).
    profile: one of ATTN_PROFILES applied to the same N(0, 1) draws before the scaling and the rounding (None / "randn": the draws as they
    are).  scaled=False: qkv stays fp32 with q unscaled (the exact-fp32 forward's operand)."""
    g = _gen(H, hd, len(lens), sum(lens), lq, seed)
    D, rows = H * hd, sum(lens)
    x = torch.randn(rows, 3 * D, generator=g)
    nq = sum(min(lq, L) if lq else L for L in lens)
    dout = torch.randn(nq, D, generator=g).to(torch.bfloat16)
    if profile not in (None, "randn"):
        _apply_profile(x, profile, H, hd, lens, g)
    if not scaled:
        return {"qkv": x, "dout": dout}
    x[:, :D] *= attn_q_scale(hd)
    return {"qkv": x.to(torch.bfloat16), "dout": dout}


def ln_case(D, kind, rows=33, seed=0):
    """rows of one of the three input kinds - the usual randn * 2 + 0.3, an offset 50 + 0.5 randn (a variance taken as E[x^2] - mean^2 loses
    it), the usual with a CONSTANT first row (rstd = eps^-1/2) - two affine sets, a per-row modality, an output permutation, and the backward's
    operands.  The row counts of the case list are prefixes of these rows."""
    g = _gen(D, LN_KINDS.index(kind), rows, seed)
    x = 50.0 + 0.5 * torch.randn(rows, D, generator=g) if kind == "offset" else torch.randn(rows, D, generator=g) * 2 + 0.3
    if kind == "const":
        x[0] = LN_CONST
    c = {"x": x.contiguous(), "g": [torch.randn(D, generator=g) * 0.1 + 1 for _ in range(2)], "b": [torch.randn(D, generator=g) * 0.1 for _ in range(2)],
         "mod": (torch.rand(rows, generator=g) > 0.5).to(torch.uint8), "dy": torch.randn(rows, D, generator=g).to(torch.bfloat16),
         "dres": torch.randn(rows, D, generator=g)}
    c["mod"][0] = 1
    if rows > 1:
        c["mod"][1] = 0
    return c
