"""Shared restatements and bounds of the exact-fp32 forward (csrc/exact.hip, engine_exact.py) for tests/test_exact_cpu.py and
tests/test_exact_gpu.py.  Pure torch; the references are fp64 on the CPU.

Bounds (u = 2^-24), each derived from the arithmetic the kernels promise, none from what they measure:
  GEMM, act 0   rowwise.gemm_bound(ref, S, K, u): K fused multiply-adds with one rounding each, three epilogue operations (+bias, +res,
                *alpha), the output rounding; S = |alpha| (|A| |B|^T + |bias| + |res|).  It holds for a sum of the K products in ANY order
                (the kernel's: chains of 32, their sums added in order - no term meets more than 32 + K / 32 roundings).
  GEMM, act 1   1.13 (pre-activation bound) + C_ERF u |x| / 2 + u |gelu(x)|: the Lipschitz constant of GELU, erff's documented error
                (C_ERF ulp of a value of size <= 1, times the x / 2 it is multiplied by), the rounding of the result.
  attention     per (row i, head): ||err|| <= (2 hd A_i + 2 L + 16) u ||P |v|||, A_i = hd^-0.5 max_j sum_d |q_id k_jd|: hd roundings in every
                score, whose error enters p_j relatively and twice (numerator and normaliser), L-term sums for the normaliser and for P.V.
  logits        EXACT_LOGIT_ABS against the reference's golden logits: 3 x the worst error measured on the six golden cases on the device
                (the project's margin for accumulation order), and never above EXACT_LOGIT_CAP = 1.2e-5 - a third of the 3.58e-5 that the
                smallest logic error of the table in test_exact_cpu.py (block LayerNorm eps 1e-5 -> 1e-6) causes.
"""
import json
import math
import os

import torch

from tests import rowwise

U = rowwise.U_F32
C_ERF = 16.0                    # ulp bound of erf in the OpenCL numerical-compliance table, which the device library's erff follows
EXACT_LOGIT_CAP = 1.2e-5
EXACT_LOGIT_ABS = 4.3e-6        # 3 x 1.431e-6, the worst of the six golden cases (ft_mm_eval; profiles/r18/exact_margins.json: logits_golden_worst)
assert EXACT_LOGIT_ABS <= EXACT_LOGIT_CAP
BF16_LOGIT_ABS, BF16_LOGIT_COS = 0.03, 0.9999        # the bf16 path's bound: tests/test_ft_gpu.py:19 (LOGIT_ABS, LOGIT_COS)
TOKEN_L2_REL, TOKEN_RTOL, TOKEN_ATOL = 1e-5, 1e-4, 1e-4   # tests/test_ft_oracle_golden.py:31-33

F64 = torch.float64

_margins = {}


def record(name, value):
    """keep the worst measured value of `name`; with AVSIAM_EXACT_MARGINS=<file> (tools/exact_margins.py) the table is rewritten there"""
    value = float(value)
    _margins[name] = max(_margins.get(name, 0.0), value)
    path = os.environ.get("AVSIAM_EXACT_MARGINS")
    if path:
        with open(path, "w") as f:
            json.dump(_margins, f, indent=1, sort_keys=True)
    return value


# ---------------------------------------------------------------------------------------------------
# GEMM
GEMM_SHAPES = [(1, 10, 32), (33, 527, 768), (129, 768, 256), (37, 768, 3072), (130, 2304, 768)]
GEMM_EPILOGUES = ("bias", "bias_res", "bias_gather_alpha2", "gelu")


def gemm_case(M, N, K, seed=0):
    g = rowwise._gen(M, N, K, seed, 18)
    return {"A": torch.randn(M, K, generator=g), "B": torch.randn(N, K, generator=g) * 0.05, "bias": torch.randn(N, generator=g),
            "res": torch.randn(M, N, generator=g), "res_pool": torch.randn(50, N, generator=g),
            "res_idx": torch.randint(0, 50, (M,), generator=g, dtype=torch.int32)}


def gemm_args(c, epilogue):
    """-> keyword operands (CPU tensors) of one epilogue: bias, res, res_idx, alpha, act"""
    kw = {"bias": c["bias"], "res": None, "res_idx": None, "alpha": 1.0, "act": 0}
    if epilogue == "bias_res":
        kw["res"] = c["res"]
    elif epilogue == "bias_gather_alpha2":
        kw.update(res=c["res_pool"], res_idx=c["res_idx"], alpha=2.0)
    elif epilogue == "gelu":
        kw["act"] = 1
    return kw


def gemm_reference(A, B, bias=None, res=None, res_idx=None, alpha=1.0, act=0):
    """-> (ref fp64, bound fp64) of out = act(alpha (A B^T + bias + res[res_idx])) on the fp32 operands"""
    K = A.shape[1]
    x, S = rowwise.gemm_nt_terms(A, B, bias=bias, res=res, res_idx=res_idx, alpha=alpha)
    bound = rowwise.gemm_bound(x, S, K, U)
    if act:
        g = rowwise.gelu64(x)
        return g, 1.13 * bound + C_ERF * U * x.abs() / 2 + U * g.abs()
    return x, bound


def gemm_emulate(A, B, bias=None, res=None, res_idx=None, alpha=1.0, act=0, kcut=0):
    """a torch fp32 evaluation on the CPU (another summation order than the kernel's; kcut: the contraction stops kcut terms early)"""
    K = A.shape[1] - kcut
    x = A[:, :K].float() @ B[:, :K].float().t()
    if bias is not None:
        x = x + bias.float()
    if res is not None:
        x = x + (res.float()[res_idx.long()] if res_idx is not None else res.float()[:A.shape[0]])
    x = x * torch.tensor(alpha, dtype=torch.float32)
    if act:
        x = 0.5 * x * (1.0 + torch.erf(x * torch.tensor(math.sqrt(0.5), dtype=torch.float32)))
    return x


def erff_ulp_estimate(got, x):
    """worst |got - gelu(x)| in units of (|x| / 2) ulp(erf(x / sqrt 2)) over |x| >= 0.5, for an EXACT pre-activation x: an upper estimate
    of erff's error in ulp (it still holds the epilogue's own two roundings)"""
    xd = x.double()
    e = torch.erf(xd / math.sqrt(2.0)).abs()
    ulp = torch.exp2(torch.floor(torch.log2(e.clamp_min(1e-30))) - 23)
    sel = xd.abs() >= 0.5
    r = (got.double() - rowwise.gelu64(xd)).abs() / (xd.abs() / 2 * ulp)
    return float(r[sel].max()) if bool(sel.any()) else 0.0


# ---------------------------------------------------------------------------------------------------
# attention over packed fp32 qkv [rows, 3 D], q unscaled
ATTN_MIXES = [[1], [5, 64, 65], [196, 512], [708]]


def attn_case(H, hd, lens, seed=0):
    g = rowwise._gen(H, hd, len(lens), sum(lens), seed, 18)
    return torch.randn(sum(lens), 3 * H * hd, generator=g)


def _split(x, H):
    L, D = x.shape
    return x.reshape(L, H, D // H).permute(1, 0, 2)


def _join(x):
    H, L, hd = x.shape
    return x.permute(1, 0, 2).reshape(L, H * hd)


def attn_eval(qkv, lens, H, dt=F64, scale=None):
    """softmax(scale q k^T) v of every sequence in dtype `dt` (fp64: the reference; fp32: an emulation in torch's order).
    -> (out [rows, D], mag [rows, D] = P |v|, A [rows, H] = scale max_j sum_d |q_id k_jd|, Lrow [rows] = the row's sequence length)"""
    D = qkv.shape[1] // 3
    hd = D // H
    sc = hd ** -0.5 if scale is None else scale
    rows = sum(lens)
    out, mag = torch.zeros(rows, D, dtype=dt), torch.zeros(rows, D, dtype=dt)
    A, Lrow = torch.zeros(rows, H, dtype=dt), torch.zeros(rows, dtype=dt)
    r0 = 0
    for L in lens:
        x = qkv[r0:r0 + L].to(dt)
        q, k, v = _split(x[:, :D], H), _split(x[:, D:2 * D], H), _split(x[:, 2 * D:], H)
        s = (q @ k.transpose(1, 2)) * torch.tensor(sc, dtype=dt)
        P = torch.softmax(s, dim=-1)
        out[r0:r0 + L] = _join(P @ v)
        mag[r0:r0 + L] = _join(P @ v.abs())
        A[r0:r0 + L] = ((q.abs() @ k.abs().transpose(1, 2)).max(dim=-1).values * sc).t()
        Lrow[r0:r0 + L] = L
        r0 += L
    return out, mag, A, Lrow


def attn_ratio(got, ref, mag, A, Lrow, H):
    """per (row, head): ||got - ref|| / ((2 hd A + 2 L + 16) u ||P |v|||) -> [rows, H]"""
    rows, D = ref.shape
    hd = D // H
    e = (got.double() - ref.double()).reshape(rows, H, hd).norm(dim=-1)
    m = mag.double().reshape(rows, H, hd).norm(dim=-1)
    bound = (2 * hd * A.double() + 2 * Lrow.double().unsqueeze(1) + 16) * U * m
    return torch.where(e == 0, torch.zeros_like(e), e / bound.clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------
# logits
def logit_check(got, ref):
    """-> (max |error|, min row cosine) of logits against the reference's, shapes asserted equal"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    g, r = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float((g - r).abs().max()), float(torch.nn.functional.cosine_similarity(g, r, dim=1).min())
