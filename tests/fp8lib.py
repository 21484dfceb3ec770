"""Exact references for the fp8 path: integer lattices on which the fp8 GEMMs are predictable bit for bit, and a per-element check of the
8-bit copies of producers that are not (GELU, LayerNorm, softmax).

Lattices.  Operand bytes whose de-quantised values are small integers (times a power-of-two scale), power-of-two de-quantisation
factors, integer biases / residuals / column-sum seeds and dyadic `aux`: every product and every partial sum of
    x = a_c ((dq A . B^T + bias) aux + res)
is then a small dyadic number, the same in ANY fp32 summation order, MFMA-internal alignment, split or atomic order.  The bf16 / fp32
outputs, the e5m2 bytes of `out8` (round to nearest even, saturating: torch.float8_*), the column sums and the recorded amax are
evaluated in fp64 on the CPU and compared with torch.equal on the bytes - there is no tolerance to derive.

8-bit copies of inexact producers.  A kernel rounds the same fp32 value v once to bf16 (b) and once, times the scale, to 8 bits (c).
v lies in b's rounding interval [lo, hi]; the fp32 product and the quantisation are monotone, so c lies in [q(lo s), q(hi s)] - for most
elements one code.  codes_within checks EVERY element this way and reports the share whose interval admits more than one code.

Pure torch (the knob context manager apart): tests/test_fp8_exact_cpu.py proves the lattices exact and the checks sharp on emulations,
tests/test_fp8_exact_gpu.py applies them to the kernels."""
import contextlib

import torch

from tests import rowwise as rw

E4M3, E5M2 = "e4m3", "e5m2"
FMT = {E4M3: (torch.float8_e4m3fn, 448.0), E5M2: (torch.float8_e5m2, 57344.0)}
U8, BF, F32, F64 = torch.uint8, torch.bfloat16, torch.float32, torch.float64
Q_STRIDE = 1024                                  # floats per device record (ops.Q_STRIDE): scale, 1 / scale, running amax, ...
KNOB_DEFAULTS = {"cu_reserve": 0, "det": 0}      # (csrc/api.cpp g_tuning)


@contextlib.contextmanager
def knobs(**kw):
    """set tuning knobs of the library for a block; the defaults are back afterwards whatever happens inside"""
    from avsiam_amd import _lib
    try:
        for k, v in kw.items():
            _lib.tuning_set(k, v)
        yield
    finally:
        for k in kw:
            _lib.tuning_set(k, KNOB_DEFAULTS[k])


# ---------------------------------------------------------------------------------------------------
# the 8-bit formats
def quant(x, scale, fmt, rne=True):
    """what the kernels' 8-bit epilogues compute: the fp32 product x * scale, clamped to the format's largest finite value, rounded to
    nearest even -> bytes.  rne=False: rounded towards zero instead (the mutant of the CPU tests)."""
    dt, fmax = FMT[fmt]
    v = (x.float() * rw.f32(scale)).clamp(-fmax, fmax)
    q = v.to(dt)
    b = q.view(U8)
    if not rne:
        b = b - (q.double().abs() > v.double().abs()).to(U8)       # the magnitude is the low 7 bits: one code towards zero
    return b


def decode(code, fmt):
    return code.contiguous().view(FMT[fmt][0]).double()


def record_rows(scales, amax=None, pow2=True):
    """contents of an ops.Fp8Records table: one record per scale, its inverse beside it, the running amax preloaded -> fp32 [n, Q_STRIDE].
    pow2: the scales of lattice operands, whose inverses the GEMMs multiply by, must be powers of two"""
    q = torch.zeros(len(scales), Q_STRIDE)
    for i, s in enumerate(scales):
        q[i, 0], q[i, 1] = s, 1.0 / s
        assert not pow2 or float(q[i, 0]) * float(q[i, 1]) == 1.0, "power-of-two scales only"
        q[i, 2] = 0.0 if amax is None else amax[i]
    return q


# ---------------------------------------------------------------------------------------------------
# lattices
def lattice_operand(vals, scale, fmt):
    """integer values times a power-of-two scale -> bytes; exact by construction, and said so"""
    b = quant(vals, scale, fmt)
    assert torch.equal(decode(b, fmt), vals.double() * scale), "not a lattice of this format"
    return b


BOOST = 64          # contraction columns that lift the last row (nt_lattice, last_row_max)


def nt_lattice(M, N, K, seed=0, a_fmt=E4M3, sa=4.0, sw=2.0, sw2=8.0, last_row_max=False, density=0.25, bias_step=1.0, bias_range=4):
    """Operands of every form of avs_gemm_nt_fp8 at one shape: A in {-2..2} (a share `density` of it non-zero), two weight sets in
    {-1, 0, 1}, biases in {-bias_range..bias_range} * bias_step, an fp32 residual in {-8..8}, a bf16 `aux` in {0, 1/4, 1/2, 3/4, 1} (3/4 makes
    the bf16 output round, ties included), integer column-sum seeds.
    last_row_max: the first BOOST contraction columns hold 1 in every weight row, 2 in A's last row and 0 in its other rows, which lifts
    row M - 1 by 2 * BOOST in every column: it then holds the column-wise and the global maximum of |x| (asserted on the CPU)."""
    g = rw._gen(M, N, K, seed, 8)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    a = ri(-2, 2, M, K) * (torch.rand(M, K, generator=g) < density)
    w, w2 = ri(-1, 1, N, K), ri(-1, 1, N, K)
    if last_row_max:
        w[:, :BOOST], w2[:, :BOOST], a[:, :BOOST] = 1.0, 1.0, 0.0
        a[M - 1, :BOOST] = 2.0
    aux = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])[torch.randint(0, 5, (M, N), generator=g)].to(BF)
    if last_row_max:
        aux[M - 1] = torch.where(aux[M - 1] < 0.75, torch.ones((), dtype=BF), aux[M - 1])      # 3/4 or 1: the row stays the largest
    return {"M": M, "N": N, "K": K, "a_fmt": a_fmt, "sa": sa, "sw": sw, "sw2": sw2,
            "A8": lattice_operand(a, sa, a_fmt), "W8": lattice_operand(w, sw, E4M3), "W8_2": lattice_operand(w2, sw2, E4M3),
            "bias": ri(-bias_range, bias_range, N) * bias_step, "bias2": ri(-bias_range, bias_range, N) * bias_step, "res": ri(-8, 8, M, N), "aux": aux,
            "colsum0": ri(-50, 50, N), "colsum0_2": ri(-50, 50, N)}


# the case list of the bytes-equal GEMM tests (the CPU proofs and the GPU tests see the same lattices)
NT_SHAPES = [(M, 512, 384) for M in (1, 17, 255, 256, 257, 513)] + [(257, 256, K) for K in (256, 384, 640)]
Q8_SCALE, Q8_SCALE_SAT = 16.0, 1024.0           # of the e5m2 copy: rounding with ties and no saturation / the one case meant to saturate
SAT_SHAPE = (257, 256, 256)
AMAX_ABOVE, AMAX_BELOW, AMAX_ABOVE_M = 1.0e4, 0.5, 255      # the record's amax before the call: above every |x| at M = 255, below elsewhere
# name -> (input-gradient form, what `out` is, nt_expected's options); scale_cols None: all N columns
NT_FORMS = {
    "fwd_bf16_cols0": (False, "bf16", dict(scale_cols=0, col_scale=0.125)),
    "fwd_bf16_cols64": (False, "bf16", dict(scale_cols=64, col_scale=0.125)),
    "fwd_bf16_cols192": (False, "bf16", dict(scale_cols=192, col_scale=0.125)),
    "fwd_bf16_colsN": (False, "bf16", dict(scale_cols=None, col_scale=0.125)),
    "fwd_f32_res": (False, "f32", dict(res=True)),
    "fwd_f32_res_records": (False, "f32", dict(res=True)),
    "dgrad_bf16": (True, "bf16", dict(bias=False, colsum=True)),
    "dgrad_bf16_out8": (True, "bf16", dict(bias=False, colsum=True, q8_scale=Q8_SCALE)),
    "dgrad_out8_only": (True, None, dict(bias=False, colsum=True, q8_scale=Q8_SCALE)),
    "dgrad_act2": (True, "bf16", dict(bias=False, aux=True, colsum=True, q8_scale=Q8_SCALE)),
    "dgrad_act2_out8_only": (True, None, dict(bias=False, aux=True, colsum=True, q8_scale=Q8_SCALE)),
}
_CASES = {}


def nt_case(M, N, K, grad, **kw):
    """the lattice of one shape (cached; nobody writes to it): e5m2 A for the input-gradient forms; row M - 1 is the largest at M = 17 / 257"""
    key = (M, N, K, grad, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = nt_lattice(M, N, K, a_fmt=E5M2 if grad else E4M3, last_row_max=M in (17, 257), **kw)
    return _CASES[key]


def nt_form_options(form, c):
    opt = dict(NT_FORMS[form][2])
    if "scale_cols" in opt and opt["scale_cols"] is None:
        opt["scale_cols"] = c["N"]
    if "q8_scale" in opt:
        opt["amax0"] = AMAX_ABOVE if c["M"] == AMAX_ABOVE_M else AMAX_BELOW
    return opt


# the GELU forms: the pre-activation x = (A . W^T) / 64 + bias, bias in {-64..64} / 64 - a fine dyadic grid over about +-9
GELU_SHAPES = [(257, 256, 256), (257, 256, 384), (513, 256, 256), (513, 256, 384)]
GELU_ALPHA = 2.0 ** -6


def gelu_case(M, N, K):
    return nt_case(M, N, K, False, density=1.0, bias_step=2.0 ** -6, bias_range=64)


def quarter_scale(amax, fmt):
    """the scale that puts the tensor's amax at a quarter of the format's largest finite value (what the suite's fp8 tests use)"""
    return rw.f32(0.25 * FMT[fmt][1] / float(amax))


def nt_expected(c, bias=True, res=False, aux=False, scale_cols=0, col_scale=1.0, m_split=0, colsum=False, q8_scale=None, amax0=0.0, alpha=None):
    """The exact outputs of avs_gemm_nt_fp8 on a lattice, by an fp64 evaluation of x = a_c ((dq A . B^T + bias) aux + res): dq = alpha
    (host) or 1 / (sa sw) (records), a_c = col_scale in columns [0, scale_cols) and 1 elsewhere (the fp8 kernel gives alpha to the product
    alone), rows from m_split meeting the second weight set (its dq, bias2, colsum2).
    -> x (fp64), bf16 / f32 (what a bf16 / fp32 `out` must hold), out8 (e5m2 bytes, with q8_scale), colsum / colsum2 (fp32, onto the
    lattice's seeds) and amax = max(amax0, max |x|)."""
    M, N = c["M"], c["N"]
    Ad = decode(c["A8"][:M], c["a_fmt"])

    def part(rows, W8, sw, b):
        dq = rw.f32(alpha) if alpha is not None else 1.0 / (c["sa"] * sw)
        x = (Ad[rows] @ decode(W8, E4M3).t()) * dq
        return x + b.double() if bias else x

    dual = 0 < m_split < M
    if dual:
        x = torch.cat([part(slice(0, m_split), c["W8"], c["sw"], c["bias"]), part(slice(m_split, M), c["W8_2"], c["sw2"], c["bias2"])])
    else:
        x = part(slice(0, M), c["W8"], c["sw"], c["bias"])
    if aux:
        x = x * c["aux"][:M].double()
    if res:
        x = x + c["res"][:M].double()
    ac = torch.ones(N, dtype=F64)
    ac[:scale_cols] = rw.f32(col_scale)
    x = x * ac
    assert torch.equal(x.float().double(), x), "not exact in fp32: not a lattice"
    e = {"x": x, "f32": x.float(), "bf16": x.float().to(BF), "amax": max(float(amax0), float(x.abs().max()))}
    if q8_scale is not None:
        e["out8"] = quant(x, q8_scale, E5M2)
    if colsum:
        top = m_split if dual else M
        e["colsum"] = (c["colsum0"].double() + x[:top].sum(0)).float()
        assert torch.equal(e["colsum"].double(), c["colsum0"].double() + x[:top].sum(0))
        if dual:
            e["colsum2"] = (c["colsum0_2"].double() + x[top:].sum(0)).float()
    return e


def mismatches(got, exp):
    """the outputs in `got` (tensors, or the float `amax`) that are not bitwise what `exp` holds under the same name -> [(name, how many, first)]"""
    bad = []
    for k, v in got.items():
        w = exp[k]
        if not torch.is_tensor(v):
            if float(v) != float(w):
                bad.append((k, float(v), float(w)))
            continue
        v = v.cpu()
        assert v.shape == w.shape and v.dtype == w.dtype, (k, v.shape, w.shape, v.dtype, w.dtype)
        if not rw.bitwise_equal(v, w):
            ne = torch.nonzero(v.float() != w.float())
            bad.append((k, int(ne.shape[0]), ne[0].tolist() if ne.shape[0] else "sign of zero / NaN bits"))
    return bad


def tn_lattice(M, N1, N2, sa, sb, seed=0, extra_rows=0):
    """Operands of avs_gemm_tn_fp8_group3: e5m2 A in {-2..2} * sa [M, N1], e4m3 B in {-1, 0, 1} * sb [M, N2], zero from row M to the next
    multiple of 64 (the contract), then `extra_rows` rows of non-zero lattice values nothing may read; an integer C to accumulate onto"""
    g = rw._gen(M, N1, N2, seed, 9)
    Mp = (M + 63) // 64 * 64
    a = torch.zeros(Mp + extra_rows, N1)
    b = torch.zeros(Mp + extra_rows, N2)
    a[:M] = torch.randint(-2, 3, (M, N1), generator=g).float()
    b[:M] = torch.randint(-1, 2, (M, N2), generator=g).float()
    if extra_rows:
        a[Mp:], b[Mp:] = 2.0, 1.0
    return {"M": M, "sa": sa, "sb": sb, "A8": lattice_operand(a, sa, E5M2), "B8": lattice_operand(b, sb, E4M3),
            "C0": torch.randint(-64, 65, (N1, N2), generator=g).float()}


TN_M = (1, 63, 64, 65, 129, 1000)
TN_SHAPES = [(256, 512), (512, 256), (256, 256)]                     # the three-problem group; the last one also runs alone
TN_SCALES = [(2.0 ** 10, 2.0 ** 4), (2.0 ** 3, 2.0 ** -2), (1.0, 2.0 ** 6)]

# the producers that are not exact on a lattice
LN_D, LN_ROWS, LN_HOST_D, LN_BWD_D, LN_BWD_ROWS = (512, 768, 1024, 1280, 1536), (1, 31, 33, 100), (768, 1280), (768, 1280), (1, 33, 130)
ATTN_HEADS, ATTN_LENS = [(2, 64), (3, 32), (2, 80)], [1, 39, 64, 65, 200]


def ln_case(D):
    """rows of rowwise.ln_case (the row counts of the tests are prefixes): two affine sets, rows of both kinds among the first eight"""
    return rw.ln_case(D, "usual", rows=130)


def tn_expected(c):
    """C_before + A^T . B / (sa sb) over the M token rows, exact in fp32 -> fp32 [N1, N2]"""
    M = c["M"]
    C = c["C0"].double() + (decode(c["A8"][:M], E5M2).t() @ decode(c["B8"][:M], E4M3)) / (c["sa"] * c["sb"])
    assert torch.equal(C.float().double(), C)
    return C.float()


# ---------------------------------------------------------------------------------------------------
# 8-bit copies beside a bf16 output
def bf16_interval(b):
    """the fp32 values that round to the bf16 value b (ties included on both sides) -> (lo, hi), fp32; the midpoints to b's neighbours are
    exact in fp32"""
    bits = b.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag, neg = bits & 0x7FFF, (bits & 0x8000) != 0
    val = lambda m: (m << 16).view(F32)
    up = (val(mag).double() + val(mag + 1).double()) / 2
    down = torch.where(mag > 0, (val(mag).double() + val((mag - 1).clamp_min(0)).double()) / 2, -up)
    lo, hi = torch.where(neg, -up, down), torch.where(neg, -down, up)
    return lo.float(), hi.float()


def codes_within(code8, bf16_out, scale, fmt):
    """every byte of the 8-bit copy lies between the codes of the two ends of its bf16 neighbour's rounding interval
    -> (flat indices of the violations, share of the elements whose interval admits more than one code)"""
    lo, hi = bf16_interval(bf16_out.cpu())
    qlo, qhi = decode(quant(lo, scale, fmt), fmt), decode(quant(hi, scale, fmt), fmt)
    v = decode(code8.cpu(), fmt)
    bad = torch.nonzero(~((qlo <= v) & (v <= qhi)).reshape(-1)).flatten()
    return bad, float((qlo != qhi).double().mean())


AMBIGUOUS_MAX = {E4M3: 0.10, E5M2: 0.05}        # 2^(3 - 7) = 6.3 % / 2^(2 - 7) = 3.1 % for values spread evenly over a binade


def amax_close(amax, bf16_out):
    """the recorded amax (of the fp32 values) against max |bf16 output|: within the bf16 unit roundoff"""
    m = float(bf16_out.float().abs().max())
    return abs(float(amax) - m) <= rw.U_BF16 * m
