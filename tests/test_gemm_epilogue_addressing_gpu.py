"""Addressing of the nt GEMM epilogue (csrc/gemm.hip: nt_epilogue, epi_load_res, epi_load_aux).

Every stream of the epilogue is addressed as a wave-uniform buffer descriptor + one 32-bit lane offset, and the hardware range check of
the descriptor stands for the row clamps and row masks.  What can go wrong is therefore a wrong base, a wrong leading dimension, a wrong
extent (a row at or behind M written, a row in front of M dropped) - so the cases are the smallest shapes with a partial last row block
(M = 17, 255, 257, 481), a tile with one valid row (M = 1, 257), the 224-row tile class and two row tiles (M = 257, 481), every output
with a leading dimension larger than N and a pointer into a larger, sentinel-filled allocation (a block of rows in front, 256 rows behind
row M: both must stay untouched), and the operands the epilogue reads (residual, gelu') allocated with exactly M rows.  Every kernel
family runs every epilogue form; references are fp32 products of the same bf16 inputs, tolerances those of test_kernels_gpu.py.

K = 128 everywhere but in the ring family: gemm_nt_ring_kernel is chosen from K = 256 on.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
MS = (1, 17, 255, 257, 481)
NS = (256, 512)
FRONT, BEHIND = 5, 256                      # sentinel rows in front of row 0 and behind row M of every output
SENTINEL = 0xA5
SPLIT = 256                                 # the dual form's m_split

# knobs that force each kernel family (csrc/gemm.hip nt_plan), its K, and the instantiation avs_gemm_nt_launch_plan must name for every case
K_TWOBUF128, K_TWOBUF128_HALF, K_RING, K_RING_HALF, K_TWOBUF256, K_NT8_ONE, K_NT8_TWO = range(7)
FAMILIES = {
    "nt8_two_heights": (dict(nt_big_min=1, nt_tile_h=0), 128, K_NT8_TWO),      # gemm_nt8_kernel<., 0, 4, 3>: at these row counts every tile is 224 rows high
    "nt8_256": (dict(nt_big_min=1, nt_tile_h=256), 128, K_NT8_ONE),            # gemm_nt8_kernel<., 0, 4, 4>
    "tile256": (dict(gemm_tile=256), 128, K_TWOBUF256),                        # gemm_nt_kernel<., 4, 8>
    "tile128": (dict(gemm_tile=128, gemm_ring=0), 128, K_TWOBUF128),           # gemm_nt_kernel<., 2, 4>
    "tile128_half": (dict(gemm_tile=128, gemm_ring=2), 128, K_TWOBUF128_HALF),  # ... its half-height tiles
    "ring": (dict(gemm_tile=128, gemm_ring=1), 256, K_RING),                   # gemm_nt_ring_kernel<., 4>
    "ring_half": (dict(gemm_tile=128, gemm_ring=2), 256, K_RING_HALF),         # gemm_nt_ring_kernel<., 2>
}
FORMS = ("bf16", "f32", "f32_res", "f32_gather", "scale_cols", "gelu", "gelu_codes", "gelu_bwd", "gelu_bwd_codes", "colsum", "dual")


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


class Guarded:
    """an output of M x N elements with leading dimension ld > N, FRONT rows into an allocation filled with sentinel bytes"""

    def __init__(self, M, N, ld, dtype):
        self.M, self.N, self.ld = M, N, ld
        self.buf = torch.empty(FRONT + M + BEHIND, ld, device=DEV, dtype=dtype)
        self.buf.view(U8).fill_(SENTINEL)
        self.ptr = self.buf.data_ptr() + FRONT * ld * self.buf.element_size()

    def rows(self):
        return self.buf[FRONT:FRONT + self.M, :self.N]

    def assert_guards_untouched(self, what):
        raw = self.buf.view(U8).clone()
        raw[FRONT:FRONT + self.M, :self.N * self.buf.element_size()] = SENTINEL
        bad = (raw != SENTINEL).nonzero()
        assert bad.numel() == 0, f"{what}: bytes outside the {self.M} x {self.N} output were written, first at (row, byte) {bad[0].tolist()} (row 0 = {FRONT})"


_data = {}


def data(M, N, K):
    """inputs and fp32 / fp64 references of one shape, made once and shared by every family and form"""
    key = (M, N, K)
    if key in _data:
        return _data[key]
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * M + N + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    d = {}
    d["A"] = rn(M, K).to(BF16)
    d["W"], d["W2"] = (rn(N, K) * 0.05).to(BF16), (rn(N, K) * 0.05).to(BF16)
    d["bias"], d["bias2"] = rn(N), rn(N)
    d["ldr"] = N + 32
    d["res"] = rn(M, d["ldr"])                                   # exactly M rows
    d["table"] = rn(50, d["ldr"])
    idx = torch.randint(0, 50, (M,), device=DEV, generator=g, dtype=torch.int32)
    idx[: min(M, 4)] = torch.tensor([49, 3, 3, 0], device=DEV, dtype=torch.int32)[: min(M, 4)]      # out of order, repeated
    d["idx"] = idx
    ref = d["A"].float() @ d["W"].float().t()                    # the fp32 product of the same bf16 inputs
    ref2 = d["A"].float() @ d["W2"].float().t()
    d["ref"], d["ref2"] = ref.double(), ref2.double()
    p = (d["ref"] + d["bias"].double()).requires_grad_(True)
    F.gelu(p).sum().backward()
    d["gelu"], d["gelu_grad"] = F.gelu(p.detach()), p.grad
    d["ldaux"] = N + 64
    aux = torch.zeros(M, d["ldaux"], device=DEV, dtype=BF16)     # exactly M rows
    aux[:, :N] = p.grad.to(BF16)
    d["aux"] = aux
    aux8 = torch.zeros(M, d["ldaux"], device=DEV, dtype=U8)      # ldaux counts bytes
    aux8[:, :N] = ((p.grad + 0.1296875) * 202.0).round().clamp(0, 255).to(U8)
    d["aux8"] = aux8
    _data[key] = d
    return d


def gemm(d, M, N, K, out, out_kind, W="W", bias=None, res=None, ldr=0, res_idx=None, aux=None, ldaux=0, out2=None, alpha=1.0, act=0, scale_cols=0,
         col_scale=1.0, colsum=None, dual=None):
    """avs_gemm_nt_bf16 / _dual with explicit pointers and leading dimensions (ops.gemm_nt takes whole contiguous tensors only)"""
    from avsiam_amd import _lib
    args = (d["A"], K, d[W], K, M, N, K, bias, res, ldr, res_idx, aux, ldaux, out.ptr, out.ld, out_kind, out2.ptr if out2 is not None else None,
            out2.ld if out2 is not None else 0, float(alpha), act, scale_cols, float(col_scale), colsum)
    if dual is None:
        _lib.call("avs_gemm_nt_bf16", *args, _lib.current_stream())
    else:
        _lib.call("avs_gemm_nt_bf16_dual", *args, SPLIT, *dual, _lib.current_stream())


def run_form(form, M, N, K, with_colsum=True):
    """one launch of one epilogue form -> {name: tensor of the M x N output rows (or a column sum)}; the guards are checked here"""
    d = data(M, N, K)
    outs, colsums = {}, {}
    if form == "bf16":
        outs["out"] = Guarded(M, N, N + 64, BF16)
        gemm(d, M, N, K, outs["out"], 0, bias=d["bias"])
    elif form == "f32":
        outs["out"] = Guarded(M, N, N + 36, F32)
        gemm(d, M, N, K, outs["out"], 1, bias=d["bias"])
    elif form == "f32_res":
        outs["out"] = Guarded(M, N, N + 36, F32)
        gemm(d, M, N, K, outs["out"], 1, bias=d["bias"], res=d["res"], ldr=d["ldr"])
    elif form == "f32_gather":
        outs["out"] = Guarded(M, N, N + 36, F32)
        gemm(d, M, N, K, outs["out"], 1, bias=d["bias"], res=d["table"], ldr=d["ldr"], res_idx=d["idx"], alpha=2.0)
    elif form == "scale_cols":
        outs["out"] = Guarded(M, N, N + 36, F32)
        gemm(d, M, N, K, outs["out"], 1, bias=d["bias"], scale_cols=64, col_scale=0.25)
    elif form == "gelu":
        outs["out"], outs["out2"] = Guarded(M, N, N + 64, BF16), Guarded(M, N, N + 128, BF16)
        gemm(d, M, N, K, outs["out"], 0, bias=d["bias"], out2=outs["out2"], act=1)
    elif form == "gelu_codes":
        outs["out"], outs["out2"] = Guarded(M, N, N + 64, U8), Guarded(M, N, N + 128, BF16)
        gemm(d, M, N, K, outs["out"], 2, bias=d["bias"], out2=outs["out2"], act=1)
    elif form == "gelu_bwd":
        outs["out"] = Guarded(M, N, N + 64, BF16)
        gemm(d, M, N, K, outs["out"], 0, aux=d["aux"], ldaux=d["ldaux"], act=2)
    elif form == "gelu_bwd_codes":
        outs["out"] = Guarded(M, N, N + 64, BF16)
        gemm(d, M, N, K, outs["out"], 0, aux=d["aux8"], ldaux=d["ldaux"], act=3)
    elif form == "colsum":
        outs["out"] = Guarded(M, N, N + 64, BF16)
        colsums["colsum"] = torch.ones(N, device=DEV)
        gemm(d, M, N, K, outs["out"], 0, bias=d["bias"], colsum=colsums["colsum"])
    elif form == "dual":
        outs["out"] = Guarded(M, N, N + 64, BF16)
        if with_colsum:
            colsums["colsum"], colsums["colsum2"] = torch.ones(N, device=DEV), torch.ones(N, device=DEV)
        gemm(d, M, N, K, outs["out"], 0, bias=d["bias"], colsum=colsums.get("colsum"), dual=(d["W2"], d["bias2"], colsums.get("colsum2")))
    else:
        raise ValueError(form)
    for name, g in outs.items():
        g.assert_guards_untouched(f"{form} M={M} N={N} {name}")
    res = {name: g.rows() for name, g in outs.items()}
    res.update(colsums)
    return res


def check_form(form, M, N, K, got):
    d = data(M, N, K)
    pre = d["ref"] + d["bias"].double()
    tag = f"{form} M={M} N={N} K={K}"
    if form in ("bf16", "colsum"):
        assert rel_err(got["out"], pre) < 4e-3, tag
        if form == "colsum":
            assert rel_err(got["colsum"], 1 + pre.sum(0)) < 2e-3, tag
    elif form == "f32":
        assert rel_err(got["out"], pre) < 1e-5, tag
    elif form == "f32_res":
        assert rel_err(got["out"], pre + d["res"][:, :N].double()) < 1e-5, tag
    elif form == "f32_gather":
        assert rel_err(got["out"], 2 * (pre + d["table"][:, :N].double()[d["idx"].long()])) < 1e-5, tag
    elif form == "scale_cols":
        want = pre.clone()
        want[:, :64] *= 0.25
        assert rel_err(got["out"], want) < 1e-5, tag
    elif form == "gelu":
        assert rel_err(got["out"], d["gelu_grad"]) < 4e-3, tag
        assert float((got["out"].double() - d["gelu_grad"]).abs().max()) < 8e-3, tag
        assert rel_err(got["out2"], d["gelu"]) < 5e-3, tag
    elif form == "gelu_codes":
        dec = got["out"].double() / 202.0 - 0.1296875
        assert float((dec - d["gelu_grad"]).abs().max()) <= 0.5 / 202 + 4e-3, tag
        assert rel_err(got["out2"], d["gelu"]) < 5e-3, tag
    elif form == "gelu_bwd":
        assert rel_err(got["out"], d["ref"] * d["aux"][:, :N].double()) < 5e-3, tag
    elif form == "gelu_bwd_codes":
        assert rel_err(got["out"], d["ref"] * (d["aux8"][:, :N].double() / 202.0 - 0.1296875)) < 5e-3, tag
    elif form == "dual":
        want = pre.clone()
        want[SPLIT:] = (d["ref2"] + d["bias2"].double())[SPLIT:]
        assert rel_err(got["out"], want) < 4e-3, tag
        assert rel_err(got["out"][SPLIT:], want[SPLIT:]) < 4e-3, tag
        if "colsum" in got:
            assert rel_err(got["colsum"], 1 + want[:SPLIT].sum(0)) < 2e-3, tag
            assert rel_err(got["colsum2"], 1 + want[SPLIT:].sum(0)) < 2e-3, tag


def cases():
    for M in MS:
        for N in NS:
            for form in FORMS:
                if form == "dual" and M <= SPLIT:
                    continue
                yield form, M, N


class forced:
    """the tuning knobs of one kernel family, restored on exit"""

    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        from avsiam_amd import _lib
        self.old = {k: _lib.tuning_get(k) for k in self.knobs}
        for k, v in self.knobs.items():
            _lib.tuning_set(k, v)

    def __exit__(self, *exc):
        from avsiam_amd import _lib
        for k, v in self.old.items():
            _lib.tuning_set(k, v)


def test_rows_are_split_when_a_stream_exceeds_4_gib():
    """The epilogue's byte offsets are 32 bits wide, so the host cuts a call whose output extent (rows x leading dimension) reaches 4 GiB
    into two calls over halves of the rows.  600 rows with a leading dimension of 3.6 M bf16 values (4.3 GB, allocated but touched only
    where the GEMM writes): both halves - the second starts behind row 2^31 bytes / ld, uses the second weight set only and a moved
    m_split - must equal the same product written with an ordinary leading dimension, bit for bit."""
    from avsiam_amd import _lib
    M, N, K = 600, 256, 128
    d = data(M, N, K)
    small = torch.zeros(M, N, device=DEV, dtype=BF16)
    ld = ((1 << 32) // (M * 2) // 8 + 1) * 8
    assert M * ld * 2 >= 1 << 32 and 512 * ld * 2 < 1 << 32
    big = torch.empty(M * ld, device=DEV, dtype=BF16)
    rows = big.view(M, ld)[:, :N]
    rows.zero_()
    for out, ldo in ((small, N), (big, ld)):
        _lib.call("avs_gemm_nt_bf16_dual", d["A"], K, d["W"], K, M, N, K, d["bias"], None, 0, None, None, 0, out, ldo, 0, None, 0, 1.0, 0, 0, 1.0, None,
                  SPLIT, d["W2"], d["bias2"], None, _lib.current_stream())
    want = d["ref"] + d["bias"].double()
    want[SPLIT:] = (d["ref2"] + d["bias2"].double())[SPLIT:]
    assert rel_err(small, want) < 4e-3
    assert torch.equal(rows, small)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_epilogue_addressing(family):
    from avsiam_amd import _lib
    _lib.load()
    knobs, K, kernel = FAMILIES[family]
    plan = (ctypes.c_int * 8)()
    with forced(knobs):
        for form, M, N in cases():
            assert _lib.load().avs_gemm_nt_launch_plan(M, N, K, SPLIT if form == "dual" else 0, plan, 8) == 0
            # (two weight sets: the 256-row class must cover the first - at these row counts that leaves no 224-row tile, so the one-class kernel runs)
            assert plan[0] == (K_NT8_ONE if (family, form) == ("nt8_two_heights", "dual") else kernel), (family, form, M, N, list(plan))
            got = run_form(form, M, N, K)
            check_form(form, M, N, K, got)
