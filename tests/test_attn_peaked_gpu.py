"""The attention kernels at peaked and shifted score distributions (rowwise.ATTN_PROFILES): every kernel form that tests/test_rowwise_gpu.py
measures on N(0, 1) inputs - the two-kernel forward + backward at both tile heights, register-staged and ring, the fused backward's length
classes, the compact-query form, the head-dim-80 instances - and the exact-fp32 forward, on inputs whose softmax is one-hot, exactly uniform,
shifted by +-300 log2 units, or climbs by 68 log2 units per key tile so that the forward's reference point moves at every tile.  Per (sequence, head,
row) against fp64 under rowwise.attention_measures_full (proved on the CPU by tests/test_attn_peaked_cpu.py), tolerances 3 x the fp32 / bf16
emulation on the same inputs; guard bands around every output.  And section (h) of the fp8 pins (tests/test_fp8_exact_gpu.py): the backward's e5m2
copy of dqkv, byte by byte.

One packed batch of eight sequences (601 rows), references evaluated on the CPU once per (head dim, profile) and shared.  The worst ratio per
kernel form, profile and quantity goes to helpers.record_margin (profiles/r22/attn_peaked_margins.json is a copy of those records)."""
import functools

import pytest
import torch

from tests import exactlib as X
from tests import fp8lib as fl
from tests import rowwise as rw
from tests.test_fp8_exact_gpu import BF8_MAX, check_codes, records
from tests.test_rowwise_gpu import (A_FUSED, A_FUSED224, PASS_BWD, PASS_FUSED, PASS_FWD, Chk, _attn_buffers, attn_meant, attn_reached, knobs,
                                    ops)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
H = 2
LENS = (1, 2, 40, 64, 65, 100, 129, 200)
ROWS = sum(LENS)
LENS_CQ = (130, 130, 130)
LENS_F32 = (1, 40, 65, 200)
FUSED_CLASSES = {32: ((0, 64), (64, 128)), 64: ((0, 64), (64, 128), (128, 224)), 80: ((0, 64),)}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """if a test leaves the device in an error state, the session ends there instead of queueing more work on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error - nothing more is started on the device: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def _ref(hd, profile, lens=LENS, lq=0):
    """case, fp64 reference and the tolerances the emulation gives on the same inputs (nobody writes to them)"""
    c = rw.attn_case(H, hd, list(lens), lq, profile=profile)
    ref = rw.attention_eval(c["qkv"], list(lens), H, c["dout"], lq)
    emu = rw.attention_eval(c["qkv"], list(lens), H, c["dout"], lq, emulate=True)
    return c, ref, rw.attention_tolerances_full(rw.attention_measures_full(emu, ref, H, list(lens)), ref)


def _measure(chk, profile, got, ref, tol, lens, case, rows_mask=None):
    for k, v in rw.attention_measures_full(got, ref, H, list(lens), rows_mask, tol=tol).items():
        chk.add(profile + "." + k, v, case)


def _grads(dqkv, rows, D):
    return {"dq": dqkv[:rows, :D].cpu(), "dk": dqkv[:rows, D:2 * D].cpu(), "dv": dqkv[:rows, 2 * D:].cpu()}


def _forward(hd, profile, tile_rows=128):
    """the buffers of the case and the forward's outputs, for the tests of a backward form"""
    o = ops()
    c, ref, tol = _ref(hd, profile)
    qkv, dout, out, lse = _attn_buffers(c, LENS, H, hd, ROWS)
    o.attn_fwd(qkv, o.AttnTiles(list(LENS), DEV, tile_rows=tile_rows), H, out, lse)
    return qkv, dout, out, lse


# ===================================================================================================
TWO_KERNEL = [(32, 64), (32, 128), (64, 64), (64, 128), (80, 64), (80, 128)]      # (the kernel table has 64-row instances of head dim 80)


@pytest.mark.parametrize("profile", rw.ATTN_PROFILES)
@pytest.mark.parametrize("hd,tile_rows", TWO_KERNEL)
def test_two_kernel_forward_and_backward(hd, tile_rows, profile):
    """out, lse, delta, dq, dk, dv of every (sequence, head, row), pad rows untouched; register-staged and ring kernels (head dim 32 / 64) bitwise
    equal"""
    o = ops()
    D = H * hd
    c, ref, tol = _ref(hd, profile)
    chk = Chk("attn_peaked.two_kernel.hd%d" % hd)
    tiles = o.AttnTiles(list(LENS), DEV, tile_rows=tile_rows)
    seen = []
    for ring in ((0,) if hd == 80 else (0, 1)):               # (head dim 80 has no ring form)
        qkv, dout, out, lse = _attn_buffers(c, LENS, H, hd, ROWS)
        with knobs(attn_ring=ring):
            assert (attn_reached(PASS_FWD, tiles, H, hd), attn_reached(PASS_BWD, tiles, H, hd)) == attn_meant(hd, tile_rows, ring)
            o.attn_fwd(qkv, tiles, H, out, lse)
            dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
            delta = torch.full_like(lse, rw.SENTINEL[F32])
            o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv)
        got = {"out": out[:ROWS].cpu(), "lse": lse[:, :ROWS].cpu(), "delta": delta[:, :ROWS].cpu(), **_grads(dqkv, ROWS, D)}
        _measure(chk, profile, got, ref, tol, LENS, (("tile_rows", tile_rows), ("ring", ring)))
        pad = torch.arange(qkv.shape[0], device=DEV) >= ROWS
        assert rw.untouched(out, pad[:out.shape[0], None]) and rw.untouched(dqkv, pad[:, None])
        assert rw.untouched(lse, pad[None, :]) and rw.untouched(delta, pad[None, :])
        seen.append((out, lse, delta, dqkv))
    if len(seen) == 2:
        assert all(rw.bitwise_equal(a, b) for a, b in zip(*seen)), (hd, tile_rows, profile, "ring and register-staged kernels differ")
    chk.done()


@pytest.mark.parametrize("profile", rw.ATTN_PROFILES)
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_fused_backward_length_classes(hd, profile):
    """avs_attn_bwd_fused for its length classes (at most 64 / 128 / 224 tokens, as the head dim has them): the rows of the class measured, every
    other row untouched"""
    o = ops()
    D = H * hd
    c, ref, tol = _ref(hd, profile)
    chk = Chk("attn_peaked.fused.hd%d" % hd)
    qkv, dout, out, lse = _forward(hd, profile)
    seq_len = torch.repeat_interleave(torch.tensor(LENS), torch.tensor(LENS))
    for lo, hi in FUSED_CLASSES[hd]:
        sq = o.AttnSeqs(list(LENS), DEV, lo, hi)
        assert sq.nseq == sum(1 for L in LENS if lo < L <= hi) > 0
        assert attn_reached(PASS_FUSED, sq, H, hd) == [(A_FUSED224 if hi == 224 else A_FUSED, 96 if hd == 80 else hd, hi // 32, 0)]
        dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
        o.attn_bwd_fused(qkv, sq, H, out, dout, lse, dqkv)
        mine = (seq_len > lo) & (seq_len <= hi)
        _measure(chk, profile, _grads(dqkv, ROWS, D), ref, tol, LENS, (("class", hi),), rows_mask=mine)
        other = torch.ones(qkv.shape[0], dtype=torch.bool)
        other[:ROWS] = ~mine
        assert rw.untouched(dqkv, other.to(DEV)[:, None]), (hd, hi)
    chk.done()


@pytest.mark.parametrize("profile", ["sharp", "staircase", "offset_neg"])
@pytest.mark.parametrize("lq", [1, 33])
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_compact_queries(hd, lq, profile):
    """three sequences of 130 tokens (three key tiles, a tail of two keys) whose first lq rows are queries; dq / lse / delta of the other rows
    untouched"""
    o = ops()
    D, rows, nq = H * hd, sum(LENS_CQ), 3 * lq
    c, ref, tol = _ref(hd, profile, LENS_CQ, lq)
    chk = Chk("attn_peaked.cq.hd%d" % hd)
    qkv, dout, out, lse = _attn_buffers(c, LENS_CQ, H, hd, nq)
    tiles = o.AttnTiles(list(LENS_CQ), DEV, tile_rows=128)
    assert (attn_reached(PASS_FWD, tiles, H, hd, lq=lq), attn_reached(PASS_BWD, tiles, H, hd, lq=lq)) == attn_meant(hd, 128)
    o.attn_fwd(qkv, tiles, H, out, lse, lq=lq)
    dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
    delta = torch.full_like(lse, rw.SENTINEL[F32])
    o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv, lq=lq)
    isq = (torch.arange(rows) % 130) < lq
    g = _grads(dqkv, rows, D)
    got = {"out": out[:nq].cpu(), "lse": lse[:, :rows].cpu() * isq, "delta": delta[:, :rows].cpu() * isq, "dq": g["dq"] * isq[:, None], "dk": g["dk"], "dv": g["dv"]}
    _measure(chk, profile, got, ref, tol, LENS_CQ, (("lq", lq),))
    notq = torch.ones(qkv.shape[0], dtype=torch.bool)
    notq[:rows] = ~isq
    notq = notq.to(DEV)
    one = torch.ones(1, 1, dtype=torch.bool, device=DEV)
    assert rw.untouched(dqkv[:, :D], notq[:, None]) and rw.untouched(lse, notq[None, :]) and rw.untouched(delta, notq[None, :])
    assert rw.untouched(dqkv[rows:], one) and rw.untouched(out[nq:], one)
    chk.done()


# ===================================================================================================
@pytest.mark.parametrize("profile", rw.ATTN_PROFILES)
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_fp32_forward(hd, profile):
    """attn_fwd_f32 on the same draws, unscaled and in fp32, under exactlib's bound exactly as it stands (it scales with the score magnitude A)"""
    o = ops()
    lens, D = list(LENS_F32), H * hd
    rows = sum(lens)
    qkv = rw.attn_case(H, hd, lens, profile=profile, scaled=False)["qkv"]
    buf, check = rw.guarded(rows, D, F32, DEV, extra_rows=40)
    o.attn_fwd_f32(qkv.to(DEV).contiguous(), o.AttnTiles(lens, DEV, tile_rows=128), H, buf)
    ref, mag, A, Lrow = X.attn_eval(qkv, lens, H)
    chk = Chk("attn_peaked.f32.hd%d" % hd)
    chk.add(profile + ".out", float(X.attn_ratio(check().cpu(), ref, mag, A, Lrow, H).max()), tuple(lens))
    chk.done()


# ===================================================================================================
# (h) the backward's e5m2 copy of dqkv (fp8 modes 2 and 3: the operand of the fp8 qkv input-gradient GEMM)
@pytest.mark.parametrize("profile", ["randn", "sharp"])
@pytest.mark.parametrize("hd", [32, 64, 80])
@pytest.mark.parametrize("form", ["two_kernel", "fused", "two_kernel_ring", "two_kernel_64_ring"])
def test_backward_e5m2_copy(form, hd, profile):
    """dqkv8 beside the bf16 dqkv, kv_bf16 1 and 0: the bf16 gradients bitwise those of the plain call (kv_bf16 = 0: the query third, the key / value
    thirds unwritten), every byte of the copy inside the rounding interval of the plain call's bf16 value, bytes of rows that are not the call's
    untouched, the recorded amax within 2^-8.  Forms: the two kernels at 128-row tiles, the fused kernel's classes, and - the copy-writing
    instantiations no other test reaches - the ring dQ kernel at both tile heights (head dim 80 has none: the knob must leave it on the
    register-staged one)."""
    with knobs(attn_ring=1 if form.endswith("ring") else 0):
        _backward_e5m2_copy(form, hd, profile)


def _backward_e5m2_copy(form, hd, profile):
    o = ops()
    D = H * hd
    qkv, dout, out, lse = _forward(hd, profile)
    seq_len = torch.repeat_interleave(torch.tensor(LENS), torch.tensor(LENS))
    if form == "fused":
        calls = [(o.AttnSeqs(list(LENS), DEV, lo, hi), (seq_len > lo) & (seq_len <= hi)) for lo, hi in FUSED_CLASSES[hd] if hi <= 128]
    else:
        calls = [(o.AttnTiles(list(LENS), DEV, tile_rows=64 if "_64" in form else 128), torch.ones(ROWS, dtype=torch.bool))]
    for which, mine in calls:
        if form == "fused":
            assert attn_reached(PASS_FUSED, which, H, hd, g8=1) == [(A_FUSED, 96 if hd == 80 else hd, which.max_len // 32, 1)]
        else:
            assert attn_reached(PASS_BWD, which, H, hd, g8=1) == attn_meant(hd, which.tile_rows, form.endswith("ring"), g8=1)[1]
        def run(rec=None, kv_bf16=True):
            dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
            d8 = torch.full(qkv.shape, rw.SENTINEL[U8], dtype=U8, device=DEV) if rec is not None else None
            kw = {} if rec is None else {"dqkv8": d8, "q8": rec, "kv_bf16": kv_bf16}
            if form == "fused":
                o.attn_bwd_fused(qkv, which, H, out, dout, lse, dqkv, **kw)
            else:
                o.attn_bwd(qkv, which, H, out, dout, lse, torch.zeros_like(lse), dqkv, **kw)
            torch.cuda.synchronize()
            return dqkv.cpu(), d8.cpu() if rec is not None else None

        plain, _ = run()
        other = torch.ones(qkv.shape[0], dtype=torch.bool)
        other[:ROWS] = ~mine
        assert rw.untouched(plain, other[:, None])
        mine_rows = torch.nonzero(mine).flatten()
        s = fl.quarter_scale(plain[mine_rows].float().abs().max(), fl.E5M2)
        for kv_bf16 in (True, False):
            rec = records([s], fmax=BF8_MAX, pow2=False)
            got, d8 = run(rec.rec(0), kv_bf16)
            if kv_bf16:
                assert rw.bitwise_equal(got, plain), (form, hd, profile)
            else:
                assert rw.bitwise_equal(got[:, :D], plain[:, :D]) and rw.untouched(got[:, D:], torch.ones(1, 1, dtype=torch.bool)), (form, hd, profile)
            check_codes("attention_dqkv8_e5m2", d8[mine_rows], plain[mine_rows], s, fl.E5M2)
            assert rw.untouched(d8, other[:, None]), (form, hd, profile, "bytes of rows outside the call's sequences were written")
            assert fl.amax_close(rec.amax(0), plain[mine_rows])


@pytest.mark.parametrize("profile", ["staircase", "offset_pos"])
@pytest.mark.parametrize("tile_rows", [64, 128])
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_forward_e4m3_copy(hd, tile_rows, profile):
    """section (g) on inputs whose reference point moves at every tile / sits 300 log2 units away: the bf16 output and lse bitwise those of the
    plain call, the e4m3 copy inside the rounding interval of the bf16 output element by element, rows behind the sequences untouched"""
    o = ops()
    D = H * hd
    c = _ref(hd, profile)[0]
    qkv = _attn_buffers(c, LENS, H, hd, ROWS)[0]
    tiles = o.AttnTiles(list(LENS), DEV, tile_rows=tile_rows)
    assert attn_reached(PASS_FWD, tiles, H, hd, g8=1) == attn_reached(PASS_FWD, tiles, H, hd) == attn_meant(hd, tile_rows)[0]      # one kernel, with and without the copy

    def run(rec=None):
        out, chk = rw.guarded(ROWS, D, BF, DEV)
        out8, chk8 = rw.guarded(ROWS, D, U8, DEV) if rec is not None else (None, None)
        lse = torch.zeros(H, qkv.shape[0], device=DEV)
        o.attn_fwd(qkv, tiles, H, out, lse, out8=out8, q8=rec)
        torch.cuda.synchronize()
        return chk().cpu(), chk8().cpu() if rec is not None else None, lse[:, :ROWS].cpu()

    out0, _, lse0 = run()
    s = fl.quarter_scale(out0.float().abs().max(), fl.E4M3)
    rec = records([s], pow2=False)
    out, out8, lse = run(rec.rec(0))
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    check_codes("attention_out8_e4m3", out8, out0, s, fl.E4M3)
    assert fl.amax_close(rec.amax(0), out0)
