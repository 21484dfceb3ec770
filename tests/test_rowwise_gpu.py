"""The MFMA GEMM, attention and LayerNorm kernels under the row-resolved measures of tests/rowwise.py (proved on the CPU by
tests/test_rowwise_cpu.py), at the smallest shapes that reach each kernel family: every element of a GEMM output against a bound derived
from fp32 accumulation, every (sequence, head, row) of the attention outputs - lse and delta included - and every LayerNorm row - mean and rstd
included - against fp64 formulas, and guard bands around every output.  The kernel families are reached through the tuning knobs; where a
case is meant to reach one, avs_gemm_nt_plan / avs_gemm_tn_plan say that it does.

References are evaluated on the CPU, once per case, and shared.  The worst ratio of every measure goes to helpers.record_margin
(profiles/r13/rowwise_margins.json is a copy of those records)."""
import contextlib
import ctypes
import functools

import pytest
import torch

from tests import rowwise as rw
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
KNOB_DEFAULTS = {"gemm_tile": 0, "gemm_persistent": 1, "gemm_nt8": 1, "nt_tile_h": 0, "nt_grid": 0, "cu_reserve": 0, "gemm_ring": 2,
                 "nt_big_min": 0, "ln_dma": 1, "ln_rpw": 0, "attn_ring": 0, "det": 0}
TWOBUF, RING, RING_HALF, TWOBUF_HALF, PERSISTENT = range(5)           # avs_gemm_nt_plan's families


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """these tests drive kernels into corners nothing else reaches: if one leaves the device in an error state, the session ends there
    instead of queueing more work on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error - nothing more is started on the device: {e}", returncode=3)


def ops():
    from avsiam_amd import ops as o
    return o


@contextlib.contextmanager
def knobs(**kw):
    from avsiam_amd import _lib
    try:
        for k, v in kw.items():
            _lib.tuning_set(k, v)
        yield
    finally:
        for k in kw:
            _lib.tuning_set(k, KNOB_DEFAULTS[k])


def nt_plan(M, N, K):
    from avsiam_amd import _lib
    fam, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().avs_gemm_nt_plan(M, N, K, ctypes.byref(fam), ctypes.byref(wgs)) == 0
    return fam.value, wgs.value


K_TWOBUF128, K_TWOBUF128_HALF, K_RING, K_RING_HALF, K_TWOBUF256, K_NT8_ONE, K_NT8_TWO = range(7)     # avs_gemm_nt_launch_plan's kernels


def nt_launch_plan(M, N, K, m_split=0):
    """the launch gemm_nt_launch makes: kernel instantiation, grid, tile-height split (include/avsiam_hip.h)"""
    from avsiam_amd import _lib
    out = (ctypes.c_int * 8)()
    assert _lib.load().avs_gemm_nt_launch_plan(M, N, K, m_split, out, 8) == 0
    return dict(zip(("kernel", "grid", "block", "lds", "tb", "m_full", "tiles", "family"), out))


def tn_plan(M, N1, N2):
    from avsiam_amd import _lib
    tile, splits = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.load().avs_gemm_tn_plan(M, N1, N2, ctypes.byref(tile), ctypes.byref(splits)) == 0
    return tile.value, splits.value


A_FWD, A_FWD_RING, A_DQ, A_DQ_RING, A_DKV, A_FUSED, A_FUSED224 = range(7)      # avs_attn_launch_plan's kernel families
PASS_FWD, PASS_BWD, PASS_FUSED = range(3)                                        # ... and passes


def attn_reached(pas, which, H, hd, g8=0, lq=0):
    """the kernels a call on `which` (AttnTiles; AttnSeqs for the fused pass) launches under the current knobs, per dispatch:
    [(family, LDS image width, waves, 8-bit-copy form)] - avs_attn_launch_plan, the plan the launcher consumes (include/avsiam_hip.h)"""
    from avsiam_amd import _lib
    rows, items = (which.max_len, which.nseq) if pas == PASS_FUSED else (which.tile_rows, which.ntiles)
    out = (ctypes.c_int * 15)()
    assert _lib.load().avs_attn_launch_plan(pas, hd, rows, g8, lq, items, H, out, 15) == 0
    d = [tuple(out[1 + 7 * i: 8 + 7 * i]) for i in range(out[0])]
    assert all(grid == items * H and block == 64 * waves for _, _, waves, _, grid, block, _ in d)
    return [x[:4] for x in d]


def attn_meant(hd, rows, ring=0, g8=0):
    """the kernels a two-kernel case is meant to reach: (forward, [dQ, dK/dV]).  Head dim 80 runs in a 96-wide LDS image and has no ring form;
    dK/dV has none at any head dim; the forward takes its 8-bit copy at run time (no kernel of its own)"""
    w, nw, r = 96 if hd == 80 else hd, rows // 32, bool(ring) and hd != 80
    return [(A_FWD_RING if r else A_FWD, w, nw, 0)], [(A_DQ_RING if r else A_DQ, w, nw, g8), (A_DKV, w, nw, g8)]


_WORST = {}


class Chk:
    """collects ratio-to-bound figures of one test: every figure is recorded (and a failing one printed) before anything is asserted"""

    def __init__(self, kernel):
        self.kernel, self.bad, self.worst = kernel, [], {}

    def add(self, measure, ratio, case):
        ratio = float(ratio)
        if not ratio <= self.worst.get(measure, (-1.0, None))[0]:
            self.worst[measure] = (ratio, case)
        if not ratio <= 1.0:
            self.bad.append((measure, ratio, case))
            print(f"[rowwise] {self.kernel} {measure}: ratio {ratio:.4g} at {case}  <-- over its bound")

    def gemm(self, name, got, ref, S, K, case, dtype=None):
        m = rw.check_gemm(got, ref, S, K, dtype)
        self.add(name + ".elem", m["elem"], case + (("at",) + m["at"],))
        self.add(name + ".row", m["row"], case)

    def done(self):
        glob = _WORST.setdefault(self.kernel, {})
        for k, (v, case) in sorted(self.worst.items()):
            print(f"[rowwise] {self.kernel} {k}: worst ratio {v:.4g} at {case}")
            if not v <= glob.get(k, (-1.0, None))[0]:
                glob[k] = (v, case)
        record_margin("rowwise/" + self.kernel, **{k: v for k, (v, _) in glob.items()}, **{k + "_at": str(c) for k, (_, c) in glob.items()})
        assert not self.bad, self.bad[:12]


def dev(c):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in c.items()}


# ===================================================================================================
# forward / input-gradient GEMM
QS = rw.attn_q_scale(64)


def nt_suite(chk, tag, M, N, K, m_split=0):
    """every epilogue of the case list at one shape, under whatever knobs the caller holds; guard rows behind `out` and `out2` in every case.
    m_split: two weight sets (different bias2 / colsum2)."""
    o = ops()
    c = rw.gemm_nt_case(M, N, K)
    g = dev(c)
    case = (tag, M, N, K) + ((("split", m_split),) if m_split else ())
    two = dict(m_split=m_split, B2=c["B2"]) if m_split else {}

    def dual(bias, cs2=None):
        return dict(dual=(m_split, g["B2"], g["bias2"] if bias else None, cs2)) if m_split else {}

    def colsums(name, got1, got2, x, S, sub):
        for got, c0, lo, hi in ((got1, c["colsum0"], 0, m_split or M), (got2, c["colsum0_2"], m_split, M)):
            if got is None:
                continue
            want = c0.double() + x[lo:hi].sum(0)
            chk.add(name + ".colsum", rw.elem_ratio(got.cpu(), want, rw.colsum_bound(x[lo:hi], S[lo:hi], K, c0))[0], sub)

    # bf16 + bias + a column scale that ends inside a 128-column tile
    for sc in (64, 192, 320):
        if sc > N or (m_split and sc != 192):
            continue
        out, check = rw.guarded(M, N, BF, DEV)
        o.gemm_nt(g["A"], g["B"], out, M, bias=g["bias"], scale_cols=sc, col_scale=QS, **dual(True))
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], scale_cols=sc, col_scale=QS, bias2=c["bias2"], **two)
        chk.gemm("bf16_scale", check().cpu(), ref, S, K, case + (("scale_cols", sc),))
    if m_split:                                   # bf16 + bias + a column sum per weight set, onto non-zero vectors
        out, check = rw.guarded(M, N, BF, DEV)
        cs1, cs2 = g["colsum0"].clone(), g["colsum0_2"].clone()
        o.gemm_nt(g["A"], g["B"], out, M, bias=g["bias"], colsum=cs1, **dual(True, cs2))
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], bias2=c["bias2"], **two)
        chk.gemm("bf16_colsum", check().cpu(), ref, S, K, case)
        colsums("bf16_colsum", cs1, cs2, ref, S, case)
    # fp32 + bias + residual (plain and row-gathered) + alpha
    for name, r, ri in (("f32_res", "res", None), ("f32_res_idx", "res_pool", "res_idx")):
        out, check = rw.guarded(M, N, F32, DEV)
        o.gemm_nt(g["A"], g["B"], out, M, bias=g["bias"], res=g[r], res_idx=g[ri] if ri else None, alpha=1.5, **dual(True))
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], res=c[r], res_idx=c[ri] if ri else None, alpha=1.5, bias2=c["bias2"], **two)
        chk.gemm(name, check().cpu(), ref, S, K, case)
    # act 1: gelu'(x) as bf16 and as 8-bit codes, gelu(x) beside it
    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], bias2=c["bias2"], **two)
    dx = rw.gemm_bound(ref, S, K, rw.U_F32)
    gr, ge = rw.gelu_grad64(ref), rw.gelu64(ref)
    for codes in (False, True):
        out, check = rw.guarded(M, N, U8 if codes else BF, DEV)
        out2, check2 = rw.guarded(M, N, BF, DEV)
        o.gemm_nt(g["A"], g["B"], out, M, bias=g["bias"], out2=out2, act=1, **dual(True))
        got = check().cpu()
        name = "act1_codes" if codes else "act1_bf16"
        chk.add(name + ".gelu_grad", rw.elem_ratio(rw.gp8_value(got) if codes else got, gr, rw.gelu_grad_bound(dx, gr, codes))[0], case)
        chk.add(name + ".gelu", rw.elem_ratio(check2().cpu(), ge, rw.gelu_bound(dx, ge))[0], case)
    # act 2: the saved gelu'(x) (bf16 or codes) multiplies the product; column sum onto a non-zero vector
    for name, aux in (("act2_bf16", "aux"), ("act2_codes", "aux8")):
        out, check = rw.guarded(M, N, BF, DEV)
        cs1 = g["colsum0"].clone()
        cs2 = g["colsum0_2"].clone() if m_split else None
        o.gemm_nt(g["A"], g["B"], out, M, aux=g[aux], act=2, colsum=cs1, **dual(False, cs2))
        ref, S = rw.gemm_nt_terms(c["A"], c["B"], None, aux=rw.gp8_decode(c[aux]) if aux == "aux8" else c[aux], **two)
        chk.gemm(name, check().cpu(), ref, S, K, case)
        colsums(name, cs1, cs2, ref, S, case)


NT_SMALL = {   # knobs, the family avs_gemm_nt_plan must name, (N, K) pairs
    "twobuf": (dict(gemm_ring=0), TWOBUF, ((128, 64), (384, 192), (512, 256), (384, 320))),
    "ring": (dict(gemm_ring=1), RING, ((128, 256), (384, 320), (512, 256))),
    "ring_half": (dict(gemm_ring=2), RING_HALF, ((128, 256), (384, 320), (512, 256))),
    "twobuf_half": (dict(gemm_ring=2), TWOBUF_HALF, ((128, 64), (384, 192), (512, 192))),
}


@pytest.mark.parametrize("family", list(NT_SMALL))
def test_gemm_nt_128_tile_families(family):
    """The 128 x 128 two-buffer kernel, the LDS-DMA ring (K = 256 fills its four slots exactly, K = 320 is the first wrap), and the half-height
    tiles of both (K = 192 falls below the ring's K >= 256: the two-buffer half-height family), at M = 1, a tile +- 1, and ragged last tiles."""
    kn, fam, shapes = NT_SMALL[family]
    chk = Chk("gemm_nt." + family)
    with knobs(**kn):
        for N, K in shapes:
            for M in rw.NT_M:
                assert nt_plan(M, N, K)[0] == fam, (family, M, N, K, nt_plan(M, N, K))
                nt_suite(chk, family, M, N, K)
    chk.done()


NT_BIG_M = (1, 65, 223, 224, 225, 255, 256, 257, 300, 600)


@pytest.mark.parametrize("tile_h,grid", [(0, 0), (256, 0), (224, 0), (0, 2), (224, 2)])
def test_gemm_nt_persistent_8phase_at_small_shapes(tile_h, grid):
    """The persistent 8-phase 256 x 256 kernel - reached by the suite's other tests only from 9000 rows up - at a few hundred rows
    (nt_big_min = 1): both tile-height classes, two K-tiles (K = 128) and an odd count (K = 320), and with nt_grid = 2 two workgroups that
    walk the (up to six) tiles.  At these row counts the automatic heights (0) make every tile 224 rows, as nt_tile_h = 224 does: the
    two-class instantiation with an empty first class; 256 is the one-class instantiation."""
    chk = Chk("gemm_nt.persistent8")
    with knobs(nt_big_min=1, nt_tile_h=tile_h, nt_grid=grid):
        for K in (128, 320):
            for M in NT_BIG_M:
                assert nt_plan(M, 512, K)[0] == PERSISTENT
                p = nt_launch_plan(M, 512, K)
                assert (p["kernel"], p["tb"]) == ((K_NT8_ONE, 0) if tile_h == 256 else (K_NT8_TWO, 0)), (tile_h, M, K, p)
                tiles = 2 * -(-M // (256 if tile_h == 256 else 224))
                assert p["tiles"] == tiles and p["grid"] == (min(grid, tiles) if grid else tiles), (tile_h, grid, M, K, p)
                nt_suite(chk, "h%d_grid%d" % (tile_h, grid), M, 512, K)
    chk.done()


def test_gemm_nt_persistent_8phase_two_height_classes_in_one_launch():
    """nt_tile_h = 240: half the row tiles of each height.  The first class holds whole row tiles and a multiple of 8 tiles (`unit` in
    nt_plan), so it is non-empty only from 8 column tiles on: M = 600, N = 2048 gives 8 tiles of 256 rows and 2 x 8 of 224."""
    chk = Chk("gemm_nt.persistent8")
    with knobs(nt_big_min=1, nt_tile_h=240):
        assert nt_plan(600, 2048, 128)[0] == PERSISTENT
        p = nt_launch_plan(600, 2048, 128)
        assert (p["kernel"], p["tb"], p["tiles"], p["grid"]) == (K_NT8_TWO, 8, 24, 24), p
        nt_suite(chk, "h240", 600, 2048, 128)
    chk.done()


@pytest.mark.parametrize("persistent", [0, 1])
def test_gemm_nt_two_buffer_256_tile_kernel(persistent):
    """gemm_nt8 = 0: the two-buffer 256 x 256 kernel, one workgroup per tile or persistent (nt_plan: the branch after the 8-phase one).
    avs_gemm_nt_plan names the family PERSISTENT for it and for the 8-phase kernels; avs_gemm_nt_launch_plan names the kernel."""
    chk = Chk("gemm_nt.twobuf256")
    with knobs(nt_big_min=1, gemm_nt8=0, gemm_persistent=persistent):
        for K in (64, 320):
            for M in (1, 255, 256, 257, 300, 600):
                assert nt_plan(M, 512, K)[0] == PERSISTENT
                p = nt_launch_plan(M, 512, K)
                assert (p["kernel"], p["m_full"], p["grid"]) == (K_TWOBUF256, M, 2 * -(-M // 256)), (persistent, M, K, p)
                nt_suite(chk, "persistent%d" % persistent, M, 512, K)
    chk.done()


@pytest.mark.parametrize("side", ["128", "256"])
def test_gemm_nt_two_weight_sets(side):
    """m_split = 256 with M = 257 (one row of the second set) and 600, different bias2 / colsum2, on the 128 x 128 kernels and on the
    persistent 256 x 256 kernel"""
    chk = Chk("gemm_nt.dual" + side)
    with knobs(nt_big_min=1 if side == "256" else 1 << 20):
        for K in (192, 320):
            for M in (257, 600):
                assert (nt_plan(M, 512, K)[0] == PERSISTENT) == (side == "256")
                nt_suite(chk, "dual" + side, M, 512, K, m_split=256)
    chk.done()


# ===================================================================================================
# weight-gradient GEMM
@functools.lru_cache(maxsize=None)
def _tn_ref(M, N1, N2):
    c = rw.gemm_tn_case(M, N1, N2)
    return (c,) + rw.gemm_tn_terms(c["A"], c["B"], c["C0"])


def _tn_run(chk, name, M, N1, N2, splits, case):
    o = ops()
    c, ref, S = _tn_ref(M, N1, N2)
    buf, check = rw.guarded(N1, N2, F32, DEV, extra_rows=8)
    buf[:N1] = c["C0"].to(DEV)
    o.gemm_tn(c["A"].to(DEV), c["B"].to(DEV), buf[:N1], M, splits)
    chk.gemm(name, check().cpu(), ref, S, M, case)


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("nt8", [0, 1])
def test_gemm_tn_tiles_and_splits(tile, nt8):
    """C += A^T B onto a non-zero C, the contraction over M = 1 ... 513 token rows (operands zero to the next multiple of 64): both output
    tile sizes, the two-buffer and the 8-phase 256 x 256 kernel, one split, two, and more than there are 64-row stages (clamped)"""
    chk = Chk("gemm_tn")
    with knobs(gemm_tile=tile, gemm_nt8=nt8):
        for M in rw.TN_M:
            for N1, N2 in rw.TN_N:
                if tile == 256 and (N1 % 256 or N2 % 256):
                    continue                                  # (tn_plan: a forced 256 applies where both N are multiples of 256)
                assert tn_plan(M, N1, N2)[0] == tile
                for splits in (1, 2, 99):
                    _tn_run(chk, "tile%d_nt8_%d" % (tile, nt8), M, N1, N2, splits, (M, N1, N2, ("splits", splits)))
    chk.done()


def test_gemm_tn_automatic_and_deterministic_plan():
    chk = Chk("gemm_tn")
    for det in (0, 1):
        with knobs(det=det):
            for M in rw.TN_M:
                for N1, N2 in rw.TN_N:
                    if det:
                        assert tn_plan(M, N1, N2)[1] == 1          # one writer per output tile
                    _tn_run(chk, "auto_det%d" % det, M, N1, N2, 0, (M, N1, N2))
    chk.done()


@pytest.mark.parametrize("shapes", [((256, 256), (256, 512)), ((256, 256), (256, 512), (512, 256)), ((128, 256), (256, 256))])
def test_gemm_tn_group(shapes):
    """two and three weight gradients over the same 513 token rows (the smallest M with 8 stages: below it avs_gemm_tn_bf16_group3 issues one
    launch per problem) in one launch; an N that is no multiple of 256 takes that fall-back too"""
    o = ops()
    M = 513
    chk = Chk("gemm_tn.group")
    jobs, checks = [], []
    for i, (N1, N2) in enumerate(shapes):
        c, ref, S = _tn_ref(M, N1, N2)
        buf, check = rw.guarded(N1, N2, F32, DEV, extra_rows=8)
        buf[:N1] = c["C0"].to(DEV)
        jobs.append((c["A"].to(DEV), c["B"].to(DEV), buf[:N1]))
        checks.append((check, ref, S, (M, N1, N2, ("problem", i))))
    o.gemm_tn_group(jobs, M)
    for check, ref, S, case in checks:
        chk.gemm("group%d" % len(shapes), check().cpu(), ref, S, M, case)
    chk.done()


# ===================================================================================================
# attention
@functools.lru_cache(maxsize=None)
def _attn_ref(hd, lens, lq=0):
    H = 2
    c = rw.attn_case(H, hd, list(lens), lq)
    ref = rw.attention_eval(c["qkv"], list(lens), H, c["dout"], lq)
    emu = rw.attention_eval(c["qkv"], list(lens), H, c["dout"], lq, emulate=True)
    return c, ref, rw.attention_tolerances(rw.attention_measures(emu, ref, H))


def _attn_buffers(c, lens, H, hd, nq):
    o = ops()
    D, rows = H * hd, sum(lens)
    rp = o.pad_rows(rows) + 128
    qkv = torch.zeros(rp, 3 * D, device=DEV, dtype=BF)
    qkv[:rows] = c["qkv"].to(DEV)
    dout = torch.zeros(o.pad_rows(nq) + 128, D, device=DEV, dtype=BF)
    dout[:nq] = c["dout"].to(DEV)
    out = torch.full((dout.shape[0], D), rw.SENTINEL[BF], device=DEV, dtype=BF)
    lse = torch.full((H, rp), rw.SENTINEL[F32], device=DEV)
    return qkv, dout, out, lse


def _attn_check(chk, got, ref, tol, H, case, rows_mask=None):
    for k, v in rw.attention_measures(got, ref, H, rows_mask, tol=tol).items():
        chk.add(k, v, case)


@pytest.mark.parametrize("hd,tile_rows,ring", [(32, 64, 0), (32, 128, 0), (32, 64, 1), (32, 128, 1), (64, 64, 0), (64, 128, 0), (64, 64, 1), (64, 128, 1),
                                               (80, 128, 0), (80, 64, 0)])      # (hd 80: no ring form - attn_reached says which kernels ran)
def test_attention_per_sequence_head_and_row(hd, tile_rows, ring):
    """One packed batch of 15 sequences of 1 ... 200 tokens (one key, a tile - 1 / tile / tile + 1 for every tile size in the kernels, a tail
    of one key): out, lse, delta, dq, dk, dv of every (sequence, head, row) against fp64, tolerances 3 x the fp32 / bf16 emulation's worst row
    on the same inputs; pad rows untouched."""
    o = ops()
    H, lens = 2, tuple(rw.ATTN_LENS)
    D, rows = H * hd, sum(lens)
    c, ref, tol = _attn_ref(hd, lens)
    chk = Chk("attention.hd%d" % hd)
    case = (("tile_rows", tile_rows), ("ring", ring))
    qkv, dout, out, lse = _attn_buffers(c, lens, H, hd, rows)
    tiles = o.AttnTiles(list(lens), DEV, tile_rows=tile_rows)
    with knobs(attn_ring=ring):
        assert (attn_reached(PASS_FWD, tiles, H, hd), attn_reached(PASS_BWD, tiles, H, hd)) == attn_meant(hd, tile_rows, ring)
        o.attn_fwd(qkv, tiles, H, out, lse)
        dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
        delta = torch.full_like(lse, rw.SENTINEL[F32])
        o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv)
    got ={"out": out[:rows].cpu(), "lse": lse[:, :rows].cpu(), "delta": delta[:, :rows].cpu(), "dq": dqkv[:rows, :D].cpu(),
           "dk": dqkv[:rows, D:2 * D].cpu(), "dv": dqkv[:rows, 2 * D:].cpu()}
    _attn_check(chk, got, ref, tol, H, case)
    pad = torch.arange(qkv.shape[0], device=DEV) >= rows
    assert rw.untouched(out, pad[:out.shape[0], None]) and rw.untouched(dqkv, pad[:, None])
    assert rw.untouched(lse, pad[None, :]) and rw.untouched(delta, pad[None, :])
    chk.done()


@pytest.mark.parametrize("hd", [32, 64, 80])
def test_attention_fused_backward_length_classes(hd):
    """avs_attn_bwd_fused for its length classes (at most 64 / 128 / 224 tokens; hd 32 has the first two, hd 80 the first): the sequences of the
    class measured per (sequence, head, row), the rows of every other sequence and the pad rows untouched"""
    o = ops()
    H, lens = 2, tuple(rw.ATTN_LENS)
    D, rows = H * hd, sum(lens)
    c, ref, tol = _attn_ref(hd, lens)
    chk = Chk("attention_fused.hd%d" % hd)
    qkv, dout, out, lse = _attn_buffers(c, lens, H, hd, rows)
    o.attn_fwd(qkv, o.AttnTiles(list(lens), DEV, tile_rows=128), H, out, lse)
    seq_len = torch.repeat_interleave(torch.tensor(lens), torch.tensor(lens))
    for lo, hi in {32: ((0, 64), (64, 128)), 64: ((0, 64), (64, 128), (128, 224)), 80: ((0, 64),)}[hd]:
        sq = o.AttnSeqs(list(lens), DEV, lo, hi)
        assert sq.nseq == sum(1 for L in lens if lo < L <= hi) > 0
        assert attn_reached(PASS_FUSED, sq, H, hd) == [(A_FUSED224 if hi == 224 else A_FUSED, 96 if hd == 80 else hd, hi // 32, 0)]
        dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
        o.attn_bwd_fused(qkv, sq, H, out, dout, lse, dqkv)
        mine = (seq_len > lo) & (seq_len <= hi)
        got = {"dq": dqkv[:rows, :D].cpu(), "dk": dqkv[:rows, D:2 * D].cpu(), "dv": dqkv[:rows, 2 * D:].cpu()}
        _attn_check(chk, got, ref, tol, H, (("class", hi),), rows_mask=mine)
        other = torch.ones(qkv.shape[0], dtype=torch.bool)
        other[:rows] = ~mine
        assert rw.untouched(dqkv, other.to(DEV)[:, None]), (hd, hi)
    chk.done()


@pytest.mark.parametrize("hd", [32, 64, 80])
@pytest.mark.parametrize("lq", [1, 33])
def test_attention_compact_queries(hd, lq):
    """the pruned form: three sequences of 65 tokens whose first lq rows are queries; out / dO compact.  dq of the rows that are not queries, and
    their lse / delta, are the caller's: untouched."""
    o = ops()
    H, lens = 2, (65, 65, 65)
    D, rows, nq = H * hd, 195, 3 * lq
    c, ref, tol = _attn_ref(hd, lens, lq)
    chk = Chk("attention_cq.hd%d" % hd)
    qkv, dout, out, lse = _attn_buffers(c, lens, H, hd, nq)
    tiles = o.AttnTiles(list(lens), DEV, tile_rows=128)
    with knobs(attn_ring=1):                       # (the compact form has no ring kernels: the knob changes nothing)
        assert (attn_reached(PASS_FWD, tiles, H, hd, lq=lq), attn_reached(PASS_BWD, tiles, H, hd, lq=lq)) == attn_meant(hd, 128)
    assert (attn_reached(PASS_FWD, tiles, H, hd, lq=lq), attn_reached(PASS_BWD, tiles, H, hd, lq=lq)) == attn_meant(hd, 128)
    o.attn_fwd(qkv, tiles, H, out, lse, lq=lq)
    dqkv = torch.full_like(qkv, rw.SENTINEL[BF])
    delta = torch.full_like(lse, rw.SENTINEL[F32])
    o.attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv, lq=lq)
    isq = (torch.arange(rows) % 65) < lq
    got = {"out": out[:nq].cpu(), "lse": lse[:, :rows].cpu() * isq, "delta": delta[:, :rows].cpu() * isq, "dq": dqkv[:rows, :D].cpu() * isq[:, None],
           "dk": dqkv[:rows, D:2 * D].cpu(), "dv": dqkv[:rows, 2 * D:].cpu()}
    _attn_check(chk, got, ref, tol, H, (("lq", lq),))
    notq = torch.ones(qkv.shape[0], dtype=torch.bool)
    notq[:rows] = ~isq
    notq = notq.to(DEV)
    assert rw.untouched(dqkv[:, :D], notq[:, None]) and rw.untouched(lse, notq[None, :]) and rw.untouched(delta, notq[None, :])
    assert rw.untouched(dqkv[rows:], torch.ones(1, 1, dtype=torch.bool, device=DEV)) and rw.untouched(out[nq:], torch.ones(1, 1, dtype=torch.bool, device=DEV))
    chk.done()


# ===================================================================================================
# LayerNorm
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _ln_ref(D, kind):
    """references over the 33 rows of the case (the row counts of the case list are prefixes): fp64 forward, the fp32 two-pass evaluation's worst
    rstd error, and for the two backward forms (fp32 dres; bf16 dres stream) the fp64 formula with its magnitude rows and the fp32
    evaluation's worst rows"""
    c = rw.ln_case(D, kind)
    fwd = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], EPS, c["mod"], c["g"][1], c["b"][1])
    emu = rw.layernorm_eval(c["x"], c["g"][0], c["b"][0], EPS, c["mod"], c["g"][1], c["b"][1], emulate=True)
    tol = {"rstd": 3.0 * max(float(((emu["rstd"].double() - fwd["rstd"]).abs() / fwd["rstd"]).max()), rw.U_F32)}
    c["mean"], c["rstd"] = fwd["mean"].float(), fwd["rstd"].float()             # the backward's inputs
    c["dres16"] = c["dres"].to(BF)
    bwd = {}
    for form, dres in (("f32", c["dres"]), ("bf16", c["dres16"])):
        r = rw.layernorm_bwd_eval(c["dy"], c["x"], c["mean"], c["rstd"], c["g"][0], dres, c["mod"], c["g"][1])
        e = rw.layernorm_bwd_eval(c["dy"], c["x"], c["mean"], c["rstd"], c["g"][0], dres, c["mod"], c["g"][1], emulate=True)
        bwd[form] = r
        tol["dx_" + form] = 3.0 * max(float(rw.mag_row_ratio(e["dx"], r["dx"], r["dx_abs"]).max()), rw.U_F32)
        tol["dxb_" + form] = 3.0 * float(rw.mag_row_ratio(e["dx"].to(BF), r["dx"], r["dx_abs"]).max())
    return c, fwd, bwd, tol


def _ln_forward(chk, D, kind, r, f32_offset=False):
    o = ops()
    c, fwd, bwd, tol = _ln_ref(D, kind)
    g = dev({k: c[k] for k in ("x", "g", "b", "mod")})
    perm = torch.randperm(r, generator=torch.Generator().manual_seed(r)).to(torch.int32)
    case = (D, kind, ("rows", r))
    for dtype in (BF, F32):
        y, check = rw.guarded(r, D, dtype, DEV, extra_rows=8)
        mean = torch.full((r + 8,), rw.SENTINEL[F32], device=DEV)
        rstd = torch.full((r + 8,), rw.SENTINEL[F32], device=DEV)
        o.layernorm_fwd(g["x"], g["g"][0], g["b"][0], y, mean, rstd, r, EPS, g["g"][1], g["b"][1], g["mod"], perm.to(DEV))
        got = check().cpu()[perm.long()]                          # output row i went to y[out_map[i]]
        name = "y_bf16" if dtype == BF else "y_f32"
        if (dtype == F32 and kind == "offset") == f32_offset:      # (the fp32 y of the offset input has the file's last test to itself)
            chk.add(name + ".row", float(rw.row_rel(got, fwd["y"][:r]).max()) / rw.NT_ROW_TOL[dtype], case)
        if f32_offset:
            continue
        if dtype == F32:                                           # and against the fp64 y of the mean the kernel stored: everything but that mean's rounding
            yk = rw.layernorm_y_given_stats(c["x"][:r], mean[:r].cpu(), fwd["rstd"][:r], c["g"][0], c["b"][0], c["mod"][:r], c["g"][1], c["b"][1])
            chk.add("y_f32.row_given_mean", float(rw.row_rel(got, yk).max()) / rw.NT_ROW_TOL[F32], case)
        chk.add("mean", float(((mean[:r].cpu().double() - fwd["mean"][:r]).abs() / rw.layernorm_mean_bound(c["x"][:r])).max()), case)
        chk.add("rstd", float(((rstd[:r].cpu().double() - fwd["rstd"][:r]).abs() / fwd["rstd"][:r]).max()) / tol["rstd"], case)
        assert rw.untouched(mean[r:], torch.ones(1, dtype=torch.bool, device=DEV)) and rw.untouched(rstd[r:], torch.ones(1, dtype=torch.bool, device=DEV))
    if kind == "const" and not f32_offset:
        chk.add("rstd_const_row", abs(float(rstd[0]) - EPS ** -0.5) / (tol["rstd"] * EPS ** -0.5), case)


def _ln_param_checks(chk, name, c, ref, r, targets, init, case, D, with_dcol):
    dg, db, dcol = targets
    for i in range(2):
        sel = (c["mod"][:r] == i)
        for t, terms, nm in ((dg[i], ref["dy_xh"][:r], "dg"), (db[i], ref["dy"][:r], "db")):
            if t is None:
                continue
            want, bound = rw.rowsum_bound(terms, sel, torch.full((D,), init))
            chk.add(name + "." + nm, rw.elem_ratio(t.cpu(), want, bound)[0], case + (("set", i),))
    if with_dcol:
        want, bound = rw.rowsum_bound(ref["dx"][:r], torch.ones(r, dtype=torch.bool), torch.full((D,), init), extra=D + 8, mag=ref["dx_abs"][:r])
        chk.add(name + ".dcol", rw.elem_ratio(dcol.cpu(), want, bound)[0], case)


def _ln_backward(chk, D, kind, r, head=False):
    """the two forms of the call under whatever knobs the caller holds: fp32 residual gradient -> fp32 dx, its bf16 copy, the parameter gradients of both
    affine sets and the column sum, all accumulated onto 0.5; bf16 residual-gradient stream -> the bf16 dx only (the LDS-DMA kernel's case)"""
    o = ops()
    c, fwd, bwd, tol = _ln_ref(D, kind)
    g = dev({k: c[k] for k in ("x", "g", "mod", "mean", "rstd", "dres", "dres16")})
    perm = torch.randperm(r, generator=torch.Generator().manual_seed(100 + r)).to(torch.int32)
    dy = torch.zeros(r, D, dtype=BF)
    dy[perm.long()] = c["dy"][:r]                                 # the backward reads row i's dy at dy[out_map[i]]
    dy, permd = dy.to(DEV), perm.to(DEV)
    ws = torch.empty(max(o.layernorm_ws(r, D), 1), device=DEV)
    init = 0.5
    for form in ("f32", "bf16"):
        ref = bwd[form]
        case = (D, kind, ("rows", r), form)
        dg = [torch.full((D,), init, device=DEV) for _ in range(2)]
        db = [torch.full((D,), init, device=DEV) for _ in range(2)]
        dcol = None if head else torch.full((D,), init, device=DEV)
        dxb, checkb = rw.guarded(r, D, BF, DEV, extra_rows=8)
        dx = check = None
        if form == "f32":
            dx, check = rw.guarded(r, D, F32, DEV, extra_rows=8)
        o.layernorm_bwd(dy, g["x"], g["mean"], g["rstd"], g["g"][0], dx, dg[0], db[0], ws, r, g["g"][1], dg[1], db[1], g["mod"], permd,
                        g["dres"] if form == "f32" else g["dres16"], dxb, dcol)
        if dx is not None:
            chk.add("dx_f32", float(rw.mag_row_ratio(check().cpu(), ref["dx"][:r], ref["dx_abs"][:r]).max()) / tol["dx_f32"], case)
        chk.add("dx_bf16", float(rw.mag_row_ratio(checkb().cpu(), ref["dx"][:r], ref["dx_abs"][:r]).max()) / tol["dxb_" + form], case)
        _ln_param_checks(chk, "bwd_" + form, c, ref, r, (dg, db, dcol), init, case, D, not head)


@pytest.mark.parametrize("kind", rw.LN_KINDS)
@pytest.mark.parametrize("D", rw.LN_D)
def test_layernorm_rows(D, kind):
    """forward (bf16 and fp32 y, mean, rstd) and backward (dx, its bf16 copy, dg / db per affine set, the column sum) of 1 ... 33 rows with two affine
    sets and a permuted output, per row; the backward under every rows-per-wave setting, with the LDS-DMA kernel and without"""
    chk = Chk("layernorm.D%d" % D)
    for r in rw.LN_ROWS:
        _ln_forward(chk, D, kind, r)
        for rpw in (0, 4, 8, 16):
            for dma in (0, 1):
                with knobs(ln_rpw=rpw, ln_dma=dma):
                    _ln_backward(chk, D, kind, r)
    chk.done()


@pytest.mark.parametrize("kind", rw.LN_KINDS)
@pytest.mark.parametrize("D", rw.LN_D_HEAD)
def test_layernorm_head_widths(D, kind):
    """the classifier-head widths: their own backward kernels (no column sum, parameter gradients reduced in the call)"""
    chk = Chk("layernorm_head.D%d" % D)
    for r in rw.LN_ROWS:
        _ln_forward(chk, D, kind, r)
        _ln_backward(chk, D, kind, r, head=True)
    chk.done()


@pytest.mark.parametrize("D", rw.LN_D)
def test_layernorm_deferred_reduce_of_one_call(D):
    """the parameter gradients left as slabs by one backward and added to their targets by avs_layernorm_bwd_reduce_batched"""
    o = ops()
    chk = Chk("layernorm.D%d" % D)
    c, fwd, bwd, tol = _ln_ref(D, "usual")
    g = dev({k: c[k] for k in ("x", "g", "mod", "mean", "rstd", "dres16")})
    for r in (17, 33):
        ref = bwd["bf16"]
        dg = [torch.full((D,), 0.5, device=DEV) for _ in range(2)]
        db = [torch.full((D,), 0.5, device=DEV) for _ in range(2)]
        dcol = torch.full((D,), 0.5, device=DEV)
        ws = torch.full((o.layernorm_bwd_slabs(r) * 5 * D,), float("nan"), device=DEV)
        batch = o.LnReduceBatch(D)
        batch.add(ws, r, dg[0], db[0], dg[1], db[1], dcol)
        batch.build(DEV)
        dxb, checkb = rw.guarded(r, D, BF, DEV, extra_rows=8)
        o.layernorm_bwd(c["dy"][:r].to(DEV), g["x"], g["mean"], g["rstd"], g["g"][0], None, dg[0], db[0], ws, r, g["g"][1], dg[1], db[1], g["mod"], None,
                        g["dres16"], dxb, dcol, defer=True)
        assert all(float((t - 0.5).abs().max()) == 0.0 for t in dg + db + [dcol])          # nothing reduced before run()
        batch.run()
        case = (D, "usual", ("rows", r), "deferred")
        chk.add("dx_bf16", float(rw.mag_row_ratio(checkb().cpu(), ref["dx"][:r], ref["dx_abs"][:r]).max()) / tol["dxb_bf16"], case)
        _ln_param_checks(chk, "deferred", c, ref, r, (dg, db, dcol), 0.5, case, D, True)
    chk.done()


# ===================================================================================================
# leading dimensions: the header documents them, the wrappers only ever pass contiguous tensors
def test_gemm_nt_output_leading_dimension():
    """avs_gemm_nt_bf16 with ldo = N + 8 (every nt kernel stores through a.ldo in nt_epilogue): the 8 columns beyond N stay untouched"""
    from avsiam_amd import _lib
    o = ops()
    M, N, K = 129, 384, 320
    c = rw.gemm_nt_case(M, N, K)
    g = dev(c)
    chk = Chk("gemm_nt.ld")
    out, check = rw.guarded(M, N, BF, DEV, extra_cols=8)
    o._call("avs_gemm_nt_bf16", g["A"], K, g["B"], K, M, N, K, g["bias"], None, 0, None, None, 0, out, N + 8, 0, None, 0, 1.0, 0, 192, rw.f32(QS), None, _lib.current_stream())
    ref, S = rw.gemm_nt_terms(c["A"], c["B"], c["bias"], scale_cols=192, col_scale=QS)
    chk.gemm("ldo", check().cpu(), ref, S, K, (M, N, K, ("ldo", N + 8)))
    chk.done()


def test_attention_forward_output_leading_dimension():
    """avs_attn_fwd with ldo = D + 8 (the forward kernels store through a.ldo)"""
    from avsiam_amd import _lib
    o = ops()
    H, hd, lens = 2, 64, tuple(rw.ATTN_LENS)
    D, rows = H * hd, sum(lens)
    c, ref, tol = _attn_ref(hd, lens)
    chk = Chk("attention.ld")
    qkv, dout, _, lse = _attn_buffers(c, lens, H, hd, rows)
    out, check = rw.guarded(rows, D, BF, DEV, extra_cols=8)
    tiles = o.AttnTiles(list(lens), DEV, tile_rows=128)
    o._call("avs_attn_fwd", qkv, 3 * D, D, H, tiles.start, tiles.len, tiles.q0, tiles.ntiles, 128, out, D + 8, lse, lse.shape[1], _lib.current_stream())
    _attn_check(chk, {"out": check().cpu(), "lse": lse[:, :rows].cpu()}, ref, tol, H, (("ldo", D + 8),))
    chk.done()


# ===================================================================================================
@pytest.mark.parametrize("D", rw.LN_D + rw.LN_D_HEAD)
def test_layernorm_fp32_output_per_row_on_the_offset_input(D):
    """The fp32 y of the rows 50 + 0.5 randn, per row, at the suite's fp32 tolerance 1e-5 (every other LayerNorm measure of these rows is in the
    tests above).  Regression test of the fp32-output forward kernel: with the mean taken from one fp32 row sum it missed this bound at three
    widths - worst row error / 1e-5 for D = 512 ... 2560:  0.90  1.34  0.84  1.02  1.44  0.41  0.90.  The row sum is ~50 D (38 400 at D = 768:
    its last additions round to 2e-3), so the mean was off by a few 1e-6 - 0.3 % of the bound asserted for `mean` - and every element of the
    row moved by that times rstd = 2, i.e. ~1e-5 of a row whose normalised values are of size 1; an fp32 two-pass torch evaluation of the same
    rows (layernorm_eval, emulate=True) gives 1.26  1.23  1.06  0.80  1.48  1.12  1.15.  ln_fwd_kernel<., true> now takes the mean of the
    centred values off again (one more wave reduction, fp32 output only, and only where it moves the normalised values by more than 2^-21, so
    that ordinary rows keep their bits): at most 0.05.  The stored mean is still one fp32 number, which is why y_f32.row_given_mean in the
    tests above sits at 0.35 - 0.38 on these rows: that is the rounding of 50 to fp32, times rstd."""
    chk = Chk("layernorm_f32_offset.D%d" % D)
    for r in rw.LN_ROWS:
        _ln_forward(chk, D, "offset", r, f32_offset=True)
    chk.done()
