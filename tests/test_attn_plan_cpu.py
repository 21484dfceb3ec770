"""avs_attn_launch_plan and engine.attention_plan (host arithmetic, no GPU).

The launch plan - kernel family, LDS image width, waves, 8-bit-copy form, grid, workgroup size, dynamic LDS of every dispatch of an attention
call - field by field against a restatement of the launch ladders as they stood BEFORE the plan existed (attn_fwd_impl, attn_bwd_impl with
the macros ATTN_BWD2 / ATTN_BWD2R, avs_attn_bwd_fused_q8 with its 224-row branch and ATTN_BWDF, of the commit "Forward GEMM launcher: one
exported host plan, one kernel table", transcribed branch by branch), over every combination below, refusals included, and against literal
anchors.  engine.attention_plan against a restatement of the old Stack._select_attention over length mixes on every threshold."""
import ctypes
import itertools
from types import SimpleNamespace

import pytest

from avsiam_amd import _lib

PASS_FWD, PASS_BWD, PASS_FUSED = range(3)                                                          # enum avs_attn_pass
FWD, FWD_RING, DQ, DQ_RING, DKV, FUSED, FUSED224 = range(7)                                        # enum avs_attn_family
FIELDS = ("family", "width", "waves", "g8", "grid", "block", "lds")                                # per dispatch, after out[0] = dispatches
SMEM224 = 3 * 224 * 64 * 2 + 224 * 128 * 2 + 2 * 224 * 4

PASSES, HDS, ROWS, G8S, LQS, RINGS, ITEMS, HEADS = (0, 1, 2), (32, 64, 80), (64, 128, 224), (0, 1), (0, 5), (0, 1), (1, 7), (1, 12)


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


class knobs:
    """tuning knobs set for a block, restored to what they were on exit"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: _lib.tuning_get(k) for k in self.kw}
        for k, v in self.kw.items():
            _lib.tuning_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.tuning_set(k, v)


def old_launch(pas, hd, rows, g8, lq, ring_knob, items, H):
    """what the old entry points launched: a list of (family, template width, template waves, template G8, grid, block, dynamic LDS) in launch
    order, or None where they returned -2.  A kernel<<<grid, block, lds>>> statement of the old text is one k(...) here."""
    grid = items * H
    if not (items > 0 and H > 0 and hd in (32, 64, 80)):                    # check_common / the fused entry point's own copy
        return None

    def k(family, width, waves, g, block, lds=0):
        return (family, width, waves, g, grid, block, lds)

    if pas == PASS_FWD:                                                      # attn_fwd_impl
        if lq < 0 or rows not in (128, 64):
            return None
        ring = ring_knob != 0 and lq == 0
        if hd == 80:
            return [k(FWD, 96, 4, 0, 256)] if rows == 128 else [k(FWD, 96, 2, 0, 128)]
        if rows == 128:
            if hd == 64:
                return [k(FWD_RING, 64, 4, 0, 256)] if ring else [k(FWD, 64, 4, 0, 256)]
            return [k(FWD_RING, 32, 4, 0, 256)] if ring else [k(FWD, 32, 4, 0, 256)]
        if hd == 64:
            return [k(FWD_RING, 64, 2, 0, 128)] if ring else [k(FWD, 64, 2, 0, 128)]
        return [k(FWD_RING, 32, 2, 0, 128)] if ring else [k(FWD, 32, 2, 0, 128)]

    if pas == PASS_BWD:                                                      # attn_bwd_impl
        if lq < 0 or rows not in (128, 64):
            return None

        def bwd2(family, g):                                                 # ATTN_BWD2(K, G)
            if hd == 80:
                return k(family, 96, 4, g, 256) if rows == 128 else k(family, 96, 2, g, 128)
            if rows == 128:
                return k(family, 64, 4, g, 256) if hd == 64 else k(family, 32, 4, g, 256)
            return k(family, 64, 2, g, 128) if hd == 64 else k(family, 32, 2, g, 128)

        def bwd2r(family, g):                                                # ATTN_BWD2R(K, G)
            if rows == 128:
                return k(family, 64, 4, g, 256) if hd == 64 else k(family, 32, 4, g, 256)
            return k(family, 64, 2, g, 128) if hd == 64 else k(family, 32, 2, g, 128)

        ring = ring_knob != 0 and hd != 80 and lq == 0
        if ring:
            first = bwd2r(DQ_RING, 1) if g8 else bwd2r(DQ_RING, 0)
        else:
            first = bwd2(DQ, 1) if g8 else bwd2(DQ, 0)
        return [first, bwd2(DKV, 1) if g8 else bwd2(DKV, 0)]

    # avs_attn_bwd_fused_q8 (it takes no lq)
    if rows not in (64, 128, 224):
        return None
    if rows == 224 and not (hd == 64 and not g8):
        return None
    if hd == 80 and rows != 64:
        return None
    if rows == 224:
        return [k(FUSED224, 64, 7, 0, 448, SMEM224)]

    def bwdf(g):                                                             # ATTN_BWDF(G)
        if hd == 80:
            return k(FUSED, 96, 2, g, 128)
        if rows == 128:
            return k(FUSED, 64, 4, g, 256) if hd == 64 else k(FUSED, 32, 4, g, 256)
        return k(FUSED, 64, 2, g, 128) if hd == 64 else k(FUSED, 32, 2, g, 128)
    return [bwdf(1) if g8 else bwdf(0)]


def launch_plan(lib, pas, hd, rows, g8, lq, items, H):
    """-> list of dispatches as tuples of FIELDS, or None for -2"""
    out = (ctypes.c_int * 15)(*([-7] * 15))
    rc = lib.avs_attn_launch_plan(pas, hd, rows, g8, lq, items, H, out, 15)
    if rc != 0:
        assert rc == -2 and b"attn_launch_plan" in lib.avs_last_error()
        return None
    return [tuple(out[1 + 7 * i: 8 + 7 * i]) for i in range(out[0])]


def test_launch_plan_equals_the_old_ladders_everywhere(lib):
    bad, n, refused = [], 0, 0
    for ring in RINGS:
        with knobs(attn_ring=ring):
            for pas, hd, rows, g8, lq, items, H in itertools.product(PASSES, HDS, ROWS, G8S, LQS, ITEMS, HEADS):
                got, want = launch_plan(lib, pas, hd, rows, g8, lq, items, H), old_launch(pas, hd, rows, g8, lq, ring, items, H)
                n += 1
                refused += want is None
                if got != want and len(bad) < 8:
                    bad.append(((pas, hd, rows, g8, lq, ring, items, H), got, want))
    assert n == 3 * 3 * 3 * 2 * 2 * 2 * 2 * 2 == 864 and 0 < refused < n
    assert not bad, bad


def test_launch_plan_refusals(lib):
    """-2 exactly where the old entry points said -2: the combinations that do not exist, and arguments no entry point accepts"""
    for args in ((PASS_FUSED, 80, 128, 0, 0, 7, 12),            # hd 80 fused above 64 rows
                 (PASS_FUSED, 32, 224, 0, 0, 7, 12),            # 224 rows with hd != 64
                 (PASS_FUSED, 64, 224, 1, 0, 7, 12),            # 224 rows with the 8-bit copy
                 (PASS_FWD, 64, 224, 0, 0, 7, 12), (PASS_BWD, 64, 224, 0, 0, 7, 12),            # 224 rows outside the fused pass
                 (PASS_FWD, 48, 128, 0, 0, 7, 12), (PASS_FWD, 64, 96, 0, 0, 7, 12), (PASS_FWD, 64, 128, 0, -1, 7, 12),
                 (PASS_BWD, 64, 128, 0, 0, 0, 12), (PASS_BWD, 64, 128, 0, 0, 7, 0), (3, 64, 128, 0, 0, 7, 12), (-1, 64, 128, 0, 0, 7, 12)):
        assert launch_plan(lib, *args) is None, args
    out = (ctypes.c_int * 15)()
    assert lib.avs_attn_launch_plan(PASS_FWD, 64, 128, 0, 0, 7, 12, None, 15) == -2
    assert lib.avs_attn_launch_plan(PASS_FWD, 64, 128, 0, 0, 7, 12, out, 0) == -2
    # ring with hd 80 and ring with lq > 0 are not refusals: the register-staged kernels run
    with knobs(attn_ring=1):
        assert launch_plan(lib, PASS_FWD, 80, 128, 0, 0, 7, 12) == [(FWD, 96, 4, 0, 84, 256, 0)]
        assert launch_plan(lib, PASS_FWD, 64, 128, 0, 5, 7, 12) == [(FWD, 64, 4, 0, 84, 256, 0)]
        assert [d[0] for d in launch_plan(lib, PASS_BWD, 80, 64, 0, 0, 7, 12)] == [DQ, DKV]
        assert [d[0] for d in launch_plan(lib, PASS_BWD, 32, 64, 0, 5, 7, 12)] == [DQ, DKV]


def test_launch_plan_anchors(lib):
    with knobs(attn_ring=0):
        # hd 64, 128-row forward: attn_fwd_kernel<64, 4>, 256 threads, no dynamic LDS, one workgroup per (tile, head)
        assert launch_plan(lib, PASS_FWD, 64, 128, 0, 0, 7, 12) == [(FWD, 64, 4, 0, 7 * 12, 256, 0)]
        # hd 80, 64-row forward: the 96-wide image, 2 waves
        assert launch_plan(lib, PASS_FWD, 80, 64, 0, 0, 3, 16) == [(FWD, 96, 2, 0, 48, 128, 0)]
        # hd 64 fused at 224 rows: 7 waves, 145 152 bytes
        assert launch_plan(lib, PASS_FUSED, 64, 224, 0, 0, 5, 12) == [(FUSED224, 64, 7, 0, 60, 448, 145152)]
        assert launch_plan(lib, PASS_FUSED, 80, 64, 1, 0, 5, 16) == [(FUSED, 96, 2, 1, 80, 128, 0)]
        assert launch_plan(lib, PASS_BWD, 32, 128, 1, 0, 4, 16) == [(DQ, 32, 4, 1, 64, 256, 0), (DKV, 32, 4, 1, 64, 256, 0)]
    with knobs(attn_ring=1):
        # the two-kernel backward with the ring knob: dQ is the ring family, dK/dV has no ring form
        assert launch_plan(lib, PASS_BWD, 64, 64, 0, 0, 7, 12) == [(DQ_RING, 64, 2, 0, 84, 128, 0), (DKV, 64, 2, 0, 84, 128, 0)]
        assert launch_plan(lib, PASS_BWD, 32, 128, 1, 0, 7, 12) == [(DQ_RING, 32, 4, 1, 84, 256, 0), (DKV, 32, 4, 1, 84, 256, 0)]
        assert launch_plan(lib, PASS_FWD, 32, 64, 1, 0, 7, 12) == [(FWD_RING, 32, 2, 0, 84, 128, 0)]        # the forward's copy is a run-time argument: g8 0
        assert launch_plan(lib, PASS_FUSED, 64, 128, 0, 0, 7, 12) == [(FUSED, 64, 4, 0, 84, 256, 0)]          # no ring form either


def test_launch_plan_short_and_long_arrays(lib):
    out = (ctypes.c_int * 20)(*([-7] * 20))
    assert lib.avs_attn_launch_plan(PASS_BWD, 64, 128, 0, 0, 7, 12, out, 4) == 0              # a shorter array receives the leading fields only
    assert list(out)[:4] == [2, DQ, 64, 4] and list(out)[4:] == [-7] * 16
    assert lib.avs_attn_launch_plan(PASS_BWD, 64, 128, 0, 0, 7, 12, out, 20) == 0             # a longer one is written up to the fields that exist
    assert list(out)[:15] == [2, DQ, 64, 4, 0, 84, 256, 0, DKV, 64, 4, 0, 84, 256, 0] and list(out)[15:] == [-7] * 5
    out = (ctypes.c_int * 20)(*([-7] * 20))
    assert lib.avs_attn_launch_plan(PASS_FWD, 64, 128, 0, 0, 7, 12, out, 20) == 0             # one dispatch: eight ints
    assert list(out)[:8] == [1, FWD, 64, 4, 0, 84, 256, 0] and list(out)[8:] == [-7] * 12


# ---------------------------------------------------------------------------------------------------
def old_select(seq_lens, hd, attn_tile, attn_fused, fused224, inference):
    """Stack._select_attention as it stood (rows = sum(seq_lens), D // H = hd, AttnSeqs(..).nseq counted here):
    -> (forward tile rows, [(lo, hi) of every fused class built], cut (None: inference has no backward), backward tile rows)"""
    def nseq(lo, hi):
        return sum(1 for L in seq_lens if lo < L <= hi)
    mean_len = sum(seq_lens) / max(1, len(seq_lens))
    force = int(attn_tile)
    if hd == 80 and not force:
        force = 128
    fwd_rows = force or (64 if mean_len < 64 else 128)
    fused = []
    if inference:
        return fwd_rows, fused, None, fwd_rows                  # self.tiles_bwd = self.tiles
    cut = 0 if not attn_fused else {32: 128, 64: 128, 80: 64}.get(hd, 0)
    if cut:
        fused = [c for c in ((0, 64), (64, cut)) if nseq(*c)]
        if hd == 64 and fused224:
            if nseq(128, 224):
                fused.append((128, 224))
                cut = 224
    long_lens = [L for L in seq_lens if L > cut]
    mean_long = sum(long_lens) / max(1, len(long_lens))
    return fwd_rows, fused, cut, force or (64 if mean_long < 256 else 128)


# length mixes on every threshold: mean length 63 / 64 / 65 (forward rows), 64 / 65 and 128 / 129 and 224 / 225 (fused classes and the cut),
# mean of the long sequences 255 / 256 (backward rows), no long sequence at all, no sequence at all
MIXES = ([63] * 3, [64] * 3, [65] * 3, [10, 116], [10, 118], [128] * 2, [129] * 2, [224] * 2, [225] * 2, [255] * 2, [256] * 2, [254, 256], [255, 257],
         [49] * 4 + [255] * 2, [49] * 4 + [256] * 2, [200, 310], [200, 312], [225, 285], [225, 287], [64, 65, 128, 129, 224, 225], [49] * 8, [2472] * 4,
         [39, 78, 117, 156, 196, 102, 204, 307, 409, 512], [])


def test_attention_plan_equals_the_old_selection():
    from avsiam_amd.engine import attention_plan
    n = 0
    for lens, hd, tile, fused, f224, inf in itertools.product(MIXES, (32, 64, 80), (0, 64, 128), (0, 1), (0, 1), (0, 1)):
        got = attention_plan(list(lens), hd, attn_tile=tile, attn_fused=bool(fused), fused224=bool(f224), inference=bool(inf))
        want = old_select(list(lens), hd, tile, fused, f224, inf)
        assert (got.fwd_rows, got.fused, got.bwd_rows) == (want[0], want[1], want[3]), (lens, hd, tile, fused, f224, inf, got, want)
        assert inf or got.cut == want[2], (lens, hd, tile, fused, f224, got, want)
        n += 1
    assert n == len(MIXES) * 3 * 3 * 2 * 2 * 2


def test_attention_plan_anchors():
    from avsiam_amd import ops
    from avsiam_amd.engine import attention_plan
    dflt = dict(attn_tile=0, attn_fused=True, fused224=False, inference=False)
    p = attention_plan([2472] * 4, 32, **dflt)                                # the decoder
    assert (p.fwd_rows, p.fused, p.bwd_rows) == (128, [], 128)
    p = attention_plan([49] * 8, 64, **dflt)                                  # an MAE video tower
    assert (p.fwd_rows, p.fused, p.bwd_rows) == (64, [(0, 64)], 64)
    assert ops.AttnTiles([49] * 8, "cpu", tile_rows=p.bwd_rows, min_len=p.cut).ntiles == 0      # every sequence went to the fused kernel
    for lens in ([51] * 4, [657, 131], [3217]):                               # hd 80: 128 rows both ways, the fused cut at 64
        p = attention_plan(lens, 80, **dflt)
        assert (p.fwd_rows, p.bwd_rows, p.cut) == (128, 128, 64)
    p = attention_plan([196, 156, 49, 512], 64, **dict(dflt, fused224=True))
    assert p.fused == [(0, 64), (128, 224)] and p.cut == 224 and p.bwd_rows == 128


def test_select_attention_builds_its_tables_from_the_plan():
    """Stack._select_attention on a stand-in stack (host tensors): the tables are those the old method built"""
    from avsiam_amd import ops
    from avsiam_amd.engine import Stack
    for lens, hd, tile, fused, f224, inf in itertools.product(([49] * 4 + [256] * 2, [64, 65, 128, 129, 224, 225], [2472] * 2), (32, 64, 80), (0, 64), (0, 1),
                                                              (0, 1), (0, 1)):
        st = SimpleNamespace(D=hd * 2, H=2, inference=bool(inf), opts=SimpleNamespace(attn_tile=tile, attn_fused=bool(fused)), _fused224=lambda: bool(f224))
        Stack._select_attention(st, lens, "cpu")
        fwd_rows, classes, cut, bwd_rows = old_select(lens, hd, tile, fused, f224, inf)
        assert st.tiles.tile_rows == fwd_rows and st.tiles.ntiles == sum((L + fwd_rows - 1) // fwd_rows for L in lens)
        assert [(sq.max_len, sq.nseq) for sq in st.fused_bwd] == [(hi, sum(1 for L in lens if lo < L <= hi)) for lo, hi in classes]
        if inf:
            assert st.tiles_bwd is st.tiles
        else:
            want = ops.AttnTiles(lens, "cpu", tile_rows=bwd_rows, min_len=cut)
            assert st.tiles_bwd.tile_rows == bwd_rows and st.tiles_bwd.start.tolist() == want.start.tolist() and st.tiles_bwd.q0.tolist() == want.q0.tolist()
