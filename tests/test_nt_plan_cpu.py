"""avs_gemm_nt_launch_plan (host arithmetic, no GPU): the launch the forward / input-gradient GEMM launcher makes - kernel instantiation, grid,
workgroup size, dynamic LDS, tile-height split - field by field against a restatement of the launcher as it stood BEFORE the plan existed
(gemm_nt_launch of the commit "GEMM epilogues: buffer descriptors + one lane offset replace row maths", transcribed branch by branch, C integer
arithmetic included), over every combination of the shapes and knobs below, and against literal anchors of the model's own shapes."""
import ctypes
import itertools
import math

import pytest

from avsiam_amd import _lib

# the fields avs_gemm_nt_launch_plan writes, in order (include/avsiam_hip.h)
FIELDS = ("kernel", "grid", "block", "lds", "tb", "m_full", "tiles", "family")
TWOBUF128, TWOBUF128_HALF, RING, RING_HALF, TWOBUF256, NT8_ONE, NT8_TWO = range(7)                  # "kernel"
FAM_TWOBUF, FAM_RING, FAM_RING_HALF, FAM_TWOBUF_HALF, FAM_PERSISTENT = range(5)                       # "family" (avs_gemm_nt_plan's)
ONE_SET = 0x7FFFFFFF                                                                                # the old launcher's "no second weight set"

MS = (1, 224, 225, 256, 257, 600, 2832, 11328, 27419, 95630)
NS = (128, 256, 384, 512, 768, 2048, 2304, 3072)
KS = (64, 128, 320)
M_SPLITS = (None, 256, 47872)
KNOBS = {"cu_reserve": (0, 64), "nt_tile_h": (0, 224, 240, 256), "gemm_nt8": (0, 1), "gemm_persistent": (0, 1), "gemm_tile": (0, 128, 256),
         "gemm_ring": (0, 1, 2), "nt_grid": (0, 2), "nt_big_min": (0, 1)}


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def cdiv(a, b):
    return (a + b - 1) // b


def old_launch(M, N, K, m_split, t, slots):
    """what the old gemm_nt_launch started for one call (no 4-GiB row split): FIELDS as a tuple.  t: the knobs, slots: avs_persistent_cu_slots()"""
    force = t["gemm_tile"]
    big_tiles = cdiv(M, 256) * (N // 256)
    # nt_use_big
    big_min = t["nt_big_min"] if t["nt_big_min"] > 0 else slots // 2
    big = (N % 256 == 0) if force == 256 else False if force == 128 else (N % 256 == 0 and big_tiles >= big_min)
    if not big:
        # launch_small; nt_small_family(M, N, K, whole = a.m_full >= M: always true here)
        nwg = cdiv(M, 128) * (N // 128)
        if t["gemm_ring"] == 2 and 2 * nwg <= slots:
            nh = cdiv(M, 64) * (N // 128)
            if K >= 256:
                return (RING_HALF, nh, 256, 98304, 0, M, nh, FAM_RING_HALF)
            return (TWOBUF128_HALF, nh, 256, 65536, 0, 0, nh, FAM_TWOBUF_HALF)            # (the copy with m_full = 0)
        if t["gemm_ring"] and nwg <= slots and K >= 256:
            return (RING, nwg, 256, 131072, 0, M, nwg, FAM_RING)
        return (TWOBUF128, nwg, 256, 65536, 0, M, nwg, FAM_TWOBUF)
    ncu = slots
    nt_n, nt_m = N // 256, cdiv(M, 256)
    persistent = t["gemm_persistent"]
    m_full = M
    if persistent and force == 0 and big_tiles > ncu:
        rows_full = ((big_tiles // ncu) * ncu) // nt_n
        if rows_full >= 1 and rows_full < nt_m and (big_tiles % ncu) * 2 <= ncu:
            m_full = rows_full * 256
    if t["gemm_nt8"] >= 1 and K >= 128 and persistent and force == 0:
        one_set = m_split >= M or m_split <= 0
        unit = nt_n * 8 // math.gcd(nt_n, 8)
        h = t["nt_tile_h"]
        tb = -1
        if one_set and h == 224:
            tb = 0
        elif one_set and h == 240:
            tb = ((nt_m // 2) * nt_n // unit) * unit
        elif h == 0:
            rounds = cdiv(nt_m * nt_n, ncu)
            nrt = (rounds * ncu) // nt_n
            num = nrt * 256 - M
            b = num // 32 if num >= 0 else -((-num) // 32)            # C division truncates
            if b > nrt:
                b = nrt
            if b > 0:
                ta = ((nrt - b) * nt_n + unit - 1) // unit * unit
                if not one_set and ta // nt_n * 256 < m_split:
                    ta = cdiv(cdiv(m_split, 256) * nt_n, unit) * unit
                if ta // nt_n <= nrt:
                    na = ta // nt_n
                    nb = cdiv(M - (na * 256 if na * 256 < M else M), 224)
                    nbig, nall = cdiv(ta, ncu), cdiv((na + nb) * nt_n, ncu)
                    cost = nbig + 0.90 * (nall - nbig)
                    if nb > 0 and nall <= rounds and cost < 0.98 * rounds:
                        tb = ta
        rest = M - (tb // nt_n) * 256 if tb >= 0 else 0
        tiles8 = nt_m * nt_n if tb < 0 else tb + cdiv(rest if rest > 0 else 0, 224) * nt_n
        grid8 = tiles8 if tiles8 < ncu else ncu
        gcap = t["nt_grid"]
        if gcap > 0 and gcap < grid8:
            grid8 = gcap
        # the 8-phase launch passes `a` (m_full = M), not the copy with the leftover rows
        return (NT8_TWO if tb >= 0 else NT8_ONE, grid8, 512, 131072, 0 if tb < 0 else tb, M, tiles8, FAM_PERSISTENT)
    tiles_b = cdiv(m_full, 256) * nt_n + (cdiv(M - m_full, 128) * nt_n if m_full < M else 0)
    grid = (tiles_b if tiles_b < ncu else ncu) if persistent else tiles_b
    return (TWOBUF256, grid, 512, 131072, 0, m_full, tiles_b, FAM_PERSISTENT)


def launch_plan(lib, M, N, K, m_split, out=None):
    out = out if out is not None else (ctypes.c_int * len(FIELDS))()
    assert lib.avs_gemm_nt_launch_plan(M, N, K, m_split, out, len(FIELDS)) == 0
    return tuple(out)


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


def test_launch_plan_equals_the_old_launcher_everywhere(lib):
    names = list(KNOBS)
    old = {k: _lib.tuning_get(k) for k in names}
    out = (ctypes.c_int * len(FIELDS))()
    fn = lib.avs_gemm_nt_launch_plan
    shapes = list(itertools.product(MS, NS, KS, M_SPLITS))
    bad, n = [], 0
    try:
        for values in itertools.product(*KNOBS.values()):
            t = dict(zip(names, values))
            for k, v in t.items():
                _lib.tuning_set(k, v)
            slots = lib.avs_persistent_cu_slots()
            for M, N, K, ms in shapes:
                assert fn(M, N, K, ms or 0, out, len(FIELDS)) == 0
                want = old_launch(M, N, K, ms or ONE_SET, t, slots)
                n += 1
                if tuple(out) != want and len(bad) < 8:
                    bad.append(((M, N, K, ms), t, dict(zip(FIELDS, out)), dict(zip(FIELDS, want))))
    finally:
        for k, v in old.items():
            _lib.tuning_set(k, v)
    assert n == len(shapes) * math.prod(len(v) for v in KNOBS.values()) == 829440
    assert not bad, bad


# (M, N, K), knobs, m_split -> kernel, tb, m_full, tiles, grid: computed by hand from the old launcher's text, for 256 slots
ANCHORS = (
    ((95630, 768, 768), {}, 0, NT8_TWO, 24, 95630, 1278, 256),                      # the headline shape: 24 + 1254 tiles = 5 full rounds
    ((95630, 768, 768), {}, 47872, NT8_TWO, 576, 95630, 1200, 256),                 # two towers: the 256-row class covers the first
    ((95630, 768, 768), {"gemm_nt8": 0}, 0, TWOBUF256, 0, 87296, 1221, 256),        # 4 whole rounds of 256^2 tiles, the rest 128 x 256
    ((95630, 3072, 768), {}, 0, NT8_ONE, 0, 95630, 4488, 256),
    ((11328, 768, 3072), {}, 0, NT8_TWO, 0, 11328, 153, 153),                       # (avs_gemm_nt_plan says 135 here: 256-row tiles)
    ((600, 2048, 128), {"nt_big_min": 1, "nt_tile_h": 240}, 0, NT8_TWO, 8, 600, 24, 24),
)


def test_launch_plan_anchors(lib):
    slots = lib.avs_persistent_cu_slots()
    assert slots == 256 or slots > 8                                   # 256 without a device (the default) and on MI355X
    if slots == 256:
        for (M, N, K), kn, ms, kernel, tb, m_full, tiles, grid in ANCHORS:
            with knobs(**kn):
                got = dict(zip(FIELDS, launch_plan(lib, M, N, K, ms)))
            want = dict(kernel=kernel, grid=grid, block=512, lds=131072, tb=tb, m_full=m_full, tiles=tiles, family=FAM_PERSISTENT)
            assert got == want, ((M, N, K), kn, ms)
    # the small kernels' workgroup size and LDS
    with knobs(gemm_tile=128, gemm_ring=2):
        assert launch_plan(lib, 600, 512, 320, 0) == (RING_HALF, 40, 256, 98304, 0, 600, 40, FAM_RING_HALF)
        assert launch_plan(lib, 600, 512, 128, 0) == (TWOBUF128_HALF, 40, 256, 65536, 0, 0, 40, FAM_TWOBUF_HALF)
    with knobs(gemm_tile=128, gemm_ring=1):
        assert launch_plan(lib, 600, 512, 320, 0) == (RING, 20, 256, 131072, 0, 600, 20, FAM_RING)
    with knobs(gemm_tile=128, gemm_ring=0):
        assert launch_plan(lib, 600, 512, 320, 0) == (TWOBUF128, 20, 256, 65536, 0, 600, 20, FAM_TWOBUF)


def test_family_plan_is_a_view_of_the_launch_plan(lib):
    """avs_gemm_nt_plan: the launch plan's coarse family; its workgroups are the launch's grid for the 128 x 128 kernels and the documented
    min(256-row tiles, slots) for the persistent family - where the real grid may differ (two tile heights, nt_grid, gemm_persistent = 0)."""
    slots = lib.avs_persistent_cu_slots()
    fam, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
    for kn in ({}, {"gemm_ring": 0}, {"nt_big_min": 1}, {"gemm_tile": 256, "gemm_persistent": 0}):
        with knobs(**kn):
            for M, N, K in itertools.product(MS, NS, KS):
                p = dict(zip(FIELDS, launch_plan(lib, M, N, K, 0)))
                assert lib.avs_gemm_nt_plan(M, N, K, ctypes.byref(fam), ctypes.byref(wgs)) == 0
                assert fam.value == p["family"]
                assert wgs.value == (min(cdiv(M, 256) * (N // 256), slots) if fam.value == FAM_PERSISTENT else p["grid"])


def test_launch_plan_arguments(lib):
    out = (ctypes.c_int * 16)(*([-7] * 16))
    assert lib.avs_gemm_nt_launch_plan(600, 512, 128, 0, out, 3) == 0              # a shorter array receives the leading fields only
    assert list(out)[3:] == [-7] * 13 and list(out)[:3] == list(launch_plan(lib, 600, 512, 128, 0))[:3]
    assert lib.avs_gemm_nt_launch_plan(600, 512, 128, 0, out, 16) == 0             # a longer one is written up to the fields that exist
    assert list(out)[:len(FIELDS)] == list(launch_plan(lib, 600, 512, 128, 0)) and list(out)[len(FIELDS):] == [-7] * (16 - len(FIELDS))
    assert launch_plan(lib, 600, 512, 128, 600) == launch_plan(lib, 600, 512, 128, 0) == launch_plan(lib, 600, 512, 128, -1)
    for args in ((100, 100, 64, 0, out, 8), (100, 128, 32, 0, out, 8), (0, 128, 64, 0, out, 8), (100, 128, 64, 0, None, 8), (100, 128, 64, 0, out, 0)):
        assert lib.avs_gemm_nt_launch_plan(*args) == -2
        assert b"gemm_nt_launch_plan" in lib.avs_last_error()
