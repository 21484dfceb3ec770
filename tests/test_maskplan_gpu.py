"""The mask-plan kernel (csrc/maskplan.hip: which tokens every training step sees) against maskplan.plan_reference, its numpy restatement,
bit for bit - every comparison here is ==, the kernel's arithmetic (integer Philox, 24-bit floats, comparisons) is exact.  The restatement's
law is tests/test_maskplan_cpu.py's business.

Kernel level: one launch with many DIFFERENT sequences whose output regions lie in a shuffled order inside sentinel-filled buffers with guard
bands (tests/planlib.py), some sequences without a decoder part or without ids; the whole buffers are compared, so a write into a neighbour's
region, into a guard band or for a sequence that has no such output shows.  Engine level: one forward of a one-layer model with device-drawn
plans; the engine's device arrays against the restatement of (its descriptors, the key it handed the kernel), then against the engine's own host
derivation of the same layout (_set_plan).

What the kernel-level tests catch - checked by hand: an emulation of the kernel's loops with one of these changes, in the kernel's place,
against the unchanged restatement (which is the same as damaging the restatement) - and which of them then fail:
  ties broken by descending index                 B (every grid: forced tokens tie at 1.1; all forced = the identity), C, D shuffled, E's unbroken call,
                                                  the golden stream; not A (unstructured noise has no ties to speak of)
  counter words (token, sequence) swapped         every test: no sequence but index 0's token 0 keeps its noise
  tmask_x ignored                                 B at t = 73 / 96 (bits 64, t - 1), C, D shuffled, the golden stream
  bit 31 of tmask_lo sign-extended into 32..63    B at t >= 64 (single bit 31), D shuffled, the golden stream
  mask_off used where dec_off belongs             A, B, C, E's unbroken call: the two regions of a sequence are placed independently
  key halves swapped                              every test but C's seeds 0 and 2^64 - 1
A padded size taken as the next power of two above L + 1 changes no output as long as the network still sorts (and does not fit the kernel's
1024-element arrays at L = 1024): case A's lengths at the network sizes are there for a mis-sorted or mis-padded network, not for that."""
import copy

import numpy as np
import pytest
import torch

from tests import planlib
from tests.planlib import SENTINEL

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _dev_buffers(sizes):
    return {k: torch.full((max(n, 1),), SENTINEL, dtype=torch.float32 if k == "mask" else torch.int32, device=DEV) for k, n in sizes.items()}


def _args(d, sizes, bits=(None, None, None)):
    """keyword arguments of ops.mask_plan for table d with fresh sentinel-filled buffers (grouped when the table's sizes say so)"""
    b = _dev_buffers(sizes)
    a = dict(seqs_dev=_dev(d), seqs_host=d, row_src=b["row_src"], row_tok=b["row_tok"], src_row=b["src_row"], mask_out=b["mask"], ids_out=b["ids"],
             seed_dev=None, grouped=(b["pos_row"], b["row_of_pos"], b["pred_id"]) if "pos_row" in b else None)
    for k, v in zip(("tmask_lo", "tmask_hi", "fmask"), bits):
        a[k] = _dev(v) if v is not None else None
    return a, b


def _launch(d, seed, sizes, bits=(None, None, None), seed_dev=False):
    """-> the buffers after one launch, as numpy.  seed_dev: the key travels in an int64 device tensor holding the same 64 bits"""
    a, b = _args(d, sizes, bits)
    if seed_dev:
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        a["seed_dev"] = torch.tensor([s - (1 << 64) if s >> 63 else s], dtype=torch.int64, device=DEV)
        seed = None
    ops().mask_plan(seed=seed, **a)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items()}


def _same(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        if not np.array_equal(got[k], want[k]):
            i = int(np.flatnonzero(got[k] != want[k])[0])
            raise AssertionError(f"{what} {k}: {int((got[k] != want[k]).sum())} elements differ, first at {i}: kernel {got[k][i]}, restatement {want[k][i]}")


def _check(d, seed, sizes, bits=(None, None, None), what="", **kw):
    got = _launch(d, seed, sizes, bits, **kw)
    _same(got, planlib.reference(d, seed, sizes, bits), what)
    return got


def _words(tbits, fbits):
    """96 time bits + 32 frequency bits -> (tmask_lo, tmask_hi, tmask_x, fmask) as int32 (bit 31 set: negative)"""
    w = np.array([tbits & 0xFFFFFFFF, (tbits >> 32) & 0xFFFFFFFF, (tbits >> 64) & 0xFFFFFFFF, fbits & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return [int(x) for x in w]


# ---- A: lengths and keeps ----------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 196, 255, 256, 257, 511, 512, 513, 657, 1023, 1024)


def test_case_a_lengths_and_keeps():
    """unstructured sequences below, at and above every padded network size (64 .. 1024) and at the model's own 196 / 256 / 657, each with
    keep in {0, 1, L // 4, L - 1, L}: ~80 different sequences in one launch, every fifth without a decoder part, every seventh without ids"""
    seqs = [dict(L=L, keep=k) for L in LENGTHS for k in sorted({0, 1, L // 4, L - 1, L})]
    for i, s in enumerate(seqs):
        s["dec"], s["ids"] = i % 5 != 3, i % 7 != 2
    assert 70 <= len(seqs) <= 100
    d, sizes = planlib.classic_table(seqs, seed=1)
    got = _check(d, 0x00C0FFEE12345678, sizes, what="case A")
    # nothing of a sequence without a decoder part / without ids anywhere: the written elements are exactly the others' regions
    assert int((got["src_row"] != SENTINEL).sum()) == int((got["mask"] != SENTINEL).sum()) == sum(s["L"] for s in seqs if s["dec"])
    assert int((got["ids"] != SENTINEL).sum()) == sum(s["L"] for s in seqs if s["ids"])
    assert int((got["row_tok"] != SENTINEL).sum()) == sum(s["keep"] for s in seqs)


# ---- B: structured grids -----------------------------------------------------------------------------------------------------------------------
def _structured_sets(t, f, rng):
    """(time set, frequency set, keep) of the structured sequences of one grid"""
    L, all_t, all_f = t * f, (1 << t) - 1, (1 << f) - 1
    forced = lambda tb, fb: (bin(tb & all_t).count("1") * f + bin(fb & all_f).count("1") * t
                             - bin(tb & all_t).count("1") * bin(fb & all_f).count("1"))
    rand_t = lambda: int.from_bytes(rng.bytes(12), "little") & int.from_bytes(rng.bytes(12), "little") & all_t       # ~ a quarter of the columns
    rand_f = lambda: int.from_bytes(rng.bytes(4), "little") & int.from_bytes(rng.bytes(4), "little") & all_f
    sets = [(0, 0, L // 4), (all_t, all_f, L // 3), (all_t, 0, L - 1), (0, all_f, L)]          # empty; everything forced (3 ways): the identity
    sets += [(1 << b, 0, L // 2) for b in sorted({0, 31, 32, 63, 64, t - 1}) if b < t]       # single time bits at the word boundaries
    sets += [(0, 1 << b, L // 2) for b in sorted({0, f - 1})]                                 # single frequency bits (bit 31 at f = 32)
    tb, fb = rand_t(), rand_f()
    sets += [(tb, fb, min(max(L - forced(tb, fb) + e, 0), L)) for e in (-1, 0, 1)]             # forced count == L - keep and one either side
    sets += [(rand_t(), rand_f(), int(rng.integers(0, L + 1))) for _ in range(2)]             # random sets
    stale_t, stale_f = ((1 << 96) - 1) & ~all_t, 0xFFFFFFFF & ~all_f
    sets += [(rand_t() | stale_t, rand_f() | stale_f, L // 2), (stale_t, stale_f, L // 4)]       # stale bits at positions >= t / >= f: ignored
    return sets


@pytest.mark.parametrize("t,f", [(64, 8), (73, 9), (96, 10), (32, 32), (16, 8), (1, 32), (96, 1)])
def test_case_b_structured_grids(t, f):
    """an [f][t] grid with every kind of bit set (see _structured_sets), between unstructured sequences whose slots of the bit arrays and whose
    tmask_x hold garbage that must be ignored"""
    rng = np.random.default_rng(1000 * t + f)
    seqs, tl, th, fm = [], [], [], []
    for i, (tb, fb, keep) in enumerate(_structured_sets(t, f, rng)):
        if i % 6 == 0:                                       # an unstructured sequence: all-ones garbage at its slot and in its tmask_x
            seqs.append(dict(L=t * f, keep=(t * f) // 4, t=0, tx=-1, dec=i % 12 == 0))
            tl.append(-1); th.append(-1); fm.append(-1)
        lo, hi, x, fw = _words(tb, fb)
        seqs.append(dict(L=t * f, keep=keep, t=t, tx=x, dec=i % 5 != 3, ids=i % 7 != 5))
        tl.append(lo); th.append(hi); fm.append(fw)
    d, sizes = planlib.classic_table(seqs, seed=t + f)
    bits = tuple(np.array(v, dtype=np.int32) for v in (tl, th, fm))
    got = _check(d, 0x0BADC0DE00000000 | (t << 8) | f, sizes, bits, what=f"case B {t}x{f}")
    # everything forced -> the order is the identity, the kept tokens are 0 .. keep - 1 (sequences 1, 2, 3 after the leading unstructured one and the empty set)
    for sq in (2, 3, 4):
        assert seqs[sq]["t"] == t and int(d[sq, 7]) >= 0
        assert np.array_equal(got["ids"][int(d[sq, 7]):int(d[sq, 7]) + t * f], np.arange(t * f))
        assert np.array_equal(got["row_tok"][int(d[sq, 2]):int(d[sq, 2]) + int(d[sq, 1])], np.arange(int(d[sq, 1])))


# ---- C: keys and entry points ------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 1 << 32, 0xFFFFFFFF, 0xFFFFFFFF00000000, 1 << 63, (1 << 64) - 1, (123 << 32) | 7)


@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
def test_case_c_keys_and_entry_points(seed):
    """one key through avs_mask_plan, avs_mask_plan_dev (the key in device memory: an int64 holding the same bits, negative from 1 << 63 on),
    avs_mask_plan_grouped with the value and with seed_dev: identical draws (row_src, row_tok, ids, mask byte for byte; src_row within each
    layout), each equal to the restatement.  The same descriptor at index 0 and index 5 draws different noise (counter word 1 = the index)."""
    seqs = [dict(L=196, keep=49), dict(L=64, keep=16, t=16), dict(L=129, keep=128), dict(L=657, keep=164, t=73, tx=0x1FF), dict(L=1, keep=1),
            dict(L=196, keep=49), dict(L=100, keep=0, dec=False), dict(L=256, keep=64, ids=False)]
    bits = tuple(np.array(v, dtype=np.uint32).view(np.int32) for v in ([0, 0x8421] + [0] * 6, [0] * 3 + [0x80000001] + [0] * 4, [0, 0x81, 0, 0x101] + [0] * 4))
    dc, sc = planlib.classic_table(seqs, seed=5)
    dg, sg = planlib.grouped_table(seqs, seed=5)
    assert np.array_equal(dc[:, :12], dg[:, :12])
    runs = [_check(dc, seed, sc, bits, what="avs_mask_plan"), _check(dc, seed, sc, bits, what="avs_mask_plan_dev", seed_dev=True),
            _check(dg, seed, sg, bits, what="avs_mask_plan_grouped"), _check(dg, seed, sg, bits, what="avs_mask_plan_grouped(seed_dev)", seed_dev=True)]
    for r in runs[1:]:
        for k in ("row_src", "row_tok", "ids", "mask"):
            assert r[k].tobytes() == runs[0][k].tobytes(), k
    assert runs[1]["src_row"].tobytes() == runs[0]["src_row"].tobytes()
    for k in ("src_row", "pos_row", "row_of_pos", "pred_id"):
        assert runs[3][k].tobytes() == runs[2][k].tobytes(), k
    i0, i5 = (runs[0]["ids"][int(dc[s, 7]):int(dc[s, 7]) + 196] for s in (0, 5))
    assert sorted(i0.tolist()) == sorted(i5.tolist()) == list(range(196)) and not np.array_equal(i0, i5)


# ---- D: grouped layout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,kv", [(32, 49), (1, 195), (127, 1)])
def test_case_d_grouped_layout_of_the_mae_pass(ka, kv):
    """B = 3, T = 2, La = 128, Lv = 196 in the MAE pass's own table ([removed audio | removed frames | kept audio | kept frames] per sample), at
    the model's keeps and at keep = 1 / keep = L - 1: all eight arrays"""
    d, sizes = planlib.engine_grouped_table(3, 2, 128, 196, ka, kv)
    got = _check(d, 0xFEED1234 + ka, sizes, what="case D")
    assert all((v != SENTINEL).all() for v in got.values())                  # the table covers every element of every array


def test_case_d_grouped_regions_in_shuffled_order():
    """the grouped layout with the removed rows, kept rows, positions and prediction rows of every sequence placed independently, keep = 0 and
    keep = L (an empty region) included, a structured sequence and sequences without a decoder part among them"""
    seqs = [dict(L=128, keep=32), dict(L=196, keep=0), dict(L=64, keep=64), dict(L=65, keep=1, dec=False), dict(L=657, keep=164, t=73, tx=0x100),
            dict(L=256, keep=255), dict(L=1, keep=0), dict(L=1, keep=1), dict(L=513, keep=128, ids=False), dict(L=30, keep=7, dec=False, ids=False)]
    d, sizes = planlib.grouped_table(seqs, seed=9)
    bits = tuple(np.array([0] * 4 + [v] + [0] * 5, dtype=np.uint32).view(np.int32) for v in (0x80000000, 0x1, 0x100))
    _check(d, 0x7777000000000001, sizes, bits, what="case D shuffled")


# ---- E: refusals -------------------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    """(name, grouped table?, roomy buffers?, edit(d, a)): one broken thing each; sequence 0 is structured (64 = 4 x 16), all but sequence 2 have a decoder part"""
    def past(field, key, length):                     # offset `field` of sequence 1 so that its region ends one element past buffer `key`
        def edit(d, a):
            buf = a[key] if not isinstance(key, int) else a["grouped"][key]
            d[1, field] = buf.numel() - length(d) + 1
        return edit
    def put(sq, **fields):
        def edit(d, a):
            for k, v in fields.items():
                d[sq, int(k[1:])] = v
        return edit
    def arg(**kw):
        return lambda d, a: a.update(kw)
    L1, keep1 = (lambda d: int(d[1, 0])), (lambda d: int(d[1, 1]))
    nm1 = lambda d: int(d[1, 0] - d[1, 1])
    short = lambda k: (lambda d, a: a.update({k: a[k][:d.shape[0] - 1]}))
    C, G = False, True
    return [
        ("L = 0", C, False, put(1, f0=0, f1=0)), ("L = 1025", C, True, put(1, f0=1025)), ("keep = -1", C, False, put(1, f1=-1)),
        ("keep > L", C, True, put(1, f1=101)), ("row_off < 0", C, False, put(1, f2=-1)), ("row_off + keep past row_src", C, False, past(2, "row_src", keep1)),
        ("row_off + keep past row_tok", C, False, lambda d, a: a.update(row_tok=a["row_tok"][:int((d[:, 2] + d[:, 1]).max()) - 1])),
        ("decoder sequence without src_row", C, False, arg(src_row=None)), ("decoder sequence without mask_out", C, False, arg(mask_out=None)),
        ("dec_off + L past src_row", C, False, past(4, "src_row", L1)), ("mask_off + L past mask_out", C, False, past(8, "mask_out", L1)),
        ("mask_off < 0", C, False, put(1, f8=-1)), ("ids_off + L past ids_out", C, False, past(7, "ids_out", L1)), ("ids wanted without ids_out", C, False, arg(ids_out=None)),
        ("structured without tmask_lo", C, False, arg(tmask_lo=None)), ("structured without tmask_hi", C, False, arg(tmask_hi=None)),
        ("structured without fmask", C, False, arg(fmask=None)), ("tmask_lo shorter than nseq", C, False, short("tmask_lo")),
        ("tmask_hi shorter than nseq", C, False, short("tmask_hi")), ("fmask shorter than nseq", C, False, short("fmask")),
        ("t_patches = 97", C, True, put(0, f0=97, f6=97)), ("L not a multiple of t_patches", C, False, put(0, f6=15)), ("L / t_patches = 33", C, False, put(0, f0=33, f6=1)),
        ("grouped descriptors without the three arrays", G, False, arg(grouped=None)), ("a classic descriptor among grouped decoder sequences", G, False, put(1, f12=-1)),
        ("dec_k_off < 0", G, False, put(1, f13=-1)), ("pred_off < 0", G, False, put(1, f14=-1)), ("pos_base < 0", G, False, put(1, f15=-1)),
        ("dec_m_off + (L - keep) past src_row", G, False, past(12, "src_row", nm1)), ("pred_off + (L - keep) past pred_id", G, False, past(14, 2, nm1)),
        ("dec_m_off + (L - keep) past pos_row", G, False, lambda d, a: a.update(grouped=(a["grouped"][0][:int((d[:, 12] + d[:, 0] - d[:, 1])[[1, 3]].max()) - 1],) + a["grouped"][1:])),
        ("seed_dev int32", C, False, lambda d, a: a.update(seed_dev=torch.zeros(2, dtype=torch.int32, device=DEV))),
        ("seed_dev int32, grouped", G, False, lambda d, a: a.update(seed_dev=torch.zeros(2, dtype=torch.int32, device=DEV))),
        ("seed_dev float64", C, False, lambda d, a: a.update(seed_dev=torch.zeros(1, dtype=torch.float64, device=DEV))),
    ]


def test_case_e_refusals():
    """ops.mask_plan checks every offset on the host copy of the table before the launch: each broken call is refused, and nothing was
    launched - the buffers still hold their sentinels.  The unbroken call of either flavour goes through (so it is the edit that is refused)."""
    from avsiam_amd import _lib
    o = ops()
    seqs = [dict(L=64, keep=16, t=16), dict(L=100, keep=25), dict(L=50, keep=10, dec=False), dict(L=70, keep=69)]
    bits = tuple(np.array([v, 0, 0, 0], dtype=np.int32) for v in (0x11, 0, 0x2))
    tables = {False: planlib.classic_table(seqs, seed=2), True: planlib.grouped_table(seqs, seed=2)}
    for d, sizes in tables.values():
        _check(d, 42, sizes, bits, what="unbroken")
    for name, grouped, roomy, edit in _refusal_cases():
        d, sizes = tables[grouped]
        d = d.copy()
        a, b = _args(d, {k: 8192 for k in sizes} if roomy else sizes, bits)
        edit(d, a)
        a["seqs_dev"] = _dev(d)
        with pytest.raises((AssertionError, _lib.AvsiamHipError)):
            o.mask_plan(seed=42, **a)
            pytest.fail(f"not refused: {name}")
        torch.cuda.synchronize()
        assert all(bool((v == SENTINEL).all()) for v in b.values()), name


# ---- the golden stream -------------------------------------------------------------------------------------------------------------------------
def test_golden_stream_holds_the_kernel(golden_dir):
    """tests/golden/plan_stream_v1.npz (written by the restatement, tools/gen_golden_plan_stream.py): the kernel draws the recorded shuffles -
    changing kernel and restatement together changes every run's mask stream and fails here and in tests/test_maskplan_cpu.py"""
    g = np.load(golden_dir + "/plan_stream_v1.npz")
    d, sizes = planlib.stream_case()[:2]
    assert np.array_equal(g["desc"], d)
    bits = (g["tmask_lo"], g["tmask_hi"], g["fmask"])
    for k, key in enumerate(g["keys"]):
        got = _launch(d, int(key), sizes, bits)
        ids = np.concatenate([got["ids"][int(o):int(o) + int(L)] for L, o in zip(d[:, 0], d[:, 7])])
        assert np.array_equal(ids, g["ids"][k].astype(np.int32)), hex(int(key))


# ---- engine level ------------------------------------------------------------------------------------------------------------------------------
def _model(cfg, B, which, plan_seed, **kw):
    """a one-layer model, its pass engine with draw_device wrapped to record the key it is handed, and inputs"""
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.weights import synth_inputs
    m = CAVMAE_BASE(cfg=cfg, init_seed=11, init_mode="random", verbose=False, plan_seed=plan_seed, **kw).cuda()
    eng = m._engine(which, B)
    keys, inner = [], eng.draw_device

    def draw_device(seed, *a, **k):
        keys.append(seed)
        return inner(seed, *a, **k)
    eng.draw_device = draw_device
    a, v = synth_inputs(cfg, B, 3)
    return m, eng, keys, a.cuda(), v.cuda()


def _engine_arrays(eng, names):
    torch.cuda.synchronize()
    return {n: getattr(eng, a).detach().cpu().numpy().copy() for n, a in names.items()}


def _restated(eng, key, arrays):
    """plan_reference of (the engine's descriptors, the key the kernel got, its bit arrays) into sentinel buffers of the engine arrays' sizes"""
    from avsiam_amd.maskplan import plan_reference
    bits = tuple(eng.bits_host) if hasattr(eng, "bits_host") else (None, None, None)
    out = {n: np.full(v.shape, SENTINEL, dtype=v.dtype) for n, v in arrays.items()}
    plan_reference(eng.desc_host, key, *bits, out=out)
    assert all((v != SENTINEL).all() for v in out.values())                  # the engine's table covers every element of its arrays
    return out


def _scribble(eng, names):
    for a in names.values():
        getattr(eng, a).fill_(SENTINEL)


MAE_ARRAYS = {"row_src": "row_src_all", "row_tok": "row_tok_all", "ids": "ids_dev", "src_row": "src_row", "mask": "mask_all"}
MAE_GROUPED = {"pos_row": "pos_row", "row_of_pos": "row_of_pos", "pred_id": "pred_id"}


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("shape", ["base_La128_T2_B3", "huge14_T1_B2"])
def test_mae_pass_device_plan_is_the_restatement_and_the_host_derivation(shape, prune):
    """one forward of the MAE pass with a device-drawn plan: row_src / row_tok / ids / src_row / mask (pruned: + pos_row / row_of_pos / pred_id)
    equal the restatement of (desc_host, the key draw_device was handed); then _set_plan(last_plan()) - the host derivation of the same layout
    from the plan read back - rewrites every array bitwise as the kernel wrote it"""
    from avsiam_amd.config import AVSiamConfig, EngineOptions, vit_huge14
    if shape.startswith("base"):
        cfg, B = AVSiamConfig(audio_tokens=128, frames=2, depth=1, dec_depth=1), 3
    else:
        cfg, B = vit_huge14(frames=1, depth=1, dec_depth=1), 2
    m, eng, keys, a, v = _model(cfg, B, "mae", 2024, options=EngineOptions(prune_dead=prune))
    assert eng.prune == prune
    m(a, v, mae_loss_weight=1, contrast_loss_weight=0)
    assert len(keys) == 1 and keys[0] is not None
    names = dict(MAE_ARRAYS, **(MAE_GROUPED if prune else {}))
    drawn = _engine_arrays(eng, names)
    _same(drawn, _restated(eng, keys[0], drawn), "MAE pass")
    plan = eng.last_plan()
    _scribble(eng, {k: v_ for k, v_ in names.items() if k != "ids"})
    eng._set_plan(plan)
    _same(_engine_arrays(eng, names), drawn, "_set_plan against the kernel:")


def _contrastive_samples(eng, cfg, B):
    """sample -> (group, kept tokens) of the audio sequences and (sample, frame) -> (group, kept tokens) of the video sequences, read from the
    engine's row arrays slot by slot (row ranges are static per slot); slot_maps[0] must send every slot to the sample its rows name"""
    torch.cuda.synchronize()
    T, d = cfg.frames, eng.desc_host
    rs, rt, sm = eng.row_src_all.cpu().numpy(), eng.row_tok_all.cpu().numpy(), eng.slot_maps[0].cpu().numpy()
    assert sorted(sm.tolist()) == list(range(2 * B))
    audio, video = {}, {}
    for sl in range(B):
        g = int(eng.slot_group[sl])
        off, keep = int(d[sl, 2]), int(d[sl, 1])
        assert keep > 0 and (rs[off:off + keep] == rs[off]).all()
        assert sm[sl] == rs[off]
        audio[int(rs[off])] = (g, rt[off:off + keep].tolist())
        for t in range(T):
            off, keep = int(d[B + sl * T + t, 2]), int(d[B + sl * T + t, 1])
            assert keep > 0 and (rs[off:off + keep] == rs[off]).all() and rs[off] % T == t
            assert sm[B + sl] == B + rs[off] // T
            video[(int(rs[off]) // T, t)] = (g, rt[off:off + keep].tolist())
    assert sorted(audio) == list(range(B)) and sorted(video) == [(b, t) for b in range(B) for t in range(T)]
    return audio, video


@pytest.mark.parametrize("shape,B", [("base_La128", 3), ("base_La128", 6), ("base_La128", 10), ("huge14", 6)])
def test_contrastive_pass_device_plan_is_the_restatement_and_the_host_draw(shape, B):
    """one forward of the contrastive pass with a device-drawn plan (B = 3 and 6: fewer than five groups; huge-14: 73 time columns, tmask_x
    live): bits_host and the descriptors' src_id / tmask_x are what draw_structured returns from a generator in the same state; row_src / row_tok /
    ids equal the restatement of (desc_host, the recorded key, bits_host); _set_plan(last_plan()) orders the slots of a group differently, so
    per sample: the same (group, kept tokens) for audio and every frame, and slot_maps[0] follows the rows"""
    from avsiam_amd.config import AVSiamConfig, vit_huge14
    from avsiam_amd.maskplan import draw_structured, group_sizes
    cfg = AVSiamConfig(audio_tokens=128, depth=1, dec_depth=1) if shape == "base_La128" else vit_huge14(frames=1, depth=1, dec_depth=1)
    m, eng, keys, a, v = _model(cfg, B, "contrastive", 77 + B)
    T = cfg.frames
    twin = copy.deepcopy(m._np_rng())
    m(a, v, mae_loss_weight=0, contrast_loss_weight=1)
    assert len(keys) == 1 and keys[0] is not None
    assert np.bincount(eng.slot_group).tolist() == group_sizes(B)
    perm_a, perm_v, bits, tx = draw_structured(cfg, eng.slot_group, twin)
    d = eng.desc_host
    assert np.array_equal(eng.bits_host[:, :B], bits) and not eng.bits_host[:, B:].any()
    assert np.array_equal(d[:B, 3], perm_a) and np.array_equal(d[B:, 3], (perm_v[:, None] * T + np.arange(T)[None, :]).reshape(-1))
    assert np.array_equal(d[:B, 9], tx) and not d[B:, 9].any()
    if shape == "huge14":
        assert tx.any()                                                       # (this generator state picks columns 64 .. 72)
    names = {"row_src": "row_src_all", "row_tok": "row_tok_all", "ids": "ids_dev"}
    drawn = _engine_arrays(eng, names)
    _same(drawn, _restated(eng, keys[0], drawn), "contrastive pass")
    by_device = _contrastive_samples(eng, cfg, B)
    plan = eng.last_plan()
    _scribble(eng, {"row_src": "row_src_all", "row_tok": "row_tok_all", "slot_maps": "slot_maps"})
    eng._set_plan(plan)
    assert _contrastive_samples(eng, cfg, B) == by_device
