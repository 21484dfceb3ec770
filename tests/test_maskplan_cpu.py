"""The law of the device-drawn mask plans, on the CPU: maskplan.plan_reference (the numpy restatement tests/test_maskplan_gpu.py holds the kernel
to, bit for bit) and maskplan.draw_structured (the host part of the contrastive draw) against the project's host generators on the same noise, and
against the distribution of make_contrastive_plan - the generator with the reference's draws (random.sample, torch.rand, randperm + chunk).

Every seed is fixed, so every outcome is deterministic.  Every z-statistic is held to |z| < Z_MAX = 5: a cap, not a measurement - the expected
maximum of ~2600 standard normal cells is about 3.5, a bias of a few percent of a cell at N = 600 lies beyond 5.  The worst |z| of each test goes to
test_out/plan_stats.json (committed as profiles/r16/plan_stats.json)."""
import math
import random

import numpy as np
import pytest
import torch

from tests import planlib
from avsiam_amd import maskplan as mp
from avsiam_amd.config import AVSiamConfig, vit_huge14

Z_MAX = 5.0


def _table(seqs, seed=0, grouped=False):
    return (planlib.grouped_table if grouped else planlib.classic_table)(seqs, seed)


def _u32(*v):
    return np.array(v, dtype=np.uint32).view(np.int32)


# ---- plan_reference against the host generators on the same noise ------------------------------------------------------------------------------
def test_noise_is_the_philox_stream_in_24_bits():
    """word 0 of Philox4x32-10 at counter (token, sequence, 0, 0), key (seed low, seed high) - tied to the Random123 vectors by
    tests/test_ft_aug_cpu.py - top 24 bits, exactly representable in float32, in [0, 1)"""
    from avsiam_amd.preprocess import philox4x32_10
    seed = 0xFEDCBA9876543210
    n = mp.plan_noise(300, 5, seed)
    assert n.dtype == np.float32 and n.min() >= 0 and n.max() < 1
    for i in (0, 1, 299):
        w = int(philox4x32_10(i, 5, 0, 0, 0x76543210, 0xFEDCBA98)[()])
        assert n[i] == np.float32((w >> 8) / 16777216.0)
    assert not np.array_equal(n, mp.plan_noise(300, 4, seed)) and not np.array_equal(n[:5], mp.plan_noise(300, 0, seed)[5:10])   # words 0 / 1 not swapped


@pytest.mark.parametrize("L,keep,t", [(196, 49, 0), (657, 164, 0), (1, 1, 0), (512, 307, 64), (657, 394, 73), (128, 25, 16), (96, 10, 96)])
def test_reference_equals_the_torch_generator_on_its_noise(L, keep, t):
    """the shuffle is maskplan._unstructured (torch's stable argsort twice) of the restatement's noise - with noise[forced] = 1.1 for a structured
    sequence, as make_contrastive_plan / make_mae_plan_regions do -, mask == (ids_restore >= keep), and every classic output follows from it"""
    rng = np.random.default_rng(L + t)
    seqs = [dict(L=7, keep=3), dict(L=L, keep=keep, t=t, tx=int(rng.integers(0, 2 ** 31))), dict(L=9, keep=0)]
    d, sizes = _table(seqs, seed=3)
    bits = tuple(rng.integers(-2 ** 31, 2 ** 31, 3).astype(np.int32) for _ in range(3))
    if t:
        bits[2][1] &= 0x5                                      # (at most two rows, so that free tokens remain)
    seed = 0x1234567800000009
    out = planlib.reference(d, seed, sizes, bits)
    noise = torch.from_numpy(mp.plan_noise(L, 1, seed).copy())
    forced = np.zeros(L, dtype=bool)
    if t:
        forced = mp.plan_forced(L, t, bits[0][1], bits[1][1], d[1, 9], bits[2][1])
        i = np.arange(L)
        tb = (int(bits[0][1]) & 0xFFFFFFFF) | (int(bits[1][1]) & 0xFFFFFFFF) << 32 | (int(d[1, 9]) & 0xFFFFFFFF) << 64
        want = np.array([(tb >> int(c)) & 1 for c in i % t], dtype=bool) | np.array([(int(bits[2][1]) >> int(r)) & 1 for r in i // t], dtype=bool)
        assert np.array_equal(forced, want) and 0 < forced.sum() < L
        noise[torch.from_numpy(forced)] = 1.1
    ids_keep, ids_restore = mp._unstructured(noise, keep)
    ids_shuffle = torch.argsort(noise, stable=True)
    _, _, row_off, src_id, dec_off, enc_base, _, ids_off, mask_off = (int(x) for x in d[1, :9])
    assert np.array_equal(out["ids"][ids_off:ids_off + L], ids_shuffle.numpy())
    assert np.array_equal(out["row_tok"][row_off:row_off + keep], ids_keep.numpy())
    assert (out["row_src"][row_off:row_off + keep] == src_id).all()
    assert np.array_equal(out["mask"][mask_off:mask_off + L], (ids_restore >= keep).float().numpy())
    assert np.array_equal(out["src_row"][dec_off:dec_off + L], torch.where(ids_restore < keep, enc_base + ids_restore, -1).numpy())
    if t:                                                     # forced tokens are kept only when the free ones run out, and then the lowest first
        nfree = int((~forced).sum())
        assert int(forced[ids_keep.numpy()].sum()) == max(0, keep - nfree)
    # nothing but the regions was written
    for k in ("ids", "row_tok", "row_src", "mask", "src_row"):
        touched = out[k] != planlib.SENTINEL
        assert int(touched.sum()) == sum(s["keep"] if k.startswith("row_") else s["L"] for s in seqs)


def test_reference_ties_go_by_index_and_all_forced_is_the_identity():
    d, sizes = _table([dict(L=512, keep=100, t=64), dict(L=96, keep=96, t=96, tx=-1)])
    out = planlib.reference(d, 99, sizes, (_u32(0xFFFFFFFF, 0xFFFFFFFF), _u32(0xFFFFFFFF, 0xFFFFFFFF), _u32(0, 0)))
    for i, L in enumerate((512, 96)):
        o = int(d[i, 7])
        assert np.array_equal(out["ids"][o:o + L], np.arange(L))
    assert np.array_equal(out["row_tok"][int(d[0, 2]):int(d[0, 2]) + 100], np.arange(100))


def test_reference_grouped_arrays_equal_the_engines_host_derivation():
    """engine.MaePass._set_plan derives the grouped decoder layout from an injected plan with torch on the host; its arithmetic (copied: the
    engine cannot be imported without a device) on the plan the restatement drew must give the restatement's arrays, element for element"""
    B, T, La, Lv, ka, kv = 3, 2, 128, 196, 32, 49
    d, sizes = planlib.engine_grouped_table(B, T, La, Lv, ka, kv)
    out = planlib.reference(d, 0xABCDEF0123, sizes)
    ids = torch.from_numpy(out["ids"]).long()
    sa, sv = ids[:B * La].view(B, La), ids[B * La:].view(B, T, Lv)
    ra, rv = torch.argsort(sa, dim=1), torch.argsort(sv, dim=-1)                              # (MaePass.last_plan)
    n_enc, Lt, ma, mv = ka + T * kv, La + T * Lv, La - ka, Lv - kv
    lq = ma + T * mv
    b = torch.arange(B).view(B, 1)
    src_a = torch.where(ra < ka, b * n_enc + ra, torch.full_like(ra, -1))
    t = torch.arange(T).view(1, T, 1)
    src_v = torch.where(rv < kv, b.view(B, 1, 1) * n_enc + ka + t * kv + rv, torch.full_like(rv, -1))
    src = torch.cat([src_a, src_v.reshape(B, T * Lv)], dim=1).reshape(-1)
    bL = b * Lt
    row_a = torch.where(ra < ka, bL + lq + ra, bL + (ra - ka))
    row_v = torch.where(rv < kv, bL.view(B, 1, 1) + lq + ka + t * kv + rv, bL.view(B, 1, 1) + ma + t * mv + (rv - kv))
    rop = torch.cat([row_a, row_v.reshape(B, T * Lv)], dim=1).reshape(-1)
    pos = torch.cat([torch.arange(La), La + torch.arange(Lv).repeat(T)]).repeat(B)
    src_d = torch.empty_like(src)
    src_d[rop] = src
    pos_d = torch.empty(B * Lt, dtype=torch.int64)
    pos_d[rop] = pos
    pid = torch.empty(B * ma + B * T * mv, dtype=torch.int64)
    tok_a = torch.arange(La).view(1, La).expand(B, La)
    sel = ra >= ka
    pid[(b * ma + (ra - ka))[sel]] = (b * La + tok_a)[sel]
    it = (b.view(B, 1, 1) * T + t)
    tok_v = torch.arange(Lv).view(1, 1, Lv).expand(B, T, Lv)
    selv = rv >= kv
    pid[(B * ma + it * mv + (rv - kv))[selv]] = (B * La + it * Lv + tok_v)[selv]
    mask = torch.cat([(ra >= ka).float().reshape(-1), (rv >= kv).float().reshape(-1)])
    for name, want in (("src_row", src_d), ("pos_row", pos_d), ("row_of_pos", rop), ("pred_id", pid), ("mask", mask)):
        assert np.array_equal(out[name], want.numpy().astype(out[name].dtype)), name
    assert np.array_equal(out["row_tok"], torch.cat([sa[:, :ka].reshape(-1), sv[..., :kv].reshape(-1)]).numpy())
    assert np.array_equal(out["row_src"], torch.cat([torch.arange(B).repeat_interleave(ka), torch.arange(B * T).repeat_interleave(kv)]).numpy())


def test_golden_stream_holds_the_restatement(golden_dir):
    """tests/golden/plan_stream_v1.npz: the recorded shuffles of three keys - whoever changes the draw changes every run's masks, on purpose"""
    g = np.load(golden_dir + "/plan_stream_v1.npz")
    desc, bits = planlib.stream_case()[0], planlib.stream_case()[2:]
    assert np.array_equal(g["desc"], desc) and all(np.array_equal(g[k], v) for k, v in zip(("tmask_lo", "tmask_hi", "fmask"), bits))
    assert [int(k) for k in g["keys"]] == list(planlib.STREAM_KEYS)
    for k, key in enumerate(planlib.STREAM_KEYS):
        assert np.array_equal(g["ids"][k], planlib.stream_ids(desc, key, bits)), hex(key)
    L = desc[:, 0]
    assert L[0] == L[7] == 196 and not np.array_equal(g["ids"][0][:196], g["ids"][0][-196:])          # sequence 0 and 7: different noise


# ---- draw_structured ---------------------------------------------------------------------------------------------------------------------------
def _slot_group(B):
    return np.array([g for g, n in enumerate(mp.group_sizes(B)) for _ in range(n)], dtype=np.int64)


def _unpack(bits, tx, t, f):
    """[B, t] / [B, f] bool pick tables from the packed words (Python integers: nothing of numpy's shifts)"""
    B = bits.shape[1]
    m = 0xFFFFFFFF
    tb = [(int(bits[0, s]) & m) | (int(bits[1, s]) & m) << 32 | (int(tx[s]) & m) << 64 for s in range(B)]
    tm = np.array([[(tb[s] >> c) & 1 for c in range(96)] for s in range(B)], dtype=bool)
    fm = np.array([[((int(bits[2, s]) & m) >> r) & 1 for r in range(32)] for s in range(B)], dtype=bool)
    assert not tm[:, t:].any() and not fm[:, f:].any()                # no bit at or above t / f
    return tm[:, :t], fm[:, :f]


@pytest.mark.parametrize("t,f", [(16, 8), (64, 8), (73, 9)])
def test_draw_structured_counts_and_packing(t, f):
    cfg = AVSiamConfig(audio_tokens=t * f, audio_f=f)
    for B in range(1, 13):
        sg = _slot_group(B)
        assert np.bincount(sg).tolist() == mp.group_sizes(B) and sum(mp.group_sizes(B)) == B
        rng = np.random.default_rng(100 + B)
        twin = np.random.default_rng(100 + B)
        perm_a, perm_v, bits, tx = mp.draw_structured(cfg, sg, rng)
        # the generator is advanced by exactly: permutation, permutation, random((B, t)), random((B, f))
        pa, pv, kt, kf = twin.permutation(B), twin.permutation(B), twin.random((B, t)), twin.random((B, f))
        assert np.array_equal(perm_a, pa) and np.array_equal(perm_v, pv) and rng.random() == twin.random()
        assert sorted(perm_a.tolist()) == sorted(perm_v.tolist()) == list(range(B))
        assert bits.shape == (3, B) and bits.dtype == np.int32 and tx.shape == (B,) and tx.dtype == np.int32
        tm, fm = _unpack(bits, tx, t, f)
        for s in range(B):
            r = mp.group_ratio(int(sg[s]))
            nt, nf = int(t * r * 0.7), int(f * r * 0.7)
            assert tm[s].sum() == nt and fm[s].sum() == nf
            # random.sample as "the n smallest of t random keys": the packing round-trips to exactly those columns / rows
            assert sorted(np.flatnonzero(tm[s]).tolist()) == sorted(np.argsort(kt[s])[:nt].tolist())
            assert sorted(np.flatnonzero(fm[s]).tolist()) == sorted(np.argsort(kf[s])[:nf].tolist())
        if t <= 64:
            assert not tx.any()


def _binom_z(k, n, p):
    k = np.asarray(k, dtype=np.float64)
    return (k - n * p) / math.sqrt(n * p * (1 - p))


def test_draw_structured_law():
    """over N draws at B = 10 (two slots per group): every column of a slot of group g is picked with frequency nt / t, every row with
    nf / f; every sample lands in every group with frequency size_g / B under both permutations; the two permutations are uncorrelated
    (joint group counts of a sample at the product of the marginals)"""
    cfg = vit_huge14(frames=1)
    t, f, B, N = cfg.audio_t, cfg.audio_f, 10, 4000
    sg, sizes = _slot_group(B), mp.group_sizes(B)
    G = len(sizes)
    rng = np.random.default_rng(20260)
    col, row = np.zeros((G, t)), np.zeros((G, f))
    ga_n, gv_n, joint = np.zeros((B, G)), np.zeros((B, G)), np.zeros((B, G, G))
    for _ in range(N):
        perm_a, perm_v, bits, tx = mp.draw_structured(cfg, sg, rng)
        tm, fm = _unpack(bits, tx, t, f)
        np.add.at(col, sg, tm)
        np.add.at(row, sg, fm)
        ga, gv = np.empty(B, dtype=np.int64), np.empty(B, dtype=np.int64)
        ga[perm_a], gv[perm_v] = sg, sg
        ga_n[np.arange(B), ga] += 1
        gv_n[np.arange(B), gv] += 1
        joint[np.arange(B), ga, gv] += 1
    zs = {"column": 0.0, "row": 0.0}
    for g in range(G):
        n = N * sizes[g]
        for what, cnt, size in (("column", col[g], t), ("row", row[g], f)):
            k = int(size * mp.group_ratio(g) * 0.7)
            if k == 0:
                assert not cnt.any()
                continue
            zs[what] = max(zs[what], float(np.abs(_binom_z(cnt, n, k / size)).max()))
    p = np.array(sizes) / B
    zs["group_a"] = float(np.abs((ga_n - N * p) / np.sqrt(N * p * (1 - p))).max())
    zs["group_v"] = float(np.abs((gv_n - N * p) / np.sqrt(N * p * (1 - p))).max())
    pj = p[:, None] * p[None, :]
    zs["joint"] = float(np.abs((joint - N * pj) / np.sqrt(N * pj * (1 - pj))).max())
    planlib.record_stat("draw_structured_law", **zs)
    assert max(zs.values()) < Z_MAX, zs


# ---- the whole contrastive audio draw against make_contrastive_plan ----------------------------------------------------------------------------
def _keep_counts_device_style(cfg, B, steps, base):
    """per (group, token) keep counts of the audio sequences over `steps` draws the way the engine draws them: draw_structured on the host, the
    restatement of the kernel under the model's keys (base << 32 | draw number), slot = sequence index"""
    La, sg = cfg.audio_tokens, _slot_group(B)
    G = int(sg.max()) + 1
    cnt = np.zeros((G, La))
    rng = np.random.default_rng(base)
    d = np.zeros((B, 16), dtype=np.int32)
    for step in range(1, steps + 1):
        _, _, bits, tx = mp.draw_structured(cfg, sg, rng)
        for sl in range(B):
            keep = mp.len_keep(La, mp.group_ratio(int(sg[sl])))
            d[sl, [0, 1, 6, 9]] = [La, keep, cfg.audio_t, tx[sl]]
            cnt[sg[sl], mp.plan_shuffle(d[sl], sl, (base << 32) | step, *bits)[:keep]] += 1
    return cnt


def _keep_counts_reference_style(cfg, B, steps, seed):
    gen, pyrng = torch.Generator().manual_seed(seed), random.Random(seed)
    cnt = np.zeros((len(mp.group_sizes(B)), cfg.audio_tokens))
    for _ in range(steps):
        plan = mp.make_contrastive_plan(cfg, B, gen, pyrng)
        for b in range(B):
            cnt[int(plan.a_group[b]), plan.a_keep[b].numpy()] += 1
    return cnt


def _two_sample_z(k1, k2, n):
    """per cell: two binomial samples of n trials each; a cell both samples agree on entirely (0 or n: group 0 keeps every token) scores 0"""
    p = (k1 + k2) / (2 * n)
    var = p * (1 - p) * 2 / n
    z = np.zeros_like(p)
    np.divide(k1 / n - k2 / n, np.sqrt(var), out=z, where=var > 0)
    assert (k1 == k2)[var == 0].all()
    return z


@pytest.mark.parametrize("name", ["La128", "huge14"])
def test_contrastive_audio_draw_has_the_reference_generators_law(name):
    """B = 10, 300 steps -> 600 sequences per group and generator: the keep frequency of every (group, token) under the device-style draw
    against make_contrastive_plan's; the same statistic between two independent runs of make_contrastive_plan shows what the bound allows"""
    cfg = AVSiamConfig(audio_tokens=128) if name == "La128" else vit_huge14(frames=1)
    B, steps = 10, 300
    n = steps * 2
    dev = _keep_counts_device_style(cfg, B, steps, 77)
    ref, ref2 = _keep_counts_reference_style(cfg, B, steps, 5), _keep_counts_reference_style(cfg, B, steps, 6)
    keeps = [mp.len_keep(cfg.audio_tokens, mp.group_ratio(g)) for g in range(5)]
    for c in (dev, ref, ref2):
        assert np.array_equal(c.sum(axis=1), n * np.array(keeps))          # the mean keep frequency of a group is exact: keep / La
    z, z0 = np.abs(_two_sample_z(dev, ref, n)), np.abs(_two_sample_z(ref, ref2, n))
    planlib.record_stat("contrastive_audio_law_" + name, device_vs_reference=z.max(), reference_vs_reference=z0.max())
    assert z0.max() < Z_MAX, z0.max()
    assert z.max() < Z_MAX, (z.max(), np.unravel_index(z.argmax(), z.shape))


# ---- independence of the streams ---------------------------------------------------------------------------------------------------------------
def _kept(sq, seed, L=196, keep=49):
    m = np.zeros(L, dtype=bool)
    m[np.argsort(mp.plan_noise(L, sq, seed), kind="stable")[:keep]] = True
    return m


def test_streams_are_independent_and_positions_uniform():
    """unstructured, L = 196, keep = 49: |kept(x) & kept(y)| of two independent draws is hypergeometric (mean keep^2 / L); z-test of its mean
    over 2000 pairs for neighbouring sequences of a launch, the same sequence under consecutive keys (consecutive draws of a model) and
    under base seeds that differ in one bit of the high word; and every position is kept with frequency keep / L"""
    L, keep, n = 196, 49, 2000
    assert mp.plan_shuffle(np.array([L, keep] + [0] * 14), 3, 17).tolist() == np.argsort(mp.plan_noise(L, 3, 17), kind="stable").tolist()
    mean = keep * keep / L
    var = keep * (keep / L) * (1 - keep / L) * (L - keep) / (L - 1)
    base = 0x5EED
    pairs = {
        "neighbour_sequences": [(_kept(2 * i, base << 32 | 1), _kept(2 * i + 1, base << 32 | 1)) for i in range(n)],
        "consecutive_keys": [(_kept(3, base << 32 | 2 * i), _kept(3, base << 32 | (2 * i + 1))) for i in range(n)],
        "base_seed_bit": [(_kept(i % 7, base << 32 | i), _kept(i % 7, (base ^ (1 << (i % 32))) << 32 | i)) for i in range(n)],
    }
    zs = {}
    for what, pr in pairs.items():
        ov = np.array([int((x & y).sum()) for x, y in pr], dtype=np.float64)
        assert ov.std() > 0
        zs[what] = float(abs(ov.mean() - mean) / math.sqrt(var / n))
    freq = np.sum([x for x, _ in pairs["neighbour_sequences"]] + [y for _, y in pairs["neighbour_sequences"]], axis=0)
    zs["position_marginal"] = float(np.abs(_binom_z(freq, 2 * n, keep / L)).max())
    planlib.record_stat("streams_independent", **zs)
    assert max(zs.values()) < Z_MAX, zs
