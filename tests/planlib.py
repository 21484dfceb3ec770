"""Shared by tests/test_maskplan_cpu.py and tests/test_maskplan_gpu.py: descriptor tables of the mask-plan kernel (csrc/maskplan.hip) whose
output regions are laid out in a shuffled order with guard bands between them, sentinel-filled output buffers, the golden stream's cases and
a log of the worst statistics."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = 16
OUTPUTS = ("row_src", "row_tok", "src_row", "mask", "ids", "pos_row", "row_of_pos", "pred_id")
SENTINEL = -7
GUARD = 5                                        # elements between two regions (and at both ends): a write beside a region lands on a sentinel


def record_stat(test, **values):
    """Log the worst statistic of a test into test_out/plan_stats.json (kept out of git), from which profiles/r16/plan_stats.json is committed (a log, never a gate)."""
    path = os.path.join(ROOT, "test_out", "plan_stats.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        data.setdefault(test, {}).update({k: float(v) for k, v in values.items()})
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except Exception:
        pass


def _place(sizes, rng):
    """offsets of regions of the given sizes (None: no region, offset -1) laid out in a shuffled order with GUARD elements around each -> (offsets, total)"""
    off = [-1] * len(sizes)
    at = GUARD
    for i in rng.permutation(len(sizes)):
        if sizes[i] is None:
            continue
        off[i] = at
        at += sizes[i] + GUARD
    return off, at


def classic_table(seqs, seed=0):
    """seqs: list of dicts L, keep, t (t_patches, 0 unstructured), tx (tmask_x), dec (bool: has a decoder part), ids (bool) ->
    (desc int32 [n, 16], sizes {output name: elements}).  Every region sits somewhere else than its descriptor's position suggests; src_id,
    enc_base differ per sequence; the decoder and mask regions are placed independently (dec_off != mask_off)."""
    rng = np.random.default_rng(seed)
    n = len(seqs)
    row_off, nrow = _place([s["keep"] for s in seqs], rng)
    dec_off, ndec = _place([s["L"] if s.get("dec", True) else None for s in seqs], rng)
    mask_off, nmask = _place([s["L"] if s.get("dec", True) else None for s in seqs], rng)
    ids_off, nids = _place([s["L"] if s.get("ids", True) else None for s in seqs], rng)
    d = np.zeros((n, FIELDS), dtype=np.int32)
    for i, s in enumerate(seqs):
        d[i] = [s["L"], s["keep"], row_off[i], 1000 + 3 * i, dec_off[i], 100000 + 2000 * i, s.get("t", 0), ids_off[i], max(mask_off[i], 0),
                s.get("tx", 0), 0, 0, -1, 0, 0, 0]
    return d, {"row_src": nrow, "row_tok": nrow, "src_row": ndec, "mask": nmask, "ids": nids}


def grouped_table(seqs, seed=0):
    """as classic_table with every decoder sequence in the GROUPED layout: the removed rows, the kept rows (both in src_row / pos_row), the
    positions (row_of_pos) and the compact prediction rows (pred_id) of a sequence are four regions placed independently"""
    d, sizes = classic_table(seqs, seed)
    rng = np.random.default_rng(seed + 1)
    dec = [s.get("dec", True) for s in seqs]
    kind = [(i, k) for i in range(len(seqs)) if dec[i] for k in (0, 1)]            # (sequence, 0 removed rows | 1 kept rows) share one row space
    off, nrows = _place([(s["L"] - s["keep"], s["keep"])[k] for i, k in kind for s in (seqs[i],)], rng)
    pred_off, npred = _place([s["L"] - s["keep"] if dec[i] else None for i, s in enumerate(seqs)], rng)
    for (i, k), o in zip(kind, off):
        d[i, 12 + k] = o
    for i, s in enumerate(seqs):
        if dec[i]:
            d[i, 14], d[i, 15] = pred_off[i], 7 * i
    sizes.update(src_row=nrows, pos_row=nrows, row_of_pos=sizes["src_row"], pred_id=npred)
    return d, sizes


def engine_grouped_table(B, T, La, Lv, ka, kv):
    """the MAE pass's own grouped table (engine.MaePass): per sample [removed audio | removed frames | kept audio | kept frames]"""
    ma, mv = La - ka, Lv - kv
    Lt, lq, n_enc = La + T * Lv, ma + T * mv, ka + T * kv
    d = np.zeros((B + B * T, FIELDS), dtype=np.int32)
    for b in range(B):
        d[b] = [La, ka, b * ka, b, b * Lt, b * n_enc, 0, b * La, b * La, 0, 0, 0, b * Lt, b * Lt + lq, b * ma, 0]
        for t in range(T):
            i = b * T + t
            d[B + i] = [Lv, kv, B * ka + i * kv, i, b * Lt + La + t * Lv, b * n_enc + ka + t * kv, 0, B * La + i * Lv, B * La + i * Lv, 0, 0, 0,
                        b * Lt + ma + t * mv, b * Lt + lq + ka + t * kv, B * ma + i * mv, La]
    n = B * La + B * T * Lv
    return d, {"row_src": B * ka + B * T * kv, "row_tok": B * ka + B * T * kv, "src_row": B * Lt, "mask": n, "ids": n, "pos_row": B * Lt,
               "row_of_pos": B * Lt, "pred_id": B * ma + B * T * mv}


def host_buffers(sizes):
    """sentinel-filled numpy outputs (mask float32, the others int32) for maskplan.plan_reference"""
    return {k: np.full(max(n, 1), SENTINEL, dtype=np.float32 if k == "mask" else np.int32) for k, n in sizes.items()}


def reference(desc, seed, sizes, bits=(None, None, None)):
    from avsiam_amd.maskplan import plan_reference
    return plan_reference(desc, seed, *bits, out=host_buffers(sizes))


# ---- the golden stream (tests/golden/plan_stream_v1.npz, written once by tools/gen_golden_plan_stream.py) ----------------------------------------
STREAM_KEYS = (0x0000007B00000001, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000000 | 0x80000003)


def stream_case():
    """-> (desc, sizes of the outputs, tmask_lo, tmask_hi, fmask): 196 unstructured tokens at sequence index 0 and 7; 512 tokens on a 64-column grid with a fixed
    bit set; 657 tokens on a 73-column grid with a column above 64 (and above 31 / 63) forced; small fillers between"""
    seqs = [dict(L=196, keep=49), dict(L=512, keep=307, t=64), dict(L=657, keep=394, t=73, tx=0x105), dict(L=64, keep=16), dict(L=65, keep=65),
            dict(L=1, keep=0), dict(L=256, keep=64), dict(L=196, keep=49)]
    d, sizes = classic_table(seqs, seed=11)
    u = lambda *v: np.array(v, dtype=np.uint32).view(np.int32)
    z = [0] * 5
    return d, sizes, u(0, 0x80010004, 0x80000001, *z), u(0, 0x80000100, 0x00400001, *z), u(0, 0x81, 0x100, *z)


def stream_ids(desc, seed, bits):
    """the shuffles of all sequences of the case, one after another (int16 [sum L])"""
    from avsiam_amd.maskplan import plan_shuffle
    return np.concatenate([plan_shuffle(desc[sq], sq, seed, *bits) for sq in range(desc.shape[0])]).astype(np.int16)
