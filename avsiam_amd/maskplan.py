"""Explicit mask plans for the two passes of the AVSiam pre-training step.

The reference draws its masks inside ``forward`` from three global RNGs (torch.rand / torch.randperm
/ python ``random.sample``) and breaks ties with an unstable argsort
(/root/reference/src/models/cav_mae_base.py:365-439,533-550), so its results are only reproducible
when the *plan* - which tokens each sample keeps - is made an explicit input.
This module holds the plan data structures and a host generator with the reference's distribution.

ContrastivePlan (pass 1, forward_encoder_mmixed :508-594)
    a_group[b], v_group[b]   multi-ratio group (0..n_groups-1) of sample b for audio / video
    a_keep[b]                1-D LongTensor of kept audio token ids (length keep(La, 0.2*group))
    v_keep[b][t]             same per frame (length keep(Lv, 0.2*group))
MaePlan (pass 2, forward_encoder :441-504, 75 % unstructured)
    ids_keep_a [B,keep_a]  ids_restore_a [B,La]  ids_keep_v [B,T,keep_v]  ids_restore_v [B,T,Lv]
"""
import math
import random as _pyrandom
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from .config import AVSiamConfig


def group_ratio(g: int) -> float:
    return 0 + 0.2 * g                                    # cav_mae_base.py:546,549 (same float expression)


def len_keep(L: int, ratio: float) -> int:
    return int(L * (1 - ratio))                           # :372,399


def group_sizes(batch: int, n_groups: int = 5):
    """Sizes produced by ``torch.chunk(perm, 5)`` (:534): ceil(B/5)-sized chunks, possibly fewer than 5."""
    c = math.ceil(batch / n_groups)
    sizes = []
    left = batch
    while left > 0:
        sizes.append(min(c, left))
        left -= c
    return sizes


@dataclass
class ContrastivePlan:
    a_group: torch.Tensor
    v_group: torch.Tensor
    a_keep: List[torch.Tensor]
    v_keep: List[List[torch.Tensor]]

    @property
    def batch(self):
        return len(self.a_keep)


@dataclass
class MaePlan:
    ids_keep_a: torch.Tensor
    ids_restore_a: torch.Tensor
    ids_keep_v: torch.Tensor
    ids_restore_v: torch.Tensor

    @property
    def batch(self):
        return self.ids_keep_a.shape[0]

    def mask_a(self):
        """0 = kept, 1 = removed, in original token order (:385-388)."""
        return (self.ids_restore_a >= self.ids_keep_a.shape[1]).float()

    def mask_v(self):
        return (self.ids_restore_v >= self.ids_keep_v.shape[-1]).float()


def _unstructured(noise: torch.Tensor, keep: int):
    ids_shuffle = torch.argsort(noise, dim=-1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=-1, stable=True)
    return ids_shuffle[..., :keep], ids_restore


def make_mae_plan(cfg: AVSiamConfig, batch: int, gen: torch.Generator) -> MaePlan:
    """random_masking_unstructured at ratio 0.75 for both modalities (:476-477, ratios hard-coded :696)."""
    na = torch.rand(batch, cfg.audio_tokens, generator=gen)
    nv = torch.rand(batch, cfg.frames, cfg.video_tokens, generator=gen)
    ka, ra = _unstructured(na, cfg.keep_a)
    kv, rv = _unstructured(nv, cfg.keep_v)
    return MaePlan(ka.contiguous(), ra.contiguous(), kv.contiguous(), rv.contiguous())


# ---- region plans (CAVMAE_BASE.inpaint): "mask THIS second of audio / THIS corner of the frame" ---------------------------------------------
def _patch_range(lo, hi, n_patches, stride, what):
    """patches of `stride` cells that intersect the half-open cell range [lo, hi), clipped to the n_patches the model covers"""
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi <= lo:
        raise ValueError(f"{what}: [{lo}, {hi}) is not a range (need 0 <= start < end)")
    p0, p1 = min(lo // stride, n_patches), min(-(-hi // stride), n_patches)
    if p1 <= p0:
        raise ValueError(f"{what}: [{lo}, {hi}) lies outside the {n_patches * stride} cells the patches cover")
    return p0, p1


def audio_time_span(cfg: AVSiamConfig, frame0, frame1):
    """bool [La]: the audio patches that intersect spectrogram frames [frame0, frame1) (all mel bands; token f * audio_t + t)"""
    t0, t1 = _patch_range(frame0, frame1, cfg.audio_t, cfg.st, "audio_time_span")
    m = torch.zeros(cfg.audio_f, cfg.audio_t, dtype=torch.bool)
    m[:, t0:t1] = True
    return m.reshape(-1)


def audio_mel_band(cfg: AVSiamConfig, bin0, bin1):
    """bool [La]: the audio patches that intersect mel bins [bin0, bin1) (the whole clip)"""
    f0, f1 = _patch_range(bin0, bin1, cfg.audio_f, cfg.st, "audio_mel_band")
    m = torch.zeros(cfg.audio_f, cfg.audio_t, dtype=torch.bool)
    m[f0:f1] = True
    return m.reshape(-1)


def frame_box(cfg: AVSiamConfig, y0, x0, y1, x1):
    """bool [Lv]: the patches of a frame that intersect rows [y0, y1) x columns [x0, x1) (token gy * grid + gx)"""
    gy0, gy1 = _patch_range(y0, y1, cfg.grid, cfg.st, "frame_box rows")
    gx0, gx1 = _patch_range(x0, x1, cfg.grid, cfg.st, "frame_box columns")
    m = torch.zeros(cfg.grid, cfg.grid, dtype=torch.bool)
    m[gy0:gy1, gx0:gx1] = True
    return m.reshape(-1)


def make_mae_plan_regions(cfg: AVSiamConfig, batch: int, gen: torch.Generator, must_mask_a=None, must_mask_v=None) -> MaePlan:
    """make_mae_plan with patches that MUST be removed: bool [B, La] / [B, T, Lv] (or anything that broadcasts to them - the helpers above
    give one sequence's worth).  The reference's own trick for structured masks (:415-422): the forced tokens' noise is overwritten with 1.1 so
    that they sort last; the model's keep counts hold (75 % leave, forced ones first, the remainder at random).  Draws the noise make_mae_plan
    draws: with nothing forced the two give the same plan."""
    na = torch.rand(batch, cfg.audio_tokens, generator=gen)
    nv = torch.rand(batch, cfg.frames, cfg.video_tokens, generator=gen)
    for noise, must, keep, what in ((na, must_mask_a, cfg.keep_a, "audio"), (nv, must_mask_v, cfg.keep_v, "frames")):
        if must is None:
            continue
        must = torch.as_tensor(must)
        if must.dtype != torch.bool:
            raise ValueError(f"make_mae_plan_regions: must_mask ({what}) must be bool, got {must.dtype}")
        try:
            must = torch.broadcast_to(must, noise.shape)
        except RuntimeError:
            raise ValueError(f"make_mae_plan_regions: must_mask ({what}) of shape {tuple(must.shape)} does not broadcast to {tuple(noise.shape)}") from None
        L = noise.shape[-1]
        count = must.sum(dim=-1)
        if int(count.max()) > L - keep:
            idx = [int(i) for i in torch.nonzero(count > L - keep)[0]]
            where = f"sample {idx[0]}" + (f", frame {idx[1]}" if len(idx) > 1 else "")
            raise ValueError(f"make_mae_plan_regions: {what}, {where}: {int(count[tuple(idx)])} patches must be masked but the model removes "
                             f"{L - keep} of {L} (keeps {keep})")
        noise[must] = 1.1
    ka, ra = _unstructured(na, cfg.keep_a)
    kv, rv = _unstructured(nv, cfg.keep_v)
    return MaePlan(ka.contiguous(), ra.contiguous(), kv.contiguous(), rv.contiguous())


def make_contrastive_plan(cfg: AVSiamConfig, batch: int, gen: torch.Generator, pyrng: _pyrandom.Random) -> ContrastivePlan:
    """Two independent batch permutations chunked into <=5 groups (:533-538); group g masks audio with
    random_masking_structured(ratio 0.2 g, t, f=8, 'tf') (:546, :392-439) and video with
    random_masking_unstructured(ratio 0.2 g) (:549)."""
    t, f = cfg.audio_t, cfg.audio_f
    sizes = group_sizes(batch, cfg.n_groups)
    perm_a = torch.randperm(batch, generator=gen)
    perm_v = torch.randperm(batch, generator=gen)
    a_group = torch.zeros(batch, dtype=torch.int64)
    v_group = torch.zeros(batch, dtype=torch.int64)
    a_keep = [None] * batch
    v_keep = [None] * batch
    off = 0
    for g, n in enumerate(sizes):
        r = group_ratio(g)
        idx_a = perm_a[off:off + n]
        idx_v = perm_v[off:off + n]
        off += n
        noise = torch.rand(n, cfg.audio_tokens, generator=gen).reshape(n, f, t)
        for i in range(n):                                    # :415-418 time columns
            for k in pyrng.sample(range(t), int(t * r * 0.7)):
                noise[i, :, k] = 1.1
        for i in range(n):                                    # :419-422 frequency rows
            for k in pyrng.sample(range(f), int(f * r * 0.7)):
                noise[i, k, :] = 1.1
        keep, _ = _unstructured(noise.reshape(n, cfg.audio_tokens), len_keep(cfg.audio_tokens, r))
        for i in range(n):
            a_group[idx_a[i]] = g
            a_keep[int(idx_a[i])] = keep[i].clone()
        nv = torch.rand(n, cfg.frames, cfg.video_tokens, generator=gen)
        keepv, _ = _unstructured(nv, len_keep(cfg.video_tokens, r))
        for i in range(n):
            v_group[idx_v[i]] = g
            v_keep[int(idx_v[i])] = [keepv[i, tt].clone() for tt in range(cfg.frames)]
    return ContrastivePlan(a_group, v_group, a_keep, v_keep)


def plan_to_arrays(plan):
    """Flatten a plan into plain int64 tensors (for .npz fixtures)."""
    if isinstance(plan, MaePlan):
        return {"ids_keep_a": plan.ids_keep_a, "ids_restore_a": plan.ids_restore_a,
                "ids_keep_v": plan.ids_keep_v, "ids_restore_v": plan.ids_restore_v}
    B = plan.batch
    T = len(plan.v_keep[0])
    la = max(k.numel() for k in plan.a_keep)
    lv = max(k.numel() for fr in plan.v_keep for k in fr)
    a_pad = torch.full((B, la), -1, dtype=torch.int64)
    v_pad = torch.full((B, T, lv), -1, dtype=torch.int64)
    for b in range(B):
        a_pad[b, :plan.a_keep[b].numel()] = plan.a_keep[b]
        for t in range(T):
            v_pad[b, t, :plan.v_keep[b][t].numel()] = plan.v_keep[b][t]
    return {"a_group": plan.a_group, "v_group": plan.v_group, "a_keep": a_pad, "v_keep": v_pad}


def plan_from_arrays(d):
    d = {k: torch.as_tensor(v) for k, v in d.items()}
    if "ids_keep_a" in d:
        return MaePlan(d["ids_keep_a"].long(), d["ids_restore_a"].long(), d["ids_keep_v"].long(), d["ids_restore_v"].long())
    B, T = d["v_keep"].shape[:2]
    a_keep = [d["a_keep"][b][d["a_keep"][b] >= 0].long() for b in range(B)]
    v_keep = [[d["v_keep"][b, t][d["v_keep"][b, t] >= 0].long() for t in range(T)] for b in range(B)]
    return ContrastivePlan(d["a_group"].long(), d["v_group"].long(), a_keep, v_keep)


# ---- the device draw, restated on the host (numpy; tests/test_maskplan_*.py hold csrc/maskplan.hip to this) -------------------------------------
PLAN_OUTPUTS = ("row_src", "row_tok", "src_row", "mask", "ids", "pos_row", "row_of_pos", "pred_id")


def plan_noise(L, sq, seed):
    """float32 [L]: the noise of tokens 0..L-1 of sequence number `sq` of a launch under the 64-bit key `seed` - word 0 of
    Philox4x32-10 with counter (token, sq, 0, 0) and key (seed low, seed high), its top 24 bits scaled into [0, 1) (like torch.rand)."""
    from .preprocess import philox4x32_10
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(np.arange(L, dtype=np.uint64), int(sq), 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def plan_forced(L, t_patches, tmask_lo, tmask_hi, tmask_x, fmask):
    """bool [L]: the tokens of an [f][t_patches] grid (token = f * t_patches + t) that structured masking forces out: time column t is in
    the 96-bit set tmask_lo | tmask_hi << 32 | tmask_x << 64, or frequency row f in the 32-bit set fmask.  The words are taken as unsigned
    (an int32 with bit 31 set is negative); bits at or above t_patches / the number of rows name nothing."""
    m = 0xFFFFFFFF
    tbits = (int(tmask_lo) & m) | ((int(tmask_hi) & m) << 32) | ((int(tmask_x) & m) << 64)
    fbits = int(fmask) & m
    rows = -(-L // t_patches)
    col = np.array([(tbits >> c) & 1 for c in range(t_patches)], dtype=bool)
    row = np.array([(fbits >> r) & 1 for r in range(rows)], dtype=bool)
    i = np.arange(L)
    return col[i % t_patches] | row[i // t_patches]


def plan_shuffle(desc_row, sq, seed, tmask_lo=None, tmask_hi=None, fmask=None):
    """int64 [L]: the shuffle of sequence `sq` (its descriptor: desc_row) - tokens by ascending noise, equal noise by ascending index"""
    L, t_p = int(desc_row[0]), int(desc_row[6])
    noise = plan_noise(L, sq, seed)
    if t_p > 0:
        noise[plan_forced(L, t_p, tmask_lo[sq], tmask_hi[sq], desc_row[9], fmask[sq])] = np.float32(1.1)    # "large value will be removed"
    return np.argsort(noise, kind="stable")


def plan_reference(desc, seed, tmask_lo=None, tmask_hi=None, fmask=None, out=None):
    """What one launch of the mask-plan kernel (csrc/maskplan.hip, ops.mask_plan) writes, restated from its contract with numpy alone.
    desc: int32 [nseq, 16] descriptors (0 L, 1 keep, 2 row_off, 3 src_id, 4 dec_off, 5 enc_base, 6 t_patches, 7 ids_off, 8 mask_off,
    9 tmask_x, 12 dec_m_off, 13 dec_k_off, 14 pred_off, 15 pos_base); seed: the 64-bit Philox key; tmask_lo / tmask_hi / fmask: the per-sequence
    bit sets of the structured sequences (read at the sequence's index, only where t_patches > 0).
    out: dict of numpy arrays named as PLAN_OUTPUTS (those a launch does not need may be missing); exactly the elements the kernel writes
    are written, every other element is left alone - pre-fill with a sentinel to see that.  -> out.

    With j the rank of token `tok` in the sequence's shuffle (plan_shuffle: stable ascending order of the noise, forced tokens at 1.1):
      row_src / row_tok[row_off + j] = src_id / tok                 j < keep
      ids[ids_off + j]               = tok                          ids_off >= 0
    and for dec_off >= 0
      mask[mask_off + tok]           = 0 kept | 1 removed
      classic (dec_m_off < 0):  src_row[dec_off + tok] = enc_base + j | -1
      grouped:                  row r = dec_k_off + j (kept) | dec_m_off + j - keep (removed);  src_row[r] = enc_base + j | -1;
                                pos_row[r] = pos_base + tok;  row_of_pos[dec_off + tok] = r;  pred_id[pred_off + j - keep] = mask_off + tok"""
    desc = np.asarray(desc)
    assert desc.ndim == 2 and desc.shape[1] == 16
    if out is None:
        out = {}
    for sq in range(desc.shape[0]):
        L, keep, row_off, src_id, dec_off, enc_base, _, ids_off, mask_off, _, _, _, dec_m, dec_k, pred_off, pos_base = (int(x) for x in desc[sq])
        tok = plan_shuffle(desc[sq], sq, seed, tmask_lo, tmask_hi, fmask)
        j = np.arange(L)
        kept = j < keep
        out["row_src"][row_off:row_off + keep] = src_id
        out["row_tok"][row_off:row_off + keep] = tok[:keep]
        if ids_off >= 0:
            out["ids"][ids_off:ids_off + L] = tok
        if dec_off < 0:
            continue
        src = np.where(kept, enc_base + j, -1)
        out["mask"][mask_off + tok] = np.where(kept, 0.0, 1.0)
        if dec_m < 0:
            out["src_row"][dec_off + tok] = src
        else:
            r = np.where(kept, dec_k + j, dec_m + j - keep)
            out["src_row"][r] = src
            out["pos_row"][r] = pos_base + tok
            out["row_of_pos"][dec_off + tok] = r
            out["pred_id"][pred_off + j[keep:] - keep] = mask_off + tok[keep:]
    return out


def draw_structured(cfg: AVSiamConfig, slot_group, nprng):
    """The host part of the contrastive pass's device draw: what forward_encoder_mmixed draws outside random_masking_* (two randperm +
    chunk, cav_mae_base.py:533-538) and the time-column / frequency-row picks of random_masking_structured mode 'tf' (:415-422).
    slot_group[sl]: the multi-ratio group of slot sl (group-major); nprng: a numpy Generator, advanced by permutation(B) twice, then
    random((B, t)) and random((B, f)).  -> (perm_a, perm_v, bits int32 [3, B], tmask_x int32 [B]): slot sl holds audio sample perm_a[sl]
    and video sample perm_v[sl]; its int(t * r * 0.7) time columns are the set bits[0] | bits[1] << 32 | tmask_x << 64 (words taken
    as unsigned), its int(f * r * 0.7) frequency rows the set bits[2]."""
    slot_group = np.asarray(slot_group)
    B = slot_group.shape[0]
    t, f = cfg.audio_t, cfg.audio_f
    perm_a, perm_v = nprng.permutation(B), nprng.permutation(B)
    ratios = np.array([group_ratio(int(g)) for g in slot_group])
    nt = np.array([int(t * r * 0.7) for r in ratios])
    nf = np.array([int(f * r * 0.7) for r in ratios])
    # random.sample(range(t), n): the n smallest of t random keys
    rank_t = np.argsort(np.argsort(nprng.random((B, t)), axis=1), axis=1)
    rank_f = np.argsort(np.argsort(nprng.random((B, f)), axis=1), axis=1)
    assert t <= 96 and f <= 32, "structured masks are bit sets: at most 96 time and 32 frequency patches"
    tm = (rank_t < nt[:, None]).astype(np.uint64)
    fm = (rank_f < nf[:, None]).astype(np.uint64)
    tbits = (tm[:, :64] << np.arange(min(t, 64), dtype=np.uint64)[None, :]).sum(axis=1)
    fbits = (fm << np.arange(f, dtype=np.uint64)[None, :]).sum(axis=1)
    bits = np.zeros((3, B), dtype=np.int32)
    bits[0] = (tbits & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    bits[1] = (tbits >> np.uint64(32)).astype(np.uint32).view(np.int32)
    bits[2] = fbits.astype(np.uint32).view(np.int32)
    tmask_x = np.zeros(B, dtype=np.int32)
    if t > 64:                                               # time patches 64.. travel in the descriptor (PlanSeq.tmask_x)
        tmask_x[:] = (tm[:, 64:] << np.arange(t - 64, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32).view(np.int32)
    return perm_a, perm_v, bits, tmask_x
