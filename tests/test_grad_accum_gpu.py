"""Gradient accumulation over micro-batches on a real MI355X (csrc/grad_accum.hip; CAVMAEFT_BASE.set_grad_accumulation).

Kernel: ``avs_grad_accum`` against ops.grad_accum_reference (pinned to torch's own .grad accumulation in tests/test_grad_accum_cpu.py) bit for
bit - one fp32 add per element has one correctly rounded answer, so there is no tolerance -, with acc and g inside sentinel margins, gaps
and a dead class that must keep their bytes, a table that sends workgroups round the chunk loop twice, two identical call sequences, and
the refusals.
Model (depth 2, batch 2, the "det" knob: one writer per gradient element): a cycle of one micro-step is the plain step byte for byte; a
cycle of three (branches mm, a, v) leaves everything alone until its last micro-step, holds the fp32 sum of the three gradient arenas -
copy on first touch per class -, and ends in ops.adam_table over the union with grad_scale 1 / 3; the epoch-end flush; parity of the
averaged gradient with autograd through the CPU oracle at the effective batch (the bounds of tests/test_ft_train_gpu.py); the guard over
the accumulated step; the refusals while micro-steps are pending; the plain step's digest; two gloo ranks sharing the GPU.
Measured margins go through tests.helpers.record_margin (profiles/r20/grad_accum_margins.json is their copy)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs, synth_state_ft
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS, EPS, WD = (0.95, 0.999), 1e-8, 5e-7
INF = float("inf")
NCLS = 5
MARGIN = 64
SENT_ACC, SENT_G = 777.25, -31337.5                      # what gaps, dead classes and the margins hold in acc / in g
# liveness of the three successive calls: class 1 is never live; class 4 is first reached by the third call (copied there); 2.0: what a class
# two ranks reached sums to
LIVES = ([1.0, 0.0, 1.0, 1.0, 0.0], [1.0, 0.0, 2.0, 1.0, 0.0], [2.0, 0.0, 0.0, 0.0, 1.0])


def _ops():
    from avsiam_amd import ops
    return ops


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
def _raw_table(segs, limit):
    """an ops.AdamTable that skips the host validation (a malformed segment must reach the kernel): chunks counted as the kernel counts"""
    ops = _ops()
    _, chunk, _ = ops.adam_table_geometry()
    t = ops.AdamTable.__new__(ops.AdamTable)
    host = np.zeros(len(segs), dtype=np.dtype([("lo", "<i8"), ("n", "<i4"), ("group", "<i4"), ("cls", "<i4"), ("pad", "<i4")]))
    for i, s in enumerate(segs):
        host[i] = tuple(s) + (0,)
    ok = lambda lo, n, g, c: n > 0 and n % 4 == 0 and lo >= 0 and lo % 4 == 0 and 0 <= g < 3 and 0 <= c < 16
    t.segs, t.ncls, t.limit = [tuple(s) for s in segs], NCLS, limit
    t.chunks = max(1, sum((n + chunk - 1) // chunk for lo, n, g, c in segs if ok(lo, n, g, c)))
    t.dev = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    return t


def _layout(lengths):
    """segments end to end, an 8-element gap behind every second one, groups and classes interleaved; one malformed segment (n = 6) in a gap"""
    segs, at = [], 8
    for i, n in enumerate(lengths):
        segs.append((at, n, i % 3, (i * 2 + i // NCLS) % NCLS))
        at += n + (8 if i % 2 == 0 else 0)
    segs.insert(len(segs) // 2, (at, 6, 0, 0))
    return segs, at + 8


def _grads(segs, total, live, seed):
    """SENT_G everywhere (gaps, the malformed segment, classes not live now); Gaussians of mixed magnitude in the segments of live classes,
    with -0.0, +-inf and NaN planted at the front of the larger ones"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((total,), SENT_G)
    for lo, n, grp, c in segs:
        if n % 4 == 0 and live[c] > 0:
            g[lo:lo + n] = torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-4, 3, (1,), generator=gen)))
            g[lo] = -0.0
            if n >= 64:
                g[lo + 1], g[lo + 2], g[lo + 3], g[lo + 5] = INF, -INF, float("nan"), (-INF if seed % 2 else INF)
    return g


def _guarded(x, sentinel):
    """x inside a buffer with MARGIN sentinel elements on either side -> (the view, the whole buffer)"""
    whole = torch.full((x.numel() + 2 * MARGIN,), sentinel, device="cuda")
    view = whole[MARGIN:MARGIN + x.numel()]
    view.copy_(x)
    return view, whole


def _same_bits(got, want, what):
    """uint32 equality; where both are NaN only the positions are compared (the payload of a NaN an add produced is the hardware's)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int((gn != wn).sum()))
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~gn
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5].tolist())


def _sequence(segs, total, lives, seed, publish_last=True):
    """`lives` successive calls (the first with first = 1, the last publishing) on the device and through the restatement.
    -> bytes of everything the calls may have written, for the determinism test"""
    ops = _ops()
    table = _raw_table(segs, total)
    ctl, actl = ops.AdamCtl("cuda"), ops.GradAccumCtl("cuda")
    ctl.step[:NCLS] = torch.tensor([3, 1, 4, 1, 5], dtype=torch.int32)
    ctl.set_lr(1e-3, 5e-2, 2e-4)
    torch.cuda.synchronize()
    head = ctl.buf[:3 + 16].clone()                                   # lr and step: never written
    acc, acc_whole = _guarded(torch.full((total,), SENT_ACC), SENT_ACC)
    ref_acc, ref_live = np.full(total, SENT_ACC, dtype=np.float32), np.zeros(16, dtype=np.float32)
    for i, live in enumerate(lives):
        g_host = _grads(segs, total, live, seed + i)
        g, g_whole = _guarded(g_host, SENT_G)
        ctl.live[:NCLS] = torch.tensor(live)
        first, publish = i == 0, publish_last and i == len(lives) - 1
        ops.grad_accum(acc, g, table, ctl, actl, first, publish)
        torch.cuda.synchronize()
        ref_acc, ref_live, ref_pub = ops.grad_accum_reference(ref_acc, g_host.numpy(), segs, live, ref_live, first)
        _same_bits(acc.cpu().numpy(), ref_acc, f"call {i}")
        assert torch.equal(g_whole.view(torch.int32), _guarded(g_host, SENT_G)[1].view(torch.int32)), "g was written"
        assert bool((acc_whole[:MARGIN] == SENT_ACC).all()) and bool((acc_whole[-MARGIN:] == SENT_ACC).all()), "a store left acc"
        r = actl.read()
        assert r["live"].tolist() == ref_live.tolist() and r["n_micro"] == i + 1 and r["n_cycles"] == int(publish), (i, r)
        want_ctl = ref_pub.tolist() if publish else list(live) + [0.0] * (16 - NCLS)
        assert ctl.live.cpu().tolist() == want_ctl, (i, "ctl.live")
        assert torch.equal(ctl.buf[:3 + 16].view(torch.int32), head.view(torch.int32)), "ctl.lr / ctl.step were written"
    # gaps, the malformed segment and the dead class: the sentinel survived every call
    owned = np.zeros(total, dtype=bool)
    touched = {c for live in lives for c in range(NCLS) if live[c] > 0}
    for lo, n, grp, c in segs:
        if n % 4 == 0 and c in touched:
            owned[lo:lo + n] = True
    final = acc.cpu().numpy()
    assert np.all(final[~owned] == np.float32(SENT_ACC)) and (~owned).sum() > 8 * 4 and not np.all(final[owned] == np.float32(SENT_ACC))
    return acc_whole.cpu().numpy().tobytes() + actl.buf.cpu().numpy().tobytes() + ctl.buf.cpu().numpy().tobytes()


SMALL = [4, 4096, 4100, 64, 8192, 12292] + [4] * 120 + [4100, 4]        # smallest, one chunk, a chunk + a 4-element tail, many small ones


def test_three_calls_equal_the_restatement_bit_for_bit():
    segs, total = _layout(SMALL)
    assert {c for *_, c in segs} == set(range(NCLS)) and {g for _, _, g, _ in segs} == {0, 1, 2}
    _sequence(segs, total, LIVES, 1)


def test_a_cycle_without_publish_leaves_ctl_live_alone():
    segs, total = _layout(SMALL[:8])
    _sequence(segs, total, LIVES[:2], 5, publish_last=False)


def test_second_trip_through_the_chunk_loop():
    """one table above grid x chunk_elems of the launch geometry: the first workgroups take a second chunk, the last chunk is a partial one"""
    grid, chunk, _ = _ops().adam_table_geometry()
    n = grid * chunk + 3 * chunk + 192
    segs = [(8, n, 2, 0), (8 + n + 8, 128, 0, 1), (8 + n + 8 + 128, 4100, 1, 3)]           # (the middle one: dead)
    total = 8 + n + 8 + 128 + 4100 + 8
    _sequence(segs, total, LIVES[:2], 9)


def test_two_identical_call_sequences_give_identical_bytes():
    segs, total = _layout(SMALL)
    assert _sequence(segs, total, LIVES, 21) == _sequence(segs, total, LIVES, 21)


def test_refusals_return_minus_two_before_any_launch():
    from avsiam_amd import _lib
    lib = _lib.load()
    ops = _ops()
    table, ctl, actl = _raw_table([(0, 64, 0, 0)], 64), ops.AdamCtl("cuda"), ops.GradAccumCtl("cuda")
    ctl.live[0] = 1.0
    acc, g = torch.full((64,), 5.0, device="cuda"), torch.ones(64, device="cuda")
    ptr = lambda t: t.data_ptr()
    good = [ptr(acc), ptr(g), ptr(table.dev), 1, 1, ptr(ctl.buf), ptr(actl.buf), 1, 1, None]
    for i, bad in ((0, None), (1, None), (2, None), (5, None), (6, None), (1, ptr(acc)), (3, 0), (3, 4097), (4, 0), (0, ptr(acc) + 4)):
        a = list(good)
        a[i] = bad
        assert lib.avs_grad_accum(*a) == -2 and b"grad_accum" in lib.avs_last_error(), (i, bad)
    with pytest.raises(_lib.AvsiamHipError, match="overlap"):
        ops.grad_accum(acc, acc[0:64], table, ctl, actl, True, False)
    torch.cuda.synchronize()
    r = actl.read()
    assert r["n_micro"] == 0 and r["n_cycles"] == 0 and float(acc.min()) == 5.0            # nothing ran
    assert lib.avs_grad_accum(*good) == 0
    torch.cuda.synchronize()
    assert actl.read()["n_micro"] == 1 and float(acc.max()) == 1.0


# ---- the model -----------------------------------------------------------------------------------------------------------------
L, B = 527, 2
CFG = AVSiamConfig(depth=2)
KW = dict(head_lr=100.0, mm_lr=100.0)
LR = 1e-4


def _model(freeze=False, seed=5):
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import apply_freeze_base
    m = CAVMAEFT_BASE(L, cfg=CFG, init_seed=seed, init_mode="random").cuda()
    m.requires_grad_(True)
    apply_freeze_base(m, freeze)
    m._train_engine(B, 1).opts.deterministic = True          # with the "det" knob: one writer per gradient element, so twins agree byte for byte
    return m


def _labels(seed, n=B):
    hot = (torch.rand(n, L, generator=torch.Generator().manual_seed(seed)) < 0.03).float()
    hot[:, 0] = 1.0
    return hot * 0.9 + 0.1 / L


def _batch(seed):
    a, v = synth_inputs(CFG, B, seed)
    return a.cuda(), v.unsqueeze(1).cuda(), _labels(seed + 1000).cuda()


def _state(m):
    lo, hi = m.arena.range[1]
    zeros = lambda: torch.zeros(hi - lo, device="cuda")
    return {"p": m.arena.p.clone(), "pb": m.arena.pb.clone().view(torch.int16),
            "m": m._opt["m"].clone() if m._opt is not None else zeros(), "v": m._opt["v"].clone() if m._opt is not None else zeros()}


def _same(x, y, what):
    for k in x:
        assert torch.equal(x[k].view(torch.int16 if x[k].element_size() == 2 else torch.int32),
                           y[k].view(torch.int16 if y[k].element_size() == 2 else torch.int32)), (what, k, int((x[k] != y[k]).sum()))


def _step(m, batch, branch="mm", ftmode="mm_grad", labels=None, **kw):
    a, v, y = batch
    return m.train_step(a, v, y if labels is None else labels, LR, ftmode, branch=branch if ftmode == "mm_grad" else None, **KW, **kw)


@pytest.fixture
def det():
    from avsiam_amd import _lib
    old = _lib.tuning_get("det")
    _lib.tuning_set("det", 1)
    yield
    _lib.tuning_set("det", old)


@pytest.mark.parametrize("freeze", [False, True])
@pytest.mark.parametrize("branch", ["mm", "a", "v", "audioonly"])
def test_a_cycle_of_one_micro_step_is_the_plain_step(det, branch, freeze):
    ftmode = "audioonly" if branch == "audioonly" else "mm_grad"
    batch = _batch(51)
    plain, acc = _model(freeze), _model(freeze)
    acc.set_grad_accumulation(2)
    l_p, l_a = _step(plain, batch, branch, ftmode), _step(acc, batch, branch, ftmode)
    assert acc.accum_state() == {"k": 2, "pending": 1} and plain.accum_state() == {"k": 1, "pending": 0}
    acc.apply_accumulated(LR, **KW)
    torch.cuda.synchronize()
    assert float(l_p) == float(l_a)
    assert acc.accum_state() == {"k": 2, "pending": 0}
    _same(_state(plain), _state(acc), "flush after one micro-step vs the plain step")
    assert acc.optimizer_steps() == plain.optimizer_steps() and set(plain.optimizer_steps().values()) == {1}
    assert all(p.grad is None for p in acc.parameters())
    acc.apply_accumulated(LR, **KW)                           # nothing pending: a no-op
    torch.cuda.synchronize()
    _same(_state(plain), _state(acc), "a flush with nothing pending")
    assert acc._acc["actl"].read()["n_cycles"] == 1


def _host_sum(m, grads, branches):
    """the numpy fp32 sum, in micro-step order, of the gradient arenas read after each micro-step: copy on first touch, per class"""
    from avsiam_amd.models.cav_mae_ft import CLASSES, live_classes
    from avsiam_amd.ft_train import OUT, OUT_A, OUT_V
    ops = _ops()
    segs = m._dps["table"].segs
    reach = {"mm": live_classes("mm_grad", OUT), "a": live_classes("audioonly", OUT_A), "v": live_classes("videoonly", OUT_V)}
    present = {CLASSES[c] for *_, c in segs}
    acc, live = np.full(grads[0].shape, np.float32(SENT_ACC)), np.zeros(16, dtype=np.float32)
    for i, (g, br) in enumerate(zip(grads, branches)):
        now = [1.0 if (c in reach[br] and c in present) else 0.0 for c in CLASSES]
        acc, live, _ = ops.grad_accum_reference(acc, g, segs, now, live, first=(i == 0))
    return acc, live, segs


def _union_mask(segs, live, n):
    mask = np.zeros(n, dtype=bool)
    for lo, cnt, grp, c in segs:
        if live[c] > 0:
            mask[lo:lo + cnt] = True
    return mask


@pytest.mark.parametrize("freeze", [False, True])
def test_a_cycle_of_three_branches(det, freeze):
    from avsiam_amd.models.cav_mae_ft import CLASSES
    ops = _ops()
    m = _model(freeze)
    m.set_grad_accumulation(3)
    lo0, hi0 = m.arena.range[1]
    branches = ("mm", "a", "v")
    before, grads = _state(m), []
    for i, br in enumerate(branches[:2]):
        _step(m, _batch(60 + i), br)
        torch.cuda.synchronize()
        grads.append(m.arena.g[lo0:hi0].cpu().numpy().copy())
        _same(_state(m), before, f"after micro-step {i + 1}")
        assert m.optimizer_steps() == {} and m.accum_state() == {"k": 3, "pending": i + 1}
    _step(m, _batch(62), branches[2])
    torch.cuda.synchronize()
    grads.append(m.arena.g[lo0:hi0].cpu().numpy().copy())
    assert m.accum_state() == {"k": 3, "pending": 0}
    # (b) the buffer: the fp32 sum in micro-step order, bit for bit over the union's segments
    want, live, segs = _host_sum(m, grads, branches)
    mask = _union_mask(segs, live, hi0 - lo0)
    got = m.accum_buffer().cpu().numpy()
    assert mask.sum() > 0 and np.array_equal(got[mask].view(np.uint32), want[mask].view(np.uint32))
    union = {CLASSES[c] for c in range(len(CLASSES)) if live[c] > 0}
    assert {"mlp_head", "mlp_head_a", "mlp_head_mm", "mm"} <= union and ("base_s" in union) == (not freeze)
    # (c) the step: ops.adam_table on clones of the pre-cycle state with that sum, the union and grad_scale 1 / 3
    ctl = ops.AdamCtl("cuda")
    ctl.live.copy_(torch.from_numpy(live))
    ctl.set_lr(LR, LR * KW["head_lr"], LR * KW["mm_lr"])
    p, pb = before["p"][lo0:hi0].clone(), before["pb"].view(torch.bfloat16)[lo0:hi0].clone()
    ops.adam_table(p, torch.from_numpy(want).cuda(), before["m"], before["v"], pb, m._dps["table"], ctl, *BETAS, EPS, WD, grad_scale=1.0 / 3)
    torch.cuda.synchronize()
    now = _state(m)
    _same({"p": now["p"][lo0:hi0], "pb": now["pb"][lo0:hi0], "m": now["m"], "v": now["v"]},
          {"p": p, "pb": pb.view(torch.int16), "m": before["m"], "v": before["v"]}, "the accumulated step vs ops.adam_table")
    assert torch.equal(now["p"][:lo0], before["p"][:lo0]) and torch.equal(now["p"][hi0:], before["p"][hi0:])
    assert not torch.equal(now["p"], before["p"])
    assert m.optimizer_steps() == {c: 1 for c in union}, "every union class steps once"


def test_the_flush_after_two_of_three_is_a_cycle_of_two(det):
    x, y = _model(), _model()
    x.set_grad_accumulation(3)
    y.set_grad_accumulation(2)
    for i, br in enumerate(("a", "mm")):
        _step(x, _batch(70 + i), br)
        _step(y, _batch(70 + i), br)
        assert x.accum_state() == {"k": 3, "pending": i + 1} and y.accum_state() == {"k": 2, "pending": (i + 1) % 2}
    x.apply_accumulated(LR, **KW)
    torch.cuda.synchronize()
    assert x.accum_state() == {"k": 3, "pending": 0}
    _same(_state(x), _state(y), "flush after 2 of 3 vs k = 2")
    assert x.optimizer_steps() == y.optimizer_steps() and set(x.optimizer_steps().values()) == {1}
    # the next cycle starts afresh on both (classes of the old cycle are not carried over)
    for i, br in enumerate(("v", "v")):
        _step(x, _batch(80 + i), br)
        _step(y, _batch(80 + i), br)
    x.apply_accumulated(LR, **KW)
    torch.cuda.synchronize()
    _same(_state(x), _state(y), "second cycle")
    assert x.optimizer_steps() == y.optimizer_steps() and x.optimizer_steps()["mlp_head_a"] == 1 and x.optimizer_steps()["mlp_head"] == 1
    assert x.optimizer_steps()["base_v"] == 2
    x.set_grad_accumulation(None)
    assert x.accum_state() == {"k": 1, "pending": 0} and x.accum_buffer() is None


# ---- parity at the effective batch ----------------------------------------------------------------------------------------------
GRAD_COS, GRAD_NORM = 0.9998, 1e-2                        # the bounds of tests/test_ft_train_gpu.py


def _oracle_grads(P, cfg, a, v, fn):
    """autograd through the CPU oracle (tests/test_ft_train_gpu.py): fn(outputs) -> loss; -> (loss, {name: grad or None})"""
    from oracle import ref_cpu
    torch.set_num_threads(16)
    leaf = {k: t.clone().requires_grad_(True) for k, t in P.items()}
    loss = fn(ref_cpu.ft_forward(leaf, cfg, a, v, fn.mode))
    loss.backward()
    return float(loss.detach()), {k: (t.grad if t.grad is not None else None) for k, t in leaf.items()}


def test_two_micro_batches_of_two_against_the_oracle_at_batch_four():
    a, v = synth_inputs(CFG, 2 * B, 91)
    v, y = v.unsqueeze(1), _labels(92, 2 * B)
    m = _model(seed=4)
    m._train_engine(B, 1).opts.deterministic = False           # parity, not bytes: the default kernels
    m.set_grad_accumulation(2)
    losses = [m.train_step(a[i:i + B].cuda(), v[i:i + B].cuda(), y[i:i + B].cuda(), LR, "mm_grad", branch="mm", **KW) for i in (0, B)]
    torch.cuda.synchronize()

    def fn(o):
        return F.binary_cross_entropy_with_logits(o[0], y)
    fn.mode = "mm_grad"
    ref_loss, ref = _oracle_grads(synth_state_ft(CFG, L, 4, "random"), CFG, a, v, fn)
    loss = sum(float(x) for x in losses) / 2
    assert abs(loss - ref_loss) <= 2e-3 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    lo0, _ = m.arena.range[1]
    buf = m.accum_buffer().double().cpu() / 2
    worst_cos, worst_norm, seen = 1.0, 0.0, 0
    for n, r in ref.items():
        if r is None or n not in m._params or not m.arena.info[n].live:
            continue
        at = m.arena.offset[n] - lo0
        g, r = buf[at:at + r.numel()], r.double().reshape(-1)
        rn = float(r.norm())
        if rn == 0:
            assert float(g.norm()) == 0, n
            continue
        cos, nr = float(g @ r) / (float(g.norm()) * rn + 1e-300), abs(float(g.norm()) / rn - 1)
        print(f"{n}: cos {cos:.7f} norm err {nr:.3e}")
        worst_cos, worst_norm, seen = min(worst_cos, cos), max(worst_norm, nr), seen + 1
    print(f"accumulated 2 x {B} vs oracle at {2 * B}: worst cos {worst_cos:.7f}, worst norm err {worst_norm:.3e} over {seen} tensors")
    record_margin("grad_accum.parity_2x2_vs_oracle_b4", worst_cos=worst_cos, worst_norm=worst_norm, loss_err=abs(loss - ref_loss), tensors=seen)
    assert seen > 20 and worst_cos >= GRAD_COS and worst_norm <= GRAD_NORM, (worst_cos, worst_norm)


# ---- the guard over the accumulated step ----------------------------------------------------------------------------------------
def test_guarded_cycle_skips_as_a_whole_and_reports_the_norm_of_the_mean(det):
    m = _model()
    m.set_grad_guard()
    m.set_grad_accumulation(3)
    _step(m, _batch(100), "mm")
    before, steps = _state(m), m.optimizer_steps()
    bad = _batch(101)[2].clone()
    bad[1, 7] = INF
    _step(m, _batch(101), "a", labels=bad)
    _step(m, _batch(102), "v")
    torch.cuda.synchronize()
    st = m.guard_stats()
    assert st["skipped"] and st["n_nonfinite"] > 0 and st["coef"] == 0.0 and (st["n_skipped"], st["n_steps"]) == (1, 1), st
    _same(_state(m), before, "a non-finite micro-step skips the whole accumulated step")
    assert m.optimizer_steps() == steps == {} and m.accum_state()["pending"] == 0
    # the next cycle is a normal step, with a finite max_norm that does not clip: the norm is that of the MEAN gradient
    lo0, hi0 = m.arena.range[1]
    for i, br in enumerate(("mm", "a", "v")):
        _step(m, _batch(110 + i), br, guard=1e30)
    torch.cuda.synchronize()
    st = m.guard_stats()
    assert not st["skipped"] and st["n_nonfinite"] == 0 and st["coef"] == 1.0 and (st["n_skipped"], st["n_steps"]) == (1, 2), st
    assert not torch.equal(m.arena.p, before["p"]) and set(m.optimizer_steps().values()) == {1}
    live = m._acc["actl"].read()["live"]
    mask = _union_mask(m._dps["table"].segs, live, hi0 - lo0)
    total = m.accum_buffer().double().cpu().numpy()[mask]
    host = np.float32(math.sqrt(math.fsum((total * total).tolist())) / 3)
    ulp = float(np.spacing(host))
    print(f"guarded cycle: device norm {st['norm']!r}, host {float(host)!r}, ulp {ulp:.3e}")
    record_margin("grad_accum.guard_norm_k3", norm=st["norm"], host_norm=float(host), ulps=abs(st["norm"] - float(host)) / ulp)
    assert abs(st["norm"] - float(host)) <= ulp, (st["norm"], float(host))
    assert abs(math.sqrt(st["norm_base"] ** 2 + st["norm_head"] ** 2 + st["norm_mm"] ** 2) - st["norm"]) <= 1e-6 * st["norm"]


# ---- the refusals while micro-steps are pending ---------------------------------------------------------------------------------
def test_pending_micro_steps_refuse_what_would_lose_them(det):
    m = _model()
    for bad in (0, -1, 2.5, True, "2"):
        with pytest.raises(ValueError, match="set_grad_accumulation"):
            m.set_grad_accumulation(bad)
    _step(m, _batch(120))                                      # a plain step first: an Adam state to save
    saved = m.optimizer_state()
    m.set_grad_accumulation(2)
    batch = _batch(121)
    _step(m, batch)
    before = _state(m)
    with pytest.raises(RuntimeError, match="pending"):
        m.requires_grad_(False)
    with pytest.raises(RuntimeError, match="pending"):
        m.adam_step(LR)
    with pytest.raises(RuntimeError, match="pending"):
        m.load_optimizer_state(saved)
    with pytest.raises(RuntimeError, match="pending"):
        m.set_distributed(1, 0)
    with pytest.raises(RuntimeError, match="pending"):
        m.set_grad_accumulation(3)
    with pytest.raises(RuntimeError, match="pending"):
        m.set_grad_accumulation(None)
    with pytest.raises(RuntimeError, match="pending"):        # a backward of the autograd path
        out = m(batch[0], batch[1], "mm_grad")
        F.binary_cross_entropy_with_logits(out[0], batch[2]).backward()
    name, p = next((n, p) for n, p in m.named_parameters() if n.startswith("mlp_head_a"))
    p.requires_grad_(False)                                    # the freeze loop: per parameter, seen at the next step
    with pytest.raises(RuntimeError, match="trainable set changed"):
        _step(m, batch)
    with pytest.raises(RuntimeError, match="trainable set changed"):
        m.apply_accumulated(LR, **KW)
    p.requires_grad_(True)
    torch.cuda.synchronize()
    _same(_state(m), before, "the refusals touched nothing")
    assert m.accum_state() == {"k": 2, "pending": 1}
    m.apply_accumulated(LR, **KW)                              # ... after which everything is allowed again
    m.requires_grad_(True)
    m.load_optimizer_state(m.optimizer_state())
    m.set_grad_accumulation(None)
    torch.cuda.synchronize()
    assert not torch.equal(m.arena.p, before["p"])
    # ... and a model that never heard of accumulation issues the calls it issued before
    _assert_plain_step_is_the_parents()


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def test_the_loop_steps_every_k_batches_and_flushes_at_the_epoch_end(tmp_path, monkeypatch):
    """traintest_ft_base.train with --accum-steps 2 over two epochs of three batches: six micro-steps, and four optimizer steps - one
    after the second batch of each epoch, one at each epoch's end for the batch left over - so that validation and the checkpoint meet a
    cycle boundary"""
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.run_cavmae_ft_base import build_parser
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, train
    ops = _ops()
    args = build_parser().parse_args(["--ftmode", "audioonly", "--n_class", str(L), "--lr", "1e-4", "--head_lr", "100", "--batch_size", str(B),
                                      "--n_epochs", "2", "--steps-per-epoch", "3", "--val-steps", "1", "--accum-steps", "2", "--exp_dir", str(tmp_path)])
    m = CAVMAEFT_BASE(L, cfg=CFG, init_seed=5, init_mode="random").cuda()
    calls = {"accum": [], "adam": 0}
    accum, adam = ops.grad_accum, ops.adam_table
    monkeypatch.setattr(ops, "grad_accum", lambda acc, g, table, ctl, actl, first, publish: (calls["accum"].append((bool(first), bool(publish))),
                                                                                           accum(acc, g, table, ctl, actl, first, publish))[1])
    monkeypatch.setattr(ops, "adam_table", lambda *a, **k: (calls.__setitem__("adam", calls["adam"] + 1), adam(*a, **k))[1])
    pending_at_validation = []
    import avsiam_amd.traintest_ft_base as loop
    validate = loop.validate
    monkeypatch.setattr(loop, "validate", lambda model, *a, **k: (pending_at_validation.append(model.accum_state()["pending"]), validate(model, *a, **k))[1])
    dev = m.arena.p.device
    out = train(m, SyntheticFtLoader(CFG, B, 3, L, dev, seed=87), SyntheticFtLoader(CFG, B, 1, L, dev, seed=88), None, args)
    torch.cuda.synchronize()
    assert calls["accum"] == [(True, False), (False, True), (True, False)] * 2 and calls["adam"] == 4
    assert pending_at_validation == [0, 0] and m.accum_state() == {"k": 2, "pending": 0}
    assert m.optimizer_steps() == {"base_a": 4, "base_s": 4, "mlp_head_a": 4}
    assert m._acc["actl"].read()["n_cycles"] == 4
    assert np.all(np.isfinite(out["result"][:, 3])) and not out.get("diverged")


# one plain fine-tuning step on the parent commit (tools/step_digest.py --ft --trace --batch 3, profiles/r14/frames_bench.json)
PARENT_DIGEST = {"trace_calls": 303, "trace": "21a456a12665402bb61ad36021b881415531210137bfe83da2f626bd146a239a", "calls_per_step": [301],
                 "p": "57f087e095055fa51785f681a6cb583fc4ce92b4c8bd85342575a3445db100b9", "g": "8717c34280ebc640d3e247807d9c6eec5f13a0d6188b234c2c9c323538cd2c46",
                 "adam_m": "887c7d3accf9731d8b7c0ad334b807b47c7b4a7ac999d026edbddab608d08406", "adam_v": "5c9624b28e55299fdb1dfa8a9d0b9526bcf2c182c6e0aa736b211926c9010abb"}


def _assert_plain_step_is_the_parents():
    """without the new call nothing moved: the library-call list of a plain step (entry points, scalar arguments, tensor shapes) and the arenas
    after it hash to what the parent commit gives"""
    r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print("step digest:", {k: got[k] for k in PARENT_DIGEST})
    assert {k: got[k] for k in PARENT_DIGEST} == PARENT_DIGEST


# ---- two ranks on one GPU -------------------------------------------------------------------------------------------------------
SEQ = {0: ("mm", "a", "v", "mm"), 1: ("v", "v", "mm", "a")}              # two cycles of k = 2, the ranks on different branches
# cycle 1 reaches everything but mlp_head_a on rank 1 and everything on rank 0; cycle 2 likewise the other way round: every class, twice
WANT_STEPS = {"base_a": 2, "base_v": 2, "base_s": 2, "mm": 2, "mlp_head_mm": 2, "mlp_head": 2, "mlp_head_a": 2}


def _sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _same_on_both_ranks(dist, value):
    box = [None, None]
    dist.all_gather_object(box, value)
    return box[0] == box[1]


def _rank_model(rank, world):
    from avsiam_amd import _lib
    from avsiam_amd.comm import HostStagedComm
    from avsiam_amd.models import CAVMAEFT_BASE
    _lib.tuning_set("det", 1)
    m = CAVMAEFT_BASE(L, cfg=CFG, init_seed=21, init_mode="random").cuda()
    m.requires_grad_(True)
    m._train_engine(B, 1).opts.deterministic = True
    m.set_distributed(world, rank, HostStagedComm())
    m.set_grad_accumulation(2)
    return m


def _cycles_section(rank, world, dist):
    m = _rank_model(rank, world)
    for i, branch in enumerate(SEQ[rank]):
        before = _sha(m.arena.p)
        _step(m, _batch(200 + 10 * i + rank), branch)
        torch.cuda.synchronize()
        assert m.accum_state()["pending"] == (i + 1) % 2
        if i % 2 == 0:
            assert _sha(m.arena.p) == before, "a micro-step that does not end the cycle moved the weights"
        else:
            assert _sha(m.arena.p) != before
            assert _same_on_both_ranks(dist, _sha(m.arena.p, m.arena.pb.view(torch.int16), m._opt["m"], m._opt["v"], m._dps["ctl"].buf,
                                                  m._acc["actl"].buf)), f"cycle {i // 2}: the ranks differ"
    assert m.optimizer_steps() == WANT_STEPS, m.optimizer_steps()


def _skip_section(rank, world, dist):
    m = _rank_model(rank, world)
    m.set_grad_guard()
    _step(m, _batch(300 + rank), "mm")
    _step(m, _batch(310 + rank), "mm")
    torch.cuda.synchronize()
    before, steps = _sha(m.arena.p, m.arena.pb.view(torch.int16), m._opt["m"], m._opt["v"]), m.optimizer_steps()
    assert set(steps.values()) == {1}
    y = _batch(320 + rank)[2].clone()
    if rank == 1:
        y[0, 3] = INF
    _step(m, _batch(320 + rank), SEQ[rank][0], labels=y)       # the bad micro-step is the FIRST of the cycle, on rank 1 alone
    _step(m, _batch(330 + rank), SEQ[rank][1])
    torch.cuda.synchronize()
    st = m.guard_stats()
    assert st["skipped"] and st["n_nonfinite"] > 0 and (st["n_skipped"], st["n_steps"]) == (1, 2), (rank, st)
    assert _sha(m.arena.p, m.arena.pb.view(torch.int16), m._opt["m"], m._opt["v"]) == before and m.optimizer_steps() == steps
    assert _same_on_both_ranks(dist, _sha(m.arena.p, m._guard.buf))


def _worker(rank, world, port, q):
    import datetime
    import traceback
    import torch.distributed as dist
    res = {}
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        for name, fn in (("cycles", _cycles_section), ("skip", _skip_section)):
            try:
                fn(rank, world, dist)
                res[name] = "ok"
            except Exception:
                res[name] = traceback.format_exc()
                break                                        # (the ranks are out of step now: the peer's collectives time out)
    except Exception:  # pragma: no cover
        res["init"] = traceback.format_exc()
    finally:
        q.put((rank, res))
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    """ONE run of two worker processes for the tests below.  The parent waits with a deadline, terminates the workers on expiry and fails."""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            rank, r = q.get(timeout=300)
            res[rank] = r
    except queue.Empty:
        pass
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    if len(res) != 2:
        pytest.fail(f"worker(s) silent at the deadline (answers: {res})")
    return res


@pytest.mark.parametrize("section", ["cycles", "skip"])
def test_two_ranks_on_one_gpu(two_ranks, section):
    """cycles: two cycles of k = 2, rank 0 on mm, a | v, mm and rank 1 on v, v | mm, a - weights, shadows, moments and both device blocks
    byte-identical on both ranks after each cycle, every class stepped once per cycle.  skip: an inf label on rank 1 alone, in the first
    micro-step of a cycle - both ranks skip the accumulated step, nothing moves on either."""
    for rank in range(2):
        got = two_ranks[rank]
        assert "init" not in got, got["init"]
        assert section in got, f"rank {rank}: not reached ({got})"
        assert got[section] == "ok", f"rank {rank}: {got[section]}"
