"""The guard of the fine-tuning step on a real MI355X (csrc/grad_guard.hip; CAVMAEFT_BASE.set_grad_guard).

1. ``avs_grad_sumsq`` against ops.grad_guard_reference (float64, math.fsum; pinned to torch's clip_grad_norm_ in tests/test_grad_guard_cpu.py).
   Gradients from the lattice k * 2^-10, |k| <= 64: every square is a multiple of 2^-20 and every partial sum stays below 2^53 of them, so ANY
   summation order is exact and the device block must equal the restatement bit for bit.  Gaussian gradients: the bound of a sum of n
   non-negative doubles in any order, |total - fsum| <= n * 2^-53 * fsum, and the norm within 1 ulp of fp32.
2. ``avs_adam_table_guarded`` against ``avs_adam_table`` byte for byte, and its skip.
3. The model: a guarded step against the plain one (depth 2, batch 3, every branch, with and without freeze_base).
4. The digest of a plain step is the parent's.
5. Two gloo ranks sharing the GPU: guarded steps leave identical bytes on both ranks, a non-finite gradient on one rank skips both.
Measured margins go through tests.helpers.record_margin (profiles/r19/grad_guard_margins.json is their copy)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS, EPS, WD = (0.95, 0.999), 1e-8, 5e-7
LRS = (1e-3, 5e-2, 2e-4)
NCLS = 5
LIVE = [1.0, 0.0, 2.0, 1.0, 1.0]                     # class 1 is dead; 2.0: what a class two ranks reached sums to
INF = float("inf")


def _ops():
    from avsiam_amd import ops
    return ops


# ---- 1. the sums -------------------------------------------------------------------------------------------------------------
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


def _fill(segs, total, kind, seed):
    """NaN everywhere (gaps, the malformed segment, dead classes); the segments of live classes from the lattice or a Gaussian"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((total,), float("nan"))
    for lo, n, grp, c in segs:
        if n % 4 == 0 and LIVE[c] > 0:
            g[lo:lo + n] = (torch.randint(-64, 65, (n,), generator=gen).float() / 1024) if kind == "lattice" else torch.randn(n, generator=gen) * 0.05
    return g


def _ctl():
    ops = _ops()
    ctl = ops.AdamCtl("cuda")
    ctl.live[:NCLS] = torch.tensor(LIVE)
    return ctl


def _sumsq(g, segs, total, scale, max_norm):
    ops = _ops()
    table, ctl, guard = _raw_table(segs, total), _ctl(), ops.GradGuard("cuda")
    ops.grad_sumsq(g.cuda(), table, ctl, guard, grad_scale=scale, max_norm=max_norm)
    torch.cuda.synchronize()
    return guard, table, ctl


def _assert_bitwise(got, ref):
    assert got["sumsq"].tobytes() == ref["sumsq"].tobytes(), (got["sumsq"], ref["sumsq"])
    assert got["sumsq_cls"].tobytes() == ref["sumsq_cls"].tobytes()
    for k in ("total", "norm", "coef"):
        assert np.float64(got[k]).tobytes() == np.float64(ref[k]).tobytes(), (k, got[k], ref[k])
    assert (got["n_nonfinite"], got["skip"]) == (ref["n_nonfinite"], ref["skip"])


SMALL = [4, 4096, 4100, 64, 8192, 12292] + [4] * 120 + [4100, 4]        # smallest, one chunk, a chunk + a 4-element tail, many small ones


@pytest.mark.parametrize("scale,max_norm", [(1.0, 0.75), (0.5, INF), (0.25, 1e-9)])
def test_sums_on_the_lattice_equal_the_restatement_bit_for_bit(scale, max_norm):
    ops = _ops()
    segs, total = _layout(SMALL)
    assert {c for *_, c in segs} == set(range(NCLS)) and {g for _, _, g, _ in segs} == {0, 1, 2}
    g = _fill(segs, total, "lattice", 1)
    guard, table, ctl = _sumsq(g, segs, total, scale, max_norm)
    got, ref = guard.read(), ops.grad_guard_reference(g.numpy(), segs, LIVE, scale, max_norm)
    _assert_bitwise(got, ref)
    assert got["n_nonfinite"] == 0 and got["skip"] == 0 and (got["n_skipped"], got["n_steps"]) == (0, 1)
    assert (got["coef"] < 1.0) == (max_norm != INF) and (max_norm != INF or got["coef"] == 1.0)
    # two calls give identical bytes (a second block and workspace; the counters of the first go on counting)
    again = ops.GradGuard("cuda")
    ops.grad_sumsq(g.cuda(), table, ctl, again, grad_scale=scale, max_norm=max_norm)
    ops.grad_sumsq(g.cuda(), table, ctl, guard, grad_scale=scale, max_norm=max_norm)
    torch.cuda.synchronize()
    assert torch.equal(again.buf.view(torch.uint8), torch.from_numpy(np.frombuffer(_block_bytes(got), dtype=np.uint8).copy()).cuda())
    assert torch.equal(again.ws, guard.ws)
    assert guard.read()["n_steps"] == 2 and guard.read()["n_skipped"] == 0


def _block_bytes(r):
    """the 184 bytes of an avs_grad_guard holding the fields of `r`"""
    return (r["sumsq"].tobytes() + r["sumsq_cls"].tobytes() + np.float64(r["total"]).tobytes() + np.float32([r["norm"], r["coef"]]).tobytes()
            + np.int32([r["n_nonfinite"], r["skip"], r["n_skipped"], r["n_steps"]]).tobytes())


def test_sums_second_trip_through_the_chunk_loop():
    """one table above grid x chunk_elems of the launch geometry: the first workgroups take a second chunk, the last chunk is a partial one"""
    ops = _ops()
    grid, chunk, _ = ops.adam_table_geometry()
    n = grid * chunk + 3 * chunk + 192
    segs = [(8, n, 2, 0), (8 + n + 8, 128, 0, 1), (8 + n + 8 + 128, 4100, 1, 3)]           # (the middle one: dead and NaN)
    total = 8 + n + 8 + 128 + 4100 + 8
    g = _fill(segs, total, "lattice", 2)
    guard, *_ = _sumsq(g, segs, total, 1.0, 3.0)
    got, ref = guard.read(), ops.grad_guard_reference(g.numpy(), segs, LIVE, 1.0, 3.0)
    _assert_bitwise(got, ref)
    assert got["coef"] < 1.0 and got["sumsq"][2] > 0 and got["sumsq"][0] == 0


def test_sums_of_gaussian_gradients_within_the_derived_bound():
    ops = _ops()
    segs, total = _layout(SMALL)
    g = _fill(segs, total, "gauss", 3)
    guard, *_ = _sumsq(g, segs, total, 0.5, 0.01)
    got, ref = guard.read(), ops.grad_guard_reference(g.numpy(), segs, LIVE, 0.5, 0.01)
    n = sum(n for lo, n, grp, c in segs if n % 4 == 0 and LIVE[c] > 0)
    err = abs(got["total"] - ref["total"]) / ref["total"]
    ulp = float(np.spacing(np.float32(ref["norm"])))
    print(f"gaussian: n {n} rel err of total {err:.3e} (bound {n * 2.0 ** -53:.3e}); norm {got['norm']!r} vs {ref['norm']!r}, ulp {ulp:.3e}")
    record_margin("grad_guard.gaussian_total", rel_err=err, bound=n * 2.0 ** -53, norm_ulps=abs(got["norm"] - ref["norm"]) / ulp)
    assert err <= n * 2.0 ** -53
    assert abs(got["norm"] - ref["norm"]) <= ulp
    for k in ("sumsq", "sumsq_cls"):
        assert np.all(np.abs(got[k] - ref[k]) <= n * 2.0 ** -53 * ref[k])
    assert got["n_nonfinite"] == 0 and 0 < got["coef"] < 1


def test_nonfinite_elements_are_counted_and_left_out():
    ops = _ops()
    segs, total = [(8, 3 * 4096 + 4, 0, 0), (8 + 3 * 4096 + 4 + 8, 64, 1, 2)], 8 + 3 * 4096 + 4 + 8 + 64 + 8
    g = _fill(segs, total, "lattice", 4)
    clean = ops.grad_guard_reference(g.numpy(), segs, LIVE, 1.0, 1.0)
    first, last = 8 + 4096, 8 + 2 * 4096 - 1                       # the second chunk's first and last element
    gone = float(g[first]) ** 2 + float(g[last]) ** 2
    g[first], g[last] = INF, float("nan")
    guard, *_ = _sumsq(g, segs, total, 1.0, 1.0)
    got = guard.read()
    _assert_bitwise(got, ops.grad_guard_reference(g.numpy(), segs, LIVE, 1.0, 1.0))
    assert got["n_nonfinite"] == 2 and got["skip"] == 1 and got["coef"] == 0.0 and (got["n_skipped"], got["n_steps"]) == (1, 1)
    assert got["sumsq"][0] == clean["sumsq"][0] - gone and got["sumsq"][1] == clean["sumsq"][1]


def test_refusals_return_minus_two_before_any_launch():
    from avsiam_amd import _lib
    lib = _lib.load()
    ops = _ops()
    segs = [(0, 64, 0, 0)]
    table, ctl, guard = _raw_table(segs, 64), _ctl(), ops.GradGuard("cuda")
    g = torch.zeros(64, device="cuda")
    ws, need = guard.workspace(table)
    assert need == lib.avs_grad_sumsq_ws_bytes(1, 1) and lib.avs_grad_sumsq_ws_bytes(0, 1) == 0 and lib.avs_grad_sumsq_ws_bytes(1, 0) == 0
    ptr = lambda t: t.data_ptr()
    good = [ptr(g), ptr(table.dev), 1, ptr(ctl.buf), 1.0, 1.0, ptr(guard.buf), ptr(ws), need, None]
    for i, bad in ((0, None), (1, None), (3, None), (6, None), (7, None), (2, 0), (2, 4097), (5, 0.0), (5, float("nan")), (4, INF), (8, need - 1), (8, 0)):
        a = list(good)
        a[i] = bad
        assert lib.avs_grad_sumsq(*a) == -2 and b"grad_sumsq" in lib.avs_last_error(), (i, bad)
    z = torch.zeros(64, device="cuda")
    adam = [ptr(z), ptr(g), ptr(z), ptr(z), None, ptr(table.dev), 1, 1, ptr(ctl.buf), 0.9, 0.999, 1e-8, 0.0, 1.0, ptr(guard.buf), None]
    for i, bad in ((0, None), (1, None), (5, None), (8, None), (14, None), (6, 0), (7, 0)):
        a = list(adam)
        a[i] = bad
        assert lib.avs_adam_table_guarded(*a) == -2 and b"adam_table_guarded" in lib.avs_last_error(), (i, bad)
    torch.cuda.synchronize()
    assert guard.read()["n_steps"] == 0 and float(z.abs().max()) == 0.0            # nothing ran


# ---- 2. the guarded Adam -----------------------------------------------------------------------------------------------------
MARGIN = 64


def _adam_state(total, seed):
    """p, m, v, p_bf16 as views into buffers with MARGIN sentinel elements on either side -> (views, whole buffers)"""
    gen = torch.Generator().manual_seed(seed)
    whole = [torch.full((total + 2 * MARGIN,), s, device="cuda") for s in (3.25, -0.5, 0.75)] + \
            [torch.full((total + 2 * MARGIN,), 9.0, dtype=torch.bfloat16, device="cuda")]
    views = [w[MARGIN:MARGIN + total] for w in whole]
    views[0].copy_(torch.randn(total, generator=gen))
    views[1].copy_(torch.randn(total, generator=gen) * 0.01)
    views[2].copy_(torch.rand(total, generator=gen) * 1e-3)
    return views, whole


ADAM_LENGTHS = [4, 4096, 4100, 64, 8192] + [4] * 40 + [12292]


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("scale,max_norm", [(0.5, 0.3), (1.0, INF)])
def test_guarded_adam_equals_adam_table_with_the_folded_scale(with_shadow, scale, max_norm):
    ops = _ops()
    segs, total = _layout(ADAM_LENGTHS)
    segs = [s for s in segs if s[1] % 4 == 0]                       # (ops.adam_table's own table: validated)
    g = torch.nan_to_num(_fill(segs, total, "gauss", 5), nan=123.0).cuda()         # dead classes and gaps: finite here, they must simply stay unread
    table = ops.AdamTable(segs, NCLS, total, "cuda")
    steps = [0, 1, 7, 1, 3]
    ctls = [_ctl(), _ctl()]
    for c in ctls:
        c.step[:NCLS] = torch.tensor(steps, dtype=torch.int32)
        c.set_lr(*LRS)
    (gv, gw), (rv, rw) = _adam_state(total, 6), _adam_state(total, 6)
    guard = ops.GradGuard("cuda")
    for call in range(2):
        ops.grad_sumsq(g, table, ctls[0], guard, grad_scale=scale, max_norm=max_norm)
        ops.adam_table_guarded(gv[0], g, gv[1], gv[2], gv[3] if with_shadow else None, table, ctls[0], guard, *BETAS, EPS, WD, grad_scale=scale)
        coef = guard.read()["coef"]
        assert (coef == 1.0) if max_norm == INF else (0 < coef < 1.0)
        folded = float(np.float32(scale) * np.float32(coef))
        ops.adam_table(rv[0], g, rv[1], rv[2], rv[3] if with_shadow else None, table, ctls[1], *BETAS, EPS, WD, grad_scale=folded)
        torch.cuda.synchronize()
        for name, a, b in zip(("p", "m", "v", "p_bf16"), gw, rw):
            assert torch.equal(a, b), (name, call, int((a != b).sum()))
        assert torch.equal(ctls[0].buf.view(torch.int32), ctls[1].buf.view(torch.int32))
    assert ctls[0].step[:NCLS].cpu().tolist() == [k + (2 if l > 0 else 0) for k, l in zip(steps, LIVE)]
    assert not torch.equal(gv[0], torch.randn(total, generator=torch.Generator().manual_seed(6)).cuda())      # (it did step)


@pytest.mark.parametrize("bad", [INF, float("nan")])
def test_guarded_adam_writes_nothing_on_skip(bad):
    ops = _ops()
    segs, total = _layout(ADAM_LENGTHS)
    segs = [s for s in segs if s[1] % 4 == 0]
    g = torch.nan_to_num(_fill(segs, total, "gauss", 7), nan=0.0)
    lo = next(lo for lo, n, grp, c in segs if LIVE[c] > 0 and n > 4096)
    g[lo + 4097] = bad
    g = g.cuda()
    table, ctl, guard = ops.AdamTable(segs, NCLS, total, "cuda"), _ctl(), ops.GradGuard("cuda")
    ctl.step[:NCLS] = torch.tensor([0, 1, 7, 1, 3], dtype=torch.int32)
    ctl.set_lr(*LRS)
    views, whole = _adam_state(total, 8)
    before, ctl_before = [w.clone() for w in whole], ctl.buf.clone()
    ops.grad_sumsq(g, table, ctl, guard, max_norm=1.0)
    ops.adam_table_guarded(views[0], g, views[1], views[2], views[3], table, ctl, guard, *BETAS, EPS, WD)
    torch.cuda.synchronize()
    r = guard.read()
    assert r["skip"] == 1 and r["n_nonfinite"] == 1 and r["coef"] == 0.0 and r["n_skipped"] == 1 and r["n_steps"] == 1
    for name, a, b in zip(("p", "m", "v", "p_bf16"), whole, before):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), name
    assert torch.equal(ctl.buf.view(torch.int32), ctl_before.view(torch.int32)), "step counts moved on a skipped step"
    # the same gradients without the bad element: the very next call steps, margins untouched
    g[lo + 4097] = 0.0
    ops.grad_sumsq(g, table, ctl, guard, max_norm=1.0)
    ops.adam_table_guarded(views[0], g, views[1], views[2], views[3], table, ctl, guard, *BETAS, EPS, WD)
    torch.cuda.synchronize()
    r = guard.read()
    assert (r["skip"], r["n_skipped"], r["n_steps"]) == (0, 1, 2) and not torch.equal(whole[0], before[0])
    for a, b in zip(whole, before):
        assert torch.equal(a[:MARGIN], b[:MARGIN]) and torch.equal(a[-MARGIN:], b[-MARGIN:])
    assert ctl.step[:NCLS].cpu().tolist() == [1, 1, 8, 2, 4]


# ---- 3. the model ------------------------------------------------------------------------------------------------------------
L, B = 527, 3
CFG = AVSiamConfig(depth=2)
KW = dict(head_lr=100.0, mm_lr=100.0)


def _model(freeze):
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import apply_freeze_base
    m = CAVMAEFT_BASE(L, cfg=CFG, init_seed=5, init_mode="random").cuda()
    m.requires_grad_(True)
    apply_freeze_base(m, freeze)
    m._train_engine(B, 1).opts.deterministic = True          # with the "det" knob: one writer per gradient element, so twins agree byte for byte
    return m


def _labels(seed):
    hot = (torch.rand(B, L, generator=torch.Generator().manual_seed(seed)) < 0.03).float()
    hot[:, 0] = 1.0
    return (hot * 0.9 + 0.1 / L).cuda()


def _state(m):
    return {"p": m.arena.p.clone(), "pb": m.arena.pb.clone().view(torch.int16), "m": m._opt["m"].clone(), "v": m._opt["v"].clone()}


def _same(x, y, what):
    for k in x:
        assert torch.equal(x[k], y[k]), (what, k, int((x[k] != y[k]).sum()))


@pytest.fixture
def det():
    from avsiam_amd import _lib
    old = _lib.tuning_get("det")
    _lib.tuning_set("det", 1)
    yield
    _lib.tuning_set("det", old)


@pytest.mark.parametrize("freeze", [False, True])
@pytest.mark.parametrize("branch", ["mm", "a", "v"])
def test_guarded_step_of_the_model(det, monkeypatch, branch, freeze):
    ops = _ops()
    a, v = synth_inputs(CFG, B, 51)
    a, v, y = a.cuda(), v.unsqueeze(1).cuda(), _labels(11)
    step = lambda m, labels=y, **kw: m.train_step(a, v, labels, 1e-4, "mm_grad", branch=branch, **KW, **kw)
    # (a) max_norm = inf: the plain step, byte for byte; the norm is the host's
    plain, g = _model(freeze), _model(freeze)
    g.set_grad_guard()
    l_p, l_g = step(plain), step(g)
    torch.cuda.synchronize()
    assert float(l_p) == float(l_g)
    grads = [p.grad for p in plain.parameters() if p.grad is not None]
    assert grads and all(p.grad is None for p in g.parameters()), ".grad stays None after a guarded step"
    _same(_state(plain), _state(g), "guard(inf) vs plain")
    assert g.optimizer_steps() == plain.optimizer_steps() and g.optimizer_steps()
    host = np.float32(math.sqrt(math.fsum(float((t.double() ** 2).sum()) for t in grads)))
    st = g.guard_stats()
    ulp = float(np.spacing(host))
    record_margin(f"grad_guard.model_norm.{branch}.freeze{int(freeze)}", norm=st["norm"], host_norm=float(host), ulps=abs(st["norm"] - float(host)) / ulp)
    assert abs(st["norm"] - float(host)) <= ulp, (st["norm"], float(host))         # (pad elements of the arena are inside the table: they are zero)
    assert st["coef"] == 1.0 and st["n_nonfinite"] == 0 and not st["skipped"] and (st["n_skipped"], st["n_steps"]) == (0, 1)
    assert abs(math.sqrt(st["norm_base"] ** 2 + st["norm_head"] ** 2 + st["norm_mm"] ** 2) - st["norm"]) <= 1e-6 * st["norm"]
    assert (st["norm_base"] == 0.0) == freeze
    # (b) max_norm at half the norm: a plain table step with grad_scale = coef
    h, t = _model(freeze), _model(freeze)
    h.set_grad_guard(0.5 * st["norm"])
    step(h)
    coef = h.guard_stats()["coef"]
    assert 0.49 < coef < 0.51
    t.set_grad_guard()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "adam_table_guarded", lambda p, gr, m_, v_, pb, table, ctl, guard, b1, b2, eps, wd, grad_scale:
                   ops.adam_table(p, gr, m_, v_, pb, table, ctl, b1, b2, eps, wd, grad_scale=float(np.float32(grad_scale) * np.float32(coef))))
        step(t)
    torch.cuda.synchronize()
    _same(_state(h), _state(t), "clipped vs table step with grad_scale = coef")
    assert not torch.equal(h.arena.p, g.arena.p)
    # (c) one inf among the labels: nothing moves, and the next step is a normal one from the same state
    before, steps_before = _state(h), h.optimizer_steps()
    bad = y.clone()
    bad[1, 7] = INF
    step(h, bad)
    st = h.guard_stats()
    assert st["n_nonfinite"] > 0 and st["skipped"] and st["coef"] == 0.0 and (st["n_skipped"], st["n_steps"]) == (1, 2)
    _same(_state(h), before, "skipped step")
    assert h.optimizer_steps() == steps_before
    step(h, guard=INF)
    step(t)
    torch.cuda.synchronize()
    _same(_state(h), _state(t), "the step after a skipped one")
    st = h.guard_stats()
    assert not st["skipped"] and st["n_nonfinite"] == 0 and (st["n_skipped"], st["n_steps"]) == (1, 3)
    assert not torch.equal(h.arena.p, before["p"])
    # (d) the guard removed: the step counts are back on the host and adam_step goes on from them
    h.set_grad_guard(None)
    assert h._dps is None and h._opt["step"] == t.optimizer_steps() and set(h._opt["step"].values()) == {2}
    step(h)                                                  # the plain step: per-run avs_adam with the host's counts
    step(t)                                                  # still guarded (inf)
    torch.cuda.synchronize()
    _same(_state(h), _state(t), "plain step after the guard was removed")
    assert h.optimizer_steps() == t.optimizer_steps() and set(h.optimizer_steps().values()) == {3}
    assert any(p.grad is not None for p in h.parameters())


# ---- 4. the default path ------------------------------------------------------------------------------------------------------
# one plain fine-tuning step: tools/step_digest.py --ft --trace --batch 3 (tests/test_exact_gpu.py asserts the same)
PARENT_DIGEST = {"trace_calls": 303, "trace": "21a456a12665402bb61ad36021b881415531210137bfe83da2f626bd146a239a"}


def test_plain_step_is_the_parents():
    r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: got[k] for k in PARENT_DIGEST} == PARENT_DIGEST


# ---- 5. two ranks on one GPU -------------------------------------------------------------------------------------------------
SEQ = {0: ("mm", "a", "v"), 1: ("v", "v", "mm")}
WANT_STEPS = {"base_a": 3, "base_v": 3, "base_s": 3, "mm": 2, "mlp_head_mm": 2, "mlp_head": 3, "mlp_head_a": 1}


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
    from avsiam_amd.comm import HostStagedComm
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(L, cfg=CFG, init_seed=21, init_mode="random").cuda()
    m.requires_grad_(True)
    m.set_distributed(world, rank, HostStagedComm())
    a, v = synth_inputs(CFG, B, 200 + rank)
    return m, a.cuda(), v.unsqueeze(1).cuda(), _labels(300 + rank)


def _clip_section(rank, world, dist):
    m, a, v, y = _rank_model(rank, world)
    m.set_grad_guard(0.05)
    for k, branch in enumerate(SEQ[rank]):
        m.train_step(a, v, y, 1e-4, "mm_grad", branch=branch, **KW)
        torch.cuda.synchronize()
        st = m.guard_stats()
        assert 0 < st["coef"] < 1.0 and not st["skipped"] and st["n_steps"] == k + 1, (k, st)
        assert _same_on_both_ranks(dist, _sha(m.arena.p, m._opt["m"], m._opt["v"], m._guard.buf)), f"step {k}: the ranks differ"
    assert m.optimizer_steps() == WANT_STEPS, m.optimizer_steps()


def _skip_section(rank, world, dist):
    m, a, v, y = _rank_model(rank, world)
    m.set_grad_guard()
    m.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", **KW)
    torch.cuda.synchronize()
    before, steps = _sha(m.arena.p, m.arena.pb.view(torch.int16), m._opt["m"], m._opt["v"]), m.optimizer_steps()
    if rank == 1:
        y = y.clone()
        y[0, 3] = INF
    m.train_step(a, v, y, 1e-4, "mm_grad", branch=SEQ[rank][0], **KW)
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
        for name, fn in (("clip", _clip_section), ("skip", _skip_section)):
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
    port = 33500 + os.getpid() % 2000
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


@pytest.mark.parametrize("section", ["clip", "skip"])
def test_two_ranks_on_one_gpu(two_ranks, section):
    """clip: three guarded steps with the clipping active, rank 0 on mm, a, v and rank 1 on v, v, mm - weights, moments and the guard block
    byte-identical on both ranks after every step.  skip: an inf label on rank 1 alone - both ranks skip, nothing moves on either."""
    for rank in range(2):
        got = two_ranks[rank]
        assert "init" not in got, got["init"]
        assert section in got, f"rank {rank}: not reached ({got})"
        assert got[section] == "ok", f"rank {rank}: {got[section]}"
