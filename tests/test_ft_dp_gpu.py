"""Data-parallel fine-tuning on a real MI355X.

1. ``avs_adam_table`` (one launch over a segment table, step counts and liveness in device memory) against per-segment ``avs_adam`` launches,
   byte for byte, on a synthetic arena.
2. One rank with the collectives forced on: the data-parallel ``train_step`` against the plain fused step of a twin model.
3. Two ranks sharing the one GPU (spawn, gloo, comm.HostStagedComm as tests/test_dp_gpu.py: RCCL refuses two ranks on one device):
   three real steps with a different branch sequence per rank.
At most 2 worker processes; the parent joins them with a deadline, terminates them on expiry, fails and starts nothing further."""
import hashlib
import os

import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_inputs
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu

FUSED_COS, FUSED_NORM = 0.9999, 1e-3      # the bounds of tests/test_ft_train_gpu.py::test_fused_step_matches_autograd_and_torch_adam
BETAS, EPS, WD = (0.95, 0.999), 1e-8, 5e-7
SENT_P, SENT_M, SENT_V = 3.25, -0.5, 0.75


def _ops():
    from avsiam_amd import ops
    return ops


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
def _arena(total, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(total, generator=g).cuda()
    gr = (torch.randn(total, generator=g) * 0.1).cuda()
    m = (torch.randn(total, generator=g) * 0.01).cuda()
    v = (torch.rand(total, generator=g) * 1e-3).cuda()
    pb = torch.full((total,), 9.0, dtype=torch.bfloat16, device="cuda")
    return p, gr, m, v, pb


def _layout(lengths, gap_after, ngroup=3, ncls=5):
    """segments (lo, n, group, cls) laid end to end with 64 unowned elements behind the segments whose index is in gap_after; groups and
    classes interleave along the arena -> (segs, total elements)"""
    segs, at = [], 64                                     # (a gap in front of the first segment too)
    for i, n in enumerate(lengths):
        segs.append((at, n, i % ngroup, (i * 2 + i // ncls) % ncls))
        at += n + (64 if i in gap_after else 0)
    return segs, at + 64


def _run_and_check(segs, total, steps, live, lrs, with_shadow, seed, calls=2, scale=0.5, sized=True):
    """`calls` consecutive avs_adam_table launches against per-segment avs_adam on copies; everything nobody owns, and every segment of a
    class that is not live, keeps its sentinel-marked bytes"""
    ops = _ops()
    ncls = len(steps)
    p, g, m, v, pb = _arena(total, seed)
    owned = torch.zeros(total, dtype=torch.bool, device="cuda")
    for lo, n, grp, c in segs:
        if live[c] > 0:
            owned[lo:lo + n] = True
    p[~owned], m[~owned], v[~owned] = SENT_P, SENT_M, SENT_V
    ctl = ops.AdamCtl("cuda")
    ctl.step[:ncls] = torch.tensor(steps, dtype=torch.int32)
    ctl.live[:ncls] = torch.tensor(live, dtype=torch.float32)
    ctl.set_lr(*lrs)
    table = ops.AdamTable(segs, ncls, total, "cuda")
    ref = [t.clone() for t in (p, m, v, pb)]
    cur = list(steps)
    for call in range(calls):
        ops.adam_table(p, g, m, v, pb if with_shadow else None, table, ctl, *BETAS, EPS, WD, grad_scale=scale, sized=sized)
        for lo, n, grp, c in segs:
            if live[c] > 0:
                s = slice(lo, lo + n)
                ops.adam(ref[0][s], g[s], ref[1][s], ref[2][s], ref[3][s] if with_shadow else None, n, lrs[grp], cur[c] + 1, *BETAS, EPS, WD, scale)
        cur = [k + (1 if live[c] > 0 else 0) for c, k in enumerate(cur)]
        torch.cuda.synchronize()
        for name, got, want in zip(("p", "m", "v", "p_bf16"), (p, m, v, pb), ref):
            assert torch.equal(got, want), (name, call, int((got != want).sum()))
        assert ctl.step[:ncls].cpu().tolist() == cur, (call, ctl.step.cpu().tolist(), cur)
        assert ctl.step[ncls:].abs().sum().item() == 0
    assert torch.all(p[~owned] == SENT_P) and torch.all(m[~owned] == SENT_M) and torch.all(v[~owned] == SENT_V)
    assert torch.all(pb[~owned] == 9.0)
    if not with_shadow:
        assert torch.all(pb == 9.0)
    assert torch.equal(ctl.live[:ncls].cpu(), torch.tensor(live, dtype=torch.float32)) and torch.allclose(ctl.lr.cpu(), torch.tensor(lrs))


LRS = (1e-3, 5e-2, 2e-4)


@pytest.mark.parametrize("with_shadow", [True, False])
def test_adam_table_matches_per_segment_adam_byte_for_byte(with_shadow):
    lengths = [64, 128, 4032, 4096, 4160, 70016, 128, 4096, 64, 4160, 4032, 70016]
    segs, total = _layout(lengths, gap_after={0, 3, 4, 7, 10})
    steps, live = [0, 1, 7, 1, 0], [1.0, 0.0, 2.0, 1.0, 0.0]          # (live = 2: what a class reached by two ranks sums to)
    assert {c for *_, c in segs} == set(range(5)) and {g for _, _, g, _ in segs} == {0, 1, 2}
    _run_and_check(segs, total, steps, live, LRS, with_shadow, seed=1)


def test_adam_table_one_segment_and_many_small_ones():
    _run_and_check([(64, 4160, 1, 0)], 4352, [3], [1.0], LRS, True, seed=2)                 # two chunks: a grid of two workgroups
    _run_and_check([(64, 4160, 1, 0)], 4352, [3], [1.0], LRS, True, seed=2, sized=False)    # avs_adam_table itself: the full grid, the same bytes
    segs, total = _layout([64] * 300, gap_after=set(range(0, 300, 7)))
    _run_and_check(segs, total, [0, 1, 7, 2, 5], [1.0, 1.0, 0.0, 1.0, 0.0], LRS, True, seed=3)


def test_adam_table_second_trip_through_the_chunk_loop():
    """One segment longer than grid x chunk elements of the kernel's own launch geometry (avs_adam_table_geometry): the first workgroups take
    a second chunk, the last chunk is a partial one."""
    grid, chunk, _ = _ops().adam_table_geometry()
    n = grid * chunk + 3 * chunk + 192
    _run_and_check([(64, n, 2, 1), (64 + n + 64, 128, 0, 0)], n + 384, [4, 0], [0.0, 1.0], LRS, True, seed=4, calls=1)


def test_adam_table_refuses_a_bad_table():
    ops = _ops()
    from avsiam_amd._lib import AvsiamHipError
    for segs, ncls in (([(0, 64, 0, 0), (32, 64, 0, 0)], 2), ([(0, 66, 0, 0)], 1), ([(2, 64, 0, 0)], 1), ([(0, 64, 3, 0)], 1), ([(0, 64, 0, 1)], 1),
                       ([(0, 64, 0, 0)], 17), ([], 1), ([(960, 128, 0, 0)], 1)):
        with pytest.raises(AvsiamHipError):
            ops.AdamTable(segs, ncls, 1024, "cuda")


# ---- 2. one rank, collectives forced on --------------------------------------------------------------------------------------
L, B = 527, 2


@pytest.fixture(scope="module")
def forced_comm():
    """a one-rank RCCL communicator that issues its collectives anyway (what --force-dp selects): one for the module"""
    from avsiam_amd.comm import RcclComm
    comm = RcclComm(rank=0, world=1, always=True)
    yield comm
    comm.close()


def _model(seed, mode="random"):
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(L, init_seed=seed, init_mode=mode).cuda()
    m.requires_grad_(True)
    return m


def _labels(n, seed):
    g = torch.Generator().manual_seed(seed)
    hot = (torch.rand(n, L, generator=g) < 0.03).float()
    hot[:, 0] = 1.0
    return hot * 0.9 + 0.1 / L


def _live_from_ctl(m):
    from avsiam_amd.models.cav_mae_ft import CLASSES
    live = m._dps["ctl"].live.cpu().tolist()
    assert all(x == 0 for x in live[len(CLASSES):])
    return {c for c, x in zip(CLASSES, live) if x > 0}


@pytest.mark.parametrize("branch", ["mm", "a", "v"])
def test_one_rank_with_collectives_matches_the_plain_fused_step(forced_comm, branch):
    from avsiam_amd.ft_train import OUT, OUT_A, OUT_V
    from avsiam_amd.models.cav_mae_ft import live_classes
    cfg = AVSiamConfig()
    a, v = synth_inputs(cfg, B, 51)
    a, v, y = a.cuda(), v.unsqueeze(1).cuda(), _labels(B, 11).cuda()
    dp, plain = _model(5), _model(5)
    dp.set_distributed(1, 0, forced_comm)
    try:
        assert dp._dp
        l_dp = dp.train_step(a, v, y, 0.0, "mm_grad", branch=branch)
        l_pl = plain.train_step(a, v, y, 0.0, "mm_grad", branch=branch)
        torch.cuda.synchronize()
        assert abs(float(l_dp) - float(l_pl)) <= 1e-4 * abs(float(l_pl)), (float(l_dp), float(l_pl))
        assert all(p.grad is None for p in dp.parameters()), ".grad stays None after a data-parallel fused step"
        want = {n for n, p in plain._params.items() if p.grad is not None}
        mode, bit = {"mm": ("mm_grad", OUT), "a": ("audioonly", OUT_A), "v": ("videoonly", OUT_V)}[branch]
        assert _live_from_ctl(dp) == live_classes(mode, bit)
        worst = 1.0
        for n in dp._params:
            if not dp.arena.info[n].live:
                continue
            g = dp.arena.gview(n).double().reshape(-1)
            if n not in want:
                assert float(g.abs().max()) == 0.0, f"{n}: outside the branch, yet a gradient"
                continue
            r = plain._params[n].grad.double().reshape(-1)
            if float(r.norm()) == 0:
                continue
            cos = float(g @ r / (g.norm() * r.norm()))
            worst = min(worst, cos)
            assert cos >= FUSED_COS and abs(float(g.norm() / r.norm()) - 1) <= FUSED_NORM, (branch, n, cos)
        record_margin(f"ft_dp.one_rank_vs_plain.{branch}", worst_cos=worst)
        assert len(dp._dps["reducer"].log) == len(dp.dp_schedule()) + 1 and dp._dps["reducer"].log[-1] == ("tail", 16)
        # a real step: exactly the tensors the plain step changes
        before = {n: p.detach().clone() for n, p in dp._params.items()}
        before_pl = {n: p.detach().clone() for n, p in plain._params.items()}
        dp.train_step(a, v, y, 1e-4, "mm_grad", branch=branch, head_lr=100.0, mm_lr=100.0)
        plain.train_step(a, v, y, 1e-4, "mm_grad", branch=branch, head_lr=100.0, mm_lr=100.0)
        torch.cuda.synchronize()
        changed = {n for n, p in dp._params.items() if not torch.equal(p.detach(), before[n])}
        changed_pl = {n for n, p in plain._params.items() if not torch.equal(p.detach(), before_pl[n])}
        assert changed == changed_pl and changed, sorted(changed ^ changed_pl)[:6]
        assert dp.optimizer_steps() == plain.optimizer_steps() == {c: 2 for c in live_classes(mode, bit)}
        with pytest.raises(RuntimeError, match="autograd path"):
            dp(a, v, "mm_grad")
    finally:
        from avsiam_amd import _lib
        _lib.tuning_set("cu_reserve", 0)                 # (process-wide knob set_distributed raised: back to the default for later tests)


# ---- 3. two ranks on one GPU -------------------------------------------------------------------------------------------------
GOLD_L2, GOLD_SAMP, GOLD_SUM, LOSS_TOL = 0.01, 0.3, 1.2, 2e-3       # the bounds of tests/test_ft_train_gpu.py::test_backward_matches_reference_golden
W2_CASES = ["ftt_w2_av", "ftt_w2_mma", "ftt_w2_vv_freeze"]
SEQ = {0: ("mm", "a", "v"), 1: ("v", "v", "mm")}
WANT_STEPS = {"base_a": 3, "base_v": 3, "base_s": 3, "mm": 2, "mlp_head_mm": 2, "mlp_head": 3, "mlp_head_a": 1}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _same_on_both_ranks(dist, value):
    box = [None, None]
    dist.all_gather_object(box, value)
    return box[0] == box[1]


def _golden_section(rank, world, dist):
    from avsiam_amd.models.cav_mae_ft import grad_class, param_group
    from tests.helpers import HostStagedComm, golden_grads, gpu_grads_vs_golden, load_golden
    from tests.test_ft_train_oracle_golden import ftt_inputs
    cfg = AVSiamConfig()
    m = None
    for case in W2_CASES:
        d = load_golden(f"{case}_r{rank}")
        if m is None:
            from avsiam_amd.models import CAVMAEFT_BASE
            m = CAVMAEFT_BASE(int(d["label_dim"]), init_seed=int(d["weight_seed"]), init_mode="random").cuda()
            m.set_distributed(world, rank, HostStagedComm())
        freeze = bool(d["freeze_base"])
        for n, p in m.named_parameters():
            p.requires_grad_(not (freeze and param_group(n) == "base"))
        a, v = ftt_inputs(d, cfg)
        branch = {"out": "mm", "out_a": "a", "out_v": "v"}[str(d["target"])]
        loss = m.train_step(a.cuda(), v.cuda(), torch.from_numpy(d["labels"]).cuda(), 0.0, "mm_grad", branch=branch)
        torch.cuda.synchronize()
        ref = float(d["loss"])
        err = abs(float(loss) - ref) / max(1.0, abs(ref))
        assert err <= LOSS_TOL, (case, float(loss), ref)
        live = _live_from_ctl(m)
        names, none, *_ = golden_grads(d)
        have = {n for n, p in m.named_parameters() if p.requires_grad and m.arena.info[n].live and grad_class(n) in live}
        assert have == set(names), (case, sorted(have ^ set(names))[:6])
        assert not any(grad_class(n) in live and m._params[n].requires_grad for n in none if m.arena.info[n].live), case
        mean = m.arena.g / world
        view = lambda n: m.arena._v(mean, n) if (n in have) else None
        for turn in range(world):                            # (one rank at a time: the margins go to one file)
            if turn == rank:
                gpu_grads_vs_golden(d, view, f"ft_dp.golden_{case}_r{rank}", l2_rel=GOLD_L2, samp_rel=GOLD_SAMP, sum_rel=GOLD_SUM)
                record_margin(f"ft_dp.golden_{case}_r{rank}", loss_err=err)
            dist.barrier()
        dead = [n for n in none if m.arena.info[n].live]
        assert all(float(m.arena.gview(n).abs().max()) == 0.0 for n in dead), case
        assert _same_on_both_ranks(dist, _sha(m.arena.g)), f"{case}: the gradient arenas differ between the ranks"


def _steps_section(rank, world, dist):
    import dataclasses
    from avsiam_amd.models import CAVMAEFT_BASE
    from tests.helpers import HostStagedComm
    cfg = AVSiamConfig()
    m = CAVMAEFT_BASE(L, init_seed=21, init_mode="random").cuda()
    m.requires_grad_(True)
    m.set_distributed(world, rank, HostStagedComm())
    a, v = synth_inputs(cfg, B, 200 + rank)
    a, v, y = a.cuda(), v.unsqueeze(1).cuda(), _labels(B, 300 + rank).cuda()
    for k, branch in enumerate(SEQ[rank]):
        m.train_step(a, v, y, 1e-4, "mm_grad", branch=branch, head_lr=100.0, mm_lr=100.0)
        torch.cuda.synchronize()
        assert _same_on_both_ranks(dist, _sha(m.arena.p)), f"step {k}: the weights differ between the ranks"
    assert m.optimizer_steps() == WANT_STEPS, m.optimizer_steps()
    if rank == 0:
        a2, v2 = synth_inputs(dataclasses.replace(cfg, frames=10), B, 400)     # (mm_grad with is_eval=True takes 10-frame clips)
        with torch.no_grad():
            got = m(a2.cuda(), v2.cuda(), "mm_grad", is_eval=True)
            fresh = CAVMAEFT_BASE(L).cuda()
            fresh.load_state_dict(m.state_dict())
            want = fresh(a2.cuda(), v2.cuda(), "mm_grad", is_eval=True)
        assert torch.equal(got, want), "a stale head copy or bf16 shadow after the data-parallel steps"


def _worker(rank, world, port, q):
    import datetime
    import traceback
    import torch.distributed as dist
    res = {}
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        for name, fn in (("golden", _golden_section), ("steps", _steps_section)):
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
    port = 31500 + os.getpid() % 2000                      # (not a fixed one: a stale listener would cost the whole deadline)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            rank, r = q.get(timeout=420)
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


@pytest.mark.parametrize("section", ["golden", "steps"])
def test_two_ranks_on_one_gpu(two_ranks, section):
    """golden: train_step(lr = 0) per case of tools/gen_golden_ft_dp.py with the golden's per-rank branch and inputs - the local loss, the
    averaged gradients (arena.g / world) and the set of live tensors against the unmodified reference under DDP(find_unused_parameters=True),
    the gradient arena byte-identical on both ranks.  steps: three real steps, rank 0 on mm, a, v and rank 1 on v, v, mm - weights
    byte-identical after every step, the step counts the union of branches implies, and inference afterwards equal to a fresh model's."""
    for rank in range(2):
        got = two_ranks[rank]
        assert "init" not in got, got["init"]
        assert section in got, f"rank {rank}: not reached ({got})"
        assert got[section] == "ok", f"rank {rank}: {got[section]}"
