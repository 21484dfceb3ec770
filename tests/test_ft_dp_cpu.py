"""Data-parallel fine-tuning, the parts that need no GPU: the rank-independent message schedule of comm.FixedScheduleReducer on the arena
layout of a real CAVMAEFT_BASE, the reducer between two real gloo processes, the argument errors of avs_adam_table, the launcher's torchrun
environment, and the optimizer-state file."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from avsiam_amd.comm import FixedScheduleReducer, fixed_schedule

L = 527
TRAINABLE_END = 102_229_440


# ---- the schedule ----------------------------------------------------------------------------------------------------------
class _Span:
    def __init__(self, a, b):
        self.a, self.b = a, b


class _FakeGrad:
    """stands in for the flat gradient buffer: a slice is just its bounds"""

    def __getitem__(self, s):
        return _Span(s.start, s.stop)


class _Handle:
    def wait(self):
        pass


class _RecordingComm:
    world, rank, active = 2, 0, True

    def __init__(self):
        self.sent = []

    def all_reduce_async(self, t):
        self.sent.append((t.a, t.b - t.a) if isinstance(t, _Span) else ("live", t.numel()))
        return _Handle()


@pytest.fixture(scope="module")
def model():
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(L)
    m.requires_grad_(True)
    return m


def _prefix_range(arena, prefix):
    from avsiam_amd.arena import ALIGN
    own = [n for n in arena.names if n.startswith(prefix) and arena.info[n].live]
    pad = lambda n: (int(np.prod(arena.info[n].shape)) + ALIGN - 1) // ALIGN * ALIGN
    return min(arena.offset[n] for n in own), max(arena.offset[n] + pad(n) for n in own)


def _ready_sequence(model, branch, freeze):
    """what ft_train.FtTrain.backward reports for a branch: the live head, the fusion blocks last to first (Stack.backward), then - unless the
    base is frozen - the encoder blocks last to first (the ranges engine.BlockParams keeps: grad_ranges)"""
    from avsiam_amd.engine import grad_ranges
    a = model.arena
    seq = [_prefix_range(a, {"mm": "mlp_head_mm.", "a": "mlp_head_a.", "v": "mlp_head."}[branch])]
    if branch == "mm":
        seq += grad_ranges(a, "mm_layer_2.") + grad_ranges(a, "mm_layer_1.")
    if not freeze:
        for i in reversed(range(model.cfg.depth)):
            seq += grad_ranges(a, f"vit_base.blocks.{i}.")
    return seq


def _classes(branch):
    from avsiam_amd.ft_train import OUT, OUT_A, OUT_V
    from avsiam_amd.models.cav_mae_ft import live_classes
    mode, bit = {"mm": ("mm_grad", OUT), "a": ("audioonly", OUT_A), "v": ("videoonly", OUT_V)}[branch]
    return live_classes(mode, bit)


def _record(model, branch, freeze, order="backward"):
    from avsiam_amd.traintest_ft_base import apply_freeze_base
    apply_freeze_base(model, freeze)
    try:
        cls = {c for c in _classes(branch) if not (freeze and c.startswith("base_"))}
        comm = _RecordingComm()
        red = FixedScheduleReducer(comm, _FakeGrad(), model.dp_schedule(), tail=torch.zeros(16))
        seq = _ready_sequence(model, branch, freeze)
        if order == "reversed":
            seq = seq[::-1]
        elif order == "shuffled":
            random.Random(5).shuffle(seq)
        red.begin(model.dp_dead_ranges(cls))
        early = None
        for r in seq:
            red.ready(*r)
            early = len(comm.sent) if early is None else early        # messages out after the first ready(): the head's
        before_finish = len(comm.sent)
        red.finish()
        assert red.log == [(a, a + n) if a != "live" else ("tail", n) for a, n in comm.sent]
        return comm.sent, early, before_finish
    finally:
        apply_freeze_base(model, False)


def test_schedule_tiles_the_trainable_range_in_backward_order(model):
    chunks = model.dp_schedule()
    lo, hi = model.arena.range[1]
    assert (lo, hi) == (0, TRAINABLE_END)
    assert sorted(chunks)[0][0] == lo and sorted(chunks)[-1][1] == hi
    assert all(x[1] == y[0] for x, y in zip(sorted(chunks), sorted(chunks)[1:])), "gap or overlap"
    a = model.arena
    fusion = _prefix_range(a, "mm_layer_1.")
    assert chunks[0][0] <= fusion[0] < fusion[1] <= chunks[0][1], "the fusion stack goes first"
    first_block = {i: next(k for k, c in enumerate(chunks) if c[0] <= a.offset[f"vit_base.blocks.{i}.attn.qkv.weight"] < c[1]) for i in range(12)}
    assert all(first_block[i] >= first_block[i + 1] for i in range(11)) and first_block[11] >= 1, "encoder blocks last to first"
    emb = next(k for k, c in enumerate(chunks) if c[0] <= a.offset["vit_base.patch_embed.proj.weight"] < c[1])
    assert emb >= first_block[0]
    big = [b - x for x, b in chunks if b - x >= 1 << 20]
    assert min(big) >= 15 << 20, "about 16 M elements per message"
    assert len(chunks) - len(big) <= 1, chunks


def test_every_branch_sends_the_same_messages(model):
    want = None
    for branch, freeze in (("mm", False), ("a", False), ("v", False), ("mm", True), ("v", True)):
        for order in ("backward", "reversed", "shuffled"):
            sent, early, before_finish = _record(model, branch, freeze, order)
            want = sent if want is None else want
            assert sent == want, (branch, freeze, order)
            assert sent[-1] == ("live", 16), "liveness travels as the last message"
            spans = sorted((a, a + n) for a, n in sent[:-1])
            assert spans[0][0] == 0 and spans[-1][1] == TRAINABLE_END and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
            if order == "backward":
                # overlap: the fusion chunk leaves as soon as the head is final (mm: once the fusion blocks are), not at finish()
                assert before_finish >= (len(sent) - 3 if not freeze else len(sent) - 2), (branch, freeze, before_finish)
                if branch != "mm":
                    assert early >= 1, "a rank on the a / v branch sends the fusion chunk right after its head"
    assert len(want) == len(model.dp_schedule()) + 1


def test_fixed_schedule_joins_touching_units_and_appends_holes():
    assert fixed_schedule([(50, 100), (30, 50), (10, 30)], 0, 100, min_elems=60) == [(30, 100), (0, 30)]
    assert fixed_schedule([(60, 100), (20, 40)], 0, 100, min_elems=10) == [(60, 100), (0, 60)]
    with pytest.raises(AssertionError):
        FixedScheduleReducer(_RecordingComm(), _FakeGrad(), [(0, 10), (5, 20)])
    with pytest.raises(AssertionError):
        FixedScheduleReducer(_RecordingComm(), _FakeGrad(), [(0, 10), (12, 20)])


# ---- two real processes ----------------------------------------------------------------------------------------------------
CHUNKS = [(60, 100), (40, 60), (25, 40), (0, 10), (10, 25)]
DEAD = {0: [(60, 100), (0, 10)], 1: [(25, 60)]}                       # what each rank's "backward" never writes


def _rank_grads(rank):
    g = torch.arange(100, dtype=torch.float32) * (rank + 1) + 0.5
    for a, b in DEAD[rank]:
        g[a:b] = 0.0
    return g


def _gloo_worker(rank, world, port, q):
    import datetime
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))     # a dead peer is an error, not a hang
        from avsiam_amd.comm import TorchDistComm
        g = _rank_grads(rank)
        live = torch.tensor([1.0, 0.0, 1.0] if rank == 0 else [0.0, 0.0, 1.0])
        red = FixedScheduleReducer(TorchDistComm(), g, CHUNKS, tail=live)
        red.begin(DEAD[rank])
        alive = [c for c in CHUNKS if not any(a <= c[0] and c[1] <= b for a, b in DEAD[rank])]
        for a, b in (alive[::-1] if rank else alive):                                 # the ranks complete their ranges in opposite orders
            red.ready(a, b)
        red.finish()
        q.put((rank, g.numpy().copy(), live.numpy().copy(), list(red.log)))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc(), None, None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_gloo_ranks_with_different_dead_sets_sum_the_same():
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29000 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r = q.get(timeout=90)
            res[r[0]] = r[1:]
    except queue.Empty:
        pass
    finally:
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.terminate()
    assert len(res) == 2, "a worker did not answer before the deadline"
    for rank, (g, live, log) in res.items():
        assert not isinstance(g, str), f"rank {rank}: {g}"
    want = (_rank_grads(0) + _rank_grads(1)).numpy()
    for rank in range(2):
        assert np.array_equal(res[rank][0], want), rank
        assert np.array_equal(res[rank][1], np.array([1.0, 0.0, 2.0], dtype=np.float32))
        assert res[rank][2] == CHUNKS + [("tail", 3)]


# ---- the C entry point -------------------------------------------------------------------------------------------------------
def test_adam_table_argument_errors_return_minus_two():
    from avsiam_amd import _lib
    lib = _lib.load()
    one = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    args = lambda **kw: [kw.get(k, one) for k in ("p", "g", "m", "v", "pb", "segs")] + [kw.get("n", 1), kw.get("ctl", one), 0.95, 0.999, 1e-8, 5e-7,
                                                                                         1.0, None]
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(segs=None), dict(ctl=None), dict(n=0), dict(n=-3), dict(n=4097)):
        assert lib.avs_adam_table(*args(**bad)) == -2, bad
        assert b"adam_table" in lib.avs_last_error()
    sized = lambda chunks: [one] * 6 + [1, chunks, one, 0.95, 0.999, 1e-8, 5e-7, 1.0, None]
    assert lib.avs_adam_table_sized(*sized(0)) == -2 and lib.avs_adam_table_sized(*sized(-1)) == -2
    assert lib.avs_adam_table_set_lr(None, 1.0, 1.0, 1.0, None) == -2
    grid, chunk, segs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.avs_adam_table_geometry(ctypes.byref(grid), ctypes.byref(chunk), ctypes.byref(segs)) == 0
    assert 1 <= grid.value <= 4096 and chunk.value % 1024 == 0 and segs.value == 4096
    assert lib.avs_adam_table_geometry(None, None, None) == 0
    assert lib.avs_abi_version() == 2


# ---- launcher ----------------------------------------------------------------------------------------------------------------
def test_launcher_honours_the_torchrun_environment(monkeypatch):
    """RANK / WORLD_SIZE / LOCAL_RANK form the process group (gloo here: cuda is reported absent, so the test needs no GPU and takes none),
    `random` is seeded 87 + local rank, and the run gets rank and world size; the group is gone afterwards."""
    import avsiam_amd.run_cavmae_ft_base as launcher
    import torch.distributed as dist
    seen = {}

    def fake_run(args):
        seen.update(rank=args.rank, world=args.world_size, gpu=args.gpu, distributed=args.distributed, group=dist.is_initialized(),
                    draw=random.uniform(0, 1))
        return "ran"

    monkeypatch.setattr(launcher, "_run", fake_run)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", str(31000 + os.getpid() % 2000))):
        monkeypatch.setenv(k, v)
    assert launcher.main(["--ftmode", "mm_grad", "--world_size", "8"]) == "ran"      # the environment decides, not the flag
    assert seen == dict(rank=0, world=1, gpu=0, distributed=True, group=True, draw=random.Random(87).uniform(0, 1))
    assert not dist.is_initialized()
    print("still printing")                                                          # (setup_for_distributed's print was restored)


# ---- optimizer state -----------------------------------------------------------------------------------------------------------
def test_optimizer_state_round_trips_through_a_file(tmp_path):
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.models.cav_mae_ft import CLASSES
    cfg = AVSiamConfig(depth=2)
    m = CAVMAEFT_BASE(7, cfg=cfg)
    assert m.optimizer_state() is None and m.optimizer_steps() == {}
    n = m.arena.range[1][1] - m.arena.range[1][0]
    g = torch.Generator().manual_seed(3)
    m._opt = {"m": torch.randn(n, generator=g), "v": torch.rand(n, generator=g), "step": {"base_s": 3, "mm": 2, "mlp_head_mm": 2, "mlp_head": 1}}
    m._rates = (1e-4, 1e-2, 5e-3)
    path = tmp_path / "best_optim_state.pth"
    torch.save(m.optimizer_state(), path)
    sd = torch.load(path, map_location="cpu")
    assert set(sd) == {"m", "v", "step", "lr"} and all(type(t) is torch.Tensor for t in sd.values())
    assert sd["step"].tolist() == [0, 0, 3, 2, 1, 0, 2, 0] and len(CLASSES) == 8
    m2 = CAVMAEFT_BASE(7, cfg=cfg)
    m2.load_optimizer_state(sd)
    assert torch.equal(m2._opt["m"], m._opt["m"]) and torch.equal(m2._opt["v"], m._opt["v"])
    assert m2.optimizer_steps() == m._opt["step"] and m2._rates == pytest.approx(m._rates)
    with pytest.raises(ValueError):
        CAVMAEFT_BASE(7, cfg=AVSiamConfig(depth=3)).load_optimizer_state(sd)


def test_step_counts_survive_dropping_the_data_parallel_state():
    """the counts live in ctl.step while data parallel; a second set_distributed (or a return to adam_step) must continue from them"""
    from avsiam_amd import ops
    from avsiam_amd.comm import LocalComm
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.models.cav_mae_ft import CLASSES
    m = CAVMAEFT_BASE(7, cfg=AVSiamConfig(depth=2))
    m._opt = {"m": torch.zeros(4), "v": torch.zeros(4), "step": {"mm": 1}}            # stale: what the host knew before the data-parallel steps
    ctl = ops.AdamCtl("cpu")
    ctl.step[CLASSES.index("mm")] = 5
    ctl.step[CLASSES.index("base_s")] = 7
    m._dps = {"ctl": ctl}
    m.set_distributed(1, 0, LocalComm())
    assert m._dps is None and m._opt["step"] == {"mm": 5, "base_s": 7} and m.optimizer_steps() == {"mm": 5, "base_s": 7}


# ---- the loop ----------------------------------------------------------------------------------------------------------------
class _TwoRankGather:
    """all_gather of a 2-rank world seen from one rank: the peer's shard is this rank's plus 100"""
    world, rank, active = 2, 0, True

    def all_gather(self, out, inp):
        out.view(2, -1)[0].copy_(inp)
        out.view(2, -1)[1].copy_(inp + 100)


def test_distributed_concat_is_rank_major_and_truncates():
    from avsiam_amd.traintest_ft_base import distributed_concat
    t = torch.arange(12, dtype=torch.float32).view(3, 2, 2)
    full = distributed_concat(_TwoRankGather(), t)
    assert full.shape == (6, 2, 2) and torch.equal(full[:3], t) and torch.equal(full[3:], t + 100)
    cut = distributed_concat(_TwoRankGather(), t, 5)                               # the sampler padded the last shard by one clip
    assert cut.shape == (5, 2, 2) and torch.equal(cut, full[:5])
    assert torch.equal(distributed_concat(_TwoRankGather(), t.transpose(1, 2), None)[:3], t.transpose(1, 2))


def test_restore_takes_only_a_fine_tuning_state_beside_best_audio_model(tmp_path, capsys):
    """The pre-training loop writes a best_optim_state.pth too, in torch.optim.Adam's format, beside ITS best_audio_model.pth: a fine-tuning
    run started from that directory must not choke on it."""
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.run_cavmae_ft_base import restore_optimizer_state
    cfg = AVSiamConfig(depth=2)
    m = CAVMAEFT_BASE(7, cfg=cfg)
    n = m.arena.range[1][1] - m.arena.range[1][0]
    ck = tmp_path / "best_audio_model.pth"
    opt = tmp_path / "best_optim_state.pth"
    assert restore_optimizer_state(m, str(ck)) is False and m._opt is None                       # no file beside it
    torch.save({"state": {0: {"step": torch.tensor(3.0), "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(5)}},
                "param_groups": [{"lr": 1e-4, "params": [0]}]}, opt)
    assert restore_optimizer_state(m, str(ck)) is False and m._opt is None
    assert "weights-only warm start" in capsys.readouterr().out
    good = {"m": torch.ones(n), "v": torch.full((n,), 2.0), "step": torch.tensor([0, 0, 3, 2, 1, 0, 2, 0]), "lr": torch.tensor([1e-4, 1e-2, 1e-2])}
    torch.save(dict(good, m=torch.ones(n - 64)), opt)                                            # another model's sizes
    assert restore_optimizer_state(m, str(ck)) is False and m._opt is None
    torch.save(good, opt)
    assert restore_optimizer_state(m, str(tmp_path / "audio_model.3.pth")) is False and m._opt is None     # only for best_audio_model.pth
    assert restore_optimizer_state(m, str(ck)) is True
    assert m.optimizer_steps() == {"base_s": 3, "mm": 2, "mlp_head": 1, "mlp_head_mm": 2} and float(m._opt["v"][0]) == 2.0
