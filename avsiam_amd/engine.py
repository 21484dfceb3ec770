"""Host-side schedule of the AVSiam pre-training hot path on the HIP kernels.

MI355X-first restructuring of ``CAVMAE_BASE.forward`` (/root/reference/src/models/cav_mae_base.py:685-741):

* every sequence of a pass is PACKED into one [rows, D] token matrix.  The contrastive pass of the reference
  issues 12 layers x (<=5 audio groups + <=5 video groups) Block calls on ragged groups (:554-558); all ops
  but attention are token-wise and the weights are shared (Siamese), so here it is 12 layers of
  {LN(row-selected affine) -> one QKV GEMM -> varlen attention -> proj GEMM(+residual) -> LN -> fc1(+GELU) -> fc2(+residual)}
  over all rows at once;
* only KEPT tokens are embedded (the reference embeds all and drops 75 %, :448-455,476-477);
* the residual stream stays fp32 (as under the reference's autocast, where pos_embed/LayerNorm keep it fp32),
  GEMM/attention operands are bf16 with fp32 accumulation;
* backward is a hand-written schedule (no autograd graph): dgrad GEMMs read pre-transposed bf16 weight copies,
  wgrad GEMMs contract over the token rows with transposing LDS reads and accumulate straight into the flat
  gradient arena.

The mask plan (which tokens each sample keeps) is an explicit input - see maskplan.py.
"""
import collections
import math
import os

from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .arena import ParamArena
from .config import AVSiamConfig, EngineOptions
from .maskplan import ContrastivePlan, MaePlan, draw_structured, group_sizes, group_ratio, len_keep

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
LN_EPS_BLOCK, LN_EPS_FINAL = 1e-5, 1e-6       # nn.LayerNorm default in Block; timm ViT final norm


def recompute_blocks(nblocks, setting):
    """number of leading blocks of a Stack of `nblocks` that are recomputed under EngineOptions.recompute ("0" | "1" | a fraction in (0, 1))"""
    f = float(setting)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"recompute must be 0, 1 or a fraction between them, not {f}")
    return min(nblocks, int(math.ceil(f * nblocks - 1e-9)))


def _z(shape, dtype, dev):
    return torch.zeros(shape, dtype=dtype, device=dev)


class BufferPool:
    """One activation pool for ALL passes of a model (opt-in: CAVMAE_BASE(share_pass_buffers=True) / AVSIAM_SHARE_PASS_BUFFERS=1).
    The training step runs its two passes one after the other (traintest_cavmae_base.py:131-152: pass 1 forward / backward / Adam, then
    pass 2), so pass 1's activations are dead when pass 2 starts - yet each pass's stacks own their buffers for the life of the model,
    and at ViT-H/14, batch 64 x 10 frames, it is the SUM of the two that does not fit the card without recomputing blocks.  With a pool
    every pass bump-allocates the buffers of its stacks from offset 0 of the same chunks of memory: the card holds the LARGER pass.
    Consequences, all handled in Stack: a buffer is zero at allocation only - another pass has written over it since - so the pad rows the
    GEMMs read beyond the token rows are re-zeroed (one launch, ops.ZeroTable) at the start of every Stack.forward; nothing in a pooled
    buffer survives into the other pass (results leave a pass as clones); and a backward over BOTH passes of one forward (the combined
    loss with gradients) is refused by the model."""

    CHUNK = 64 << 20          # smallest chunk; a chunk is 8 x the request that opens it (bump allocation: <= 1/8 lost at its end - a chunk
                              # sized request + 1 GiB was tried in round 5 and wasted 45 % at ViT-H, whose requests are all ~1.2 GiB: each
                              # chunk then holds ONE); when the card cannot give 8 x any more, 2 x and then the request itself are tried
                              # before the allocation fails (a late request must not fail while it would fit)

    def __init__(self, dev):
        self.dev = dev
        self.chunks = []
        self.owner = None                      # the pass whose forward ran last (its activations are what the memory holds)
        self.rewind()

    def rewind(self):
        """the next pass starts over at the first byte of every chunk"""
        self.offs = [0] * len(self.chunks)

    def alloc(self, shape, dtype):
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = (n * torch.empty((), dtype=dtype).element_size() + 255) & ~255
        for i, c in enumerate(self.chunks):                # first fit: a later, smaller request may still use the room a larger one left
            if self.offs[i] + nbytes <= c.numel():
                break
        else:
            chunk = None
            for mult in (8, 2, 1):
                try:
                    chunk = torch.zeros((max(self.CHUNK if mult == 8 else 0, mult * nbytes),), dtype=U8, device=self.dev)
                    break
                except torch.OutOfMemoryError:
                    if mult == 1:
                        raise
            self.chunks.append(chunk)
            self.offs.append(0)
            i, c = len(self.chunks) - 1, self.chunks[-1]
        t = c[self.offs[i]:self.offs[i] + nbytes].view(dtype)[:n].view(shape)
        self.offs[i] += nbytes
        return t

    def nbytes(self):
        return sum(c.numel() for c in self.chunks)

    def used(self):
        """bytes handed out since the last rewind (the live requests of the pass that owns the pool now)"""
        return sum(self.offs)

    def release(self):
        """give the memory back (every engine built on this pool must be dropped by the caller: CAVMAE_BASE.release_buffers)"""
        self.chunks, self.offs, self.owner = [], [], None


class Linear:
    """Arena views of one nn.Linear: bf16 weight [N,K], transposed copy [K,N], fp32 bias, gradient views."""

    def __init__(self, arena: ParamArena, wname, bname, need_t=True):
        self.w = arena.wb(wname)
        self.wt = arena.wtb(wname) if need_t and wname in arena.t_offset else None
        self.b = arena.w(bname)
        grads = arena.g is not None
        self.gw = arena.gw(wname) if grads else None
        self.gb = arena.gw(bname) if grads else None


class Norm:
    def __init__(self, arena: ParamArena, prefix):
        self.g, self.b = arena.w(prefix + ".weight"), arena.w(prefix + ".bias")
        grads = arena.g is not None
        self.dg, self.db = (arena.gw(prefix + ".weight"), arena.gw(prefix + ".bias")) if grads else (None, None)


def grad_ranges(arena, prefix, min_elems=1 << 20):
    """Contiguous ranges of the flat gradient arena covered by the live parameters named `prefix`*, smallest first.
    Only ranges of at least `min_elems` elements are returned: the reducer sends what is left (LayerNorm vectors sitting in
    another liveness class of the arena, embeddings, heads) in its final message instead of one tiny message each."""
    spans = sorted((arena.offset[n], arena.offset[n] + (math.prod(s.shape) + 63) // 64 * 64) for n, s in arena.info.items()
                   if n.startswith(prefix) and s.live)
    out = []
    for a, b in spans:
        if out and a == out[-1][1]:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [(a, b) for a, b in out if b - a >= min_elems]


class BlockParams:
    """One transformer Block (cav_mae_base.py:102-211); `sfx0`/`sfx1` name the LayerNorm sets for row_mod 0/1
    ('' plain, '_a', '_v')."""

    def __init__(self, arena, prefix, sfx0, sfx1=None):
        self.arena, self.prefix = arena, prefix
        self.ranges = grad_ranges(arena, prefix + ".")
        self.n1 = [Norm(arena, f"{prefix}.norm1{sfx0}")] + ([Norm(arena, f"{prefix}.norm1{sfx1}")] if sfx1 is not None else [])
        self.n2 = [Norm(arena, f"{prefix}.norm2{sfx0}")] + ([Norm(arena, f"{prefix}.norm2{sfx1}")] if sfx1 is not None else [])
        self.qkv = Linear(arena, f"{prefix}.attn.qkv.weight", f"{prefix}.attn.qkv.bias")
        self.proj = Linear(arena, f"{prefix}.attn.proj.weight", f"{prefix}.attn.proj.bias")
        self.fc1 = Linear(arena, f"{prefix}.mlp.fc1.weight", f"{prefix}.mlp.fc1.bias")
        self.fc2 = Linear(arena, f"{prefix}.mlp.fc2.weight", f"{prefix}.mlp.fc2.bias")


def _ln_fwd(x, norms, y, mean, rstd, rows, eps, row_mod=None, out_map=None, y8=None, q8_dev=None):
    n0 = norms[0]
    n1 = norms[1] if len(norms) > 1 else None
    ops.layernorm_fwd(x, n0.g, n0.b, y, mean, rstd, rows, eps, n1.g if n1 else None, n1.b if n1 else None,
                      row_mod if n1 else None, out_map, y8=y8, q8_dev=q8_dev)


class _LnBatch:
    """The LayerNorm backwards of one stack backward with their parameter-gradient reduces deferred to ONE launch (ops.LnReduceBatch): the first
    backward allocates a slab workspace per call and collects the table, later ones walk the same calls in the same order - after check()."""

    def __init__(self, D, dev):
        self.batch, self.dev, self.k, self.slabs = ops.LnReduceBatch(D), dev, 0, {}

    def check(self):
        """the table froze one slab count per workspace (self.slabs: by the rows of the call); the kernels write as many as the library's ln_rpw knob
        says NOW: under another value the one reduce would add stale slabs, or the workspaces would be too small"""
        for rows, slabs in self.slabs.items():
            if slabs != ops.layernorm_bwd_slabs(rows):
                raise RuntimeError(f"a batched LayerNorm reduce was built for {slabs} slabs over {rows} rows and the library now writes another number: "
                                   "the ln_rpw knob has changed - rebuild the stack (set_options / release_buffers) or restore the knob")

    def slot(self, rows, n0, n1, dcol):
        """the workspace of the next LayerNorm backward of this stack backward"""
        b = self.batch
        if b.desc is None:
            ws = _z((ops.layernorm_bwd_slabs(rows) * 5 * b.D,), F32, self.dev)
            b.add(ws, rows, n0.dg, n0.db, n1.dg if n1 else None, n1.db if n1 else None, dcol)
            self.slabs[rows] = b.entries[-1][1]
        else:
            assert self.k < len(b.entries), "a stack's backward issued more LayerNorm backwards than its first one"
        ws = b.keep[self.k][0]
        self.k += 1
        return ws

    def finish(self):
        b = self.batch
        if b.desc is None:
            b.build(self.dev)
        assert self.k == len(b.entries), "a stack's backward issued fewer LayerNorm backwards than its first one"
        self.k = 0
        b.run()


def _ln_bwd(dy, x, mean, rstd, norms, dx, ws, rows, row_mod=None, out_map=None, dres=None, dx_bf16=None, dcol=None, dx8=None, q8=None, batch=None):
    """dcol: bias gradient of the Linear whose output gradient is the dx produced here (column sum fused in-kernel).
    dx8 / q8: 8-bit copy of dx for an input-gradient GEMM on 8-bit operands, and its device record (Stack._ln_bwd_copy).
    batch (_LnBatch): the parameter gradients are reduced by the batch's one launch at the end of the stack's backward, not here."""
    n0 = norms[0]
    n1 = norms[1] if len(norms) > 1 else None
    if batch is not None:
        ops.layernorm_bwd(dy, x, mean, rstd, n0.g, dx, None, None, batch.slot(rows, n0, n1, dcol), rows, n1.g if n1 else None, None, None,
                          row_mod if n1 else None, out_map, dres, dx_bf16, None, dx8=dx8, q8=q8, defer=True)
        return
    ops.layernorm_bwd(dy, x, mean, rstd, n0.g, dx, n0.dg, n0.db, ws, rows, n1.g if n1 else None, n1.dg if n1 else None,
                      n1.db if n1 else None, row_mod if n1 else None, out_map, dres, dx_bf16, dcol, dx8=dx8, q8=q8)


def _dx_in(stack, lo=0):
    """fp32 buffer, from row lo, for the gradient a stack's backward STARTS from: only the fp32 gradient stream reads it"""
    return None if stack.g16 else stack.dx[0][lo:]


class _SideStream:
    """Weight-gradient GEMMs on a second HIP stream.  A wgrad only needs its two operands to exist and must finish before the
    backward of the NEXT block overwrites the shared scratch it read; nothing downstream waits for its result until the
    optimizer.  AVSIAM_WGRAD_STREAM selects how far that is used:
      2 (default)  wgrads run beside the attention backward, the LayerNorm backward and the column sums only; every
                   forward/dgrad GEMM waits for them (join), so those GEMMs - the kernel bench.py's roofline times - keep
                   the chip to themselves.  -1.0 % step time.
      1            no such restriction (one event per scratch buffer): wgrads also fill the partly empty last rounds of the
                   forward/dgrad GEMMs.  -2.6 % step time, but a GEMM's launch-to-end time then includes the share of the
                   chip the concurrent wgrad holds (per-launch rate reads 0.29 of peak instead of 0.34).
      0            everything on one stream."""

    def __init__(self, dev):
        self.stream = torch.cuda.Stream(device=dev)
        self.done = {}

    def run(self, key, fn):
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        self.stream.wait_event(ready)
        with torch.cuda.stream(self.stream):
            fn()
            d = torch.cuda.Event()
            d.record(self.stream)
        self.done[key] = d

    def before_write(self, key):
        e = self.done.pop(key, None)
        if e is not None:
            torch.cuda.current_stream().wait_event(e)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)
        self.done.clear()


# (EngineOptions.wgrad_stream / wgrad_group: runtime options of the model, config.py)
_side_streams = {}


def _side_stream(dev):
    """One second stream per device for the whole process (a torch.cuda.Stream per backward call would leak pool entries)."""
    key = (dev.type, dev.index)
    if key not in _side_streams:
        _side_streams[key] = _SideStream(dev)
    s = _side_streams[key]
    s.done.clear()
    return s


class _Inline:
    def run(self, key, fn):
        fn()

    def before_write(self, key):
        pass

    def join(self):
        pass


_NO_COPY = {}          # what the 8-bit-copy hooks of Stack add to a kernel call: nothing


def fp8_applies(opts, D, hidden):
    """whether a stack of width D with an MLP of width `hidden` runs on 8-bit GEMM operands: EngineOptions.fp8 asks for it and the fp8 GEMM's
    tile constraints (N % 256, K % 128) hold; any other stack of the model stays bf16"""
    return opts.fp8 in ("1", "2", "3") and D % 256 == 0 and hidden % 256 == 0 and D >= 256


# what a stack's attention runs with: forward tile rows, the (lo, hi] length classes of the fused backward that hold at least one sequence, the
# length above which a sequence takes the two-kernel backward, and that backward's tile rows
AttentionPlan = collections.namedtuple("AttentionPlan", "fwd_rows fused cut bwd_rows")


def attention_plan(seq_lens, hd, *, attn_tile, attn_fused, fused224, inference):
    """The attention kernels' tiling for a packed batch of sequences at head dim `hd` (no device involved): Stack._select_attention builds its
    tile tables from this, tools/bench_attn.py its step mixes.  attn_tile / attn_fused: EngineOptions; fused224: whether the 7-wave fused
    backward may be selected (Stack._fused224); inference: no backward (bwd_rows = fwd_rows, no fused class)."""
    # rows per attention workgroup (4 or 2 waves of 32 queries / keys), by the mean sequence length of the stack - measured on the
    # step's mixes (tools/bench_attn.py --step): the backward of the contrastive pass (39-196 video, 102-512 audio tokens) is 12 %
    # faster with 64-row workgroups, its forward 11 % slower; 49/128-token towers: forward 10 % faster; 618 and 2472 tokens: 128
    mean_len = sum(seq_lens) / max(1, len(seq_lens))
    force = int(attn_tile)                                                # A/B switch: 64 | 128 for every stack and direction
    if hd == 80 and not force:
        force = 128                                                       # hd 80 (ViT-H): the 64-row instantiations exist and lose (round 6, tools/bench_attn.py --huge --tile64:
                                                                          # backward +25 % on the contrastive mix - 232-256 registers, the dK/dV kernel spills)
    fwd_rows = force or (64 if mean_len < 64 else 128)
    if inference:
        return AttentionPlan(fwd_rows, [], 0, fwd_rows)
    # backward: sequences that fit one workgroup (<= 64 / <= 128 tokens: the encoder's video sequences, the MAE towers) take the
    # fused kernel (one read of q, k, v, o, dO and one S / exp evaluation for dq, dk and dv; ops.attn_bwd_fused), the longer ones the
    # two-kernel form.  AVSIAM_ATTN_FUSED=0: everything through the two kernels (A/B).
    # (head dim 80 has the 64-row fused form only - a 128-row workgroup would need 81 KB of LDS: the MAE towers' 64-token frame sequences and the
    #  contrastive pass's 51-token ones; -27 % / -2 % on those stacks' backward attention, tools/bench_attn.py --huge)
    cut = 0 if not attn_fused else {32: 128, 64: 128, 80: 64}.get(hd, 0)
    fused = []
    if cut:
        fused = [(lo, hi) for lo, hi in ((0, 64), (64, cut)) if any(lo < L <= hi for L in seq_lens)]
        # round 6: sequences of 129 .. 224 tokens at head dim 64 (the encoder's 156 / 196-token frames, 204-token audio) in one 7-wave workgroup
        # per (sequence, head) whose dS image holds the queries in two halves (attn_bwd_fused224_kernel)
        if hd == 64 and fused224 and any(128 < L <= 224 for L in seq_lens):
            fused.append((128, 224))
            cut = 224
    long_lens = [L for L in seq_lens if L > cut]
    mean_long = sum(long_lens) / max(1, len(long_lens))
    return AttentionPlan(fwd_rows, fused, cut, force or (64 if mean_long < 256 else 128))


def make_stack(dev, rows, D, H, hidden, seq_lens, blocks, row_mod=None, *, blocks2=None, split=0, inference=False, pool=None, opts=None, q_rows=0):
    """The stack every pass builds (arguments: Stack.__init__): an engine_fp8.Fp8Stack where fp8_applies(), else the bf16 Stack."""
    opts = opts if opts is not None else EngineOptions.from_env()
    cls = Stack
    if fp8_applies(opts, D, hidden):
        from .engine_fp8 import Fp8Stack as cls            # (imported here: engine_fp8 imports this module)
    return cls(dev, rows, D, H, hidden, seq_lens, blocks, row_mod, blocks2=blocks2, split=split, inference=inference, pool=pool, opts=opts, q_rows=q_rows)


class Stack:
    """The transformer blocks `blocks` (BlockParams) over a packed [rows, D] fp32 residual stream with saved activations, GEMM operands in bf16.
    A stack is bound to its parameters when it is built: forward() and backward() run self.blocks (and self.blocks2 from row self.split).
    Methods marked (hook) are what engine_fp8.Fp8Stack overrides to run the same schedule on 8-bit operands; build stacks with make_stack()."""

    fp8 = fp8_bwd = fp8_wgrad = fp8_lean = False          # (the model and the tests ask every stack; Fp8Stack sets them)

    def __init__(self, dev, rows, D, H, hidden, seq_lens, blocks, row_mod=None, *, blocks2=None, split=0, inference=False, pool=None, opts=None, q_rows=0):
        """blocks2 / split: rows [split, rows) run through a SECOND set of blocks (the MAE pass's visual tower next to its audio tower,
        cav_mae_base.py:487,489) in the same launches - every GEMM takes both weight sets (ops.gemm_nt(dual=...)), the LayerNorm picks the
        affine per row (row_mod: 0 below split, 1 from it).
        inference=True: forward only - no activation is kept, every block reuses one set of buffers (the residual stream
        ping-pongs between two) and the backward scratch is not allocated.
        pool (BufferPool): the stack's per-token buffers come from the model's shared activation pool instead of torch.zeros.
        opts (config.EngineOptions): the MODEL's options object, shared by reference - structural fields are read here, runtime fields
        (wgrad_stream, wgrad_group, deterministic) on every backward.
        q_rows > 0 (the decoder, EngineOptions.prune_dead): only the first q_rows rows of every (equal-length) sequence leave the LAST block - the rows
        whose prediction is scored; the others are needed there as keys / values only (cav_mae_base.py:629-635,679-682: loss * mask).  The last
        block then computes LayerNorm-1 and qkv for all rows, attention for q_rows queries per sequence against all keys, and proj / LayerNorm-2 /
        MLP on the COMPACT rows [nseq * q_rows] (sequence s owns rows s * q_rows ..): its att / xmid / ln2 / fc1 / act buffers, x[nblocks] and the
        gradient the backward starts from (dxb[0]) are compact.  `self.lq` says whether the form applies (else 0: plain stack)."""
        assert sum(seq_lens) == rows
        assert pool is None or not inference
        assert blocks2 is None or (len(blocks2) == len(blocks) and row_mod is not None and 0 < split < rows)
        nblocks = len(blocks)
        self.blocks, self.blocks2, self.split = blocks, blocks2, split if blocks2 is not None else 0
        # what reduces over rows into a parameter gradient runs once per row range (lo, hi, the blocks that own those rows)
        self.ranges = [(0, rows, blocks)] if blocks2 is None else [(0, split, blocks), (split, rows, blocks2)]
        self.one = blocks2 is not None               # a row range has ONE affine set; the packed single-tower case selects by row_mod
        self.pool = pool
        self.opts = opts = opts if opts is not None else EngineOptions.from_env()
        self.g16 = opts.grad_stream == "bf16"        # the residual gradient travels between the LayerNorm backwards in bf16 only
        self._pads = ops.ZeroTable() if pool is not None else None

        def _z(shape, dtype, dev_):          # (shadows the module's _z for every allocation below)
            if pool is None:
                return torch.zeros(shape, dtype=dtype, device=dev_)
            t = pool.alloc(shape, dtype)
            if len(shape) == 2 and shape[0] > rows:                          # [token rows + pad, columns]: the pad rows must read as zeros
                self._pads.add(t[rows:])
            return t
        self.rows, self.D, self.H, self.hidden, self.nblocks = rows, D, H, hidden, nblocks
        self.lq = 0                             # (set below when the pruned last block applies)
        self.row_mod = row_mod
        self.inference = inference
        self.nrecomp = 0 if inference else recompute_blocks(nblocks, opts.recompute)     # blocks [0, nrecomp) keep no activations (one shared set)
        self.recompute = self.nrecomp > 0
        self._ln_batch = self._vm_batch = None            # batched reduces of the backward: built by the first backward that uses them
        self._alloc_operand_copies(_z, dev)
        rp = ops.pad_rows(rows, 128)
        self.rp = rp
        self._select_attention(seq_lens, dev)
        self.q_scale = ops.attn_q_scale(D // H)          # q leaves the qkv GEMM ready for the attention kernels

        def per_block(shape, dtype):
            if inference:                                     # one buffer for all blocks
                return [_z(shape, dtype, dev)] * nblocks
            # recomputed blocks share one buffer, refilled in front of each one's backward; the others keep their own
            one = _z(shape, dtype, dev) if self.nrecomp else None
            return [one if i < self.nrecomp else _z(shape, dtype, dev) for i in range(nblocks)]

        if inference:
            ping = [_z((rp, D), F32, dev) for _ in range(2)]
            self.x = [ping[i & 1] for i in range(nblocks + 1)]
        else:
            self.x = [_z((rp, D), F32, dev) for _ in range(nblocks + 1)]     # x[i] = input of block i; x[-1] = output
        def one_for_all(shape, dtype):
            return [_z(shape, dtype, dev)] * nblocks
        shared, codes = self._buffer_policy()
        operand = one_for_all if shared else per_block
        self.xmid = per_block((rp, D), F32)
        self.ln1 = operand((rp, D), BF16)
        self.ln2 = self.ln1 if (inference or shared) else per_block((rp, D), BF16)
        self.qkv = per_block((rp, 3 * D), BF16)
        self.att = per_block((rp, D), BF16)
        self.fc1 = per_block((rp, hidden), U8 if codes else BF16)      # gelu'(fc1 output): all the backward needs of the pre-activation (gemm act 1 / 2)
        self.act = operand((rp, hidden), BF16)
        self.lse = per_block((H, rp), F32)
        nshared = nblocks if inference else self.nrecomp
        st = [_z((rp,), F32, dev) for _ in range(4)] if nshared else None
        self.stats = [st if i < nshared else [_z((rp,), F32, dev) for _ in range(4)] for i in range(nblocks)]   # mean1 rstd1 mean2 rstd2
        if inference:
            return
        # backward scratch (shared by all blocks)
        self.dx = [_z((rp, D), F32, dev) for _ in range(2)]
        self.dxb = [_z((rp, D), BF16, dev) for _ in range(2)]
        self.dfc1 = _z((rp, hidden), BF16, dev)
        self.dln = _z((rp, D), BF16, dev)
        self.datt = _z((rp, D), BF16, dev)
        self.dqkv = _z((rp, 3 * D), BF16, dev)
        self.delta = _z((H, rp), F32, dev)
        self.lnws = _z((ops.layernorm_ws(rows, D),), F32, dev)
        self._setup_pruned(q_rows, seq_lens, dev)

    def _select_attention(self, seq_lens, dev):
        """tile tables of the attention kernels (attention_plan): self.tiles (forward), self.fused_bwd / self.tiles_bwd (backward)"""
        plan = attention_plan(seq_lens, self.D // self.H, attn_tile=self.opts.attn_tile, attn_fused=self.opts.attn_fused, fused224=self._fused224(),
                              inference=self.inference)
        self.tiles = ops.AttnTiles(seq_lens, dev, tile_rows=plan.fwd_rows)
        self.fused_bwd = [ops.AttnSeqs(seq_lens, dev, lo, hi) for lo, hi in plan.fused]
        self.tiles_bwd = self.tiles if self.inference else ops.AttnTiles(seq_lens, dev, tile_rows=plan.bwd_rows, min_len=plan.cut)

    def _setup_pruned(self, q_rows, seq_lens, dev):
        """the pruned last block (Stack.__init__, q_rows): sets self.lq and the row maps where the form applies"""
        rows, nblocks, row_mod = self.rows, self.nblocks, self.row_mod
        # applies to stacks of equal-length sequences with plain norms, the bf16 gradient stream and the
        # two-kernel attention backward (the decoder: 2 472-token sequences)
        if (q_rows and row_mod is None and self.g16 and self.tiles.uniform_len and self.tiles_bwd.uniform_len
                and not self.fused_bwd and 0 < q_rows < seq_lens[0] and nblocks >= 1):
            assert self.blocks2 is None, "the pruned last block has one weight set"
            L, nseq = seq_lens[0], len(seq_lens)
            self.lq, self.Mq = int(q_rows), nseq * int(q_rows)
            c = torch.arange(self.Mq)
            self.q_full = ((c // q_rows) * L + c % q_rows).to(I32).to(dev)                       # compact row -> packed row (residual gather of proj)
            r = torch.arange(rows)
            self.q_compact = torch.where(r % L < q_rows, (r // L) * q_rows + r % L, torch.full_like(r, -1)).to(I32).to(dev)     # packed row -> compact row | -1
            # rows [Mq, next multiple of 128) of the compact activations are read by the weight-gradient GEMMs (whole 64-row stages): they must be
            # zero whatever another block (shared recompute buffers) or another pass (pooled memory) left there
            self._qpads = ops.ZeroTable()
            last = nblocks - 1
            padq = ops.pad_rows(self.Mq, 128)
            if padq > self.Mq:
                for buf in (self.att[last], self.ln2[last], self.act[last]):
                    self._qpads.add(buf[self.Mq:padq])
                self._qpads.build(dev)

    # ---- hooks of the constructor
    def _alloc_operand_copies(self, z, dev):
        """(hook) buffers allocated ahead of the activations (z: the constructor's allocator): none here"""

    def _fused224(self):
        """(hook) whether the 7-wave fused attention backward (129 .. 224 tokens) may be selected"""
        return self.opts.attn_fused224

    def _buffer_policy(self):
        """(hook) (shared, codes).  shared: the GEMM operands ln1 / ln2 / act live in one buffer for all blocks instead of one per block;
        codes: gelu'(x) travels from fc1 to the fc2 input-gradient GEMM as 8-bit fixed-point codes instead of bf16 (EngineOptions.gelu8)"""
        return False, bool(self.opts.gelu8 and not self.inference)

    @property
    def out(self):
        return self.x[self.nblocks]

    def forward(self):
        if self._pads is not None:            # pooled buffers: another pass has written over them since this stack last ran
            if self._pads.desc is None and self._pads.entries:
                self._pads.build(self.x[0].device)
            self._pads.run()
        self._forward_begin()
        for i in range(self.nblocks):
            self._block_forward(i)

    def _forward_begin(self):
        """(hook) in front of the first block of a forward: nothing here"""

    def _block_forward(self, i, last_gemm=True):
        """(hook) Block i: x[i] -> x[i + 1] and everything its backward reads.  last_gemm=False (recompute in front of the backward): x[i + 1]
        is not needed again, the fc2 GEMM is skipped."""
        M = Mu = self.rows
        bp, b2 = self.blocks[i], self.blocks2[i] if self.blocks2 is not None else None
        x, st = self.x[i], self.stats[i]
        n1 = bp.n1 if b2 is None else [bp.n1[0], b2.n1[0]]
        n2 = bp.n2 if b2 is None else [bp.n2[0], b2.n2[0]]
        lq, res_idx = 0, None
        if self.lq and i == self.nblocks - 1:
            # pruned last block (see __init__; one weight set, no row_mod): every row is a key / value, the first lq rows of a sequence are the
            # queries; from the attention output on the block lives on the compact rows
            self._qpads.run()
            Mu, lq, res_idx = self.Mq, self.lq, self.q_full
        dq = dp = d1 = d2 = None
        if b2 is not None:
            dq, dp = (self.split, b2.qkv.w, b2.qkv.b, None), (self.split, b2.proj.w, b2.proj.b, None)
            d1, d2 = (self.split, b2.fc1.w, b2.fc1.b, None), (self.split, b2.fc2.w, b2.fc2.b, None)
        _ln_fwd(x, n1, self.ln1[i], st[0], st[1], M, LN_EPS_BLOCK, self.row_mod)
        ops.gemm_nt(self.ln1[i], bp.qkv.w, self.qkv[i], M, bias=bp.qkv.b, scale_cols=self.D, col_scale=self.q_scale, dual=dq)
        ops.attn_fwd(self.qkv[i], self.tiles, self.H, self.att[i], self.lse[i], lq=lq)
        ops.gemm_nt(self.att[i], bp.proj.w, self.xmid[i], Mu, bias=bp.proj.b, res=x, res_idx=res_idx, dual=dp)
        _ln_fwd(self.xmid[i], n2, self.ln2[i], st[2], st[3], Mu, LN_EPS_BLOCK, self.row_mod)
        ops.gemm_nt(self.ln2[i], bp.fc1.w, self.fc1[i], Mu, bias=bp.fc1.b, out2=self.act[i], act=1, dual=d1)
        if last_gemm:
            ops.gemm_nt(self.act[i], bp.fc2.w, self.x[i + 1], Mu, bias=bp.fc2.b, res=self.xmid[i], dual=d2)

    # ---- backward: backward() is the schedule of one call; `c` carries the call's arguments and choices to the per-block methods
    def backward(self, last_fc2_bias_done=False, reducer=None, accumulate=False):
        """In: d(out) in self.dxb[0] (bf16) - and in self.dx[0] (fp32) when GRAD_STREAM is "fp32".  Out: d(x[0]) in self.dx[0] (fp32)
        and self.dxb[0].
        reducer (comm.GradReducer, data parallel): told which ranges of the gradient arena are final as the blocks complete.
        Bias gradients of fc2 / proj are column sums of the residual-stream gradient and come out of the LayerNorm
        backward that produces it (`dcol`); `last_fc2_bias_done` says the caller's LN backward already did that for
        the last block.
        accumulate: the parameter gradients may already hold another pass's contribution (one backward over both passes of a
        combined forward): quantities derived FROM a parameter gradient then use this backward's increment only.
        Two weight sets (blocks2): the input-gradient GEMMs take both in one launch; everything that reduces over rows into a
        parameter gradient (weight-gradient GEMMs, bias column sums, LayerNorm backward with its gamma/beta/bias sums) runs once
        per row range (self.ranges) on row slices of the same buffers."""
        assert not self.inference, "Stack(inference=True) keeps no activations"
        det = bool(self.opts.deterministic)          # one stream, no epilogue atomics; the library's own reductions follow the "det" knob (the model sets it)
        # the small per-block reduces in ONE launch each at the end of the stack's backward - unless something wants a block's gradients final as it
        # completes (the data-parallel reducer), the gradients accumulate over two passes, or the deterministic forms are asked for
        batched = reducer is None and not accumulate and not det and self.opts.batch_reduce
        if batched and self._ln_batch is not None:
            self._ln_batch.check()                   # (raises before a gradient epoch is claimed or a kernel of this backward is queued)
        self._claim_epoch(accumulate)
        c = SimpleNamespace(reducer=reducer, accumulate=accumulate, last_fc2_bias_done=last_fc2_bias_done, done=set(), det=det,
                            ln_batch=None, vm_batch=None)
        c.side, c.excl, c.grp = self._stream_mode()
        if batched:
            c.ln_batch, c.vm_batch = self._reduce_batches()
        self._backward_begin(c)
        for i in reversed(range(self.nblocks)):
            self._block_backward(c, i)
        c.side.join()
        if c.ln_batch is not None:
            c.ln_batch.finish()        # (before the value thirds: they read the complete proj bias gradients, which are LayerNorm-2 column sums)
        if c.vm_batch is not None:
            c.vm_batch.run()
        for j in reversed(range(self.nblocks)):        # (mode 2 has reported all but block 0 on the way)
            self._block_done(c, j)

    def _claim_epoch(self, accumulate):
        """a second backward over a block since its gradients were zeroed must say accumulate=True (the value third of the qkv bias gradient is
        a vector-matrix product of the WHOLE accumulated proj bias gradient) - checked before any kernel is queued, so a refused call
        leaves the gradient arena untouched"""
        owned = [bp for lo_, hi_, bl in self.ranges for bp in bl]
        for bp in owned:
            if not accumulate and bp.arena.gb_epoch.get(bp.prefix) == bp.arena.zero_epoch:
                raise RuntimeError(f"{bp.prefix}: second backward over this block since its gradients were zeroed - pass accumulate=True "
                                   "(or zero the gradients with arena.zero_grad_range)")
        for bp in owned:
            bp.arena.gb_epoch[bp.prefix] = bp.arena.zero_epoch

    def _stream_mode(self):
        """(side, excl, grp) of one backward (_SideStream).  side: where the weight-gradient GEMMs run; excl (mode 2): beside the attention /
        LayerNorm backward and the column sums only - every nt GEMM waits for them; grp: a block's fc2 / fc1 / proj weight gradients are
        issued together (one grouped launch) - mode 1 issues each as early as its operands exist.
        Recompute: the blocks share ONE set of activation buffers, refilled in front of every block's backward - weight-gradient GEMMs still
        reading them on a second stream would race with the refill, so everything runs on one stream (a partially recomputed stack uses the
        second stream for the blocks that keep their own buffers and joins it in front of the first recomputed block, _block_backward)."""
        mode = "0" if (self.nrecomp >= self.nblocks or self.opts.deterministic) else self.opts.wgrad_stream
        if mode == "auto":            # small stacks: the weight gradients also fill the partial rounds of the forward / input-gradient GEMMs (config.EngineOptions)
            mode = "2" if self.rows >= 32768 else "1"
        side = _side_stream(self.dx[0].device) if mode in ("1", "2") else _Inline()
        return side, mode == "2", mode in ("2", "0")

    def _reduce_batches(self):
        """(ln_batch, vm_batch): the parameter-gradient reduces of the LayerNorm backwards (_LnBatch) and the value thirds of the blocks' qkv bias
        gradients (a [D] x [D, D] product each, _attn_backward) as one launch each instead of one ~10-us launch per block"""
        dev = self.dx[0].device
        if self._ln_batch is None:
            self._ln_batch = _LnBatch(self.D, dev)
        self._ln_batch.k = 0
        if self._vm_batch is None:
            self._vm_batch = ops.VecmatBatch()
            for lo_, hi_, bl in self.ranges:
                for bp in bl:
                    self._vm_batch.add(bp.proj.gb, bp.proj.w, bp.qkv.gb[2 * self.D:])
            self._vm_batch.build(dev)
        return self._ln_batch, self._vm_batch

    def _block_done(self, c, j):
        """Every kernel writing block j's parameter gradients is queued on the current stream or joined into it."""
        if j in c.done:
            return
        c.done.add(j)
        if c.reducer is not None:
            for lo_, hi_, bl in self.ranges:
                for a, b in bl[j].ranges:
                    c.reducer.ready(a, b)

    def _wgrads(self, c, blk, key, *jobs, rows=None):
        """Weight gradients (gradient, layer input, Linear) of block blk on c.side; the jobs of one call share their token rows.
        rows: the jobs' token rows when they are not the stack's (the pruned last block's compact rows)"""
        def fn():
            for lo, hi, bl in (self.ranges if rows is None else [(0, rows, self.blocks)]):
                self._wgrad(blk, jobs, bl, lo, hi)
        c.side.run(key, fn)

    def _wgrad(self, blk, jobs, bl, lo, hi):
        """(hook) the jobs over one row range [lo, hi) into the gradients of bl[blk]: one grouped launch (ops.gemm_tn_group)"""
        trip = [(a[lo:], b[lo:], getattr(bl[blk], name).gw) for a, b, name in jobs]
        if self.opts.wgrad_group:
            ops.gemm_tn_group(trip, hi - lo)
        else:
            for A, B, C in trip:
                ops.gemm_tn(A, B, C, hi - lo)

    def _backward_begin(self, c):
        """(hook) in front of the last block's backward: nothing here"""

    def _dgrad(self, c, i, name, dy, out, M):
        """(hook) input-gradient GEMM of block i's Linear `name` over M rows: out = dy @ W, both weight sets in one launch.
        fc2: times the gelu'(x) fc1 saved, + the fc1 bias gradient as the epilogue's column sum (not in deterministic mode)"""
        bp, b2 = self.blocks[i], self.blocks2[i] if self.blocks2 is not None else None
        if name != "fc2":
            ops.gemm_nt(dy, getattr(bp, name).wt, out, M, dual=(self.split, getattr(b2, name).wt, None, None) if b2 is not None else None)
            return
        ops.gemm_nt(dy, bp.fc2.wt, out, M, aux=self.fc1[i], act=2, colsum=None if c.det else bp.fc1.gb,
                    dual=(self.split, b2.fc2.wt, None, None if c.det else b2.fc1.gb) if b2 is not None else None)

    def _ln_bwd_copy(self, blk, name, lo):
        """(hook) what a LayerNorm backward is passed to also write an 8-bit copy, from row lo, of the gradient `name` (dbo | dbm) of block blk"""
        return _NO_COPY

    def _attn_bwd_copy(self, i):
        """(hook) the same for the attention backward kernels and dqkv"""
        return _NO_COPY

    def _block_backward(self, c, i):
        if i < self.nrecomp:
            if not isinstance(c.side, _Inline):      # from here down the blocks share one set of activation buffers: one stream
                c.side.join()
                if c.excl and i + 1 < self.nblocks:
                    self._block_done(c, i + 1)
                c.side, c.excl, c.grp = _Inline(), False, True
            self._block_forward(i, last_gemm=False)
        pruned = bool(self.lq) and i == self.nblocks - 1        # the block's upper half (proj ... fc2) lives on the compact rows [0, Mq)
        self._mlp_backward(c, i, pruned)
        self._attn_backward(c, i, pruned)

    def _mlp_backward(self, c, i, pruned):
        """fc2, fc1 and LayerNorm-2 of block i: d(x[i + 1]) in dxb[0] (and dx[0]) -> d(xmid) in dxb[1] (and dx[1])"""
        side, grp, st = c.side, c.grp, self.stats[i]
        dxo, dxm = self.dx
        dbo, dbm = self.dxb
        Mu = self.Mq if pruned else self.rows
        ranges, rows = ([(0, Mu, self.blocks)], Mu) if pruned else (self.ranges, None)
        # fc2: d(gelu out) fused with GELU' -> d(fc1 pre-activation)
        if c.excl:
            side.join()
            if i + 1 < self.nblocks:
                self._block_done(c, i + 1)     # its last wgrad (qkv) was the side stream's tail; fc2's bias came from this LN backward
        else:
            side.before_write("dfc1")
        self._dgrad(c, i, "fc2", dbo, self.dfc1, Mu)
        if c.det:                 # deterministic mode: the fc1 bias gradient by the column-sum kernel (one writer per element) instead of the epilogue's atomics
            for lo, hi, bl in ranges:
                ops.colsum(self.dfc1[lo:], bl[i].fc1.gb, hi - lo)
        if not grp:
            self._wgrads(c, i, "dbo", (dbo, self.act[i], "fc2"), rows=rows)
        if i == self.nblocks - 1 and not c.last_fc2_bias_done:
            for lo, hi, bl in ranges:
                ops.colsum(dbo[lo:], bl[i].fc2.gb, hi - lo)
        # fc1
        self._dgrad(c, i, "fc1", self.dfc1, self.dln, Mu)
        if not grp:
            self._wgrads(c, i, "dfc1", (self.dfc1, self.ln2[i], "fc1"), rows=rows)
            side.before_write("dbm")
        for lo, hi, bl in ranges:
            if c.accumulate:          # value third of the qkv bias gradient (_attn_backward): minus what proj.gb holds before this block adds to it
                ops.vecmat(bl[i].proj.gb, bl[i].proj.w, bl[i].qkv.gb[2 * self.D:], -1.0)
            _ln_bwd(self.dln[lo:], self.xmid[i][lo:], st[2][lo:], st[3][lo:], bl[i].n2, None if self.g16 else dxm[lo:], self.lnws, hi - lo,
                    None if self.one else self.row_mod, dres=(dbo if self.g16 else dxo)[lo:], dx_bf16=dbm[lo:], dcol=bl[i].proj.gb,
                    batch=c.ln_batch, **self._ln_bwd_copy(i, "dbm", lo))

    def _attn_backward(self, c, i, pruned):
        """proj, attention, qkv and LayerNorm-1 of block i: d(xmid) in dxb[1] (and dx[1]) -> d(x[i]) in dxb[0] (and dx[0])"""
        side, excl, st, M, D = c.side, c.excl, self.stats[i], self.rows, self.D
        dxo, dxm = self.dx
        dbo, dbm = self.dxb
        rows = self.Mq if pruned else None
        # proj
        self._dgrad(c, i, "proj", dbm, self.datt, rows or M)
        if c.grp:                 # the three wgrads whose operands exist now run beside the attention backward
            self._wgrads(c, i, "blockA", (dbo, self.act[i], "fc2"), (self.dfc1, self.ln2[i], "fc1"), (dbm, self.att[i], "proj"), rows=rows)
        else:
            self._wgrads(c, i, "dbm", (dbm, self.att[i], "proj"), rows=rows)
            side.before_write("dqkv")
        copy = self._attn_bwd_copy(i)
        if pruned:
            # queries: the first lq rows of every sequence (out / dO compact); dk, dv for every row.  The query third of the other rows of dqkv
            # is zero by definition (they asked nothing), and the residual gradient of the compact rows goes back into the packed numbering
            # for LayerNorm-1's backward - zeros for the rows that were keys / values only - through the freed dO buffer
            ops.attn_bwd(self.qkv[i], self.tiles_bwd, self.H, self.att[i], self.datt, self.lse[i], self.delta, self.dqkv, lq=self.lq)
            ops.expand_rows(None, self.q_compact, self.dqkv, M, cols=D)
            ops.expand_rows(dbm, self.q_compact, self.datt, M)
        elif self.tiles_bwd.ntiles:
            ops.attn_bwd(self.qkv[i], self.tiles_bwd, self.H, self.att[i], self.datt, self.lse[i], self.delta, self.dqkv, **copy)
        for sq in self.fused_bwd:
            ops.attn_bwd_fused(self.qkv[i], sq, self.H, self.att[i], self.datt, self.lse[i], self.dqkv, **copy)
        # qkv
        if excl:
            side.join()
        self._dgrad(c, i, "qkv", self.dqkv, self.dln, M)
        self._wgrads(c, i, "dqkv", (self.dqkv, self.ln1[i], "qkv"))
        if not excl:
            side.before_write("dbo")
        for lo, hi, bl in self.ranges:
            # qkv bias gradient: only the query third needs the dqkv matrix.  value third = column sum of dO = (proj bias
            # gradient, complete since this block's LayerNorm-2 backward) . W_proj; key third = 0 exactly (ops.vecmat)
            ops.colsum(self.dqkv[lo:, :D], bl[i].qkv.gb[:D], hi - lo)
            # (the vector-matrix product reads the WHOLE accumulated proj bias gradient: a second backward over the same block
            #  between two zero-fills must say accumulate=True, or the value third would be counted twice - ADVICE r3; _claim_epoch)
            if c.vm_batch is None:
                ops.vecmat(bl[i].proj.gb, bl[i].proj.w, bl[i].qkv.gb[2 * D:])
            # (the 8-bit copy: the block below reads this gradient through its fc2 input-gradient GEMM)
            _ln_bwd(self.dln[lo:], self.x[i][lo:], st[0][lo:], st[1][lo:], bl[i].n1, None if self.g16 and i > 0 else dxo[lo:], self.lnws,
                    hi - lo, None if self.one else self.row_mod, dres=(self.datt if pruned else dbm if self.g16 else dxm)[lo:], dx_bf16=dbo[lo:],
                    dcol=bl[i - 1].fc2.gb if i > 0 else None, batch=c.ln_batch, **self._ln_bwd_copy(i - 1, "dbo", lo))


class PatchEmbedder:
    """Kept-token patch embedding: im2col gather -> GEMM with fused (+bias +pos_embed[token]) * 2 epilogue
    (cav_mae_base.py:444-455: conv, +pos, then `x + norm_pre(x)` with norm_pre = Identity)."""

    def __init__(self, arena, dev, rows, audio, cfg, row_src=None, row_tok=None):
        self.audio, self.rows, self.cfg = audio, rows, cfg
        pre = "vit_base.patch_embed_a" if audio else "vit_base.patch_embed"
        self.lin = Linear(arena, pre + ".proj.weight", pre + ".proj.bias", need_t=False)
        pname = "vit_base.pos_embed_a" if audio else "vit_base.pos_embed"
        D = cfg.embed_dim
        skip = 0 if audio else 1          # the visual table starts with the cls row (pos_embed[:, 1:, :], cav_mae_base.py:453): token t is row 1 + t
        self.pos = arena.view(pname).view(-1, D)[skip:]
        self.gpos = arena.gview(pname).view(-1, D)[skip:] if arena.g is not None else None
        K = cfg.patch * cfg.patch * (1 if audio else cfg.in_chans)
        rp = ops.pad_rows(rows, 128)
        self.cols = _z((rp, K), BF16, dev)
        self.dy = _z((rp, D), BF16, dev)
        # sample (audio) / frame image (video) and token id of each row; may be slices of a buffer the mask-plan kernel fills
        self.row_src = row_src if row_src is not None else _z((rows,), I32, dev)
        self.row_tok = row_tok if row_tok is not None else _z((rows,), I32, dev)      # = row of self.pos / self.gpos

    def set_rows(self, row_src, row_tok):
        self.row_src.copy_(row_src, non_blocking=True)
        self.row_tok.copy_(row_tok, non_blocking=True)

    def forward(self, inp, out, xf=None, aug=None):
        """inp: audio [B,time,mel] / video [NF,3,H,W] fp32 - or the raw input (un-normalised fbank / uint8 frames) with its
        transform `xf` (ops.InputXf); out: fp32 [rows(+pad), D] slice of the residual stream.
        aug (ops.FtAug, audio only): the fine-tuning augmentation applied inside the gather.  The gathered rows (self.cols) ARE the augmented
        patches, and the weight gradient of backward() reads those saved rows: the backward needs nothing of `xf` or `aug`."""
        if self.audio:
            if aug is not None:
                ops.im2col_audio(inp, self.row_src, self.row_tok, self.cols, self.rows, self.cfg.audio_t, xf, stride=self.cfg.st, aug=aug)
            else:
                ops.im2col_audio(inp, self.row_src, self.row_tok, self.cols, self.rows, self.cfg.audio_t, xf, stride=self.cfg.st)
        else:
            ops.im2col_video(inp, self.row_src, self.row_tok, self.cols, self.rows, xf, stride=self.cfg.st)
        ops.gemm_nt(self.cols, self.lin.w, out, self.rows, bias=self.lin.b, res=self.pos, res_idx=self.row_tok, alpha=2.0)

    def backward(self, dx):
        """dx: fp32 [rows, D] gradient of the embedding output."""
        D = self.cfg.embed_dim
        ops.cast_scale(dx, self.dy, self.rows * D, 2.0)
        ops.gemm_tn(self.dy, self.cols, self.lin.gw, self.rows)
        ops.colsum(self.dy, self.lin.gb, self.rows)
        ops.scatter_add_rows(self.dy, self.row_tok, self.gpos, self.rows)


def _fold_frames(imgs, T):
    if imgs.dim() == 4:
        assert T == 1
        return imgs
    assert imgs.shape[1] == T
    return imgs.reshape(imgs.shape[0] * T, *imgs.shape[2:])


# =====================================================================================================
class ContrastivePass:
    """Pass 1 (forward_encoder_mmixed + forward_contrastive, cav_mae_base.py:508-594,641-661)."""

    def __init__(self, arena: ParamArena, cfg: AVSiamConfig, batch, dev, world=1, rank=0, comm=None, pool=None, opts=None):
        self.arena, self.cfg, self.B, self.dev, self.world, self.rank = arena, cfg, batch, dev, world, rank
        self.comm = comm
        self.pool = pool
        self.opts = opts = opts if opts is not None else EngineOptions.from_env()
        if pool is not None:
            pool.rewind()                      # (BufferPool: this pass's stacks start at the first byte, over the other pass's)
        assert world == 1 or comm is not None, "data parallel needs a collective (model.set_distributed)"
        self.dp = comm is not None and getattr(comm, "active", world > 1)
        T, D = cfg.frames, cfg.embed_dim
        sizes = group_sizes(batch, cfg.n_groups)
        self.sizes = sizes
        self.keep_a = [len_keep(cfg.audio_tokens, group_ratio(g)) for g in range(len(sizes))]
        self.keep_v = [len_keep(cfg.video_tokens, group_ratio(g)) for g in range(len(sizes))]
        lens_a = [self.keep_a[g] for g, n in enumerate(sizes) for _ in range(n)]
        lens_v = [self.keep_v[g] for g, n in enumerate(sizes) for _ in range(n * T)]
        self.rows_a, self.rows_v = sum(lens_a), sum(lens_v)
        rows = self.rows_a + self.rows_v
        self.rows = rows
        row_mod = torch.cat([torch.zeros(self.rows_a, dtype=U8), torch.ones(self.rows_v, dtype=U8)]).to(dev)
        self.blocks = [BlockParams(arena, f"vit_base.blocks.{i}", "_a", "_v") for i in range(cfg.depth)]
        self.stack = make_stack(dev, rows, D, cfg.num_heads, D * cfg.mlp_ratio, lens_a + lens_v, self.blocks, row_mod, pool=pool, opts=opts)
        self.final = [Norm(arena, "vit_base.norm_a"), Norm(arena, "vit_base.norm")]
        self.row_src_all, self.row_tok_all = _z((rows,), I32, dev), _z((rows,), I32, dev)
        self.emb_a = PatchEmbedder(arena, dev, self.rows_a, True, cfg, self.row_src_all[:self.rows_a], self.row_tok_all[:self.rows_a])
        self.emb_v = PatchEmbedder(arena, dev, self.rows_v, False, cfg, self.row_src_all[self.rows_a:], self.row_tok_all[self.rows_a:])
        # device-side plan: sequence descriptors (static except src_id = the sample a slot holds this step)
        La, Lv = cfg.audio_tokens, cfg.video_tokens
        nseq = batch + batch * T
        d = np.zeros((nseq, ops.PLAN_FIELDS), dtype=np.int32)
        self.slot_group = np.array([g for g, n in enumerate(sizes) for _ in range(n)], dtype=np.int64)
        off = 0
        for sl in range(batch):
            g = self.slot_group[sl]
            d[sl] = [La, self.keep_a[g], off, 0, -1, 0, cfg.audio_t, sl * La, 0, 0, 0, 0] + ops.PLAN_CLASSIC
            off += self.keep_a[g]
        for sl in range(batch):
            g = self.slot_group[sl]
            for t in range(T):
                d[batch + sl * T + t] = [Lv, self.keep_v[g], off, 0, -1, 0, 0, batch * La + (sl * T + t) * Lv, 0, 0, 0, 0] + ops.PLAN_CLASSIC
                off += self.keep_v[g]
        assert off == rows
        self.desc_host = d
        self.desc_dev = torch.from_numpy(d).to(dev)
        self.bits_host = np.zeros((3, nseq), dtype=np.int32)           # tmask_lo, tmask_hi, fmask per sequence
        self.bits_dev = torch.zeros((3, nseq), dtype=I32, device=dev)
        self.ids_dev = _z((batch * La + batch * T * Lv,), I32, dev)
        self.last_perm = None
        # pooling segments: B audio sequences then B video samples (T frames each), slot order = group-major
        seg = [0]
        for L in lens_a:
            seg.append(seg[-1] + L)
        k = 0
        for g, n in enumerate(sizes):
            for _ in range(n):
                seg.append(seg[-1] + T * self.keep_v[g])
        self.seg_start = torch.tensor(seg, dtype=I32, device=dev)
        self.yf = _z((self.stack.rp, D), F32, dev)
        self.fstat = [_z((self.stack.rp,), F32, dev) for _ in range(2)]
        # slot (group-major position in the packed stack) -> sample: row 0 maps a slot to its row of `reps` ([a samples | v samples]),
        # row 1 to its row of `dAV` ([dA of all W*B samples | dV ...]: this rank's slice) - both folded into the token-mean kernels
        self.slot_maps = _z((2, 2 * batch), I32, dev)
        self.reps = _z((2 * batch, D), F32, dev)
        N = world * batch
        self.N = N
        self.all_reps = _z((world, 2 * batch, D), F32, dev)
        if world == 1:
            self.A, self.V = self.reps[:batch], self.reps[batch:]         # one rank: the embeddings ARE the batch
        else:
            self.A, self.V = _z((N, D), F32, dev), _z((N, D), F32, dev)
        self.An, self.Vn = _z((N, D), F32, dev), _z((N, D), F32, dev)
        self.na, self.nv = _z((N,), F32, dev), _z((N,), F32, dev)
        self.total, self.dtotal = _z((N, N), F32, dev), _z((N, N), F32, dev)
        self.nstats, self.nout = _z((N, 4), F32, dev), _z((3,), F32, dev)
        self.dAn, self.dVn = _z((N, D), F32, dev), _z((N, D), F32, dev)
        self.dAV = _z((2 * N, D), F32, dev)
        self.dA, self.dV = self.dAV[:N], self.dAV[N:]

    # ---- plan -> index arrays (host, O(rows) ints) --------------------------------------------------
    def _set_plan(self, plan: ContrastivePlan):
        B, T = self.B, self.cfg.frames
        assert plan.batch == B
        ag, vg = plan.a_group.numpy(), plan.v_group.numpy()
        counts_a = np.bincount(ag, minlength=len(self.sizes)).tolist()
        counts_v = np.bincount(vg, minlength=len(self.sizes)).tolist()
        assert counts_a[:len(self.sizes)] == self.sizes and counts_v[:len(self.sizes)] == self.sizes, "plan groups do not match torch.chunk sizes"
        order_a = np.argsort(ag, kind="stable")
        order_v = np.argsort(vg, kind="stable")
        src_a, tok_a = [], []
        for s in order_a:
            ids = plan.a_keep[s]
            assert ids.numel() == self.keep_a[ag[s]]
            tok_a.append(ids)
            src_a.append(torch.full((ids.numel(),), int(s), dtype=torch.int64))
        src_v, tok_v = [], []
        for s in order_v:
            for t in range(T):
                ids = plan.v_keep[s][t]
                assert ids.numel() == self.keep_v[vg[s]]
                tok_v.append(ids)
                src_v.append(torch.full((ids.numel(),), int(s) * T + t, dtype=torch.int64))
        self.emb_a.set_rows(torch.cat(src_a).to(I32), torch.cat(tok_a).to(I32))
        self.emb_v.set_rows(torch.cat(src_v).to(I32), torch.cat(tok_v).to(I32))
        self._set_slot_maps(np.concatenate([order_a, B + order_v]))

    def _set_slot_maps(self, s2r):
        """s2r[slot] = row of `reps` (a sample below B, B + v sample from B) the slot's sequence(s) belong to"""
        B, r, N = self.B, self.rank, self.N
        s2r = np.asarray(s2r, dtype=np.int64)
        assert s2r.shape == (2 * B,) and sorted(s2r.tolist()) == list(range(2 * B))
        src = np.where(s2r < B, r * B + s2r, N + r * B + (s2r - B))           # the same sample's row of dAV (this rank's slice)
        self.slot_maps.copy_(torch.from_numpy(np.stack([s2r, src]).astype(np.int32)), non_blocking=True)

    def draw_device(self, seed, nprng, seed_dev=None, host=True):
        """Draw this step's plan on the device (ops.mask_plan): the host only picks the two batch permutations
        (torch.chunk(randperm) at cav_mae_base.py:533-538) and the structured time/frequency selections (:415-422).
        host=False: the host part (draw_host: numpy draws + three small host-to-device copies) has been done by the caller - a step
        replayed from a captured graph (graph_step) does it in front of every replay; seed_dev: the Philox key in device memory."""
        if host:
            self.draw_host(nprng)
        ops.mask_plan(self.desc_dev, self.desc_host, seed, self.row_src_all, self.row_tok_all, self.bits_dev[0], self.bits_dev[1], self.bits_dev[2],
                      ids_out=self.ids_dev, seed_dev=seed_dev)

    def draw_host(self, nprng):
        B, T = self.B, self.cfg.frames
        perm_a, perm_v, bits, tmask_x = draw_structured(self.cfg, self.slot_group, nprng)      # (the numpy part: maskplan.py)
        d = self.desc_host
        d[:B, 3] = perm_a
        d[B:, 3] = (perm_v[:, None] * T + np.arange(T)[None, :]).reshape(-1)
        self.bits_host[:] = 0
        self.bits_host[:, :B] = bits
        d[:B, 9] = tmask_x                                       # time patches 64.. travel in the descriptor (PlanSeq.tmask_x)
        self.desc_dev.copy_(torch.from_numpy(d), non_blocking=True)
        self.bits_dev.copy_(torch.from_numpy(self.bits_host), non_blocking=True)
        self._set_slot_maps(np.concatenate([perm_a, B + perm_v]))
        self.last_perm = (perm_a, perm_v)

    def last_plan(self):
        """Rebuild the ContrastivePlan the device drew (tests / debugging; synchronises)."""
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        La, Lv = cfg.audio_tokens, cfg.video_tokens
        ids = self.ids_dev.cpu().long()
        perm_a, perm_v = self.last_perm
        a_group, v_group = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
        a_keep, v_keep = [None] * B, [None] * B
        for sl in range(B):
            g = int(self.slot_group[sl])
            a_group[perm_a[sl]] = g
            v_group[perm_v[sl]] = g
            a_keep[int(perm_a[sl])] = ids[sl * La: sl * La + self.keep_a[g]].clone()
            base = B * La + sl * T * Lv
            v_keep[int(perm_v[sl])] = [ids[base + t * Lv: base + t * Lv + self.keep_v[g]].clone() for t in range(T)]
        return ContrastivePlan(a_group, v_group, a_keep, v_keep)

    def forward(self, audio, imgs, plan, weight=1.0, xf=(None, None)):
        """-> (weight * nce [1] device tensor, c_acc [1] device tensor); leaves everything backward needs in place.
        plan: a ContrastivePlan to inject, or None when draw_device() already filled the index arrays.
        xf: (audio, frames) input transforms when the inputs are raw (ops.InputXf), else None."""
        cfg, st = self.cfg, self.stack
        if self.pool is not None:
            self.pool.owner = self             # (whose activations the shared memory holds: checked by backward)
        if plan is not None:
            self._set_plan(plan)
        x0 = st.x[0]
        self.emb_a.forward(audio, x0[:self.rows_a], xf[0])
        self.emb_v.forward(_fold_frames(imgs, cfg.frames), x0[self.rows_a:], xf[1])
        st.forward()
        _ln_fwd(st.out, self.final, self.yf, self.fstat[0], self.fstat[1], self.rows, LN_EPS_FINAL, st.row_mod)
        B, W, D = self.B, self.world, cfg.embed_dim
        ops.segment_mean_fwd(self.yf, self.seg_start, self.reps, 2 * B, row_map=self.slot_maps[0], max_row=2 * B)   # slot -> sample order
        if self.dp:
            self.comm.all_gather(self.all_reps.view(W * 2 * B, D), self.reps)             # c2: one [2,B,D] message per rank (RCCL)
        if W > 1:
            self.A.copy_(self.all_reps[:, :B].reshape(W * B, D))
            self.V.copy_(self.all_reps[:, B:].reshape(W * B, D))
        N = self.N
        ops.l2norm_fwd(self.A, self.An, self.na)
        ops.l2norm_fwd(self.V, self.Vn, self.nv)
        ops.gemm_f32_small(self.An, self.Vn, self.total, N, N, D, (D, 1), (1, D), 1.0 / cfg.temperature)
        ops.infonce_fwd(self.total, self.nstats, self.nout, weight)
        return self.nout[2:3], self.nout[1:2]

    def backward(self, gout, weight, reducer=None, accumulate=False):
        """gout: [1] fp32 device tensor (d loss / d loss_c_weighted); weight = contrast_loss_weight.
        accumulate: the gradient arena already holds the other pass's contribution (Stack.backward)."""
        cfg, st = self.cfg, self.stack
        if self.pool is not None and self.pool.owner is not self:
            raise RuntimeError("shared activation pool: another pass ran its forward since this one's - its activations are gone")
        B, W, D, N = self.B, self.world, cfg.embed_dim, self.N
        ops.infonce_dlogits(self.total, self.nstats, gout, weight, self.dtotal)
        ops.gemm_f32_small(self.dtotal, self.Vn, self.dAn, N, D, N, (N, 1), (D, 1), 1.0 / cfg.temperature)
        ops.gemm_f32_small(self.dtotal, self.An, self.dVn, N, D, N, (1, N), (D, 1), 1.0 / cfg.temperature)
        ops.l2norm_bwd(self.dAn, self.An, self.na, self.dA)
        ops.l2norm_bwd(self.dVn, self.Vn, self.nv, self.dV)
        # GatherLayer.backward all-reduces W identical copies and keeps the own slice (gather_layer.py:35-37):
        # that is W x the own-slice gradient, no collective needed.  The slot's row of this rank's slice of
        # [dA | dV] comes through the row map.
        ops.segment_mean_bwd(self.dAV, self.seg_start, self.yf, 2 * B, float(W), row_map=self.slot_maps[1], max_row=2 * N)
        _ln_bwd(self.yf, st.out, self.fstat[0], self.fstat[1], self.final, _dx_in(st), st.lnws, self.rows, st.row_mod,
                dx_bf16=st.dxb[0], dcol=self.blocks[-1].fc2.gb)
        st.backward(last_fc2_bias_done=True, reducer=reducer, accumulate=accumulate)
        self.emb_a.backward(st.dx[0][:self.rows_a])
        self.emb_v.backward(st.dx[0][self.rows_a:])


# =====================================================================================================
class MaePass:
    """Pass 2 (forward_encoder + mm layers + forward_decoder + forward_mae_loss, cav_mae_base.py:441-504,597-638,
    663-683,694-707)."""

    def __init__(self, arena: ParamArena, cfg: AVSiamConfig, batch, dev, pool=None, opts=None):
        self.arena, self.cfg, self.B, self.dev = arena, cfg, batch, dev
        self.pool = pool
        self.opts = opts = opts if opts is not None else EngineOptions.from_env()
        if pool is not None:
            pool.rewind()
        B, T, D, Dd = batch, cfg.frames, cfg.embed_dim, cfg.dec_dim
        ka, kv, La, Lv = cfg.keep_a, cfg.keep_v, cfg.audio_tokens, cfg.video_tokens
        self.rows_a, self.rows_v = B * ka, B * T * kv
        self.n_enc = ka + T * kv
        self.Ltot = La + T * Lv
        hid = D * cfg.mlp_ratio
        # The audio tower (ast_base blocks, plain norms) and the visual tower (vit_base blocks, '_v' norms) are independent and
        # structurally identical: when the audio rows end on a 256-row tile boundary they run as ONE packed stack whose GEMMs
        # take both weight sets per launch (8 192 audio rows alone fill 37 % of the chip with 256^2 tiles).  Otherwise two stacks.
        self.grouped = self.rows_a % 256 == 0 and opts.group_towers               # (EngineOptions.group_towers False: A/B measurements)
        self.blk_a = [BlockParams(arena, f"ast_base.blocks.{i}", "") for i in range(cfg.depth)]      # :489
        self.blk_v = [BlockParams(arena, f"vit_base.blocks.{i}", "_v") for i in range(cfg.depth)]   # :487
        self.blk_mm = [BlockParams(arena, "mm_layer_1", "_a"), BlockParams(arena, "mm_layer_2", "_a")]   # :699-700
        self.blk_dec = [BlockParams(arena, f"decoder_blocks.{i}", "") for i in range(cfg.dec_depth)]
        self.st_t = self.st_a = self.st_v = None
        if self.grouped:
            row_mod = torch.cat([torch.zeros(self.rows_a, dtype=U8), torch.ones(self.rows_v, dtype=U8)]).to(dev)
            self.st_t = make_stack(dev, self.rows_a + self.rows_v, D, cfg.num_heads, hid, [ka] * B + [kv] * (B * T), self.blk_a, row_mod,
                                   blocks2=self.blk_v, split=self.rows_a, pool=pool, opts=opts)
            self.tower_stacks, on_a, on_v = [self.st_t], (self.st_t, 0, self.rows_a), (self.st_t, self.rows_a, None)
        else:
            self.st_a = make_stack(dev, self.rows_a, D, cfg.num_heads, hid, [ka] * B, self.blk_a, pool=pool, opts=opts)
            self.st_v = make_stack(dev, self.rows_v, D, cfg.num_heads, hid, [kv] * (B * T), self.blk_v, pool=pool, opts=opts)
            self.tower_stacks, on_a, on_v = [self.st_a, self.st_v], (self.st_a, 0, None), (self.st_v, 0, None)
        self.st_mm = make_stack(dev, B * self.n_enc, D, cfg.num_heads, hid, [self.n_enc] * B, self.blk_mm, pool=pool, opts=opts)
        # EngineOptions.prune_dead: the decoder's rows are laid out [scored tokens (mask 1) | kept tokens] per sample and the last decoder block, decoder_norm,
        # the prediction heads and the loss run on the scored rows only (Stack q_rows; exact: unscored rows have zero loss and zero gradient, :679-682)
        self.ma, self.mv = La - ka, Lv - kv                                       # scored (masked) tokens per audio sequence / frame
        self.lq = self.ma + T * self.mv
        self.st_dec = make_stack(dev, B * self.Ltot, Dd, cfg.dec_heads, Dd * cfg.mlp_ratio, [self.Ltot] * B, self.blk_dec, pool=pool, opts=opts,
                            q_rows=self.lq if opts.prune_dead else 0)
        self.prune = self.st_dec.lq > 0
        self.fin_a, self.fin_v = [Norm(arena, "ast_base.norm_a")], [Norm(arena, "vit_base.norm")]   # :495,492
        self.dec_norm = [Norm(arena, "decoder_norm")]
        rows_e = self.rows_a + self.rows_v
        self.row_src_all, self.row_tok_all = _z((rows_e,), I32, dev), _z((rows_e,), I32, dev)
        self.emb_a = PatchEmbedder(arena, dev, self.rows_a, True, cfg, self.row_src_all[:self.rows_a], self.row_tok_all[:self.rows_a])
        self.emb_v = PatchEmbedder(arena, dev, self.rows_v, False, cfg, self.row_src_all[self.rows_a:], self.row_tok_all[self.rows_a:])
        self.dec_embed = Linear(arena, "decoder_embed.weight", "decoder_embed.bias")
        self.pred_a = Linear(arena, "decoder_pred_a.weight", "decoder_pred_a.bias")
        self.pred_v = Linear(arena, "decoder_pred_v.weight", "decoder_pred_v.bias")
        self.fstat_a = [_z((ops.pad_rows(self.rows_a, 128),), F32, dev) for _ in range(2)]
        self.fstat_v = [_z((ops.pad_rows(self.rows_v, 128),), F32, dev) for _ in range(2)]
        # static row maps: tower rows -> joint [B, n_enc] layout (torch.cat((ca, cv), dim=1), :503)
        b = torch.arange(B).view(B, 1)
        self.map_a = (b * self.n_enc + torch.arange(ka).view(1, ka)).reshape(-1).to(I32).to(dev)
        bt = torch.arange(B * T).view(B * T, 1)
        self.map_v = ((bt // T) * self.n_enc + ka + (bt % T) * kv + torch.arange(kv).view(1, kv)).reshape(-1).to(I32).to(dev)
        # the towers as (stack, its rows [lo, hi) of that stack's buffers - hi None: to their padded end -, final Norm, fstat pair, out map, rows,
        # embedder, blocks): both on the packed stack, or one stack each
        self.towers = [on_a + (self.fin_a, self.fstat_a, self.map_a, self.rows_a, self.emb_a, self.blk_a),
                       on_v + (self.fin_v, self.fstat_v, self.map_v, self.rows_v, self.emb_v, self.blk_v)]
        rj = self.st_mm.rp
        self.xj_b = _z((rj, D), BF16, dev)                    # bf16 copy of the mm output (decoder_embed operand)
        self.de = _z((rj, Dd), F32, dev)                      # decoder_embed output
        self.dde = _z((rj, Dd), F32, dev)
        self.dde_b = _z((rj, Dd), BF16, dev)
        # un-shuffle index arrays (src_row depends on the plan; pos/modality are static in the position-ordered layout)
        rows_d = B * self.Ltot
        self.src_row = _z((rows_d,), I32, dev)
        P = cfg.patch * cfg.patch
        ma, mv, lq = self.ma, self.mv, self.lq
        if not self.prune:
            pos = torch.cat([torch.arange(La), La + torch.arange(Lv).repeat(T)]).repeat(B)
            self.pos_row = pos.to(I32).to(dev)
            self.dmod = torch.cat([torch.zeros(La, dtype=U8), torch.ones(T * Lv, dtype=U8)]).repeat(B).to(dev)
            # decoder_norm output, modality-major: [B*La audio rows | pad | B*T*Lv video rows | pad]
            self.na_rows, self.nv_rows = B * La, B * T * Lv
            self.dn_rows_in = rows_d
            l = torch.arange(self.Ltot).view(1, -1)
            bb = torch.arange(B).view(B, 1)
            self.v_off = ops.pad_rows(self.na_rows, 128)
            omap = torch.where(l < La, bb * La + l, self.v_off + bb * (T * Lv) + (l - La))
            self.row_of_pos = self.pred_id = None
        else:
            # grouped layout of a sample's Ltot decoder rows: [scored audio (ma) | scored frame 0 .. T-1 (mv each) | kept audio (ka) | kept frames (kv each)];
            # WHICH token sits in a row comes from the plan (pos_row / row_of_pos / pred_id: csrc/maskplan.hip), the modality of a row is static
            self.pos_row = _z((rows_d,), I32, dev)
            self.row_of_pos = _z((rows_d,), I32, dev)
            self.pred_id = _z((B * ma + B * T * mv,), I32, dev)
            self.dmod = torch.cat([torch.zeros(ma, dtype=U8), torch.ones(T * mv, dtype=U8), torch.zeros(ka, dtype=U8), torch.ones(T * kv, dtype=U8)]).repeat(B).to(dev)
            # decoder_norm runs on the COMPACT rows the last block leaves (sample b: rows b * lq ..) -> modality-major compact predictions
            self.na_rows, self.nv_rows = B * ma, B * T * mv
            self.dn_rows_in = B * lq
            j = torch.arange(lq).view(1, -1)
            bb = torch.arange(B).view(B, 1)
            self.v_off = ops.pad_rows(self.na_rows, 128)
            omap = torch.where(j < ma, bb * ma + j, self.v_off + bb * (T * mv) + (j - ma))
        self.dn_map = omap.reshape(-1).to(I32).to(dev)
        dn_rows = self.v_off + ops.pad_rows(self.nv_rows, 128)
        self.dn = _z((dn_rows, Dd), BF16, dev)
        self.ddn = _z((dn_rows, Dd), BF16, dev)
        self.dn_stat = [_z((self.st_dec.rp,), F32, dev) for _ in range(2)]
        self.p_a = _z((ops.pad_rows(self.na_rows), P), F32, dev)
        self.p_v = _z((ops.pad_rows(self.nv_rows), P * cfg.in_chans), F32, dev)
        self.dp_a = _z((ops.pad_rows(self.na_rows), P), BF16, dev)
        self.dp_v = _z((ops.pad_rows(self.nv_rows), P * cfg.in_chans), BF16, dev)
        self.mask_all = _z((B * La + B * T * Lv,), F32, dev)       # [mask_a | mask_v], filled by the plan kernel
        self.mask_a = self.mask_all[:B * La].view(B, La)
        self.mask_v = self.mask_all[B * La:].view(B, T * Lv)
        # device-side plan: every descriptor field is static for this pass (75 % unstructured on all sequences)
        nseq = B + B * T
        d = np.zeros((nseq, ops.PLAN_FIELDS), dtype=np.int32)
        Lt = self.Ltot
        for b in range(B):
            g = [b * Lt, b * Lt + lq, b * ma, 0] if self.prune else ops.PLAN_CLASSIC       # dec_m_off, dec_k_off, pred_off, pos_base (csrc/maskplan.hip)
            d[b] = [La, ka, b * ka, b, b * Lt, b * self.n_enc, 0, b * La, b * La, 0, 0, 0] + g
            for t in range(T):
                i = b * T + t
                # (pos_base La for every frame: the frames share ONE positional table, decoder_pos_embed_v - as `pos` of the classic layout above)
                g = [b * Lt + ma + t * mv, b * Lt + lq + ka + t * kv, B * ma + i * mv, La] if self.prune else ops.PLAN_CLASSIC
                d[B + i] = [Lv, kv, self.rows_a + i * kv, i, b * Lt + La + t * Lv, b * self.n_enc + ka + t * kv, 0,
                            B * La + i * Lv, B * La + i * Lv, 0, 0, 0] + g
        self.desc_host = d
        self.desc_dev = torch.from_numpy(d).to(dev)
        self.ids_dev = _z((B * La + B * T * Lv,), I32, dev)
        self.rl_a, self.rl_v = _z((self.na_rows,), F32, dev), _z((self.nv_rows,), F32, dev)
        self.pid_a, self.pid_v = (self.pred_id[:B * ma], self.pred_id[B * ma:]) if self.prune else (None, None)
        self.losses = _z((3,), F32, dev)                       # loss_a, loss_v, loss_mae
        self.nmask_a = float(B * (La - ka))
        self.nmask_v = float(B * T * (Lv - kv))
        # parameter views used by the un-shuffle
        a = arena
        self.tok = {k: a.view(k).reshape(-1) for k in ("mask_token", "decoder_pos_embed_a", "decoder_pos_embed_v",
                                                      "decoder_modality_a", "decoder_modality_v")}
        self.gtok = {k: a.gview(k).reshape(-1) for k in self.tok}

    def _set_plan(self, plan: MaePlan):
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        ka, kv, La, Lv = cfg.keep_a, cfg.keep_v, cfg.audio_tokens, cfg.video_tokens
        assert plan.batch == B and plan.ids_keep_a.shape == (B, ka) and plan.ids_keep_v.shape == (B, T, kv)
        self.emb_a.set_rows(torch.arange(B).repeat_interleave(ka).to(I32), plan.ids_keep_a.reshape(-1).to(I32))
        self.emb_v.set_rows(torch.arange(B * T).repeat_interleave(kv).to(I32), plan.ids_keep_v.reshape(-1).to(I32))
        ra, rv = plan.ids_restore_a, plan.ids_restore_v                                  # [B,La], [B,T,Lv]
        b = torch.arange(B).view(B, 1)
        src_a = torch.where(ra < ka, b * self.n_enc + ra, torch.full_like(ra, -1))
        t = torch.arange(T).view(1, T, 1)
        src_v = torch.where(rv < kv, b.view(B, 1, 1) * self.n_enc + ka + t * kv + rv, torch.full_like(rv, -1))
        src = torch.cat([src_a, src_v.reshape(B, T * Lv)], dim=1).reshape(-1).to(I32)            # indexed by POSITION (b, l)
        if self.prune:
            # the grouped decoder layout from an injected plan - what the plan kernel writes on the device (csrc/maskplan.hip): the rank of a token
            # in its sequence's shuffle decides its decoder row
            Lt, ma, mv, lq = self.Ltot, self.ma, self.mv, self.lq
            bL = b * Lt
            row_a = torch.where(ra < ka, bL + lq + ra, bL + (ra - ka))                                                        # [B, La]
            row_v = torch.where(rv < kv, bL.view(B, 1, 1) + lq + ka + t * kv + rv, bL.view(B, 1, 1) + ma + t * mv + (rv - kv))    # [B, T, Lv]
            rop = torch.cat([row_a, row_v.reshape(B, T * Lv)], dim=1).reshape(-1)                                             # position -> decoder row
            pos = torch.cat([torch.arange(La), La + torch.arange(Lv).repeat(T)]).repeat(B)      # which positional row a position takes (frames share one table)
            src_d = torch.empty_like(src)
            src_d[rop] = src
            pos_d = torch.empty(B * Lt, dtype=torch.int64)
            pos_d[rop] = pos
            pid = torch.empty(B * ma + B * T * mv, dtype=torch.int64)
            tok_a = torch.arange(La).view(1, La).expand(B, La)
            sel = ra >= ka
            pid[(b * ma + (ra - ka))[sel]] = (b * La + tok_a)[sel]
            it = (b.view(B, 1, 1) * T + t)                                                                                   # frame image index [B, T, 1]
            tok_v = torch.arange(Lv).view(1, 1, Lv).expand(B, T, Lv)
            selv = rv >= kv
            pid[(B * ma + it * mv + (rv - kv))[selv]] = (B * La + it * Lv + tok_v)[selv]
            self.src_row.copy_(src_d, non_blocking=True)
            self.pos_row.copy_(pos_d.to(I32), non_blocking=True)
            self.row_of_pos.copy_(rop.to(I32), non_blocking=True)
            self.pred_id.copy_(pid.to(I32), non_blocking=True)
        else:
            self.src_row.copy_(src, non_blocking=True)
        self.mask_a.copy_((ra >= ka).float(), non_blocking=True)                         # :385-388
        self.mask_v.copy_((rv >= kv).float().reshape(B, T * Lv), non_blocking=True)

    def draw_device(self, seed, nprng=None, seed_dev=None, host=True):
        """75 % unstructured masks of every audio / video sequence, drawn on the device (one launch; no host part)."""
        ops.mask_plan(self.desc_dev, self.desc_host, seed, self.row_src_all, self.row_tok_all, src_row=self.src_row,
                      mask_out=self.mask_all, ids_out=self.ids_dev, seed_dev=seed_dev,
                      grouped=(self.pos_row, self.row_of_pos, self.pred_id) if self.prune else None)

    def draw_host(self, nprng=None):
        pass

    def last_plan(self):
        """Rebuild the MaePlan the device drew (tests / debugging; synchronises)."""
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        La, Lv, ka, kv = cfg.audio_tokens, cfg.video_tokens, cfg.keep_a, cfg.keep_v
        ids = self.ids_dev.cpu().long()
        sa = ids[:B * La].view(B, La)
        sv = ids[B * La:].view(B, T, Lv)
        return MaePlan(sa[:, :ka].contiguous(), torch.argsort(sa, dim=1), sv[..., :kv].contiguous(), torch.argsort(sv, dim=-1))

    def forward(self, audio, imgs, plan, xf=(None, None)):
        """plan: a MaePlan to inject, or None when draw_device() already filled the index arrays.
        xf: (audio, frames) input transforms when the inputs are raw (ops.InputXf), else None."""
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        La, Lv = cfg.audio_tokens, cfg.video_tokens
        if self.pool is not None:
            self.pool.owner = self
        if plan is not None:
            self._set_plan(plan)
        self.audio, self.imgs, self.xf, self.imgs_shape = audio, _fold_frames(imgs, T), xf, tuple(imgs.shape)
        for st, lo, hi, fin, fstat, omap, rows, emb, blks in self.towers:
            emb.forward(audio if emb.audio else self.imgs, st.x[0][lo:hi], xf[0 if emb.audio else 1])
        for st in self.tower_stacks:
            st.forward()
        xj = self.st_mm.x[0]
        for st, lo, hi, fin, fstat, omap, rows, emb, blks in self.towers:
            _ln_fwd(st.out[lo:hi], fin, xj, fstat[0], fstat[1], rows, LN_EPS_FINAL, out_map=omap)
        self.st_mm.forward()
        rows_j = B * self.n_enc
        ops.cast_scale(self.st_mm.out, self.xj_b, rows_j * cfg.embed_dim, 1.0)
        ops.gemm_nt(self.xj_b, self.dec_embed.w, self.de, rows_j, bias=self.dec_embed.b)                  # :600
        rows_d = B * self.Ltot
        ops.unshuffle_fwd(self.de, self.src_row, self.pos_row, self.dmod, self.tok["mask_token"], self.tok["decoder_pos_embed_a"],
                          self.tok["decoder_pos_embed_v"], self.tok["decoder_modality_a"], self.tok["decoder_modality_v"],
                          self.st_dec.x[0], rows_d)
        self.st_dec.forward()
        # (prune: st_dec.out holds the scored rows only, compact; decoder_norm, the heads and the loss see nothing else)
        _ln_fwd(self.st_dec.out, self.dec_norm, self.dn, self.dn_stat[0], self.dn_stat[1], self.dn_rows_in, LN_EPS_BLOCK, out_map=self.dn_map)
        ops.gemm_nt(self.dn[:self.v_off], self.pred_a.w, self.p_a, self.na_rows, bias=self.pred_a.b)       # :634
        ops.gemm_nt(self.dn[self.v_off:], self.pred_v.w, self.p_v, self.nv_rows, bias=self.pred_v.b)       # :635
        ops.mae_loss_fwd(self.p_a, audio, self.mask_a.view(-1), self.rl_a, self.losses[0:1], True, La, self.nmask_a,
                         total=self.losses[2:3], total_init=True, xf=xf[0], stride=cfg.st, row_id=self.pid_a, id_base=0)
        ops.mae_loss_fwd(self.p_v, self.imgs, self.mask_v.view(-1), self.rl_v, self.losses[1:2], False, Lv, self.nmask_v,
                         total=self.losses[2:3], total_init=False, xf=xf[1], stride=cfg.st, row_id=self.pid_v, id_base=B * La)    # loss_mae = a + v (:707)
        return self.losses[2:3], self.losses[0:1], self.losses[1:2], self.mask_a, self.mask_v

    def predictions(self):
        """(pred_a [B, La, P], pred_v [B, T * Lv, P * C]) of the last forward, in the reference's layout (cav_mae_base.py:634-635).  With
        EngineOptions.prune_dead only the scored rows (mask 1) were computed: the others read NaN.  Tests / debugging (synchronises)."""
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        La, Lv = cfg.audio_tokens, cfg.video_tokens
        pa, pv = self.p_a[:self.na_rows].float().cpu(), self.p_v[:self.nv_rows].float().cpu()
        if not self.prune:
            return pa.view(B, La, -1), pv.view(B, T * Lv, -1)
        ida, idv = self.pid_a.cpu().long(), self.pid_v.cpu().long() - B * La
        fa = torch.full((B * La, pa.shape[1]), float("nan"))
        fv = torch.full((B * T * Lv, pv.shape[1]), float("nan"))
        fa[ida] = pa
        fv[idv] = pv
        return fa.view(B, La, -1), fv.view(B, T * Lv, -1)

    def reconstruct(self, paste_kept=True, raw=False):
        """The last forward's predictions as pictures (unpatchify, cav_mae_base.py:353-363; csrc/inpaint.hip), on the device, nothing copied to
        the host and no synchronisation: -> (audio [B, T, F], imgs in the shape forward() was given, err_a [B, La], err_v [B, T * Lv]).
        paste_kept: the kept patches (mask 0) and the cells no patch covers are the input as the model saw it, bit for bit; False: every patch
        is the decoder's prediction - every row must then have been predicted (EngineOptions.prune_dead off).  raw: in the units of the RAW
        inputs the forward was given (un-normalised fbank, uint8 frames: the inverse of their ops.InputXf); a modality that came in
        normalised stays as it is.  err_*: per-token mean squared error of the scored tokens (the loss kernel's row sums), 0 on kept ones."""
        cfg, B = self.cfg, self.B
        if getattr(self, "audio", None) is None:
            raise RuntimeError("MaePass.reconstruct: no forward has run")
        if self.pool is not None and self.pool.owner is not self:
            raise RuntimeError("shared activation pool: another pass ran its forward since this one's - its activations are gone")
        if not paste_kept and self.prune:
            raise ValueError("MaePass.reconstruct(paste_kept=False) needs every row predicted: with EngineOptions.prune_dead the decoder computes "
                             "the scored rows (mask 1) only - build the model with prune_dead=False")
        La, Lv = cfg.audio_tokens, cfg.video_tokens
        outs = []
        for pred, inp, mask, rl, audio, L, xf, pid, base in ((self.p_a, self.audio, self.mask_a, self.rl_a, True, La, self.xf[0], self.pid_a, 0),
                                                             (self.p_v, self.imgs, self.mask_v, self.rl_v, False, Lv, self.xf[1], self.pid_v, B * La)):
            want_raw = bool(raw) and xf is not None
            out, raw_out, err = ops.unpatchify(pred, inp, mask, audio, L, xf=xf, stride=cfg.st, row_id=pid, id_base=base, paste_kept=paste_kept,
                                               raw=want_raw, row_loss=rl, model_units=not want_raw)
            outs.append((raw_out if want_raw else out, err))
        return outs[0][0], outs[1][0].view(self.imgs_shape), outs[0][1], outs[1][1]

    def backward(self, gout, reducer=None, accumulate=False):
        cfg, B, T = self.cfg, self.B, self.cfg.frames
        if self.pool is not None and self.pool.owner is not self:
            raise RuntimeError("shared activation pool: another pass ran its forward since this one's - its activations are gone")
        La, Lv, D, Dd = cfg.audio_tokens, cfg.video_tokens, cfg.embed_dim, cfg.dec_dim
        ops.mae_loss_bwd(self.p_a, self.audio, self.mask_a.view(-1), gout, self.dp_a, True, La, self.nmask_a, xf=self.xf[0], stride=cfg.st,
                         row_id=self.pid_a, id_base=0)
        ops.mae_loss_bwd(self.p_v, self.imgs, self.mask_v.view(-1), gout, self.dp_v, False, Lv, self.nmask_v, xf=self.xf[1], stride=cfg.st,
                         row_id=self.pid_v, id_base=B * La)
        # prediction heads
        ops.gemm_nt(self.dp_a, self.pred_a.wt, self.ddn[:self.v_off], self.na_rows)
        ops.gemm_tn(self.dp_a, self.dn[:self.v_off], self.pred_a.gw, self.na_rows)
        ops.colsum(self.dp_a, self.pred_a.gb, self.na_rows)
        ops.gemm_nt(self.dp_v, self.pred_v.wt, self.ddn[self.v_off:], self.nv_rows)
        ops.gemm_tn(self.dp_v, self.dn[self.v_off:], self.pred_v.gw, self.nv_rows)
        ops.colsum(self.dp_v, self.pred_v.gb, self.nv_rows)
        sd = self.st_dec
        rows_d = B * self.Ltot
        _ln_bwd(self.ddn, sd.out, self.dn_stat[0], self.dn_stat[1], self.dec_norm, _dx_in(sd), sd.lnws, self.dn_rows_in,
                out_map=self.dn_map, dx_bf16=sd.dxb[0], dcol=self.blk_dec[-1].fc2.gb)
        sd.backward(last_fc2_bias_done=True, reducer=reducer, accumulate=accumulate)
        g = self.gtok
        ops.unshuffle_bwd(sd.dx[0], self.src_row, B, T, La, Lv, self.dde, g["decoder_pos_embed_a"], g["decoder_pos_embed_v"],
                          g["mask_token"], g["decoder_modality_a"], g["decoder_modality_v"], row_of_pos=self.row_of_pos)
        rows_j = B * self.n_enc
        ops.cast_scale(self.dde, self.dde_b, rows_j * Dd, 1.0)
        sm = self.st_mm
        if self.opts.grad_stream == "bf16":                       # the joint layers' backward starts from the bf16 gradient alone
            ops.gemm_nt(self.dde_b, self.dec_embed.wt, sm.dxb[0], rows_j)
        else:
            ops.gemm_nt(self.dde_b, self.dec_embed.wt, sm.dx[0], rows_j)
            ops.cast_scale(sm.dx[0], sm.dxb[0], rows_j * D, 1.0)
        ops.gemm_tn(self.dde_b, self.xj_b, self.dec_embed.gw, rows_j)
        ops.colsum(self.dde_b, self.dec_embed.gb, rows_j)
        sm.backward(reducer=reducer, accumulate=accumulate)
        for st in self.tower_stacks:
            mine = [t for t in self.towers if t[0] is st]
            for st_, lo, hi, fin, fstat, omap, rows, emb, blks in mine:
                _ln_bwd(sm.dx[0], st.out[lo:], fstat[0], fstat[1], fin, _dx_in(st, lo), st.lnws, rows, out_map=omap, dx_bf16=st.dxb[0][lo:],
                        dcol=blks[-1].fc2.gb)
            st.backward(last_fc2_bias_done=True, reducer=reducer, accumulate=accumulate)
            for st_, lo, hi, fin, fstat, omap, rows, emb, blks in mine:
                emb.backward(st.dx[0][lo:hi])
