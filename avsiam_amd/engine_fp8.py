"""The fp8 modes of the packed transformer stack (EngineOptions.fp8 = "1" | "2" | "3"; BASELINE configs[4]'s "fp8 MFMA path", never the default):
Fp8Stack runs engine.Stack's schedule with 8-bit GEMM operands by overriding its hooks.  engine.make_stack() builds one where
engine.fp8_applies() - the mode is on and the stack's widths meet the fp8 GEMM's tile constraints.

Mode 1 (AVSIAM_FP8=1 / bench.py --fp8): the four forward GEMMs of a block (qkv, proj, fc1, fc2) take OCP e4m3 operands with per-tensor DELAYED
scaling and accumulate in fp32.  Every quantised tensor has a device record {scale, 1/scale, running amax, saturation events} (ops.Fp8Records):
the kernel that produces an operand (the LayerNorm in front of qkv / fc1, the attention epilogue in front of proj, fc1's GELU epilogue in front of
fc2, a quantising pass for the weights) reads the scale from the record and folds the |max| it saw into it; once per forward one tiny kernel turns
the amax history (16 steps) into the next scales, 448 / (2 * max) - no host synchronisation anywhere, saturation is counted, the state is saved
with the checkpoint (CAVMAE_BASE.fp8_state).  The first time a GEMM runs its operands are calibrated on the spot (absmax -> scale, still on the
device) and the activation is quantised by a pass.  The MAE pass's two towers run as one stack with two weight sets here too.  Everything the
backward reads is still produced in bf16.

Mode 2 (bench.py --fp8 --fp8-dgrad) extends the mode into the backward: ALL FOUR input-gradient GEMMs of a block - fc2 (with its GELU' epilogue),
fc1, proj and qkv - run on e5m2 gradient operands, written, beside the bf16 gradient the weight-gradient GEMMs and LayerNorm still read, by the
kernels that produce them: the LayerNorm backward (residual gradient), the fc2 input-gradient epilogue and the three attention backward kernels
(dqkv; avs_attn_bwd_q8 / avs_attn_bwd_fused_q8); own records, fmax 57344 - against the e4m3 copy of the transposed weight (the forward's weight
scale).  The weight gradients stay bf16.  gelu'(x) travels from fc1 to the fc2 input-gradient epilogue as 8-bit fixed-point codes (a uint8
`out` / `aux` of ops.gemm_nt_fp8): half the bytes of the two epilogues that write and read it (EngineOptions.fp8_gelu8 False: A/B).

Mode 3 (bench.py --fp8 --fp8-wgrad): the four weight gradients of a block on fp8 operands too (ops.gemm_tn_fp8_group: e5m2 gradient copies x e4m3
activation copies).  The e4m3 copy of an activation is then KEPT per block (one more byte per element beside the bf16 copy the attention /
LayerNorm backward still read) instead of living in one buffer per stack.  Four bf16 tensors of a block then have no reader left once their
consumers' records are calibrated: the two LayerNorm outputs and gelu(x) (read by qkv / fc1 / fc2 and their weight gradients - all in e4m3) and
the fc2 input gradient (read by fc1's input- and weight-gradient GEMMs in e5m2; fc1's bias gradient is the fused column sum).
EngineOptions.fp8_lean (default on): their producers write the 8-bit copy ONLY (NULL bf16 output) and the three activations live in one shared
buffer per stack instead of one per block - 2 x D + hidden fewer bf16 values written and kept per token and block, and the GEMM epilogues that
wrote them (bound by the write burst of all CUs at once) shrink to 3/5 (fc1) and 1/3 (fc2 input gradient) of their bytes.  Off: A/B.
"""
import torch

from . import ops
from .engine import LN_EPS_BLOCK, U8, Stack, _ln_fwd, fp8_applies

_GEMM = {"qkv": 0, "proj": 1, "fc1": 2, "fc2": 3}            # a block's GEMMs: three records each (activation, weight, second weight set)
_GRAD = {"dbo": 0, "dfc1": 1, "dbm": 2, "dqkv": 3}           # a block's e5m2 gradient operands: one record each
_GRAD_OF = {"fc2": "dbo", "fc1": "dfc1", "proj": "dbm", "qkv": "dqkv"}      # Linear -> the operand of its input- and weight-gradient GEMMs


class Fp8Stack(Stack):
    """engine.Stack on 8-bit GEMM operands (module docstring).  fp8_bwd / fp8_wgrad / fp8_lean: modes 2 - 3 / mode 3 / mode 3's 8-bit-only outputs.
    The records, the calibrated sets and the frozen weight tables (w8_batch, wt8_batch) belong to the blocks the stack is built with."""

    fp8 = True

    def __init__(self, dev, rows, D, H, hidden, seq_lens, blocks, row_mod=None, *, blocks2=None, split=0, inference=False, pool=None, opts=None, q_rows=0):
        """arguments: Stack.__init__ (q_rows: the pruned last block is a bf16 form - not applied here)"""
        assert opts is not None and fp8_applies(opts, D, hidden)
        self.fp8_bwd = opts.fp8 in ("2", "3") and not inference
        self.fp8_wgrad = self.fp8_bwd and opts.fp8 == "3"
        self.fp8_lean = self.fp8_wgrad and opts.fp8_lean
        super().__init__(dev, rows, D, H, hidden, seq_lens, blocks, row_mod, blocks2=blocks2, split=split, inference=inference, pool=pool, opts=opts, q_rows=0)

    # ---- constructor hooks
    def _alloc_operand_copies(self, z, dev):
        rows, D, hidden, nblocks = self.rows, self.D, self.hidden, self.nblocks
        r8 = ops.pad_rows(rows, 256)
        self.a8 = z((r8, max(D, hidden)), U8, dev)       # calibration step only: an activation quantised by a pass
        # persistent e4m3 copies of the stack's weights (two sets: the MAE pass's second tower), re-quantised with the step's scales by
        # ONE batched launch per forward once every GEMM is calibrated (ops.Fp8Batch); per block: qkv | proj | fc1 | fc2
        per_blk = 4 * D * D + 2 * D * hidden
        self.w8_flat = torch.zeros((2 * nblocks * per_blk,), dtype=U8, device=dev)
        self.w8_off = {"qkv": 0, "proj": 3 * D * D, "fc1": 4 * D * D, "fc2": 4 * D * D + D * hidden}
        self.w8_per_blk = per_blk
        self.w8_batch = None                                                   # built after the calibration forward

        def blocks8(cols, shared=None):     # per block when the weight gradients read them (recomputed blocks share one, like their bf16 copies)
            if not self.fp8_wgrad:
                one = shared if shared is not None else z((r8, cols), U8, dev)
                return [one] * nblocks
            one = z((r8, cols), U8, dev) if self.nrecomp else None
            return [one if i < self.nrecomp else z((r8, cols), U8, dev) for i in range(nblocks)]
        self.ln1_8 = blocks8(D)                                                # e4m3 copy a LayerNorm writes for qkv ...
        self.ln2_8 = blocks8(D, None if self.fp8_wgrad else self.ln1_8[0])     # ... and for fc1 (one buffer serves both unless they are kept)
        self.att8 = blocks8(D)                                                 # ... the attention epilogue for proj
        self.act8 = blocks8(hidden)                                            # ... and fc1's GELU epilogue for fc2
        self.f8 = ops.Fp8Records(nblocks * 12, dev)                            # per block: 4 GEMMs x (activation, weight, second weight set)
        self.f8_seen = set()                                                   # (block, gemm) whose records hold a calibrated scale
        if not self.fp8_bwd:
            return
        self.g8 = ops.Fp8Records(nblocks * 4, dev, fmax=ops.BF8_MAX)           # per block: the e5m2 operands dbo (fc2), dfc1 (fc1), dbm (proj), dqkv (qkv)
        self.g8_seen, self.g8_have = set(), set()        # (block, operand) calibrated / whose e5m2 copy a producer has written in this backward
        self.dx8 = [z((r8, D), U8, dev) for _ in range(2)]      # e5m2 copies of dbo / dbm
        self.dfc1_8 = z((r8, hidden), U8, dev)
        self.dqkv8 = z((r8, 3 * D), U8, dev)             # e5m2 copy of dqkv, written by the attention backward kernels
        self._grad8 = {"dbo": self.dx8[0], "dbm": self.dx8[1], "dfc1": self.dfc1_8, "dqkv": self.dqkv8}
        self._x8 = {"fc2": self.act8, "fc1": self.ln2_8, "proj": self.att8, "qkv": self.ln1_8}      # the e4m3 copy of a Linear's input, per block
        # transposed copies the fp8 input-gradient GEMMs read: fc2 | fc1 | proj | qkv
        self.wt8_flat = torch.zeros((2 * nblocks * per_blk,), dtype=U8, device=dev)
        self.wt8_off = {"fc2": 0, "fc1": D * hidden, "proj": 2 * D * hidden, "qkv": 2 * D * hidden + D * D}
        self.wt8_per_blk = per_blk
        self.wt8_batch, self._wt8_pending = None, []     # the batched launch, and its table as the first backward collects it

    def _fused224(self):
        return super()._fused224() and not self.fp8_bwd          # (that kernel does not write the e5m2 copy of dqkv)

    def _buffer_policy(self):
        # lean: a bf16 operand only the calibration step still writes; the gelu'(x) codes belong to the fp8 backward (EngineOptions.fp8_gelu8)
        return self.fp8_lean, bool(self.fp8_bwd and self.opts.fp8_gelu8)

    # ---- records and persistent weight copies
    def _rec(self, i, name, operand=0):
        return self.f8.rec((i * 4 + _GEMM[name]) * 3 + operand)

    def _w8(self, i, name, which=0):
        """persistent e4m3 copy [N, K] of block i's weight `name` (which: weight set 0 / 1)"""
        D, Hd = self.D, self.hidden
        N, K = {"qkv": (3 * D, D), "proj": (D, D), "fc1": (Hd, D), "fc2": (D, Hd)}[name]
        o = (which * self.nblocks + i) * self.w8_per_blk + self.w8_off[name]
        return self.w8_flat[o:o + N * K].view(N, K)

    def _wt8(self, i, name, which=0):
        """persistent e4m3 copy of the TRANSPOSED weight (B operand [K_in, N_out] of the input-gradient GEMM)"""
        D, Hd = self.D, self.hidden
        N, K = {"fc2": (Hd, D), "fc1": (D, Hd), "proj": (D, D), "qkv": (D, 3 * D)}[name]
        o = (which * self.nblocks + i) * self.wt8_per_blk + self.wt8_off[name]
        return self.wt8_flat[o:o + N * K].view(N, K)

    def fp8_state(self):
        """delayed-scaling state for the checkpoint"""
        st = {**self.f8.state(), "seen": sorted(self.f8_seen)}
        if self.fp8_bwd:
            st["grad"] = {**self.g8.state(), "seen": sorted(self.g8_seen)}
        return st

    def load_fp8_state(self, st):
        if st is not None:
            self.f8.load(st)
            self.f8_seen = {tuple(k) for k in st["seen"]}
            if self.fp8_bwd and "grad" in st:
                self.g8.load(st["grad"])
                self.g8_seen = {tuple(k) for k in st["grad"]["seen"]}

    # ---- forward
    def _forward_begin(self):
        self.f8.update()                   # delayed scaling: last forward's amax -> history -> this forward's scales (one launch)
        if self.w8_batch is None and len(self.f8_seen) == 4 * self.nblocks:      # every GEMM calibrated: freeze the weight table
            self.w8_batch = ops.Fp8Batch(self.f8)
            for i, bp in enumerate(self.blocks):
                for name in ("qkv", "proj", "fc1", "fc2"):
                    for st_, bl in enumerate((bp,) if self.blocks2 is None else (bp, self.blocks2[i])):
                        self.w8_batch.add(getattr(bl, name).w, self._w8(i, name, st_), (i * 4 + _GEMM[name]) * 3 + 1 + st_)
            self.w8_batch.build(self.x[0].device)
        if self.w8_batch is not None:
            self.w8_batch.run()            # all weights of the stack -> e4m3 with this step's scales (one launch)

    def _block_forward(self, i, last_gemm=True):
        """The block's forward with e4m3 GEMM operands.  Once a GEMM's records are calibrated its activation arrives in e4m3 from the kernel
        that produces it; before that (first use) it is quantised by a pass."""
        M = self.rows
        bp, b2 = self.blocks[i], self.blocks2[i] if self.blocks2 is not None else None
        x, st = self.x[i], self.stats[i]
        n1 = bp.n1 if b2 is None else [bp.n1[0], b2.n1[0]]
        n2 = bp.n2 if b2 is None else [bp.n2[0], b2.n2[0]]
        seen = lambda name: (i, name) in self.f8_seen
        r = lambda name: self._rec(i, name)
        l1, l2, at8, ac8 = self.ln1_8[i], self.ln2_8[i], self.att8[i], self.act8[i]
        lean = self.fp8_lean               # a calibrated consumer reads the e4m3 copy only, and so does its weight gradient: no bf16 output
        _ln_fwd(x, n1, None if lean and seen("qkv") else self.ln1[i], st[0], st[1], M, LN_EPS_BLOCK, self.row_mod, y8=l1 if seen("qkv") else None,
                q8_dev=r("qkv") if seen("qkv") else None)
        self._gemm_fp8(i, "qkv", self.ln1[i], l1, bp.qkv, b2.qkv if b2 else None, self.qkv[i], scale_cols=self.D, col_scale=self.q_scale)
        ops.attn_fwd(self.qkv[i], self.tiles, self.H, self.att[i], self.lse[i], **({"out8": at8, "q8": r("proj")} if seen("proj") else {}))
        self._gemm_fp8(i, "proj", self.att[i], at8, bp.proj, b2.proj if b2 else None, self.xmid[i], res=x)
        _ln_fwd(self.xmid[i], n2, None if lean and seen("fc1") else self.ln2[i], st[2], st[3], M, LN_EPS_BLOCK, self.row_mod, y8=l2 if seen("fc1") else None,
                q8_dev=r("fc1") if seen("fc1") else None)
        # (the fc2 weight gradient reads the e4m3 copy of gelu(x) too: with fp8 weight gradients it is written even when fc2 itself is skipped)
        o8 = {"out8": ac8, "q8": r("fc2")} if (seen("fc2") and (last_gemm or self.fp8_wgrad)) else {}
        self._gemm_fp8(i, "fc1", self.ln2[i], l2, bp.fc1, b2.fc1 if b2 else None, self.fc1[i], out2=None if lean and o8 else self.act[i], act=1, **o8)
        if last_gemm:
            self._gemm_fp8(i, "fc2", self.act[i], ac8, bp.fc2, b2.fc2 if b2 else None, self.x[i + 1], res=self.xmid[i])
        elif self.fp8_wgrad and not seen("fc2"):
            raise RuntimeError("fp8 weight gradients: a recomputed block met an uncalibrated fc2 record")

    def _gemm_fp8(self, i, name, A, a8, lin, lin2, out, **kw):
        """One forward GEMM on e4m3 operands.  a8: where this GEMM's activation lives in e4m3 once its producer writes it."""
        M = self.rows
        W, W2 = lin.w, (lin2.w if lin2 is not None else None)
        N, K = W.shape
        ra, rw, rw2 = self._rec(i, name, 0), self._rec(i, name, 1), self._rec(i, name, 2)
        first = (i, name) not in self.f8_seen
        if first:                                  # calibrate on the spot, on the device: amax -> record -> scale (no host sync)
            ops.absmax_into(A, ra)
            ops.absmax_into(W, rw)
            if W2 is not None:
                ops.absmax_into(W2, rw2)
            self.f8.update(first=(i * 4 + _GEMM[name]) * 3, count=3)
            self.f8_seen.add((i, name))
            if self.fp8_wgrad:                     # the block's own e4m3 copy: the weight gradient of this step reads it
                a8 = a8[:A.shape[0]]
            else:
                a8 = self.a8[:A.shape[0], :K] if self.a8.shape[1] == K else self.a8.view(-1)[:A.shape[0] * K].view(A.shape[0], K)
            ops.quantize_fp8(A, 1.0, out=a8, q=ra)
        w8 = self._w8(i, name, 0)
        w8b = self._w8(i, name, 1) if W2 is not None else None
        if self.w8_batch is None:                  # until the table exists (calibration forward): one quantising pass per weight
            ops.quantize_fp8(W, 1.0, out=w8, q=rw)
            if W2 is not None:
                ops.quantize_fp8(W2, 1.0, out=w8b, q=rw2)
        dual = (self.split, w8b, lin2.b, rw2) if W2 is not None else None
        ops.gemm_nt_fp8(a8, w8, out, M, bias=lin.b, qa=ra, qw=rw, dual=dual, **kw)

    # ---- backward (modes 2 / 3; mode 1 keeps the bf16 backward)
    def _backward_begin(self, c):
        if not self.fp8_bwd:
            return
        self.g8.update()                   # delayed scaling of the gradient operands: last backward's amax -> this backward's scales
        self.g8_have = set()
        if self.wt8_batch is None and len(self._wt8_pending) == 4 * self.nblocks * len(self.ranges):
            self.wt8_batch = ops.Fp8Batch(self.f8)      # the transposed copies use the forward's weight records (the same tensors)
            for src, dst, ridx in self._wt8_pending:
                self.wt8_batch.add(src, dst, ridx)
            self.wt8_batch.build(self.dx[0].device)
        if self.wt8_batch is not None:
            self.wt8_batch.run()

    def _grad_copy(self, blk, name):
        """(e5m2 buffer, record) of a gradient operand its producer is to write in this backward - once calibrated, else (None, None)"""
        if not self.fp8_bwd or blk < 0 or (blk, name) not in self.g8_seen:
            return None, None
        self.g8_have.add((blk, name))
        return self._grad8[name], self.g8.rec(blk * 4 + _GRAD[name])

    def _ln_bwd_copy(self, blk, name, lo):
        d8, q8 = self._grad_copy(blk, name)
        return {"dx8": d8[lo:], "q8": q8} if d8 is not None else {}

    def _attn_bwd_copy(self, i):
        # (lean: the qkv input- and weight-gradient GEMMs read the e5m2 copy; of the bf16 dqkv only the query third has a reader)
        d8, q8 = self._grad_copy(i, "dqkv")
        return {"dqkv8": d8, "q8": q8, "kv_bf16": not self.fp8_lean} if d8 is not None else {}

    def _dgrad(self, c, i, name, dy, out, M):
        if not self.fp8_bwd:
            return super()._dgrad(c, i, name, dy, out, M)
        bp, b2 = self.blocks[i], self.blocks2[i] if self.blocks2 is not None else None
        kw = {}
        if name == "fc2":                  # GELU' epilogue; the fc1 bias gradient as its column sum (deterministic mode: by the column-sum kernel)
            kw = {"act": 2, "aux": self.fc1[i], "colsum": None if c.det else bp.fc1.gb, "colsum2": None if c.det or b2 is None else b2.fc1.gb}
            o8, q8 = self._grad_copy(i, "dfc1")
            if o8 is not None:
                kw.update(out8=o8, q8=q8)
                if self.fp8_lean and not c.det:        # once this epilogue writes the e5m2 copy nothing reads the bf16 gradient: no bf16 output
                    out = None                         # (deterministic mode keeps it: the column-sum kernel reads it)
        gname = _GRAD_OF[name]
        self._dgrad_fp8(i, gname, name, dy, self._grad8[gname], getattr(bp, name), getattr(b2, name) if b2 is not None else None, out, **kw)

    def _dgrad_fp8(self, i, gname, wname, A, a8, lin, lin2, out, colsum2=None, **kw):
        """One input-gradient GEMM on an e5m2 gradient operand (A: its bf16 form, a8: where its e5m2 copy lives - written by the
        producer when (i, gname) is in g8_have, else by a pass here) and the e4m3 copy of the transposed weight, quantised with the
        scale of the forward's weight record (the same tensor)."""
        M = self.rows
        idx = i * 4 + _GRAD[gname]
        rec = self.g8.rec(idx)
        if (i, gname) not in self.g8_seen:            # first use: calibrate on the device
            ops.absmax_into(A, rec)
            self.g8.update(first=idx, count=1)
            self.g8_seen.add((i, gname))
        if (i, gname) not in self.g8_have:
            ops.quantize_fp8(A, 1.0, out=a8[:A.shape[0]], q=rec, e5m2=True)
        rw, rw2 = self._rec(i, wname, 1), self._rec(i, wname, 2)
        w8 = self._wt8(i, wname, 0)
        w8b = self._wt8(i, wname, 1) if lin2 is not None else None
        if self.wt8_batch is None:                 # first backward: per-weight passes, and the table for the batched launch is collected
            base = (i * 4 + _GEMM[wname]) * 3
            ops.quantize_fp8(lin.wt, 1.0, out=w8, q=rw)
            self._wt8_pending.append((lin.wt, w8, base + 1))
            if lin2 is not None:
                ops.quantize_fp8(lin2.wt, 1.0, out=w8b, q=rw2)
                self._wt8_pending.append((lin2.wt, w8b, base + 2))
        dual = (self.split, w8b, None, rw2, colsum2) if lin2 is not None else None
        ops.gemm_nt_fp8(a8, w8, out, M, qa=rec, qw=rw, grad=True, dual=dual, **kw)

    def _wgrad(self, blk, jobs, bl, lo, hi):
        if not self.fp8_wgrad:
            return super()._wgrad(blk, jobs, bl, lo, hi)
        # mode 3: the e5m2 copy of the gradient (written by its producer or by the input-gradient GEMM's quantising pass just before) x the
        # block's e4m3 copy of the layer input, with the two operands' device records
        jobs8 = []
        for a, b, name in jobs:
            gname = _GRAD_OF[name]
            assert (blk, gname) in self.g8_seen and (blk, name) in self.f8_seen
            jobs8.append((self._grad8[gname][lo:], self._x8[name][blk][lo:], getattr(bl[blk], name).gw, self.g8.rec(blk * 4 + _GRAD[gname]), self._rec(blk, name, 0)))
        ops.gemm_tn_fp8_group(jobs8, hi - lo)
