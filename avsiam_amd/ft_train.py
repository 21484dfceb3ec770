"""Training forms of the fine-tuned model's modes on the HIP kernels: forward with kept activations, and the hand-scheduled reverse.

What is trained (the reference's src/traintest_ft_base.py:133-175): ``audioonly`` and ``videoonly`` (any T: every frame is its own sequence),
and ``mm_grad`` with is_eval=False (T == 1, cav_mae_base.py:983-1035), whose three outputs (out, out_a, out_v) each have a head.
``retrieval`` and every is_eval form stay inference-only (ft_engine.py), as in the reference.

Reverse schedule of one backward (only what a live output reaches is computed):
  1. per live head: logits gradient -> dW = dlogits^T h, db = column sum (exact fp32, ops.gemm_f32_small), dh = dlogits W, LayerNorm backward
     (the fusion head normalises 2 D: avs_layernorm_bwd's classifier-head widths);
  2. pooled gradients -> token rows (segment_mean_bwd); for mm_grad the rows are in the fusion stack's [La | Lv] layout;
  3. fusion blocks backward (only when `out` is live); the pooled heads out_a / out_v then ADD their token gradient to the stack's dx
     (avs_segment_mean_bwd_acc), which maps back to the encoder rows through the forward's maps_a / map_v in
  4. the final LayerNorm backward (norm_a / norm), then
  5. the shared encoder's Stack.backward and 6. the patch embeddings (conv weights, biases, pos_embed / pos_embed_a) - both only when some
     base parameter requires a gradient (freeze_base, traintest_ft_base.py:68-71, stops at the fusion stack's input).
The encoder kinds a / v / av are built on first use and bump-allocate their activations from ONE engine.BufferPool (one of them runs per step).
The fused step of traintest_ft_base.train_step runs the `a` / `v` branches of mm_grad on that modality's encoder alone - exactly what the
reference's autograd computes for loss_fn(out_a, ...) / loss_fn(out_v, ...) (out_a / out_v read nothing of the other modality).
"""
import math

import torch

from . import ops
from .arena import ALIGN, ParamArena
from .config import AVSiamConfig, EngineOptions
from .engine import F32, I32, LN_EPS_BLOCK, LN_EPS_FINAL, BlockParams, BufferPool, Norm, _dx_in, _ln_bwd, _ln_fwd, _z, make_stack
from .ft_engine import Encoder, Head

OUT, OUT_A, OUT_V = 1, 2, 4          # live-output bits of a backward


class TrainHead(Head):
    """Head with what its backward reads: an fp32 copy of the normalised input (operand of the exact fp32 weight-gradient product)."""

    def __init__(self, arena: ParamArena, name, width, label_dim, max_rows, dev):
        super().__init__(arena, name, width, label_dim, max_rows, dev)
        rp = ops.pad_rows(max_rows, 256)
        self.hf = _z((rp, width), F32, dev)
        self.dlog = _z((rp, self.npad), F32, dev)         # logits gradient (the loss kernel's output, or the autograd gradient copied in)
        self.dh = _z((rp, width), F32, dev)
        self.ones = torch.ones(rp, dtype=F32, device=dev)
        self.lnws = _z((ops.layernorm_ws(rp, width),), F32, dev)
        self.wf = arena.w(f"{name}.1.weight")              # fp32 master [L, width]
        self.gw, self.gb = arena.gw(f"{name}.1.weight"), arena.gw(f"{name}.1.bias").view(1, label_dim)
        own = [n for n in arena.names if n.startswith(name + ".") and arena.info[n].live]
        self.grange = (min(arena.offset[n] for n in own), max(arena.offset[n] + ops.pad_rows(math.prod(arena.info[n].shape), ALIGN) for n in own))
        self.x = None

    def forward(self, x, n):
        out = super().forward(x, n)                        # the inference path's logits, bit for bit
        ops.layernorm_fwd(x, self.norm.g, self.norm.b, self.hf, self.stat[0], self.stat[1], n, LN_EPS_BLOCK)
        self.x = x
        return out

    def backward(self, n, dx):
        """self.dlog[:n, :L] holds d loss / d logits -> parameter gradients (stored / LayerNorm: accumulated) and dx [n, width] (fp32)."""
        L, W, ld = self.L, self.width, self.npad
        ops.gemm_f32_small(self.dlog, self.wf, self.dh, n, W, L, (ld, 1), (W, 1))              # dh = dlogits . W
        ops.gemm_f32_small(self.dlog, self.hf, self.gw, L, W, n, (1, ld), (W, 1))              # dW = dlogits^T . h
        ops.gemm_f32_small(self.ones, self.dlog, self.gb, 1, L, n, (n, 1), (ld, 1))            # db = 1^T . dlogits
        ops.layernorm_bwd(self.dh, self.x, self.stat[0], self.stat[1], self.norm.g, dx, self.norm.dg, self.norm.db, self.lnws, n)


class FtTrain:
    """Training forward / backward of the fine-tune modes for one (batch, frames) shape."""

    def __init__(self, arena: ParamArena, cfg: AVSiamConfig, label_dim, batch, frames, dev, opts: EngineOptions = None):
        assert arena.g is not None and arena.wt is not None, "ParamArena.enable_training() first"
        self.opts = opts if opts is not None else EngineOptions()
        if self.opts.fp8 != "0":
            raise ValueError("fine-tuning runs the bf16 path only (fp8 fine-tuning is not implemented)")
        self.arena, self.cfg, self.B, self.T, self.dev, self.L = arena, cfg, batch, frames, dev, label_dim
        D = cfg.embed_dim
        self.blocks = [BlockParams(arena, f"vit_base.blocks.{i}", "_a", "_v") for i in range(cfg.depth)]
        self.final = [Norm(arena, "vit_base.norm_a"), Norm(arena, "vit_base.norm")]
        self.blk_mm = [BlockParams(arena, "mm_layer_1", "_a"), BlockParams(arena, "mm_layer_2", "_a")]
        nmax = batch * max(frames, 1)
        self.head_v = TrainHead(arena, "mlp_head", D, label_dim, nmax, dev)
        self.head_a = TrainHead(arena, "mlp_head_a", D, label_dim, batch, dev)
        self.head_mm = TrainHead(arena, "mlp_head_mm", 2 * D, label_dim, batch, dev)
        self.pool = BufferPool(dev)
        self._enc = {}
        self._joint = None
        self.state = None                 # (mode, kind, live heads, token) of the last training forward
        self.token = 0

    def refresh_heads(self):
        for h in (self.head_v, self.head_a, self.head_mm):
            h.refresh()

    def encoder(self, kind):
        if kind not in self._enc:
            na = self.B if "a" in kind else 0
            nv = self.B * self.T if "v" in kind else 0
            self.pool.rewind()
            enc = Encoder(self.arena, self.cfg, na, nv, self.blocks, self.final, self.dev, inference=False, pool=self.pool, opts=self.opts)
            enc.dpool = _z(tuple(enc.pooled.shape), F32, self.dev)
            self._enc[kind] = enc
        return self._enc[kind]

    def joint(self):
        """The two fusion blocks over B sequences [La audio tokens | Lv frame tokens] (cav_mae_base.py:1022-1024)."""
        if self._joint is None:
            cfg, B, dev = self.cfg, self.B, self.dev
            La, Lv, D = cfg.audio_tokens, cfg.video_tokens, cfg.embed_dim
            Lj = La + Lv
            st = make_stack(dev, B * Lj, D, cfg.num_heads, D * cfg.mlp_ratio, [Lj] * B, self.blk_mm, opts=self.opts)
            b = torch.arange(B).view(B, 1)
            map_a = (b * Lj + torch.arange(La).view(1, La)).reshape(-1).to(I32).to(dev)
            map_v = (b * Lj + La + torch.arange(Lv).view(1, Lv)).reshape(-1).to(I32).to(dev)
            seg = []
            for q in range(B):
                seg += [q * Lj, q * Lj + La]
            seg.append(B * Lj)
            seg_start = torch.tensor(seg, dtype=I32, device=dev)
            # joint segment 2q (audio of clip q) <- pooled row q, 2q + 1 (its frame) <- pooled row B + q of the encoder's [audio | frames]
            rmap = torch.stack([torch.arange(B), B + torch.arange(B)], dim=1).reshape(-1).to(I32).to(dev)
            pooled = _z((ops.pad_rows(2 * B, 256), D), F32, dev)
            dpooled = _z((ops.pad_rows(2 * B, 256), D), F32, dev)
            self._joint = dict(st=st, map_a=map_a, map_v=map_v, seg=seg_start, rmap=rmap, pooled=pooled, dpooled=dpooled)
        return self._joint

    # ---- forward ---------------------------------------------------------------------------------------------
    def forward(self, mode, audio, frames, heads, xf=(None, None), aug=None):
        """xf: (audio, frames) raw-input transforms or None each; aug: the step's augmentation plan (ops.FtAug) - both applied inside the
        patch gathers (ft_engine.Encoder.forward).  The backward is unchanged: the patch embedding's weight gradient reads the saved rows.
        mode: "audioonly" | "videoonly" | "mm_grad" | "mm_a" | "mm_v" (mm_grad's out_a / out_v branch on its modality's encoder alone).
        heads: live-output bits to compute (OUT, OUT_A, OUT_V; mm_grad only - the single-output modes always compute theirs).
        -> {bit: logits view}"""
        B, T = self.B, self.T
        res = {}
        if mode in ("audioonly", "mm_a"):
            kind = "a"
            enc = self.encoder(kind)
            self.pool.owner = enc
            enc.forward(audio, None, xf, aug)
            res[OUT_A] = self.head_a.forward(enc.pool(), B)
        elif mode in ("videoonly", "mm_v"):
            kind = "v"
            enc = self.encoder(kind)
            self.pool.owner = enc
            enc.forward(None, frames, xf)
            res[OUT_V] = self.head_v.forward(enc.pool(), B * T)
        elif mode == "mm_grad":
            if T != 1:
                raise ValueError(f"mm_grad training needs single-frame clips (cav_mae_base.py:1022), got {T} frames")
            kind = "av"
            enc = self.encoder(kind)
            self.pool.owner = enc
            enc.forward(audio, frames, xf, aug)
            if heads & OUT:
                j = self.joint()
                st, so = j["st"], enc.stack.out
                _ln_fwd(so, self.final[:1], st.x[0], enc.fstat[0], enc.fstat[1], enc.rows_a, LN_EPS_FINAL, out_map=j["map_a"])
                _ln_fwd(so[enc.rows_a:], self.final[1:], st.x[0], enc.fstat[0][enc.rows_a:], enc.fstat[1][enc.rows_a:], enc.rows_v, LN_EPS_FINAL,
                        out_map=j["map_v"])
                st.forward()
                ops.segment_mean_fwd(st.out, j["seg"], j["pooled"], 2 * B)                   # [a-part mean | v-part mean] per clip (:1027-1030)
                res[OUT] = self.head_mm.forward(j["pooled"].view(-1, 2 * self.cfg.embed_dim), B)
            if heads & (OUT_A | OUT_V):
                pa = enc.pool()
                if heads & OUT_A:
                    res[OUT_A] = self.head_a.forward(pa, B)                                  # :1019
                if heads & OUT_V:
                    res[OUT_V] = self.head_v.forward(pa[B:], B)                              # :1020
        else:
            raise ValueError(f"mode {mode!r} has no training form (audioonly, videoonly, mm_grad)")
        self.token += 1
        self.state = dict(mode=mode, kind=kind, heads=sum(res), token=self.token, done=False)
        return res

    # ---- backward ----------------------------------------------------------------------------------------------
    def check(self, token):
        st = self.state
        if st is None or st["token"] != token:
            raise RuntimeError("CAVMAEFT_BASE: another training forward of this shape ran since this output was computed - its activations "
                               "are gone (backward each forward before the next one)")
        if st["done"]:
            raise RuntimeError("CAVMAEFT_BASE: second backward through one forward; gradients are delivered once per forward "
                               "(run the forward again)")
        enc = self._enc[st["kind"]]
        if self.pool.owner is not enc:
            raise RuntimeError("CAVMAEFT_BASE: another encoder kind ran its forward since this one's - the shared activations are gone")

    def backward(self, token, live, base=True, reducer=None):
        """live: output bits whose logits gradient is in the heads' dlog buffers; base: the encoder (final norms, blocks, patch embeddings)
        needs gradients.  The caller has zeroed the gradient arena (ParamArena.zero_grad_range).
        reducer (comm.FixedScheduleReducer, data parallel): told the heads' and the blocks' gradient ranges as they become final; the final
        norms and the patch embeddings are left to its finish()."""
        self.check(token)
        st_ = self.state
        st_["done"] = True
        mode, B, T = st_["mode"], self.B, self.T
        live &= st_["heads"]
        enc = self._enc[st_["kind"]]
        st = enc.stack
        if mode != "mm_grad":
            head, n = (self.head_a, B) if st_["kind"] == "a" else (self.head_v, B * T)
            if not live:
                return
            head.backward(n, enc.dpool)
            if reducer is not None:
                reducer.ready(*head.grange)
            if not base:
                return
            ops.segment_mean_bwd(enc.dpool, enc.seg_start, enc.yf, enc.nseq)
            _ln_bwd(enc.yf, st.out, enc.fstat[0], enc.fstat[1], self.final, _dx_in(st), st.lnws, enc.rows, st.row_mod,
                    dx_bf16=st.dxb[0], dcol=self.blocks[-1].fc2.gb)
        else:
            if not live:
                return
            D = self.cfg.embed_dim
            j = self.joint() if live & OUT else None
            if live & (OUT_A | OUT_V):
                if live & (OUT_A | OUT_V) != (OUT_A | OUT_V):
                    enc.dpool[:2 * B].zero_()
                if live & OUT_A:
                    self.head_a.backward(B, enc.dpool)
                    if reducer is not None:
                        reducer.ready(*self.head_a.grange)
                if live & OUT_V:
                    self.head_v.backward(B, enc.dpool[B:])
                    if reducer is not None:
                        reducer.ready(*self.head_v.grange)
            if live & OUT:
                sm = j["st"]
                self.head_mm.backward(B, j["dpooled"].view(-1, 2 * D))
                if reducer is not None:
                    reducer.ready(*self.head_mm.grange)
                ops.segment_mean_bwd(j["dpooled"], j["seg"], sm.dx[0], 2 * B)
                ops.cast_scale(sm.dx[0], sm.dxb[0], sm.rows * D, 1.0)
                sm.backward(reducer=reducer)
                dy = sm.dx[0]
                if not base:
                    return
                if live & (OUT_A | OUT_V):                       # the pooled heads add to what the fusion blocks left on the same rows
                    ops.segment_mean_bwd_acc(enc.dpool, j["seg"], dy, 2 * B, row_map=j["rmap"], max_row=2 * B)
                maps = (j["map_a"], j["map_v"])
            else:
                if not base:
                    return
                ops.segment_mean_bwd(enc.dpool, enc.seg_start, enc.yf, enc.nseq)
                dy, maps = enc.yf, (None, None)
            ra = enc.rows_a
            for lo, fin, rows, omap in ((0, self.final[:1], ra, maps[0]), (ra, self.final[1:], enc.rows_v, maps[1])):
                _ln_bwd(dy if omap is not None else dy[lo:], st.out[lo:], enc.fstat[0][lo:], enc.fstat[1][lo:], fin,
                        _dx_in(st, lo), st.lnws, rows, out_map=omap, dx_bf16=st.dxb[0][lo:], dcol=self.blocks[-1].fc2.gb)
        st.backward(last_fc2_bias_done=True, reducer=reducer)
        if enc.na:
            enc.emb_a.backward(st.dx[0][:enc.rows_a])
        if enc.nv:
            enc.emb_v.backward(st.dx[0][enc.rows_a:])
