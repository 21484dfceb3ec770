"""Exact-fp32 forward of a transformer stack: the schedule of engine.Stack._block_forward on fp32 buffers and the fp32 master weights.

Per block: LN (fp32 y, row-selected affine) -> qkv GEMM -> varlen attention -> proj GEMM (+residual) -> LN -> fc1 (+exact GELU) -> fc2 (+residual),
on ops.gemm_nt_f32 / ops.attn_fwd_f32 (csrc/exact.hip: f32-input MFMA, an accumulation order that depends on nothing but the contraction
index, erff / expf of the device library).  The weights are read where they live - ``arena.w(name)``, the fp32 masters the optimizer steps - so there is no bf16 shadow to
refresh and nothing cached that a training step could leave stale.  q leaves the qkv GEMM unscaled; the attention kernel applies hd^-0.5 to
the fp32 scores, as the reference does.

Forward only, for the inference forms of the fine-tuned model (ft_engine.py, ``exact=True``).  The pre-training passes (dual towers, pruned
decoder rows, pooled buffers) and every backward are not built on this path and are refused.
"""
from . import ops
from .engine import F32, I32, LN_EPS_BLOCK, _ln_fwd, _z


class _F32Linear:
    """fp32 master weight [N, K] and bias of one nn.Linear, straight from the arena"""

    def __init__(self, arena, prefix):
        self.w, self.b = arena.w(prefix + ".weight"), arena.w(prefix + ".bias")


class ExactStack:
    """`blocks` (engine.BlockParams: their arena / prefix name the masters, their n1 / n2 the LayerNorm vectors, which are fp32 already) over a
    packed [rows, D] fp32 residual stream.  Exposes what ft_engine.Encoder and the fusion stage use of engine.Stack: x, out, rp, row_mod, rows,
    forward()."""

    def __init__(self, dev, rows, D, H, hidden, seq_lens, blocks, row_mod=None, *, blocks2=None, split=0, inference=True, pool=None, opts=None, q_rows=0):
        if blocks2 is not None or split:
            raise ValueError("ExactStack: the two-tower form (blocks2 / split) of the MAE pass is not built on the exact-fp32 path")
        if q_rows:
            raise ValueError("ExactStack: the pruned last block (q_rows) of the decoder is not built on the exact-fp32 path")
        if pool is not None:
            raise ValueError("ExactStack: pooled activation buffers (pool) belong to the training passes; the exact-fp32 path owns its buffers")
        if not inference:
            raise ValueError("ExactStack is forward-only (inference=True): no activation is kept and there is no backward")
        assert sum(seq_lens) == rows
        if D // H not in (32, 64, 80) or D % H:
            raise ValueError(f"ExactStack: head dim {D}/{H} not supported (32, 64, 80)")
        self.blocks, self.rows, self.D, self.H, self.hidden, self.nblocks = blocks, rows, D, H, hidden, len(blocks)
        self.row_mod, self.inference = row_mod, True
        self.lin = [{k: _F32Linear(bp.arena, f"{bp.prefix}.{n}") for k, n in (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))}
                    for bp in blocks]
        self.rp = rp = ops.pad_rows(rows, 128)
        self.tiles = ops.AttnTiles(seq_lens, dev, tile_rows=128)
        ping = [_z((rp, D), F32, dev) for _ in range(2)]
        self.x = [ping[i & 1] for i in range(self.nblocks + 1)]
        self.xmid = _z((rp, D), F32, dev)
        self.ln = _z((rp, D), F32, dev)
        self.qkv = _z((rp, 3 * D), F32, dev)
        self.att = _z((rp, D), F32, dev)
        self.act = _z((rp, hidden), F32, dev)
        self.stats = [_z((rp,), F32, dev) for _ in range(4)]

    @property
    def out(self):
        return self.x[self.nblocks]

    def forward(self):
        for i in range(self.nblocks):
            self._block_forward(i)

    def _block_forward(self, i):
        M, bp, w, st = self.rows, self.blocks[i], self.lin[i], self.stats
        x = self.x[i]
        _ln_fwd(x, bp.n1, self.ln, st[0], st[1], M, LN_EPS_BLOCK, self.row_mod)
        ops.gemm_nt_f32(self.ln, w["qkv"].w, self.qkv, M, bias=w["qkv"].b)
        ops.attn_fwd_f32(self.qkv, self.tiles, self.H, self.att)
        ops.gemm_nt_f32(self.att, w["proj"].w, self.xmid, M, bias=w["proj"].b, res=x)
        _ln_fwd(self.xmid, bp.n2, self.ln, st[2], st[3], M, LN_EPS_BLOCK, self.row_mod)
        ops.gemm_nt_f32(self.ln, w["fc1"].w, self.act, M, bias=w["fc1"].b, act=1)
        ops.gemm_nt_f32(self.act, w["fc2"].w, self.x[i + 1], M, bias=w["fc2"].b, res=self.xmid)


class ExactPatchEmbedder:
    """engine.PatchEmbedder with fp32 patch rows and the master conv weight: gather -> gemm_nt_f32(cols, w32, out, bias, res=pos[row_tok], alpha=2)."""

    def __init__(self, arena, dev, rows, audio, cfg):
        self.audio, self.rows, self.cfg = audio, rows, cfg
        pre = "vit_base.patch_embed_a" if audio else "vit_base.patch_embed"
        self.w, self.b = arena.w(pre + ".proj.weight"), arena.w(pre + ".proj.bias")
        D = cfg.embed_dim
        skip = 0 if audio else 1          # the visual table starts with the cls row (engine.PatchEmbedder)
        self.pos = arena.view("vit_base.pos_embed_a" if audio else "vit_base.pos_embed").view(-1, D)[skip:]
        K = cfg.patch * cfg.patch * (1 if audio else cfg.in_chans)
        self.cols = _z((ops.pad_rows(rows, 128), K), F32, dev)
        self.row_src = _z((rows,), I32, dev)
        self.row_tok = _z((rows,), I32, dev)

    def set_rows(self, row_src, row_tok):
        self.row_src.copy_(row_src, non_blocking=True)
        self.row_tok.copy_(row_tok, non_blocking=True)

    def forward(self, inp, out, xf=None, aug=None):
        if aug is not None:
            raise ValueError("the exact-fp32 path has no augmentation form of the patch gather")
        if self.audio:
            ops.im2col_audio_f32(inp, self.row_src, self.row_tok, self.cols, self.rows, self.cfg.audio_t, xf, stride=self.cfg.st)
        else:
            ops.im2col_video_f32(inp, self.row_src, self.row_tok, self.cols, self.rows, xf, stride=self.cfg.st)
        ops.gemm_nt_f32(self.cols, self.w, out, self.rows, bias=self.b, res=self.pos, res_idx=self.row_tok, alpha=2.0)
