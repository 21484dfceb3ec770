"""``CAVMAEFT_BASE`` - the fine-tuned classifier on the hand-written gfx950 kernels: its inference modes, and fine-tuning.

Boundary kept: the constructor and ``forward(a, v, mode, is_eval=False)`` of
/root/reference/src/models/cav_mae_base.py:744-746,827 and the 553-key ``state_dict()`` schema (so the checkpoints the
reference's fine-tuning writes, traintest_ft_base.py:255-264, load here, ``module.`` prefix or not; a pre-training CAVMAE_BASE checkpoint
loads with strict=False as run_cavmae_ft_base.py:243-249 does), with the return shapes of every mode (:847,866,892,961,1035).

Scope.  By default the model is inference-only: parameters are registered with ``requires_grad=False``, outputs carry no autograd graph,
and only the forward buffers exist.  Fine-tuning is switched on the standard way - ``model.requires_grad_(True)``, or per parameter as
the reference's freeze_base loop does (traintest_ft_base.py:68-71).  Then, with grad mode on and a trainable mode (``audioonly``,
``videoonly``, ``mm_grad`` with is_eval=False; ``retrieval`` and the is_eval forms stay inference-only, as in the reference), ``forward``
returns its outputs from ONE autograd node whose backward is the hand-scheduled reverse of ft_train.py: an output that gets no gradient
is skipped, the encoder's backward runs only when a base parameter requires a gradient, and ``.grad`` is delivered as views of a flat
gradient arena (allocated, with the transposed weight copies, on first training use) to exactly the parameters the reference's autograd
would reach.  One backward per forward, and every ``.grad`` must be cleared (set to None, torch's default zero_grad) before the next
backward: gradient accumulation across backwards is refused with an error.
``train_step`` (traintest_ft_base.train_step) is the fused step: forward of the loss's branch only, the HIP loss kernel, the backward and
the HIP Adam over the reference's three parameter groups, without a host sync.  The bf16 path only (fp8 fine-tuning is refused).
Data parallel (``set_distributed`` with an active comm; the reference's DistributedDataParallel(find_unused_parameters=True),
traintest_ft_base.py:91-92): ranks may run different branches in one step, so the gradients are summed in a message schedule fixed by the
arena layout (comm.FixedScheduleReducer), the union of the ranks' live gradient classes reaches the device as the schedule's last message,
and ONE avs_adam_table launch over the whole trainable arena steps exactly those classes - rates, step counts and liveness in device
memory, no host sync.  ``.grad`` stays None after such a step and the autograd path raises.  No run with more than one rank on RCCL exists:
verified are the arithmetic and the schedule (tests/test_ft_dp_*.py), not the scaling.
Gradient accumulation (``set_grad_accumulation(k)``; the fused step only - the autograd path keeps refusing it): every train_step is a
micro-step whose gradients avs_grad_accum adds into an fp32 buffer over the trainable range, the union of the gradient classes the
micro-steps reached is kept on the device, and the k-th micro-step (or ``apply_accumulated``) takes ONE optimizer step over that union with
the gradients divided by the micro-steps (and the ranks).
There is no CPU/eager fallback: ``forward`` without a GPU and libavsiam_hip.so raises.
"""
import math
import os

import torch
import torch.nn as nn

from .. import _lib
from ..arena import ParamArena
from ..config import AVSiamConfig
from ..param_spec import build_spec_ft
from ..weights import synth_state_ft
from .cav_mae_base import _attach


def _padded(info):
    """elements a tensor occupies in the arena (ALIGN-padded)"""
    from ..arena import ALIGN
    return (math.prod(info.shape) + ALIGN - 1) // ALIGN * ALIGN

MODES = ("audioonly", "videoonly", "retrieval", "mm_grad")
TRAIN_MODES = ("audioonly", "videoonly", "mm_grad")
MAX_ENGINES = 4          # (batch, frames) shapes whose activation buffers are kept resident
MAX_TRAIN_ENGINES = 2    # ... of them with training activations


def param_group(name):
    """The reference's optimizer groups (traintest_ft_base.py:47-57): names containing 'mlp_head' -> "head" (lr * head_lr), 'mm_layer' ->
    "mm" (lr * mm_lr), everything else -> "base" (lr; the group freeze_base freezes)."""
    if "mlp_head" in name:
        return "head"
    if "mm_layer" in name:
        return "mm"
    return "base"


def _modality(name):
    """'a' / 'v' for base parameters only one modality's rows read (patch embeddings, positional tables, the _a / _v LayerNorms, the final
    norms), 's' for the shared ones (cav_mae_base.py:829-841,852-860)."""
    if any(k in name for k in ("patch_embed_a.", "pos_embed_a", "norm_a.", "norm1_a.", "norm2_a.")):
        return "a"
    if any(k in name for k in ("patch_embed.", "pos_embed", "vit_base.norm.", "norm1_v.", "norm2_v.")):
        return "v"
    return "s"


def grad_class(name):
    """Unit of gradient liveness: parameters of one class get a gradient in exactly the same backwards (and so share an Adam step count)."""
    g = param_group(name)
    if g == "head":
        return name.split(".")[0]                       # mlp_head | mlp_head_a | mlp_head_mm | mlp_head_mm_v2
    if g == "mm":
        return "mm"
    return "base_" + _modality(name)


def live_classes(mode, live):
    """Classes the reference's autograd reaches from the live outputs (ft_train OUT / OUT_A / OUT_V bits) of a training mode."""
    from ..ft_train import OUT, OUT_A, OUT_V
    if mode == "audioonly":
        return {"base_a", "base_s", "mlp_head_a"} if live else set()
    if mode == "videoonly":
        return {"base_v", "base_s", "mlp_head"} if live else set()
    out = set()
    if live & OUT:
        out |= {"base_a", "base_v", "base_s", "mm", "mlp_head_mm"}
    if live & OUT_A:
        out |= {"base_a", "base_s", "mlp_head_a"}
    if live & OUT_V:
        out |= {"base_v", "base_s", "mlp_head"}
    return out


GROUPS = ("base", "head", "mm")                                        # index = avs_adam_ctl.lr[]
CLASSES = ("base_a", "base_v", "base_s", "mm", "mlp_head", "mlp_head_a", "mlp_head_mm", "mlp_head_mm_v2")      # index = avs_adam_ctl.step[] / live[]


class _FtNode(torch.autograd.Function):
    """One node for a training forward of CAVMAEFT_BASE: forward launches the kernel schedule, backward the hand-written reverse."""

    @staticmethod
    def forward(ctx, anchor, model, eng, mode, a, v, xf, aug):
        ctx.set_materialize_grads(False)
        from ..ft_train import OUT, OUT_A, OUT_V
        heads = (OUT | OUT_A | OUT_V) if mode == "mm_grad" else 0
        res = eng.forward(mode, a, v, heads) if xf is None and aug is None else eng.forward(mode, a, v, heads, xf or (None, None), aug)
        ctx.model, ctx.eng, ctx.mode, ctx.token = model, eng, mode, eng.token
        if mode == "audioonly":
            ctx.bits = (OUT_A,)
            return res[OUT_A].clone()
        if mode == "videoonly":
            ctx.bits = (OUT_V,)
            return res[OUT_V].view(eng.B, eng.T, eng.L).squeeze(1).clone()
        ctx.bits = (OUT, OUT_A, OUT_V)
        return res[OUT].clone(), res[OUT_A].clone(), res[OUT_V].clone()

    @staticmethod
    def backward(ctx, *grads):
        eng = ctx.eng
        from ..ft_train import OUT, OUT_A, OUT_V
        heads = {OUT: eng.head_mm, OUT_A: eng.head_a, OUT_V: eng.head_v}
        live = 0
        for bit, g in zip(ctx.bits, grads):
            if g is None:
                continue
            live |= bit
            h = heads[bit]
            n = g.numel() // eng.L
            h.dlog[:n, :eng.L].copy_(g.reshape(n, eng.L))
        ctx.model._backward(eng, ctx.token, ctx.mode, live)
        return (None,) * 8


class CAVMAEFT_BASE(nn.Module):
    def __init__(self, label_dim, img_size=224, audio_length=1024, patch_size=16, in_chans=3, embed_dim=768,
                 modality_specific_depth=23, num_heads=16, mlp_ratio=4., norm_layer=nn.LayerNorm, norm_pix_loss=False,
                 tr_pos=True, *, cfg: AVSiamConfig = None, init_seed=0, init_mode="init"):
        """As in the reference every argument but ``label_dim`` is accepted and ignored (the dimensions are fixed by the
        ViT-B skeleton, :749-766); keyword-only ``cfg=`` selects other shapes."""
        super().__init__()
        self.cfg = cfg if cfg is not None else AVSiamConfig()
        self.label_dim = int(label_dim)
        self._spec = build_spec_ft(self.cfg, self.label_dim)
        self.arena = ParamArena(self.cfg, self._spec, transposed=False, grads=False)
        self.arena.load_state(synth_state_ft(self.cfg, self.label_dim, init_seed, init_mode))
        self._params = {}
        for info in self._spec:
            p = nn.Parameter(self.arena.view(info.name), requires_grad=False)
            self._params[info.name] = p
            _attach(self, info.name, p)
        self.my_blocks = self.vit_base.blocks                      # same module object, two names (:749,782)
        first = ("vit_base", "my_blocks")                          # registration order of the reference => same state_dict key order
        mods = dict(self._modules)
        self._modules.clear()
        for k in first + tuple(k for k in mods if k not in first):
            self._modules[k] = mods[k]
        self._engines = {}
        self._train_engines = {}
        self._shadow_dirty = True
        self._versions = None
        self._opt = None                                           # HIP Adam state of train_step / adam_step
        self._world, self._rank, self._comm, self._dp = 1, 0, None, False
        self._dps = None                                           # data-parallel / guarded step state (_dp_state)
        self._guard_max = None                                     # set_grad_guard: max_norm of the guarded step; None: no guard
        self._guard = None                                         # ops.GradGuard: the guard's device block (made at the first guarded step)
        self._rates = None                                         # (base, head, mm) learning rates of the last Adam step
        self._accum_k = None                                       # set_grad_accumulation: micro-steps per optimizer step; None: no accumulation
        self._acc = None                                           # the accumulation buffer, its device block and the pending count (_micro_step)
        self._guard_scale = None                                   # grad_scale of the last segment-table step (guard_stats)
        self._aug_seed = None                                      # set_aug_seed; None: derived from torch's seed at the first draw
        self._aug_st = None                                        # ops.FtAugState: the augmentation draws' key and counter, on the device
        self._aug_plans = {}                                       # batch -> the ops.FtAug buffer draw_aug draws into

    def __create_fusion__(self):
        """mm_layer_1/2 <- copies of blocks 10 and 11 (:824-826; the fine-tune CLI calls it after loading a pre-trained
        checkpoint that lacks them)."""
        with torch.no_grad():
            for dst, src in (("mm_layer_1", self.cfg.depth - 2), ("mm_layer_2", self.cfg.depth - 1)):
                pre = f"vit_base.blocks.{src}."
                for name, p in self._params.items():
                    if name.startswith(pre):
                        self._params[dst + "." + name[len(pre):]].copy_(p)
        self._shadow_dirty = True

    def _apply(self, fn, recurse=True):
        probe = fn(torch.empty(0, dtype=torch.float32, device=self.arena.p.device))
        if probe.dtype != torch.float32:
            raise TypeError("CAVMAEFT_BASE keeps fp32 master weights; bf16 shadows are managed internally")
        if probe.device != self.arena.p.device:
            self.arena.to(probe.device)
            for name, p in self._params.items():
                p.data = self.arena.view(name)
                p.grad = None
            self._engines.clear()
            self._train_engines.clear()
            self._opt = None
            self._dps = None
            self._guard = None
            self._acc = None
            self._aug_st, self._aug_plans = None, {}
            self._shadow_dirty = True
        return self

    def load_state_dict(self, state_dict, strict=True, assign=False):
        if any(k.startswith("module.") for k in state_dict):       # DDP-wrapped checkpoints (traintest_ft_base.py:255)
            state_dict = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        out = super().load_state_dict(state_dict, strict=strict)
        self._shadow_dirty = True
        return out

    def mark_weights_changed(self):
        self._shadow_dirty = True

    def _engine(self, batch, frames, exact=False):
        key = (batch, frames, True) if exact else (batch, frames)  # exact-fp32 engines share the cache and its limit
        if key not in self._engines:
            from ..ft_engine import FtForward
            while len(self._engines) >= MAX_ENGINES:               # serving with many batch shapes: drop the oldest buffers
                self._engines.pop(next(iter(self._engines)))
            self._engines[key] = FtForward(self.arena, self.cfg, self.label_dim, batch, frames, self.arena.p.device, **({"exact": True} if exact else {}))
        else:
            self._engines[key] = self._engines.pop(key)            # most recently used last
        return self._engines[key]

    # ---- fine-tuning ---------------------------------------------------------------------------------------------
    def _trainable(self):
        return [n for n, p in self._params.items() if p.requires_grad]

    def _train_engine(self, batch, frames):
        if self.arena.enable_training():
            self._shadow_dirty = True
        key = (batch, frames)
        if key not in self._train_engines:
            from ..ft_train import FtTrain
            while len(self._train_engines) >= MAX_TRAIN_ENGINES:
                self._train_engines.pop(next(iter(self._train_engines)))
            self._train_engines[key] = FtTrain(self.arena, self.cfg, self.label_dim, batch, frames, self.arena.p.device)
        return self._train_engines[key]

    def _sync_shadows(self):
        # an optimizer the model does not know about (torch.optim.Adam over .grad, in-place ops on the parameters under no_grad) changes the fp32
        # masters in place: every such op bumps the parameter's version counter, so a changed sum marks the bf16 shadows stale (checked only once
        # training is switched on).  Edits through `p.data` do NOT show here (`.data` has a version counter of its own): call
        # mark_weights_changed() after them, as after any write the model cannot see.
        if self.arena.with_grads:
            ver = sum(p._version for p in self._params.values())
            if ver != self._versions:
                self._versions = ver
                self._shadow_dirty = True
        if self._shadow_dirty:
            self.arena.refresh_shadows(None)
            for e in list(self._engines.values()) + list(self._train_engines.values()):
                e.refresh_heads()
            self._shadow_dirty = False
            if self.arena.with_grads:
                self._versions = sum(p._version for p in self._params.values())

    def _input_xf(self, input_xf, mode):
        """-> (audio transform | None, frame transform | None) for the inputs `mode` reads, kinds checked; None when input_xf is None"""
        if input_xf is None:
            return None
        from ..ops import InputXf
        xa, xv = tuple(input_xf)
        if mode != "videoonly" and not (isinstance(xa, InputXf) and xa.kind == 1):
            raise ValueError("input_xf = (ops.InputXf.audio(mean, std), ops.InputXf.frames()): the first entry must be an audio transform")
        if mode != "audioonly" and not (isinstance(xv, InputXf) and xv.kind == 2):
            raise ValueError("input_xf = (ops.InputXf.audio(mean, std), ops.InputXf.frames()): the second entry must be a frame transform")
        return (xa if mode != "videoonly" else None, xv if mode != "audioonly" else None)

    # ---- augmentation draws (SpecAugment masks, noise, time roll: ops.FtAug) ---------------------------------------
    def set_aug_seed(self, seed):
        """Seed of this model's augmentation draws; the draw counter restarts.  Default (never called): torch.initial_seed() % 2^31 at the
        first draw, as CAVMAE_BASE derives its plan seed.  The Philox key is (seed, rank): data-parallel ranks augment differently (their
        weights stay identical byte for byte all the same - that is the reducer's doing, not the inputs')."""
        self._aug_seed = int(seed)
        self._aug_st, self._aug_plans = None, {}

    def _aug_state(self):
        if self._aug_st is None:
            from ..ops import FtAugState
            seed = self._aug_seed if self._aug_seed is not None else int(torch.initial_seed() % (2 ** 31))
            self._aug_st = FtAugState(self.arena.p.device, ((seed & 0xFFFFFFFF) << 32) | (self._rank & 0xFFFFFFFF))
        return self._aug_st

    def aug_counter(self):
        """augmentation plans drawn so far (synchronises)"""
        return self._aug_state().counter()

    def draw_aug(self, batch, freqm=0, timem=0, noise=False, fill=0.0):
        """The next training step's augmentation plan for `batch` clips, drawn on the device (no host sync) into this model's buffer for that
        batch size - pass it to the step that follows, before the next draw.  fill: what a masked cell of an already normalised input takes
        ((0 - dataset_mean) / dataset_std reproduces the reference); raw inputs (input_xf) get that value by themselves."""
        from ..ops import FtAug
        st = self._aug_state()
        plan = FtAug.draw(st, batch, self.cfg.audio_len, self.cfg.n_mels, freqm, timem, noise, out=self._aug_plans.get(batch), fill=fill)
        plan.fill = float(fill)
        self._aug_plans[batch] = plan
        return plan

    def _prepare(self, a, v, mode, xf=None):
        """-> (a, v folded to [B*T, C, H, W], B, T) on the model's device, shapes checked.  xf (from _input_xf): the inputs are raw - `a` the
        un-normalised fp32 fbank, `v` uint8 frames, which stay uint8"""
        cfg, dev = self.cfg, self.arena.p.device
        need_a, need_v = mode != "videoonly", mode != "audioonly"
        B = (a if need_a else v).shape[0]
        T = 1
        if need_a:
            if tuple(a.shape[1:]) != (cfg.audio_len, cfg.n_mels):
                raise ValueError(f"a must be [B,{cfg.audio_len},{cfg.n_mels}], got {tuple(a.shape)}")
            a = a.to(dev, torch.float32).contiguous()
        if need_v:
            if v.dim() != 5 or tuple(v.shape[2:]) != (cfg.in_chans, cfg.img_size, cfg.img_size) or v.shape[0] != B:
                raise ValueError(f"v must be [B,T,{cfg.in_chans},{cfg.img_size},{cfg.img_size}], got {tuple(v.shape)}")
            T = v.shape[1]
            if xf is not None:
                if v.dtype != torch.uint8:
                    raise ValueError("input_xf for the frames expects uint8 images")
                v = v.to(dev).contiguous().view(B * T, cfg.in_chans, cfg.img_size, cfg.img_size)
            else:
                v = v.to(dev, torch.float32).contiguous().view(B * T, cfg.in_chans, cfg.img_size, cfg.img_size)
        return a, v, B, T

    def _check_aug(self, aug, B, mode):
        from ..ops import FtAug
        if not isinstance(aug, FtAug):
            raise TypeError("aug must be an ops.FtAug plan (model.draw_aug, ops.FtAug.draw / from_arrays)")
        if mode == "videoonly":
            raise ValueError("aug augments the audio input; videoonly reads none")
        if aug.n < B:
            raise ValueError(f"aug holds {aug.n} sample records for a batch of {B}")

    def _backward(self, eng, token, mode, live):
        """Zero the gradient arena, run the reverse of the training forward `token` for the live outputs, deliver .grad.
        Gradient accumulation across backwards is refused: the arena holds ONE backward's gradients, so every .grad must have been cleared
        (set to None, torch's default zero_grad) since the last one - a backward would otherwise overwrite the gradients still delivered."""
        eng.check(token)
        self._check_not_accumulating("backward")
        held = [n for n, p in self._params.items() if p.grad is not None]
        if held:
            raise RuntimeError(f"CAVMAEFT_BASE: {len(held)} parameter(s) (e.g. {held[0]}) still hold .grad from an earlier backward; gradient "
                               "accumulation across backwards is not supported - clear the gradients (optimizer.zero_grad() / model.zero_grad(), "
                               "set_to_none=True) before the next backward")
        trainable = set(self._trainable())
        cls = live_classes(mode, live)
        names = [n for n in trainable if grad_class(n) in cls and self.arena.info[n].live]
        base = any(param_group(n) == "base" for n in names)
        from .. import ops as _ops
        _ops.timed("torch_zero_grads", lambda: self.arena.zero_grad_range(1))
        eng.backward(token, live if names else 0, base=base)
        for n in names:
            self._params[n].grad = self.arena.gview(n)
        return names

    def train_step(self, a, v, labels, lr, ftmode="mm_grad", branch=None, loss="BCE", head_lr=1.0, mm_lr=1.0, beta1=0.95, beta2=0.999,
                   eps=1e-8, weight_decay=5e-7, *, input_xf=None, aug=None, guard=None):
        """One fused fine-tuning step (traintest_ft_base.py:133-175 without the host): the forward of the loss's branch only, the HIP
        classification loss, the backward and the HIP Adam of the reference's three groups.  -> the loss (device tensor [1], no sync).
        branch (mm_grad only): "mm" (loss on out), "a" (out_a: the audio encoder alone), "v" (out_v: the frame encoder alone).
        Data parallel (set_distributed with an active comm): the loss is this rank's batch mean; the gradients are summed over the ranks in a
        rank-independent message schedule and divided by the world size inside the one-launch Adam, which steps every gradient class that ANY
        rank reached (DistributedDataParallel(find_unused_parameters=True)); ``.grad`` is left None after such a step, and the step counts
        live on the device (optimizer_steps()).
        input_xf = (ops.InputXf.audio(mean, std), ops.InputXf.frames()): `a` is the un-normalised fbank and `v` uint8 frames, normalised
        inside the patch gathers.  aug (ops.FtAug, e.g. draw_aug()): the step's SpecAugment masks, noise and time roll, applied inside the
        audio patch gather - to the raw fbank with input_xf, to a normalised `a` without; ignored by the branches that read no audio ("v").
        Guarded (set_grad_guard, or guard = a max_norm for this call alone): between the gradients and Adam the device computes the gradient
        norm, the clip_grad_norm_ coefficient and whether any gradient is inf or NaN; Adam scales the gradients by the coefficient, or - on a
        non-finite gradient - writes nothing at all and keeps its step counts.  Still no host sync: guard_stats() reads the outcome.  A
        guarded step takes the segment-table route of the data-parallel step on one rank too: ``.grad`` is left None after it, and the
        step counts live on the device (optimizer_steps())."""
        from .. import ops
        from ..ft_train import OUT, OUT_A, OUT_V
        if ftmode not in TRAIN_MODES:
            raise ValueError(f"ftmode {ftmode!r} has no training form ({', '.join(TRAIN_MODES)})")
        if loss not in ("BCE", "CE"):
            raise ValueError(f"loss must be BCE or CE, not {loss!r}")
        if not self.arena.p.is_cuda:
            raise _lib.AvsiamHipError("CAVMAEFT_BASE.train_step needs a GPU (no CPU/eager fallback). Move the model with .cuda() first.")
        _lib.load()
        if ftmode == "mm_grad":
            branch = "mm" if branch is None else branch
            if branch not in ("mm", "a", "v"):
                raise ValueError(f"branch must be mm, a or v, not {branch!r}")
            mode, bit = {"mm": ("mm_grad", OUT), "a": ("mm_a", OUT_A), "v": ("mm_v", OUT_V)}[branch]
            cls_mode = {"mm": "mm_grad", "a": "audioonly", "v": "videoonly"}[branch]
        else:
            mode, cls_mode, bit = ftmode, ftmode, (OUT_A if ftmode == "audioonly" else OUT_V)
        for p in self._params.values():                           # the step owns the gradients: optimizer.zero_grad() of :168
            p.grad = None
        in_mode = "mm_grad" if mode == "mm_grad" else cls_mode
        xf = self._input_xf(input_xf, in_mode)
        a, v, B, T = self._prepare(a, v, in_mode, xf)
        if aug is not None:
            if in_mode == "videoonly":
                aug = None
            else:
                self._check_aug(aug, B, in_mode)
        eng = self._train_engine(B, T)
        self._sync_shadows()
        res = eng.forward(mode, a, v, bit) if xf is None and aug is None else eng.forward(mode, a, v, bit, xf or (None, None), aug)
        head = {OUT: eng.head_mm, OUT_A: eng.head_a, OUT_V: eng.head_v}[bit]
        x = res[bit]
        n = x.shape[0]
        y = labels.to(x.device, torch.float32).reshape(n, self.label_dim).contiguous()
        if not hasattr(eng, "loss_buf") or eng.loss_buf[0].numel() < n:
            eng.loss_buf = (torch.zeros(max(n, B * T), dtype=torch.float32, device=x.device), torch.zeros(1, dtype=torch.float32, device=x.device))
        rows, out = eng.loss_buf
        ops.cls_loss(x, y, n, self.label_dim, ops.CLS_BCE if loss == "BCE" else ops.CLS_CE, rows, out, dx=head.dlog)
        gmax = self._guard_max if guard is None else self._check_max_norm(guard)
        if self._accum_k is not None:
            self._micro_step(eng, cls_mode if mode != "mm_grad" else "mm_grad", bit, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, gmax)
            return out.clone()
        if self._dp or gmax is not None:
            self._dp_step(eng, cls_mode if mode != "mm_grad" else "mm_grad", bit, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, gmax)
            return out.clone()
        names = self._backward(eng, eng.token, cls_mode if mode != "mm_grad" else "mm_grad", bit if mode == "mm_grad" else (OUT_A if cls_mode == "audioonly" else OUT_V))
        self.adam_step(lr, head_lr, mm_lr, names, beta1, beta2, eps, weight_decay)
        return out.clone()

    def adam_step(self, lr, head_lr=1.0, mm_lr=1.0, names=None, beta1=0.95, beta2=0.999, eps=1e-8, weight_decay=5e-7):
        """torch.optim.Adam([base lr | mlp_head* lr * head_lr | mm_layer* lr * mm_lr], weight_decay=5e-7, betas=(0.95, 0.999)) of
        traintest_ft_base.py:78-83 over the gradients of the last backward (`names`: the parameters that got one; default: every trainable
        parameter whose .grad is set).  Parameters without a gradient are untouched and, as in torch, keep their own step count: one count
        per gradient class (grad_class), one launch per contiguous run of the arena."""
        from .. import ops
        a = self.arena
        self._check_not_accumulating("adam_step")
        if names is None:
            names = [n for n in self._trainable() if self._params[n].grad is not None and a.info[n].live]
        if not names:
            return
        if self._dps is not None and not self._dp:                 # guarded steps counted on the device: the counts come back first (a sync)
            self._drop_dp_state()
        lo0, hi0 = a.range[1]
        if self._opt is None:
            self._opt = {"m": torch.zeros(hi0 - lo0, device=a.p.device), "v": torch.zeros(hi0 - lo0, device=a.p.device), "step": {}}
        st = self._opt
        classes = {grad_class(n) for n in names}
        for c in classes:
            st["step"][c] = st["step"].get(c, 0) + 1
        mult = {"base": 1.0, "head": head_lr, "mm": mm_lr}
        self._rates = (lr, lr * head_lr, lr * mm_lr)
        spans = sorted((a.offset[n], a.offset[n] + _padded(a.info[n]),
                        lr * mult[param_group(n)], st["step"][grad_class(n)]) for n in names)
        runs = []
        for lo, hi, l, k in spans:
            if runs and runs[-1][1] == lo and runs[-1][2] == l and runs[-1][3] == k:
                runs[-1][1] = hi
            else:
                runs.append([lo, hi, l, k])
        for lo, hi, l, k in runs:
            ops.adam(a.p[lo:hi], a.g[lo:hi], st["m"][lo - lo0:hi - lo0], st["v"][lo - lo0:hi - lo0], a.pb[lo:hi], hi - lo, l, k, beta1, beta2, eps,
                     weight_decay)
        a.refresh_shadows(None, cast=False)
        for e in list(self._engines.values()) + list(self._train_engines.values()):
            e.refresh_heads()
        if a.with_grads:
            self._versions = sum(p._version for p in self._params.values())

    # ---- data-parallel fine-tuning ------------------------------------------------------------------------------
    def set_distributed(self, world, rank, comm=None):
        """comm: the collectives to use (comm.TorchDistComm = RCCL by default; tests inject their own).  With an inactive comm (world 1 and
        not forced on) nothing changes: train_step, adam_step and the autograd path run what they run without this call.
        Unlike DistributedDataParallel's constructor this does NOT broadcast rank 0's weights: the ranks must hold identical weights when
        they call it (the same init seed, or the same --pretrain_path) - from then on the step keeps them identical byte for byte.
        Step counts of data-parallel steps already taken move back to the host, so a second call (another comm) or a return to the
        single-process adam_step continues from them."""
        from ..comm import default_comm
        self._check_not_accumulating("set_distributed")
        self._world, self._rank = world, rank
        self._comm = comm if comm is not None else default_comm(world)
        assert self._comm.world == world and self._comm.rank == rank, "comm does not match (world, rank)"
        self._dp = getattr(self._comm, "active", world > 1)
        self._drop_dp_state()
        self._aug_st, self._aug_plans = None, {}                   # the rank is part of the augmentation key
        # the gradient all-reduce overlaps the backward: RCCL's kernels need compute units WHILE a persistent GEMM holds the chip
        # (CAVMAE_BASE.set_distributed; the knob is process-wide, AVSIAM_CU_RESERVE overrides)
        if self.arena.p.is_cuda and _lib.env_value("AVSIAM_CU_RESERVE") is None:
            overlap = os.environ.get("AVSIAM_DP_OVERLAP", "1") != "0"
            _lib.tuning_set("cu_reserve", 8 if (self._dp and overlap) else 0)

    # ---- the guarded step ---------------------------------------------------------------------------------------
    @staticmethod
    def _check_max_norm(max_norm):
        max_norm = float(max_norm)
        if not max_norm > 0:
            raise ValueError(f"max_norm must be > 0 (float('inf'): skip non-finite steps without clipping), not {max_norm}")
        return max_norm

    def set_grad_guard(self, max_norm=float("inf")):
        """Guard every train_step from now on: gradients clipped to the total norm `max_norm` (torch.nn.utils.clip_grad_norm_; the default
        inf never clips) and a step whose gradients hold inf or NaN skipped as a whole - weights, moments, bf16 shadows and step counts
        keep their bytes (what the reference's GradScaler.step does, traintest_ft_base.py:162-165).  All of it on the device, between the
        gradient all-reduce and Adam; data parallel, the norm is that of the rank-averaged gradients and every rank takes the same decision.
        set_grad_guard(None) removes the guard: the step counts move back to the host (a sync, unless a data-parallel comm is active) and
        train_step issues the calls it issued before.  The counters of guard_stats() start at the first guarded step."""
        if max_norm is None:
            self._guard_max = None
            if not self._dp and self._accum_k is None:         # (accumulating steps stay on the segment-table route, counts on the device)
                self._drop_dp_state()
            return
        self._guard_max = self._check_max_norm(max_norm)

    def guard_stats(self):
        """The guard's device block after the last guarded step, as host numbers.  SYNCHRONISES (one small copy behind everything queued on
        the stream): call it where the loop syncs anyway.  -> norm (the total norm of the gradients Adam was given, before clipping),
        norm_base / norm_head / norm_mm (per parameter group), coef (what the gradients were multiplied by; 0 on a skipped step),
        n_nonfinite (inf / NaN gradient elements of the last step), skipped (the last step), n_skipped, n_steps (since the first guarded
        step).  None before the first guarded step."""
        if self._guard is None:
            return None
        r = self._guard.read()
        scale = self._guard_scale if self._guard_scale is not None else (1.0 / self._world if self._dp else 1.0)   # (accumulated: 1 / (j * world))
        out = {"norm": r["norm"], "coef": r["coef"], "n_nonfinite": r["n_nonfinite"], "skipped": bool(r["skip"]), "n_skipped": r["n_skipped"],
               "n_steps": r["n_steps"]}
        for i, grp in enumerate(GROUPS):
            out["norm_" + grp] = math.sqrt(float(r["sumsq"][i])) * scale
        return out

    def _drop_dp_state(self):
        """forget the device state of the data-parallel step, keeping its step counts: the host dictionary is not maintained while ctl.step
        counts on the device, and _dp_state() / adam_step start from that dictionary"""
        if self._dps is not None and self._opt is not None:
            self._opt["step"] = self.optimizer_steps()
        self._dps = None

    def dp_schedule(self):
        """The ordered [a, b) messages of the data-parallel gradient all-reduce: a function of the arena layout alone, the same on every rank
        whatever branch runs or is frozen.  Order of the mm branch's backward: heads and fusion blocks, encoder blocks last to first, then what
        is left (embeddings, final norms)."""
        from ..comm import _union, fixed_schedule
        a = self.arena
        lo0, hi0 = a.range[1]
        span = lambda names: _union((a.offset[n], a.offset[n] + _padded(a.info[n])) for n in names)
        live = [n for n in a.names if a.info[n].live]
        units = span(n for n in live if param_group(n) != "base")
        for i in reversed(range(self.cfg.depth)):
            units += span(n for n in live if n.startswith(f"vit_base.blocks.{i}."))
        return fixed_schedule([tuple(u) for u in units], lo0, hi0)

    def dp_dead_ranges(self, classes):
        """[a, b) ranges of the trainable gradient range that a backward reaching the gradient classes `classes` never writes: every tensor of
        another class, and every frozen one.  They hold zeros after the step's zero-fill - final from the start (FixedScheduleReducer.begin)."""
        from ..comm import _union
        a = self.arena
        return [tuple(r) for r in _union((a.offset[n], a.offset[n] + _padded(a.info[n])) for n, p in self._params.items()
                                         if a.info[n].live and (not p.requires_grad or grad_class(n) not in classes))]

    def _adam_table(self, trainable):
        """ops.AdamTable over the live tensors among `trainable` (offsets from the start of the trainable range), the runs of equal
        (group, class) merged; None when there are none"""
        from .. import ops
        a = self.arena
        lo0, hi0 = a.range[1]
        spans = sorted((a.offset[n] - lo0, _padded(a.info[n]), GROUPS.index(param_group(n)), CLASSES.index(grad_class(n)))
                       for n in trainable if a.info[n].live)
        segs = []
        for lo, n, grp, cls in spans:
            if segs and segs[-1][0] + segs[-1][1] == lo and segs[-1][2:] == [grp, cls]:
                segs[-1][1] += n
            else:
                segs.append([lo, n, grp, cls])
        return ops.AdamTable(segs, len(CLASSES), hi0 - lo0, a.p.device) if segs else None

    def _dp_state(self):
        """Device state of the data-parallel step: avs_adam_ctl, the moments, the reducer, and - rebuilt when the trainable set changes - the
        segment table (runs of equal (group, class) merged; frozen tensors are in no segment)."""
        from .. import ops
        from ..comm import FixedScheduleReducer, _union
        a = self.arena
        dev = a.p.device
        lo0, hi0 = a.range[1]
        st = self._dps
        if st is None:
            if self._opt is None:
                self._opt = {"m": torch.zeros(hi0 - lo0, device=dev), "v": torch.zeros(hi0 - lo0, device=dev), "step": {}}
            ctl = ops.AdamCtl(dev)
            if self._opt["step"]:                                  # steps taken before set_distributed: the counts move to the device
                ctl.step.copy_(torch.tensor([self._opt["step"].get(c, 0) for c in CLASSES] + [0] * (ops.ADAM_TABLE_NCLS - len(CLASSES)),
                                            dtype=torch.int32))
            # (one rank, guarded: the same state without a reducer - liveness is then what this rank's branch reaches)
            red = FixedScheduleReducer(self._comm, a.g, self.dp_schedule(), tail=ctl.live) if self._dp else None
            st = self._dps = {"ctl": ctl, "trainable": None, "reducer": red, "dead": {}, "livevec": {}}
        trainable = tuple(self._trainable())
        if st["trainable"] != trainable:
            st["table"] = self._adam_table(trainable)
            st["trainable"], st["dead"] = trainable, {}
        return st

    def _dp_step(self, eng, cls_mode, bit, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm=None):
        """Backward with the fixed-schedule all-reduce, liveness as its last message, and the one-launch Adam.  No host synchronisation.
        max_norm (a guarded step): avs_grad_sumsq over the summed gradients, then the guarded Adam.  Without an active comm (one rank,
        guarded) there is no reducer: the same table, liveness set from the classes this branch reaches."""
        a = self.arena
        lo0, hi0 = a.range[1]
        st = self._dp_gradients(eng, cls_mode, bit)
        self._dp_apply(st, a.g[lo0:hi0], 1.0 / self._world if st["reducer"] is not None else 1.0, lr, head_lr, mm_lr, beta1, beta2, eps,
                       weight_decay, max_norm)

    def _dp_gradients(self, eng, cls_mode, bit):
        """The gradient half of the segment-table step: the zero-fill, the backward (with the reducer when a comm is active) and ctl.live of
        this step - the union over the ranks once the reducer has finished.  -> the step's device state (_dp_state)."""
        from .. import ops
        a = self.arena
        st = self._dp_state()
        ctl, red = st["ctl"], st["reducer"]
        reach = live_classes(cls_mode, bit)
        names = [n for n in st["trainable"] if grad_class(n) in reach and a.info[n].live]
        cls = frozenset(grad_class(n) for n in names)
        base = any(param_group(n) == "base" for n in names)
        if red is not None and cls not in st["dead"]:
            # what this rank's backward never writes: every tensor outside the classes it reaches, and the frozen ones
            st["dead"][cls] = self.dp_dead_ranges(cls)
        if cls not in st["livevec"]:
            st["livevec"][cls] = torch.tensor([1.0 if c in cls else 0.0 for c in CLASSES] + [0.0] * (ops.ADAM_TABLE_NCLS - len(CLASSES)),
                                              dtype=torch.float32).to(a.p.device)
        ops.timed("torch_zero_grads", lambda: a.zero_grad_range(1))          # the WHOLE range: other ranks' classes arrive in it
        if red is not None:
            red.begin(st["dead"][cls])
        eng.backward(eng.token, bit if names else 0, base=base, reducer=red)
        ctl.live.copy_(st["livevec"][cls])
        if red is not None:
            red.finish()
        return st

    def _dp_apply(self, st, g, scale, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm):
        """The optimizer half: the rates, the (guarded) one-launch Adam over the classes live in ctl with the gradients `g` (the arena's
        trainable range, or the accumulation buffer) scaled by `scale`, then the refreshes every step ends with."""
        from .. import ops
        a = self.arena
        lo0, hi0 = a.range[1]
        ctl = st["ctl"]
        self._rates = (lr, lr * head_lr, lr * mm_lr)
        self._guard_scale = scale
        if st["table"] is not None:
            ctl.set_lr(*self._rates)
            m, v = self._opt["m"], self._opt["v"]
            if max_norm is None:
                ops.adam_table(a.p[lo0:hi0], g, m, v, a.pb[lo0:hi0], st["table"], ctl, beta1, beta2, eps, weight_decay,
                               grad_scale=scale)
            else:
                if self._guard is None:
                    self._guard = ops.GradGuard(a.p.device)
                ops.grad_sumsq(g, st["table"], ctl, self._guard, grad_scale=scale, max_norm=max_norm)
                ops.adam_table_guarded(a.p[lo0:hi0], g, m, v, a.pb[lo0:hi0], st["table"], ctl, self._guard, beta1, beta2, eps,
                                       weight_decay, grad_scale=scale)
        a.refresh_shadows(None, cast=False)
        for e in list(self._engines.values()) + list(self._train_engines.values()):
            e.refresh_heads()
        if a.with_grads:
            self._versions = sum(p._version for p in self._params.values())

    # ---- gradient accumulation over micro-batches ---------------------------------------------------------------------------------
    def set_grad_accumulation(self, k):
        """k >= 2: every train_step from now on is a MICRO-step; the k-th applies the sum of the k gradients, divided by k (and by the world
        size), in one optimizer step - the step a batch k times as large would take, for a model whose activations bound the batch.  1 or
        None: no accumulation; the buffer is freed and train_step issues the calls it issued before.
        A micro-step takes the segment-table route of the guarded and data-parallel steps (``.grad`` stays None, the step counts live on
        the device): the zero-fill, the backward - with the all-reduce when a comm is active, every micro-step, as DistributedDataParallel
        does outside no_sync -, then avs_grad_accum from the gradient arena into an fp32 buffer over the trainable range (allocated at the
        first micro-step).  Which gradient classes the cycle reached is kept on the device: under mm_grad every micro-step may run another
        branch, and data parallel the set is the union over the ranks.  Micro-steps 1 .. k-1 launch nothing else - no Adam, no shadow or
        head refresh; weights, moments, shadows and step counts keep their bytes.  The k-th runs the (guarded) one-launch Adam over the
        union with ITS lr, head_lr, mm_lr, betas, eps, weight_decay and guard; every class of the union steps once.  Guarded, the norm is
        that of the averaged gradients, n_steps counts optimizer steps, and a non-finite gradient in ANY micro-step (inf and NaN survive
        the sum) skips the whole accumulated step.
        Every micro-step returns its own loss, the mean of its micro-batch; all micro-steps weigh 1 / k whatever their sizes.
        While micro-steps are pending this call, a change of the trainable set, adam_step, a backward of the autograd path,
        load_optimizer_state and set_distributed raise RuntimeError: apply_accumulated() first.  optimizer_state() does not hold a pending
        cycle - take checkpoints at cycle boundaries (the loop's epoch-end apply_accumulated guarantees one)."""
        self._check_not_accumulating("set_grad_accumulation")
        if k is None or (k == 1 and isinstance(k, int) and not isinstance(k, bool)):
            self._accum_k, self._acc = None, None
            if not self._dp and self._guard_max is None:
                self._drop_dp_state()
            return
        if isinstance(k, bool) or not isinstance(k, int) or k < 2:
            raise ValueError(f"set_grad_accumulation: k must be an integer >= 2 (1 or None: no accumulation), not {k!r}")
        self._accum_k = k

    def accum_state(self):
        """{"k": micro-steps per optimizer step (1: no accumulation), "pending": micro-steps accumulated and not yet applied}: host integers,
        no sync."""
        return {"k": self._accum_k or 1, "pending": self._acc["pending"] if self._acc is not None else 0}

    def accum_buffer(self):
        """The fp32 accumulation buffer over the trainable range (the offsets of the Adam moments), for tests and diagnostics; None before
        the first micro-step.  Meaningful on the segments of the classes the running cycle has reached; elsewhere it holds stale sums."""
        return self._acc["buf"] if self._acc is not None else None

    def _check_not_accumulating(self, what):
        if self._acc is not None and self._acc["pending"]:
            raise RuntimeError(f"CAVMAEFT_BASE.{what}: {self._acc['pending']} micro-step(s) of a gradient-accumulation cycle are pending; "
                               "apply them first (apply_accumulated)")

    def requires_grad_(self, requires_grad=True):
        self._check_not_accumulating("requires_grad_")
        return super().requires_grad_(requires_grad)

    def _accum_check_trainable(self, what):
        if self._acc is not None and self._acc["pending"] and self._acc["trainable"] != tuple(self._trainable()):
            raise RuntimeError(f"CAVMAEFT_BASE.{what}: the trainable set changed while {self._acc['pending']} micro-step(s) of a gradient-"
                               "accumulation cycle are pending; restore it and apply them first (apply_accumulated)")

    def _micro_step(self, eng, cls_mode, bit, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm):
        """One micro-step of a cycle of self._accum_k: the gradients of the segment-table route, accumulated; the k-th applies the cycle."""
        from .. import ops
        a = self.arena
        lo0, hi0 = a.range[1]
        self._accum_check_trainable("train_step")
        st = self._dp_gradients(eng, cls_mode, bit)
        if self._acc is None:
            self._acc = {"buf": torch.zeros(hi0 - lo0, dtype=torch.float32, device=a.p.device), "actl": ops.GradAccumCtl(a.p.device), "pending": 0,
                         "trainable": None}
        acc = self._acc
        first, last = acc["pending"] == 0, acc["pending"] + 1 >= self._accum_k
        if first:
            acc["trainable"] = st["trainable"]
        if st["table"] is not None:
            ops.grad_accum(acc["buf"], a.g[lo0:hi0], st["table"], st["ctl"], acc["actl"], first, last)
        acc["pending"] += 1
        if last:
            self._accum_apply(st, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm)

    def _accum_apply(self, st, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm):
        """ctl.live holds the cycle's union: one optimizer step over it with the accumulated gradients divided by the pending micro-steps
        (and the world size) - the quotient 1 / (j * world) taken in double and rounded once, where grad_scale becomes a float"""
        j = self._acc["pending"]
        world = self._world if st["reducer"] is not None else 1
        self._acc["pending"] = 0
        self._dp_apply(st, self._acc["buf"], 1.0 / (j * world), lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, max_norm)

    def apply_accumulated(self, lr, head_lr=1.0, mm_lr=1.0, beta1=0.95, beta2=0.999, eps=1e-8, weight_decay=5e-7, *, guard=None):
        """Apply the j pending micro-steps now, as one optimizer step with the gradients divided by j (and the world size): what the loop
        calls after the last batch of an epoch, so that no gradient crosses an epoch (or a checkpoint).  A no-op when none are pending.
        Data parallel every rank calls it at the same point (the ranks hold the same union: it was all-reduced micro-step by micro-step).
        guard: as in train_step."""
        if self._acc is None or not self._acc["pending"]:
            return
        self._accum_check_trainable("apply_accumulated")
        gmax = self._guard_max if guard is None else self._check_max_norm(guard)
        st = self._dp_state()
        actl = self._acc["actl"]
        st["ctl"].live.copy_(actl.live)                          # what a publishing micro-step would have left: the union so far
        actl.n_cycles.add_(1)
        self._accum_apply(st, lr, head_lr, mm_lr, beta1, beta2, eps, weight_decay, gmax)

    def optimizer_steps(self):
        """{gradient class: Adam updates it has had}.  Data parallel: copied from the device (synchronises)."""
        if self._dps is not None:
            steps = self._dps["ctl"].step.cpu().tolist()
            return {c: steps[i] for i, c in enumerate(CLASSES) if steps[i]}
        return dict(self._opt["step"]) if self._opt is not None else {}

    def optimizer_state(self):
        """The Adam state as plain CPU tensors (synchronises): moments over the trainable range, steps per gradient class (CLASSES order),
        the three rates of the last step.  None before the first step."""
        if self._opt is None:
            return None
        steps = self.optimizer_steps()
        return {"m": self._opt["m"].detach().cpu(), "v": self._opt["v"].detach().cpu(),
                "step": torch.tensor([steps.get(c, 0) for c in CLASSES], dtype=torch.int64),
                "lr": torch.tensor(self._rates if self._rates is not None else (0.0, 0.0, 0.0), dtype=torch.float64)}

    def load_optimizer_state(self, state):
        self._check_not_accumulating("load_optimizer_state")
        lo0, hi0 = self.arena.range[1]
        if state["m"].numel() != hi0 - lo0 or state["v"].numel() != hi0 - lo0 or state["step"].numel() != len(CLASSES):
            raise ValueError("load_optimizer_state: the state does not fit this model's trainable range / gradient classes")
        dev = self.arena.p.device
        steps = [int(x) for x in state["step"].tolist()]
        self._opt = {"m": state["m"].to(dev, torch.float32).clone(), "v": state["v"].to(dev, torch.float32).clone(),
                     "step": {c: k for c, k in zip(CLASSES, steps) if k}}
        self._rates = tuple(float(x) for x in state["lr"].tolist())
        self._dps = None                                           # (rebuilt from _opt at the next data-parallel step)

    def forward(self, a, v, mode, is_eval=False, *, input_xf=None, aug=None, exact=False):
        """a: [B, 1024, 128] fbank; v: [B, T, 3, 224, 224] frames (either may be None when the mode ignores it).
        Returns what the reference returns for the mode; any other mode returns None as there (no else branch).
        input_xf (extension, every mode): (ops.InputXf.audio(mean, std), ops.InputXf.frames()) - `a` is then the UN-normalised fbank and
        `v` uint8 frames as the reference's dataset holds them before its own arithmetic, normalised inside the kernels that read them.
        aug (extension, the training forms only): an ops.FtAug plan - SpecAugment masks, noise and time roll inside the audio patch gather
        (dataloader_ft.py:527-548, which the reference applies to the training set alone).  With input_xf=None the masks fall on the
        normalised `a` (masked cells take aug.fill).  Refused with is_eval=True, in an inference-only mode and on a model without gradients.
        exact (extension, every mode): the exact-fp32 forward (engine_exact / csrc/exact.hip) - fp32 operands on the f32-input MFMA, read from
        the fp32 master weights, with a fixed accumulation order: the logits are what an fp32 evaluation of the reference gives up to
        summation order, a clip's result does not depend on its batch, and two calls give the same bytes.  Always an inference output (no
        autograd node, whatever requires_grad says); refuses `aug`.  Slower than the bf16 path by the ratio of the matrix rates."""
        if mode not in MODES:
            return None
        if exact and aug is not None:
            raise ValueError("exact=True is an inference form: it takes no training augmentation (aug)")
        if not self.arena.p.is_cuda:
            raise _lib.AvsiamHipError("CAVMAEFT_BASE.forward needs a GPU: the path runs only on libavsiam_hip.so "
                                      "(no CPU/eager fallback). Move the model with .cuda() first.")
        _lib.load()
        if exact:
            with torch.no_grad():
                xf = self._input_xf(input_xf, mode)
                a, v, B, T = self._prepare(a, v, mode, xf)
                return self._run_inference(self._engine(B, T, exact=True), a, v, mode, is_eval, xf, T)      # (masters are read: no shadow sync)
        if torch.is_grad_enabled() and mode in TRAIN_MODES and not is_eval:        # every is_eval form stays inference-only
            trainable = self._trainable()
            if trainable:
                if self._dp:
                    raise RuntimeError("CAVMAEFT_BASE: the autograd path (forward + loss.backward()) is not synchronised between ranks; with "
                                       "set_distributed active, train with train_step (or evaluate under torch.no_grad() / is_eval=True)")
                xf = self._input_xf(input_xf, mode)
                a, v, B, T = self._prepare(a, v, mode, xf)
                if aug is not None:
                    self._check_aug(aug, B, mode)
                eng = self._train_engine(B, T)
                self._sync_shadows()
                return _FtNode.apply(self._params[trainable[0]], self, eng, mode, a, v, xf, aug)
        if aug is not None:
            raise ValueError("aug is a training augmentation (the reference applies it to the training set only): it needs a trainable mode "
                             f"({', '.join(TRAIN_MODES)}) with is_eval=False, grad mode on and a parameter that requires a gradient")
        xf = self._input_xf(input_xf, mode)
        a, v, B, T = self._prepare(a, v, mode, xf)
        eng = self._engine(B, T)
        if self._shadow_dirty or self.arena.with_grads:
            self._sync_shadows()
        return self._run_inference(eng, a, v, mode, is_eval, xf, T)

    def _run_inference(self, eng, a, v, mode, is_eval, xf, T):
        """the mode's engine call and the reference's output shapes (`eng`: the bf16 or the exact-fp32 FtForward)"""
        xfa = () if xf is None else (xf,)                          # (no transform: the engine calls of before, argument for argument)
        if mode == "audioonly":
            out = eng.audioonly(a, *xfa).clone()
            return out.unsqueeze(1) if is_eval else out                                    # :845-847
        if mode == "videoonly":
            return eng.videoonly(v, *xfa).clone().squeeze(1)                               # :865
        if mode == "retrieval":
            if T <= 5:
                raise IndexError(f"retrieval returns frame 5 of each clip (cav_mae_base.py:892); got {T} frames")
            ta, tv = eng.retrieval(a, v, **({} if xf is None else {"xf": xf}))
            return ta.clone(), tv.clone()
        res = eng.mm_grad(a, v, bool(is_eval), *xfa)
        if is_eval:
            return res.clone()
        return tuple(r.clone() for r in res)

    @torch.no_grad()
    def retrieval_features(self, a, v, frame_index=5, out_a=None, out_v=None, exact=False):
        """Clip-level retrieval features: what the retrieval experiment makes of ``forward(a, v, "retrieval")`` (src/retrieval.py:70-78: mean
        over the tokens, L2 normalisation) -> (audio [B, D], video [B, D]) fp32 unit vectors.  Only frame `frame_index` of every clip goes
        through the encoder (frames are independent sequences, cav_mae_base.py:901-920), so any T > frame_index is accepted and a ten-frame
        clip costs 512 + 196 encoder rows instead of 512 + 1960.  out_a / out_v: fp32 [B, D] contiguous device tensors to write into
        (row slices of a dataset-level feature buffer); None: new tensors.  exact: the exact-fp32 forward (see forward())."""
        if not self.arena.p.is_cuda:
            raise _lib.AvsiamHipError("CAVMAEFT_BASE.retrieval_features needs a GPU: the path runs only on libavsiam_hip.so "
                                      "(no CPU/eager fallback). Move the model with .cuda() first.")
        _lib.load()
        frame_index = int(frame_index)
        a, v, B, T = self._prepare(a, v, "retrieval")
        if not 0 <= frame_index < T:
            raise IndexError(f"retrieval returns frame {frame_index} of each clip (cav_mae_base.py:892); got {T} frames")
        dev, D = self.arena.p.device, self.cfg.embed_dim
        outs = []
        for name, t in (("out_a", out_a), ("out_v", out_v)):
            if t is None:
                t = torch.empty((B, D), dtype=torch.float32, device=dev)
            elif t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (B, D) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous fp32 [{B}, {D}] tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            outs.append(t)
        if exact:
            self._engine(B, T, exact=True).retrieval_feats(a, v, outs[0], outs[1], frame_index)
            return outs[0], outs[1]
        eng = self._engine(B, T)
        if self._shadow_dirty or self.arena.with_grads:
            self._sync_shadows()
        eng.retrieval_feats(a, v, outs[0], outs[1], frame_index)
        return outs[0], outs[1]


CAVMAEFT = CAVMAEFT_BASE      # (/root/reference/src/models/__init__.py:8 exports the name; same signature family)


class CAVMAEFT_LARGE(CAVMAEFT_BASE):
    """``models.CAVMAEFT_LARGE`` (/root/reference/src/models/__init__.py:9; source file absent from the snapshot): the same inference modes on
    the ViT-L/16 skeleton (``config.vit_large()``); oracle-only parity (oracle/ref_cpu.py::ft_forward is shape-generic)."""

    def __init__(self, label_dim, *args, cfg: AVSiamConfig = None, **kw):
        from ..config import vit_large
        if cfg is not None and (cfg.embed_dim, cfg.num_heads) != (1024, 16):
            raise ValueError("CAVMAEFT_LARGE: cfg must be a ViT-L shape (config.vit_large(...))")
        super().__init__(label_dim, *args, cfg=cfg if cfg is not None else vit_large(), **kw)


class CAVMAEFT_HUGE(CAVMAEFT_BASE):
    """``models.CAVMAEFT_HUGE`` (/root/reference/src/models/__init__.py:13; source file absent): ViT-H/14 skeleton (``config.vit_huge14()``)."""

    def __init__(self, label_dim, *args, cfg: AVSiamConfig = None, **kw):
        from ..config import vit_huge14
        if cfg is not None and (cfg.embed_dim, cfg.num_heads) != (1280, 16):
            raise ValueError("CAVMAEFT_HUGE: cfg must be a ViT-H shape (config.vit_huge14(...) / config.vit_huge(...))")
        super().__init__(label_dim, *args, cfg=cfg if cfg is not None else vit_huge14(), **kw)
