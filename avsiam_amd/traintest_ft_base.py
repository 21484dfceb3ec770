"""Fine-tuning loop of the reference (src/traintest_ft_base.py) on the HIP path.

``train_step`` is the fused step (forward of the loss's branch, the HIP classification loss, the hand-scheduled backward and the HIP Adam of
the three parameter groups, no host sync); ``train`` / ``validate`` keep the reference's signatures and returns, branch draw (:133-160), losses
(:105-110), schedulers (:91-97), freeze_base (:68-71) and artefacts (models/audio_model.{epoch}.pth, best_audio_model.pth, result.csv).
Deliberate differences: the reference's stray forward outside autocast (:143, which would also break every mode but mm_grad) is not
reproduced; weight averaging (--wa) is not implemented; mixup only from waveforms (below).
Augmentation (dataloader_ft.py:527-548: SpecAugment masks, noise, time roll - training batches only): ``train`` draws one plan per step on the
device (``model.draw_aug`` from args.freqm / timem / noise) and the step applies it inside the audio patch gather; ``validate`` and
``evaluate_frames`` never augment and never touch the draw state.  args.raw_input: the loaders yield un-normalised fbank and uint8 frames,
normalised inside the gathers (args.dataset_mean / dataset_std).  Mixup is not a function of a [B, T, F] batch of spectrograms - the reference
mixes waveforms before the fbank (dataloader_ft.py:321-325), mixes frames with a second weight (:457-458) and draws the partner from the whole
dataset (:400-417) - so ``train`` itself never mixes: it lives where the waveforms are, in ``SyntheticWaveFtLoader`` (the launcher's
--wave-input), which runs the device fbank (``ops.kaldi_fbank``: the mix inside its sample read), ``ops.mix_frames`` and
``preprocess.mixup_labels`` and hands ``train`` the (a, v, labels) it always took.
Data parallel (the model's set_distributed with an active comm; the reference wraps the model in DistributedDataParallel(
find_unused_parameters=True), :91-92): every rank draws its own branch and trains on its own shard, the fused step sums the gradients in a
rank-independent schedule and steps what any rank reached (CAVMAEFT_BASE.train_step); ``validate`` gathers the predictions and targets of
all ranks (distributed_concat, :22-27); rank 0 alone writes checkpoints, result.csv and the prints.  Verified with gloo ranks sharing one
GPU and with one rank's collectives forced on; no run with more than one rank on RCCL exists.

Metrics (mAP, mAUC, acc).  ``calculate_stats`` is the host path and the default: numpy on the [N, C] sigmoid outputs copied from the device.
``calculate_stats_device`` (``validate`` with ``args.device_metrics``) keeps outputs and targets on the device: the HIP counting kernel
(``ops.classification_stats``) returns exact integer counts per class, one small copy brings them to the host, and the two divisions per class
happen there in float64.  The two paths define AUC identically; AP differs where scores tie: the device path groups equal scores into one
threshold - the definition of the reference's sklearn ``average_precision_score`` - while ``_average_precision`` ranks tied scores in sample
order.  Both give NaN for a class without positives (auc: also without negatives), which ``train`` averages over with ``nanmean``.
``evaluate_frames`` is the reference launcher's multi-frame protocol (run_cavmae_ft_base.py:326-369): the metric of every frame's predictions
and of their mean over the frames, from one forward pass and one kernel call, written to exp_dir/mul_frame_res.csv.
"""
import os
import random
import statistics
import time

import numpy as np
import torch

from .models.cav_mae_ft import param_group


def draw_branch(prob):
    """traintest_ft_base.py:153-160: prob > 0.5 -> loss on out, prob < 0.25 -> out_a, otherwise out_v"""
    if prob > 0.5:
        return "mm"
    if prob < 0.25:
        return "a"
    return "v"


def train_step(model, a, v, labels, lr, ftmode, branch=None, loss="BCE", head_lr=50.0, mm_lr=None, input_xf=None, aug=None):
    """One fused step; -> the loss (device tensor [1]).  mm_lr None -> head_lr, as the reference's default --mm_lr None would fail
    (lr * None) and every launcher passes it.  input_xf / aug: CAVMAEFT_BASE.train_step."""
    extra = {k: x for k, x in (("input_xf", input_xf), ("aug", aug)) if x is not None}
    return model.train_step(a, v, labels, lr, ftmode, branch=branch, loss=loss, head_lr=head_lr, mm_lr=head_lr if mm_lr is None else mm_lr, **extra)


def guard_max_norm(args):
    """-> the max_norm of the guarded step the launcher's flags ask for: --clip-grad-norm X gives X (and skips non-finite steps, as every
    guarded step does), --skip-nonfinite alone inf (never clips), neither None (no guard: the plain step)"""
    clip = getattr(args, "clip_grad_norm", None)
    if clip is not None:
        if not float(clip) > 0:
            raise SystemExit(f"--clip-grad-norm {clip}: a total gradient norm > 0")
        return float(clip)
    return float("inf") if getattr(args, "skip_nonfinite", False) else None


def guard_diverged(steps, skipped):
    """more than half of the steps since the last print were skipped for non-finite gradients"""
    return steps > 0 and 2 * skipped > steps


def accum_steps_of(args):
    """-> the batches per optimizer step the launcher's --accum-steps asks for (absent: 1, no accumulation)"""
    k = getattr(args, "accum_steps", 1)
    k = 1 if k is None else k
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise SystemExit(f"--accum-steps {k}: the batches per optimizer step, an integer >= 1 (1: no accumulation)")
    return k


def input_xf_of(args):
    """the raw-input transforms of a run (args.raw_input): (InputXf.audio(dataset_mean, dataset_std), InputXf.frames()), else None"""
    if not getattr(args, "raw_input", False):
        return None
    from .ops import InputXf
    return InputXf.audio(getattr(args, "dataset_mean", -5.081), getattr(args, "dataset_std", 4.4849)), InputXf.frames()


def apply_freeze_base(model, freeze):
    for name, p in model.named_parameters():
        p.requires_grad_(not (freeze and param_group(name) == "base"))


# ---- metrics (numpy; the reference's utilities.calculate_stats uses sklearn) -----------------------------------------------
def _average_precision(y, s):
    order = np.argsort(-s, kind="stable")
    y = y[order]
    npos = y.sum()
    if npos == 0:
        return np.nan
    hits = np.cumsum(y)
    prec = hits / np.arange(1, len(y) + 1)
    return float((prec * y).sum() / npos)


def _auc(y, s):
    npos, nneg = y.sum(), len(y) - y.sum()
    if npos == 0 or nneg == 0:
        return np.nan
    order = np.argsort(s, kind="stable")
    ranks = np.empty(len(s))
    ss = s[order]
    i = 0
    while i < len(ss):                                    # average ranks of ties
        j = i
        while j + 1 < len(ss) and ss[j + 1] == ss[i]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2 + 1
        i = j + 1
    return float((ranks[y > 0].sum() - npos * (npos + 1) / 2) / (npos * nneg))


def calculate_stats(output, target):
    """Per class {'AP', 'auc', 'acc'} as the reference's utilities.stats.calculate_stats (acc: top-1 of the argmaxes, class-independent)."""
    target = (np.asarray(target) > 0.5).astype(np.float64)
    output = np.asarray(output, dtype=np.float64)
    acc = float(np.mean(np.argmax(target, 1) == np.argmax(output, 1)))
    return [{"AP": _average_precision(target[:, k], output[:, k]), "auc": _auc(target[:, k], output[:, k]), "acc": acc}
            for k in range(target.shape[1])]


def _stats_from_counts(n_pos, auc_num, ap_sum, n_correct, N):
    P = n_pos.astype(np.float64)
    Nn = N - P
    with np.errstate(divide="ignore", invalid="ignore"):
        ap = np.where(P > 0, ap_sum / P, np.nan)
        auc = np.where((P > 0) & (Nn > 0), auc_num.astype(np.float64) / (2.0 * P * Nn), np.nan)
    acc = float(n_correct) / N
    return [{"AP": float(ap[k]), "auc": float(auc[k]), "acc": acc} for k in range(len(P))]


def calculate_stats_device(output, target):
    """calculate_stats without leaving the device: output fp32 [N, C] (or [S, N, C]: S prediction sets against one target) and target
    [N, C] are device tensors; -> the same list of {'AP', 'auc', 'acc'} per class (a list of S such lists for a 3-D output).
    AP = ap_sum / P and auc = auc_num / (2 P Nn) in float64 from the kernel's counts (ops.classification_stats), after ONE device-to-host copy
    of the packed per-class results.  AP is NaN for P = 0, auc for P = 0 or Nn = 0 - this module's convention, as calculate_stats.  Equal
    scores share one threshold in AP (sklearn's definition; see the module docstring).  A NaN among the outputs raises ValueError."""
    from . import ops
    res = ops.classification_stats(output.float(), target.float())
    S = 1 if output.dim() == 2 else output.shape[0]
    N, C = target.shape
    h = {k: v.numpy() for k, v in ops.cls_stats_views(res["packed"].cpu(), S, C).items()}
    if h["n_nonfinite"].any():
        raise ValueError(f"calculate_stats_device: {int(h['n_nonfinite'].sum())} NaN value(s) among the outputs (per set: {h['n_nonfinite'].tolist()})")
    sets = [_stats_from_counts(h["n_pos"][s], h["auc_num"][s], h["ap_sum"][s], h["n_correct"][s], N) for s in range(S)]
    return sets[0] if output.dim() == 2 else sets


def stats_summary(stats):
    """-> {'mAP', 'mAUC', 'd_prime', 'acc'} of a per-class stats list: nan-means over the classes, d' = sqrt(2) * Phi^-1(mAUC) (the reference's
    utilities.stats.d_prime; NaN where mAUC is not inside (0, 1))."""
    mAP = float(np.nanmean([s["AP"] for s in stats]))
    mAUC = float(np.nanmean([s["auc"] for s in stats]))
    d = statistics.NormalDist().inv_cdf(mAUC) * np.sqrt(2.0) if 0.0 < mAUC < 1.0 else float("nan")
    return {"mAP": mAP, "mAUC": mAUC, "d_prime": float(d), "acc": stats[0]["acc"]}


def validate(audio_model, val_loader, val_sampler, args, output_pred=False):
    """validate of the reference (:292-350): no-grad forward in args.ftmode_test with is_eval=True (mm_grad: one joint logit row per frame of
    10-frame clips), loss = args.loss on the mean over dim 1 per batch, sigmoid of the outputs, stats of their mean over dim 1.
    -> (stats, loss), or (stats, sigmoid outputs, targets) with output_pred - as the reference.
    Differences, deliberate: args.ftmode_test None (the launchers do not pass it; the reference would then select no mode and fail) falls back to
    args.ftmode; a two-dimensional output (videoonly with one frame squeezes its frame axis, :865) gets that axis back before the mean, where
    the reference would average over the classes.  args.device_metrics (absent: False): the stats
    come from calculate_stats_device, and no [N, C] tensor is copied to the host.  args.exact_eval (absent: False): the forwards run on the
    exact-fp32 path (forward(..., exact=True)); evaluate_frames goes through here and follows it.
    Data parallel (the model has an active comm): predictions and targets of all ranks are gathered rank-major and truncated to
    len(val_sampler.dataset) when a sampler is given (distributed_concat, :22-27); every rank computes the same statistics; the loss stays
    this rank's own mean, as in the reference."""
    device = audio_model.arena.p.device
    mode = getattr(args, "ftmode_test", None) or args.ftmode
    loss_fn = torch.nn.BCEWithLogitsLoss() if args.loss == "BCE" else torch.nn.CrossEntropyLoss()
    outs, tgts, losses = [], [], []
    xf = input_xf_of(args)
    extra = {"input_xf": xf} if xf is not None else {}     # never an augmentation: the reference augments the training set only
    if getattr(args, "exact_eval", False):
        extra["exact"] = True
    with torch.no_grad():
        for a_input, v_input, labels in val_loader:
            out = audio_model(a_input.to(device), v_input.to(device), mode, is_eval=True, **extra)
            if out.dim() == 2:
                out = out.unsqueeze(1)
            labels = labels.to(device)
            losses.append(loss_fn(out.mean(dim=1), labels))
            outs.append(out)
            tgts.append(labels)
    loss = float(torch.stack(losses).mean()) if losses else float("nan")
    audio_output = torch.sigmoid(torch.cat(outs).float())
    target = torch.cat(tgts).float()
    comm = getattr(audio_model, "_comm", None)
    if comm is not None and getattr(audio_model, "_dp", False):
        limit = len(val_sampler.dataset) if val_sampler is not None else None
        audio_output, target = distributed_concat(comm, audio_output, limit), distributed_concat(comm, target, limit)
    if getattr(args, "device_metrics", False):
        stats = calculate_stats_device(audio_output.mean(dim=1), target)
    else:
        stats = calculate_stats(audio_output.mean(dim=1).cpu().numpy(), target.cpu().numpy())
    if output_pred:
        return stats, audio_output, target
    return stats, loss


def distributed_concat(comm, t, num_total_examples=None):
    """:22-27 of the reference: every rank's `t` (equal shapes) concatenated rank-major along dim 0, truncated to num_total_examples (the
    sampler pads the last shard)."""
    t = t.contiguous()
    out = torch.empty((comm.world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    comm.all_gather(out.view(-1), t.view(-1))
    return out if num_total_examples is None else out[:num_total_examples]


def evaluate_frames(audio_model, loader, args):
    """The multi-frame evaluation of the reference's launcher (run_cavmae_ft_base.py:326-369): args.metrics ('mAP' or 'acc') of every
    frame's predictions, then of the ensemble - the mean of the sigmoid outputs over the frames.  One validate(..., output_pred=True) pass in
    the multi-frame test mode gives the outputs [N, F, C]; ONE ops.classification_stats call scores the F + 1 prediction sets.
    -> list of F + 1 floats, also written to exp_dir/mul_frame_res.csv.
    Differences, deliberate: the reference runs one pass over the data per frame and applies a second sigmoid (or a softmax) to outputs that
    validate already passed through one; here the sigmoid outputs are scored as they are.  mAP is the nan-mean over the classes."""
    _, out, target = validate(audio_model, loader, None, args, output_pred=True)
    if out.dim() != 3 or out.shape[1] < 2:
        raise ValueError(f"evaluate_frames: expected per-frame outputs [N, F, C] with F > 1, got {tuple(out.shape)} (test mode mm_grad with multi-frame clips)")
    sets = torch.cat([out.permute(1, 0, 2), out.mean(dim=1).unsqueeze(0)]).contiguous()
    metric = getattr(args, "metrics", "mAP")
    res = [s[0]["acc"] if metric == "acc" else float(np.nanmean([c["AP"] for c in s])) for s in calculate_stats_device(sets, target)]
    for f, r in enumerate(res[:-1]):
        print(f"{metric} of frame {f} is {r:.4f}", flush=True)
    print(f"multi-frame {metric} is {res[-1]:.4f}", flush=True)
    if getattr(audio_model, "_rank", 0) == 0:             # (data parallel: every rank holds the gathered predictions, rank 0 writes)
        os.makedirs(args.exp_dir, exist_ok=True)
        np.savetxt(os.path.join(args.exp_dir, "mul_frame_res.csv"), res, delimiter=",")
    return res


class SyntheticFtLoader:
    """AudioSet-shaped synthetic clips (no dataset here): a ~ N(0,1) [B, target_length, 128], v ~ N(0,1) [B, frames, 3, 224, 224] and
    label-smoothed multi-hot labels (dataloader.py: 1 - label_smooth on the positives, label_smooth / n_class elsewhere).
    raw=True yields what the reference's dataset holds BEFORE its normalisation, as traintest_cavmae_base.SyntheticAVLoader does:
    un-normalised fbank (AudioSet's mean / std) and uint8 frames, for a consumer that passes input_xf."""

    def __init__(self, cfg, batch_size, steps, n_class, device, seed=87, label_smooth=0.1, frames=1, raw=False):
        import dataclasses
        from .weights import synth_inputs
        a, v = synth_inputs(dataclasses.replace(cfg, frames=frames), batch_size, seed)
        if raw:
            a = a * 4.4849 - 5.081
            v = (v * 0.25 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8)
        self.raw = raw
        g = torch.Generator().manual_seed(seed)
        hot = (torch.rand(batch_size, n_class, generator=g) < 0.02).float()
        hot[torch.arange(batch_size), torch.randint(0, n_class, (batch_size,), generator=g)] = 1.0
        y = hot * (1.0 - label_smooth) + label_smooth / n_class
        self.a, self.v, self.y, self.steps = a.to(device), (v.unsqueeze(1) if frames == 1 else v).to(device), y.to(device), steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.a, self.v, self.y


class SyntheticWaveFtLoader:
    """What a decoder produces, synthetic (``--wave-input``): 16 kHz float32 waveforms [B, 160 000] with per-batch lengths drawn in 9.0 - 10.0 s
    (so the padding to ``cfg.audio_len`` rows is exercised), uint8 frames [B, frames, 3, H, W] and multi-hot labels; with ``mixup`` p > 0 also
    a partner clip per sample (the batch rolled by one; choosing partners from a dataset stays a real loader's job).  The per-sample draws stay
    on the host, as in the reference's Dataset (dataloader_ft.py:420-424, 457): mixed with probability p, lambda ~ Beta(10, 10), an independent
    uniform frame weight - from a numpy Generator seeded by ``seed`` (per rank); the B scalars travel with the batch.
    Iterating runs the front end on the device and yields what ``train`` / ``validate`` take, (a, v, labels):
      a       ``ops.kaldi_fbank(wave, lengths, partner=..., lam=..., norm=(mean, std))`` - the waveform mixup inside the kernel's sample read
      v       ``ops.mix_frames`` (training with mixup) or ``preprocess.normalize_frames``
      labels  ``preprocess.mixup_labels`` (:470-475; unmixed rows: the plain smoothed labels)
    ``a`` is the NORMALISED fbank: ``train`` then applies SpecAugment / noise / roll through ``aug`` with fill = (0 - mean) / std - the
    reference's order, SpecAugment on the un-normalised fbank, normalisation, noise, roll.  train=False (validation): lam None, no mixing.
    frame_size=(H, W): the uint8 frames stay at the decoded size [B, frames, 3, H, W]; every batch draws a size per clip (and per partner) from
    FRAME_CROPS of (H, W) - the full frame or a narrower crop, so one padded buffer holds clips of several sizes - and ``v`` comes from
    ``ops.resize_frames`` (:136-139, 434-459: / 255, antialiased bicubic Resize to the model's size, Normalize, the mix with ``weight``); the
    sizes are in ``last_draw`` as ``sizes`` / ``partner_sizes``.  None: frames at the model's size, as above.
    sample_rate=R or [R, ...] (cycled over the clips of a batch), channels=C: the audio stays as decoded, float32 [B, C, samples * max R / 16 000]
    at each clip's own rate, the drawn lengths scaled to it (``src_lengths`` / ``partner_src_lengths`` in ``last_draw``); every batch runs
    ``ops.resample_wave`` (:272-277, 298-306: windowed-sinc resample to 16 kHz, channel mean) on the clips and on the partners, each by its own
    rate, and hands the 16 kHz audio and its device-side lengths to the fbank call above.  None: the 16 kHz mono waveforms of before."""

    FRAME_CROPS = ((1.0, 1.0), (1.0, 0.75))                  # (h, w) fractions of frame_size a clip's size is drawn from

    def __init__(self, cfg, batch_size, steps, n_class, device, seed=87, label_smooth=0.1, frames=1, mixup=0.0, norm=(-5.081, 4.4849), train=True,
                 samples=160000, frame_size=None, sample_rate=None, channels=1):
        g = torch.Generator().manual_seed(seed)
        B = batch_size
        self.wave = (torch.randn(B, samples, generator=g) * 0.1).to(device)
        self.rates = None
        if sample_rate is None:
            if int(channels) != 1:
                raise ValueError("SyntheticWaveFtLoader: channels names the decoded audio of sample_rate=: pass a sample rate with it")
        else:
            sr = [sample_rate] if not hasattr(sample_rate, "__len__") else list(sample_rate)
            if not sr or any(isinstance(r, bool) or int(r) != r or int(r) < 1 for r in sr) or not 1 <= int(channels) <= 8:
                raise ValueError(f"SyntheticWaveFtLoader: sample_rate {sample_rate!r} (positive integers), channels {channels!r} (1 .. 8)")
            self.rates = [int(sr[b % len(sr)]) for b in range(B)]
            src = max(-((-samples * r) // 16000) for r in self.rates)
            gs = torch.Generator().manual_seed(seed + 7919)      # its own stream: the frames and labels below are those of sample_rate=None
            self.wave = (torch.randn(B, int(channels), src, generator=gs) * 0.1).to(device)
        self.frame_size = None if frame_size is None else (int(frame_size[0]), int(frame_size[1]))
        self.img_size = cfg.img_size
        fh, fw = self.frame_size or (cfg.img_size, cfg.img_size)
        self.v = (torch.randn(B, frames, cfg.in_chans, fh, fw, generator=g) * 0.25 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8).to(device)
        hot = (torch.rand(B, n_class, generator=g) < 0.02).float()
        hot[torch.arange(B), torch.randint(0, n_class, (B,), generator=g)] = 1.0
        self.hot = hot.to(device)
        self.mixup = float(mixup) if train else 0.0
        if self.mixup > 0:
            self.wave2, self.v2, self.hot2 = (torch.roll(t, 1, 0).contiguous() for t in (self.wave, self.v, self.hot))
            self.rates2 = None if self.rates is None else self.rates[-1:] + self.rates[:-1]
        self.rng = np.random.default_rng(seed)
        self.steps, self.samples, self.norm, self.label_smooth, self.T = steps, samples, norm, label_smooth, cfg.audio_len
        self.last_draw = None

    def __len__(self):
        return self.steps

    def draw(self):
        """the host draws of one batch -> dict of numpy arrays: lengths (and partner_lengths, lam, weight under mixup; lam < 0: not mixed)"""
        B = self.wave.shape[0]
        d = {"lengths": self.rng.integers(int(0.9 * self.samples), self.samples + 1, B).astype(np.int32)}
        if self.mixup > 0:
            mixed = self.rng.random(B) < self.mixup
            d["partner_lengths"] = self.rng.integers(int(0.9 * self.samples), self.samples + 1, B).astype(np.int32)
            d["lam"] = np.where(mixed, self.rng.beta(10, 10, B), -1.0).astype(np.float32)
            d["weight"] = np.where(mixed, self.rng.random(B), 1.0).astype(np.float32)
        if self.rates is not None:                           # (no draw of its own: the 16 kHz lengths at each clip's rate)
            d["src_lengths"] = (d["lengths"].astype(np.int64) * np.asarray(self.rates) // 16000).astype(np.int32)
            if self.mixup > 0:
                d["partner_src_lengths"] = (d["partner_lengths"].astype(np.int64) * np.asarray(self.rates2) // 16000).astype(np.int32)
        if self.frame_size is not None:                      # (drawn last: the draws above are those of frame_size=None)
            crops = np.array([[max(1, round(self.frame_size[0] * fh)), max(1, round(self.frame_size[1] * fw))] for fh, fw in self.FRAME_CROPS], dtype=np.int32)
            d["sizes"] = crops[self.rng.integers(0, len(crops), B)]
            if self.mixup > 0:
                d["partner_sizes"] = crops[self.rng.integers(0, len(crops), B)]
        return d

    def __iter__(self):
        from . import ops, preprocess
        for _ in range(self.steps):
            d = self.last_draw = self.draw()
            wave, lengths = self.wave, d["lengths"]
            wave2, lengths2 = (self.wave2, d["partner_lengths"]) if self.mixup > 0 else (None, None)
            if self.rates is not None:
                wave, lengths = ops.resample_wave(self.wave, self.rates, d["src_lengths"])
                if self.mixup > 0:
                    wave2, lengths2 = ops.resample_wave(self.wave2, self.rates2, d["partner_src_lengths"])
            if self.mixup > 0:
                a = ops.kaldi_fbank(wave, lengths, partner=wave2, partner_lengths=lengths2, lam=d["lam"], target_length=self.T, norm=self.norm)
                v = (ops.mix_frames(self.v, self.v2, d["weight"]) if self.frame_size is None else
                     ops.resize_frames(self.v, d["sizes"], partner=self.v2, partner_sizes=d["partner_sizes"], weight=d["weight"], size=self.img_size))
                y = preprocess.mixup_labels(self.hot, self.hot2, torch.from_numpy(d["lam"]).to(self.hot.device), self.label_smooth)
            else:
                a = ops.kaldi_fbank(wave, lengths, target_length=self.T, norm=self.norm)
                v = preprocess.normalize_frames(self.v) if self.frame_size is None else ops.resize_frames(self.v, d["sizes"], size=self.img_size)
                y = preprocess.mixup_labels(self.hot, None, -1.0, self.label_smooth)
            yield a, v, y


class _LrHolder:
    """The parameter groups the reference's schedulers drive (base, mlp, mm: :78-83); train_step reads the three rates back."""

    def __init__(self, lr, head_lr, mm_lr):
        self._p = torch.nn.Parameter(torch.zeros(1))
        self.opt = torch.optim.SGD([{"params": [self._p], "lr": lr}, {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr * head_lr},
                                    {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr * mm_lr}], lr=lr)

    def rates(self):
        base, head, mm = (g["lr"] for g in self.opt.param_groups)
        return base, head / base if base else 0.0, mm / base if base else 0.0


def train(audio_model, train_loader, test_loader, test_sampler, args):
    """train of the reference (:29-290) with the fused step.  args: ftmode, loss, lr, head_lr, mm_lr, freeze_base, n_epochs, lr_adapt,
    lr_patience, lrscheduler_start / _step / _decay, metrics, exp_dir, save_model, n_print_steps; optional freqm, timem, noise (the
    per-step augmentation of the training batches), raw_input with dataset_mean / dataset_std; optional clip_grad_norm (a max_norm) and
    skip_nonfinite: the guarded step (CAVMAEFT_BASE.set_grad_guard) - at print steps, where the loss is read anyway, the gradient norm, the
    clipping coefficient and the steps skipped so far are printed too, and a run that skipped more than half of the steps since the last
    print ends with the reference's "training diverged..." (:184-186; there a NaN loss average) and "diverged": True in the result.
    Optional accum_steps K > 1 (CAVMAEFT_BASE.set_grad_accumulation): every batch is a micro-step, every K-th takes the optimizer step, and
    what is pending after the last batch of an epoch is applied there with the epoch's rates - validation, the checkpoint and the next
    epoch's rates all meet a cycle boundary.  global_step keeps counting batches, as the reference's loop does; the guard's counters (and
    so the "diverged" rule) count optimizer steps."""
    max_norm = guard_max_norm(args)
    if max_norm is not None:
        audio_model.set_grad_guard(max_norm)
    world = getattr(audio_model, "_world", 1)
    if getattr(args, "world_size", 1) > 1 and world != args.world_size:
        raise SystemExit(f"data-parallel fine-tuning: args.world_size is {args.world_size} but the model's collectives are set for {world} rank(s) "
                         "(call model.set_distributed(world, rank) first, as run_cavmae_ft_base.main does under torchrun)")
    master = getattr(audio_model, "_rank", 0) == 0            # rank 0 alone writes checkpoints, result.csv and the prints
    say = print if master else (lambda *a, **k: None)
    exp_dir = args.exp_dir
    if master:
        os.makedirs(os.path.join(exp_dir, "models"), exist_ok=True)
    apply_freeze_base(audio_model, bool(getattr(args, "freeze_base", False)))
    accum = accum_steps_of(args)
    if accum > 1:
        audio_model.set_grad_accumulation(accum)
    mm_lr = args.mm_lr if getattr(args, "mm_lr", None) is not None else args.head_lr
    hold = _LrHolder(args.lr, args.head_lr, mm_lr)
    if getattr(args, "lr_adapt", False):
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(hold.opt, mode="max", factor=0.5, patience=args.lr_patience)
    else:
        scheduler = torch.optim.lr_scheduler.MultiStepLR(hold.opt, list(range(args.lrscheduler_start, 1000, args.lrscheduler_step)),
                                                         gamma=args.lrscheduler_decay)
    main_metrics = getattr(args, "metrics", "mAP")
    best_mAP, best_acc, best_epoch = -np.inf, -np.inf, 0
    result = np.zeros([args.n_epochs, 4])
    global_step, stale = 0, 0
    seen_steps, seen_skipped = 0, 0                        # the guard's counters at the last print step
    xf = input_xf_of(args)
    freqm, timem, noise = int(getattr(args, "freqm", 0) or 0), int(getattr(args, "timem", 0) or 0), bool(getattr(args, "noise", False))
    augment = (freqm > 0 or timem > 0 or noise) and args.ftmode != "videoonly"
    # a masked cell is 0.0 BEFORE the normalisation: raw inputs get that by themselves, a normalised input takes the value by name
    fill = (0.0 - getattr(args, "dataset_mean", -5.081)) / getattr(args, "dataset_std", 4.4849)
    for epoch in range(1, args.n_epochs + 1):
        t0 = time.time()
        losses = []
        base_lr, head_lr, mm_ratio = hold.rates()
        for a_input, v_input, labels in train_loader:
            prob = random.uniform(0, 1)
            branch = draw_branch(prob) if args.ftmode == "mm_grad" else None
            extra = {"input_xf": xf} if xf is not None else {}
            if augment:
                extra["aug"] = audio_model.draw_aug(a_input.shape[0], freqm, timem, noise, fill=fill)
            losses.append(audio_model.train_step(a_input, v_input, labels, base_lr, args.ftmode, branch=branch, loss=args.loss,
                                                 head_lr=head_lr, mm_lr=mm_ratio, **extra))
            global_step += 1
            if global_step % args.n_print_steps == 0:
                say(f"Epoch: [{epoch}][{global_step}] train loss {float(losses[-1]):.5f}", flush=True)
                gs = audio_model.guard_stats() if max_norm is not None else None      # (the loss was just read: the stream is drained)
                if gs is not None:
                    say(f"Epoch: [{epoch}][{global_step}] grad norm {gs['norm']:.5g} (base {gs['norm_base']:.5g} head {gs['norm_head']:.5g} "
                        f"mm {gs['norm_mm']:.5g}) clip coef {gs['coef']:.5g} skipped {gs['n_skipped']} of {gs['n_steps']} steps", flush=True)
                    if guard_diverged(gs["n_steps"] - seen_steps, gs["n_skipped"] - seen_skipped):
                        say("training diverged...", flush=True)
                        return {"best_epoch": best_epoch, "best_mAP": best_mAP, "best_acc": best_acc, "result": result, "diverged": True}
                    seen_steps, seen_skipped = gs["n_steps"], gs["n_skipped"]
        if accum > 1:                                      # no gradient crosses the epoch (validation, the checkpoint, a new rate): a cycle boundary
            audio_model.apply_accumulated(base_lr, head_lr=head_lr, mm_lr=mm_ratio)
        train_loss = float(torch.stack(losses).mean()) if losses else float("nan")
        stats, valid_loss = validate(audio_model, test_loader, test_sampler, args)
        mAP = float(np.nanmean([s["AP"] for s in stats]))
        mAUC = float(np.nanmean([s["auc"] for s in stats]))
        acc = stats[0]["acc"]
        result[epoch - 1, :] = [acc if main_metrics == "acc" else mAP, mAUC, base_lr, train_loss]
        if master:
            np.savetxt(os.path.join(exp_dir, "result.csv"), result, delimiter=",")
        say(f"epoch {epoch}: mAP {mAP:.6f} mAUC {mAUC:.6f} acc {acc:.6f} train loss {train_loss:.6f} valid loss {valid_loss:.6f} "
              f"({time.time() - t0:.1f}s)", flush=True)
        better = mAP > best_mAP if main_metrics == "mAP" else acc > best_acc
        stale = 0 if mAP > best_mAP else stale + 1
        best_mAP, best_acc = max(best_mAP, mAP), max(best_acc, acc)
        if better:
            best_epoch = epoch
        if stale == 3:                                     # :229-251: three epochs without a better mAP end the run - here a return, not exit()
            say(f"early stop at epoch {epoch}: no better mAP for three epochs", flush=True)
            break
        if master:
            sd = {"module." + k: t.detach().cpu() for k, t in audio_model.state_dict().items()}
            if better:
                torch.save(sd, os.path.join(exp_dir, "models", "best_audio_model.pth"))
                opt_state = audio_model.optimizer_state()                   # :256 of the reference: the optimizer beside the best weights
                if opt_state is not None:
                    torch.save(opt_state, os.path.join(exp_dir, "models", "best_optim_state.pth"))
            if getattr(args, "save_model", False):
                torch.save(sd, os.path.join(exp_dir, "models", f"audio_model.{epoch}.pth"))
        hold.opt.step()                                   # (no gradients: a no-op that keeps the scheduler's step order)
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(mAP if main_metrics == "mAP" else acc)
        else:
            scheduler.step()
    return {"best_epoch": best_epoch, "best_mAP": best_mAP, "best_acc": best_acc, "result": result}
