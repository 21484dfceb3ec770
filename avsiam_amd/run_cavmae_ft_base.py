"""Fine-tuning entry point with the flag surface of the reference (src/run_cavmae_ft_base.py:63-139).

    python -m avsiam_amd.run_cavmae_ft_base --model cav-mae-ft --ftmode mm_grad --n_class 527 --loss BCE --lr 1e-4 --head_lr 100 \\
        --mm_lr 100 --batch_size 8 --n_epochs 15 --pretrain_path exp/models/audio_model.20.pth --exp_dir ./ft_base ...

Data flags: --data_train / --data_val '' or 'synthetic' give AudioSet-shaped synthetic clips with label-smoothed multi-hot labels; a path is
the CAV-MAE json of a dataset of WAV files and extracted frames (see "Training from files" below; mp4 / video decoding is out of scope).  --pretrain_path loads a CAVMAE_BASE checkpoint
(with or without the 'module.' prefix) with strict=False (:243-249).  --freqm / --timem / --noise are the reference's training augmentation
(dataloader_ft.py:527-548: SpecAugment masks on the un-normalised fbank, normalisation, noise, time roll), drawn per step on the device and
applied inside the audio patch gather; validation never augments.  Accepted but not implemented: --wa (weight averaging), --bal, and --mixup
without --wave-input - a warning names each one set to a non-default value (mixup: the reference mixes waveforms before the fbank, frames with
a second weight, and draws the partner from the whole dataset - not reproducible from a batch of spectrograms); --warmup, distillation
weights and logging are inert.  Validation uses 10-frame synthetic clips when the test mode is mm_grad.
--wave-input: the loaders yield what a decoder produces - float32 16 kHz waveforms (9 - 10 s, so the padding to 1024 rows is exercised) and
uint8 frames - and the Kaldi fbank (dataloader_ft.py:325), its normalisation and, with --mixup p, the reference's mixup run on the device:
waveforms mixed inside the fbank kernel's sample read (:308-322), frames with an independent weight (:457-458), labels as :470-475; the
per-sample draws (mixed with probability p, lambda ~ Beta(10, 10), the frame weight) stay on the host, seeded per rank.  --freqm / --timem /
--noise then act on the normalised fbank with fill (0 - mean) / std, which is the reference's SpecAugment -> normalise -> noise -> roll.
The synthetic partner is the batch rolled by one.  Refused together with --raw-input.
Training from files: --data_train FILE.json / --data_val FILE.json with --label_csv FILE.csv (dataset_ft: {"data": [{"wav", "labels", "video_id",
"video_path"}]}, the csv index,mid,display_name, frames at video_path/frame_{k}/{video_id}.npy | .jpg | .png) replace the synthetic loader of that
side and imply --wave-input: WAV files are parsed on the host (preprocess.parse_wav), their PCM payload is decoded on the device
(ops.decode_pcm) and runs through resample -> fbank -> mixup as above, the frames through ops.resize_frames; the mixup partner is drawn from
the whole dataset (dataloader_ft.py:372), the training frame from --total-frame frames (:352), validation takes the middle frame or, in the
mm_grad test mode and for --eval-frames, all of them.  --n_class must equal the csv's classes.  One side may stay synthetic.  --num_workers
read and parse files; every draw stays in the main process.  A worker inherits the open GPU, so the request is cut to what keeps one
machine at 16 processes, ranks and the workers of both sides counted (dataset_ft.worker_share: one rank with one file side starts at most
15, with two 7 each, 8 ranks 1 or none); validation workers end with every pass.  An unreadable clip is reported once, replaced by silence
and a grey frame and counted; --strict-data raises instead.  --sample-rate / --audio-channels / --frame-size describe the synthetic side only: a
file brings its own.  Not built: mp4 / video and compressed-audio decoding, --bal.
--frame-size H W (only with --wave-input): the loaders keep their uint8 frames at the decoded size H x W, every batch draws a size per clip (the
full size or a narrower crop, so one padded buffer holds clips of several sizes) and ops.resize_frames runs what the reference's loader does
to them (dataloader_ft.py:136-139, 434-459: / 255, Resize([224, 224], BICUBIC, antialias=True), Normalize, the frame mix) in one launch; H and W
lie in 1 .. 2240 (at most 10 x the model's 224).  Not built: video decoding and frame selection.
Extensions: --raw-input (the loaders yield un-normalised fbank and uint8 frames, normalised on the device inside the kernels that read
them, as in the pre-training launcher); --steps-per-epoch / --val-steps (synthetic epoch lengths); --device-metrics: the validation metrics come from the HIP counting
kernel and the [N, C] outputs never leave the device (traintest_ft_base.calculate_stats_device; AP then groups tied scores as sklearn does);
--eval-frames: after training, the reference launcher's multi-frame protocol (:326-369) on the validation clips - the metric of every frame and
of the mean over the frames, written to exp_dir/mul_frame_res.csv (needs the mm_grad test mode).

Data parallel: launch through torchrun, one process per GPU, as the reference's recipes do (VGGSound: 8 ranks).  RANK / WORLD_SIZE /
LOCAL_RANK form the process group (utils.init_distributed_mode), the model gets its collectives (CAVMAEFT_BASE.set_distributed: RCCL) and
`random` is seeded 87 + local rank, so every rank draws its own mm_grad branch per step as in the reference; each rank trains on its own
synthetic shard, rank 0 writes the artefacts.  --world_size N without that environment starts nothing and is refused.  --force-dp: issue
the collectives at world size 1 too (what one GPU can run of this path).  No run with more than one rank on RCCL exists: what is verified
is the arithmetic and the message schedule (gloo ranks sharing one GPU), not the scaling.
--clip-grad-norm X / --skip-nonfinite: the guarded step (CAVMAEFT_BASE.set_grad_guard) - the gradient norm, torch's clip_grad_norm_
coefficient and the reference's skip of a step with inf / NaN gradients (GradScaler.step, traintest_ft_base.py:162-165), all on the device
between the gradient all-reduce and Adam; the print steps add the norm, the coefficient and the steps skipped, and a run that skips more
than half of its steps between two prints ends with "training diverged...".
--accum-steps K: gradient accumulation (CAVMAEFT_BASE.set_grad_accumulation) - the effective batch the reference's recipes reach through
several GPUs, on one: every batch is a micro-step whose gradients are summed on the device, every K-th batch takes the optimizer step over
their mean, and what is pending after the last batch of an epoch is applied there.  The printed step keeps counting batches; the guard's
counters count optimizer steps.
--pretrain_path <dir>/best_audio_model.pth also restores <dir>/best_optim_state.pth (Adam moments, per-class steps) when it is there and
is a fine-tuning state of this model; the pre-training loop's file of the same name (torch.optim.Adam's format) is left alone.
"""
import argparse
import ast
import os


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--data_train", type=str, default='', help="training data json ('' or 'synthetic': synthetic tensors)")
    p.add_argument("--data_val", type=str, default='', help="validation data json ('' or 'synthetic')")
    p.add_argument("--data_eval", type=str, default=None)
    p.add_argument("--label_csv", type=str, default='')
    p.add_argument("--n_class", type=int, default=527)
    p.add_argument("--model", type=str, default='cav-mae-ft', choices=["cav-mae-ft"])
    p.add_argument("--dataset", type=str, default="audioset")
    p.add_argument("--dataset_mean", type=float, default=-5.081)
    p.add_argument("--dataset_std", type=float, default=4.4849)
    p.add_argument("--target_length", type=int, default=1024)
    p.add_argument("--noise", type=ast.literal_eval, default=False)
    p.add_argument("--exp_dir", type=str, default="")
    p.add_argument('--lr', '--learning-rate', default=0.001, type=float)
    p.add_argument("--optim", type=str, default="adam", choices=["sgd", "adam"])
    p.add_argument('-b', '--batch_size', default=48, type=int)
    p.add_argument('-w', '--num_workers', default=32, type=int)
    p.add_argument("--n_epochs", type=int, default=10)
    p.add_argument("--lr_patience", type=int, default=1)
    p.add_argument("--lr_adapt", type=ast.literal_eval, default=False)
    p.add_argument("--metrics", type=str, default="mAP", choices=["mAP", "acc"])
    p.add_argument("--loss", type=str, default="BCE", choices=["BCE", "CE"])
    p.add_argument('--warmup', type=ast.literal_eval, default='True')
    p.add_argument("--lrscheduler_start", default=2, type=int)
    p.add_argument("--lrscheduler_step", default=1, type=int)
    p.add_argument("--lrscheduler_decay", default=0.5, type=float)
    p.add_argument('--freqm', type=int, default=0)
    p.add_argument('--timem', type=int, default=0)
    p.add_argument("--wa", type=ast.literal_eval, default=False)
    p.add_argument("--wa_start", type=int, default=1)
    p.add_argument("--wa_end", type=int, default=10)
    p.add_argument("--n-print-steps", dest="n_print_steps", type=int, default=100)
    p.add_argument('--save_model', type=ast.literal_eval, default=False)
    p.add_argument("--mixup", type=float, default=0)
    p.add_argument("--bal", type=str, default=None)
    p.add_argument("--label_smooth", type=float, default=0.1)
    p.add_argument("--weight_file", type=str, default=None)
    p.add_argument("--pretrain_path", type=str, default='None')
    p.add_argument("--ftmode", type=str, default='multimodal')
    p.add_argument("--ftmode_test", type=str, default=None)
    p.add_argument("--head_lr", type=float, default=50.0)
    p.add_argument("--mm_lr", type=float, default=None)
    p.add_argument('--freeze_base', type=ast.literal_eval, default=False)
    p.add_argument('--skip_frame_agg', type=ast.literal_eval, default=False)
    p.add_argument("--dis_w", type=float, default=0)
    p.add_argument("--dis_w_2", type=float, default=0)
    p.add_argument("--master_addr", type=str)
    p.add_argument("--nproc_per_node", type=int)
    p.add_argument("--wandb", type=int, default=0)
    p.add_argument('--model_name', type=str, default=None)
    p.add_argument('--world_size', default=1, type=int)
    p.add_argument('--local_rank', default=-1, type=int)
    p.add_argument('--dist_url', default='env://')
    p.add_argument('--steps-per-epoch', dest="steps_per_epoch", default=20, type=int, help="synthetic-data epoch length")
    p.add_argument('--val-steps', dest="val_steps", default=2, type=int, help="synthetic validation batches per epoch")
    p.add_argument('--device-metrics', dest="device_metrics", action="store_true", help="validation metrics on the device (exact counting kernel)")
    p.add_argument('--force-dp', dest="force_dp", action="store_true", help="issue the data-parallel collectives at world size 1 too")
    p.add_argument('--raw-input', dest="raw_input", action="store_true",
                   help="feed un-normalised fbank + uint8 frames and normalise on the device (dataloader_ft.py:534, 461-462)")
    p.add_argument('--wave-input', dest="wave_input", action="store_true",
                   help="feed float32 waveforms + uint8 frames: Kaldi fbank, normalisation and --mixup on the device (dataloader_ft.py:277-340, 441-475)")
    p.add_argument('--frame-size', dest="frame_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="with --wave-input: uint8 frames at the decoded size H x W, resized (antialiased bicubic), normalised and mixed on the device "
                        "(dataloader_ft.py:136-139, 434-459)")
    p.add_argument('--sample-rate', dest="sample_rate", type=int, nargs='+', default=None, metavar="R",
                   help="with --wave-input: the audio stays at the files' own rates (cycled over the clips of a batch) and is resampled to 16 kHz on the "
                        "device (dataloader_ft.py:272-277)")
    p.add_argument('--audio-channels', dest="audio_channels", type=int, default=None, metavar="C",
                   help="with --wave-input --sample-rate: channels of the decoded audio, averaged on the device (dataloader_ft.py:298-306)")
    p.add_argument('--eval-frames', dest="eval_frames", action="store_true",
                   help="after training: per-frame and frame-ensemble metric of the validation clips -> exp_dir/mul_frame_res.csv (mm_grad test mode)")
    p.add_argument('--exact-eval', dest="exact_eval", action="store_true",
                   help="validation and --eval-frames forwards on the exact-fp32 path (fp32 operands from the master weights; slower, training unchanged)")
    p.add_argument('--clip-grad-norm', dest="clip_grad_norm", type=float, default=None, metavar="X",
                   help="clip the total gradient norm to X on the device (torch.nn.utils.clip_grad_norm_) and skip steps with inf / NaN gradients")
    p.add_argument('--skip-nonfinite', dest="skip_nonfinite", action="store_true",
                   help="skip steps whose gradients hold inf or NaN, without clipping (what the reference's GradScaler.step does, "
                        "traintest_ft_base.py:162-165)")
    p.add_argument('--strict-data', dest="strict_data", action="store_true",
                   help="with a file dataset: an unreadable clip raises instead of being replaced by silence and a grey frame")
    p.add_argument('--total-frame', dest="total_frame", type=int, default=10, metavar="F",
                   help="with a file dataset: the frames extracted per clip, video_path/frame_0 .. frame_{F-1} (dataloader_ft.py:344-359)")
    p.add_argument('--accum-steps', dest="accum_steps", type=int, default=1, metavar="K",
                   help="gradient accumulation: every K batches take ONE optimizer step over the mean of their gradients, summed on the device "
                        "(CAVMAEFT_BASE.set_grad_accumulation); what is left at the end of an epoch is applied there")
    return p


def load_pretrained(model, path):
    """run_cavmae_ft_base.py:243-249: strict=False load of a (pre-training or fine-tuning) checkpoint -> (missing, unexpected)"""
    import torch
    sd = torch.load(path, map_location="cpu")
    miss, unexpected = model.load_state_dict(sd, strict=False)
    print("now load cav-mae pretrained weights from ", path)
    print("Missing: ", miss)
    print("Unexpected: ", unexpected)
    return miss, unexpected


def restore_optimizer_state(model, pretrain_path):
    """Continue Adam where a fine-tuning run left it: only for <dir>/best_audio_model.pth with a best_optim_state.pth beside it that train()
    of traintest_ft_base wrote (plain tensors m / v / step / lr fitting this model).  The pre-training loop writes a file of the same name in
    torch.optim.Adam's {'state', 'param_groups'} format beside ITS checkpoints: that one, and anything else that does not fit, is left alone -
    a weights-only warm start, said so.  -> True when the state was restored."""
    import torch
    if os.path.basename(pretrain_path) != 'best_audio_model.pth':
        return False
    opt_path = os.path.join(os.path.dirname(pretrain_path), 'best_optim_state.pth')
    if not os.path.exists(opt_path):
        return False
    state = torch.load(opt_path, map_location='cpu')
    lo, hi = model.arena.range[1]
    from .models.cav_mae_ft import CLASSES
    fits = (isinstance(state, dict) and set(state) >= {"m", "v", "step", "lr"} and all(torch.is_tensor(state[k]) for k in ("m", "v", "step", "lr"))
            and state["m"].numel() == hi - lo and state["v"].numel() == hi - lo and state["step"].numel() == len(CLASSES)
            and state["lr"].numel() == 3)
    if not fits:
        print('{:s} is not a fine-tuning Adam state of this model (a pre-training run writes a file of that name): weights-only warm start, '
              'Adam restarts'.format(opt_path))
        return False
    model.load_optimizer_state(state)
    print('restored the Adam state (moments, steps {}) from {:s}'.format(model.optimizer_steps(), opt_path))
    return True


MIXUP_REASON = ("mixup is not reproducible from a batch of spectrograms: the reference mixes the two WAVEFORMS before the fbank "
                "(dataloader_ft.py:321-325), mixes the frames with a second, independent weight (:457-458) and draws the partner from the whole "
                "dataset (:400-417)")


def inert_flag_warnings(args):
    """-> the warning lines for flags this path accepts and ignores (--freqm / --timem / --noise are implemented and not among them; nor is
    --mixup under --wave-input, where the waveforms it mixes exist)"""
    live_mixup = bool(getattr(args, "wave_input", False))
    inert = [f"--{k} {getattr(args, k)}" for k, off in (("mixup", 0), ("wa", False), ("bal", None))
             if getattr(args, k) not in (off, 'None') and not (k == "mixup" and live_mixup)]
    out = []
    if inert:
        out.append("WARNING: not implemented on this path, ignored: " + ", ".join(inert) + " - this run trains without them")
    if getattr(args, "mixup", 0) not in (0, 'None') and not live_mixup:
        out.append("WARNING: " + MIXUP_REASON)
    return out


def data_plan(args):
    """-> {"train": "file" | "synthetic", "val": ...}, checked: a json side needs --label_csv, both files must exist, and --n_class must equal
    the classes the csv lists (SystemExit otherwise).  Any file side implies the wave path."""
    plan = {side: "synthetic" if getattr(args, "data_" + side) in ('', 'synthetic') else "file" for side in ("train", "val")}
    if "file" not in plan.values():
        return plan
    if not args.label_csv:
        raise SystemExit("--data_train / --data_val name a dataset json: pass its --label_csv (index,mid,display_name) with it")
    for path in [args.label_csv] + [getattr(args, "data_" + side) for side in plan if plan[side] == "file"]:
        if not os.path.isfile(path):
            raise SystemExit(f"{path}: no such file")
    from .dataset_ft import make_index_dict
    try:
        n = len(make_index_dict(args.label_csv))
    except (ValueError, KeyError) as e:
        raise SystemExit(str(e))
    if n != args.n_class:
        raise SystemExit(f"--n_class {args.n_class} does not match --label_csv {args.label_csv}, which lists {n} classes")
    if args.total_frame < 1:
        raise SystemExit(f"--total-frame {args.total_frame}: the frames extracted per clip, an integer >= 1")
    if plan["val"] == "file" and (args.ftmode_test or args.ftmode) == "mm_grad" and args.total_frame != 10:
        raise SystemExit(f"--total-frame {args.total_frame}: the mm_grad test mode scores all frames of a validation clip and the model takes 10 "
                         "(cav_mae_base.py:940); extract 10 frames per clip, or validate in another mode (--ftmode_test)")
    return plan


def main(argv=None):
    args = build_parser().parse_args(argv)
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.world_size > 1 and not launched:
        raise SystemExit("data-parallel fine-tuning is launched through torchrun, one process per GPU (RANK / WORLD_SIZE / LOCAL_RANK in the "
                         "environment form the process group): --world_size alone starts no ranks")
    args.data_plan = data_plan(args)
    if "file" in args.data_plan.values():
        args.wave_input = True                                                 # a file loader yields what the wave loaders yield
    if args.ftmode not in ("audioonly", "videoonly", "mm_grad"):
        raise SystemExit(f"--ftmode {args.ftmode}: the trainable modes are audioonly, videoonly and mm_grad")
    if args.eval_frames and (args.ftmode_test or args.ftmode) != "mm_grad":
        raise SystemExit("--eval-frames scores the frames of multi-frame clips: it needs the mm_grad test mode (--ftmode_test mm_grad)")
    if args.wave_input and args.raw_input:
        raise SystemExit("--wave-input and --raw-input both name the loader's output (waveforms + uint8 frames | un-normalised fbank + uint8 frames): "
                         "pass one of them")
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0:
        raise SystemExit(f"--clip-grad-norm {args.clip_grad_norm}: a total gradient norm > 0")
    if args.accum_steps < 1:
        raise SystemExit(f"--accum-steps {args.accum_steps}: the batches per optimizer step, an integer >= 1 (1: no accumulation)")
    if args.wave_input and not 0.0 <= args.mixup <= 1.0:
        raise SystemExit(f"--mixup {args.mixup}: a probability")
    if args.frame_size is not None:
        if not args.wave_input:
            raise SystemExit("--frame-size names the size of the decoded uint8 frames of --wave-input: pass it with --wave-input")
        if not all(1 <= x <= 2240 for x in args.frame_size):
            raise SystemExit(f"--frame-size {args.frame_size[0]} {args.frame_size[1]}: H and W lie in 1 .. 2240 (at most 10 x the model's 224)")
    if args.sample_rate is not None or args.audio_channels is not None:
        if not args.wave_input:
            raise SystemExit("--sample-rate / --audio-channels name the decoded audio of --wave-input: pass them with --wave-input")
        if args.sample_rate is None:
            raise SystemExit("--audio-channels names the channels of the audio that --sample-rate resamples: pass --sample-rate with it (16000: only the "
                             "channel mean is taken)")
        if not all(1 <= r <= 768000 for r in args.sample_rate) or len(set(args.sample_rate)) > 8:
            raise SystemExit(f"--sample-rate {' '.join(map(str, args.sample_rate))}: at most 8 distinct rates in 1 .. 768000 Hz")
        if args.audio_channels is not None and not 1 <= args.audio_channels <= 8:
            raise SystemExit(f"--audio-channels {args.audio_channels}: 1 .. 8")
    for w in inert_flag_warnings(args):
        print(w, flush=True)
    import random
    import torch
    from . import utils
    args.local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if launched:
        random.seed(87 + args.local_rank)                                     # the reference's per-rank branch draw (run_cavmae_ft_base.py)
    utils.init_distributed_mode(args)
    try:
        return _run(args)
    finally:
        utils.restore_print()
        if args.distributed and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def _run(args):
    import torch
    from .config import AVSiamConfig
    from .models import CAVMAEFT_BASE
    from .traintest_ft_base import SyntheticFtLoader, evaluate_frames, train
    cfg = AVSiamConfig()
    model = CAVMAEFT_BASE(label_dim=args.n_class)
    if args.pretrain_path != 'None':
        load_pretrained(model, args.pretrain_path)
    model = model.to(torch.device("cuda", getattr(args, "gpu", 0)))
    if args.pretrain_path != 'None':
        restore_optimizer_state(model, args.pretrain_path)
    if args.world_size > 1 or args.force_dp:
        from .comm import RcclComm, TorchDistComm
        if os.environ.get("AVSIAM_COMM", "torch") == "rccl" or not torch.distributed.is_initialized():
            comm = RcclComm(rank=args.rank, world=args.world_size, always=args.force_dp)
        else:
            comm = TorchDistComm(always=args.force_dp)
        model.set_distributed(args.world_size, args.rank, comm)
    dev = model.arena.p.device
    val_frames = 10 if (args.ftmode_test or args.ftmode) == "mm_grad" else 1          # validate() runs is_eval=True: mm_grad wants 10 frames
    plan = getattr(args, "data_plan", {"train": "synthetic", "val": "synthetic"})
    if args.wave_input:
        from .traintest_ft_base import SyntheticWaveFtLoader
        norm = (args.dataset_mean, args.dataset_std)
        source = {} if args.sample_rate is None else dict(sample_rate=args.sample_rate, channels=args.audio_channels or 1)

        def synthetic_train():
            return SyntheticWaveFtLoader(cfg, args.batch_size, args.steps_per_epoch, args.n_class, dev, seed=87 + args.rank, label_smooth=args.label_smooth,
                                         mixup=args.mixup, norm=norm, train=True, frame_size=args.frame_size, **source)

        def synthetic_val():
            return SyntheticWaveFtLoader(cfg, args.batch_size, args.val_steps, args.n_class, dev, seed=88 + 1000 * args.rank,
                                         label_smooth=args.label_smooth, frames=val_frames, norm=norm, train=False, frame_size=args.frame_size, **source)
    else:
        def synthetic_train():
            return SyntheticFtLoader(cfg, args.batch_size, args.steps_per_epoch, args.n_class, dev, seed=87 + args.rank, label_smooth=args.label_smooth,
                                     raw=args.raw_input)

        def synthetic_val():
            return SyntheticFtLoader(cfg, args.batch_size, args.val_steps, args.n_class, dev, seed=88 + 1000 * args.rank, label_smooth=args.label_smooth,
                                     frames=val_frames, raw=args.raw_input)

    def file_loader(path, **kw):
        from .dataset_ft import FileFtLoader, FtFileDataset, worker_share
        # the ranks of this machine (torchrun's LOCAL_WORLD_SIZE; without it, all of them) and the file loaders of this rank share 16 processes
        ranks = int(os.environ.get("LOCAL_WORLD_SIZE", args.world_size))
        workers = worker_share(args.num_workers, loaders=list(plan.values()).count("file"), ranks=ranks)
        return FileFtLoader(FtFileDataset(path, args.label_csv, args.n_class), cfg, args.batch_size, dev, label_smooth=args.label_smooth, norm=norm,
                            total_frame=args.total_frame, num_workers=workers, rank=args.rank, world=args.world_size, strict=args.strict_data, **kw)

    train_loader = file_loader(args.data_train, seed=87, mixup=args.mixup, train=True) if plan["train"] == "file" else synthetic_train()
    val_loader = (file_loader(args.data_val, seed=88, train=False, frames="all" if val_frames > 1 else "middle") if plan["val"] == "file"
                  else synthetic_val())
    # data parallel: validate() truncates the gathered, padded shards of a file set to len(dataset)
    val_sampler = val_loader.sampler if plan["val"] == "file" and args.world_size > 1 else None
    os.makedirs(args.exp_dir or ".", exist_ok=True)
    args.exp_dir = args.exp_dir or "."
    result = train(model, train_loader, val_loader, val_sampler, args)
    for name, loader in (("training", train_loader), ("validation", val_loader)):
        if getattr(loader, "n_bad", 0):
            print(f"{loader.n_bad} unreadable {name} clip(s) were replaced by silence / a grey frame", flush=True)
    if args.eval_frames:
        result["frame_res"] = evaluate_frames(model, val_loader, args)
    for loader in (train_loader, val_loader):
        if hasattr(loader, "close"):
            loader.close()                                                   # the training workers end here
    return result


if __name__ == "__main__":
    main()
