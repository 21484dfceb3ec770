"""Look at what a pre-trained checkpoint fills in: mask a span of the audio, a mel band or a box of the frames, run the MAE pass and write
the reconstructions (CAVMAE_BASE.inpaint; unpatchify kernel csrc/inpaint.hip).

    python -m avsiam_amd.inpaint --checkpoint exp/models/audio_model.pth --synthetic 4 --mask-time 256 512 --mask-box 0 0 112 112 --out recon/

Without --checkpoint the model keeps its synthetic initial state (what a reconstruction of an untrained model looks like).  Inputs are
AudioSet-shaped synthetic clips, as in the other launchers (file decoding is out of scope); --raw-input feeds the un-normalised fbank and
uint8 frames and returns the reconstructions in those units.  --out DIR receives recon.npz - audio / imgs (what the model was given),
recon_audio / recon_imgs, mask_a / mask_v, err_a / err_v (per-token mean squared error of the masked tokens), loss_mae_a / loss_mae_v - and,
only when PIL is installed, one PNG per clip and modality (input above reconstruction).  No masks given: the model's own random 75 %.
"""
import argparse
import os

from .run_cavmae_pretrain_base import MODELS


def build_parser():
    p = argparse.ArgumentParser(prog="python -m avsiam_amd.inpaint", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Reconstructions from the MAE pass: mask chosen regions, write what the model fills in.")
    p.add_argument("--checkpoint", type=str, default=None, help="state dict of the pre-training model (this loop's or the reference's, 'module.' prefix allowed); "
                                                                "default: the synthetic initial state")
    p.add_argument("--synthetic", type=int, default=2, metavar="N", help="number of synthetic AudioSet-shaped clips")
    p.add_argument("--model", type=str, default="cav-mae", choices=list(MODELS), help="model skeleton, as the pre-training launcher")
    p.add_argument("--target_length", type=int, default=1024, help="spectrogram frames")
    p.add_argument("--frames", type=int, default=1, help="video frames per clip")
    p.add_argument("--depth", type=int, default=None, help="(tests) encoder depth override of the chosen skeleton")
    p.add_argument("--mask-time", dest="mask_time", type=int, nargs=2, metavar=("A", "B"), default=None,
                   help="mask every audio patch that intersects spectrogram frames [A, B)")
    p.add_argument("--mask-mel", dest="mask_mel", type=int, nargs=2, metavar=("A", "B"), default=None, help="mask every audio patch that intersects mel bins [A, B)")
    p.add_argument("--mask-box", dest="mask_box", type=int, nargs=4, metavar=("Y0", "X0", "Y1", "X1"), default=None,
                   help="mask every patch of every frame that intersects rows [Y0, Y1) x columns [X0, X1)")
    p.add_argument("--raw-input", dest="raw_input", action="store_true", help="feed un-normalised fbank + uint8 frames; reconstructions come back in those units")
    p.add_argument("--dataset_mean", type=float, default=-5.081)
    p.add_argument("--dataset_std", type=float, default=4.4849)
    p.add_argument("--seed", type=int, default=87, help="seed of the synthetic clips and of the random remainder of the masks")
    p.add_argument("--out", type=str, required=True, metavar="DIR", help="directory for recon.npz (and PNGs when PIL is installed)")
    return p


def make_config(args):
    from . import config as _config
    cls_name, shape_fn, stride = MODELS[args.model]
    if args.synthetic < 1:
        raise SystemExit("--synthetic: at least one clip")
    if args.target_length < stride or args.frames < 1:
        raise SystemExit("--target_length / --frames: nothing to reconstruct")
    kw = {"audio_tokens": args.target_length // stride * (128 // stride), "frames": args.frames}
    if args.depth is not None:
        kw["depth"] = args.depth
    return cls_name, getattr(_config, shape_fn)(**kw)


def make_plan(args, cfg):
    """the region plan of the --mask-* flags (maskplan.make_mae_plan_regions), or None: the model draws its own 75 %"""
    import torch
    from . import maskplan
    if args.mask_time is None and args.mask_mel is None and args.mask_box is None:
        return None
    must_a = None
    try:
        if args.mask_time is not None:
            must_a = maskplan.audio_time_span(cfg, *args.mask_time)
        if args.mask_mel is not None:
            band = maskplan.audio_mel_band(cfg, *args.mask_mel)
            must_a = band if must_a is None else must_a | band
        must_v = maskplan.frame_box(cfg, *args.mask_box) if args.mask_box is not None else None
        return maskplan.make_mae_plan_regions(cfg, args.synthetic, torch.Generator().manual_seed(args.seed), must_a, must_v)
    except ValueError as e:
        raise SystemExit(f"inpaint: {e}") from None


def write_pngs(out_dir, arrays):
    """one picture per clip and modality, input above reconstruction, grey levels scaled to the input's range.  Only with PIL."""
    try:
        from PIL import Image
    except ImportError:
        return 0
    import numpy as np

    def grey(x, lo, hi):
        return np.clip((x.astype(np.float32) - lo) / max(hi - lo, 1e-12) * 255.0, 0, 255).astype(np.uint8)

    n = 0
    for b in range(arrays["audio"].shape[0]):
        a, r = arrays["audio"][b], arrays["recon_audio"][b]
        lo, hi = float(a.min()), float(a.max())
        Image.fromarray(np.concatenate([grey(a.T, lo, hi), grey(r.T, lo, hi)], axis=0)).save(os.path.join(out_dir, f"audio_{b}.png"))
        v, rv = arrays["imgs"][b], arrays["recon_imgs"][b]
        v, rv = v.reshape(-1, *v.shape[-3:]), rv.reshape(-1, *rv.shape[-3:])
        for t in range(v.shape[0]):
            if v.dtype == np.uint8:
                top, bot = v[t], rv[t]
            else:
                lo, hi = float(v[t].min()), float(v[t].max())
                top, bot = grey(v[t], lo, hi), grey(rv[t], lo, hi)
            Image.fromarray(np.concatenate([top, bot], axis=1).transpose(1, 2, 0)).save(os.path.join(out_dir, f"frame_{b}_{t}.png"))
        n += 1 + v.shape[0]
    return n


def main(argv=None):
    args = build_parser().parse_args(argv)
    cls_name, cfg = make_config(args)
    plan = make_plan(args, cfg)                                   # (argument errors before anything touches the GPU)
    import numpy as np
    import torch
    from . import models
    from .ops import InputXf
    from .traintest_cavmae_base import SyntheticAVLoader
    model = getattr(models, cls_name)(cfg=cfg, verbose=False)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        miss, unexpected = model.load_state_dict(sd, strict=False)
        if len(miss) >= len(model.state_dict()):
            raise SystemExit(f"--checkpoint {args.checkpoint}: none of this model's keys is in it - not a checkpoint of {cls_name}")
        print(f"loaded {args.checkpoint}: {len(miss)} keys keep their initial value, {len(unexpected)} checkpoint keys ignored")
    model = model.cuda()
    loader = SyntheticAVLoader(cfg, args.synthetic, 1, torch.device("cuda"), args.seed, raw=args.raw_input)
    xf = (InputXf.audio(args.dataset_mean, args.dataset_std), InputXf.frames()) if args.raw_input else None
    res = model.inpaint(loader.a, loader.v, mask_plan=plan, input_xf=xf, raw=args.raw_input)
    arrays = {"audio": loader.a, "imgs": loader.v, "recon_audio": res.audio, "recon_imgs": res.imgs, "mask_a": res.mask_a, "mask_v": res.mask_v,
              "err_a": res.err_a, "err_v": res.err_v, "loss_mae_a": res.loss_mae_a, "loss_mae_v": res.loss_mae_v}
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "recon.npz"), stride=np.array(cfg.st), **arrays)
    pngs = write_pngs(args.out, arrays)
    print("inpaint: {:d} clips, loss_mae_a {:.4f} loss_mae_v {:.4f}, masked {:d}/{:d} audio and {:d}/{:d} frame patches per clip -> {:s}/recon.npz{:s}".format(
        args.synthetic, float(arrays["loss_mae_a"]), float(arrays["loss_mae_v"]), int(arrays["mask_a"][0].sum()), cfg.audio_tokens,
        int(arrays["mask_v"][0].sum()), cfg.frames * cfg.video_tokens, args.out, f" and {pngs} PNGs" if pngs else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
