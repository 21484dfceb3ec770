"""Audio-visual retrieval evaluation (the reference's src/retrieval.py) on the HIP path.

    python -m avsiam_amd.retrieval --synthetic 256 --direction both
    python -m avsiam_amd.retrieval --model exp/models/audio_model.25.pth --model-type pretrain ...   (with a loader of your own: eval_retrieval)

The reference's names and return values - ``get_similarity``, ``get_sim_mat``, ``compute_metrics``, ``print_computed_metrics`` (numpy),
``get_retrieval_result``, ``eval_retrieval`` - importable without side effects (the reference's module runs its experiment at import).
What differs underneath:
  * features: ``CAVMAEFT_BASE.retrieval_features`` embeds only the frame that is used (frame 5 of 10) and pools + normalises on the device;
    the features of the whole set stay in two device buffers, and ONE extraction pass serves both directions;
  * ranks: ``ops.retrieval_rank`` streams the fp32 similarity through the matrix cores and counts, per query, the gallery entries that beat
    its true match - the N x N matrix of get_sim_mat (a Python double loop of numpy.dot there) is never built, and only the [N] rank vector
    crosses to the host, once.  ``metrics_from_ranks`` turns it into the reference's four numbers.
Ties: compute_metrics emits one entry per column that ties with the match (its len(ind) then exceeds N); the device path reports the
optimistic rank (strictly better entries only) and prints the number of tied rows when there are any.  On tie-free features - anything but
duplicated clips - the two agree exactly.

Real datasets: the reference's AudiosetDataset needs torchaudio; any loader yielding ``(a_input [B, 1024, 128], v_input [B, T, 3, 224, 224],
labels)`` works.  ``--synthetic N`` builds N paired synthetic clips so that the entry point runs without a dataset.
"""
import argparse
import sys

import numpy as np

DIRECTIONS = ("audio", "video")          # 'audio': audio -> visual retrieval, 'video': visual -> audio (src/retrieval.py:61)


# ---- the reference's numpy helpers --------------------------------------------------------------------------------------------------------
def get_similarity(a, b):
    """cosine similarity of two vectors (src/retrieval.py:27-29)"""
    a, b = np.asarray(a), np.asarray(b)
    return np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))


def get_sim_mat(a, b):
    """[B, B] float64 matrix of get_similarity(a[i], b[j]) (src/retrieval.py:32-38), as one product instead of B * B numpy.dot calls; the
    arithmetic stays in the inputs' precision, as the reference's, and differs from it by summation order only (<= 2 D 2^-24 for fp32)."""
    a, b = np.asarray(a), np.asarray(b)
    B = a.shape[0]
    sim = (a @ b[:B].T) / np.outer(np.linalg.norm(a, axis=1), np.linalg.norm(b[:B], axis=1))
    return sim.astype(np.float64)


def _metrics_of(ind):
    n = len(ind)
    return {"R1": float(np.sum(ind == 0)) / n, "R5": float(np.sum(ind < 5)) / n, "R10": float(np.sum(ind < 10)) / n, "MR": np.median(ind) + 1}


def compute_metrics(x):
    """R@1 / R@5 / R@10 / median rank of the diagonal of a similarity matrix, with the reference's behaviour on ties (src/retrieval.py:40-52):
    row i contributes one entry per column equal to x[i, i] - positions rank, rank + 1, ... of the descending sort - so a row with ties
    counts more than once and a NaN diagonal not at all."""
    x = np.asarray(x)
    d = np.diag(x)[:, None]
    better = (x > d).sum(1)
    equal = (x == d).sum(1)                                      # the diagonal itself included
    first = np.cumsum(equal) - equal
    ind = np.repeat(better, equal) + (np.arange(int(equal.sum())) - np.repeat(first, equal))
    return _metrics_of(ind)


def metrics_from_ranks(rank):
    """The same four numbers from a rank vector (rank[i] = number of gallery entries strictly more similar than query i's match, as
    ops.retrieval_rank returns it): MR = median(rank) + 1."""
    return _metrics_of(np.asarray(rank).reshape(-1))


def print_computed_metrics(metrics):
    print('R@1: {:.4f} - R@5: {:.4f} - R@10: {:.4f} - Median R: {}'.format(metrics['R1'], metrics['R5'], metrics['R10'], metrics['MR']))


# ---- feature extraction + ranking on the device ----------------------------------------------------------------------------------------------
def _dataset_size(loader):
    for probe in (lambda: len(loader.dataset), lambda: loader.num_clips):
        try:
            return int(probe())
        except (AttributeError, TypeError):
            pass
    return None


def extract_features(audio_model, val_loader, frame_index=5, exact=False):
    """exact: features from the exact-fp32 forward (retrieval_features(exact=True); models that have the mode).  One pass over the loader -> (audio [N, D], video [N, D]) fp32 unit vectors on the model's device.  When the loader tells its size
    (``len(loader.dataset)`` or ``loader.num_clips``) every batch is written straight into its rows of the two [N, D] buffers."""
    import torch
    model = audio_model.module if hasattr(audio_model, "module") else audio_model
    if not model.arena.p.is_cuda:
        model = model.cuda()
    model.eval()
    dev, D = model.arena.p.device, model.cfg.embed_dim
    n = _dataset_size(val_loader)
    fa = fv = None
    if n is not None:
        fa, fv = torch.empty((n, D), dtype=torch.float32, device=dev), torch.empty((n, D), dtype=torch.float32, device=dev)
    chunks, at = [], 0
    ex = {"exact": True} if exact else {}                           # (without the flag: the call of before, argument for argument)
    for batch in val_loader:
        a_input, v_input = batch[0], batch[1]
        B = a_input.shape[0]
        if fa is not None and at + B <= n:
            model.retrieval_features(a_input, v_input, frame_index, out_a=fa[at:at + B], out_v=fv[at:at + B], **ex)
        else:                                                       # size unknown (or misreported): keep the batches, join at the end
            if fa is not None:
                chunks, fa, fv = [(fa[:at], fv[:at])], None, None
            chunks.append(model.retrieval_features(a_input, v_input, frame_index, **ex))
        at += B
    if fa is None:
        if not chunks:
            raise ValueError("retrieval: the loader yielded no batch")
        fa, fv = torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks])
    return fa[:at], fv[:at]


def rank_features(fa, fv, direction="both", return_topk=0):
    """-> ({direction: (R1, R5, R10, MR)}, {direction: (topk_idx, topk_sim)}) from the two feature matrices: audio -> visual ranks the video
    features with the audio features as queries, visual -> audio the other way (src/retrieval.py:84-89)."""
    import torch
    from . import ops
    dirs = DIRECTIONS if direction == "both" else (direction,)
    outs = {d: ops.retrieval_rank(fa, fv, topk=return_topk) if d == "audio" else ops.retrieval_rank(fv, fa, topk=return_topk) for d in dirs}
    host = torch.stack([torch.stack((outs[d]["rank"], outs[d]["ties"])) for d in dirs]).cpu().numpy()      # the only device -> host copy
    results, topk = {}, {}
    for i, d in enumerate(dirs):
        tied = int((host[i, 1] > 0).sum())
        if tied:
            print(f"note: {tied} of {host.shape[2]} queries tie with another gallery entry; optimistic ranks are reported")
        m = metrics_from_ranks(host[i, 0])
        print_computed_metrics(m)
        results[d] = (m["R1"], m["R5"], m["R10"], m["MR"])
        if return_topk:
            topk[d] = (outs[d]["topk_idx"], outs[d]["topk_sim"])
    return results, topk


def get_retrieval_result(audio_model, val_loader, direction='audio', frame_index=5, return_topk=0, exact=False):
    """(R1, R5, R10, MR) of one direction as the reference (src/retrieval.py:62-92); direction='both': {'audio': (...), 'video': (...)} from
    ONE extraction pass.  return_topk=K (1..16): also the top-K gallery indices / similarities of every query (device tensors [N, K]), as a
    second return value of the same form.  exact: extract_features(exact=True)."""
    if direction not in DIRECTIONS + ("both",):
        raise ValueError(f"direction must be 'audio', 'video' or 'both', not {direction!r}")
    fa, fv = extract_features(audio_model, val_loader, frame_index, **({"exact": True} if exact else {}))
    results, topk = rank_features(fa, fv, direction, return_topk)
    res = results if direction == "both" else results[direction]
    if return_topk:
        return res, (topk if direction == "both" else topk[direction])
    return res


def load_model(model, num_class, model_type='finetune', cfg=None):
    """A checkpoint path or state dict -> CAVMAEFT_BASE on the GPU, loaded with strict=False after stripping 'module.'.  'pretrain': a
    CAVMAE_BASE checkpoint goes into the same class - it is how the fine-tuning launcher loads one (run_cavmae_ft_base.py:243-249): the
    encoder keys load, the fusion blocks and heads (not used by retrieval) keep their initial values.  The keys that did not load are
    printed, as the reference prints `msg` (src/retrieval.py:117-118)."""
    import torch
    from .models import CAVMAEFT_BASE
    if model_type not in ("pretrain", "finetune"):
        raise ValueError(f"model_type must be 'pretrain' or 'finetune', not {model_type!r}")
    if isinstance(model, torch.nn.Module):
        return model.cuda()
    sd = torch.load(model, map_location="cpu") if isinstance(model, (str, bytes)) or hasattr(model, "__fspath__") else model
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    net = CAVMAEFT_BASE(label_dim=num_class, cfg=cfg)
    msg = net.load_state_dict(sd, strict=False)
    print(msg)
    return net.cuda()


def eval_retrieval(model, loader, direction, num_class, model_type='finetune', frame_index=5, return_topk=0, cfg=None):
    """The reference's eval_retrieval (src/retrieval.py:94-121) for any loader yielding (a_input, v_input, labels)."""
    net = load_model(model, num_class, model_type, cfg)
    return get_retrieval_result(net, loader, direction, frame_index, return_topk)


# ---- synthetic paired clips -----------------------------------------------------------------------------------------------------------------
class SyntheticPairs:
    """N paired clips without a dataset.  Clip i has a latent z_i ~ N(0, I_k / k) and a grey picture G_i = sum_k z_ik P_k, with the patterns
    P [k, 224, 224] drawn by weights.synth_inputs.  Every frame of the clip is G_i in all three channels (divided by 3) plus noise; its
    spectrogram is made of the SAME 16 x 16 patches - the 196 patches of G_i laid cyclically into the 64 x 8 patch grid of the
    [1024, 128] fbank (transposed: the audio patch embedding sees mel x time) - plus noise.  A freshly constructed model embeds an audio
    patch with the channel mean of the visual kernel (the constructor's initialisation, cav_mae_base.py:291-294), so the two modalities
    of a clip then yield related token sets, and retrieval on untrained weights is neither trivial nor chance; `noise` sets how hard it
    is.  Batches are built on `device`, deterministically from (seed, batch index)."""

    def __init__(self, cfg, n, batch_size, frames=10, seed=87, latent_dim=4, noise=1.0, num_class=2, device="cuda"):
        import dataclasses
        import torch
        from .weights import synth_inputs
        if (cfg.img_size, cfg.patch, cfg.st) != (224, 16, 16) or (cfg.audio_len, cfg.n_mels) != (1024, 128):
            raise ValueError("SyntheticPairs builds 224 x 224 frames and [1024, 128] spectrograms of 16 x 16 patches")
        _, pv = synth_inputs(dataclasses.replace(cfg, frames=1), latent_dim, seed)
        self.p = pv[:, 0].to(device)                                                   # [k, 224, 224]
        self.z = torch.randn(n, latent_dim, generator=torch.Generator().manual_seed(seed)).to(device) / latent_dim ** 0.5
        self.slot = (torch.arange(512) % 196).to(device)                                # audio patch slot -> picture patch
        self.num_clips, self.batch_size, self.frames, self.seed, self.noise, self.num_class, self.device = n, batch_size, frames, seed, noise, num_class, device

    def __len__(self):
        return (self.num_clips + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        import torch
        for i, lo in enumerate(range(0, self.num_clips, self.batch_size)):
            z = self.z[lo:lo + self.batch_size]
            B = z.shape[0]
            g = torch.Generator(device=self.device).manual_seed(self.seed * 100003 + i)
            pic = torch.einsum("bk,khw->bhw", z, self.p)                                                         # [B, 224, 224]
            patches = pic.view(B, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(B, 196, 16, 16)[:, self.slot]  # [B, 512, 16, 16]
            a = patches.transpose(-1, -2).reshape(B, 64, 8, 16, 16).permute(0, 1, 3, 2, 4).reshape(B, 1024, 128)
            a = a + self.noise * torch.randn(a.shape, generator=g, device=self.device)
            v = (pic / 3.0).view(B, 1, 1, 224, 224).expand(B, self.frames, 3, 224, 224)
            v = v + self.noise * torch.randn(v.shape, generator=g, device=self.device)
            yield a.contiguous(), v.contiguous(), torch.zeros(B, self.num_class, device=self.device)


# ---- entry point ----------------------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m avsiam_amd.retrieval", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="audio-visual retrieval evaluation: R@1 / R@5 / R@10 / median rank")
    p.add_argument("--model", type=str, default=None, help="checkpoint (state dict) to evaluate; none: freshly initialised weights")
    p.add_argument("--model-type", dest="model_type", choices=("pretrain", "finetune"), default="pretrain")
    p.add_argument("--direction", choices=DIRECTIONS + ("both",), default="both", help="audio: audio -> visual, video: visual -> audio")
    p.add_argument("--batch-size", dest="batch_size", type=int, default=100)
    p.add_argument("--frame-use", dest="frame_use", type=int, default=5, help="the frame of each clip that represents it")
    p.add_argument("--frames", type=int, default=10, help="frames per synthetic clip")
    p.add_argument("--num-class", dest="num_class", type=int, default=309)
    p.add_argument("--topk", type=int, default=0, help="also print the top-K gallery indices of the first queries (0..16)")
    p.add_argument("--out", type=str, default="retrieval_result.csv", help="rows dataset,direction,r1,r5,r10,mr")
    p.add_argument("--dataset", type=str, default="synthetic", help="name written into the first column")
    p.add_argument("--synthetic", type=int, default=0, metavar="N", help="evaluate on N paired synthetic clips")
    p.add_argument("--seed", type=int, default=87)
    p.add_argument("--exact", action="store_true", help="features from the exact-fp32 forward (fine-tuned models; slower)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.synthetic <= 0:
        raise SystemExit("no dataset reader here (the reference's needs torchaudio): pass --synthetic N, or call eval_retrieval(model, loader, ...) "
                         "with a loader yielding (a_input, v_input, labels)")
    if not 0 <= args.topk <= 16:
        raise SystemExit("--topk must lie in 0..16")
    if not 0 <= args.frame_use < args.frames:
        raise SystemExit(f"--frame-use {args.frame_use} needs clips of more than {args.frame_use} frames (--frames {args.frames})")
    from .config import AVSiamConfig
    from .models import CAVMAEFT_BASE
    cfg = AVSiamConfig()
    net = load_model(args.model, args.num_class, args.model_type) if args.model else CAVMAEFT_BASE(label_dim=args.num_class).cuda()
    loader = SyntheticPairs(cfg, args.synthetic, args.batch_size, frames=args.frames, seed=args.seed, num_class=args.num_class, device=net.arena.p.device)
    got = get_retrieval_result(net, loader, args.direction, args.frame_use, args.topk, **({"exact": True} if args.exact else {}))
    res, topk = got if args.topk else (got, None)
    if args.direction != "both":
        res, topk = {args.direction: res}, {args.direction: topk}
    rows = [[args.dataset, d] + list(res[d]) for d in ("video", "audio") if d in res]          # the reference's order (src/retrieval.py:128)
    if args.topk:
        for d in res:
            print(f"top-{args.topk} of the first queries ({d}):", topk[d][0][:4].tolist())
    np.savetxt(args.out, rows, delimiter=',', fmt='%s')
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
