"""Fine-tuning from files: the CAV-MAE json / label csv / WAV / frame dataset behind --data_train / --data_val / --label_csv, and the loader that
feeds it to the device front end (the reference's AudiosetDataset, dataloader_ft.py, without its video and sqlite readers).

Data format.  The json is {"data": [{"wav", "labels", "video_id", "video_path"}, ...]} (pro_data, :198-202), `labels` a comma-separated list of
mids; the label csv has the columns index,mid,display_name (make_index_dict, :33-41).  A clip's frame k lies at
video_path/frame_{k}/{video_id}.npy (uint8 [H, W, 3]; always read) or .jpg / .png (read with PIL where it is importable); a missing frame falls
back to the next lower index, as randselect_img does (:344-359).  Audio: WAV files that preprocess.parse_wav accepts.  Not built: mp4 / video
decoding and compressed audio.

Who does what.  Every random draw of an epoch comes from ONE numpy Generator in the main process, seeded by (seed, epoch, rank): the epoch's
draws are made before the first file is opened, so they cannot depend on the number of workers.  Per training item, in this order:
partner = integers(0, n) (:372), u = random() - the item is mixed when u < mixup (:420) -, then for a mixed item lam = beta(10, 10) (:424) and
weight = random() (:457), and frame = integers(0, total_frame) (:352, :459; the partner is read at the same frame index, as :458-459 mix before they
pick).  Evaluation draws nothing: the frame is frame_use, the middle frame int(total_frame / 2) (:348), or all total_frame frames.  The
workers (torch.utils.data.DataLoader) read and parse the WAV files and read the frames; the main process packs the batch
(FileFtLoader.collate): payload bytes into a pinned [B, byte_stride] staging buffer, frames into one padded [B, F, 3, Hmax, Wmax] uint8 buffer
with per-clip sizes, both uploaded with non-blocking copies.

Channel counts.  ops.resample_wave divides by one channel count per call and the reference resamples per channel before the mean, so a batch's
payloads are STAGED ordered by channel count and decode + resample run once per distinct count, on a contiguous slice of the staging rows.
The 16 kHz rows are written back to the clips' own batch rows (the copy into the common [B, S] buffer that the fbank reads happens anyway),
so the batch itself keeps its drawn order: labels, frames and - in validation, where data-parallel shards are padded at their END and
truncated after the gather - targets never move.  The partners are staged the same way, in their own order.

A clip that cannot be read is reported by name (once), replaced by one second of silence (audio) or a grey frame (frames), keeps its labels
and is counted in FileFtLoader.n_bad, the number of DISTINCT clips replaced so far - the reference substitutes constants and prints
(:425-430, :463-465); strict=True raises instead.  "Cannot be read" includes a WAV without a sample frame and a rate that ops.resample_wave
refuses (preprocess.resample_rate_problem): both are known when the header is parsed, so neither can stop an epoch half way.

Processes.  A worker is forked from the process that holds the GPU and inherits its open device, so it counts as a process with the GPU
open.  worker_share keeps one machine at MAX_PROCESSES = 16 such processes (and as many busy CPUs): ranks x (1 + the workers of all file
loaders of a rank) <= 16.  Only a training loader keeps its workers between epochs; an evaluation loader's workers end with every pass."""
import csv
import json
import os

import numpy as np
import torch

from . import preprocess

FRAME_EXTS = (".npy", ".jpg", ".png")
SILENCE_RATE, SILENCE_FRAMES = 16000, 16000                  # what stands in for unreadable audio: one second of S16 mono zeros
GREY_SIZE = 8                                                # ... and for unreadable frames: GREY_SIZE x GREY_SIZE pixels of 128
MAX_FRAME_SIDE = 2240                                        # ops.resize_frames: at most 10 x the model's 224 per axis
MAX_PROCESSES = 16                                           # processes of one machine that may hold the GPU open: the ranks and all their workers


def worker_share(requested, loaders=1, ranks=1):
    """the workers ONE file loader may start when a machine runs `ranks` processes that each own `loaders` file loaders:
    ranks * (1 + loaders * workers) <= MAX_PROCESSES, and no more than was asked for"""
    room = MAX_PROCESSES // max(1, int(ranks)) - 1               # what a rank may fork beside itself
    return max(0, min(int(requested), room // max(1, int(loaders))))


def rate_groups(channels, rates, max_rates=8):
    """staged rows (ordered by channel count) -> the [start, end) slices that one decode + resample call takes: rows of one channel count
    with at most `max_rates` distinct rates other than 16 kHz (ops.resample_wave's limit per call)"""
    out, s, seen = [], 0, set()
    for r in range(len(channels) + 1):
        new = set() if r == len(channels) or rates[r] == SILENCE_RATE else {rates[r]}
        if r == len(channels) or channels[r] != channels[s] or len(seen | new) > max_rates:
            if r > s:
                out.append((s, r))
            s, seen = r, set()
        seen |= new
    return out


def make_index_dict(label_csv):
    """mid -> class index of a label csv with the columns index,mid,display_name"""
    with open(label_csv, "r", newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows or "mid" not in rows[0] or "index" not in rows[0]:
        raise ValueError(f"{label_csv}: a label csv has the columns index,mid,display_name")
    return {r["mid"]: int(r["index"]) for r in rows}


def find_frame(video_path, video_id, k, exts=FRAME_EXTS, say=print):
    """the path of frame k of a clip, falling back to the next lower index while the frame is missing (:354-357) -> (path or None, index used)"""
    while True:
        for ext in exts:
            p = os.path.join(video_path, f"frame_{k}", video_id + ext)
            if os.path.exists(p):
                return p, k
        if k < 1:
            return None, k
        say(f"{video_id}: no frame_{k} under {video_path}, trying frame_{k - 1}")
        k -= 1


def read_frame(path):
    """one frame file -> uint8 [3, H, W]"""
    if path.endswith(".npy"):
        x = np.load(path, allow_pickle=False)
    else:
        from PIL import Image
        with Image.open(path) as im:
            x = np.asarray(im.convert("RGB"))
    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3 or not (1 <= x.shape[0] <= MAX_FRAME_SIDE and 1 <= x.shape[1] <= MAX_FRAME_SIDE):
        raise ValueError(f"{path}: a frame is uint8 [H, W, 3] with H, W in 1 .. {MAX_FRAME_SIDE}, got {x.dtype} {x.shape}")
    return np.ascontiguousarray(x.transpose(2, 0, 1))


class FtFileDataset(torch.utils.data.Dataset):
    """The host side: entries of the json, their multi-hot labels, and __getitem__((index, frame indices)) -> what a worker reads for one clip:
    {"index", "wav", "info" (preprocess.WavInfo), "payload" (uint8 tensor, the data chunk's whole frames), "frames" (uint8 [F, 3, H, W]),
    "frame_used" (the indices the fallback ended on), "audio_error" / "frame_error" (None, or the reason as text)}."""

    def __init__(self, data_json, label_csv, n_class=None, say=print):
        with open(data_json, "r") as f:
            data = json.load(f)["data"]
        self.path, self.say = data_json, say
        self.entries = [(str(d["wav"]), str(d["labels"]), str(d["video_id"]), str(d["video_path"])) for d in data]
        if not self.entries:
            raise ValueError(f"{data_json}: no clips")
        self.index_dict = make_index_dict(label_csv)
        self.n_class = len(self.index_dict) if n_class is None else int(n_class)
        if self.n_class != len(self.index_dict):
            raise ValueError(f"n_class {self.n_class} does not match {label_csv}: it lists {len(self.index_dict)} classes")
        if sorted(self.index_dict.values()) != list(range(self.n_class)):
            raise ValueError(f"{label_csv}: the index column must number the classes 0 .. {self.n_class - 1}")
        try:
            import PIL  # noqa: F401
            self.exts = FRAME_EXTS
        except ImportError:
            self.exts = FRAME_EXTS[:1]
        self.hot = np.zeros((len(self.entries), self.n_class), dtype=np.float32)
        for i, (_, labels, _, _) in enumerate(self.entries):
            for mid in labels.split(","):
                if mid.strip() not in self.index_dict:
                    raise ValueError(f"{data_json}: clip {i} has the label {mid!r}, which {label_csv} does not list")
                self.hot[i, self.index_dict[mid.strip()]] = 1.0

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, request):
        index, frames = request
        wav, _, video_id, video_path = self.entries[index]
        item = {"index": index, "wav": wav, "audio_error": None, "frame_error": None, "info": None, "payload": None, "frames": None, "frame_used": []}
        try:
            raw = np.fromfile(wav, dtype=np.uint8)
            info = preprocess.parse_wav(raw, name=wav)
            if info.n_frames < 1:
                raise ValueError(f"{wav}: the data chunk holds no sample frame")
            problem = preprocess.resample_rate_problem(info.rate, SILENCE_RATE)
            if problem:
                raise ValueError(f"{wav}: {problem}")
            item["info"] = info
            # (torch tensors: a worker hands them to the main process through shared memory, a numpy array would be pickled through a pipe)
            item["payload"] = torch.from_numpy(raw[info.data_offset:info.data_offset + info.data_bytes])
        except (OSError, ValueError) as e:
            item["audio_error"] = f"{wav}: {e}" if isinstance(e, OSError) else str(e)
        try:
            got = []
            for k in frames:
                p, used = find_frame(video_path, video_id, int(k), self.exts, self.say)
                if p is None:
                    raise ValueError(f"{video_path}: no frame of {video_id} at or below frame_{int(k)} ({', '.join(self.exts)})")
                got.append(read_frame(p))
                item["frame_used"].append(used)
            if any(g.shape != got[0].shape for g in got):
                raise ValueError(f"{video_path}: the frames of {video_id} differ in size: {sorted({g.shape[1:] for g in got})}")
            item["frames"] = torch.from_numpy(np.stack(got))
        except (OSError, ValueError) as e:
            item["frame_error"] = str(e)
        return item


def _keep(items):
    """the DataLoader's collate function: the workers' items as they are (the batch is packed in the main process, where pinned memory lives)"""
    return items


class _Requests:
    """the DataLoader's batch sampler: the current epoch's requests, swapped by the loader before every epoch"""

    def __init__(self):
        self.batches = []

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class _Sampler:
    """what validate() asks of a sampler: len(sampler.dataset), the examples before the shards were padded"""

    def __init__(self, dataset):
        self.dataset = dataset


class FileFtLoader:
    """Batches of a FtFileDataset through the device front end; iterating yields what SyntheticWaveFtLoader yields, (a, v, labels):
      a       ops.decode_pcm -> ops.resample_wave -> ops.kaldi_fbank(partner=, lam=, norm=): fp32 [B, target_length, 128], normalised
      v       ops.resize_frames(partner=, weight=): fp32 [B, F, 3, 224, 224]
      labels  preprocess.mixup_labels with label_smooth
    train=True: a new permutation per epoch, rank r of `world` takes every world-th index of it, and the tail is dropped (per rank and per
    batch) so that every rank runs the same number of steps; mixup as the module docstring states.  train=False: the clips in order, in
    contiguous shards padded (by repeating the last clip) to equal length - validate() truncates the gathered predictions to len(dataset);
    frames: 'middle' (frame_use -1), an int (frame_use), or 'all' (total_frame frames per clip).
    num_workers is cut to MAX_PROCESSES - 1 here; a caller with several file loaders or ranks shares them out with worker_share.  Only a
    training loader keeps its workers between epochs; close() ends them.
    The draws of the last batch are in `last_draw` (index, partner, lam, weight, frame, in the batch's order); `n_bad` is the number of
    distinct clips replaced so far (`bad_clips`: their dataset indices)."""

    def __init__(self, dataset, cfg, batch_size, device, seed=87, label_smooth=0.1, mixup=0.0, norm=(-5.081, 4.4849), train=True, frames="middle",
                 total_frame=10, num_workers=0, rank=0, world=1, strict=False, say=print):
        self.ds, self.B, self.device = dataset, int(batch_size), torch.device(device)
        self.seed, self.label_smooth, self.norm, self.train = int(seed), float(label_smooth), norm, bool(train)
        self.mixup = float(mixup) if train else 0.0
        self.total_frame = int(total_frame)
        if self.total_frame < 1 or self.B < 1:
            raise ValueError(f"FileFtLoader: batch_size {batch_size}, total_frame {total_frame}: positive integers")
        if not train and frames not in ("middle", "all") and not (isinstance(frames, int) and 0 <= frames < self.total_frame):
            raise ValueError(f"FileFtLoader: frames {frames!r}: 'middle', 'all' or a frame index in 0 .. {self.total_frame - 1}")
        self.frames = frames
        self.num_workers = worker_share(num_workers)
        self.rank, self.world, self.strict, self.say = int(rank), int(world), bool(strict), say
        self.T, self.img_size = cfg.audio_len, cfg.img_size
        self.sampler = _Sampler(dataset)
        self.epoch, self.bad_clips, self.last_draw = 0, set(), None
        self.hot = torch.from_numpy(dataset.hot)
        self._requests, self._loader = _Requests(), None

    # ---- the plan of an epoch: indices and draws, all in the main process ------------------------------------------------------------------------
    def indices(self, epoch):
        n = len(self.ds)
        if self.train:
            perm = np.random.default_rng([self.seed, epoch]).permutation(n)      # one permutation for all ranks
            mine = perm[self.rank::self.world][:n // self.world] if n >= self.world else perm[:0]
            steps = len(mine) // self.B if len(mine) >= self.B else (1 if len(mine) else 0)
            return [mine[s * self.B:(s + 1) * self.B] for s in range(steps)]
        per = -(-n // self.world)
        mine = np.minimum(np.arange(self.rank * per, (self.rank + 1) * per), n - 1)
        return [mine[s:s + self.B] for s in range(0, per, self.B)]

    def __len__(self):
        return len(self.indices(0))

    @property
    def n_bad(self):
        return len(self.bad_clips)

    def close(self):
        """end the workers (a training loader keeps them between epochs)"""
        self._loader = None

    def eval_frames(self):
        if self.frames == "all":
            return tuple(range(self.total_frame))
        return (int(self.total_frame / 2) if self.frames == "middle" else int(self.frames),)

    def plan(self, epoch):
        """-> the epoch's batches: dicts of numpy arrays index, partner (-1: none), lam (-1: not mixed), weight (1: not mixed) and frame [B, F]"""
        rng = np.random.default_rng([self.seed, epoch, self.rank + 1])
        n, out = len(self.ds), []
        for idx in self.indices(epoch):
            B = len(idx)
            d = {"index": np.asarray(idx, dtype=np.int64), "partner": np.full(B, -1, dtype=np.int64), "lam": np.full(B, -1.0, dtype=np.float32),
                 "weight": np.ones(B, dtype=np.float32)}
            if self.train:
                d["frame"] = np.zeros((B, 1), dtype=np.int64)
                for b in range(B):
                    partner = int(rng.integers(0, n))
                    if rng.random() < self.mixup:
                        d["partner"][b], d["lam"][b], d["weight"][b] = partner, rng.beta(10, 10), rng.random()
                    d["frame"][b, 0] = rng.integers(0, self.total_frame)
            else:
                d["frame"] = np.tile(np.asarray(self.eval_frames(), dtype=np.int64), (B, 1))
            out.append(d)
        return out

    # ---- one batch: host side ------------------------------------------------------------------------------------------------------------------
    def _replace_bad(self, item):
        errs = [e for e in (item["audio_error"], item["frame_error"]) if e]
        if errs and self.strict:
            raise RuntimeError("unreadable clip (--strict-data): " + "; ".join(errs))
        if errs and item["index"] not in self.bad_clips:         # (a clip drawn again, as a partner or as validation padding: said and counted once)
            self.bad_clips.add(item["index"])
            for e in errs:
                self.say(f"unreadable clip {item['index']}, {'silence' if e is item['audio_error'] else 'a grey frame'} stands in: {e}", flush=True)
        return bool(errs)

    def _stage_audio(self, items, order):
        """items in `order` -> {"payload": pinned uint8 [n, byte_stride], "desc": int32 [n, 2] = (format, n_frames), "channels", "rates", "n_frames"}"""
        infos = [items[i]["info"] or preprocess.WavInfo(preprocess.PCM_S16, 1, SILENCE_RATE, SILENCE_FRAMES, 0, 2 * SILENCE_FRAMES) for i in order]
        byte_stride = max(16, -(-max(f.data_bytes for f in infos) // 16) * 16)
        pin = torch.cuda.is_available()
        stage = torch.empty((len(order), byte_stride), dtype=torch.uint8, pin_memory=pin)
        for r, (i, f) in enumerate(zip(order, infos)):
            if items[i]["payload"] is not None:
                stage[r, :f.data_bytes] = items[i]["payload"]
                stage[r, f.data_bytes:] = 0                    # (the slack is never decoded; it is zeroed so that a batch's bytes are defined)
            else:
                stage[r] = 0
        desc = torch.tensor([[f.format, f.n_frames] for f in infos], dtype=torch.int32)
        return {"payload": stage, "desc": desc, "channels": [f.channels for f in infos], "rates": [f.rate for f in infos], "n_frames": [f.n_frames for f in infos]}

    def _stage_frames(self, items, F):
        """-> (pinned uint8 [n, F, 3, Hmax, Wmax], sizes int32 [n, 2]); a clip without frames: grey"""
        got = [it["frames"] if it["frames"] is not None else torch.full((F, 3, GREY_SIZE, GREY_SIZE), 128, dtype=torch.uint8) for it in items]
        H, W = max(g.shape[2] for g in got), max(g.shape[3] for g in got)
        buf = torch.empty((len(got), F, 3, H, W), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        for r, g in enumerate(got):
            if tuple(g.shape[2:]) != (H, W):
                buf[r] = 0                                     # the padding of a smaller clip
            buf[r, :, :, :g.shape[2], :g.shape[3]] = g
        return buf, np.asarray([[g.shape[2], g.shape[3]] for g in got], dtype=np.int32)

    def collate(self, pairs, draw):
        """the workers' (clip, partner) items of one batch and its draws -> the staged batch (host tensors, pinned where a GPU is there) and the
        draws.  The audio is staged ordered by channel count (stable); "audio_rows" / "partner_rows" name the batch row of every staged row"""
        clips = [p[0] for p in pairs]
        for it in clips + [p[1] for p in pairs if p[1] is not None]:
            self._replace_bad(it)
        ch = [(it["info"].channels if it["info"] is not None else 1) for it in clips]
        order = sorted(range(len(clips)), key=lambda i: ch[i])                      # stable: equal counts keep the drawn order
        F = draw["frame"].shape[1]
        batch = {"draw": draw, "F": F, "audio_rows": order}
        batch["audio"] = self._stage_audio(clips, order)
        batch["frames"], batch["sizes"] = self._stage_frames(clips, F)
        mixed = [b for b, p in enumerate(pairs) if p[1] is not None]
        batch["mixed"] = mixed
        if mixed:
            partners = [p[1] for p in pairs]
            ch2 = {b: (partners[b]["info"].channels if partners[b]["info"] is not None else 1) for b in mixed}
            rows = sorted(mixed, key=lambda b: ch2[b])                              # the partners' own order; `rows` scatters them back
            batch["partner_rows"] = rows
            batch["partner_audio"] = self._stage_audio(partners, rows)
            grey = {"frames": None}
            batch["partner_frames"], batch["partner_sizes"] = self._stage_frames([partners[b] if b in ch2 else grey for b in range(len(pairs))], F)
        draw["frame_used"] = np.asarray([c["frame_used"] if c["frames"] is not None else [-1] * F for c in clips], dtype=np.int64)
        return batch

    # ---- one batch: device side ----------------------------------------------------------------------------------------------------------------
    def _audio(self, audio, rows, B):
        """staged payloads (rows sorted by channel count) -> (16 kHz mono fp32 [B, S], lengths int32 [B]): staged row r lands in batch row rows[r];
        decode + resample once per distinct channel count, on the contiguous slice of rows that share it (rate_groups: a slice with more
        distinct rates than one resample call takes is cut again)"""
        from . import ops
        dev, channels = self.device, audio["channels"]
        payload, desc = audio["payload"].to(dev, non_blocking=True), audio["desc"].to(dev, non_blocking=True)
        parts = []
        for s, e in rate_groups(channels, audio["rates"]):
            stride = max(4, -(-max(audio["n_frames"][s:e]) // 4) * 4)           # the group's longest clip, a multiple of 4 (16-byte stores)
            pcm, n = ops.decode_pcm(payload[s:e], desc[s:e], channels[s], stride)
            parts.append((s, e) + ops.resample_wave(pcm, audio["rates"][s:e], n))
        S = max(400, max(p[2].shape[1] for p in parts))                         # (ops.kaldi_fbank wants a row of at least one frame)
        wave = torch.zeros((B, S), dtype=torch.float32, device=dev)
        lengths = torch.ones(B, dtype=torch.int32, device=dev)
        rows = list(rows)
        ridx = None if rows == list(range(B)) else torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
        for s, e, w, n in parts:
            where = slice(s, e) if ridx is None else ridx[s:e]
            wave[where, :w.shape[1]] = w
            lengths[where] = n
        return wave, lengths

    def front_end(self, batch):
        """a staged batch -> (a, v, labels) on the device; no host synchronisation"""
        from . import ops
        d, dev = batch["draw"], self.device
        B = len(d["index"])
        wave, lengths = self._audio(batch["audio"], batch["audio_rows"], B)
        frames = batch["frames"].to(dev, non_blocking=True)
        hot = self.hot[torch.from_numpy(d["index"])].to(dev, non_blocking=True)
        if batch["mixed"]:
            wave2, lengths2 = self._audio(batch["partner_audio"], batch["partner_rows"], B)
            lam = torch.from_numpy(d["lam"]).to(dev, non_blocking=True)
            a = ops.kaldi_fbank(wave, lengths, partner=wave2, partner_lengths=lengths2, lam=lam, target_length=self.T, norm=self.norm)
            v = ops.resize_frames(frames, batch["sizes"], partner=batch["partner_frames"].to(dev, non_blocking=True), partner_sizes=batch["partner_sizes"],
                                  weight=torch.from_numpy(d["weight"]).to(dev, non_blocking=True), size=self.img_size)
            hot2 = self.hot[torch.from_numpy(np.maximum(d["partner"], 0))].to(dev, non_blocking=True)
            y = preprocess.mixup_labels(hot, hot2, lam, self.label_smooth)
        else:
            a = ops.kaldi_fbank(wave, lengths, target_length=self.T, norm=self.norm)
            v = ops.resize_frames(frames, batch["sizes"], size=self.img_size)
            y = preprocess.mixup_labels(hot, None, -1.0, self.label_smooth)
        return a, v, y

    # ---- iteration -----------------------------------------------------------------------------------------------------------------------------
    def requests(self, plan):
        """the DataLoader's batch sampler: per batch, the (clip request, partner request or None) pairs the workers serve"""
        for d in plan:
            yield [((int(i), tuple(int(k) for k in f)), ((int(p), tuple(int(k) for k in f)) if p >= 0 else None))
                   for i, p, f in zip(d["index"], d["partner"], d["frame"])]

    def staged(self, epoch=None):
        """the epoch's batches, staged on the host (what the loader's host side costs: read, parse, collate)"""
        epoch = self.epoch if epoch is None else epoch
        plan = self.plan(epoch)
        if self._loader is None:
            # a training loader starts its workers once and keeps them across epochs (starting a worker from a process that holds a GPU context
            # is slow); every epoch hands them its own requests through the batch sampler, which the DataLoader reads in the main process.  An
            # evaluation loader's workers end with every pass, so they do not idle beside the training workers.
            self._loader = torch.utils.data.DataLoader(_Pairs(self.ds), batch_sampler=self._requests, collate_fn=_keep, num_workers=self.num_workers,
                                                       persistent_workers=self.train and self.num_workers > 0)
        self._requests.batches = list(self.requests(plan))
        for pairs, d in zip(self._loader, plan):                   # (the DataLoader first: it sees its own end, where an evaluation loader's workers leave)
            yield self.collate(pairs, d)

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        for batch in self.staged(epoch):
            self.last_draw = batch["draw"]
            yield self.front_end(batch)


class _Pairs(torch.utils.data.Dataset):
    """(clip request, partner request or None) -> the two items"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, request):
        clip, partner = request
        return self.ds[clip], (self.ds[partner] if partner is not None else None)
