"""Training from files on a real MI355X: the PCM decode kernel (ops.decode_pcm = avs_decode_pcm) against its numpy restatement bit for bit
(preprocess.decode_pcm_reference, which tests/test_decode_cpu.py holds to scipy's samples), WAV files through parse_wav -> the loader's collate
-> decode -> resample -> fbank against the float64 chain on the same quantised samples, and the file loader, a training step and the launcher
on a five-clip dataset.

The decode is exact for PCM16 and PCM24, so the chain test introduces no tolerance: the energy and log bounds and the cap on excluded cells are
those of tests/test_resample_gpu.py, imported from there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avsiam_amd import preprocess as pp
from avsiam_amd.config import AVSiamConfig
from tests.filedata import make_dataset, quantise, wav_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT, ISENT = -123.5, -777
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [pp.PCM_U8, pp.PCM_S16, pp.PCM_S24, pp.PCM_S32, pp.PCM_F32, pp.PCM_F64]
RAGGED = [0, 1, 1023, 1024, 1025, 2049]                       # the tile tails and the second tile (csrc/decode.hip DP_TILE = 1024)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def random_payload(rng, fmt, channels, n):
    """n frames whose samples cover the format: every byte pattern for the integer formats and F32 (NaN payloads, -0.0, subnormals, inf among
    them); doubles over 100 decades for F64 (overflow to inf, fp32 subnormals, underflow to zero; no NaN: its payload is not specified)"""
    if fmt == pp.PCM_F64:
        x = rng.standard_normal(n * channels) * 10.0 ** rng.uniform(-50, 50, n * channels)
        x[:min(6, x.size)] = [1e39, -1e39, 1e-40, -1e-46, -0.0, 1.0 + 2.0 ** -24][:min(6, x.size)]
        return x.astype("<f8").tobytes()
    return rng.integers(0, 256, n * channels * pp.PCM_BYTES[fmt], dtype=np.uint8).tobytes()


def stage(payloads, slack=48):
    """payload rows whose slack holds 0xA5 -> uint8 [B, byte_stride] on the device"""
    byte_stride = -(-(max(len(p) for p in payloads) + slack) // 16) * 16
    rows = np.full((len(payloads), byte_stride), 0xA5, dtype=np.uint8)
    for r, p in enumerate(payloads):
        rows[r, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return torch.from_numpy(rows).to(DEV)


def run_guarded(payload, desc, C, stride, lead=64):
    """ops.decode_pcm into an output and a length vector that sit between sentinels -> (out, out_lengths), both checked"""
    B = payload.shape[0]
    buf = torch.full((B * C * stride + lead + 64,), SENT, dtype=torch.float32, device=DEV)
    lbuf = torch.full((B + 16,), ISENT, dtype=torch.int32, device=DEV)
    out, ol = buf[lead:lead + B * C * stride].view(B, C, stride), lbuf[8:8 + B]
    got, got_l = ops().decode_pcm(payload, desc, C, stride, out=out, out_lengths=ol)
    assert got.data_ptr() == out.data_ptr() and got_l.data_ptr() == ol.data_ptr()
    assert bool((buf[:lead] == SENT).all()) and bool((buf[lead + B * C * stride:] == SENT).all()), "the kernel wrote outside its output"
    assert bool((lbuf[:8] == ISENT).all()) and bool((lbuf[8 + B:] == ISENT).all()), "the kernel wrote outside out_lengths"
    assert not bool((bits(out) == bits(torch.tensor([SENT], device=DEV))).all(dim=-1).any()), "a row of the output was not written"
    return got, got_l


def expected(payloads, fmts, C, lengths, stride):
    want = np.zeros((len(payloads), C, stride), dtype=np.float32)
    for b, (p, f, n) in enumerate(zip(payloads, fmts, lengths)):
        want[b, :, :n] = pp.decode_pcm_reference(p, f, C, n)
    return torch.from_numpy(want.view(np.int32)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement, bit for bit
@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS, ids=pp.PCM_NAMES)
def test_kernel_is_the_restatement(fmt, C):
    rng = np.random.default_rng(1000 + 10 * fmt + C)
    payloads = [random_payload(rng, fmt, C, n) for n in RAGGED]
    payload, desc, stride = stage(payloads), [[fmt, n] for n in RAGGED], 2052
    got, got_l = run_guarded(payload, desc, C, stride)
    assert got_l.tolist() == RAGGED
    want = expected(payloads, [fmt] * 6, C, RAGGED, stride)
    assert torch.equal(bits(got), want), [(b, int((bits(got[b]) != want[b]).sum())) for b in range(6)]
    for b, n in enumerate(RAGGED):                              # zero beyond each length (as bits: -0.0 would not do)
        assert not bool(bits(got[b, :, n:]).any())
    again, again_l = ops().decode_pcm(payload, desc, C, stride)
    assert torch.equal(bits(again), bits(got)) and torch.equal(again_l, got_l)          # two calls: identical bytes
    for b, n in enumerate(RAGGED):                              # each clip alone gives its row's bytes
        alone, alone_l = run_guarded(payload[b:b + 1], [[fmt, n]], C, stride)
        assert torch.equal(bits(alone[0]), bits(got[b])) and alone_l.tolist() == [n]


@pytest.mark.parametrize("fmt,C", [(pp.PCM_S16, 2), (pp.PCM_S24, 1), (pp.PCM_F64, 3), (pp.PCM_U8, 1)], ids=["S16x2", "S24x1", "F64x3", "U8x1"])
def test_rows_that_are_not_16_byte_aligned(fmt, C):
    """a stride that is no multiple of 4 and an output that starts 4 bytes off a 16-byte boundary: the scalar stores write the same values"""
    rng = np.random.default_rng(2000 + 10 * fmt + C)
    payloads = [random_payload(rng, fmt, C, n) for n in RAGGED]
    for stride, lead in ((2051, 64), (2052, 61), (2049, 63)):
        got, got_l = run_guarded(stage(payloads), [[fmt, n] for n in RAGGED], C, stride, lead=lead)
        assert got_l.tolist() == RAGGED and torch.equal(bits(got), expected(payloads, [fmt] * 6, C, RAGGED, stride))


def test_one_call_mixes_formats_and_cuts_device_side_lengths():
    rng = np.random.default_rng(3000)
    C, stride = 2, 1500
    held = [1300, 1400, 1500, 1100, 1200, 1024]                 # frames the rows really hold, per format
    payloads = [random_payload(rng, f, C, n) for f, n in zip(FORMATS, held)]
    payload = stage(payloads, slack=0)
    got, got_l = run_guarded(payload, [[f, n] for f, n in zip(FORMATS, held)], C, stride)
    assert got_l.tolist() == held and torch.equal(bits(got), expected(payloads, FORMATS, C, held, stride))
    # device-side descriptors are taken at their word and cut on the device: to the output row, to the payload row, to zero
    byte_stride = payload.shape[1]
    claims = [10 ** 9, 2 ** 31 - 1, 1501, -5, 1200, 5000]
    cut = [max(0, min(n, stride, byte_stride // (C * pp.PCM_BYTES[f]))) for f, n in zip(FORMATS, claims)]
    assert cut == [1500, 1500, 1500, 0, 1200, 1024]            # the output row three times, the sign, as claimed, the payload row (F64: 16 384 bytes)
    desc = torch.tensor([[f, n] for f, n in zip(FORMATS, claims)], dtype=torch.int32, device=DEV)
    got, got_l = run_guarded(payload, desc, C, stride)
    assert got_l.tolist() == cut
    rows = payload.cpu().numpy()
    assert torch.equal(bits(got), expected([rows[b].tobytes() for b in range(6)], FORMATS, C, cut, stride))
    # an unknown format decodes to nothing
    desc = torch.tensor([[6, 100], [-1, 100], [1, 100], [99, 100], [2, 7], [0, 0]], dtype=torch.int32, device=DEV)
    got, got_l = run_guarded(payload, desc, C, stride)
    assert got_l.tolist() == [0, 0, 100, 0, 7, 0] and not bool(bits(got[0]).any()) and not bool(bits(got[3]).any())


def test_wrapper_refusals():
    from avsiam_amd._lib import AvsiamHipError
    o = ops()
    pay = torch.zeros((2, 64), dtype=torch.uint8, device=DEV)
    for bad in ([[6, 1], [0, 1]], [[-1, 1], [0, 1]], [[1, 17], [1, 1]], [[1, 9], [1, 1]], [[1, -1], [1, 1]]):      # format, row bytes (C = 2), stride, sign
        with pytest.raises(ValueError):
            o.decode_pcm(pay, bad, 2, 8)
    for bad in (lambda: o.decode_pcm(pay, [[1, 1]], 2, 8), lambda: o.decode_pcm(pay, [[1, 1]] * 2, 9, 8), lambda: o.decode_pcm(pay, [[1, 1]] * 2, 0, 8),
                lambda: o.decode_pcm(pay, [[1, 1]] * 2, 1, 0), lambda: o.decode_pcm(pay.cpu(), [[1, 1]] * 2, 1, 8),
                lambda: o.decode_pcm(pay.float(), [[1, 1]] * 2, 1, 8), lambda: o.decode_pcm(pay[:, :40], [[1, 1]] * 2, 1, 8),
                lambda: o.decode_pcm(torch.zeros((2, 40), dtype=torch.uint8, device=DEV), [[1, 1]] * 2, 1, 8),
                lambda: o.decode_pcm(torch.zeros(2 * 64 + 16, dtype=torch.uint8, device=DEV)[8:8 + 128].view(2, 64), [[1, 1]] * 2, 1, 8),
                lambda: o.decode_pcm(pay, torch.zeros((2, 2), dtype=torch.int64, device=DEV), 1, 8),
                lambda: o.decode_pcm(pay, [[1, 1]] * 2, 1, 8, out=torch.empty((2, 1, 9), device=DEV)),
                lambda: o.decode_pcm(pay, [[1, 1]] * 2, 1, 8, out_lengths=torch.empty(3, dtype=torch.int32, device=DEV))):
        with pytest.raises(AvsiamHipError):
            bad()
    got, got_l = o.decode_pcm(pay, [[1, 8], [1, 0]], 2, 8)
    assert got.shape == (2, 2, 8) and got_l.tolist() == [8, 0] and not bool(got.any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. files -> parse_wav -> collate -> decode -> resample -> fbank against the float64 chain
class FrontCfg:
    audio_len, img_size = 1024, 224


CHAIN_CLIPS = [(pp.PCM_S16, 2, 44100, 52920), (pp.PCM_S24, 1, 48000, 57001)]       # 1.2 s stereo PCM16, 1.19 s mono PCM24 (an extensible fmt)


def chain_signals():
    """the Gaussian-noise and noise-plus-tone signals of tests/test_resample_gpu.py's chain test (its generator, its seed)"""
    from tests.test_resample_gpu import FB_LENGTHS, FB_RATES
    assert FB_RATES == [c[2] for c in CHAIN_CLIPS] and FB_LENGTHS == [c[3] for c in CHAIN_CLIPS]
    rng = np.random.default_rng(20241017)
    S = max(FB_LENGTHS) + 3
    noise = (rng.standard_normal((2, 2, S)) * 0.1).astype(np.float32)
    t = np.arange(S)[None, None, :] / np.asarray(FB_RATES, dtype=np.float64)[:, None, None]
    return {"noise": noise, "tone": (noise + 0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)}


def float64_chain(payloads):
    """kaldi_fbank_reference(resample_reference(.)) in float64 on the quantised samples, clip by clip -> (energies, frames, lengths)"""
    energies, frames, lengths = [], [], []
    for (fmt, C, rate, n), p in zip(CHAIN_CLIPS, payloads):
        x = pp.decode_pcm_reference(p, fmt, C).astype(np.float64)
        r64, ol = pp.resample_reference(x[None], [rate], [n])
        m = pp.fbank_frames(int(ol[0]))
        _, e = pp.kaldi_fbank_reference(r64, ol, target_length=m, return_energy=True)
        energies.append(e[0]); frames.append(m); lengths.append(int(ol[0]))
    return energies, frames, lengths


def test_fbank_of_decoded_files(tmp_path):
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    from tests.helpers import record_margin
    from tests.test_resample_gpu import CHAIN_ENERGY_BOUND, CHAIN_LOG_BOUND, EXCLUDED_MAX, chain_errors
    (tmp_path / "labels.csv").write_text("index,mid,display_name\n0,/m/a,a\n")
    os.makedirs(tmp_path / "video" / "frame_0")
    margins = {}
    for name, x in chain_signals().items():
        payloads, data = [], []
        for b, (fmt, C, rate, n) in enumerate(CHAIN_CLIPS):
            payloads.append(quantise(x[b, :C, :n], fmt))
            wav = tmp_path / f"{name}{b}.wav"
            wav.write_bytes(wav_bytes(fmt, C, rate, payloads[-1], fmt_size=40 if fmt == pp.PCM_S24 else 16, before=[(b"LIST", b"INFOodd")]))
            np.save(tmp_path / "video" / "frame_0" / f"{name}{b}.npy", np.full((8, 8, 3), 128, dtype=np.uint8))
            data.append({"wav": str(wav), "labels": "/m/a", "video_id": f"{name}{b}", "video_path": str(tmp_path / "video")})
        (tmp_path / f"{name}.json").write_text(json.dumps({"data": data}))
        ld = FileFtLoader(FtFileDataset(str(tmp_path / f"{name}.json"), str(tmp_path / "labels.csv")), FrontCfg, 2, DEV, train=False, total_frame=1)
        (batch,) = list(ld.staged(0))
        assert ld.n_bad == 0 and batch["audio"]["channels"] == [1, 2] and batch["audio_rows"] == [1, 0]
        wave, lengths = ld._audio(batch["audio"], batch["audio_rows"], 2)
        energies, frames, want_lengths = float64_chain(payloads)
        assert lengths.tolist() == want_lengths
        out = ops().kaldi_fbank(wave, lengths, target_length=max(frames)).cpu().numpy()
        for b, m in enumerate(frames):
            assert not out[b, m:].any(), ("pad rows", b)
        ref_e = np.zeros((2, max(frames), 128))
        for b, m in enumerate(frames):
            ref_e[b, :m] = energies[b][:m]
        energy, log, excluded = chain_errors(out, ref_e, frames)
        margins[name] = {"kernel_energy": energy, "kernel_log": log, "excluded_share": excluded}
        print(f"files -> decode + resample + fbank vs the float64 chain ({name}): energy {energy:.3e}, log {log:.3e}, excluded {excluded:.4f}")
        record_margin(f"decode.fbank_chain_vs_f64.{name}", **margins[name], bound_energy=CHAIN_ENERGY_BOUND, bound_log=CHAIN_LOG_BOUND)
    for name, m in margins.items():
        assert m["kernel_energy"] <= CHAIN_ENERGY_BOUND, (name, m)
        if name != "tone":                                      # as in tests/test_resample_gpu.py: the tone is held to the energy measure only
            assert m["excluded_share"] <= EXCLUDED_MAX, (name, m)
            assert m["kernel_log"] <= CHAIN_LOG_BOUND, (name, m)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. loader, model and launcher on a five-clip dataset
CFG = AVSiamConfig(depth=2)
MEAN, STD = -5.081, 4.4849


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("five"))


@pytest.fixture(scope="module")
def ten(tmp_path_factory):
    """the same five clips with the 10 frames per clip that the mm_grad test mode scores"""
    return make_dataset(tmp_path_factory.mktemp("ten"), total_frame=10)


def by_hand(ld, five, d):
    """the front end called clip by clip on the draws `d`: decode -> resample per file, then ONE fbank / resize / label call as the loader's"""
    o = ops()
    B = len(d["index"])

    def audio(indices):
        rows = []
        for i in indices:
            if i < 0:
                rows.append((torch.zeros(1, device=DEV), 1))
                continue
            raw = open(five["wavs"][i], "rb").read()
            info = pp.parse_wav(raw)
            pay = np.zeros(-(-info.data_bytes // 16) * 16, dtype=np.uint8)
            pay[:info.data_bytes] = np.frombuffer(raw, np.uint8, info.data_bytes, info.data_offset)
            pcm, n = o.decode_pcm(torch.from_numpy(pay)[None].to(DEV), [[info.format, info.n_frames]], info.channels, -(-info.n_frames // 4) * 4)
            w, n16 = o.resample_wave(pcm, [info.rate], n)
            rows.append((w[0], int(n16[0])))
        S = max(400, max(w.numel() for w, _ in rows))
        wave = torch.zeros((B, S), device=DEV)
        for b, (w, _) in enumerate(rows):
            wave[b, :w.numel()] = w
        return wave, torch.tensor([n for _, n in rows], dtype=torch.int32, device=DEV)

    def frames(indices):
        got = [np.load(os.path.join(five["video"], f"frame_{five['frame_at'](i, int(k))}", f"clip{i}.npy")).transpose(2, 0, 1)[None] if i >= 0
               else np.full((1, 3, 8, 8), 128, dtype=np.uint8) for i, k in zip(indices, d["frame"][:, 0])]
        H, W = max(g.shape[2] for g in got), max(g.shape[3] for g in got)
        buf = np.zeros((B, 1, 3, H, W), dtype=np.uint8)
        for b, g in enumerate(got):
            buf[b, :, :, :g.shape[2], :g.shape[3]] = g
        return torch.from_numpy(buf).to(DEV), [[g.shape[2], g.shape[3]] for g in got]

    wave, lengths = audio(d["index"])
    v1, s1 = frames(d["index"])
    hot = torch.from_numpy(ld.ds.hot[d["index"]]).to(DEV)
    if (d["partner"] >= 0).any():
        wave2, lengths2 = audio(d["partner"])
        v2, s2 = frames(d["partner"])
        a = o.kaldi_fbank(wave, lengths, partner=wave2, partner_lengths=lengths2, lam=d["lam"], target_length=CFG.audio_len, norm=(MEAN, STD))
        v = o.resize_frames(v1, s1, partner=v2, partner_sizes=s2, weight=d["weight"], size=CFG.img_size)
        y = pp.mixup_labels(hot, torch.from_numpy(ld.ds.hot[np.maximum(d["partner"], 0)]).to(DEV), torch.from_numpy(d["lam"]).to(DEV), 0.1)
    else:
        a = o.kaldi_fbank(wave, lengths, target_length=CFG.audio_len, norm=(MEAN, STD))
        v = o.resize_frames(v1, s1, size=CFG.img_size)
        y = pp.mixup_labels(hot, None, -1.0, 0.1)
    return a, v, y


def test_loader_batch_is_the_chain_by_hand_and_trains(five):
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    from avsiam_amd.models.cav_mae_ft import CAVMAEFT_BASE
    ld = FileFtLoader(FtFileDataset(five["json"], five["csv"]), CFG, 3, DEV, seed=87, mixup=0.5, norm=(MEAN, STD), train=True, total_frame=3, num_workers=2)
    seen = {"mixed": 0, "plain": 0, "batches": []}
    for epoch in range(4):
        for a, v, y in ld:
            d = ld.last_draw
            assert a.shape == (3, CFG.audio_len, 128) and v.shape == (3, 1, 3, CFG.img_size, CFG.img_size) and y.shape == (3, 7)
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(v).all())
            a2, v2, y2 = by_hand(ld, five, d)
            assert torch.equal(bits(a), bits(a2)) and torch.equal(bits(v), bits(v2)) and torch.equal(bits(y), bits(y2))
            seen["mixed"] += int((d["lam"] >= 0).sum()); seen["plain"] += int((d["lam"] < 0).sum())
            seen["batches"].append((a, v, y))
    assert seen["mixed"] and seen["plain"] and ld.n_bad == 0
    # validation: every frame of the clips, no mixing, the last batch short
    va = FileFtLoader(FtFileDataset(five["json"], five["csv"]), CFG, 3, DEV, seed=88, norm=(MEAN, STD), train=False, frames="all", total_frame=3)
    shapes = [(a.shape[0], v.shape[1]) for a, v, y in va]
    assert shapes == [(3, 3), (2, 3)]
    model = CAVMAEFT_BASE(7, cfg=CFG, init_seed=6, init_mode="random").to(DEV)
    a, v, y = seen["batches"][0]
    loss = model.train_step(a, v, y, 1e-4, "mm_grad", branch="mm", loss="BCE", head_lr=100.0, mm_lr=100.0)
    assert np.isfinite(float(loss))


def launch(monkeypatch, argv):
    import avsiam_amd.config as config
    import avsiam_amd.models as models
    import avsiam_amd.run_cavmae_ft_base as launcher
    monkeypatch.setattr(config, "AVSiamConfig", lambda: CFG)
    monkeypatch.setattr(models, "CAVMAEFT_BASE", lambda label_dim: models.cav_mae_ft.CAVMAEFT_BASE(label_dim, cfg=CFG, init_seed=6, init_mode="random"))
    return launcher.main(argv)


def test_launcher_trains_from_files(ten, tmp_path, capsys, monkeypatch):
    """--data_train / --data_val / --label_csv with mixup, SpecAugment and noise on a depth-2 model at batch 3: one epoch and its validation
    finish with finite, recorded losses, and --eval-frames scores the validation json's frames"""
    exp = tmp_path / "ft"
    out = launch(monkeypatch, ["--ftmode", "mm_grad", "--n_class", "7", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "3", "--n_epochs", "1",
                               "--exp_dir", str(exp), "--label_smooth", "0.1", "--data_train", ten["json"], "--data_val", ten["json"], "--label_csv", ten["csv"],
                               "--num_workers", "2", "--mixup", "0.5", "--freqm", "48", "--timem", "192", "--noise", "True", "--eval-frames",
                               "--device-metrics"])
    said = capsys.readouterr().out
    assert "not implemented" not in said and "there is an error" not in said
    res = np.loadtxt(exp / "result.csv", delimiter=",").reshape(-1, 4)
    assert res.shape == (1, 4) and np.all(np.isfinite(res)), res
    assert "valid loss" in said and "nan" not in said.split("valid loss")[1].split()[0]
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3])
    frame_res = np.loadtxt(exp / "mul_frame_res.csv", delimiter=",")
    assert frame_res.shape == (11,) and len(out["frame_res"]) == 11 and np.all(np.isfinite(frame_res))    # ten frames and their ensemble


def test_launcher_file_training_with_synthetic_validation(ten, tmp_path, capsys, monkeypatch):
    exp = tmp_path / "ft"
    out = launch(monkeypatch, ["--ftmode", "mm_grad", "--n_class", "7", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "3", "--n_epochs", "1",
                               "--exp_dir", str(exp), "--data_train", ten["json"], "--label_csv", ten["csv"], "--num_workers", "0",
                               "--val-steps", "1", "--mixup", "0.5"])
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3]) and "not implemented" not in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. nothing else moved
def test_synthetic_loaders_are_built_and_draw_as_before(tmp_path, monkeypatch):
    """with no data flags the launcher builds the synthetic loaders with the arguments it always gave them, and their host draws are the
    sequence they always were (restated here from numpy's Generator)"""
    import avsiam_amd.run_cavmae_ft_base as launcher
    import avsiam_amd.traintest_ft_base as tt
    built = []

    class Recording(tt.SyntheticWaveFtLoader):
        def __init__(self, *a, **k):
            built.append((a[1:4], {x: k[x] for x in sorted(k)}))
            super().__init__(*a, **k)

    monkeypatch.setattr(tt, "SyntheticWaveFtLoader", Recording)
    monkeypatch.setattr(tt, "train", lambda model, tr, va, sampler, args: {"loaders": (tr, va, sampler)})
    out = launch(monkeypatch, ["--ftmode", "mm_grad", "--n_class", "7", "--batch_size", "3", "--exp_dir", str(tmp_path), "--steps-per-epoch", "2", "--val-steps", "1",
                               "--wave-input", "--mixup", "0.5"])
    norm = (MEAN, STD)
    assert built == [((3, 2, 7), dict(frame_size=None, label_smooth=0.1, mixup=0.5, norm=norm, seed=87, train=True)),
                     ((3, 1, 7), dict(frame_size=None, frames=10, label_smooth=0.1, norm=norm, seed=88, train=False))]
    tr, va, sampler = out["loaders"]
    assert sampler is None and type(tr) is Recording and type(va) is Recording
    rng = np.random.default_rng(87)
    for _ in range(2):
        d = tr.draw()
        lengths = rng.integers(144000, 160001, 3).astype(np.int32)
        mixed = rng.random(3) < 0.5
        partner_lengths = rng.integers(144000, 160001, 3).astype(np.int32)
        lam = np.where(mixed, rng.beta(10, 10, 3), -1.0).astype(np.float32)
        weight = np.where(mixed, rng.random(3), 1.0).astype(np.float32)
        assert sorted(d) == ["lam", "lengths", "partner_lengths", "weight"]
        assert all(np.array_equal(d[k], w) for k, w in (("lengths", lengths), ("partner_lengths", partner_lengths), ("lam", lam), ("weight", weight)))
    g = torch.Generator().manual_seed(87)
    assert torch.equal(tr.wave.cpu(), torch.randn(3, 160000, generator=g) * 0.1)


# the digest of one plain fine-tuning step on the parent commit (tools/step_digest.py --ft --trace --batch 3)
PARENT_DIGEST = {"trace_calls": 303, "trace": "21a456a12665402bb61ad36021b881415531210137bfe83da2f626bd146a239a", "calls_per_step": [301],
                 "p": "57f087e095055fa51785f681a6cb583fc4ce92b4c8bd85342575a3445db100b9", "g": "8717c34280ebc640d3e247807d9c6eec5f13a0d6188b234c2c9c323538cd2c46",
                 "adam_m": "887c7d3accf9731d8b7c0ad334b807b47c7b4a7ac999d026edbddab608d08406", "adam_v": "5c9624b28e55299fdb1dfa8a9d0b9526bcf2c182c6e0aa736b211926c9010abb"}


def test_plain_step_is_the_parents():
    """the library-call list of a plain step (entry points, scalar arguments, tensor shapes) and the arenas after it hash to what the parent
    commit gives: the change adds a kernel and a loader and edits nothing on that path"""
    r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print("step digest:", {k: got[k] for k in PARENT_DIGEST})
    assert {k: got[k] for k in PARENT_DIGEST} == PARENT_DIGEST
