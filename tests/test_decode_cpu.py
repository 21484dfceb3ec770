"""Training from files without a device: the WAV container walk (preprocess.parse_wav) against stdlib `wave` and scipy.io.wavfile.read, the
specification of the decode kernel (preprocess.decode_pcm_reference) against scipy's samples scaled in float64 and rounded once to fp32, and the
host side of the file loader (dataset_ft): its draws, labels, frame fallback, bad files and the launcher's parsing.

Nothing here was recorded from torchaudio (it was never available): the scaling convention is the one decode_pcm_reference's docstring states."""
import io
import json
import os
import struct
import wave

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from avsiam_amd import preprocess as pp
from tests.filedata import GUID_TAIL, make_dataset, wav_bytes

RNG = np.random.default_rng(20241101)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the parser
def scipy_read(buf):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # (scipy warns about chunks it does not know)
        return scipy.io.wavfile.read(io.BytesIO(buf))


def stdlib_wave(channels, width, rate, frames):
    f = io.BytesIO()
    with wave.open(f, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(frames)
    return f.getvalue()


def payload_of(fmt, channels, n):
    """n random frames of a format -> payload bytes"""
    if fmt == pp.PCM_F32:
        return RNG.standard_normal(n * channels).astype("<f4").tobytes()
    if fmt == pp.PCM_F64:
        return RNG.standard_normal(n * channels).astype("<f8").tobytes()
    return RNG.integers(0, 256, n * channels * pp.PCM_BYTES[fmt], dtype=np.uint8).tobytes()


STDLIB_CASES = [("pcm16 stereo 44.1k", pp.PCM_S16, 2, 44100, 301), ("pcm24 mono 48k", pp.PCM_S24, 1, 48000, 257), ("u8 mono 8k", pp.PCM_U8, 1, 8000, 99),
                ("s32 mono 22.05k", pp.PCM_S32, 1, 22050, 130)]


@pytest.mark.parametrize("name,fmt,channels,rate,n", STDLIB_CASES, ids=[c[0] for c in STDLIB_CASES])
def test_parser_against_stdlib_wave_and_scipy(name, fmt, channels, rate, n):
    payload = payload_of(fmt, channels, n)
    buf = stdlib_wave(channels, pp.PCM_BYTES[fmt], rate, payload)
    info = pp.parse_wav(buf)
    with wave.open(io.BytesIO(buf), "rb") as w:
        assert (info.channels, info.rate, info.n_frames) == (w.getnchannels(), w.getframerate(), w.getnframes())
        assert pp.PCM_BYTES[info.format] == w.getsampwidth()
    sr, x = scipy_read(buf)
    assert sr == info.rate and x.shape[0] == info.n_frames and (x.ndim == 1) == (info.channels == 1)
    assert info.format == fmt and info.data_offset == 44 and info.data_bytes == len(payload)
    assert buf[info.data_offset:info.data_offset + info.data_bytes] == payload


def test_parser_reads_a_path(tmp_path):
    buf = stdlib_wave(2, 2, 44100, payload_of(pp.PCM_S16, 2, 10))
    p = tmp_path / "a.wav"
    p.write_bytes(buf)
    assert pp.parse_wav(p) == pp.parse_wav(buf) == pp.parse_wav(str(p))


def test_parser_float_list_extensible_streamed_truncated():
    # F32 stereo at 16 kHz with an 18-byte fmt and a 'fact' chunk, as float writers produce it
    pay = payload_of(pp.PCM_F32, 2, 77)
    buf = wav_bytes(pp.PCM_F32, 2, 16000, pay, fmt_size=18, before=[(b"fact", struct.pack("<I", 77))])
    info = pp.parse_wav(buf)
    sr, x = scipy_read(buf)
    assert (info.format, info.channels, info.rate, info.n_frames) == (pp.PCM_F32, 2, sr, x.shape[0]) == (pp.PCM_F32, 2, 16000, 77)
    assert buf[info.data_offset:info.data_offset + info.data_bytes] == pay
    # a LIST chunk of odd size (padded) before data, and a chunk after it
    pay = payload_of(pp.PCM_S16, 1, 64)
    buf = wav_bytes(pp.PCM_S16, 1, 32000, pay, before=[(b"LIST", b"INFOabc")], after=[(b"id3 ", b"xyz")])
    info = pp.parse_wav(buf)
    sr, x = scipy_read(buf)
    assert (info.rate, info.n_frames, info.channels) == (sr, x.shape[0], 1) and info.data_offset == 12 + 24 + 8 + 8 + 8
    assert np.array_equal(np.frombuffer(buf, "<i2", info.n_frames, info.data_offset), x)
    # a 40-byte extensible fmt: PCM 24 and IEEE float 64
    for fmt, channels in ((pp.PCM_S24, 2), (pp.PCM_F64, 1), (pp.PCM_S16, 8)):
        pay = payload_of(fmt, channels, 33)
        buf = wav_bytes(fmt, channels, 48000, pay, fmt_size=40)
        info = pp.parse_wav(buf)
        sr, x = scipy_read(buf)
        assert (info.format, info.channels, info.rate, info.n_frames) == (fmt, channels, sr, x.shape[0]) and info.data_offset == 12 + 48 + 8
    # a data size of 0xFFFFFFFF and of 0: the data runs to the end of the file, floored to whole frames
    pay = payload_of(pp.PCM_S16, 2, 50)
    for size in (0xFFFFFFFF, 0):
        buf = wav_bytes(pp.PCM_S16, 2, 44100, pay + b"\x01", data_size=size)
        info = pp.parse_wav(buf)
        assert (info.n_frames, info.data_offset, info.data_bytes) == (50, 44, 200)
    # a truncated data chunk: the header promises 50 frames, the file holds 30 and a half
    buf = wav_bytes(pp.PCM_S16, 2, 44100, pay)[:44 + 122]
    info = pp.parse_wav(buf)
    assert (info.n_frames, info.data_bytes) == (30, 120)


def test_parser_refusals_name_the_file_and_the_reason():
    pay = payload_of(pp.PCM_S16, 1, 8)
    good = wav_bytes(pp.PCM_S16, 1, 16000, pay)

    def refused(buf, *words):
        with pytest.raises(ValueError) as e:
            pp.parse_wav(buf, name="clip7.wav")
        assert "clip7.wav" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    refused(b"RIFX" + good[4:], "RIFX", "big-endian")
    refused(b"OggS" + good[4:], "RIFF")
    refused(good[:8] + b"AVI " + good[12:], "WAVE")
    refused(good[:10], "RIFF header")
    refused(wav_bytes(pp.PCM_U8, 1, 8000, pay, tag=6), "A-law")
    refused(wav_bytes(pp.PCM_U8, 1, 8000, pay, tag=7), "mu-law")
    refused(wav_bytes(pp.PCM_U8, 1, 8000, pay, tag=2), "ADPCM")
    refused(wav_bytes(pp.PCM_U8, 1, 8000, pay, tag=0x11), "ADPCM")
    refused(wav_bytes(pp.PCM_S16, 9, 16000, payload_of(pp.PCM_S16, 9, 4)), "9 channels")
    refused(wav_bytes(pp.PCM_S16, 2, 16000, pay, block_align=2), "block_align 2", "2 * 2")
    refused(wav_bytes(pp.PCM_S16, 1, 16000, pay, bits=12), "12-bit")
    refused(wav_bytes(pp.PCM_F32, 1, 16000, pay, bits=16), "16-bit IEEE float")
    refused(wav_bytes(pp.PCM_S16, 1, 16000, pay, fmt_size=40, guid_tail=b"\x01" + GUID_TAIL[1:]), "sub-format GUID")
    refused(good[:12] + good[36:], "no 'fmt ' chunk")
    refused(good[:36], "no 'data' chunk")
    with pytest.raises(ValueError) as e:
        pp.parse_wav(b"RIFX" + good[4:])
    assert "<bytes>" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the specification of the kernel
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def once_rounded(buf):
    """scipy's samples scaled in float64 and rounded once to fp32 -> [C, n]"""
    _, x = scipy_read(buf)
    x = x.reshape(x.shape[0], -1)
    if x.dtype == np.uint8:
        y = (x.astype(np.float64) - 128.0) * 2.0 ** -7
    elif x.dtype == np.int16:
        y = x.astype(np.float64) * 2.0 ** -15
    elif x.dtype == np.int32:                                    # 24-bit samples arrive left-justified in int32: 2^-31 for them too
        y = x.astype(np.float64) * 2.0 ** -31
    else:
        return np.ascontiguousarray(x.T)
    return y.astype(np.float32).T


@pytest.mark.parametrize("fmt", [pp.PCM_U8, pp.PCM_S16, pp.PCM_S24, pp.PCM_S32, pp.PCM_F32])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_reference_against_scipy(fmt, channels):
    pay = payload_of(fmt, channels, 501)
    buf = wav_bytes(fmt, channels, 44100, pay)
    info = pp.parse_wav(buf)
    got = pp.decode_pcm_reference(buf[info.data_offset:info.data_offset + info.data_bytes], info.format, info.channels)
    want = once_rounded(buf)
    assert got.dtype == np.float32 and got.shape == (channels, 501) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(pp.decode_pcm_reference(pay, fmt, channels, 17)), bits(want[:, :17]))


def test_reference_f64_against_scipy():
    x = np.concatenate([RNG.standard_normal(100), [1e39, -1e39, 1e-40, -1e-46, 0.1, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50]])
    buf = wav_bytes(pp.PCM_F64, 1, 16000, x.astype("<f8").tobytes())
    _, y = scipy_read(buf)
    got = pp.decode_pcm_reference(x.astype("<f8").tobytes(), pp.PCM_F64, 1)[0]
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(bits(got), bits(y.astype(np.float32)))
    assert got[100] == np.inf and got[101] == -np.inf                    # overflow
    assert got[102] == np.float32(1e-40) and 0 < got[102] < np.finfo(np.float32).tiny           # a subnormal survives
    assert bits(got[103:104])[0] == 0x80000000                           # ... and what lies under the smallest one is -0.0
    assert got[105] == 1.0 and got[106] == np.float32(1.0 + 2.0 ** -23)  # the tie goes to even, just above it up


def test_reference_exact_values():
    def one(fmt, raw):
        return pp.decode_pcm_reference(bytes(raw), fmt, 1)[0]
    s24 = one(pp.PCM_S24, [0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80, 0xFF, 0xFF, 0xFF, 0x01, 0x00, 0x00])
    assert s24.tolist() == [(2 ** 23 - 1) / 2 ** 23, -1.0, -(2.0 ** -23), 2.0 ** -23]
    s32 = one(pp.PCM_S32, struct.pack("<4i", -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3))
    assert s32.tolist() == [-1.0, 1.0, 2.0 ** -7, (2 ** 24 + 4) / 2.0 ** 31]         # INT_MAX rounds to 2^31; 2^24 + 1 and + 3 are ties: to even
    u8 = one(pp.PCM_U8, [0, 128, 255])
    assert u8.tolist() == [-1.0, 0.0, 127 / 128]
    s16 = one(pp.PCM_S16, struct.pack("<3h", -32768, 32767, -1))
    assert s16.tolist() == [-1.0, 32767 / 32768, -1 / 32768]
    words = np.array([0x7FC12345, 0xFFA00001, 0x80000000, 0x00000001, 0x7F800000], dtype="<u4")      # NaN payloads, -0.0, a subnormal, inf
    assert np.array_equal(bits(one(pp.PCM_F32, words.tobytes())), words)
    # planar output of interleaved frames
    st = pp.decode_pcm_reference(struct.pack("<6h", 1, -1, 2, -2, 3, -3), pp.PCM_S16, 2)
    assert (st * 32768).tolist() == [[1, 2, 3], [-1, -2, -3]]
    for bad in (lambda: pp.decode_pcm_reference(b"\0" * 8, 6, 1), lambda: pp.decode_pcm_reference(b"\0" * 8, 1, 9), lambda: pp.decode_pcm_reference(b"\0" * 8, 1, 1, 5)):
        with pytest.raises(ValueError):
            bad()


def test_quantised_chain_inputs_stay_under_the_excluded_cap():
    """what tests/test_decode_gpu.py's chain test relies on, with the float64 restatement alone: quantising the noise signals of
    tests/test_resample_gpu.py to PCM16 / PCM24 leaves the share of cells the log measure excludes (energy under 1e-6 of the row's largest) at
    the 1.5 % it was, under that file's 3 % cap"""
    from tests.filedata import quantise
    rates, lengths = [44100, 48000], [52920, 57001]                      # FB_RATES, FB_LENGTHS of tests/test_resample_gpu.py, and its generator
    noise = (np.random.default_rng(20241017).standard_normal((2, 2, max(lengths) + 3)) * 0.1).astype(np.float32)
    for b, (fmt, C) in enumerate(((pp.PCM_S16, 2), (pp.PCM_S24, 1))):
        x = noise[b, :C, :lengths[b]]
        q = pp.decode_pcm_reference(quantise(x, fmt), fmt, C)
        assert np.abs(q - x).max() <= 2.0 ** -(8 * pp.PCM_BYTES[fmt])                  # half a step of the format
        r64, ol = pp.resample_reference(q[None].astype(np.float64), [rates[b]], [lengths[b]])
        m = pp.fbank_frames(int(ol[0]))
        _, e = pp.kaldi_fbank_reference(r64, ol, target_length=m, return_energy=True)
        excluded = 1.0 - (e[0, :m] >= 1e-6 * e[0, :m].max(axis=1, keepdims=True)).mean()
        print(f"clip {b}: excluded share {excluded:.4f}")
        assert excluded <= 0.03


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the loader's host side
class Cfg:
    audio_len, img_size = 1024, 224


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("five"))


def loader(five, **kw):
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    kw = {**dict(seed=87, mixup=0.5, train=True, total_frame=3, say=lambda *a, **k: None), **kw}
    return FileFtLoader(FtFileDataset(five["json"], five["csv"], say=kw["say"]), Cfg, 3, "cpu", **kw)


def staged_epochs(ld, epochs=2):
    return [list(ld.staged(e)) for e in range(epochs)]


def test_draws_do_not_depend_on_the_workers(five):
    a, b = staged_epochs(loader(five, num_workers=0)), staged_epochs(loader(five, num_workers=2))
    assert len(a[0]) == 1 and len(a[0][0]["draw"]["index"]) == 3                  # five clips at batch 3: one full batch, the tail dropped
    for ea, eb in zip(a, b):
        for x, y in zip(ea, eb):
            assert x["draw"].keys() == y["draw"].keys() and all(np.array_equal(x["draw"][k], y["draw"][k]) for k in x["draw"])
            assert torch.equal(x["audio"]["payload"], y["audio"]["payload"]) and torch.equal(x["frames"], y["frames"])
            assert torch.equal(x["audio"]["desc"], y["audio"]["desc"]) and x["audio"]["rates"] == y["audio"]["rates"]
    assert not np.array_equal(a[0][0]["draw"]["index"], a[1][0]["draw"]["index"]) or not np.array_equal(a[0][0]["draw"]["lam"], a[1][0]["draw"]["lam"])
    # another rank: other clips, other draws; the same rank again: the same
    r1 = staged_epochs(loader(five, rank=1, world=2), 1)
    r0 = staged_epochs(loader(five, rank=0, world=2), 1)
    assert len(r0[0]) == len(r1[0]) == 1 and not set(r0[0][0]["draw"]["index"]) & set(r1[0][0]["draw"]["index"])
    assert len(r0[0][0]["draw"]["index"]) == 2                                   # 5 // 2 per rank, under the batch size: one short batch each


def test_plan_is_the_stated_sequence(five):
    """partner, mixed, lam, weight, frame per item from one Generator seeded (seed, epoch, rank + 1); the permutation from (seed, epoch)"""
    ld = loader(five)
    for epoch in (0, 3):
        rng = np.random.default_rng([87, epoch, 1])
        idx = np.random.default_rng([87, epoch]).permutation(5)[:3]
        (d,) = ld.plan(epoch)
        assert d["index"].tolist() == idx.tolist()
        for b in range(3):
            partner, u = int(rng.integers(0, 5)), rng.random()
            if u < 0.5:
                lam, weight = rng.beta(10, 10), rng.random()
                assert (d["partner"][b], d["lam"][b], d["weight"][b]) == (partner, np.float32(lam), np.float32(weight))
            else:
                assert (d["partner"][b], d["lam"][b], d["weight"][b]) == (-1, -1.0, 1.0)
            assert d["frame"][b, 0] == rng.integers(0, 3)
    mixed = np.concatenate([ld.plan(e)[0]["lam"] for e in range(40)]) >= 0
    assert 0.3 < mixed.mean() < 0.7


def expected_target(class_sets, own, other, lam, smooth, n_class):
    """the target of one item from the class-index sets of its clip and of its partner (other None: not mixed), in float64.  What
    dataloader_ft.py:470-475 (mixed) and :480, :523-524 (plain) compute: every class starts at smooth / n_class; a mixed item adds
    lam (1 - smooth) per class of its own set and (1 - lam) (1 - smooth) per class of the partner's; a plain item sets its classes to 1 - smooth"""
    t = np.full(n_class, smooth / n_class, dtype=np.float64)
    keep = 1.0 - smooth
    if other is None:
        t[sorted(class_sets[own])] = keep
    else:
        np.add.at(t, sorted(class_sets[own]), lam * keep)
        np.add.at(t, sorted(class_sets[other]), (1.0 - lam) * keep)
    return torch.from_numpy(t).float()


def test_partner_lam_and_labels(five):
    ld = loader(five)
    # every clip's classes, read from the json's mids through the csv's index column (not through the loader's own multi-hot table)
    class_sets = [{ld.ds.index_dict[mid] for mid in labels.split(",")} for _, labels, _, _ in ld.ds.entries]
    seen_mixed = seen_plain = 0
    for epoch in range(6):
        for batch in ld.staged(epoch):
            d = batch["draw"]
            ch, rows = batch["audio"]["channels"], batch["audio_rows"]
            assert ch == sorted(ch) and ch == [five["channels"][d["index"][b]] for b in rows] and sorted(rows) == [0, 1, 2]      # staged by channel count
            hot = ld.hot[torch.from_numpy(d["index"])]
            hot2 = ld.hot[torch.from_numpy(np.maximum(d["partner"], 0))]
            y = pp.mixup_labels(hot, hot2, torch.from_numpy(d["lam"]), 0.1) if batch["mixed"] else pp.mixup_labels(hot, None, -1.0, 0.1)
            for b in range(len(d["index"])):
                is_mixed = d["lam"][b] >= 0
                assert is_mixed == (d["partner"][b] >= 0) == (b in batch["mixed"])
                want = expected_target(class_sets, d["index"][b], d["partner"][b] if is_mixed else None, float(d["lam"][b]), 0.1, len(ld.ds.index_dict))
                assert torch.allclose(y[b], want, rtol=0, atol=2e-7), (epoch, b)
                seen_mixed, seen_plain = seen_mixed + is_mixed, seen_plain + (not is_mixed)
            if batch["mixed"]:
                rows = batch["partner_rows"]
                assert sorted(rows) == batch["mixed"] and batch["partner_audio"]["channels"] == sorted(five["channels"][d["partner"][b]] for b in rows)
                assert batch["partner_audio"]["channels"] == [five["channels"][d["partner"][b]] for b in rows]
    assert seen_mixed and seen_plain


def test_staging_holds_the_files_bytes(five):
    ld = loader(five, train=False, frames="all")
    batches = list(ld.staged(0))
    assert [len(b["draw"]["index"]) for b in batches] == [3, 2] and sorted(np.concatenate([b["draw"]["index"] for b in batches]).tolist()) == [0, 1, 2, 3, 4]
    for batch in batches:
        pay, desc = batch["audio"]["payload"], batch["audio"]["desc"]
        assert pay.shape[1] % 16 == 0 and pay.dtype == torch.uint8 and batch["frames"].shape[1:3] == (3, 3)
        assert batch["audio"]["channels"] == sorted(batch["audio"]["channels"])
        for b, i in enumerate(batch["draw"]["index"]):
            info = pp.parse_wav(five["wavs"][i])
            r = batch["audio_rows"].index(b)                       # the staged row of batch row b
            assert desc[r].tolist() == [info.format, info.n_frames] and batch["audio"]["rates"][r] == info.rate
            raw = open(five["wavs"][i], "rb").read()[info.data_offset:info.data_offset + info.data_bytes]
            assert bytes(pay[r, :info.data_bytes].numpy()) == raw and not pay[r, info.data_bytes:].any()
            h, w = batch["sizes"][b]
            assert (h, w) == five["sizes"][i]
            for f in range(3):
                want = np.load(os.path.join(five["video"], f"frame_{five['frame_at'](i, f)}", f"clip{i}.npy")).transpose(2, 0, 1)
                assert np.array_equal(batch["frames"][b, f, :, :h, :w].numpy(), want)
            assert not batch["frames"][b, :, :, h:].any() and not batch["frames"][b, :, :, :, w:].any()
    # data-parallel validation: contiguous shards padded to equal length
    got = [np.concatenate([b["draw"]["index"] for b in loader(five, train=False, rank=r, world=2).staged(0)]).tolist() for r in (0, 1)]
    assert got == [[0, 1, 2], [3, 4, 4]]
    assert len(loader(five, train=False).sampler.dataset) == 5
    # the middle frame, and a named one
    assert list(loader(five, train=False).staged(0))[0]["draw"]["frame"].tolist() == [[1]] * 3
    assert list(loader(five, train=False, frames=2).staged(0))[0]["draw"]["frame"].tolist() == [[2]] * 3


def test_missing_frame_falls_back(five):
    """clip 3 has no frame_2: the loader reads frame_1, as randselect_img walks down"""
    said = []
    ld = loader(five, train=False, frames=2, say=lambda *a, **k: said.append(" ".join(map(str, a))))
    used = {int(i): u.tolist() for b in ld.staged(0) for i, u in zip(b["draw"]["index"], b["draw"]["frame_used"])}
    assert used == {0: [2], 1: [2], 2: [2], 3: [1], 4: [2]}
    assert any("clip3" in s and "no frame_2" in s for s in said) and ld.n_bad == 0


def test_bad_files_are_counted_or_raise(five, tmp_path):
    data = json.load(open(five["json"]))["data"]
    broken = tmp_path / "broken.wav"
    broken.write_bytes(b"RIFX" + open(five["wavs"][0], "rb").read()[4:])
    data[1] = {**data[1], "wav": str(broken)}
    data[2] = {**data[2], "wav": str(tmp_path / "absent.wav")}
    data[4] = {**data[4], "video_id": "nothing"}
    p = tmp_path / "bad.json"
    p.write_text(json.dumps({"data": data}))
    from avsiam_amd.dataset_ft import SILENCE_FRAMES, FileFtLoader, FtFileDataset
    said = []
    say = lambda *a, **k: said.append(" ".join(map(str, a)))       # noqa: E731
    ld = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 5, "cpu", train=False, total_frame=3, say=say)
    (batch,) = list(ld.staged(0))
    assert ld.n_bad == 3
    assert any("broken.wav" in s and "RIFX" in s for s in said) and any("absent.wav" in s for s in said) and any("nothing" in s for s in said)
    for b, i in enumerate(batch["draw"]["index"]):
        r = batch["audio_rows"].index(b)
        if i in (1, 2):
            assert batch["audio"]["desc"][r].tolist() == [pp.PCM_S16, SILENCE_FRAMES] and not batch["audio"]["payload"][r].any() and batch["audio"]["rates"][r] == 16000
        if i == 4:
            h, w = batch["sizes"][b]
            assert bool((batch["frames"][b, :, :, :h, :w] == 128).all())
    assert torch.equal(ld.hot, torch.from_numpy(FtFileDataset(five["json"], five["csv"]).hot))       # the labels stay
    strict = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 5, "cpu", train=False, total_frame=3, strict=True, say=say)
    with pytest.raises(RuntimeError) as e:
        list(strict.staged(0))
    assert "broken.wav" in str(e.value) or "absent.wav" in str(e.value)


def test_a_bad_clip_is_counted_and_reported_once(five, tmp_path):
    """n_bad is the number of distinct clips replaced: a bad clip met again - a second epoch, validation padding, a mixup partner - adds nothing"""
    data = json.load(open(five["json"]))["data"]
    data[4] = {**data[4], "wav": str(tmp_path / "absent.wav")}
    p = tmp_path / "bad.json"
    p.write_text(json.dumps({"data": data}))
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    said = []
    say = lambda *a, **k: said.append(" ".join(map(str, a)))       # noqa: E731
    # validation on rank 1 of 2: its shard is [3, 4, 4], the bad clip and its repetition as padding
    ld = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 3, "cpu", train=False, total_frame=3, rank=1, world=2, say=say)
    for epoch in range(2):
        (batch,) = list(ld.staged(epoch))
        assert batch["draw"]["index"].tolist() == [3, 4, 4]
    assert ld.n_bad == 1 and ld.bad_clips == {4} and sum("absent.wav" in s for s in said) == 1
    # training with mixup 1: clip 4 comes as a clip and as a partner over the epochs
    tr = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 3, "cpu", mixup=1.0, train=True, total_frame=3, say=say)
    as_clip = as_partner = 0
    for epoch in range(8):
        for batch in tr.staged(epoch):
            as_clip, as_partner = as_clip + int((batch["draw"]["index"] == 4).sum()), as_partner + int((batch["draw"]["partner"] == 4).sum())
    assert as_clip >= 1 and as_partner >= 1 and as_clip + as_partner >= 3 and tr.n_bad == 1


def test_unusable_audio_becomes_a_bad_clip(five, tmp_path):
    """a WAV without a sample frame, and one at a rate the resample kernel refuses, are set aside when the header is parsed: counted and
    replaced like any unreadable clip (strict: raised), never handed to the device chain"""
    header = open(five["wavs"][0], "rb").read()[:pp.parse_wav(five["wavs"][0]).data_offset]
    empty = tmp_path / "empty.wav"
    empty.write_bytes(header[:-4] + struct.pack("<I", 0))           # a data chunk of size 0 at the end of the file: no frames
    assert pp.parse_wav(str(empty)).n_frames == 0
    odd = tmp_path / "odd_rate.wav"
    with wave.open(str(odd), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(44101), w.writeframes(b"\0\0" * 500)
    assert pp.resample_rate_problem(44101) and "44101" in pp.resample_rate_problem(44101)
    for rate in (16000, 8000, 11025, 22050, 32000, 44100, 48000, 96000):
        assert pp.resample_rate_problem(rate) is None, rate
    data = json.load(open(five["json"]))["data"]
    data[0], data[1] = {**data[0], "wav": str(empty)}, {**data[1], "wav": str(odd)}
    p = tmp_path / "unusable.json"
    p.write_text(json.dumps({"data": data}))
    from avsiam_amd.dataset_ft import SILENCE_FRAMES, FileFtLoader, FtFileDataset
    said = []
    say = lambda *a, **k: said.append(" ".join(map(str, a)))       # noqa: E731
    ld = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 5, "cpu", train=False, total_frame=3, say=say)
    (batch,) = list(ld.staged(0))
    assert ld.bad_clips == {0, 1}
    assert any("empty.wav" in s and "no sample frame" in s for s in said) and any("odd_rate.wav" in s and "44101" in s for s in said)
    for b in (0, 1):
        r = batch["audio_rows"].index(b)
        assert batch["audio"]["desc"][r].tolist() == [pp.PCM_S16, SILENCE_FRAMES] and batch["audio"]["rates"][r] == 16000
    assert all(n >= 1 for n in batch["audio"]["n_frames"])
    strict = FileFtLoader(FtFileDataset(str(p), five["csv"]), Cfg, 5, "cpu", train=False, total_frame=3, strict=True, say=say)
    with pytest.raises(RuntimeError, match="empty.wav|odd_rate.wav"):
        list(strict.staged(0))


def test_rate_groups_keep_a_call_within_eight_rates():
    """one decode + resample call takes rows of one channel count and at most 8 distinct rates other than 16 kHz"""
    from avsiam_amd.dataset_ft import rate_groups
    assert rate_groups([1, 1, 2, 2, 2], [44100, 16000, 48000, 48000, 8000]) == [(0, 2), (2, 5)]
    assert rate_groups([2], [16000]) == [(0, 1)] and rate_groups([], []) == []
    rates = [8000 + 1000 * k for k in range(12)]                    # 12 distinct rates, 16 000 among them (free), in one channel group
    groups = rate_groups([1] * 12, rates)
    assert groups == [(0, 9), (9, 12)]                              # rows 0 .. 8 hold 8 rates other than 16 kHz; row 9 would be the ninth
    for s, e in groups:
        assert len({r for r in rates[s:e] if r != 16000}) <= 8
    assert rate_groups([1] * 10 + [2], [8000] * 10 + [8000]) == [(0, 10), (10, 11)]          # repeated rates do not count twice
    assert rate_groups([1] * 3, [1, 2, 3], max_rates=1) == [(0, 1), (1, 2), (2, 3)]


def test_workers_are_capped_for_a_shared_gpu(five, monkeypatch):
    """a worker inherits the open GPU: ranks x (1 + the workers of all file loaders of a rank) stays at or under 16 processes, whatever is asked"""
    from avsiam_amd import dataset_ft
    from avsiam_amd import run_cavmae_ft_base as launcher
    share = dataset_ft.worker_share
    default = launcher.build_parser().parse_args([]).num_workers
    assert default == 32                                            # the reference's default: what a run without the flag asks for
    assert share(default) == 15 and share(default, loaders=2) == 7 and share(6) == 6 and share(6, loaders=2) == 6 and share(0, loaders=2) == 0
    assert share(default, loaders=1, ranks=8) == 1 and share(default, loaders=2, ranks=8) == 0 and share(default, ranks=16) == 0 and share(default, ranks=64) == 0
    for ranks in (1, 2, 3, 4, 8, 16):
        for loaders in (1, 2):
            assert ranks * (1 + loaders * share(default, loaders, ranks)) <= dataset_ft.MAX_PROCESSES
    assert loader(five, num_workers=default).num_workers == 15      # a loader built directly cannot exceed the machine either
    # what each loader hands to torch: a training loader keeps its workers between epochs, an evaluation loader's end with every pass
    built = []

    class Recorder:
        def __init__(self, dataset, **kw):
            built.append(kw)

        def __iter__(self):
            return iter(())

    monkeypatch.setattr(torch.utils.data, "DataLoader", Recorder)
    for train in (True, False):
        list(loader(five, num_workers=default, train=train).staged(0))
    assert [(kw["num_workers"], kw["persistent_workers"]) for kw in built] == [(15, True), (15, False)]


def test_evaluation_workers_end_with_the_pass(five):
    import multiprocessing
    before = set(multiprocessing.active_children())
    ld = loader(five, num_workers=2, train=False)
    assert [len(b["draw"]["index"]) for b in ld.staged(0)] == [3, 2]
    assert not [p for p in set(multiprocessing.active_children()) - before if p.is_alive()]
    tr = loader(five, num_workers=2)
    list(tr.staged(0))
    kept = [p for p in set(multiprocessing.active_children()) - before if p.is_alive()]
    assert len(kept) == 2                                           # the training workers wait for the next epoch ...
    tr.close()
    for p in kept:
        p.join(10)
    assert not [p for p in kept if p.is_alive()]                    # ... and close() ends them


def test_dataset_refusals(five, tmp_path):
    from avsiam_amd.dataset_ft import FtFileDataset
    with pytest.raises(ValueError, match="n_class 9"):
        FtFileDataset(five["json"], five["csv"], n_class=9)
    p = tmp_path / "unknown.json"
    p.write_text(json.dumps({"data": [{"wav": "a.wav", "labels": "/m/zzz", "video_id": "a", "video_path": "."}]}))
    with pytest.raises(ValueError, match="/m/zzz"):
        FtFileDataset(str(p), five["csv"])


def test_launcher_parsing(five):
    from avsiam_amd import run_cavmae_ft_base as launcher
    parse = launcher.build_parser().parse_args
    base = ["--label_csv", five["csv"], "--n_class", "7"]
    assert launcher.data_plan(parse(["--data_train", five["json"]] + base)) == {"train": "file", "val": "synthetic"}
    assert launcher.data_plan(parse(["--data_val", five["json"], "--data_train", "synthetic"] + base)) == {"train": "synthetic", "val": "file"}
    assert launcher.data_plan(parse(["--data_train", five["json"], "--data_val", five["json"]] + base)) == {"train": "file", "val": "file"}
    assert launcher.data_plan(parse([])) == launcher.data_plan(parse(["--data_train", "synthetic", "--n_class", "3"])) == {"train": "synthetic", "val": "synthetic"}
    a = parse(["--data_train", five["json"]] + base)
    assert (a.strict_data, a.total_frame) == (False, 10) and parse(["--strict-data", "--total-frame", "4"]).total_frame == 4
    for argv, words in ((["--data_train", five["json"], "--label_csv", five["csv"], "--n_class", "527"], ("--n_class 527", "7 classes")),
                        (["--data_train", five["json"], "--n_class", "7"], ("--label_csv",)),
                        (["--data_train", five["json"] + ".absent"] + base, ("no such file",)),
                        (["--data_train", five["json"], "--total-frame", "0"] + base, ("--total-frame",)),
                        (["--data_val", five["json"], "--total-frame", "3", "--ftmode", "mm_grad"] + base, ("--total-frame 3", "10"))):
        with pytest.raises(SystemExit) as e:
            launcher.main(argv)                                    # refused before anything touches a device
        assert all(w in str(e.value) for w in words), str(e.value)
    # with a file set --mixup is live: no warning calls it ignored; without one the warnings are what they were
    live = parse(["--data_train", five["json"], "--mixup", "0.5"] + base)
    live.wave_input = True                                         # (what main sets for a file side)
    assert launcher.inert_flag_warnings(live) == []
    assert len(launcher.inert_flag_warnings(parse(["--mixup", "0.5"]))) == 2


def test_png_and_jpg_frames_are_read_where_pil_is(five, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from avsiam_amd.dataset_ft import FileFtLoader, FtFileDataset
    rng = np.random.default_rng(3)
    png, jpg = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8), np.full((24, 16, 3), 200, dtype=np.uint8)
    for k, (x, ext) in enumerate(((png, "png"), (jpg, "jpg"))):
        os.makedirs(tmp_path / f"frame_{k}")
        Image.fromarray(x).save(tmp_path / f"frame_{k}" / f"c.{ext}")
    p = tmp_path / "one.json"
    p.write_text(json.dumps({"data": [{"wav": five["wavs"][0], "labels": "/m/a", "video_id": "c", "video_path": str(tmp_path)}]}))
    ds = FtFileDataset(str(p), five["csv"])
    a, b = ds[(0, (0,))], ds[(0, (1,))]
    assert a["frame_error"] is None and np.array_equal(a["frames"][0].numpy(), png.transpose(2, 0, 1))           # png is lossless
    assert b["frame_error"] is None and b["frames"].shape == (1, 3, 24, 16) and int(abs(b["frames"].int() - 200).max()) <= 2
    both = ds[(0, (0, 1))]                                         # frames of one clip must agree in size
    assert both["frames"] is None and "differ in size" in both["frame_error"]
    ld = FileFtLoader(ds, Cfg, 1, "cpu", train=False, frames="all", total_frame=2, say=lambda *a, **k: None)
    (batch,) = list(ld.staged(0))
    assert ld.n_bad == 1 and bool((batch["frames"] == 128).all())
