"""WAV files written by hand and a five-clip file dataset for the decode / file-loader tests (tests/test_decode_cpu.py, tests/test_decode_gpu.py)."""
import json
import os
import struct

import numpy as np

from avsiam_amd import preprocess as pp

GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_bytes(fmt, channels, rate, payload, fmt_size=16, before=(), after=(), data_size=None, tag=None, bits=None, block_align=None, guid_tail=GUID_TAIL):
    """a RIFF / WAVE file: 'fmt ' of 16, 18 or 40 (extensible) bytes, the chunks `before`, 'data' (its size field `data_size` if given), `after`"""
    bps = pp.PCM_BYTES[fmt]
    bits = 8 * bps if bits is None else bits
    align = channels * bps if block_align is None else block_align
    real = (3 if fmt in (pp.PCM_F32, pp.PCM_F64) else 1) if tag is None else tag
    body = struct.pack("<HHIIHH", 0xFFFE if fmt_size == 40 else real, channels, rate, rate * align, align, bits)
    if fmt_size == 18:
        body += struct.pack("<H", 0)
    elif fmt_size == 40:
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", real) + guid_tail
    out = chunk(b"fmt ", body)
    for cid, b in before:
        out += chunk(cid, b)
    data = chunk(b"data", payload)
    if data_size is not None:
        data = b"data" + struct.pack("<I", data_size) + data[8:]
    out += data
    for cid, b in after:
        out += chunk(cid, b)
    return b"RIFF" + struct.pack("<I", 4 + len(out)) + b"WAVE" + out


def quantise(x, fmt):
    """float samples [C, n] in -1 .. 1 -> the interleaved payload bytes of a format"""
    x = np.asarray(x, dtype=np.float64).T                        # frames first
    if fmt == pp.PCM_U8:
        return (np.clip(np.rint(x * 128.0), -128, 127) + 128).astype(np.uint8).tobytes()
    if fmt == pp.PCM_S16:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
    if fmt == pp.PCM_S24:
        v = np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype("<i4")
        return np.ascontiguousarray(v.reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    if fmt == pp.PCM_S32:
        return np.clip(np.rint(x * 2147483648.0), -2147483648, 2147483647).astype("<i4").tobytes()
    return x.astype("<f4" if fmt == pp.PCM_F32 else "<f8").tobytes()


# (format, channels, rate, seconds, extensible fmt, labels, frame size)
FIVE = [(pp.PCM_S16, 2, 44100, 0.30, False, "/m/a,/m/c", (40, 64)), (pp.PCM_S24, 1, 48000, 0.25, True, "/m/b", (37, 53)),
        (pp.PCM_U8, 1, 8000, 0.35, False, "/m/c,/m/d,/m/g", (40, 64)), (pp.PCM_F32, 2, 16000, 0.28, False, "/m/e", (37, 53)),
        (pp.PCM_S16, 1, 22050, 0.32, False, "/m/f,/m/a", (40, 64))]
MISSING = (3, 2)                                                  # clip 3 has no frame_2


def make_dataset(root, total_frame=3, seed=5):
    """five clips of mixed formats, channel counts and rates with .npy frames of two sizes under `root` -> paths and what the files hold"""
    root = str(root)
    rng = np.random.default_rng(seed)
    video = os.path.join(root, "video")
    with open(os.path.join(root, "labels.csv"), "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{c},\"name {c}\"\n" for i, c in enumerate("abcdefg")))
    data, wavs = [], []
    for i, (fmt, ch, rate, sec, ext, labels, (h, w)) in enumerate(FIVE):
        n = int(rate * sec)
        x = rng.standard_normal((ch, n)) * 0.1 + 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)[None]
        path = os.path.join(root, f"clip{i}.wav")
        with open(path, "wb") as f:
            f.write(wav_bytes(fmt, ch, rate, quantise(x, fmt), fmt_size=40 if ext else 16, before=[(b"LIST", b"INFOxyz")] if i == 4 else ()))
        wavs.append(path)
        for k in range(total_frame):
            if (i, k) == MISSING:
                continue
            os.makedirs(os.path.join(video, f"frame_{k}"), exist_ok=True)
            np.save(os.path.join(video, f"frame_{k}", f"clip{i}.npy"), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        data.append({"wav": path, "labels": labels, "video_id": f"clip{i}", "video_path": video})
    with open(os.path.join(root, "data.json"), "w") as f:
        json.dump({"data": data}, f)
    return {"json": os.path.join(root, "data.json"), "csv": os.path.join(root, "labels.csv"), "wavs": wavs, "video": video,
            "channels": [c[1] for c in FIVE], "sizes": [c[6] for c in FIVE], "frame_at": lambda i, k: k - 1 if (i, k) == MISSING else k}
