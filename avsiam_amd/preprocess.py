"""Input normalisation on the device - the per-sample host work of the reference dataloader
(/root/reference/src/dataloader.py:505-513 audio, :461-462 + :152-155 frames) as two HBM-bound kernels, so that raw
AudioSet-shaped tensors can be fed to ``CAVMAE_BASE.forward`` without a CPU pass.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from . import _lib

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def normalize_fbank(fbank, norm_mean, norm_std, noise=False, seed=0, rng=None, shift=None, amp=None):
    """fbank [B, T, F] fp32 (GPU) -> (fbank - norm_mean) / norm_std (dataloader.py:505-506).  ``noise=True`` adds the
    reference's training augmentation (:510-513): + U[0,1) * amp with amp = rand()/10 per sample, then a roll along time
    by a per-sample shift in [-T, T); amp and shift come from ``rng`` (a numpy Generator, default seeded by ``seed``) unless
    given explicitly (int32 / fp32 device tensors), the per-element noise from a device Philox stream keyed by ``seed``.
    (The training path does not call this: forward(..., input_xf=) applies the same arithmetic inside the kernels that read
    the input; this two-pass form is what tests compare it with.)"""
    if not (fbank.is_cuda and fbank.dtype == torch.float32 and fbank.dim() == 3 and fbank.is_contiguous()):
        raise _lib.AvsiamHipError("normalize_fbank: need a contiguous fp32 [B, T, F] GPU tensor")
    B, T, F = fbank.shape
    out = torch.empty_like(fbank)
    if noise and shift is None:
        rng = rng if rng is not None else np.random.default_rng(seed)
        amp = torch.from_numpy((rng.random(B) / 10).astype(np.float32)).to(fbank.device)
        shift = torch.from_numpy(rng.integers(-T, T, B).astype(np.int32)).to(fbank.device)
    _lib.call("avs_normalize_audio", fbank, out, B, T, F, float(norm_mean), float(norm_std), shift, amp, int(seed), _lib.current_stream())
    return out


def augment_fbank(fbank, plan, norm_mean=0.0, norm_std=1.0, raw=True, fill=None):
    """The fine-tuning augmentation (dataloader_ft.py:527-548) as a pass of its own: fbank [B, T, F] fp32 (GPU) and an ``ops.FtAug`` plan ->
    the fp32 tensor the model sees - SpecAugment masks (value 0.0 on the un-normalised fbank), (x - norm_mean) / norm_std, noise, time roll.
    raw=False: ``fbank`` is already normalised; masked cells then take ``fill`` (default: the plan's ``fill``).  raw=True: ``fill`` defaults
    to what the reference's order gives a masked cell, (0 - norm_mean) / norm_std.  (The training path does not call this:
    ``train_step(..., aug=)`` applies the same arithmetic inside the patch gather; this two-pass form is what tests compare it with.)"""
    from . import ops
    out = torch.empty_like(fbank)
    ops.augment_audio(fbank, out, plan, 1 if raw else 0, norm_mean, norm_std, fill)
    return out


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """First output word of Philox4x32-10 (Salmon et al., SC'11) on numpy arrays / ints -> uint32 array: the restatement of the device
    streams (csrc/common.h xf_philox / xf_philox4)."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint32)


def noise_reference(noise_key, B, T, F):
    """U(ts * F + f, b) of the augmentation's noise field (and of normalize_fbank's for seed = noise_key): float32 [B, T, F] in [0, 1),
    indexed by the UN-rolled frame ts."""
    e = np.arange(T * F, dtype=np.uint64)[None, :]
    b = np.arange(B, dtype=np.uint64)[:, None]
    w = philox4x32_10(e, b, 0, 0, int(noise_key) & 0xFFFFFFFF, (int(noise_key) >> 32) & 0xFFFFFFFF)
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).reshape(B, T, F)


def draw_plan_reference(key, counter, B, T, F, freqm, timem, noise):
    """numpy restatement of avs_ft_aug_draw (include/avsiam_hip.h states the formulas): the plan draw number `counter` of the 64-bit `key`
    for B samples -> dict of int32 arrays f0, fn, t0, tn, shift, float32 amp (all [B]) and the int `noise_key`.  Integer arithmetic only
    (Python ints / uint64), amp one float32 division: equal to the device draw bit for bit.  For tests, and for loaders that draw on the host
    (``ops.FtAug.from_arrays``)."""
    if not (0 <= freqm <= F and 0 <= timem <= T and 0 < T < 32768 and 0 < F < 32768 and B > 0):
        raise ValueError(f"draw_plan_reference: freqm {freqm} / timem {timem} outside 0..F ({F}) / 0..T ({T}), or a size outside 1..32767")
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    c = int(counter) & 0xFFFFFFFF
    b = np.arange(B, dtype=np.uint64)
    u = [(philox4x32_10(b, q, c, 1, k0, k1) >> np.uint32(8)).astype(np.uint64) for q in range(6)]

    def span(u1, u2, param, size):
        value = u1 * np.uint64(param)                                   # < 2^39
        n = value >> np.uint64(24)
        start = (u2 * ((np.uint64(size) << np.uint64(24)) - value)) >> np.uint64(48)          # < 2^63: no wrap
        return start.astype(np.int32), n.astype(np.int32)

    zero = np.zeros(B, dtype=np.int32)
    f0, fn = span(u[0], u[1], freqm, F) if freqm > 0 else (zero.copy(), zero.copy())
    t0, tn = span(u[2], u[3], timem, T) if timem > 0 else (zero.copy(), zero.copy())
    if noise:
        shift = ((u[4] * np.uint64(2 * T)) >> np.uint64(24)).astype(np.int64) - T
        amp = (u[5].astype(np.float32) * np.float32(1.0 / 16777216.0)) / np.float32(10.0)
    else:
        shift, amp = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float32)
    nk = int(philox4x32_10(c, 0, 0, 2, k0, k1)[()]) | (int(philox4x32_10(c, 1, 0, 2, k0, k1)[()]) << 32)
    return {"f0": f0, "fn": fn, "t0": t0, "tn": tn, "shift": shift.astype(np.int32), "amp": amp.astype(np.float32), "noise_key": nk}


def normalize_frames(frames_u8, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
    """frames [..., 3, H, W] uint8 (GPU) -> fp32 (x / 255 - mean_c) / std_c (dataloader.py:461-462 and my_normalize)."""
    if not (frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() >= 3 and frames_u8.shape[-3] == 3
            and frames_u8.is_contiguous()):
        raise _lib.AvsiamHipError("normalize_frames: need a contiguous uint8 [..., 3, H, W] GPU tensor")
    plane = frames_u8.shape[-1] * frames_u8.shape[-2]
    n = frames_u8.numel() // (3 * plane)
    out = torch.empty(frames_u8.shape, dtype=torch.float32, device=frames_u8.device)
    m3 = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s3 = (ctypes.c_float * 3)(*[float(x) for x in std])
    _lib.call("avs_normalize_frames_u8", frames_u8, out, n, plane, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p),
              _lib.current_stream())
    return out
