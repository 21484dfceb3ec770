"""Input normalisation on the device - the per-sample host work of the reference dataloader
(/root/reference/src/dataloader.py:505-513 audio, :461-462 + :152-155 frames) as two HBM-bound kernels, so that raw
AudioSet-shaped tensors can be fed to ``CAVMAE_BASE.forward`` without a CPU pass.  No CPU fallback.

Waveform input (the fine-tuning loader, dataloader_ft.py:277-340, 441-475): ``kaldi_fbank_reference`` is the float64 numpy SPECIFICATION of the device
fbank (``ops.kaldi_fbank``, csrc/frontend.hip) - the Kaldi definition with the arguments of the reference's call, restated, not recorded:
torchaudio was not available where this was written, so no golden from ``torchaudio.compliance.kaldi.fbank`` exists - and ``mixup_labels`` is
the label side of mixup.  The frame side is ``ops.mix_frames``."""
import collections
import ctypes
import os

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


# ---- waveform input: the Kaldi fbank of the fine-tuning loader (dataloader_ft.py:277-340) -----------------------------------------------
FBANK_FRAME, FBANK_SHIFT, FBANK_NFFT, FBANK_SR = 400, 160, 512, 16000
FLT_EPSILON = 1.1920929e-07
FBANK_FLOOR = np.float32(np.log(np.float64(np.float32(FLT_EPSILON))))        # -15.942385: what an energy at or below FLT_EPSILON becomes


def fbank_frames(n):
    """frames of an n-sample clip under snip_edges=True, 25 ms / 10 ms at 16 kHz"""
    return 1 + (int(n) - FBANK_FRAME) // FBANK_SHIFT if n >= FBANK_FRAME else 0


def fbank_mel_weights(n_mels=128):
    """[n_mels, 257] float64 triangles of the Kaldi definition (htk_compat changes nothing without use_energy): mel(f) = 1127 ln(1 + f / 700),
    low 20 Hz, high Nyquist, evaluated at the mel of every FFT bin; bin 256 has weight 0.  At 128 filters filter 3 holds no bin."""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    lo, hi = mel(20.0), mel(FBANK_SR / 2)
    delta = (hi - lo) / (n_mels + 1)
    left = lo + np.arange(n_mels, dtype=np.float64)[:, None] * delta
    centre = left + delta
    right = centre + delta
    m = mel((FBANK_SR / FBANK_NFFT) * np.arange(FBANK_NFFT // 2))[None, :]
    w = np.maximum(0.0, np.minimum((m - left) / delta, (right - m) / delta))
    return np.concatenate([w, np.zeros((n_mels, 1))], axis=1)


def kaldi_fbank_reference(wave, lengths=None, partner=None, partner_lengths=None, lam=None, target_length=1024, n_mels=128, norm=None,
                          dtype=np.float64, return_energy=False):
    """The specification of ``ops.kaldi_fbank`` in numpy: torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=16000,
    use_energy=False, window_type='hanning', num_mel_bins=n_mels, dither=0.0, frame_shift=10) with torchaudio's other defaults (25 ms frames,
    preemphasis 0.97, remove_dc_offset, round_to_power_of_two, snip_edges, low_freq 20, high_freq Nyquist, power, log), restated from the Kaldi
    definition - torchaudio itself was never available to record from - plus what the loader does around it (dataloader_ft.py:277-340).

    wave [B, S] (or [S]); lengths [B] samples per clip (None: S), each >= 400 (ValueError otherwise; the reference's try/except constant is not
    reproduced).  Plain clip: w - mean(w).  Mixed clip (partner given and lam[b] >= 0): a = w1 - mean(w1), c = w2 - mean(w2) over the
    partner's own length, THEN zero-padded or cut to the clip's length, mix = lam a + (1 - lam) c, the waveform is mix - mean(mix).
    Frames: m = 1 + (n - 400) // 160; per frame: subtract the mean, y[i] = x[i] - 0.97 x[max(i - 1, 0)], Hann 0.5 - 0.5 cos(2 pi i / 399),
    zero-pad to 512, |rfft|^2, the mel triangles, ln(max(E, FLT_EPSILON)).  Rows m .. target_length - 1 are 0, frames beyond are cut.
    norm=(mean, std): (out - mean) / std on every row, pad rows included.  dtype=np.float32 runs the same steps in single precision
    (scipy.fft keeps float32): what plain fp32 arithmetic gets.  -> [B, target_length, n_mels] of `dtype`; with return_energy also the mel
    energies E before floor and log (same shape, pad rows 0), the quantity the kernel's energy-domain error is measured against."""
    import scipy.fft
    dt = np.dtype(dtype).type
    wave = np.asarray(wave)
    if wave.ndim == 1:
        wave = wave[None]
    B, S = wave.shape
    lengths = np.full(B, S, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(B)
    if partner is not None:
        partner = np.asarray(partner)
        partner = partner[None] if partner.ndim == 1 else partner
        partner_lengths = (np.full(B, partner.shape[1], dtype=np.int64) if partner_lengths is None
                           else np.asarray(partner_lengths, dtype=np.int64).reshape(B))
    lam = None if (lam is None or partner is None) else np.asarray(lam, dtype=np.float64).reshape(B)
    if (lengths < FBANK_FRAME).any() or (lengths > S).any():
        raise ValueError(f"kaldi_fbank: every clip needs 400 .. {S} samples, got lengths {lengths.tolist()}")
    i = np.arange(FBANK_FRAME, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FBANK_FRAME - 1))).astype(dt)
    melw = fbank_mel_weights(n_mels).astype(dt)
    out = np.zeros((B, target_length, n_mels), dtype=dt)
    energies = np.zeros((B, target_length, n_mels), dtype=dt)
    for b in range(B):
        n = int(lengths[b])
        w = wave[b, :n].astype(dt)
        w = w - w.mean(dtype=dt)
        if lam is not None and lam[b] >= 0:
            n2 = int(partner_lengths[b])
            if not 1 <= n2 <= partner.shape[1]:
                raise ValueError(f"kaldi_fbank: partner length {n2} outside 1 .. {partner.shape[1]}")
            w2 = partner[b, :n2].astype(dt)
            w2 = w2 - w2.mean(dtype=dt)
            c = np.zeros(n, dtype=dt)
            c[:min(n, n2)] = w2[:n]
            mix = dt(lam[b]) * w + (dt(1.0) - dt(lam[b])) * c
            w = mix - mix.mean(dtype=dt)
        m = min(fbank_frames(n), target_length)
        idx = FBANK_SHIFT * np.arange(m)[:, None] + np.arange(FBANK_FRAME)[None, :]
        fr = w[idx]
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=dt)
        fr = (fr - dt(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)) * window
        spec = scipy.fft.rfft(fr, n=FBANK_NFFT, axis=1)
        power = (spec.real * spec.real + spec.imag * spec.imag).astype(dt)
        energy = power @ melw.T
        energies[b, :m] = energy
        out[b, :m] = np.log(np.maximum(energy, dt(FLT_EPSILON)))
    if norm is not None:
        out = ((out - dt(norm[0])) / dt(norm[1])).astype(dt)
    return (out, energies) if return_energy else out


def mixup_labels(y1_hot, y2_hot, lam, label_smooth):
    """Labels of the fine-tuning loader (torch).  y1_hot / y2_hot [B, C] multi-hot (0 / 1), lam [B] (or a float), label_smooth s.  Mixed rows
    (lam >= 0): s / C + lam (1 - s) hot1 + (1 - lam) (1 - s) hot2 (dataloader_ft.py:470-475); rows with lam < 0 (or y2_hot None): the plain
    smoothed labels, 1 - s on the positives and s / C elsewhere (:480, :524)."""
    y1 = y1_hot.to(torch.float32)
    B, C = y1.shape
    lam = torch.as_tensor(lam, dtype=torch.float32, device=y1.device).expand(B).reshape(B, 1)
    s = float(label_smooth)
    plain = torch.where(y1 > 0.5, torch.full_like(y1, 1.0 - s), torch.full_like(y1, s / C))
    if y2_hot is None:
        return plain
    mixed = s / C + lam * (1.0 - s) * y1 + (1.0 - lam) * (1.0 - s) * y2_hot.to(torch.float32)
    return torch.where(lam >= 0, mixed, plain)


# ---- decoded-size frames: the antialiased bicubic Resize of the fine-tuning loader (dataloader_ft.py:136-139, 434-459) ----------------------
RESIZE_MAX_SCALE, RESIZE_MAX_TAPS = 10, 41


def _resize_cubic(x):
    """the cubic convolution kernel, a = -0.5, every product and sum rounded on its own in the order csrc/frontend_math.h's rz_cubic writes"""
    ax = np.abs(x)
    near = (1.5 * ax - 2.5) * ax * ax + 1.0
    far = (((ax - 5.0) * ax + 8.0) * ax - 4.0) * -0.5
    return np.where(ax < 1.0, near, np.where(ax < 2.0, far, 0.0))


def resize_taps_reference(I, O):
    """One axis of torch.nn.functional.interpolate(mode='bicubic', align_corners=False, antialias=True) from I to O samples, in float64:
    scale = I / O, s = max(scale, 1), support = 2 s; output index i: centre = scale (i + 0.5), start = max(int(centre - support + 0.5), 0),
    end = min(int(centre + support + 0.5), I), w_j = cubic((j + start - centre + 0.5) / s) for j < end - start, divided by their sum (added
    in tap order).  -> (start int32 [O], count int32 [O], weights float64 [O, max count], zero beyond each count).  Rounded once to fp32 the
    weights are the kernel's, bit for bit (avs_resize_taps)."""
    I, O = int(I), int(O)
    if I < 1 or O < 1:
        raise ValueError(f"resize_taps: sizes {I} -> {O}")
    scale = np.float64(I) / np.float64(O)
    s = max(scale, np.float64(1.0))
    support = 2.0 * s
    start, count, rows = np.zeros(O, dtype=np.int32), np.zeros(O, dtype=np.int32), []
    for i in range(O):
        centre = scale * (np.float64(i) + 0.5)
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), I)
        w = _resize_cubic(((np.arange(lo, hi, dtype=np.float64) - centre) + 0.5) / s)
        total = np.float64(0.0)
        for v in w:
            total = total + v
        start[i], count[i] = lo, hi - lo
        rows.append(w / total)
    weights = np.zeros((O, int(count.max())), dtype=np.float64)
    for i, w in enumerate(rows):
        weights[i, :len(w)] = w
    return start, count, weights


def _resize_matrix(I, O, dtype):
    """the taps of one axis as a dense [O, I] matrix (weights rounded to `dtype` first)"""
    start, count, w = resize_taps_reference(I, O)
    m = np.zeros((O, I), dtype=dtype)
    for i in range(O):
        m[i, start[i]:start[i] + count[i]] = w[i, :count[i]].astype(dtype)
    return m


def resize_frames_reference(frames_u8, sizes=None, partner=None, partner_sizes=None, weight=None, size=224, mean=IMAGENET_DEFAULT_MEAN,
                            std=IMAGENET_DEFAULT_STD, dtype=np.float64):
    """The specification of ``ops.resize_frames`` in numpy float64: what the reference's loader does to decoded frames
    (dataloader_ft.py:136-139, 434-459), with torchvision's Resize restated from torch's interpolate (``resize_taps_reference``).

    frames_u8 uint8 [B, 3, Hs, Ws] or [B, F, 3, Hs, Ws], a padded buffer: clip b fills the top-left sizes[b] = (h, w) corner (None: Hs x Ws);
    what lies outside is never read.  size: int or (out_h, out_w).  Per clip and channel:
      1. x = the clip's h x w pixels as float (the division by 255 comes after the resize, where the kernel has it: the filter is linear)
      2. horizontal pass: r[y, i] = sum_j wx[i, j] x[y, start_x[i] + j]
      3. vertical pass:   r[i, :] = sum_j wy[i, j] r[start_y[i] + j, :]            (no clamping: overshoot outside [0, 255] stays)
      4. n(r) = (r / 255 - mean_c) / std_c
      5. with a partner (its own buffer and sizes): weight_b n(r) + (1 - weight_b) n(r_partner)            (:457-458)
    dtype=np.float32 runs the same steps with fp32 weights and fp32 sums.  -> [..., 3, out_h, out_w] of `dtype`."""
    dt = np.dtype(dtype).type
    out_h, out_w = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)

    def one(buf, szs):
        buf = np.asarray(buf)
        if buf.dtype != np.uint8 or buf.ndim not in (4, 5) or buf.shape[-3] != 3:
            raise ValueError(f"resize_frames: need uint8 [B, 3, H, W] or [B, F, 3, H, W], got {buf.dtype} {buf.shape}")
        B, (Hs, Ws) = buf.shape[0], buf.shape[-2:]
        szs = np.tile([[Hs, Ws]], (B, 1)) if szs is None else np.asarray(szs, dtype=np.int64).reshape(B, 2)
        res = np.zeros(buf.shape[:-2] + (out_h, out_w), dtype=dt)
        for b in range(B):
            h, w = int(szs[b, 0]), int(szs[b, 1])
            if not (1 <= h <= Hs and 1 <= w <= Ws) or h > RESIZE_MAX_SCALE * out_h or w > RESIZE_MAX_SCALE * out_w:
                raise ValueError(f"resize_frames: clip {b} is {h} x {w}: sizes lie in 1 .. {Hs} x {Ws} and within {RESIZE_MAX_SCALE} times the output")
            mx, my = _resize_matrix(w, out_w, dt), _resize_matrix(h, out_h, dt)
            x = buf[b, ..., :h, :w].astype(dt)
            r = np.matmul(my, np.matmul(x, mx.T))
            n = (r / dt(255.0) - mean.astype(dt)[:, None, None]) / std.astype(dt)[:, None, None]
            res[b] = n
        return res

    a = one(frames_u8, sizes)
    if partner is None:
        if partner_sizes is not None or weight is not None:
            raise ValueError("resize_frames: partner_sizes / weight without a partner")
        return a
    c = one(partner, partner_sizes)
    if c.shape != a.shape:
        raise ValueError(f"resize_frames: the partner gives {c.shape}, the clips {a.shape}")
    wgt = np.asarray(weight, dtype=dt).reshape((a.shape[0],) + (1,) * (a.ndim - 1))
    return (wgt * a + (dt(1.0) - wgt) * c).astype(dt)


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


def unpatchify_reference(rows, base, audio, stride=16, mask=None):
    """numpy restatement of avs_unpatchify (unpatchify, cav_mae_base.py:353-363, on 16 x 16 patch storage): rows [n, L, 256 * C] -> a copy of
    ``base`` ([n, T, F] spectrograms, or [n, C, H, W] frames) with the stride x stride cells of every token (``mask`` [n, L] given: of the
    tokens whose mask is 1) taken from its row.  Audio: token f * tP + t, element p * 16 + q -> cell (t * S + q, f * S + p); frames: token
    gy * G + gx, element (p * 16 + q) * C + c -> cell (c, gy * S + p, gx * S + q).  Cells no patch covers keep ``base``.  Pure data movement:
    the result holds the rows' and the base's values bit for bit."""
    rows, out = np.asarray(rows), np.array(base, copy=True)
    S = int(stride)
    if audio:
        n, T, F = out.shape
        C, nr, nc = 1, T // S, F // S                                       # time patches, mel patches
    else:
        n, C, H, W = out.shape
        nr, nc = H // S, W // S
    L = nr * nc
    if rows.shape != (n, L, 256 * C) or not 0 < S <= 16:
        raise ValueError(f"unpatchify_reference: rows {rows.shape} for {n} pictures of {L} tokens x {256 * C}, stride {S}")
    take = np.ones((n, L), dtype=bool) if mask is None else np.asarray(mask).reshape(n, L) == 1
    if audio:
        r = rows.reshape(n, nc, nr, 16, 16)[:, :, :, :S, :S]                # [n, f, t, p, q]
        full = r.transpose(0, 2, 4, 1, 3).reshape(n, nr * S, nc * S)        # [n, t, q, f, p]
        tk = take.reshape(n, nc, nr).transpose(0, 2, 1)                     # [n, t, f]
        tk = np.repeat(np.repeat(tk, S, axis=1), S, axis=2)
        view = out[:, :nr * S, :nc * S]
    else:
        r = rows.reshape(n, nr, nc, 16, 16, C)[:, :, :, :S, :S]             # [n, gy, gx, p, q, c]
        full = r.transpose(0, 5, 1, 3, 2, 4).reshape(n, C, nr * S, nc * S)  # [n, c, gy, p, gx, q]
        tk = np.repeat(np.repeat(take.reshape(n, 1, nr, nc), S, axis=2), S, axis=3)
        tk = np.broadcast_to(tk, full.shape)
        view = out[:, :, :nr * S, :nc * S]
    view[tk] = full[tk]
    return out


def unnormalize_reference(x, mean, std, audio):
    """numpy float32 restatement of avs_unpatchify's raw output: audio x * std + mean; frames [..., 3, H, W] -> uint8
    rint((x * std_c + mean_c) * 255) clamped to 0..255.  Multiply and add are rounded separately, as the kernel does."""
    x = np.asarray(x, dtype=np.float32)
    if audio:
        return x * np.float32(std) + np.float32(mean)
    shape = (3, 1, 1)
    v = (x * np.asarray(std, dtype=np.float32).reshape(shape) + np.asarray(mean, dtype=np.float32).reshape(shape)) * np.float32(255.0)
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.rint(v), nan=0.0), 0, 255).astype(np.uint8)


# ---- source-rate audio: the windowed-sinc resample of the fine-tuning loader (dataloader_ft.py:272-277, 298-306) ---------------------------
RESAMPLE_MAX_RATES, RESAMPLE_MAX_CHANNELS, RESAMPLE_MAX_WORDS = 8, 8, 16384


def _resample_ratio(orig_freq, new_freq):
    """(o, n): the two rates over their gcd; ValueError for anything but positive integers"""
    import math
    import numbers
    for f in (orig_freq, new_freq):
        if isinstance(f, bool) or not isinstance(f, numbers.Integral) or int(f) < 1:
            raise ValueError(f"resample: rates must be positive integers, got {orig_freq!r} -> {new_freq!r}")
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


_rate_problems = {}           # (orig, new) -> None or the reason


def resample_rate_problem(orig_freq, new_freq=16000):
    """None where ops.resample_wave takes a clip at `orig_freq`, else the reason as text - on the host, without a device: the caps that
    ops.resample_table applies to a rate pair (csrc/resample.hip: a compact table of at most 16 384 words, an input span of at most 16 384
    samples per tile of 1 024 outputs), so that a file loader can set such a clip aside when it parses the header."""
    import math
    key = (orig_freq, new_freq)
    if key in _rate_problems:
        return _rate_problems[key]
    try:
        o, n = _resample_ratio(orig_freq, new_freq)
    except ValueError as e:
        return str(e)
    tile, max_span, why = 1024, 16384, None
    width = math.ceil(6 * o / (min(o, n) * 0.99))
    if o == n:
        pass                                                            # (a clip at the target rate is not filtered)
    elif n * 14 > RESAMPLE_MAX_WORDS:
        why = f"{orig_freq} -> {new_freq} Hz has {n} filter phases: more than the resample kernel's table holds"
    elif ((tile - 1) // n + 2) * o + 2 * width + 3 > max_span:
        why = f"{orig_freq} -> {new_freq} Hz: the input span of {tile} outputs is over {max_span} samples"
    else:
        taps = resample_compact_table(resample_table_reference(orig_freq, new_freq)[0])[1].shape[1]
        if n * ((taps | 1) + 1) > RESAMPLE_MAX_WORDS:
            why = f"{orig_freq} -> {new_freq} Hz: {n} phases x {taps} taps: more than the resample kernel's table holds"
    if len(_rate_problems) < 4096:
        _rate_problems[key] = why
    return why


def _resample_phase(n):
    """the phase term of the table, -p / n for p = 0 .. n - 1 as torch promotes it: an int64 arange divided by an int is FLOAT32"""
    return torch.arange(0, -n, -1)[:, None, None] / n


def resample_table_reference(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The filter bank of torchaudio.functional.resample(waveform, orig_freq, new_freq) - torchaudio's _get_sinc_resample_kernel with
    resampling_method='sinc_interp_hann' and dtype=None, as functional.resample calls it - restated in torch on the CPU so that torch's own
    type promotion decides the dtypes.  The formula is written down from the maintainer's memory of torchaudio: torchaudio was not available
    where this was written, NO RECORDING EXISTS TO CHECK IT AGAINST, and someone with torchaudio can add a golden under tests/golden/.

      g = gcd(orig, new); o = orig // g; n = new // g
      base  = min(o, n) * rolloff
      width = ceil(lowpass_filter_width * o / base)
      idx   = arange(-width, width + o, dtype=float64)[None, None] / o
      t     = arange(0, -n, -1)[:, None, None] / n + idx        the int64 arange divided by an int is float32; the sum with idx is float64
      t    *= base; t.clamp_(-lowpass_filter_width, lowpass_filter_width)
      window = cos(t * pi / lowpass_filter_width / 2) ** 2
      t    *= pi
      k     = where(t == 0, 1.0, sin(t) / t) * window * (base / o)
      table = k.to(float32)

    The float32 phase term is deliberate: it is what the torch expression does; against a float64 phase it moves table entries by up to
    1.9e-6 (44 100 Hz), 7.4e-6 (22 050 Hz), 1.4e-5 (11 025 Hz).  -> (table float32 [n, 1, 2 * width + o], width)."""
    import math
    o, n = _resample_ratio(orig_freq, new_freq)
    lpw = int(lowpass_filter_width)
    if lpw < 1 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError(f"resample: lowpass_filter_width {lowpass_filter_width} / rolloff {rolloff}")
    base = min(o, n) * float(rolloff)
    width = math.ceil(lpw * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = _resample_phase(n) + idx
    t *= base
    t.clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t *= math.pi
    scale = base / o
    k = torch.where(t == 0, torch.tensor(1.0, dtype=t.dtype), t.sin() / t)
    k = k * window * scale
    return k.to(torch.float32), width


def resample_compact_table(table):
    """The table as the kernel reads it.  In fp32 every phase's non-zero taps form one contiguous run (ValueError otherwise): per phase the
    index `first` of the run's first tap and the run's weights, padded with the zeros that follow to K = the largest run of the table.
    `first` is moved down to L - K where the run ends at the row's end, so that first + K <= L for every phase.  table float32 [n, 1, L] (or
    [n, L]) -> (first int32 [n], weights float32 [n, K]), numpy."""
    t = np.asarray(table, dtype=np.float32)
    t = t.reshape(t.shape[0], t.shape[-1])
    n, L = t.shape
    nz = t != 0
    if not nz.any(axis=1).all():
        raise ValueError("resample: a phase of the table has no non-zero tap")
    lo = nz.argmax(axis=1)
    hi = L - nz[:, ::-1].argmax(axis=1)                                  # one past the last non-zero tap
    if int((hi - lo).sum()) != int(nz.sum()):
        raise ValueError("resample: the non-zero taps of a phase are not one contiguous run")
    K = int((hi - lo).max())
    first = np.minimum(lo, L - K).astype(np.int32)
    weights = t[np.arange(n)[:, None], first[:, None] + np.arange(K)[None, :]]
    return first, np.ascontiguousarray(weights)


def resample_expand_table(first, weights, L):
    """the dense [n, L] float32 table of a compact one (resample_compact_table's inverse)"""
    first, weights = np.asarray(first), np.asarray(weights, dtype=np.float32)
    n, K = weights.shape
    t = np.zeros((n, int(L)), dtype=np.float32)
    t[np.arange(n)[:, None], first[:, None] + np.arange(K)[None, :]] = weights
    return t


def resample_out_length(length, orig_freq, new_freq):
    """ceil(n * length / o) in exact integers: the samples torchaudio's resample returns for `length` input samples"""
    o, n = _resample_ratio(orig_freq, new_freq)
    return -((-n * int(length)) // o)


def resample_channels(x, table, width, o, n, m):
    """outputs 0 .. m - 1 of every channel of one clip, before the channel mean: x float64 [C, len], table float64 [n, 2 width + o] ->
    [C, m] with out[c, q n + p] = sum_m table[p, m] x[c, q o + m - width], samples outside the clip zero.  (Called with |table| and |x| it
    gives the sum of the products' magnitudes: what the tests' error bounds are made of.)"""
    C, ln = x.shape
    L = table.shape[1]
    nq = -(-int(m) // n) if m else 0
    padded = np.zeros((C, width + nq * o + L), dtype=np.float64)
    padded[:, width:width + ln] = x
    acc = np.zeros((C, nq, n), dtype=np.float64)
    for q in range(nq):
        acc[:, q, :] = padded[:, q * o:q * o + L] @ table.T
    return acc.reshape(C, nq * n)[:, :m]


def resample_reference(wave, rates, lengths=None, new_freq=16000):
    """The specification of ``ops.resample_wave`` in float64: what the reference's loader does to decoded audio ahead of the fbank
    (dataloader_ft.py:272-277, 298-306) - torchaudio.functional.resample(waveform, sr, 16000) when sr != 16000, then waveform.mean(dim=0).

    wave [B, C, stride] or [B, stride] (one channel); rates: an int or B ints, the clips' own sample rates; lengths [B] samples per clip
    (None: stride).  Per clip of `len` samples at a rate with o = rate / gcd, n = new_freq / gcd and table [n, L], L = 2 width + o
    (``resample_table_reference``; its fp32 values taken as doubles), per channel and output j = q n + p, 0 <= p < n:
        out[j] = sum_m table[p, m] * x[q o + m - width]          for j < ceil(n len / o); samples outside 0 .. len - 1 count as zero
    then the mean over the channels.  A clip whose rate equals new_freq is not filtered: only its channel mean is taken (the reference's
    `if sr != 16000`).  Two quirks of the reference are NOT rebuilt (INTEGRATION.md 2(a'')): it hands the file's sr to the fbank after
    resampling, and it resamples the mixup partner by the first file's sr.
    -> (out float64 [B, out_stride], out_lengths int64 [B]); the tail of every row is zero; out_stride is the largest ceil(n stride / o) over
    the call's rates."""
    wave = np.asarray(wave)
    if wave.ndim == 2:
        wave = wave[:, None, :]
    if wave.ndim != 3:
        raise ValueError(f"resample: need [B, C, stride] or [B, stride], got {wave.shape}")
    B, C, stride = wave.shape
    rates = [int(rates)] * B if np.isscalar(rates) else [int(r) for r in rates]
    if len(rates) != B:
        raise ValueError(f"resample: {len(rates)} rates for {B} clips")
    lengths = np.full(B, stride, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(B)
    if (lengths < 0).any() or (lengths > stride).any():
        raise ValueError(f"resample: lengths must lie in 0 .. {stride}, got {lengths.tolist()}")
    out_stride = max(resample_out_length(stride, r, new_freq) for r in rates)
    out = np.zeros((B, out_stride), dtype=np.float64)
    out_lengths = np.zeros(B, dtype=np.int64)
    tables = {}
    for b in range(B):
        ln = int(lengths[b])
        x = wave[b, :, :ln].astype(np.float64)
        if rates[b] == int(new_freq):
            out[b, :ln] = x.mean(axis=0)
            out_lengths[b] = ln
            continue
        if rates[b] not in tables:
            tab, width = resample_table_reference(rates[b], new_freq)
            tables[rates[b]] = (tab[:, 0, :].numpy().astype(np.float64), width)
        tab, width = tables[rates[b]]
        o, n = _resample_ratio(rates[b], new_freq)
        m = resample_out_length(ln, rates[b], new_freq)
        out[b, :m] = resample_channels(x, tab, width, o, n, m).mean(axis=0)
        out_lengths[b] = m
    return out, out_lengths


# ---- WAV files: the container walk on the host and the specification of the PCM decode kernel (dataloader_ft.py:272: torchaudio.load) ----------
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = range(6)                 # csrc/decode.hip
PCM_NAMES = ("U8", "S16", "S24", "S32", "F32", "F64")
PCM_BYTES = (1, 2, 3, 4, 4, 8)
PCM_MAX_CHANNELS = 8
_WAVE_TAGS = {0x0002: "ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10", 0x0055: "MPEG layer 3"}
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")               # a sub-format GUID after its two tag bytes


class WavInfo(collections.namedtuple("WavInfo", "format channels rate n_frames data_offset data_bytes")):
    """parse_wav's result: format (PCM_U8 .. PCM_F64), channels, rate (Hz), n_frames (whole sample frames), data_offset (of the payload in the
    file) and data_bytes = n_frames * channels * PCM_BYTES[format]"""
    __slots__ = ()


def parse_wav(src, name=None):
    """The RIFF / WAVE container of one file on the host: `src` bytes (bytearray, memoryview, a uint8 numpy array) or a path; `name` is what an error calls the file
    (default: the path, or '<bytes>').  -> WavInfo(format, channels, rate, n_frames, data_offset, data_bytes).

    The chunks are walked as the container defines them: an odd-sized chunk is followed by a pad byte, and chunks other than 'fmt ' and 'data'
    (LIST, fact, bext ...) may stand anywhere.  'fmt ' of 16, 18 or 40 bytes; WAVE_FORMAT_EXTENSIBLE is resolved through its sub-format GUID to
    PCM or IEEE float.  A 'data' size of 0 or 0xFFFFFFFF (a streamed file) means the data runs to the end of the file, and a data chunk
    that the file cuts short is floored to whole sample frames.  Refused with a ValueError naming the file and the reason: anything that is
    not RIFF / WAVE (RIFX is big endian), a compressed coding (A-law, mu-law, ADPCM ...), a sample size outside 8 / 16 / 24 / 32 bit PCM and
    32 / 64 bit float, more than 8 channels, and a block_align other than channels * bytes per sample."""
    import struct
    if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
        buf, name = memoryview(src).cast("B"), name or "<bytes>"           # (no copy: a loader hands the whole file over)
    else:
        name = name or os.fspath(src)
        with open(src, "rb") as f:
            buf = memoryview(f.read())

    def bad(reason):
        return ValueError(f"{name}: {reason}")

    if len(buf) < 12:
        raise bad(f"not a WAV file: {len(buf)} bytes are too few for a RIFF header")
    if buf[:4] == b"RIFX":
        raise bad("RIFX (big-endian) files are not supported")
    if buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise bad(f"not a RIFF / WAVE file (it starts with {bytes(buf[:4])!r} .. {bytes(buf[8:12])!r})")
    fmt, data, pos = None, None, 12
    while pos + 8 <= len(buf):
        cid, size = bytes(buf[pos:pos + 4]), struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + 16 > len(buf):
                raise bad(f"'fmt ' chunk of {size} bytes: at least 16 are needed")
            fmt = bytes(buf[body:body + min(size, len(buf) - body)])
        elif cid == b"data":
            avail = len(buf) - body
            open_end = size in (0, 0xFFFFFFFF)
            data = (body, avail if open_end else min(size, avail))
            if open_end:
                break
        pos = body + size + (size & 1)
    if fmt is None:
        raise bad("no 'fmt ' chunk")
    if data is None:
        raise bad("no 'data' chunk")
    tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise bad(f"WAVE_FORMAT_EXTENSIBLE with a 'fmt ' chunk of {len(fmt)} bytes: 40 are needed")
        if fmt[26:40] != _KSDATAFORMAT_TAIL:
            raise bad(f"WAVE_FORMAT_EXTENSIBLE with an unknown sub-format GUID {fmt[24:40].hex()}")
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if tag == 1:
        code = {8: PCM_U8, 16: PCM_S16, 24: PCM_S24, 32: PCM_S32}.get(bits)
        if code is None:
            raise bad(f"{bits}-bit PCM: 8, 16, 24 and 32 bits are decoded")
    elif tag == 3:
        code = {32: PCM_F32, 64: PCM_F64}.get(bits)
        if code is None:
            raise bad(f"{bits}-bit IEEE float: 32 and 64 bits are decoded")
    else:
        raise bad(f"format tag 0x{tag:04x} ({_WAVE_TAGS.get(tag, 'not PCM or IEEE float')}): compressed audio is not decoded")
    if not 1 <= channels <= PCM_MAX_CHANNELS:
        raise bad(f"{channels} channels: 1 .. {PCM_MAX_CHANNELS} are supported")
    if rate < 1:
        raise bad("a sample rate of 0 Hz")
    if block_align != channels * PCM_BYTES[code]:
        raise bad(f"block_align {block_align} is not channels * bytes per sample = {channels} * {PCM_BYTES[code]}")
    n_frames = data[1] // block_align
    return WavInfo(code, int(channels), int(rate), int(n_frames), int(data[0]), int(n_frames * block_align))


def decode_pcm_reference(payload, fmt, channels, n_frames=None):
    """The specification of ``ops.decode_pcm``, bit for bit: the payload of a data chunk (bytes or a uint8 array; interleaved sample frames,
    little endian) -> float32 [channels, n_frames], the convention of torchaudio.load(normalize=True) - written down from memory: torchaudio was
    not available where this was written, and no recording exists to check it against.
        U8   (x - 128) * 2^-7         S16  x * 2^-15         S24  (3 bytes, sign-extended) x * 2^-23            all exact in fp32
        S32  float32(x), rounded to nearest even, * 2^-31 (INT_MAX gives 1.0)        F64  float32(x): one rounding each
        F32  the bits: NaN payloads and -0.0 pass untouched
    n_frames None: every whole frame of the payload."""
    fmt, C = int(fmt), int(channels)
    if not 0 <= fmt < len(PCM_BYTES) or not 1 <= C <= PCM_MAX_CHANNELS:
        raise ValueError(f"decode_pcm: format {fmt} (0 .. 5), channels {C} (1 .. {PCM_MAX_CHANNELS})")
    raw = np.frombuffer(payload, dtype=np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
    bps = PCM_BYTES[fmt]
    held = raw.size // (C * bps)
    n = held if n_frames is None else int(n_frames)
    if not 0 <= n <= held:
        raise ValueError(f"decode_pcm: {n} frames of {C} x {bps} bytes in a payload of {raw.size} bytes")
    raw = raw[:n * C * bps]
    if fmt == PCM_U8:
        x = (raw.astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)
    elif fmt == PCM_S16:
        x = raw.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif fmt == PCM_S24:
        b3 = raw.reshape(-1, 3).astype(np.int32)
        v = b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) * np.float32(2.0 ** -23)
    elif fmt == PCM_S32:
        x = raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == PCM_F32:
        x = raw.view("<u4").astype(np.uint32).view(np.float32)
    else:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            x = raw.view("<f8").astype(np.float32)
    return np.ascontiguousarray(x.reshape(n, C).T)
