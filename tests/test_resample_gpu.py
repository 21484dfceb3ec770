"""Source-rate audio on a real MI355X: the resample kernel (ops.resample_wave = avs_resample_wave) against its float64 specification
(preprocess.resample_reference, which tests/test_resample_cpu.py holds to the literal torch chain), its exact cells, ragged batches,
pass-through clips, the wrapper's refusals, the fbank on the kernel's audio, and the loader and launcher with --sample-rate.

Nothing here was recorded from torchaudio (it was never available).

Exact cells.  A unit sample at input i reaches output j = q n + p through one tap, m = i - q o + width: the output is table[p, m] - one product
with 1.0 and sums with zeros, exact in fp32 - or 0 where m lies outside the row.  With two channels and the impulse in one, the other channel
adds 0 and the division by 2 is exact: the values times 0.5.

The bound of the kernel's error is derived, not fitted.  u = 2^-24, g(k) = k u / (1 - k u) (Higham's gamma), t the taps the kernel runs over
per phase (the compact table's K; the specification multiplies the very same fp32 weights and fp32 samples in float64):
  a channel's output     an fp32 sum of t products, whatever the order and with or without fused multiply-adds, is within
                         E_c = g(t) A_c of the exact sum, A_c = sum_m |w_m x_m|            (g(t) <= (t + 1) u for t (t + 1) u <= 1)
  the channel sum        C - 1 fp32 additions of the computed values: |s - sum a_c| <= sum E_c + g(C - 1) (sum A_c + sum E_c)
  the division by C      one correctly rounded fp32 division: |out - sum a_c / C| <= (1 + u) |s - sum a_c| / C + u sum A_c / C
so  E = ((sum E_c + g(C - 1) (sum A_c + sum E_c)) (1 + u) + u sum A_c) / C  for C > 1 and  E = g(t) A  for C = 1, per output, with A_c from
preprocess.resample_channels on |table| and |x|.  No factor is added.  The worst observed error / E goes to the margin log
(tests.helpers.record_margin), from which profiles/r17/resample_margins.json is committed."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
ISENT = -777
U = 2.0 ** -24
TILE = 1024                                                    # outputs per workgroup (csrc/resample.hip RS_TILE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def pp():
    from avsiam_amd import preprocess
    return preprocess


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(DEV)


def ratio(rate):
    g = math.gcd(rate, 16000)
    return rate // g, 16000 // g


def out_len(length, rate):
    o, n = ratio(rate)
    return -((-n * int(length)) // o)


def run_guarded(wave, rates, lengths=None):
    """ops.resample_wave into an output and a length vector that sit between sentinels -> (out, out_lengths), both checked"""
    B, stride = wave.shape[0], wave.shape[-1]
    rl = [rates] * B if np.isscalar(rates) else list(rates)
    S = max(out_len(stride, r) for r in rl)
    buf = torch.full((B * S + 128,), SENT, dtype=torch.float32, device=DEV)
    lbuf = torch.full((B + 16,), ISENT, dtype=torch.int32, device=DEV)
    out, ol = buf[64:64 + B * S].view(B, S), lbuf[8:8 + B]
    got, got_l = ops().resample_wave(wave, rates, lengths, out=out, out_lengths=ol)
    assert got.data_ptr() == out.data_ptr() and got_l.data_ptr() == ol.data_ptr()
    assert bool((buf[:64] == SENT).all()) and bool((buf[64 + B * S:] == SENT).all()), "the kernel wrote outside its output"
    assert bool((lbuf[:8] == ISENT).all()) and bool((lbuf[8 + B:] == ISENT).all()), "the kernel wrote outside out_lengths"
    assert not bool((out == SENT).any()), "a cell of the output was not written"
    return got, got_l


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. exact cells
def impulse_length(rate):
    """the shortest clip whose outputs fill two tiles and leave a last tile of ONE output; an 8 kHz source gives 2 L outputs, never an odd
    count: there the last tile holds two"""
    o, n = ratio(rate)
    for extra in (1, 2):
        for tiles in range(2, 12):
            want = tiles * TILE + extra
            L = (want * o) // n
            if out_len(L, rate) == want:
                return L, want
    raise AssertionError(rate)


def impulse_expectation(rate, L, positions):
    table, width = pp().resample_table_reference(rate, 16000)
    t = table[:, 0].numpy()
    o, n = ratio(rate)
    m_out = out_len(L, rate)
    j = np.arange(m_out)
    q, p = j // n, j % n
    want = np.zeros((len(positions), m_out), dtype=np.float32)
    for b, i in enumerate(positions):
        m = i - q * o + width
        ok = (m >= 0) & (m < t.shape[1])
        want[b, ok] = t[p[ok], m[ok]]
    return want


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [44100, 48000, 8000, 11025])
def test_impulses_give_the_table(rate, channels):
    o, n = ratio(rate)
    L, m_out = impulse_length(rate)
    assert m_out > 2 * TILE and m_out % TILE in (1, 2)
    positions = [0, 1, o - 1, o, L // 2, L - 2, L - 1]          # one clip each: they are closer than the filter
    x = np.zeros((len(positions), channels, L), dtype=np.float32)
    for b, i in enumerate(positions):
        x[b, channels - 1, i] = 1.0                             # (two channels: the impulse is in the second)
    got, got_l = run_guarded(dev(x if channels > 1 else x[:, 0]), rate)
    want = impulse_expectation(rate, L, positions) * np.float32(1.0 / channels)
    assert got.shape == want.shape and got_l.tolist() == [m_out] * len(positions)
    assert (want != 0).any(axis=1).all()
    assert torch.equal(got.cpu(), torch.from_numpy(want)), int((got.cpu() != torch.from_numpy(want)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the kernel against the float64 restatement: a ragged batch at three rates in one call
RATES3, LENGTHS3 = [44100, 48000, 8000], [4001, 12347, 9000]


def _signal(kind, channels, stride):
    rng = np.random.default_rng(20241020 + channels)
    x = rng.standard_normal((3, channels, stride)) * 0.1
    if kind == "tone":
        x = x + 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(stride)[None, None, :] / np.asarray(RATES3, dtype=np.float64)[:, None, None])
    return x.astype(np.float32)


def derived_bound(x, rates, lengths, ref_l, stride_out):
    """E of the module docstring per output, [B, stride_out]; a pass-through clip has exact channel values: E_c = 0, A_c = |x_c|"""
    g = lambda k: k * U / (1.0 - k * U)
    channels = x.shape[1]
    bound = np.zeros((x.shape[0], stride_out))
    for b, (rate, ln) in enumerate(zip(rates, lengths)):
        xa = np.abs(x[b, :, :ln].astype(np.float64))
        if rate == 16000:
            A, E = xa, np.zeros_like(xa)
        else:
            table, width = pp().resample_table_reference(rate, 16000)
            t = pp().resample_compact_table(table)[1].shape[1]
            o, n = ratio(rate)
            A = pp().resample_channels(xa, np.abs(table[:, 0].numpy().astype(np.float64)), width, o, n, int(ref_l[b]))
            E = g(t) * A
        if channels == 1:
            bound[b, :ref_l[b]] = E[0]
        else:
            bound[b, :ref_l[b]] = ((E.sum(0) + g(channels - 1) * (A.sum(0) + E.sum(0))) * (1 + U) + U * A.sum(0)) / channels
    return bound


@pytest.fixture(scope="module")
def ragged_cases():
    """inputs, float64 specification and per-output bound of every case: computed once, shared, never modified.  stride 12348: rows on 16-byte
    boundaries (the kernel's float4 span loads); 12347: the scalar loads"""
    cases = {}
    for kind in ("noise", "tone"):
        for channels in (1, 2):
            for stride in (12348, 12347):
                x = _signal(kind, channels, stride)
                ref, ref_l = pp().resample_reference(x, RATES3, LENGTHS3)
                bound = derived_bound(x, RATES3, LENGTHS3, ref_l, ref.shape[1])
                cases[(kind, channels, stride)] = dict(x=x, ref=ref, ref_l=ref_l, bound=bound)
    return cases


@pytest.mark.parametrize("stride", [12348, 12347])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("kind", ["noise", "tone"])
def test_kernel_against_the_float64_specification(ragged_cases, kind, channels, stride):
    from tests.helpers import record_margin
    c = ragged_cases[(kind, channels, stride)]
    got, got_l = run_guarded(dev(c["x"] if channels > 1 else c["x"][:, 0]), RATES3, LENGTHS3)
    assert got_l.tolist() == c["ref_l"].tolist() == [out_len(ln, r) for ln, r in zip(LENGTHS3, RATES3)]
    assert got.shape == c["ref"].shape == (3, 2 * stride)                     # the 8 kHz clip's row decides
    g64 = got.double().cpu().numpy()
    worst = {}
    for b, rate in enumerate(RATES3):
        m = int(c["ref_l"][b])
        assert not g64[b, m:].any(), ("tail", b)
        err = np.abs(g64[b, :m] - c["ref"][b, :m])
        assert (c["bound"][b, :m] > 0).all()
        worst[rate] = (float((err / c["bound"][b, :m]).max()), float(err.max()), float(c["bound"][b, :m].max()))
        print(f"resample vs float64 ({kind}, C = {channels}, stride {stride}, {rate} Hz): max error {worst[rate][1]:.3e}, largest bound {worst[rate][2]:.3e}, "
              f"worst error / bound {worst[rate][0]:.3f}")
        record_margin(f"resample.kernel_vs_float64.{kind}_c{channels}_stride{stride}_{rate}", ratio=worst[rate][0], max_err=worst[rate][1], max_bound=worst[rate][2])
    assert all(w[0] <= 1.0 for w in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. ragged equals alone, short clips, pass-through, determinism
@pytest.mark.parametrize("channels", [1, 2])
def test_ragged_equals_alone(ragged_cases, channels):
    c = ragged_cases[("noise", channels, 12348)]
    x = dev(c["x"] if channels > 1 else c["x"][:, 0])
    got, got_l = run_guarded(x, RATES3, LENGTHS3)
    for b, (rate, ln) in enumerate(zip(RATES3, LENGTHS3)):
        one, one_l = run_guarded(x[b:b + 1].contiguous(), rate, [ln])
        m = out_len(ln, rate)
        assert one_l.tolist() == [m] and int(got_l[b]) == m
        assert same_bits(one[0, :m], got[b, :m]), b
        assert not bool(one[0, m:].any()) and not bool(got[b, m:].any()), b
        # the same clip in a buffer cut to its length: what lies beyond the length is never read
        cut, cut_l = run_guarded(x[b:b + 1, ..., :ln].contiguous(), rate)
        assert cut_l.tolist() == [m] and same_bits(cut[0, :m], got[b, :m]), b
    # device-side lengths are taken at their word and cut to the stride
    dl, dl_l = run_guarded(x, RATES3, torch.tensor([4001, 99999, -5], dtype=torch.int32, device=DEV))
    assert dl_l.tolist() == [out_len(4001, 44100), out_len(12348, 48000), 0] and same_bits(dl[0], got[0]) and not bool(dl[2].any())


@pytest.mark.parametrize("length", [1, 5])
def test_clips_shorter_than_every_filter(length):
    rates = [44100, 48000, 8000, 11025, 16000]
    x = (np.random.default_rng(length).standard_normal((5, 2, 8)) * 0.1).astype(np.float32)
    want, want_l = pp().resample_reference(x, rates, [length] * 5)
    got, got_l = run_guarded(dev(x), rates, [length] * 5)
    assert got_l.tolist() == want_l.tolist() == [out_len(length, r) for r in rates] and got.shape == want.shape
    assert (np.abs(got.double().cpu().numpy() - want) <= derived_bound(x, rates, [length] * 5, want_l, want.shape[1])).all()
    for b in range(5):
        assert not bool(got[b, int(want_l[b]):].any())


def test_pass_through():
    rng = np.random.default_rng(7)
    x1 = (rng.standard_normal((2, 3001)) * 0.1).astype(np.float32)
    x1[0, :4] = [-0.0, 0.0, np.float32(1e-40), -1.0]            # the bytes, a negative zero and a subnormal included
    got, got_l = run_guarded(dev(x1), 16000, [3001, 2000])
    assert got_l.tolist() == [3001, 2000] and got.shape == (2, 3001)
    assert same_bits(got[0], dev(x1)[0]) and same_bits(got[1, :2000], dev(x1)[1, :2000]) and not bool(got[1, 2000:].any())
    x3 = (rng.standard_normal((2, 3, 3001)) * 0.1).astype(np.float32)
    got3, _ = run_guarded(dev(x3), [16000, 16000])
    want3 = ((x3[:, 0] + x3[:, 1]) + x3[:, 2]) / np.float32(3.0)
    assert want3.dtype == np.float32 and same_bits(got3, dev(want3))
    # a pass-through clip beside a 44.1 kHz one: each is what it is alone
    mixed, mixed_l = run_guarded(dev(x3), [16000, 44100], [3001, 3001])
    alone, _ = run_guarded(dev(x3[1:]), 44100)
    m = out_len(3001, 44100)
    assert mixed_l.tolist() == [3001, m] and mixed.shape == (2, 3001)
    assert same_bits(mixed[0], dev(want3)[0]) and same_bits(mixed[1, :m], alone[0]) and not bool(mixed[1, m:].any())


def test_two_calls_give_the_same_bytes(ragged_cases):
    x = dev(ragged_cases[("tone", 2, 12348)]["x"])
    a, al = ops().resample_wave(x, RATES3, LENGTHS3)
    b, bl = ops().resample_wave(x, RATES3, LENGTHS3)
    assert same_bits(a, b) and torch.equal(al, bl) and a.data_ptr() != b.data_ptr()


def test_the_ten_rates():
    """every promised rate into 16 kHz: a 1 kHz sine comes out as the 16 kHz sine (the row sum of the table, 1.00004 - 1.0009, and the
    transition at the ends aside)"""
    rates = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000]
    for group in (rates[:8], rates[8:]):
        lengths = [r // 4 for r in group]                       # 0.25 s each
        stride = max(lengths)
        x = np.zeros((len(group), stride), dtype=np.float32)
        for b, (r, ln) in enumerate(zip(group, lengths)):
            x[b, :ln] = np.sin(2 * np.pi * 1000.0 * np.arange(ln) / r)
        got, got_l = run_guarded(dev(x), group, lengths)
        assert got_l.tolist() == [4000] * len(group)
        want = np.sin(2 * np.pi * 1000.0 * np.arange(4000) / 16000.0)
        err = np.abs(got[:, :4000].double().cpu().numpy() - want[None])[:, 100:-100].max(axis=1)
        print("1 kHz sine into 16 kHz:", dict(zip(group, err.round(6).tolist())))
        assert (err <= 2e-3).all(), dict(zip(group, err.tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
def test_wrapper_refusals():
    from avsiam_amd._lib import AvsiamHipError
    o = ops()
    x = dev(np.zeros((2, 2, 64), dtype=np.float32))
    for bad in (44100.0, 0, -8000, "44100", None, True):
        with pytest.raises(ValueError):
            o.resample_wave(x, bad)
    with pytest.raises(ValueError):
        o.resample_wave(x, [44100, 0])
    with pytest.raises(ValueError):
        o.resample_wave(x, 44100, new_freq=0)
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, [44100])                                                                  # one rate for two clips
    with pytest.raises(AvsiamHipError):
        o.resample_wave(dev(np.zeros((9, 64), dtype=np.float32)), [11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000])      # nine distinct rates
    o.resample_wave(dev(np.zeros((9, 64), dtype=np.float32)), [16000, 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000])  # eight and a pass-through: accepted
    with pytest.raises(AvsiamHipError):
        o.resample_wave(dev(np.zeros((1, 9, 64), dtype=np.float32)), 44100)                          # nine channels
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, 16001)                                                                    # 16 000 phases: over the table cap
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, 44100, new_freq=16001)
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, 768000)                                                                   # o = 48: the span of a tile is over the cap
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x.double(), 44100)
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x.cpu(), 44100)
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x[..., ::2], 44100)                                                          # not contiguous
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x[0, 0], 44100)                                                              # one dimension
    with pytest.raises(ValueError):
        o.resample_wave(x, 44100, [65, 1])                                                           # beyond the stride
    with pytest.raises(ValueError):
        o.resample_wave(x, 44100, [-1, 1])
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, 44100, [1, 2, 3])
    with pytest.raises(AvsiamHipError):
        o.resample_wave(x, 44100, torch.tensor([1, 2], device=DEV))                                  # int64 lengths on the device
    m = out_len(64, 44100)
    for bad in (torch.empty((2, m + 1), device=DEV), torch.empty((2, m), device=DEV, dtype=torch.float64), torch.empty((2, m)), torch.empty((3, m), device=DEV)):
        with pytest.raises(AvsiamHipError):
            o.resample_wave(x, 44100, out=bad)
    for bad in (torch.empty(3, device=DEV, dtype=torch.int32), torch.empty(2, device=DEV, dtype=torch.int64), torch.empty(2, dtype=torch.int32)):
        with pytest.raises(AvsiamHipError):
            o.resample_wave(x, 44100, out_lengths=bad)
    got, got_l = o.resample_wave(x, 44100, out=torch.empty((2, m), device=DEV))
    assert got.shape == (2, m) and got_l.tolist() == [m, m] and not bool(got.any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. into the fbank
MEAN, STD = -5.081, 4.4849
FLT_EPSILON = np.float64(np.float32(1.1920929e-07))
FB_RATES, FB_LENGTHS = [44100, 48000], [52920, 57001]          # 1.2 s and 1.19 s, stereo; down-sampling only: an 8 kHz source leaves the upper mel
#                                                                bins at stop-band level, and the log measure would exclude nearly all of them
# 3 x the measured maxima of ops.kaldi_fbank(*ops.resample_wave(x)) against the float64 chain (profiles/r17/resample_margins.json: energy 5.4e-7
# noise / 1.09e-6 tone, log 5.4e-5); the same chain in numpy float32 on the CPU gets 3.6e-7 / 3.8e-7 and 5.1e-5 and excludes 1.5 % of the cells
# (the float64 chain alone excludes them: the share does not depend on the kernel)
CHAIN_ENERGY_BOUND, CHAIN_LOG_BOUND = 3.3e-6, 1.6e-4
EXCLUDED_MAX = 0.03


def chain_errors(out, ref_e, frames):
    """the two measures of tests/test_frontend_gpu.py over every clip's own frame rows -> (energy error, log error, largest excluded share)"""
    out = np.asarray(out, dtype=np.float64)
    energy, log, excluded = 0.0, 0.0, 0.0
    for b, m in enumerate(frames):
        o, e64 = out[b, :m], ref_e[b, :m]
        row_max = e64.max(axis=1, keepdims=True)
        energy = max(energy, float((np.abs(np.exp(o) - np.maximum(e64, FLT_EPSILON)) / row_max).max()))
        keep = e64 >= 1e-6 * row_max
        log = max(log, float(np.abs(o - np.log(np.where(keep, e64, 1.0)))[keep].max()))
        excluded = max(excluded, float(1.0 - keep.mean()))
    return energy, log, excluded


@pytest.fixture(scope="module")
def chain_inputs():
    rng = np.random.default_rng(20241017)
    S = max(FB_LENGTHS) + 3
    noise = (rng.standard_normal((2, 2, S)) * 0.1).astype(np.float32)
    t = np.arange(S)[None, None, :] / np.asarray(FB_RATES, dtype=np.float64)[:, None, None]
    tone = (noise + 0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    cases = {}
    for name, x in (("noise", noise), ("tone", tone)):
        r64, ol = pp().resample_reference(x, FB_RATES, FB_LENGTHS)
        frames = [pp().fbank_frames(n) for n in ol]
        ref, energy = pp().kaldi_fbank_reference(r64, ol, target_length=max(frames), return_energy=True)
        cases[name] = dict(x=x, ref=ref, energy=energy, frames=frames, lengths=ol)
    return cases


def test_fbank_of_the_resampled_audio(chain_inputs):
    from tests.helpers import record_margin
    margins = {}
    for name, c in chain_inputs.items():
        wave, lengths = ops().resample_wave(dev(c["x"]), FB_RATES, FB_LENGTHS)
        assert lengths.tolist() == c["lengths"].tolist()
        out = ops().kaldi_fbank(wave, lengths, target_length=max(c["frames"])).cpu().numpy()
        for b, m in enumerate(c["frames"]):
            assert not out[b, m:].any(), ("pad rows", b)
        energy, log, excluded = chain_errors(out, c["energy"], c["frames"])
        margins[name] = {"kernel_energy": energy, "kernel_log": log, "excluded_share": excluded}
        print(f"resample + fbank vs the float64 chain ({name}): energy {energy:.3e}, log {log:.3e}, excluded {excluded:.4f}")
        record_margin(f"resample.fbank_chain_vs_f64.{name}", **margins[name], bound_energy=CHAIN_ENERGY_BOUND, bound_log=CHAIN_LOG_BOUND)
    for name, m in margins.items():
        assert m["kernel_energy"] <= CHAIN_ENERGY_BOUND, (name, m)
        if name != "tone":                                      # the tone concentrates a row's energy in a few filters: energy measure only
            assert m["excluded_share"] <= EXCLUDED_MAX, (name, m)
            assert m["kernel_log"] <= CHAIN_LOG_BOUND, (name, m)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. loader and launcher
CFG = AVSiamConfig(depth=2)
LBL = 7


def test_wave_loader_with_a_sample_rate():
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    kw = dict(seed=87, mixup=0.5, norm=(MEAN, STD), samples=8000)
    tr = SyntheticWaveFtLoader(CFG, 3, 2, LBL, DEV, sample_rate=[44100, 48000], channels=2, **kw)
    assert tr.wave.shape == (3, 2, 24000) and tr.wave.dtype == torch.float32
    for a, v, y in tr:
        d = tr.last_draw
        assert a.shape == (3, CFG.audio_len, 128) and bool(torch.isfinite(a).all()) and y.shape == (3, LBL)
        w1, l1 = ops().resample_wave(tr.wave, tr.rates, d["src_lengths"])
        w2, l2 = ops().resample_wave(tr.wave2, tr.rates2, d["partner_src_lengths"])
        assert l1.tolist() == [out_len(n, r) for n, r in zip(d["src_lengths"], tr.rates)]
        want = ops().kaldi_fbank(w1, l1, partner=w2, partner_lengths=l2, lam=d["lam"], target_length=CFG.audio_len, norm=(MEAN, STD))
        assert same_bits(a, want)
    va = SyntheticWaveFtLoader(CFG, 2, 1, LBL, DEV, seed=88, mixup=0.5, train=False, samples=8000, sample_rate=16000, channels=2, norm=(MEAN, STD))
    (a, v, y), = list(va)
    mean = (va.wave[:, 0] + va.wave[:, 1]) / 2.0
    assert same_bits(a, ops().kaldi_fbank(mean, va.last_draw["src_lengths"], target_length=CFG.audio_len, norm=(MEAN, STD)))
    # sample_rate=None: the loader's bytes and draws of before
    old = SyntheticWaveFtLoader(CFG, 3, 2, LBL, DEV, **kw)
    new = SyntheticWaveFtLoader(CFG, 3, 2, LBL, DEV, sample_rate=None, channels=1, **kw)
    for (a0, v0, y0), (a1, v1, y1) in zip(old, new):
        assert same_bits(a0, a1) and same_bits(v0, v1) and same_bits(y0, y1) and "src_lengths" not in new.last_draw
        assert all(np.array_equal(old.last_draw[k], new.last_draw[k]) for k in old.last_draw)


def test_launcher_with_a_sample_rate(tmp_path, capsys, monkeypatch):
    """--wave-input --sample-rate 44100 48000 --audio-channels 2 --mixup 0.5 on a depth-2 model at batch 3: one epoch and its validation finish
    with finite, recorded losses"""
    import avsiam_amd.config as config
    import avsiam_amd.models as models
    import avsiam_amd.run_cavmae_ft_base as launcher
    monkeypatch.setattr(config, "AVSiamConfig", lambda: CFG)
    monkeypatch.setattr(models, "CAVMAEFT_BASE", lambda label_dim: models.cav_mae_ft.CAVMAEFT_BASE(label_dim, cfg=CFG, init_seed=6, init_mode="random"))
    exp = tmp_path / "ft"
    out = launcher.main(["--ftmode", "mm_grad", "--n_class", "527", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "3", "--n_epochs", "1",
                         "--exp_dir", str(exp), "--steps-per-epoch", "3", "--val-steps", "1", "--label_smooth", "0.1", "--wave-input", "--sample-rate", "44100",
                         "48000", "--audio-channels", "2", "--mixup", "0.5"])
    said = capsys.readouterr().out
    assert "not implemented" not in said
    res = np.loadtxt(exp / "result.csv", delimiter=",").reshape(-1, 4)
    assert res.shape == (1, 4) and np.all(np.isfinite(res)), res
    assert "valid loss" in said and "nan" not in said.split("valid loss")[1].split()[0]
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3])


# the digest of one plain fine-tuning step on the parent commit (tools/step_digest.py --ft --trace --batch 3, profiles/r14/frames_bench.json)
PARENT_DIGEST = {"trace_calls": 303, "trace": "21a456a12665402bb61ad36021b881415531210137bfe83da2f626bd146a239a", "calls_per_step": [301],
                 "p": "57f087e095055fa51785f681a6cb583fc4ce92b4c8bd85342575a3445db100b9", "g": "8717c34280ebc640d3e247807d9c6eec5f13a0d6188b234c2c9c323538cd2c46",
                 "adam_m": "887c7d3accf9731d8b7c0ad334b807b47c7b4a7ac999d026edbddab608d08406", "adam_v": "5c9624b28e55299fdb1dfa8a9d0b9526bcf2c182c6e0aa736b211926c9010abb"}


def test_plain_step_is_the_parents():
    """without the new flags nothing moved: the library-call list of a plain step (entry points, scalar arguments, tensor shapes) and the arenas
    after it hash to what the parent commit gives"""
    r = subprocess.run([sys.executable, os.path.join("tools", "step_digest.py"), "--ft", "--trace", "--batch", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print("step digest:", {k: got[k] for k in PARENT_DIGEST})
    assert {k: got[k] for k in PARENT_DIGEST} == PARENT_DIGEST
