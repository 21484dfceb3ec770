"""Source-rate audio without a device: the definition of the resampler (preprocess.resample_table_reference / resample_reference), the compact
table the kernel reads, the launch geometry of the ten rates the project promises, and the launcher's refusals.

Nothing here was recorded from torchaudio (it was never available): the table's shape and support figures below were computed from the
definition in the table function's docstring, and the index arithmetic is held to the literal torch chain (pad, conv1d at stride o,
transpose, reshape, cut) in float64."""
import ctypes
import math

import numpy as np
import pytest
import torch

from avsiam_amd import preprocess as pp

# rate -> (width, non-zero taps of the widest phase), into 16 kHz
SHAPES = {44100: (17, 34), 48000: (19, 37), 22050: (9, 17), 32000: (13, 25), 8000: (7, 13), 11025: (7, 13)}
TEN_RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000]


@pytest.mark.parametrize("rate", sorted(SHAPES))
def test_table_shape_and_support(rate):
    width, taps = SHAPES[rate]
    table, w = pp.resample_table_reference(rate, 16000)
    g = math.gcd(rate, 16000)
    o, n = rate // g, 16000 // g
    assert w == width and table.dtype == torch.float32 and tuple(table.shape) == (n, 1, 2 * width + o)
    t = table[:, 0].numpy()
    nz = t != 0
    assert int(nz.sum(axis=1).max()) == taps
    for p in range(n):                                          # one contiguous run per phase
        idx = np.flatnonzero(nz[p])
        assert len(idx) > 0 and idx[-1] - idx[0] + 1 == len(idx), p
    sums = t.astype(np.float64).sum(axis=1)
    assert 1.00003 <= sums.min() and sums.max() <= 1.0009, (sums.min(), sums.max())


def test_phase_term_is_float32():
    """torch divides an int64 arange by an int in float32: the table function's own phase term has that dtype, and a float64 phase gives
    another table"""
    assert pp._resample_phase(160).dtype == torch.float32
    assert torch.equal(pp._resample_phase(160), torch.arange(0, -160, -1)[:, None, None] / 160)
    table, width = pp.resample_table_reference(44100, 16000)
    o, n, base = 441, 160, 160 * 0.99
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = (t * base).clamp(-6, 6)
    k64 = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), torch.sin(t * math.pi) / (t * math.pi)) * torch.cos(t * math.pi / 12) ** 2 * (base / o)
    diff = float((table.double() - k64).abs().max())
    assert 0 < diff < 4e-6, diff                                 # 1.9e-6 measured


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 8000])
def test_index_arithmetic_against_the_torch_chain(rate):
    L = 1000
    x = np.random.default_rng(rate).standard_normal(L)
    table, width = pp.resample_table_reference(rate, 16000)
    g = math.gcd(rate, 16000)
    o, n = rate // g, 16000 // g
    xt = torch.from_numpy(x)[None, None]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xt, (width, width + o)), table.double(), stride=o)
    y = y.transpose(1, 2).reshape(1, -1)[0, :math.ceil(n * L / o)].numpy()
    got, lengths = pp.resample_reference(x[None], rate)
    assert lengths.tolist() == [len(y)] and got.shape == (1, len(y)) and got.dtype == np.float64
    err = float(np.abs(got[0] - y).max())
    print(f"resample_reference vs pad/conv1d/reshape at {rate}: {err:.2e}")
    assert err <= 1e-13


def test_it_is_a_resampler():
    t = np.arange(44100) / 44100.0
    got, lengths = pp.resample_reference(np.sin(2 * np.pi * 1000.0 * t)[None], 44100)
    assert lengths.tolist() == [16000] and got.shape == (1, 16000)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(16000) / 16000.0)
    err = float(np.abs(got[0] - want)[100:-100].max())
    print(f"1 kHz sine, 44.1 -> 16 kHz: {err:.2e}")
    assert err <= 1e-3


def test_channels_ragged_lengths_and_pass_through():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 2, 900))
    got, lengths = pp.resample_reference(x, [44100, 16000, 8000], [900, 700, 5])
    assert lengths.tolist() == [math.ceil(160 * 900 / 441), 700, 10] and got.shape == (3, 1800)
    assert np.array_equal(got[1, :700], x[1, :, :700].mean(axis=0)) and not got[1, 700:].any() and not got[2, 10:].any()
    a, _ = pp.resample_reference(x[0, 0][None], 44100)
    b, _ = pp.resample_reference(x[0, 1][None], 44100)
    assert np.abs(got[0, :lengths[0]] - 0.5 * (a[0] + b[0])).max() <= 1e-15
    assert pp.resample_out_length(2 ** 31 - 1, 8000, 16000) == 2 ** 32 - 2        # exact integers, no 32-bit product
    for bad in (0, -1, 44100.0, True):
        with pytest.raises(ValueError):
            pp.resample_table_reference(bad, 16000)
    with pytest.raises(ValueError):
        pp.resample_reference(x, [44100, 16000], None)
    with pytest.raises(ValueError):
        pp.resample_reference(x, 44100, [901, 1, 1])


@pytest.mark.parametrize("rate", TEN_RATES)
def test_compaction_and_launch_geometry(rate):
    """re-expanding the compact table gives the dense table exactly; first + K stays inside the row; the compact table and the span of a
    1024-output tile are inside the kernel's caps (avs_resample_plan: host arithmetic of the library, no device)"""
    from avsiam_amd import _lib
    table, width = pp.resample_table_reference(rate, 16000)
    first, weights = pp.resample_compact_table(table)
    n, L = table.shape[0], table.shape[2]
    K = weights.shape[1]
    assert first.dtype == np.int32 and weights.dtype == np.float32 and weights.shape == (n, K)
    assert first.min() >= 0 and int((first + K).max()) <= L
    assert np.array_equal(pp.resample_expand_table(first, weights, L), table[:, 0].numpy())            # (a dense -0 outside the run comes back as 0)
    if rate in SHAPES:
        assert K == SHAPES[rate][1]
    tw, sw = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("avs_resample_plan", L - 2 * width, n, width, K, ctypes.cast(ctypes.byref(tw), ctypes.c_void_p), ctypes.cast(ctypes.byref(sw), ctypes.c_void_p))
    assert tw.value == n * ((K | 1) + 1) <= pp.RESAMPLE_MAX_WORDS and 0 < sw.value <= 16384, (tw.value, sw.value)


def test_compaction_refuses_a_split_run():
    t = np.zeros((2, 9), dtype=np.float32)
    t[0, 2:5] = 1.0
    t[1, [1, 3]] = 1.0
    with pytest.raises(ValueError):
        pp.resample_compact_table(t)
    first, w = pp.resample_compact_table(t[:1])
    assert first.tolist() == [2] and w.tolist() == [[1.0, 1.0, 1.0]]
    t[1] = 0
    t[1, 7:] = 1.0                                               # a short run at the row's end: first moves down, zeros lead
    first, w = pp.resample_compact_table(t)
    assert first.tolist() == [2, 6] and w[1].tolist() == [0.0, 1.0, 1.0]


BASE = ["--ftmode", "mm_grad", "--n_class", "527", "--batch_size", "2", "--n_epochs", "1"]


@pytest.mark.parametrize("extra, said", [
    (["--sample-rate", "44100"], "--wave-input"),
    (["--audio-channels", "2"], "--wave-input"),
    (["--raw-input", "--sample-rate", "44100", "--audio-channels", "2"], "--wave-input"),
    (["--wave-input", "--audio-channels", "2"], "--sample-rate"),
    (["--wave-input", "--sample-rate", "0"], "--sample-rate 0"),
    (["--wave-input", "--sample-rate", "44100", "--audio-channels", "9"], "--audio-channels 9"),
    (["--wave-input", "--sample-rate"] + [str(8000 + i) for i in range(9)], "8 distinct"),
])
def test_launcher_refusals(extra, said):
    from avsiam_amd.run_cavmae_ft_base import main
    with pytest.raises(SystemExit) as e:
        main(BASE + extra)
    assert said in str(e.value), e.value


def test_loader_arguments_need_no_device():
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    cfg = AVSiamConfig(depth=2)
    with pytest.raises(ValueError):
        SyntheticWaveFtLoader(cfg, 2, 1, 5, "cpu", samples=800, channels=2)
    with pytest.raises(ValueError):
        SyntheticWaveFtLoader(cfg, 2, 1, 5, "cpu", samples=800, sample_rate=[44100, 0])
    ld = SyntheticWaveFtLoader(cfg, 3, 1, 5, "cpu", samples=800, sample_rate=[44100, 48000], channels=2, mixup=0.5)
    assert ld.rates == [44100, 48000, 44100] and ld.rates2 == [44100, 44100, 48000] and ld.wave.shape == (3, 2, 2400) and ld.wave2.shape == ld.wave.shape
    d = ld.draw()
    assert d["src_lengths"].tolist() == [int(l) * r // 16000 for l, r in zip(d["lengths"], ld.rates)]
    assert d["partner_src_lengths"].tolist() == [int(l) * r // 16000 for l, r in zip(d["partner_lengths"], ld.rates2)]
    # sample_rate=None: the buffers and draws of before
    old, new = (SyntheticWaveFtLoader(cfg, 3, 1, 5, "cpu", samples=800, mixup=0.5, **kw) for kw in ({}, dict(sample_rate=None, channels=1)))
    assert torch.equal(old.wave, new.wave) and torch.equal(old.v, new.v) and new.rates is None
    assert torch.equal(old.v, ld.v) and torch.equal(old.hot, ld.hot)                  # frames and labels do not depend on the audio's rate
    d0, d1 = old.draw(), new.draw()
    assert sorted(d0) == sorted(d1) and all(np.array_equal(d0[k], d1[k]) for k in d0) and "src_lengths" not in d1
