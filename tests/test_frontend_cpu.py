"""Waveform input, the parts that need no GPU: the float64 specification of the Kaldi fbank (preprocess.kaldi_fbank_reference - restated
from the Kaldi definition; torchaudio was never available to record from), the label mixing, the launcher's --wave-input flag, the new
C-ABI symbols and the host tables of the kernel against the specification's."""
import ctypes
import types

import numpy as np
import pytest
import torch

from avsiam_amd import _lib
from avsiam_amd import preprocess as pp

FLOOR = np.float32(np.log(np.float64(np.float32(1.1920929e-07))))


def _noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape) * 0.1


@pytest.mark.parametrize("n, m", [(400, 1), (559, 1), (560, 2)])
def test_frame_count(n, m):
    assert pp.fbank_frames(n) == m
    out = pp.kaldi_fbank_reference(_noise(n, 1, n), target_length=4)
    assert out.shape == (1, 4, 128) and out.dtype == np.float64
    assert np.all(out[0, :m, 0] != 0) and np.all(out[0, m:] == 0)
    # trailing samples beyond the last whole frame are ignored (they move the clip mean only, which the frame mean removes again)
    x = _noise(7, 1, 560)
    live = np.arange(128) != 3
    a = pp.kaldi_fbank_reference(x, lengths=[559], target_length=2)[0, 0]
    assert np.abs(a - pp.kaldi_fbank_reference(x[:, :400], target_length=2)[0, 0])[live].max() <= 1e-9


def test_short_clip_is_refused():
    with pytest.raises(ValueError):
        pp.kaldi_fbank_reference(_noise(0, 1, 399))
    with pytest.raises(ValueError):
        pp.kaldi_fbank_reference(_noise(0, 2, 1000), lengths=[1000, 399])


def test_empty_filter_and_constant_clip_give_the_floor():
    w = pp.fbank_mel_weights()
    count = (w > 0).sum(axis=1)
    assert count[3] == 0 and (np.delete(count, 3) > 0).all() and count.max() == 10      # filter 3 holds no FFT bin; no filter is wider than 10 bins
    assert (w > 0).sum(axis=0).max() == 2 and not w[:, 256].any()                      # a bin feeds at most two filters; Nyquist has weight 0
    out = pp.kaldi_fbank_reference(_noise(3, 2, 2000), target_length=11)
    assert np.all(out[:, :11, 3].astype(np.float32) == FLOOR) and pp.FBANK_FLOOR == FLOOR
    assert abs(float(FLOOR) + 15.942385) < 1e-6
    const = pp.kaldi_fbank_reference(np.full((1, 1500), 0.25), target_length=7)
    assert np.all(const.astype(np.float32) == FLOOR)                                    # m = 7: every row a frame, every cell the floor
    const32 = pp.kaldi_fbank_reference(np.full((1, 1500), 0.25, dtype=np.float32), target_length=9, dtype=np.float32)
    assert const32.dtype == np.float32 and np.all(const32[0, :7] == FLOOR) and np.all(const32[0, 7:] == 0)


def test_a_constant_offset_changes_nothing():
    x = _noise(11, 2, 3000)
    a, ea = pp.kaldi_fbank_reference(x, target_length=18, return_energy=True)
    b, eb = pp.kaldi_fbank_reference(x + 0.37, target_length=18, return_energy=True)
    assert np.abs(ea - eb).max() <= 1e-12 * ea.max()
    live = ea > 1e-9
    assert np.abs(a - b)[live].max() <= 1e-9


@pytest.mark.parametrize("n2", [2500, 1700, 3100], ids=["equal", "pad", "cut"])
def test_mixed_path_equals_the_plain_path_on_a_hand_mixed_waveform(n2):
    n1, lam = 2500, 0.43
    w1, w2 = _noise(21, n1), _noise(22, 3200)
    a = w1 - w1.mean()
    c = w2[:n2] - w2[:n2].mean()                               # the partner's mean over ITS length, before padding / cutting
    cc = np.zeros(n1)
    cc[:min(n1, n2)] = c[:n1]
    mix = lam * a + (1 - lam) * cc
    want = pp.kaldi_fbank_reference(mix[None], target_length=16)
    wave = np.zeros((1, 2600))
    wave[0, :n1] = w1
    wave[0, n1:] = 50.0                                        # beyond the length: never read
    got = pp.kaldi_fbank_reference(wave, lengths=[n1], partner=w2[None], partner_lengths=[n2], lam=[lam], target_length=16)
    assert np.abs(got - want).max() <= 1e-9
    if n2 < n1:
        # the order matters at the seam: padding BEFORE the partner's mean is subtracted is another waveform
        wrong = np.zeros(n1)
        wrong[:n2] = w2[:n2]
        wrong = wrong - wrong.mean()
        other = pp.kaldi_fbank_reference((lam * a + (1 - lam) * wrong)[None], target_length=16)
        assert np.abs(other - want).max() > 1e-3


def test_negative_lam_and_no_partner_agree():
    x, y = _noise(31, 3, 2000), _noise(32, 3, 1800)
    plain = pp.kaldi_fbank_reference(x, lengths=[2000, 1500, 400], target_length=12)
    got = pp.kaldi_fbank_reference(x, lengths=[2000, 1500, 400], partner=y, lam=[-1.0, 0.3, -1.0], target_length=12)
    assert np.array_equal(got[[0, 2]], plain[[0, 2]]) and not np.array_equal(got[1], plain[1])
    assert np.array_equal(pp.kaldi_fbank_reference(x, partner=y, lam=None, target_length=12), pp.kaldi_fbank_reference(x, target_length=12))
    # lam = 1 keeps the clip (up to the rounding of a - mean(a)); lam = 0 is the partner, cut to the clip's length
    one = pp.kaldi_fbank_reference(x, partner=y, lam=[1.0] * 3, target_length=12)
    assert np.abs(one - pp.kaldi_fbank_reference(x, target_length=12)).max() <= 1e-9


def test_norm_turns_pad_rows_into_the_normalised_zero():
    mean, std = -5.081, 4.4849
    x = _noise(41, 1, 1000)                                    # 4 frames
    raw = pp.kaldi_fbank_reference(x, target_length=6)
    out = pp.kaldi_fbank_reference(x, target_length=6, norm=(mean, std))
    assert np.all(out[0, 4:] == (0.0 - mean) / std) and np.allclose(out[0, :4], (raw[0, :4] - mean) / std, rtol=0, atol=1e-12)
    cut = pp.kaldi_fbank_reference(x, target_length=3)
    assert np.array_equal(cut[0], raw[0, :3])                  # frames beyond target_length are cut


def test_mixup_labels_against_the_loops_of_the_reference():
    C, s = 12, 0.1
    set1, set2, lam = [1, 4, 7], [4, 9], 0.37                  # two label sets that overlap in class 4
    want = np.zeros(C) + (s / C)                               # dataloader_ft.py:470-475, literally
    for k in set1:
        want[k] += lam * (1.0 - s)
    for k in set2:
        want[k] += (1.0 - lam) * (1.0 - s)
    plain = np.zeros(C) + (s / C)                              # :480, :524
    for k in set1:
        plain[k] = 1.0 - s
    h1, h2 = torch.zeros(2, C), torch.zeros(2, C)
    h1[:, set1] = 1.0
    h2[:, set2] = 1.0
    got = pp.mixup_labels(h1, h2, torch.tensor([lam, -1.0]), s)
    assert got.dtype == torch.float32 and got.shape == (2, C)
    assert np.abs(got[0].double().numpy() - want).max() <= 1e-7 and np.abs(got[1].double().numpy() - plain).max() <= 1e-7
    assert abs(float(got[0, 4]) - (s / C + (1 - s))) <= 1e-6    # in both sets: lam + (1 - lam)
    assert torch.equal(pp.mixup_labels(h1, None, -1.0, s), got[1:].expand(2, C))


def test_launcher_wave_input_flag():
    from avsiam_amd.run_cavmae_ft_base import MIXUP_REASON, build_parser, inert_flag_warnings, main
    p = build_parser()
    assert p.parse_args([]).wave_input is False
    args = p.parse_args(["--wave-input", "--mixup", "0.5", "--freqm", "48", "--timem", "192", "--noise", "True"])
    assert args.wave_input is True and args.mixup == 0.5
    assert inert_flag_warnings(args) == []                      # mixup is live here
    warn = inert_flag_warnings(p.parse_args(["--wave-input", "--mixup", "0.5", "--wa", "True"]))
    assert len(warn) == 1 and "--wa True" in warn[0] and "mixup" not in warn[0]
    # without the flag: today's two lines, word for word; a namespace that does not know the flag sees the same
    old = ["WARNING: not implemented on this path, ignored: --mixup 0.5 - this run trains without them", "WARNING: " + MIXUP_REASON]
    assert inert_flag_warnings(p.parse_args(["--mixup", "0.5"])) == old
    assert inert_flag_warnings(types.SimpleNamespace(mixup=0.5, wa=False, bal=None)) == old
    assert inert_flag_warnings(types.SimpleNamespace(mixup=0, wa=False, bal=None)) == []
    assert "dataloader_ft.py:321-325" in MIXUP_REASON
    with pytest.raises(SystemExit, match="--wave-input and --raw-input"):
        main(["--ftmode", "mm_grad", "--wave-input", "--raw-input"])


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def test_new_symbols_are_declared_and_exported(lib):
    protos = _lib.parse_header()
    for name in ("avs_wave_sums", "avs_kaldi_fbank", "avs_mix_frames_u8", "avs_fbank_tables"):
        assert name in protos and hasattr(lib, name), name
    assert protos["avs_kaldi_fbank"][1].count("ptr") == 8 and protos["avs_wave_sums"][1][-1] == "ptr"
    # argument validation precedes every launch: testable without a GPU
    one = ctypes.c_void_p(16)
    rc = lib.avs_kaldi_fbank(one, 1000, None, None, 0, None, None, one, 1, 8, 64, one, 0, 0.0, 1.0, None)
    assert rc == -2 and b"128 mel bins" in lib.avs_last_error()
    assert lib.avs_kaldi_fbank(one, 399, None, None, 0, None, None, one, 1, 8, 128, one, 0, 0.0, 1.0, None) == -2      # no clip can hold a frame
    assert lib.avs_kaldi_fbank(one, 1000, None, None, 0, None, one, one, 1, 8, 128, one, 0, 0.0, 1.0, None) == -2     # lam without a partner
    assert lib.avs_kaldi_fbank(one, 1000, None, None, 0, None, None, one, 1, 8, 128, one, 1, 0.0, 0.0, None) == -2    # zero std
    assert lib.avs_wave_sums(one, 1000, None, None, 0, one, 1, one, None) == -2                                       # lengths of no partner
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.avs_mix_frames_u8(one, one, one, one, 3, 2, 16, m3, m3, None) == -2                                    # 3 images, 2 per sample
    assert lib.avs_mix_frames_u8(one, one, one, one, 2, 1, 18, m3, m3, None) == -2                                    # plane % 4


def test_kernel_tables_are_the_specifications_rounded_once(lib):
    """twiddles, window and mel weights of the kernel (computed on the host in float64, rounded once) against numpy's float64 rounded once:
    the same first bin and width per filter, weights within one fp32 ulp (two libms), filter 3 empty"""
    W = 2960
    tab = np.zeros(W, dtype=np.float32)
    assert lib.avs_fbank_tables(tab.ctypes.data_as(ctypes.c_void_p), W) == 0
    assert lib.avs_fbank_tables(tab.ctypes.data_as(ctypes.c_void_p), W - 1) == -2
    k = np.arange(512)
    tw = tab[:1024].reshape(512, 2)
    assert np.abs(tw[:, 0] - np.cos(2 * np.pi * k / 512)).max() <= 6e-8 and np.abs(tw[:, 1] + np.sin(2 * np.pi * k / 512)).max() <= 6e-8
    i = np.arange(400)
    assert np.abs(tab[1024:1424] - (0.5 - 0.5 * np.cos(2 * np.pi * i / 399))).max() <= 6e-8
    melw, first, count = tab[1424:2704].reshape(128, 10), tab[2704:2832].view(np.int32), tab[2832:2960].view(np.int32)
    w = pp.fbank_mel_weights()
    for f in range(128):
        nz = np.nonzero(w[f])[0]
        assert count[f] == len(nz), f
        if len(nz):
            assert first[f] == nz[0] and nz[-1] - nz[0] + 1 == len(nz)
            want = w[f, nz].astype(np.float32)
            assert np.abs(melw[f, :len(nz)] - want).max() <= np.spacing(want.max()), f
        assert not melw[f, len(nz):].any()
    assert count[3] == 0 and (first + count).max() <= 256
