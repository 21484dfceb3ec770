"""Fine-tuning augmentation (SpecAugment masks, noise, time roll where the input is read), the parts that need no GPU: the numpy restatement
of the device's plan draw and its invariants, the C ABI surface (symbols, ABI version, bad arguments refused before any launch) and the
launcher's flags."""
import ctypes

import numpy as np
import pytest

from avsiam_amd import _lib
from avsiam_amd.preprocess import draw_plan_reference, noise_reference, philox4x32_10

T, F = 1024, 128


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def test_philox_restatement_matches_the_published_vectors():
    """Random123's known-answer vectors of philox4x32-10 (kat_vectors): first output word"""
    assert int(philox4x32_10(0, 0, 0, 0, 0, 0)[()]) == 0x6627E8D5
    assert int(philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)[()]) == 0x408F276D
    assert int(philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)[()]) == 0xD16CFE09


@pytest.mark.parametrize("freqm,timem", [(48, 192), (F, T), (1, 1)])
def test_draw_invariants(freqm, timem):
    """over 4096 samples x 2 draws: 0 <= n < max(param, 1), start + n <= size, -T <= shift < T, 0 <= amp < 0.1"""
    for counter in (0, 77):
        p = draw_plan_reference(0x0123456789ABCDEF, counter, 4096, T, F, freqm, timem, True)
        for start, n, param, size in ((p["f0"], p["fn"], freqm, F), (p["t0"], p["tn"], timem, T)):
            assert start.dtype == np.int32 and n.dtype == np.int32
            assert (n >= 0).all() and (n < max(param, 1)).all()
            assert (start >= 0).all() and (start.astype(np.int64) + n <= size).all()
            if param > 1:
                assert n.max() > param // 2 and len(np.unique(start)) > 8          # the draws do vary
        assert (p["shift"] >= -T).all() and (p["shift"] < T).all() and p["shift"].min() < 0 < p["shift"].max()
        assert p["amp"].dtype == np.float32 and (p["amp"] >= 0).all() and (p["amp"] < np.float32(0.1)).all() and p["amp"].max() > 0.09


def test_draw_switches_and_reproducibility():
    key = (1234 << 32) | 3
    p = draw_plan_reference(key, 5, 3000, T, F, 0, 0, False)
    for k in ("f0", "fn", "t0", "tn", "shift"):
        assert not p[k].any(), k
    assert not p["amp"].any()
    p = draw_plan_reference(key, 5, 3000, T, F, 0, 192, True)
    assert not p["fn"].any() and not p["f0"].any() and p["tn"].any() and p["shift"].any() and p["amp"].any()
    p = draw_plan_reference(key, 5, 3000, T, F, 48, 0, False)
    assert p["fn"].any() and not p["tn"].any() and not p["t0"].any() and not p["shift"].any() and not p["amp"].any()
    a, b, c = (draw_plan_reference(key, n, 64, T, F, 48, 192, True) for n in (5, 5, 6))
    for k in ("f0", "fn", "t0", "tn", "shift", "amp"):
        assert np.array_equal(a[k], b[k]), k
        assert not np.array_equal(a[k], c[k]), k
    assert a["noise_key"] == b["noise_key"] != c["noise_key"]
    d = draw_plan_reference(key + 1, 5, 64, T, F, 48, 192, True)           # the next rank's key
    assert not np.array_equal(a["fn"], d["fn"]) and a["noise_key"] != d["noise_key"]
    # a larger batch extends a smaller one: the draw of sample b does not depend on B
    e = draw_plan_reference(key, 5, 7, T, F, 48, 192, True)
    assert all(np.array_equal(a[k][:7], e[k]) for k in ("f0", "fn", "t0", "tn", "shift", "amp"))
    for bad in (dict(freqm=F + 1), dict(timem=T + 1), dict(freqm=-1), dict(B=0)):
        kw = dict(B=4, T=T, F=F, freqm=48, timem=192)
        kw.update(bad)
        with pytest.raises(ValueError):
            draw_plan_reference(key, 0, kw["B"], kw["T"], kw["F"], kw["freqm"], kw["timem"], True)


def test_span_formula_is_torchaudio_mask_along_axis():
    """n = floor(u1 * param), start = floor(u2 * (size - u1 * param)) with u = k / 2^24, in exact rational arithmetic"""
    from fractions import Fraction
    key, B = 99, 257
    p = draw_plan_reference(key, 3, B, T, F, 48, 192, True)
    b = np.arange(B)
    u = [(philox4x32_10(b, q, 3, 1, key & 0xFFFFFFFF, key >> 32) >> np.uint32(8)).astype(np.int64) for q in range(6)]
    for i in range(B):
        for (q, param, size, s, n) in ((0, 48, F, "f0", "fn"), (2, 192, T, "t0", "tn")):
            value = Fraction(int(u[q][i]), 1 << 24) * param
            lo = Fraction(int(u[q + 1][i]), 1 << 24) * (size - value)
            assert p[n][i] == value.numerator // value.denominator and p[s][i] == lo.numerator // lo.denominator
        sh = Fraction(int(u[4][i]), 1 << 24) * 2 * T
        assert p["shift"][i] == sh.numerator // sh.denominator - T


def test_noise_reference_is_a_uniform_field():
    u = noise_reference(0xDEADBEEF12345678, 2, 16, 32)
    assert u.shape == (2, 16, 32) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert 0.4 < u.mean() < 0.6 and not np.array_equal(u[0], u[1])


def test_symbols_and_abi_version(lib):
    protos = _lib.parse_header()
    for name, nargs in (("avs_ft_aug_draw", 9), ("avs_im2col_audio_aug", 15), ("avs_augment_audio", 11)):
        assert name in protos and len(protos[name][1]) == nargs and hasattr(lib, name), name
    assert lib.avs_abi_version() == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)                # any non-NULL values: every call must fail before touching them

    def rc(r, word):
        assert r == -2 and word in lib.avs_last_error(), (r, lib.avs_last_error())

    rc(lib.avs_ft_aug_draw(None, one, 4, T, F, 48, 192, 1, None), b"ft_aug_draw")
    rc(lib.avs_ft_aug_draw(one, None, 4, T, F, 48, 192, 1, None), b"ft_aug_draw")
    rc(lib.avs_ft_aug_draw(one, two, 0, T, F, 48, 192, 1, None), b"ft_aug_draw")
    rc(lib.avs_ft_aug_draw(one, two, 4, T, F, F + 1, 192, 1, None), b"freqm")
    rc(lib.avs_ft_aug_draw(one, two, 4, T, F, 48, T + 1, 1, None), b"timem")
    rc(lib.avs_ft_aug_draw(one, two, 4, T, F, -1, 192, 1, None), b"freqm")
    rc(lib.avs_ft_aug_draw(one, two, 4, 32768, F, 48, 192, 1, None), b"ft_aug_draw")
    gather = lambda plan, kind, std, stride=16, rows=4: lib.avs_im2col_audio_aug(one, one, one, two, rows, 48, 32, 3, stride, plan, kind, -5.0, std, 1.1, None)   # noqa: E731
    rc(gather(None, 1, 4.5), b"no augmentation plan")
    rc(gather(one, 2, 4.5), b"kind 2")
    rc(gather(one, -1, 4.5), b"kind -1")
    rc(gather(one, 1, 0.0), b"zero std")
    rc(gather(one, 1, 4.5, stride=17), b"stride 17")
    rc(gather(one, 1, 4.5, stride=0), b"stride 0")
    rc(gather(one, 1, 4.5, rows=0), b"im2col_audio_aug")
    rc(lib.avs_im2col_audio_aug(one, one, one, two, 4, 48, 32, 3, 16, one, 0, 0.0, 1.0, float("nan"), None), b"NaN")
    two_pass = lambda inp, out, plan, kind, std, Fm=32: lib.avs_augment_audio(inp, out, 4, 48, Fm, plan, kind, -5.0, std, 1.1, None)   # noqa: E731
    rc(two_pass(one, two, None, 1, 4.5), b"no augmentation plan")
    rc(two_pass(one, two, one, 2, 4.5), b"kind 2")
    rc(two_pass(one, two, one, 1, 0.0), b"zero std")
    rc(two_pass(one, one, one, 1, 4.5), b"augment_audio")              # in place
    rc(two_pass(one, two, one, 1, 4.5, Fm=30), b"augment_audio")       # F % 4
    rc(two_pass(None, two, one, 1, 4.5), b"augment_audio")


def test_plan_layout_mirrors_the_header():
    """ops.FtAug / FtAugState are the int32 images of avs_ft_aug_hdr + avs_ft_aug_sample[] / avs_ft_aug_state of include/avsiam_hip.h"""
    import re
    from avsiam_amd import ops
    src = open(_lib.HEADER).read()
    words = {}
    for name in ("avs_ft_aug_state", "avs_ft_aug_hdr", "avs_ft_aug_sample"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        n = 0
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                n += sum(int(m.group(1)) if (m := re.search(r"\[(\d+)\]", part)) else 1 for part in decl.split(","))
        words[name] = n
    assert words == {"avs_ft_aug_state": 4, "avs_ft_aug_hdr": ops.FtAug.HDR, "avs_ft_aug_sample": ops.FtAug.REC}
    plan = ops.FtAug.from_arrays([1, 2], [3, 4], [5, 6], [7, 8], [-9, 10], [0.05, 0.0], seed=(7 << 32) | 11, device="cpu", fill=1.25)
    h = plan.buf.numpy()
    assert h[:4].tolist() == [11, 7, 0, 2] and not h[4:8].any()
    assert h[8:16].tolist()[:5] == [1, 3, 5, 7, -9] and h[16:24].tolist()[:5] == [2, 4, 6, 8, 10]
    assert h[8:16][5:6].view(np.float32)[0] == np.float32(0.05) and plan.fill == 1.25 and plan.n == 2
    back = plan.arrays()
    assert back["noise_key"] == (7 << 32) | 11 and back["shift"].tolist() == [-9, 10] and back["n"] == 2
    with pytest.raises(_lib.AvsiamHipError):
        ops.FtAug.from_arrays([1], [3, 4], [5, 6], [7, 8], [9, 10], [0.05, 0.0], seed=0, device="cpu")
    with pytest.raises(_lib.AvsiamHipError):
        ops.FtAug.from_arrays([-1, 0], [3, 4], [5, 6], [7, 8], [9, 10], [0.05, 0.0], seed=0, device="cpu")
    st = ops.FtAugState("cpu", key=(0x89ABCDEF << 32) | 0xFEDCBA98, counter=3)
    assert st.buf.numpy().view(np.uint32).tolist() == [0xFEDCBA98, 0x89ABCDEF, 3, 0] and st.counter() == 3


def test_launcher_flags():
    from avsiam_amd.run_cavmae_ft_base import build_parser, inert_flag_warnings
    p = build_parser()
    args = p.parse_args(["--freqm", "48", "--timem", "192", "--noise", "True", "--raw-input"])
    assert args.raw_input is True and (args.freqm, args.timem, args.noise) == (48, 192, True)
    assert p.parse_args([]).raw_input is False
    assert inert_flag_warnings(args) == []
    warn = inert_flag_warnings(p.parse_args(["--mixup", "0.5", "--freqm", "48"]))
    assert any("not implemented" in w and "--mixup 0.5" in w for w in warn)
    assert not any("freqm" in w or "timem" in w or "noise" in w.split("not implemented")[0] for w in warn if "not implemented" in w)
    assert any("waveform" in w.lower() and "dataloader_ft.py:321-325" in w for w in warn)          # the reason mixup stays out
    warn = inert_flag_warnings(p.parse_args(["--wa", "True", "--bal", "bal"]))
    assert len(warn) == 1 and "--wa True" in warn[0] and "--bal bal" in warn[0]


def test_model_refuses_aug_where_nothing_trains():
    """argument checks that run before the device is needed"""
    import torch
    from avsiam_amd import ops
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(7, cfg=AVSiamConfig(depth=2))
    with pytest.raises(_lib.AvsiamHipError):                              # no GPU: still the first thing said
        m(torch.zeros(1, 1024, 128), None, "audioonly")
    assert m._input_xf(None, "mm_grad") is None
    xa, xv = ops.InputXf.audio(-5.081, 4.4849), ops.InputXf.frames()
    assert m._input_xf((xa, xv), "audioonly") == (xa, None) and m._input_xf((xa, xv), "videoonly") == (None, xv)
    with pytest.raises(ValueError):
        m._input_xf((xv, xa), "mm_grad")
    plan = ops.FtAug.from_arrays([0], [0], [0], [0], [0], [0.0], seed=0, device="cpu")
    with pytest.raises(ValueError):
        m._check_aug(plan, 2, "mm_grad")                                  # one record for two clips
    with pytest.raises(ValueError):
        m._check_aug(plan, 1, "videoonly")
    with pytest.raises(TypeError):
        m._check_aug((1, 2), 1, "mm_grad")
