"""Decoded-size frames, the parts that need no GPU: the float64 specification of the antialiased bicubic resize
(preprocess.resize_taps_reference / resize_frames_reference) against torch's own interpolate in float64 - what torchvision's Resize calls;
torchvision itself was never available to record from -, the kernel's tap arithmetic on the host (avs_resize_taps) against the specification
bit for bit, the launch plan, the argument checks of the new C-ABI symbols and the launcher's --frame-size flag."""
import ctypes

import numpy as np
import pytest
import torch

from avsiam_amd import _lib
from avsiam_amd import preprocess as pp

MAX_TAPS = 41
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _taps(lib, I, O, max_taps=MAX_TAPS):
    start, count, w = np.zeros(O, dtype=np.int32), np.zeros(O, dtype=np.int32), np.full((O, max_taps), 7.0, dtype=np.float32)
    rc = lib.avs_resize_taps(I, O, _ptr(start), _ptr(count), _ptr(w), max_taps)
    return rc, start, count, w


@pytest.mark.parametrize("I, O", [(360, 224), (640, 224), (1080, 224), (1920, 224), (2240, 224), (37, 16), (53, 16), (9, 16), (16, 16), (1, 4)])
def test_host_taps_are_the_specifications_bit_for_bit(lib, I, O):
    rc, start, count, w = _taps(lib, I, O)
    assert rc == 0
    rs, rn, rw = pp.resize_taps_reference(I, O)
    assert np.array_equal(start, rs) and np.array_equal(count, rn)
    assert count.min() >= 1 and count.max() <= MAX_TAPS and (start + count).max() <= I
    want = np.zeros((O, MAX_TAPS), dtype=np.float32)
    want[:, :rw.shape[1]] = rw.astype(np.float32)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))            # rounded once, zero beyond the count
    assert np.abs(rw.sum(axis=1) - 1.0).max() <= 1e-15 * MAX_TAPS


def test_tap_counts_of_the_common_sizes():
    """the counts the kernel's LDS regions are sized for: 7 / 12 at 360 x 640, 20 / 35 at 1080p, 4 when nothing shrinks"""
    got = {I: int(pp.resize_taps_reference(I, 224)[1].max()) for I in (360, 640, 1080, 1920, 240, 224)}
    assert got == {360: 7, 640: 12, 1080: 20, 1920: 35, 240: 5, 224: 4}
    assert int(pp.resize_taps_reference(9, 16)[1].max()) == 4 and int(pp.resize_taps_reference(2240, 224)[1].max()) <= MAX_TAPS


def test_host_taps_refuse_what_is_outside_the_range(lib):
    assert _taps(lib, 2241, 224)[0] == -2 and b"limited to 10" in lib.avs_last_error()
    assert _taps(lib, 640, 224, max_taps=12)[0] == -2 and b"max_taps" in lib.avs_last_error()     # 12 taps occur; the cap of the scale is 13
    assert _taps(lib, 640, 224, max_taps=13)[0] == 0
    assert _taps(lib, 0, 224)[0] == -2
    one = np.zeros(4, dtype=np.int32)
    assert lib.avs_resize_taps(4, 4, None, _ptr(one), _ptr(one), 8) == -2


def test_identity_taps_are_exactly_0_1_0_0(lib):
    rc, start, count, w = _taps(lib, 16, 16, max_taps=5)
    assert rc == 0
    for i in range(16):
        got = {start[i] + j: w[i, j] for j in range(count[i])}
        assert got.pop(i) == 1.0 and not any(got.values()), i                  # (+-0 elsewhere)


INTERP = [((37, 53), (16, 16)), ((9, 11), (16, 16)), ((75, 130), (16, 24))]


@pytest.mark.parametrize("src, dst", INTERP)
def test_reference_is_torchs_float64_interpolate(src, dst, record_property):
    """<= 1e-13 on values in [0, 1] (the two differ by the order of a few float64 roundings: about 1e-15); beside it, for context, how far
    torch's own float32 path is from its float64 path (it computes scale and centres in float32)"""
    g = np.random.default_rng(src[0])
    x = g.integers(0, 256, (2, 3) + src, dtype=np.uint8)
    want = torch.nn.functional.interpolate(torch.from_numpy(x).double() / 255, size=dst, mode="bicubic", align_corners=False, antialias=True)
    got = pp.resize_frames_reference(x, size=dst, mean=ZERO, std=ONE)
    assert got.dtype == np.float64 and got.shape == (2, 3) + dst
    err = np.abs(got - want.numpy()).max()
    t32 = torch.nn.functional.interpolate(torch.from_numpy(x).float() / 255, size=dst, mode="bicubic", align_corners=False, antialias=True)
    err32 = np.abs(t32.double().numpy() - want.numpy()).max()
    ours32 = np.abs(pp.resize_frames_reference(x, size=dst, mean=ZERO, std=ONE, dtype=np.float32).astype(np.float64) - want.numpy()).max()
    print(f"{src} -> {dst}: reference vs torch float64 {err:.2e}; torch float32 vs float64 {err32:.2e}; the steps in fp32 vs float64 {ours32:.2e}")
    record_property("reference_vs_torch64", float(err))
    record_property("torch32_vs_torch64", float(err32))
    assert err <= 1e-13


def test_overshoot_stays():
    """nothing clamps: a step edge, enlarged, rings below 0 and above 1 - in torch and here alike"""
    x = np.zeros((1, 3, 9, 11), dtype=np.uint8)
    x[..., 5:] = 255
    got = pp.resize_frames_reference(x, size=16, mean=ZERO, std=ONE)
    want = torch.nn.functional.interpolate(torch.from_numpy(x).double() / 255, size=(16, 16), mode="bicubic", align_corners=False, antialias=True).numpy()
    assert got.min() < -0.01 and got.max() > 1.01 and np.abs(got - want).max() <= 1e-13


def test_identity_gives_the_input_exactly():
    x = np.random.default_rng(3).integers(0, 256, (2, 2, 3, 16, 24), dtype=np.uint8)
    got = pp.resize_frames_reference(x, size=(16, 24))
    m, s = np.asarray(pp.IMAGENET_DEFAULT_MEAN)[:, None, None], np.asarray(pp.IMAGENET_DEFAULT_STD)[:, None, None]
    assert np.array_equal(got, (x.astype(np.float64) / 255.0 - m) / s)
    assert np.array_equal(pp.resize_frames_reference(x, size=(16, 24), mean=ZERO, std=ONE), x / 255.0)


def test_ragged_clips_in_a_padded_buffer_equal_the_clips_cropped():
    g = np.random.default_rng(5)
    buf = g.integers(0, 256, (3, 2, 3, 40, 64), dtype=np.uint8)
    sizes = [(37, 53), (20, 64), (16, 16)]
    got = pp.resize_frames_reference(buf, sizes, size=16)
    poisoned = buf.copy()
    for b, (h, w) in enumerate(sizes):
        poisoned[b, ..., h:, :] = 255
        poisoned[b, ..., :, w:] = 255
        want = pp.resize_frames_reference(np.ascontiguousarray(buf[b:b + 1, ..., :h, :w]), size=16)
        assert np.array_equal(got[b:b + 1], want), b
    assert np.array_equal(pp.resize_frames_reference(poisoned, sizes, size=16), got)          # the padding is never read
    # the mix, and its ends
    p = g.integers(0, 256, (3, 2, 3, 30, 30), dtype=np.uint8)
    psz = [(30, 30), (16, 16), (9, 11)]
    wgt = np.array([0.25, 1.0, 0.0])
    mixed = pp.resize_frames_reference(buf, sizes, partner=p, partner_sizes=psz, weight=wgt, size=16)
    pr = pp.resize_frames_reference(p, psz, size=16)
    assert np.array_equal(mixed[1], got[1]) and np.array_equal(mixed[2], pr[2])
    assert np.abs(mixed[0] - (0.25 * got[0] + 0.75 * pr[0])).max() <= 1e-15 * 8
    with pytest.raises(ValueError):
        pp.resize_frames_reference(buf, [(41, 53), (20, 64), (16, 16)], size=16)
    with pytest.raises(ValueError):
        pp.resize_frames_reference(buf, sizes, weight=wgt, size=16)
    with pytest.raises(ValueError):
        pp.resize_frames_reference(np.zeros((1, 3, 161, 8), dtype=np.uint8), size=16)         # scale above 10


def test_launcher_frame_size_flag():
    from avsiam_amd.run_cavmae_ft_base import build_parser, main
    p = build_parser()
    assert p.parse_args([]).frame_size is None
    args = p.parse_args(["--wave-input", "--frame-size", "360", "640", "--mixup", "0.5"])
    assert args.wave_input is True and list(args.frame_size) == [360, 640]
    with pytest.raises(SystemExit, match="--frame-size"):
        main(["--ftmode", "mm_grad", "--frame-size", "360", "640"])
    with pytest.raises(SystemExit, match="--frame-size"):
        main(["--ftmode", "mm_grad", "--raw-input", "--frame-size", "360", "640"])
    with pytest.raises(SystemExit, match="--frame-size"):
        main(["--ftmode", "mm_grad", "--wave-input", "--frame-size", "0", "640"])
    with pytest.raises(SystemExit, match="--frame-size"):
        main(["--ftmode", "mm_grad", "--wave-input", "--frame-size", "2241", "640"])          # more than 10 x 224


def test_new_symbols_are_declared_and_exported(lib):
    protos = _lib.parse_header()
    for name in ("avs_resize_taps", "avs_resize_plan", "avs_resize_frames_u8"):
        assert name in protos and hasattr(lib, name), name
    assert protos["avs_resize_frames_u8"][1].count("ptr") == 9 and len(protos["avs_resize_frames_u8"][1]) == 21
    assert protos["avs_resize_plan"][1] == ["int"] * 4 + ["ptr"] * 2


def _resize(lib, in1=16, Hs=40, Ws=64, sizes=None, mh=40, mw=64, in2=None, Hs2=0, Ws2=0, sizes2=None, mh2=0, mw2=0, weight=None, out=16, n=2, per=1,
            oh=16, ow=16, mean=True, std=(0.5, 0.5, 0.5)):
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5) if mean else None
    s3 = (ctypes.c_float * 3)(*std) if std else None
    v = lambda p: ctypes.c_void_p(p) if p else None
    return lib.avs_resize_frames_u8(v(in1), Hs, Ws, v(sizes), mh, mw, v(in2), Hs2, Ws2, v(sizes2), mh2, mw2, v(weight), v(out), n, per, oh, ow, m3, s3, None)


def test_the_abi_refuses_before_any_launch(lib):
    """every refusal is -2 from the host checks (no GPU here: a launch would fail with another code)"""
    assert _resize(lib, mh=161, Hs=161) == -2 and b"limited to 10" in lib.avs_last_error()          # scale above 10, rows
    assert _resize(lib, mw=161, Ws=161) == -2                                                       # and columns
    assert _resize(lib, ow=18) == -2 and b"multiple of 4" in lib.avs_last_error()
    assert _resize(lib, in1=0) == -2 and _resize(lib, out=0) == -2 and _resize(lib, mean=False) == -2 and _resize(lib, std=None) == -2
    assert _resize(lib, out=8) == -2 and b"16-byte" in lib.avs_last_error()
    assert _resize(lib, mh=41) == -2 and b"must fit the buffer" in lib.avs_last_error()
    assert _resize(lib, mh=0) == -2 and _resize(lib, mw=0) == -2
    assert _resize(lib, n=3, per=2) == -2
    assert _resize(lib, std=(0.5, 0.0, 0.5)) == -2 and b"zero std" in lib.avs_last_error()
    assert _resize(lib, weight=16) == -2 and b"without a partner" in lib.avs_last_error()
    assert _resize(lib, sizes2=16) == -2
    assert _resize(lib, in2=16, Hs2=30, Ws2=30, mh2=30, mw2=30) == -2 and b"needs a weight" in lib.avs_last_error()
    assert _resize(lib, in2=16, Hs2=30, Ws2=30, mh2=31, mw2=30, weight=16) == -2
    assert _resize(lib, in2=16, Hs2=200, Ws2=30, mh2=161, mw2=30, weight=16) == -2                  # the partner's scale


def _plan(lib, mh, mw, oh=224, ow=224):
    rows, lds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.avs_resize_plan(mh, mw, oh, ow, ctypes.byref(rows), ctypes.byref(lds))
    return rc, rows.value, lds.value


LDS_LIMIT = 96 * 1024          # two workgroups of the common sizes per CU (160 KiB); the largest supported case needs 93 KiB for one row


def test_plan_is_monotone_and_within_the_lds_limit(lib):
    assert _plan(lib, 2241, 224)[0] == -2 and _plan(lib, 224, 2241)[0] == -2 and _plan(lib, 224, 224, ow=222)[0] == -2
    assert lib.avs_resize_plan(224, 224, 224, 224, None, None) == -2
    seen = set()
    for mw in (224, 640, 1920, 2240):
        last = 1 << 30
        for mh in sorted(set(list(range(1, 2241, 13)) + [224, 360, 1080, 2240])):
            rc, rows, lds = _plan(lib, mh, mw)
            assert rc == 0 and rows in (1, 2, 4, 8, 16, 32) and 0 < lds <= LDS_LIMIT, (mh, mw, rows, lds)
            assert rows <= last, (mh, mw)                                      # a larger scale never gives more rows per workgroup
            last = rows
            seen.add(rows)
    for mh in (360, 1080):                                                      # and the same along the other axis
        last = 1 << 30
        for mw in range(4, 2241, 12):
            rows = _plan(lib, mh, mw)[1]
            assert rows <= last
            last = rows
    assert _plan(lib, 2240, 2240)[0] == 0                                       # the whole supported range has a plan at 224 x 224
    assert _plan(lib, 360, 640)[1] >= 16 and _plan(lib, 1080, 1920)[1] >= 2
    # the band of source rows the plan sizes the intermediate for holds every band: checked from the taps themselves
    for I, O in ((360, 224), (1080, 224), (2240, 224), (160, 16), (37, 16), (9, 16)):
        start, count, _ = pp.resize_taps_reference(I, O)
        rows = _plan(lib, I, 4 * O if O < 64 else 640, O, 224 if O >= 64 else 16)[1]
        for y0 in range(0, O, rows):
            y1 = min(y0 + rows, O) - 1
            span = start[y1] + count[y1] - start[y0]
            scale = I / O
            assert span <= min(I, int(np.ceil(scale * (rows - 1) + 4 * max(scale, 1.0))) + 2), (I, O, y0)
