"""Decoded-size frames on a real MI355X: the resize kernel (ops.resize_frames = avs_resize_frames_u8) against its float64 specification
(preprocess.resize_frames_reference, which tests/test_frames_cpu.py holds to torch's float64 interpolate), its exact cells, ragged batches,
the wrapper's refusals, the model on the kernel's frames, and the loader and launcher with --frame-size.

The bound of the kernel's error is derived, not fitted.  u = 2^-24 (fp32 unit roundoff), t the largest tap count and S the largest
sum |w| of an axis (from resize_taps_reference of the case's sizes):
  resized value, uint8 units   the horizontal sum of t_x products of fp32-rounded weights with exact integers is within (t_x + 1) u S_x 255 of
                               the float64 sum; the vertical sum adds (t_y + 1) u S_y max|h| and carries the first error times S_y:
                               E_r = (t_x + t_y + 2) u S_x S_y 255
  n(r) = (r c - mean) inv      c = fp32(1 / 255), the product, the fp32 mean, the subtraction, fp32(std), its reciprocal and the last product
                               are seven roundings, with A = S_x S_y >= |r| / 255:
                               E_n = (E_r / 255 + u (6 A + 5 |mean|)) / std
  mix w a + (1 - w) b          E = w E_a + (1 - w) E_b + 3 u (w max|a| + (1 - w) max|b|)            (1 - w, two products, one sum)
each times 1.01 for the second-order terms.  A numpy fp32 emulation of the accumulation sits at 0.05 - 0.17 of E_r; a tap start off by one
misses it by orders of magnitude.  The measured kernel-to-bound ratios go to the margin log (tests.helpers.record_margin), from which
profiles/r14/frames_margins.json is committed."""
import types

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
U = 2.0 ** -24
MEAN3 = np.array([0.485, 0.456, 0.406])
STD3 = np.array([0.229, 0.224, 0.225])


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


def u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def dev_u8(x, misalign=0):
    """the array on the device; misalign: its first byte sits that many bytes behind an aligned address, between bytes of 255"""
    x = np.ascontiguousarray(x)
    flat = torch.full((x.size + 8,), 255, dtype=torch.uint8, device=DEV)
    view = flat[misalign:misalign + x.size]
    view.copy_(torch.from_numpy(x).reshape(-1))
    return view.view(x.shape)


def guarded_out(shape):
    """an output tensor inside a larger buffer of sentinels (16-byte aligned: the guards are multiples of four floats) -> (out, check)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), SENT, dtype=torch.float32, device=DEV)
    out = buf[64:64 + n].view(shape)
    return out, lambda: bool((buf[:64] == SENT).all()) and bool((buf[64 + n:] == SENT).all())


def axis_stats(I, O):
    _, count, w = pp().resize_taps_reference(I, O)
    return int(count.max()), float(np.abs(w).sum(axis=1).max())


def bound_n(sizes, out_hw):
    """E_n per channel [3] for clips of `sizes` resized to out_hw, and A = S_x S_y"""
    e_r, A = 0.0, 0.0
    for h, w in sizes:
        ty, sy = axis_stats(h, out_hw[0])
        tx, sx = axis_stats(w, out_hw[1])
        e_r, A = max(e_r, (tx + ty + 2) * U * sx * sy * 255.0), max(A, sx * sy)
    return 1.01 * (e_r / 255.0 + U * (6.0 * A + 5.0 * np.abs(MEAN3))) / STD3, A


def plan(mh, mw, oh, ow):
    return ops().resize_plan(mh, mw, oh, ow)[0]


def ratio_to_bound(got, want, bound3):
    """max over the elements of |got - want| / bound of the element's channel (the channel axis is -3)"""
    err = np.abs(got.double().cpu().numpy() - want)
    return float((err / bound3.reshape(3, 1, 1)).max()), float(err.max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the float64 restatement
CASES = [((37, 53), (16, 16), 3), ((9, 11), (16, 16), 1), ((75, 130), (16, 24), 2), ((160, 40), (16, 16), 0), ((20, 300), (16, 260), 1)]


def _check_case(src, dst, misalign):
    from tests.helpers import record_margin
    x = u8(src[0] * 1000 + src[1], 2, 3, *src)
    want = pp().resize_frames_reference(x, size=dst)
    out, intact = guarded_out((2, 3) + dst)
    got = ops().resize_frames(dev_u8(x, misalign), size=dst, out=out)
    assert got.data_ptr() == out.data_ptr() and intact()
    b3, _ = bound_n([src], dst)
    ratio, err = ratio_to_bound(got, want, b3)
    tx, ty = axis_stats(src[1], dst[1])[0], axis_stats(src[0], dst[0])[0]
    rows = plan(src[0], src[1], *dst)
    print(f"resize {src} -> {dst}: taps {ty}/{tx}, rows per workgroup {rows}, max error {err:.3e}, bound {b3.max():.3e}, error / bound {ratio:.3f}")
    record_margin(f"frames.kernel_vs_float64.{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}", ratio=ratio, max_err=err, bound=float(b3.max()), taps_y=ty,
                  taps_x=tx, rows_per_wg=rows)
    assert ratio <= 1.0, (src, dst, ratio)


@pytest.mark.parametrize("src, dst, misalign", CASES, ids=[f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d, _ in CASES])
def test_kernel_against_the_float64_specification(src, dst, misalign):
    """taps 10/14, an enlargement, taps 19/22, scale 10 on one axis, and an output wider than one trip of the horizontal pass's threads; source
    rows at every byte alignment (widths that are no multiple of 4, a buffer that starts 1 - 3 bytes behind an aligned address)"""
    _check_case(src, dst, misalign)


def test_every_variant_the_plan_can_choose():
    """the smallest source height that reaches each rows-per-workgroup value of avs_resize_plan, at output 16 x 224 (the LDS regions scale with
    the output width: a narrow output always takes the largest value) and source widths 224 and 2240 (41 column taps)"""
    found = {}
    for w in (224, 2240):
        for h in range(1, 161):
            found.setdefault(plan(h, w, 16, 224), (h, w))
    assert set(found) == {32, 16, 8, 4, 2, 1}, found
    for rows, hw in sorted(found.items()):
        _check_case(hw, (16, 224), 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. exact cells
def test_a_clip_at_the_output_size_is_normalize_frames():
    o = ops()
    v = dev_u8(u8(1, 2, 2, 3, 16, 24))
    assert same_bits(o.resize_frames(v, size=(16, 24)), pp().normalize_frames(v))
    # and inside a padded buffer, beside clips that are resized
    buf = u8(2, 3, 3, 40, 64)
    got = o.resize_frames(dev_u8(buf), [(37, 53), (16, 16), (40, 64)], size=16)
    assert same_bits(got[1], pp().normalize_frames(dev_u8(buf[1, :, :16, :16])))
    # two clips at the output size, mixed: mix_frames' bytes
    p = dev_u8(u8(3, 2, 2, 3, 16, 24))
    w = torch.tensor([0.37, 0.81], device=DEV)
    assert same_bits(o.resize_frames(v, partner=p, weight=w, size=(16, 24)), o.mix_frames(v, p, w))


def test_weight_one_is_the_plain_path_and_two_calls_agree():
    o = ops()
    v, p = dev_u8(u8(3, 3, 2, 3, 40, 64)), dev_u8(u8(4, 3, 2, 3, 30, 50), 1)
    sizes, psz = [(37, 53), (20, 64), (16, 16)], [(30, 50), (9, 11), (25, 25)]
    plain = o.resize_frames(v, sizes, size=16)
    assert same_bits(o.resize_frames(v, sizes, partner=p, partner_sizes=psz, weight=[1.0, 1.0, 1.0], size=16), plain)
    assert same_bits(o.resize_frames(v, sizes, size=16), plain)
    w = torch.tensor([0.3, 1.0, 0.0], device=DEV)
    a, b = (o.resize_frames(v, sizes, partner=p, partner_sizes=psz, weight=w, size=16) for _ in range(2))
    assert same_bits(a, b) and same_bits(a[1], plain[1]) and same_bits(a[2], o.resize_frames(p, psz, size=16)[2])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. a ragged batch
def test_ragged_batch_equals_its_clips_cropped():
    from tests.helpers import record_margin
    o = ops()
    sizes, psz = [(37, 53), (20, 64), (16, 16)], [(30, 30), (16, 16), (9, 11)]
    buf, par = u8(5, 3, 2, 3, 40, 64), u8(6, 3, 2, 3, 30, 30)
    for b, (h, w) in enumerate(sizes):                                            # the padding: 255, never read
        buf[b, ..., h:, :] = 255
        buf[b, ..., :, w:] = 255
    for b, (h, w) in enumerate(psz):
        par[b, ..., h:, :] = 255
        par[b, ..., :, w:] = 255
    out, intact = guarded_out((3, 2, 3, 16, 16))
    got = o.resize_frames(dev_u8(buf), sizes, size=16, out=out)
    assert intact()
    for b, (h, w) in enumerate(sizes):
        alone = o.resize_frames(dev_u8(buf[b:b + 1, ..., :h, :w]), size=16)
        assert same_bits(got[b:b + 1], alone), b
    b3, _ = bound_n(sizes, (16, 16))
    ratio, err = ratio_to_bound(got, pp().resize_frames_reference(buf, sizes, size=16), b3)
    # the mix: partner buffers of other sizes
    weight = np.array([0.25, 0.6, 0.83], dtype=np.float32)
    mixed = o.resize_frames(dev_u8(buf), sizes, partner=dev_u8(par, 2), partner_sizes=psz, weight=weight, size=16)
    want = pp().resize_frames_reference(buf, sizes, partner=par, partner_sizes=psz, weight=weight, size=16)
    worst = 0.0
    for b in range(3):
        ea, A = bound_n([sizes[b]], (16, 16))
        eb, Ab = bound_n([psz[b]], (16, 16))
        top_a, top_b = (A + np.abs(MEAN3)) / STD3, (Ab + np.abs(MEAN3)) / STD3
        wb = float(weight[b])
        e = 1.01 * (wb * ea + (1 - wb) * eb + 3 * U * (wb * top_a + (1 - wb) * top_b))
        r, _ = ratio_to_bound(mixed[b], want[b], e)
        worst = max(worst, r)
    print(f"ragged batch: plain error / bound {ratio:.3f} (max error {err:.3e}), mixed error / bound {worst:.3f}")
    record_margin("frames.ragged_batch", plain_ratio=ratio, plain_max_err=err, mixed_ratio=worst)
    assert ratio <= 1.0 and worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the wrapper's refusals
def test_wrapper_refusals():
    from avsiam_amd import _lib
    o = ops()
    v = dev_u8(u8(7, 2, 3, 40, 64))
    with pytest.raises(_lib.AvsiamHipError, match="host values"):
        o.resize_frames(v, torch.tensor([[37, 53], [20, 64]], dtype=torch.int32, device=DEV), size=16)
    with pytest.raises(_lib.AvsiamHipError, match="without a partner"):
        o.resize_frames(v, size=16, weight=[0.5, 0.5])
    with pytest.raises(_lib.AvsiamHipError, match="without a partner"):
        o.resize_frames(v, size=16, partner_sizes=[(4, 4), (4, 4)])
    with pytest.raises(_lib.AvsiamHipError):
        o.resize_frames(v, size=16, out=torch.zeros(2, 3, 16, 20, device=DEV))
    with pytest.raises(_lib.AvsiamHipError):
        o.resize_frames(v, size=(16, 18))
    with pytest.raises(_lib.AvsiamHipError):
        o.resize_frames(v, size=16, partner=dev_u8(u8(8, 3, 3, 30, 30)), weight=[0.5, 0.5])          # another B
    with pytest.raises(_lib.AvsiamHipError):
        o.resize_frames(v, size=16, partner=dev_u8(u8(8, 2, 3, 30, 30)))                             # no weight
    with pytest.raises(_lib.AvsiamHipError):
        o.resize_frames(v.float(), size=16)
    with pytest.raises(ValueError):
        o.resize_frames(v, [(41, 64), (20, 64)], size=16)                                            # beyond the buffer
    with pytest.raises(ValueError):
        o.resize_frames(v, [(0, 64), (20, 64)], size=16)
    with pytest.raises(ValueError):
        o.resize_frames(dev_u8(u8(9, 1, 3, 8, 164)), size=16)                                        # scale above 10


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the model on the kernel's frames
LBL, MB = 7, 3
CFG = AVSiamConfig(depth=2)
# 3 x the measured values (profiles/r14/frames_margins.json: mm loss 7.4e-5, 1 - cosine 9.8e-6, norm 2.0e-4; v 2.9e-5, 3.3e-6, 3.1e-5; the same
# figures in every run) - the two inputs differ by ~1e-6 and round to different bf16 patch values here and there
STEP_BOUNDS = {"mm": dict(loss_rel=2.3e-4, cos=1 - 3.0e-5, norm=6.2e-4), "v": dict(loss_rel=9.0e-5, cos=1 - 1.0e-5, norm=9.3e-5)}


@pytest.fixture(scope="module")
def model_case():
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.weights import synth_inputs
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()
    m.requires_grad_(True)
    a, _ = synth_inputs(CFG, MB, 61)
    frames, partner = u8(11, MB, 1, 3, 40, 64), u8(12, MB, 1, 3, 30, 50)
    kw = dict(sizes=[(37, 53), (40, 64), (20, 48)], partner_sizes=[(30, 50), (16, 16), (25, 33)], weight=np.array([0.4, 1.0, 0.7], dtype=np.float32))
    v_ref = pp().resize_frames_reference(frames, kw["sizes"], partner=partner, partner_sizes=kw["partner_sizes"], weight=kw["weight"], size=CFG.img_size)
    v_dev = ops().resize_frames(dev_u8(frames), kw["sizes"], partner=dev_u8(partner), partner_sizes=kw["partner_sizes"], weight=kw["weight"],
                                size=CFG.img_size)
    g = torch.Generator().manual_seed(3)
    hot = (torch.rand(MB, LBL, generator=g) < 0.3).float()
    hot[:, 0] = 1.0
    y = (hot * 0.9 + 0.1 / LBL).cuda()
    return types.SimpleNamespace(m=m, a=a.cuda(), v_dev=v_dev, v_ref=torch.from_numpy(v_ref.astype(np.float32)).to(DEV), y=y)


@pytest.mark.parametrize("branch", ["mm", "v"])
def test_train_step_on_the_kernels_frames_equals_the_step_on_the_specification(model_case, branch):
    """the fused step on ops.resize_frames output (ragged, partly mixed clips enlarged to the model's size) against the step on the float64
    specification of the same clips cast to fp32: relative loss difference, worst gradient cosine and worst norm ratio over the parameters"""
    from tests.helpers import record_margin
    c = model_case
    assert c.v_dev.shape == (MB, 1, 3, CFG.img_size, CFG.img_size) and c.v_dev.dtype == torch.float32
    steps = []
    for v in (c.v_dev, c.v_ref):
        loss = float(c.m.train_step(c.a, v, c.y, 0.0, "mm_grad", branch=branch))
        steps.append((loss, {n: p.grad.clone() for n, p in c.m._params.items() if p.grad is not None}))
    (l_dev, g_dev), (l_ref, g_ref) = steps
    assert np.isfinite(l_dev) and set(g_dev) == set(g_ref) and len(g_dev) > 0
    worst_cos, worst_norm = 1.0, 0.0
    for n, r in g_ref.items():
        g, r = g_dev[n].double().reshape(-1), r.double().reshape(-1)
        if float(r.norm()) == 0:
            assert float(g.norm()) == 0, n
            continue
        cos, nr = float(g @ r / (g.norm() * r.norm())), abs(float(g.norm() / r.norm()) - 1)
        worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, nr)
    loss_rel = abs(l_dev - l_ref) / abs(l_ref)
    bounds = STEP_BOUNDS[branch]
    print(f"frames step ({branch}): loss {l_dev:.6f} / {l_ref:.6f} (relative {loss_rel:.3e}), worst cosine {worst_cos:.8f}, worst norm error {worst_norm:.3e}")
    record_margin(f"frames.step_on_kernel_frames.{branch}", worst_cos=worst_cos, worst_norm=worst_norm, loss_rel=loss_rel, bound_loss_rel=bounds["loss_rel"],
                  bound_cos=bounds["cos"], bound_norm=bounds["norm"])
    assert loss_rel <= bounds["loss_rel"] and worst_cos >= bounds["cos"] and worst_norm <= bounds["norm"], (loss_rel, worst_cos, worst_norm)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. loader and launcher
def test_wave_loader_with_a_frame_size():
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    kw = dict(seed=87, mixup=0.5, norm=(-5.081, 4.4849), samples=8000)
    tr = SyntheticWaveFtLoader(CFG, 4, 2, LBL, DEV, frames=2, frame_size=(40, 64), **kw)
    assert tr.v.shape == (4, 2, 3, 40, 64) and tr.v.dtype == torch.uint8
    seen = set()
    for a, v, y in tr:
        d = tr.last_draw
        assert v.shape == (4, 2, 3, CFG.img_size, CFG.img_size) and v.dtype == torch.float32 and bool(torch.isfinite(v).all())
        assert d["sizes"].shape == (4, 2) and d["partner_sizes"].shape == (4, 2)
        seen |= {tuple(s) for s in d["sizes"].tolist()}
        want = ops().resize_frames(tr.v, d["sizes"], partner=tr.v2, partner_sizes=d["partner_sizes"], weight=d["weight"], size=CFG.img_size)
        assert same_bits(v, want)
    assert seen <= {(40, 64), (40, 48)} and len(seen) == 2                      # the full frame and the narrower crop both occur
    va = SyntheticWaveFtLoader(CFG, 2, 1, LBL, DEV, seed=88, mixup=0.5, frames=10, train=False, samples=8000, frame_size=(40, 64))
    (a, v, y), = list(va)
    assert v.shape == (2, 10, 3, CFG.img_size, CFG.img_size) and "partner_sizes" not in va.last_draw
    assert same_bits(v, ops().resize_frames(va.v, va.last_draw["sizes"], size=CFG.img_size))
    # frame_size=None: the loader's bytes and draws of before
    old = SyntheticWaveFtLoader(CFG, 4, 2, LBL, DEV, **kw)
    new = SyntheticWaveFtLoader(CFG, 4, 2, LBL, DEV, frame_size=None, **kw)
    assert old.v.shape == (4, 1, 3, CFG.img_size, CFG.img_size)
    for (a0, v0, y0), (a1, v1, y1) in zip(old, new):
        assert same_bits(a0, a1) and same_bits(v0, v1) and same_bits(y0, y1) and "sizes" not in new.last_draw
        assert same_bits(v0, ops().mix_frames(old.v, old.v2, old.last_draw["weight"]))
        # the draws every loader shares do not depend on the frame size
        assert all(np.array_equal(old.last_draw[k], new.last_draw[k]) for k in old.last_draw)


def test_launcher_with_a_frame_size(tmp_path, capsys):
    """--wave-input --frame-size 40 64 --mixup 0.5 at the smallest synthetic setting of the launcher tests: one epoch and its validation finish
    with finite, recorded losses"""
    from avsiam_amd.run_cavmae_ft_base import main
    exp = tmp_path / "ft"
    out = main(["--ftmode", "mm_grad", "--n_class", "527", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "2", "--n_epochs", "1",
                "--exp_dir", str(exp), "--steps-per-epoch", "3", "--val-steps", "1", "--label_smooth", "0.1", "--wave-input", "--frame-size", "40", "64",
                "--mixup", "0.5"])
    said = capsys.readouterr().out
    assert "not implemented" not in said
    res = np.loadtxt(exp / "result.csv", delimiter=",").reshape(-1, 4)
    assert res.shape == (1, 4) and np.all(np.isfinite(res)), res
    assert "valid loss" in said and "nan" not in said.split("valid loss")[1].split()[0]
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3])
