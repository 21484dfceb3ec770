"""Reconstructions from the MAE pass on the device: the unpatchify kernel (csrc/inpaint.hip) called directly, MaePass.reconstruct /
CAVMAE_BASE.inpaint at the parity shapes, the region plans through inpaint(), training left undisturbed, and the command-line tool.

The kernel only moves values (and, for raw outputs, applies one multiply, one add and one rounding that numpy float32 restates), so every
kernel-level comparison is bit for bit: against preprocess.unpatchify_reference built from the same rows, with the outputs inside sentinel
guard bands.  Model level: masked cells against eng.predictions() re-arranged (bit for bit), kept cells against the input (bit for bit), and
against the CPU oracle with the bound test_parity_gpu already puts on the same predictions (2e-2 relative L2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
SENT8 = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    torch.manual_seed(0)


def ops():
    from avsiam_amd import ops as o
    return o


def refused():
    from avsiam_amd import _lib
    return pytest.raises((_lib.AvsiamHipError, AssertionError, ValueError))


def guarded(shape, dtype, guard):
    """a buffer of sentinels with a window of `shape` behind `guard` elements (64: the window stays 16-byte aligned - the kernel's 4-wide stores;
    3: it does not - the element-wise stores) -> (buffer, window as a flat view)"""
    n = int(np.prod(shape))
    buf = torch.full((guard + n + 64,), SENT8 if dtype == torch.uint8 else SENT, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n]


def guards_intact(buf, guard, n):
    fill = SENT8 if buf.dtype == torch.uint8 else SENT
    return bool((buf[:guard] == fill).all().item()) and bool((buf[guard + n:] == fill).all().item())


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel.  Three samples (frames: three clips of two frames): one fully kept, one fully masked, one mixed.
def _case(audio, stride):
    """-> dict(inp [n, ...] fp32 numpy, rows [n, L, P] fp32, mask [n, L], n, L, C, clip sample of every picture)"""
    rng = np.random.default_rng(100 * stride + audio)
    if audio:
        shape = (3, 64, 32) if stride == 16 else (3, 56, 30)            # stride 14: mel bins 28, 29 belong to no patch
        n, L, C = 3, (shape[1] // stride) * (shape[2] // stride), 1
        sample = np.arange(3)
    else:
        side = 32 if stride == 16 else 28
        shape = (6, 3, side, side)                                      # [3 * 2, 3, H, W]
        n, L, C = 6, (side // stride) ** 2, 3
        sample = np.arange(6) // 2
    inp = rng.standard_normal(shape).astype(np.float32)
    rows = rng.standard_normal((n, L, 256 * C)).astype(np.float32)
    mask = np.zeros((n, L), dtype=np.float32)
    mask[sample == 1] = 1.0
    mixed = rng.random((n, L)) < 0.5
    mixed[:, 0], mixed[:, -1] = True, False                             # both kinds in every picture of the mixed sample
    mask[sample == 2] = mixed[sample == 2].astype(np.float32)
    return dict(inp=inp, rows=rows, mask=mask, n=n, L=L, C=C)


def _compact(case, id_base, rng):
    """the scored rows only, in a shuffled order, and their ids (as maskplan.hip's pred_id: position + id_base)"""
    pos = np.flatnonzero(case["mask"].reshape(-1) == 1)
    pos = pos[rng.permutation(pos.size)]
    rows = case["rows"].reshape(case["n"] * case["L"], -1)[pos]
    return np.ascontiguousarray(rows), (pos + id_base).astype(np.int32)


@pytest.mark.parametrize("guard", [64, 3])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("stride", [16, 14])
@pytest.mark.parametrize("audio", [True, False])
def test_kernel_matches_the_numpy_reference_bit_for_bit(audio, stride, compact, guard):
    from avsiam_amd.preprocess import unpatchify_reference
    c = _case(audio, stride)
    want = unpatchify_reference(c["rows"], c["inp"], audio, stride, c["mask"])
    inp = torch.from_numpy(c["inp"]).to(DEV)
    mask = torch.from_numpy(c["mask"]).to(DEV)
    id_base = 0 if audio else 3 * 7                                     # frames: the engine passes B * La
    if compact:
        rows, ids = _compact(c, id_base, np.random.default_rng(5))
        pred, row_id = torch.from_numpy(rows).to(DEV), torch.from_numpy(ids).to(DEV)
    else:
        pred, row_id = torch.from_numpy(c["rows"].reshape(c["n"] * c["L"], -1)).to(DEV), None
    row_loss = torch.rand(pred.shape[0], device=DEV) + 0.5
    if not compact:
        row_loss = row_loss * mask.view(-1)                             # what mae_loss_fwd leaves on kept rows
    got = []
    for _ in range(2):
        buf, win = guarded(c["inp"].shape, torch.float32, guard)
        ebuf, ewin = guarded(c["mask"].shape, torch.float32, guard)
        ops().unpatchify(pred, inp, mask, audio, c["L"], stride=stride, row_id=row_id, id_base=id_base, row_loss=row_loss, out=win, err=ewin)
        torch.cuda.synchronize()
        assert guards_intact(buf, guard, win.numel()) and guards_intact(ebuf, guard, ewin.numel())
        got.append((win.cpu().numpy().reshape(c["inp"].shape), ewin.cpu().numpy().reshape(c["mask"].shape)))
    assert same_bits(got[0][0], want)
    assert same_bits(got[1][0], got[0][0]) and same_bits(got[1][1], got[0][1])           # a second call: identical bytes
    # the error map: row_loss scattered by row_id, 0 on kept tokens
    err = np.zeros(c["n"] * c["L"], dtype=np.float32)
    rl = row_loss.cpu().numpy()
    if compact:
        err[row_id.cpu().numpy() - id_base] = rl
    else:
        err = rl.copy()
    assert same_bits(got[0][1], err.reshape(c["mask"].shape))
    # (uncovered cells at stride 14: the input)
    if audio and stride == 14:
        assert same_bits(got[0][0][:, :, 28:], c["inp"][:, :, 28:])


@pytest.mark.parametrize("stride", [16, 14])
@pytest.mark.parametrize("audio", [True, False])
def test_kernel_every_patch_from_the_rows(audio, stride):
    """paste_kept off: every covered cell is its row's, whatever the mask; uncovered cells stay the input"""
    from avsiam_amd.preprocess import unpatchify_reference
    c = _case(audio, stride)
    want = unpatchify_reference(c["rows"], c["inp"], audio, stride, None)
    buf, win = guarded(c["inp"].shape, torch.float32, 64)
    ops().unpatchify(torch.from_numpy(c["rows"].reshape(c["n"] * c["L"], -1)).to(DEV), torch.from_numpy(c["inp"]).to(DEV),
                     torch.from_numpy(c["mask"]).to(DEV), audio, c["L"], stride=stride, paste_kept=False, out=win)
    torch.cuda.synchronize()
    assert guards_intact(buf, 64, win.numel())
    assert same_bits(win.cpu().numpy().reshape(c["inp"].shape), want)


MEAN_A, STD_A = -5.081, 4.4849


@pytest.mark.parametrize("guard", [64, 3])
@pytest.mark.parametrize("stride", [16, 14])
def test_kernel_raw_audio(stride, guard):
    """un-normalised fbank + InputXf: kept cells are what avs_input_xf gives (normalize_fbank, the two-pass form), bit for bit; the raw output
    is x * std + mean in float32, multiply and add rounded separately"""
    from avsiam_amd.preprocess import normalize_fbank, unnormalize_reference, unpatchify_reference
    c = _case(True, stride)
    fbank = (c["inp"] * 4.0 - 5.0).astype(np.float32)
    fb = torch.from_numpy(fbank).to(DEV)
    # (avs_normalize_audio wants F % 4 == 0: the 30 mel bins of the stride-14 case go through it padded to 32 - the arithmetic is per element)
    padded = torch.zeros(fbank.shape[0], fbank.shape[1], -(-fbank.shape[2] // 4) * 4, device=DEV)
    padded[:, :, :fbank.shape[2]] = fb
    seen = np.ascontiguousarray(normalize_fbank(padded, MEAN_A, STD_A).cpu().numpy()[:, :, :fbank.shape[2]])
    xf = ops().InputXf.audio(MEAN_A, STD_A)
    want = unpatchify_reference(c["rows"], seen, True, stride, c["mask"])
    buf, win = guarded(fbank.shape, torch.float32, guard)
    rbuf, rwin = guarded(fbank.shape, torch.float32, guard)
    ops().unpatchify(torch.from_numpy(c["rows"].reshape(c["n"] * c["L"], -1)).to(DEV), fb, torch.from_numpy(c["mask"]).to(DEV), True, c["L"], xf=xf,
                     stride=stride, raw=True, out=win, raw_out=rwin)
    torch.cuda.synchronize()
    assert guards_intact(buf, guard, win.numel()) and guards_intact(rbuf, guard, rwin.numel())
    assert same_bits(win.cpu().numpy().reshape(fbank.shape), want)
    assert same_bits(rwin.cpu().numpy().reshape(fbank.shape), unnormalize_reference(want, MEAN_A, STD_A, True))


@pytest.mark.parametrize("guard", [64, 3])
@pytest.mark.parametrize("stride", [16, 14])
def test_kernel_raw_frames(stride, guard):
    """uint8 frames + InputXf: kept cells equal normalize_frames bit for bit; raw=True gives the original uint8 on kept cells exactly and the
    numpy float32 restatement rint((x * std_c + mean_c) * 255), clamped, on masked cells exactly (the rows reach well outside 0..255)"""
    from avsiam_amd.preprocess import IMAGENET_DEFAULT_MEAN as M, IMAGENET_DEFAULT_STD as S, normalize_frames, unnormalize_reference, unpatchify_reference
    c = _case(False, stride)
    rng = np.random.default_rng(9)
    u8 = rng.integers(0, 256, c["inp"].shape, dtype=np.uint8)
    u8[0, 0, 0, :4] = (0, 255, 1, 254)
    fr = torch.from_numpy(u8).to(DEV)
    seen = normalize_frames(fr).cpu().numpy()
    rows = (c["rows"] * 2.0).astype(np.float32)                        # (x * 0.229 + 0.485) * 255 then spans about -400 .. 650
    want = unpatchify_reference(rows, seen, False, stride, c["mask"])
    xf = ops().InputXf.frames()
    buf, win = guarded(u8.shape, torch.float32, guard)
    rbuf, rwin = guarded(u8.shape, torch.uint8, guard)
    ops().unpatchify(torch.from_numpy(rows.reshape(c["n"] * c["L"], -1)).to(DEV), fr, torch.from_numpy(c["mask"]).to(DEV), False, c["L"], xf=xf,
                     stride=stride, raw=True, out=win, raw_out=rwin)
    torch.cuda.synchronize()
    assert guards_intact(buf, guard, win.numel()) and guards_intact(rbuf, guard, rwin.numel())
    assert same_bits(win.cpu().numpy().reshape(u8.shape), want)
    raw = rwin.cpu().numpy().reshape(u8.shape)
    assert same_bits(raw, unnormalize_reference(want, M, S, False))
    kept = unpatchify_reference(np.ones_like(rows), np.zeros_like(seen), False, stride, c["mask"]) == 0       # cells that came from the input
    assert kept.any() and (~kept).any() and np.array_equal(raw[kept], u8[kept])


def test_kernel_refusals():
    c = _case(True, 16)
    pred = torch.from_numpy(c["rows"].reshape(c["n"] * c["L"], -1)).to(DEV)
    inp, mask = torch.from_numpy(c["inp"]).to(DEV), torch.from_numpy(c["mask"]).to(DEV)
    shift = torch.zeros(3, dtype=torch.int32, device=DEV)
    amp = torch.zeros(3, device=DEV)
    noisy = ops().InputXf.audio(MEAN_A, STD_A, shift=shift, amp=amp, seed=3)
    with refused():                                                     # a transform that carries shift / amp, together with raw
        ops().unpatchify(pred, inp, mask, True, c["L"], xf=noisy, raw=True)
    from avsiam_amd import _lib
    out, raw = torch.empty_like(inp), torch.empty_like(inp)
    with pytest.raises(_lib.AvsiamHipError, match="shift / amp"):       # ... and the library itself refuses it too
        _lib.call("avs_unpatchify", pred, inp, mask, out, raw, None, None, pred.shape[0], 1, 3, c["L"], 1, 64, 32, 16, ops()._xf_arg(noisy, 1, 3),
                  None, 0, None, 1, _lib.current_stream())
    ops().unpatchify(pred, inp, mask, True, c["L"], xf=noisy)           # (without raw the same transform is fine)
    with refused():                                                     # raw without a transform
        ops().unpatchify(pred, inp, mask, True, c["L"], raw=True)
    with refused():                                                     # L that does not fit the picture
        ops().unpatchify(pred, inp, mask, True, c["L"] + 1)
    with refused():                                                     # too few prediction rows
        ops().unpatchify(pred[:5], inp, mask, True, c["L"])
    with refused():
        ops().unpatchify(pred.double(), inp, mask, True, c["L"])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the model.  Shapes of tests/test_parity_gpu.py: ViT-B with 128 audio tokens at (B, T) = (4, 1) and (2, 3), ViT-H/14 (stride 14) at B = 2.
ORACLE_REL_L2 = 2e-2          # test_parity_gpu.test_pass_matches_oracle_full_gradients' bound on the same scored predictions


def _cfg(name):
    from avsiam_amd.config import AVSiamConfig, vit_huge14
    if name == "huge14":
        return vit_huge14(frames=2, depth=2), 2
    B, T = (4, 1) if name == "b4_t1" else (2, 3)
    return AVSiamConfig(audio_tokens=128, frames=T), B


def _model(cfg, seed=4321, **kw):
    from avsiam_amd.models import CAVMAE_BASE, CAVMAE_HUGE
    cls = CAVMAE_HUGE if cfg.embed_dim == 1280 else CAVMAE_BASE
    return cls(cfg=cfg, init_seed=seed, init_mode="random", verbose=False, **kw).cuda()


def _inputs(cfg, B, seed=99):
    from avsiam_amd.weights import synth_inputs
    a, v = synth_inputs(cfg, B, seed)
    return a, v


def _fold(x, cfg):
    """frames as [B * T, C, H, W] numpy"""
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return x.reshape(-1, *x.shape[-3:])


def _masked_rel_l2(got, want, cells):
    g, w = got.astype(np.float64)[cells], want.astype(np.float64)[cells]
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


def _cells(mask, shape, audio, stride):
    """bool cell mask of the tokens whose mask is 1"""
    from avsiam_amd.preprocess import unpatchify_reference
    n, L = mask.shape
    C = 1 if audio else shape[1]
    return unpatchify_reference(np.ones((n, L, 256 * C), dtype=np.float32), np.zeros(shape, dtype=np.float32), audio, stride, mask) == 1


@pytest.mark.parametrize("name", ["b4_t1", "b2_t3", "huge14"])
def test_inpaint_is_the_mae_pass_rearranged(name):
    """injected plan: masked cells are eng.predictions() re-arranged and kept cells the input, both bit for bit; the losses are forward()'s under
    no_grad, bit for bit (same kernels, same order); the masks are equal; the error map is the loss's own row terms; and against the CPU oracle
    the masked cells stay inside the bound the parity test puts on the same predictions."""
    from avsiam_amd.maskplan import make_mae_plan
    from avsiam_amd.preprocess import unpatchify_reference
    from avsiam_amd.weights import synth_state
    from oracle import ref_cpu
    cfg, B = _cfg(name)
    S, T, La, Lv = cfg.st, cfg.frames, cfg.audio_tokens, cfg.video_tokens
    a, v = _inputs(cfg, B)
    plan = make_mae_plan(cfg, B, torch.Generator().manual_seed(7))
    m = _model(cfg)
    ag, vg = a.cuda(), v.cuda()
    with torch.no_grad():
        out = m(ag, vg, mae_loss_weight=1, contrast_loss_weight=0, mask_plan=plan)
    eng = m._engine("mae", B)
    pa, pv = (p.numpy() for p in eng.predictions())
    with torch.enable_grad():                                             # whatever the caller's grad mode
        res = m.inpaint(ag, vg, mask_plan=plan)
    assert all(t.is_cuda and not t.requires_grad for t in res)
    assert res.audio.shape == a.shape and res.imgs.shape == v.shape and res.err_a.shape == (B, La) and res.err_v.shape == (B, T * Lv)
    assert torch.equal(res.mask_a, out[5]) and torch.equal(res.mask_v, out[6])
    assert torch.equal(res.mask_a.cpu(), plan.mask_a()) and torch.equal(res.mask_v.cpu(), plan.mask_v().reshape(B, T * Lv))
    assert res.loss_mae_a.shape == () and same_bits(res.loss_mae_a.cpu().numpy(), out[2].cpu().numpy()) and same_bits(res.loss_mae_v.cpu().numpy(), out[3].cpu().numpy())
    mask_a, mask_v = plan.mask_a().numpy(), plan.mask_v().reshape(B * T, Lv).numpy()
    want_a = unpatchify_reference(pa, a.numpy(), True, S, mask_a)
    want_v = unpatchify_reference(pv.reshape(B * T, Lv, -1), _fold(v, cfg), False, S, mask_v)
    got_a, got_v = res.audio.cpu().numpy(), _fold(res.imgs, cfg)
    assert np.isfinite(want_a).all() and np.isfinite(want_v).all()
    assert same_bits(got_a, want_a) and same_bits(got_v, want_v)
    ca, cv = _cells(mask_a, a.shape, True, S), _cells(mask_v, got_v.shape, False, S)
    assert same_bits(got_a[~ca], a.numpy()[~ca]) and same_bits(got_v[~cv], _fold(v, cfg)[~cv])          # (kept cells: the input - spelled out)
    # the error map: 0 on kept tokens, the loss's row terms on masked ones (their mean over the masked tokens is the loss)
    ea, ev = res.err_a.cpu().numpy(), res.err_v.cpu().numpy()
    assert (ea[mask_a == 0] == 0).all() and (ev.reshape(B * T, Lv)[mask_v == 0] == 0).all() and (ea[mask_a == 1] > 0).all()
    np.testing.assert_allclose(ea.astype(np.float64).sum() / mask_a.sum(), float(res.loss_mae_a), rtol=1e-5)
    np.testing.assert_allclose(ev.astype(np.float64).sum() / mask_v.sum(), float(res.loss_mae_v), rtol=1e-5)
    assert eng.prune                                                      # compact rows: row_loss scattered by row_id, bit for bit
    for e, rl, pid, base in ((ea, eng.rl_a, eng.pid_a, 0), (ev, eng.rl_v, eng.pid_v, B * La)):
        want = np.zeros(e.size, dtype=np.float32)
        want[pid.cpu().numpy() - base] = rl.cpu().numpy()
        assert same_bits(e.reshape(-1), want)
    # the CPU oracle
    torch.set_num_threads(16)
    P = synth_state(cfg, 4321, "random", include_dead=False)
    extras = {}
    with torch.no_grad():
        ref_cpu.forward(P, cfg, a, v, plan, mae_loss_weight=1, contrast_loss_weight=0, extras=extras)
    ora_a = unpatchify_reference(extras["pred_a"].numpy().reshape(B, La, -1), a.numpy(), True, S, mask_a)
    ora_v = unpatchify_reference(extras["pred_v"].numpy().reshape(B * T, Lv, -1), _fold(v, cfg), False, S, mask_v)
    ra, rv = _masked_rel_l2(got_a, ora_a, ca), _masked_rel_l2(got_v, ora_v, cv)
    print(f"inpaint {name}: masked-cell relative L2 against the oracle: audio {ra:.3e} frames {rv:.3e}")
    assert ra < ORACLE_REL_L2 and rv < ORACLE_REL_L2, (ra, rv)


def test_inpaint_against_the_reference_golden():
    """m_w1_b4 (the unmodified reference, full ViT-B shape): the masked-cell L2 of each reconstruction within the oracle bound of the reference's"""
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.weights import synth_inputs
    from tests.helpers import golden_plan, load_golden, sample_positions
    g, base = load_golden("inp_m_w1_b4"), load_golden("m_w1_b4")
    cfg = AVSiamConfig()
    B = int(base["batch"])
    a, v = synth_inputs(cfg, B, int(base["input_seed"]), None)
    m = _model(cfg, int(base["weight_seed"]))
    res = m.inpaint(a.cuda(), v.cuda(), mask_plan=golden_plan(base))
    assert np.array_equal(res.mask_a.cpu().numpy(), base["mask_a"]) and np.array_equal(res.mask_v.cpu().numpy(), base["mask_v"])
    for k, got, mask, audio in (("recon_a", res.audio.cpu().numpy(), base["mask_a"], True), ("recon_v", res.imgs.cpu().numpy(), base["mask_v"], False)):
        cells = _cells(mask, got.shape, audio, 16)
        assert int(cells.sum()) == int(g[k + "_masked_cells"])
        l2 = float(np.linalg.norm(got.astype(np.float64)[cells]))
        print(f"inpaint golden {k}: masked-cell L2 {l2:.6f} (reference {float(g[k + '_masked_l2']):.6f})")
        assert abs(l2 - g[k + "_masked_l2"]) < ORACLE_REL_L2 * g[k + "_masked_l2"]
        # the sampled cells the reference recorded that are KEPT cells are the input: exactly the reference's input * 1 + recon * 0
        pos = sample_positions(k, got.size, 64)
        kept = ~cells.reshape(-1)[pos]
        assert kept.any() and np.array_equal(got.reshape(-1)[pos].astype(np.float64)[kept], g[k + "_samples"][kept])


def test_every_patch_from_the_decoder_needs_every_row():
    """EngineOptions(prune_dead=False), paste_kept=False: the full reconstruction is unpatchify_reference of ALL predictions, bit for bit; with
    pruning on that call raises and says why"""
    from avsiam_amd.config import EngineOptions
    from avsiam_amd.maskplan import make_mae_plan
    from avsiam_amd.preprocess import unpatchify_reference
    cfg, B = _cfg("b2_t3")
    S, T, Lv = cfg.st, cfg.frames, cfg.video_tokens
    a, v = _inputs(cfg, B)
    plan = make_mae_plan(cfg, B, torch.Generator().manual_seed(7))
    m = _model(cfg, options=EngineOptions(prune_dead=False))
    res = m.inpaint(a.cuda(), v.cuda(), mask_plan=plan, paste_kept=False)
    eng = m._engine("mae", B)
    assert not eng.prune
    pa, pv = (p.numpy() for p in eng.predictions())
    assert np.isfinite(pa).all() and np.isfinite(pv).all()
    assert same_bits(res.audio.cpu().numpy(), unpatchify_reference(pa, a.numpy(), True, S, None))
    assert same_bits(_fold(res.imgs, cfg), unpatchify_reference(pv.reshape(B * T, Lv, -1), _fold(v, cfg), False, S, None))
    mp_ = _model(cfg)
    assert mp_.options.prune_dead
    with pytest.raises(ValueError, match="prune_dead"):
        mp_.inpaint(a.cuda(), v.cuda(), mask_plan=plan, paste_kept=False)


def test_region_plan_through_inpaint():
    from avsiam_amd import maskplan as mp
    cfg, B = _cfg("b2_t3")
    S, T, Lv = cfg.st, cfg.frames, cfg.video_tokens
    a, v = _inputs(cfg, B)
    span, box = mp.audio_time_span(cfg, 40, 100), mp.frame_box(cfg, 100, 20, 180, 90)
    plan = mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(3), span, box)
    m = _model(cfg)
    res = m.inpaint(a.cuda(), v.cuda(), mask_plan=plan)
    ma, mv = res.mask_a.cpu(), res.mask_v.cpu().reshape(B, T, Lv)
    assert bool((ma[:, span] == 1).all()) and bool((mv[..., box] == 1).all())
    assert int(ma.sum()) == B * (cfg.audio_tokens - cfg.keep_a) and int(mv.sum()) == B * T * (Lv - cfg.keep_v)
    got_a, got_v = res.audio.cpu().numpy(), _fold(res.imgs, cfg)
    ca, cv = _cells(ma.numpy(), a.shape, True, S), _cells(mv.reshape(B * T, Lv).numpy(), got_v.shape, False, S)
    assert same_bits(got_a[~ca], a.numpy()[~ca]) and same_bits(got_v[~cv], _fold(v, cfg)[~cv])          # differs from the input only on masked cells
    assert (got_a[ca] != a.numpy()[ca]).mean() > 0.99 and (got_v[cv] != _fold(v, cfg)[cv]).mean() > 0.99
    assert ca[:, 40:100].all() and cv[:, :, 100:180, 20:90].all()                                        # the user's region is inside the masked cells


def test_inpaint_raw_inputs_and_argument_errors():
    """raw inputs through the model: kept cells come back as the original fbank (to the float32 restatement) and the original uint8 exactly"""
    from avsiam_amd.preprocess import normalize_fbank, unnormalize_reference
    cfg, B = _cfg("b4_t1")
    a, v = _inputs(cfg, B)
    fb = (a * STD_A + MEAN_A).cuda()
    u8 = (v * 0.25 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8).cuda()
    xf = (ops().InputXf.audio(MEAN_A, STD_A), ops().InputXf.frames())
    m = _model(cfg)
    res = m.inpaint(fb, u8, input_xf=xf, raw=True)                       # a plan drawn on the device
    assert res.imgs.dtype == torch.uint8 and res.imgs.shape == u8.shape and res.audio.dtype == torch.float32
    ca = _cells(res.mask_a.cpu().numpy(), a.shape, True, 16)
    cv = _cells(res.mask_v.cpu().numpy(), u8.shape, False, 16)
    assert int(res.mask_a.sum()) == B * (cfg.audio_tokens - cfg.keep_a)
    assert np.array_equal(res.imgs.cpu().numpy()[~cv], u8.cpu().numpy()[~cv])
    seen = normalize_fbank(fb, MEAN_A, STD_A).cpu().numpy()
    assert same_bits(res.audio.cpu().numpy()[~ca], unnormalize_reference(seen, MEAN_A, STD_A, True)[~ca])
    norm = m.inpaint(fb, u8, input_xf=xf)                                # model units from raw inputs
    assert norm.imgs.dtype == torch.float32 and same_bits(norm.audio.cpu().numpy()[~_cells(norm.mask_a.cpu().numpy(), a.shape, True, 16)],
                                                          seen[~_cells(norm.mask_a.cpu().numpy(), a.shape, True, 16)])
    with pytest.raises(ValueError, match="raw"):
        m.inpaint(a.cuda(), v.cuda(), raw=True)                          # raw without input_xf
    shift, amp = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV)
    with pytest.raises(ValueError, match="shift / amp"):
        m.inpaint(fb, u8, input_xf=(ops().InputXf.audio(MEAN_A, STD_A, shift, amp, seed=1), xf[1]), raw=True)
    with pytest.raises(ValueError, match="audio must be"):
        m.inpaint(a[:, :100].cuda(), v.cuda())
    with pytest.raises(TypeError):
        m.inpaint(a.cuda(), v.cuda(), mask_plan={"mae": None})


def test_training_is_undisturbed_by_inpaint():
    """deterministic=True: two training steps (device-drawn plans) with an inpaint() call - itself with a device-drawn plan - between them leave the
    weights and both Adam moments bit-identical to two steps without it"""
    from avsiam_amd.config import AVSiamConfig, EngineOptions
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.param_spec import P1, P2
    from avsiam_amd.traintest_cavmae_base import train_step
    cfg = AVSiamConfig(audio_tokens=128, frames=1, depth=2)
    B = 3
    a, v = _inputs(cfg, B, 17)
    a, v = a.cuda(), v.cuda()

    def run(look):
        m = CAVMAE_BASE(cfg=cfg, init_seed=4, init_mode="random", verbose=False, plan_seed=33, options=EngineOptions(deterministic=True)).cuda()
        m.publish_grads = False
        losses = [train_step(m, a, v, 2e-4)[0].item()]
        if look:
            res = m.inpaint(a, v)
            assert bool(torch.isfinite(res.audio).all())
        losses.append(train_step(m, a, v, 2e-4)[0].item())
        torch.cuda.synchronize()
        return m, losses

    m0, l0 = run(False)
    m1, l1 = run(True)
    assert l0 == l1, (l0, l1)
    assert torch.equal(m0.arena.p, m1.arena.p)
    for w in (P1, P2):
        assert torch.equal(m0._opt_state[w]["m"], m1._opt_state[w]["m"]) and torch.equal(m0._opt_state[w]["v"], m1._opt_state[w]["v"])
        assert m0._opt_state[w]["step"] == m1._opt_state[w]["step"] == 2


def test_inpaint_counts_as_a_forward_of_the_mae_pass():
    """shared activation pool: a contrastive forward after inpaint() owns the pool - reconstruct() of the MAE engine then refuses, by the check
    backward() already makes (no second bookkeeping)"""
    cfg, B = _cfg("b4_t1")
    a, v = _inputs(cfg, B)
    m = _model(cfg, share_pass_buffers=True)
    m.inpaint(a.cuda(), v.cuda())
    eng = m._engine("mae", B)
    assert eng.pool is not None and eng.pool.owner is eng
    eng.reconstruct()                                                    # still this pass's activations
    with torch.no_grad():
        m(a.cuda(), v.cuda(), mae_loss_weight=0, contrast_loss_weight=1)
    with pytest.raises(RuntimeError, match="another pass ran its forward"):
        eng.reconstruct()


def test_cli_writes_reconstructions(tmp_path):
    out = tmp_path / "recon"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "avsiam_amd.inpaint", "--synthetic", "2", "--depth", "2", "--mask-time", "256", "512", "--mask-box", "0", "0", "112", "112",
                        "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = np.load(out / "recon.npz")
    assert {"audio", "imgs", "recon_audio", "recon_imgs", "mask_a", "mask_v", "err_a", "err_v", "loss_mae_a", "loss_mae_v"} <= set(d.files)
    a, v, ra, rv, ma, mv = (d[k] for k in ("audio", "imgs", "recon_audio", "recon_imgs", "mask_a", "mask_v"))
    assert a.shape == ra.shape == (2, 1024, 128) and v.shape == rv.shape == (2, 3, 224, 224) and ma.shape == (2, 512) and mv.shape == (2, 196)
    assert (ma.sum(1) == 384).all() and (mv.sum(1) == 147).all()
    ca, cv = _cells(ma, a.shape, True, 16), _cells(mv, v.shape, False, 16)
    assert ca[:, 256:512].all() and cv[:, :, :112, :112].all()
    assert same_bits(ra[~ca], a[~ca]) and same_bits(rv[~cv], v[~cv])                                     # kept cells: the input, bit for bit
    assert (ra[ca] != a[ca]).mean() > 0.99 and np.isfinite(ra).all() and np.isfinite(rv).all()
    np.testing.assert_allclose(d["err_a"].astype(np.float64).sum() / ma.sum(), float(d["loss_mae_a"]), rtol=1e-5)
    np.testing.assert_allclose(d["err_v"].astype(np.float64).sum() / mv.sum(), float(d["loss_mae_v"]), rtol=1e-5)
