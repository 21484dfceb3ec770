"""Reconstructions from the MAE pass, the parts that need no GPU: the numpy restatement of the unpatchify kernel against the oracle's patchify,
the oracle's reconstruction against the golden vectors of the unmodified reference (tools/gen_golden_inpaint.py), the region plans and their
helpers, and the argument errors of the command-line tool."""
import numpy as np
import pytest
import torch

from avsiam_amd import maskplan as mp
from avsiam_amd.config import AVSiamConfig, vit_huge14
from avsiam_amd.preprocess import unnormalize_reference, unpatchify_reference
from avsiam_amd.weights import synth_inputs, synth_state
from tests.helpers import golden_plan, load_golden, sample_positions


def _corner(rows, C, S):
    n, L = rows.shape[:2]
    return rows.reshape(n, L, 16, 16, C)[:, :, :S, :S].reshape(n, L, S * S * C)


# ---- 1. unpatchify_reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [16, 14])
def test_reference_frames_round_trip_through_the_oracles_patchify(stride):
    from oracle import ref_cpu
    rng = np.random.default_rng(stride)
    n, C, gy, gx = 2, 3, 2, 3
    H, W = gy * stride + (2 if stride == 14 else 0), gx * stride + (1 if stride == 14 else 0)       # stride 14: a rim no patch covers
    rows = rng.standard_normal((n, gy * gx, 256 * C)).astype(np.float32)
    base = rng.standard_normal((n, C, H, W)).astype(np.float32)
    before = base.copy()
    out = unpatchify_reference(rows, base, False, stride)
    assert out.dtype == np.float32 and out.shape == base.shape and np.array_equal(base, before)      # (the base is not written)
    back = ref_cpu.patchify(torch.from_numpy(out[:, :, :gy * stride, :gx * stride].copy()), C, gy, gx, stride).numpy()
    assert np.array_equal(back.view(np.uint32), _corner(rows, C, stride).view(np.uint32))          # bit for bit
    rim = np.ones(base.shape, dtype=bool)
    rim[:, :, :gy * stride, :gx * stride] = False
    assert np.array_equal(out[rim], base[rim])                                                       # the rest is untouched


@pytest.mark.parametrize("stride", [16, 14])
def test_reference_audio_round_trip_through_the_oracles_patchify(stride):
    """audio: the loss patchifies the TRANSPOSED spectrogram (cav_mae_base.py:666-668) - token f * tP + t, element p * 16 + q <-> cell (t S + q, f S + p)"""
    from oracle import ref_cpu
    rng = np.random.default_rng(3 + stride)
    n, tP, fP = 2, 4, 2
    T, F = tP * stride, fP * stride + (2 if stride == 14 else 0)                                     # stride 14: the last two mel bins are uncovered
    rows = rng.standard_normal((n, tP * fP, 256)).astype(np.float32)
    base = rng.standard_normal((n, T, F)).astype(np.float32)
    out = unpatchify_reference(rows, base, True, stride)
    img = torch.from_numpy(out[:, :, :fP * stride].copy()).unsqueeze(1).transpose(2, 3)              # [n, 1, F, T]
    back = ref_cpu.patchify(img, 1, fP, tP, stride).numpy()
    assert np.array_equal(back.view(np.uint32), _corner(rows, 1, stride).view(np.uint32))
    assert np.array_equal(out[:, :, fP * stride:], base[:, :, fP * stride:])
    # one cell by hand: token (f 1, t 2), element (p 3, q 5)
    assert out[1, 2 * stride + 5, 1 * stride + 3] == rows[1, 1 * tP + 2, 3 * 16 + 5]


def test_reference_mask_selects_tokens_and_keeps_the_rest():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((2, 4, 768)).astype(np.float32)
    rows[0, 1] = np.nan                                                                              # a row nobody predicted (pruned decoder)
    base = rng.standard_normal((2, 3, 32, 32)).astype(np.float32)
    mask = np.array([[1, 0, 0, 1], [0, 0, 0, 0]], dtype=np.float32)
    out = unpatchify_reference(rows, base, False, 16, mask)
    assert np.array_equal(out[1], base[1]) and np.array_equal(out[0, :, :16, 16:], base[0, :, :16, 16:]) and np.isfinite(out).all()
    assert out[0, 2, 3, 5] == rows[0, 0, (3 * 16 + 5) * 3 + 2] and out[0, 1, 16 + 7, 16 + 2] == rows[0, 3, (7 * 16 + 2) * 3 + 1]
    with pytest.raises(ValueError):
        unpatchify_reference(rows[:, :3], base, False, 16)


def test_unnormalize_reference_rounds_and_clamps():
    x = np.zeros((1, 3, 1, 4), dtype=np.float32)
    x[0, :, 0] = [-10.0, 0.0, 10.0, 0.3]
    m, s = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u = unnormalize_reference(x, m, s, False)
    assert u.dtype == np.uint8 and list(u[0, 0, 0]) == [0, 124, 255, int(np.rint((np.float32(0.3) * np.float32(0.229) + np.float32(0.485)) * np.float32(255)))]
    a = unnormalize_reference(np.float32([1.5]), -5.081, 4.4849, True)
    assert a.dtype == np.float32 and a[0] == np.float32(1.5) * np.float32(4.4849) + np.float32(-5.081)


# ---- 2. the oracle's reconstruction against the reference's -------------------------------------------------------------------------------------
def test_oracle_reconstruction_matches_reference_golden():
    """ref_cpu.forward predictions -> unpatchify_reference -> compose, against the reference class's own unpatchify and
    input * (1 - mask) + recon * mask (tools/gen_golden_inpaint.py).  Bounds: those tests/test_oracle_golden.py puts on the same predictions."""
    from oracle import ref_cpu
    torch.set_num_threads(8)
    g, base = load_golden("inp_m_w1_b4"), load_golden("m_w1_b4")
    cfg = AVSiamConfig()
    B = int(base["batch"])
    a, v = synth_inputs(cfg, B, int(base["input_seed"]), None)
    P = synth_state(cfg, int(base["weight_seed"]), "random")
    plan = golden_plan(base)
    extras = {}
    with torch.no_grad():
        out = ref_cpu.forward(P, cfg, a, v, plan, mae_loss_weight=1, contrast_loss_weight=0, extras=extras)
    for k, inp, pred, mask, audio in (("recon_a", a, extras["pred_a"], out[5], True), ("recon_v", v, extras["pred_v"], out[6], False)):
        rows = pred.numpy().reshape(B, mask.shape[1], -1)
        rec = unpatchify_reference(rows, inp.numpy(), audio, 16, mask.numpy())
        flat = rec.astype(np.float64).reshape(-1)
        assert abs(np.linalg.norm(flat) - g[k + "_l2"]) <= 1e-5 * g[k + "_l2"]
        s = np.array([flat[i] for i in sample_positions(k, flat.size, 64)])
        np.testing.assert_allclose(s, g[k + "_samples"], rtol=1e-4, atol=1e-5)
        only = unpatchify_reference(rows, np.zeros_like(inp.numpy()), audio, 16, mask.numpy()).astype(np.float64)
        assert abs(np.linalg.norm(only) - g[k + "_masked_l2"]) <= 1e-5 * g[k + "_masked_l2"]
        cells = unpatchify_reference(np.ones_like(rows), np.zeros_like(inp.numpy()), audio, 16, mask.numpy())
        assert int(cells.sum()) == int(g[k + "_masked_cells"])


# ---- 3. region plans --------------------------------------------------------------------------------------------------------------------------
CFGS = {"base": AVSiamConfig(audio_tokens=128, frames=2), "huge14": vit_huge14(frames=2, depth=2)}


@pytest.mark.parametrize("name", ["base", "huge14"])
def test_region_plan_masks_what_it_must_and_keeps_the_counts(name):
    cfg = CFGS[name]
    B, T, La, Lv = 3, cfg.frames, cfg.audio_tokens, cfg.video_tokens
    must_a = (mp.audio_time_span(cfg, 20, 50) | mp.audio_mel_band(cfg, 0, 5)).repeat(B, 1)
    must_a[2] = False                                                                                # a sample with nothing forced
    must_v = torch.zeros(B, T, Lv, dtype=torch.bool)
    must_v[0, 0] = mp.frame_box(cfg, 0, 0, 100, 100)
    must_v[1, 1] = mp.frame_box(cfg, 200, 10, 224, 60)
    plan = mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(11), must_a, must_v)
    ma, mv = plan.mask_a(), plan.mask_v()
    assert ma.shape == (B, La) and mv.shape == (B, T, Lv)
    assert bool((ma[must_a] == 1).all()) and bool((mv[must_v] == 1).all())                           # every forced patch is masked
    assert torch.equal(ma.sum(1), torch.full((B,), float(La - cfg.keep_a)))                          # exactly L - keep, per sample ...
    assert torch.equal(mv.sum(-1), torch.full((B, T), float(Lv - cfg.keep_v)))                       # ... and frame
    assert torch.equal(plan.ids_restore_a.sort(1).values, torch.arange(La).expand(B, La))            # permutations
    assert torch.equal(plan.ids_restore_v.sort(-1).values, torch.arange(Lv).expand(B, T, Lv))
    assert plan.ids_keep_a.shape == (B, cfg.keep_a) and plan.ids_keep_v.shape == (B, T, cfg.keep_v)
    assert bool((torch.gather(ma, 1, plan.ids_keep_a) == 0).all()) and bool((torch.gather(mv, 2, plan.ids_keep_v) == 0).all())
    again = mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(11), must_a, must_v)      # the same generator state: the same plan
    assert all(torch.equal(getattr(plan, f), getattr(again, f)) for f in ("ids_keep_a", "ids_restore_a", "ids_keep_v", "ids_restore_v"))
    other = mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(12), must_a, must_v)
    assert not torch.equal(plan.ids_restore_a, other.ids_restore_a)                                   # the remainder is random
    # nothing forced: make_mae_plan's plan, draw for draw
    p0, p1 = mp.make_mae_plan(cfg, B, torch.Generator().manual_seed(5)), mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(5))
    assert torch.equal(p0.ids_restore_a, p1.ids_restore_a) and torch.equal(p0.ids_restore_v, p1.ids_restore_v)
    # one sequence's worth broadcasts over the batch and the frames
    bc = mp.make_mae_plan_regions(cfg, B, torch.Generator().manual_seed(11), mp.audio_time_span(cfg, 20, 50), mp.frame_box(cfg, 0, 0, 30, 30))
    assert bool((bc.mask_a()[:, mp.audio_time_span(cfg, 20, 50)] == 1).all()) and bool((bc.mask_v()[..., mp.frame_box(cfg, 0, 0, 30, 30)] == 1).all())


def test_region_plan_over_quota_names_the_sample_and_the_counts():
    cfg = CFGS["base"]                                                                               # La 128 keeps 32: at most 96 forced; Lv 196 keeps 49: 147
    must_a = torch.zeros(3, 128, dtype=torch.bool)
    must_a[1, :97] = True
    with pytest.raises(ValueError, match=r"audio, sample 1: 97 patches .* 96 of 128"):
        mp.make_mae_plan_regions(cfg, 3, torch.Generator().manual_seed(0), must_a)
    must_a[1, 96] = False                                                                            # exactly the quota: every masked patch is a forced one
    plan = mp.make_mae_plan_regions(cfg, 3, torch.Generator().manual_seed(0), must_a)
    assert torch.equal(plan.mask_a()[1].bool(), must_a[1])
    must_v = torch.zeros(3, 2, 196, dtype=torch.bool)
    must_v[2, 1, :148] = True
    with pytest.raises(ValueError, match=r"frames, sample 2, frame 1: 148 patches .* 147 of 196"):
        mp.make_mae_plan_regions(cfg, 3, torch.Generator().manual_seed(0), None, must_v)
    with pytest.raises(ValueError, match="bool"):
        mp.make_mae_plan_regions(cfg, 3, torch.Generator().manual_seed(0), must_a.float())
    with pytest.raises(ValueError, match="broadcast"):
        mp.make_mae_plan_regions(cfg, 3, torch.Generator().manual_seed(0), must_a[:2])


def test_region_helpers_at_patch_boundaries():
    cfg = CFGS["base"]                                                                               # 16 time patches x 8 mel patches (256 x 128 cells), 14 x 14 frame patches of 16
    t = lambda m: sorted(set((torch.nonzero(m).reshape(-1) % cfg.audio_t).tolist()))                 # noqa: E731  time patches hit
    f = lambda m: sorted(set((torch.nonzero(m).reshape(-1) // cfg.audio_t).tolist()))                # noqa: E731  mel patches hit
    assert t(mp.audio_time_span(cfg, 16, 32)) == [1] and f(mp.audio_time_span(cfg, 16, 32)) == list(range(8))
    assert t(mp.audio_time_span(cfg, 15, 32)) == [0, 1] and t(mp.audio_time_span(cfg, 16, 33)) == [1, 2] and t(mp.audio_time_span(cfg, 31, 32)) == [1]
    assert t(mp.audio_time_span(cfg, 250, 256)) == [15] and t(mp.audio_time_span(cfg, 250, 500)) == [15]        # the last range, clipped
    assert f(mp.audio_mel_band(cfg, 0, 16)) == [0] and f(mp.audio_mel_band(cfg, 0, 17)) == [0, 1] and f(mp.audio_mel_band(cfg, 127, 128)) == [7]
    assert int(mp.audio_mel_band(cfg, 16, 48).sum()) == 2 * cfg.audio_t
    box = mp.frame_box(cfg, 16, 32, 32, 64).reshape(14, 14)
    assert torch.nonzero(box).tolist() == [[1, 2], [1, 3]]
    assert torch.nonzero(mp.frame_box(cfg, 15, 31, 17, 33).reshape(14, 14)).tolist() == [[0, 1], [0, 2], [1, 1], [1, 2]]
    assert torch.nonzero(mp.frame_box(cfg, 208, 208, 224, 224).reshape(14, 14)).tolist() == [[13, 13]]
    for bad in ((32, 32), (40, 30), (-1, 5), (256, 270)):
        with pytest.raises(ValueError):
            mp.audio_time_span(cfg, *bad)
    with pytest.raises(ValueError):
        mp.frame_box(cfg, 0, 224, 10, 230)


def test_region_helpers_at_stride_14():
    cfg = CFGS["huge14"]                                                                             # 73 time x 9 mel patches of 14; 16 x 16 frame patches of 14
    assert cfg.st == 14 and cfg.audio_t == 73 and cfg.audio_f == 9 and cfg.grid == 16
    m = mp.audio_time_span(cfg, 14, 28).reshape(9, 73)
    assert torch.nonzero(m[0]).reshape(-1).tolist() == [1] and bool(m.all(0)[1])
    assert torch.nonzero(mp.audio_time_span(cfg, 13, 29).reshape(9, 73)[0]).reshape(-1).tolist() == [0, 1, 2]
    assert torch.nonzero(mp.audio_time_span(cfg, 1010, 1024).reshape(9, 73)[0]).reshape(-1).tolist() == [72]      # 1022 frames are covered: clipped
    with pytest.raises(ValueError):
        mp.audio_time_span(cfg, 1022, 1024)                                                          # wholly outside what the patches cover
    assert torch.nonzero(mp.audio_mel_band(cfg, 112, 128).reshape(9, 73)[:, 0]).reshape(-1).tolist() == [8]       # bins 126, 127 belong to no patch
    assert torch.nonzero(mp.frame_box(cfg, 13, 14, 14, 29).reshape(16, 16)).tolist() == [[0, 1], [0, 2]]


# ---- 4. the command-line tool's argument errors (all before anything touches a GPU) --------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["--synthetic", "2"], None),                                                                    # --out is required
    (["--out", "x", "--mask-time", "5"], None),                                                      # two numbers
    (["--out", "x", "--mask-box", "0", "0", "10"], None),
    (["--out", "x", "--model", "no-such-model"], None),
    (["--out", "x", "--mask-time", "300", "100"], "not a range"),
    (["--out", "x", "--mask-mel", "128", "140"], "outside"),
    (["--out", "x", "--mask-time", "0", "1024"], "must be masked"),                                  # more than the 75 % the model removes
    (["--out", "x", "--synthetic", "0"], "at least one clip"),
])
def test_cli_argument_errors(argv, msg, capsys, tmp_path):
    from avsiam_amd import inpaint
    argv = [str(tmp_path / a) if a == "x" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        inpaint.main(argv)
    assert e.value.code not in (0, None)
    if msg is not None:
        assert msg in str(e.value.code)
    assert not (tmp_path / "x").exists()
    assert "--mask-time" in inpaint.build_parser().format_help() and "--raw-input" in inpaint.build_parser().format_help()
