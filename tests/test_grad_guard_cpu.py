"""The guard of the fine-tuning step without a GPU: ops.grad_guard_reference - the numpy restatement the GPU tests hold avs_grad_sumsq to -
against torch.nn.utils.clip_grad_norm_ itself, its edge cases, and the launcher's flags."""
import math

import numpy as np
import pytest
import torch

from avsiam_amd.ops import grad_guard_reference

REL = 1e-12


def _params(seed, sizes, scale):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in sizes]
    for p in ps:
        p.grad = torch.randn(p.numel(), generator=g, dtype=torch.float64) * scale
    return ps


def _table(sizes):
    """the parameters laid end to end with a 4-element gap behind each, groups and classes interleaved"""
    segs, at = [], 4
    for i, n in enumerate(sizes):
        segs.append((at, n, i % 3, (2 * i) % 5))
        at += n + 4
    return segs, at


@pytest.mark.parametrize("max_norm,clips", [(0.5, True), (1e6, False)])
def test_reference_matches_clip_grad_norm(max_norm, clips):
    sizes = [4, 64, 4096, 4100, 12]
    ps = _params(1, sizes, 0.3)
    segs, total = _table(sizes)
    flat = np.zeros(total)
    for (lo, n, _, _), p in zip(segs, ps):
        flat[lo:lo + n] = p.grad.numpy()
    ref = grad_guard_reference(flat, segs, [1.0] * 5, grad_scale=1.0, max_norm=max_norm)
    want = [p.grad.clone() for p in ps]
    norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    # norm64 / coef64: the same formulas before the device block's fp32 roundings - what torch computes on float64 parameters
    assert abs(ref["norm64"] - norm) <= REL * norm
    assert (ref["coef64"] < 1.0) == clips and (ref["coef"] < 1.0) == clips
    for p, g0 in zip(ps, want):
        assert float((g0 * ref["coef64"] - p.grad).abs().max()) <= REL * float(p.grad.abs().max())
    # the device block's fp32 fields: norm one rounding of norm64, coef the literal fp32 formula (an add, a divide: two more roundings)
    assert abs(ref["norm"] - ref["norm64"]) <= 2.0 ** -24 * ref["norm64"]
    assert abs(ref["coef"] - ref["coef64"]) <= 3 * 2.0 ** -24 * ref["coef64"]
    assert ref["skip"] == 0 and ref["n_nonfinite"] == 0
    for grp in range(3):                                   # per group and per class: the same elements, exactly rounded
        w = math.fsum(float(x) ** 2 for (_, _, g_, _), g0 in zip(segs, want) if g_ == grp for x in g0.tolist())
        assert abs(ref["sumsq"][grp] - w) <= REL * w
    for cls in range(5):
        w = math.fsum(float(x) ** 2 for (_, _, _, c), g0 in zip(segs, want) if c == cls for x in g0.tolist())
        assert abs(ref["sumsq_cls"][cls] - w) <= REL * max(w, 1e-300)


def test_inf_max_norm_and_zero_gradients_give_coef_one():
    segs = [(0, 8, 0, 0), (8, 8, 2, 1)]
    g = np.linspace(-3, 3, 16).astype(np.float32)
    r = grad_guard_reference(g, segs, [1, 1], max_norm=float("inf"))
    assert r["coef"] == 1.0 and r["skip"] == 0 and r["norm"] > 0
    z = grad_guard_reference(np.zeros(16, np.float32), segs, [1, 1], max_norm=0.25)
    assert z["coef"] == 1.0 and z["norm"] == 0.0 and z["total"] == 0.0
    z = grad_guard_reference(np.zeros(16, np.float32), segs, [1, 1], max_norm=1e-9)        # even a bound below the 1e-6 of the formula
    assert 0 < z["coef"] < 1.0 and z["coef"] == float(np.float32(1e-9) / np.float32(1e-6))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_element_skips_and_leaves_the_finite_sum(bad):
    segs = [(0, 8, 0, 0), (8, 8, 1, 1)]
    g = np.arange(16, dtype=np.float32) / 8
    clean = grad_guard_reference(g, segs, [1, 1], max_norm=1.0)
    g2 = g.copy()
    g2[11] = bad
    r = grad_guard_reference(g2, segs, [1, 1], max_norm=1.0)
    assert r["skip"] == 1 and r["n_nonfinite"] == 1 and r["coef"] == 0.0
    gone = float(g[11]) ** 2
    assert r["sumsq"][0] == clean["sumsq"][0] and r["sumsq"][1] == clean["sumsq"][1] - gone
    assert r["sumsq_cls"][1] == clean["sumsq_cls"][1] - gone and math.isfinite(r["norm"])


def test_dead_classes_gaps_and_malformed_segments_change_nothing():
    g = np.full(64, np.nan, dtype=np.float32)
    g[4:12] = 0.5
    g[20:24] = 2.0
    segs = [(4, 8, 0, 0), (20, 4, 1, 2), (28, 8, 2, 1),                 # class 1 is dead and NaN-filled
            (40, 6, 0, 0), (46, 4, 0, 0), (48, 4, 3, 0), (52, 4, 0, 16), (56, 0, 0, 0), (-4, 4, 0, 0)]      # malformed: own nothing
    r = grad_guard_reference(g, segs, [1.0, 0.0, 2.0], max_norm=float("inf"))
    assert r["skip"] == 0 and r["n_nonfinite"] == 0
    assert r["sumsq"].tolist() == [2.0, 16.0, 0.0] and r["total"] == 18.0
    assert r["sumsq_cls"][:3].tolist() == [2.0, 0.0, 16.0] and r["norm"] == float(np.float32(math.sqrt(18.0)))
    half = grad_guard_reference(g, segs, [1.0, 0.0, 2.0], grad_scale=0.5, max_norm=1.0)
    assert half["total"] == 18.0 and half["norm"] == float(np.float32(math.sqrt(18.0) * 0.5))
    assert half["coef"] == float(np.float32(1.0) / (np.float32(half["norm"]) + np.float32(1e-6)))


def test_launcher_flags():
    from avsiam_amd.run_cavmae_ft_base import build_parser, main
    from avsiam_amd.traintest_ft_base import guard_diverged, guard_max_norm
    p = build_parser()
    assert guard_max_norm(p.parse_args([])) is None
    assert guard_max_norm(p.parse_args(["--skip-nonfinite"])) == float("inf")
    assert guard_max_norm(p.parse_args(["--clip-grad-norm", "2.5"])) == 2.5
    assert guard_max_norm(p.parse_args(["--clip-grad-norm", "2.5", "--skip-nonfinite"])) == 2.5
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit, match="clip-grad-norm"):
            main(["--ftmode", "mm_grad", "--clip-grad-norm", bad])
    assert not guard_diverged(0, 0) and not guard_diverged(10, 5) and guard_diverged(10, 6) and guard_diverged(1, 1)


def test_set_grad_guard_validates_without_a_gpu():
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    import dataclasses
    m = CAVMAEFT_BASE(8, cfg=dataclasses.replace(AVSiamConfig(), depth=2))
    assert m._guard_max is None and m.guard_stats() is None
    m.set_grad_guard()
    assert m._guard_max == float("inf")
    m.set_grad_guard(0.5)
    assert m._guard_max == 0.5
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            m.set_grad_guard(bad)
    m.set_grad_guard(None)
    assert m._guard_max is None
