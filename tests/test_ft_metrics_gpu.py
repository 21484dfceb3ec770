"""avs_cls_stats on the MI355X: exact integer counts against int64 numpy on tie-ridden inputs at every shape where the kernel takes another
path (one sample, a score tile plus one, several class tiles, a chunk of positives plus one, one positive, all but one), strided and multi-set
inputs, the reference's recorded sklearn results (tests/golden/ftm_*.npz), degenerate classes, NaN input, determinism, and the fine-tuning
loop's validate / evaluate_frames on the device path.  The float64 counting restatement lives in tests/test_ft_metrics_cpu.py, where it is
checked against the same goldens without a GPU."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import load_golden, record_margin
from tests.test_ft_metrics_cpu import CASES, counting_stats

pytestmark = pytest.mark.gpu

KEYS = ("n_pos", "auc_num", "ap_sum", "n_correct", "n_nonfinite")


def _lattice(rng, *shape):
    """scores on 8 levels: every class is full of ties, between positives, between negatives and across the two"""
    return (rng.integers(0, 8, shape) / 8.0).astype(np.float32)


def _check_exact(scores, target, dev_scores=None, dev_target=None):
    """scores [S, N, C] / target [N, C] numpy; the device tensors default to their dense copies"""
    from avsiam_amd import ops
    S, N, C = scores.shape
    ds = torch.from_numpy(scores).cuda() if dev_scores is None else dev_scores
    dt = torch.from_numpy(target).cuda() if dev_target is None else dev_target
    res = ops.classification_stats(ds, dt)
    got = {k: res[k].cpu().numpy() for k in KEYS}
    for k in KEYS:
        assert got[k].shape == ((S, C) if k in KEYS[:3] else (S,)), (k, got[k].shape)
    assert got["n_pos"].dtype == np.int32 and got["auc_num"].dtype == np.int64 and got["ap_sum"].dtype == np.float64
    for s in range(S):
        ref = counting_stats(scores[s], target)
        assert np.array_equal(got["n_pos"][s], ref["n_pos"])
        assert np.array_equal(got["auc_num"][s], ref["auc_num"]), (s, got["auc_num"][s], ref["auc_num"])
        assert int(got["n_correct"][s]) == ref["n_correct"]
        assert int(got["n_nonfinite"][s]) == 0
        # P terms of at most 1, one rounding each, added in another order than numpy's; the factor 4 is slack
        bound = ref["n_pos"] * 2.0 ** -52 * 4
        assert (np.abs(got["ap_sum"][s] - ref["ap_sum"]) <= bound).all(), (s, np.abs(got["ap_sum"][s] - ref["ap_sum"]).max())
    return got


def _shapes():
    from avsiam_amd import ops
    return [(1, 1), (ops.CLS_STATS_TILE + 1, 5), (257, 67)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_exact_counts_on_a_lattice(which):
    N, C = _shapes()[which]
    rng = np.random.default_rng(10 + which)
    target = (rng.random((N, C)) < 0.3).astype(np.float32)
    if N == 1:
        target[:] = 1.0
    _check_exact(_lattice(rng, 1, N, C), target)


def test_exact_counts_at_the_chunk_boundaries():
    """classes with P = positives-per-workgroup + 1 (a second chunk with one live lane), P = 1, P = N - 1, P = 2 chunks exactly and P = 0"""
    from avsiam_amd import ops
    N, C, W = 300, 5, ops.CLS_STATS_PPW
    rng = np.random.default_rng(20)
    target = np.zeros((N, C), np.float32)
    for k, P in enumerate((W + 1, 1, N - 1, 2 * W, 0)):
        target[rng.permutation(N)[:P], k] = 1.0
    got = _check_exact(_lattice(rng, 1, N, C), target)
    assert got["n_pos"][0].tolist() == [W + 1, 1, N - 1, 2 * W, 0]


def test_three_sets_and_strided_views():
    """S = 3 prediction sets against one target, dense and as views with padded rows (the class axis stays dense)"""
    N, C = 257, 67
    rng = np.random.default_rng(30)
    scores, target = _lattice(rng, 3, N, C), (rng.random((N, C)) < 0.2).astype(np.float32)
    dense = _check_exact(scores, target)
    buf = torch.full((3, N + 2, 80), float("nan"), device="cuda")
    buf[:, :N, :C] = torch.from_numpy(scores).cuda()
    tbuf = torch.full((N, 70), 1.0, device="cuda")
    tbuf[:, :C] = torch.from_numpy(target).cuda()
    view = _check_exact(scores, target, buf[:, :N, :C], tbuf[:, :C])
    for k in KEYS:
        assert np.array_equal(dense[k], view[k]), k
    # a 2-D input: [C] / 0-dim results, the values of set 0
    from avsiam_amd import ops
    one = ops.classification_stats(buf[1, :N, :C], tbuf[:, :C])
    assert one["n_pos"].shape == (C,) and one["n_correct"].dim() == 0
    for k in KEYS:
        assert np.array_equal(one[k].cpu().numpy(), dense[k][1]), k


def test_wrapper_refuses_what_the_kernel_must_not_see():
    from avsiam_amd import _lib, ops
    s, t = torch.zeros(4, 6, device="cuda"), torch.zeros(4, 6, device="cuda")
    for bad_s, bad_t in ((s.cpu(), t), (s.double(), t), (s[:, :5], t), (s.t().contiguous().t(), t), (torch.zeros(0, 6, device="cuda"), torch.zeros(0, 6, device="cuda")),
                         (torch.zeros(4, 2, 6, device="cuda").permute(1, 0, 2), t)):
        with pytest.raises(_lib.AvsiamHipError):
            ops.classification_stats(bad_s, bad_t)
    with pytest.raises(_lib.AvsiamHipError):
        ops.classification_stats(s, t, ws=torch.empty(16, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("case", CASES)
def test_reference_goldens(case):
    """per-class AP and auc within 1e-10 of sklearn's: both sides are float64 sums of at most 1 000 terms of at most 1 (a few P 1.1e-16, about
    1e-12, apart), and one misplaced rank or one ungrouped tie moves a class by at least 1 / (P N^2) >= 1e-8 at these shapes.
    The measured gaps are recorded with record_margin."""
    from avsiam_amd.traintest_ft_base import calculate_stats_device
    d = load_golden(case)
    stats = calculate_stats_device(torch.from_numpy(d["scores"]).cuda(), torch.from_numpy(d["target"]).cuda())
    ap, auc = np.array([s["AP"] for s in stats]), np.array([s["auc"] for s in stats])
    e_ap, e_auc = float(np.abs(ap - d["AP"]).max()), float(np.abs(auc - d["auc"]).max())
    print(f"{case}: max |AP - sklearn| = {e_ap:.3e}, max |auc - sklearn| = {e_auc:.3e}")
    record_margin("ft_metrics_" + case, ap_gap=e_ap, auc_gap=e_auc, bound=1e-10)
    assert e_ap <= 1e-10 and e_auc <= 1e-10
    assert all(s["acc"] == float(d["acc"]) for s in stats)


def test_degenerate_classes_follow_the_nan_convention():
    from avsiam_amd import ops
    from avsiam_amd.traintest_ft_base import calculate_stats, calculate_stats_device
    N, C = 50, 4
    rng = np.random.default_rng(40)
    scores = rng.random((N, C)).astype(np.float32)                                     # continuous: no ties, the two AP definitions agree
    assert all(len(np.unique(scores[:, k])) == N for k in range(C))
    target = (rng.random((N, C)) < 0.3).astype(np.float32)
    target[:, 0], target[:, 1] = 0.0, 1.0
    ds, dt = torch.from_numpy(scores).cuda(), torch.from_numpy(target).cuda()
    assert ops.classification_stats(ds, dt)["n_pos"].tolist()[:2] == [0, N]
    stats = calculate_stats_device(ds, dt)
    assert np.isnan(stats[0]["AP"]) and np.isnan(stats[0]["auc"])
    assert stats[1]["AP"] == 1.0 and np.isnan(stats[1]["auc"])
    host = calculate_stats(scores, target)
    for key in ("AP", "auc"):
        a, b = np.array([s[key] for s in stats]), np.array([s[key] for s in host])
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert abs(np.nanmean(a) - np.nanmean(b)) <= 1e-12                              # (float64 sums of <= 50 terms in two orders)
    assert stats[0]["acc"] == host[0]["acc"]


def test_nan_scores_are_counted_and_refused():
    from avsiam_amd import ops
    from avsiam_amd.traintest_ft_base import calculate_stats_device
    rng = np.random.default_rng(50)
    scores, target = _lattice(rng, 2, 70, 9), (rng.random((70, 9)) < 0.3).astype(np.float32)
    scores[1, 3, 2] = scores[1, 69, 8] = scores[1, 0, 0] = np.nan
    scores[1, 5, :] = np.nan                                                           # a row of nothing else
    ds, dt = torch.from_numpy(scores).cuda(), torch.from_numpy(target).cuda()
    res = ops.classification_stats(ds, dt)
    torch.cuda.synchronize()
    assert res["n_nonfinite"].tolist() == [0, 12]
    ref = counting_stats(scores[0], target)                                            # the clean set beside it is untouched
    assert np.array_equal(res["auc_num"][0].cpu().numpy(), ref["auc_num"]) and int(res["n_correct"][0]) == ref["n_correct"]
    with pytest.raises(ValueError, match="NaN"):
        calculate_stats_device(ds, dt)
    with pytest.raises(ValueError, match="NaN"):
        calculate_stats_device(ds[1], dt)
    assert len(calculate_stats_device(ds[0], dt)) == 9


def test_bytes_do_not_depend_on_the_call():
    from avsiam_amd import ops
    N, C = 700, 19
    rng = np.random.default_rng(60)
    scores = torch.sigmoid(torch.from_numpy(rng.standard_normal((3, N, C)).astype(np.float32) * 3)).cuda()
    target = torch.from_numpy((rng.random((N, C)) < 0.25).astype(np.float32)).cuda()
    a = ops.classification_stats(scores, target)
    b = ops.classification_stats(scores, target)
    assert torch.equal(a["packed"], b["packed"])
    for s in range(3):
        one = ops.classification_stats(scores[s], target)
        for k in KEYS:
            assert torch.equal(one[k].reshape(-1).view(torch.uint8), a[k][s].reshape(-1).view(torch.uint8)), (s, k)


def test_one_larger_case_against_the_counting_restatement():
    """N = 4 099 (two score tiles and three entries), C = 67 (two class tiles), continuous fp32 sigmoids; float64 sums of <= 4 099 terms of at
    most 1 differ by a few P 1.1e-16 < 1e-11 < the bound"""
    from avsiam_amd.traintest_ft_base import calculate_stats_device
    N, C = 4099, 67
    rng = np.random.default_rng(70)
    target = (rng.random((N, C)) < 0.03).astype(np.float32)
    target[:, 5] = (rng.random(N) < 0.6).astype(np.float32)                             # one class with many chunks of positives
    scores = torch.sigmoid(torch.from_numpy((rng.standard_normal((N, C)) * 2 + 2 * target).astype(np.float32))).numpy()
    stats = calculate_stats_device(torch.from_numpy(scores).cuda(), torch.from_numpy(target).cuda())
    ref = counting_stats(scores, target)
    e_ap = float(np.abs(np.array([s["AP"] for s in stats]) - ref["AP"]).max())
    e_auc = float(np.abs(np.array([s["auc"] for s in stats]) - ref["auc"]).max())
    record_margin("ft_metrics_4099x67", ap_gap=e_ap, auc_gap=e_auc, bound=1e-10)
    assert e_ap <= 1e-10 and e_auc <= 1e-10
    assert stats[0]["acc"] == ref["acc"]


def _close(stats, ref, tol=1e-10):
    for key in ("AP", "auc"):
        a = np.array([s[key] for s in stats])
        assert np.array_equal(np.isnan(a), np.isnan(ref[key])), key
        assert (np.abs(a - ref[key])[~np.isnan(a)] <= tol).all(), key
    assert all(s["acc"] == ref["acc"] for s in stats)


def test_validate_and_evaluate_frames_on_the_device_path(tmp_path):
    """2 batches of 4 ten-frame clips, 7 classes, mm_grad.  The synthetic loader repeats its batch, so every score occurs twice: ties."""
    from avsiam_amd.config import AVSiamConfig
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.traintest_ft_base import SyntheticFtLoader, evaluate_frames, validate
    L, F = 7, 10
    model = CAVMAEFT_BASE(L, init_seed=5, init_mode="random").cuda()
    loader = SyntheticFtLoader(AVSiamConfig(), 4, 2, L, model.arena.p.device, seed=9, frames=F)
    args = types.SimpleNamespace(ftmode="mm_grad", ftmode_test=None, loss="BCE", metrics="mAP", exp_dir=str(tmp_path), device_metrics=True)
    stats, out, target = validate(model, loader, None, args, output_pred=True)
    assert out.is_cuda and target.is_cuda and tuple(out.shape) == (8, F, L)
    _close(stats, counting_stats(out.mean(dim=1).cpu().numpy(), target.cpu().numpy()))
    _, loss_dev = validate(model, loader, None, args)
    args.device_metrics = False
    host_stats, loss_host = validate(model, loader, None, args)
    assert loss_dev == loss_host                                                        # the same forward, the same float
    assert len(host_stats) == L

    res = evaluate_frames(model, loader, args)
    assert len(res) == F + 1
    want = [float(np.nanmean(counting_stats(out[:, f].cpu().numpy(), target.cpu().numpy())["AP"])) for f in range(F)]
    want.append(float(np.nanmean(counting_stats(out.mean(dim=1).cpu().numpy(), target.cpu().numpy())["AP"])))
    assert np.abs(np.array(res) - np.array(want)).max() <= 1e-10
    assert np.array_equal(np.loadtxt(tmp_path / "mul_frame_res.csv", delimiter=","), np.array(res))
    args.metrics = "acc"
    acc = evaluate_frames(model, loader, args)
    assert acc == [counting_stats(out[:, f].cpu().numpy(), target.cpu().numpy())["acc"] for f in range(F)] + [counting_stats(out.mean(dim=1).cpu().numpy(), target.cpu().numpy())["acc"]]
