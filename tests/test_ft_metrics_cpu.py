"""Fine-tuning metrics without a GPU: the counting formulation (kept here in float64 numpy) against the reference's recorded results
(tests/golden/ftm_*.npz, written by tools/gen_golden_ft_metrics.py from the unmodified utilities/stats.py), the host half of the device path
(counts -> AP / auc / acc, the NaN convention, stats_summary), the C ABI of avs_cls_stats and the launcher's flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.helpers import ROOT, load_golden

CASES = ["ftm_a", "ftm_b", "ftm_c"]


def counting_stats(scores, target):
    """The sort-free definition the kernel implements, in numpy: per class over its positives i (target > 0.5)
        ap_sum = sum tp(s >= s_i) / cnt(s >= s_i)            AP = ap_sum / P
        auc_num = sum 2 neg(s < s_i) + neg(s == s_i)        auc = auc_num / (2 P Nn)
    counts in int64, the quotients and their sum (pairwise, numpy's) in float64; NaN where P = 0 (auc: or Nn = 0).
    n_correct: rows where the first-index argmax of the scores equals that of the binarised target."""
    s = np.asarray(scores)
    y = np.asarray(target) > 0.5
    N, C = s.shape
    out = {"n_pos": y.sum(0).astype(np.int64), "auc_num": np.zeros(C, np.int64), "ap_sum": np.zeros(C), "AP": np.full(C, np.nan), "auc": np.full(C, np.nan),
           "n_correct": int((np.argmax(y, 1) == np.argmax(s, 1)).sum())}
    for k in range(C):
        sk, pos, neg = s[:, k], s[y[:, k], k], s[~y[:, k], k]
        P, Nn = len(pos), len(neg)
        if P == 0:
            continue
        cnt_ge = (sk[None, :] >= pos[:, None]).sum(1, dtype=np.int64)
        tp_ge = (pos[None, :] >= pos[:, None]).sum(1, dtype=np.int64)
        lt = (neg[None, :] < pos[:, None]).sum(dtype=np.int64)
        eq = (neg[None, :] == pos[:, None]).sum(dtype=np.int64)
        out["auc_num"][k] = 2 * lt + eq
        out["ap_sum"][k] = (tp_ge / cnt_ge).sum()
        out["AP"][k] = out["ap_sum"][k] / P
        if Nn:
            out["auc"][k] = out["auc_num"][k] / (2.0 * P * Nn)
    out["acc"] = out["n_correct"] / N
    return out


@pytest.mark.parametrize("case", CASES)
def test_counting_restatement_reproduces_the_reference(case):
    d = load_golden(case)
    got = counting_stats(d["scores"], d["target"])
    e_ap, e_auc = np.abs(got["AP"] - d["AP"]).max(), np.abs(got["auc"] - d["auc"]).max()
    print(f"{case}: max |AP - sklearn| = {e_ap:.2e}, max |auc - sklearn| = {e_auc:.2e}")
    assert e_ap <= 1e-12 and e_auc <= 1e-12
    assert got["acc"] == float(d["acc"])


def test_goldens_cover_what_they_claim():
    a, b, c = (load_golden(n) for n in CASES)
    assert a["scores"].shape == (200, 10) and b["scores"].shape == (384, 12) and c["scores"].shape == (1000, 33)
    for d in (a, b, c):
        assert d["scores"].dtype == np.float32 and d["target"].dtype == np.float32 and d["AP"].dtype == np.float64 and d["auc"].dtype == np.float64
        P = (d["target"] > 0.5).sum(0)
        assert (P >= 1).all() and (P < len(d["target"])).all()
    assert all(len(np.unique(a["scores"][:, k])) == 200 for k in range(10))                  # a: no ties
    assert (b["target"].sum(1) == 1).all() and np.array_equal(np.unique(b["scores"] * 8), np.round(np.unique(b["scores"] * 8)))   # b: one-hot, lattice
    assert (c["scores"] == 0.0).any() and (c["scores"] == 1.0).any()                          # c: saturated sigmoids
    for n in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) < 200_000


def test_goldens_tell_the_two_ap_definitions_apart():
    """with ties the stable-sort AP of calculate_stats is not sklearn's: the goldens must see the difference (and agree where there are no ties)"""
    from avsiam_amd.traintest_ft_base import calculate_stats
    b = load_golden("ftm_b")
    host = calculate_stats(b["scores"], b["target"])
    assert np.abs(np.array([s["AP"] for s in host]) - b["AP"]).max() > 1e-6
    assert np.abs(np.array([s["auc"] for s in host]) - b["auc"]).max() <= 1e-12                # AUC is one definition
    a = load_golden("ftm_a")
    assert np.abs(np.array([s["AP"] for s in calculate_stats(a["scores"], a["target"])]) - a["AP"]).max() <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_stats_summary_matches_the_reference_d_prime(case):
    from avsiam_amd.traintest_ft_base import stats_summary
    d = load_golden(case)
    stats = [{"AP": float(p), "auc": float(u), "acc": float(d["acc"])} for p, u in zip(d["AP"], d["auc"])]
    s = stats_summary(stats)
    assert abs(s["d_prime"] - float(d["d_prime"])) <= 1e-9
    assert s["mAP"] == float(np.mean(d["AP"])) and s["mAUC"] == float(np.mean(d["auc"])) and s["acc"] == float(d["acc"])


def test_stats_summary_skips_nan_classes_and_guards_the_quantile():
    from avsiam_amd.traintest_ft_base import stats_summary
    s = stats_summary([{"AP": 0.5, "auc": 0.75, "acc": 0.25}, {"AP": float("nan"), "auc": float("nan"), "acc": 0.25}])
    assert s["mAP"] == 0.5 and s["mAUC"] == 0.75 and s["acc"] == 0.25 and np.isfinite(s["d_prime"])
    assert np.isnan(stats_summary([{"AP": 1.0, "auc": 1.0, "acc": 1.0}])["d_prime"])


def test_counts_to_stats_follow_the_nan_convention():
    """the host half of calculate_stats_device: P = 0 -> AP and auc NaN; Nn = 0 -> auc NaN, AP defined"""
    from avsiam_amd.traintest_ft_base import _stats_from_counts
    N = 10
    st = _stats_from_counts(np.array([0, 10, 4], np.int32), np.array([0, 0, 36], np.int64), np.array([0.0, 10.0, 3.0]), np.int32(7), N)
    assert np.isnan(st[0]["AP"]) and np.isnan(st[0]["auc"])
    assert st[1]["AP"] == 1.0 and np.isnan(st[1]["auc"])
    assert st[2]["AP"] == 0.75 and st[2]["auc"] == 36 / (2.0 * 4 * 6)
    assert all(s["acc"] == 0.7 for s in st)


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd import _lib
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def test_abi_declared_exported_and_constants_in_step(lib):
    from avsiam_amd import _lib, build, ops
    protos = _lib.parse_header()
    assert protos["avs_cls_stats"] == ("int", ["ptr", "ll", "ll", "int", "int", "int", "ptr", "ll"] + ["ptr"] * 6 + ["size", "ptr"])
    assert protos["avs_cls_stats_ws_bytes"] == ("size", ["int", "int", "int"])
    assert hasattr(lib, "avs_cls_stats") and hasattr(lib, "avs_cls_stats_ws_bytes")
    assert lib.avs_abi_version() == 2
    assert "metrics.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "metrics.hip")).read()
    assert int(re.search(r"#define CS_TILE (\d+)", src).group(1)) == ops.CLS_STATS_TILE
    assert int(re.search(r"#define CS_PPW (\d+)", src).group(1)) == ops.CLS_STATS_PPW
    # the class-major copy of the scores dominates: 4 S N C bytes, plus less than 2 N C words of lists and partials
    N, C = 20000, 527
    for S in (1, 11):
        need = lib.avs_cls_stats_ws_bytes(S, N, C)
        assert 4 * S * N * C < need < 4 * (S + 2) * N * C
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 22) + 1, 4), (65535, 4, 4)):
        assert lib.avs_cls_stats_ws_bytes(*bad) == 0


def test_argument_errors_before_any_launch(lib):
    one = ctypes.c_void_p(16)                      # any non-NULL value: the call must fail before touching it
    big = 1 << 40

    def call(scores=one, set_stride=32, row_stride=8, S=1, N=4, C=8, target=one, ldt=8, n_pos=one, auc=one, ap=one, ncor=one, nnf=one, ws=one,
             ws_bytes=big):
        rc = lib.avs_cls_stats(scores, set_stride, row_stride, S, N, C, target, ldt, n_pos, auc, ap, ncor, nnf, ws, ws_bytes, None)
        return rc, lib.avs_last_error()

    for kw, word in ((dict(N=0), b"positive"), (dict(C=0), b"positive"), (dict(S=0), b"positive"), (dict(N=-3), b"positive"),
                     (dict(N=(1 << 22) + 1), b"N ="), (dict(row_stride=7), b"row_stride"), (dict(ldt=7), b"ldt"),
                     (dict(S=2, set_stride=31), b"set_stride"), (dict(S=2, set_stride=8), b"set_stride"), (dict(scores=None), b"scores is NULL"),
                     (dict(target=None), b"target is NULL"), (dict(ap=None), b"output"), (dict(nnf=None), b"output"), (dict(ws=None), b"ws"),
                     (dict(ws_bytes=64), b"ws")):
        rc, msg = call(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    # S = 1 does not look at the set stride: that call gets past the stride checks (and then fails on the workspace, still before a launch)
    rc, msg = call(set_stride=0, ws_bytes=64)
    assert rc == -2 and b"ws" in msg


def test_launcher_flags():
    from avsiam_amd import run_cavmae_ft_base as run
    args = run.build_parser().parse_args([])
    assert args.device_metrics is False and args.eval_frames is False
    args = run.build_parser().parse_args(["--device-metrics", "--eval-frames"])
    assert args.device_metrics is True and args.eval_frames is True
    with pytest.raises(SystemExit) as e:            # refused before a model is built
        run.main(["--ftmode", "audioonly", "--eval-frames"])
    assert "mm_grad" in str(e.value)
