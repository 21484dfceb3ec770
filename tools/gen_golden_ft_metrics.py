"""Golden vectors of the fine-tuning metrics: runs ``calculate_stats`` and ``d_prime`` of the UNMODIFIED reference ``src/utilities/stats.py``
(sklearn's average_precision_score / roc_auc_score / accuracy_score, scipy's normal quantile) on seeded synthetic predictions.

    python tools/gen_golden_ft_metrics.py     # writes tests/golden/ftm_{a,b,c}.npz (needs the reference checkout, sklearn and scipy)

The file is loaded by path (its package's __init__ cannot be imported).  Stored, data only: scores fp32 [N, C], target fp32 [N, C] (0 / 1),
the reference's AP [C] and auc [C] as float64, its acc, and d_prime of the mean auc.
  a  N = 200,  C = 10  multi-hot, continuous scores: no two scores of a class are equal (asserted)
  b  N = 384,  C = 12  one-hot labels, scores on the lattice of multiples of 1/8: ties everywhere; the case where acc means something
  c  N = 1000, C = 33  multi-hot at about 3 %, fp32 sigmoids of logits wide enough that some saturate to exactly 0.0 and 1.0 (asserted)
Every class of every case has a positive and a negative (asserted): degenerate classes follow this project's NaN convention, not sklearn's
version-dependent answers, and are tested against that.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import                                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_stats_module():
    path = os.path.join(ref_import.REFERENCE_ROOT, "src", "utilities", "stats.py")
    sys.dont_write_bytecode = True                              # never write .pyc into the reference tree
    spec = importlib.util.spec_from_file_location("reference_utilities_stats", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_a(rng):
    N, C = 200, 10
    target = (rng.random((N, C)) < 0.2).astype(np.float32)
    scores = (0.5 * rng.random((N, C)) + 0.3 * target + 0.2 * rng.random((N, C))).astype(np.float32)
    for k in range(C):
        assert len(np.unique(scores[:, k])) == N, "case a must not have ties"
    return scores, target


def case_b(rng):
    N, C = 384, 12
    cls = rng.integers(0, C, N)
    cls[:C] = np.arange(C)                                      # every class occurs
    target = np.zeros((N, C), dtype=np.float32)
    target[np.arange(N), cls] = 1.0
    scores = (np.round((0.65 * rng.random((N, C)) + 0.35 * target) * 8.0) / 8.0).astype(np.float32)
    assert len(np.unique(scores)) <= 9
    return scores, target


def case_c(rng):
    N, C = 1000, 33
    target = (rng.random((N, C)) < 0.03).astype(np.float32)
    logits = (45.0 * rng.standard_normal((N, C)) + 30.0 * target).astype(np.float32)
    scores = torch.sigmoid(torch.from_numpy(logits)).numpy()
    assert scores.dtype == np.float32 and (scores == 0.0).sum() > 10 and (scores == 1.0).sum() > 10, "case c needs saturated sigmoids"
    return scores, target


def main():
    if not ref_import.reference_available():
        raise SystemExit("the reference checkout is needed to (re)generate the goldens")
    ref = reference_stats_module()
    rng = np.random.default_rng(0)
    for name, make in (("ftm_a", case_a), ("ftm_b", case_b), ("ftm_c", case_c)):
        scores, target = make(rng)
        P = target.sum(0)
        assert (P >= 1).all() and (P <= len(target) - 1).all(), "every class needs a positive and a negative"
        stats = ref.calculate_stats(scores, target)
        AP = np.array([s["AP"] for s in stats], dtype=np.float64)
        auc = np.array([s["auc"] for s in stats], dtype=np.float64)
        assert (auc >= 0).all(), "the reference's roc_auc_score failed for a class"
        acc = np.float64(stats[0]["acc"])
        dp = np.float64(ref.d_prime(auc.mean()))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), scores=scores, target=target, AP=AP, auc=auc, acc=acc, d_prime=dp)
        ties = sum(len(target) - len(np.unique(scores[:, k])) for k in range(scores.shape[1]))
        print(f"{name}: N={scores.shape[0]} C={scores.shape[1]}  mAP={AP.mean():.6f} mAUC={auc.mean():.6f} acc={acc:.4f} d'={dp:.6f}  "
              f"P {int(P.min())}..{int(P.max())}  tied entries {ties}")


if __name__ == "__main__":
    main()
