"""Golden vectors of the retrieval metrics: runs the three pure functions of the UNMODIFIED reference ``src/retrieval.py`` - ``get_similarity``,
``get_sim_mat``, ``compute_metrics`` - on synthetic feature pairs.

    python tools/gen_golden_retrieval.py      # writes tests/golden/retr_{a,b,c}.npz (needs the reference checkout; oracle/ref_import.py)

The module itself cannot be imported (it runs an experiment with hard-coded paths at import), so its source is parsed and only those three
function definitions are compiled, from the reference tree where it lies.  Stored (data only): the fp32 feature pairs a / v
(v = a + noise * randn, numpy.random.default_rng(0)), the reference's similarity matrix and its four metrics [R1, R5, R10, MR] - the matrix
is float64 there but every entry is an fp32 value (get_similarity works in the inputs' precision), so it is stored as fp32 without loss
(asserted below) at half the size, and only for cases a and b: the 200 x 200 matrix of case c would be the bulk of the fixture and is
reproducible bit for bit by this script, so case c keeps the features, the metrics and the gap;
plus the smallest gap between a diagonal entry and any other entry of its row, which must exceed the fp32 error of the device path
(tests/test_retrieval_gpu.py).
"""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import                                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WANTED = ("get_similarity", "get_sim_mat", "compute_metrics")
#         name      N    D   noise
CASES = [("retr_a", 64, 32, 1.5), ("retr_b", 96, 48, 2.5), ("retr_c", 200, 64, 4.0)]


def reference_functions():
    path = os.path.join(ref_import.REFERENCE_ROOT, "src", "retrieval.py")
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in body) == sorted(WANTED), [n.name for n in body]
    ns = {"np": np, "dot": np.dot, "norm": np.linalg.norm}       # the names the module imports for them (:14,17,18)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    if not ref_import.reference_available():
        raise SystemExit("the reference checkout is needed to (re)generate the goldens")
    ref = reference_functions()
    rng = np.random.default_rng(0)
    for name, N, D, noise in CASES:
        a = rng.standard_normal((N, D)).astype(np.float32)
        v = (a + noise * rng.standard_normal((N, D))).astype(np.float32)
        sim = ref["get_sim_mat"](a, v)
        m = ref["compute_metrics"](sim)
        d = np.diag(sim)[:, None]
        gap = np.abs(sim - d)[~np.eye(N, dtype=bool)].min()
        assert gap > 0, "the case has a tie with the diagonal"
        assert sim.dtype == np.float64 and np.array_equal(sim.astype(np.float32).astype(np.float64), sim)
        extra = {"sim": sim.astype(np.float32)} if N <= 96 else {}
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), a=a, v=v, metrics=np.array([m["R1"], m["R5"], m["R10"], m["MR"]], dtype=np.float64),
                            min_gap=np.float64(gap), **extra)
        print(f"{name}: N={N} D={D} noise={noise}  R1={m['R1']:.4f} R5={m['R5']:.4f} R10={m['R10']:.4f} MR={m['MR']}  smallest gap {gap:.2e}")


if __name__ == "__main__":
    main()
