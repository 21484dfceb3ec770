"""Retrieval evaluation without a GPU: the numpy metrics against the reference's recorded results (tests/golden/retr_*.npz, written by
tools/gen_golden_retrieval.py from the unmodified reference functions), the C ABI of avs_retrieval_rank (declared, exported, argument errors
before any launch), and the entry point's command line."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT, load_golden

CASES = ["retr_a", "retr_b", "retr_c"]
KEYS = ("R1", "R5", "R10", "MR")


def _want(d):
    return dict(zip(KEYS, d["metrics"].tolist()))


@pytest.mark.parametrize("case", CASES)
def test_numpy_metrics_reproduce_the_reference(case):
    """similarity within 2 D 2^-24 (<= 7.6e-6 at D <= 64: the reference sums its fp32 products in another order - the worst case of two fp32
    dot products of unit-scale vectors, not a measurement); the metrics EQUAL, from the recorded matrix and from ours"""
    from avsiam_amd import retrieval
    d = load_golden(case)
    D = d["a"].shape[1]
    assert D <= 64
    N = d["a"].shape[0]
    sim = retrieval.get_sim_mat(d["a"], d["v"])
    assert sim.dtype == np.float64 and sim.shape == (N, N)
    assert retrieval.compute_metrics(sim) == _want(d)
    if "sim" not in d:              # case c records no matrix (it would be the bulk of the fixture): metrics, and the recorded gap against the bound
        assert d["min_gap"] > 2 * D * 2.0 ** -24
        return
    err = np.abs(sim - d["sim"].astype(np.float64)).max()
    print(f"{case}: max |sim - reference| = {err:.3e}")
    assert err <= 2 * D * 2.0 ** -24
    assert retrieval.compute_metrics(d["sim"].astype(np.float64)) == _want(d)
    i, j = 3, 7
    assert abs(retrieval.get_similarity(d["a"][i], d["v"][j]) - d["sim"][i, j]) <= 2 * D * 2.0 ** -24


def test_goldens_are_not_degenerate():
    r1 = [load_golden(c)["metrics"][0] for c in CASES]
    assert r1[0] > r1[1] > r1[2] > 0.1 and r1[0] < 1.0
    assert load_golden("retr_c")["metrics"][3] == 6.0


@pytest.mark.parametrize("case", CASES)
def test_metrics_from_ranks_equal_the_reference(case):
    from avsiam_amd import retrieval
    d = load_golden(case)
    # case c has no recorded matrix: ours differs from the reference's by < its smallest gap to the diagonal (asserted above), so the ranks agree
    x = d["sim"].astype(np.float64) if "sim" in d else retrieval.get_sim_mat(d["a"], d["v"])
    diag = np.diag(x)[:, None]
    assert ((x == diag).sum(1) == 1).all()                           # ties absent
    assert retrieval.metrics_from_ranks((x > diag).sum(1)) == _want(d)


def test_compute_metrics_keeps_the_reference_behaviour_on_ties():
    """one entry per column that equals the diagonal: positions rank, rank + 1, ... (src/retrieval.py:40-46), so len(ind) exceeds N"""
    from avsiam_amd import retrieval
    x = np.array([[0.5, 0.5, 0.1], [0.9, 0.2, 0.2], [0.3, 0.1, 0.7]])
    # row 0: diagonal 0.5 ties with column 1 -> entries 0, 1; row 1: 0.2 behind 0.9, tied with column 2 -> 1, 2; row 2: first -> 0
    ind = np.array([0, 1, 1, 2, 0])
    m = retrieval.compute_metrics(x)
    assert m == {"R1": 2 / 5, "R5": 1.0, "R10": 1.0, "MR": np.median(ind) + 1}
    assert retrieval.metrics_from_ranks([0, 1, 0])["R1"] == 2 / 3     # the optimistic ranks of the same matrix


@pytest.fixture(scope="module")
def lib():
    from avsiam_amd import _lib
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def test_abi_declared_and_exported(lib):
    from avsiam_amd import _lib
    protos = _lib.parse_header()
    assert protos["avs_retrieval_rank"][0] == "int" and len(protos["avs_retrieval_rank"][1]) == 19
    assert protos["avs_retrieval_rank_ws_bytes"] == ("size", ["int", "int", "int"])
    assert hasattr(lib, "avs_retrieval_rank") and hasattr(lib, "avs_retrieval_rank_ws_bytes")
    assert lib.avs_abi_version() == 2
    # O(nq * segments * topk), never O(nq * ng)
    assert 0 < lib.avs_retrieval_rank_ws_bytes(65536, 65536, 16) < 64 << 20
    assert lib.avs_retrieval_rank_ws_bytes(1545, 1545, 0) < 1 << 20


def test_argument_errors_before_any_launch(lib):
    one = ctypes.c_void_p(16)                      # any non-NULL value: the call must fail before touching it
    big = 1 << 30

    def call(q=one, ldq=8, nq=4, g=one, ldg=8, ng=4, D=8, target=None, rank=one, ties=None, tsim=None, topk=0, tidx=None, tsim_k=None, sim=None, ldsim=0,
             ws=one, ws_bytes=big):
        rc = lib.avs_retrieval_rank(q, ldq, nq, g, ldg, ng, D, target, rank, ties, tsim, topk, tidx, tsim_k, sim, ldsim, ws, ws_bytes, None)
        return rc, lib.avs_last_error()

    for kw, word in ((dict(q=None), b"q is NULL"), (dict(g=None), b"g is NULL"), (dict(rank=None), b"rank is NULL"),
                     (dict(topk=17, tidx=one, tsim_k=one), b"topk"), (dict(topk=-1), b"topk"), (dict(topk=4), b"topk_idx"),
                     (dict(ldq=7), b"ldq"), (dict(ldg=7), b"ldg"), (dict(nq=5), b"target"), (dict(sim=one, ldsim=3), b"ldsim"),
                     (dict(ws=None), b"ws"), (dict(ws_bytes=8), b"ws"), (dict(D=0), b"D")):
        rc, msg = call(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    # nq > ng is fine once a target is given: that call gets past the identity check (and then fails on the workspace, still before a launch)
    rc, msg = call(nq=5, target=one, ws_bytes=8)
    assert rc == -2 and b"ws" in msg


def test_segment_knob_is_range_checked(lib):
    from avsiam_amd import _lib
    assert _lib.tuning_get("retr_segments") == 0
    with pytest.raises(_lib.AvsiamHipError):
        _lib.tuning_set("retr_segments", 65)
    try:
        _lib.tuning_set("retr_segments", 1)
        one = lib.avs_retrieval_rank_ws_bytes(4096, 4096, 8)
        _lib.tuning_set("retr_segments", 8)
        assert lib.avs_retrieval_rank_ws_bytes(4096, 4096, 8) > one
        assert lib.avs_retrieval_rank_ws_bytes(4096, 4096, 0) == lib.avs_retrieval_rank_ws_bytes(4096, 128, 0)     # no top-K: nothing per segment
    finally:
        _lib.tuning_set("retr_segments", 0)


def test_help_parses_and_import_has_no_side_effects(capsys):
    from avsiam_amd import retrieval
    with pytest.raises(SystemExit) as e:
        retrieval.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--model", "--model-type", "--direction", "--batch-size", "--frame-use", "--num-class", "--topk", "--out", "--synthetic"):
        assert flag in out
    args = retrieval.build_parser().parse_args([])
    assert args.frame_use == 5 and args.out == "retrieval_result.csv"
    # a fresh interpreter: importing the module prints nothing and loads neither the kernel library nor torch's GPU runtime
    code = ("import sys; import avsiam_amd.retrieval as r; import avsiam_amd._lib as l; "
            "assert l._lib is None; t = sys.modules.get('torch'); assert t is None or not t.cuda.is_initialized(); print('ok')")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.stdout, res.stderr)


def test_main_without_a_dataset_says_what_to_do():
    from avsiam_amd import retrieval
    with pytest.raises(SystemExit) as e:
        retrieval.main([])
    assert "--synthetic" in str(e.value)
