#!/usr/bin/env python3
"""Measured worst ratio of every bound of the exact-fp32 mode (tests/exactlib.py) -> profiles/r18/exact_margins.json:

    python tools/exact_margins.py [--out profiles/r18/exact_margins.json]

Runs tests/test_exact_gpu.py (all but the step digest) on the GPU with AVSIAM_EXACT_MARGINS set: every test records what it measured
before it asserts.  Keys: gemm_act0 / gemm_act1 / attn_hd* = worst error over bound; erff_ulp_upper; logits_golden_worst = the figure
EXACT_LOGIT_ABS is 3 x of; *_over_bound = worst error over the bound the test holds it to."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "exact_margins.json"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp"
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_exact_gpu.py", "-q", "-s", "-k", "not plain_step"], cwd=ROOT,
                       env=dict(os.environ, AVSIAM_EXACT_MARGINS=tmp))
    with open(tmp) as f:
        res = json.load(f)
    os.remove(tmp)
    sys.path.insert(0, ROOT)
    from tests import exactlib as X
    res.update(EXACT_LOGIT_ABS=X.EXACT_LOGIT_ABS, EXACT_LOGIT_CAP=X.EXACT_LOGIT_CAP, C_ERF=X.C_ERF, pytest_rc=r.returncode)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
