"""Write tests/golden/plan_stream_v1.npz: the mask stream of three keys over the case of tests/planlib.stream_case, from the host restatement
(maskplan.plan_reference's shuffle).  Run once, after tests/test_maskplan_gpu.py has held the kernel to the restatement on a device; from then on
the file pins both - a change of the draw changes every run's masks and has to replace this file on purpose (as plan_stream_v2)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import planlib  # noqa: E402

desc, _, tl, th, fm = planlib.stream_case()
ids = np.stack([planlib.stream_ids(desc, k, (tl, th, fm)) for k in planlib.STREAM_KEYS])
path = os.path.join(ROOT, "tests", "golden", "plan_stream_v1.npz")
np.savez_compressed(path, desc=desc, tmask_lo=tl, tmask_hi=th, fmask=fm, keys=np.array(planlib.STREAM_KEYS, dtype=np.uint64), ids=ids)
print(path, ids.shape, os.path.getsize(path), "bytes")
