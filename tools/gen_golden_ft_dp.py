"""Golden vectors of DATA-PARALLEL fine-tuning: two CPU processes (gloo over 127.0.0.1) run the UNMODIFIED reference ``CAVMAEFT_BASE``
under ``DistributedDataParallel(find_unused_parameters=True)`` (traintest_ft_base.py:91-92), each rank with its own batch and its own branch
of mm_grad - what the reference's per-rank ``random.uniform`` draw (:153-160) produces.

    python tools/gen_golden_ft_dp.py      # writes tests/golden/ftt_w2_<case>_r<rank>.npz (needs the reference checkout; oracle/ref_import.py)

Stored per case and rank (data only, the ftt_* format of tools/gen_golden_ft_train.py): the labels, the LOCAL loss, the logits, and the
gradient statistics of the AVERAGED gradients DDP leaves in .grad - with the names whose .grad stays None: the parameters NO rank reached.
Inputs: ft_inputs(cfg, 2, 1, 91 + rank), labels(2, 527, 91 + 527 + rank); weights synth_state_ft(cfg, 527, 4321, "random").
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from avsiam_amd.config import AVSiamConfig                      # noqa: E402
from avsiam_amd.param_spec import alias_of, state_dict_keys_ft  # noqa: E402
from avsiam_amd.weights import synth_state_ft                   # noqa: E402
from gen_golden_ft_train import INPUT_SEED, WEIGHT_SEED, is_base, labels, loss_of   # noqa: E402
from oracle import ref_import                                   # noqa: E402
from oracle.gen_golden import grad_stats                        # noqa: E402
from oracle.gen_golden_ft import ft_inputs                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
L, B, T, WORLD = 527, 2, 1, 2
#        name                 target per rank      freeze_base
CASES = [("ftt_w2_av",        ("out_a", "out_v"),  False),
         ("ftt_w2_mma",       ("out", "out_a"),    False),
         ("ftt_w2_vv_freeze", ("out_v", "out_v"),  True)]


def worker(rank, port):
    import datetime
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=600))
    torch.set_num_threads(max(1, min(8, (os.cpu_count() or 2) // 2)))
    cfg = AVSiamConfig()
    m = ref_import.build_reference_ft_model(L)
    st = synth_state_ft(cfg, L, WEIGHT_SEED, "random")
    m.load_state_dict({k: st[alias_of(k)] for k in state_dict_keys_ft(cfg, L)}, strict=True)
    m.eval()
    a, v = ft_inputs(cfg, B, T, INPUT_SEED + rank)
    y = labels(B, L, INPUT_SEED + L + rank)
    for name, targets, freeze in CASES:
        for n, p in m.named_parameters():
            p.requires_grad_(not (freeze and is_base(n)))
            p.grad = None
        ddp = DDP(m, find_unused_parameters=True)
        out = ddp(a, v, "mm_grad")
        outs = dict(zip(("out", "out_a", "out_v"), out))
        lo = loss_of(outs, y, "BCE", targets[rank])
        lo.backward()
        d = {"mode": np.array("mm_grad"), "label_dim": np.array(L), "batch": np.array(B), "frames": np.array(T), "loss_kind": np.array("BCE"),
             "target": np.array(targets[rank]), "freeze_base": np.array(freeze), "input_seed": np.array(INPUT_SEED + rank),
             "label_seed": np.array(INPUT_SEED + L + rank), "weight_seed": np.array(WEIGHT_SEED), "world": np.array(WORLD), "rank": np.array(rank),
             "labels": y.numpy().astype(np.float32), "loss": np.array(lo.item())}
        for k, o in outs.items():
            d["logits_" + k] = o.detach().numpy().astype(np.float32)
        d.update(grad_stats([(n, p.grad) for n, p in m.named_parameters()]))
        np.savez_compressed(os.path.join(GOLDEN, f"{name}_r{rank}.npz"), **d)
        print(name, "rank", rank, targets[rank], "loss", lo.item(), "live", len(json.loads(str(d["grad_names"]))), "none",
              len(json.loads(str(d["grad_none"]))), flush=True)
        del ddp
    dist.destroy_process_group()


def main():
    if not ref_import.reference_available():
        print("reference not present - nothing to generate")
        return
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = 29300 + os.getpid() % 500
    procs = [ctx.Process(target=worker, args=(r, port)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=900)
        if p.is_alive():
            p.terminate()
            raise SystemExit("a rank did not finish")
        if p.exitcode:
            raise SystemExit(f"a rank failed ({p.exitcode})")


if __name__ == "__main__":
    main()
