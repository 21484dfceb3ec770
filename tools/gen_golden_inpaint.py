"""Golden vectors of the reconstructions: runs the UNMODIFIED reference ``CAVMAE_BASE`` on CPU in fp32 for the ``m_w1_b4`` case (its inputs,
weights and mask plan are reproducible from seeds: oracle/gen_golden.py), takes ``pred_a`` / ``pred_v`` of its decoder, puts them back into
pictures with the reference class's OWN ``unpatchify`` (cav_mae_base.py:353-363; for audio the inverse of the transpose of :666-668) and
composes ``input * (1 - mask) + recon * mask`` per cell.

    python tools/gen_golden_inpaint.py       # writes tests/golden/inp_m_w1_b4.npz (needs the reference checkout; oracle/ref_import.py)

Stored (data only), per modality, what the MAE golden stores for the predictions: the float64 L2 of the composed reconstruction, 64 sampled
cells at ``sample_positions("recon_a" / "recon_v", numel, 64)``, and the L2 over the masked cells alone.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avsiam_amd.config import AVSiamConfig                      # noqa: E402
from avsiam_amd.weights import synth_inputs                     # noqa: E402
from oracle import ref_import                                   # noqa: E402
from oracle.gen_golden import WEIGHT_SEED, full_state, sample_positions      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASE = "m_w1_b4"


def cell_mask(mask, h, w, c, p=16):
    """[N, L] token mask -> the [N, c, h * p, w * p] cell mask, by the same unpatchify the predictions go through"""
    return mask.reshape(mask.shape[0], h * w, 1).expand(-1, -1, p * p * c)


def main():
    if not ref_import.reference_available():
        print("reference not present - nothing to generate")
        return
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    base = np.load(os.path.join(GOLDEN, CASE + ".npz"), allow_pickle=False)
    cfg = AVSiamConfig()
    B, seed = int(base["batch"]), int(base["input_seed"])
    model = ref_import.build_reference_model()
    model.load_state_dict(full_state(cfg, WEIGHT_SEED, "random"), strict=True)
    model.train()
    a, v = synth_inputs(cfg, B, seed, None)
    torch.manual_seed(1000 + seed)                              # oracle/gen_golden.py::run_case: the reference then draws the recorded plan
    random.seed(2000 + seed)
    cap = {}
    orig_fd = model.forward_decoder

    def fd(*args, **kw):
        pa, pv = orig_fd(*args, **kw)
        cap["pred_a"], cap["pred_v"] = pa.detach().clone(), pv.detach().clone()
        return pa, pv

    model.forward_decoder = fd
    with torch.no_grad():
        out = model(a, v, 0.75, 0.75, mae_loss_weight=1, contrast_loss_weight=0)
    del model.forward_decoder
    mask_a, mask_v = out[5], out[6]
    assert np.array_equal(mask_a.numpy(), base["mask_a"]) and np.array_equal(mask_v.numpy(), base["mask_v"]), "not the plan of " + CASE
    np.testing.assert_allclose([out[i].item() for i in (1, 2, 3)], base["out_scalars"][1:4], rtol=1e-6)
    tP, fP, G = cfg.audio_t, cfg.audio_f, cfg.grid
    # audio: the loss patchifies the transposed spectrogram [N, 1, F, T] with h = F / 16, w = T / 16 (:666-668)
    rec_a = model.unpatchify(cap["pred_a"], 1, fP, tP, 16).squeeze(1).transpose(1, 2)                   # [N, T, F]
    cm_a = model.unpatchify(cell_mask(mask_a, fP, tP, 1), 1, fP, tP, 16).squeeze(1).transpose(1, 2)
    rec_v = model.unpatchify(cap["pred_v"], 3, G, G, 16)                                                 # [N, 3, H, W]
    cm_v = model.unpatchify(cell_mask(mask_v, G, G, 3), 3, G, G, 16)
    d = {"case": np.array(CASE), "batch": np.array(B), "input_seed": np.array(seed), "weight_seed": np.array(WEIGHT_SEED)}
    for k, inp, rec, cm in (("recon_a", a, rec_a, cm_a), ("recon_v", v, rec_v, cm_v)):
        comp = (inp * (1 - cm) + rec * cm).double()
        flat = comp.reshape(-1)
        d[k + "_l2"] = np.array(flat.norm().item())
        d[k + "_samples"] = np.array([flat[i].item() for i in sample_positions(k, flat.numel(), 64)])
        d[k + "_masked_l2"] = np.array((rec.double() * cm.double()).norm().item())
        d[k + "_masked_cells"] = np.array(int(cm.sum().item()))
        print(k, "l2", d[k + "_l2"], "masked l2", d[k + "_masked_l2"], "masked cells", d[k + "_masked_cells"], flush=True)
    np.savez_compressed(os.path.join(GOLDEN, "inp_" + CASE + ".npz"), **d)


if __name__ == "__main__":
    main()
