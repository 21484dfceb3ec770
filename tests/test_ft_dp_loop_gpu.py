"""The loop-level half of data-parallel fine-tuning on a real MI355X, through the command line: one rank with the collectives forced on
(--force-dp: a one-rank RCCL communicator) runs train() / validate() / evaluate_frames with their data-parallel branches, the early stop and
the optimizer-state file; and the launcher started from a PRE-TRAINING run's directory, whose best_optim_state.pth is another format."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = ["--ftmode", "mm_grad", "--n_class", "527", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "2", "--steps-per-epoch", "2",
        "--val-steps", "1", "--n-print-steps", "1"]


def test_force_dp_run_stops_early_and_its_adam_state_round_trips(tmp_path, monkeypatch, capsys):
    """lr = 0: the weights never move, every epoch validates to the same mAP, so epochs 2-4 bring no better one and train() returns after
    epoch 4 of 6.  The Adam state written beside best_audio_model.pth (epoch 1) is what a second run started from that file continues from."""
    import avsiam_amd.traintest_ft_base as loop
    from avsiam_amd.run_cavmae_ft_base import main
    exp = tmp_path / "ft"
    seen = {}
    real_validate = loop.validate

    def validate(model, loader, sampler, args, output_pred=False):
        seen["dp"] = model._dp and model._comm.active
        seen["steps"] = model.optimizer_steps()                       # (read from the device block: the model is data parallel)
        return real_validate(model, loader, sampler, args, output_pred)

    monkeypatch.setattr(loop, "validate", validate)
    out = main(BASE + ["--lr", "0", "--n_epochs", "6", "--exp_dir", str(exp), "--force-dp", "--device-metrics", "--eval-frames"])
    monkeypatch.setattr(loop, "validate", real_validate)
    assert seen["dp"], "--force-dp did not put the collectives on the path"
    assert out["best_epoch"] == 1 and len(out["frame_res"]) == 11
    res = np.loadtxt(exp / "result.csv", delimiter=",")
    assert res.shape == (6, 4) and np.all(res[:4, 0] == res[0, 0]) and np.all(res[4:] == 0), res          # epochs 5 and 6 never ran
    assert "early stop at epoch 4" in capsys.readouterr().out
    assert (exp / "mul_frame_res.csv").exists() and (exp / "models" / "best_audio_model.pth").exists()
    sd = torch.load(exp / "models" / "best_optim_state.pth", map_location="cpu")
    assert set(sd) == {"m", "v", "step", "lr"} and int(sd["step"].sum()) > 0 and float(sd["v"].abs().sum()) > 0
    assert sum(seen["steps"].values()) >= int(sd["step"].sum())        # (the file is epoch 1's, the run went on for three more)
    # a second run from that checkpoint: the state is restored before training starts
    got = {}

    def fake_train(model, train_loader, test_loader, test_sampler, args):
        got.update(steps=model.optimizer_state()["step"].clone(), m=model._opt["m"].detach().cpu().clone(), rates=model._rates)
        return {"best_epoch": 0}

    monkeypatch.setattr(loop, "train", fake_train)
    main(BASE + ["--lr", "0", "--n_epochs", "1", "--exp_dir", str(tmp_path / "again"), "--pretrain_path", str(exp / "models" / "best_audio_model.pth")])
    assert torch.equal(got["steps"], sd["step"]) and torch.equal(got["m"], sd["m"]) and got["rates"] == pytest.approx(tuple(sd["lr"].tolist()))


def test_launcher_starts_from_a_pretraining_directory(tmp_path):
    """<pretrain exp>/models as the pre-training train() leaves it - the two calls it makes for a best epoch (traintest_cavmae_base.py:
    _save_checkpoint, then torch.save(optimizer_state_dict(P1, lr)) as best_optim_state.pth, torch.optim.Adam's format): fine-tuning from
    that best_audio_model.pth is a weights-only warm start, not a KeyError."""
    from avsiam_amd.models import CAVMAE_BASE
    from avsiam_amd.param_spec import P1
    from avsiam_amd.run_cavmae_ft_base import main
    from avsiam_amd.traintest_cavmae_base import _save_checkpoint
    models = tmp_path / "pretrain" / "models"
    models.mkdir(parents=True)
    pre = CAVMAE_BASE()
    _save_checkpoint(pre, str(models / "best_audio_model.pth"))
    state = pre.optimizer_state_dict(P1, 5e-5)
    assert "state" in state and "param_groups" in state
    torch.save(state, models / "best_optim_state.pth")
    out = main(BASE + ["--lr", "1e-4", "--n_epochs", "1", "--exp_dir", str(tmp_path / "ft"), "--pretrain_path", str(models / "best_audio_model.pth")])
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3])
