"""Waveform input on a real MI355X: the Kaldi fbank kernel (ops.kaldi_fbank = avs_wave_sums + avs_kaldi_fbank) against its float64
specification (preprocess.kaldi_fbank_reference), the frame mix, the model on the kernel's output, and the launcher's --wave-input.

Nothing here was recorded from torchaudio (it was never available); the yardstick is the float64 restatement of the Kaldi definition.

Two measures of the kernel's error, each over the frame rows of a case:
  energy  |exp(out) - max(E64, FLT_EPSILON)| / max over the row of E64, over ALL cells.  (The output is ln(max(E, FLT_EPSILON)), so exp(out)
          estimates the floored energy; against the unfloored E64 the empty filter 3 alone would read FLT_EPSILON / max_row, which measures the
          definition and not the kernel.)
  log     |out - ln E64| over the cells with E64 >= 1e-6 max_row(E64).  The share of cells this excludes is a condition, not a measurement:
          at most 3 % for the noise and the mixed input (the specification alone excludes about 1.5 % there, 0.8 % of it the empty filter).
          The tone input (a 1 kHz sine of amplitude 0.5 over the noise) concentrates a row's energy in a few filters and is used for the
          energy measure only.
Bounds: ~3 x the kernel's measured maxima (the project's convention, profiles/r06/parity_margins.json); the measured values, beside the errors
of kaldi_fbank_reference(dtype=float32) on the same inputs, are logged through tests.helpers.record_margin (the project's margin log), from
which profiles/r12/frontend_margins.json is committed.

Exact cells.  Filter 3 holds no FFT bin, an all-zero clip and a constant clip have no energy, pad rows are 0: each is one constant, bit for
bit - FLOOR = fp32(ln(float64(FLT_EPSILON))) or 0.  With norm=(mean, std) the kernel computes (c - mean) * inv_std in fp32 with
inv_std = fp32(1) / fp32(std): the tests evaluate that very form in numpy float32."""
import types

import numpy as np
import pytest
import torch

from avsiam_amd.config import AVSiamConfig

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
MEAN, STD = -5.081, 4.4849
FLT_EPSILON = np.float64(np.float32(1.1920929e-07))
FLOOR = np.float32(np.log(FLT_EPSILON))
GRAD_COS, GRAD_NORM, LOSS_REL = 0.9998, 1e-2, 1e-4             # the bounds of tests/test_ft_aug_gpu.py
# ~3 x the kernel's measured maxima over the three inputs (profiles/r12/frontend_margins.json: energy 1.11e-6 on the tone - 5.7e-7 / 6.3e-7 on
# noise / mixed -, log 4.5e-5; kaldi_fbank_reference(dtype=float32) gets 4.2e-7 and 5.5e-5 there)
ENERGY_BOUND, LOG_BOUND = 3.4e-6, 1.4e-4
EXCLUDED_MAX = 0.03


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def pp():
    from avsiam_amd import preprocess
    return preprocess


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def norm_f32(c):
    """(c - mean) * inv_std the way the kernel states it: fp32 throughout, inv_std = fp32(1) / fp32(std)"""
    return (np.float32(c) - np.float32(MEAN)) * (np.float32(1.0) / np.float32(STD))


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(DEV)


def errors(out, ref_out, ref_e, m):
    """the two measures over rows 0 .. m - 1 of every clip -> (energy error, log error, excluded share)"""
    out = np.asarray(out, dtype=np.float64)[:, :m]
    e64 = ref_e[:, :m]
    row_max = e64.max(axis=2, keepdims=True)
    energy = float((np.abs(np.exp(out) - np.maximum(e64, FLT_EPSILON)) / row_max).max())
    keep = e64 >= 1e-6 * row_max
    log = float(np.abs(out - np.log(np.where(keep, e64, 1.0)))[keep].max())
    return energy, log, float(1.0 - keep.mean())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64
N_ACC, T_ACC = 6000, 36                                        # 36 frames: two full tiles of 16 and one of 4


@pytest.fixture(scope="module")
def acc_inputs():
    """three inputs, their float64 specification and the float32 restatement: computed once, shared, never modified"""
    rng = np.random.default_rng(20240612)
    noise = (rng.standard_normal((2, N_ACC)) * 0.1).astype(np.float32)
    t = np.arange(N_ACC) / 16000.0
    tone = (noise + 0.5 * np.sin(2 * np.pi * 1000.0 * t)[None, :]).astype(np.float32)
    partner = (rng.standard_normal((2, 5200)) * 0.1).astype(np.float32)
    cases = {"noise": dict(wave=noise), "tone": dict(wave=tone),
             "mixed": dict(wave=noise, partner=partner, partner_lengths=[5200, 4100], lam=[0.43, 0.62])}
    for c in cases.values():
        kw = {k: v for k, v in c.items() if k != "wave"}
        c["ref"], c["energy"] = pp().kaldi_fbank_reference(c["wave"], target_length=T_ACC, return_energy=True, **kw)
        c["ref32"] = pp().kaldi_fbank_reference(c["wave"], target_length=T_ACC, dtype=np.float32, **kw)
    return cases


def _run(c, **extra):
    kw = {k: (dev(v) if k == "partner" else v) for k, v in c.items() if k in ("partner", "partner_lengths", "lam")}
    return ops().kaldi_fbank(dev(c["wave"]), target_length=T_ACC, **kw, **extra)


def test_kernel_against_float64(acc_inputs):
    from tests.helpers import record_margin
    margins = {}
    for name, c in acc_inputs.items():
        out = _run(c).cpu().numpy()
        energy, log, excluded = errors(out, c["ref"], c["energy"], T_ACC)
        e32, l32, _ = errors(c["ref32"], c["ref"], c["energy"], T_ACC)
        margins[name] = {"kernel_energy": energy, "kernel_log": log, "excluded_share": excluded, "fp32_restatement_energy": e32,
                         "fp32_restatement_log": l32}
        print(f"kaldi_fbank vs float64 ({name}): energy {energy:.3e} (fp32 restatement {e32:.3e}), log {log:.3e} ({l32:.3e}), excluded {excluded:.4f}")
        record_margin(f"frontend.kaldi_fbank_vs_f64.{name}", **margins[name])
    for name, m in margins.items():
        assert m["kernel_energy"] <= ENERGY_BOUND, (name, m)
        if name != "tone":
            assert m["excluded_share"] <= EXCLUDED_MAX, (name, m)
            assert m["kernel_log"] <= LOG_BOUND, (name, m)


def test_exact_cells():
    o = ops()
    rng = np.random.default_rng(5)
    wave = np.zeros((3, 2000), dtype=np.float32)
    wave[0] = rng.standard_normal(2000) * 0.1
    wave[1] = 0.0
    wave[2] = 0.25
    lengths = [2000, 1500, 1999]                               # 11, 7 and 10 frames
    T = 12
    out = o.kaldi_fbank(dev(wave), lengths, target_length=T).cpu().numpy()
    outn = o.kaldi_fbank(dev(wave), lengths, target_length=T, norm=(MEAN, STD)).cpu().numpy()
    floor_n, zero_n = norm_f32(FLOOR), norm_f32(0.0)
    for got, floor, zero in ((out, FLOOR, np.float32(0.0)), (outn, floor_n, zero_n)):
        assert got.dtype == np.float32
        assert np.array_equal(got[0, :11, 3].view(np.int32), np.full(11, floor).view(np.int32)), "filter 3 holds no bin"
        assert np.array_equal(got[1, :7].view(np.int32), np.full((7, 128), floor).view(np.int32)), "an all-zero clip"
        assert np.array_equal(got[2, :10].view(np.int32), np.full((10, 128), floor).view(np.int32)), "a 0.25-constant clip"
        for b, m in enumerate((11, 7, 10)):
            assert np.array_equal(got[b, m:].view(np.int32), np.full((T - m, 128), zero).view(np.int32)), ("pad rows", b)
    assert (out[0, :11, np.arange(128) != 3] > FLOOR).all()    # the noise clip has energy everywhere else
    # the normalised output is the plain output through the stated fp32 form, everywhere
    want = (out - np.float32(MEAN)) * (np.float32(1.0) / np.float32(STD))
    assert np.array_equal(outn.view(np.int32), want.astype(np.float32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. edges
def _len(k, r=0):
    return 400 + 160 * k + r


EDGES = {
    # one frame; stride = the length
    "one_frame": dict(lengths=[400], stride=400, T=8),
    # r = 0 and r = 159 give the same frame count; three lengths in one call; m < T, m < T, m = T; T = 21: a full tile and one of 5 rows
    "remainders_and_full": dict(lengths=[_len(5), _len(5, 159), _len(20)], stride=_len(20) + 77, T=21),
    # m > T: cut, and T = 17 leaves a last tile of one row; a fourth clip shorter than the cut
    "cut_partial_tile": dict(lengths=[_len(30, 1), _len(16), _len(40, 159), _len(3)], stride=_len(41), T=17),
    # partner shorter / equal / longer than the clip, lam 0.43 / 0 / 1 / -1 in one batch, partner stride differs from the clip's
    "partner": dict(lengths=[3000, 3000, 2500, 2777, 3000], stride=3100, T=20, partner_lengths=[1700, 3000, 3300, 2000, 2100], partner_stride=3300,
                    lam=[0.43, 0.0, 1.0, -1.0, 0.43]),
    # T = 16 rows from clips of exactly 16 frames: one whole tile, nothing else
    "exact_tile": dict(lengths=[_len(15), _len(15, 80)], stride=_len(15, 80), T=16),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name):
    o = ops()
    e = EDGES[name]
    B, T, stride = len(e["lengths"]), e["T"], e["stride"]
    rng = np.random.default_rng(sum(map(ord, name)))
    wave = (rng.standard_normal((B, stride)) * 0.1).astype(np.float32)
    for b, n in enumerate(e["lengths"]):
        wave[b, n:] = 1.0e4                                    # beyond the clip: a read there shows in every measure
    kw, kw_ref = {}, {}
    if "lam" in e:
        partner = (rng.standard_normal((B, e["partner_stride"])) * 0.1).astype(np.float32)
        for b, n in enumerate(e["partner_lengths"]):
            partner[b, n:] = 1.0e4
        kw = dict(partner=dev(partner), partner_lengths=e["partner_lengths"], lam=e["lam"])
        kw_ref = dict(partner=partner, partner_lengths=e["partner_lengths"], lam=e["lam"])
    buf = torch.full((B + 2, T, 128), SENT, device=DEV)
    got = o.kaldi_fbank(dev(wave), e["lengths"], target_length=T, out=buf[1:B + 1], **kw)
    assert got.data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == SENT).all()) and bool((buf[B + 1] == SENT).all()), "the kernel wrote outside its output"
    out = got.cpu().numpy()
    assert np.isfinite(out).all() and not (out == SENT).any()
    ref, energy = pp().kaldi_fbank_reference(wave, e["lengths"], target_length=T, return_energy=True, **kw_ref)
    for b, n in enumerate(e["lengths"]):
        m = min(T, 1 + (n - 400) // 160)
        assert np.array_equal(out[b, m:].view(np.int32), np.zeros((T - m, 128), dtype=np.int32)), ("pad rows", b)
        en, lg, _ = errors(out[b:b + 1], ref[b:b + 1], energy[b:b + 1], m)
        assert en <= ENERGY_BOUND and lg <= LOG_BOUND, (name, b, en, lg)
    if name == "remainders_and_full":
        # the trailing 159 samples are ignored by the framing; they move the clip mean, which each frame's own mean removes again
        assert pp().fbank_frames(e["lengths"][0]) == pp().fbank_frames(e["lengths"][1]) == 6
    if "lam" in e:
        plain = o.kaldi_fbank(dev(wave), e["lengths"], target_length=T)
        for b, l in enumerate(e["lam"]):
            if l < 0:
                assert same_bits(got[b], plain[b]), ("lam < 0 rows are the bytes of a call without a partner", b)
            elif l < 1:                                        # (lam = 1 is 1 * a + 0 * c - 0: the clip itself, no claim either way)
                assert not same_bits(got[b], plain[b]), ("a mixed row", b)
        # device-resident per-clip vectors give the same bytes as host ones
        again = o.kaldi_fbank(dev(wave), dev(e["lengths"], torch.int32), partner=kw["partner"], partner_lengths=dev(e["partner_lengths"], torch.int32),
                              lam=dev(e["lam"]), target_length=T)
        assert same_bits(again, got)


def test_wrapper_refusals():
    o = ops()
    from avsiam_amd import _lib
    w = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError):
        o.kaldi_fbank(w, [1000, 399], target_length=8)         # a clip without a frame
    with pytest.raises(ValueError):
        o.kaldi_fbank(w, [1000, 1001], target_length=8)        # beyond the stride
    with pytest.raises(ValueError):
        o.kaldi_fbank(torch.zeros(2, 399, device=DEV), target_length=8)
    with pytest.raises(_lib.AvsiamHipError, match="128 mel bins"):
        o.kaldi_fbank(w, target_length=8, n_mels=64)
    with pytest.raises(_lib.AvsiamHipError):
        o.kaldi_fbank(w, target_length=8, lam=[0.5, 0.5])      # lam without a partner
    with pytest.raises(_lib.AvsiamHipError):
        o.kaldi_fbank(w, target_length=8, out=torch.zeros(2, 9, 128, device=DEV))
    with pytest.raises(_lib.AvsiamHipError):
        o.kaldi_fbank(w.double(), target_length=8)


def test_two_calls_give_the_same_bytes(acc_inputs):
    o = ops()
    c = acc_inputs["mixed"]
    a, b = _run(c, norm=(MEAN, STD)), _run(c, norm=(MEAN, STD))
    assert same_bits(a, b)
    w, p = dev(c["wave"]), dev(c["partner"])
    n1, n2 = dev([N_ACC, 5000], torch.int32), dev(c["partner_lengths"], torch.int32)
    s1, s2 = o.wave_sums(w, n1, p, n2), o.wave_sums(w, n1, p, n2)
    assert s1.dtype == torch.float64 and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    want = np.array([[c["wave"][b, :n].astype(np.float64).sum(), c["partner"][b, :m].astype(np.float64).sum(),
                      c["partner"][b, :min(n, m)].astype(np.float64).sum()] for b, (n, m) in enumerate(zip([N_ACC, 5000], c["partner_lengths"]))])
    assert np.abs(s1.cpu().numpy() - want).max() <= 1e-9       # fp64 sums of a few thousand fp32 values of size 0.1
    alone = o.wave_sums(w, n1).cpu().numpy()
    assert np.array_equal(alone[:, 0], s1.cpu().numpy()[:, 0]) and not alone[:, 1:].any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. frames
@pytest.mark.parametrize("shape", [(3, 2, 3, 20, 18), (1, 1, 3, 36, 36), (5, 3, 24, 44)], ids=["B3_two_frames_tail", "two_blocks_tail", "B5_no_frame_axis"])
def test_mix_frames(shape):
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    v1 = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)
    v2 = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)
    B = shape[0]
    buf = torch.full((B + 2,) + tuple(shape[1:]), SENT, device=DEV)
    one = o.mix_frames(v1, v2, [1.0] * B, out=buf[1:B + 1])
    assert bool((buf[0] == SENT).all()) and bool((buf[B + 1] == SENT).all())
    assert same_bits(one, pp().normalize_frames(v1)), "weight 1 is normalize_frames, bit for bit"
    weight = np.linspace(0.0, 0.83, B).astype(np.float32)
    got = o.mix_frames(v1, v2, dev(weight)).double().cpu()
    mean = torch.tensor(pp().IMAGENET_DEFAULT_MEAN, dtype=torch.float64).reshape(3, 1, 1)
    std = torch.tensor(pp().IMAGENET_DEFAULT_STD, dtype=torch.float64).reshape(3, 1, 1)
    n1, n2 = ((v.double().cpu() / 255 - mean) / std for v in (v1, v2))
    wb = torch.from_numpy(weight.astype(np.float64)).reshape((B,) + (1,) * (len(shape) - 1))
    err = float((got - (wb * n1 + (1 - wb) * n2)).abs().max())
    print(f"mix_frames vs float64 {shape}: {err:.3e}")
    assert err <= 1e-6
    from avsiam_amd import _lib
    with pytest.raises(_lib.AvsiamHipError):
        o.mix_frames(v1, v2[:, ..., :-1].contiguous(), [1.0] * B)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the model
LBL, MB = 7, 3
CFG = AVSiamConfig(depth=2)
# library calls of one fused plain step of this model (fresh, second step), as tests/test_ft_aug_gpu.py counts them on the parent commit
PARENT_CALLS = {"mm": 113, "a": 67}


@pytest.fixture(scope="module")
def model_case():
    from avsiam_amd.models import CAVMAEFT_BASE
    from avsiam_amd.weights import synth_inputs
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()
    m.requires_grad_(True)
    rng = np.random.default_rng(77)
    n = 20000                                                  # 123 frames; the other 901 rows of the 1024 are pad rows
    wave = (rng.standard_normal((MB, n)) * 0.1 * np.linspace(0.2, 1.0, n)[None, :]).astype(np.float32)
    partner = (rng.standard_normal((MB, 18000)) * 0.1).astype(np.float32)
    kw = dict(lengths=[n, n - 1234, n - 77], partner_lengths=[18000, 15000, 18000], lam=[0.43, -1.0, 0.55])
    a_ref = pp().kaldi_fbank_reference(wave, partner=partner, target_length=CFG.audio_len, norm=(MEAN, STD), **kw)
    a_dev = ops().kaldi_fbank(dev(wave), kw["lengths"], partner=dev(partner), partner_lengths=kw["partner_lengths"], lam=kw["lam"],
                              target_length=CFG.audio_len, norm=(MEAN, STD))
    _, v = synth_inputs(CFG, MB, 61)
    g = torch.Generator().manual_seed(3)
    hot = (torch.rand(MB, LBL, generator=g) < 0.3).float()
    hot[:, 0] = 1.0
    y = (hot * 0.9 + 0.1 / LBL).cuda()
    return types.SimpleNamespace(m=m, a_dev=a_dev, a_ref=dev(a_ref.astype(np.float32)), v=v.unsqueeze(1).cuda(), y=y)


@pytest.mark.parametrize("branch", ["mm", "a"])
def test_train_step_on_the_kernels_fbank_equals_the_step_on_the_specification(model_case, branch):
    """the fused step on ops.kaldi_fbank(norm=) output against the step on the float64 specification of the same (partly mixed) clips cast to
    fp32; bounds of tests/test_ft_aug_gpu.py.  Measured (profiles/r12/frontend_margins.json): loss within 5.3e-5 (mm) / 8.4e-6 (a) relative,
    cosine >= 0.99998938, norms within 2.1e-4 - the two inputs differ by ~1e-5 and round to different bf16 patch values here and there."""
    from tests.helpers import record_margin
    c = model_case
    steps = []
    for a in (c.a_dev, c.a_ref):
        loss = float(c.m.train_step(a, c.v, c.y, 0.0, "mm_grad", branch=branch))
        steps.append((loss, {n: p.grad.clone() for n, p in c.m._params.items() if p.grad is not None}))
    (l_dev, g_dev), (l_ref, g_ref) = steps
    assert np.isfinite(l_dev) and abs(l_dev - l_ref) <= LOSS_REL * abs(l_ref), (l_dev, l_ref)
    assert set(g_dev) == set(g_ref) and len(g_dev) > 0
    worst_cos, worst_norm = 1.0, 0.0
    for n, r in g_ref.items():
        g, r = g_dev[n].double().reshape(-1), r.double().reshape(-1)
        if float(r.norm()) == 0:
            assert float(g.norm()) == 0, n
            continue
        cos, nr = float(g @ r / (g.norm() * r.norm())), abs(float(g.norm() / r.norm()) - 1)
        worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, nr)
        assert cos >= GRAD_COS and nr <= GRAD_NORM, (branch, n, cos, nr)
    print(f"frontend step ({branch}): loss {l_dev:.6f} / {l_ref:.6f}, worst cosine {worst_cos:.8f}, worst norm error {worst_norm:.3e}")
    record_margin(f"frontend.step_on_kernel_fbank.{branch}", worst_cos=worst_cos, worst_norm=worst_norm, loss_rel=abs(l_dev - l_ref) / abs(l_ref))


def test_plain_step_issues_the_parents_calls(model_case):
    """a plain step (aug=None, no wave input) issues the library calls the parent commit issued: the counts tests/test_ft_aug_gpu.py holds for
    this model, batch and counting (mm 113, a 67); a step on the kernel's fbank is a plain step too - the front end is two more calls, outside"""
    from avsiam_amd import _lib
    from avsiam_amd.models import CAVMAEFT_BASE
    c = model_case
    m = CAVMAEFT_BASE(LBL, cfg=CFG, init_seed=6, init_mode="random").cuda()
    m.requires_grad_(True)
    for br in ("mm", "a"):
        m.train_step(c.a_ref, c.v, c.y, 0.0, "mm_grad", branch=br)
        c0 = _lib.calls
        m.train_step(c.a_dev, c.v, c.y, 0.0, "mm_grad", branch=br)
        assert _lib.calls - c0 == PARENT_CALLS[br], (br, _lib.calls - c0)
    c0 = _lib.calls
    ops().kaldi_fbank(torch.zeros(2, 1000, device=DEV), target_length=8)
    assert _lib.calls - c0 == 2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the launcher
def test_launcher_wave_input_with_the_audioset_recipe(tmp_path, capsys):
    """--wave-input --mixup 0.5 --freqm 48 --timem 192 --noise True at the smallest synthetic setting of the launcher tests: one epoch and
    its validation finish with finite, recorded losses, and nothing is said about mixup"""
    from avsiam_amd.run_cavmae_ft_base import main
    exp = tmp_path / "ft"
    out = main(["--ftmode", "mm_grad", "--n_class", "527", "--lr", "1e-4", "--head_lr", "100", "--mm_lr", "100", "--batch_size", "2", "--n_epochs", "1",
                "--exp_dir", str(exp), "--steps-per-epoch", "3", "--val-steps", "1", "--label_smooth", "0.1", "--wave-input", "--mixup", "0.5",
                "--freqm", "48", "--timem", "192", "--noise", "True"])
    said = capsys.readouterr().out
    assert not any("mixup" in line.lower() for line in said.splitlines() if "WARNING" in line) and "not implemented" not in said
    res = np.loadtxt(exp / "result.csv", delimiter=",").reshape(-1, 4)
    assert res.shape == (1, 4) and np.all(np.isfinite(res)), res
    assert "valid loss" in said and "nan" not in said.split("valid loss")[1].split()[0]
    assert out["best_epoch"] == 1 and np.isfinite(out["result"][0, 3])


def test_wave_loader_draws_on_the_host_and_mixes_on_the_device():
    """SyntheticWaveFtLoader: lengths in 9 - 10 s, lam < 0 for unmixed samples (weight 1 there), a batch = the kernel on those draws; validation never mixes"""
    from avsiam_amd.traintest_ft_base import SyntheticWaveFtLoader
    tr = SyntheticWaveFtLoader(CFG, 4, 2, LBL, DEV, seed=87, mixup=0.5, norm=(MEAN, STD), samples=8000)
    batches = []
    for a, v, y in tr:
        d = tr.last_draw
        assert a.shape == (4, CFG.audio_len, 128) and v.shape == (4, 1, 3, CFG.img_size, CFG.img_size) and v.dtype == torch.float32 and y.shape == (4, LBL)
        assert ((d["lengths"] >= 7200) & (d["lengths"] <= 8000)).all() and ((d["lam"] < 0) == (d["weight"] == 1.0)).all()
        want = ops().kaldi_fbank(tr.wave, d["lengths"], partner=tr.wave2, partner_lengths=d["partner_lengths"], lam=d["lam"], target_length=CFG.audio_len,
                                 norm=(MEAN, STD))
        assert same_bits(a, want)
        m = int(pp().fbank_frames(int(d["lengths"][0])))
        assert bool((a[0, m:] == float(norm_f32(0.0))).all()) and m < CFG.audio_len
        lam, n1, n2 = torch.from_numpy(d["lam"]).to(DEV), tr.hot.sum(1), tr.hot2.sum(1)
        mixed_sum = 0.1 + 0.9 * (lam * n1 + (1 - lam) * n2)                     # s + (1 - s) (lam |hot1| + (1 - lam) |hot2|)
        plain_sum = 0.9 * n1 + (0.1 / LBL) * (LBL - n1)
        assert torch.allclose(y.sum(1), torch.where(lam >= 0, mixed_sum, plain_sum), atol=1e-5)
        batches.append(d)
    assert len(batches) == 2 and not np.array_equal(batches[0]["lengths"], batches[1]["lengths"])
    va = SyntheticWaveFtLoader(CFG, 2, 1, LBL, DEV, seed=88, mixup=0.5, frames=10, train=False, samples=8000)
    (a, v, y), = list(va)
    assert "lam" not in va.last_draw and v.shape[1] == 10
    assert same_bits(a, ops().kaldi_fbank(va.wave, va.last_draw["lengths"], target_length=CFG.audio_len, norm=(MEAN, STD)))
