"""The exact-fp32 mode's bounds, on the CPU: (1) the table that motivates the mode, as a test - the unmodified oracle sits inside
EXACT_LOGIT_ABS of the reference's golden logits while three logic errors (a wrong LayerNorm eps, either positional table rolled by one
token) fall outside 3 x that bound and all PASS the bf16 path's 0.03 / 0.9999; (2) the kernel bounds of tests/exactlib.py accept a torch
fp32 evaluation of every formula and reject a dropped bias, a contraction cut short, a wrong alpha and a wrong softmax scale; (3) the host
refusals that need no device."""
import pytest
import torch

from avsiam_amd.config import AVSiamConfig
from avsiam_amd.weights import synth_state_ft
from oracle import ref_cpu
from tests import exactlib as X
from tests import rowwise
from tests.helpers import ft_case_inputs, ft_outputs_as_dict, load_golden

CASES = ["ft_audio", "ft_video", "ft_mm"]
# which outputs of a case a mutant reaches: the block eps all of them; a positional table the outputs that see its modality
REACH = {"eps": {"ft_audio": ("out",), "ft_video": ("out",), "ft_mm": ("out", "out_a", "out_v")},
         "pos_a": {"ft_audio": ("out",), "ft_video": (), "ft_mm": ("out", "out_a")},
         "pos_v": {"ft_audio": (), "ft_video": ("out",), "ft_mm": ("out", "out_v")}}

_cache = {}


def _case(name):
    """golden, inputs, weights and the unmodified oracle's outputs of a case, evaluated once"""
    if name not in _cache:
        torch.set_num_threads(8)
        d = load_golden(name)
        cfg = AVSiamConfig()
        a, v = ft_case_inputs(d, cfg)
        P = synth_state_ft(cfg, int(d["label_dim"]), int(d["weight_seed"]), "random")
        _cache[name] = (d, cfg, a, v, P, _oracle(d, cfg, a, v, P))
    return _cache[name]


def _oracle(d, cfg, a, v, P):
    with torch.no_grad():
        return ft_outputs_as_dict(d, ref_cpu.ft_forward(P, cfg, a, v, str(d["mode"]), bool(d["is_eval"])))


@pytest.mark.parametrize("name", CASES)
def test_unmodified_oracle_is_inside_the_exact_bound(name):
    assert X.EXACT_LOGIT_ABS <= X.EXACT_LOGIT_CAP == 1.2e-5
    d, *_, out = _case(name)
    for k, t in out.items():
        err, _ = X.logit_check(t, d[k])
        print(f"{name}.{k}: oracle against golden {err:.2e}")
        assert err <= X.EXACT_LOGIT_ABS, (name, k, err)


@pytest.mark.parametrize("mutant", ["eps", "pos_a", "pos_v"])
@pytest.mark.parametrize("name", CASES)
def test_logic_errors_pass_the_bf16_bound_and_fail_the_exact_one(name, mutant, monkeypatch):
    reach = REACH[mutant][name]
    if not reach:
        return                                                            # (the mutant does not touch this case's modality)
    d, cfg, a, v, P, _ = _case(name)
    if mutant == "eps":
        monkeypatch.setattr(ref_cpu, "LN_EPS_BLOCK", 1e-6)
        Pm = P
    else:
        key = "vit_base.pos_embed_a" if mutant == "pos_a" else "vit_base.pos_embed"
        Pm = dict(P)
        Pm[key] = torch.roll(P[key], 1, dims=1)
    out = _oracle(d, cfg, a, v, Pm)
    for k in reach:
        err, cos = X.logit_check(out[k], d[k])
        print(f"{name}.{k} with {mutant}: max |error| {err:.3e}, min row cosine {cos:.6f}")
        assert err > 3 * X.EXACT_LOGIT_ABS, (name, k, mutant, err)        # the exact mode sees it ...
        assert err <= X.BF16_LOGIT_ABS and cos >= X.BF16_LOGIT_COS, (name, k, mutant, err, cos)      # ... the bf16 bound does not


# ---- the kernel bounds on emulations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 527, 768), (37, 768, 3072)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_bounds_accept_fp32_and_reject_damage(shape):
    M, N, K = shape
    c = X.gemm_case(M, N, K)
    for ep in X.GEMM_EPILOGUES:
        kw = X.gemm_args(c, ep)
        ref, bound = X.gemm_reference(c["A"], c["B"], **kw)
        honest, _ = rowwise.elem_ratio(X.gemm_emulate(c["A"], c["B"], **kw), ref, bound)
        assert honest <= 1.0, (shape, ep, honest)                      # (not loose: each damage below falls outside)
        no_bias, _ = rowwise.elem_ratio(X.gemm_emulate(c["A"], c["B"], **dict(kw, bias=None)), ref, bound)
        cut, _ = rowwise.elem_ratio(X.gemm_emulate(c["A"], c["B"], kcut=1, **kw), ref, bound)
        assert no_bias > 1.0 and cut > 1.0, (shape, ep, no_bias, cut)
        if kw["alpha"] != 1.0:
            a1, _ = rowwise.elem_ratio(X.gemm_emulate(c["A"], c["B"], **dict(kw, alpha=1.0)), ref, bound)
            assert a1 > 1.0, (shape, ep, a1)


@pytest.mark.parametrize("hd", [64, 80])
def test_attention_bound_accepts_fp32_and_rejects_a_wrong_scale(hd):
    H, lens = 2, [5, 64, 65, 196]
    qkv = X.attn_case(H, hd, lens)
    ref, mag, A, Lrow = X.attn_eval(qkv, lens, H)
    honest = float(X.attn_ratio(X.attn_eval(qkv, lens, H, dt=torch.float32)[0], ref, mag, A, Lrow, H).max())
    wrong = float(X.attn_ratio(X.attn_eval(qkv, lens, H, dt=torch.float32, scale=(hd + 1) ** -0.5)[0], ref, mag, A, Lrow, H).max())
    print(f"hd {hd}: fp32 emulation {honest:.3f} of the bound, (hd + 1)^-0.5 {wrong:.1f}")
    assert honest <= 1.0 < wrong, (hd, honest, wrong)


# ---- host refusals ------------------------------------------------------------------------------------------------------------------------------
def test_exact_refuses_aug_and_needs_a_gpu():
    from avsiam_amd.models import CAVMAEFT_BASE
    m = CAVMAEFT_BASE(10)
    a = torch.zeros(1, 1024, 128)
    with pytest.raises(ValueError, match="aug"):
        m(a, None, "audioonly", exact=True, aug=object())
    with pytest.raises(Exception, match="needs a GPU") as plain:
        m(a, None, "audioonly")
    with pytest.raises(type(plain.value), match="needs a GPU") as exact:
        m(a, None, "audioonly", exact=True)
    assert str(exact.value) == str(plain.value)
    with pytest.raises(type(plain.value), match="needs a GPU"):
        m.retrieval_features(a, torch.zeros(1, 6, 3, 224, 224), exact=True)
    assert m(None, None, "joint_av", exact=True) is None


def test_exact_stack_refuses_what_it_does_not_build():
    from avsiam_amd.engine_exact import ExactStack
    for kw, what in (({"blocks2": [], "split": 4}, "blocks2"), ({"q_rows": 2}, "q_rows"), ({"pool": object()}, "pool"), ({"inference": False}, "forward-only")):
        with pytest.raises(ValueError, match=what):
            ExactStack("cpu", 8, 768, 12, 3072, [8], [], **kw)
