"""Gradient accumulation without a GPU (csrc/grad_accum.hip; CAVMAEFT_BASE.set_grad_accumulation; run_cavmae_ft_base --accum-steps).

1. ops.grad_accum_reference - the numpy restatement the kernel is held to on the GPU (tests/test_grad_accum_gpu.py) - against torch's own
   accumulation of ``.grad`` across backwards, bit for bit: ``(p * c).sum().backward()`` gives the gradient ``c`` exactly, the first backward
   that reaches a parameter SETS its .grad (a copy), every later one adds one fp32 add per element, a parameter no backward reached keeps
   .grad None.  Those are the restatement's three rules: copy on first touch, add, class not in the published vector.
2. The launcher's --accum-steps.
3. The ABI: the header declares avs_grad_accum, and its argument refusals return -2 before any launch (so without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from avsiam_amd import _lib

NCLS = 16
# six parameters = six gradient classes; (lo, n, group, cls) in an arena with a gap behind every second one
SIZES = [4, 4096, 4100, 64, 12, 8]


def _segs():
    segs, at = [], 8
    for i, n in enumerate(SIZES):
        segs.append((at, n, i % 3, i))
        at += n + (8 if i % 2 == 0 else 0)
    return segs, at + 8


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _coeffs(seed, n, kind="gauss"):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-3, 4, (1,), generator=gen)))


def _run_cycle(reach, special=None):
    """k = len(reach) backwards; backward i reaches the parameters reach[i].  special: {(micro-step, parameter): tensor} overrides a
    coefficient.  -> (torch's parameters, the restatement's acc, acc_live, published, the arena before the cycle)"""
    from avsiam_amd import ops
    segs, total = _segs()
    params = [torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(100 + i))) for i, n in enumerate(SIZES)]
    stale = np.full(total, 777.25, dtype=np.float32)                  # what an earlier cycle left behind: never zero-filled
    acc, acc_live, published = stale.copy(), np.zeros(NCLS, dtype=np.float32), None
    for step, classes in enumerate(reach):
        g = np.full(total, np.nan, dtype=np.float32)                  # gaps and unreached classes: poison that must stay unread
        loss = None
        for c in classes:
            coef = (special or {}).get((step, c))
            coef = _coeffs(1000 * step + c, SIZES[c]) if coef is None else coef
            lo = segs[c][0]
            g[lo:lo + SIZES[c]] = coef.numpy()
            term = (params[c] * coef).sum()
            loss = term if loss is None else loss + term
        if loss is not None:
            loss.backward()                                          # torch accumulates into .grad: set on first touch, += afterwards
        live = [1.0 if c in classes else 0.0 for c in range(len(SIZES))]
        acc, acc_live, published = ops.grad_accum_reference(acc, g, segs, live, acc_live, first=(step == 0))
    return params, acc, acc_live, published, stale


REACH = [
    [{0, 1, 2, 3}, {1, 2, 4}, {0, 1, 4}],              # class 4 first reached in micro-step 2, class 5 never
    [{5}, set(), {5, 0}],                               # a micro-step that reaches nothing
    [{0, 1, 2, 3, 4, 5}],                               # a cycle of one: the bytes of g
    [{1}, {1}, {1}, {1}, {2}],
]


@pytest.mark.parametrize("reach", REACH)
def test_restatement_equals_torchs_own_accumulation_bit_for_bit(reach):
    segs, total = _segs()
    params, acc, acc_live, published, stale = _run_cycle(reach)
    reached = set().union(*reach)
    for c, p in enumerate(params):
        lo, n = segs[c][0], segs[c][1]
        if c in reached:
            assert p.grad is not None
            assert np.array_equal(_bits(p.grad.numpy()), _bits(acc[lo:lo + n])), c
        else:
            assert p.grad is None
            assert np.array_equal(_bits(acc[lo:lo + n]), _bits(stale[lo:lo + n])), "an unreached class must not be written"
    want = [1.0 if params[c].grad is not None else 0.0 for c in range(len(SIZES))] + [0.0] * (NCLS - len(SIZES))
    assert published.tolist() == want and acc_live.tolist() == want
    # the gaps belong to nobody
    owned = np.zeros(total, dtype=bool)
    for lo, n, _, _ in segs:
        owned[lo:lo + n] = True
    assert np.array_equal(_bits(acc[~owned]), _bits(stale[~owned]))
    assert not np.isnan(acc).any(), "the poison of gaps and unreached classes was read"


def test_negative_zero_survives_the_first_touch_and_a_late_class_is_copied():
    segs, _ = _segs()
    neg = torch.full((SIZES[0],), -0.0)
    late = _coeffs(5, SIZES[4])
    params, acc, *_ = _run_cycle([{0, 1}, {1, 4}], special={(0, 0): neg, (1, 4): late})
    lo0, lo4 = segs[0][0], segs[4][0]
    assert np.all(_bits(acc[lo0:lo0 + SIZES[0]]) == 0x80000000) and np.all(_bits(params[0].grad.numpy()) == 0x80000000)
    # class 4 was reached in micro-step 2 only: the stale 777.25 is overwritten, not added to
    assert np.array_equal(_bits(acc[lo4:lo4 + SIZES[4]]), _bits(late.numpy()))
    assert np.array_equal(_bits(params[4].grad.numpy()), _bits(late.numpy()))
    # -0.0 + -0.0 stays -0.0, -0.0 + 0.0 is +0.0: the add is the IEEE one
    params, acc, *_ = _run_cycle([{0}, {0}], special={(0, 0): neg, (1, 0): neg})
    assert np.all(_bits(acc[lo0:lo0 + SIZES[0]]) == 0x80000000)
    params, acc, *_ = _run_cycle([{0}, {0}], special={(0, 0): neg, (1, 0): torch.zeros(SIZES[0])})
    assert np.all(_bits(acc[lo0:lo0 + SIZES[0]]) == 0) and np.all(_bits(params[0].grad.numpy()) == 0)


def test_inf_then_minus_inf_is_nan():
    segs, _ = _segs()
    up, down = torch.ones(SIZES[3]), torch.ones(SIZES[3])
    up[5], down[5] = float("inf"), float("-inf")
    up[9] = float("inf")
    params, acc, *_ = _run_cycle([{3}, {3}], special={(0, 3): up, (1, 3): down})
    seg = acc[segs[3][0]:segs[3][0] + SIZES[3]]
    assert np.isnan(seg[5]) and np.isinf(seg[9]) and seg[0] == 2.0
    got = params[3].grad.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(seg)) and np.array_equal(_bits(got)[~np.isnan(got)], _bits(seg)[~np.isnan(seg)])


def test_restatement_rules_of_the_table():
    """malformed segments own nothing; `first` ignores the union so far; the input is not modified"""
    from avsiam_amd import ops
    acc = np.arange(64, dtype=np.float32)
    g = np.full(64, 2.0, dtype=np.float32)
    segs = [(0, 8, 0, 0), (8, 6, 0, 0), (18, 4, 0, 0), (24, 8, 3, 0), (32, 8, 0, 16), (40, 8, 1, 1), (48, 0, 0, 0), (-4, 4, 0, 0)]
    new, live, pub = ops.grad_accum_reference(acc, g, segs, [1.0, 0.0], [1.0, 1.0], first=False)
    want = acc.copy()
    want[0:8] += 2.0
    assert np.array_equal(new, want) and np.array_equal(acc, np.arange(64, dtype=np.float32))
    assert live.tolist() == [1.0, 1.0] + [0.0] * 14 and pub.tolist() == live.tolist()
    new, live, _ = ops.grad_accum_reference(acc, g, segs, [2.0, 0.0], [1.0, 1.0], first=True)
    want = acc.copy()
    want[0:8] = 2.0
    assert np.array_equal(new, want) and live.tolist() == [1.0] + [0.0] * 15


# ---- 2. the launcher ---------------------------------------------------------------------------------------------------------
def test_accum_steps_flag():
    from avsiam_amd.run_cavmae_ft_base import build_parser, inert_flag_warnings, main
    from avsiam_amd.traintest_ft_base import accum_steps_of
    p = build_parser()
    base = ["--ftmode", "mm_grad", "--n_class", "527"]
    plain, one, four = p.parse_args(base), p.parse_args(base + ["--accum-steps", "1"]), p.parse_args(base + ["--accum-steps", "4"])
    assert plain.accum_steps == 1 and vars(one) == vars(plain), "--accum-steps 1 is the default: nothing else in the namespace moves"
    assert four.accum_steps == 4 and {k for k in vars(four) if vars(four)[k] != vars(plain)[k]} == {"accum_steps"}
    assert inert_flag_warnings(one) == inert_flag_warnings(plain) == [] and inert_flag_warnings(four) == []
    assert accum_steps_of(plain) == 1 and accum_steps_of(four) == 4
    import argparse
    assert accum_steps_of(argparse.Namespace()) == 1, "callers of train() that predate the flag"
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit, match="--accum-steps"):       # refused before a model is built
            main(base + ["--accum-steps", bad])
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(SystemExit, match="--accum-steps"):
            accum_steps_of(argparse.Namespace(accum_steps=bad))
    with pytest.raises(SystemExit):                                   # argparse's own refusal of a non-integer
        p.parse_args(base + ["--accum-steps", "two"])


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from avsiam_amd.build import build
    build(verbose=False)
    return _lib.load()


def test_header_declares_grad_accum(lib):
    protos = _lib.parse_header()
    assert protos["avs_grad_accum"] == ("int", ["ptr", "ptr", "ptr", "int", "ll", "ptr", "ptr", "int", "int", "ptr"])
    assert hasattr(lib, "avs_grad_accum") and lib.avs_abi_version() == 2
    src = open(_lib.HEADER).read()
    assert "typedef struct avs_grad_accum_ctl" in src and "float live[16];" in src and "int n_micro;" in src and "int n_cycles;" in src


def test_grad_accum_refusals_need_no_gpu(lib):
    """argument validation precedes every launch: any non-NULL value serves as a pointer, the call must fail before touching it"""
    acc, g, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16)
    good = [acc, g, other, 1, 1, other, other, 1, 0, None]
    for i, bad in ((0, None), (1, None), (2, None), (5, None), (6, None), (1, acc), (3, 0), (3, -1), (3, 4097), (4, 0), (4, -5)):
        a = list(good)
        a[i] = bad
        assert lib.avs_grad_accum(*a) == -2 and b"grad_accum" in lib.avs_last_error(), (i, bad)
