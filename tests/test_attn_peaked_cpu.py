"""Proof, without a GPU, of what tests/test_attn_peaked_gpu.py relies on: the score profiles of rowwise.attn_case reach the code they are meant
to reach (the forward's moving reference point, |lse| in the hundreds, one-hot and exactly uniform rows, tiles that underflow), the full
measure (rowwise.attention_measures_full) accepts the honest fp32 / bf16 emulation on every profile where the row-resolved measure of
N(0, 1) inputs cannot judge it, damage that no N(0, 1) case can see is rejected, and the element-by-element check of an 8-bit copy stays sharp
on gradients of such inputs.  Run with -s to see the figures."""
import functools
import math

import pytest
import torch

from tests import fp8lib as fl
from tests import rowwise as rw

H = 2
LENS = [1, 2, 40, 64, 65, 100, 129, 200]
HDS = (32, 64, 80)
START = {L: sum(LENS[:i]) for i, L in enumerate(LENS)}
GRADS = ("dq", "dk", "dv")


def say(*a):
    print("[attn_peaked]", *a)


@functools.lru_cache(maxsize=None)
def measured(hd, profile):
    """case, fp64 reference, honest emulation, its full measures and the tolerances they give"""
    c = rw.attn_case(H, hd, LENS, profile=profile)
    ref = rw.attention_eval(c["qkv"], LENS, H, c["dout"])
    emu = rw.attention_eval(c["qkv"], LENS, H, c["dout"], emulate=True)
    m = rw.attention_measures_full(emu, ref, H, LENS)
    return c, ref, emu, m, rw.attention_tolerances_full(m, ref)


@functools.lru_cache(maxsize=None)
def lazy(hd, profile, mutant=None):
    c = measured(hd, profile)[0]
    return rw.attention_forward_lazy(c["qkv"], LENS, H, mutant=mutant)


def seq_rows(L):
    return slice(START[L], START[L] + L)


@pytest.mark.parametrize("hd", HDS)
def test_honest_emulation_under_the_full_measure(hd):
    """dq / dk / dv of the honest emulation under the full measure: at most a third of their cap on every profile, so that 3 x the emulation is a
    tolerance the cap does not clip.  out / out_rel are measured as before and stay under their cap (a third of it they never met: 3.4e-3 of 6e-3
    on N(0, 1) already - one bf16 rounding of P and one of the output).  The old magnitude rows (|.| of the sums dP and delta) put the same honest
    emulation over the caps on `sharp` and `staircase`: the reason the full measure exists."""
    for profile in ("randn",) + rw.ATTN_PROFILES:
        c, ref, emu, m, tol = measured(hd, profile)
        old = rw.attention_measures(emu, ref, H)
        say(f"emulation hd {hd} {profile:15s} full: " + ", ".join(f"{k} {m[k]:.2e}" for k in ("dq", "dk", "dv", "out", "out_rel", "lse", "delta"))
            + " | old: " + ", ".join(f"{k} {old[k]:.2e}" for k in GRADS))
        for k in GRADS:
            assert m[k] <= rw.ATTN_WHOLE_TOL[k] / 3, (hd, profile, k, m[k])
            assert tol[k] == 3.0 * m[k]                                      # (not clipped)
        assert m["out"] <= rw.ATTN_WHOLE_TOL["out"] and m["out_rel"] <= rw.ATTN_WHOLE_TOL["out"], (hd, profile, m)
        assert tol["lse"] >= 4.0 * rw.U_F32 * float(ref["lse"].abs().max())
        if profile in ("sharp", "staircase"):
            assert max(old[k] for k in GRADS) > 1.5e-2, (hd, profile, old)
        # the restated tile walk is an honest forward too
        out, lse, _ = lazy(hd, profile)
        r = rw.attention_measures_full({"out": out, "lse": lse}, ref, H, LENS, tol=tol)
        say(f"  tile walk over its tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (hd, profile, r)


@pytest.mark.parametrize("hd", HDS)
def test_profiles_reach_what_they_are_meant_to_reach(hd):
    D = H * hd
    for L in (200, 129):
        rs = seq_rows(L)
        moves = lazy(hd, "staircase")[2][:, rs]
        say(f"hd {hd} L {L} staircase: reference moves per row {int(moves.min())} ... {int(moves.max())}")
        assert int(moves.min()) >= 2
        moves = lazy(hd, "late_spike")[2][:, rs]
        say(f"hd {hd} L {L} late_spike: rows whose reference moved, per head {[int((moves[h] > 0).sum()) for h in range(H)]}")
        assert all(int(moves[h].max()) >= 1 for h in range(H))
        assert int(lazy(hd, "randn")[2].max()) == 0                        # N(0, 1) never takes the branch
        for profile in ("offset_pos", "offset_neg"):
            lse = measured(hd, profile)[1]["lse"][:, rs]
            say(f"hd {hd} L {L} {profile}: lse {float(lse.min()):.1f} ... {float(lse.max()):.1f}")
            # (the offset is 210 nat; the log-sum-exp of the rows' own spread - up to +40 nat over 200 keys - adds to it for offset_pos and takes from
            # it for offset_neg, so "every row" holds at 150, and 200 is reached by the sequence, on offset_pos by every row)
            assert float(lse.abs().max()) >= 200.0 and float(lse.abs().min()) >= 150.0 and (float(lse.max()) < 0) == (profile == "offset_neg")
            assert profile == "offset_neg" or float(lse.abs().min()) >= 200.0

        def probs(profile):
            c, ref = measured(hd, profile)[:2]
            x = c["qkv"][rs].double()
            s = torch.einsum("ihd,jhd->hij", x[:, :D].reshape(L, H, hd), x[:, D:2 * D].reshape(L, H, hd)) * rw.LN2        # nat
            return s, s - ref["lse"][:, rs].unsqueeze(-1)

        s, logp = probs("sharp")
        pmax = float(logp.max(dim=-1).values.exp().mean())
        say(f"hd {hd} L {L} sharp: mean largest P {pmax:.3f}")
        assert pmax >= 0.5
        s, logp = probs("ties")
        lse = measured(hd, "ties")[1]["lse"][:, rs]
        assert float((lse - (math.log(L) + s[:, :, 0])).abs().max()) <= 1e-13 * (1 + float(lse.abs().max()))
        assert float((logp.exp() * L - 1).abs().max()) <= 1e-12
        s, logp = probs("first_tile_high")
        say(f"hd {hd} L {L} first_tile_high: largest log2 P beyond key 63 {float(logp[:, :, 64:].max()) / rw.LN2:.1f}")
        assert float(logp[:, :, 64:].max()) / rw.LN2 < -126.0


def _existing_tolerance(hd):
    """the tolerances tests/test_rowwise_gpu.py would hold this packed batch to on N(0, 1)"""
    c, ref, emu, _, _ = measured(hd, "randn")
    return ref, rw.attention_tolerances(rw.attention_measures(emu, ref, H))


def test_mutants_pass_on_n01_and_are_rejected_on_a_profile():
    """Four ways a kernel can be wrong where N(0, 1) inputs never look.  Each stays under EVERY existing tolerance on the N(0, 1) case (three of
    them are bit for bit the honest result there: the branch is not taken) and is rejected by a profile under the full measure."""
    hd = 64
    ref0, tol0 = _existing_tolerance(hd)
    found = {}
    # the forward's three: through the restated tile walk
    for mutant, what in (("no_o_rescale", "the move rescales l but not the accumulated o"), ("no_remask", "the move does not re-mask the tail tile"),
                         ("lse_first_ref", "lse saved from the first reference point")):
        out, lse, _ = lazy(hd, "randn", mutant)
        on_n01 = max(rw.attention_measures({"out": out, "lse": lse}, ref0, H, tol=tol0).values())
        assert rw.bitwise_equal(out, lazy(hd, "randn")[0]) and rw.bitwise_equal(lse, lazy(hd, "randn")[1])
        worst = (0.0, None, None)
        for profile in rw.ATTN_PROFILES:
            c, ref, emu, m, tol = measured(hd, profile)
            out, lse, _ = lazy(hd, profile, mutant)
            for k, v in rw.attention_measures_full({"out": out, "lse": lse}, ref, H, LENS, tol=tol).items():
                if v > worst[0]:
                    worst = (v, profile, k)
        found[what] = (on_n01, worst)
    # the backward's: one query row of the 129-token sequence also sees key 129, the next sequence's first row
    L, h = 129, 1
    c0 = measured(hd, "randn")[0]
    mut = rw.attention_eval(c0["qkv"], LENS, H, c0["dout"], emulate=True, mutant=("bwd_tail_key", L, h))
    on_n01 = max(rw.attention_measures(mut, ref0, H, tol=tol0).values())
    assert not rw.bitwise_equal(mut["dq"], measured(hd, "randn")[2]["dq"])      # (it does change dq there)
    worst = (0.0, None, None)
    for profile in rw.ATTN_PROFILES:
        c, ref, emu, m, tol = measured(hd, profile)
        mut = rw.attention_eval(c["qkv"], LENS, H, c["dout"], emulate=True, mutant=("bwd_tail_key", L, h))
        for k, v in rw.attention_measures_full(mut, ref, H, LENS, tol=tol).items():
            if v > worst[0]:
                worst = (v, profile, k)
    found["the backward's tail-key mask off by one key (one row, one head, L = 129)"] = (on_n01, worst)
    for what, (on_n01, (ratio, profile, k)) in found.items():
        say(f"mutant {what}: N(0, 1) ratio to the existing tolerances {on_n01:.3f} (accepted up to 1); {profile} {k} ratio {ratio:.3g} (rejected above 1)")
        assert on_n01 <= 1.0, what
        assert ratio > 1.0, what


@pytest.mark.parametrize("hd", HDS)
def test_e5m2_copy_check_stays_sharp_on_peaked_gradients(hd):
    """fp8lib.codes_within on e5m2 codes of the emulated dq | dk | dv (taken from the fp32 values, as the kernels take them) at the scale the suite
    uses: no violation, and the share of elements whose bf16 neighbour admits two codes under the bound that keeps the check sharp"""
    for profile in ("randn", "sharp", "staircase", "offset_neg"):
        emu = measured(hd, profile)[2]
        raw = torch.cat([emu[k + "_raw"] for k in GRADS], dim=1)
        b16 = raw.to(torch.bfloat16)
        s = fl.quarter_scale(b16.float().abs().max(), fl.E5M2)
        bad, amb = fl.codes_within(fl.quant(raw, s, fl.E5M2), b16, s, fl.E5M2)
        say(f"e5m2 copy of the emulated dqkv hd {hd} {profile}: ambiguous share {amb:.4f}")
        assert bad.numel() == 0 and amb <= fl.AMBIGUOUS_MAX[fl.E5M2], (hd, profile, bad.numel(), amb)
        assert rw.bitwise_equal(b16.float(), torch.cat([emu[k] for k in GRADS], dim=1))
