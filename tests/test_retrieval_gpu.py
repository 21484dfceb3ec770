"""Retrieval evaluation on a real MI355X: the streaming similarity -> rank / ties / top-K kernel against exact integer arithmetic and
against float64, the device path against the reference's recorded metrics (tests/golden/retr_*.npz), the single-frame feature
extraction against the existing forward(..., "retrieval"), and the public module end to end.

Bounds are derived, not measured: eps = D * 2^-24 is the worst-case error of an fp32 dot product of two unit vectors of length D
(D products and D additions, each within 2^-24 relative of a partial sum that never exceeds 1 in magnitude)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_golden, record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from avsiam_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def ops():
    from avsiam_amd import ops as o
    return o


def _exact_reference(q, g, target, topk):
    """int64 numpy: similarity, rank (strict), ties, and the top-K order (similarity descending, index ascending)"""
    s = q.astype(np.int64) @ g.astype(np.int64).T
    nq, ng = s.shape
    d = s[np.arange(nq), target][:, None]
    other = np.ones_like(s, dtype=bool)
    other[np.arange(nq), target] = False
    order = np.argsort(-s, axis=1, kind="stable")[:, :topk]            # stable: equal similarities keep ascending index
    return s, ((s > d) & other).sum(1), ((s == d) & other).sum(1), d[:, 0], order


LATTICE = [(512, 640, 768, True), (130, 257, 70, True), (1, 1, 768, True), (512, 640, 768, False), (130, 257, 70, False)]


@pytest.mark.parametrize("nq,ng,D,with_target", LATTICE)
@pytest.mark.parametrize("topk", [1, 5, 16])
def test_exact_on_integer_lattice(nq, ng, D, with_target, topk):
    """Entries in -3..3: every dot product is an integer below 2^24, exact in fp32 in any order, so every output must EQUAL int64 numpy."""
    rng = np.random.default_rng(1)
    q = rng.integers(-3, 4, size=(nq, D)).astype(np.float32)
    g = rng.integers(-3, 4, size=(ng, D)).astype(np.float32)
    target = rng.integers(0, ng, size=nq).astype(np.int32) if with_target else np.arange(nq, dtype=np.int32)
    s, rank, ties, d, order = _exact_reference(q, g, target, topk)
    assert np.abs(s).max() < 2 ** 24
    if nq >= 512 and with_target:
        assert (ties > 0).mean() > 0.5 and rank.min() < ng // 8 and rank.max() > ng // 2     # the strict / equal split is exercised
    out = ops().retrieval_rank(torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV),
                               torch.from_numpy(target).to(DEV) if with_target else None, topk=topk, want_sim=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["sim"].astype(np.int64), s) and np.array_equal(got["sim"], s.astype(np.float32))
    assert np.array_equal(got["rank"], rank)
    assert np.array_equal(got["ties"], ties)
    assert np.array_equal(got["target_sim"].astype(np.int64), d)
    k = min(topk, ng)
    assert np.array_equal(got["topk_idx"][:, :k], order[:, :k])
    assert np.array_equal(got["topk_sim"][:, :k].astype(np.int64), np.take_along_axis(s, order[:, :k], 1))
    assert (got["topk_idx"][:, k:] == -1).all() and np.isneginf(got["topk_sim"][:, k:]).all()


def _unit_pairs(N, D, noise, seed=1):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N, D))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    v = a + noise * rng.standard_normal((N, D))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return a.astype(np.float32), v.astype(np.float32)


def _recalls(rank):
    return [float((rank < k).mean()) for k in (1, 5, 10)]


def test_real_valued_ranks_inside_float64_intervals():
    """N = 2635, D = 768 unit vectors, v = a + 0.3 randn renormalised.  Reference: float64 matmul of the same fp32 inputs.  With
    eps = D * 2^-24 every rank must lie in [#{s > d + eps}, #{s > d - eps} - 1] (the diagonal itself is in the second count); a row whose
    interval is one value is decided and must match exactly.  The reference alone leaves 203 / 2635 = 7.7 % undecided; the condition is <= 10 %."""
    N, D = 2635, 768
    eps = D * 2.0 ** -24
    a, v = _unit_pairs(N, D, 0.3)
    s = a.astype(np.float64) @ v.astype(np.float64).T
    d = np.diag(s)[:, None]
    lo = (s > d + eps).sum(1)
    hi = (s > d - eps).sum(1) - 1
    assert (lo <= hi).all()
    undecided = int((lo != hi).sum())
    print(f"undecided rows {undecided} / {N}, widest interval {int((hi - lo).max())}")
    assert undecided <= 0.10 * N
    out = ops().retrieval_rank(torch.from_numpy(a).to(DEV), torch.from_numpy(v).to(DEV), want_sim=True)
    torch.cuda.synchronize()
    rank, tsim, sim = out["rank"].cpu().numpy(), out["target_sim"].cpu().numpy(), out["sim"].cpu().numpy()
    exact = ((s > d) & ~np.eye(N, dtype=bool)).sum(1)
    sim_err = float(np.abs(sim - s).max())
    print(f"max |sim - float64| {sim_err:.3e} (bound {eps:.3e}); rows whose rank differs from float64: {int((rank != exact).sum())}")
    record_margin("retrieval_real_valued", undecided_rows=undecided, rows=N, widest_interval=int((hi - lo).max()), sim_max_abs_err=sim_err, eps=eps,
                  rows_rank_differs_from_float64=int((rank != exact).sum()), r1=_recalls(rank)[0], r10=_recalls(rank)[2], median_rank=float(np.median(rank) + 1))
    assert np.abs(tsim - d[:, 0]).max() <= eps
    assert sim_err <= eps
    assert np.array_equal(tsim, np.diag(sim)), "target similarity must be the very bits the tile loop produced"
    assert ((rank >= lo) & (rank <= hi)).all()
    decided = lo == hi
    assert np.array_equal(rank[decided], lo[decided])
    for got, best, worst in zip(_recalls(rank), _recalls(lo), _recalls(hi)):
        assert worst <= got <= best


@pytest.mark.parametrize("case", ["retr_a", "retr_b", "retr_c"])
def test_goldens_on_the_device(case):
    """Recorded features -> normalise (as get_similarity does) -> ops.retrieval_rank -> metrics_from_ranks EQUAL the reference's metrics.
    fp32 error of a unit-vector dot product at D <= 64: 3.8e-6 per side, 7.6e-6 together, below the smallest gap (9.2e-6, case c)."""
    from avsiam_amd import retrieval
    d = load_golden(case)
    a = torch.nn.functional.normalize(torch.from_numpy(d["a"]).to(DEV), dim=-1)
    v = torch.nn.functional.normalize(torch.from_numpy(d["v"]).to(DEV), dim=-1)
    out = ops().retrieval_rank(a, v)
    got = retrieval.metrics_from_ranks(out["rank"].cpu().numpy())
    want = dict(zip(("R1", "R5", "R10", "MR"), d["metrics"].tolist()))
    assert int(out["ties"].sum()) == 0
    assert got == want, (got, want)


def test_deterministic_and_independent_of_the_segment_count():
    from avsiam_amd import _lib
    a, v = _unit_pairs(1545, 768, 0.3, seed=2)
    rng = np.random.default_rng(3)
    v[rng.integers(0, 1545, 200)] = v[rng.integers(0, 1545, 200)]                    # duplicated gallery rows: exact ties in every query row
    q, g = torch.from_numpy(a).to(DEV), torch.from_numpy(v).to(DEV)
    target = torch.from_numpy(rng.integers(0, 1545, 1545).astype(np.int32)).to(DEV)
    keys = ("rank", "ties", "target_sim", "topk_idx", "topk_sim", "sim")

    def run():
        out = ops().retrieval_rank(q, g, target, topk=16, want_sim=True)
        torch.cuda.synchronize()
        return {k: out[k].cpu().numpy().tobytes() for k in keys}

    base = run()
    assert run() == base
    try:
        for s in (1, 3, 13):
            _lib.tuning_set("retr_segments", s)
            got = run()
            for k in keys:
                assert got[k] == base[k], (s, k)
    finally:
        _lib.tuning_set("retr_segments", 0)
    assert np.frombuffer(base["ties"], dtype=np.int32).max() >= 1


def test_gallery_size_without_the_square_matrix():
    """N = 65536, D = 768: the N x N fp32 matrix would be 17 GB; the call may grow peak device memory by less than 1 GiB over the features."""
    N, D = 65536, 768
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * N * D * 4 + (2 << 30):
        pytest.skip(f"only {free >> 20} MiB of device memory free: not enough for two {N} x {D} fp32 feature matrices")
    gen = torch.Generator(device=DEV).manual_seed(0)
    a = torch.nn.functional.normalize(torch.randn(N, D, device=DEV, generator=gen), dim=-1)
    v = torch.nn.functional.normalize(a + 0.3 * torch.nn.functional.normalize(torch.randn(N, D, device=DEV, generator=gen), dim=-1), dim=-1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops().retrieval_rank(a, v, topk=16)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak device memory grew by {grown / 2 ** 20:.1f} MiB")
    record_margin("retrieval_gallery_65536", peak_growth_mib=grown / 2 ** 20)
    assert grown < (1 << 30)
    rank = out["rank"].cpu().numpy()
    assert rank.min() == 0 and (rank < 10).mean() > 0.9            # noise 0.3 on a unit vector: cos(match) ~ 0.96 against ~ N(0, 1/768) for the rest
    # spot check of 64 rows against torch's fp32 product of the same rows: top-1 and the match's rank within the eps interval
    rows = torch.arange(0, N, N // 64, device=DEV)
    s = (a[rows].double() @ v.double().T)
    dd = s[torch.arange(len(rows)), rows][:, None]
    eps = D * 2.0 ** -24
    lo, hi = (s > dd + eps).sum(1).cpu().numpy(), (s > dd - eps).sum(1).cpu().numpy() - 1
    r = rank[rows.cpu().numpy()]
    assert ((r >= lo) & (r <= hi)).all()


# ---- feature extraction and the public module ---------------------------------------------------------------------------------------------
_model = {}


def _ft_model(mode="random"):
    """'random': every tensor drawn independently (the goldens' weights); 'init': the constructor's initial state, where the audio patch
    embedding is the channel mean of the visual one - what retrieval.SyntheticPairs is built for"""
    from avsiam_amd.models import CAVMAEFT_BASE
    if mode not in _model:
        _model[mode] = CAVMAEFT_BASE(527, init_seed=4321, init_mode=mode).cuda()
    return _model[mode]


@pytest.mark.parametrize("T", [6, 10])
def test_retrieval_features_match_the_existing_mode(T):
    """forward(a, v, "retrieval") -> mean over tokens -> F.normalize (the yardstick: unchanged, pinned to the reference by ft_retrieval.npz)
    against retrieval_features, which embeds frame 5 alone.  Not bitwise: the encoder rows agree, but the yardstick pools and normalises in
    torch (mean, F.normalize) and the new path in the HIP kernels, which round the last bit differently - measured on the MI355X
    max |delta| = 2.2e-8 on components of ~ 0.036 (profiles/r08/retrieval_margins.json).  So, as the rule for the non-bitwise case says, the
    bound is 1e-3 on the unit vectors (a condition, not that measurement: a wrong frame, a missing normalisation or a wrong modality norm
    miss it by more than 10 x).  The new path itself must give the same bytes on a second call."""
    from avsiam_amd.config import AVSiamConfig
    cfg = AVSiamConfig()
    m = _ft_model()
    B = 4
    g = torch.Generator().manual_seed(11)
    a = torch.randn(B, cfg.audio_len, cfg.n_mels, generator=g).cuda()
    v = torch.randn(B, T, 3, cfg.img_size, cfg.img_size, generator=g).cuda()
    ta, tv = m(a, v, "retrieval")
    ra, rv = torch.nn.functional.normalize(ta.mean(1), dim=-1), torch.nn.functional.normalize(tv.mean(1), dim=-1)
    fa, fv = m.retrieval_features(a, v)
    assert fa.shape == fv.shape == (B, cfg.embed_dim) and fa.dtype == torch.float32
    gap_a, gap_v = float((fa - ra).abs().max()), float((fv - rv).abs().max())
    bitwise = bool(torch.equal(fa, ra) and torch.equal(fv, rv))
    print(f"T={T}: max |delta| audio {gap_a:.3e} video {gap_v:.3e} bitwise {bitwise}")
    record_margin(f"retrieval_features_T{T}", max_abs_audio=gap_a, max_abs_video=gap_v, bitwise=bitwise, bound=1e-3)
    assert max(gap_a, gap_v) <= 1e-3
    fa2, fv2 = m.retrieval_features(a, v)
    assert torch.equal(fa, fa2) and torch.equal(fv, fv2)             # the new path itself is deterministic
    assert abs(float(fa.norm(dim=1).mean()) - 1) < 1e-5 and abs(float(fv.norm(dim=1).mean()) - 1) < 1e-5
    # another frame: against v[:, k] of the full path (the all-frames encoder output holds every frame's tokens)
    k = 2
    m(a, v, "retrieval")
    enc = m._engine(B, T).encoder("av")
    tok = enc.yf[enc.rows_a:enc.rows].view(B, T, cfg.video_tokens, cfg.embed_dim)
    rk = torch.nn.functional.normalize(tok[:, k].mean(1), dim=-1)
    _, fk = m.retrieval_features(a, v, frame_index=k)
    gap_k = float((fk - rk).abs().max())
    record_margin(f"retrieval_features_T{T}", max_abs_video_frame2=gap_k)
    assert gap_k <= 1e-3
    assert float((fk - rv).abs().max()) > 1e-2                     # and it IS another frame
    # caller-provided rows of a dataset-level buffer
    buf_a, buf_v = torch.zeros(3 * B, cfg.embed_dim, device=DEV), torch.zeros(3 * B, cfg.embed_dim, device=DEV)
    m.retrieval_features(a, v, out_a=buf_a[B:2 * B], out_v=buf_v[B:2 * B])
    assert torch.equal(buf_a[B:2 * B], fa) and torch.equal(buf_v[B:2 * B], fv) and float(buf_a[:B].abs().max()) == 0 and float(buf_v[2 * B:].abs().max()) == 0


def test_retrieval_features_refuse_short_clips():
    from avsiam_amd.config import AVSiamConfig
    cfg = AVSiamConfig()
    m = _ft_model()
    a = torch.zeros(2, cfg.audio_len, cfg.n_mels).cuda()
    v = torch.zeros(2, 5, 3, cfg.img_size, cfg.img_size).cuda()
    with pytest.raises(IndexError):
        m.retrieval_features(a, v)                                 # frame 5 of 5 frames, as the mode (cav_mae_base.py:892)
    with pytest.raises(IndexError):
        m.retrieval_features(a, v, frame_index=7)
    fa, fv = m.retrieval_features(a, v, frame_index=4)
    assert bool(torch.isfinite(fa).all() and torch.isfinite(fv).all())


class _RecordingModel:
    """passes everything to the model and keeps the features it returned, for the numpy yardstick"""

    def __init__(self, model):
        self.model, self.arena, self.cfg, self.feats = model, model.arena, model.cfg, []

    def eval(self):
        return self

    def retrieval_features(self, *a, **k):
        out = self.model.retrieval_features(*a, **k)
        self.feats.append((out[0].clone(), out[1].clone()))
        return out


def _pairs_loader(n=96, batch=32):
    from avsiam_amd import retrieval
    from avsiam_amd.config import AVSiamConfig
    return retrieval.SyntheticPairs(AVSiamConfig(), n, batch, frames=6, seed=87, device=DEV)


def test_end_to_end_equals_numpy_on_the_extracted_features():
    """get_retrieval_result(model, loader, 'both') against numpy on the features it extracted; 'audio' / 'video' alone return the same tuples.

    Interval form.  Equality with compute_metrics(get_sim_mat(...)) would need every gap between a diagonal entry and the rest of its row to
    exceed the fp32 error of both sides (eps = D * 2^-24 = 4.6e-5 each), and no seed gives that: the 95 off-diagonal similarities of a row
    spread over a range of ~0.19, so over 96 rows the closest one comes within ~1e-6 of its diagonal (measured on the MI355X for seeds
    87 / 1 / 2 / 3 and both directions: smallest gap 9.8e-8 ... 4.7e-6, R@1 0.02 - 0.04; profiles/r08/retrieval_margins.json).  So, as for the
    real-valued kernel test: every row's rank from the device lies in [#{s > d + eps}, #{s > d - eps} - 1] of the float64 similarity of the
    SAME features, rows whose interval is one value match exactly, R@k lies between the two ends, and the tuples returned are exactly
    metrics_from_ranks of those device ranks.  The strict ranks of numpy's get_sim_mat (fp32 as well) must lie in the same intervals."""
    from avsiam_amd import retrieval
    rec = _RecordingModel(_ft_model("init"))
    res = retrieval.get_retrieval_result(rec, _pairs_loader(), "both")
    assert set(res) == {"audio", "video"}
    fa_d, fv_d = torch.cat([f[0] for f in rec.feats]), torch.cat([f[1] for f in rec.feats])
    fa, fv = fa_d.cpu().numpy(), fv_d.cpu().numpy()
    assert fa.shape == (96, 768)
    eps = 768 * 2.0 ** -24
    for d, (q, g, qd, gd) in (("audio", (fa, fv, fa_d, fv_d)), ("video", (fv, fa, fv_d, fa_d))):
        s64 = q.astype(np.float64) @ g.astype(np.float64).T
        dd = np.diag(s64)[:, None]
        gap = np.abs(s64 - dd)[~np.eye(96, dtype=bool)].min()
        lo, hi = (s64 > dd + eps).sum(1), (s64 > dd - eps).sum(1) - 1
        print(f"{d}: {res[d]}  smallest gap to the diagonal {gap:.3e} (eps {eps:.3e}), undecided rows {int((lo != hi).sum())} / 96")
        record_margin("retrieval_end_to_end", **{f"{d}_r1": res[d][0], f"{d}_r10": res[d][2], f"{d}_min_gap": gap, f"{d}_undecided_rows": int((lo != hi).sum())})
        rank = ops().retrieval_rank(qd, gd)["rank"].cpu().numpy()
        assert ((rank >= lo) & (rank <= hi)).all()
        assert np.array_equal(rank[lo == hi], lo[lo == hi])
        m = retrieval.metrics_from_ranks(rank)
        assert res[d] == (m["R1"], m["R5"], m["R10"], m["MR"])
        for got, best, worst in zip(res[d][:3], _recalls(lo), _recalls(hi)):
            assert worst <= got <= best
        # the numpy yardstick (fp32 too) through its per-row ranks: compute_metrics itself counts a row once per tied column, and at these
        # gaps fp32 numpy does produce exact ties (seen: 97 entries for 96 rows), so its R@k has another denominator and is not compared
        x = retrieval.get_sim_mat(q, g)
        rank_np = (x > np.diag(x)[:, None]).sum(1)
        assert ((rank_np >= lo) & (rank_np <= hi)).all()
        assert np.array_equal(rank_np[lo == hi], rank[lo == hi])
        assert 0.0 < res[d][0] < 1.0, "the synthetic pairs must be neither trivially separable nor unrelated"
    for d in ("audio", "video"):
        assert retrieval.get_retrieval_result(_ft_model("init"), _pairs_loader(), d) == res[d]
    both, topk = retrieval.get_retrieval_result(_ft_model("init"), _pairs_loader(), "both", return_topk=5)
    assert both == res and topk["audio"][0].shape == (96, 5)
    s = torch.from_numpy(fa).to(DEV).double() @ torch.from_numpy(fv).to(DEV).double().T
    assert float((topk["audio"][1][:, 0].double() - s.max(1).values).abs().max()) <= eps


def test_main_writes_the_reference_csv(tmp_path):
    from avsiam_amd import retrieval
    out = tmp_path / "retrieval_result.csv"
    rows = retrieval.main(["--synthetic", "64", "--direction", "both", "--frames", "6", "--batch-size", "32", "--out", str(out)])
    lines = out.read_text().strip().splitlines()
    assert len(lines) == 2 and len(rows) == 2
    for line, direction in zip(lines, ("video", "audio")):           # the reference's order of rows and columns (src/retrieval.py:128-146)
        f = line.split(",")
        assert f[0] == "synthetic" and f[1] == direction and len(f) == 6
        r1, r5, r10, mr = (float(x) for x in f[2:])
        assert 0 <= r1 <= r5 <= r10 <= 1 and mr >= 1
