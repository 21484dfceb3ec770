"""Host-side wrappers of the C ABI: shape/dtype/device validation, then one kernel launch on torch's current
stream.  Every function here runs ONLY on the HIP kernels; there is no eager fallback.

Shapes are validated on the host before any launch: a hand-written kernel that faults can reset the GPU.
"""
import ctypes

import torch

from . import _lib

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8


def _chk(t, dtype, name, ndim=None):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.AvsiamHipError(f"{name}: tensor must live on the GPU")
    if t.dtype != dtype:
        raise _lib.AvsiamHipError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.AvsiamHipError(f"{name}: tensor must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise _lib.AvsiamHipError(f"{name}: expected {ndim} dims, got {tuple(t.shape)}")


def _stream():
    return _lib.current_stream()


class KernelProfiler:
    """HIP-event timing of individual launches on torch's current stream (the stream the kernels run on).
    Enabled by bench.py over its timed region: `ops.prof = KernelProfiler()`; read with .summary() after a sync.
    `only`: kind prefixes to time; `stride`: time every stride-th launch of those kinds.  An event pair costs the stream
    ~5 us, so the default bench run samples the dominant kernel only: with a stride co-prime to the launches per step
    every launch position of the step is covered equally often over the timed steps, and the sample mean equals the mean
    over all launches."""

    def __init__(self, only=None, stride=1):
        self.rec = {}
        self.only = tuple(only) if only else None
        self.stride = max(1, int(stride))
        self.seen = 0

    def wants(self, kind):
        if self.only is not None and not kind.startswith(self.only):
            return False
        self.seen += 1
        return (self.seen - 1) % self.stride == 0

    def add(self, kind, e0, e1, work, dispatches=1):
        """work: FLOP (or bytes) of the launch, or a pair (FLOP, algorithmic HBM bytes) for kernels priced against both roofs"""
        w, b = work if isinstance(work, tuple) else (work, 0.0)
        self.rec.setdefault(kind, []).append((e0, e1, w, dispatches, b))

    def summary(self):
        out = {}
        for kind, lst in self.rec.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in lst)
            work = sum(r[2] for r in lst)
            out[kind] = {"launches": len(lst), "dispatches": sum(r[3] for r in lst), "total_ms": ms, "avg_us": 1e3 * ms / len(lst), "work": work,
                         "rate": work / (ms * 1e-3) if ms > 0 else 0.0, "bytes": sum(r[4] for r in lst)}
        return out


prof = None


def _launch(kind, work, cname, *args):
    if prof is None or not prof.wants(kind):
        return _lib.call(cname, *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    count = cname.startswith("avs_gemm_nt_bf16")         # a call is one or two kernel dispatches (leftover rows)
    d0 = _lib.load().avs_gemm_nt_dispatches() if count else 0
    e0.record()
    _lib.call(cname, *args)
    e1.record()
    prof.add(kind, e0, e1, work, _lib.load().avs_gemm_nt_dispatches() - d0 if count else 1)


def _call(cname, *args):
    """A kernel launch that is not one of the roofline families: timed (kind = the entry point's name) only when the profiler times
    every kind - bench.py's single-stream pass, where the per-family times must add up to the step."""
    if prof is None or prof.only is not None:
        return _lib.call(cname, *args)
    return timed(cname[4:] if cname.startswith("avs_") else cname, lambda: _lib.call(cname, *args))


def timed(kind, fn):
    """run fn() between two HIP events on the current stream when the profiler wants `kind` (torch-side work of the step, e.g. the
    gradient zero-fills, goes through here so that it shows up in bench.py's per-family sum)"""
    if prof is None or not prof.wants(kind):
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    prof.add(kind, e0, e1, 0.0)
    return out


def pad_rows(n, mult=128):
    return (n + mult - 1) // mult * mult


# ---------------------------------------------------------------------------------------------------
def layernorm_ws(rows, D):
    return _lib.load().avs_layernorm_ws_floats(rows, D)


def layernorm_fwd(x, g0, b0, y, mean, rstd, rows, eps, g1=None, b1=None, row_mod=None, out_map=None, y8=None, q8=1.0, q8_dev=None):
    """y may be None beside y8: the e4m3 copy is then the only output (fp8 mode 3: nothing reads the bf16 one)."""
    D = x.shape[1]
    assert y is not None or y8 is not None
    _chk(x, F32, "ln.x", 2); _chk(mean, F32, "ln.mean"); _chk(rstd, F32, "ln.rstd")
    if y is not None:
        _chk(y, y.dtype if y.dtype in (BF16, F32) else BF16, "ln.y", 2)
        assert y.shape[1] == D
    _chk(g0, F32, "ln.g0"); _chk(b0, F32, "ln.b0"); _chk(g1, F32, "ln.g1"); _chk(b1, F32, "ln.b1")
    _chk(row_mod, U8, "ln.row_mod"); _chk(out_map, I32, "ln.out_map")
    assert x.shape[0] >= rows and mean.numel() >= rows and rstd.numel() >= rows
    assert g0.numel() == D and b0.numel() == D
    if row_mod is not None:
        assert row_mod.numel() >= rows and g1 is not None and b1 is not None and g1.numel() == D
    if out_map is not None:
        assert out_map.numel() >= rows
    else:
        assert y is None or y.shape[0] >= rows
    if y8 is not None:
        _chk(y8, U8, "ln.y8", 2)
        assert y8.shape[1] == D and y8.shape[0] >= rows and (y is None or y.dtype == BF16) and out_map is None
    ysz = (y.element_size() if y is not None else 0) + (1 if y8 is not None else 0)
    _launch("layernorm_fwd", float(rows) * D * (4 + ysz), "avs_layernorm_fwd_q8", x, g0, b0, g1, b1, row_mod, out_map, y, 1 if (y is not None and y.dtype == F32) else 0, mean, rstd, rows, D,
              float(eps), y8, float(q8), _qrec(q8_dev), _stream())


def layernorm_bwd_slabs(rows):
    """per-block slabs (5 * D floats each) a backward over `rows` rows leaves in its workspace (LnReduceBatch)"""
    return _lib.load().avs_layernorm_bwd_slabs(int(rows))


class LnReduceBatch:
    """The parameter-gradient reduces of many LayerNorm backwards in ONE launch (avs_layernorm_bwd_reduce_batched): each backward runs with
    defer=True on a workspace of its own and leaves its per-block partial sums there; run() adds them all to their targets."""

    def __init__(self, D):
        self.D, self.entries, self.keep, self.desc = D, [], [], None

    def add(self, ws, rows, dg0, db0, dg1=None, db1=None, dcol=None):
        assert self.desc is None, "table already built"
        slabs = layernorm_bwd_slabs(rows)
        _chk(ws, F32, "lnbatch.ws")
        assert ws.numel() >= slabs * 5 * self.D
        for t in (dg0, db0, dg1, db1, dcol):
            _chk(t, F32, "lnbatch.target")
            assert t is None or t.numel() == self.D
        self.entries.append([ws.data_ptr(), slabs] + [t.data_ptr() if t is not None else 0 for t in (dg0, db0, dg1, db1, dcol)])
        self.keep.append((ws, dg0, db0, dg1, db1, dcol))

    def build(self, dev):
        self.desc = torch.tensor(self.entries, dtype=torch.int64, device=dev)

    def run(self):
        _call("avs_layernorm_bwd_reduce_batched", self.desc, len(self.entries), self.D, _stream())


def layernorm_bwd(dy, x, mean, rstd, g0, dx, dg0, db0, ws, rows, g1=None, dg1=None, db1=None, row_mod=None,
                  out_map=None, dres=None, dx_bf16=None, dcol=None, dx8=None, q8=None, defer=False):
    """dres: fp32, or bf16 (the residual-gradient stream kept in bf16: the previous call's dx_bf16); dx (fp32) may be None when
    dx_bf16 is given.  defer: the parameter gradients (dg*, db*, dcol) are NOT formed here - the per-block partial sums stay in `ws`
    (this call's own, layernorm_bwd_slabs(rows) * 5 * D floats) for an LnReduceBatch holding the same targets."""
    D = x.shape[1]
    _chk(dy, dy.dtype if dy.dtype in (BF16, F32) else BF16, "lnb.dy", 2); _chk(x, F32, "lnb.x", 2); _chk(dx, F32, "lnb.dx", 2)
    _chk(dres, dres.dtype if dres is not None and dres.dtype in (BF16, F32) else F32, "lnb.dres", 2)
    _chk(dx_bf16, BF16, "lnb.dx_bf16", 2); _chk(dcol, F32, "lnb.dcol")
    assert dcol is None or dcol.numel() == D
    assert dx is not None or dx_bf16 is not None
    _chk(dx8, U8, "lnb.dx8", 2)
    assert (dx8 is None) == (q8 is None) and (dx8 is None or (dx8.shape[0] >= rows and dx8.shape[1] == D))
    if dx_bf16 is not None:
        assert dx_bf16.shape[0] >= rows and dx_bf16.shape[1] == D
        assert dres is None or dres.dtype != BF16 or dres.data_ptr() != dx_bf16.data_ptr(), "dx_bf16 must not alias a bf16 dres"
    _chk(ws, F32, "lnb.ws"); _chk(row_mod, U8, "lnb.row_mod"); _chk(out_map, I32, "lnb.out_map")
    for t, n in ((g0, "g0"), (g1, "g1"), (dg0, "dg0"), (db0, "db0"), (dg1, "dg1"), (db1, "db1"), (mean, "mean"), (rstd, "rstd")):
        _chk(t, F32, "lnb." + n)
    assert x.shape[0] >= rows and dy.shape[1] == D and (dx is None or (dx.shape[0] >= rows and dx.shape[1] == D))
    assert ws.numel() >= (layernorm_bwd_slabs(rows) * 5 * D if defer else layernorm_ws(rows, D))
    if defer:
        dg0 = db0 = dg1 = db1 = dcol = None
    if out_map is None:
        assert dy.shape[0] >= rows
    if dres is not None:
        assert dres.shape[0] >= rows and dres.shape[1] == D
    nbytes = dy.element_size() + 4 + (4 if dx is not None else 0) + (dres.element_size() if dres is not None else 0) + (2 if dx_bf16 is not None else 0)
    _launch("layernorm_bwd", float(rows) * D * nbytes,
            "avs_layernorm_bwd", dy, 1 if dy.dtype == F32 else 0, x, mean, rstd, g0, g1, row_mod, out_map, dres,
            1 if dres is not None and dres.dtype == BF16 else 0, dx, dx_bf16, dg0, db0, dg1, db1, dcol, ws, rows, D, dx8, _qrec(q8), _stream())


# ---------------------------------------------------------------------------------------------------
def gemm_nt(A, B, out, M, bias=None, res=None, res_idx=None, aux=None, out2=None, alpha=1.0, act=0, scale_cols=0, col_scale=1.0, colsum=None,
            dual=None):
    """x[M,N] = alpha * (A[M,K] @ B[N,K]^T + bias [* aux] + res[res_idx]); columns [0, scale_cols) also * col_scale.
    act 0: out = x.  act 1 (fc1 + GELU): out = gelu'(x), out2 = gelu(x).  act 2 (fc2 input gradient): aux = the gelu'(x) act 1 saved.
    colsum[n] += sum_m out[m, n] (bf16 output only).
    dual = (m_split, B2, bias2, colsum2): rows [m_split, M) use the second weight set (one launch for two towers)."""
    _chk(A, BF16, "gemm.A", 2); _chk(B, BF16, "gemm.B", 2); _chk(bias, F32, "gemm.bias"); _chk(res, F32, "gemm.res", 2)
    # gelu'(x) as 8-bit fixed-point codes (EngineOptions.gelu8; the fp8 GEMMs' convention, gemm_nt_fp8): a uint8 `out` with act 1 / a uint8 `aux` with act 2
    gp8_out = out.dtype == U8
    gp8_aux = aux is not None and aux.dtype == U8
    assert not gp8_out or act == 1, "a uint8 `out` is the 8-bit gelu'(x) of act 1"
    assert not gp8_aux or act == 2, "a uint8 `aux` is the 8-bit gelu'(x) read by act 2"
    _chk(res_idx, I32, "gemm.res_idx"); _chk(aux, U8 if gp8_aux else BF16, "gemm.aux", 2); _chk(out2, BF16, "gemm.out2", 2)
    if out.dtype not in (BF16, F32, U8) or not out.is_cuda or not out.is_contiguous() or out.dim() != 2:
        raise _lib.AvsiamHipError("gemm.out: need contiguous 2-D bf16/fp32 GPU tensor")
    N, K = B.shape
    assert A.shape[1] == K and A.shape[0] >= M and out.shape[0] >= M and out.shape[1] == N, (A.shape, B.shape, out.shape, M)
    if bias is not None:
        assert bias.numel() == N
    if res is not None:
        assert res.shape[1] == N
        if res_idx is None:
            assert res.shape[0] >= M
        else:
            assert res_idx.numel() >= M
    if colsum is not None:
        _chk(colsum, F32, "gemm.colsum")
        assert colsum.numel() == N and out.dtype == BF16
    if act == 1:
        assert out2 is not None and out2.shape[0] >= M and out2.shape[1] == N
    if act == 2:
        assert aux is not None and aux.shape[0] >= M and aux.shape[1] == N
    args = (A, A.stride(0), B, B.stride(0), M, N, K, bias, res, res.stride(0) if res is not None else 0,
            res_idx, aux, aux.stride(0) if aux is not None else 0, out, out.stride(0), 2 if gp8_out else 1 if out.dtype == F32 else 0, out2,
            out2.stride(0) if out2 is not None else 0, float(alpha), 3 if gp8_aux else act, int(scale_cols), float(col_scale), colsum)
    if dual is None:
        _launch("gemm_nt_act%d" % act, 2.0 * M * N * K, "avs_gemm_nt_bf16", *args, _stream())
    else:
        m_split, B2, bias2, colsum2 = dual
        _chk(B2, BF16, "gemm.B2", 2); _chk(bias2, F32, "gemm.bias2"); _chk(colsum2, F32, "gemm.colsum2")
        assert B2.shape == B.shape and B2.stride(0) == B.stride(0) and 0 < m_split < M and m_split % 256 == 0
        assert (bias2 is None) == (bias is None) and (colsum2 is None) == (colsum is None)
        assert bias2 is None or bias2.numel() == N
        assert colsum2 is None or colsum2.numel() == N
        _launch("gemm_nt_act%d" % act, 2.0 * M * N * K, "avs_gemm_nt_bf16_dual", *args, int(m_split), B2, bias2, colsum2, _stream())


FP8_MAX = 448.0          # largest finite OCP e4m3 value
BF8_MAX = 57344.0        # ... and OCP e5m2 (the gradient operands of the fp8 input-gradient GEMMs)


Q_STRIDE = 1024          # floats per device quantisation record (csrc/common.h AVS_Q_STRIDE): a 256-byte header line (scale, 1 / scale, amax
                         # floor, saturation events) + 15 amax shards, each in a 256-byte line of its own


def _qrec(q):
    """a device quantisation record (fp32 [1024]: scale, 1 / scale, running amax, saturation events | 15 amax shards; csrc/common.h AVS_Q_*) or None"""
    if q is None:
        return None
    if not (q.is_cuda and q.dtype == F32 and q.numel() == Q_STRIDE and q.is_contiguous()):
        raise _lib.AvsiamHipError(f"fp8 record: need a contiguous fp32 GPU tensor of {Q_STRIDE} elements")
    return q


class Fp8Records:
    """Device-resident fp8 quantisation state of `n` tensors with delayed scaling (engine.FP8): records q[n, 4] and an amax history
    ring hist[nhist, n].  update() is one tiny launch and never synchronises: hist[pos] <- amax since the last update,
    scale <- 448 / (margin * max(hist)), amax <- 0, saturation counter += (amax * old scale > 448)."""

    def __init__(self, n, dev, nhist=16, margin=2.0, fmax=FP8_MAX):
        """fmax: largest finite value of the format these tensors are quantised to - 448 (e4m3) or 57344 (e5m2, gradients)"""
        self.n, self.nhist, self.margin, self.pos, self.fmax = n, nhist, margin, 0, float(fmax)
        self.q = torch.zeros((n, Q_STRIDE), dtype=F32, device=dev)
        self.hist = torch.zeros((nhist, n), dtype=F32, device=dev)

    def rec(self, i):
        return self.q[i]

    def amax(self, i):
        """the amax gathered since the last update (synchronises: tests)"""
        return float(torch.cat([self.q[i, 2:3], self.q[i, 64::64]]).max().item())

    def update(self, first=0, count=None):
        """count None: the whole table, and the history ring advances (once per forward).  A sub-range (calibration of tensors seen
        for the first time) is written into the current history slot without advancing."""
        whole = count is None
        count = self.n - first if whole else count
        if count <= 0:
            return
        assert 0 <= first and first + count <= self.n
        _call("avs_fp8_scale_update", self.q, self.hist, self.n, self.nhist, self.pos, float(self.margin), int(first), int(count), self.fmax, _stream())
        if whole and first == 0:
            self.pos = (self.pos + 1) % self.nhist

    def state(self):
        return {"q": self.q.detach().cpu().clone(), "hist": self.hist.detach().cpu().clone(), "pos": self.pos, "margin": self.margin}

    def load(self, st):
        assert tuple(st["q"].shape) == tuple(self.q.shape) and tuple(st["hist"].shape) == tuple(self.hist.shape), "fp8 state of another shape"
        self.q.copy_(st["q"]); self.hist.copy_(st["hist"])
        self.pos, self.margin = int(st["pos"]), float(st["margin"])

    def saturation_events(self):
        """total number of (tensor, update) pairs that saturated under the scale they were quantised with (synchronises: tests / logs)"""
        return float(self.q[:, 3].sum().item())


def absmax(x):
    """max |x| of a fp32 / bf16 GPU tensor, as a python float (synchronises: calibration / tests; a training loop would keep it on the device)"""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (F32, BF16)
    out = torch.zeros(1, device=x.device)
    _call("avs_absmax", x, 1 if x.dtype == F32 else 0, x.numel(), out, _stream())
    return float(out.item())


def absmax_into(x, q):
    """fold max |x| into the running amax of the device record q (no synchronisation)"""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (F32, BF16)
    _call("avs_absmax", x, 1 if x.dtype == F32 else 0, x.numel(), _qrec(q)[2:3], _stream())


def quantize_fp8(x, scale, out=None, q=None, e5m2=False):
    """x (fp32 / bf16, contiguous) -> uint8 tensor holding OCP e4m3 of clamp(x * scale, +-448) (e5m2: +-57344); with a device record q the
    scale is q[0] and max |x| is folded into q[2]"""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (F32, BF16) and x.numel() % 4 == 0
    y = out if out is not None else torch.empty(x.shape, dtype=U8, device=x.device)
    assert y.dtype == U8 and y.numel() == x.numel() and y.is_contiguous()
    _call("avs_quantize_fp8", x, 1 if x.dtype == F32 else 0, y, x.numel(), float(scale), _qrec(q), 1 if e5m2 else 0, _stream())
    return y


class Fp8Batch:
    """Quantise many bf16 tensors (a stack's weights) into their persistent fp8 copies with ONE launch: entries (src bf16, dst u8,
    record index into `records`); build() freezes the table.  The tensors must stay where they are (arena views do)."""

    def __init__(self, records, e5m2=False):
        self.records, self.e5m2 = records, e5m2
        self.entries, self.keep = [], []
        self.desc = self.cmap = None

    def add(self, src, dst, rec_index):
        assert self.desc is None, "table already built"
        _chk(src, BF16, "fp8batch.src"); _chk(dst, U8, "fp8batch.dst")
        assert src.numel() == dst.numel() and src.numel() % 4 == 0 and 0 <= rec_index < self.records.n
        self.entries.append((src.data_ptr(), dst.data_ptr(), src.numel() // 4, int(rec_index)))
        self.keep.append((src, dst))

    def build(self, dev):
        cmap = []
        for d, (_, _, n4, _) in enumerate(self.entries):
            cmap += [[d, g] for g in range(0, n4, 2048)]
        self.desc = torch.tensor(self.entries, dtype=torch.int64, device=dev)
        self.cmap = torch.tensor(cmap, dtype=I32, device=dev)
        self.nchunks = len(cmap)

    def run(self):
        _call("avs_quantize_fp8_batched", self.desc, self.cmap, self.nchunks, self.records.q, 1 if self.e5m2 else 0, _stream())


class ZeroTable:
    """Regions (row slices of contiguous 2-D tensors) zeroed together by one launch (avs_zero_batched)."""

    def __init__(self):
        self.entries, self.keep = [], []
        self.desc = self.cmap = None

    def add(self, t):
        assert self.desc is None, "table already built"
        nbytes = t.numel() * t.element_size()
        if nbytes == 0:
            return
        assert t.is_contiguous() and t.data_ptr() % 16 == 0 and nbytes % 16 == 0, "zero table: 16-byte aligned regions"
        self.entries.append((t.data_ptr(), nbytes // 16))
        self.keep.append(t)

    nchunks = 0

    def build(self, dev):
        cmap = []
        for d, (_, n16) in enumerate(self.entries):
            cmap += [[d, g] for g in range(0, n16, 4096)]
        self.nchunks = len(cmap)
        if self.nchunks:
            self.desc = torch.tensor(self.entries, dtype=torch.int64, device=dev)
            self.cmap = torch.tensor(cmap, dtype=I32, device=dev)

    def run(self):
        if self.nchunks:
            _call("avs_zero_batched", self.desc, self.cmap, self.nchunks, _stream())


def gemm_nt_fp8(A8, B8, out, M, alpha=1.0, bias=None, res=None, out2=None, act=0, scale_cols=0, col_scale=1.0, out8=None, out8_scale=1.0,
                qa=None, qw=None, q8=None, dual=None, grad=False, aux=None, colsum=None):
    """x = alpha * (A8[M, K] @ B8[N, K]^T) + bias (+ res); act 0: out = x; act 1: out = gelu'(x), out2 = gelu(x) (like gemm_nt).
    A8 / B8: uint8 tensors of e4m3 values (quantize_fp8), alpha = 1 / (scale_A * scale_B) - or the device records qa / qw (delayed
    scaling: the kernel reads qa[1] * qw[1]); q8: the record of out8.  dual = (m_split, B8_2, bias2, qw2[, colsum2]): a second weight set.
    grad=True: the input-gradient form - A8 holds e5m2 gradients; act 0 or 2 (aux = saved gelu'(x), colsum = fc1 bias gradient); out8
    then receives e5m2(out) for the next input-gradient GEMM."""
    _chk(A8, U8, "gemm8.A", 2); _chk(B8, U8, "gemm8.B", 2); _chk(bias, F32, "gemm8.bias"); _chk(res, F32, "gemm8.res", 2); _chk(out2, BF16, "gemm8.out2", 2)
    _chk(out8, U8, "gemm8.out8", 2); _chk(colsum, F32, "gemm8.colsum")
    # gelu'(x) as 8-bit fixed-point codes (fp8 backward, round 5): a uint8 `out` with act 1 / a uint8 `aux` with act 2 - the two epilogues that write and read it
    gp8_out = out is not None and out.dtype == U8
    gp8_aux = aux is not None and aux.dtype == U8
    _chk(aux, U8 if gp8_aux else BF16, "gemm8.aux", 2)
    assert not gp8_out or (act == 1 and not grad), "a uint8 `out` is the 8-bit gelu'(x) of act 1"
    assert not gp8_aux or (act == 2 and grad), "a uint8 `aux` is the 8-bit gelu'(x) read by act 2"
    N, K = B8.shape
    # 8-bit-only outputs (fp8 mode 3): out=None in the input-gradient form beside out8; out2=None with act 1 beside out8
    assert out is not None or (grad and out8 is not None)
    assert out is None or (out.dtype in (BF16, F32, U8) and out.dim() == 2 and out.is_contiguous() and out.shape[0] >= M and out.shape[1] == N)
    assert A8.shape[1] == K and A8.shape[0] >= M
    assert (qa is None) == (qw is None)
    assert act in (0, 1, 2) and (act != 2 or (grad and aux is not None and aux.shape[0] >= M and aux.shape[1] == N)) and (act != 1 or not grad)
    assert act != 1 or out2 is not None or out8 is not None
    assert colsum is None or (grad and colsum.numel() == N and (out is None or out.dtype == BF16))
    assert out8 is None or (out8.shape[0] >= M and out8.shape[1] == N)
    m_split, B2, bias2, qw2, colsum2 = (tuple(dual) + (None,))[:5] if dual is not None else (0, None, None, None, None)
    if dual is not None:
        _chk(B2, U8, "gemm8.B2", 2); _chk(bias2, F32, "gemm8.bias2"); _chk(colsum2, F32, "gemm8.colsum2")
        assert B2.shape == B8.shape and B2.stride(0) == B8.stride(0) and 0 < m_split < M and m_split % 256 == 0 and qa is not None and qw2 is not None
        assert (bias2 is None) == (bias is None) and (colsum2 is None) == (colsum is None)
    _launch("gemm_nt_fp8", 2.0 * M * N * K, "avs_gemm_nt_fp8", A8, A8.stride(0), B8, B8.stride(0), M, N, K, bias, res, res.stride(0) if res is not None else 0,
            out, out.stride(0) if out is not None else 0, 2 if gp8_out else 1 if (out is not None and out.dtype == F32) else 0, out2, out2.stride(0) if out2 is not None else 0, float(alpha), int(act), int(scale_cols),
            float(col_scale), out8, out8.stride(0) if out8 is not None else 0, float(out8_scale), _qrec(qa), _qrec(qw), _qrec(q8),
            int(m_split), B2, bias2, _qrec(qw2), 2 if gp8_aux else 1 if grad else 0, aux, aux.stride(0) if aux is not None else 0, colsum, colsum2, _stream())


def gemm_tn(A, B, C, M, splits=0):
    """C[N1,N2] += A[M,N1]^T @ B[M,N2]; A/B zero-padded to a multiple of 64 rows."""
    _chk(A, BF16, "wgrad.A", 2); _chk(B, BF16, "wgrad.B", 2); _chk(C, F32, "wgrad.C")
    N1, N2 = A.shape[1], B.shape[1]
    need = pad_rows(M, 64)
    assert A.shape[0] >= need and B.shape[0] >= need, "wgrad operands must be allocated (zero) to a multiple of 64 rows"
    assert C.numel() == N1 * N2
    _launch("gemm_tn", 2.0 * M * N1 * N2, "avs_gemm_tn_bf16", A, A.stride(0), B, B.stride(0), C, N2, M, N1, N2, splits, _stream())


def gemm_tn_group(jobs, M):
    """jobs: 1-3 triples (A[M,N1], B[M,N2], C[N1*N2]) over the same M token rows: C += A^T @ B, in ONE launch when the shapes allow
    (avs_gemm_tn_bf16_group3: fewer splits of the token rows, i.e. less fp32 atomic traffic, than one launch each)."""
    assert 1 <= len(jobs) <= 3
    if len(jobs) == 1:
        return gemm_tn(jobs[0][0], jobs[0][1], jobs[0][2], M)
    need = pad_rows(M, 64)
    args, flops = [], 0.0
    for A, B, C in jobs:
        _chk(A, BF16, "wgrad.A", 2); _chk(B, BF16, "wgrad.B", 2); _chk(C, F32, "wgrad.C")
        N1, N2 = A.shape[1], B.shape[1]
        assert A.shape[0] >= need and B.shape[0] >= need, "wgrad operands must be allocated (zero) to a multiple of 64 rows"
        assert C.numel() == N1 * N2 and N1 % 128 == 0 and N2 % 128 == 0
        args += [A, A.stride(0), B, B.stride(0), C, N1, N2]
        flops += 2.0 * M * N1 * N2
    args += [None, 0, None, 0, None, 0, 0] * (3 - len(jobs))
    _launch("gemm_tn", flops, "avs_gemm_tn_bf16_group3", *args, M, _stream())


def gemm_tn_fp8_group(jobs, M):
    """jobs: 1-3 tuples (A8 [M,N1] e5m2 gradient copy, B8 [M,N2] e4m3 activation copy, C [N1*N2] fp32, qa, qb) over the same M token rows:
    C += A8^T @ B8 / (scale_a * scale_b) in ONE launch of the fp8 weight-gradient kernel (avs_gemm_tn_fp8_group3; fp8 mode 3)"""
    assert 1 <= len(jobs) <= 3
    need = pad_rows(M, 64)
    args, flops = [], 0.0
    for A, B, C, qa, qb in jobs:
        _chk(A, U8, "wgrad8.A", 2); _chk(B, U8, "wgrad8.B", 2); _chk(C, F32, "wgrad8.C")
        N1, N2 = A.shape[1], B.shape[1]
        assert A.shape[0] >= need and B.shape[0] >= need, "wgrad operands must be allocated (zero) to a multiple of 64 rows"
        assert C.numel() == N1 * N2 and N1 % 256 == 0 and N2 % 256 == 0
        args += [A, A.stride(0), B, B.stride(0), C, N1, N2, _qrec(qa), _qrec(qb)]
        flops += 2.0 * M * N1 * N2
    args += [None, 0, None, 0, None, 0, 0, None, None] * (3 - len(jobs))
    _launch("gemm_tn_fp8", flops, "avs_gemm_tn_fp8_group3", *args, M, _stream())


# ---------------------------------------------------------------------------------------------------
class AttnTiles:
    """(sequence start, length, q0) per tile of `tile_rows` (128 or 64) rows for a packed batch of sequences."""

    def __init__(self, seq_lens, device, start_row=0, tile_rows=None, min_len=0):
        """min_len: only sequences LONGER than this get tiles (the shorter ones go to attn_bwd_fused); rows are still counted"""
        starts, lens, q0s = [], [], []
        row = start_row
        if tile_rows is None:      # 128-row (4-wave) workgroups measured faster than 64-row ones at every length (tools/bench_attn.py)
            tile_rows = 128
        assert tile_rows in (64, 128)
        self.tile_rows = tile_rows
        taken = []
        for L in seq_lens:
            if L > min_len:
                taken.append(L)
                for q0 in range(0, L, tile_rows):
                    starts.append(row); lens.append(L); q0s.append(q0)
            row += L
        self.rows = float(sum(taken))
        self.ntiles = len(starts)
        self.start = torch.tensor(starts, dtype=I32, device=device)
        self.len = torch.tensor(lens, dtype=I32, device=device)
        self.q0 = torch.tensor(q0s, dtype=I32, device=device)
        self.max_row = row
        self.sum_sq = float(sum(L * L for L in taken))           # sum of L^2: attention FLOPs = 4 * sum_sq * D
        # the common length when every sequence has it and all of them have tiles (the pruned last decoder block needs both), else 0
        self.uniform_len = seq_lens[0] if (len(seq_lens) and all(L == seq_lens[0] for L in seq_lens) and len(taken) == len(seq_lens) and start_row == 0) else 0


def attn_q_scale(hd):
    """Factor the q columns of qkv must carry for attn_fwd/attn_bwd: softmax scale hd^-0.5 times log2(e)."""
    return hd ** -0.5 * 1.4426950408889634


def attn_fwd(qkv, tiles, H, out, lse, out8=None, q8=None, lq=0):
    """out8 / q8 (fp8 mode): also write the e4m3 copy of the output for the proj GEMM, scaled by the device record q8.
    lq > 0 (equal-length sequences; avs_attn_fwd_cq): only the first lq rows of every sequence are queries, `out` is compact
    (sequence s owns rows s * lq ..) - the decoder's last block in the pruned form (engine.Stack).  That form differs in the rows `out`
    must hold, in the work estimate (the query fraction) and in the entry point."""
    _chk(qkv, BF16, "attn.qkv", 2); _chk(out, BF16, "attn.out", 2); _chk(lse, F32, "attn.lse", 2); _chk(out8, U8, "attn.out8", 2)
    assert (out8 is None) == (q8 is None) and (out8 is None or (out8.shape[0] >= tiles.max_row and out8.shape[1] == out.shape[1]))
    assert not lq or (out8 is None and tiles.uniform_len and 0 < lq <= tiles.uniform_len)
    D = qkv.shape[1] // 3
    assert qkv.shape[1] == 3 * D and out.shape[1] == D and D % H == 0 and D // H in (32, 64, 80)
    assert qkv.shape[0] >= tiles.max_row and out.shape[0] >= (tiles.max_row // tiles.uniform_len * lq if lq else tiles.max_row)
    assert lse.shape[0] == H and lse.shape[1] >= tiles.max_row
    frac = lq / tiles.uniform_len if lq else 1.0
    # algorithmic HBM bytes: q, k, v read and o written once per row (bf16), lse written per head and row
    cost = (4.0 * tiles.sum_sq * frac * D, tiles.rows * ((4.0 + 4.0 * frac) * D + 4.0 * H * frac))
    tail = (int(lq),) if lq else (out8, out8.stride(0) if out8 is not None else 0, _qrec(q8))
    _launch("attn_fwd_hd%d" % (D // H), cost, "avs_attn_fwd_cq" if lq else "avs_attn_fwd_q8", qkv, qkv.stride(0), D, H, tiles.start, tiles.len, tiles.q0, tiles.ntiles,
            tiles.tile_rows, out, out.stride(0), lse, lse.shape[1], *tail, _stream())


def attn_bwd(qkv, tiles, H, out, dout, lse, delta, dqkv, dqkv8=None, q8=None, kv_bf16=True, lq=0):
    """dqkv8 / q8 (fp8 backward): also write the e5m2 copy of dqkv - the gradient operand of the fp8 qkv input-gradient GEMM - scaled by
    the device record q8, whose running amax takes the largest |dqkv| written.  kv_bf16=False (with dqkv8): the key / value thirds of
    the bf16 dqkv are not written.
    lq > 0 (avs_attn_bwd_cq): the backward of attn_fwd(lq=): out / dout compact, dq written for the first lq rows of every sequence only."""
    assert kv_bf16 or dqkv8 is not None
    _chk(qkv, BF16, "attnb.qkv", 2); _chk(out, BF16, "attnb.out", 2); _chk(dout, BF16, "attnb.dout", 2); _chk(dqkv8, U8, "attnb.dqkv8", 2)
    assert (dqkv8 is None) == (q8 is None) and (dqkv8 is None or (dqkv8.shape[0] >= tiles.max_row and dqkv8.shape[1] == qkv.shape[1]))
    assert not lq or (dqkv8 is None and tiles.uniform_len and 0 < lq <= tiles.uniform_len)
    _chk(lse, F32, "attnb.lse", 2); _chk(delta, F32, "attnb.delta", 2); _chk(dqkv, BF16, "attnb.dqkv", 2)
    D = qkv.shape[1] // 3
    assert dqkv.shape == qkv.shape and out.shape[1] == D and dout.shape == out.shape and delta.shape == lse.shape and D // H in (32, 64, 80)
    assert qkv.shape[0] >= tiles.max_row and out.shape[0] >= (tiles.max_row // tiles.uniform_len * lq if lq else tiles.max_row)
    assert lse.shape[0] == H and lse.shape[1] >= tiles.max_row
    frac = lq / tiles.uniform_len if lq else 1.0
    # algorithmic FLOP: 8 * sum L^2 * D - the four products of the backward (dV, dP, dQ, dK); the recomputation of S = Q.K^T that the
    # kernels pay instead of keeping an L x L tensor is NOT counted.  Algorithmic HBM bytes of the two kernels: dQ
    # reads q, k, v, o, dO and writes dq (+ delta); dK/dV reads q, k, v, dO and writes dk, dv
    cost = (8.0 * tiles.sum_sq * frac * D, tiles.rows * ((16.0 + 8.0 * frac) * D + 16.0 * H * frac))
    tail = (int(lq),) if lq else (dqkv8, dqkv8.stride(0) if dqkv8 is not None else 0, _qrec(q8), 1 if kv_bf16 else 0)
    _launch("attn_bwd_hd%d" % (D // H), cost, "avs_attn_bwd_cq" if lq else "avs_attn_bwd_q8", qkv, qkv.stride(0), D, H, tiles.start, tiles.len, tiles.q0, tiles.ntiles,
            tiles.tile_rows, out, dout, out.stride(0), lse, delta, lse.shape[1], dqkv, *tail, _stream())


class AttnSeqs:
    """(start row, length) of the sequences of a packed batch that the fused backward takes: min_len < L <= max_len"""

    def __init__(self, seq_lens, device, min_len, max_len):
        starts, lens, row = [], [], 0
        for L in seq_lens:
            if min_len < L <= max_len:
                starts.append(row); lens.append(L)
            row += L
        self.nseq, self.max_len, self.max_row = len(starts), max_len, row
        self.start = torch.tensor(starts, dtype=I32, device=device)
        self.len = torch.tensor(lens, dtype=I32, device=device)
        self.rows = float(sum(lens))
        self.sum_sq = float(sum(L * L for L in lens))


def attn_bwd_fused(qkv, seqs, H, out, dout, lse, dqkv, dqkv8=None, q8=None, kv_bf16=True):
    """dq, dk, dv of the sequences in `seqs` (each at most seqs.max_len = 64 | 128 | 224 tokens; 224: head dim 64, no e5m2 copy; head dim 80: 64 only) in one
    kernel: one read of q, k, v, o, dO and one evaluation of S per (sequence, head).  Rows of other sequences are not touched."""
    _chk(qkv, BF16, "attnf.qkv", 2); _chk(out, BF16, "attnf.out", 2); _chk(dout, BF16, "attnf.dout", 2)
    _chk(lse, F32, "attnf.lse", 2); _chk(dqkv, BF16, "attnf.dqkv", 2); _chk(dqkv8, U8, "attnf.dqkv8", 2)
    assert (dqkv8 is None) == (q8 is None) and (dqkv8 is None or (dqkv8.shape[0] >= seqs.max_row and dqkv8.shape[1] == qkv.shape[1]))
    D = qkv.shape[1] // 3
    assert seqs.nseq > 0 and seqs.max_len in (64, 128, 224) and D // H in (32, 64, 80) and D % H == 0
    assert seqs.max_len != 224 or (D // H == 64 and dqkv8 is None)
    assert D // H != 80 or seqs.max_len == 64
    assert dqkv.shape == qkv.shape and out.shape[1] == D and dout.shape == out.shape
    assert qkv.shape[0] >= seqs.max_row and out.shape[0] >= seqs.max_row and lse.shape[0] == H and lse.shape[1] >= seqs.max_row
    # algorithmic work: 8 * sum L^2 * D FLOP; q, k, v, o, dO read and dq, dk, dv written once (bf16), lse read
    _launch("attn_bwd_hd%d" % (D // H), (8.0 * seqs.sum_sq * D, seqs.rows * (16.0 * D + 4.0 * H)), "avs_attn_bwd_fused_q8", qkv, qkv.stride(0), D, H, seqs.start,
            seqs.len, seqs.nseq, seqs.max_len, out, dout, out.stride(0), lse, lse.shape[1], dqkv, dqkv8, dqkv8.stride(0) if dqkv8 is not None else 0,
            _qrec(q8), 1 if kv_bf16 else 0, _stream())


# ---------------------------------------------------------------------------------------------------
class InputXf(ctypes.Structure):
    """include/avsiam_hip.h: avs_input_xf - how a raw input becomes the tensor the model sees (read on the host at call time)."""
    _fields_ = [("kind", ctypes.c_int), ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3), ("shift", ctypes.c_void_p),
                ("amp", ctypes.c_void_p), ("seed", ctypes.c_ulonglong)]

    @classmethod
    def audio(cls, mean, std, shift=None, amp=None, seed=0):
        """un-normalised fp32 fbank: (x - mean) / std [+ amp_b * U, rolled by shift_b] (dataloader.py:505-513)"""
        x = cls(1, (ctypes.c_float * 3)(float(mean), 0, 0), (ctypes.c_float * 3)(float(std), 1, 1), None, None, int(seed) & 0xFFFFFFFFFFFFFFFF)
        if (shift is None) != (amp is None):
            raise _lib.AvsiamHipError("InputXf.audio: shift and amp go together (the loader's noise augmentation draws both per sample)")
        if shift is not None:
            _chk(shift, I32, "xf.shift"); _chk(amp, F32, "xf.amp")
            x.shift, x.amp = shift.data_ptr(), amp.data_ptr()
            x._keep = (shift, amp)
        return x

    @classmethod
    def frames(cls, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        """uint8 frames: (x / 255 - mean_c) / std_c (dataloader.py:461-462, 152-155)"""
        return cls(2, (ctypes.c_float * 3)(*[float(m) for m in mean]), (ctypes.c_float * 3)(*[float(v) for v in std]), None, None, 0)


def _xf_arg(xf, kind, per_sample=None):
    if xf is None:
        return None
    if not isinstance(xf, InputXf) or xf.kind != kind:
        raise _lib.AvsiamHipError(f"input transform of kind {kind} expected")
    if per_sample is not None and xf.shift:
        assert xf._keep[0].numel() >= per_sample and xf._keep[1].numel() >= per_sample
    return ctypes.addressof(xf)


class FtAugState:
    """include/avsiam_hip.h: avs_ft_aug_state on the device - {key_lo, key_hi, counter, pad} as ONE int32 [4] buffer.  avs_ft_aug_draw reads
    the key and the counter and advances the counter; nothing else writes it."""

    def __init__(self, device, key=0, counter=0):
        key = int(key) & 0xFFFFFFFFFFFFFFFF
        self.key = key
        import numpy as np
        self.buf = torch.from_numpy(np.array([key & 0xFFFFFFFF, key >> 32, int(counter) & 0xFFFFFFFF, 0], dtype=np.uint32).view(np.int32).copy()).to(device)

    def counter(self):
        """draws so far (synchronises)"""
        return int(self.buf[2].item())


class FtAug:
    """include/avsiam_hip.h: the augmentation plan of one step on the device - avs_ft_aug_hdr {noise_lo, noise_hi, counter, n, pad[4]} followed
    by n avs_ft_aug_sample {f0, fn, t0, tn, shift, amp (fp32 bits), pad[2]}: ONE int32 [8 + 8 n] buffer.  ``fill``: what a masked cell of an
    already NORMALISED input (kind 0) takes; an un-normalised input (kind 1) always takes (0 - mean) * (1 / std), the reference's result."""
    HDR, REC = 8, 8

    def __init__(self, buf, n, fill=0.0):
        self.buf, self.n, self.fill = buf, int(n), float(fill)

    @classmethod
    def draw(cls, state, B, T, F, freqm, timem, noise, out=None, fill=0.0):
        """draw the next step's plan on the device (no host synchronisation) and advance ``state``.  out: an FtAug of at least B records to
        draw into (a captured step keeps one buffer); None: a new one."""
        B, T, F, freqm, timem = int(B), int(T), int(F), int(freqm), int(timem)
        if not (B > 0 and 0 < T < 32768 and 0 < F < 32768 and 0 <= freqm <= F and 0 <= timem <= T):
            raise _lib.AvsiamHipError(f"FtAug.draw: B {B}, T {T}, F {F}, freqm {freqm}, timem {timem}: need B > 0, 0 < T, F < 32768, 0 <= freqm <= F, 0 <= timem <= T")
        _chk(state.buf, I32, "ft_aug.state")
        if out is None:
            out = cls(torch.zeros(cls.HDR + cls.REC * B, dtype=I32, device=state.buf.device), B, fill)
        _chk(out.buf, I32, "ft_aug.plan")
        if out.buf.numel() < cls.HDR + cls.REC * B or out.buf.device != state.buf.device:
            raise _lib.AvsiamHipError(f"FtAug.draw: the plan buffer holds {out.buf.numel()} words on {out.buf.device}, {cls.HDR + cls.REC * B} needed on {state.buf.device}")
        out.n = B
        _call("avs_ft_aug_draw", state.buf, out.buf, B, T, F, freqm, timem, 1 if noise else 0, _stream())
        return out

    @classmethod
    def from_arrays(cls, f0, fn, t0, tn, shift, amp, seed, device="cuda", fill=0.0):
        """a plan from per-sample host arrays (a loader that draws on the host, tests); seed: the 64-bit Philox key of the noise field"""
        import numpy as np
        cols = [np.asarray(x, dtype=np.int64).astype(np.int32).reshape(-1) for x in (f0, fn, t0, tn, shift)]
        amp = np.asarray(amp, dtype=np.float32).reshape(-1)
        n = amp.size
        if n < 1 or any(c.size != n for c in cols):
            raise _lib.AvsiamHipError("FtAug.from_arrays: f0, fn, t0, tn, shift and amp need one value per sample each")
        if any((c < 0).any() for c in cols[:4]) or not np.isfinite(amp).all():
            raise _lib.AvsiamHipError("FtAug.from_arrays: mask starts / lengths must not be negative, amp must be finite")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        host = np.zeros(cls.HDR + cls.REC * n, dtype=np.int32)
        host[:4] = np.array([seed & 0xFFFFFFFF, seed >> 32, 0, n], dtype=np.uint32).view(np.int32)
        rec = host[cls.HDR:].reshape(n, cls.REC)
        for j, c in enumerate(cols):
            rec[:, j] = c
        rec[:, 5] = amp.view(np.int32)
        return cls(torch.from_numpy(host).to(device), n, fill)

    def arrays(self):
        """the plan back on the host (synchronises): dict of int32 f0, fn, t0, tn, shift, float32 amp, ints noise_key, counter, n"""
        import numpy as np
        h = self.buf.cpu().numpy()
        n = int(h[3])
        rec = h[self.HDR:self.HDR + self.REC * n].reshape(n, self.REC)
        u = h[:2].view(np.uint32)
        out = {k: rec[:, j].copy() for j, k in enumerate(("f0", "fn", "t0", "tn", "shift"))}
        out.update(amp=rec[:, 5].copy().view(np.float32), noise_key=int(u[0]) | (int(u[1]) << 32), counter=int(h[2]), n=n)
        return out


def _aug_args(aug, xf, kind, mean, std, fill, who):
    """-> (plan buffer, kind, mean, std, fill) of an augmented read.  From an audio InputXf (kind 1: its mean / std; it must carry no shift /
    amp of its own - the plan holds the step's) or from explicit kind / mean / std; fill None: the reference's value for the kind."""
    if not isinstance(aug, FtAug):
        raise _lib.AvsiamHipError(f"{who}: aug must be an ops.FtAug plan")
    _chk(aug.buf, I32, f"{who}.plan")
    if aug.buf.numel() < FtAug.HDR + FtAug.REC * aug.n:
        raise _lib.AvsiamHipError(f"{who}: the plan buffer is shorter than its {aug.n} records")
    if xf is not None:
        if not isinstance(xf, InputXf) or xf.kind != 1:
            raise _lib.AvsiamHipError("input transform of kind 1 expected")
        if xf.shift or xf.amp:
            raise _lib.AvsiamHipError(f"{who}: the input transform carries a shift / amp of its own beside an augmentation plan (the plan holds the step's)")
        kind, mean, std = 1, xf.mean[0], xf.std[0]
    kind = int(kind)
    if fill is None:
        import numpy as np
        # (0 - mean) * (1 / std) in fp32, as the kernel normalises
        fill = float((np.float32(0.0) - np.float32(mean)) * (np.float32(1.0) / np.float32(std))) if kind == 1 and std != 0 else aug.fill
    return aug.buf, kind, float(mean), float(std), float(fill)


def im2col_audio(a, row_b, row_tok, out, rows, t_patches, xf=None, stride=16, aug=None):
    """stride < 16: patch stride on 16 x 16 patch storage (config.stride) - the S x S corner of every 256-wide row is filled, the rest zero.
    aug (FtAug): the fine-tuning augmentation applied to every element read; `a` is then the un-normalised fbank when `xf` (an
    InputXf.audio(mean, std)) is given, the normalised tensor otherwise."""
    _chk(a, F32, "im2col.a", 3); _chk(row_b, I32, "im2col.row_b"); _chk(row_tok, I32, "im2col.row_tok"); _chk(out, BF16, "im2col.out", 2)
    assert out.shape[1] == 256 and out.shape[0] >= rows and row_b.numel() >= rows and row_tok.numel() >= rows
    assert a.shape[1] == t_patches * stride and a.shape[2] % stride == 0
    if aug is not None:
        plan, kind, mean, std, fill = _aug_args(aug, xf, 0, 0.0, 1.0, None, "im2col_audio")
        _call("avs_im2col_audio_aug", a, row_b, row_tok, out, rows, a.shape[1], a.shape[2], t_patches, int(stride), plan, kind, mean, std, fill, _stream())
        return
    _call("avs_im2col_audio_s", a, row_b, row_tok, out, rows, a.shape[1], a.shape[2], t_patches, int(stride), _xf_arg(xf, 1, a.shape[0]), _stream())


def augment_audio(a, out, aug, kind, mean=0.0, std=1.0, fill=None):
    """the two-pass form of the augmented read: a [B, T, F] fp32 -> out (fp32, same shape, another tensor) as the model sees it"""
    _chk(a, F32, "augment_audio.in", 3); _chk(out, F32, "augment_audio.out", 3)
    if tuple(out.shape) != tuple(a.shape) or out.data_ptr() == a.data_ptr() or a.shape[2] % 4 or a.numel() == 0:
        raise _lib.AvsiamHipError(f"augment_audio: in {tuple(a.shape)} / out {tuple(out.shape)}: same non-empty shape, different tensors, F % 4 == 0")
    plan, kind, mean, std, fill = _aug_args(aug, None, kind, mean, std, fill, "augment_audio")
    _call("avs_augment_audio", a, out, a.shape[0], a.shape[1], a.shape[2], plan, kind, mean, std, fill, _stream())


def im2col_video(v, row_img, row_tok, out, rows, xf=None, stride=16):
    _chk(v, U8 if xf is not None else F32, "im2col.v", 4); _chk(row_img, I32, "im2col.row_img"); _chk(row_tok, I32, "im2col.row_tok"); _chk(out, BF16, "im2col.out", 2)
    NF, C, H, W = v.shape
    assert out.shape[1] == C * 256 and out.shape[0] >= rows and row_img.numel() >= rows and row_tok.numel() >= rows and W % stride == 0
    _call("avs_im2col_video_s", v, row_img, row_tok, out, rows, C, H, W, int(stride), _xf_arg(xf, 2), _stream())


# ---------------------------------------------------------------------------------------------------
# exact-fp32 forward (csrc/exact.hip; engine_exact.py)
def gemm_nt_f32(A, B, out, M, bias=None, res=None, res_idx=None, alpha=1.0, act=0):
    """out[M,N] = act(alpha * (A[M,K] @ B[N,K]^T + bias + res[res_idx])), every operand fp32 (B: the arena's master weight itself).
    act 0 | 1 (exact GELU on erff).  A, B, res and out are row views: the last dimension contiguous, the row stride free (A, B: a multiple of 4).
    Any M, N >= 1; K % 32 == 0.  A fixed accumulation order per element (k-ordered chains per 32-wide slab, slab sums in slab order): a row's
    result depends on nothing but that row."""
    for t, name in ((A, "A"), (B, "B"), (out, "out"), (res, "res")):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != F32 or t.dim() != 2 or t.stride(1) != 1:
            raise _lib.AvsiamHipError(f"gemm_f32.{name}: need a 2-D fp32 GPU tensor with contiguous rows, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    _chk(bias, F32, "gemm_f32.bias"); _chk(res_idx, I32, "gemm_f32.res_idx")
    N, K = B.shape
    if K % 32:
        raise _lib.AvsiamHipError(f"gemm_nt_f32: K={K} is not a multiple of 32")
    if act not in (0, 1):
        raise _lib.AvsiamHipError(f"gemm_nt_f32: act must be 0 or 1, got {act}")
    assert M >= 1 and A.shape[1] == K and A.shape[0] >= M and out.shape[0] >= M and out.shape[1] == N, (A.shape, B.shape, out.shape, M)
    if bias is not None:
        assert bias.numel() == N
    if res is not None:
        assert res.shape[1] == N
        if res_idx is None:
            assert res.shape[0] >= M
        else:
            assert res_idx.numel() >= M
    else:
        assert res_idx is None
    _launch("gemm_nt_f32_act%d" % act, (2.0 * M * N * K, 4.0 * (M * K + N * K + M * N * (2 if res is not None else 1))), "avs_gemm_nt_f32", A, A.stride(0), B, B.stride(0),
            M, N, K, bias, res, res.stride(0) if res is not None else 0, res_idx, out, out.stride(0), float(alpha), int(act), _stream())


def attn_fwd_f32(qkv, tiles, H, out):
    """softmax(hd^-0.5 q k^T) v per sequence over packed fp32 qkv [rows, 3 D] with UNscaled q -> fp32 out [rows, D]; tiles: AttnTiles."""
    _chk(qkv, F32, "attn_f32.qkv", 2); _chk(out, F32, "attn_f32.out", 2)
    D = qkv.shape[1] // 3
    if qkv.shape[1] != 3 * D or D % H or D // H not in (32, 64, 80):
        raise _lib.AvsiamHipError(f"attn_fwd_f32: qkv {tuple(qkv.shape)} with {H} heads: head dim must be 32, 64 or 80")
    assert out.shape[1] == D and qkv.shape[0] >= tiles.max_row and out.shape[0] >= tiles.max_row and tiles.ntiles > 0
    _launch("attn_fwd_f32_hd%d" % (D // H), (4.0 * tiles.sum_sq * D, tiles.rows * 16.0 * D), "avs_attn_fwd_f32", qkv, qkv.stride(0), D, H, tiles.start, tiles.len, tiles.q0,
            tiles.ntiles, tiles.tile_rows, out, out.stride(0), _stream())


def im2col_audio_f32(a, row_b, row_tok, out, rows, t_patches, xf=None, stride=16):
    """im2col_audio with fp32 rows out (no augmentation form)"""
    _chk(a, F32, "im2col.a", 3); _chk(row_b, I32, "im2col.row_b"); _chk(row_tok, I32, "im2col.row_tok"); _chk(out, F32, "im2col.out", 2)
    assert out.shape[1] == 256 and out.shape[0] >= rows and row_b.numel() >= rows and row_tok.numel() >= rows
    assert a.shape[1] == t_patches * stride and a.shape[2] % stride == 0
    _call("avs_im2col_audio_f32", a, row_b, row_tok, out, rows, a.shape[1], a.shape[2], t_patches, int(stride), _xf_arg(xf, 1, a.shape[0]), _stream())


def im2col_video_f32(v, row_img, row_tok, out, rows, xf=None, stride=16):
    """im2col_video with fp32 rows out"""
    _chk(v, U8 if xf is not None else F32, "im2col.v", 4); _chk(row_img, I32, "im2col.row_img"); _chk(row_tok, I32, "im2col.row_tok"); _chk(out, F32, "im2col.out", 2)
    NF, C, H, W = v.shape
    assert out.shape[1] == C * 256 and out.shape[0] >= rows and row_img.numel() >= rows and row_tok.numel() >= rows and W % stride == 0 and H % stride == 0
    _call("avs_im2col_video_f32", v, row_img, row_tok, out, rows, C, H, W, int(stride), _xf_arg(xf, 2), _stream())


PLAN_FIELDS = 16      # int32 per sequence descriptor of avs_mask_plan (csrc/maskplan.hip PlanSeq; fields 12..15: the grouped decoder layout)
PLAN_CLASSIC = [-1, 0, 0, 0]      # fields 12..15 of a sequence in the classic (position-ordered) decoder layout


def mask_plan(seqs_dev, seqs_host, seed, row_src, row_tok, tmask_lo=None, tmask_hi=None, fmask=None, src_row=None, mask_out=None,
              ids_out=None, seed_dev=None, grouped=None):
    """Draw the random masks of every sequence in `seqs` on the device.  seqs_host (numpy int32 [nseq, PLAN_FIELDS]) is the host copy
    of seqs_dev used to validate every offset before the launch.  seed_dev (int64 [1] device tensor): the Philox key is read from it
    when the kernel runs instead of `seed` (graph_step: kernel arguments are frozen in a captured graph).
    grouped = (pos_row, row_of_pos, pred_id): the sequences with a decoder part are laid out in the GROUPED decoder order (scored rows of a
    sample first: csrc/maskplan.hip) and the three extra index arrays are written."""
    _chk(seqs_dev, I32, "plan.seqs", 2); _chk(row_src, I32, "plan.row_src"); _chk(row_tok, I32, "plan.row_tok")
    _chk(src_row, I32, "plan.src_row"); _chk(mask_out, F32, "plan.mask"); _chk(ids_out, I32, "plan.ids")
    for t in (tmask_lo, tmask_hi, fmask):
        _chk(t, I32, "plan.bitmask")
    nseq = seqs_host.shape[0]
    assert seqs_dev.shape == (nseq, PLAN_FIELDS) and seqs_host.shape[1] == PLAN_FIELDS
    L, keep, row_off, dec_off, t_p, ids_off, mask_off = (seqs_host[:, i] for i in (0, 1, 2, 4, 6, 7, 8))
    assert (L > 0).all() and (L <= 1024).all() and (keep >= 0).all() and (keep <= L).all()
    assert (row_off >= 0).all() and int((row_off + keep).max()) <= min(row_src.numel(), row_tok.numel())
    if (dec_off >= 0).any():
        sel = dec_off >= 0
        assert src_row is not None and mask_out is not None
        assert int((dec_off[sel] + L[sel]).max()) <= src_row.numel() and int((mask_off[sel] + L[sel]).max()) <= mask_out.numel()
        assert (mask_off[sel] >= 0).all()
    if (ids_off >= 0).any():
        sel = ids_off >= 0
        assert ids_out is not None and int((ids_off[sel] + L[sel]).max()) <= ids_out.numel()
    if (t_p > 0).any():
        assert all(t is not None and t.numel() >= nseq for t in (tmask_lo, tmask_hi, fmask))
        sel = t_p > 0
        # time patches: 64 bits in tmask_lo / tmask_hi + 32 in the descriptor (field 9, PlanSeq.tmask_x); frequency patches: 32 bits
        assert (t_p[sel] <= 96).all() and (L[sel] % t_p[sel] == 0).all() and (L[sel] // t_p[sel] <= 32).all()
    dm = seqs_host[:, 12]
    if grouped is None:
        assert (dm < 0).all(), "grouped decoder layout in the descriptors but no index arrays for it"
    else:
        pos_row, row_of_pos, pred_id = grouped
        _chk(pos_row, I32, "plan.pos_row"); _chk(row_of_pos, I32, "plan.row_of_pos"); _chk(pred_id, I32, "plan.pred_id")
        sel = dec_off >= 0
        assert sel.any() and (dm[sel] >= 0).all() and src_row is not None and mask_out is not None
        dk, po, pb = seqs_host[:, 13], seqs_host[:, 14], seqs_host[:, 15]
        nm = L - keep
        assert (dk[sel] >= 0).all() and (po[sel] >= 0).all() and (pb[sel] >= 0).all()
        assert int((dm[sel] + nm[sel]).max()) <= min(src_row.numel(), pos_row.numel()) and int((dk[sel] + keep[sel]).max()) <= min(src_row.numel(), pos_row.numel())
        assert int((dec_off[sel] + L[sel]).max()) <= row_of_pos.numel() and int((po[sel] + nm[sel]).max()) <= pred_id.numel()
        if seed_dev is not None:
            assert seed_dev.dtype == torch.int64 and seed_dev.is_cuda and seed_dev.numel() >= 1
        _call("avs_mask_plan_grouped", seqs_dev, nseq, tmask_lo, tmask_hi, fmask, (int(seed) & 0xFFFFFFFFFFFFFFFF) if seed_dev is None else 0, seed_dev,
              row_src, row_tok, src_row, mask_out, ids_out, pos_row, row_of_pos, pred_id, _stream())
        return
    if seed_dev is not None:
        assert seed_dev.dtype == torch.int64 and seed_dev.is_cuda and seed_dev.numel() >= 1
        _call("avs_mask_plan_dev", seqs_dev, nseq, tmask_lo, tmask_hi, fmask, seed_dev, row_src, row_tok, src_row, mask_out, ids_out, _stream())
        return
    _call("avs_mask_plan", seqs_dev, nseq, tmask_lo, tmask_hi, fmask, int(seed) & 0xFFFFFFFFFFFFFFFF, row_src, row_tok, src_row,
              mask_out, ids_out, _stream())


def cast_scale(x, y, n, alpha):
    _chk(x, F32, "cast.x"); _chk(y, BF16, "cast.y")
    assert x.numel() >= n and y.numel() >= n and n % 4 == 0
    _call("avs_cast_scale_bf16", x, y, n, float(alpha), _stream())


def scatter_add_rows(src, idx, dst, rows, scale=1.0):
    _chk(src, BF16, "scatter.src", 2); _chk(idx, I32, "scatter.idx"); _chk(dst, F32, "scatter.dst")
    D = src.shape[1]
    assert src.shape[0] >= rows and idx.numel() >= rows and dst.numel() % D == 0
    _call("avs_scatter_add_rows", src, idx, dst, rows, D, float(scale), _stream())


def colsum(x, out, rows):
    """out[c] += sum_r x[r, c]; x may be a column range of a wider row-major matrix (stride(1) == 1)"""
    if not (x.is_cuda and x.dtype == BF16 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.storage_offset() % 8 == 0):
        raise _lib.AvsiamHipError("colsum.x: need a row-major bf16 GPU matrix (or a column range of one, 16-byte aligned)")
    _chk(out, F32, "colsum.out")
    assert x.shape[0] >= rows and out.numel() == x.shape[1]
    _call("avs_colsum_bf16", x, x.stride(0), out, rows, x.shape[1], _stream())


def _chk_vecmat_w(W):
    """row-major bf16 [K, N] on the GPU, or a column range of a wider one (the kernels take the leading dimension): 8-byte aligned rows"""
    if not (W.is_cuda and W.dtype == BF16 and W.dim() == 2 and W.stride(1) == 1 and W.stride(0) >= W.shape[1] and W.stride(0) % 4 == 0
            and W.storage_offset() % 4 == 0):
        raise _lib.AvsiamHipError("vecmat.W: need a row-major bf16 GPU matrix (or a column range of one, 8-byte aligned)")


def vecmat(x, W, y, alpha=1.0):
    """y[n] += alpha * sum_k x[k] * W[k, n]   (x fp32 [K], W bf16 [K, N], y fp32 [N]); W may be a column range of a wider row-major matrix"""
    _chk(x, F32, "vecmat.x"); _chk_vecmat_w(W); _chk(y, F32, "vecmat.y")
    K, N = W.shape
    assert x.numel() == K and y.numel() == N and N % 256 == 0 and K % 32 == 0
    _call("avs_vecmat_bf16", x, W, W.stride(0), y, K, N, float(alpha), _stream())


class VecmatBatch:
    """y_i += x_i . W_i for many (x, W, y) of one shape with ONE launch (avs_vecmat_bf16_batched): the value thirds of a stack's qkv bias gradients"""

    def __init__(self):
        self.entries, self.keep, self.desc, self.shape = [], [], None, None

    def add(self, x, W, y):
        assert self.desc is None, "table already built"
        _chk(x, F32, "vecmat.x"); _chk_vecmat_w(W); _chk(y, F32, "vecmat.y")
        K, N = W.shape
        assert x.numel() == K and y.numel() == N and N % 256 == 0 and K % 32 == 0
        shape = (K, N, W.stride(0))
        assert self.shape in (None, shape), "one shape per batch"
        self.shape = shape
        self.entries.append((x.data_ptr(), W.data_ptr(), y.data_ptr()))
        self.keep.append((x, W, y))

    def build(self, dev):
        self.desc = torch.tensor(self.entries, dtype=torch.int64, device=dev)

    def run(self, alpha=1.0):
        K, N, ld = self.shape
        _call("avs_vecmat_bf16_batched", self.desc, len(self.entries), ld, K, N, float(alpha), _stream())


def unshuffle_fwd(x, src_row, pos_row, row_mod, mask_token, pos_a, pos_v, mod_a, mod_v, out, rows):
    _chk(x, F32, "unshuffle.x", 2); _chk(out, F32, "unshuffle.out", 2); _chk(src_row, I32, "unshuffle.src"); _chk(pos_row, I32, "unshuffle.pos")
    _chk(row_mod, U8, "unshuffle.mod")
    D = x.shape[1]
    for t in (mask_token, pos_a, pos_v, mod_a, mod_v):
        _chk(t, F32, "unshuffle.param")
    assert out.shape[1] == D and out.shape[0] >= rows and src_row.numel() >= rows and pos_row.numel() >= rows and row_mod.numel() >= rows
    assert mask_token.numel() == D and mod_a.numel() == D and mod_v.numel() == D
    _call("avs_unshuffle_fwd", x, src_row, pos_row, row_mod, mask_token, pos_a, pos_v, pos_a.numel() // D, mod_a, mod_v, out,
              rows, D, _stream())


def unshuffle_bwd(dout, src_row, B, T, La, Lv, dx, dpos_a, dpos_v, dmask, dmod_a, dmod_v, row_of_pos=None):
    """row_of_pos (grouped decoder layout): the decoder row of position (b, l); None: the rows are in position order"""
    _chk(dout, F32, "unshuffleb.dout", 2); _chk(dx, F32, "unshuffleb.dx", 2); _chk(src_row, I32, "unshuffleb.src"); _chk(row_of_pos, I32, "unshuffleb.map")
    D = dout.shape[1]
    assert dout.shape[0] >= B * (La + T * Lv) and src_row.numel() >= B * (La + T * Lv) and dx.shape[1] == D
    assert dpos_a.numel() == La * D and dpos_v.numel() == Lv * D and dmask.numel() == D
    assert row_of_pos is None or row_of_pos.numel() >= B * (La + T * Lv)
    _call("avs_unshuffle_bwd_map", dout, src_row, B, T, La, Lv, dx, dpos_a, dpos_v, dmask, dmod_a, dmod_v, D, row_of_pos, _stream())


def expand_rows(inp, src_row, out, rows, cols=None):
    """out[r, :cols] = inp[src_row[r], :cols] where src_row[r] >= 0, else 0 (bf16).  inp None: only the rows with src_row[r] < 0 are zeroed."""
    _chk(inp, BF16, "expand.in", 2); _chk(out, BF16, "expand.out", 2); _chk(src_row, I32, "expand.src")
    cols = out.shape[1] if cols is None else cols
    assert out.shape[0] >= rows and src_row.numel() >= rows and cols <= out.shape[1] and (inp is None or inp.shape[1] >= cols)
    _call("avs_expand_rows_bf16", inp, inp.stride(0) if inp is not None else 0, src_row, out, out.stride(0), rows, cols, _stream())


def segment_mean_fwd(y, seg_start, reps, nseg, row_map=None, max_row=None):
    """row_map (int32 [nseg], values < max_row <= reps rows; validated by the caller who built it): segment s -> reps[row_map[s]]"""
    _chk(y, F32, "segmean.y", 2); _chk(seg_start, I32, "segmean.seg"); _chk(reps, F32, "segmean.reps", 2); _chk(row_map, I32, "segmean.map")
    assert seg_start.numel() >= nseg + 1 and reps.shape[0] >= (nseg if row_map is None else max_row) and reps.shape[1] == y.shape[1]
    assert row_map is None or (row_map.numel() >= nseg and max_row is not None)
    _call("avs_segment_mean_fwd", y, seg_start, reps, nseg, y.shape[1], row_map, _stream())


def segment_mean_bwd(dreps, seg_start, dy, nseg, scale=1.0, row_map=None, max_row=None):
    _chk(dy, F32, "segmeanb.dy", 2); _chk(seg_start, I32, "segmeanb.seg"); _chk(dreps, F32, "segmeanb.dreps", 2); _chk(row_map, I32, "segmeanb.map")
    assert seg_start.numel() >= nseg + 1 and dreps.shape[0] >= (nseg if row_map is None else max_row) and dreps.shape[1] == dy.shape[1]
    assert row_map is None or (row_map.numel() >= nseg and max_row is not None)
    _call("avs_segment_mean_bwd", dreps, seg_start, dy, nseg, dy.shape[1], float(scale), row_map, _stream())


def segment_mean_bwd_acc(dreps, seg_start, dy, nseg, scale=1.0, row_map=None, max_row=None, accumulate=True):
    """segment_mean_bwd that ADDS to dy (accumulate=True): the pooled heads' gradient on token rows another branch already wrote"""
    _chk(dy, F32, "segmeanba.dy", 2); _chk(seg_start, I32, "segmeanba.seg"); _chk(dreps, F32, "segmeanba.dreps", 2); _chk(row_map, I32, "segmeanba.map")
    assert seg_start.numel() >= nseg + 1 and dreps.shape[0] >= (nseg if row_map is None else max_row) and dreps.shape[1] == dy.shape[1]
    assert row_map is None or (row_map.numel() >= nseg and max_row is not None)
    _call("avs_segment_mean_bwd_acc", dreps, seg_start, dy, nseg, dy.shape[1], float(scale), row_map, int(bool(accumulate)), _stream())


CLS_BCE, CLS_CE = 0, 1


def cls_loss(x, y, n, L, kind, row_loss, loss, dx=None, gout=None, weight=1.0):
    """BCE-with-logits (kind CLS_BCE) / cross-entropy with probability targets (CLS_CE) of logits x [>= n, >= L] (row-major, a column range of a
    padded buffer is fine) against targets y [n, L]: loss[0] = weight * mean loss, dx [n, >= L] = gout[0] * weight * d(mean)/dx (gout None: 1)"""
    for t, nm in ((x, "x"), (y, "y"), (dx, "dx")):
        if t is not None and not (t.is_cuda and t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= n and t.shape[1] >= L):
            raise _lib.AvsiamHipError(f"cls_loss.{nm}: need a row-major fp32 GPU matrix of at least [{n}, {L}]")
    _chk(row_loss, F32, "cls_loss.row_loss"); _chk(loss, F32, "cls_loss.loss"); _chk(gout, F32, "cls_loss.gout")
    assert kind in (CLS_BCE, CLS_CE) and row_loss.numel() >= n and loss.numel() >= 1
    _call("avs_cls_loss", x, x.stride(0), y, y.stride(0), n, L, kind, gout, float(weight), row_loss, loss, dx, dx.stride(0) if dx is not None else 0, _stream())


def mae_loss_fwd(pred, inp, mask, row_loss, loss, audio, L, nmask, total=None, total_init=True, xf=None, stride=16, row_id=None, id_base=0):
    """row_id / id_base (compact predictions: only the scored rows exist): prediction row r scores the (sample, token) row_id[r] - id_base of mask"""
    _chk(row_id, I32, "mae.row_id")
    _chk(pred, F32, "mae.pred", 2); _chk(inp, U8 if (xf is not None and not audio) else F32, "mae.inp"); _chk(mask, F32, "mae.mask"); _chk(row_loss, F32, "mae.row_loss"); _chk(loss, F32, "mae.loss")
    _chk(total, F32, "mae.total")
    rows = mask.numel()
    if audio:
        C, H, W = 1, inp.shape[1], inp.shape[2]          # [B, time, mel]
        assert inp.dim() == 3 and rows == inp.shape[0] * L and pred.shape[1] == 256 and (H // stride) * (W // stride) == L
    else:
        C, H, W = inp.shape[-3:]
        assert rows == inp.numel() // (C * H * W) * L and pred.shape[1] == 256 * C and (H // stride) * (W // stride) == L
    prows = rows if row_id is None else row_id.numel()
    assert pred.shape[0] >= prows and row_loss.numel() >= prows
    _call("avs_mae_loss_fwd_id", pred, inp, mask, row_loss, loss, total, int(bool(total_init)), prows, int(audio), L, C, H, W,
              float(nmask), int(stride), _xf_arg(xf, 1 if audio else 2, inp.shape[0] if audio else None), row_id, int(id_base), _stream())


def mae_loss_bwd(pred, inp, mask, gout, dpred, audio, L, nmask, xf=None, stride=16, row_id=None, id_base=0):
    _chk(row_id, I32, "maeb.row_id")
    _chk(pred, F32, "maeb.pred", 2); _chk(inp, U8 if (xf is not None and not audio) else F32, "maeb.inp"); _chk(mask, F32, "maeb.mask"); _chk(gout, F32, "maeb.gout"); _chk(dpred, BF16, "maeb.dpred", 2)
    rows = mask.numel()
    if audio:
        C, H, W = 1, inp.shape[1], inp.shape[2]
    else:
        C, H, W = inp.shape[-3:]
    prows = rows if row_id is None else row_id.numel()
    assert pred.shape[0] >= prows and dpred.shape[0] >= prows and dpred.shape[1] == pred.shape[1] == 256 * C
    _call("avs_mae_loss_bwd_id", pred, inp, mask, gout, dpred, prows, int(audio), L, C, H, W, float(nmask), int(stride),
              _xf_arg(xf, 1 if audio else 2, inp.shape[0] if audio else None), row_id, int(id_base), _stream())


def unpatchify(pred, inp, mask, audio, L, xf=None, stride=16, row_id=None, id_base=0, paste_kept=True, raw=False, row_loss=None, out=None, raw_out=None, err=None,
               model_units=True):
    """The way back from prediction rows (include/avsiam_hip.h: avs_unpatchify): -> (out, raw_out, err).  out: fp32 in the shape of ``inp``, the
    scored patches (mask 1; paste_kept False: every patch that has a row) from ``pred``, everything else ``inp`` through ``xf``.  raw: also the
    picture in the input's own units (audio fp32, frames uint8; needs xf without shift / amp), else raw_out is None.  row_loss: also the
    per-token error map err [mask.shape], else None.  out / raw_out / err: buffers to write into (the tests' guard bands); None allocates.
    model_units False (with raw): only the raw picture is wanted, out is None."""
    _chk(row_id, I32, "unp.row_id")
    _chk(pred, F32, "unp.pred", 2); _chk(inp, U8 if (xf is not None and not audio) else F32, "unp.inp"); _chk(mask, F32, "unp.mask"); _chk(row_loss, F32, "unp.row_loss")
    _chk(out, F32, "unp.out"); _chk(raw_out, F32 if audio else U8, "unp.raw_out"); _chk(err, F32, "unp.err")
    npos = mask.numel()
    if audio:
        C, H, W = 1, inp.shape[1], inp.shape[2]          # [B, time, mel]
        assert inp.dim() == 3
    else:
        assert inp.dim() >= 3
        C, H, W = inp.shape[-3:]
    n = inp.numel() // (C * H * W)
    assert npos == n * L and pred.shape[1] == 256 * C and (H // stride) * (W // stride) == L and 0 < stride <= 16
    prows = npos if row_id is None else row_id.numel()
    assert pred.shape[0] >= prows and (row_loss is None or row_loss.numel() >= prows)
    if raw:
        if xf is None:
            raise _lib.AvsiamHipError("unpatchify: raw=True needs the input transform it inverts (xf)")
        if xf.shift:
            raise _lib.AvsiamHipError("unpatchify: raw=True is refused with a per-sample shift / amp: a rolled, noised input has no original units")
    elif raw_out is not None:
        raise _lib.AvsiamHipError("unpatchify: raw_out given without raw=True")
    if err is not None and row_loss is None:
        raise _lib.AvsiamHipError("unpatchify: err given without row_loss")
    dev = pred.device
    if out is None and (model_units or not raw):
        out = torch.empty(inp.shape, dtype=F32, device=dev)
    if raw and raw_out is None:
        raw_out = torch.empty(inp.shape, dtype=F32 if audio else U8, device=dev)
    if row_loss is not None and err is None:
        err = torch.empty(mask.shape, dtype=F32, device=dev)
    assert (out is None or out.numel() >= inp.numel()) and (raw_out is None or raw_out.numel() >= inp.numel()) and (err is None or err.numel() >= npos)
    inv = torch.empty(npos, dtype=I32, device=dev) if row_id is not None else None
    _call("avs_unpatchify", pred, inp, mask, out, raw_out, row_loss, err, prows, int(audio), n, L, C, H, W, int(stride),
          _xf_arg(xf, 1 if audio else 2, inp.shape[0] if audio else None), row_id, int(id_base), inv, int(bool(paste_kept)), _stream())
    return out, raw_out, err


def l2norm_fwd(x, xn, norm):
    _chk(x, F32, "l2.x", 2); _chk(xn, F32, "l2.xn", 2); _chk(norm, F32, "l2.norm")
    assert xn.shape == x.shape and norm.numel() >= x.shape[0]
    _call("avs_l2norm_fwd", x, xn, norm, x.shape[0], x.shape[1], _stream())


def l2norm_bwd(dxn, xn, norm, dx, scale=1.0):
    for t in (dxn, xn, dx):
        _chk(t, F32, "l2b", 2)
    _chk(norm, F32, "l2b.norm")
    assert dxn.shape == xn.shape == dx.shape
    _call("avs_l2norm_bwd", dxn, xn, norm, dx, xn.shape[0], xn.shape[1], float(scale), _stream())


def gemm_f32_small(A, B, C, M, N, K, sa, sb, alpha=1.0):
    """C[M,N] = alpha * sum_k A(m,k) B(k,n); sa = (stride_m, stride_k) of A, sb = (stride_k, stride_n) of B, in elements."""
    _chk(A, F32, "sgemm.A"); _chk(B, F32, "sgemm.B"); _chk(C, F32, "sgemm.C", 2)
    assert C.shape[0] >= M and C.shape[1] == N
    assert (M - 1) * sa[0] + (K - 1) * sa[1] < A.numel() and (K - 1) * sb[0] + (N - 1) * sb[1] < B.numel()
    _call("avs_gemm_f32_small", A, sa[0], sa[1], B, sb[0], sb[1], C, C.stride(0), M, N, K, float(alpha), _stream())


def infonce_fwd(total, stats, out, weight=1.0):
    """out = {nce, c_acc, weight * nce}"""
    _chk(total, F32, "nce.total", 2); _chk(stats, F32, "nce.stats", 2); _chk(out, F32, "nce.out")
    N = total.shape[0]
    assert total.shape[1] == N and stats.shape == (N, 4) and out.numel() >= 3
    _call("avs_infonce_fwd", total, stats, out, N, float(weight), _stream())


def infonce_dlogits(total, stats, gout, weight, dtotal):
    _chk(total, F32, "nceb.total", 2); _chk(stats, F32, "nceb.stats", 2); _chk(gout, F32, "nceb.gout"); _chk(dtotal, F32, "nceb.dtotal", 2)
    N = total.shape[0]
    assert dtotal.shape == total.shape
    _call("avs_infonce_dlogits", total, stats, gout, float(weight), dtotal, N, _stream())


def transpose_bf16(x, out):
    _chk(x, BF16, "tr.x", 2); _chk(out, BF16, "tr.out", 2)
    assert out.shape == (x.shape[1], x.shape[0])
    _call("avs_transpose_bf16", x, out, x.shape[0], x.shape[1], _stream())


def transpose_batched(desc, tile_map, ntiles):
    """desc: int64 [nmat, 6] on the device, built (and bounds-checked) by ParamArena from its own views."""
    _chk(desc, torch.int64, "trb.desc", 2); _chk(tile_map, I32, "trb.map")
    assert desc.shape[1] == 6 and tile_map.numel() == ntiles
    _call("avs_transpose_batched", desc, tile_map, ntiles, _stream())


def cast_bf16(x, y, n):
    _chk(x, F32, "castb.x"); _chk(y, BF16, "castb.y")
    assert x.numel() >= n and y.numel() >= n
    _call("avs_cast_bf16", x, y, n, _stream())


def adam(p, g, m, v, p_bf16, n, lr, step, beta1=0.95, beta2=0.999, eps=1e-8, weight_decay=5e-7, grad_scale=1.0, step_dev=None):
    """step_dev (int32 [1] device tensor): the step count is read from it when the kernel runs instead of `step` (graph_step)"""
    for t in (p, g, m, v):
        _chk(t, F32, "adam")
    _chk(p_bf16, BF16, "adam.p_bf16")
    assert n % 4 == 0 and all(t.numel() >= n for t in (p, g, m, v)) and (p_bf16 is None or p_bf16.numel() >= n)
    if step_dev is not None:
        assert step_dev.dtype == torch.int32 and step_dev.is_cuda and step_dev.numel() >= 1
        _call("avs_adam_dev", p, g, m, v, p_bf16, n, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), step_dev,
              float(grad_scale), _stream())
        return
    _call("avs_adam", p, g, m, v, p_bf16, n, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
              float(grad_scale), _stream())


ADAM_TABLE_NCLS, ADAM_TABLE_NGROUP = 16, 3


def adam_table_geometry():
    """(workgroups, elements per chunk, largest n_segs) of avs_adam_table's update kernel"""
    grid, chunk, segs = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().avs_adam_table_geometry(ctypes.byref(grid), ctypes.byref(chunk), ctypes.byref(segs))
    return grid.value, chunk.value, segs.value


class AdamCtl:
    """avs_adam_ctl on the device, {float lr[3]; int step[16]; float live[16]}: ONE 35-word buffer with typed views.  `live` is a contiguous
    fp32 view an all-reduce can sum in place."""

    def __init__(self, device):
        self.buf = torch.zeros(3 + 2 * ADAM_TABLE_NCLS, dtype=F32, device=device)
        self.lr = self.buf[:3]
        self.step = self.buf[3:3 + ADAM_TABLE_NCLS].view(I32)
        self.live = self.buf[3 + ADAM_TABLE_NCLS:]

    def set_lr(self, lr_base, lr_head, lr_mm):
        """the three rates by value, through a one-thread kernel on the current stream (no staging buffer to race with a step in flight)"""
        _call("avs_adam_table_set_lr", self.buf, float(lr_base), float(lr_head), float(lr_mm), _stream())


class AdamTable:
    """avs_adam_seg[] on the device, validated on the host when it is built: segs = [(lo, n, group, cls), ...] with lo, n multiples of 4,
    n > 0, 0 <= lo, lo + n <= limit, group 0..2, cls 0..ncls-1 (ncls <= 16), no two segments overlapping."""

    def __init__(self, segs, ncls, limit, device):
        import numpy as np
        segs = [tuple(int(x) for x in s) for s in segs]
        _, chunk, max_segs = adam_table_geometry()
        if not 1 <= ncls <= ADAM_TABLE_NCLS:
            raise _lib.AvsiamHipError(f"adam_table: ncls {ncls} out of range (1..{ADAM_TABLE_NCLS})")
        if not 1 <= len(segs) <= max_segs:
            raise _lib.AvsiamHipError(f"adam_table: {len(segs)} segments (1..{max_segs})")
        end = 0
        for lo, n, grp, cls in sorted(segs):
            if n <= 0 or n % 4 or lo % 4 or lo < end or lo + n > limit or n >= 1 << 31:
                raise _lib.AvsiamHipError(f"adam_table: segment [{lo}, {lo + n}) is empty, misaligned, overlaps its neighbour or leaves the arena ({limit})")
            if not 0 <= grp < ADAM_TABLE_NGROUP or not 0 <= cls < ncls:
                raise _lib.AvsiamHipError(f"adam_table: segment [{lo}, {lo + n}): group {grp} / class {cls} out of range")
            end = lo + n
        host = np.zeros(len(segs), dtype=np.dtype([("lo", "<i8"), ("n", "<i4"), ("group", "<i4"), ("cls", "<i4"), ("pad", "<i4")]))
        for i, s in enumerate(segs):
            host[i] = s + (0,)
        self.segs, self.ncls, self.limit = segs, ncls, limit
        self.chunks = sum((n + chunk - 1) // chunk for _, n, _, _ in segs)            # sizes the grid (avs_adam_table_sized)
        self.dev = torch.from_numpy(host.view(np.uint8).copy()).to(device)


def adam_table(p, g, m, v, p_bf16, table: AdamTable, ctl: AdamCtl, beta1=0.95, beta2=0.999, eps=1e-8, weight_decay=5e-7, grad_scale=1.0,
               sized=True):
    """Adam over every segment of `table` whose class is live in `ctl`, one launch; then ctl.step += (ctl.live > 0).  p, g, m, v (and p_bf16)
    share the table's element offsets and hold at least table.limit elements.  sized=False: the full grid of avs_adam_table instead of one
    bounded by the table's chunk count (the same bytes)."""
    for t in (p, g, m, v):
        _chk(t, F32, "adam_table")
    _chk(p_bf16, BF16, "adam_table.p_bf16")
    _chk(table.dev, U8, "adam_table.segs"); _chk(ctl.buf, F32, "adam_table.ctl")
    assert all(t.numel() >= table.limit for t in (p, g, m, v)) and (p_bf16 is None or p_bf16.numel() >= table.limit)
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v)) and (p_bf16 is None or p_bf16.data_ptr() % 8 == 0)
    if not sized:
        _call("avs_adam_table", p, g, m, v, p_bf16, table.dev, len(table.segs), ctl.buf, float(beta1), float(beta2), float(eps),
              float(weight_decay), float(grad_scale), _stream())
        return
    _call("avs_adam_table_sized", p, g, m, v, p_bf16, table.dev, len(table.segs), table.chunks, ctl.buf, float(beta1), float(beta2), float(eps),
          float(weight_decay), float(grad_scale), _stream())


# ---- the guard of the fine-tuning step: gradient norm, clipping coefficient, non-finite skip (csrc/grad_guard.hip) -----------------------------
class GradGuard:
    """avs_grad_guard on the device, {double sumsq[3], sumsq_cls[16], total; float norm, coef; int n_nonfinite, skip, n_skipped, n_steps}:
    ONE 184-byte buffer with typed views, zeroed here (n_skipped and n_steps count from its creation), and the workspace of grad_sumsq,
    grown when a table needs more."""

    def __init__(self, device):
        self.buf = torch.zeros(23, dtype=torch.float64, device=device)
        self.sumsq, self.sumsq_cls, self.total = self.buf[:3], self.buf[3:3 + ADAM_TABLE_NCLS], self.buf[19:20]
        tail = self.buf[20:]
        self.norm, self.coef = tail.view(F32)[0:1], tail.view(F32)[1:2]
        self.n_nonfinite, self.skip, self.n_skipped, self.n_steps = (tail.view(I32)[i:i + 1] for i in range(2, 6))
        self.ws = None

    def workspace(self, table):
        """-> (buffer, bytes grad_sumsq needs for `table`)"""
        need = _lib.load().avs_grad_sumsq_ws_bytes(len(table.segs), table.chunks)
        if need == 0:
            raise _lib.AvsiamHipError(f"grad_sumsq: no workspace size for {len(table.segs)} segments / {table.chunks} chunks")
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.zeros(need, dtype=U8, device=self.buf.device)
        return self.ws, need

    def read(self):
        """the block as a dict of host numbers (synchronises)"""
        import numpy as np
        raw = self.buf.cpu().numpy()
        f, i = raw[20:].view(np.float32), raw[20:].view(np.int32)
        return {"sumsq": raw[:3].copy(), "sumsq_cls": raw[3:19].copy(), "total": float(raw[19]), "norm": float(f[0]), "coef": float(f[1]),
                "n_nonfinite": int(i[2]), "skip": int(i[3]), "n_skipped": int(i[4]), "n_steps": int(i[5])}


def grad_sumsq(g, table: AdamTable, ctl: AdamCtl, guard: GradGuard, grad_scale=1.0, max_norm=float("inf")):
    """guard <- the squared norm of `g` over every segment of `table` whose class is live in `ctl` (fp64, non-finite elements counted and
    left out), by group and by class, and from it norm = sqrt(total) * grad_scale, skip and the clip_grad_norm_ coefficient of max_norm
    (include/avsiam_hip.h, avs_grad_sumsq).  Two launches on the current stream, no host sync."""
    _chk(g, F32, "grad_sumsq.g")
    _chk(table.dev, U8, "grad_sumsq.segs"); _chk(ctl.buf, F32, "grad_sumsq.ctl"); _chk(guard.buf, torch.float64, "grad_sumsq.guard")
    assert g.numel() >= table.limit and g.data_ptr() % 16 == 0
    if not max_norm > 0:
        raise _lib.AvsiamHipError(f"grad_sumsq: max_norm must be > 0 (inf: no clipping), got {max_norm}")
    ws, need = guard.workspace(table)
    _call("avs_grad_sumsq", g, table.dev, len(table.segs), ctl.buf, float(grad_scale), float(max_norm), guard.buf, ws, need, _stream())


def adam_table_guarded(p, g, m, v, p_bf16, table: AdamTable, ctl: AdamCtl, guard: GradGuard, beta1=0.95, beta2=0.999, eps=1e-8,
                       weight_decay=5e-7, grad_scale=1.0):
    """adam_table with the block grad_sumsq wrote: guard.skip set - nothing is written and ctl.step stays; otherwise the update with the
    gradient scale fl32(grad_scale * guard.coef), read on the device."""
    for t in (p, g, m, v):
        _chk(t, F32, "adam_table_guarded")
    _chk(p_bf16, BF16, "adam_table_guarded.p_bf16")
    _chk(table.dev, U8, "adam_table_guarded.segs"); _chk(ctl.buf, F32, "adam_table_guarded.ctl")
    _chk(guard.buf, torch.float64, "adam_table_guarded.guard")
    assert all(t.numel() >= table.limit for t in (p, g, m, v)) and (p_bf16 is None or p_bf16.numel() >= table.limit)
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v)) and (p_bf16 is None or p_bf16.data_ptr() % 8 == 0)
    _call("avs_adam_table_guarded", p, g, m, v, p_bf16, table.dev, len(table.segs), table.chunks, ctl.buf, float(beta1), float(beta2),
          float(eps), float(weight_decay), float(grad_scale), guard.buf, _stream())


def grad_guard_reference(g, segs, live, grad_scale=1.0, max_norm=float("inf")):
    """The numpy restatement of avs_grad_sumsq, the yardstick of its tests.  g: float array; segs: [(lo, n, group, cls), ...] - a segment that
    breaks avs_adam_table's rules owns nothing; live: per-class liveness (> 0: live).  Sums in float64 by math.fsum (exactly rounded), the
    coefficient in fp32 as the kernel and torch.nn.utils.clip_grad_norm_ write it.  -> dict with the fields of GradGuard.read() but the
    cumulative counters, and norm64 / coef64: norm and coef without the fp32 roundings."""
    import math
    import numpy as np
    g = np.asarray(g)
    f32 = np.float32
    by_group = [[] for _ in range(ADAM_TABLE_NGROUP)]
    by_cls = [[] for _ in range(ADAM_TABLE_NCLS)]
    bad = 0
    for lo, n, grp, cls in segs:
        if n <= 0 or n % 4 or lo < 0 or lo % 4 or not 0 <= grp < ADAM_TABLE_NGROUP or not 0 <= cls < ADAM_TABLE_NCLS:
            continue
        if not (cls < len(live) and live[cls] > 0):
            continue
        x = g[lo:lo + n].astype(np.float64)
        fin = np.abs(x) <= float(np.finfo(np.float32).max) if g.dtype == np.float32 else np.isfinite(x)
        bad += int((~fin).sum())
        sq = (x[fin] * x[fin]).tolist()
        by_group[grp] += sq
        by_cls[cls] += sq
    sumsq = np.array([math.fsum(s) for s in by_group], dtype=np.float64)
    sumsq_cls = np.array([math.fsum(s) for s in by_cls], dtype=np.float64)
    total = (sumsq[0] + sumsq[1]) + sumsq[2]
    norm = f32(math.sqrt(total) * float(f32(grad_scale)))
    skip = int(bad > 0)
    with np.errstate(over="ignore"):
        coef = f32(0.0) if skip else min(f32(1.0), f32(max_norm) / (norm + f32(1e-6)))
    norm64 = math.sqrt(total) * float(grad_scale)                 # the same two formulas before the block's fp32 roundings
    coef64 = 0.0 if skip else min(1.0, float(max_norm) / (norm64 + 1e-6))
    return {"sumsq": sumsq, "sumsq_cls": sumsq_cls, "total": float(total), "norm": float(norm), "coef": float(coef), "n_nonfinite": bad,
            "skip": skip, "norm64": norm64, "coef64": coef64}


# ---- gradient accumulation over micro-batches (csrc/grad_accum.hip) ---------------------------------------------------------------------------
class GradAccumCtl:
    """avs_grad_accum_ctl on the device, {float live[16]; int n_micro; int n_cycles}: ONE 72-byte buffer with typed views, zeroed here.  live:
    the gradient classes the micro-steps of the running cycle reached; n_micro: micro-steps in it; n_cycles: cycles published."""

    def __init__(self, device):
        self.buf = torch.zeros(ADAM_TABLE_NCLS + 2, dtype=F32, device=device)
        self.live = self.buf[:ADAM_TABLE_NCLS]
        self.n_micro = self.buf[ADAM_TABLE_NCLS:ADAM_TABLE_NCLS + 1].view(I32)
        self.n_cycles = self.buf[ADAM_TABLE_NCLS + 1:].view(I32)

    def read(self):
        """the block as a dict of host numbers (synchronises)"""
        import numpy as np
        raw = self.buf.cpu().numpy()
        i = raw[ADAM_TABLE_NCLS:].view(np.int32)
        return {"live": raw[:ADAM_TABLE_NCLS].copy(), "n_micro": int(i[0]), "n_cycles": int(i[1])}


def grad_accum(acc, g, table: AdamTable, ctl: AdamCtl, actl: GradAccumCtl, first, publish):
    """One micro-step's gradients `g` into `acc` over every segment of `table` whose class is live in `ctl`: a copy when `first` is set or the
    class has not been touched in this cycle (actl.live), one fp32 add per element otherwise; then actl.live <- the cycle's union, and with
    `publish` ctl.live <- that union (include/avsiam_hip.h, avs_grad_accum).  acc and g share the table's element offsets and do not overlap.
    Two launches on the current stream, no host sync."""
    _chk(acc, F32, "grad_accum.acc"); _chk(g, F32, "grad_accum.g")
    _chk(table.dev, U8, "grad_accum.segs"); _chk(ctl.buf, F32, "grad_accum.ctl"); _chk(actl.buf, F32, "grad_accum.actl")
    assert acc.numel() >= table.limit and g.numel() >= table.limit and acc.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    lo, hi = acc.data_ptr(), acc.data_ptr() + 4 * table.limit
    if g.data_ptr() < hi and lo < g.data_ptr() + 4 * table.limit:
        raise _lib.AvsiamHipError("grad_accum: acc and g overlap")
    _call("avs_grad_accum", acc, g, table.dev, len(table.segs), table.chunks, ctl.buf, actl.buf, int(bool(first)), int(bool(publish)), _stream())


def grad_accum_reference(acc, g, segs, live, acc_live, first):
    """The numpy restatement of avs_grad_accum, the yardstick of its tests.  acc, g: float32 arrays; segs: [(lo, n, group, cls), ...] - a segment
    that breaks avs_adam_table's rules owns nothing; live: per-class liveness of this micro-step (> 0: live); acc_live: the cycle's union so
    far (ignored when `first`).  -> (the new acc - a copy; untouched outside the segments of classes live now, the bits of g where a class is
    first touched, acc + g in fp32 elsewhere -, the new acc_live as 0.0 / 1.0 over the 16 classes, the vector a publishing call writes to
    ctl.live: the same union)."""
    import numpy as np
    acc = np.array(acc, dtype=np.float32, copy=True)
    g = np.asarray(g, dtype=np.float32)
    now = [c < len(live) and live[c] > 0 for c in range(ADAM_TABLE_NCLS)]
    had = [(not first) and c < len(acc_live) and acc_live[c] > 0 for c in range(ADAM_TABLE_NCLS)]
    for lo, n, grp, cls in segs:
        if n <= 0 or n % 4 or lo < 0 or lo % 4 or not 0 <= grp < ADAM_TABLE_NGROUP or not 0 <= cls < ADAM_TABLE_NCLS:
            continue
        if not now[cls]:
            continue
        if had[cls]:
            with np.errstate(invalid="ignore", over="ignore"):
                acc[lo:lo + n] = acc[lo:lo + n] + g[lo:lo + n]
        else:
            acc[lo:lo + n] = g[lo:lo + n]
    union = np.array([1.0 if (h or w) else 0.0 for h, w in zip(had, now)], dtype=np.float32)
    return acc, union, union.copy()


# ---- retrieval evaluation -------------------------------------------------------------------------------------------------------------
RETRIEVAL_MAX_TOPK = 16
_retr_ws = {}            # (device, stream) -> cached workspace: calls on different streams never share one; grown when a call needs more, so no
                         # allocation per call after the first of a shape.  retrieval_rank_release() drops them


def _chk_rows(t, name):
    """fp32 [n, D] on the GPU whose rows are dense (a row range or row-strided view of a feature buffer is fine)"""
    if not t.is_cuda:
        raise _lib.AvsiamHipError(f"{name}: tensor must live on the GPU")
    if t.dtype != F32:
        raise _lib.AvsiamHipError(f"{name}: expected {F32}, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise _lib.AvsiamHipError(f"{name}: expected a non-empty [n, D] matrix, got {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise _lib.AvsiamHipError(f"{name}: rows must be dense (strides {t.stride()})")


def retrieval_rank_ws_bytes(nq, ng, topk=0):
    return int(_lib.load().avs_retrieval_rank_ws_bytes(int(nq), int(ng), int(topk)))


def retrieval_rank_release():
    """free the cached workspaces (16 MiB after a 65 536-clip call with topk = 16)"""
    _retr_ws.clear()


def retrieval_rank(q, g, target=None, topk=0, want_sim=False, ws=None):
    """Rank every query's true match in the gallery without materialising the similarity matrix (src/retrieval.py:32-52).

    q [nq, D], g [ng, D] fp32 (normalised or not); s = q @ g.T in exact fp32, one k-ascending chain per element.  target: int32 [nq] gallery
    index of each query's match (None: query i matches gallery entry i; needs nq <= ng; values must lie in 0..ng-1 - a value outside is
    not read and gives target_sim NaN, rank 0).  Returns a dict of device tensors:
      rank [nq] int32        number of OTHER gallery entries strictly more similar than the match (0 = retrieved first)
      ties [nq] int32        number of other entries exactly as similar as the match.  The reference's compute_metrics emits one entry per tied
                             column (so its len(ind) exceeds N); here the optimistic rank and the tie count are reported instead
      target_sim [nq] fp32   s[i, target[i]], the very bits the comparison used
      topk_idx / topk_sim    [nq, topk] (topk in 1..16): best entries by (similarity descending, index ascending); -1 / -inf beyond ng
      sim [nq, ng]           only with want_sim
    ws: a uint8 device tensor of at least retrieval_rank_ws_bytes(nq, ng, topk) bytes from the caller's pool; None: a cached one.
    Deterministic: two calls return identical bytes."""
    _chk_rows(q, "retrieval.q"); _chk_rows(g, "retrieval.g")
    nq, D = q.shape
    ng = g.shape[0]
    if g.shape[1] != D or g.device != q.device:
        raise _lib.AvsiamHipError(f"retrieval: q {tuple(q.shape)} on {q.device} and g {tuple(g.shape)} on {g.device} do not match")
    topk = int(topk)
    if not 0 <= topk <= RETRIEVAL_MAX_TOPK:
        raise _lib.AvsiamHipError(f"retrieval: topk = {topk} outside 0..{RETRIEVAL_MAX_TOPK}")
    if target is None:
        if nq > ng:
            raise _lib.AvsiamHipError(f"retrieval: target=None pairs query i with gallery entry i, but nq = {nq} > ng = {ng}")
    else:
        _chk(target, I32, "retrieval.target", 1)
        if target.numel() != nq or target.device != q.device:
            raise _lib.AvsiamHipError(f"retrieval.target: expected {nq} indices on {q.device}, got {tuple(target.shape)} on {target.device}")
    dev = q.device
    need = retrieval_rank_ws_bytes(nq, ng, topk)
    if ws is None:
        key = (dev, _stream())
        ws = _retr_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _retr_ws[key] = torch.empty(need, dtype=U8, device=dev)
    else:
        _chk(ws, U8, "retrieval.ws")
        if ws.numel() < need or ws.device != dev:
            raise _lib.AvsiamHipError(f"retrieval.ws: {ws.numel()} bytes on {ws.device}, need {need} on {dev}")
    out = {"rank": torch.empty(nq, dtype=I32, device=dev), "ties": torch.empty(nq, dtype=I32, device=dev),
           "target_sim": torch.empty(nq, dtype=F32, device=dev)}
    if topk:
        out["topk_idx"] = torch.empty((nq, topk), dtype=I32, device=dev)
        out["topk_sim"] = torch.empty((nq, topk), dtype=F32, device=dev)
    if want_sim:
        out["sim"] = torch.empty((nq, ng), dtype=F32, device=dev)
    ldq = q.stride(0) if nq > 1 else D
    ldg = g.stride(0) if ng > 1 else D
    _launch("retrieval_rank", 2.0 * nq * ng * D, "avs_retrieval_rank", q, ldq, nq, g, ldg, ng, D, target, out["rank"], out["ties"], out["target_sim"],
            topk, out.get("topk_idx"), out.get("topk_sim"), out.get("sim"), ng if want_sim else 0, ws, ws.numel(), _stream())
    return out


# ---- classification metrics (fine-tuning validation) ----------------------------------------------------------------------------------
CLS_STATS_TILE = 2048    # csrc/metrics.hip CS_TILE: scores of a class staged in LDS at a time
CLS_STATS_PPW = 64       # csrc/metrics.hip CS_PPW: positives per workgroup (a chunk; also the unit of ap_sum's summation order)
CLS_STATS_MAX_N = 1 << 22
_cls_ws = {}             # (device, stream) -> cached workspace, as _retr_ws.  classification_stats_release() drops them


def classification_stats_ws_bytes(S, N, C):
    return int(_lib.load().avs_cls_stats_ws_bytes(int(S), int(N), int(C)))


def classification_stats_release():
    """free the cached workspaces (about 4 (S + 1.3) N C bytes each: 0.55 GB after a call with 11 sets of 20 000 x 527)"""
    _cls_ws.clear()


def cls_stats_views(buf, S, C):
    """the five results inside the packed byte buffer of classification_stats (a device tensor or its host copy) -> dict of [S, C] / [S] views"""
    sc = S * C
    o_np = 16 * sc
    o_s = o_np + (4 * sc + 7) // 8 * 8
    return {"ap_sum": buf[:8 * sc].view(torch.float64).view(S, C), "auc_num": buf[8 * sc:16 * sc].view(torch.int64).view(S, C),
            "n_pos": buf[o_np:o_np + 4 * sc].view(I32).view(S, C), "n_correct": buf[o_s:o_s + 4 * S].view(I32),
            "n_nonfinite": buf[o_s + 4 * S:o_s + 8 * S].view(I32)}


def classification_stats(scores, target, ws=None):
    """Exact per-class counts behind mAP / mAUC / acc (utilities/stats.py calculate_stats) of S prediction sets against one target, on the device.

    scores fp32 [N, C] or [S, N, C], target fp32 [N, C] (positives: > 0.5); the class axis is dense, rows (and sets) may be strided views with
    strides of at least the dense ones.  N <= 2^22.  Returns a dict of device tensors, [S, C] / [S] ([C] / 0-dim for a 2-D `scores`):
      n_pos int32        P, the positives of the class
      auc_num int64      sum over positives of 2 #{negatives below} + #{negatives tied}: AUC = auc_num / (2 P (N - P)), exact
      ap_sum float64     sum over positives of #{positives >= s_i} / #{all >= s_i}: AP = ap_sum / P with tied scores sharing a threshold (sklearn's
                         definition); the summation order is fixed by the positives' sample indices alone
      n_correct int32    rows whose first-index argmax equals that of the binarised target row (numpy.argmax semantics)
      n_nonfinite int32  NaN scores of the set; when it is not 0 the set's other results mean nothing (the call itself does not fault)
      packed uint8       the buffer the five are views of (cls_stats_views): ONE device-to-host copy fetches everything
    No host synchronisation.  ws: a uint8 device tensor of at least classification_stats_ws_bytes(S, N, C) bytes; None: a cached one.
    Deterministic: two calls return identical bytes, and S sets in one call the bytes of S separate calls."""
    for t, name in ((scores, "classification_stats.scores"), (target, "classification_stats.target")):
        if not t.is_cuda:
            raise _lib.AvsiamHipError(f"{name}: tensor must live on the GPU")
        if t.dtype != F32:
            raise _lib.AvsiamHipError(f"{name}: expected {F32}, got {t.dtype}")
    squeeze = scores.dim() == 2
    if squeeze:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3 or target.dim() != 2 or min(scores.shape) < 1 or tuple(scores.shape[1:]) != tuple(target.shape):
        raise _lib.AvsiamHipError(f"classification_stats: scores {tuple(scores.shape)} and target {tuple(target.shape)}: expected [S, N, C] or [N, C] "
                                  "and [N, C], none of them empty")
    if scores.device != target.device:
        raise _lib.AvsiamHipError(f"classification_stats: scores on {scores.device}, target on {target.device}")
    S, N, C = scores.shape
    if N > CLS_STATS_MAX_N:
        raise _lib.AvsiamHipError(f"classification_stats: N = {N} above {CLS_STATS_MAX_N}")
    row = scores.stride(1) if N > 1 else C
    sset = scores.stride(0) if S > 1 else N * C
    ldt = target.stride(0) if N > 1 else C
    if scores.stride(2) != 1 or row < C or sset < N * C:
        raise _lib.AvsiamHipError(f"classification_stats.scores: the class axis must be dense and the row / set strides at least C / N * C (strides {scores.stride()})")
    if target.stride(1) != 1 or ldt < C:
        raise _lib.AvsiamHipError(f"classification_stats.target: rows must be dense (strides {target.stride()})")
    dev = scores.device
    need = classification_stats_ws_bytes(S, N, C)
    if need == 0:
        raise _lib.AvsiamHipError(f"classification_stats: shape S={S} N={N} C={C} is outside what avs_cls_stats accepts")
    if ws is None:
        key = (dev, _stream())
        ws = _cls_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _cls_ws[key] = torch.empty(need, dtype=U8, device=dev)
    else:
        _chk(ws, U8, "classification_stats.ws")
        if ws.numel() < need or ws.device != dev:
            raise _lib.AvsiamHipError(f"classification_stats.ws: {ws.numel()} bytes on {ws.device}, need {need} on {dev}")
    # zero-filled: the alignment gap behind n_pos belongs to the bytes a caller may compare or hash
    packed = torch.zeros(16 * S * C + (4 * S * C + 7) // 8 * 8 + 8 * S, dtype=U8, device=dev)
    out = cls_stats_views(packed, S, C)
    # work: the comparisons of the counting pass are data-dependent (N * sum_k P_k); the estimate prices the transposing and argmax passes' bytes
    _launch("cls_stats", (0.0, 12.0 * S * N * C), "avs_cls_stats", scores, sset, row, S, N, C, target, ldt, out["n_pos"], out["auc_num"], out["ap_sum"],
            out["n_correct"], out["n_nonfinite"], ws, ws.numel(), _stream())
    if squeeze:
        out = {k: v[0] for k, v in out.items()}
    out["packed"] = packed
    return out


# ---- waveform input (fine-tuning loader: dataloader_ft.py:277-340, 441-458) -------------------------------------------------------------
FBANK_FRAME, FBANK_SHIFT, FBANK_NMEL = 400, 160, 128      # csrc/frontend_math.h


def _per_clip(x, B, dtype, name, dev, lo=None, hi=None):
    """a per-clip vector for a kernel: None stays None; a device tensor is taken as it is (its values are the caller's word - nothing here
    synchronises to read them); host values (sequence, numpy, CPU tensor) are range-checked and uploaded"""
    if x is None:
        return None
    if torch.is_tensor(x) and x.is_cuda:
        _chk(x, dtype, name, 1)
        if x.numel() != B or x.device != dev:
            raise _lib.AvsiamHipError(f"{name}: expected {B} values on {dev}, got {tuple(x.shape)} on {x.device}")
        return x
    h = torch.as_tensor(x).reshape(-1)
    if h.numel() != B:
        raise _lib.AvsiamHipError(f"{name}: expected {B} values, got {h.numel()}")
    if lo is not None and B and (int(h.min()) < lo or int(h.max()) > hi):
        raise ValueError(f"{name}: values must lie in {lo} .. {hi}, got {h.tolist()}")
    return h.to(dtype).to(dev)


def wave_sums(wave, lengths=None, partner=None, partner_lengths=None, out=None):
    """The three sums per clip the fbank's sample read needs (avs_wave_sums): [B, 3] float64 = sum w1 over its length, sum w2 over its length,
    sum w2 over min of the two lengths (the last two 0 without a partner).  wave / partner fp32 [B, stride]; lengths / partner_lengths int32
    device tensors or None (the stride).  One fixed-order reduction per clip: two calls give identical bytes."""
    _chk(wave, F32, "wave_sums.wave", 2)
    B = wave.shape[0]
    _chk(lengths, I32, "wave_sums.lengths", 1); _chk(partner, F32, "wave_sums.partner", 2); _chk(partner_lengths, I32, "wave_sums.partner_lengths", 1)
    if partner is not None and (partner.shape[0] != B or partner.device != wave.device):
        raise _lib.AvsiamHipError(f"wave_sums: partner {tuple(partner.shape)} on {partner.device} does not match wave {tuple(wave.shape)} on {wave.device}")
    for t, name in ((lengths, "lengths"), (partner_lengths, "partner_lengths")):
        if t is not None and (t.numel() != B or t.device != wave.device):
            raise _lib.AvsiamHipError(f"wave_sums.{name}: expected {B} values on {wave.device}")
    if partner is None and partner_lengths is not None:
        raise _lib.AvsiamHipError("wave_sums: partner_lengths without a partner")
    if out is None:
        out = torch.empty((B, 3), dtype=torch.float64, device=wave.device)
    else:
        _chk(out, torch.float64, "wave_sums.out", 2)
        if tuple(out.shape) != (B, 3) or out.device != wave.device:
            raise _lib.AvsiamHipError(f"wave_sums.out: expected [{B}, 3] on {wave.device}, got {tuple(out.shape)} on {out.device}")
    _call("avs_wave_sums", wave, wave.shape[1], lengths, partner, partner.shape[1] if partner is not None else 0, partner_lengths, B, out, _stream())
    return out


def kaldi_fbank(wave, lengths=None, *, partner=None, partner_lengths=None, lam=None, target_length=1024, n_mels=128, norm=None, out=None):
    """Kaldi log-mel filterbank of a batch of waveforms on the device (avs_wave_sums + avs_kaldi_fbank; the specification is
    preprocess.kaldi_fbank_reference): what torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=16000, use_energy=False,
    window_type='hanning', num_mel_bins=128, dither=0.0, frame_shift=10) and the loader around it compute (dataloader_ft.py:277-340).

    wave fp32 [B, stride] (16 kHz); lengths: samples per clip, None = stride.  partner / partner_lengths / lam: waveform mixup (:298-322) -
    clip b with lam[b] >= 0 becomes lam (w1 - mean) + (1 - lam) (w2 - mean, zero-padded or cut to the clip's length), minus its mean;
    lam[b] < 0, lam None or partner None: the plain path, w - mean.  The per-clip vectors may be host values (sequences, numpy, CPU
    tensors: checked here - a clip under 400 samples or beyond the stride is a ValueError - and uploaded) or device tensors (int32 / fp32,
    taken at their word: a clip under 400 samples then gives pad rows only).  norm=(mean, std): every row becomes
    (value - mean) * fp32(1 / std), pad rows included.  n_mels must be 128 (512-point FFT at 16 kHz).
    -> [B, target_length, 128] fp32: rows 0 .. m - 1 the clip's frames (m = 1 + (n - 400) // 160, cut at target_length), the rest 0 (or the
    normalised 0).  Two launches, no host synchronisation, no atomics: two calls give identical bytes."""
    _chk(wave, F32, "kaldi_fbank.wave", 2)
    B, stride = wave.shape
    dev = wave.device
    if int(n_mels) != FBANK_NMEL:
        raise _lib.AvsiamHipError(f"kaldi_fbank: n_mels = {n_mels}: the kernel is built for 128 mel bins over a 512-point FFT at 16 kHz")
    if B < 1 or stride < FBANK_FRAME:
        raise ValueError(f"kaldi_fbank: wave {tuple(wave.shape)}: need at least one clip of at least {FBANK_FRAME} samples")
    target_length = int(target_length)
    if target_length < 1:
        raise _lib.AvsiamHipError(f"kaldi_fbank: target_length = {target_length}")
    _chk(partner, F32, "kaldi_fbank.partner", 2)
    if partner is None and (partner_lengths is not None or lam is not None):
        raise _lib.AvsiamHipError("kaldi_fbank: partner_lengths / lam without a partner")
    if partner is not None and (partner.shape[0] != B or partner.device != dev or partner.shape[1] < 1):
        raise _lib.AvsiamHipError(f"kaldi_fbank: partner {tuple(partner.shape)} on {partner.device} does not match wave {tuple(wave.shape)} on {dev}")
    lengths = _per_clip(lengths, B, I32, "kaldi_fbank.lengths", dev, FBANK_FRAME, stride)
    partner_lengths = _per_clip(partner_lengths, B, I32, "kaldi_fbank.partner_lengths", dev, 1, partner.shape[1] if partner is not None else 0)
    lam = _per_clip(lam, B, F32, "kaldi_fbank.lam", dev)
    if out is None:
        out = torch.empty((B, target_length, FBANK_NMEL), dtype=F32, device=dev)
    else:
        _chk(out, F32, "kaldi_fbank.out", 3)
        if tuple(out.shape) != (B, target_length, FBANK_NMEL) or out.device != dev:
            raise _lib.AvsiamHipError(f"kaldi_fbank.out: expected {(B, target_length, FBANK_NMEL)} on {dev}, got {tuple(out.shape)} on {out.device}")
    mean, std = (float(norm[0]), float(norm[1])) if norm is not None else (0.0, 1.0)
    if std == 0.0:
        raise _lib.AvsiamHipError("kaldi_fbank: zero std")
    sums = wave_sums(wave, lengths, partner, partner_lengths)
    m = min(target_length, 1 + (stride - FBANK_FRAME) // FBANK_SHIFT)
    _launch("kaldi_fbank", (0.0, 4.0 * B * (m * FBANK_SHIFT * (2 if partner is not None else 1) + target_length * FBANK_NMEL)), "avs_kaldi_fbank", wave, stride,
            lengths, partner, partner.shape[1] if partner is not None else 0, partner_lengths, lam, sums, B, target_length, FBANK_NMEL, out,
            1 if norm is not None else 0, mean, std, _stream())
    return out


def mix_frames(v_u8, partner_u8, weight, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None):
    """The frame side of mixup (dataloader_ft.py:441-458): v_u8, partner_u8 uint8 [B, ..., 3, H, W] -> fp32 weight_b n(v) + (1 - weight_b) n(partner),
    n(x) = (x / 255 - mean_c) / std_c as preprocess.normalize_frames.  weight: [B] fp32 (device tensor, or host values that are uploaded);
    weight_b = 1 gives normalize_frames(v_u8)'s bytes.  One launch, no host synchronisation."""
    _chk(v_u8, U8, "mix_frames.v"); _chk(partner_u8, U8, "mix_frames.partner")
    if v_u8.dim() < 4 or v_u8.shape[-3] != 3 or v_u8.shape != partner_u8.shape or v_u8.device != partner_u8.device:
        raise _lib.AvsiamHipError(f"mix_frames: need two uint8 [B, ..., 3, H, W] tensors of one shape on one device, got {tuple(v_u8.shape)} and {tuple(partner_u8.shape)}")
    B = v_u8.shape[0]
    plane = v_u8.shape[-1] * v_u8.shape[-2]
    if B < 1 or plane < 1 or plane % 4:
        raise _lib.AvsiamHipError(f"mix_frames: H * W = {plane} must be a positive multiple of 4, B = {B} positive")
    n = v_u8.numel() // (3 * plane)
    weight = _per_clip(weight, B, F32, "mix_frames.weight", v_u8.device)
    if weight is None:
        raise _lib.AvsiamHipError("mix_frames: weight is None")
    if out is None:
        out = torch.empty(v_u8.shape, dtype=F32, device=v_u8.device)
    else:
        _chk(out, F32, "mix_frames.out")
        if out.shape != v_u8.shape or out.device != v_u8.device:
            raise _lib.AvsiamHipError(f"mix_frames.out: expected {tuple(v_u8.shape)} on {v_u8.device}")
    m3 = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s3 = (ctypes.c_float * 3)(*[float(x) for x in std])
    _call("avs_mix_frames_u8", v_u8, partner_u8, weight, out, n, n // B, plane, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), _stream())
    return out


RESIZE_MAX_SCALE = 10                                     # csrc/frontend_math.h


def resize_plan(max_h, max_w, out_h, out_w):
    """(output rows per workgroup, LDS bytes) of the resize launch for a batch whose largest clip is max_h x max_w (avs_resize_plan; host only)"""
    rows, lds = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("avs_resize_plan", int(max_h), int(max_w), int(out_h), int(out_w), ctypes.cast(ctypes.byref(rows), ctypes.c_void_p),
              ctypes.cast(ctypes.byref(lds), ctypes.c_void_p))
    return rows.value, lds.value


def _clip_sizes(x, B, Hs, Ws, out_h, out_w, name, dev):
    """per-clip (h, w) of a padded frame buffer: host values only - the launch is planned from the largest.  -> (device int32 [B, 2] or None,
    max h, max w)"""
    if x is None:
        hw = torch.tensor([[Hs, Ws]], dtype=torch.int64)
    else:
        if torch.is_tensor(x) and x.is_cuda:
            raise _lib.AvsiamHipError(f"{name}: the clip sizes are host values (sequence, numpy array or CPU tensor): the launch is planned from the largest")
        hw = torch.as_tensor(x).reshape(-1)
        if hw.numel() != 2 * B:
            raise _lib.AvsiamHipError(f"{name}: expected {B} (h, w) pairs, got {hw.numel()} values")
        hw = hw.to(torch.int64).reshape(B, 2)
    mh, mw = int(hw[:, 0].max()), int(hw[:, 1].max())
    if int(hw.min()) < 1 or mh > Hs or mw > Ws:
        raise ValueError(f"{name}: sizes must lie in 1 .. {Hs} x {Ws}, got {hw.tolist()}")
    if mh > RESIZE_MAX_SCALE * out_h or mw > RESIZE_MAX_SCALE * out_w:
        raise ValueError(f"{name}: {mh} x {mw} -> {out_h} x {out_w}: the scale per axis is limited to {RESIZE_MAX_SCALE}")
    return (None if x is None else hw.to(I32).to(dev)), mh, mw


def resize_frames(v_u8, sizes=None, *, partner=None, partner_sizes=None, weight=None, size=224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                  out=None):
    """Decoded-size uint8 frames to the model's fp32 frames in one launch (avs_resize_frames_u8; the specification is
    preprocess.resize_frames_reference): / 255, torchvision Resize(size, BICUBIC, antialias=True) - torch's interpolate(mode='bicubic',
    align_corners=False, antialias=True), no clamping -, Normalize(mean, std) and, with a partner, the frame mix (dataloader_ft.py:136-139, 434-459).

    v_u8 uint8 [B, 3, Hs, Ws] or [B, F, 3, Hs, Ws], a padded buffer: clip b fills the top-left sizes[b] = (h, w) corner.  sizes / partner_sizes:
    HOST values ([B, 2] sequence, numpy array or CPU tensor; None: the buffer's size), range-checked (ValueError) and uploaded - a device tensor
    is refused, the launch is planned from the largest clip.  1 <= h <= Hs, 1 <= w <= Ws, at most 10 x the output per axis.  partner: its own
    buffer [B, (F,) 3, Hs2, Ws2] and sizes; weight [B] fp32 as in mix_frames (device tensor, or host values that are uploaded): out = weight_b n(r)
    + (1 - weight_b) n(r_partner).  size: int or (out_h, out_w), out_w % 4 == 0.
    -> fp32 [B, (F,) 3, out_h, out_w].  A clip at the output size gives normalize_frames' bytes, weight 1 the plain call's; no atomics: two calls
    give identical bytes."""
    _chk(v_u8, U8, "resize_frames.v"); _chk(partner, U8, "resize_frames.partner")
    if v_u8.dim() not in (4, 5) or v_u8.shape[-3] != 3 or v_u8.shape[0] < 1 or v_u8.numel() == 0:
        raise _lib.AvsiamHipError(f"resize_frames: need uint8 [B, 3, H, W] or [B, F, 3, H, W], got {tuple(v_u8.shape)}")
    dev, B = v_u8.device, v_u8.shape[0]
    Hs, Ws = v_u8.shape[-2:]
    out_h, out_w = (int(size[0]), int(size[1])) if hasattr(size, "__len__") else (int(size), int(size))
    if out_h < 1 or out_w < 4 or out_w % 4:
        raise _lib.AvsiamHipError(f"resize_frames: output {out_h} x {out_w}: out_w must be a positive multiple of 4")
    if partner is None and (partner_sizes is not None or weight is not None):
        raise _lib.AvsiamHipError("resize_frames: partner_sizes / weight without a partner")
    if partner is not None and (partner.dim() != v_u8.dim() or partner.shape[:-2] != v_u8.shape[:-2] or partner.device != dev or partner.numel() == 0):
        raise _lib.AvsiamHipError(f"resize_frames: partner {tuple(partner.shape)} on {partner.device} does not match frames {tuple(v_u8.shape)} on {dev}")
    n = v_u8.numel() // (3 * Hs * Ws)
    sizes, mh, mw = _clip_sizes(sizes, B, Hs, Ws, out_h, out_w, "resize_frames.sizes", dev)
    Hs2 = Ws2 = mh2 = mw2 = 0
    if partner is not None:
        Hs2, Ws2 = partner.shape[-2:]
        partner_sizes, mh2, mw2 = _clip_sizes(partner_sizes, B, Hs2, Ws2, out_h, out_w, "resize_frames.partner_sizes", dev)
        weight = _per_clip(weight, B, F32, "resize_frames.weight", dev)
        if weight is None:
            raise _lib.AvsiamHipError("resize_frames: a partner needs a weight per clip")
    shape = tuple(v_u8.shape[:-2]) + (out_h, out_w)
    if out is None:
        out = torch.empty(shape, dtype=F32, device=dev)
    else:
        _chk(out, F32, "resize_frames.out")
        if tuple(out.shape) != shape or out.device != dev:
            raise _lib.AvsiamHipError(f"resize_frames.out: expected {shape} on {dev}, got {tuple(out.shape)} on {out.device}")
    m3 = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s3 = (ctypes.c_float * 3)(*[float(x) for x in std])
    nbytes = float(v_u8.numel() + (partner.numel() if partner is not None else 0) + 4 * out.numel())
    _launch("resize_frames", (0.0, nbytes), "avs_resize_frames_u8", v_u8, Hs, Ws, sizes, mh, mw, partner, Hs2, Ws2, partner_sizes, mh2, mw2, weight, out, n,
            n // B, out_h, out_w, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), _stream())
    return out


# ---- source-rate audio (fine-tuning loader: dataloader_ft.py:272-277, 298-306) -----------------------------------------------------------
RESAMPLE_MAX_RATES, RESAMPLE_MAX_CHANNELS, RESAMPLE_MAX_WORDS, RESAMPLE_MAX_SPAN, RESAMPLE_TILE = 8, 8, 16384, 16384, 1024      # csrc/resample.hip
_resample_tables = {}         # (orig, new, device) -> (device table, (o, n, width, taps))
_resample_index = {}          # (per-clip table indices, device) -> int32 device tensor


def resample_table(orig_freq, new_freq, device):
    """The compact filter bank of one rate pair on `device`, built once from preprocess.resample_table_reference (torch on the CPU: the
    kernel's weights are that table's bits) and kept: -> (fp32 device tensor of n + n * pitch words: int32 first[n], then w[n][pitch], pitch =
    taps | 1; (o, n, width, taps)).  A rate pair whose compact table or whose tile span is over the kernel's caps is refused before the
    dense table is built."""
    import math
    import numpy as np
    from . import preprocess
    device = torch.device(device)
    key = (int(orig_freq), int(new_freq), device)
    hit = _resample_tables.get(key)
    if hit is not None:
        return hit
    o, n = preprocess._resample_ratio(orig_freq, new_freq)
    width = math.ceil(6 * o / (min(o, n) * 0.99))
    if n * 14 > RESAMPLE_MAX_WORDS:                                     # a phase has at least 12 taps: 2 * 6 zero crossings
        raise _lib.AvsiamHipError(f"resample_wave: {orig_freq} -> {new_freq} Hz has {n} phases: compact tables above {RESAMPLE_MAX_WORDS} words are refused")
    if ((RESAMPLE_TILE - 1) // n + 2) * o + 2 * width + 3 > RESAMPLE_MAX_SPAN:
        raise _lib.AvsiamHipError(f"resample_wave: {orig_freq} -> {new_freq} Hz: the input span of {RESAMPLE_TILE} outputs is over {RESAMPLE_MAX_SPAN} samples")
    table, width = preprocess.resample_table_reference(orig_freq, new_freq)
    first, weights = preprocess.resample_compact_table(table)
    taps = weights.shape[1]
    pitch = taps | 1
    if n * (pitch + 1) > RESAMPLE_MAX_WORDS:
        raise _lib.AvsiamHipError(f"resample_wave: {orig_freq} -> {new_freq} Hz: {n} phases x {taps} taps: compact tables above {RESAMPLE_MAX_WORDS} words are refused")
    block = np.zeros(n + n * pitch, dtype=np.float32)
    block[:n] = first.view(np.float32)
    block[n:].reshape(n, pitch)[:, :taps] = weights
    hit = (torch.from_numpy(block).to(device), (o, n, int(width), taps))
    _resample_tables[key] = hit
    return hit


def resample_wave(wave, rates, lengths=None, *, new_freq=16000, out=None, out_lengths=None):
    """Decoded PCM at the files' own rates to mono audio at `new_freq` in one launch (avs_resample_wave, csrc/resample.hip; the specification is
    preprocess.resample_reference): torchaudio.functional.resample(waveform, sr, new_freq) - windowed sinc, sinc_interp_hann, width 6, rolloff
    0.99 - when sr != new_freq, and waveform.mean(dim=0) (dataloader_ft.py:272-277, 298-306).

    wave fp32 [B, stride] or [B, C, stride], 1 <= C <= 8.  rates: a HOST int or B host ints, each clip's own rate (the loader knows it from the
    file header); at most 8 distinct rates other than new_freq per call.  lengths: samples per clip, None = stride; host values are checked
    (0 .. stride, ValueError) and uploaded, an int32 device tensor is taken at its word and cut to 0 .. stride on the device.
    -> (out fp32 [B, out_stride], out_lengths int32 [B] on the device): out_lengths[b] = ceil(n len / o) in exact integers, the row is zero from
    there; out_stride is the largest ceil(n stride / o) over the call's rates; `out` / `out_lengths` given: written in place.  A clip at new_freq is not filtered: its channel mean (C = 1:
    its bytes).  One launch (plus a table upload on a rate's first use), no host synchronisation, no atomics: two calls give identical bytes."""
    from . import preprocess
    _chk(wave, F32, "resample_wave.wave")
    if wave.dim() not in (2, 3):
        raise _lib.AvsiamHipError(f"resample_wave: need fp32 [B, stride] or [B, C, stride], got {tuple(wave.shape)}")
    B, stride = wave.shape[0], wave.shape[-1]
    C = wave.shape[1] if wave.dim() == 3 else 1
    dev = wave.device
    if B < 1 or stride < 1 or C < 1:
        raise _lib.AvsiamHipError(f"resample_wave: wave {tuple(wave.shape)}: need at least one clip, one channel and one sample")
    if C > RESAMPLE_MAX_CHANNELS:
        raise _lib.AvsiamHipError(f"resample_wave: {C} channels: at most {RESAMPLE_MAX_CHANNELS}")
    if isinstance(rates, (str, bytes)):
        raise ValueError(f"resample_wave: rates {rates!r}: a host int or {B} host ints")
    rates = [rates] * B if not hasattr(rates, "__len__") else list(rates)
    if len(rates) != B:
        raise _lib.AvsiamHipError(f"resample_wave: {len(rates)} rates for {B} clips")
    ratios = [preprocess._resample_ratio(r, new_freq) for r in rates]                      # ValueError: not positive integers
    new_freq = int(new_freq)
    distinct = sorted({int(r) for r in rates if int(r) != new_freq})
    if len(distinct) > RESAMPLE_MAX_RATES:
        raise _lib.AvsiamHipError(f"resample_wave: {len(distinct)} distinct rates in one call: at most {RESAMPLE_MAX_RATES}")
    tabs = [resample_table(r, new_freq, dev) for r in distinct]
    idx = tuple(distinct.index(int(r)) if int(r) != new_freq else -1 for r in rates)
    tab_idx = _resample_index.get((idx, dev))
    if tab_idx is None:
        if len(_resample_index) >= 256:
            _resample_index.clear()
        tab_idx = _resample_index[(idx, dev)] = torch.tensor(idx, dtype=I32).to(dev)
    out_stride = max(-((-n * stride) // o) for o, n in ratios)
    lengths = _per_clip(lengths, B, I32, "resample_wave.lengths", dev, 0, stride)
    if out is None:
        out = torch.empty((B, out_stride), dtype=F32, device=dev)
    else:
        _chk(out, F32, "resample_wave.out", 2)
        if tuple(out.shape) != (B, out_stride) or out.device != dev:
            raise _lib.AvsiamHipError(f"resample_wave.out: expected {(B, out_stride)} on {dev}, got {tuple(out.shape)} on {out.device}")
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=I32, device=dev)
    else:
        _chk(out_lengths, I32, "resample_wave.out_lengths", 1)
        if out_lengths.numel() != B or out_lengths.device != dev:
            raise _lib.AvsiamHipError(f"resample_wave.out_lengths: expected {B} values on {dev}, got {tuple(out_lengths.shape)} on {out_lengths.device}")
    ptrs = (ctypes.c_void_p * max(1, len(tabs)))(*[t.data_ptr() for t, _ in tabs])
    geo = (ctypes.c_int * max(4, 4 * len(tabs)))(*[v for _, g in tabs for v in g])
    _launch("resample_wave", (0.0, 4.0 * (wave.numel() + out.numel())), "avs_resample_wave", wave, B, C, stride, lengths, tab_idx, len(tabs),
            ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(geo, ctypes.c_void_p), out, out_stride, out_lengths, _stream())
    return out, out_lengths


# ---- PCM decode (fine-tuning loader: dataloader_ft.py:272, torchaudio.load) ---------------------------------------------------------------------
DECODE_MAX_CHANNELS, DECODE_TILE = 8, 1024                                      # csrc/decode.hip


def decode_pcm(payload, desc, channels, stride, *, out=None, out_lengths=None):
    """The payloads of WAV data chunks to planar fp32 channels in one launch (avs_decode_pcm, csrc/decode.hip; the specification is
    preprocess.decode_pcm_reference, bit for bit): what torchaudio.load(normalize=True) returns for the file (dataloader_ft.py:272).

    payload uint8 [B, byte_stride] on the device, byte_stride % 16 == 0: row b holds clip b's interleaved little-endian sample frames from
    byte 0 (preprocess.parse_wav gives a file's data_offset and data_bytes).  desc [B, 2] = (format, n_frames) per clip, format one of
    preprocess.PCM_U8 .. PCM_F64: host values (sequence, numpy, CPU tensor) are checked - a format outside 0 .. 5, or more frames than the row
    or `stride` hold, is a ValueError - and uploaded; an int32 device tensor is taken at its word, and its n_frames is cut on the device to what
    the two rows hold (an unknown format decodes to no frames).  channels: the channel count of EVERY clip of the call, 1 .. 8 (the loader
    groups a batch by it); stride: the samples per channel row of the output.
    -> (out fp32 [B, channels, stride], out_lengths int32 [B] on the device): zero from out_lengths[b] to stride; `out` / `out_lengths` given:
    written in place.  One launch, no atomics: two calls give identical bytes.  With a device descriptor (what the loader passes) the call
    does not synchronise with the host; host values are checked pair by pair in Python and uploaded with a blocking copy."""
    from . import preprocess
    _chk(payload, U8, "decode_pcm.payload", 2)
    B, byte_stride = payload.shape
    C, stride = int(channels), int(stride)
    dev = payload.device
    if B < 1 or byte_stride < 16 or byte_stride % 16 or payload.data_ptr() % 16:
        raise _lib.AvsiamHipError(f"decode_pcm: payload {tuple(payload.shape)}: need at least one 16-byte aligned row whose length is a positive multiple of 16")
    if not 1 <= C <= DECODE_MAX_CHANNELS:
        raise _lib.AvsiamHipError(f"decode_pcm: {C} channels: 1 .. {DECODE_MAX_CHANNELS}")
    if stride < 1:
        raise _lib.AvsiamHipError(f"decode_pcm: stride = {stride}")
    if torch.is_tensor(desc) and desc.is_cuda:
        _chk(desc, I32, "decode_pcm.desc", 2)
        if tuple(desc.shape) != (B, 2) or desc.device != dev:
            raise _lib.AvsiamHipError(f"decode_pcm.desc: expected [{B}, 2] on {dev}, got {tuple(desc.shape)} on {desc.device}")
    else:
        h = torch.as_tensor(desc).reshape(-1).to(torch.int64)
        if h.numel() != 2 * B:
            raise _lib.AvsiamHipError(f"decode_pcm.desc: expected {B} (format, n_frames) pairs, got {h.numel()} values")
        h = h.reshape(B, 2)
        for b, (f, n) in enumerate(h.tolist()):
            if not 0 <= f < len(preprocess.PCM_BYTES):
                raise ValueError(f"decode_pcm.desc: clip {b}: format {f} (0 .. {len(preprocess.PCM_BYTES) - 1})")
            if not 0 <= n <= min(stride, byte_stride // (C * preprocess.PCM_BYTES[f])):
                raise ValueError(f"decode_pcm.desc: clip {b}: {n} {preprocess.PCM_NAMES[f]} frames of {C} channels do not fit {byte_stride} bytes / {stride} samples")
        desc = h.to(I32).to(dev)
    if out is None:
        out = torch.empty((B, C, stride), dtype=F32, device=dev)
    else:
        _chk(out, F32, "decode_pcm.out", 3)
        if tuple(out.shape) != (B, C, stride) or out.device != dev:
            raise _lib.AvsiamHipError(f"decode_pcm.out: expected {(B, C, stride)} on {dev}, got {tuple(out.shape)} on {out.device}")
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=I32, device=dev)
    else:
        _chk(out_lengths, I32, "decode_pcm.out_lengths", 1)
        if out_lengths.numel() != B or out_lengths.device != dev:
            raise _lib.AvsiamHipError(f"decode_pcm.out_lengths: expected {B} values on {dev}, got {tuple(out_lengths.shape)} on {out_lengths.device}")
    _launch("decode_pcm", (0.0, float(payload.numel() + 4 * out.numel())), "avs_decode_pcm", payload, byte_stride, desc, B, C, out, stride, out_lengths, _stream())
    return out, out_lengths
