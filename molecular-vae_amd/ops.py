"""Tensor-level wrappers over the C ABI (include/mvae.h).  torch is plumbing only: device memory + streams.

Every function launches HIP kernels on torch's current stream and raises on any non-zero status.
"""
import ctypes as C
import weakref

import torch

from . import _lib as L
from ._lib import ptr, check, stream_ptr, dt_code


def _pad(n, m):
    return (n + m - 1) // m * m


# Optional device-side timing of tagged launch groups (bench.py's roofline leg): {tag: [(start, end) events]}.
# Events are recorded on torch's current stream, which is the stream every kernel here is launched on.
PROFILE = None


# roctx ranges (tracing): with MVAE_ROCTX=1 in the environment (or ops.enable_roctx()) every tagged launch group and every phase
# of the step (encoder / decoder forward and backward, the optimiser, the MOSES halves) is bracketed by roctxRangePush / Pop, so that a
# `rocprofv3 --kernel-trace --marker-trace` timeline groups the kernels by kernel family.  Off by default: two ctypes calls per range.
_ROCTX = {"lib": None, "on": None}


def enable_roctx(on=True):
    if on and _ROCTX["lib"] is None:
        for name in ("libroctx64.so", "librocprofiler-sdk-roctx.so", "/opt/rocm/lib/libroctx64.so"):
            try:
                lib = C.CDLL(name)
                lib.roctxRangePushA.argtypes = [C.c_char_p]
                _ROCTX["lib"] = lib
                break
            except OSError:
                continue
    _ROCTX["on"] = bool(on) and _ROCTX["lib"] is not None
    return _ROCTX["on"]


def _roctx_on():
    if _ROCTX["on"] is None:
        import os
        enable_roctx(os.environ.get("MVAE_ROCTX", "0") not in ("", "0"))
    return _ROCTX["on"]


class trace_range:
    """with ops.trace_range("dec_lstm_fwd"): ...   -- a named roctx range around the launches enqueued inside (no-op unless enabled)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.live = bool(self.name) and _roctx_on()
        if self.live:
            _ROCTX["lib"].roctxRangePushA(self.name.encode())
        return self

    def __exit__(self, *a):
        if self.live:
            _ROCTX["lib"].roctxRangePop()
        return False


def traced(name):
    """Decorator form of trace_range (the autograd Functions' forward / backward)."""
    def deco(fn):
        def wrapper(*a, **k):
            with trace_range(name):
                return fn(*a, **k)
        wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
        return wrapper
    return deco


class _Timed:
    def __init__(self, tag):
        self.tag = tag
        self.range = trace_range(tag)

    def __enter__(self):
        self.range.__enter__()
        if PROFILE is not None and self.tag:
            self.s = torch.cuda.Event(enable_timing=True); self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if PROFILE is not None and self.tag:
            self.e.record()
            PROFILE.setdefault(self.tag, []).append((self.s, self.e))
        self.range.__exit__()
        return False


# One side stream per device for the whole process, picked so that it does NOT share a hardware queue with the main stream: HIP maps streams
# onto a few hardware queues (4 by default, the null stream holds one), further streams double up round-robin, and two streams on one queue
# execute strictly one after the other -- a fork onto such a stream is no fork at all (measured: the 4th stream a process creates turned the
# b = 128 step from 8.2 into 14.4 ms).  Nothing in the API tells which queue a stream got, so the pick is a 1 ms probe at first use -- the
# models probe at their first FORWARD (MolecularVAE's prepack fork, mosesvae.VAE.forward), not inside a backward pass.
_SIDE_STREAMS = {}
SIDE_STREAM_INFO = {}     # device index -> dict(tries, concurrent, ratio): which candidate was taken and whether it passed the probe (logs / bench line)


def side_stream(device):
    device = torch.device(device)
    s = _SIDE_STREAMS.get(device.index)
    if s is None:
        s = _SIDE_STREAMS[device.index] = _pick_concurrent_stream(device)
    return s


def _pick_concurrent_stream(device, tries=6):
    """Probe: ~0.4 ms of fills on the main stream, a tiny fill on the candidate issued behind them; the candidate runs concurrently iff its fill
    finishes long before the main stream's.  16 MB of scratch, freed on return.  When no candidate passes (a co-tenant or a profiler can skew
    the wall-clock test) the first one is used and SIDE_STREAM_INFO says so -- the results are the same, only the overlap is lost."""
    main = torch.cuda.current_stream(device)
    big = torch.empty(1 << 22, dtype=torch.float32, device=device)       # 16 MB: a fill takes ~5 us
    small = torch.empty(256, dtype=torch.float32, device=device)
    first, info = None, dict(tries=0, concurrent=False, ratio=None)
    pick = None
    for _ in range(tries):
        cand = torch.cuda.Stream(device=device)
        first = first or cand
        info["tries"] += 1
        torch.cuda.synchronize(device)
        e0, e_main, e_c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(main)
        for _ in range(96):
            big.fill_(1.0)                                                # ~0.4 ms of work on the main stream
        e_main.record(main)
        with torch.cuda.stream(cand):
            small.fill_(0.0)                                              # independent of it: finishes at once -- unless it queues behind
            e_c.record(cand)
        torch.cuda.synchronize(device)
        info["ratio"] = e0.elapsed_time(e_c) / max(e0.elapsed_time(e_main), 1e-6)
        if info["ratio"] < 0.5:
            pick, info["concurrent"] = cand, True
            break
    del big, small
    SIDE_STREAM_INFO[device.index] = info
    return pick or first


class ForkState:
    """Side-stream bookkeeping of ONE model (a MolDecoder and the MolEncoder whose backward follows it share one): `pending` = events of work
    forked onto a side stream that nobody has joined yet (joined by the encoder's backward / FusedAdam.step); `deferred` = (side stream,
    callable, stage): throughput-bound work its owner parked so that the peer can release it at a chosen point of ITS launch sequence.
    The decoder parks its weight-gradient GEMMs in two stages: stage 0 is released by the encoder's backward once its head section (a dozen
    tiny launches that would otherwise each wait for a chip-filling GEMM workgroup to retire) is enqueued, stage 1 right before its
    row-resident LSTM backward, whose 128 workgroups leave half the CUs idle.  Whoever reaches run_deferred() / join() first runs it.
    Per model, not per process: two models stepping in one process never see each other's parked work."""
    _all = weakref.WeakSet()

    def __init__(self):
        self.pending, self.deferred = [], []
        ForkState._all.add(self)

    def park(self, side, fn, stage):
        self.deferred.append((side, fn, stage))

    def run_deferred(self, stage=None):
        """Launch the parked work of stages <= `stage` (None: all) on its side stream, ordered after everything issued so far on the current stream."""
        keep = []
        while self.deferred:
            side, fn, st = self.deferred.pop(0)
            if stage is not None and st > stage:
                keep.append((side, fn, st))
                continue
            ev = torch.cuda.Event(); ev.record()
            side.wait_event(ev)
            with torch.cuda.stream(side):
                fn()
                e2 = torch.cuda.Event(); e2.record()
            self.pending.append(e2)
        self.deferred.extend(keep)

    def join(self):
        """Make the current stream wait for every forked piece of work of this model (weight-gradient GEMMs on the side stream)."""
        self.run_deferred()
        while self.pending:
            torch.cuda.current_stream().wait_event(self.pending.pop())


def join_pending():
    """Join the forked work of EVERY live model (FusedAdam.step: an optimiser may hold the parameters of several)."""
    for fs in list(ForkState._all):
        fs.join()


def release_caches():
    """Drop the op-internal scratch buffers and any forgotten fork bookkeeping (between benchmark configurations / models)."""
    join_pending()
    Scratch._bufs.clear()


class Scratch:
    """Grow-only byte scratch for split-K slabs and op-internal temporaries (one per device AND stream: two streams must
    never share split-K slabs)."""
    _bufs = {}

    @classmethod
    def get(cls, nbytes, device, tag="", zeroed=False):
        """zeroed: the buffer is allocated zero and only ever handed to call sites of this `tag` (kernels that keep a self-resetting
        counter in it, e.g. the loss's ticket)."""
        key = (device.type, device.index, torch.cuda.current_stream().cuda_stream if device.type == "cuda" else 0, tag)
        b = cls._bufs.get(key)
        if b is None or b.numel() < nbytes:
            if zeroed:
                b = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
            else:
                b = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            cls._bufs[key] = b
        return b


def gemm_nt(A, B, out, M, N, K, lda=None, ldb=None, ldc=None, bias=None, act=L.ACT_NONE, accumulate=False, x3=False):
    """out[M,N] = act(A[M,K] . B[N,K]^T + bias).  A, B same dtype (f32 / bf16); out f32 or bf16.
    x3 (fp32 operands): products on the bf16 MFMA as hi.hi + hi.lo + lo.hi (MVAE_F32X3, ~16 mantissa bits)."""
    lib = L.load()
    dt = dt_code(A.dtype)
    assert B.dtype == A.dtype
    if x3:
        assert A.dtype == torch.float32
        dt = L.MVAE_F32X3
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    need = lib.mvae_gemm_nt_workspace(M, N, K, dt)
    ws = Scratch.get(need, A.device) if need else None
    check(lib.mvae_gemm_nt(dt, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, dt_code(out.dtype), ptr(bias), act,
                           1 if accumulate else 0, ptr(ws), need, stream_ptr()), "mvae_gemm_nt")
    return out


def gemm_tn(A, B, out, M, N, K, lda=None, ldb=None, ldc=None, bias=None, act=L.ACT_NONE, accumulate=False):
    """out[M,N] = act(A[:K,:M]^T . B[:K,:N] + bias): A [K, lda], B [K, ldb] bf16, K-major (weight gradients)."""
    lib = L.load()
    dt = dt_code(A.dtype)
    assert B.dtype == A.dtype
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    need = lib.mvae_gemm_tn_workspace(M, N, K, dt)
    ws = Scratch.get(need, A.device) if need else None
    check(lib.mvae_gemm_tn(dt, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, dt_code(out.dtype), ptr(bias), act,
                           1 if accumulate else 0, ptr(ws), need, stream_ptr()), "mvae_gemm_tn")
    return out


def gemm_tn_f32_colsum(A, B, out, colsum_out, M, N, K, lda=None, ldb=None, ldc=None, accumulate=False, colsum_accumulate=False):
    """fp32: out[M,N] (+)= A[:K,:M]^T . B[:K,:N]  and  colsum_out[m] (+)= sum_k A[k,m]  in ONE launch (the bias gradient as a virtual ones column)."""
    lib = L.load()
    assert A.dtype == B.dtype == torch.float32
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    need = lib.mvae_gemm_tn_workspace(M, N, K, L.MVAE_F32)
    ws = Scratch.get(need, A.device) if need else None
    check(lib.mvae_gemm_tn_f32_colsum(M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, 1 if accumulate else 0, ptr(colsum_out),
                                      1 if colsum_accumulate else 0, ptr(ws), need, stream_ptr()), "mvae_gemm_tn_f32_colsum")
    return out


def gemm_tn_colsum_supported(A, M, N, K):
    return A.dtype == torch.bfloat16 and bool(L.load().mvae_gemm_tn_colsum_supported(M, N, K))


def gemm_tn_colsum(A, B, out, colsum_out, M, N, K, lda=None, ldb=None, colsum_accumulate=False):
    """bf16: out[M,N] = A[:K,:M]^T . B[:K,:N]  and  colsum_out[m] (+)= sum_k A[k,m] from the same pass over A.  Returns False (nothing
    launched) when the shape is not served by the fused kernel -- the caller then runs gemm_tn + colsum_t."""
    lib = L.load()
    if A.dtype != torch.bfloat16 or not lib.mvae_gemm_tn_colsum_supported(M, N, K):
        return False
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    need = lib.mvae_gemm_tn_colsum_workspace(M, N, K)
    ws = Scratch.get(need, A.device) if need else None
    check(lib.mvae_gemm_tn_colsum(M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), out.stride(0), 0, ptr(colsum_out),
                                  1 if colsum_accumulate else 0, ptr(ws), need, stream_ptr()), "mvae_gemm_tn_colsum")
    return True


def gemm_tn_grouped_supported(A, M, N, K, lda, ldb):
    return A.dtype == torch.bfloat16 and bool(L.load().mvae_gemm_tn_grouped_supported(M, N, K, lda, ldb))


def gemm_tn_grouped(problems, max_workgroups=0):
    """problems: list of dict(A, B, out, M, N, K, lda, ldb[, colsum_out, colsum_accumulate, accumulate]) -- bf16 K-major operands; ONE launch
    for all of them, each 256 x 256 tile accumulated over its full K (no split-K slabs / reduction launch).  max_workgroups > 0: that many
    workgroups at most, looping over the tiles (leaves compute units to another stream)."""
    lib = L.load()
    n = len(problems)
    arr = (L.GemmTnProblem * n)()
    for i, q in enumerate(problems):
        a = arr[i]
        a.M, a.N, a.K = q["M"], q["N"], q["K"]
        a.A, a.lda, a.B, a.ldb = q["A"].data_ptr(), q["lda"], q["B"].data_ptr(), q["ldb"]
        a.C, a.ldc, a.accumulate = q["out"].data_ptr(), q["out"].stride(0), 1 if q.get("accumulate") else 0
        cs = q.get("colsum_out")
        a.colsum_out = cs.data_ptr() if cs is not None else None
        a.colsum_accumulate = 1 if q.get("colsum_accumulate") else 0
    need = lib.mvae_gemm_tn_grouped_workspace(n, arr)
    ws = Scratch.get(need, problems[0]["A"].device, tag="tn_grouped") if need else None
    check(lib.mvae_gemm_tn_grouped_capped(n, arr, int(max_workgroups), ptr(ws), need, stream_ptr()), "mvae_gemm_tn_grouped_capped")


class TnF32Batch:
    """Collects exact-f32 (or 3 x bf16) TN contractions that only feed the optimiser -- the parameter gradients of an encoder's backward pass --
    and runs them as ONE launch + ONE split-K reduction (mvae_gemm_tn_f32_multi) instead of a dozen half-empty ones.  Operands must stay alive
    and unchanged until run(); run() of more than MVAE_TN_F32_MULTI_MAX problems issues several launches."""
    MAX = 16

    def __init__(self, device):
        self.device, self.probs, self.keep, self.after = device, [], [], []

    def add(self, A, B, out, M, N, K, lda=None, ldb=None, ldc=None, colsum_out=None, colsum_accumulate=False, accumulate=False, x3=False,
            b_group=0, b_gstride=0):
        """out[M, N] (+)= A[:K, :M]^T . B[:K, :N]; colsum_out[m] (+)= sum_k A[k, m].  b_group > 0: row r of B starts at element
        (r // b_group) * b_gstride + (r % b_group) * ldb (a permuted view of a [T, B, W] buffer, see MolEncoder's table gradient)."""
        assert A.dtype == B.dtype == out.dtype == torch.float32
        q = L.GemmTnF32Problem()
        q.M, q.N, q.K = M, N, K
        q.A, q.lda, q.a_group, q.a_gstride = A.data_ptr(), (A.stride(0) if lda is None else lda), 0, 0
        q.B, q.ldb, q.b_group, q.b_gstride = B.data_ptr(), (B.stride(0) if ldb is None else ldb), b_group, b_gstride
        q.C, q.ldc, q.accumulate = out.data_ptr(), (out.stride(0) if ldc is None else ldc), 1 if accumulate else 0
        q.colsum_out = colsum_out.data_ptr() if colsum_out is not None else None
        q.colsum_accumulate, q.x3 = (1 if colsum_accumulate else 0), (1 if x3 else 0)
        self.probs.append(q)
        self.keep += [A, B, out, colsum_out]

    def add_conv_dw(self, B, W, Cin, ldx, x_bs, Cout, ldo, k, dzp, x, dwp, dw, db, x3=False):
        """The weight / bias gradient of a channels-last Conv1d whose mvae_conv1d_act_bwd call skipped it (dw = None): dwp is the packed
        scratch [Cout, k * ldx]; after run() it is unpacked into the parameter layout dw [Cout, Cin, k]."""
        q = L.GemmTnF32Problem()
        check(L.load().mvae_conv1d_dw_problem(B, W, Cin, ldx, x_bs, Cout, ldo, k, ptr(dzp), ptr(x), ptr(dwp), ptr(db), 1 if x3 else 0, C.byref(q)),
              "mvae_conv1d_dw_problem")
        self.probs.append(q)
        self.keep += [dzp, x, dwp, db, dw]
        self.after.append(lambda: check(L.load().mvae_conv1d_unpack_dw(Cin, Cout, k, ptr(dwp), ldx, ptr(dw), stream_ptr()), "mvae_conv1d_unpack_dw"))

    def run(self):
        lib = L.load()
        for i in range(0, len(self.probs), self.MAX):
            part = self.probs[i:i + self.MAX]
            arr = (L.GemmTnF32Problem * len(part))(*part)
            need = lib.mvae_gemm_tn_f32_multi_workspace(len(part), arr)
            ws = Scratch.get(need, self.device, tag="tn_f32_multi") if need else None
            check(lib.mvae_gemm_tn_f32_multi(len(part), arr, ptr(ws), need, stream_ptr()), "mvae_gemm_tn_f32_multi")
        for fn in self.after:
            fn()
        self.probs, self.keep, self.after = [], [], []


def colsum_t(X, M, N, out, ldx=None):
    lib = L.load()
    need = lib.mvae_colsum_t_workspace(M, N)
    ws = Scratch.get(need, X.device)
    check(lib.mvae_colsum_t(dt_code(X.dtype), M, N, ptr(X), X.stride(0) if ldx is None else ldx, ptr(out), ptr(ws), need,
                            stream_ptr()), "mvae_colsum_t")


def cast_transpose(src, R, C_, dst=None, dstT=None, lds=None):
    lib = L.load()
    lds = src.stride(0) if lds is None else lds
    d = dst if dst is not None else dstT
    check(lib.mvae_cast_transpose(dt_code(src.dtype), dt_code(d.dtype), R, C_, ptr(src), lds,
                                  ptr(dst), dst.stride(0) if dst is not None else 0,
                                  ptr(dstT), dstT.stride(0) if dstT is not None else 0, stream_ptr()), "mvae_cast_transpose")


class PackList:
    """A list of weight-packing jobs run as ONE launch (mvae_pack_multi).  Build it once per set of buffers (`key`), call run() after every
    optimiser step: the job table stays in device memory.  Methods mirror cast_transpose / torch.add / copy_; every tensor handed in must
    stay alive and in place (parameters inside FusedAdam's flat buffer and workspace buffers do)."""

    def __init__(self):
        self.jobs, self.keep, self.table, self.total = [], [], None, 0

    def _job(self, kind, src, R, C_, lds, dst=None, ldd=0, dstT=None, ldt=0, src2=None, dst_dtype=None):
        j = L.PackJob()
        j.kind, j.R, j.C = kind, R, C_
        j.src_dtype = dt_code(src.dtype)
        d = dst if dst is not None else dstT
        j.dst_dtype = dt_code(d.dtype if dst_dtype is None else dst_dtype)
        j.src, j.lds = src.data_ptr(), lds
        j.dst, j.ldd = (dst.data_ptr() if dst is not None else None), ldd
        j.dstT, j.ldt = (dstT.data_ptr() if dstT is not None else None), ldt
        j.src2 = src2.data_ptr() if src2 is not None else None
        self.jobs.append(j)
        self.keep += [t for t in (src, dst, dstT, src2) if t is not None]
        self.table = None

    def cast_transpose(self, src, R, C_, dst=None, dstT=None, lds=None):
        if R <= 0 or C_ <= 0:
            return
        if src.stride(-1) != 1 or (dst is not None and dst.stride(-1) != 1) or (dstT is not None and dstT.stride(-1) != 1):
            raise L.MvaeError("PackList: innermost dimension must be contiguous")
        self._job(0, src, R, C_, src.stride(0) if lds is None else lds, dst, dst.stride(0) if dst is not None else 0,
                  dstT, dstT.stride(0) if dstT is not None else 0)

    def add(self, a, b, out):
        assert a.dtype == b.dtype == out.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and out.is_contiguous()
        self._job(1, a, 1, a.numel(), a.numel(), dst=out, ldd=out.numel(), src2=b)

    def copy(self, src, dst):
        """dst[r, c] = src[r, c] for 2-D (or 1-D) fp32 views with contiguous rows."""
        assert src.dtype == dst.dtype == torch.float32 and src.shape == dst.shape
        if src.dim() == 1:
            src, dst = src.unsqueeze(0), dst.unsqueeze(0)
        assert src.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
        self._job(2, src, src.shape[0], src.shape[1], src.stride(0) if src.shape[0] > 1 else src.shape[1],
                  dst=dst, ldd=dst.stride(0) if dst.shape[0] > 1 else dst.shape[1])

    def run(self):
        if not self.jobs:
            return
        lib = L.load()
        if self.table is None:
            n = len(self.jobs)
            arr = (L.PackJob * n)()
            tot = 0
            for i, j in enumerate(self.jobs):
                j.block0 = tot
                tot += lib.mvae_pack_job_blocks(C.byref(j))
                arr[i] = j
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            dev = self.keep[0].device
            self.table, self.total = host.to(dev), tot
        check(lib.mvae_pack_multi(len(self.jobs), ptr(self.table), self.total, stream_ptr()), "mvae_pack_multi")


def permute021(inp, out, N, A, Bd):
    check(L.load().mvae_permute021(N, A, Bd, ptr(inp), ptr(out), stream_ptr()), "mvae_permute021")


def onehot_tb(idx, out, B, Lq, nrows):
    """out[(t*B + b), c] = (idx[b, t] == c) for c < ld (bf16, time-major rows): the K-major operand that turns the table scatter
    dtable = sum_rows onehot^T . d into one TN GEMM."""
    check(L.load().mvae_onehot_tb(ptr(idx), B, Lq, nrows, ptr(out), out.stride(0), stream_ptr()), "mvae_onehot_tb")


def onehot_f32(idx, out, nrows):
    """out[r, c] = (idx.flat[r] == c), fp32, rows in idx's own order."""
    check(L.load().mvae_onehot_f32(ptr(idx), idx.numel(), nrows, ptr(out), out.stride(0), stream_ptr()), "mvae_onehot_f32")


def gather_rows_tb(idx, table, out, B, Lq, nrows, W, base=None):
    check(L.load().mvae_gather_rows_tb(ptr(idx), B, Lq, nrows, ptr(table), W, ptr(base), ptr(out), stream_ptr()), "mvae_gather_rows_tb")


def expand_indices(store, rows, idx, ohe, B, Lq, C_):
    check(L.load().mvae_expand_indices(ptr(store), ptr(rows), B, Lq, C_, ptr(idx), ptr(ohe), stream_ptr()), "mvae_expand_indices")


def moses_collate(tokens, offsets, rows, x_pad, lengths, T, N, bos, eos, pad, rows_sorted=None, err=None):
    """The MOSES collate in one launch (include/mvae.h): corpus rows `rows` (int64 [B]) of the CSR corpus (tokens uint8, offsets int64
    [N + 1]) -> x_pad[:, :T] int64 (stable length-descending order, bos / eos / pad) and lengths int32 [B]; rows_sorted / err optional."""
    check(L.load().mvae_moses_collate(ptr(tokens), ptr(offsets), ptr(rows), rows.numel(), T, N, bos, eos, pad, ptr(x_pad), x_pad.stride(0),
                                      ptr(lengths), ptr(rows_sorted), ptr(err), stream_ptr()), "mvae_moses_collate")


def corpus_index_build(tokens, offsets, N, slots, n_distinct=None):
    """Fills the exact hash index `slots` (int64 [n_slots], n_slots a power of two > N; cleared by the launch itself) over the CSR corpus
    (tokens uint8, offsets int64 [N + 1]); n_distinct (int64 [1], optional) := the number of distinct rows (mvae_corpus_index_build)."""
    check(L.load().mvae_corpus_index_build(ptr(tokens), ptr(offsets), N, ptr(slots), slots.numel(), ptr(n_distinct), stream_ptr()),
          "mvae_corpus_index_build")


def corpus_index_probe(tokens, offsets, N, slots, x, eos, match):
    """match [B] int64 := the lowest corpus row whose tokens equal x[b, 1:] cut before its first `eos` (x int64 [B, T], bos first), -1 for
    none -- exact, one launch (mvae_corpus_index_probe)."""
    B, T = x.shape
    check(L.load().mvae_corpus_index_probe(ptr(tokens), ptr(offsets), N, ptr(slots), slots.numel(), B, T, ptr(x), x.stride(0), int(eos),
                                           ptr(match), stream_ptr()), "mvae_corpus_index_probe")


def relu_bwd(dy, y):
    check(L.load().mvae_relu_bwd(dy.numel(), ptr(dy), ptr(y), stream_ptr()), "mvae_relu_bwd")


def mask_rows_tb(buf, T, B, lengths):
    """rows (t*B + b) with t >= lengths[b] of the time-major [T*B, ld] buffer := 0."""
    check(L.load().mvae_mask_rows_tb(dt_code(buf.dtype), T, B, buf.stride(0), ptr(lengths), ptr(buf), stream_ptr()), "mvae_mask_rows_tb")


def permute102(inp, out, T, B, V):
    check(L.load().mvae_permute102(T, B, V, ptr(inp), ptr(out), stream_ptr()), "mvae_permute102")


def _sample_head(h_top, ldh, w_fc, bias, temp, filt, seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out, B, V, H):
    """The arguments the four sampling launches share, `dtype, B, V, H, h_top ... w_out`; filt: () or (top_k, top_p), which follow temp."""
    return (dt_code(h_top.dtype), B, V, H, ptr(h_top), ldh, ptr(w_fc), w_fc.stride(0), ptr(bias), float(temp), *filt, int(seed) & 0xFFFFFFFF,
            int(step), int(eos_id), ptr(table), table.shape[1], ptr(base), ptr(add_out), ptr(x), x.stride(0), ptr(end_pads), ptr(eos_mask),
            ptr(w_out))


def moses_sample_step(h_top, ldh, w_fc, bias, temp, seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out, B, V, H):
    """One generated token behind the GRU step: head GEMV, temperature softmax, multinomial draw (counter hash of (seed, step, row)), the
    reference's eos / end-pad bookkeeping and the next step's layer-0 addend rows -- one launch (mvae_moses_sample_step)."""
    head = _sample_head(h_top, ldh, w_fc, bias, temp, (), seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out, B, V, H)
    check(L.load().mvae_moses_sample_step(*head, stream_ptr()), "mvae_moses_sample_step")


def moses_sample_filtered_step(h_top, ldh, w_fc, bias, temp, top_k, top_p, seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out,
                               B, V, H, logq=None, hash=None):
    """moses_sample_step with top-k (0: off) / top-p (>= 1: off) truncation; logq [B] fp32 accumulates the drawn token's log-probability
    under the truncated distribution and hash [B] int64 the FNV-1a hash of the row's tokens, for the rows that had not ended -- one launch
    (mvae_moses_sample_filtered_step)."""
    head = _sample_head(h_top, ldh, w_fc, bias, temp, (int(top_k), float(top_p)), seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask,
                        w_out, B, V, H)
    check(L.load().mvae_moses_sample_filtered_step(*head, ptr(logq), ptr(hash), stream_ptr()), "mvae_moses_sample_filtered_step")


def moses_sample_syntax_step(h_top, ldh, w_fc, bias, temp, top_k, top_p, seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out,
                             B, V, H, tok_info, gstate, max_len, logq=None, hash=None):
    """moses_sample_filtered_step under the SMILES syntax automaton: tok_info int32 [V] (vocab.smiles_token_table), gstate int32 [B, 2] the
    packed state of every row (advanced by the drawn token for the rows that had not ended).  Tokens the automaton refuses, or after which
    the string could not be finished by step max_len - 1, are masked before the softmax -- one launch (mvae_moses_sample_syntax_step)."""
    head = _sample_head(h_top, ldh, w_fc, bias, temp, (int(top_k), float(top_p)), seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask,
                        w_out, B, V, H)
    check(L.load().mvae_moses_sample_syntax_step(*head, ptr(logq), ptr(hash), ptr(tok_info), ptr(gstate), int(max_len), stream_ptr()),
          "mvae_moses_sample_syntax_step")


def moses_sample_forced_step(h_top, ldh, w_fc, bias, temp, top_k, top_p, seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask, w_out,
                             B, V, H, forced, tok_info=None, gstate=None, max_len=0, logq=None, hash=None):
    """moses_sample_filtered_step (tok_info / gstate None) or moses_sample_syntax_step with forced tokens: forced int32 [B, >= step + 1],
    forced[b, step] >= 0 is written in place of a drawn token -- bookkeeping, hash and automaton state as for a drawn one, nothing added
    to logq --, -1 leaves the row to the draw of the sibling launch -- one launch (mvae_moses_sample_forced_step)."""
    head = _sample_head(h_top, ldh, w_fc, bias, temp, (int(top_k), float(top_p)), seed, step, eos_id, table, base, add_out, x, end_pads, eos_mask,
                        w_out, B, V, H)
    check(L.load().mvae_moses_sample_forced_step(*head, ptr(logq), ptr(hash), ptr(tok_info), ptr(gstate), int(max_len), ptr(forced),
                                                 forced.stride(0), stream_ptr()), "mvae_moses_sample_forced_step")


def smiles_prefix_state(ids, lens, tok_info, state, need, bad_pos):
    """The SMILES automaton over prefixes: ids int32 [B, P] (any row stride), lens int32 [B]; per row the packed state int32 [B, 2] reached
    after ids[b, :lens[b]], need [B] int32 = the tokens still required to finish from it (<eos> included) and bad_pos [B] int32 = the index
    of the first refused token, -1 if none (mvae_smiles_prefix_state)."""
    B, P = ids.shape
    check(L.load().mvae_smiles_prefix_state(B, P, tok_info.numel(), ptr(ids), ids.stride(0), ptr(lens), ptr(tok_info), ptr(state), ptr(need),
                                            ptr(bad_pos), stream_ptr()), "mvae_smiles_prefix_state")


def smiles_syntax_check(x, tok_info, eos_id, valid, bad_pos=None):
    """valid [B] uint8 = 1 where the token row x[b] (int64 [B, T], bos first) is a well-formed SMILES string ending in <eos>; bad_pos [B]
    int32: the first refused index, T without <eos>, -1 when valid (mvae_smiles_syntax_check)."""
    B, T = x.shape
    check(L.load().mvae_smiles_syntax_check(B, T, tok_info.numel(), ptr(x), x.stride(0), ptr(tok_info), int(eos_id), ptr(valid), ptr(bad_pos),
                                            stream_ptr()), "mvae_smiles_syntax_check")


def _beam_head(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H):
    """The arguments the three beam launches share, `dtype, B, K, V, H, layers, state ... hist_par`."""
    return (dt_code(state.dtype), B, K, V, H, state.shape[0], ptr(state), state.stride(0), state.stride(1), ldh, ptr(w_fc), w_fc.stride(0),
            ptr(bias), int(step), int(eos_id), int(pad_id), ptr(table), table.shape[1], ptr(base), ptr(add_out), ptr(score), ptr(fin), ptr(ends),
            ptr(hist_tok), ptr(hist_par))


def moses_beam_step(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H):
    """One beam-search token behind the GRU step: head GEMV, log-softmax, per-beam top-K, per-molecule merge, backpointers and the next
    step's layer-0 addend rows, and the recurrent state reordered from state[:, 1] (just written) into state[:, 0] (the next h0) -- one
    launch (mvae_moses_beam_step).  state: [layers, 2, B*K, ldh] in the compute dtype."""
    head = _beam_head(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H)
    check(L.load().mvae_moses_beam_step(*head, stream_ptr()), "mvae_moses_beam_step")


def moses_beam_syntax_step(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H,
                           tok_info, gstate, max_len):
    """moses_beam_step over well-formed SMILES strings only: tok_info int32 [V] (vocab.smiles_token_table), gstate int32 [B*K, 2] the packed
    automaton state of every beam row (reordered and advanced with the beams).  A row proposes only tokens the automaton takes and after
    which the string can still be finished by step max_len - 1; the scores stay log-probabilities over all V classes -- one launch
    (mvae_moses_beam_syntax_step)."""
    head = _beam_head(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H)
    check(L.load().mvae_moses_beam_syntax_step(*head, ptr(tok_info), ptr(gstate), int(max_len), stream_ptr()), "mvae_moses_beam_syntax_step")


def moses_beam_forced_step(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H,
                           forced, tok_info=None, gstate=None, max_len=0):
    """moses_beam_step (tok_info / gstate None) or moses_beam_syntax_step with forced tokens: forced int32 [B, >= step + 1], one row per
    molecule; forced[m, step] >= 0 is the only candidate an active beam of molecule m proposes (at score + logp[forced], unmasked), -1
    leaves the molecule to the sibling launch's search -- one launch (mvae_moses_beam_forced_step)."""
    head = _beam_head(state, ldh, w_fc, bias, step, eos_id, pad_id, table, base, add_out, score, fin, ends, hist_tok, hist_par, B, K, V, H)
    check(L.load().mvae_moses_beam_forced_step(*head, ptr(tok_info), ptr(gstate), int(max_len), ptr(forced), forced.stride(0), stream_ptr()),
          "mvae_moses_beam_forced_step")


def moses_beam_finalize(hist_tok, hist_par, ends, score, ids, ends_out, score_out, bos_id, B, K, max_len):
    """ids [B, K, max_len] int64 from the beam search's backpointers, in score order; ends / scores copied out (mvae_moses_beam_finalize)."""
    check(L.load().mvae_moses_beam_finalize(B, K, max_len, int(bos_id), ptr(hist_tok), ptr(hist_par), ptr(ends), ptr(score), ptr(ids),
                                            ptr(ends_out), ptr(score_out), stream_ptr()), "mvae_moses_beam_finalize")


def ce_rows(logits, ldl, x, pad, out, B, T, V):
    """out[b] = log p(x[b] | z) from time-major teacher-forced logits, pad targets ignored (mvae_ce_rows_fwd)."""
    check(L.load().mvae_ce_rows_fwd(B, T, V, ptr(logits), ldl, ptr(x), pad, ptr(out), stream_ptr()), "mvae_ce_rows_fwd")

def gauss_iw_draw(mu, logvar, z_out, logw_out, B, K, dz, eps=None, seed=0, offset=0, ld=None):
    """K draws per molecule from N(mu_b, exp(logvar_b)): z_out [B*K, dz] (row b*K + k), logw_out [B*K] = log N(z; 0, I) - log N(z; mu, sigma^2);
    eps [B*K, dz] injected, or None: the counter normal n(seed, offset + row*dz + d) (mvae_gauss_iw_draw)."""
    check(L.load().mvae_gauss_iw_draw(B, K, dz, ptr(mu), ptr(logvar), ld or dz, ptr(eps), int(seed) & 0xFFFFFFFF, int(offset), ptr(z_out),
                                      ptr(logw_out), stream_ptr()), "mvae_gauss_iw_draw")


def group_logmeanexp(a, lme_out, mean_out, G, K, b=None):
    """Per group of K values v = a (+ b): lme_out[g] = log mean_k exp(v), mean_out[g] = mean_k v (mvae_group_logmeanexp)."""
    check(L.load().mvae_group_logmeanexp(G, K, ptr(a), ptr(b), ptr(lme_out), ptr(mean_out), stream_ptr()), "mvae_group_logmeanexp")


def gauss_pairwise_lse(z, mu, logvar, out, Nz, Nx, dz, ldz=None, ldp=None):
    """out[i] = logsumexp_j log N(z_i; mu_j, exp(logvar_j)) (mvae_gauss_pairwise_lse; its workspace comes from Scratch)."""
    lib = L.load()
    nb = lib.mvae_gauss_pairwise_lse_workspace(Nz, Nx, dz)
    ws = Scratch.get(nb, out.device, "pairwise_lse") if nb else None
    check(lib.mvae_gauss_pairwise_lse(Nz, Nx, dz, ptr(z), ldz or dz, ptr(mu), ptr(logvar), ldp or dz, ptr(out), ptr(ws), nb, stream_ptr()),
          "mvae_gauss_pairwise_lse")


def _knn_outputs(Q, k, dev, value_dtype, exclude, values, idx):
    """What the three k-NN wrappers share: exclude (int64 [Q] or None) checked and made contiguous, values [Q, k] of value_dtype and idx
    [Q, k] int64 allocated where not given, and checked."""
    if exclude is not None:
        assert exclude.dtype == torch.int64 and exclude.shape == (Q,) and exclude.device == dev
        exclude = exclude.contiguous()
    if values is None:
        values = torch.empty(Q, max(k, 0), dtype=value_dtype, device=dev)
    if idx is None:
        idx = torch.empty(Q, max(k, 0), dtype=torch.int64, device=dev)
    assert values.shape == (Q, k) and idx.shape == (Q, k) and values.is_contiguous() and idx.is_contiguous()
    assert values.dtype == value_dtype and idx.dtype == torch.int64 and values.device == dev == idx.device
    return exclude, values, idx


def latent_knn(q, table, k, exclude=None, dist=None, idx=None):
    """The k nearest rows of table [N, dz] for every row of q [Q, dz] (float32, unit stride along d; row strides are passed through) by
    squared Euclidean distance, summed as direct f32 differences: (dist [Q, k] float32, idx [Q, k] int64), ascending in (distance, row);
    exclude (int64 [Q], optional) names one table row per query to skip (-1: none); rows at a NaN distance are skipped; a short tail
    is (+inf, -1) (mvae_latent_knn; its workspace comes from Scratch)."""
    lib = L.load()
    assert q.dim() == 2 and table.dim() == 2 and q.shape[1] == table.shape[1], (q.shape, table.shape)
    assert q.dtype == table.dtype == torch.float32 and q.device == table.device
    Q, dz = q.shape
    N, k = table.shape[0], int(k)
    if dz > 1 and q.stride(1) != 1:
        q = q.contiguous()
    if dz > 1 and table.stride(1) != 1:
        table = table.contiguous()
    ldq = q.stride(0) if Q > 1 else max(q.stride(0), dz)
    ldt = table.stride(0) if N > 1 else max(table.stride(0), dz)
    exclude, dist, idx = _knn_outputs(Q, k, q.device, torch.float32, exclude, dist, idx)
    nb = lib.mvae_latent_knn_workspace(Q, N, dz, k)
    ws = Scratch.get(nb, q.device, "latent_knn") if nb else None
    check(lib.mvae_latent_knn(Q, N, dz, k, ptr(q), ldq, ptr(table), ldt, ptr(exclude), ptr(dist), ptr(idx), ptr(ws), nb, stream_ptr()),
          "mvae_latent_knn")
    return dist, idx


EDIT_PATTERN_MAX = 128                       # include/mvae.h: MVAE_EDIT_PATTERN_MAX, the longest content on the pattern side
EDIT_K_MAX = 32
EDIT_V_MAX = 64
EDIT_NONE = 2147483647                       # MVAE_EDIT_NONE: the distance of an empty k-NN entry


def _csr(tokens, offsets, N):
    assert tokens.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.numel() >= N + 1 and tokens.device == offsets.device
    assert tokens.is_contiguous() and offsets.is_contiguous()


def _token_rows(t, name):
    assert t.dim() == 2 and t.dtype == torch.int64 and t.shape[0] >= 1 and t.shape[1] >= 1, (name, t.dtype, tuple(t.shape))
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def edit_distance_rows(a, b, eos, V, dist=None):
    """dist [B] int32 := the token-level Levenshtein distance between the content of a[i] and of b[i] (int64 [B, Ta] / [B, Tb], bos first;
    the content is what stands between column 0 and the first `eos`, or the last column), ids outside [0, V) equal to nothing -- one
    launch (mvae_edit_distance_rows).  The distance is symmetric, so the narrower tensor goes to the kernel's pattern side (at most 129
    columns); ValueError when both are wider."""
    a, lda = _token_rows(a, "a")
    b, ldb = _token_rows(b, "b")
    assert a.shape[0] == b.shape[0] and a.device == b.device, (a.shape, b.shape)
    if min(a.shape[1], b.shape[1]) - 1 > EDIT_PATTERN_MAX:
        raise ValueError(f"edit_distance_rows: one side must have at most {EDIT_PATTERN_MAX + 1} columns, got {a.shape[1]} and {b.shape[1]}")
    if a.shape[1] > b.shape[1]:
        a, lda, b, ldb = b, ldb, a, lda
    B = a.shape[0]
    if dist is None:
        dist = torch.empty(B, dtype=torch.int32, device=a.device)
    assert dist.shape == (B,) and dist.dtype == torch.int32 and dist.is_contiguous() and dist.device == a.device
    check(L.load().mvae_edit_distance_rows(B, int(V), int(eos), ptr(a), lda, a.shape[1], ptr(b), ldb, b.shape[1], ptr(dist), stream_ptr()),
          "mvae_edit_distance_rows")
    return dist


def edit_knn(x, tokens, offsets, N, k, eos, V, exclude=None, dist=None, idx=None):
    """The k corpus rows of the CSR corpus (tokens uint8, offsets int64 [N + 1]) at the smallest token-level Levenshtein distance from the
    content of every row of x (int64 [Q, T], bos first, T <= 129): (dist [Q, k] int32, idx [Q, k] int64), ascending in (distance, row);
    exclude (int64 [Q], optional) names one corpus row per query to skip (-1: none); a short tail is (EDIT_NONE, -1) (mvae_edit_knn; its
    workspace comes from Scratch)."""
    lib = L.load()
    x, ldx = _token_rows(x, "x")
    Q, T = x.shape
    N, k = int(N), int(k)
    _csr(tokens, offsets, N)
    assert tokens.device == x.device
    exclude, dist, idx = _knn_outputs(Q, k, x.device, torch.int32, exclude, dist, idx)
    nb = lib.mvae_edit_knn_workspace(Q, N, k)
    ws = Scratch.get(nb, x.device, "edit_knn") if nb else None
    check(lib.mvae_edit_knn(Q, T, int(V), int(eos), ptr(x), ldx, ptr(tokens), ptr(offsets), N, k, ptr(exclude), ptr(dist), ptr(idx), ptr(ws), nb,
                            stream_ptr()), "mvae_edit_knn")
    return dist, idx


SMILES_ELEMENTS = 11                          # include/mvae.h: MVAE_SMILES_ELEMENTS, the columns of `formula`
SMILES_DESC = 8                               # MVAE_SMILES_DESC, the columns of `desc`
SMILES_CONTENT_MAX = 127                      # MVAE_SMILES_CONTENT_MAX: a well-formed row with more content tokens is TOO_LONG
SMILES_DESC_NAMES = ("heavy_atoms", "bonds", "rings", "ring_atoms", "aromatic_atoms", "hydrogens", "charge", "hetero_atoms")
(SMILES_OK, SMILES_SYNTAX, SMILES_VALENCE, SMILES_CHARGE, SMILES_RING_BOND, SMILES_AROMATIC, SMILES_TOO_LONG) = range(7)
SMILES_STATUS_NAMES = ("ok", "syntax", "valence", "charge", "ring_bond", "aromatic", "too_long")


def _outputs(n, dev, spec, given):
    """The output tensors of an entry over n rows.  spec: per output (dtype, trailing shape, may be False); given: the caller's tensors in
    the same order -- None: allocated here; False where the spec allows it: not computed, None in its place."""
    out = []
    for (dt, tail, optional), t in zip(spec, given):
        if t is None:
            t = torch.empty(n, *tail, dtype=dt, device=dev)
        elif t is False and optional:
            t = None
        assert t is None or (t.dtype == dt and tuple(t.shape) == (n,) + tail and t.is_contiguous() and t.device == dev), (dt, (n,) + tail)
        out.append(t)
    return tuple(out)


# status, bad_pos, desc, formula: the outputs of a family as _outputs reads them, in the order of the C entries' arguments
_GRAPH_OUT = ((torch.int32, (), False), (torch.int32, (), False), (torch.int32, (SMILES_DESC,), False), (torch.int32, (SMILES_ELEMENTS,), False))


def _graph_tables(tok_info, chem_info, dev):
    assert tok_info.dtype == chem_info.dtype == torch.int32 and tok_info.dim() == 1 and tok_info.shape == chem_info.shape
    assert tok_info.is_contiguous() and chem_info.is_contiguous() and tok_info.device == chem_info.device == dev


def _smiles_rows(fn, spec, x, tok_info, chem_info, eos_id, given, host=False):
    """What the mvae_smiles_<family>_rows and _host entries share: the tensor checks, the outputs of `spec`, the call.  fn: the C entry."""
    x, ldx = _token_rows(x, "x")
    assert not host or x.device.type == "cpu", x.device
    _graph_tables(tok_info, chem_info, x.device)
    out = _outputs(x.shape[0], x.device, spec, given)
    check(fn(x.shape[0], x.shape[1], tok_info.numel(), ptr(x), ldx, ptr(tok_info), ptr(chem_info), int(eos_id), *map(ptr, out),
             *(() if host else (stream_ptr(),))), fn.__name__)
    return out


def _smiles_corpus(fn, spec, tokens, offsets, N, tok_info, chem_info, given):
    """The same for the mvae_smiles_<family>_corpus entries."""
    N = int(N)
    _csr(tokens, offsets, N)
    _graph_tables(tok_info, chem_info, tokens.device)
    out = _outputs(max(N, 0), tokens.device, spec, given)
    check(fn(ptr(tokens), ptr(offsets), N, tok_info.numel(), ptr(tok_info), ptr(chem_info), *map(ptr, out), stream_ptr()), fn.__name__)
    return out


def smiles_graph_rows(x, tok_info, chem_info, eos_id, status=None, bad_pos=None, desc=None, formula=None):
    """The SMILES graph walk over token rows x (int64 [B, T], bos first) on the device: (status [B], bad_pos [B], desc [B, 8],
    formula [B, 11]), all int32 -- status 0 where the row is well-formed AND valence-consistent (include/mvae.h, "SMILES graph"), the
    counts and the molecular formula of those rows, zeros for the others.  tok_info / chem_info: vocab.smiles_token_table /
    smiles_chem_table on x's device.  One launch (mvae_smiles_graph_rows)."""
    return _smiles_rows(L.load().mvae_smiles_graph_rows, _GRAPH_OUT, x, tok_info, chem_info, eos_id, (status, bad_pos, desc, formula))


def smiles_graph_corpus(tokens, offsets, N, tok_info, chem_info, status=None, bad_pos=None, desc=None, formula=None):
    """smiles_graph_rows over the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a row acting as <eos>,
    bad_pos 0-based in the row): one launch (mvae_smiles_graph_corpus)."""
    return _smiles_corpus(L.load().mvae_smiles_graph_corpus, _GRAPH_OUT, tokens, offsets, N, tok_info, chem_info, (status, bad_pos, desc, formula))


def smiles_graph_host(x, tok_info, chem_info, eos_id, status=None, bad_pos=None, desc=None, formula=None):
    """smiles_graph_rows on HOST tensors: the same walk compiled for the CPU, a plain loop over the rows (mvae_smiles_graph_host) -- for
    tests and for machines without a device; not a fallback of the device entries."""
    return _smiles_rows(L.load().mvae_smiles_graph_host, _GRAPH_OUT, x, tok_info, chem_info, eos_id, (status, bad_pos, desc, formula), host=True)


_ATOMIC_WEIGHTS = {}                          # device -> vocab.ATOMIC_WEIGHTS as float32 [11]


def graph_descriptors(status, bad_pos, desc, formula):
    """The outputs of a smiles_graph_* launch as the dict VAE.descriptors documents: status, bad_pos, the eight desc columns by name,
    formula and weight = formula . vocab.ATOMIC_WEIGHTS (float32; 0 for rows that are not ok, whose formula is zero)."""
    from .vocab import ATOMIC_WEIGHTS
    dev = formula.device
    w = _ATOMIC_WEIGHTS.get(dev)
    if w is None:                                # uploaded once per device, so that later calls never wait
        w = _ATOMIC_WEIGHTS[dev] = torch.tensor(ATOMIC_WEIGHTS, dtype=torch.float32).to(dev)
    out = {"status": status, "bad_pos": bad_pos}
    out.update((name, desc[:, i]) for i, name in enumerate(SMILES_DESC_NAMES))
    out["formula"] = formula
    out["weight"] = formula.float() @ w
    return out


FP_WORDS = 16                                 # include/mvae.h: MVAE_FP_WORDS, the int64 words of a fingerprint (1024 bits)
TANIMOTO_K_MAX = 32
_FP_OUT = ((torch.int32, (), False), (torch.int64, (FP_WORDS,), False))                                  # status, fp


def smiles_fp_rows(x, tok_info, chem_info, eos_id, status=None, fp=None):
    """The circular fingerprint of token rows x (int64 [B, T], bos first) on the device: (status int32 [B], fp int64 [B, 16]) -- the
    status of smiles_graph_rows and 1024 bits per row, radius 2, built like ECFP4 but NOT rdkit's Morgan fingerprint (include/mvae.h,
    "Circular fingerprint"); all zeros for a row whose status is not 0.  One launch (mvae_smiles_fp_rows)."""
    return _smiles_rows(L.load().mvae_smiles_fp_rows, _FP_OUT, x, tok_info, chem_info, eos_id, (status, fp))


def smiles_fp_corpus(tokens, offsets, N, tok_info, chem_info, status=None, fp=None):
    """smiles_fp_rows over the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a row acting as
    <eos>): one launch (mvae_smiles_fp_corpus)."""
    return _smiles_corpus(L.load().mvae_smiles_fp_corpus, _FP_OUT, tokens, offsets, N, tok_info, chem_info, (status, fp))


def smiles_fp_host(x, tok_info, chem_info, eos_id, status=None, fp=None):
    """smiles_fp_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows (mvae_smiles_fp_host) -- for tests
    and for machines without a device; not a fallback of the device entries."""
    return _smiles_rows(L.load().mvae_smiles_fp_host, _FP_OUT, x, tok_info, chem_info, eos_id, (status, fp), host=True)


def _fp_table(t, name):
    assert t.dim() == 2 and t.shape[1] == FP_WORDS and t.dtype == torch.int64 and t.shape[0] >= 1, (name, t.dtype, tuple(t.shape))
    return t.contiguous()


def tanimoto_knn(q, table, k, exclude=None, sim=None, idx=None):
    """The k rows of table [N, 16] most similar to every row of q [Q, 16] (int64 fingerprints) by Tanimoto similarity |a & b| / |a | b|
    (0 for an empty union; one correctly rounded f32 division): (sim [Q, k] float32, idx [Q, k] int64), ordered by (similarity
    descending, row ascending); exclude (int64 [Q], optional) names one table row per query to skip (-1: none); a short tail is
    (-1.0, -1) (mvae_tanimoto_knn; its workspace comes from Scratch)."""
    lib = L.load()
    q, table = _fp_table(q, "q"), _fp_table(table, "table")
    assert q.device == table.device
    Q, N, k = q.shape[0], table.shape[0], int(k)
    exclude, sim, idx = _knn_outputs(Q, k, q.device, torch.float32, exclude, sim, idx)
    nb = lib.mvae_tanimoto_knn_workspace(Q, N, k)
    ws = Scratch.get(nb, q.device, "tanimoto_knn") if nb else None
    check(lib.mvae_tanimoto_knn(Q, N, k, ptr(q), ptr(table), ptr(exclude), ptr(sim), ptr(idx), ptr(ws), nb, stream_ptr()), "mvae_tanimoto_knn")
    return sim, idx


def tanimoto_sum(a, b, skip_diagonal=False, out=None):
    """out (float64 [1], on the device) := the sum of the f32 Tanimoto similarities over all ordered pairs of a [M, 16] and b [N, 16]
    (int64 fingerprints); skip_diagonal leaves out the pairs with i == j.  Accumulated in float64 in a fixed order, two runs are bitwise
    equal (mvae_tanimoto_sum; its workspace comes from Scratch).  IntDiv = 1 - tanimoto_sum(a, a) / M^2 is the MOSES form (diagonal
    included); skip_diagonal and M (M - 1) give the other convention."""
    lib = L.load()
    a, b = _fp_table(a, "a"), _fp_table(b, "b")
    assert a.device == b.device
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=a.device)
    assert out.dtype == torch.float64 and out.shape == (1,) and out.device == a.device
    M, N = a.shape[0], b.shape[0]
    nb = lib.mvae_tanimoto_sum_workspace(M, N)
    ws = Scratch.get(nb, a.device, "tanimoto_sum")
    check(lib.mvae_tanimoto_sum(M, N, ptr(a), ptr(b), int(bool(skip_diagonal)), ptr(out), ptr(ws), nb, stream_ptr()), "mvae_tanimoto_sum")
    return out


GRAPH_KEY_ROUNDS = 8                          # include/mvae.h: MVAE_GRAPH_KEY_ROUNDS
SCAFFOLD_DESC = ("atoms", "bonds", "linker_atoms", "exo_atoms")      # the columns of desc [*, 4]
# status, mask, desc, key
_SCAFFOLD_OUT = ((torch.int32, (), False), (torch.int64, (2,), True), (torch.int32, (4,), False), (torch.int64, (2,), False))


def smiles_scaffold_rows(x, tok_info, chem_info, eos_id, status=None, mask=None, desc=None, key=None):
    """The Murcko scaffold and the graph keys of token rows x (int64 [B, T], bos first) on the device: (status int32 [B], mask int64
    [B, 2], desc int32 [B, 4], key int64 [B, 2]) -- the status of smiles_graph_rows; bit a of mask word a >> 6 = atom a (string order) is in
    the scaffold; desc = scaffold atoms, scaffold bonds, linker atoms, exo atoms; key = (molecule key, scaffold key), 0 = none.  Defined
    on the walk's graph, NOT rdkit's MurckoScaffold, and the keys ignore stereochemistry (include/mvae.h, "Murcko scaffold", "Graph
    key").  Zeros for a row whose status is not 0.  ``mask=False``: no mask is computed (None is returned in its place).  One launch
    (mvae_smiles_scaffold_rows)."""
    return _smiles_rows(L.load().mvae_smiles_scaffold_rows, _SCAFFOLD_OUT, x, tok_info, chem_info, eos_id, (status, mask, desc, key))


def smiles_scaffold_corpus(tokens, offsets, N, tok_info, chem_info, status=None, mask=None, desc=None, key=None):
    """smiles_scaffold_rows over the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a row acting as
    <eos>): one launch (mvae_smiles_scaffold_corpus)."""
    return _smiles_corpus(L.load().mvae_smiles_scaffold_corpus, _SCAFFOLD_OUT, tokens, offsets, N, tok_info, chem_info, (status, mask, desc, key))


def smiles_scaffold_host(x, tok_info, chem_info, eos_id, status=None, mask=None, desc=None, key=None):
    """smiles_scaffold_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_scaffold_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    return _smiles_rows(L.load().mvae_smiles_scaffold_host, _SCAFFOLD_OUT, x, tok_info, chem_info, eos_id, (status, mask, desc, key), host=True)


def scaffold_dict(status, mask, desc, key):
    """The outputs of the scaffold entries under their names: status, mask, atoms, bonds, linker_atoms, exo_atoms, mol_key, scaffold_key."""
    out = {"status": status, "mask": mask}
    out.update((name, desc[:, i]) for i, name in enumerate(SCAFFOLD_DESC))
    out["mol_key"], out["scaffold_key"] = key[:, 0], key[:, 1]
    return out


SMILES_STATUS_KEKULE = 7                      # include/mvae.h: MVAE_SMILES_KEKULE, given by the kekule entries only
KEKULE_STATUS_NAMES = SMILES_STATUS_NAMES + ("kekule",)
KEKULE_DESC = ("n_atoms", "n_bonds", "pairs", "deficiency")          # the columns of desc [*, 4]: |N|, |E|, maximum matching, |N| - 2 pairs
_KEKULE_OUT = ((torch.int32, (), False), (torch.int32, (4,), False), (torch.uint8, (128,), True))        # status, desc, mate


def smiles_kekule_rows(x, tok_info, chem_info, eos_id, status=None, desc=None, mate=None):
    """The kekulisation test of token rows x (int64 [B, T], bos first) on the device: (status int32 [B], desc int32 [B, 4], mate uint8
    [B, 128]) -- the status of smiles_graph_rows, except that a row it calls 0 whose aromatic atoms cannot all take their one ring double
    bond gets SMILES_STATUS_KEKULE (7); desc = |N|, |E|, the size of a maximum matching, the deficiency, for status 0 and 7 (zeros
    otherwise); mate[a] = the partner of atom a in the matching found, 255 = none.  Status 0 here means "kekulisable": a tighter
    necessary condition than valence-consistent, NOT rdkit's Kekulize or SanitizeMol, no aromaticity perception (include/mvae.h,
    "Kekulisation").  ``mate=False``: no mate is written (None is returned in its place).  One launch (mvae_smiles_kekule_rows)."""
    return _smiles_rows(L.load().mvae_smiles_kekule_rows, _KEKULE_OUT, x, tok_info, chem_info, eos_id, (status, desc, mate))


def smiles_kekule_corpus(tokens, offsets, N, tok_info, chem_info, status=None, desc=None, mate=None):
    """smiles_kekule_rows over the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a row acting as
    <eos>): one launch (mvae_smiles_kekule_corpus)."""
    return _smiles_corpus(L.load().mvae_smiles_kekule_corpus, _KEKULE_OUT, tokens, offsets, N, tok_info, chem_info, (status, desc, mate))


def smiles_kekule_host(x, tok_info, chem_info, eos_id, status=None, desc=None, mate=None):
    """smiles_kekule_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows (mvae_smiles_kekule_host) --
    for tests and for machines without a device; not a fallback of the device entries."""
    return _smiles_rows(L.load().mvae_smiles_kekule_host, _KEKULE_OUT, x, tok_info, chem_info, eos_id, (status, desc, mate), host=True)


def kekule_dict(status, desc, mate):
    """The outputs of the kekule entries under their names: status, n_atoms, n_bonds, pairs, deficiency, mate."""
    out = {"status": status}
    out.update((name, desc[:, i]) for i, name in enumerate(KEKULE_DESC))
    out["mate"] = mate
    return out


# include/mvae.h, "SMILES rewrite": MVAE_SMILES_STEREO .. MVAE_SMILES_NO_TOKEN, given by the rewrite entries only
(SMILES_STATUS_STEREO, SMILES_STATUS_RING_MULTI, SMILES_STATUS_RING_DIGITS, SMILES_STATUS_DEPTH, SMILES_STATUS_LONG,
 SMILES_STATUS_NO_TOKEN) = range(8, 14)
REWRITE_STATUS_NAMES = KEKULE_STATUS_NAMES + ("stereo", "ring_multi", "ring_digits", "depth", "long", "no_token")
REWRITE_COUNTS = 16                           # the length of the per-status histogram
REWRITE_EMIT = 48                             # include/mvae.h: MVAE_REWRITE_EMIT


def _rewrite_tables(tok_info, chem_info, emit, draw, counts, n, dev, max_content, n_counts=16):
    _graph_tables(tok_info, chem_info, dev)
    assert emit.dtype == torch.int32 and emit.shape == (REWRITE_EMIT,) and emit.is_contiguous() and emit.device == dev, (emit.dtype, emit.shape)
    if not 1 <= int(max_content) <= 127:
        raise ValueError(f"smiles_rewrite: max_content must be in [1, 127], got {max_content}")
    if draw is not None:                         # uint32 [n], carried as int32 bits
        assert draw.dtype == torch.int32 and draw.shape == (n,) and draw.is_contiguous() and draw.device == dev, (draw.dtype, tuple(draw.shape))
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.shape == (n_counts,) and counts.is_contiguous() and counts.device == dev


def draw_words(values):
    """An integer tensor (any values; taken mod 2^32) as the int32 tensor whose bits are the uint32 `draw` argument of the rewrite entries."""
    v = values.to(torch.int64) & 0xFFFFFFFF
    return torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)


CANON_INFO = ("atoms", "first_classes", "rounds", "ties")          # the columns of info [*, 4] (include/mvae.h: MVAE_CANON_INFO)
_CANON_OUT = ((torch.int32, (len(CANON_INFO),), True), (torch.uint8, (128,), True))      # info, rank: what canon writes beside the row


def _writer_rows(name, host, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, family_in, max_content, T_out, extra, given, counts,
                 family_ints=(), n_counts=None):
    """What the mvae_smiles_rewrite / _canon _rows and _host entries share: the tensor checks, the outputs, the call of the C entry
    `name`.  family_in: (seed, draw) where the entry takes them (behind pad_id), () where not; extra: the spec of the outputs behind
    (out, out_len, status), which the C entries take behind counts; given: the caller's outputs, all of them, as ``_outputs`` reads them;
    family_ints: the integers an entry takes in front of those outputs (frag); n_counts: the length of its counts where not 16."""
    x, ldx = _token_rows(x, "x")
    assert not host or x.device.type == "cpu", x.device
    B, T = x.shape
    seed, draw = family_in or (0, None)
    _rewrite_tables(tok_info, chem_info, emit, draw, counts, B, x.device, max_content, n_counts or REWRITE_COUNTS)
    T_out = max(T, int(max_content) + 2) if T_out is None else int(T_out)
    res = _outputs(B, x.device, ((torch.int64, (T_out,), False), (torch.int32, (), False), (torch.int32, (), False)) + extra, given)
    check(getattr(L.load(), name)(B, T, tok_info.numel(), ptr(x), ldx, ptr(tok_info), ptr(chem_info), ptr(emit), int(bos_id), int(eos_id),
                                  int(pad_id), *((int(seed) & 0xFFFFFFFF, ptr(draw)) if family_in else ()), int(max_content), T_out,
                                  *map(ptr, res[:3]), *(() if host else (ptr(counts),)), *map(int, family_ints), *map(ptr, res[3:]),
                                  *(() if host else (stream_ptr(),))), name)
    return res


def _writer_corpus(name, tokens, offsets, N, rows, tok_info, chem_info, emit, family_in, max_content, stride, extra, given, counts, err,
                   family_ints=(), n_counts=None):
    """The same for the _corpus entries; given = (tokens_out, offsets_out, status) and the outputs of `extra`."""
    N, B = int(N), rows.numel()
    dev = tokens.device
    _csr(tokens, offsets, N)
    assert rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous() and rows.device == dev and B >= 1
    seed, draw = family_in or (0, None)
    _rewrite_tables(tok_info, chem_info, emit, draw, counts, B, dev, max_content, n_counts or REWRITE_COUNTS)
    stride = int(max_content) if stride is None else int(stride)
    offsets_out, = _outputs(2 * B + 1, dev, ((torch.int64, (), False),), given[1:2])
    tokens_out, status, *more = _outputs(B, dev, ((torch.uint8, (stride,), False), (torch.int32, (), False)) + extra, given[:1] + given[2:])
    assert err is None or (err.dtype == torch.int32 and err.numel() == 1 and err.device == dev)
    check(getattr(L.load(), name)(ptr(tokens), ptr(offsets), N, ptr(rows), B, tok_info.numel(), ptr(tok_info), ptr(chem_info), ptr(emit),
                                  *((int(seed) & 0xFFFFFFFF, ptr(draw)) if family_in else ()), int(max_content), stride, ptr(tokens_out),
                                  ptr(offsets_out), ptr(status), ptr(counts), ptr(err), *map(int, family_ints), *map(ptr, more), stream_ptr()), name)
    return (tokens_out, offsets_out, status, *more)


def smiles_rewrite_rows(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, seed=0, draw=None, max_content=127, T_out=None, out=None,
                        out_len=None, status=None, counts=None):
    """A randomised respelling of token rows x (int64 [B, T], bos first) on the device: (out int64 [B, T_out], out_len int32 [B], status
    int32 [B]) -- every row read into the walk's graph and written back from a random root in a random neighbour order, a pure function
    of (row, seed, draw[b]) (include/mvae.h, "SMILES rewrite"); a row that cannot be respelled (status != 0: the walk's 1 - 6, or
    SMILES_STATUS_STEREO .. SMILES_STATUS_NO_TOKEN) is copied through unchanged.  draw: int32 [B] holding uint32 bits (``draw_words``),
    None for the row number; T_out defaults to max(T, max_content + 2), so that nothing is cut; counts (int32 [16], optional, zeroed by
    the caller) += the per-status histogram.  NOT a canonical SMILES, no stereo, not rdkit's doRandom.  One launch
    (mvae_smiles_rewrite_rows)."""
    return _writer_rows("mvae_smiles_rewrite_rows", False, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (seed, draw), max_content, T_out,
                        (), (out, out_len, status), counts)


def smiles_rewrite_host(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, seed=0, draw=None, max_content=127, T_out=None, out=None,
                        out_len=None, status=None):
    """smiles_rewrite_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows (mvae_smiles_rewrite_host) --
    for tests and for machines without a device; not a fallback of the device entries."""
    return _writer_rows("mvae_smiles_rewrite_host", True, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (seed, draw), max_content, T_out,
                        (), (out, out_len, status), None)


def smiles_rewrite_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, seed=0, draw=None, max_content=127, stride=None, tokens_out=None,
                          offsets_out=None, status=None, counts=None, err=None):
    """smiles_rewrite_rows over the rows `rows` (int64 [B]) of the CSR corpus (tokens uint8, offsets int64 [N + 1]), one launch
    (mvae_smiles_rewrite_corpus): (tokens_out uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B]).  offsets_out = 0, len_0,
    stride, stride + len_1, ...: tokens_out is a CSR of 2 B rows whose even rows are the batch members, so ``moses_collate`` with rows =
    0, 2, 4, ... collates it unchanged.  stride defaults to max_content; err (int32 [1], optional, zeroed by the caller) is raised to 1
    by a copied-through row longer than stride and to 2 by a row id outside [0, N)."""
    return _writer_corpus("mvae_smiles_rewrite_corpus", tokens, offsets, N, rows, tok_info, chem_info, emit, (seed, draw), max_content, stride, (),
                          (tokens_out, offsets_out, status), counts, err)


def smiles_canon_rows(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None,
                      info=None, rank=None, counts=None):
    """The canonical spelling of token rows x (int64 [B, T], bos first) on the device: (out int64 [B, T_out], out_len int32 [B], status
    int32 [B], info int32 [B, 4], rank uint8 [B, 128]) -- ``smiles_rewrite_rows`` with the atoms ordered by a canonical rank instead of a
    hash (include/mvae.h, "SMILES canon"), so no seed and no draw: two spellings of one graph give one row (tested, not proved; no
    aromaticity perception, no stereo, NOT rdkit's canonical SMILES).  The statuses and the copy-through of a refused row are the
    rewrite's.  info = atoms, classes after the first refinement, rounds, ties (``CANON_INFO``); rank[k] = the canonical rank of atom k,
    0xFF beyond the atoms; ``info=False`` / ``rank=False``: not written (None in its place).  One launch (mvae_smiles_canon_rows)."""
    return _writer_rows("mvae_smiles_canon_rows", False, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out, _CANON_OUT,
                        (out, out_len, status, info, rank), counts)


def smiles_canon_host(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None,
                      info=None, rank=None):
    """smiles_canon_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows (mvae_smiles_canon_host) -- for
    tests and for machines without a device; not a fallback of the device entries."""
    return _writer_rows("mvae_smiles_canon_host", True, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out, _CANON_OUT,
                        (out, out_len, status, info, rank), None)


def smiles_canon_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, max_content=127, stride=None, tokens_out=None, offsets_out=None,
                        status=None, info=None, rank=None, counts=None, err=None):
    """smiles_canon_rows over the rows `rows` (int64 [B]) of the CSR corpus, one launch (mvae_smiles_canon_corpus): (tokens_out uint8
    [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4], rank uint8 [B, 128]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``, with its counts and err; ``info=False`` / ``rank=False``: not written (None in its place)."""
    return _writer_corpus("mvae_smiles_canon_corpus", tokens, offsets, N, rows, tok_info, chem_info, emit, (), max_content, stride, _CANON_OUT,
                          (tokens_out, offsets_out, status, info, rank), counts, err)


SMILES_STATUS_NO_RING = 14                    # include/mvae.h: MVAE_SMILES_NO_RING, given by the scaffold SMILES entries only
SCAFFOLD_SMILES_STATUS_NAMES = REWRITE_STATUS_NAMES + ("no_ring",)
SCAFFOLD_SMILES_INFO = ("atoms", "bonds", "new_brackets", "lost")      # the columns of info [*, 4] (MVAE_SCAFFOLD_SMILES_INFO)
_SCAFFOLD_SMILES_OUT = ((torch.int32, (len(SCAFFOLD_SMILES_INFO),), True),)


def smiles_scaffold_smiles_rows(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None,
                                status=None, info=None, counts=None):
    """The Murcko scaffold of token rows x (int64 [B, T], bos first) as token rows, on the device: (out int64 [B, T_out], out_len int32
    [B], status int32 [B], info int32 [B, 4]) -- the scaffold atom set of ``smiles_scaffold_rows`` cut out of the row's graph, every lost
    bond turned into hydrogens, in the spelling of ``smiles_canon_rows`` (include/mvae.h, "Scaffold SMILES").  A row without a scaffold
    (status != 0, ``SCAFFOLD_SMILES_STATUS_NAMES``: the canon entries' reasons, or 14 "no_ring") gets the EMPTY row bos, eos, pad..., and
    out_len 2 -- never a copy.  info = atoms and bonds of the scaffold, atoms that became bracket atoms, bond orders lost
    (``SCAFFOLD_SMILES_INFO``); ``info=False``: not written (None in its place).  NOT rdkit's MurckoScaffoldSmiles: nothing is sanitised,
    no aromaticity perception, no stereo.  One launch (mvae_smiles_scaffold_smiles_rows)."""
    return _writer_rows("mvae_smiles_scaffold_smiles_rows", False, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _SCAFFOLD_SMILES_OUT, (out, out_len, status, info), counts)


def smiles_scaffold_smiles_host(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None,
                                status=None, info=None):
    """smiles_scaffold_smiles_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_scaffold_smiles_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    return _writer_rows("mvae_smiles_scaffold_smiles_host", True, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _SCAFFOLD_SMILES_OUT, (out, out_len, status, info), None)


def smiles_scaffold_smiles_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, max_content=127, stride=None, tokens_out=None,
                                  offsets_out=None, status=None, info=None, counts=None, err=None):
    """smiles_scaffold_smiles_rows over the rows `rows` (int64 [B]) of the CSR corpus, one launch (mvae_smiles_scaffold_smiles_corpus):
    (tokens_out uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``, with its counts and err; a row without a scaffold is a slice of length 0."""
    return _writer_corpus("mvae_smiles_scaffold_smiles_corpus", tokens, offsets, N, rows, tok_info, chem_info, emit, (), max_content, stride,
                          _SCAFFOLD_SMILES_OUT, (tokens_out, offsets_out, status, info), counts, err)


FRAGMENT_MAX = 16                             # include/mvae.h: MVAE_FRAGMENT_MAX, the fragment slots of a row
SMILES_STATUS_FRAG_MANY = 15                  # MVAE_SMILES_FRAG_MANY, given by the fragment entries only: more than 16 fragments
SMILES_STATUS_NO_FRAGMENT = 16                # MVAE_SMILES_NO_FRAGMENT, given by the fragment SMILES entries only
FRAGMENT_STATUS_NAMES = SCAFFOLD_SMILES_STATUS_NAMES + ("frag_many",)                   # index = status; 7 - 14 are never given here
FRAGMENT_SMILES_STATUS_NAMES = FRAGMENT_STATUS_NAMES + ("no_fragment",)                 # 14 and 15 are never given here
FRAGMENT_DESC = ("fragments", "cuts", "acyl_cuts", "largest")       # the columns of desc [*, 4]
FRAGMENT_SMILES_INFO = SCAFFOLD_SMILES_INFO                         # the columns of info [*, 4] (MVAE_FRAGMENT_SMILES_INFO)
FRAGMENT_SMILES_COUNTS = 32                                         # MVAE_FRAGMENT_SMILES_COUNTS: the per-status histogram has a slot 16
# status, mask, desc, key
_FRAGMENT_OUT = ((torch.int32, (), False), (torch.int64, (FRAGMENT_MAX, 2), True), (torch.int32, (4,), False), (torch.int64, (FRAGMENT_MAX,), False))
_FRAGMENT_SMILES_OUT = ((torch.int32, (len(FRAGMENT_SMILES_INFO),), True),)


def smiles_fragment_rows(x, tok_info, chem_info, eos_id, status=None, mask=None, desc=None, key=None):
    """The fragments of token rows x (int64 [B, T], bos first) on the device: (status int32 [B], mask int64 [B, 16, 2], desc int32 [B, 4],
    key int64 [B, 16]) -- every row cut at its ring substituent bonds and its acyl-heteroatom bonds (include/mvae.h, "Fragments": this
    library's own rule, NOT BRICS, not RECAP, no agreement with a toolkit claimed); the fragments are numbered by their lowest atom; bit
    a of mask[b, f] word a >> 6 = atom a (string order) is in fragment f; desc = fragments, cuts, cuts by the acyl rule alone, atoms of
    the largest fragment; key[b, f] = the graph key of fragment f made as the scaffold key is, 0 in unused slots.  Zeros for a row whose
    status is not 0; a row with more than 16 fragments gets SMILES_STATUS_FRAG_MANY (15), zero mask and keys and its true desc.
    ``mask=False``: no mask is computed (None is returned in its place).  One launch (mvae_smiles_fragment_rows)."""
    return _smiles_rows(L.load().mvae_smiles_fragment_rows, _FRAGMENT_OUT, x, tok_info, chem_info, eos_id, (status, mask, desc, key))


def smiles_fragment_corpus(tokens, offsets, N, tok_info, chem_info, status=None, mask=None, desc=None, key=None):
    """smiles_fragment_rows over the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a row acting as
    <eos>): one launch (mvae_smiles_fragment_corpus)."""
    return _smiles_corpus(L.load().mvae_smiles_fragment_corpus, _FRAGMENT_OUT, tokens, offsets, N, tok_info, chem_info, (status, mask, desc, key))


def smiles_fragment_host(x, tok_info, chem_info, eos_id, status=None, mask=None, desc=None, key=None):
    """smiles_fragment_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_fragment_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    return _smiles_rows(L.load().mvae_smiles_fragment_host, _FRAGMENT_OUT, x, tok_info, chem_info, eos_id, (status, mask, desc, key), host=True)


def fragment_dict(status, mask, desc, key):
    """The outputs of the fragment entries under their names: status, mask, fragments, cuts, acyl_cuts, largest, keys."""
    out = {"status": status, "mask": mask}
    out.update((name, desc[:, i]) for i, name in enumerate(FRAGMENT_DESC))
    out["keys"] = key
    return out


def _frag(frag):
    if int(frag) < 0:
        raise ValueError(f"smiles_fragment_smiles: frag must be >= 0, got {frag}")
    return (int(frag),)


def smiles_fragment_smiles_rows(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, frag=0, max_content=127, T_out=None, out=None,
                                out_len=None, status=None, info=None, counts=None):
    """Fragment number ``frag`` (by lowest atom, from 0) of token rows x (int64 [B, T], bos first) as token rows, on the device: (out
    int64 [B, T_out], out_len int32 [B], status int32 [B], info int32 [B, 4]) -- the fragment of ``smiles_fragment_rows`` cut out of the
    row's graph, every lost bond turned into hydrogens, in the spelling of ``smiles_canon_rows`` (include/mvae.h, "Fragments").  A row
    without that fragment (status != 0, ``FRAGMENT_SMILES_STATUS_NAMES``: the canon entries' reasons, or 16 "no_fragment") gets the EMPTY
    row bos, eos, pad..., and out_len 2 -- never a copy.  info = atoms and bonds of the fragment, atoms that became bracket atoms, bond
    orders lost; ``info=False``: not written.  counts: int32 [32].  NOT BRICS, not RECAP: this library's own rule.  One launch
    (mvae_smiles_fragment_smiles_rows)."""
    return _writer_rows("mvae_smiles_fragment_smiles_rows", False, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _FRAGMENT_SMILES_OUT, (out, out_len, status, info), counts, _frag(frag), FRAGMENT_SMILES_COUNTS)


def smiles_fragment_smiles_host(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, frag=0, max_content=127, T_out=None, out=None,
                                out_len=None, status=None, info=None):
    """smiles_fragment_smiles_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_fragment_smiles_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    return _writer_rows("mvae_smiles_fragment_smiles_host", True, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _FRAGMENT_SMILES_OUT, (out, out_len, status, info), None, _frag(frag), FRAGMENT_SMILES_COUNTS)


def smiles_fragment_smiles_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, frag=0, max_content=127, stride=None, tokens_out=None,
                                  offsets_out=None, status=None, info=None, counts=None, err=None):
    """smiles_fragment_smiles_rows over the rows `rows` (int64 [B]) of the CSR corpus, one launch (mvae_smiles_fragment_smiles_corpus):
    (tokens_out uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``, with its err and counts (int32 [32]); a row without that fragment is a slice of length 0."""
    return _writer_corpus("mvae_smiles_fragment_smiles_corpus", tokens, offsets, N, rows, tok_info, chem_info, emit, (), max_content, stride,
                          _FRAGMENT_SMILES_OUT, (tokens_out, offsets_out, status, info), counts, err, _frag(frag), FRAGMENT_SMILES_COUNTS)


SMILES_STATUS_NOT_AROMATIC = 17               # include/mvae.h: MVAE_SMILES_NOT_AROMATIC, given by the aromatize entries only
AROMATIZE_STATUS_NAMES = FRAGMENT_SMILES_STATUS_NAMES + ("not_aromatic",)               # index = status; 14 - 16 are never given here
AROMATIZE_INFO = ("atoms", "aromatic", "raised", "lowered_bonds")   # the columns of info [*, 4] (MVAE_AROMATIZE_INFO)
AROMATIZE_COUNTS = 32                                               # MVAE_AROMATIZE_COUNTS: the per-status histogram has a slot 17
_AROMATIZE_OUT = ((torch.int32, (len(AROMATIZE_INFO),), True), (torch.uint8, (128,), True))        # info, arom


def smiles_aromatize_rows(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None,
                          info=None, arom=None, counts=None):
    """The aromatic normal form of token rows x (int64 [B, T], bos first) on the device: (out int64 [B, T_out], out_len int32 [B], status
    int32 [B], info int32 [B, 4], arom uint8 [B, 128]) -- every row read into its graph, aromaticity perceived on it by this library's
    own rule (include/mvae.h, "Aromatic normal form": candidates by electrons, simple cycles of 5 - 7 atoms with 4 k + 2 of them), and
    the perceived graph written in the spelling of ``smiles_canon_rows``, so that C1=CC=CC=C1 and c1ccccc1 give one row.  A refused row
    (status != 0, ``AROMATIZE_STATUS_NAMES``: the canon entries' reasons, 7 "kekule", or 17 "not_aromatic" for a lower-case atom the
    rule does not find aromatic) is copied through.  info = atoms, aromatic atoms, atoms raised from upper case, double bonds lowered
    (``AROMATIZE_INFO``); arom[k] = 1 / 0 for atom k of the input, 0xFF beyond the atoms and for a refused row; ``info=False`` /
    ``arom=False``: not written (None in its place).  counts: int32 [32].  NOT rdkit's aromaticity model or canonical SMILES; no stereo.
    One launch (mvae_smiles_aromatize_rows)."""
    return _writer_rows("mvae_smiles_aromatize_rows", False, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _AROMATIZE_OUT, (out, out_len, status, info, arom), counts, (), AROMATIZE_COUNTS)


def smiles_aromatize_host(x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None,
                          info=None, arom=None):
    """smiles_aromatize_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_aromatize_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    return _writer_rows("mvae_smiles_aromatize_host", True, x, tok_info, chem_info, emit, bos_id, eos_id, pad_id, (), max_content, T_out,
                        _AROMATIZE_OUT, (out, out_len, status, info, arom), None, (), AROMATIZE_COUNTS)


def smiles_aromatize_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, max_content=127, stride=None, tokens_out=None, offsets_out=None,
                            status=None, info=None, arom=None, counts=None, err=None):
    """smiles_aromatize_rows over the rows `rows` (int64 [B]) of the CSR corpus, one launch (mvae_smiles_aromatize_corpus): (tokens_out
    uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4], arom uint8 [B, 128]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``, with its err and counts (int32 [32]); ``info=False`` / ``arom=False``: not written (None in its place)."""
    return _writer_corpus("mvae_smiles_aromatize_corpus", tokens, offsets, N, rows, tok_info, chem_info, emit, (), max_content, stride,
                          _AROMATIZE_OUT, (tokens_out, offsets_out, status, info, arom), counts, err, (), AROMATIZE_COUNTS)


SELFIES_STATUS_CAPACITY = 18                  # include/mvae.h: MVAE_SELFIES_CAPACITY, given by the SELFIES encode entries only
SELFIES_STATUS_NAMES = AROMATIZE_STATUS_NAMES + ("selfies_capacity",)                   # index = status; 14 - 17 are never given here
SELFIES_DECODE_INFO = ("atoms", "ring_bonds", "reparented", "bad_column")      # the columns of info [*, 4] of the decode entries
SELFIES_ENCODE_INFO = ("atoms", "branch_symbols", "ring_symbols", "capacity_atom")      # ... of the encode entries
SELFIES_COUNTS = 32                                                  # MVAE_SELFIES_COUNTS
SELFIES_EMIT = 529                                                   # MVAE_SELFIES_EMIT
_SELFIES_OUT = ((torch.int32, (4,), True),)


def _selfies_tables(dev, tables, counts, max_content):
    for t, n in tables:
        assert t.dtype == torch.int32 and t.dim() == 1 and (n is None or t.numel() == n) and t.is_contiguous() and t.device == dev, (t.dtype, t.shape)
    if not 1 <= int(max_content) <= 127:
        raise ValueError(f"selfies: max_content must be in [1, 127], got {max_content}")
    assert counts is None or (counts.dtype == torch.int32 and counts.shape == (SELFIES_COUNTS,) and counts.is_contiguous() and counts.device == dev)


def _selfies_rows(name, host, x, front, tables, ids, max_content, T_out, given, counts):
    """What the mvae_selfies_*_rows and _host entries share.  front: the arguments between x_ld and the output ids; tables: (tensor,
    length or None) of every table among them; ids: the output's (bos, eos, pad)."""
    x, ldx = _token_rows(x, "x")
    assert not host or x.device.type == "cpu", x.device
    B, T = x.shape
    _selfies_tables(x.device, tables, counts, max_content)
    T_out = max(T, int(max_content) + 2) if T_out is None else int(T_out)
    res = _outputs(B, x.device, ((torch.int64, (T_out,), False), (torch.int32, (), False), (torch.int32, (), False)) + _SELFIES_OUT, given)
    check(getattr(L.load(), name)(B, T, tables[0][0].numel(), ptr(x), ldx, *front, *map(int, ids), int(max_content), T_out, *map(ptr, res[:3]),
                                  *(() if host else (ptr(counts),)), ptr(res[3]), *(() if host else (stream_ptr(),))), name)
    return res


def _selfies_corpus(name, tokens, offsets, N, rows, front, tables, max_content, stride, given, counts, err):
    """The same for the _corpus entries; given = (tokens_out, offsets_out, status, info)."""
    N, B = int(N), rows.numel()
    dev = tokens.device
    _csr(tokens, offsets, N)
    assert rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous() and rows.device == dev and B >= 1
    _selfies_tables(dev, tables, counts, max_content)
    stride = int(max_content) if stride is None else int(stride)
    offsets_out, = _outputs(2 * B + 1, dev, ((torch.int64, (), False),), given[1:2])
    tokens_out, status, info = _outputs(B, dev, ((torch.uint8, (stride,), False), (torch.int32, (), False)) + _SELFIES_OUT, given[:1] + given[2:])
    assert err is None or (err.dtype == torch.int32 and err.numel() == 1 and err.device == dev)
    check(getattr(L.load(), name)(ptr(tokens), ptr(offsets), N, ptr(rows), B, tables[0][0].numel(), *front, int(max_content), stride,
                                  ptr(tokens_out), ptr(offsets_out), ptr(status), ptr(counts), ptr(err), ptr(info), stream_ptr()), name)
    return tokens_out, offsets_out, status, info


def selfies_decode_rows(x, sinfo, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None, info=None,
                        counts=None):
    """SELFIES token rows x (int64 [B, T], bos first; sinfo = ``vocab.selfies_info_table`` of their vocabulary) decoded on the device to
    SMILES token rows: (out int64 [B, T_out], out_len int32 [B], status int32 [B], info int32 [B, 4]) -- every row derived into a graph by
    this library's own SELFIES rules (include/mvae.h, "SELFIES") and written in the canonical Kekule spelling of ``smiles_canon_rows``
    in the SMILES vocabulary that emit (``vocab.smiles_emit_table``) and bos_id / eos_id / pad_id describe.  status
    (``SELFIES_STATUS_NAMES``): 0, 1 (a token that is no symbol, or no atom), or the writer's 9 - 13; a row that is not written gives
    the EMPTY row, never a copy.  info = ``SELFIES_DECODE_INFO``; ``info=False``: not written.  counts: int32 [32].  NOT the selfies
    package's decoder: agreement with it is neither tested nor claimed.  One launch (mvae_selfies_decode_rows)."""
    return _selfies_rows("mvae_selfies_decode_rows", False, x, (ptr(sinfo), ptr(emit)), ((sinfo, None), (emit, REWRITE_EMIT)),
                         (bos_id, eos_id, pad_id), max_content, T_out, (out, out_len, status, info), counts)


def selfies_decode_host(x, sinfo, emit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None, status=None, info=None):
    """selfies_decode_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows (mvae_selfies_decode_host) --
    for tests and for machines without a device; not a fallback of the device entries."""
    return _selfies_rows("mvae_selfies_decode_host", True, x, (ptr(sinfo), ptr(emit)), ((sinfo, None), (emit, REWRITE_EMIT)),
                         (bos_id, eos_id, pad_id), max_content, T_out, (out, out_len, status, info), None)


def selfies_decode_corpus(tokens, offsets, N, rows, sinfo, emit, max_content=127, stride=None, tokens_out=None, offsets_out=None, status=None,
                          info=None, counts=None, err=None):
    """selfies_decode_rows over the rows `rows` (int64 [B]) of a CSR corpus of SELFIES tokens, one launch (mvae_selfies_decode_corpus):
    (tokens_out uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``; a row id outside [0, N) gives status 1 and err 2."""
    return _selfies_corpus("mvae_selfies_decode_corpus", tokens, offsets, N, rows, (ptr(sinfo), ptr(emit)), ((sinfo, None), (emit, REWRITE_EMIT)),
                           max_content, stride, (tokens_out, offsets_out, status, info), counts, err)


def selfies_encode_rows(x, tok_info, chem_info, emit, eos_in, semit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None,
                        status=None, info=None, counts=None):
    """SMILES token rows x (int64 [B, T], bos first; tok_info, chem_info, emit and eos_in describe their vocabulary) encoded on the device
    to SELFIES token rows: (out, out_len, status, info) -- the atoms in their string order, parentheses as branch symbols with a length,
    the second ring digit as a ring symbol with a distance, bond orders from the matching of ``smiles_kekule_rows`` (include/mvae.h,
    "SELFIES": Encode), in the SELFIES vocabulary that semit (``vocab.selfies_emit_table``) and bos_id / eos_id / pad_id describe.
    status: the walk's 1 - 6, 7 "kekule", 8 "stereo", 12 "long", 13 for a symbol the vocabulary lacks, 18 "selfies_capacity" for an atom
    over the capacity of its symbol; a refused row gives the EMPTY row.  info = ``SELFIES_ENCODE_INFO``.  NOT the selfies package's
    encoder.  One launch (mvae_selfies_encode_rows)."""
    _graph_tables(tok_info, chem_info, x.device)
    return _selfies_rows("mvae_selfies_encode_rows", False, x, (ptr(tok_info), ptr(chem_info), ptr(emit), int(eos_in), ptr(semit)),
                         ((tok_info, None), (chem_info, None), (emit, REWRITE_EMIT), (semit, SELFIES_EMIT)), (bos_id, eos_id, pad_id), max_content,
                         T_out, (out, out_len, status, info), counts)


def selfies_encode_host(x, tok_info, chem_info, emit, eos_in, semit, bos_id, eos_id, pad_id, max_content=127, T_out=None, out=None, out_len=None,
                        status=None, info=None):
    """selfies_encode_rows on HOST tensors (mvae_selfies_encode_host) -- for tests and for machines without a device; not a fallback."""
    _graph_tables(tok_info, chem_info, x.device)
    return _selfies_rows("mvae_selfies_encode_host", True, x, (ptr(tok_info), ptr(chem_info), ptr(emit), int(eos_in), ptr(semit)),
                         ((tok_info, None), (chem_info, None), (emit, REWRITE_EMIT), (semit, SELFIES_EMIT)), (bos_id, eos_id, pad_id), max_content,
                         T_out, (out, out_len, status, info), None)


def selfies_encode_corpus(tokens, offsets, N, rows, tok_info, chem_info, emit, semit, max_content=127, stride=None, tokens_out=None,
                          offsets_out=None, status=None, info=None, counts=None, err=None):
    """selfies_encode_rows over the rows `rows` (int64 [B]) of the CSR corpus of SMILES tokens, one launch (mvae_selfies_encode_corpus):
    (tokens_out uint8 [B, stride], offsets_out int64 [2 B + 1], status int32 [B], info int32 [B, 4]) in the gapped CSR layout of
    ``smiles_rewrite_corpus``; a row id outside [0, N) gives status 1 and err 2."""
    _graph_tables(tok_info, chem_info, tokens.device)
    return _selfies_corpus("mvae_selfies_encode_corpus", tokens, offsets, N, rows, (ptr(tok_info), ptr(chem_info), ptr(emit), ptr(semit)),
                           ((tok_info, None), (chem_info, None), (emit, REWRITE_EMIT), (semit, SELFIES_EMIT)), max_content, stride,
                           (tokens_out, offsets_out, status, info), counts, err)


SUBSTRUCT_QATOMS = 32                         # include/mvae.h: MVAE_SUBSTRUCT_QATOMS, the atoms of a query and the columns of `map`
SUBSTRUCT_QUERIES = 64                        # MVAE_SUBSTRUCT_QUERIES, the queries of one launch: one bit of an int64 each
SUBSTRUCT_WORDS = 100                         # MVAE_SUBSTRUCT_WORDS, the int32 words of one compiled query
SUBSTRUCT_MAX_STEPS = 1 << 20                 # MVAE_SUBSTRUCT_MAX_STEPS, the largest step budget
SUBSTRUCT_STEPS = 1 << 16                     # the budget the Python surface defaults to
SMILES_STATUS_QUERY_ATOMS = 14                # MVAE_SMILES_QUERY_ATOMS: a query of more than 32 atoms (the compile entry alone)
SUBSTRUCT_QSTATUS_NAMES = REWRITE_STATUS_NAMES + ("query_atoms",)


def smiles_substruct_compile(xq, tok_info, chem_info, emit, eos_id, table=None, qstatus=None):
    """Query rows xq (int64 [Q, Tq] on the HOST, bos first, Q <= 64) compiled into the table the substructure entries take: (table int32
    [Q, 100], qstatus int32 [Q]) on the host (mvae_smiles_substruct_compile_host; include/mvae.h, "SMILES substructure").  qstatus 0: a
    query; anything else (``SUBSTRUCT_QSTATUS_NAMES``): refused -- a walk status other than ok / aromatic, a stereo token, more than 32
    atoms -- and its table is a query without atoms, which no row contains.  emit: vocab.smiles_emit_table, for its stereo mask."""
    xq, ldx = _token_rows(xq, "xq")
    assert xq.device.type == "cpu", xq.device
    _graph_tables(tok_info, chem_info, xq.device)
    assert emit.dtype == torch.int32 and emit.shape == (REWRITE_EMIT,) and emit.device == xq.device, (emit.dtype, emit.shape)
    Q = xq.shape[0]
    if Q > SUBSTRUCT_QUERIES:
        raise ValueError(f"smiles_substruct_compile: at most {SUBSTRUCT_QUERIES} queries, got {Q}")
    table, qstatus = _outputs(Q, xq.device, ((torch.int32, (SUBSTRUCT_WORDS,), False), (torch.int32, (), False)), (table, qstatus))
    lo, hi = (int(emit[43 + k]) & 0xFFFFFFFF for k in range(2))
    check(L.load().mvae_smiles_substruct_compile_host(Q, xq.shape[1], tok_info.numel(), ptr(xq), ldx, ptr(tok_info), ptr(chem_info), lo, hi,
                                                      int(eos_id), ptr(table), ptr(qstatus)), "mvae_smiles_substruct_compile_host")
    return table, qstatus


def _substruct_out(Q):
    return ((torch.int32, (), False), (torch.int64, (), False), (torch.int64, (), False), (torch.uint8, (SUBSTRUCT_QATOMS,), True),
            (torch.int32, (Q,), True))


def _substruct_entry(name, front, table, max_steps, map_query, counts, dev):
    """The C entry `name` as _smiles_rows / _smiles_corpus call it: the query arguments go in behind its first `front` arguments and
    counts behind its five per-row outputs."""
    assert table.dtype == torch.int32 and table.dim() == 2 and table.shape[1] == SUBSTRUCT_WORDS and table.is_contiguous() and table.device == dev
    Q = table.shape[0]
    if not 1 <= Q <= SUBSTRUCT_QUERIES:
        raise ValueError(f"smiles_substruct: 1 to {SUBSTRUCT_QUERIES} queries a launch, got {Q}")
    if not 1 <= int(max_steps) <= SUBSTRUCT_MAX_STEPS:
        raise ValueError(f"smiles_substruct: max_steps must be in [1, {SUBSTRUCT_MAX_STEPS}], got {max_steps}")
    if map_query is not None and not 0 <= int(map_query) < Q:
        raise ValueError(f"smiles_substruct: map_query must be in [0, {Q}), got {map_query}")
    assert counts is None or (counts.dtype == torch.int32 and counts.shape == (Q, 2) and counts.is_contiguous() and counts.device == dev)
    fn = getattr(L.load(), name)
    query = (Q, ptr(table), int(max_steps), -1 if map_query is None else int(map_query))

    # front: the arguments of the C entry before Q -- 8 for _rows / _host (B, T, V, x, x_ld, tok_info, chem_info, eos_id), 6 for _corpus
    # (tokens, offsets, N, V, tok_info, chem_info); then come the five outputs of _substruct_out and, on the device, the stream
    n_args = len(L.SIGNATURES[name][1])

    def entry(*a):
        assert len(a) + len(query) + 1 == n_args and len(a) - front in (5, 6), (name, len(a), n_args)
        return fn(*a[:front], *query, *a[front:front + 5], ptr(counts), *a[front + 5:])
    entry.__name__ = name
    return entry, Q


def smiles_substruct_rows(x, tok_info, chem_info, eos_id, table, max_steps=SUBSTRUCT_STEPS, map_query=None, status=None, hit=None,
                          undecided=None, map=None, steps=None, counts=None):
    """Which of the Q compiled queries `table` (int32 [Q, 100], ``smiles_substruct_compile``, on x's device) the token rows x (int64
    [B, T], bos first) contain: (status int32 [B], hit int64 [B], undecided int64 [B], map uint8 [B, 32], steps int32 [B, Q]) -- bit q
    of hit: the row's graph contains query q as a monomorphism on (element, aromatic, charge) and the bond classes (include/mvae.h,
    "SMILES substructure"; NOT SMARTS, not rdkit's HasSubstructMatch); bit q of undecided: the backtracking search used up its
    ``max_steps`` candidates on that (row, query) and says neither.  map: the first (lexicographically smallest) embedding for the one
    query ``map_query``, 0xFF beyond its atoms and where there is no hit; None without a map_query.  ``steps=False``: not written.
    counts (int32 [Q, 2], optional, zeroed by the caller) += the rows that hit / are undecided per query.  Rows of status != 0 hit
    nothing.  One launch (mvae_smiles_substruct_rows), the row's graph built once for all queries."""
    fn, Q = _substruct_entry("mvae_smiles_substruct_rows", 8, table, max_steps, map_query, counts, x.device)
    given = (status, hit, undecided, False if map_query is None else map, steps)
    return _smiles_rows(fn, _substruct_out(Q), x, tok_info, chem_info, eos_id, given)


def smiles_substruct_host(x, tok_info, chem_info, eos_id, table, max_steps=SUBSTRUCT_STEPS, map_query=None, status=None, hit=None,
                          undecided=None, map=None, steps=None, counts=None):
    """smiles_substruct_rows on HOST tensors: the same source compiled for the CPU, a plain loop over the rows
    (mvae_smiles_substruct_host) -- for tests and for machines without a device; not a fallback of the device entries."""
    fn, Q = _substruct_entry("mvae_smiles_substruct_host", 8, table, max_steps, map_query, counts, x.device)
    given = (status, hit, undecided, False if map_query is None else map, steps)
    return _smiles_rows(fn, _substruct_out(Q), x, tok_info, chem_info, eos_id, given, host=True)


def smiles_substruct_corpus(tokens, offsets, N, tok_info, chem_info, table, max_steps=SUBSTRUCT_STEPS, map_query=None, status=None, hit=None,
                            undecided=None, map=None, steps=None, counts=None):
    """smiles_substruct_rows over all N rows of the CSR corpus (tokens uint8, offsets int64 [N + 1]; rows without specials, the end of a
    row acting as <eos>), one launch (mvae_smiles_substruct_corpus)."""
    fn, Q = _substruct_entry("mvae_smiles_substruct_corpus", 6, table, max_steps, map_query, counts, tokens.device)
    given = (status, hit, undecided, False if map_query is None else map, steps)
    return _smiles_corpus(fn, _substruct_out(Q), tokens, offsets, N, tok_info, chem_info, given)


def substruct_bits(words, Q):
    """hit or undecided (int64 [B]) as bool [B, Q]: column q is bit q."""
    return ((words.reshape(-1, 1) >> torch.arange(Q, dtype=torch.int64, device=words.device)) & 1).bool()


def key_histogram(keys, weights=None):
    """The distinct non-zero keys of an int64 tensor, ascending (as signed integers), and how often each occurs -- or, with ``weights``
    (an integer tensor of the same shape), the sum of its weights: (keys int64 [n], counts int64 [n]) on the keys' device.  One
    torch.sort and a segment sum, all integer; the one read-back is the size n of the result."""
    keys = keys.reshape(-1)
    assert keys.dtype == torch.int64, keys.dtype
    w = torch.ones_like(keys) if weights is None else weights.reshape(-1).to(torch.int64)
    assert w.shape == keys.shape and w.device == keys.device
    if keys.numel() == 0:
        return keys.clone(), w.clone()
    ks, order = torch.sort(keys)
    first = torch.ones_like(ks, dtype=torch.bool)
    first[1:] = ks[1:] != ks[:-1]
    run = torch.cumsum(first, 0) - 1
    sums = torch.zeros_like(ks).index_add_(0, run, w[order])[run]
    keep = first & (ks != 0)
    return ks[keep], sums[keep]


def keys_in(sorted_keys, q):
    """bool, q's shape: which elements of q (int64) occur in the ascending int64 tensor sorted_keys.  No host wait."""
    if sorted_keys.numel() == 0:
        return torch.zeros_like(q, dtype=torch.bool)
    pos = torch.searchsorted(sorted_keys, q).clamp_(max=sorted_keys.numel() - 1)
    return sorted_keys[pos] == q


def histogram_cosine(ka, ca, kb, cb):
    """The cosine similarity of two key histograms (what key_histogram returns: distinct ascending keys and int64 counts), as a float64
    0-d tensor on their device: dot / sqrt(|a|^2 |b|^2) with the dot product and the two squared norms exact in int64, one sqrt and one
    division.  NaN if either side is empty.  This is the MOSES Scaf figure when the keys are scaffold keys.  No host wait."""
    for k, c in ((ka, ca), (kb, cb)):
        assert k.dtype == c.dtype == torch.int64 and k.dim() == 1 and k.shape == c.shape and k.device == ka.device
    if ka.numel() == 0 or kb.numel() == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=ka.device)
    pos = torch.searchsorted(kb, ka).clamp_(max=kb.numel() - 1)
    dot = (ca * torch.where(kb[pos] == ka, cb[pos], torch.zeros_like(ca))).sum()
    na, nb = (ca * ca).sum(), (cb * cb).sum()
    return dot.double() / torch.sqrt(na.double() * nb.double())


def scaffold_split_rows(scaffold_key, test_fraction, seed=0):
    """(train_rows, test_rows), int64 ascending on the keys' device, of rows with the given scaffold keys (int64 [N], 0 = no scaffold):
    whole scaffolds go to the test side, in an order drawn from ``seed`` (a CPU generator: the same split on every device), until at
    least ``test_fraction`` of the rows with a non-zero key are there; rows with key 0 stay in train.  No non-zero key occurs on both
    sides.  Deterministic."""
    if not 0.0 <= float(test_fraction) <= 1.0:
        raise ValueError(f"scaffold_split: test_fraction must be in [0, 1], got {test_fraction!r}")
    assert scaffold_key.dtype == torch.int64 and scaffold_key.dim() == 1
    dev = scaffold_key.device
    ks, cs = key_histogram(scaffold_key)
    in_test = torch.zeros(scaffold_key.shape[0], dtype=torch.bool, device=dev)
    if ks.numel():
        order = torch.randperm(ks.numel(), generator=torch.Generator().manual_seed(int(seed))).to(dev)
        c = cs[order]
        before = torch.cumsum(c, 0) - c                            # rows already on the test side when this scaffold's turn comes
        total = cs.sum()
        # a scaffold is taken while fewer than test_fraction * total rows are there (float64: the counts are far below 2^53)
        taken = before.double() < float(test_fraction) * total.double()
        key_in_test = torch.zeros(ks.numel(), dtype=torch.bool, device=dev)
        key_in_test[order] = taken
        pos = torch.searchsorted(ks, scaffold_key).clamp_(max=ks.numel() - 1)
        in_test = (ks[pos] == scaffold_key) & key_in_test[pos]
    rows = torch.arange(scaffold_key.shape[0], dtype=torch.int64, device=dev)
    return rows[~in_test], rows[in_test]


def sample_uniform(seed, step, B):
    """Host restatement of the sampling step's uniforms u(b) = hash(seed, step * B + b) / 2^32 (tests)."""
    import numpy as np
    idx = (np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    h = ((idx * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(seed & 0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.float64) / 4294967296.0


def moses_latent_fwd(mu, logvar, eps, z, kl, B, dz, seed=0, offset=0, eps_out=None):
    """eps None: the noise is drawn inside the launch from the counter hash of (seed, offset + i) and written to eps_out."""
    lib = L.load()
    need = lib.mvae_moses_latent_workspace(B)
    ws = Scratch.get(need, mu.device)
    check(lib.mvae_moses_latent_fwd(B, dz, ptr(mu), ptr(logvar), ptr(eps), int(seed) & 0xFFFFFFFF, int(offset), ptr(eps_out), ptr(z), ptr(kl),
                                    ptr(ws), need, stream_ptr()), "mvae_moses_latent_fwd")


def moses_latent_bwd(mu, logvar, eps, dz_in, dkl, dlogvar_ext, dmu, dlogvar, B, dz):
    check(L.load().mvae_moses_latent_bwd(B, dz, ptr(mu), ptr(logvar), ptr(eps), ptr(dz_in), ptr(dkl), ptr(dlogvar_ext), ptr(dmu), ptr(dlogvar),
                                         stream_ptr()), "mvae_moses_latent_bwd")


def moses_latent_fb_fwd(mu, logvar, eps, z, kl2, kl_dim, B, dz, free_bits, seed=0, offset=0, eps_out=None):
    """moses_latent_fwd with free bits: kl_dim [dz] = the per-dimension batch-mean KL m_j, kl2[0] = sum_j max(m_j, free_bits) (the
    objective), kl2[1] = sum_j m_j (the KL); z / eps_out bitwise as moses_latent_fwd writes them (mvae_moses_latent_fb_fwd)."""
    lib = L.load()
    need = lib.mvae_moses_latent_fb_workspace(B, dz)
    ws = Scratch.get(need, mu.device)
    check(lib.mvae_moses_latent_fb_fwd(B, dz, ptr(mu), ptr(logvar), ptr(eps), int(seed) & 0xFFFFFFFF, int(offset), ptr(eps_out), float(free_bits),
                                       ptr(z), ptr(kl2), ptr(kl_dim), ptr(ws), need, stream_ptr()), "mvae_moses_latent_fb_fwd")


def moses_latent_fb_bwd(mu, logvar, eps, dz_in, dkl, dlogvar_ext, kl_dim, free_bits, dmu, dlogvar, B, dz):
    """moses_latent_bwd with the KL term of dimension j switched by kl_dim[j] >= free_bits (mvae_moses_latent_fb_bwd)."""
    check(L.load().mvae_moses_latent_fb_bwd(B, dz, ptr(mu), ptr(logvar), ptr(eps), ptr(dz_in), ptr(dkl), ptr(dlogvar_ext), ptr(kl_dim),
                                            float(free_bits), ptr(dmu), ptr(dlogvar), stream_ptr()), "mvae_moses_latent_fb_bwd")


def token_dropout(x, lengths, x_out, B, T, unk_id, p, seed=0, keep_mask=None, n_dropped=None):
    """Word dropout: x_out[b, t] = unk_id at the eligible positions (1 <= t <= lengths[b] - 2) that are not kept, x[b, t] elsewhere.  Kept =
    keep_mask [B, T] bytes when given, else the counter hash at b * T + t -- dropout_keep_mask(seed, (B, T), p) restates it on the host.
    n_dropped (int32 [1], optional) receives the number of replaced positions (mvae_token_dropout)."""
    check(L.load().mvae_token_dropout(ptr(x), ptr(lengths), B, T, int(unk_id), float(p), int(seed) & 0xFFFFFFFF, ptr(keep_mask), ptr(x_out),
                                      ptr(n_dropped), stream_ptr()), "mvae_token_dropout")


def ce_loss_fwd(logits, ldl, x, pad, loss2, B, T, V):
    lib = L.load()
    need = lib.mvae_ce_loss_workspace(B, T)
    ws = Scratch.get(need, logits.device)
    check(lib.mvae_ce_loss_fwd(B, T, V, ptr(logits), ldl, ptr(x), pad, ptr(loss2), ptr(ws), need, stream_ptr()), "mvae_ce_loss_fwd")


def ce_loss_bwd(logits, ldl, x, pad, loss2, grad_out, dy_ext, dl, B, T, V):
    check(L.load().mvae_ce_loss_bwd(dt_code(dl.dtype), B, T, V, ptr(logits), ldl, ptr(x), pad, ptr(loss2), ptr(grad_out), ptr(dy_ext), ptr(dl),
                                    dl.stride(0), stream_ptr()), "mvae_ce_loss_bwd")


def scatter_rows_tb(idx, d, dtable, B, Lq, nrows, W, ldd=None):
    lib = L.load()
    need = lib.mvae_scatter_rows_tb_workspace(B, Lq, nrows, W)
    ws = Scratch.get(need, d.device)
    check(lib.mvae_scatter_rows_tb(dt_code(d.dtype), ptr(idx), B, Lq, nrows, ptr(d), W if ldd is None else ldd, W, ptr(dtable), ptr(ws), need,
                                   stream_ptr()), "mvae_scatter_rows_tb")


def rowsum(X, R, C_, out, ldx=None, accumulate=False):
    check(L.load().mvae_rowsum(dt_code(X.dtype), R, C_, ptr(X), X.stride(0) if ldx is None else ldx, ptr(out),
                               1 if accumulate else 0, stream_ptr()), "mvae_rowsum")


def timesum(X, T, B, W, out):
    check(L.load().mvae_timesum(dt_code(X.dtype), T, B, W, ptr(X), ptr(out), stream_ptr()), "mvae_timesum")


def colsum(X, M, N, out, ldx=None):
    lib = L.load()
    need = lib.mvae_colsum_workspace(M, N)
    ws = Scratch.get(need, X.device)
    check(lib.mvae_colsum(M, N, ptr(X), X.stride(0) if ldx is None else ldx, ptr(out), ptr(ws), need, stream_ptr()), "mvae_colsum")


def selu_bwd(dy, y):
    check(L.load().mvae_selu_bwd(dy.numel(), ptr(dy), ptr(y), stream_ptr()), "mvae_selu_bwd")


def conv1d_pack_weights(w, Cin, Cout, k, ldx, wp, ldo=0, wq=None):
    """wp[o][j*ldx + c] = w[o][c][j];  wq[c][j*ldo + o] = w[o][c][k-1-j]  (pads zero)."""
    check(L.load().mvae_conv1d_pack_weights(Cin, Cout, k, ptr(w), ldx, ptr(wp), ldo, ptr(wq), stream_ptr()), "mvae_conv1d_pack_weights")


def conv1d_selu_fwd(x, B, W, ldx, x_bs, Cout, k, wp, bias, y, ldy, act=L.ACT_SELU):
    """Channels-last sliding-window conv + bias + activation: x[b, w, c] at b*x_bs + w*ldx + c (pad channels zero) -> y[(b*Wout + w), o] (ldy)."""
    lib = L.load()
    need = lib.mvae_conv1d_selu_fwd_workspace(B, W, ldx, Cout, k)
    ws = Scratch.get(need, x.device) if need else None
    check(lib.mvae_conv1d_act_fwd(act, B, W, ldx, x_bs, Cout, k, ptr(x), ptr(wp), ptr(bias), ptr(y), ldy, ptr(ws), need, stream_ptr()),
          "mvae_conv1d_act_fwd")


def conv1d_selu_bwd(B, W, Cin, ldx, x_bs, Cout, ldo, k, dy, y, x, wq, dzp, dw, db, dx, lddx, act=L.ACT_SELU, x3=False):
    """x3: the input-gradient GEMM multiplies its fp32 operands as 3 x bf16 products (MVAE_CONV_BWD_X3: gradients of the bf16 training mode).
    dw None: only dzp and dx are produced (the weight gradient joins a TnF32Batch: add_conv_dw)."""
    lib = L.load()
    if x3:
        act = act | L.CONV_BWD_X3
    need = lib.mvae_conv1d_selu_bwd_workspace(B, W, Cin, ldx, Cout, ldo, k)
    ws = Scratch.get(need, dy.device)
    check(lib.mvae_conv1d_act_bwd(act, B, W, Cin, ldx, x_bs, Cout, ldo, k, ptr(dy), ptr(y), ptr(x), ptr(wq), ptr(dzp), ptr(dw), ptr(db),
                                  ptr(dx), lddx, ptr(ws), need, stream_ptr()), "mvae_conv1d_act_bwd")


def lambda_fwd(mulv, eps, z, mu, logvar, B, o, scale=1.0, seed=0, offset=0, eps_out=None):
    """eps None: eps_out[i] = scale * n(seed, offset + i) is drawn inside the launch (the draw of models.py:92 as part of the op)."""
    check(L.load().mvae_lambda_fwd(B, o, ptr(mulv), ptr(eps), float(scale), int(seed) & 0xFFFFFFFF, int(offset), ptr(eps_out), ptr(z), ptr(mu),
                                   ptr(logvar), stream_ptr()), "mvae_lambda_fwd")


def normal_fill(out, scale, seed, offset):
    """out.flat[i] = scale * n(seed, offset + i): the library's counter-hash normal (randn_like without generator state)."""
    assert out.dtype == torch.float32 and out.is_contiguous()
    check(L.load().mvae_normal_fill(out.numel(), float(scale), int(seed) & 0xFFFFFFFF, int(offset), ptr(out), stream_ptr()), "mvae_normal_fill")
    return out


def normal_draw(seed, offset, n, scale=1.0):
    """Host restatement (numpy, float64) of the n normals the kernels draw for counters offset .. offset + n - 1 of stream `seed`
    (include/mvae.h: mvae_lambda_fwd).  The hash words are bit-exact (tests hold them to mvae_normal_words); the transform is in double."""
    import numpy as np
    M = np.uint64(0xFFFFFFFF)

    def H(seed_, idx):
        h = ((idx * np.uint64(0x9E3779B1)) & M) ^ seed_
        h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & M
        h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & M
        h ^= h >> np.uint64(16)
        return h
    c = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    s = H(np.uint64(seed & 0xFFFFFFFF), (c >> np.uint64(31)) ^ np.uint64(0x6A09E667))
    lo = (c << np.uint64(1)) & M
    w1 = H(s, lo)
    w2 = H(s ^ np.uint64(0xBB67AE85), lo | np.uint64(1))
    u1 = ((w1 >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = (w2 >> np.uint64(8)).astype(np.float64) / 16777216.0
    return scale * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), w1.astype(np.uint32), w2.astype(np.uint32)


class NoiseStream:
    """One device-side normal stream: an explicit 32-bit seed and a running 64-bit element counter -- all the state there is (picklable; a
    checkpoint may carry `state()`).  take(n) hands out the (seed, offset) of the next n elements.  The default seed comes from
    torch.initial_seed() (so torch.manual_seed makes a run reproducible), the rank of the default process group (ranks draw different noise
    for their shards) and a per-process instance number (two models in one process draw different streams)."""
    _instances = [0]

    def __init__(self, seed=None):
        self.seed, self.counter = seed, 0

    def _default_seed(self):
        import torch.distributed as dist
        try:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        except (ValueError, RuntimeError):        # no default process group after all
            rank = 0
        NoiseStream._instances[0] += 1
        words = (C.c_uint32 * 2)()
        L.load().mvae_normal_words(torch.initial_seed() & 0xFFFFFFFF, (rank << 20) + NoiseStream._instances[0], words)
        return int(words[0])

    def reseed(self, seed, counter=0):
        self.seed, self.counter = int(seed) & 0xFFFFFFFF, int(counter)

    def take(self, n):
        if self.seed is None:
            self.seed = self._default_seed()
        off = self.counter
        self.counter += int(n)
        return self.seed, off

    def state(self):
        return dict(seed=self.seed, counter=self.counter)


def lambda_bwd(mulv, eps, dz, dmu, dlogvar, dmulv, B, o):
    check(L.load().mvae_lambda_bwd(B, o, ptr(mulv), ptr(eps), ptr(dz), ptr(dmu), ptr(dlogvar), ptr(dmulv), stream_ptr()),
          "mvae_lambda_bwd")


def softmax_tb_fwd(logits, ldl, recon, B, Lq, C_):
    check(L.load().mvae_softmax_tb_fwd(B, Lq, C_, ptr(logits), ldl, ptr(recon), stream_ptr()), "mvae_softmax_tb_fwd")


def softmax_tb_bwd(recon, drecon, dl, dlT, B, Lq, C_):
    check(L.load().mvae_softmax_tb_bwd(dt_code(dl.dtype), B, Lq, C_, ptr(recon), ptr(drecon), ptr(dl), dl.stride(0),
                                       ptr(dlT), dlT.stride(0) if dlT is not None else 0, stream_ptr()), "mvae_softmax_tb_bwd")


def bce_kl_loss_fwd(recon, target, mu, logvar, max_len, out3):
    lib = L.load()
    need = lib.mvae_bce_kl_loss_workspace(recon.numel(), mu.numel())
    ws = Scratch.get(need, recon.device, tag="bce_kl_ticket", zeroed=True)     # the kernel's ticket counter lives in its last 16 bytes
    check(lib.mvae_bce_kl_loss_fwd(recon.numel(), ptr(recon), ptr(target), mu.numel(), ptr(mu), ptr(logvar), float(max_len),
                                   ptr(out3), ptr(ws), need, stream_ptr()), "mvae_bce_kl_loss_fwd")


def bce_kl_loss_bwd(recon, target, mu, logvar, max_len, grad_out, drecon, dmu, dlogvar):
    check(L.load().mvae_bce_kl_loss_bwd(recon.numel(), ptr(recon), ptr(target), mu.numel(), ptr(mu), ptr(logvar), float(max_len),
                                        ptr(grad_out), ptr(drecon), ptr(dmu), ptr(dlogvar), stream_ptr()), "mvae_bce_kl_loss_bwd")


def bce_kl_logits_fwd(logits, ldl, idx, mu, logvar, max_len, out3, B, Lq, C_, pred_out=None):
    """ELBO from time-major logits and int64 index targets (mvae_bce_kl_logits_fwd); pred_out: optional int64 [B, Lq] arg-max."""
    lib = L.load()
    need = lib.mvae_bce_kl_logits_workspace(B, Lq)
    ws = Scratch.get(need, logits.device, tag="elbo_ticket", zeroed=True)        # the kernel's ticket counter lives in its last 16 bytes
    check(lib.mvae_bce_kl_logits_fwd(B, Lq, C_, ptr(logits), ldl, ptr(idx), mu.numel(), ptr(mu), ptr(logvar), float(max_len), ptr(out3),
                                     ptr(pred_out), ptr(ws), need, stream_ptr()), "mvae_bce_kl_logits_fwd")


def bce_kl_logits_bwd(logits, ldl, idx, mu, logvar, max_len, grad_out, dl, dlT, dmu, dlogvar, B, Lq, C_):
    check(L.load().mvae_bce_kl_logits_bwd(dt_code(dl.dtype), B, Lq, C_, ptr(logits), ldl, ptr(idx), mu.numel(), ptr(mu), ptr(logvar),
                                          float(max_len), ptr(grad_out), ptr(dl), dl.stride(0), ptr(dlT),
                                          dlT.stride(0) if dlT is not None else 0, ptr(dmu), ptr(dlogvar), stream_ptr()),
          "mvae_bce_kl_logits_bwd")


def _fill(arr, tensors):
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None


def dropout_keep_mask(seed, shape_lt_b_h, p):
    """Host restatement of the device-generated inter-layer dropout mask (mvae_dropout_keep): uint8 [layers-1... as given][T][B][H], element
    index = flat position.  Used by the tests / the oracle to draw exactly what the kernels draw."""
    import numpy as np
    n = int(np.prod(shape_lt_b_h))
    idx = np.arange(n, dtype=np.uint64)
    h = ((idx * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(seed & 0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    return (h >= thresh).astype(np.uint8).reshape(shape_lt_b_h)


# Schedules with BOUNDED SPINS: the weights-resident dataflow passes of the decoder LSTM (rnn_persist*.hip; the per-rank shape of the 8-GPU
# configuration: 4 x 1024, b = 128 / 256, bf16) and the layer-concurrent row-resident encoder passes (rnn_rowres.hip).  Such a launch cannot hang,
# but it can GIVE UP (a workgroup not resident because something else held a compute unit): it then leaves a status record -- the library says
# where (status_out of mvae_rnn_fwd / mvae_rnn_bwd) -- and, when the caller passed a `poison` slot, a NaN there.  Two ways to survive that:
#   * poison given (a training step under FusedAdam): nothing waits.  The NaN sits in the spare slot behind the flat gradient buffer, so the
#     optimiser kernel skips the whole update of that step on the device (in data parallel the slot is all-reduced with the gradient: every rank
#     skips together); the status record is copied to pinned memory behind the launch and looked at later (persist_check).
#   * no poison (evaluation, plain torch optimisers): the call waits for its status record and, on a failure, runs the pass again on the
#     schedule without spins -- same buffers, every one of them is written as a whole by either schedule.
# Either way the failure is counted and reported once (warning); after PERSIST_MAX_FAILURES of them the spinning schedules are switched off
# for the rest of the process (`no_spin` in the descriptors).  PERSIST_DEFAULT: "1" = use them wherever the library serves the shape.
PERSIST_DEFAULT = "1"
PERSIST_MAX_FAILURES = 3
PERSIST_STATS = {"launches": 0, "rowres_pipe": 0, "bwd_launches": 0, "failures": 0, "reruns": 0, "disabled": False}     # passes that took a spinning schedule; what went wrong (tests / logs / bench line)
_PERSIST_PENDING = []      # [(pinned int32[4], event, what)]
_PERSIST_WARNED = [False]
PERSIST_LAST_FAILURE = [None]     # (what, [code, block, layer, 0]) of the latest launch that gave up


def _spin_failure(what, rec):
    PERSIST_STATS["failures"] += 1
    PERSIST_LAST_FAILURE[0] = (what, list(rec))
    if PERSIST_STATS["failures"] >= PERSIST_MAX_FAILURES and not PERSIST_STATS["disabled"]:
        PERSIST_STATS["disabled"] = True
    if not _PERSIST_WARNED[0] or PERSIST_STATS["disabled"]:
        import warnings
        warnings.warn(f"mvae: {what}: a launch with bounded spins gave up waiting for a hand-off (status {list(rec)}: code, block, layer) -- not "
                      "all of its workgroups were resident (another kernel held compute units).  Its outputs were discarded (training: the "
                      "optimiser skipped that step on the device; otherwise the pass was run again on the schedule without spins)."
                      + (f"  {PERSIST_STATS['failures']} such failures: these schedules are now off for this process." if PERSIST_STATS["disabled"] else ""),
                      RuntimeWarning, stacklevel=3)
        _PERSIST_WARNED[0] = True


def persist_check(sync=False):
    """Look at the status records that have arrived (sync: wait for all of them); a failed hand-off is counted and warned about (see above) --
    nothing is raised: the device has already kept the garbage out of the weights.  Returns the number of failures found by this call."""
    keep, found = [], 0
    for host, ev, what in _PERSIST_PENDING:
        if sync:
            ev.synchronize()
        if not ev.query():
            keep.append((host, ev, what))
            continue
        if int(host[0]) != 0:
            found += 1
            _spin_failure(what, host.tolist())
    _PERSIST_PENDING[:] = keep
    return found


_STATUS_RING = {"buf": None, "n": 0}


def _status_slot():
    """One int32[4] slot of a pinned ring allocated ONCE (a fresh pinned allocation per launch is a hipHostMalloc per launch, and that call
    waits for the device: with a 1.4 ms persistent kernel in flight it kept the host from enqueueing the launches behind it).  512 slots:
    persist_check() retires completed records at every call, so a slot is long done when the ring comes round."""
    r = _STATUS_RING
    if r["buf"] is None:
        r["buf"] = torch.zeros(512, 4, dtype=torch.int32).pin_memory()
    r["n"] += 1
    return r["buf"][r["n"] % 512]


def _status_view(addr, bufs):
    """int32[4] view of the status record at device address `addr`, which lies inside one of the scratch tensors `bufs`."""
    for b in bufs:
        if b is not None and b.data_ptr() <= addr and addr + 16 <= b.data_ptr() + b.numel() * b.element_size():
            off = addr - b.data_ptr()
            return b.view(torch.uint8)[off:off + 16].view(torch.int32)
    raise L.MvaeError("mvae_rnn_*: the status record the library reported lies outside the scratch buffers of the call")


def _after_spin_launch(what, addr, bufs, poison, rerun):
    """A launch with bounded spins was enqueued; its status record is at `addr`.  poison given: asynchronous bookkeeping only.  Otherwise wait
    for the record and run `rerun()` (the same pass with no_spin set) if the launch gave up."""
    rec = _status_view(addr, bufs)
    host = _status_slot()
    host.copy_(rec, non_blocking=True)
    ev = torch.cuda.Event(); ev.record()
    if poison is not None:
        _PERSIST_PENDING.append((host, ev, what))
        if len(_PERSIST_PENDING) > 64:
            persist_check()
        return
    ev.synchronize()
    if int(host[0]) != 0:
        _spin_failure(what, host.tolist())
        PERSIST_STATS["reruns"] += 1
        rerun()


def rnn_fwd(cell, dtype, T, B, H, add0, add0_tstride, w_ih, ldw_ih, w_hh, ldw_hh, bias, hs, ldh, cs, gates, cstate,
            x0=None, x0_ld=0, in0=0, h0=None, ldh0=0, lengths=None, zero_padded_k=False, tag=None,
            hdrop=None, drop_mask=None, drop_p=0.0, drop_seed=0, add_table=None, add_index=None, persist=None, poison=None):
    """add_table [rows, G*H] fp32 + add_index [B, L >= T] int64: layer 0 adds table row add_index[b, t] in its epilogue (no gathered copy).
    persist: True / False / None (= PERSIST_DEFAULT): the schedules with bounded spins (weights-resident dataflow pass / layer-concurrent
    row-resident pass) where the library serves the shape.  poison: the optimiser's poison slot (see the note above PERSIST_DEFAULT); None:
    the call verifies such a launch itself and re-runs the pass on a failure."""
    d = L.RnnFwdDesc()
    NL = len(w_hh)
    d.cell, d.dtype, d.layers, d.T, d.B, d.H, d.in0 = cell, dt_code(dtype), NL, T, B, H, in0
    d.x0 = x0.data_ptr() if x0 is not None else None
    d.x0_ld = x0_ld
    d.add0 = add0.data_ptr() if add0 is not None else None
    d.add0_tstride = add0_tstride
    if add_table is not None:
        assert add_table.dtype == torch.float32 and add_table.is_contiguous() and add_table.shape[1] == 4 * H
        assert add_index.dtype == torch.int64 and add_index.stride(1) == 1
        d.add_table, d.add_index = add_table.data_ptr(), add_index.data_ptr()
        d.add_index_ld, d.add_table_rows = add_index.stride(0), add_table.shape[0]
    _fill(d.w_ih, w_ih); _fill(d.w_hh, w_hh); _fill(d.bias, bias)
    for i in range(NL):
        d.ldw_ih[i] = ldw_ih[i]
        d.ldw_hh[i] = ldw_hh[i]
    if h0 is not None:
        _fill(d.h0, h0)
    d.ldh0 = ldh0
    d.lengths = lengths.data_ptr() if lengths is not None else None
    _fill(d.hs, hs); d.ldh = ldh
    if cs is not None:
        _fill(d.cs, cs)
    if gates is not None:
        _fill(d.gates, gates)
    if cstate is not None:
        _fill(d.cstate, cstate)
    d.zero_padded_k = 1 if zero_padded_k else 0
    if hdrop is not None:
        _fill(d.hdrop, hdrop)
        if drop_mask is not None:
            _fill(d.drop_mask, drop_mask)
        d.drop_p, d.drop_seed = float(drop_p), int(drop_seed) & 0xFFFFFFFF
    use_p = ((PERSIST_DEFAULT != "0") if persist is None else bool(persist)) and not PERSIST_STATS["disabled"]
    pws = None
    if use_p:
        persist_check()
        need = L.load().mvae_rnn_fwd_persist_workspace(C.byref(d))
        if need:
            pws = Scratch.get(need, hs[0].device, tag="rnn_persist")
            d.persist_ws, d.persist_ws_bytes = pws.data_ptr(), need
        elif persist:
            raise L.MvaeError("rnn_fwd(persist=True): this shape / device is not served by the persistent schedule")
    d.no_spin = 0 if use_p else 1
    d.poison = poison.data_ptr() if poison is not None else None
    status = C.c_void_p()
    with _Timed(tag):
        check(L.load().mvae_rnn_fwd(C.byref(d), stream_ptr(), C.byref(status)), "mvae_rnn_fwd")
    if status.value:                 # the library took a schedule with bounded spins and says where its status record is
        PERSIST_STATS["launches" if dtype == torch.bfloat16 else "rowres_pipe"] += 1

        def rerun():
            d.no_spin, d.poison = 1, None
            check(L.load().mvae_rnn_fwd(C.byref(d), stream_ptr(), None), "mvae_rnn_fwd (again, without spins)")
        _after_spin_launch(tag or "mvae_rnn_fwd", status.value, (pws,), poison, rerun)


def rnn_bwd_persist_wanted(cell, dtype, NL, B, H, ldg, device):
    """Would rnn_bwd take the weights-resident dataflow schedule for this shape if it is given the output gradient as `dy`?  (The library has
    the last word -- mvae_rnn_bwd_persist_workspace -- this only lets the caller choose the gradient's form; a wrong guess costs speed, not
    correctness.)"""
    if L.knob("MVAE_PERSIST_BWD", PERSIST_DEFAULT) == "0" or PERSIST_STATS["disabled"]:
        return False
    if cell != L.CELL_LSTM or dtype != torch.bfloat16 or NL != 4 or H != 1024 or B not in (128, 256) or ldg != 4 * H + 64:
        return False
    return torch.cuda.get_device_properties(device).multi_processor_count == 256


def rnn_bwd(cell, dtype, T, B, H, w_hhT, ldw_hhT, w_ihT, ldw_ihT, dy, dy_ld, hs, ldh, cs, gates, dG, dstate,
            ldg=None, h0=None, ldh0=0, lengths=None, dh_last=None, dGh=None, dh0=None, tag=None,
            drop_mask=None, drop_p=0.0, drop_seed=0, dy_a=None, dy_w=None, dy_k=0, persist=None, poison=None):
    """dy_a [T*B, ld] / dy_w [H, ld] (dtype, zero-padded to dy_k columns): the output gradient as a product dy = dy_a . dy_w^T, contracted
    by the top layer's cell itself (no [T, B, H] fp32 dy tensor).
    dGh: reserved and ignored -- it fills mvae_rnn_bwd_desc.dGh, which no kernel reads or writes (the GRU's W_hh-side gradient rows are the
    slots r, z, n*r of dG); do not pass it.
    persist: True / False / None (= PERSIST_DEFAULT): the weights-resident dataflow backward where the library serves the shape (it wants the
    output gradient as `dy`, see rnn_bwd_persist_served), and the layer-concurrent row-resident form of the narrow f32 stacks.  poison: as in
    rnn_fwd."""
    d = L.RnnBwdDesc()
    NL = len(w_hhT)
    d.cell, d.dtype, d.layers, d.T, d.B, d.H = cell, dt_code(dtype), NL, T, B, H
    _fill(d.w_hhT, w_hhT); _fill(d.w_ihT, w_ihT)
    for i in range(NL):
        d.ldw_hhT[i] = ldw_hhT[i]
        d.ldw_ihT[i] = ldw_ihT[i]
    d.lengths = lengths.data_ptr() if lengths is not None else None
    d.dy = dy.data_ptr() if dy is not None else None
    d.dy_ld = dy_ld
    if dy_a is not None:
        d.dy_a, d.dy_a_ld, d.dy_w, d.dy_w_ld, d.dy_k = dy_a.data_ptr(), dy_a.stride(0), dy_w.data_ptr(), dy_w.stride(0), dy_k
    if dh_last is not None:
        _fill(d.dh_last, dh_last)
    _fill(d.hs, hs); d.ldh = ldh
    if h0 is not None:
        _fill(d.h0, h0)
    d.ldh0 = ldh0
    if cs is not None:
        _fill(d.cs, cs)
    _fill(d.gates, gates); _fill(d.dG, dG)
    d.ldg = ldg if ldg is not None else {"LSTM": 4, "GRU": 3}["LSTM" if cell == L.CELL_LSTM else "GRU"] * H
    if dGh is not None:
        _fill(d.dGh, dGh)
    _fill(d.dstate, dstate)
    if dh0 is not None:
        _fill(d.dh0, dh0)
    if drop_p > 0.0:
        if drop_mask is not None:
            _fill(d.drop_mask, drop_mask)
        d.drop_p, d.drop_seed = float(drop_p), int(drop_seed) & 0xFFFFFFFF
    need = L.load().mvae_rnn_bwd_workspace(C.byref(d))     # scratch of the split-K schedules (used only when the shape qualifies)
    sws = Scratch.get(need, dy.device if dy is not None else dG[0].device, tag="rnn_split")
    d.split_ws, d.split_ws_bytes = sws.data_ptr(), need
    use_p = ((L.knob("MVAE_PERSIST_BWD", PERSIST_DEFAULT) != "0") if persist is None else bool(persist)) and not PERSIST_STATS["disabled"]
    pws = None
    if use_p:
        pneed = L.load().mvae_rnn_bwd_persist_workspace(C.byref(d))
        if pneed:
            persist_check()
            pws = Scratch.get(pneed, dG[0].device, tag="rnn_persist_bwd")
            d.persist_ws, d.persist_ws_bytes = pws.data_ptr(), pneed
        elif persist:
            raise L.MvaeError("rnn_bwd(persist=True): this shape / device / gradient form is not served by the persistent schedule")
    d.no_spin = 0 if use_p else 1
    d.poison = poison.data_ptr() if poison is not None else None
    status = C.c_void_p()
    with _Timed(tag):
        check(L.load().mvae_rnn_bwd(C.byref(d), stream_ptr(), C.byref(status)), "mvae_rnn_bwd")
    if status.value:                 # which schedule ran is the library's knowledge: it reports the status record of a launch with bounded spins
        if pws is not None and pws.data_ptr() <= status.value < pws.data_ptr() + pws.numel():
            PERSIST_STATS["bwd_launches"] += 1
        else:
            PERSIST_STATS["rowres_pipe"] += 1

        def rerun():
            d.no_spin, d.poison = 1, None
            check(L.load().mvae_rnn_bwd(C.byref(d), stream_ptr(), None), "mvae_rnn_bwd (again, without spins)")
        _after_spin_launch(tag or "mvae_rnn_bwd", status.value, (pws, sws), poison, rerun)


def sumsq(g, partial):
    check(L.load().mvae_sumsq(g.numel(), ptr(g), ptr(partial), stream_ptr()), "mvae_sumsq")


def clip_adam(p, g, m, v, partial, grad_scale, max_norm, lr, b1, b2, eps, step, norm_out, poison_reset=None):
    """norm_out [>= 1]: [0] = the pre-clip norm; [1] (when present) counts the steps the kernel skipped because the norm was not finite.
    poison_reset: the poison slot, set back to zero by the launch."""
    check(L.load().mvae_clip_adam(p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(partial), partial.numel(), float(grad_scale),
                                  float(max_norm), float(lr), float(b1), float(b2), float(eps), int(step), ptr(norm_out), norm_out.numel(),
                                  ptr(poison_reset), stream_ptr()), "mvae_clip_adam")


def clip_sgd(p, g, buf, partial, grad_scale, max_norm, lr, momentum, dampening, weight_decay, nesterov, initialised, parity, norm_out=None,
             poison_reset=None):
    """torch.optim.SGD.step() behind the global-norm clip (mvae_clip_sgd).  buf / initialised (int32 [2]) are used only with momentum != 0;
    parity: the host step's parity (which word of `initialised` this launch reads).  norm_out / poison_reset as in clip_adam."""
    check(L.load().mvae_clip_sgd(p.numel(), ptr(p), ptr(g), ptr(buf), ptr(partial), partial.numel(), float(grad_scale), float(max_norm),
                                 float(lr), float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), ptr(initialised),
                                 int(parity), ptr(norm_out), norm_out.numel() if norm_out is not None else 0, ptr(poison_reset), stream_ptr()),
          "mvae_clip_sgd")
