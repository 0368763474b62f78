"""Thin host wrappers over the C ABI: torch tensors in, torch tensors out, on the caller's HIP
stream.  PyTorch is only the allocator / stream provider here; all arithmetic is in libbcbf."""
import ctypes
import math

import os

import torch

from . import _lib
from ._lib import lib, check

_SUF = {torch.float32: "_f32", torch.float64: "_f64"}


def _suf(t):
    try:
        return _SUF[t.dtype]
    except KeyError:
        raise TypeError("libbcbf supports float32 / float64 tensors, got %s" % t.dtype)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(*ts):
    ref = ts[0]
    if not ref.is_cuda:
        raise RuntimeError("libbcbf kernels need ROCm device tensors (got a CPU tensor); there is no CPU path")
    for t in ts:
        if t is None:
            continue
        if t.device != ref.device:
            raise RuntimeError("all tensors must live on the same device")
        if t.dtype not in (ref.dtype, torch.int32):
            raise TypeError("mixed dtypes: %s vs %s" % (t.dtype, ref.dtype))
        if not t.is_contiguous():
            raise RuntimeError("libbcbf needs contiguous row-major tensors")


def lop_elems(N, dtype):
    return int(getattr(lib, "bcbf_lop_elems" + _SUF[dtype])(N))


def hbm_read_probe(buf, launches=10, warm=2):
    """Measured read-only HBM ceiling of this device in GB/s over the caller's (large, resident) buffer `buf`:
    `launches` timed launches of `bcbf_hbm_read_probe` (16-byte non-temporal loads, nothing written), each between its own
    pair of HIP events on the current stream.  Returns dict(best_gbs, mean_gbs, bytes, launches)."""
    if not buf.is_cuda or not buf.is_contiguous():
        raise RuntimeError("hbm_read_probe needs a contiguous device buffer")
    nbytes = buf.numel() * buf.element_size()
    sink = torch.zeros(256, dtype=torch.float32, device=buf.device)
    got = ctypes.c_size_t(0)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for _ in range(warm):
        check(lib.bcbf_hbm_read_probe(_p(buf), nbytes, _p(sink), ctypes.byref(got), _stream(buf)), "bcbf_hbm_read_probe")
    for e0, e1 in evs:
        e0.record()
        check(lib.bcbf_hbm_read_probe(_p(buf), nbytes, _p(sink), ctypes.byref(got), _stream(buf)), "bcbf_hbm_read_probe")
        e1.record()
    torch.cuda.synchronize(buf.device)
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    return dict(best_gbs=got.value / (min(ms) * 1e-3) / 1e9, mean_gbs=got.value / (sum(ms) / len(ms) * 1e-3) / 1e9,
                bytes=int(got.value), launches=launches)


DATA_KERNELS = ("rbf", "matern52", "rbf_matern52")       # (index = the library's kernel_kind; the last two are opt-in)
_KSUF = {"rbf": "", "matern52": "_matern52", "rbf_matern52": "_rbfm52"}    # entry-point suffix of a data kernel


def kb_build(X, UH, Bm, ell, s2, jitter=None, lin=None, kernel="rbf"):
    """K_b[Bt,N,N]  (control_affine_model.py:370-372 + make_psd diagonal :907-910); lin[Bt] adds the linear part of
    the CoGP comparator's data kernel, k = s2 (exp(..) + lin x'x') (:1121-1122).  kernel="matern52": the opt-in
    Matern-5/2 data kernel (bcbf.h; parity unpinned -- the reference has no Matern kernel)."""
    _chk(X, UH, Bm, ell, s2, jitter, lin)
    Bt, N, n = X.shape
    m = UH.shape[2] - 1
    Kb = torch.empty(Bt, N, N, dtype=X.dtype, device=X.device)
    if kernel not in DATA_KERNELS:
        raise ValueError("data kernel %r: one of %s" % (kernel, DATA_KERNELS))
    if kernel != "rbf":
        if lin is not None:
            raise ValueError("the opt-in data kernels have no linear part")
        check(getattr(lib, "bcbf_kb_build" + _KSUF[kernel] + _suf(X))(_p(X), _p(UH), _p(Bm), _p(ell), _p(s2), _p(jitter), _p(Kb),
                                                                      Bt, N, n, m, _stream(X)), "bcbf_kb_build" + _KSUF[kernel])
        return Kb
    if lin is not None:
        check(getattr(lib, "bcbf_kb_build_rbflin" + _suf(X))(_p(X), _p(UH), _p(Bm), _p(ell), _p(s2), _p(lin), _p(jitter),
                                                             _p(Kb), Bt, N, n, m, _stream(X)), "bcbf_kb_build_rbflin")
        return Kb
    check(getattr(lib, "bcbf_kb_build" + _suf(X))(_p(X), _p(UH), _p(Bm), _p(ell), _p(s2), _p(jitter), _p(Kb),
                                                  Bt, N, n, m, _stream(X)), "bcbf_kb_build")
    return Kb


def _kern(base, kernel):
    if kernel not in DATA_KERNELS:
        raise ValueError("kernel %r: one of %s" % (kernel, DATA_KERNELS))
    return base + _KSUF[kernel]


# Launch forms of the refit (bcbf.h: BCBF_FORM_*).  form=None is AUTO -- the library's measured choice; the others are for parity
# tests and measurements.  REFIT_WAVE takes one REFIT_SUPER_* and one REFIT_OCC* value or-ed in (64-column super-panels on / off,
# register allocation for 1 / 2 waves per SIMD).
REFIT_AUTO, REFIT_WORKGROUP, REFIT_WAVE, REFIT_PAIR, REFIT_TEAM4, REFIT_TEAM8 = range(6)
REFIT_SUPER_ON, REFIT_SUPER_OFF, REFIT_OCC1, REFIT_OCC2 = 0x10, 0x20, 0x40, 0x80


def _refit_form(X, UH, Bm, ell, s2, jitter, Kdense, Lop, UHB, Ld, prev_info, info, Bt, N, n, m, kernel, form, like):
    """bcbf_refit_form: the one entry behind refit, refit_retry and potrf."""
    _kern("", kernel)
    check(getattr(lib, "bcbf_refit_form" + _suf(like))(_p(X), _p(UH), _p(Bm), _p(ell), _p(s2), _p(jitter), _p(Kdense), _p(Lop), _p(UHB),
                                                       _p(Ld), _p(prev_info), _p(info), Bt, N, n, m, DATA_KERNELS.index(kernel),
                                                       REFIT_AUTO if form is None else int(form), _stream(like)), "bcbf_refit_form")


def refit(X, UH, Bm, ell, s2, jitter=None, want_dense=False, out=None, kernel="rbf", form=None):
    """Fused K_b build + Cholesky + packing.  Returns (Lop[Bt,E], UHB[Bt,N,C], info[Bt], Ldense|None).
    out = (Lop, UHB, info): write into the caller's buffers (a closed loop that has bound their addresses).
    kernel="matern52": the opt-in Matern-5/2 data kernel.  form: a REFIT_* launch form (None: the library chooses)."""
    _chk(X, UH, Bm, ell, s2, jitter)
    Bt, N, n = X.shape
    C = UH.shape[2]
    if out is not None:
        Lop, UHB, info = out
        _chk(X, Lop, UHB, info)
        assert Lop.shape == (Bt, lop_elems(N, X.dtype)) and UHB.shape == (Bt, N, C) and info.shape == (Bt,)
    else:
        Lop = torch.empty(Bt, lop_elems(N, X.dtype), dtype=X.dtype, device=X.device)
        UHB = torch.empty(Bt, N, C, dtype=X.dtype, device=X.device)
        info = torch.empty(Bt, dtype=torch.int32, device=X.device)
    Ld = torch.empty(Bt, N, N, dtype=X.dtype, device=X.device) if want_dense else None
    if Bt > 0:
        _refit_form(X, UH, Bm, ell, s2, jitter, None, Lop, UHB, Ld, None, info, Bt, N, n, C - 1, kernel, form, X)
    return Lop, UHB, info, Ld


def refit_retry(X, UH, Bm, ell, s2, jitter, Lop, UHB, prev_info, info, kernel="rbf", form=None):
    """Factor again ONLY the instances with prev_info[b] != 0 (no host round trip), with the jitter the caller has raised
    for them; writes `info` (a different buffer than prev_info)."""
    _chk(X, UH, Bm, ell, s2, jitter, Lop, UHB, prev_info, info)
    Bt, N, n = X.shape
    if prev_info is None:
        raise ValueError("refit_retry: prev_info is required")
    if Bt > 0:
        _refit_form(X, UH, Bm, ell, s2, jitter, None, Lop, UHB, None, prev_info, info, Bt, N, n, UH.shape[2] - 1, kernel, form, X)
    return info


def refit_with_retries(X, UH, Bm, ell, s2, jitter, out, levels=3, scratch=None, level=None, counts=None, kernel="rbf"):
    """bcbf_refit followed by `levels` unconditional retry launches (x10 jitter on the instances that failed: make_psd's
    schedule, control_affine_model.py:903-919) -- nothing waits for the host.  out = (Lop, UHB, info); `jitter` is raised IN
    PLACE for the failed instances (it is the record of what every point was factored with), and so is `level[Bt]` (the
    instance's jitter level, kept by callers that start the next refit near the level that worked).  counts[levels + 1]
    (optional, int64 on the device): += the instances each launch had to factor.  Returns info (0, or the pivot of an instance
    that failed every level)."""
    Lop, UHB, info = out
    refit(X, UH, Bm, ell, s2, jitter, out=(Lop, UHB, info), kernel=kernel)
    if counts is not None:
        counts[0] += X.shape[0]
    other = torch.empty_like(info) if scratch is None else scratch
    cur, nxt = info, other
    for k in range(levels):
        fac = torch.where(cur != 0, 10.0, 1.0).to(jitter.dtype)
        jitter.mul_(fac[:, None])
        if level is not None:
            level.mul_(fac)
        if counts is not None:
            counts[k + 1] += (cur != 0).sum()
        refit_retry(X, UH, Bm, ell, s2, jitter, Lop, UHB, cur, nxt, kernel=kernel)
        cur, nxt = nxt, cur
    if cur is not info:
        info.copy_(cur)
    return info


def gram(W, Wp=None, out=None):
    """G[b,bp,C,C] = einsum("bkc,pkd->bpcd", W, Wp) on the matrix cores (bcbf_gram); Wp None = W (symmetric: half the tiles)."""
    Wp = W if Wp is None else Wp
    _chk(W, Wp, out)
    b, Np, C = W.shape
    bp = Wp.shape[0]
    if Wp.shape[1] != Np or Wp.shape[2] != C:
        raise ValueError("gram: W %s vs Wp %s" % (tuple(W.shape), tuple(Wp.shape)))
    G = torch.empty(b, bp, C, C, dtype=W.dtype, device=W.device) if out is None else out
    check(getattr(lib, "bcbf_gram" + _suf(W))(_p(W), _p(Wp), _p(G), b, bp, Np, C, _stream(W)), "bcbf_gram")
    return G


def predict_fullmat(Lop, Vw, X, UHB, ell, s2, Bm, M0, A, Xq, jitter=None, want_BkXX=False, want_kron=True, kernel="rbf"):
    """query -> Gram -> assembly in ONE host call (bcbf_predict_fullmat).  Returns (Mk[b,n,C], BkXX | None, Kron | None)."""
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, A, Xq, jitter)
    if X.shape[0] != 1:
        raise ValueError("predict_fullmat: GP tensors of ONE model (leading axis 1)")
    N, n = X.shape[1], X.shape[2]
    C, b = UHB.shape[2], Xq.shape[0]
    f = dict(dtype=X.dtype, device=X.device)
    Np = (N + 31) // 32 * 32
    Mk, Bk, W, G = torch.empty(b, n, C, **f), torch.empty(b, C, C, **f), torch.empty(b, Np, C, **f), torch.empty(b, b, C, C, **f)
    BkXX = torch.empty(b, b, C, C, **f) if want_BkXX else None
    Kron = torch.empty(b * C * n, b * C * n, **f) if want_kron else None
    check(getattr(lib, "bcbf_predict_fullmat" + _suf(X))(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(A), _p(Xq),
                                                         _p(jitter), _p(Mk), _p(Bk), _p(W), _p(G), _p(BkXX), _p(Kron), b, N, n, C - 1,
                                                         DATA_KERNELS.index(kernel), _stream(X)), "bcbf_predict_fullmat")
    return Mk, BkXX, Kron


def potrf(Kb, want_dense=False, form=None):
    """Cholesky of caller-supplied SPD matrices (torch.linalg.cholesky, control_affine_model.py:911)."""
    _chk(Kb)
    Bt, N, _ = Kb.shape
    Lop = torch.empty(Bt, lop_elems(N, Kb.dtype), dtype=Kb.dtype, device=Kb.device)
    info = torch.empty(Bt, dtype=torch.int32, device=Kb.device)
    Ld = torch.empty(Bt, N, N, dtype=Kb.dtype, device=Kb.device) if want_dense else None
    if Bt > 0:
        _refit_form(None, None, None, None, None, None, Kb, Lop, None, Ld, None, info, Bt, N, 0, 0, "rbf", form, Kb)
    return Lop, info, Ld


def potrs(Lop, Xdot, UH, M0, want_alpha=True, out_Vw=None):
    """Vw = L^-1 (Xdot - UH M0), alpha = K_b^-1 (Xdot - UH M0)  (control_affine_model.py:525-545)."""
    _chk(Lop, Xdot, UH, M0, out_Vw)
    Bt, N, n = Xdot.shape
    m = UH.shape[2] - 1
    Vw = torch.empty(Bt, N, n, dtype=Xdot.dtype, device=Xdot.device) if out_Vw is None else out_Vw
    assert Vw.shape == (Bt, N, n)
    alpha = torch.empty_like(Vw) if want_alpha else None
    check(getattr(lib, "bcbf_potrs" + _suf(Xdot))(_p(Lop), _p(Xdot), _p(UH), _p(M0), _p(Vw), _p(alpha),
                                                  Bt, N, n, m, _stream(Xdot)), "bcbf_potrs")
    return Vw, alpha


SUBSAMPLE_MAX_POOL = 8192          # bcbf_subsample_rows sorts the pool in LDS


def subsample_rows(keys, X, UH, Y, N, lo=0, P=None, out=None):
    """Random N-row subset of every instance's pool = stream rows lo .. lo+P-1 of X[B,Ntot,n], UH[B,Ntot,1+m], Y[B,Ntot,n]
    (bcbf_subsample_rows): the reference's shuffle of the whole buffer + first max_train (unicycle_move_to_pose.py:377-384)
    with the caller's draws keys[B, >=P] (fp32 uniform in [0,1), for both precisions).  Output row j = the pool row with the
    j-th smallest key, ties to the lower index: idx == torch.sort(keys[:, :P], stable=True).indices[:, :N] + lo.
    Returns (Xo[B,N,n], UHo[B,N,1+m], Yo[B,N,n], idx[B,N] int32 stream rows); out = the same four buffers to write into."""
    _chk(X, UH, Y)
    _chk(keys)
    if keys.dtype != torch.float32 or keys.device != X.device or keys.dim() != 2:
        raise TypeError("subsample_rows: keys must be a [B, >=P] float32 tensor on the streams' device")
    B, Ntot, n = X.shape
    C = UH.shape[2]
    P = Ntot - lo if P is None else int(P)
    if UH.shape[:2] != (B, Ntot) or Y.shape != (B, Ntot, n) or keys.shape[0] != B:
        raise ValueError("subsample_rows: X %s, UH %s, Y %s, keys %s" % (tuple(X.shape), tuple(UH.shape), tuple(Y.shape), tuple(keys.shape)))
    f = dict(dtype=X.dtype, device=X.device)
    if out is None:
        out = (torch.empty(B, N, n, **f), torch.empty(B, N, C, **f), torch.empty(B, N, n, **f),
               torch.empty(B, N, dtype=torch.int32, device=X.device))
    Xo, UHo, Yo, idx = out
    _chk(X, Xo, UHo, Yo, idx)
    if Xo.shape != (B, N, n) or UHo.shape != (B, N, C) or Yo.shape != (B, N, n) or idx.shape != (B, N) or idx.dtype != torch.int32:
        raise ValueError("subsample_rows: output buffers of the wrong shape / dtype")
    rc = getattr(lib, "bcbf_subsample_rows" + _suf(X))(_p(keys), keys.shape[1], lo, P, _p(X), _p(UH), _p(Y), Ntot, n, C - 1, N,
                                                       _p(Xo), _p(UHo), _p(Yo), _p(idx), B, _stream(X))
    if rc != 0:
        raise _lib.BcbfError("bcbf_subsample_rows failed (rc=%d): %s" % (rc, lib.bcbf_last_error().decode()))
    return Xo, UHo, Yo, idx


def trigger_interval(x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL=1e-4, zeta=1e-2, L_alpha=1.0, out=None):
    """Self-triggering interval of B instances in one launch (bcbf_trigger_interval; the per-step body of the reference's
    unicycle_trigger_interval_compute, trigger_interval.py:128-167): x[B,n], test-point offsets off[Nte,n] shared by the batch
    (Xtest = off + x is formed in the kernel), ls[Bh,n], sf[Bh], Adiag[Bh,n] with Bh = B or 1 (one model for all instances),
    uBu[B] = uh' B uh, xvel[B], Lh[B]; r = pdist(grid) of the reference, a scalar.  Returns (Lfh[B], tau[B], Lkd[B,n]) on the
    device; out = the same three buffers to write into (no allocation: the call is capturable in a graph)."""
    _chk(x, off, ls, sf, Adiag, uBu, xvel, Lh)
    if x.dim() != 2 or off.dim() != 2 or off.shape[1] != x.shape[1]:
        raise ValueError("trigger_interval: x %s must be [B, n] and off %s [Nte, n]" % (tuple(x.shape), tuple(off.shape)))
    B, n = x.shape
    Nte = off.shape[0]
    Bh = ls.shape[0] if ls.dim() == 2 else -1
    if ls.dim() != 2 or ls.shape[1] != n or sf.shape != (Bh,) or Adiag.shape != (Bh, n) or Bh not in (1, B):
        raise ValueError("trigger_interval: ls %s, sf %s, Adiag %s must be [Bh, n], [Bh], [Bh, n] with Bh = B = %d or 1"
                         % (tuple(ls.shape), tuple(sf.shape), tuple(Adiag.shape), B))
    if uBu.shape != (B,) or xvel.shape != (B,) or Lh.shape != (B,):
        raise ValueError("trigger_interval: uBu %s, xvel %s, Lh %s must be [B]" % (tuple(uBu.shape), tuple(xvel.shape), tuple(Lh.shape)))
    if out is None:
        out = (torch.empty(B, dtype=x.dtype, device=x.device), torch.empty(B, dtype=x.dtype, device=x.device),
               torch.empty(B, n, dtype=x.dtype, device=x.device))
    Lfh, tau, Lkd = out
    _chk(x, Lfh, tau, Lkd)
    if Lfh.shape != (B,) or tau.shape != (B,) or Lkd.shape != (B, n) or Lkd.dtype != x.dtype:
        raise ValueError("trigger_interval: output buffers of the wrong shape / dtype")
    rc = getattr(lib, "bcbf_trigger_interval" + _suf(x))(_p(x), _p(off), _p(ls), _p(sf), _p(Adiag), _p(uBu), _p(xvel), _p(Lh), float(r),
                                                         float(deltaL), float(zeta), float(L_alpha), _p(Lkd), _p(Lfh), _p(tau), B, Bh, Nte,
                                                         n, _stream(x))
    if rc != 0:
        raise _lib.BcbfError("bcbf_trigger_interval failed (rc=%d): %s" % (rc, lib.bcbf_last_error().decode()))
    return Lfh, tau, Lkd


def chol_append(Lop, knew, kappa, N):
    _chk(Lop, knew, kappa)
    Bt = Lop.shape[0]
    out = torch.empty(Bt, lop_elems(N + 1, Lop.dtype), dtype=Lop.dtype, device=Lop.device)
    info = torch.empty(Bt, dtype=torch.int32, device=Lop.device)
    check(getattr(lib, "bcbf_chol_append" + _suf(Lop))(_p(Lop), _p(knew), _p(kappa), _p(out), _p(info), Bt, N,
                                                       _stream(Lop)), "bcbf_chol_append")
    return out, info


GP_APPEND_STREAM_MIN_N = int(os.environ.get("BCBF_APPEND_STREAM_MIN_N", "384"))


def gp_append(Lop, Vw, X, UHB, ell, s2, Bm, M0, x_new, uh_new, xdot_new, jitter_new=None, kernel="rbf"):
    """Online update: one observation per instance enters the GP without refactorisation.
    Returns (Lop', Vw'[Bt,N+1,n], X'[Bt,N+1,n], UHB'[Bt,N+1,C], info).  The operator is updated in place
    (the returned Lop' IS Lop) while N+1 stays inside the same 32-row padding, re-packed otherwise.
    From N = GP_APPEND_STREAM_MIN_N on the forward solve l = L^-1 k runs on the streaming posterior kernel
    (bcbf_gp_append_stream: W = L^-1 Phi(x_new) at the HBM roofline, l = W uh_new)."""
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, x_new, uh_new, xdot_new, jitter_new)
    Bt, N, n = X.shape
    C = UHB.shape[2]
    f = dict(dtype=X.dtype, device=X.device)
    same_pad = (N + 31) // 32 == (N + 32) // 32
    Lout = Lop if same_pad else torch.empty(Bt, lop_elems(N + 1, X.dtype), **f)
    Vw2, X2, UHB2 = torch.empty(Bt, N + 1, n, **f), torch.empty(Bt, N + 1, n, **f), torch.empty(Bt, N + 1, C, **f)
    info = torch.empty(Bt, dtype=torch.int32, device=X.device)
    if kernel != "rbf" and N >= GP_APPEND_STREAM_MIN_N:  # opt-in kernels, large N: the forward solve on that kind's streaming kernel
        _kern("bcbf_gp_append", kernel)
        Np = (N + 31) // 32 * 32
        Ww, Mkw, Bkw = torch.empty(Bt, Np, C, **f), torch.empty(Bt, n, C, **f), torch.empty(Bt, C, C, **f)
        check(getattr(lib, "bcbf_gp_append_stream_kind" + _suf(X))(
            _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(x_new), _p(uh_new), _p(xdot_new),
            _p(jitter_new), _p(Lout), _p(Vw2), _p(X2), _p(UHB2), _p(info), _p(Ww), _p(Mkw), _p(Bkw), Bt, N, n, C - 1,
            DATA_KERNELS.index(kernel), _stream(X)), "bcbf_gp_append_stream_kind")
        return Lout, Vw2, X2, UHB2, info
    if kernel != "rbf":                                # opt-in kernels: the simple forward solve
        check(getattr(lib, _kern("bcbf_gp_append", kernel) + _suf(X))(
            _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(x_new), _p(uh_new), _p(xdot_new),
            _p(jitter_new), _p(Lout), _p(Vw2), _p(X2), _p(UHB2), _p(info), Bt, N, n, C - 1, _stream(X)), "bcbf_gp_append")
        return Lout, Vw2, X2, UHB2, info
    if N >= GP_APPEND_STREAM_MIN_N:
        Np = (N + 31) // 32 * 32
        Ww, Mkw, Bkw = torch.empty(Bt, Np, C, **f), torch.empty(Bt, n, C, **f), torch.empty(Bt, C, C, **f)
        check(getattr(lib, "bcbf_gp_append_stream" + _suf(X))(
            _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(x_new), _p(uh_new), _p(xdot_new),
            _p(jitter_new), _p(Lout), _p(Vw2), _p(X2), _p(UHB2), _p(info), _p(Ww), _p(Mkw), _p(Bkw), Bt, N, n, C - 1,
            _stream(X)), "bcbf_gp_append_stream")
        return Lout, Vw2, X2, UHB2, info
    check(getattr(lib, "bcbf_gp_append" + _suf(X))(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0),
                                                   _p(x_new), _p(uh_new), _p(xdot_new), _p(jitter_new), _p(Lout),
                                                   _p(Vw2), _p(X2), _p(UHB2), _p(info), Bt, N, n, C - 1, _stream(X)),
          "bcbf_gp_append")
    return Lout, Vw2, X2, UHB2, info


class ReservedGP:
    """Capacity-reserving storage of Bt independent GPs for the online path (bcbf.h: bcbf_gp_reserve,
    bcbf_posterior_query_reserved, bcbf_gp_append_reserved).  Built from a fitted state of N points
    (`refit` / `potrs` outputs); `append` enters one observation per instance IN PLACE -- no allocation, no copy of
    the per-instance arrays, no re-pack of the operator -- until N reaches `capacity`; `grow(capacity)` re-reserves.
    The work buffers of the forward solve are allocated once.  `N` is the live size; `Lop`, `Vw`, `X`, `UHB` are the
    reserved buffers ([Bt, lop_elems(capacity)], [Bt, capacity, .]).

    window = W (with the raw data of the initial points: UH, Xdot, jitter): a SLIDING WINDOW over the most recent points at
    the granularity of the packed layout's 32-row blocks (the reference keeps a random subsample of at most
    `max_train` points and refactorises from scratch, unicycle_move_to_pose.py:373-384, controllers.py:348-352).  The live
    size runs between W and W + 31; the append that would make it W + 32 first drops the OLDEST 32 points
    (`drop_oldest_block`): the remaining rows move up and the factor of the window is recomputed from the data by the
    batched refit kernel.  Why a refit and not the rank-32 update L22' L22'' = L22 L22' + L21 L21' of the trailing factor: the
    update is 32 dependent sweeps of Givens-type row operations over the whole trailing factor (2 * 32 N^2 flop = 17 MFLOP at
    N = 512, latency bound, plus re-inverting every diagonal block of the packed layout), the refit is N^3 / 3 = 45 MFLOP on
    the matrix cores at 18-50 TFLOP/s -- 0.5 ms for 256 windows of 512 points in fp64, once per 32 appends of 0.47 ms each --
    and it leaves EXACTLY the factor a from-scratch refit of the window gives (no accumulation over wrap-arounds).
    Needs capacity >= W + 32.  `drop` = k (default 32) forgets the k oldest points at a time instead (the live size then
    runs between W and W + k - 1, capacity >= W + k): the reference's refit cadence `train_every_n_steps` = 40
    (unicycle_move_to_pose.py:340-386) is `drop=40`.  What this is and is not: a REFIT SCHEDULE on in-place storage, not a
    down-date kernel -- between two drops the appends are true rank-one updates in place, the drop itself recomputes the
    window's factor from the data.
    A failed factorisation of the window (after `max_tries` jitter levels) is reported: `drop_info[Bt]` holds the last
    drop's per-instance pivot index, `drop_failures` counts instances over all drops, and the next `append` returns an
    `info` that carries it (OR-ed in as a negative value) so a caller that only watches `append`'s result sees it."""

    BLOCK = 32

    TAIL_MAX = 64            # tail rows the tail step holds (bcbf_gp_tail_step: tcap <= 64)

    def __init__(self, Lop, Vw, X, UHB, ell, s2, Bm, M0, capacity, A=None, window=None, UH=None, Xdot=None, jitter=None,
                 drop=None, tail=False, retry_levels=None, factor_dtype=None, min_jitter_level=1e-5, kernel="rbf"):
        """kernel: the data kernel of the state ("rbf"; opt-in "matern52", "rbf_matern52": the `*_kind` entry points of bcbf.h --
        queries, appends, the tail step and the window refits -- bcbf_refit_retry_kind with retry_levels -- evaluate it).
        factor_dtype (retry_levels mode; e.g. float64 for an fp32 model): the window refits factor in that precision and ROUND the
        operator / UH B / Vw into the buffers the passes read (the packed layout is the same element for element) -- the passes then
        add cond(L) eps, not cond(K_b) eps.  min_jitter_level: floor of the per-instance level (fp32 passes cannot resolve a posterior
        variance below ~ sqrt(cond K_b) eps32 of the prior: 1e-3 for fp32 passes on fp64 factors).
        retry_levels = k (window mode): the window refit of a drop never waits for the host -- bcbf_refit followed by k
        unconditional bcbf_refit_retry launches (x10 jitter on the instances that failed), into a second operator buffer that
        is swapped in (no allocation per drop).  `drop_info` then holds the last level's info; `drop_failures` is counted only
        when asked for (`count_drop_failures()`: one host read).  None: ten levels with a look at the device per level."""
        _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0)
        _kern("", kernel)
        self.kernel, self._kind = kernel, DATA_KERNELS.index(kernel)
        self.retry_levels = retry_levels
        self.factor_dtype = factor_dtype if (factor_dtype is not None and factor_dtype != X.dtype) else None
        self.min_jitter_level = float(min_jitter_level)
        if self.factor_dtype is not None and retry_levels is None:
            raise ValueError("factor_dtype: mixed precision is built on the host-free window refit (retry_levels=...)")
        self._alt = None
        # retry_levels mode: the jitter LEVEL of every instance (make_psd starts at 1e-5 and goes x10 per failure; a window refit here
        # starts one level below the one that last worked) -- `jitter_level` is also what a caller scales a new point's draw with
        self.jitter_level = torch.full((X.shape[0],), float(min_jitter_level), dtype=X.dtype, device=X.device)
        self.retry_counts = torch.zeros((retry_levels or 0) + 1, dtype=torch.int64, device=X.device)
        self.Bt, self.N, self.n = X.shape
        self.C = UHB.shape[2]
        self.ell, self.s2, self.Bm, self.M0, self.A = ell, s2, Bm, M0, A
        self.capacity = 0
        self.window = None if window is None else int(window)
        self.drops = 0
        self.drop = self.BLOCK if drop is None else int(drop)
        self.drop_failures = 0
        self.drop_info = None
        self._fill(Lop, Vw, X, UHB, self.N, int(capacity))
        if self.window is not None:
            if UH is None or Xdot is None:
                raise ValueError("a sliding window refits from the data: pass UH and Xdot (and the jitter) of the initial points")
            if self.drop < 1 or self.capacity < self.window + self.drop or self.N > self.window + self.drop - 1:
                raise ValueError("window %d needs capacity >= %d and at most %d initial points" % (self.window, self.window + self.drop,
                                                                                                   self.window + self.drop - 1))
            _chk(UH, Xdot, jitter)
            f = dict(dtype=X.dtype, device=X.device)
            # raw rows of the live points (the reserved arrays hold derived quantities: UH B, L^-1 (Xdot - UH M0))
            self._rUH, self._rY = torch.zeros(self.Bt, self.capacity, self.C, **f), torch.zeros(self.Bt, self.capacity, self.n, **f)
            self._rJ = torch.zeros(self.Bt, self.capacity, **f)
            self._rUH[:, :self.N], self._rY[:, :self.N] = UH, Xdot
            if jitter is not None:
                self._rJ[:, :self.N] = jitter
        # tail=True (window mode): the points observed since the last window refit are kept as contiguous ROWS of a bordered factor
        # beside the window's own (bcbf_gp_tail_step) instead of being written into the operator's columns one element at a time
        self.tail = bool(tail)
        self.N0, self.t = self.N, 0
        if self.tail and self.window is None:
            # GROWTH with a tail (no window): the appends since the last commit are rows of a bordered factor beside the reserved
            # operator; every 32nd append commits them as one whole block row (bcbf_gp_tail_commit: full-line writes into the
            # column layout).  The live size then is N0 (committed, a multiple of 32) + t.
            if self.N % self.BLOCK or self.n > 4:
                raise ValueError("tail=True without a window starts from a multiple of %d points (and n <= 4)" % self.BLOCK)
            f = dict(dtype=X.dtype, device=X.device)
            Npc = (self.capacity + 31) // 32 * 32
            self._tcap = self.BLOCK
            self._Rb = torch.zeros(self.Bt, self._tcap, Npc, **f)
            self._Rinv = torch.zeros(self.Bt, self._tcap, self._tcap, **f)
            self._Wfull = torch.empty(self.Bt, Npc, self.C + 1, **f)
            self._sw = torch.empty(self.Bt, 1 + self.n, **f)
            self._ones = torch.ones(self.Bt, self.C, **f)
            self._Lcap = self.capacity
            self._rUH = self._rY = self._rJ = None
        elif self.tail:
            # rows the tail must hold: until the first window refit window + drop - N_init of them, `drop` after every refit
            # (N0 = window, t = 0 there) -- whichever is larger (N_init > window makes the first period the shorter one)
            self._tcap = max(self.drop, self.window + self.drop - self.N)
            if self._tcap > self.TAIL_MAX or self.n > 4:
                raise ValueError("tail=True holds at most %d points between two window refits (needs %d here) and n <= 4"
                                 % (self.TAIL_MAX, self._tcap))
            f = dict(dtype=X.dtype, device=X.device)
            Npc = (self.capacity + 31) // 32 * 32
            self._Rb = torch.zeros(self.Bt, self._tcap, Npc, **f)
            self._Rinv = torch.zeros(self.Bt, self._tcap, self._tcap, **f)
            self._Wfull = torch.empty(self.Bt, Npc, self.C + 1, **f)
            self._sw = torch.empty(self.Bt, 1 + self.n, **f)
            self._ones = torch.ones(self.Bt, self.C, **f)
            self._Lcap = self.capacity           # what the operator is laid out for: the reservation now, the window after a refit

    def _fill(self, Lop, Vw, X, UHB, N, capacity, cap_in=0, reuse=False):
        if capacity < N:
            raise ValueError("capacity %d < %d live points" % (capacity, N))
        f = dict(dtype=X.dtype, device=X.device)
        Bt, n, C = self.Bt, self.n, self.C
        if reuse:                                     # re-lay a packed state out INTO the buffers this object already owns
            Lr, Vr, Xr, Ur = self.Lop, self.Vw, self.X, self.UHB
        else:
            Lr = torch.empty(Bt, lop_elems(capacity, X.dtype), **f)
            Vr, Xr, Ur = torch.empty(Bt, capacity, n, **f), torch.empty(Bt, capacity, n, **f), torch.empty(Bt, capacity, C, **f)
        check(getattr(lib, "bcbf_gp_reserve" + _suf(X))(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(Lr), _p(Vr), _p(Xr), _p(Ur), Bt, N,
                                                        cap_in, capacity, n, C - 1, _stream(X)), "bcbf_gp_reserve")
        if reuse:
            return
        self.Lop, self.Vw, self.X, self.UHB, self.capacity = Lr, Vr, Xr, Ur, capacity
        Npc = (capacity + 31) // 32 * 32
        self._Ww, self._Mkw, self._Bkw = torch.empty(Bt, Npc, C, **f), torch.empty(Bt, n, C, **f), torch.empty(Bt, C, C, **f)
        self.info = torch.empty(Bt, dtype=torch.int32, device=X.device)

    def grow(self, capacity):
        """Re-reserve for a larger capacity: ONE copy of the state (geometric growth amortises it to O(1) per append)."""
        if capacity <= self.capacity:
            return self
        if self.window is not None:
            raise RuntimeError("a windowed ReservedGP keeps its capacity (window + 32 suffices)")
        self._fill(self.Lop, self.Vw, self.X, self.UHB, self.N, int(capacity), cap_in=self.capacity)
        return self

    def drop_oldest_block(self, max_tries=10):
        """Window mode: forget the `drop` (default 32) oldest points.  The raw rows move up, the window's factor and whitened targets are
        recomputed from them (`refit` with the jitter every point ENTERED with -- an instance whose factorisation fails
        retries with its jitter x10, as make_psd does, control_affine_model.py:903-919) and laid out into the reserved
        buffers this object already owns.  Returns info[Bt] of the last factorisation (0 = fine)."""
        if self.window is None:
            raise RuntimeError("drop_oldest_block needs a ReservedGP built with window=...")
        k = self.drop
        N2 = self.N - k
        if N2 < 1:
            raise RuntimeError("nothing would be left")
        X = self.X[:, k:self.N].contiguous()
        UH, Y, J = self._rUH[:, k:self.N].contiguous(), self._rY[:, k:self.N].contiguous(), self._rJ[:, k:self.N].contiguous()
        if self.retry_levels is not None:
            # no host round trip, no allocation: the refit and its retries write the operator buffer that is NOT being read
            f = dict(dtype=X.dtype, device=X.device)
            if self._alt is None or self._alt[0].shape[1] != lop_elems(N2, X.dtype):
                self._alt = (torch.empty(self.Bt, lop_elems(N2, X.dtype), **f), torch.empty(self.Bt, N2, self.C, **f),
                             torch.empty(self.Bt, dtype=torch.int32, device=X.device), torch.empty(self.Bt, dtype=torch.int32, device=X.device))
            Lop, UHB, info, scratch = self._alt
            # a FRESH draw for every point of the window at the instance's level, as make_psd draws one per factorisation (:907-910)
            # (raising the points' stored jitter x10 per failed refit instead would compound from window to window)
            # (starting at the level that last worked; one level down every `level_decay_every`-th refit -- 1: make_psd's restart, one
            #  level below, at every refit)
            every = getattr(self, "level_decay_every", 1)
            if every and (self.drops + 1) % every == 0:
                self.jitter_level.div_(10).clamp_(min=self.min_jitter_level)
            J = (self.jitter_level[:, None] * torch.rand(self.Bt, N2, **f)).contiguous()
            Vw_wide = None
            if self.factor_dtype is not None:
                # factor in the wide precision on the rows cast up; round the results into the buffers the passes read
                wd = self.factor_dtype
                fw = dict(dtype=wd, device=X.device)
                if getattr(self, "_wide", None) is None or self._wide[0].shape[1] != lop_elems(N2, wd):
                    self._wide = (torch.empty(self.Bt, lop_elems(N2, wd), **fw), torch.empty(self.Bt, N2, self.C, **fw))
                up = lambda t_: t_.to(wd)
                Xd, UHd, Yd, Jd, lvl = up(X), up(UH), up(Y), up(J), up(self.jitter_level)
                refit_with_retries(Xd, UHd, up(self.Bm), up(self.ell), up(self.s2), Jd, (self._wide[0], self._wide[1], info),
                                   levels=self.retry_levels, scratch=scratch, level=lvl, counts=self.retry_counts, kernel=self.kernel)
                Vw_wide, _ = potrs(self._wide[0], Yd, UHd, up(self.M0), want_alpha=False)
                Lop.copy_(self._wide[0]); UHB.copy_(self._wide[1]); J.copy_(Jd); self.jitter_level.copy_(lvl)
            else:
                refit_with_retries(X, UH, self.Bm, self.ell, self.s2, J, (Lop, UHB, info), levels=self.retry_levels, scratch=scratch,
                                   level=self.jitter_level, counts=self.retry_counts, kernel=self.kernel)
            if self.tail:
                self._alt = (self.Lop if self.Lop.shape == Lop.shape else None, UHB, info, scratch)    # the buffer now read is the next drop's target
                if self._alt[0] is None:
                    self._alt = None
        else:
            for ntry in range(max_tries):
                Lop, UHB, info, _ = refit(X, UH, self.Bm, self.ell, self.s2, J, kernel=self.kernel)
                bad = info != 0
                if not bool(bad.any()):                   # (one host round trip per drop: ~30 us against the refit's milliseconds;
                    break                                 #  speculative jitter levels would cost two more refits per drop instead)
                if ntry + 1 < max_tries:
                    J = torch.where(bad[:, None], J * 10, J)
            else:
                # still failing after max_tries levels: the instance's window is laid out as the (garbage) factor the kernel left;
                # say so where callers look -- drop_info, the failure count, and the next append's info
                self.drop_failures += int(bad.sum())
        self.drop_info = info
        if self.retry_levels is not None and self.factor_dtype is not None:
            Vw = Vw_wide.to(X.dtype)
        else:
            Vw, _ = potrs(Lop, Y, UH, self.M0, want_alpha=False)
        self._rUH[:, :N2], self._rY[:, :N2], self._rJ[:, :N2] = UH, Y, J
        if self.tail:
            # the window's operator is only read until the next refit: the packed one the refit wrote serves as it is (no re-layout
            # into the reservation, 1.3 ms of a 4.9 ms window refit at 4096 x 472); the arrays keep their reserved rows
            self.Lop, self._Lcap = Lop, N2
            self.Vw[:, :N2], self.X[:, :N2], self.UHB[:, :N2] = Vw, X, UHB
        else:
            self._fill(Lop, Vw, X, UHB, N2, self.capacity, reuse=True)
        self.N = self.N0 = N2
        self.t = 0
        self.drops += 1
        return info

    def count_drop_failures(self):
        """Host read of the last window refit's info (retry_levels mode keeps it on the device): instances still failing."""
        return 0 if self.drop_info is None else int((self.drop_info != 0).sum())

    def _tail_step(self, xq, x_new, uh_new, xdot_new, jitter_new, Mk, Bk, do_append):
        # (the pointers of this object's own buffers are converted once per window: a closed loop on part batches makes this call
        #  thousands of times and the host side of it is what bounds four part batches)
        st = self.__dict__.get("_tail_static")
        if st is None or st[0] is not self.Lop:
            st = self._tail_static = (self.Lop, getattr(lib, ("bcbf_gp_tail_step_kind" if self._kind else "bcbf_gp_tail_step") + _suf(self.X)),
                                      (_p(self.Lop), _p(self.Vw), _p(self.X), _p(self.UHB), _p(self.ell), _p(self.s2), _p(self.Bm), _p(self.M0)),
                                      (_p(self._Rb), _p(self._Rinv), _p(self.info), _p(self._Wfull), _p(self._sw)),
                                      (_p(self._rUH), _p(self._rY), _p(self._rJ)))
        check(st[1](*st[2], _p(xq), _p(x_new), _p(uh_new), _p(xdot_new), _p(jitter_new), *st[3], _p(Mk), _p(Bk), *st[4], self.Bt,
                    self.N0, self.t, self._tcap, self.capacity, self._Lcap, self.n, self.C - 1, int(do_append),
                    *((self._kind,) if self._kind else ()), _stream(self.X)),
              "bcbf_gp_tail_step")

    def posterior(self, xq, jitter2=None, want_W=False, out=None):
        """(Mk[Bt,n,C], Bk[Bt,C,C]) (+ W[Bt,Np,C]) at one query per instance on the live points."""
        _chk(self.X, xq, jitter2)
        f = dict(dtype=self.X.dtype, device=self.X.device)
        if out is None:
            Mk, Bk = torch.empty(self.Bt, self.n, self.C, **f), torch.empty(self.Bt, self.C, self.C, **f)
        else:
            Mk, Bk = out
        if self.tail:
            if jitter2 is not None or want_W:
                raise NotImplementedError("tail=True: the posterior at one query per instance, no jitter, no W")
            self._tail_step(xq, xq, self._ones, None, None, Mk, Bk, False)
            return Mk, Bk
        W = torch.empty(self.Bt, (self.N + 31) // 32 * 32, self.C, **f) if want_W else None
        check(getattr(lib, ("bcbf_posterior_query_reserved_kind" if self._kind else "bcbf_posterior_query_reserved") + _suf(self.X))(
            _p(self.Lop), _p(self.Vw), _p(self.X), _p(self.UHB), _p(self.ell), _p(self.s2), _p(self.Bm), _p(self.M0), _p(xq),
            _p(jitter2), _p(Mk), _p(Bk), _p(W), self.Bt, self.N, self.capacity, self.n, self.C - 1,
            *((self._kind,) if self._kind else ()), _stream(self.X)),
            "bcbf_posterior_query_reserved")
        return (Mk, Bk, W) if want_W else (Mk, Bk)

    def append(self, x_new, uh_new, xdot_new, jitter_new=None, query=None, out=None):
        """One observation per instance, in place.  Returns info[Bt] (0, or N+1 where the new pivot was not positive: that
        instance gained a neutral point -- retrying is the caller's business, as with `gp_append`).
        query[Bt,n] (with out = (Mk, Bk), or allocated): the posterior at `query` on the points BEFORE the append, computed
        on the same pass over the factors as the append's forward solve -- a "posterior, then append" step for the traffic
        of one; then returns (info, Mk, Bk)."""
        if self.window is not None and self.N >= self.window + self.drop:
            raise RuntimeError("window mode: the live size is already window + %d (drop_oldest_block failed?)" % self.drop)
        if self.N >= self.capacity:
            raise RuntimeError("ReservedGP is full (%d points): reserve a larger capacity" % self.capacity)
        _chk(self.X, x_new, uh_new, xdot_new, jitter_new, query)
        if self.tail:
            if self.t >= self._tcap:
                raise RuntimeError("tail=True: %d points since the last window refit -- drop_oldest_block first" % self.t)
            f = dict(dtype=self.X.dtype, device=self.X.device)
            if query is not None:
                Mk, Bk = out if out is not None else (torch.empty(self.Bt, self.n, self.C, **f), torch.empty(self.Bt, self.C, self.C, **f))
            else:
                Mk, Bk = self._Mkw, self._Bkw
            self._tail_step(x_new if query is None else query, x_new, uh_new, xdot_new, jitter_new, Mk, Bk, True)
            self.t += 1
            if self.window is None and self.t == self._tcap:
                # growth: the 32 tail rows become block row N0 / 32 of the reserved operator (one launch, full-line writes)
                check(getattr(lib, "bcbf_gp_tail_commit" + _suf(self.X))(_p(self.Lop), _p(self._Rb), _p(self._Rinv), self.Bt, self.N0, self.t,
                                                                          self._tcap, self.capacity, _stream(self.X)), "bcbf_gp_tail_commit")
                self.N0 += self._tcap
                self.t = 0
            return self._appended(query, Mk, Bk)
        Mk = Bk = None
        if query is not None:
            f = dict(dtype=self.X.dtype, device=self.X.device)
            Mk, Bk = out if out is not None else (torch.empty(self.Bt, self.n, self.C, **f), torch.empty(self.Bt, self.C, self.C, **f))
            if self._Ww.shape[0] != 2 * self.Bt:                      # work buffers for two queries per instance
                self._Ww = torch.empty(2 * self.Bt, *self._Ww.shape[1:], **f)
                self._Mkw, self._Bkw = torch.empty(2 * self.Bt, self.n, self.C, **f), torch.empty(2 * self.Bt, self.C, self.C, **f)
        head = (_p(self.Lop), _p(self.Vw), _p(self.X), _p(self.UHB), _p(self.ell), _p(self.s2), _p(self.Bm), _p(self.M0),
                _p(x_new), _p(uh_new), _p(xdot_new), _p(jitter_new), _p(self.info), _p(self._Ww), _p(self._Mkw), _p(self._Bkw),
                _p(query), _p(Mk), _p(Bk))
        tail = (self.Bt, self.N, self.capacity, self.n, self.C - 1, _stream(self.X))
        if self._kind:
            raw = (_p(self._rUH), _p(self._rY), _p(self._rJ)) if self.window is not None else (None, None, None)
            check(getattr(lib, "bcbf_gp_append_reserved_kind" + _suf(self.X))(*head, *raw, *tail[:-1], self._kind, tail[-1]),
                  "bcbf_gp_append_reserved_kind")
        elif self.window is not None:
            # window mode: the same launches also record the point's RAW row (uh, xdot, jitter) -- neutral (0, 0, unit pivot)
            # where the new pivot failed, which is what the in-place path holds -- for the next refit of the window
            check(getattr(lib, "bcbf_gp_append_reserved_raw" + _suf(self.X))(*head, _p(self._rUH), _p(self._rY), _p(self._rJ), *tail),
                  "bcbf_gp_append_reserved_raw")
        else:
            check(getattr(lib, "bcbf_gp_append_reserved" + _suf(self.X))(*head, *tail), "bcbf_gp_append_reserved")
        return self._appended(query, Mk, Bk)

    def _appended(self, query, Mk, Bk):
        self.N += 1
        info = self.info
        if self.window is not None and self.N >= self.window + self.drop:
            dinfo = self.drop_oldest_block()          # AFTER the append: the posterior the caller asked for saw every point
            if self.drop_failures:                    # a window that could not be factored: carried in the returned info (< 0)
                info = torch.where(dinfo != 0, -dinfo.abs() - 1, info)
        return info if query is None else (info, Mk, Bk)

    def live(self):
        """Views of the live rows: (Vw[Bt,N,n], X[Bt,N,n], UHB[Bt,N,C]) (strided: not inputs of the packed-layout kernels)."""
        return self.Vw[:, :self.N], self.X[:, :self.N], self.UHB[:, :self.N]


def kb_inverse(Lop, N, gemm=True):
    """Dense K_b^-1 [Bt,N,N] from the packed factor (fit path only).  gemm=True: L^-1 from bcbf_trtri (the forward half of
    the solve) and K_b^-1 = L^-T L^-1 on the matrix cores (bcbf_syrk_lt: 32 x 32 tiles of the triangular product);
    gemm=False: bcbf_potri (forward + backward solves of the identity: its backward half is latency bound, 2 ms at
    N = 512 for one model against 0.3 ms this way)."""
    _chk(Lop)
    Bt = Lop.shape[0]
    Kinv = torch.empty(Bt, N, N, dtype=Lop.dtype, device=Lop.device)
    if gemm:
        Linv = torch.empty(Bt, N, N, dtype=Lop.dtype, device=Lop.device)
        check(getattr(lib, "bcbf_trtri" + _suf(Lop))(_p(Lop), _p(Linv), Bt, N, _stream(Lop)), "bcbf_trtri")
        check(getattr(lib, "bcbf_syrk_lt" + _suf(Lop))(_p(Linv), _p(Kinv), Bt, N, _stream(Lop)), "bcbf_syrk_lt")
        return Kinv
    check(getattr(lib, "bcbf_potri" + _suf(Lop))(_p(Lop), _p(Kinv), Bt, N, _stream(Lop)), "bcbf_potri")
    return Kinv


_MLL_WORK = {}


def _mll_work(Bt, N, m, device):
    """Workspace of bcbf_mll_grad's split form (partial sums; reused between the iterations of a fit).  One buffer per
    (device, HIP stream): fits on different streams / threads never share partial sums, and a buffer is only ever
    replaced by a LARGER one on its own stream, where stream order puts the free behind the launches that read it (the
    launches go through ctypes, so torch's allocator sees no other stream using the block)."""
    nbytes = int(lib.bcbf_mll_grad_work_bytes(Bt, N, m))
    if nbytes == 0:
        return None
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    buf = _MLL_WORK.get(key)
    if buf is None or buf.numel() * 8 < nbytes:
        buf = _MLL_WORK[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    return buf


def mll_grad(Lop, alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin=None, kernel="rbf"):
    """O(N^2) sums of the marginal-log-likelihood gradient (bcbf.h K12).  Returns
    (g_ell[Bt,n], g_s2[Bt], g_B[Bt,C,C], logdetK[Bt], RtA[Bt,nt,nt], UHtA[Bt,C,nt]) (+ g_lin[Bt] when `lin` is given:
    RBF + Linear data kernel, nt = R.shape[2] target columns)."""
    _chk(Lop, alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin)
    Bt, N, n = X.shape
    C = UH.shape[2]
    f = dict(dtype=X.dtype, device=X.device)
    if lin is not None:
        nt = R.shape[2]
        g_ell, g_s2, g_B, g_lin = torch.empty(Bt, n, **f), torch.empty(Bt, **f), torch.empty(Bt, C, C, **f), torch.empty(Bt, **f)
        logdet, RtA, UHtA = torch.empty(Bt, **f), torch.empty(Bt, nt, nt, **f), torch.empty(Bt, C, nt, **f)
        check(getattr(lib, "bcbf_mll_grad_rbflin" + _suf(X))(
            _p(Lop), _p(alpha), _p(Kinv), _p(X), _p(UH), _p(R), _p(Ainv), _p(Bm), _p(ell), _p(s2), _p(lin), _p(g_ell),
            _p(g_s2), _p(g_lin), _p(g_B), _p(logdet), _p(RtA), _p(UHtA), Bt, N, n, C - 1, nt,
            _p(_mll_work(Bt, N, C - 1, X.device)), _stream(X)), "bcbf_mll_grad_rbflin")
        return g_ell, g_s2, g_B, logdet, RtA, UHtA, g_lin
    g_ell, g_s2, g_B = torch.empty(Bt, n, **f), torch.empty(Bt, **f), torch.empty(Bt, C, C, **f)
    logdet, RtA, UHtA = torch.empty(Bt, **f), torch.empty(Bt, n, n, **f), torch.empty(Bt, C, n, **f)
    check(getattr(lib, _kern("bcbf_mll_grad", kernel) + _suf(X))(_p(Lop), _p(alpha), _p(Kinv), _p(X), _p(UH), _p(R), _p(Ainv), _p(Bm),
                                                  _p(ell), _p(s2), _p(g_ell), _p(g_s2), _p(g_B), _p(logdet), _p(RtA),
                                                  _p(UHtA), Bt, N, n, C - 1, _p(_mll_work(Bt, N, C - 1, X.device)),
                                                  _stream(X)), "bcbf_mll_grad")
    return g_ell, g_s2, g_B, logdet, RtA, UHtA


def kinv_apply(Kinv, R, out=None):
    """alpha[Bt,N,nt] = Kinv R for the dense symmetric K_b^-1 (bcbf_kinv_apply: the fit iteration's `Kinv @ R` without a
    library GEMM)."""
    _chk(Kinv, R, out)
    Bt, N, nt = R.shape
    alpha = torch.empty_like(R) if out is None else out
    check(getattr(lib, "bcbf_kinv_apply" + _suf(R))(_p(Kinv), _p(R), _p(alpha), Bt, N, nt, _stream(R)), "bcbf_kinv_apply")
    return alpha


def fit_param_count(n, m, rA=None, rB=None):
    """Raw parameters per model of the batched fit (bcbf.h: theta's layout)."""
    P = int(lib.bcbf_fit_param_count(n, m, n if rA is None else rA, 1 + m if rB is None else rB))
    if P < 0:
        raise ValueError("unsupported fit shape n=%d m=%d ranks %s %s" % (n, m, rA, rB))
    return P


def fit_derive(theta, n, m, rA, rB, want_Ainv=True):
    """theta[Bt,P] -> dict(ell, s2, A, Bm, M0[, Ainv, logdetA]) (bcbf_fit_derive)."""
    _chk(theta)
    Bt, C = theta.shape[0], 1 + m
    f = dict(dtype=theta.dtype, device=theta.device)
    out = dict(ell=torch.empty(Bt, n, **f), s2=torch.empty(Bt, **f), A=torch.empty(Bt, n, n, **f), Bm=torch.empty(Bt, C, C, **f),
               M0=torch.empty(Bt, C, n, **f))
    if want_Ainv:
        out.update(Ainv=torch.empty(Bt, n, n, **f), logdetA=torch.empty(Bt, **f))
    check(getattr(lib, "bcbf_fit_derive" + _suf(theta))(_p(theta), _p(out["ell"]), _p(out["s2"]), _p(out["A"]), _p(out["Bm"]),
                                                        _p(out["M0"]), _p(out.get("Ainv")), _p(out.get("logdetA")), Bt, n, m, rA, rB,
                                                        _stream(theta)), "bcbf_fit_derive")
    return out


def fit_adam_step(theta, mom1, mom2, sums, Ainv, logdetA, N, n, m, rA, rB, step, lr, betas=(0.9, 0.999), eps=1e-8, skip=None,
                  gamma_prior=None, want_grad=False):
    """One Adam update of every model from mll_grad's `sums` = (g_ell, g_s2, g_B, logdetK, RtA, UHtA) (bcbf_fit_adam_step).
    Returns (loss[Bt], grad[Bt,P] | None); step = 0: value and gradient only."""
    g_ell, g_s2, g_B, logdetK, RtA, UHtA = sums[:6]
    _chk(theta, mom1, mom2, g_ell, g_s2, g_B, logdetK, RtA, UHtA, Ainv, logdetA, skip)
    Bt = theta.shape[0]
    loss = torch.empty(Bt, dtype=theta.dtype, device=theta.device)
    grad = torch.empty_like(theta) if want_grad else None
    prior = None if gamma_prior is None else (ctypes.c_double * 2)(float(gamma_prior[0]), float(gamma_prior[1]))
    check(getattr(lib, "bcbf_fit_adam_step" + _suf(theta))(
        _p(theta), _p(mom1), _p(mom2), _p(g_ell), _p(g_s2), _p(g_B), _p(logdetK), _p(RtA), _p(UHtA), _p(Ainv), _p(logdetA), _p(skip),
        _p(loss), _p(grad), Bt, N, n, m, rA, rB, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), prior,
        _stream(theta)), "bcbf_fit_adam_step")
    return loss, grad


def posterior_step(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2=None, out=None):
    """(Mk[Bt,n,C], Bk[Bt,C,C]) at one query per instance  (control_affine_model.py:1051-1091, b=1)."""
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2)
    Bt, N, n = X.shape
    C = UHB.shape[2]
    if out is None:
        Mk = torch.empty(Bt, n, C, dtype=X.dtype, device=X.device)
        Bk = torch.empty(Bt, C, C, dtype=X.dtype, device=X.device)
    else:
        Mk, Bk = out
    check(getattr(lib, "bcbf_posterior_step" + _suf(X))(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm),
                                                        _p(M0), _p(xq), _p(jitter2), _p(Mk), _p(Bk), Bt, N, n, C - 1,
                                                        _stream(X)), "bcbf_posterior_step")
    return Mk, Bk


def posterior_query(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2=None, shared=True, want_W=False, lin=None, kernel="rbf"):
    """b queries against one shared GP (shared=True; GP tensors carry a leading axis of 1) or one query per
    instance.  Returns (Mk[b,n,C], Bk[b,C,C], W[b,Np,C] | None).  lin: linear part of the data kernel (CoGP);
    kernel="matern52": the opt-in Matern-5/2 data kernel (streaming kernel)."""
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2, lin)
    N, n = X.shape[1], X.shape[2]
    C = UHB.shape[2]
    b = xq.shape[0]
    if shared and X.shape[0] != 1:
        raise ValueError("shared query: GP tensors must have a leading axis of 1")
    Mk = torch.empty(b, n, C, dtype=X.dtype, device=X.device)
    Bk = torch.empty(b, C, C, dtype=X.dtype, device=X.device)
    Np = (N + 31) // 32 * 32
    W = torch.empty(b, Np, C, dtype=X.dtype, device=X.device) if want_W else None
    if kernel not in DATA_KERNELS:
        raise ValueError("data kernel %r: one of %s" % (kernel, DATA_KERNELS))
    if kernel != "rbf":
        if lin is not None:
            raise ValueError("the opt-in data kernels have no linear part")
        check(getattr(lib, "bcbf_posterior_query" + _KSUF[kernel] + _suf(X))(
            _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(xq), _p(jitter2), _p(Mk), _p(Bk), _p(W),
            1 if shared else 0, b, N, n, C - 1, _stream(X)), "bcbf_posterior_query" + _KSUF[kernel])
        return Mk, Bk, W
    if lin is not None:
        check(getattr(lib, "bcbf_posterior_query_rbflin" + _suf(X))(
            _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(lin), _p(Bm), _p(M0), _p(xq), _p(jitter2), _p(Mk), _p(Bk),
            _p(W), 1 if shared else 0, b, N, n, C - 1, _stream(X)), "bcbf_posterior_query_rbflin")
        return Mk, Bk, W
    check(getattr(lib, "bcbf_posterior_query" + _suf(X))(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm),
                                                         _p(M0), _p(xq), _p(jitter2), _p(Mk), _p(Bk), _p(W),
                                                         1 if shared else 0, b, N, n, C - 1, _stream(X)),
          "bcbf_posterior_query")
    return Mk, Bk, W


def posterior_shared(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2=None, want_W=False, kernel="rbf"):
    """b queries against one GP on the matrix cores (GP tensors carry a leading axis of 1; fp64: N <= 512, n <= 4).
    posterior_query(shared=True) routes here for b >= 16; this entry forces the MFMA kernel for any b.
    kernel="matern52": the opt-in Matern-5/2 data kernel (bcbf_posterior_shared_matern52)."""
    if kernel not in DATA_KERNELS:
        raise ValueError("kernel must be one of %s" % (DATA_KERNELS,))
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, jitter2)
    if X.dtype == torch.float64 and (X.shape[1] > 512 or X.shape[2] > 4):
        raise ValueError("posterior_shared in fp64 holds the solution in registers: N <= 512, n <= 4 (posterior_query streams the rest)")
    if X.shape[0] != 1:
        raise ValueError("shared query: GP tensors must have a leading axis of 1")
    N, n = X.shape[1], X.shape[2]
    C = UHB.shape[2]
    b = xq.shape[0]
    Mk = torch.empty(b, n, C, dtype=X.dtype, device=X.device)
    Bk = torch.empty(b, C, C, dtype=X.dtype, device=X.device)
    Np = (N + 31) // 32 * 32
    W = torch.empty(b, Np, C, dtype=X.dtype, device=X.device) if want_W else None
    fn = getattr(lib, "bcbf_posterior_shared" + _KSUF[kernel] + _suf(X))
    check(fn(_p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(xq),
             _p(jitter2), _p(Mk), _p(Bk), _p(W), b, N, n, C - 1, _stream(X)), "bcbf_posterior_shared")
    return Mk, Bk, W


def posterior_jets(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq, shared=False, want_W=False, kernel="rbf"):
    """(Mk, Bk, G[b,CT,CT], Mj[b,n,CT]) with CT = (1+m)(1+n): value + first x-derivative jets
    (replaces autograd through custom_predict in GradientGP, gp_algebra.py:340-402).  want_W: also
    Wj[b,Np,CT] = L^-1 [Phi, dPhi/dx_d] (fifth return value), for derivative kernels between different states."""
    _chk(Lop, Vw, X, UHB, ell, s2, Bm, M0, xq)
    N, n = X.shape[1], X.shape[2]
    C = UHB.shape[2]
    b = xq.shape[0]
    CT = C * (1 + n)
    f = dict(dtype=X.dtype, device=X.device)
    Mk, Bk = torch.empty(b, n, C, **f), torch.empty(b, C, C, **f)
    G, Mj = torch.empty(b, CT, CT, **f), torch.empty(b, n, CT, **f)
    Wj = torch.empty(b, (N + 31) // 32 * 32, CT, **f) if want_W else None
    check(getattr(lib, _kern("bcbf_posterior_jets", kernel) + _suf(X))(
        _p(Lop), _p(Vw), _p(X), _p(UHB), _p(ell), _p(s2), _p(Bm), _p(M0), _p(xq), _p(Mk), _p(Bk), _p(G), _p(Mj), _p(Wj),
        1 if shared else 0, b, N, n, C - 1, _stream(X)), "bcbf_posterior_jets")
    return (Mk, Bk, G, Mj, Wj) if want_W else (Mk, Bk, G, Mj)


def predict_assemble(G, Xq, Xqp, ell, s2, Bm, A=None, jitter=None, want_BkXX=True, want_kron=False, kernel="rbf"):
    """Predictive covariance of a query set against ONE GP in one launch, from the Gram G[b, b', 1+m, 1+m] = W_b' W'_b' of its
    whitened cross-covariances (`posterior_query(..., want_W=True)`; `torch.einsum("bnc,pnd->bpcd", W, Wp)`):
    BkXX[b, b', 1+m, 1+m] = k(x_b, x'_b') Bm - G (+ `jitter`[b (1+m)] on its diagonal: make_psd, control_affine_model.py:1089)
    and / or kron(Bk2, A) [b (1+m) n, b' (1+m) n] (`custom_predict_fullmat`, :963-980).
    Xq[b, n], Xqp[b', n], ell[n], s2[1], Bm[1+m, 1+m], A[n, n]."""
    _chk(G, Xq, Xqp, ell, s2, Bm, A, jitter)
    if kernel not in DATA_KERNELS:
        raise ValueError("kernel %r: one of %s" % (kernel, DATA_KERNELS))
    b, bp, C, _ = G.shape
    n = Xq.shape[1]
    if G.shape[3] != C or Xq.shape[0] != b or Xqp.shape[0] != bp or Xqp.shape[1] != n:
        raise ValueError("predict_assemble: inconsistent shapes")
    if want_kron and A is None:
        raise ValueError("predict_assemble: the Kronecker product needs A")
    BkXX = torch.empty(b, bp, C, C, dtype=G.dtype, device=G.device) if want_BkXX else None
    Kron = torch.empty(b * C * n, bp * C * n, dtype=G.dtype, device=G.device) if want_kron else None
    check(getattr(lib, "bcbf_predict_assemble" + _suf(G))(
        _p(G), _p(Xq), _p(Xqp), _p(ell), _p(s2), _p(Bm), _p(A) if A is not None else None,
        _p(jitter) if jitter is not None else None, _p(BkXX) if want_BkXX else None, _p(Kron) if want_kron else None,
        b, bp, n, C - 1, DATA_KERNELS.index(kernel), _stream(G)), "bcbf_predict_assemble")
    return BkXX, Kron


HESSIAN_MODES = {"reference": 0, "project": 1}


def clean_hessian(H, eigeps=2e-3, mode="reference"):
    """The eigenvalue clean-up GradientGP.knl(x, x) applies to its Hessian (gp_algebra.py:384-392) on a batch H[b,n,n]
    (n <= 4) on the device.  mode "reference": `eigenvectors.T @ diag(evalz) @ eigenvectors` with the general solver's
    eigenvectors (csrc/geev_small.h); "project": spectral projection of the symmetric part.  Returns (H_clean, status):
    status 0 untouched, 1 an eigenvalue <= -eigeps (H returned unchanged; the reference asserts), 4 / 6 cleaned."""
    _chk(H)
    b, n, _ = H.shape
    out = torch.empty_like(H)
    status = torch.empty(b, dtype=torch.int32, device=H.device)
    check(getattr(lib, "bcbf_clean_hessian" + _suf(H))(_p(H), _p(out), _p(status), b, n, float(eigeps),
                                                       HESSIAN_MODES[mode], _stream(H)), "bcbf_clean_hessian")
    return out, status


def cbc2_terms(Mk, Bk, G, Mj, A, Bm, ell, s2, h, gh, Hh, kalpha, u0, hessian_mode="reference", kernel="rbf"):
    """Rel-degree-2 terms (cbc2_gp + cbc2_quadratic_terms, cbc2.py:7-33).  Returns
    ((mean_A[b,m], mean_b[b]), (Q[b,m,m], p[b,m], r[b]), mean[b], var[b], status[b]); status 1 = the reference's
    positive-definiteness assert fails, 4 / 6 = the Hessian clean-up ran (`clean_hessian`), 0 otherwise."""
    _chk(Mk, Bk, G, Mj, A, Bm, ell, s2, h, gh, Hh, kalpha, u0)
    b, n, C = Mk.shape
    m = C - 1
    out = torch.empty(b, m + 1 + m * m + m + 1 + 2, dtype=Mk.dtype, device=Mk.device)
    status = torch.empty(b, dtype=torch.int32, device=Mk.device)
    check(getattr(lib, "bcbf_cbc2_terms" + _suf(Mk))(_p(Mk), _p(Bk), _p(G), _p(Mj), _p(A), _p(Bm), _p(ell), _p(s2),
                                                     _p(h), _p(gh), _p(Hh), _p(kalpha), _p(u0), _p(out), _p(status),
                                                     b, n, m, HESSIAN_MODES[hessian_mode], DATA_KERNELS.index(kernel),
                                                     _stream(Mk)), "bcbf_cbc2_terms")
    o = 0
    mean_A = out[:, o:o + m]; o += m
    mean_b = out[:, o]; o += 1
    Q = out[:, o:o + m * m].reshape(b, m, m); o += m * m
    p = out[:, o:o + m]; o += m
    r = out[:, o]; o += 1
    return (mean_A, mean_b), (Q, p, r), out[:, o], out[:, o + 1], status


def terms_width(m):
    return m + 1 + m * m + m + 1


def cone_width(m):
    return (m + 1) * m + (m + 1) + m + 1


def cbc_terms(Mk, Bk, A, grad, cst, sign, fhat, ghat, want_terms=True, out=None):
    """Rel-degree-1 constraint terms + cone form (cbc2.py:7-23, unicycle_move_to_pose.py:837-916)."""
    _chk(Mk, Bk, A, grad, cst, sign, fhat, ghat)
    Bt, K, n = grad.shape
    m = ghat.shape[2]
    if out is None:
        terms = torch.empty(Bt, K, terms_width(m), dtype=Mk.dtype, device=Mk.device) if want_terms else None
        cones = torch.empty(Bt, K, cone_width(m), dtype=Mk.dtype, device=Mk.device)
        cstatus = torch.empty(Bt, K, dtype=torch.int32, device=Mk.device)
    else:
        terms, cones, cstatus = out
    check(getattr(lib, "bcbf_cbc_terms" + _suf(Mk))(_p(Mk), _p(Bk), _p(A), _p(grad), _p(cst), _p(sign), _p(fhat),
                                                    _p(ghat), _p(terms), _p(cones), _p(cstatus), Bt, K, n, m,
                                                    _stream(Mk)), "bcbf_cbc_terms")
    return terms, cones, cstatus


def unpack_terms(terms, m):
    o = 0
    bfe = terms[..., o:o + m]; o += m
    e = terms[..., o]; o += 1
    V = terms[..., o:o + m * m].reshape(*terms.shape[:-1], m, m); o += m * m
    bfv = terms[..., o:o + m]; o += m
    v = terms[..., o]
    return bfe, e, V, bfv, v


def unpack_cones(cones, m):
    o = 0
    A = cones[..., o:o + (m + 1) * m].reshape(*cones.shape[:-1], m + 1, m); o += (m + 1) * m
    b = cones[..., o:o + m + 1]; o += m + 1
    c = cones[..., o:o + m]; o += m
    d = cones[..., o]
    return A, b, c, d


def pack_cones(A, b, c, d):
    lead = A.shape[:-2]
    return torch.cat([A.reshape(*lead, -1), b, c, d.reshape(*lead, 1)], dim=-1).contiguous()


def socp(w, r, cones, relax_mask, rho, max_iters=100, out=None):
    """The CLF-CBF program of ControllerCLFBayesian.control (unicycle_move_to_pose.py:926-953).
    Returns (y[Bt,m+1] = [u, relax], status[Bt], iters[Bt])."""
    _chk(w, r, cones, relax_mask, rho)
    Bt, K, _ = cones.shape
    m = r.shape[1]
    if K > 4:                                  # more cones than the quad kernel's four lanes: the generic solver
        return _socp_generic(w, r, cones, relax_mask, rho, max_iters, out)
    if out is None:
        y = torch.empty(Bt, m + 1, dtype=w.dtype, device=w.device)
        status = torch.empty(Bt, dtype=torch.int32, device=w.device)
        iters = torch.empty(Bt, dtype=torch.int32, device=w.device)
    else:
        y, status, iters = out
    check(getattr(lib, "bcbf_socp" + _suf(w))(_p(w), _p(r), _p(cones), _p(relax_mask), _p(rho), _p(y), _p(status),
                                              _p(iters), Bt, K, m, max_iters, _stream(w)), "bcbf_socp")
    return y, status, iters


def _socp_generic(w, r, cones, relax_mask, rho, max_iters=100, out=None):
    """The CLF-CBF program with more than four cones (e.g. a third obstacle), through `bcbf_coneqp_f64`:
    min sum w_i (u_i - r_i)^2 + w_m relax^2  s.t.  c_k'u + d_k + relax_mask_k relax >= rho |A_k u + b_k|
    as  min 1/2 y'P y + q'y, G y + s = h, s in Q^{m+2} x ... (rows [-c', -relax_mask; -rho A, 0], h = [d; rho b]).
    Row assembly is host-side tensor plumbing; the solve is the library's (fp64)."""
    Bt, K, _ = cones.shape
    m = r.shape[1]
    f64 = dict(dtype=torch.float64, device=w.device)
    A, b, c, d = (t.to(torch.float64) for t in unpack_cones(cones, m))
    nv, D = m + 1, m + 2
    rho64 = rho.to(torch.float64)
    G = torch.zeros(Bt, K, D, nv, **f64)
    G[:, :, 0, :m] = -c
    G[:, :, 0, m] = -relax_mask.to(torch.float64)[None, :]
    G[:, :, 1:, :m] = -rho64[:, None, None, None] * A
    h = torch.cat([d[..., None], rho64[:, None, None] * b], dim=-1)
    P = torch.diag_embed(2.0 * w.to(torch.float64)).contiguous()
    q = torch.zeros(Bt, nv, **f64)
    q[:, :m] = -2.0 * w[:, :m].to(torch.float64) * r.to(torch.float64)
    x, status, iters = coneqp(P, q, G.reshape(Bt, K * D, nv).contiguous(), h.reshape(Bt, K * D).contiguous(), 0, [D] * K,
                              max_iters=max_iters)
    y = x.to(w.dtype)
    if out is not None:
        out[0].copy_(y); out[1].copy_(status); out[2].copy_(iters)
        return out
    return y, status, iters


def cbc_socp(Mk, Bk, A, grad, cst, sign, fhat, ghat, w, r, relax_mask, rho, max_iters=100, want_terms=False):
    """cbc_terms + socp in one launch (four lanes per instance).  Returns (y, status, iters, cones, cstatus, terms)."""
    _chk(Mk, Bk, A, grad, cst, sign, fhat, ghat, w, r, relax_mask, rho)
    Bt, K, n = grad.shape
    m = ghat.shape[2]
    if K > 4:                                  # two launches + the generic solver (see `socp`)
        terms, cones, cstatus = cbc_terms(Mk, Bk, A, grad, cst, sign, fhat, ghat, want_terms=want_terms)
        y, status, iters = _socp_generic(w, r, cones, relax_mask, rho, max_iters)
        status = torch.where((cstatus != 0).any(dim=1), torch.full_like(status, 3), status)
        return y, status, iters, cones, cstatus, terms
    f = dict(dtype=Mk.dtype, device=Mk.device)
    terms = torch.empty(Bt, K, terms_width(m), **f) if want_terms else None
    cones = torch.empty(Bt, K, cone_width(m), **f)
    cstatus = torch.empty(Bt, K, dtype=torch.int32, device=Mk.device)
    y = torch.empty(Bt, m + 1, **f)
    status = torch.empty(Bt, dtype=torch.int32, device=Mk.device)
    iters = torch.empty(Bt, dtype=torch.int32, device=Mk.device)
    check(getattr(lib, "bcbf_cbc_socp" + _suf(Mk))(_p(Mk), _p(Bk), _p(A), _p(grad), _p(cst), _p(sign), _p(fhat),
                                                   _p(ghat), _p(w), _p(r), _p(relax_mask), _p(rho), _p(terms),
                                                   _p(cones), _p(cstatus), _p(y), _p(status), _p(iters), Bt, K, n, m,
                                                   max_iters, _stream(Mk)), "bcbf_cbc_socp")
    return y, status, iters, cones, cstatus, terms


def coneqp(P, q, G, h, l, qdims, max_iters=100):
    """Generic small cone QP, fp64 (optimizers.py:42-116)."""
    _chk(P, q, G, h)
    if P.dtype != torch.float64:
        raise TypeError("coneqp is fp64 only")
    Bt, nv = q.shape
    qd = (ctypes.c_int * max(1, len(qdims)))(*qdims)
    x = torch.empty(Bt, nv, dtype=P.dtype, device=P.device)
    status = torch.empty(Bt, dtype=torch.int32, device=P.device)
    iters = torch.empty(Bt, dtype=torch.int32, device=P.device)
    check(lib.bcbf_coneqp_f64(_p(P), _p(q), _p(G), _p(h), nv, l, qd, len(qdims), _p(x), _p(status), _p(iters), Bt,
                              max_iters, _stream(P)), "bcbf_coneqp")
    return x, status, iters


def controller_cones(terms, u_ref, kinds, factors=None, ctrl_reg=1.0, relax_weight=1.0, extravars=2, objective=True):
    """Rows (G[Bt,Kt,nv], h[Bt,Kt], qdims, l, cstatus) of the SOCPController / QPController program over
    y = [extravars.., u] (controllers.py:396-540, 614-662) from packed quadratic terms[Bt,K,T]."""
    K = len(kinds)
    if K:
        _chk(terms)
    ref = terms if K else u_ref
    Bt = ref.shape[0]
    m = u_ref.shape[1] if u_ref is not None else None
    if m is None:
        T = terms.shape[2]
        m = next(mm for mm in range(1, 8) if terms_width(mm) == T)
    kd = (ctypes.c_int * max(1, K))(*kinds)
    fc = (ctypes.c_double * max(1, K))(*([1.0] * K if factors is None else [float(f) for f in factors]))
    Kt = lib.bcbf_controller_cones_rows(kd, K, m, int(bool(objective)))
    if Kt < 0:
        raise ValueError("bad constraint kinds %r" % (kinds,))
    nv = extravars + m
    G = torch.empty(Bt, Kt, nv, dtype=torch.float64, device=ref.device)
    h = torch.empty(Bt, Kt, dtype=torch.float64, device=ref.device)
    cstatus = torch.zeros(Bt, max(K, 1), dtype=torch.int32, device=ref.device)
    check(getattr(lib, "bcbf_controller_cones" + _suf(ref))(
        _p(terms if K else None), _p(u_ref.contiguous() if u_ref is not None else None), kd, fc, float(ctrl_reg),
        float(relax_weight), extravars, int(bool(objective)), _p(G), _p(h), _p(cstatus), Bt, K, m, _stream(ref)),
        "bcbf_controller_cones")
    l = sum(1 for k in kinds if k == 2)
    qdims = ([m + 2] if objective else []) + [m + 2 for k in kinds if k != 2]
    return G, h, qdims, l, cstatus[:, :K]


def unicycle_constraints(x, plan, dot_plan, Kp, clf_gamma, centers, radii, tw, gammas, L_mean, out=None):
    """CLC row + obstacle rows: (grad[Bt,1+Kob,3], cst[Bt,1+Kob], fhat[Bt,3], ghat[Bt,3,2])."""
    _chk(x, plan, dot_plan, Kp, centers, radii, tw, gammas)
    Bt = x.shape[0]
    Kob = 0 if centers is None else centers.shape[1]
    if out is None:
        grad = torch.empty(Bt, 1 + Kob, 3, dtype=x.dtype, device=x.device)
        cst = torch.empty(Bt, 1 + Kob, dtype=x.dtype, device=x.device)
        fhat = torch.empty(Bt, 3, dtype=x.dtype, device=x.device)
        ghat = torch.empty(Bt, 3, 2, dtype=x.dtype, device=x.device)
    else:
        grad, cst, fhat, ghat = out
    check(getattr(lib, "bcbf_unicycle_constraints" + _suf(x))(
        _p(x), _p(plan), _p(dot_plan), _p(Kp), clf_gamma, _p(centers), _p(radii), _p(tw), _p(gammas), L_mean,
        _p(grad), _p(cst), _p(fhat), _p(ghat), Bt, Kob, _stream(x)), "bcbf_unicycle_constraints")
    return grad, cst, fhat, ghat


def unicycle_step(x, u, dt, L_true):
    """In-place explicit Euler step of the Ackermann plant (unicycle_move_to_pose.py:277-282)."""
    _chk(x, u)
    check(getattr(lib, "bcbf_unicycle_step" + _suf(x))(_p(x), _p(u), dt, L_true, x.shape[0], _stream(x)),
          "bcbf_unicycle_step")
    return x


def rollout_stats(cst, y, status, w, gammas, min_h, cost, fails):
    """Safety bookkeeping of one closed-loop step (bcbf_rollout_stats): min_h, cost, fails updated in place."""
    _chk(cst, y, w, gammas, min_h, cost)
    Bt, Kob = cst.shape[0], cst.shape[1] - 1
    check(getattr(lib, "bcbf_rollout_stats" + _suf(cst))(_p(cst), _p(y), _p(status), _p(w), _p(gammas), _p(min_h), _p(cost),
                                                         _p(fails), Bt, Kob, y.shape[1], _stream(cst)), "bcbf_rollout_stats")


def _bind_call(fn, what, x, stream, out):
    """What every bound step does per call: `call(ev_start, ev_stop, args)` runs fn(*args, ev_start, ev_stop, stream) -- on `stream`
    when one was fixed, else on the current stream at call time -- checks the return code under the entry's name and returns `out`."""
    dev = x.device
    fixed = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None

    def call(ev_start, ev_stop, args):
        ev0 = ctypes.c_void_p(ev_start.cuda_event) if ev_start is not None else None
        ev1 = ctypes.c_void_p(ev_stop.cuda_event) if ev_stop is not None else None
        rc = fn(*args, ev0, ev1, fixed if fixed is not None else ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc:
            check(rc, what)
        return out
    return call


def _control_step_args(gp, task, ws, x):
    """Argument checks shared by the two forms below: returns (gp with every key present, A[Bt,n,n], N, shared)."""
    Bt = x.shape[0]
    if gp.get("Lop") is None:              # fixed-kernel model: ws["Mk"], ws["Bk"] are inputs, gp carries only A
        _chk(x, gp["A"], task["plan"], ws["y"], ws["Mk"], ws["Bk"])
        N, shared = 0, False
        gp = dict(gp, Lop=None, Vw=None, X=None, UHB=None, ell=None, s2=None, Bm=None, M0=None)
    else:
        _chk(x, gp["Lop"], gp["Vw"], gp["X"], gp["UHB"], task["plan"], ws["y"])
        N = gp["X"].shape[1]
        shared = gp["X"].shape[0] == 1 and Bt > 1
        if not shared and gp["X"].shape[0] != Bt:
            raise ValueError("GP tensors must carry a leading axis of 1 (shared model) or Bt")
    A = gp["A"]
    if A.shape[0] != Bt:                     # per-instance kernel matrix A for the fused terms+SOCP kernel
        if ws.get("A_shared_src") is not A:
            ws["A_shared"], ws["A_shared_src"] = A.expand(Bt, *A.shape[1:]).contiguous(), A
        A = ws["A_shared"]
    return gp, A, N, shared


def unicycle_control_step(gp, task, ws, x, dt=0.0, L_true=1.0, L_mean=1.0, clf_gamma=10.0, max_iters=100,
                          ev_start=None, ev_stop=None):
    """One control step for a batch of unicycle instances in ONE host call
    (ControllerCLFBayesian.control, unicycle_move_to_pose.py:926-995).

    gp:   dict(Lop, Vw, X, UHB, ell, s2, Bm, M0, A), or dict(A) alone for the fixed-kernel model (then ws['Mk'], ws['Bk']
    are inputs: 0 and I);  task: dict(plan, dot_plan, Kp, centers, radii, tw, gammas,
    w, r, sign, relax_mask, rho);  ws: dict of workspaces (grad, cst, fhat, ghat, Mk, Bk, cones, cstatus, y,
    status, iters) from `control_workspace`.  x[Bt,3] is advanced in place when dt > 0.  Returns ws['y'].
    GP tensors with a leading axis of 1 and Bt > 1 = one learned model shared by all instances (Monte-Carlo
    rollouts of a fixed model): the posterior runs as a shared query (fp32: the matrix-core kernel)."""
    if task["centers"].shape[1] + 1 > 4:       # more constraints than the fused kernel's four lanes: composed path
        return _unicycle_control_step_composed(gp, task, ws, x, dt, L_true, L_mean, clf_gamma, max_iters)
    return unicycle_control_step_prepare(gp, task, ws, x, dt, L_true, L_mean, clf_gamma, max_iters)(ev_start, ev_stop)


def _unicycle_control_step_composed(gp, task, ws, x, dt, L_true, L_mean, clf_gamma, max_iters):
    """The control step as separate entry points (task rows -> posterior -> terms -> generic cone solver -> plant step on
    the solved instances): for programs with more than four constraints."""
    gp, A, N, shared = _control_step_args(gp, task, ws, x)
    unicycle_constraints(x, task["plan"], task["dot_plan"], task["Kp"], clf_gamma, task["centers"], task["radii"],
                         task["tw"], task["gammas"], L_mean, out=(ws["grad"], ws["cst"], ws["fhat"], ws["ghat"]))
    kernel = gp.get("kernel", "rbf")
    if gp["Lop"] is not None:
        if shared or kernel != "rbf":
            Mk, Bk, _ = posterior_query(gp["Lop"], gp["Vw"], gp["X"], gp["UHB"], gp["ell"], gp["s2"], gp["Bm"], gp["M0"], x,
                                        shared=shared, kernel=kernel)
            ws["Mk"].copy_(Mk); ws["Bk"].copy_(Bk)
        else:
            posterior_step(gp["Lop"], gp["Vw"], gp["X"], gp["UHB"], gp["ell"], gp["s2"], gp["Bm"], gp["M0"], x,
                           out=(ws["Mk"], ws["Bk"]))
    y, status, iters, cones, cstatus, _ = cbc_socp(ws["Mk"], ws["Bk"], A, ws["grad"], ws["cst"], task["sign"], ws["fhat"],
                                                   ws["ghat"], task["w"], task["r"], task["relax_mask"], task["rho"],
                                                   max_iters=max_iters)
    ws["y"].copy_(y); ws["status"].copy_(status); ws["iters"].copy_(iters)
    ws["cones"].copy_(cones); ws["cstatus"].copy_(cstatus)
    if dt > 0:
        u = torch.where((status == 0)[:, None], y[:, :2], torch.zeros_like(y[:, :2])).contiguous()
        unicycle_step(x, u, dt, L_true)        # unsolved instances: zero displacement (they keep their state)
    return ws["y"]


def unicycle_control_step_prepare(gp, task, ws, x, dt=0.0, L_true=1.0, L_mean=1.0, clf_gamma=10.0, max_iters=100,
                                  stream=None, observe=None, sampled=None):
    """Bind every argument of `unicycle_control_step` once and return `step(ev_start=None, ev_stop=None)`.
    A closed loop calls the same entry point with the same buffers thousands of times; converting ~40 tensors to
    pointers per call costs more host time than the two launches take on the device for small batches.  The tensors
    must keep their storage (update them in place); the closure keeps them alive.
    stream: a fixed torch stream for both launches (default: the current stream at call time).
    observe = dict(xq=[Bt,3] | None, xq_next=[Bt,3] | None, shift_invariant=True, advance_plan=False): the loop LEARNS FROM ITSELF
    (bcbf_unicycle_control_step_observe; RBF models): the posterior is queried at `xq`, and the solve / plant launch writes this
    step's observation row where the call says -- `step(ev_start, ev_stop, obs=(obs_x, obs_uh, obs_y, ld))`, three-column
    tensors whose row b * ld is instance b's (ld = 1: [Bt,3] tensors) -- and the next query into `xq_next`.
    sampled = dict(z=[Bt,3], xdot_s=[Bt,3] | None, cbc_s=[Bt,1+Kob] | None): the plant is DRAWN FROM THE MODEL'S POSTERIOR
    (bcbf_unicycle_control_step_sampled; any data kernel): a solved instance advances by xdot_s = fhat + ghat u + M_k ubar +
    sqrt(ubar' B_k ubar) chol(A) z instead of by the true drive (L_true is ignored), cbc_s = sign_k (grad_k . xdot_s + cst_k) is the
    condition on the draw.  `z` holds the caller's standard-normal draws: refill it in place before every step (the library draws
    no random numbers).  Draws of different steps are independent -- exact per-step marginals, not one function drawn along the
    trajectory.  The buffers are the caller's (`control_workspace` does not hold them); combines with `observe`, whose rows then
    record the sampled plant."""
    gp, A, N, shared = _control_step_args(gp, task, ws, x)
    Bt = x.shape[0]
    Kob = task["centers"].shape[1]
    kernel = gp.get("kernel", "rbf")                       # data kernel of the learned model: "rbf" (the reference's) | "matern52"
    if kernel not in DATA_KERNELS:
        raise ValueError("gp['kernel'] must be one of %s" % (DATA_KERNELS,))
    if observe is not None and kernel != "rbf" and sampled is None:
        raise NotImplementedError("the observing control step is built for the reference's RBF data kernel")
    name = "bcbf_unicycle_control_step" + ("_sampled" if sampled is not None else "_observe" if observe is not None else _KSUF[kernel])
    head = (_p(gp["Lop"]), _p(gp["Vw"]), _p(gp["X"]), _p(gp["UHB"]), _p(gp["ell"]), _p(gp["s2"]), _p(gp["Bm"]),
            _p(gp["M0"]), _p(A), _p(x), _p(task["plan"]), _p(task["dot_plan"]), _p(task["Kp"]), clf_gamma,
            _p(task["centers"]), _p(task["radii"]), _p(task["tw"]), _p(task["gammas"]), L_mean, _p(task["w"]),
            _p(task["r"]), _p(task["sign"]), _p(task["relax_mask"]), _p(task["rho"]), _p(ws["grad"]), _p(ws["cst"]),
            _p(ws["fhat"]), _p(ws["ghat"]), _p(ws["Mk"]), _p(ws["Bk"]), _p(ws["cones"]), _p(ws["cstatus"]), _p(ws["y"]),
            _p(ws["status"]), _p(ws["iters"]), dt, L_true, Bt, N, Kob, max_iters, 1 if shared else 0)
    keep = (dict(gp), dict(task), dict(ws), x, A, stream, observe)      # the pointers above are only valid while these live
    call = _bind_call(getattr(lib, name + _suf(x)), name, x, stream, ws["y"])
    if observe is None and sampled is None:
        def step(ev_start=None, ev_stop=None):
            return call(ev_start, ev_stop, head)
        step.keep = keep
        return step

    tail = ()                                              # the sampled entry: (kernel_kind, z, xdot_s, cbc_s)
    if sampled is not None:
        z, xdot_s, cbc_s = sampled["z"], sampled.get("xdot_s"), sampled.get("cbc_s")
        _chk(x, z, xdot_s, cbc_s)
        if z is None or tuple(z.shape) != (Bt, 3):
            raise ValueError("sampled['z'] must be a [Bt,3] tensor of standard-normal draws")
        if (xdot_s is not None and tuple(xdot_s.shape) != (Bt, 3)) or (cbc_s is not None and tuple(cbc_s.shape) != (Bt, 1 + Kob)):
            raise ValueError("sampled['xdot_s'] is [Bt,3] and sampled['cbc_s'] is [Bt,1+Kob]")
        tail = (DATA_KERNELS.index(kernel), _p(z), _p(xdot_s), _p(cbc_s))
        keep += (dict(sampled),)
    obs_cfg = observe or {}
    xq, xq_next = obs_cfg.get("xq"), obs_cfg.get("xq_next")
    _chk(x, xq, xq_next)
    p_xq, p_next = _p(xq), _p(xq_next)
    flags = (1 if obs_cfg.get("shift_invariant", True) else 0) | (2 if obs_cfg.get("advance_plan", False) else 0)

    def step(ev_start=None, ev_stop=None, obs=None):
        o = (None, None, None, 1) if obs is None else (_p(obs[0]), _p(obs[1]), _p(obs[2]), int(obs[3]))
        return call(ev_start, ev_stop, (*head, p_xq, *o, p_next, flags, *tail))
    step.keep = keep
    return step


def rollout_risk(cbc_s, status, viol, solved, min_cbc):
    """Risk bookkeeping of one step on a posterior-drawn plant (bcbf_rollout_risk): where status == 0, solved += 1,
    viol[b,k-1] += (cbc_s[b,k] < 0) (non-finite counts) and min_cbc takes the running minimum, in place; one launch."""
    _chk(cbc_s, min_cbc)
    Bt, Kob = cbc_s.shape[0], cbc_s.shape[1] - 1
    if viol.dtype != torch.int32 or solved.dtype != torch.int32 or status.dtype != torch.int32:
        raise ValueError("rollout_risk: status, viol and solved are int32 tensors")
    check(getattr(lib, "bcbf_rollout_risk" + _suf(cbc_s))(_p(cbc_s), _p(status), _p(viol), _p(solved), _p(min_cbc), Bt, Kob,
                                                         _stream(cbc_s)), "bcbf_rollout_risk")


class ConcurrentControlLoop:
    """The unicycle control step for a batch split into `parts` part batches, each on its OWN HIP stream (posterior
    launch, then solve launch, in stream order).  Instances never interact, so this is the same computation as
    `unicycle_control_step` on the whole batch -- every instance takes one control step per `step()` -- but the device
    runs one part's solve launch (task rows + terms + SOCP + plant step: latency bound, one wave per CU) beside another
    part's posterior stream (HBM bound), and a part's posterior fills the tail of the other's.  At the BASELINE config the
    serialized solve launch is 15-19 % of a single-stream step.  BASELINE config, ms per step: 1 part 0.408, 2 parts
    0.358, 3 parts 0.314, 4 parts 0.309 -- PROVIDED the runtime has a hardware queue per part stream: ROCm maps the
    streams of a process onto GPU_MAX_HW_QUEUES (default 4) queues, the null stream included, and two streams that share
    a queue serialize (4 parts at the default: 0.446).  Export GPU_MAX_HW_QUEUES=8 before HIP initialises for four parts
    (bench.py does), use three otherwise.  From three parts on the solves are hidden completely and the staggered
    posterior launches stream at a higher rate than one big launch (0.90 of the HBM peak against 0.84).  (An event-chained variant -- all posterior launches on one
    stream, solves on side streams -- was measured and rejected: each cross-stream dependency costs ~10 us on this
    stack, which ate the whole gain.)  gp / task tensors with a leading axis of Bt are sliced per part; `x` [Bt,3] is
    advanced in place.

    step(events=None): events = [(ev_start, ev_stop)] per part brackets that part's posterior kernel on its stream.
    Results: `y`, `status`, `iters` ([Bt,...] buffers); call `synchronize()` before reading them on another stream."""

    GP_INSTANCE_KEYS = ("Lop", "Vw", "X", "UHB", "ell", "s2", "Bm", "M0")       # + "A" when it carries the batch axis
    TASK_INSTANCE_KEYS = ("x", "x0", "xg", "plan", "dot_plan", "centers", "radii", "w", "r", "rho")

    def __init__(self, gp, task, x, parts=2, dt=0.0, L_true=1.0, L_mean=1.0, clf_gamma=10.0, max_iters=100):
        Bt = x.shape[0]
        if not 1 <= parts <= Bt:
            raise ValueError("cannot split a batch of %d into %d parts" % (Bt, parts))
        dev = x.device
        # contiguous part batches, the first Bt % parts of them one instance longer (4096 -> 1366 + 1365 + 1365)
        base, rem = divmod(Bt, parts)
        self.bounds = [(c * base + min(c, rem), (c + 1) * base + min(c + 1, rem)) for c in range(parts)]
        self.parts, self.x, self.device = parts, x, dev
        Kob = task["centers"].shape[1]
        self.ws = control_workspace(Bt, Kob, x.dtype, dev)
        self.y, self.status, self.iters = self.ws["y"], self.ws["status"], self.ws["iters"]
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(parts)]
        self._steps = []
        shared_model = gp.get("Lop") is not None and gp["X"].shape[0] == 1 and Bt > 1
        cur = torch.cuda.current_stream(dev)
        A = gp["A"]                                  # [Bt,n,n], or [1,n,n] = one kernel matrix for every instance
        a_key = ("A",) if (A.dim() == 3 and A.shape[0] == Bt and Bt > 1) else ()
        gp_keys = a_key if shared_model else self.GP_INSTANCE_KEYS + a_key
        for c in range(parts):
            sl = slice(*self.bounds[c])
            # per-instance tensors are named, not inferred from their shape (with a small batch a global task tensor --
            # Kp[3], sign[3], tw[Kob], gammas[Kob], relax_mask[3] -- can have a leading dimension equal to Bt)
            def cut(k, v, keys):
                if not (torch.is_tensor(v) and k in keys):
                    return v
                if v.dim() == 0 or v.shape[0] != Bt:
                    raise ValueError("%s: expected a per-instance tensor with leading dimension %d, got %s" % (k, Bt, tuple(v.shape)))
                return v[sl]
            gpc = {k: cut(k, v, gp_keys) for k, v in gp.items()}
            taskc = {k: cut(k, v, self.TASK_INSTANCE_KEYS) for k, v in task.items()}
            wsc = {k: v[sl] for k, v in self.ws.items()}
            self._steps.append(unicycle_control_step_prepare(
                gpc, taskc, wsc, x[sl], dt=dt, L_true=L_true, L_mean=L_mean, clf_gamma=clf_gamma, max_iters=max_iters,
                stream=self.streams[c]))
            self.streams[c].wait_stream(cur)       # whatever produced the inputs on the current stream happens first

    def step(self, events=None):
        for c, st in enumerate(self._steps):
            if events is None:
                st()
            else:
                st(events[c][0], events[c][1])

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


def control_workspace(Bt, Kob, dtype, device, n=3, m=2):
    K = 1 + Kob
    f = dict(dtype=dtype, device=device)
    i = dict(dtype=torch.int32, device=device)
    return dict(grad=torch.empty(Bt, K, n, **f), cst=torch.empty(Bt, K, **f), fhat=torch.empty(Bt, n, **f),
                ghat=torch.empty(Bt, n, m, **f), Mk=torch.empty(Bt, n, 1 + m, **f), Bk=torch.empty(Bt, 1 + m, 1 + m, **f),
                cones=torch.empty(Bt, K, cone_width(m), **f), cstatus=torch.empty(Bt, K, **i),
                y=torch.empty(Bt, m + 1, **f), status=torch.empty(Bt, **i), iters=torch.empty(Bt, **i))


# ------------------------------------------------------------------------------------------------ obstacle fields
# (bcbf.h "Obstacle fields": a working set of S <= 3 discs in the fused solver, certified against a field of up to MAX_FIELD)
MAX_FIELD = 256
FIELD_CERTIFIED, FIELD_FULL, FIELD_UNSOLVED, FIELD_UNCERTIFIED = 1, 2, 3, 6
# (tol_f, tol_a) of the audit: fp64 = the solvers' acceptance and ten times it; fp32 measured, bcbf.h BCBF_FIELD_TOL_*_F32
FIELD_TOLERANCES = {torch.float64: (1e-7, 1e-6), torch.float32: (5e-7, 7e-6)}


def _field_args(x, field):
    """(centers_f[Bf,Kf,2], radii_f[Bf,Kf], field_stride, Kf) of field = dict(centers, radii): a leading axis of 1 (or none) is one
    field shared by every instance, a leading axis of Bt one field per instance."""
    cen, rad = field["centers"], field["radii"]
    if cen.dim() == 2:
        cen, rad = cen[None], rad[None]
    _chk(x, cen, rad)
    Bt, Kf = x.shape[0], rad.shape[1]
    if cen.shape != (rad.shape[0], Kf, 2) or rad.shape[0] not in (1, Bt):
        raise ValueError("field: centers[Bf,Kf,2] and radii[Bf,Kf] with Bf = 1 (shared) or Bt")
    if not 1 <= Kf <= MAX_FIELD:
        raise ValueError("a field holds 1..%d discs, got %d" % (MAX_FIELD, Kf))
    return cen, rad, (1 if rad.shape[0] == Bt and Bt > 1 else 0), Kf


def obstacle_field_workspace(Bt, S, dtype, device):
    """Buffers of the obstacle-field step: the working set (idx[Bt,S], centers_sel[Bt,S,2], radii_sel[Bt,S] -- the control step's
    task['centers'] / task['radii']), the certificate (cert, rounds, worst_margin, worst_idx, nviol, status_eff) and the loop's
    statistics (min_h = +inf, cost = 0, fails = 0)."""
    f = dict(dtype=dtype, device=device)
    i = dict(dtype=torch.int32, device=device)
    return dict(idx=torch.zeros(Bt, S, **i), centers_sel=torch.zeros(Bt, S, 2, **f), radii_sel=torch.ones(Bt, S, **f),
                cert=torch.zeros(Bt, **i), rounds=torch.zeros(Bt, **i), worst_margin=torch.zeros(Bt, **f),
                worst_idx=torch.zeros(Bt, **i), nviol=torch.zeros(Bt, **i), status_eff=torch.zeros(Bt, **i),
                min_h=torch.full((Bt,), float("inf"), **f), cost=torch.zeros(Bt, **f), fails=torch.zeros(Bt, **i))


def obstacle_field_select(x, field, tw, fws):
    """bcbf_obstacle_field_select: the S = fws['idx'].shape[1] discs of smallest h_k(x) into the working set; min_h over the whole
    field; cert = rounds = 0."""
    cen, rad, stride, Kf = _field_args(x, field)
    _chk(x, tw, fws["idx"], fws["centers_sel"], fws["radii_sel"], fws["min_h"], fws["cert"], fws["rounds"])
    Bt, S = fws["idx"].shape
    check(getattr(lib, "bcbf_obstacle_field_select" + _suf(x))(
        _p(x), _p(cen), _p(rad), stride, _p(tw), _p(fws["idx"]), _p(fws["centers_sel"]), _p(fws["radii_sel"]), _p(fws["min_h"]),
        _p(fws["cert"]), _p(fws["rounds"]), Bt, Kf, S, _stream(x)), "bcbf_obstacle_field_select")
    return fws["idx"]


def obstacle_field_audit(x, ws, A, rho, field, tw, gamma, fws, tol_f=None, tol_a=None):
    """bcbf_obstacle_field_audit at the control ws['y'] of the working-set solve (run with dt = 0, so x is the state the program
    was formed at): certify, declare the working set full, or swap the worst violator in for the slack-most slot (bcbf.h)."""
    cen, rad, stride, Kf = _field_args(x, field)
    _chk(x, ws["y"], ws["status"], ws["Mk"], ws["Bk"], A, ws["fhat"], ws["ghat"], rho, tw, fws["idx"], fws["centers_sel"],
         fws["radii_sel"], fws["cert"], fws["rounds"], fws["worst_margin"], fws["worst_idx"], fws["nviol"])
    Bt, S = fws["idx"].shape
    if A.shape[0] != Bt:
        raise ValueError("A must be [Bt,3,3] (one kernel matrix per instance, as the fused step reads it)")
    d_f, d_a = FIELD_TOLERANCES[x.dtype]
    check(getattr(lib, "bcbf_obstacle_field_audit" + _suf(x))(
        _p(x), _p(ws["y"]), _p(ws["status"]), _p(ws["Mk"]), _p(ws["Bk"]), _p(A), _p(ws["fhat"]), _p(ws["ghat"]), _p(rho),
        _p(cen), _p(rad), stride, _p(tw), float(gamma), d_f if tol_f is None else float(tol_f),
        d_a if tol_a is None else float(tol_a), _p(fws["idx"]), _p(fws["centers_sel"]), _p(fws["radii_sel"]), _p(fws["cert"]),
        _p(fws["rounds"]), _p(fws["worst_margin"]), _p(fws["worst_idx"]), _p(fws["nviol"]), Bt, Kf, S, _stream(x)),
        "bcbf_obstacle_field_audit")
    return fws["cert"]


def obstacle_field_commit(x, y, status, fws, dt=0.0, L_true=1.0):
    """bcbf_obstacle_field_commit: status_eff (0 = certified optimum of the full program), and the plant step of exactly those."""
    _chk(x, y, status, fws["cert"], fws["status_eff"])
    check(getattr(lib, "bcbf_obstacle_field_commit" + _suf(x))(
        _p(x), _p(y), _p(status), _p(fws["cert"]), _p(fws["status_eff"]), dt, L_true, x.shape[0], _stream(x)),
        "bcbf_obstacle_field_commit")
    return fws["status_eff"]


_FIELD_RISK_STEP = ("xdot_s", "cbc_min", "cbc_argmin", "tight_idx", "cbc_tight", "nneg")
_FIELD_RISK_SUMS = ("solved", "viol_tight", "viol_any", "viol_unselected", "viol_discs", "min_cbc")


def obstacle_field_risk_workspace(Bt, dtype, device):
    """Buffers of `obstacle_field_commit_sampled`: the caller's normals z[Bt,3]; the outputs of one step -- xdot_s[Bt,3], cbc_min,
    cbc_tight [Bt], cbc_argmin, tight_idx, nneg [Bt] int32; and the accumulators -- solved, viol_tight, viol_any, viol_unselected,
    viol_discs [Bt] int32 = 0, min_cbc[Bt] = +inf."""
    f = dict(dtype=dtype, device=device)
    i = dict(dtype=torch.int32, device=device)
    ws = dict(z=torch.zeros(Bt, 3, **f), xdot_s=torch.zeros(Bt, 3, **f), cbc_min=torch.zeros(Bt, **f), cbc_tight=torch.zeros(Bt, **f),
              min_cbc=torch.full((Bt,), float("inf"), **f))
    ws.update({k: torch.zeros(Bt, **i) for k in ("cbc_argmin", "tight_idx", "nneg") + _FIELD_RISK_SUMS[:5]})
    return ws


def obstacle_field_commit_sampled(x, ws, A, rho, field, tw, gamma, fws, risk, dt=0.0):
    """bcbf_obstacle_field_commit_sampled, in place of `obstacle_field_commit` on a plant DRAWN FROM THE MODEL'S POSTERIOR: writes
    status_eff as the plain commit does; an instance with status_eff = 0 advances by one draw xdot_s = fhat + ghat u + M_k ubar +
    sqrt(ubar' B_k ubar) chol(A) z (risk['z']: the caller's standard normals, refilled before every step), and the condition of
    EVERY disc of the field is evaluated on that draw at the state before the step: cbc_min / cbc_argmin, the tightest cone (smallest
    audit margin) tight_idx and its drawn condition cbc_tight, nneg = the number of negative conditions, and the accumulators of
    `obstacle_field_risk_workspace`.  Every other instance keeps its state and its accumulators.  dt = 0: the state stays."""
    cen, rad, stride, Kf = _field_args(x, field)
    _chk(x, ws["y"], ws["status"], ws["Mk"], ws["Bk"], A, ws["fhat"], ws["ghat"], rho, tw, fws["idx"], fws["cert"], fws["status_eff"],
         *(risk[k] for k in ("z",) + _FIELD_RISK_STEP + _FIELD_RISK_SUMS))
    Bt, S = fws["idx"].shape
    if A.shape[0] != Bt:
        raise ValueError("A must be [Bt,3,3] (one kernel matrix per instance, as the fused step reads it)")
    if tuple(risk["z"].shape) != (Bt, 3) or risk["z"].dtype != x.dtype:
        raise ValueError("risk['z'] must be a [Bt,3] tensor of standard-normal draws in x's dtype")
    for k in _FIELD_RISK_STEP + _FIELD_RISK_SUMS:
        want = x.dtype if k in ("xdot_s", "cbc_min", "cbc_tight", "min_cbc") else torch.int32
        if risk[k].dtype != want or tuple(risk[k].shape) != ((Bt, 3) if k == "xdot_s" else (Bt,)):
            raise ValueError("risk[%r]: the buffers of obstacle_field_risk_workspace(Bt, x.dtype, x.device)" % k)
    check(getattr(lib, "bcbf_obstacle_field_commit_sampled" + _suf(x))(
        _p(x), _p(ws["y"]), _p(ws["status"]), _p(fws["cert"]), _p(ws["Mk"]), _p(ws["Bk"]), _p(A), _p(ws["fhat"]), _p(ws["ghat"]),
        _p(rho), _p(cen), _p(rad), stride, _p(tw), float(gamma), _p(fws["idx"]), _p(risk["z"]), _p(fws["status_eff"]),
        *(_p(risk[k]) for k in _FIELD_RISK_STEP + _FIELD_RISK_SUMS), float(dt), Bt, Kf, S, _stream(x)),
        "bcbf_obstacle_field_commit_sampled")
    return fws["status_eff"]


def unicycle_field_control_step_prepare(gp, task, field, ws, x, rounds=3, dt=0.0, L_true=1.0, L_mean=1.0, clf_gamma=10.0,
                                        max_iters=100, fws=None, tol_f=None, tol_a=None, stats=True, sampled=None):
    """The chance-constrained control step among the Kf <= 256 discs of `field` = dict(centers[Bf,Kf,2], radii[Bf,Kf]) (Bf = 1: one
    field for all instances).  Returns step(): on the current stream, with no host look at the device (capturable),
        select -> the fused control step on the working set (dt = 0) -> audit
        -> (rounds - 1) x [the same step in its Lop = NULL form on ws['Mk'], ws['Bk'] -> audit] -> commit -> rollout_stats.
    An instance certified in an earlier round is solved again and reproduces its y (the solver is deterministic and
    position-independent); the audit leaves it alone.  task: as `unicycle_control_step`, for S = task['sign'].shape[0] - 1 <= 3
    obstacle slots -- sign[1+S], relax_mask[1+S], gammas[S] all equal (one gamma for the field; mixed gammas raise ValueError);
    its 'centers' / 'radii' are replaced by the working set's.  ws = control_workspace(Bt, S); fws = obstacle_field_workspace(Bt, S)
    (made here when None): step.fws.  status_eff[b] = 0 where the step is the certified optimum of the FULL program and the plant
    moved (dt > 0); BCBF_FIELD_UNCERTIFIED (6) where `rounds` did not suffice or the working set is full; the solver's status
    where the working-set program was not solved.
    sampled = dict(z=[Bt,3], risk=obstacle_field_risk_workspace(Bt, ...)): the plant is DRAWN FROM THE MODEL'S POSTERIOR -- the
    commit is `obstacle_field_commit_sampled` (L_true is ignored), reading the caller's normals from `z` (refill it in place before
    every step; risk['z'] when `z` is absent) and counting the drawn conditions of every disc into `risk`.  Still capturable.
    sampled = None enqueues exactly the true-plant step.  The observing and self-triggered steps are out of scope."""
    if rounds < 1:
        raise ValueError("rounds must be >= 1")
    Bt = x.shape[0]
    S = task["sign"].shape[0] - 1
    if not 1 <= S <= 3:
        raise ValueError("the working set holds 1..3 obstacle slots (task['sign'] has 1 + S rows), got %d" % S)
    gam = task["gammas"]
    if gam.shape[0] != S or not bool((gam == gam[0]).all()):
        raise ValueError("an obstacle field has one gamma: task['gammas'] must hold S equal values")
    gamma = float(gam[0])
    cen, rad, stride, Kf = _field_args(x, field)
    if Kf < S:
        raise ValueError("the field holds fewer discs (%d) than the working set has slots (%d)" % (Kf, S))
    if fws is None:
        fws = obstacle_field_workspace(Bt, S, x.dtype, x.device)
    task = dict(task, centers=fws["centers_sel"], radii=fws["radii_sel"])
    field = dict(centers=cen, radii=rad)
    first = unicycle_control_step_prepare(gp, task, ws, x, 0.0, L_true, L_mean, clf_gamma, max_iters)
    again = first
    if rounds > 1 and gp.get("Lop") is not None:
        again = unicycle_control_step_prepare(dict(A=gp["A"]), task, ws, x, 0.0, L_true, L_mean, clf_gamma, max_iters)
    _, A, _, _ = _control_step_args(gp, task, ws, x)
    tw, rho, w = task["tw"], task["rho"], task["w"]
    risk = None
    if sampled is not None:
        risk = dict(sampled["risk"])
        if sampled.get("z") is not None:
            risk["z"] = sampled["z"]

    def step():
        obstacle_field_select(x, field, tw, fws)
        first()
        obstacle_field_audit(x, ws, A, rho, field, tw, gamma, fws, tol_f, tol_a)
        for _ in range(rounds - 1):
            again()
            obstacle_field_audit(x, ws, A, rho, field, tw, gamma, fws, tol_f, tol_a)
        if risk is None:
            obstacle_field_commit(x, ws["y"], ws["status"], fws, dt, L_true)
        else:
            obstacle_field_commit_sampled(x, ws, A, rho, field, tw, gamma, fws, risk, dt)
        if stats:
            rollout_stats(ws["cst"], ws["y"], fws["status_eff"], w, gam, fws["min_h"], fws["cost"], fws["fails"])
        return ws["y"]
    step.fws = fws
    step.keep = (first, again, task, field, A, risk)
    return step


def trigger_workspace(Bt, dtype, device):
    """Buffers of `unicycle_trigger_step_prepare`: every instance's clock t[Bt] (fp64 whatever the working type) and event count
    events[Bt] (int32), both zero, and the outputs of one event -- tau, dt_used, Lfh, Lkd[Bt,3], Lh, xvel, uBu (zero: a finished
    instance's rows are never written)."""
    f = dict(dtype=dtype, device=device)
    ws = {k: torch.zeros(Bt, **f) for k in ("tau", "dt_used", "Lfh", "Lh", "xvel", "uBu")}
    ws.update(Lkd=torch.zeros(Bt, 3, **f), t=torch.zeros(Bt, dtype=torch.float64, device=device),
              events=torch.zeros(Bt, dtype=torch.int32, device=device))
    return ws


def trigger_audit_workspace(Bt, Kob, dtype, device):
    """Buffers of `unicycle_trigger_step_prepare(sampled=..., audit=...)` (bcbf_unicycle_trigger_step_audit), as
    dict(sampled=dict(z[Bt,3], xdot_s[Bt,3], cbc_s[Bt,1+Kob], viol[Bt,Kob], solved[Bt], min_cbc[Bt,Kob]),
    audit=dict(u_held[Bt,2], held[Bt], held_mean[Bt,Kob], held_margin[Bt,Kob], audit_n[Bt], audit_neg[Bt,Kob,2],
    audit_min[Bt,Kob,2])): the two dicts that call takes.  Counters and flags (int32) are zero, the running minima +inf; `z`
    is the caller's to refill with standard normals before every event (the library draws no random numbers)."""
    f = dict(dtype=dtype, device=device)
    i = dict(dtype=torch.int32, device=device)
    sampled = dict(z=torch.zeros(Bt, 3, **f), xdot_s=torch.zeros(Bt, 3, **f), cbc_s=torch.zeros(Bt, 1 + Kob, **f),
                   viol=torch.zeros(Bt, Kob, **i), solved=torch.zeros(Bt, **i), min_cbc=torch.full((Bt, Kob), float("inf"), **f))
    audit = dict(u_held=torch.zeros(Bt, 2, **f), held=torch.zeros(Bt, **i), held_mean=torch.zeros(Bt, Kob, **f),
                 held_margin=torch.zeros(Bt, Kob, **f), audit_n=torch.zeros(Bt, **i), audit_neg=torch.zeros(Bt, Kob, 2, **i),
                 audit_min=torch.full((Bt, Kob, 2), float("inf"), **f))
    return dict(sampled=sampled, audit=audit)


def trigger_observe_workspace(Bt, rows, dtype, device):
    """The observation stream of `unicycle_trigger_step_prepare(observe=...)` (bcbf_unicycle_trigger_step_observe), as the dict that
    call takes: obs = (X[Bt,rows,3], UH[Bt,rows,3], Y[Bt,rows,3]), ld = rows, row0 = 0, every = 1, xq_next[Bt,3] (zero),
    shift_invariant = True, L_mean = 1.0 -- change row0 / every / L_mean in the dict before binding.  Every row starts as the plant
    AT REST, X = 0, UH = (1, 0, 0), Y = 0: a true, uninformative observation (u = 0 moves nothing), so a row that is never written --
    the instance finished, or its row index is past the stream -- is still a valid training row (U = 0 for the oracle)."""
    f = dict(dtype=dtype, device=device)
    UH = torch.zeros(Bt, rows, 3, **f)
    UH[:, :, 0] = 1
    return dict(obs=(torch.zeros(Bt, rows, 3, **f), UH, torch.zeros(Bt, rows, 3, **f)), ld=int(rows), row0=0, every=1,
                xq_next=torch.zeros(Bt, 3, **f), shift_invariant=True, L_mean=1.0)


def _trigger_want(v, dtype, shape, what):
    """ValueError unless v is a contiguous tensor of this dtype and shape; `what` names it in the message."""
    if v.dtype != dtype or not v.is_contiguous() or tuple(v.shape) != shape:
        raise ValueError("trigger step: %s (%s %s) must be a contiguous %s tensor of shape %s" % (what, v.dtype, tuple(v.shape), dtype, shape))


_TRIGGER_OBSERVE_KEYS = ("obs", "ld", "row0", "every", "xq_next", "shift_invariant", "L_mean")


def _trigger_observe_check(x, observe):
    """Shape and dtype checks (ValueError) of group O; returns ([obs_x, obs_uh, obs_y, xq_next] (None where absent), the entry's
    scalar arguments (L_mean, ld, row0, every, flags))."""
    Bt = x.shape[0]
    unknown = set(observe) - set(_TRIGGER_OBSERVE_KEYS)
    if unknown:
        raise ValueError("trigger step: observe has no key %s" % sorted(unknown))
    obs, xq_next = observe.get("obs"), observe.get("xq_next")
    ld, row0, every = (int(observe.get(k, d)) for k, d in (("ld", 1), ("row0", 0), ("every", 1)))
    L_mean = float(observe.get("L_mean", 1.0))
    if obs is not None:
        if len(obs) != 3 or any(v is None for v in obs):
            raise ValueError("trigger step: observe['obs'] is the three stream buffers (obs_x, obs_uh, obs_y), or None")
        if ld < 1 or row0 < 0 or every < 1:
            raise ValueError("trigger step: observe needs ld >= 1, row0 >= 0, every >= 1 (got %d, %d, %d)" % (ld, row0, every))
        if not (L_mean != 0.0 and L_mean == L_mean):
            raise ValueError("trigger step: observe['L_mean'] must be a number other than 0")
        for name, v in zip(("obs_x", "obs_uh", "obs_y"), obs):
            _trigger_want(v, x.dtype, (Bt, ld, 3), "observe['obs'] %s" % name)
    if xq_next is not None:
        _trigger_want(xq_next, x.dtype, (Bt, 3), "observe['xq_next']")
    tensors = (list(obs) if obs is not None else [None] * 3) + [xq_next]
    return tensors, (L_mean, ld, row0, every, 1 if observe.get("shift_invariant", True) else 0)


_TRIGGER_SAMPLED_KEYS = ("z", "xdot_s", "cbc_s", "viol", "solved", "min_cbc")
_TRIGGER_AUDIT_KEYS = ("u_held", "held", "held_mean", "held_margin", "audit_n", "audit_neg", "audit_min")


def _trigger_audit_check(task, ws, x, gp_A, sampled, audit):
    """Shape and dtype checks (ValueError) of what bcbf_unicycle_trigger_step_audit takes beyond the plain entry; returns the
    tensors in the entry's order: [Bk, A, grad, cst, sign, rho], the six of `sampled`, the seven of `audit` (None where absent)."""
    Bt, Kob = x.shape[0], task["centers"].shape[1]
    if gp_A is None:
        raise ValueError("trigger step: sampled / audit need gp_A, the kernel matrix A[Bt,3,3] (or [1,3,3]) the solve ran with")
    if gp_A.dim() != 3 or tuple(gp_A.shape[1:]) != (3, 3) or gp_A.shape[0] not in (1, Bt):
        raise ValueError("trigger step: gp_A %s must be [Bt, 3, 3] or [1, 3, 3]" % (tuple(gp_A.shape),))
    A = gp_A if gp_A.shape[0] == Bt else gp_A.expand(Bt, 3, 3).contiguous()
    for k, shape in dict(Bk=(Bt, 3, 3), grad=(Bt, 1 + Kob, 3), cst=(Bt, 1 + Kob)).items():
        if tuple(ws[k].shape) != shape:
            raise ValueError("trigger step: ws[%r] %s must be %s" % (k, tuple(ws[k].shape), shape))
    if tuple(task["sign"].shape) != (1 + Kob,) or tuple(task["rho"].shape) != (Bt,):
        raise ValueError("trigger step: task['sign'] must be [1+Kob] and task['rho'] [Bt]")
    ints = ("viol", "solved", "held", "audit_n", "audit_neg")

    def group(d, keys, shapes, required, name):
        if d is None:
            return [None] * len(keys)
        unknown = set(d) - set(keys)
        if unknown:
            raise ValueError("trigger step: %s has no buffer %s" % (name, sorted(unknown)))
        out = []
        for k in keys:
            v = d.get(k)
            if v is None:
                if k in required:
                    raise ValueError("trigger step: %s[%r] is required" % (name, k))
            else:
                _trigger_want(v, torch.int32 if k in ints else x.dtype, shapes[k], "%s[%r]" % (name, k))
            out.append(v)
        return out

    s_shapes = dict(z=(Bt, 3), xdot_s=(Bt, 3), cbc_s=(Bt, 1 + Kob), viol=(Bt, Kob), solved=(Bt,), min_cbc=(Bt, Kob))
    a_shapes = dict(u_held=(Bt, 2), held=(Bt,), held_mean=(Bt, Kob), held_margin=(Bt, Kob), audit_n=(Bt,), audit_neg=(Bt, Kob, 2),
                    audit_min=(Bt, Kob, 2))
    sv = group(sampled, _TRIGGER_SAMPLED_KEYS, s_shapes, ("z",), "sampled")
    if len({v is None for v in sv[3:]}) != 1:
        raise ValueError("trigger step: sampled['viol'], ['solved'], ['min_cbc'] are given together or not at all")
    av = group(audit, _TRIGGER_AUDIT_KEYS, a_shapes, _TRIGGER_AUDIT_KEYS, "audit")
    return [ws["Bk"], A, ws["grad"], ws["cst"], task["sign"], task["rho"]] + sv + av


def unicycle_trigger_step_prepare(task, ws, tws, x, off, r, hyper, plan_all, dplan_all, dt_plan, t_end, tau_min, tau_max,
                                  L_true=1.0, deltaL=1e-4, zeta=1e-2, L_alpha=1.0, stream=None, gp_A=None, sampled=None, audit=None,
                                  observe=None):
    """Bind the buffers of one EVENT of the self-triggered loop once and return `step()` (bcbf_unicycle_trigger_step, one launch):
    run it after the `step()` of `unicycle_control_step_prepare(..., dt=0)` on the same task / ws / x.  It computes the trigger
    time tau of the control in ws['y'] (uBu, xvel, Lh, Lkd, Lfh, tau as `trigger_interval.trigger_interval_batch` does, on the test
    points off[Nte,3] + x), holds the control for dt_b = min(clamp(tau, tau_min, tau_max), t_end - t) on the true plant (unsolved
    instances keep their state and let min(tau_max, t_end - t) pass), advances tws['t'], tws['events'] and copies the planner rows
    of the new time, min(floor(t / dt_plan), P - 1) of plan_all[P,3] / dplan_all[P,3], into task['plan'], task['dot_plan'].
    Instances with t >= t_end are left alone.  hyper = dict(ls[Bh,3], sf[Bh], Adiag[Bh,3], B[Bh,3,3]), Bh = Bt or 1; r = pdist(off)
    (`trigger_interval._grid_norm`); tws from `trigger_workspace`.  The tensors must keep their storage; the closure keeps them.
    sampled / audit (dicts from `trigger_audit_workspace`; either, both or neither) bind bcbf_unicycle_trigger_step_audit instead,
    which also reads the rows of the FUSED solve in ws (Bk, grad, cst), task['sign'], task['rho'] and gp_A, the kernel matrix
    A[Bt,3,3] or [1,3,3] that solve ran with:
    sampled = dict(z[Bt,3], xdot_s | None, cbc_s | None, and viol, solved, min_cbc together | None): the control is held on a
    plant DRAWN FROM THE MODEL'S POSTERIOR, xdot_s = fhat + ghat u + M_k ubar + sqrt(ubar' B_k ubar) chol(A) z (L_true is ignored),
    cbc_s = sign_k (grad_k . xdot_s + cst_k), and the risk counters of `rollout_risk` are kept for the instances that took the event;
    refill `z` in place before every event.
    audit = dict(u_held, held, held_mean, held_margin, audit_n, audit_neg, audit_min), all seven: where the instance's previous
    event was solved, the mean and the margin mean - rho std of every obstacle row's condition under the control of THAT event,
    on this event's rows (the state where the control is released), with counts of negative values and running minima.
    observe = dict(obs=(obs_x, obs_uh, obs_y) | None, ld, row0, every, xq_next | None, shift_invariant, L_mean) (from
    `trigger_observe_workspace`; needs gp_A too, composes with sampled / audit) binds bcbf_unicycle_trigger_step_observe: the loop
    LEARNS FROM ITSELF.  After the plant step the event is written as an observation row -- input = the state before the step,
    (0, 0, theta) when shift_invariant; (1, u); target = (x_new - x_old) / dt_b - g(theta; L_mean) u with the event's own hold dt_b;
    an unsolved instance writes the plant at rest -- into row row0 + e // every of the instance's stream obs_*[Bt, ld, 3], e its
    event count before the event, when e % every == 0 and the row exists (a row past ld is skipped), and the regressor's input
    at the new state into xq_next at every event.  With `sampled` the rows record the drawn plant.
    With none of the three it is the plain entry, unchanged."""
    Bt = x.shape[0]
    more = _trigger_audit_check(task, ws, x, gp_A, sampled, audit) if (sampled is not None or audit is not None or observe is not None) else []
    obs_t, obs_scalars = _trigger_observe_check(x, observe) if observe is not None else ([], ())
    _chk(x, *obs_t)
    ls, sf, Adiag, Bh_ = hyper["ls"], hyper["sf"], hyper["Adiag"], hyper["B"]
    _chk(x, *more)
    _chk(x, off, ls, sf, Adiag, Bh_, plan_all, dplan_all, task["plan"], task["dot_plan"], task["centers"], task["tw"], ws["y"],
         ws["fhat"], ws["ghat"], ws["Mk"], tws["tau"], tws["dt_used"], tws["Lfh"], tws["Lkd"], tws["Lh"], tws["xvel"], tws["uBu"])
    if x.dim() != 2 or x.shape[1] != 3 or off.dim() != 2 or off.shape[1] != 3:
        raise ValueError("trigger step: x %s must be [Bt, 3] and off %s [Nte, 3]" % (tuple(x.shape), tuple(off.shape)))
    Bh = ls.shape[0] if ls.dim() == 2 else -1
    if (tuple(ls.shape), tuple(sf.shape), tuple(Adiag.shape), tuple(Bh_.shape)) != ((Bh, 3), (Bh,), (Bh, 3), (Bh, 3, 3)):
        raise ValueError("trigger step: ls %s, sf %s, Adiag %s, B %s must be [Bh, 3], [Bh], [Bh, 3], [Bh, 3, 3]"
                         % (tuple(ls.shape), tuple(sf.shape), tuple(Adiag.shape), tuple(Bh_.shape)))
    P = plan_all.shape[0]
    if tuple(plan_all.shape) != (P, 3) or tuple(dplan_all.shape) != (P, 3):
        raise ValueError("trigger step: plan_all %s and dplan_all %s must be [P, 3]" % (tuple(plan_all.shape), tuple(dplan_all.shape)))
    Kob = task["centers"].shape[1]
    if tuple(task["centers"].shape) != (Bt, Kob, 2) or task["tw"].numel() != 2:
        raise ValueError("trigger step: centers must be [Bt, Kob, 2] and tw [2]")
    t, events = tws["t"], tws["events"]
    if t.dtype != torch.float64 or events.dtype != torch.int32 or ws["status"].dtype != torch.int32 or not (
            t.is_contiguous() and events.is_contiguous() and t.shape == events.shape == (Bt,)):
        raise ValueError("trigger step: t is a float64 and events an int32 [Bt] tensor")
    for k in ("tau", "dt_used", "Lfh", "Lh", "xvel", "uBu", "Lkd"):
        if tuple(tws[k].shape) != ((Bt, 3) if k == "Lkd" else (Bt,)):
            raise ValueError("trigger step: output buffer %s of the wrong shape" % k)
    entry = "bcbf_unicycle_trigger_step_observe" if observe is not None else ("bcbf_unicycle_trigger_step_audit" if more else "bcbf_unicycle_trigger_step")
    tail, keep_more = tuple(_p(v) for v in more), (tuple(more), tuple(obs_t))
    if observe is not None:
        L_mean, ld, row0, every, flags = obs_scalars
        tail += (L_mean, _p(obs_t[0]), _p(obs_t[1]), _p(obs_t[2]), ld, row0, every, _p(obs_t[3]), flags)
    fn = getattr(lib, entry + _suf(x))
    args = (_p(x), _p(ws["y"]), _p(ws["status"]), _p(ws["fhat"]), _p(ws["ghat"]), _p(ws["Mk"]), _p(task["centers"]), _p(task["tw"]),
            _p(off), float(r), _p(ls), _p(sf), _p(Adiag), _p(Bh_), float(deltaL), float(zeta), float(L_alpha), float(tau_min),
            float(tau_max), float(t_end), float(L_true), _p(plan_all), _p(dplan_all), float(dt_plan), _p(t), _p(events),
            _p(task["plan"]), _p(task["dot_plan"]), _p(tws["tau"]), _p(tws["dt_used"]), _p(tws["Lfh"]), _p(tws["Lkd"]), _p(tws["Lh"]),
            _p(tws["xvel"]), _p(tws["uBu"])) + tail + (Bt, Bh, Kob, off.shape[0], P)
    keep = (dict(task), dict(ws), dict(tws), x, off, dict(hyper), plan_all, dplan_all, stream) + keep_more
    dev = x.device
    fixed = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None

    def step():
        rc = fn(*args, fixed if fixed is not None else ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc:
            raise _lib.BcbfError("%s failed (rc=%d): %s" % (entry, rc, lib.bcbf_last_error().decode()))
        return tws["dt_used"]
    step.keep = keep
    return step


# ---------------------------------------------------------------------------------------------------------------------
# The pendulum's rel-degree-2 safety loop (bcbf_pendulum_control_step_f64): SOCPController(cbfs=[RadialCBFRelDegree2],
# clf=None) with the greedy nominal controller, one host call per step for a batch of pendulums (fp64).
def pendulum_plant_step(x, u, mass=1.0, gravity=10.0, length=1.0, dt=0.002):
    """In-place explicit Euler step of the true pendulum with the theta wrap of PendulumDynamicsModel.step; x[Bt,2], u[Bt,1]."""
    _chk(x, u)
    check(getattr(lib, "bcbf_pendulum_plant_step" + _suf(x))(_p(x), _p(u), mass, gravity, length, dt, x.shape[0],
                                                             _stream(x)), "bcbf_pendulum_plant_step")
    return x


def pendulum_workspace(Bt, dtype=torch.float64, device="cuda"):
    """Caller-owned buffers of `pendulum_control_step` (they also expose the step's intermediates): the jets (Mk, Bk, G, Mj),
    the barrier (h, gh, Hh), the nominal control u_ref, the terms (terms2 = bcbf_cbc2_terms' row, terms = its packed
    (bfe, e, V, bfv, v)), the program (Gc[Bt,6,3], hc[Bt,6], P, q), the solve (y = [y_1, rho, u], sstatus, iters) and the
    outcome (u[Bt,1], status[Bt]: bcbf.h's pendulum status codes)."""
    if dtype != torch.float64:
        raise TypeError("the pendulum control step is fp64 (the reference runs this demo in float64)")
    f = dict(dtype=dtype, device=device)
    i = dict(dtype=torch.int32, device=device)
    return dict(Mk=torch.zeros(Bt, 2, 2, **f), Bk=torch.zeros(Bt, 2, 2, **f), G=torch.zeros(Bt, 6, 6, **f),
                Mj=torch.zeros(Bt, 2, 6, **f), h=torch.empty(Bt, **f), gh=torch.empty(Bt, 2, **f),
                Hh=torch.empty(Bt, 2, 2, **f), u_ref=torch.empty(Bt, 1, **f), terms2=torch.empty(Bt, 7, **f),
                terms=torch.empty(Bt, 1, 5, **f), tstatus=torch.zeros(Bt, **i), Gc=torch.empty(Bt, 6, 3, **f),
                hc=torch.empty(Bt, 6, **f), cstatus=torch.zeros(Bt, 1, **i), P=torch.empty(Bt, 3, 3, **f),
                q=torch.empty(Bt, 3, **f), y=torch.empty(Bt, 3, **f), sstatus=torch.zeros(Bt, **i),
                iters=torch.zeros(Bt, **i), u=torch.empty(Bt, 1, **f), status=torch.zeros(Bt, **i))


def pendulum_control_step_prepare(gp, ws, x, mean_model=None, true_model=(1.0, 10.0, 1.0), dt=0.002,
                                  theta_c=math.pi / 4, delta_c=math.pi / 8, k_alpha=(1.0, 3.0), x_goal=(0.0, 0.0),
                                  Q_goal=((1.0, 0.0), (0.0, 1.0)), R=1.0, u_ref=None, max_unsafe_prob=0.01, ctrl_reg=1.0,
                                  relax_weight=100.0, hessian_mode="reference", max_iters=100, stats=None, stream=None, *,
                                  prior=False, explore=None, eps=0.0, ctrl_range=None, observe=False, sampled=None,
                                  nominal="greedy", numSteps=None, t=0, t_dev=None, lstatus=None, nominal_entry=False):
    """Bind every argument of `bcbf_pendulum_control_step_f64` once and return `step(ev_start=None, ev_stop=None)`.

    gp: dict(Lop, Vw, X, UHB, ell, s2, Bm, M0, A[, kernel]) of a learned model -- a leading axis of 1 on the GP tensors is
    one model shared by every instance (regime S), Bt one model per instance (regime I) -- or None for the no-GP mode
    (the mean model is the whole model; ControlCBFCLFGroundTruth).  mean_model: None (ZeroDynamicsModel) or the pendulum
    (mass, gravity, length) added to the learned mean; true_model: the plant's (mass, gravity, length).  The defaults are
    those of ControlPendulumCBFLearned / run_pendulum_control_online_learning (pendulum.py:909-1048).  u_ref: a [Bt,1]
    tensor read at every step instead of the greedy nominal control.  stats = (min_h[Bt], fails[Bt] int32), updated in
    place.  x[Bt,2] (fp64) advances in place by dt at every step; the tensors must keep their storage.

    The keyword-only options route the step to `bcbf_pendulum_control_step_observe_f64` (the loop that learns online,
    ControlPendulumCBFLearned; without any of them the plain entry runs):
      prior=True: gp is the hyper-parameter dict (ell, s2, Bm, M0, A; leading axis 1 or Bt) of a regressor that holds no
        data, without Lop -- the learned part is its GP prior (Mk = M0', Bk = s2 Bm, G = Mj = 0, cbc2.posterior_for);
      explore=[Bt,2] uniform draws (coin, action), eps, ctrl_range=(lo, hi): the epsilon-greedy wrapper around the greedy
        u_ref (EpsilonGreedyController: the action lo + a (hi - lo) where coin < eps, then clipped to ctrl_range);
        ctrl_range alone clips;
      observe=True: the step writes its observation row (x_t, (1, u_t), (x_{t+1} - x_t)/dt - mean) where the call says.
    With any of them the returned step is `step(ev_start=None, ev_stop=None, eps=None, explore=None, obs=None)`: eps and
    explore replace the bound ones for this call (eps varies per step), obs = (obs_x, obs_uh, obs_y, ld) are [.,2] tensors
    whose row b * ld is instance b's (ld = 1: [Bt,2] tensors; a column t of [Bt,T,2] stream buffers: ld = T).

    sampled = dict(z=[Bt,2,4], xdot_s=[Bt,2] | None, cbc_s=[Bt,2] | None[, relaxed=[Bt] int32, viol_relaxed=[Bt] int32,
    rho_tol=1e-6]): the plant is DRAWN FROM THE MODEL'S POSTERIOR (bcbf_pendulum_control_step_sampled_f64; composes with every
    option above, the same `step` signature).  The four jet columns the condition reads are drawn as mean + L_A z L_Sigma4' from
    the caller's standard normals z (read at every call: refill the tensor between steps), every instance advances by
    xdot_s = f_s + g_s u dt on the draw -- true_model is ignored -- and cbc_s = (L_f h, CBC2) on the same draw at the applied
    control is what `rollout_risk` counts.  relaxed / viol_relaxed (together) count the solved steps whose slack rho = y[1]
    exceeds rho_tol and the violations among them.  The observation rows then record the sampled plant.

    nominal="lqr" (with numSteps; t=0 or t_dev, an int32 device tensor [1] the kernel reads; lstatus[Bt] int32, allocated when
    None and returned as step.lstatus): the nominal control is the reference's LQRController (`lqr_nominal`, horizon
    max(numSteps - t, 1)) on the mean-shifted jets instead of GreedyController, then explore and clip as above
    (bcbf_pendulum_control_step_nominal_f64; composes with every option, excludes u_ref).  The step takes `t=` per call.
    nominal_entry=True runs nominal="greedy" through that entry too (nominal = 0: the observing / sampled entry bit for bit)."""
    from .cbc2 import cbc2_safety_factor
    Bt = x.shape[0]
    f = dict(dtype=x.dtype, device=x.device)
    if x.dtype != torch.float64:
        raise TypeError("the pendulum control step is fp64")
    if nominal not in ("greedy", "lqr"):
        raise ValueError("nominal must be 'greedy' or 'lqr', got %r" % (nominal,))
    nom = None
    if nominal == "lqr":
        if numSteps is None or u_ref is not None:
            raise ValueError("nominal='lqr' needs numSteps (the LQR horizon) and excludes a caller's u_ref")
        if lstatus is None:
            lstatus = torch.zeros(Bt, dtype=torch.int32, device=x.device)
        for name, v, size in (("t_dev", t_dev, 1), ("lstatus", lstatus, Bt)):
            if v is not None and (v.dtype != torch.int32 or v.device != x.device or v.numel() != size or not v.is_contiguous()):
                raise ValueError("%s must be a contiguous int32 tensor of %d element(s) on x's device" % (name, size))
        nom = dict(code=1, numSteps=int(numSteps), t=int(t), t_dev=t_dev, lstatus=lstatus)
    elif nominal_entry:            # the greedy controller through the nominal entry (bit for bit the observing / sampled entry)
        nom = dict(code=0, numSteps=1, t=0, t_dev=None, lstatus=None)
    learn = bool(prior) or explore is not None or ctrl_range is not None or bool(observe) or sampled is not None or nom is not None
    if prior and (gp is None or gp.get("Lop") is not None):
        raise ValueError("prior=True takes the hyper-parameters (ell, s2, Bm, M0, A) of a regressor without data, no Lop")
    if prior:                      # a regressor with no data: its GP prior, with its own hyper-parameters per instance
        gp = {k: (gp[k] if gp[k].shape[0] == Bt else gp[k].expand(Bt, *gp[k].shape[1:])).contiguous()
              for k in ("ell", "s2", "Bm", "M0", "A")}
        _chk(x, gp["M0"])
        gp.update(Lop=None, Vw=None, X=None, UHB=None)
        N, shared, kernel = 0, 0, "rbf"
    elif gp is None:               # no learned model: s2 = 0 removes every variance term of the rel-degree-2 terms
        gp = dict(Lop=None, Vw=None, X=None, UHB=None, M0=None, ell=torch.ones(Bt, 2, **f), s2=torch.zeros(Bt, **f),
                  Bm=torch.eye(2, **f).expand(Bt, 2, 2).contiguous(), A=torch.eye(2, **f).expand(Bt, 2, 2).contiguous())
        N, shared, kernel = 0, 0, "rbf"
    else:
        _chk(x, gp["Lop"], gp["Vw"], gp["X"], gp["UHB"], gp["M0"])
        N = gp["X"].shape[1]
        shared = 1 if gp["X"].shape[0] == 1 else 0
        if not shared and gp["X"].shape[0] != Bt:
            raise ValueError("GP tensors must carry a leading axis of 1 (shared model) or Bt")
        kernel = gp.get("kernel", "rbf")
        if kernel not in DATA_KERNELS:
            raise ValueError("gp['kernel'] must be one of %s" % (DATA_KERNELS,))
        gp = dict(gp)
        for k in ("ell", "s2", "Bm", "A"):                   # the terms kernel reads these per instance
            v = gp[k]
            if v.shape[0] != Bt:
                gp[k] = v.expand(Bt, *v.shape[1:]).contiguous()
    _chk(x, gp["ell"], gp["s2"], gp["Bm"], gp["A"], ws["Mk"], ws["y"], u_ref)
    kalpha = torch.tensor(k_alpha, **f)
    xg = (ctypes.c_double * 2)(*[float(v) for v in x_goal])
    Qg = (ctypes.c_double * 4)(*[float(v) for row in Q_goal for v in row])
    mm = (0, 1.0, 1.0, 1.0) if mean_model is None else (1,) + tuple(float(v) for v in mean_model)
    min_h, fails = stats if stats is not None else (None, None)
    if stats is not None:
        _chk(x, min_h, fails)
    head = (_p(gp["Lop"]), _p(gp["Vw"]), _p(gp["X"]), _p(gp["UHB"]), _p(gp["ell"]), _p(gp["s2"]), _p(gp["Bm"]),
            _p(gp["M0"]), _p(gp["A"]), N, shared, DATA_KERNELS.index(kernel), mm[0], mm[1], mm[2], mm[3], float(theta_c),
            float(delta_c), _p(kalpha), xg, Qg, float(R), _p(u_ref), cbc2_safety_factor(max_unsafe_prob), float(ctrl_reg),
            float(relax_weight), HESSIAN_MODES[hessian_mode], int(max_iters), float(true_model[0]), float(true_model[1]),
            float(true_model[2]), float(dt), _p(x)) + tuple(
        _p(ws[k]) for k in ("Mk", "Bk", "G", "Mj", "h", "gh", "Hh", "u_ref", "terms2", "terms", "tstatus", "Gc", "hc",
                            "cstatus", "P", "q", "y", "sstatus", "iters", "u", "status")) + (_p(min_h), _p(fails))
    keep = (gp, dict(ws), x, kalpha, xg, Qg, u_ref, stats, stream)      # the pointers above live as long as these
    if learn:
        return _pendulum_observe_step(head, keep, x, ws["u"], stream, prior, explore, eps, ctrl_range, u_ref, sampled, nom)
    call = _bind_call(lib.bcbf_pendulum_control_step_f64, "bcbf_pendulum_control_step", x, stream, ws["u"])
    args = head + (Bt, 2, 1)

    def step(ev_start=None, ev_stop=None):
        return call(ev_start, ev_stop, args)
    step.keep = keep
    return step


def _pendulum_sampled_args(x, sampled):
    """`pendulum_control_step_prepare(sampled=...)` checked, as the entry's (z, xdot_s, cbc_s, relaxed, viol_relaxed, rho_tol)."""
    Bt = x.shape[0]
    z, xdot_s, cbc_s = sampled["z"], sampled.get("xdot_s"), sampled.get("cbc_s")
    relaxed, viol_relaxed = sampled.get("relaxed"), sampled.get("viol_relaxed")
    _chk(x, z, xdot_s, cbc_s)
    if z is None or tuple(z.shape) != (Bt, 2, 4):
        raise ValueError("sampled['z'] must be a [Bt,2,4] tensor of standard-normal draws")
    if any(v is not None and tuple(v.shape) != (Bt, 2) for v in (xdot_s, cbc_s)):
        raise ValueError("sampled['xdot_s'] and sampled['cbc_s'] are [Bt,2]")
    if (relaxed is None) != (viol_relaxed is None):
        raise ValueError("sampled['relaxed'] and sampled['viol_relaxed'] are given together or not at all")
    for v in (relaxed, viol_relaxed):
        if v is not None and (v.dtype != torch.int32 or tuple(v.shape) != (Bt,) or v.device != x.device or not v.is_contiguous()):
            raise ValueError("sampled['relaxed'] and sampled['viol_relaxed'] are contiguous int32 [Bt] tensors on x's device")
    return (_p(z), _p(xdot_s), _p(cbc_s), _p(relaxed), _p(viol_relaxed), float(sampled.get("rho_tol", 1e-6)))


def _pendulum_observe_step(head, keep, x, out, stream, prior, explore, eps, ctrl_range, u_ref, sampled=None, nom=None):
    """The step of `pendulum_control_step_prepare` on bcbf_pendulum_control_step_observe_f64 (head: the arguments every entry
    takes, up to `fails`), or with `sampled` on bcbf_pendulum_control_step_sampled_f64, or with `nom` (the LQR nominal
    controller's numSteps, t, t_dev, lstatus) on bcbf_pendulum_control_step_nominal_f64."""
    if explore is not None and u_ref is not None:
        raise ValueError("explore wraps the greedy u_ref; it cannot be combined with a caller's u_ref")
    _chk(x, explore)
    rng = None if ctrl_range is None else (ctypes.c_double * 2)(*[float(v) for v in ctrl_range])
    Bt, what, draw = x.shape[0], "bcbf_pendulum_control_step_observe", ()
    if sampled is not None:
        what, draw = "bcbf_pendulum_control_step_sampled", _pendulum_sampled_args(x, sampled)
    if nom is not None:
        what, draw = "bcbf_pendulum_control_step_nominal", draw or (None, None, None, None, None, 1e-6)
    call = _bind_call(getattr(lib, what + "_f64"), what, x, stream, out)
    bound = dict(eps=float(eps), explore=explore)
    keep = keep + (rng, explore, None if sampled is None else dict(sampled), nom)

    def step(ev_start=None, ev_stop=None, eps=None, explore=None, obs=None, t=None):
        ex = bound["explore"] if explore is None else explore
        if explore is not None:
            _chk(x, explore)
        o = (None, None, None, 1) if obs is None else (_p(obs[0]), _p(obs[1]), _p(obs[2]), int(obs[3]))
        lq = () if nom is None else (nom["code"], nom["numSteps"], nom["t"] if t is None else int(t), _p(nom["t_dev"]), _p(nom["lstatus"]))
        return call(ev_start, ev_stop, (*head, 1 if prior else 0, _p(ex), float(bound["eps"] if eps is None else eps), rng, *o, *draw,
                                        *lq, Bt, 2, 1))
    step.keep = keep
    step.lstatus = None if nom is None else nom["lstatus"]
    return step


def pendulum_control_step(gp, ws, x, **kw):
    """One control step of the pendulum safety filter for a batch (see `pendulum_control_step_prepare`); returns ws['u']."""
    return pendulum_control_step_prepare(gp, ws, x, **kw)()


# ---------------------------------------------------------------------------------------------------------------------
# The reference's LQR nominal controller (bcbf_lqr_nominal_*: LQRController.control, controllers.py:64-115), batched.
def lqr_nominal(Mk, Mj, x, x_goal, Q, R, dt, numSteps, t=0, t_dev=None, want_u0=False, out=None):
    """LQRController.control for a batch: Mk[Bt,n,1+m] and Mj[Bt,n,(1+m)(1+n)] in the jets' layout (`posterior_jets`; g and the
    x-Jacobians of f and g are read, f is not), x[Bt,n]; x_goal[n], Q[n,n], R[m,m] host values (sequences / CPU tensors).  Two
    backward passes of T = max(numSteps - t, 1) iterations of the recursion of affine_backpropagation (ilqr.py:43-76), the second
    linearised at the first's control; t_dev (an int32 device tensor [1]) replaces t and is read by the kernel, so a captured
    graph can replay a shrinking horizon.  ctrl_range is not applied (the reference's LQR does not clip).
    Returns (u[Bt,m], status[Bt]) or (u, u0, status) with want_u0; status 1 = some R + B'PB had a pivot that is not > 0 (u = u0 =
    0 there).  out = (u, u0 | None, status) reuses the caller's buffers."""
    _chk(x, Mk, Mj)
    Bt, n = x.shape
    m = Mk.shape[2] - 1 if Mk.dim() == 3 else -1
    if x.dim() != 2 or tuple(Mk.shape) != (Bt, n, 1 + m) or tuple(Mj.shape) != (Bt, n, (1 + m) * (1 + n)):
        raise ValueError("lqr_nominal: x %s must be [Bt,n], Mk %s [Bt,n,1+m] and Mj %s [Bt,n,(1+m)(1+n)]"
                         % (tuple(x.shape), tuple(Mk.shape), tuple(Mj.shape)))
    ct = ctypes.c_float if x.dtype == torch.float32 else ctypes.c_double
    host = []
    for name, v, size in (("x_goal", x_goal, n), ("Q", Q, n * n), ("R", R, m * m)):
        flat = [float(e) for e in torch.as_tensor(v, dtype=torch.float64).reshape(-1).tolist()]
        if len(flat) != size:
            raise ValueError("lqr_nominal: %s must hold %d values, got %d" % (name, size, len(flat)))
        host.append((ct * size)(*flat))
    if t_dev is not None and (t_dev.dtype != torch.int32 or t_dev.device != x.device or t_dev.numel() < 1):
        raise ValueError("lqr_nominal: t_dev is an int32 tensor on x's device")
    if out is None:
        out = (torch.empty(Bt, m, dtype=x.dtype, device=x.device),
               torch.empty(Bt, m, dtype=x.dtype, device=x.device) if want_u0 else None,
               torch.empty(Bt, dtype=torch.int32, device=x.device))
    u, u0, status = out
    _chk(x, u, u0, status)
    check(getattr(lib, "bcbf_lqr_nominal" + _suf(x))(_p(Mk), _p(Mj), _p(x), *host, float(dt), int(numSteps), int(t), _p(t_dev),
                                                    _p(u), _p(u0), _p(status), Bt, n, m, _stream(x)), "bcbf_lqr_nominal")
    return (u, u0, status) if want_u0 else (u, status)


# ---------------------------------------------------------------------------------------------------------------------
# The pendulum's CLF-CBF quadratic program on the known model (bcbf_pendulum_clf_cbf_control / _rollout):
# PendulumCBFCLFDirect, the controller the Bayesian one is measured against.  fp32 and fp64.
_PENDULUM_CBF_KINDS = {"reldeg2": 0, "radial": 1, 0: 0, 1: 1}


def _pendulum_model_rows(model, Bt, like, what):
    """(tensor, stride) of a pendulum model for the library: a (mass, gravity, length) triple or a tensor[3] is one shared
    row (stride 0), a tensor[Bt,3] one row per instance (stride 3)."""
    if not torch.is_tensor(model):
        model = torch.tensor([float(v) for v in model], dtype=like.dtype, device=like.device)
    if model.dtype != like.dtype or model.device != like.device or not model.is_contiguous():
        raise TypeError("%s must be a contiguous %s tensor on %s" % (what, like.dtype, like.device))
    if tuple(model.shape) == (3,):
        return model, 0
    if tuple(model.shape) == (Bt, 3):
        return model, 3
    raise ValueError("%s must be (mass, gravity, length), a tensor[3] or a tensor[Bt,3]; got %s" % (what, tuple(model.shape)))


def _pendulum_qp_task(x, clf_c, k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight):
    ct = ctypes.c_float if x.dtype == torch.float32 else ctypes.c_double
    try:
        kind = _PENDULUM_CBF_KINDS[cbf_kind]
    except KeyError:
        raise ValueError("cbf_kind must be 'reldeg2' (0) or 'radial' (1), got %r" % (cbf_kind,))
    return [clf_c, (ct * 2)(float(k_alpha[0]), float(k_alpha[1])), theta_c, delta_c, cbf_gamma, kind, slack_weight]


def pendulum_clf_cbf_control(x, ctrl_model=(1.0, 10.0, 1.0), clf_c=1.0, k_alpha=(1.0, 3.0), theta_c=math.pi / 4,
                             delta_c=math.pi / 8, cbf_gamma=1.0, cbf_kind="reldeg2", slack_weight=100.0):
    """One evaluation of the pendulum's CLF-CBF controller on a known model for a batch of states x[Bt,2]: the rows of
    EnergyCLF (relaxed, slack weight `slack_weight`) and of RadialCBFRelDegree2 (cbf_kind 'reldeg2') or RadialCBF ('radial'),
    and the optimum of control_QP_cbf_clf in closed form.  ctrl_model: (mass, gravity, length) or a tensor[Bt,3].
    Returns dict(A[Bt,2], b[Bt,2], values[Bt,2] = (V, h), u[Bt], rho[Bt], status[Bt]); status 1 = the program is
    infeasible (u, rho are then NaN: the library leaves them unwritten)."""
    _chk(x)
    Bt = x.shape[0]
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("x must be [Bt,2]")
    cm, cs = _pendulum_model_rows(ctrl_model, Bt, x, "ctrl_model")
    out = dict(A=torch.empty(Bt, 2, dtype=x.dtype, device=x.device), b=torch.empty(Bt, 2, dtype=x.dtype, device=x.device),
               values=torch.empty(Bt, 2, dtype=x.dtype, device=x.device),
               u=torch.full((Bt,), float("nan"), dtype=x.dtype, device=x.device),
               rho=torch.full((Bt,), float("nan"), dtype=x.dtype, device=x.device),
               status=torch.zeros(Bt, dtype=torch.int32, device=x.device))
    task = _pendulum_qp_task(x, clf_c, k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight)
    check(getattr(lib, "bcbf_pendulum_clf_cbf_control" + _suf(x))(
        _p(x), _p(cm), cs, *task, _p(out["A"]), _p(out["b"]), _p(out["values"]), _p(out["u"]), _p(out["rho"]),
        _p(out["status"]), Bt, _stream(x)), "bcbf_pendulum_clf_cbf_control")
    return out


def pendulum_clf_cbf_records(t_offset, numSteps, record_every):
    """How many of the global steps t_offset .. t_offset + numSteps - 1 are multiples of record_every (0: none recorded)."""
    if record_every <= 0:
        return 0
    first = -(-t_offset // record_every)
    last = -(-(t_offset + numSteps) // record_every)
    return last - first


def pendulum_clf_cbf_rollout(x, min_h, damage, status, numSteps, dt=0.002, ctrl_model=(1.0, 10.0, 1.0), true_model=None,
                             clf_c=1.0, k_alpha=(1.0, 3.0), theta_c=math.pi / 4, delta_c=math.pi / 8, cbf_gamma=1.0,
                             cbf_kind="reldeg2", slack_weight=100.0, traj=None, u_rec=None, record_every=0, t_offset=0):
    """numSteps steps of the closed loop (controller of `pendulum_clf_cbf_control` on ctrl_model, explicit Euler on the plant
    true_model -- None: the controller's model) for every instance in ONE launch.  In place: x[Bt,2], min_h[Bt],
    damage[Bt] (int32), status[Bt] (int32; the 1-based global step t_offset + t + 1 at which an instance's program became
    infeasible -- it is frozen from there on).  Calls compose bit for bit (the second with t_offset = the steps done).
    traj[r,Bt,2] / u_rec[r,Bt]: (x_t, u_t) of the global steps that are multiples of record_every, this call's first at
    row 0; r = pendulum_clf_cbf_records(t_offset, numSteps, record_every).  Returns x."""
    _chk(x, min_h, damage, status, traj, u_rec)
    Bt = x.shape[0]
    if x.ndim != 2 or x.shape[1] != 2 or tuple(min_h.shape) != (Bt,) or min_h.dtype != x.dtype:
        raise ValueError("x must be [Bt,2] and min_h [Bt] of the same dtype")
    for name, t in (("damage", damage), ("status", status)):
        if tuple(t.shape) != (Bt,) or t.dtype != torch.int32:
            raise ValueError("%s must be an int32 tensor [Bt]" % name)
    cm, cs = _pendulum_model_rows(ctrl_model, Bt, x, "ctrl_model")
    tm, ts = (cm, cs) if true_model is None else _pendulum_model_rows(true_model, Bt, x, "true_model")
    nrec = pendulum_clf_cbf_records(t_offset, numSteps, record_every)
    for name, t, shape in (("traj", traj, (Bt, 2)), ("u_rec", u_rec, (Bt,))):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape[1:]) != shape or t.shape[0] < nrec):
            raise ValueError("%s must be a %s tensor [>= %d, %s]" % (name, x.dtype, nrec, ", ".join(map(str, shape))))
    task = _pendulum_qp_task(x, clf_c, k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight)
    check(getattr(lib, "bcbf_pendulum_clf_cbf_rollout" + _suf(x))(
        _p(x), _p(cm), cs, _p(tm), ts, *task, dt, _p(min_h), _p(damage), _p(status), _p(traj), _p(u_rec), record_every,
        t_offset, numSteps, Bt, _stream(x)), "bcbf_pendulum_clf_cbf_rollout")
    return x


# ---------------------------------------------------------------------------------------------------------------------
# The unicycle's CLF-CBF quadratic program on the mean model (bcbf_clf_cbf_qp2 / bcbf_unicycle_clf_cbf_control / _rollout):
# ControllerCLF, the controller the Bayesian one is measured against.  fp32 and fp64.
_UNICYCLE_CLF_KINDS = {"cartesian": 0, "polar": 1, 0: 0, 1: 1}
_UNICYCLE_PLANNER_KINDS = {"none": 0, "piecewise": 1, 0: 0, 1: 1}
UNICYCLE_CTRL_MIN, UNICYCLE_CTRL_MAX = (-10.0, -5 * math.pi), (10.0, 5 * math.pi)


def _host(like, values, n, what):
    """A host array of the tensor's precision (the library's HOST-pointer arguments)."""
    ct = ctypes.c_float if like.dtype == torch.float32 else ctypes.c_double
    values = [float(v) for v in (values.tolist() if torch.is_tensor(values) else values)]
    if len(values) != n:
        raise ValueError("%s must have %d values, got %d" % (what, n, len(values)))
    return (ct * max(n, 1))(*values)


def _unicycle_scalar_rows(v, Bt, like, what):
    """(tensor, stride) of a wheelbase for the library: a number or a tensor[1] is shared (stride 0), a tensor[Bt] one value
    per instance (stride 1)."""
    if not torch.is_tensor(v):
        v = torch.tensor([float(v)], dtype=like.dtype, device=like.device)
    if v.dtype != like.dtype or v.device != like.device or not v.is_contiguous():
        raise TypeError("%s must be a contiguous %s tensor on %s" % (what, like.dtype, like.device))
    if v.numel() == 1 and v.ndim <= 1:
        return v.reshape(1), 0
    if tuple(v.shape) == (Bt,):
        return v, 1
    raise ValueError("%s must be a number, a tensor[1] or a tensor[Bt]; got %s" % (what, tuple(v.shape)))


def _unicycle_obstacles(centers, radii, Bt, like):
    """(centers, radii, stride, Kob): centers[Kob,2] / radii[Kob] shared (stride 0) or centers[Bt,Kob,2] / radii[Bt,Kob] per
    instance (stride 1); None: no obstacles."""
    if centers is None or radii is None:
        if centers is not None or radii is not None:
            raise ValueError("centers and radii come together")
        return None, None, 0, 0
    for name, t in (("centers", centers), ("radii", radii)):
        if t.dtype != like.dtype or t.device != like.device or not t.is_contiguous():
            raise TypeError("%s must be a contiguous %s tensor on %s" % (name, like.dtype, like.device))
    if centers.ndim == 2 and centers.shape[1] == 2 and tuple(radii.shape) == (centers.shape[0],):
        return centers, radii, 0, centers.shape[0]
    if centers.ndim == 3 and centers.shape[0] == Bt and centers.shape[2] == 2 and tuple(radii.shape) == tuple(centers.shape[:2]):
        return centers, radii, 1, centers.shape[1]
    raise ValueError("obstacles must be centers[Kob,2] / radii[Kob] or centers[Bt,Kob,2] / radii[Bt,Kob]; got %s / %s"
                     % (tuple(centers.shape), tuple(radii.shape)))


def _unicycle_qp_task(x, Kp, clf_kind, clf_gamma, relax_weight, lo, hi, L_ctrl, centers, radii, tw, gammas):
    """The task arguments of the control / rollout entries from `Kp` to `gammas`, in the library's order, and Kob."""
    Bt = x.shape[0]
    try:
        kind = _UNICYCLE_CLF_KINDS[clf_kind]
    except KeyError:
        raise ValueError("clf_kind must be 'cartesian' (0) or 'polar' (1), got %r" % (clf_kind,))
    Kp = list(Kp.tolist() if torch.is_tensor(Kp) else Kp)
    Kp = Kp + [0.0] * (4 - len(Kp))                      # CLFCartesian has three gains
    Lc, Ls = _unicycle_scalar_rows(L_ctrl, Bt, x, "L_ctrl")
    centers, radii, ostride, Kob = _unicycle_obstacles(centers, radii, Bt, x)
    gam = list(gammas.tolist() if torch.is_tensor(gammas) else gammas) if Kob else []
    args = [_host(x, Kp, 4, "Kp"), kind, clf_gamma, relax_weight, _host(x, lo, 2, "lo"), _host(x, hi, 2, "hi"), _p(Lc), Ls,
            _p(centers), _p(radii), ostride, _host(x, tw, 2, "tw") if Kob else None,
            _host(x, gam, Kob, "gammas") if Kob else None]
    return args, Kob, (Lc, centers, radii)


def clf_cbf_qp2(a, b, lo=UNICYCLE_CTRL_MIN, hi=UNICYCLE_CTRL_MAX, relax_weight=10.0, want=("u", "relax", "active", "status")):
    """The program  min |u|^2 + relax_weight relax  s.t.  lo <= u <= hi,  a[:,0].u + b[:,0] - relax <= 0,  a[:,k].u + b[:,k] >= 0
    (k >= 1)  for a batch: a[Bt,K,2], b[Bt,K], 1 <= K <= 4.  The unique optimum in closed form (projection of
    -(relax_weight/2) a_0 onto the polygon, active sets of size <= 2 enumerated).
    Returns dict(u[Bt,2], relax[Bt], active[Bt] (int32 bitmask over lo0, lo1, hi0, hi1, hard rows), status[Bt]) of the outputs
    named in `want`; status 1 = infeasible (u, relax are then NaN and active -1: the library leaves them unwritten)."""
    _chk(a, b)
    if a.ndim != 3 or a.shape[2] != 2 or tuple(b.shape) != tuple(a.shape[:2]):
        raise ValueError("a must be [Bt,K,2] and b [Bt,K]")
    Bt, K = b.shape
    out = _unicycle_qp_outputs(a, Bt, want)
    check(getattr(lib, "bcbf_clf_cbf_qp2" + _suf(a))(
        _p(a), _p(b), _host(a, lo, 2, "lo"), _host(a, hi, 2, "hi"), relax_weight, _p(out.get("u")), _p(out.get("relax")),
        _p(out.get("active")), _p(out.get("status")), Bt, K, _stream(a)), "bcbf_clf_cbf_qp2")
    return out


def _unicycle_qp_outputs(like, Bt, want, K=None):
    f = dict(dtype=like.dtype, device=like.device)
    make = dict(a=lambda: torch.empty(Bt, K, 2, **f), b=lambda: torch.empty(Bt, K, **f), values=lambda: torch.empty(Bt, K, **f),
                u=lambda: torch.full((Bt, 2), float("nan"), **f), relax=lambda: torch.full((Bt,), float("nan"), **f),
                active=lambda: torch.full((Bt,), -1, dtype=torch.int32, device=like.device),
                status=lambda: torch.zeros(Bt, dtype=torch.int32, device=like.device))
    unknown = [w for w in want if w not in make or (K is None and w in ("a", "b", "values"))]
    if unknown:
        raise ValueError("unknown outputs %s" % unknown)
    return {w: make[w]() for w in want}


def unicycle_clf_cbf_control(x, plan, dot_plan, Kp=(0.9, 1.5, 4.0), clf_kind="cartesian", clf_gamma=10.0, relax_weight=10.0,
                             lo=UNICYCLE_CTRL_MIN, hi=UNICYCLE_CTRL_MAX, L_ctrl=1.0, centers=None, radii=None, tw=(0.5, 0.5),
                             gammas=(), want=("a", "b", "values", "u", "relax", "active", "status")):
    """One evaluation of the unicycle's mean-model CLF-CBF controller (ControllerCLF.control) for a batch of states x[Bt,3]
    with plan[Bt,3], dot_plan[Bt,3]: the rows of CLFCartesian + ObstacleCBF on AckermannDrive(L_ctrl) (clf_kind 'cartesian')
    or of CLFPolar on PolarDynamics through cartesian2polar ('polar', no obstacles), and the optimum of the program in closed
    form.  L_ctrl: a number or a tensor[Bt]; obstacles: centers[Kob,2] / radii[Kob] shared or [Bt,Kob,2] / [Bt,Kob] per instance.
    Returns dict(a[Bt,1+Kob,2], b[Bt,1+Kob], values[Bt,1+Kob] = (V, h_k), u[Bt,2], relax[Bt], active[Bt], status[Bt]) of the
    outputs named in `want`; status 1 = infeasible (u, relax NaN, active -1)."""
    _chk(x, plan, dot_plan)
    Bt = x.shape[0]
    if x.ndim != 2 or x.shape[1] != 3 or tuple(plan.shape) != (Bt, 3) or tuple(dot_plan.shape) != (Bt, 3):
        raise ValueError("x, plan and dot_plan must be [Bt,3]")
    task, Kob, keep = _unicycle_qp_task(x, Kp, clf_kind, clf_gamma, relax_weight, lo, hi, L_ctrl, centers, radii, tw, gammas)
    out = _unicycle_qp_outputs(x, Bt, want, 1 + Kob)
    check(getattr(lib, "bcbf_unicycle_clf_cbf_control" + _suf(x))(
        _p(x), _p(plan), _p(dot_plan), *task, _p(out.get("a")), _p(out.get("b")), _p(out.get("values")), _p(out.get("u")),
        _p(out.get("relax")), _p(out.get("active")), _p(out.get("status")), Bt, Kob, _stream(x)),
        "bcbf_unicycle_clf_cbf_control")
    return out


def unicycle_clf_cbf_records(t_offset, numSteps, record_every):
    """How many of the global steps t_offset .. t_offset + numSteps - 1 are multiples of record_every (0: none recorded)."""
    return pendulum_clf_cbf_records(t_offset, numSteps, record_every)


def unicycle_planner_steps(numStepsPlan, frac_time_to_reach_goal=0.7):
    """(t2, lookahead) of PiecewiseLinearPlanner(numStepsPlan, ., frac) as planner.py computes them: the integers the
    rollout entry takes from the host."""
    return min(int(numStepsPlan * frac_time_to_reach_goal), numStepsPlan - 1), max(int(0.1 * numStepsPlan), 1)


def unicycle_clf_cbf_rollout(x, goal, cost, status, numSteps, dt=0.05, min_h=None, converged_at=None, planner="none",
                             x0_plan=None, numStepsPlan=0, frac_time_to_reach_goal=0.7, Kp=(0.9, 1.5, 4.0),
                             clf_kind="cartesian", clf_gamma=10.0, relax_weight=10.0, lo=UNICYCLE_CTRL_MIN,
                             hi=UNICYCLE_CTRL_MAX, L_ctrl=1.0, L_true=None, centers=None, radii=None, tw=(0.5, 0.5), gammas=(),
                             stop_rho=0.0, traj=None, u_rec=None, record_every=0, t_offset=0):
    """numSteps steps of the closed loop (controller of `unicycle_clf_cbf_control` on L_ctrl, explicit Euler on the plant's
    wheelbase L_true -- None: the controller's) for every instance in ONE launch.  planner 'none': plan = goal[Bt,3];
    'piecewise': PiecewiseLinearPlanner(x0_plan[Bt,3], goal, numStepsPlan, dt, frac_time_to_reach_goal) evaluated inside the
    kernel at the global step.  In place: x[Bt,3], min_h[Bt] (needed with obstacles), cost[Bt] (sum |u|^2), status[Bt] (int32;
    the 1-based global step at which an instance's program became infeasible -- it is frozen from there on), converged_at[Bt]
    (int32, -1 = running; needed with stop_rho > 0: the global step before which |goal - x| < stop_rho, the instance stops
    there).  Calls compose bit for bit (the second with t_offset = the steps done).  traj[r,Bt,3] / u_rec[r,Bt,2]: (x_t, u_t)
    of the global steps that are multiples of record_every, this call's first at row 0;
    r = unicycle_clf_cbf_records(t_offset, numSteps, record_every).  Returns x."""
    _chk(x, goal, cost, status, min_h, converged_at, x0_plan, traj, u_rec)
    Bt = x.shape[0]
    if x.ndim != 2 or x.shape[1] != 3 or tuple(goal.shape) != (Bt, 3) or goal.dtype != x.dtype:
        raise ValueError("x and goal must be [Bt,3] of the same dtype")
    for name, t in (("cost", cost), ("min_h", min_h)):
        if t is not None and (tuple(t.shape) != (Bt,) or t.dtype != x.dtype):
            raise ValueError("%s must be a %s tensor [Bt]" % (name, x.dtype))
    for name, t in (("status", status), ("converged_at", converged_at)):
        if t is not None and (tuple(t.shape) != (Bt,) or t.dtype != torch.int32):
            raise ValueError("%s must be an int32 tensor [Bt]" % name)
    try:
        pkind = _UNICYCLE_PLANNER_KINDS[planner]
    except KeyError:
        raise ValueError("planner must be 'none' (0) or 'piecewise' (1), got %r" % (planner,))
    t2 = look = 0
    if pkind == 1:
        if x0_plan is None or tuple(x0_plan.shape) != (Bt, 3) or x0_plan.dtype != x.dtype:
            raise ValueError("planner 'piecewise' needs x0_plan [Bt,3]")
        t2, look = unicycle_planner_steps(int(numStepsPlan), frac_time_to_reach_goal)
    task, Kob, keep = _unicycle_qp_task(x, Kp, clf_kind, clf_gamma, relax_weight, lo, hi, L_ctrl, centers, radii, tw, gammas)
    Lt, Lts = (keep[0], task[7]) if L_true is None else _unicycle_scalar_rows(L_true, Bt, x, "L_true")
    nrec = unicycle_clf_cbf_records(t_offset, numSteps, record_every)
    for name, t, shape in (("traj", traj, (Bt, 3)), ("u_rec", u_rec, (Bt, 2))):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape[1:]) != shape or t.shape[0] < nrec):
            raise ValueError("%s must be a %s tensor [>= %d, %s]" % (name, x.dtype, nrec, ", ".join(map(str, shape))))
    check(getattr(lib, "bcbf_unicycle_clf_cbf_rollout" + _suf(x))(
        _p(x), _p(goal), _p(x0_plan), pkind, t2, look, int(numStepsPlan), *task[:8], _p(Lt), Lts, *task[8:], dt, stop_rho,
        _p(min_h), _p(cost), _p(status), _p(converged_at), _p(traj), _p(u_rec), record_every, t_offset, numSteps, Bt, Kob,
        _stream(x)), "bcbf_unicycle_clf_cbf_rollout")
    return x
