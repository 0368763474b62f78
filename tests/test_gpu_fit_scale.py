"""The batched-fit kernels (bcbf_refit -> bcbf_trtri -> bcbf_syrk_lt -> bcbf_kinv_apply -> bcbf_mll_grad -> bcbf_fit_adam_step)
against plain torch fp64 references (tests/_fit_reference.py) at the batch sizes and the N where their dispatchers switch form:
every branch of bcbf_mll_grad's launcher and every tile edge of its row form, the benchmarked 4099 x 512 batch with every model
compared, one-pair probes that isolate a single term of the sums, the inverse chain at full occupancy and at N > 512 (the
left-looking trtri form), value and gradient through the batch forms against an independent likelihood, and the Adam step with one
thread per model incl. its skip branch.  The default dispatch is what is under test (the development switches are static per
process and are not touched).

fp32 pair sums: the figures in MEASURED_F32 are the worst err / abs_sum of this module's own fp32 cases against the fp64 reference
on an MI355X (listing: profiles/r07_fit_scale_tol_report.txt); the assertion is min(4 x measured, 1 / (4 N)) -- 1 / (4 N) is a
quarter of what a lost row or column of pairs moves a sum by and is a cap, not a measurement."""
import math

import pytest
import torch

import _fit_reference as ref
from _tolreport import _record

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -23
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])

# worst err / abs_sum of the fp32 pair sums against the fp64 reference, per (form, N), measured on an MI355X with the cases of this
# module (rows = mll_grad_rows_kernel: fp32 sums, __expf; pairs = mll_grad_kernel: fp64 sums of fp32 inputs).  A key that is not
# listed is held to the cap alone.
MEASURED_F32 = {("rows", 1): 7.53e-8, ("rows", 63): 2.45e-8, ("rows", 64): 4.71e-8, ("rows", 65): 5.02e-8, ("rows", 127): 1.72e-8, ("rows", 128): 1.20e-8,
                ("rows", 129): 3.10e-8, ("rows", 255): 1.81e-8, ("rows", 256): 2.30e-8, ("rows", 257): 2.00e-8, ("rows", 300): 2.43e-8,
                ("rows", 511): 7.48e-9, ("rows", 512): 1.44e-8, ("rows", 513): 1.05e-8, ("rows", 1024): 6.77e-9, ("rows", 2048): 1.17e-9,
                ("pairs", 64): 9.50e-9, ("pairs", 65): 4.01e-8, ("pairs", 100): 1.37e-8, ("pairs", 129): 4.63e-8, ("pairs", 257): 1.89e-9,
                ("pairs", 300): 5.15e-9, ("pairs", 512): 6.02e-10, ("pairs", 513): 9.61e-9}
# fp64: below 1 / (4 N^2) of the largest N tested (6e-8 at N = 2048), so that ONE dropped or double-counted average pair fails
TOL_PAIR_SUMS_F64 = 1e-11


def _pair_sum_tol(dtype, form, N):
    if dtype == F64:
        return TOL_PAIR_SUMS_F64
    cap = 1.0 / (4.0 * N)
    return min(4.0 * MEASURED_F32[(form, N)], cap) if (form, N) in MEASURED_F32 else cap


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _sym_randn(Bt, N, dtype, g):
    """Bt symmetric N x N matrices with entries of variance 2, exactly symmetric in `dtype` (a + b == b + a), built chunk-wise."""
    S = torch.randn(Bt, N, N, dtype=dtype, device=DEV, generator=g)
    step = max(1, (1 << 26) // (N * N))
    for c in range(0, Bt, step):
        S[c:c + step] = S[c:c + step] + S[c:c + step].transpose(1, 2)
    return S


def _mll_inputs(Bt, N, n, m, nt, dtype, seed, lin=False, box=2.0):
    """Random well-scaled inputs of bcbf_mll_grad in `dtype`: any alpha and any symmetric Kinv define G, so no factorisation and no
    conditioning stand between the inputs and the pair sums.  X inside a box of `box` per side (ell in 0.6 .. 1.2): every pair
    carries weight, none underflows.  Bm symmetric positive definite (the non-symmetric variant: `Bm_ns`)."""
    g = _gen(seed)
    C = m + 1
    rn = lambda *s: torch.randn(*s, dtype=F64, device=DEV, generator=g)
    ru = lambda *s: torch.rand(*s, dtype=F64, device=DEV, generator=g)
    W, Wb = rn(Bt, nt, nt), rn(Bt, C, 1)
    d = dict(alpha=rn(Bt, N, nt), X=box * ru(Bt, N, n), UH=torch.cat([torch.ones(Bt, N, 1, dtype=F64, device=DEV), rn(Bt, N, m)], dim=2),
             R=rn(Bt, N, nt), Ainv=W @ W.transpose(1, 2) / nt + torch.eye(nt, dtype=F64, device=DEV),
             Bm=Wb @ Wb.transpose(1, 2) + torch.diag_embed(0.5 + ru(Bt, C)), ell=0.6 + 0.6 * ru(Bt, n), s2=0.5 + ru(Bt))
    d["Bm_ns"] = d["Bm"] + 0.3 * rn(Bt, C, C)
    if lin:
        d["lin"] = 0.2 + 0.5 * ru(Bt)
    d["jitter_u"] = 0.5 + 0.5 * ru(Bt, N)
    d = {k: v.to(dtype).contiguous() for k, v in d.items()}
    d["Kinv"] = _sym_randn(Bt, N, dtype, g)
    return d


def _reference(d, Bm, kind="rbf", jitter=None, chunk=None):
    """ref.mll_sums over the batch in chunks of about 64 x 512 x 512 pair terms (fp64, on the device)."""
    Bt, N = d["X"].shape[:2]
    chunk = chunk or max(1, min(Bt, (64 * 512 * 512) // (N * N)))
    outs = []
    for c in range(0, Bt, chunk):
        s = slice(c, c + chunk)
        outs.append(ref.mll_sums(d["alpha"][s], d["Kinv"][s], d["X"][s], d["UH"][s], d["R"][s], d["Ainv"][s], Bm[s], d["ell"][s], d["s2"][s],
                                 lin=d["lin"][s] if "lin" in d else None, kind=kind, jitter=None if jitter is None else jitter[s]))
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def _compare(got, want, d, dtype, form, what, logdet=None, acc=None):
    """Every output of one bcbf_mll_grad launch against the reference, every model: the pair sums on abs_sum, R'alpha and UH'alpha
    on their own sums of absolute terms (fp64 accumulation in a fixed order: N x 2.2e-16 <= 5e-13 of it, plus half an ulp of the
    output type), logdet K_b on sum |2 log L_ii| at the project's figures for the likelihood sums (1e-9 / 2e-3)."""
    Bt, N = d["X"].shape[:2]
    names = ("g_ell", "g_s2", "g_B", "logdetK", "RtA", "UHtA", "g_lin")
    got = dict(zip(names, got))
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), what
    tol = _pair_sum_tol(dtype, form, N)
    worst = 0.0
    for k in ("g_ell", "g_s2", "g_B") + (("g_lin",) if "g_lin" in want else ()):
        sc = want["abs_sum"].reshape((Bt,) + (1,) * (want[k].dim() - 1))
        err = ((got[k].double() - want[k]).abs() / sc).amax()
        worst = max(worst, float(err))
    acc = {} if acc is None else acc
    note = lambda k, v: acc.__setitem__(k, max(acc.get(k, 0.0), v))
    note("pair sums", worst)
    assert worst <= tol, "%s: pair sums off by %.3e of abs_sum (tolerance %.3e), N = %d, Bt = %d" % (what, worst, tol, N, Bt)
    small_tol = 1e-12 if dtype == F64 else 2.0 * EPS32
    for k, a, b in (("RtA", d["R"], d["alpha"]), ("UHtA", d["UH"], d["alpha"])):
        sc = a.double().abs().transpose(1, 2) @ b.double().abs()
        err = float(((got[k].double() - want[k]).abs() / sc).amax())
        note("RtA, UHtA", err)
        assert err <= small_tol, "%s %s: %.3e" % (what, k, err)
    if logdet is not None:
        ld, ld_abs = logdet
        ld_tol = 1e-9 if dtype == F64 else 2e-3
        err = float(((got["logdetK"].double() - ld).abs() / ld_abs).amax())
        note("logdetK", err)
        assert err <= ld_tol, "%s logdetK: %.3e" % (what, err)
    return worst


def _report(acc, dtype, form, N):
    """One line per test case and quantity in the tolerance report: the worst figure over the kernels and both kinds of Bm."""
    for k, tol in (("pair sums", _pair_sum_tol(dtype, form, N)), ("RtA, UHtA", 1e-12 if dtype == F64 else 2.0 * EPS32),
                   ("logdetK", 1e-9 if dtype == F64 else 2e-3)):
        if k in acc:                  # (the fp32 pair sums are listed per N, as they are asserted; the rest once per form)
            _record(("%s (%s, N %d)" if dtype == F32 and k == "pair sums" else "%s (%s) N=%d") % (k, form, N), acc[k], tol)


def _jitter(d, dtype):
    """Diagonal shift of the factorisation behind logdet K_b (the only output that needs a factor): large enough that K_b of N points
    inside a box of two length scales factors in the kernel's precision (cond about N s2 |u'Bu| / jitter: 1e6 in fp64, 1e4 in fp32)."""
    return (d["jitter_u"] * (1e-2 if dtype == F64 else 1.0)).contiguous()


# (Bt, N, n, m): the row form (workspace, n <= 4, m <= 3).  Bt < 64: column slices; Bt >= 64: JS = 1.  N > 128: several column tiles;
# N > 256: several row chunks.  N = 2048 at small Bt only.
ROW_CASES = [(1, 1, 1, 1), (3, 63, 2, 1), (63, 64, 3, 2), (64, 65, 4, 3), (70, 127, 1, 1), (1, 128, 2, 1), (3, 129, 3, 2), (63, 255, 4, 3),
             (64, 256, 1, 1), (70, 257, 2, 1), (3, 300, 3, 2), (70, 300, 4, 3), (63, 511, 4, 3), (64, 512, 3, 2), (1, 512, 1, 1), (70, 513, 2, 1),
             (63, 513, 3, 2), (64, 129, 4, 3), (64, 1024, 3, 2), (3, 1024, 4, 3), (1, 2048, 2, 1), (3, 2048, 3, 2)]
# the pair form behind the same entry points: n > 4 (split over workgroups below 64 models, one workgroup per model from 64 on)
PAIR_CASES = [(3, 300, 5, 2), (64, 129, 8, 3), (1, 513, 8, 3), (70, 65, 5, 2)]


@DTYPES
@pytest.mark.parametrize("Bt,N,n,m", ROW_CASES + PAIR_CASES, ids=lambda v: str(v))
def test_mll_grad_default_forms_against_the_fp64_reference(Bt, N, n, m, dtype):
    """Form sweep of bcbf_mll_grad / _matern52 / _rbfm52 through ops.mll_grad (workspace given): every output of every model against
    ref.mll_sums, symmetric and non-symmetric Bm, logdet K_b from bcbf_refit's factor of K_b + the given jitter."""
    from bayesian_cbf_amd import ops
    form = "rows" if n <= 4 else "pairs"
    d = _mll_inputs(Bt, N, n, m, n, dtype, seed=1000 * n + N + Bt)
    jit = _jitter(d, dtype)
    acc = {}
    for kernel in ref.KINDS:
        Lop, _, info, _ = ops.refit(d["X"], d["UH"], d["Bm"], d["ell"], d["s2"], jit, kernel=kernel)
        assert int((info != 0).sum()) == 0, "the test's own input did not factor"
        logdet = None
        for sym in (True, False):
            Bm = d["Bm"] if sym else d["Bm_ns"]
            got = ops.mll_grad(Lop, d["alpha"], d["Kinv"], d["X"], d["UH"], d["R"], d["Ainv"], Bm, d["ell"], d["s2"], kernel=kernel)
            want = _reference(d, Bm, kind=kernel, jitter=jit if sym else None)
            if sym:
                logdet = (want["logdetK"], want["logdet_abs"])
            _compare(got, want, d, dtype, form, "%s, Bm %ssymmetric" % (kernel, "" if sym else "not "), logdet=logdet, acc=acc)
    _report(acc, dtype, form, N)


@DTYPES
@pytest.mark.parametrize("Bt,N,n,m", [(3, 257, 3, 2), (2, 512, 4, 3), (65, 64, 2, 1), (2, 100, 8, 3)], ids=lambda v: str(v))
def test_mll_grad_without_a_workspace_against_the_fp64_reference(Bt, N, n, m, dtype):
    """The entry point called WITHOUT a workspace: one workgroup per model, every ordered pair, stores straight from the kernel."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.ops import _p, _suf, _stream, lib
    d = _mll_inputs(Bt, N, n, m, n, dtype, seed=77 + N)
    jit = _jitter(d, dtype)
    Lop, _, info, _ = ops.refit(d["X"], d["UH"], d["Bm"], d["ell"], d["s2"], jit)
    assert int((info != 0).sum()) == 0
    f = dict(dtype=dtype, device=DEV)
    C = m + 1
    logdet, acc = None, {}
    for sym in (True, False):
        Bm = d["Bm"] if sym else d["Bm_ns"]
        out = [torch.full(s, float("nan"), **f) for s in ((Bt, n), (Bt,), (Bt, C, C), (Bt,), (Bt, n, n), (Bt, C, n))]
        rc = getattr(lib, "bcbf_mll_grad" + _suf(d["X"]))(_p(Lop), _p(d["alpha"]), _p(d["Kinv"]), _p(d["X"]), _p(d["UH"]), _p(d["R"]), _p(d["Ainv"]),
                                                          _p(Bm), _p(d["ell"]), _p(d["s2"]), *(_p(o) for o in out), Bt, N, n, m, None, _stream(d["X"]))
        assert rc == 0
        torch.cuda.synchronize()
        want = _reference(d, Bm, jitter=jit if sym else None)
        if sym:
            logdet = (want["logdetK"], want["logdet_abs"])
        _compare(out, want, d, dtype, "pairs", "no workspace, Bm %ssymmetric" % ("" if sym else "not "), logdet=logdet, acc=acc)
    _report(acc, dtype, "pairs", N)


@DTYPES
@pytest.mark.parametrize("Bt,N,n,m", [(3, 300, 3, 2), (64, 129, 3, 3), (2, 257, 3, 5), (64, 100, 2, 8), (1, 512, 1, 11)], ids=lambda v: str(v))
def test_mll_grad_rbflin_against_the_fp64_reference(Bt, N, n, m, dtype):
    """bcbf_mll_grad_rbflin (data kernel s2 (exp(..) + lin x'x'), nt = 1 target column: the CoGP comparator's shape) -- always the pair
    form, split over workgroups below 64 models; m + 1 > BCBF_MAX_CTRL_DIM + 1 columns of UH take the CM = BCBF_MAX_TASK_DIM
    instantiation.  The factor behind logdet comes from bcbf_potrf of the reference's K_b + jitter (rounded to the kernel's type)."""
    from bayesian_cbf_amd import ops
    d = _mll_inputs(Bt, N, n, m, 1, dtype, seed=500 + N + m, lin=True)
    jit = _jitter(d, dtype)
    Kb = ref.kb_matrix(*(d[k].double() for k in ("X", "UH", "Bm", "ell", "s2")), lin=d["lin"].double()) + torch.diag_embed(jit.double())
    Kb = Kb.to(dtype).contiguous()
    Lop, info, _ = ops.potrf(Kb)
    assert int((info != 0).sum()) == 0
    logdet = ref.logdet_chol(torch.tril(Kb.double()) + torch.tril(Kb.double(), -1).transpose(1, 2))
    acc = {}
    for sym in (True, False):
        Bm = d["Bm"] if sym else d["Bm_ns"]
        got = ops.mll_grad(Lop, d["alpha"], d["Kinv"], d["X"], d["UH"], d["R"], d["Ainv"], Bm, d["ell"], d["s2"], lin=d["lin"])
        _compare(got, _reference(d, Bm), d, dtype, "pairs", "rbflin C=%d, Bm %ssymmetric" % (m + 1, "" if sym else "not "), logdet=logdet, acc=acc)
    _report(acc, dtype, "pairs", N)


@DTYPES
def test_mll_grad_at_the_benchmarked_size_every_model(dtype):
    """Bt = 4099 (not a multiple of 64 or of the eight XCDs), N = 512, n = 3, m = 2: the form the fit benchmark runs (row form, two
    row chunks, four column tiles, JS = 1).  EVERY model is compared, the reference evaluated on the device in fp64 in chunks of 64."""
    from bayesian_cbf_amd import ops
    Bt, N, n, m = 4099, 512, 3, 2
    d = _mll_inputs(Bt, N, n, m, n, dtype, seed=4099)
    jit = _jitter(d, dtype)
    Lop, _, info, _ = ops.refit(d["X"], d["UH"], d["Bm"], d["ell"], d["s2"], jit)
    assert int((info != 0).sum()) == 0
    logdet, acc = None, {}
    for sym in (True, False):
        Bm = d["Bm"] if sym else d["Bm_ns"]
        got = ops.mll_grad(Lop, d["alpha"], d["Kinv"], d["X"], d["UH"], d["R"], d["Ainv"], Bm, d["ell"], d["s2"])
        again = ops.mll_grad(Lop, d["alpha"], d["Kinv"], d["X"], d["UH"], d["R"], d["Ainv"], Bm, d["ell"], d["s2"])
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "two launches on the same inputs differ"
        want = _reference(d, Bm, jitter=jit if sym else None, chunk=64)
        if sym:
            logdet = (want["logdetK"], want["logdet_abs"])
        _compare(got, want, d, dtype, "rows", "4099 models, Bm %ssymmetric" % ("" if sym else "not "), logdet=logdet, acc=acc)
    _report(acc, dtype, "rows", N)


# ---- one-pair probes -----------------------------------------------------------------------------------------------------------
def _probe_pairs(N):
    """(i, j) on both sides of every edge of the row form: waves of 64 rows, column tiles / slices of 128, row chunks of 256, the
    first and the last point; every combination of the edge indices (incl. the diagonal) and j = i +- 1."""
    E = sorted(e for e in {0, 63, 64, 127, 128, 191, 192, 255, 256, 383, 384, 511, 512, N - 2, N - 1} if 0 <= e < N)
    pairs = [(i, j) for i in E for j in E]
    pairs += [(e, e + s) for e in E for s in (-1, 1) if 0 <= e + s < N and (e, e + s) not in pairs]
    return pairs


@DTYPES
@pytest.mark.parametrize("N", [300, 512, 640])
def test_mll_grad_one_pair_probes(N, dtype):
    """Model b gets alpha = 0 and Kinv = e_i e_j' + e_j e_i' (e_i e_i' on the diagonal) for ONE pair (i_b, j_b): G has one pair of
    entries -nt/2, so every sum is a single term and a dropped, doubled or mis-weighted pair is an error of 50 .. 100 % of it --
    which no whole-sum tolerance in fp32 can see.  All pairs in one launch (>= 64 models: JS = 1) and in launches of 50 (column
    slices).  X inside a box of ONE length scale per side (no k_ij below exp(-n/2)), |u| <= 1.5, Bm diagonally dominant, so every output
    is at most about 5 nt/2 times t = sum_ac |uh_ia Bm_ac uh_jc| s2 k_ij (the mean of both orders of (i, j): Bm is not symmetric);
    compared relative to nt t.  Measured on an MI355X: 5e-16 (fp64), 2.5e-7 (fp32) of nt t.
    Tolerance, from the arithmetic and not from the kernel: fp64 1e-12 (some 20 operations of 1.1e-16 on terms up to 5 t); fp32
    64 x 2^-23 = 7.6e-6 (about 12 roundings of 6e-8 on terms up to 5 t, and __expf = exp2(x log2 e) whose argument product adds
    |x| 6e-8 <= 1.2e-7 for |x| <= n/2 = 2)."""
    from bayesian_cbf_amd import ops
    n, m, nt = 3, 2, 3
    pairs = _probe_pairs(N)
    Bt = len(pairs)
    assert Bt >= 64
    d = _mll_inputs(Bt, N, n, m, nt, dtype, seed=N)
    g = _gen(N + 1)
    ell = d["ell"].double()
    d["X"] = (torch.rand(Bt, N, n, dtype=F64, device=DEV, generator=g) * ell[:, None, :]).to(dtype).contiguous()
    U = 3.0 * torch.rand(Bt, N, m, dtype=F64, device=DEV, generator=g) - 1.5
    d["UH"] = torch.cat([torch.ones(Bt, N, 1, dtype=F64, device=DEV), U], dim=2).to(dtype).contiguous()
    C = m + 1
    Bm = 0.3 * torch.randn(Bt, C, C, dtype=F64, device=DEV, generator=g) + torch.diag_embed(1.0 + torch.rand(Bt, C, dtype=F64, device=DEV, generator=g))
    Bm = Bm.to(dtype).contiguous()                                             # (not symmetric: u_i'B u_j != u_j'B u_i)
    d["alpha"] = torch.zeros_like(d["alpha"])
    ii = torch.tensor([p[0] for p in pairs], device=DEV)
    jj = torch.tensor([p[1] for p in pairs], device=DEV)
    bb = torch.arange(Bt, device=DEV)
    Kinv = torch.zeros(Bt, N, N, dtype=dtype, device=DEV)
    Kinv[bb, ii, jj] = 1.0
    Kinv[bb, jj, ii] = 1.0
    d["Kinv"] = Kinv
    Lop = torch.ones(Bt, ops.lop_elems(N, dtype), dtype=dtype, device=DEV)      # (a unit diagonal: logdet = 0; the probes are about the pair sums)
    want = _reference(d, Bm)
    Xd, UHd = d["X"].double(), d["UH"].double()
    z = (Xd[bb, ii] - Xd[bb, jj]) / ell
    kij = d["s2"].double() * torch.exp(-0.5 * (z * z).sum(1))
    t = 0.5 * kij * ((UHd[bb, ii][:, :, None] * Bm.double() * UHd[bb, jj][:, None, :]).abs().sum((1, 2))
                     + (UHd[bb, jj][:, :, None] * Bm.double() * UHd[bb, ii][:, None, :]).abs().sum((1, 2)))      # (both orders: Bm is not symmetric)
    assert float((want["abs_sum"] / (nt * t)).max()) <= 1.0 + 1e-12 and float(t.min()) > 0.0
    tol = 1e-12 if dtype == F64 else 64.0 * EPS32
    sel = lambda s: (Lop[s], d["alpha"][s], d["Kinv"][s], d["X"][s], d["UH"][s], d["R"][s], d["Ainv"][s], Bm[s], d["ell"][s], d["s2"][s])
    for mode, step in (("one launch", Bt), ("launches of 50", 50)):
        worst = 0.0
        for c in range(0, Bt, step):
            s = slice(c, min(Bt, c + step))
            got = ops.mll_grad(*(a.contiguous() for a in sel(s)))
            torch.cuda.synchronize()
            for k, gv in zip(("g_ell", "g_s2", "g_B"), got[:3]):
                sc = (nt * t[s]).reshape((-1,) + (1,) * (gv.dim() - 1))
                err = ((gv.double() - want[k][s]).abs() / sc).reshape(gv.shape[0], -1).amax(1)
                bad = int(err.argmax())
                worst = max(worst, float(err[bad]))
                assert float(err[bad]) <= tol, "%s, %s: pair (i, j) = %s of N = %d is off by %.3e of its term (got %s, want %s)" % (
                    mode, k, pairs[c + bad], N, float(err[bad]), gv[bad].flatten().tolist(), want[k][c + bad].flatten().tolist())
            assert float(got[3].abs().max()) == 0.0 and float(got[4].abs().max()) == 0.0 and float(got[5].abs().max()) == 0.0
        _record("N%d probes, %s" % (N, mode), worst, tol)


# ---- trtri / syrk_lt / kinv_apply ----------------------------------------------------------------------------------------------
SENTINEL = -7.25e17


def _guarded(Bt, tail, dtype):
    """An output for Bt models carved out of a buffer with one model of sentinel before and after it."""
    buf = torch.full((Bt + 2,) + tail, SENTINEL, dtype=dtype, device=DEV)
    out = buf[1:Bt + 1]
    out.fill_(float("nan"))
    return buf, out


def _guards_untouched(buf):
    return bool((buf[0] == SENTINEL).all()), bool((buf[-1] == SENTINEL).all())


def _inverse_chain(Bt, N, dtype, seed, report=False):
    """refit -> trtri -> syrk_lt -> kinv_apply of Bt well conditioned models, each kernel against ITS OWN input in torch fp64, every
    model; every kernel launched twice (bit-identical), outputs between sentinel guard bands.  Normalisations and fp figures are
    those of tests/test_gpu_fit.py (1e-9 / 2e-3 trtri residual over cond_scale, 1e-13 / 2e-6 x N/32 syrk, 1e-13 / 2e-6 kinv_apply),
    applied per model."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.ops import _p, _suf, _stream, lib
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == F64
    p = make_instances(Bt, N, 3, 2, dtype=dtype, device=DEV, seed=seed)
    X = (p["X"] * 3.0).contiguous()                        # well conditioned: the check is on the arithmetic
    jit = (p["jitter"] * (1 if f64 else 1e3)).contiguous()
    chunk = max(1, min(Bt, (128 * 512 * 512) // (N * N)))
    chunks = [slice(c, min(Bt, c + chunk)) for c in range(0, Bt, chunk)]
    # a condition on the INPUTS: torch's fp64 Cholesky of every K_b succeeds
    min_pivot = math.inf
    for s in chunks:
        Kb = ref.kb_matrix(X[s].double(), p["UH"][s].double(), p["Bm"][s].double(), p["ell"][s].double(), p["s2"][s].double())
        L, tinfo = torch.linalg.cholesky_ex(Kb + torch.diag_embed(jit[s].double()))
        assert int((tinfo != 0).sum()) == 0, "input: torch's fp64 Cholesky failed"
        min_pivot = min(min_pivot, float(L.diagonal(dim1=1, dim2=2).min()))
        del Kb, L
    assert min_pivot > 0.0
    Lop, _, info, Ld = ops.refit(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit, want_dense=True)
    assert int((info != 0).sum()) == 0, "no model may be left out: %d of %d did not factor" % (int((info != 0).sum()), Bt)
    suf, st = _suf(Lop), _stream(Lop)
    worst = {}

    def twice(launch, tail, name):
        buf, out = _guarded(Bt, tail, dtype)
        launch(out)
        second = torch.full((Bt,) + tail, float("nan"), dtype=dtype, device=DEV)
        launch(second)
        torch.cuda.synchronize()
        assert _guards_untouched(buf) == (True, True), "%s wrote outside its output (before, after) = %s" % (name, _guards_untouched(buf))
        assert torch.equal(out, second), "%s: two launches on the same inputs differ" % name
        del second
        return buf, out

    # L^-1
    lbuf, Linv = twice(lambda o: ops.check(getattr(lib, "bcbf_trtri" + suf)(_p(Lop), _p(o), Bt, N, st), "bcbf_trtri"), (N, N), "bcbf_trtri")
    eye = torch.eye(N, dtype=F64, device=DEV)
    w = 0.0
    for s in chunks:
        Li, L = Linv[s].double(), Ld[s].double()
        assert bool(torch.isfinite(Li).all())
        assert float(torch.triu(Li, diagonal=1).abs().max()) == 0.0
        res = (L @ Li - eye).abs().amax(dim=(1, 2)) / (Li.abs().amax(dim=(1, 2)) * L.abs().amax(dim=(1, 2)))
        w = max(w, float(res.max()))
        del Li, L
    worst["trtri residual"] = (w, 1e-9 if f64 else 2e-3)
    del Ld
    # K^-1 = L^-T L^-1
    kbuf, Kinv = twice(lambda o: ops.check(getattr(lib, "bcbf_syrk_lt" + suf)(_p(Linv), _p(o), Bt, N, st), "bcbf_syrk_lt"), (N, N), "bcbf_syrk_lt")
    w = 0.0
    for s in chunks:
        K, Li = Kinv[s], Linv[s].double()
        assert bool(torch.isfinite(K).all())
        assert torch.equal(K, K.transpose(1, 2)), "K_b^-1 is not exactly symmetric"
        want = Li.transpose(1, 2) @ Li
        w = max(w, float(((K.double() - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2))).max()))
        del Li, want
    worst["syrk_lt"] = (w, (1e-13 if f64 else 2e-6) * (N / 32))
    del Linv, lbuf
    # alpha = K^-1 R
    R = torch.randn(Bt, N, 3, dtype=dtype, device=DEV, generator=_gen(seed + 5))
    abuf, alpha = twice(lambda o: ops.kinv_apply(Kinv, R, out=o), (N, 3), "bcbf_kinv_apply")
    w = 0.0
    for s in chunks:
        want = Kinv[s].double() @ R[s].double()
        assert bool(torch.isfinite(alpha[s]).all())
        w = max(w, float(((alpha[s].double() - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2))).max()))
    worst["kinv_apply"] = (w, 1e-13 if f64 else 2e-6)
    for k, (v, tol) in worst.items():
        _record("%s (Bt=%d) N=%d" % (k, Bt, N), v, tol)
    if report:
        print("\n[fit_scale] Bt=%d N=%d %s: smallest pivot of torch's fp64 Cholesky %.3e; %s; peak device memory %.2f GB" % (
            Bt, N, "f64" if f64 else "f32", min_pivot, ", ".join("%s %.2e" % (k, v) for k, (v, _) in worst.items()),
            torch.cuda.max_memory_allocated() / 1e9))
    for k, (v, tol) in worst.items():
        assert v < tol, "%s: %.3e (tolerance %.1e), Bt = %d, N = %d" % (k, v, tol, Bt, N)


@DTYPES
def test_inverse_chain_at_full_occupancy_every_model(dtype):
    """Bt = 4099 (not a multiple of the eight XCDs; a ragged last group of eight), N = 512: trtri's pair form, syrk's 128-block form
    through the LDS ring, kinv_apply's vector form, many workgroups per XCD.  All 4099 models factor (info == 0) and all are checked."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    _inverse_chain(4099, 512, dtype, seed=11, report=True)
    torch.cuda.empty_cache()


@DTYPES
@pytest.mark.parametrize("Bt,N", [(4, 513), (17, 513), (4, 544), (17, 544), (4, 1000), (17, 1000), (4, 1024), (17, 1024), (4, 2048), (17, 2048),
                                  (4, 512), (7, 512), (8, 512), (9, 512), (15, 512), (16, 512)], ids=lambda v: str(v))
def test_inverse_chain_above_512_and_at_group_boundaries(Bt, N, dtype):
    """N > 512 at Bt >= 4: trtri's left-looking matrix-core form (more than 16 blocks of 32), then syrk_lt (2 x 2 tiles; the 128-block
    form at 1024 / 2048) and kinv_apply (vector form up to 1024, scalar at 2048); N = 512 at the batch sizes around the pair form's
    groups of eight."""
    _inverse_chain(Bt, N, dtype, seed=N + Bt)
    torch.cuda.empty_cache()


# ---- value and gradient through the batch forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Bt,N,rank,prior", [(72, 256, None, None), (20, 384, None, None), (72, 256, 1, (1e-3, 1e-3))],
                         ids=["72x256", "20x384", "72x256-rank-one+prior"])
def test_value_and_gradient_through_the_batch_forms_vs_independent_likelihood(Bt, N, rank, prior):
    """BatchedHyperFit.value_and_grad (fp64, n = 3, m = 2, given jitter draws) at sizes that reach trtri's pair form, syrk's tile form,
    kinv_apply's vector form and the row form of mll_grad (JS = 1 at 72 models, column slices at 20) together: the loss (1e-9) and
    EVERY gradient entry of EVERY model against ref.neg_mll's autograd gradient.  Gradient bound per model: 10 x the reference's own
    sensitivity -- the difference between its gradient with K_b^-1 by Cholesky and by torch.linalg.inv, both fp64 -- with a floor of
    1e-10, relative to the gradient's largest entry.  Measured on an MI355X with these inputs: sensitivity 1.0e-15 of the largest
    entry (so the floor of 1e-10 is what binds), the kernels' gradient within 1.4e-15 and the loss within 4.2e-16 relative."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.batched_fit import BatchedHyperFit
    from bayesian_cbf_amd.synthetic import make_instances
    n, m = 3, 2
    p = make_instances(Bt, N, n, m, dtype=F64, device=DEV, seed=N + Bt)
    X = (p["X"] * 3.0).contiguous()
    g = _gen(31 + N)
    P = ops.fit_param_count(n, m, *ref.fit_ranks(n, m, rank))
    theta = (0.3 * torch.randn(Bt, P, dtype=F64, device=DEV, generator=g)).contiguous()
    bf = BatchedHyperFit(theta, n, m, rank=rank, gamma_length_scale_prior=prior)
    draws = 0.1 + 0.8 * torch.rand(Bt, N, dtype=F64, device=DEV, generator=g)
    bf.jitter_rand = lambda idx, N_: draws[idx]
    loss, grad, skip = bf.value_and_grad(X, p["UH"], p["Xdot"])
    assert int(skip.sum()) == 0 and grad.shape == (Bt, P)
    assert float(bf.jitter_level.max()) == 1e-5
    jit = 1e-5 * draws
    want_loss, want_grad = ref.neg_mll_value_and_grad(theta, X, p["UH"], p["Xdot"], jit, n, m, rank, prior, "cholesky")
    _, grad_inv = ref.neg_mll_value_and_grad(theta, X, p["UH"], p["Xdot"], jit, n, m, rank, prior, "inv")
    gmax = want_grad.abs().amax(1)
    sens = (want_grad - grad_inv).abs().amax(1) / gmax
    tol = torch.clamp(10.0 * sens, min=1e-10)
    err = (grad - want_grad).abs().amax(1) / gmax
    lerr = float(((loss - want_loss).abs() / (1e-10 + 1e-9 * want_loss.abs())).max())
    _record("loss N=%d" % N, lerr * 1e-9, 1e-9)
    _record("gradient / largest entry N=%d" % N, float(err.max()), float(tol[err.argmax()]))
    _record("reference sensitivity (Cholesky vs inv) N=%d" % N, float(sens.max()), 1e-11)
    assert lerr <= 1.0, "loss: %.3e of its tolerance" % lerr
    bad = int((err / tol).argmax())
    assert bool((err <= tol).all()), "model %d: gradient off by %.3e of its largest entry (tolerance %.3e, reference sensitivity %.3e)" % (
        bad, float(err[bad]), float(tol[bad]), float(sens[bad]))


# ---- bcbf_fit_adam_step / bcbf_fit_derive at a batch ------------------------------------------------------------------------------
BT_REP, N_BASE = 4099, 5


def _replicated_fit_inputs(dtype, rank, seed=9):
    """5 distinct models (raw parameters, sums of a real bcbf_mll_grad launch on random inputs) repeated over 4099 rows, row b = model
    b % 5 (5 is coprime to the 64 threads of a workgroup: every lane position sees every model)."""
    from bayesian_cbf_amd import ops
    n, m, N = 3, 2, 65
    rA, rB = ref.fit_ranks(n, m, rank)
    P = ops.fit_param_count(n, m, rA, rB)
    theta0 = (0.4 * torch.randn(N_BASE, P, dtype=F64, device=DEV, generator=_gen(seed))).to(dtype).contiguous()
    hp = ops.fit_derive(theta0, n, m, rA, rB, want_Ainv=True)
    d = _mll_inputs(N_BASE, N, n, m, n, dtype, seed=seed + 1)
    Lop, _, info, _ = ops.refit(d["X"], d["UH"], hp["Bm"], hp["ell"], hp["s2"], _jitter(d, dtype))
    assert int((info != 0).sum()) == 0
    sums = ops.mll_grad(Lop, d["alpha"], d["Kinv"], d["X"], d["UH"], d["R"], hp["Ainv"], hp["Bm"], hp["ell"], hp["s2"])
    idx = torch.arange(BT_REP, device=DEV) % N_BASE
    rep = lambda t: t[idx].contiguous()
    return dict(n=n, m=m, N=N, rA=rA, rB=rB, P=P, theta0=theta0, sums=sums, Ainv=hp["Ainv"], logdetA=hp["logdetA"], idx=idx, rep=rep)


def _close(got, want, dtype, floor=0.0, what=""):
    """fp64: 1e-12 of the array's largest entry.  fp32: 2 ulp (2 x 2^-23 relative) elementwise, `floor` = the magnitude below which an
    entry is a difference of larger numbers."""
    got, want = got.double(), want.double()
    if dtype == F64:
        err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        _record(what, err, 1e-12)
        assert err <= 1e-12, "%s: %.3e" % (what, err)
    else:
        ratio = float(((got - want).abs() / torch.clamp(want.abs(), min=max(floor, 1e-37))).max())
        _record(what, ratio, 2.0 * EPS32)
        assert ratio <= 2.0 * EPS32, "%s: %.3e (= %.2f ulp of fp32)" % (what, ratio, ratio / EPS32)


@DTYPES
@pytest.mark.parametrize("rank,prior", [(None, None), (1, (1e-3, 1e-3)), (None, (2.0, 3.0))], ids=["full", "rank-one+prior", "full+prior"])
def test_fit_adam_step_at_a_batch_and_the_skip_branch(rank, prior, dtype):
    """bcbf_fit_adam_step over 4099 rows (one thread per model, 65 workgroups, a ragged last one): every row equals its base model
    bit for bit; the 5 base rows equal the documented update restated in torch fp64 (ref.loss_and_grad_from_sums: autograd for the
    chain rule; ref.adam_step with the kernel's roundings in fp32) over two steps; with skip[b] = 1 on a scattered set the skipped rows
    keep theta, mom1, mom2 bit for bit and report loss = NaN, every other row is what it is without a mask."""
    from bayesian_cbf_amd import ops
    c = _replicated_fit_inputs(dtype, rank)
    n, m, N, rA, rB, idx, rep = c["n"], c["m"], c["N"], c["rA"], c["rB"], c["idx"], c["rep"]
    sums, Ainv, logdetA = tuple(rep(s) for s in c["sums"]), rep(c["Ainv"]), rep(c["logdetA"])
    theta, mom1, mom2 = rep(c["theta0"]), torch.zeros(BT_REP, c["P"], dtype=dtype, device=DEV), torch.zeros(BT_REP, c["P"], dtype=dtype, device=DEV)
    lr = 0.1
    for step in (1, 2):
        before = tuple(t[:N_BASE].clone() for t in (theta, mom1, mom2))
        saved = tuple(t.clone() for t in (theta, mom1, mom2))
        loss, grad = ops.fit_adam_step(theta, mom1, mom2, sums, Ainv, logdetA, N, n, m, rA, rB, step, lr, gamma_prior=prior, want_grad=True)
        torch.cuda.synchronize()
        for name, t in (("theta", theta), ("mom1", mom1), ("mom2", mom2), ("loss", loss), ("grad", grad)):
            assert torch.equal(t, t[:N_BASE][idx]), "step %d: %s differs between rows of the same model" % (step, name)
        want_loss, want_grad = ref.loss_and_grad_from_sums(before[0], c["sums"], c["Ainv"], c["logdetA"], N, n, m, rank, prior)
        w_theta, w_m1, w_m2 = ref.adam_step(before[0], before[1], before[2], want_grad, step, lr, dtype)
        tag = "step %d " % step
        _close(loss[:N_BASE], want_loss, dtype, what=tag + "loss")
        _close(grad[:N_BASE], want_grad, dtype, floor=1e-6 * float(want_grad.abs().max()), what=tag + "grad")
        _close(mom1[:N_BASE], w_m1, dtype, floor=1e-7 * float(w_m1.abs().max()), what=tag + "mom1")
        _close(mom2[:N_BASE], w_m2, dtype, floor=1e-12 * float(w_m2.abs().max()), what=tag + "mom2")
        _close(theta[:N_BASE], w_theta, dtype, floor=lr, what=tag + "theta")
        # the same step with a skip mask, from the same state
        skipped = torch.tensor([0, 1, 62, 63, 64, 65, 127, 128, 1000, 2047, 2048, 4031, 4032, 4095, 4096, 4097, 4098], device=DEV)
        skip = torch.zeros(BT_REP, dtype=torch.int32, device=DEV)
        skip[skipped] = 1
        keep = skip == 0
        th2, m1b, m2b = (t.clone() for t in saved)
        loss2, _ = ops.fit_adam_step(th2, m1b, m2b, sums, Ainv, logdetA, N, n, m, rA, rB, step, lr, skip=skip, gamma_prior=prior, want_grad=True)
        torch.cuda.synchronize()
        for name, t2, t0, t1 in (("theta", th2, saved[0], theta), ("mom1", m1b, saved[1], mom1), ("mom2", m2b, saved[2], mom2)):
            assert torch.equal(t2[skipped], t0[skipped]), "step %d: a skipped model's %s changed" % (step, name)
            assert torch.equal(t2[keep], t1[keep]), "step %d: %s of a model that was not skipped depends on the mask" % (step, name)
        assert bool(torch.isnan(loss2[skipped]).all()) and torch.equal(loss2[keep], loss[keep])
        assert not torch.equal(theta[skipped], saved[0][skipped])                      # (without the mask those rows do move)


@DTYPES
@pytest.mark.parametrize("rank", [None, 1, 0], ids=["full", "rank-one", "diag"])
def test_fit_derive_at_a_batch(rank, dtype):
    """bcbf_fit_derive over the same 4099 replicated rows: bit-identical per base model, and the base rows equal softplus /
    W W' + diag softplus restated in torch fp64 (rounded once to the output type: 2 ulp in fp32), A^-1 to cond(A) x 1e-13 more."""
    from bayesian_cbf_amd import ops
    c = _replicated_fit_inputs(dtype, rank)
    n, m, idx = c["n"], c["m"], c["idx"]
    out = ops.fit_derive(c["rep"](c["theta0"]), n, m, c["rA"], c["rB"], want_Ainv=True)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(v, v[:N_BASE][idx]), k
    want = ref.derive(c["theta0"].double(), n, m, rank)
    eps = 1e-12 if dtype == F64 else 2.0 * EPS32
    for k in ("ell", "s2", "A", "Bm", "M0"):
        got, w = out[k][:N_BASE].double(), want[k]
        scale = w.abs().max() if dtype == F64 else torch.clamp(w.abs(), min=1e-6 * float(w.abs().max()))
        err = float(((got - w).abs() / scale).max())
        _record("derive " + k, err, eps)
        assert err <= eps, "%s: %.3e" % (k, err)
    wi = torch.linalg.inv(want["A"])
    cond = torch.linalg.cond(want["A"])
    err = (out["Ainv"][:N_BASE].double() - wi).abs().amax((1, 2)) / wi.abs().amax((1, 2))
    assert bool((err <= eps + 1e-13 * cond).all()), ("Ainv", err.tolist(), cond.tolist())
    wl = torch.logdet(want["A"])
    assert bool(((out["logdetA"][:N_BASE].double() - wl).abs() <= eps * wl.abs() + 1e-13 * n).all()), "logdetA"
