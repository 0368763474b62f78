"""The conic solvers at every compiled shape: `socp_quad_kernel` behind bcbf_socp / bcbf_cbc_socp (four lanes per instance,
m = 1..3, K = 1..4) and `coneqp_kernel` behind bcbf_coneqp_f64 (one lane per instance, narrow and wide instantiation), held to
an optimality bound that does not trust the numpy port's `x` (tests/_conic_reference.py: feasibility + objective against a
Lagrangian lower bound), to their statuses, to independence of an instance's position in the batch, and to the rule that an
instance reported OPTIMAL is optimal also when it leaves through the best-iterate fallback.  Tolerances: ten times the numpy
port's own worst figure on the family, never above the solvers' accept level 1e-7 (`cr.tolerances`)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _conic_reference as cr  # noqa: E402
from _tolreport import rel_close, all_close  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
OPTIMAL, MAXITER, DIVERGED = 0, 1, 2
EINVAL = -1
LOW_ITERS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def host(t):
    return t.detach().cpu().double().numpy()


def ihost(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ shared checks
def check_optimal(progs, sols, kept, y, family, rounded=False, eps=None, sel=None, what=""):
    """Section 1 of the helper on every program the reference solved (and `sel` selects): at most 2 % left out, multipliers
    in K, feasibility and objective-vs-lower-bound figures within (eps_f, eps_g)."""
    eps_f, eps_g = eps if eps is not None else cr.tolerances(family)
    assert (~kept).sum() <= cr.LEFT_OUT_CAP * len(kept), "reference left out %d of %d" % ((~kept).sum(), len(kept))
    idx = [i for i in range(len(progs)) if kept[i] and (sel is None or sel[i])]
    if not idx:
        return
    assert max(cr.z_in_cone_figure(sols[i]["z"], progs[i][4]) for i in idx) <= 1e-12
    figs = [cr.figures(progs[i], sols[i]["z"], y[i], rounded) for i in idx]
    rel_close(np.array([f for f, _ in figs]), 0.0, eps_f, scale=1.0, what=what + " cone feasibility")
    if eps_g is not None:
        rel_close(np.maximum([g for _, g in figs], 0.0), 0.0, eps_g, scale=1.0, what=what + " objective - lower bound")


def check_against_x(sols, kept, y, rtol, atol, what):
    ref = np.stack([s["x"] for s in sols])
    all_close(y[kept], ref[kept], rtol, atol, what=what)


def x_tol(dtype):
    """The y-vs-oracle tolerance of test_gpu_parity.py::test_socp_vs_oracle."""
    return (1e-6, 1e-7) if dtype == F64 else (1e-3, 1e-3)


def solve_quad(ops, p, mask, dtype, max_iters=100, order=None):
    """ops.socp on a CLF-CBF batch (optionally with its instances reordered): (y, status, iters) on the host."""
    sel = slice(None) if order is None else order
    cones = ops.pack_cones(*(dev(p[k][sel], dtype) for k in ("A", "b", "c", "d")))
    y, st, it = ops.socp(dev(p["w"][sel], dtype), dev(p["r"][sel], dtype), cones, dev(mask, dtype), dev(p["rho"][sel], dtype),
                         max_iters=max_iters)
    return host(y), ihost(st), ihost(it)


def solve_generic(ops, p, max_iters=100, order=None):
    sel = slice(None) if order is None else order
    x, st, it = ops.coneqp(*(dev(p[k][sel], F64) for k in ("P", "q", "G", "h")), p["dims"]["l"], p["dims"]["q"],
                           max_iters=max_iters)
    return host(x), ihost(st), ihost(it)


def check_low_iteration_runs(run, progs, sols, kept, family, what):
    """`run(max_iters) -> (y, status, iters)` for max_iters in LOW_ITERS: what reports OPTIMAL is optimal at the accept level,
    everything else is MAXITER at exactly max_iters, some instance is cut off at max_iters = 1, and OPTIMAL is kept by
    every larger max_iters."""
    was_optimal = np.zeros(len(progs), dtype=bool)
    for mi in LOW_ITERS:
        y, st, it = run(mi)
        opt = st == OPTIMAL
        assert (st[~opt] == MAXITER).all() and (it[~opt] == mi).all(), (mi, st, it)
        assert (it <= mi).all()
        if mi == 1:
            assert (~opt).any()
        assert opt[was_optimal].all(), (mi, np.nonzero(was_optimal & ~opt)[0])
        was_optimal |= opt
        check_optimal(progs, sols, kept, y, family, eps=(cr.ACCEPT, cr.ACCEPT), sel=opt, what="%s max_iters=%d" % (what, mi))


# ------------------------------------------------------------------------------------------------ bcbf_socp
def _quad_case(ops, m, K, pattern, dtype, Bt):
    f32 = dtype == F32
    p, mask, progs, sols, kept = cr.clf_cbf_case(cr.clf_cbf_seed(m, K), Bt, m, K, pattern, f32)
    y, st, it = solve_quad(ops, p, mask, dtype)
    assert (st == OPTIMAL).all(), st
    assert it.max() <= 40, it.max()
    check_optimal(progs, sols, kept, y, "clf_cbf", rounded=f32, what="socp m=%d K=%d" % (m, K))
    check_against_x(sols, kept, y, *x_tol(dtype), what="y vs oracle socp")


@DTYPES
@pytest.mark.parametrize("pattern", cr.MASKS)
@pytest.mark.parametrize("m,K", cr.QUAD_SHAPES)
def test_socp_is_optimal_at_every_compiled_shape(ops, m, K, pattern, dtype):
    """Bt = 67: four full waves of 16 instances and a ragged one whose last quads shadow instance 66; rho, slack, weights
    and reference drawn per instance, so one wave holds half-planes (rho = 0) beside cones."""
    _quad_case(ops, m, K, pattern, dtype, cr.QUAD_BT)


@DTYPES
@pytest.mark.parametrize("Bt", [1, 17])
def test_socp_single_quad_and_one_quad_past_a_wave(ops, Bt, dtype):
    _quad_case(ops, 2, 3, "first", dtype, Bt)


@pytest.mark.parametrize("m,K", [(1, 1), (2, 3), (3, 2), (3, 4)])
def test_socp_result_does_not_depend_on_the_position_in_the_batch(ops, m, K):
    p, mask, _, _, _ = cr.clf_cbf_case(cr.clf_cbf_seed(m, K), cr.QUAD_BT, m, K, "first", False)
    order = np.random.default_rng(1).permutation(cr.QUAD_BT)
    y0, st0, it0 = solve_quad(ops, p, mask, F64)
    y1, st1, it1 = solve_quad(ops, p, mask, F64, order=order)
    assert np.array_equal(y1, y0[order]) and np.array_equal(st1, st0[order]) and np.array_equal(it1, it0[order])


@pytest.mark.parametrize("m,K", [(2, 3), (3, 4)])
def test_socp_claimed_optimum_is_an_optimum_under_low_iteration_caps(ops, m, K):
    p, mask, progs, sols, kept = cr.clf_cbf_case(cr.clf_cbf_seed(m, K), cr.QUAD_BT, m, K, "first", False)
    check_low_iteration_runs(lambda mi: solve_quad(ops, p, mask, F64, max_iters=mi), progs, sols, kept, "clf_cbf",
                             "socp m=%d K=%d" % (m, K))


def test_socp_statuses_inside_a_mixed_wave(ops):
    """An infeasible program, a NaN and an inf among 17 feasible ones in two waves: flagged, and nobody else disturbed."""
    p, mask, _, _, _ = cr.clf_cbf_case(cr.clf_cbf_seed(2, 3), 20, 2, 3, "first", False)
    y0, st0, it0 = solve_quad(ops, p, mask, F64)
    assert (st0 == OPTIMAL).all()
    q = {k: v.copy() for k, v in p.items()}
    # instance 5: two contradictory half-planes (u0 >= 1 + rho |.| and -u0 >= 1 + rho |.|), no relaxation on them
    q["A"][5, 1] = q["A"][5, 2] = np.eye(3)[:, 1:]
    q["b"][5, 1] = q["b"][5, 2] = [1.0, 0, 0]
    q["c"][5, 1], q["c"][5, 2] = [1.0, 0.0], [-1.0, 0.0]
    q["d"][5, 1] = q["d"][5, 2] = -1.0
    q["d"][11, 1] = np.nan
    q["w"][12, 0] = np.inf
    y, st, it = solve_quad(ops, q, mask, F64)
    bad = [5, 11, 12]
    assert (st[bad] != OPTIMAL).all(), st[bad]
    rest = np.delete(np.arange(20), bad)
    assert np.array_equal(y[rest], y0[rest]) and np.array_equal(st[rest], st0[rest]) and np.array_equal(it[rest], it0[rest])


# ------------------------------------------------------------------------------------------------ bcbf_cbc_socp
@DTYPES
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("m", [1, 3])
def test_fused_cbc_socp_equals_two_step_path_at_the_edge_sizes(ops, m, n, dtype):
    """bcbf_cbc_socp == bcbf_cbc_terms + bcbf_socp for random SPD A and B_k (cstatus 0), every cone relaxed (every program
    feasible), and the solved y is optimal for the cones the device wrote."""
    rng = np.random.default_rng(300 + 10 * m + n)
    Bt, K, C = 19, 4, m + 1

    def spd(k):
        a = rng.normal(size=(Bt, k, k))
        return a @ a.transpose(0, 2, 1) * rng.uniform(0.01, 1.0, size=(Bt, 1, 1)) + 1e-3 * np.eye(k)

    t = dict(Mk=0.3 * rng.normal(size=(Bt, n, C)), Bk=spd(C), A=spd(n), grad=rng.normal(size=(Bt, K, n)),
             cst=rng.normal(size=(Bt, K)), sign=rng.choice([-1.0, 1.0], size=K), fhat=rng.normal(size=(Bt, n)),
             ghat=rng.normal(size=(Bt, n, m)), w=0.33 * 10.0 ** rng.uniform(-3, 3, size=(Bt, C)),
             r=5.0 * rng.normal(size=(Bt, m)), mask=np.ones(K), rho=rng.choice(cr.RHOS, size=Bt))
    d = {k: dev(v, dtype) for k, v in t.items()}
    terms, cones, cstatus = ops.cbc_terms(d["Mk"], d["Bk"], d["A"], d["grad"], d["cst"], d["sign"], d["fhat"], d["ghat"])
    y1, st1, it1 = ops.socp(d["w"], d["r"], cones, d["mask"], d["rho"])
    y2, st2, it2, cones2, cstatus2, terms2 = ops.cbc_socp(d["Mk"], d["Bk"], d["A"], d["grad"], d["cst"], d["sign"], d["fhat"],
                                                          d["ghat"], d["w"], d["r"], d["mask"], d["rho"], want_terms=True)
    assert (ihost(cstatus) == 0).all()
    tol = 1e-12 if dtype == F64 else 1e-5                  # (the tolerances of test_fused_cbc_socp_equals_two_step_path)
    rel_close(host(terms2), host(terms), tol, what="terms")
    rel_close(host(cones2), host(cones), tol, what="cones")
    assert torch.equal(cstatus, cstatus2) and torch.equal(st1, st2)
    st = ihost(st2)
    assert (st == OPTIMAL).all(), st
    all_close(host(y2), host(y1), *x_tol(dtype), what="fused y vs two-step y")
    # the program the device solved: its own cones (as stored), the inputs as the device read them
    A_, b_, c_, d_ = (host(v) for v in ops.unpack_cones(cones2, m))
    p = dict(A=A_, b=b_, c=c_, d=d_, w=host(d["w"]), r=host(d["r"]), rho=host(d["rho"]))
    progs = [cr.clf_cbf_generic_form(p, t["mask"], i) for i in range(Bt)]
    sols, kept = cr.solve_batch(progs)
    # these programs are not a family of the helper: the reference's worst figure is taken on them, beside the family's
    ref = [cr.figures(progs[i], sols[i]["z"], sols[i]["x"]) for i in range(Bt) if kept[i]]
    eps = tuple(min(cr.ACCEPT, 10.0 * max(w, max(f[j] for f in ref))) for j, w in enumerate(cr.REF_WORST["clf_cbf"]))
    check_optimal(progs, sols, kept, host(y2), "clf_cbf", rounded=dtype == F32, eps=eps, what="cbc_socp m=%d n=%d" % (m, n))


# ------------------------------------------------------------------------------------------------ bcbf_coneqp_f64
@pytest.mark.parametrize("shape", cr.GENERIC_SHAPES, ids=str)
def test_coneqp_is_optimal_up_to_its_limits(ops, shape):
    """Narrow (<= 4 cones) and wide instantiation up to nv = 6, l = 8, cone dimension 6, eight cones (56 rows); Bt = 65 puts
    one lane alone into a second workgroup."""
    p, progs, sols, kept = cr.generic_case("generic", cr.generic_seed(*shape), cr.CONEQP_BT, *shape)
    x, st, it = solve_generic(ops, p)
    assert (st == OPTIMAL).all(), st
    check_optimal(progs, sols, kept, x, "generic", what="coneqp %s" % (shape,))
    check_against_x(sols, kept, x, 1e-7, 1e-8, what="x vs oracle coneqp")


@pytest.mark.parametrize("shape", cr.P0_SHAPES, ids=str)
def test_coneqp_without_a_quadratic_term(ops, shape):
    """P = 0 batched -- what SOCPController and the pendulum step send.  No lower bound exists there: x is held to the
    reference (whose own KKT residuals are asserted small), feasibility as everywhere."""
    p, progs, sols, kept = cr.generic_case("p0", cr.generic_seed(*shape), cr.CONEQP_BT, *shape)
    assert all(cr.p0_reference_is_a_solution(pr, s) for pr, s, k in zip(progs, sols, kept) if k)
    x, st, it = solve_generic(ops, p)
    assert (st == OPTIMAL).all(), st
    check_optimal(progs, sols, kept, x, "p0", what="coneqp P=0 %s" % (shape,))
    check_against_x(sols, kept, x, 1e-7, 1e-8, what="x vs oracle coneqp P=0")


def test_coneqp_result_does_not_depend_on_the_position_in_the_batch(ops):
    p, _, _, _ = cr.generic_case("generic", cr.generic_seed(*cr.MIXED_SHAPE), cr.CONEQP_BT, *cr.MIXED_SHAPE)
    order = np.random.default_rng(2).permutation(cr.CONEQP_BT)
    x0, st0, it0 = solve_generic(ops, p)
    x1, st1, it1 = solve_generic(ops, p, order=order)
    assert np.array_equal(x1, x0[order]) and np.array_equal(st1, st0[order]) and np.array_equal(it1, it0[order])


def test_coneqp_claimed_optimum_is_an_optimum_under_low_iteration_caps(ops):
    p, progs, sols, kept = cr.generic_case("generic", cr.generic_seed(*cr.MIXED_SHAPE), cr.CONEQP_BT, *cr.MIXED_SHAPE)
    check_low_iteration_runs(lambda mi: solve_generic(ops, p, max_iters=mi), progs, sols, kept, "generic", "coneqp")


def test_coneqp_statuses_inside_a_mixed_wave(ops):
    """This solver has no infeasibility exit: the infeasible instance ends MAXITER or DIVERGED, never OPTIMAL."""
    p0, _, _, _ = cr.generic_case("generic", cr.generic_seed(*cr.MIXED_SHAPE), 20, *cr.MIXED_SHAPE)
    x0, st0, it0 = solve_generic(ops, p0)
    assert (st0 == OPTIMAL).all()
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p["G"][5, 0], p["h"][5, 0] = [1.0, 0.0, 0.0], -2.0          # x0 <= -2
    p["G"][5, 1], p["h"][5, 1] = [-1.0, 0.0, 0.0], -2.0         # x0 >= 2
    p["h"][11, 3] = np.nan
    p["P"][12, 0, 0] = np.inf
    x, st, it = solve_generic(ops, p)
    bad = [5, 11, 12]
    assert np.isin(st[bad], (MAXITER, DIVERGED)).all(), st[bad]
    rest = np.delete(np.arange(20), bad)
    assert np.array_equal(x[rest], x0[rest]) and np.array_equal(st[rest], st0[rest]) and np.array_equal(it[rest], it0[rest])


# ------------------------------------------------------------------------------------------------ argument refusals
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


SENTINEL = -7


@pytest.mark.parametrize("nv,l,qdims", [(7, 1, []), (3, 9, []), (3, 0, [1]), (3, 0, [7]), (3, 0, [2] * 9), (3, 0, [])],
                         ids=["nv7", "l9", "cone1", "cone7", "nine_cones", "no_rows"])
def test_coneqp_refuses_sizes_outside_its_limits(ops, nv, l, qdims):
    from bayesian_cbf_amd._lib import lib
    Bt, Kt = 3, max(1, l + sum(qdims))
    P, q = torch.zeros(Bt, nv, nv, dtype=F64, device=DEV), torch.zeros(Bt, nv, dtype=F64, device=DEV)
    G, h = torch.zeros(Bt, Kt, nv, dtype=F64, device=DEV), torch.ones(Bt, Kt, dtype=F64, device=DEV)
    x = torch.full((Bt, nv), float(SENTINEL), dtype=F64, device=DEV)
    st = torch.full((Bt,), SENTINEL, dtype=torch.int32, device=DEV)
    it = torch.full((Bt,), SENTINEL, dtype=torch.int32, device=DEV)
    qd = (ctypes.c_int * max(1, len(qdims)))(*qdims)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.bcbf_coneqp_f64(_p(P), _p(q), _p(G), _p(h), nv, l, qd, len(qdims), _p(x), _p(st), _p(it), Bt, 100, stream)
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert (x == SENTINEL).all() and (st == SENTINEL).all() and (it == SENTINEL).all()          # nothing was launched


@pytest.mark.parametrize("m,K", [(2, 5), (4, 2)], ids=["K5", "m4"])
def test_socp_refuses_sizes_outside_its_limits(ops, m, K):
    from bayesian_cbf_amd._lib import lib
    Bt = 3
    w, r = torch.ones(Bt, m + 1, dtype=F64, device=DEV), torch.zeros(Bt, m, dtype=F64, device=DEV)
    cones = torch.zeros(Bt, K, ops.cone_width(m), dtype=F64, device=DEV)
    mask, rho = torch.zeros(K, dtype=F64, device=DEV), torch.ones(Bt, dtype=F64, device=DEV)
    y = torch.full((Bt, m + 1), float(SENTINEL), dtype=F64, device=DEV)
    st = torch.full((Bt,), SENTINEL, dtype=torch.int32, device=DEV)
    it = torch.full((Bt,), SENTINEL, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.bcbf_socp_f64(_p(w), _p(r), _p(cones), _p(mask), _p(rho), _p(y), _p(st), _p(it), Bt, K, m, 100, stream)
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert (y == SENTINEL).all() and (st == SENTINEL).all() and (it == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ ops._socp_generic
@DTYPES
@pytest.mark.parametrize("m,K", cr.WIDE_SHAPES)
def test_socp_with_five_and_eight_cones_is_optimal(ops, m, K, dtype):
    """K = 5 and K = 8 = BCBF_MAX_CONSTRAINTS for every m, per-instance rho: `ops.socp` routes to `_socp_generic`, the bound is
    taken on the program in the generic form it assembles."""
    f32 = dtype == F32
    p, mask, progs, sols, kept = cr.clf_cbf_case(cr.clf_cbf_seed(m, K), cr.WIDE_BT, m, K, "first", f32)
    y, st, it = solve_quad(ops, p, mask, dtype)
    assert (st == OPTIMAL).all(), st
    check_optimal(progs, sols, kept, y, "clf_cbf", rounded=f32, what="socp_generic m=%d K=%d" % (m, K))
    check_against_x(sols, kept, y, *x_tol(dtype), what="y vs oracle socp_generic")


@DTYPES
def test_quad_and_generic_solver_agree_on_the_same_programs(ops, dtype):
    """K = 4, m = 2: two independent device solvers, one set of programs."""
    p, mask, _, _, _ = cr.clf_cbf_case(cr.clf_cbf_seed(2, 4), cr.QUAD_BT, 2, 4, "first", dtype == F32)
    cones = ops.pack_cones(*(dev(p[k], dtype) for k in ("A", "b", "c", "d")))
    args = (dev(p["w"], dtype), dev(p["r"], dtype), cones, dev(mask, dtype), dev(p["rho"], dtype))
    yq, stq, _ = ops.socp(*args)
    yg, stg, _ = ops._socp_generic(*args)
    assert (ihost(stq) == OPTIMAL).all() and (ihost(stg) == OPTIMAL).all()
    all_close(host(yq), host(yg), *x_tol(dtype), what="quad y vs generic y")
