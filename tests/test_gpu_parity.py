"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the golden
vectors recorded from the executed reference.  Tolerances (BASELINE.json north_star):
fp64 1e-5 relative (we hold 1e-8 or better), fp32 1e-3 relative -- relative to the scale of the
quantity (for the posterior covariance: the prior scale s2*|Bm|, because B_k is a difference of
nearly equal numbers near training data; see DESIGN.md "Tolerances")."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cbc as ocbc
from oracle import gp_posterior as ogp
from oracle import socp as osocp
from oracle import unicycle as ouni

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POSTERIOR_FILES = sorted(glob.glob(os.path.join(GOLDEN, "posterior_*.npz")))
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def host(t):
    return t.detach().cpu().double().numpy()


from _tolreport import rel_close, all_close  # noqa: E402,F401


TOL = {torch.float64: 1e-8, torch.float32: 1e-3}


# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("path", POSTERIOR_FILES, ids=os.path.basename)
def test_refit_and_posterior_vs_reference_golden(ops, path, dtype):
    """K1+K2+K3+K5 on the golden cases recorded from the reference (N in {8,16,64}: padding paths)."""
    g = np.load(path)
    tol = TOL[dtype]
    X, U, Xdot = g["X"], g["U"], g["Xdot"]
    N, n = X.shape
    m = U.shape[1]
    UH = ogp.homogeneous_controls(U)
    jit = 1e-5 * g["jitter_rand"][0]
    args = [dev(a[None], dtype) for a in (X, UH, g["B"], g["ell"], np.array(float(g["s2"])), jit)]
    Kb = ops.kb_build(*args)
    Kb_ref = ogp.kb_matrix(X, UH, g["B"], g["ell"], float(g["s2"])) + np.diag(jit)
    rel_close(host(Kb)[0], Kb_ref, 1e-12 if dtype == torch.float64 else 1e-6, what="Kb")
    Lop, UHB, info, Ld = ops.refit(*args, want_dense=True)
    assert int(info[0]) == 0
    rel_close(host(Ld)[0], g["L"], tol, what="L")
    rel_close(host(UHB)[0], UH @ g["B"], tol, what="UHB")
    # potrf on the dense matrix gives the same operator
    Lop2, info2, Ld2 = ops.potrf(Kb, want_dense=True)
    assert int(info2[0]) == 0
    rel_close(host(Ld2)[0], g["L"], tol, what="L(potrf)")
    if dtype == torch.float64:     # the inverted diagonal blocks are ill-conditioned: compare them in fp64 only
        rel_close(host(Lop2), host(Lop), tol, what="Lop(potrf)")
    Vw, alpha = ops.potrs(Lop, dev(Xdot[None], dtype), args[1], dev(g["M0"][None], dtype))
    Y = ogp.residual_targets(Xdot, UH, g["M0"])
    import scipy.linalg as sla
    # Vw = L^-1 Y and alpha = K_b^-1 Y are outputs of the C ABI (bcbf_potrs).  Entry by entry they carry cond(K_b) eps (the
    # reference only exposes mean / cov); fp64 is held to the oracle's values, fp32 through what DEFINES them -- the residuals
    # L Vw = Y and K_b alpha = Y at north_star's 1e-3 (of |Y|) -- and loosely entry by entry
    itol = tol if dtype == torch.float64 else 2e-2
    rel_close(host(Vw)[0], sla.solve_triangular(g["L"], Y, lower=True), itol, what="Vw")
    if dtype == torch.float64:
        rel_close(host(alpha)[0], ogp.cholesky_solve(Y, g["L"]), tol, what="alpha")
    Kb_j = Kb_ref
    rel_close(g["L"] @ host(Vw)[0], Y, 1e-9 if dtype == torch.float64 else 1e-3, scale=np.abs(Y).max(), what="L Vw = Y")
    rel_close(Kb_j @ host(alpha)[0], Y, 1e-7 if dtype == torch.float64 else 1e-3, scale=np.abs(Y).max(), what="K_b alpha = Y")
    # per-step posterior at the golden single query, explicit second jitter
    xq = g["Xtest"][:1]
    j2 = 1e-5 * g["one_jitter2"][None]
    Mk, Bk = ops.posterior_step(Lop, Vw, args[0], UHB, args[3], args[4], args[2], dev(g["M0"][None], dtype),
                                dev(xq, dtype), dev(j2, dtype))
    prior = float(g["s2"]) * np.abs(g["B"]).max()
    rel_close(host(Mk)[0], g["one_mean_k"][0], tol, scale=max(1.0, np.abs(g["one_mean_k"]).max()), what="Mk")
    rel_close(host(Bk)[0], g["one_BkXX"][0, 0], tol, scale=prior, what="Bk")


@pytest.mark.parametrize("dtype,N,n,m,variant", [
    (torch.float64, 256, 2, 1, "dense"),      # BASELINE config 2 shape
    (torch.float32, 512, 3, 2, "dense"),      # BASELINE config 3 shape
    (torch.float64, 512, 3, 2, "theta"),      # rank-deficient shift-invariant inputs, fp64
    (torch.float32, 100, 3, 2, "dense"),      # ragged N (padding to 128)
    (torch.float32, 1024, 3, 3, "dense"),     # 2 waves per instance, m = 3
    (torch.float64, 96, 1, 1, "dense"),
    (torch.float32, 200, 6, 2, "dense"),      # state dimension > 4: the NS = 8 instantiations
    (torch.float64, 130, 5, 3, "dense"),
])
def test_posterior_pipeline_vs_oracle(ops, dtype, N, n, m, variant):
    from bayesian_cbf_amd.synthetic import make_instances
    Bt = 6
    tol = TOL[dtype]
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=7 + N, variant=variant)
    Lop, UHB, info, Ld = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], want_dense=True)
    assert (info == 0).all()
    Vw, alpha = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    Mk, Bk = ops.posterior_step(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"], p["jitter2"])
    h = {k: host(v) for k, v in p.items()}
    for i in range(Bt):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jitter"][i][None] / 1e-5)
        Lref = st["L"]
        # factor: compare through the reconstruction (robust to conditioning), fp32 only loosely
        Lg = host(Ld)[i]
        rec = Lg @ Lg.T
        rel_close(rec, st["Kbp"], 1e-12 if dtype == torch.float64 else 2e-6, what="L L' = Kb")
        if dtype == torch.float64 and variant == "dense":
            rel_close(Lg, Lref, 1e-8, what="L")
        Mk_o, Bk_o = ogp.posterior_step(Lref[None], st["alpha"][None], h["X"][i][None], st["UHB"][None],
                                        h["ell"][i][None], h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None],
                                        h["xq"][i][None], jitter2=h["jitter2"][i][None])
        prior = h["s2"][i] * np.abs(h["Bm"][i]).max()
        t = tol if variant == "dense" else 1e-5
        rel_close(host(Mk)[i], Mk_o[0], t, scale=max(1.0, np.abs(Mk_o).max()), what="Mk[%d]" % i)
        rel_close(host(Bk)[i], Bk_o[0], t, scale=prior, what="Bk[%d]" % i)


def test_cholesky_failure_is_reported_per_instance(ops):
    """info = 1-based index of the failing pivot; healthy instances are unaffected (make_psd retry
    protocol, control_affine_model.py:905-919)."""
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(3, 64, 2, 1, dtype=torch.float64, device=DEV, seed=3)
    X = p["X"].clone()
    X[1, 40] = X[1, 7]                      # duplicated point ...
    UH = p["UH"].clone()
    UH[1, 40] = UH[1, 7]
    jit = p["jitter"].clone()
    jit[1] = 0.0                            # ... and no jitter: K_b is singular
    jit[1, 40] = -1e-3
    Lop, UHB, info, _ = ops.refit(X, UH, p["Bm"], p["ell"], p["s2"], jit)
    info = info.cpu().numpy()
    assert info[0] == 0 and info[2] == 0 and info[1] == 41


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_chol_append_equals_refit(ops, dtype):
    from bayesian_cbf_amd.synthetic import make_instances
    tol = 1e-9 if dtype == torch.float64 else 1e-3      # (fp32 measured: 4.9e-7, tools/tol_report.py)
    for N in (31, 32, 45, 64):     # append inside a block, across a block boundary
        p = make_instances(4, N + 1, 3, 2, dtype=dtype, device=DEV, seed=N)
        full = ops.kb_build(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
        Lop_full, info_f, Ld_full = ops.potrf(full, want_dense=True)
        Lop_N, info_n, _ = ops.potrf(full[:, :N, :N].contiguous())
        knew = full[:, N, :N].contiguous()
        kappa = full[:, N, N].contiguous()
        Lop_app, info_a = ops.chol_append(Lop_N, knew, kappa, N)
        assert (info_a == 0).all() and (info_f == 0).all()
        rel_close(host(Lop_app), host(Lop_full), tol, what="chol_append N=%d" % N)


# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tag", ["fixed", "learned_N40"])
def test_unicycle_terms_vs_reference_golden(ops, tag, dtype):
    """Task functions (K8 inputs), rel-degree-1 terms and cone conversion against the vectors
    recorded from ControllerCLFBayesian._clc_terms/_cbc_terms (jitter replayed explicitly)."""
    g = np.load(os.path.join(GOLDEN, "unicycle_terms_%s.npz" % tag))
    learning = bool(g["enable_learning"])
    tol = 1e-8 if dtype == torch.float64 else 2e-4
    S = len(g["ts"])
    x = dev(g["states"], dtype)
    plan = dev(np.stack([g["s%d_plan" % i] for i in range(S)]), dtype)
    dplan = dev(np.stack([g["s%d_dot_plan" % i] for i in range(S)]), dtype)
    centers = dev(np.broadcast_to(g["obst_centers"], (S, 2, 2)), dtype)
    radii = dev(np.broadcast_to(g["obst_radii"], (S, 2)), dtype)
    grad, cst, fhat, ghat = ops.unicycle_constraints(x, plan, dplan, dev(g["Kp"], dtype), float(g["clf_gamma"]),
                                                     centers, radii, dev(g["term_weights"], dtype),
                                                     dev(g["cbf_gammas"], dtype), float(g["mean_L"]))
    for i in range(S):
        p = "s%d_" % i
        rel_close(host(grad)[i, 0], g[p + "grad_V"], tol, scale=max(1.0, np.abs(g[p + "grad_V"]).max()), what="grad_V")
        rel_close(host(grad)[i, 1:], g[p + "grad_h"], tol, scale=max(1.0, np.abs(g[p + "grad_h"]).max()), what="grad_h")
        rel_close(host(cst)[i, 1:], g["cbf_gammas"] * g[p + "h"], tol, scale=max(1.0, np.abs(g[p + "h"]).max() * 5), what="gamma h")
    # model at each state
    if learning:
        X, U, Xdot = g["X"], g["U"], g["Xdot"]
        UH = ogp.homogeneous_controls(U)
        rep = lambda a: dev(np.broadcast_to(a, (S,) + np.shape(a)), dtype)
        Lop, info, _ = ops.potrf(rep(g["L"] @ g["L"].T))
        assert (info == 0).all()
        Vw, _ = ops.potrs(Lop, rep(Xdot), rep(UH), rep(g["M0"]))
        A = rep(g["A"])
    else:
        A = dev(np.broadcast_to(np.diag(g["kernel_diag_A"]), (S, 3, 3)), dtype)
    sign = dev(np.array([-1.0, 1.0, 1.0]), dtype)
    names = ("bfe", "e", "V", "bfv", "v")
    for k in range(3):       # constraint k uses its own jitter draw in the reference -> one pass per k
        if learning:
            j2 = []
            for i in range(S):
                draws = [g["s%d_draw%d" % (i, q)] for q in range(int(g["s%d_ndraws" % i]))]
                if i == 0:
                    draws = [draws[0]] + draws[2:]
                j2.append(1e-5 * draws[3 * k + 1])
            Mk, Bk = ops.posterior_step(Lop, Vw, rep(X), rep(UH @ g["B"]), rep(g["ell"]), rep(np.array(float(g["s2"]))),
                                        rep(g["B"]), rep(g["M0"]), x, dev(np.stack(j2), dtype))
        else:
            Mk = torch.zeros(S, 3, 3, dtype=dtype, device=DEV)
            Bk = torch.eye(3, dtype=dtype, device=DEV).expand(S, 3, 3).contiguous()
        terms, cones, cstatus = ops.cbc_terms(Mk, Bk, A, grad, cst, sign, fhat, ghat)
        assert (cstatus == 0).all()
        got = [host(t) for t in ops.unpack_terms(terms, 2)]
        gotc = [host(t) for t in ops.unpack_cones(cones, 2)]
        for i in range(S):
            p = "s%d_" % i
            for name, val in zip(names, got):
                ref = g[p + "clc_" + name] if k == 0 else g[p + "cbc_" + name][k - 1]
                rel_close(val[i, k], ref, tol, scale=max(np.abs(ref).max(), 1e-2), what="%s[%d,%d]" % (name, i, k))
            for name, val in zip(("A", "b", "c", "d"), gotc):
                ref = g[p + "clc_socp_" + name] if k == 0 else g[p + "cbc_socp_" + name][k - 1]
                rel_close(val[i, k], ref, tol * 5, scale=max(np.abs(ref).max(), 1e-2), what="cone %s[%d,%d]" % (name, i, k))


# --------------------------------------------------------------------------------------------
def _random_programs(rng, Bt, m=2, K=3, rho=2.326):
    A = np.zeros((Bt, K, m + 1, m)); b = np.zeros((Bt, K, m + 1)); c = np.zeros((Bt, K, m)); d = np.zeros((Bt, K))
    for i in range(Bt):
        u_f = rng.normal(size=m)
        for k in range(K):
            Asq = rng.normal(size=(m + 1, m + 1))
            Asq = Asq @ Asq.T * rng.uniform(0.001, 1) + 1e-4 * np.eye(m + 1)
            Lc = np.linalg.cholesky(Asq)
            A[i, k], b[i, k] = Lc.T[:, 1:], Lc.T[:, 0]
            c[i, k] = rng.normal(size=m) * 3
            slack = rng.uniform(0.01, 2.0) * (1 if k else rng.choice([-1, 1]))
            d[i, k] = rho * np.linalg.norm(A[i, k] @ u_f + b[i, k]) - c[i, k] @ u_f + slack
    return A, b, c, d


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("m,K", [(2, 3), (1, 2), (3, 4), (2, 1)])
def test_socp_vs_oracle(ops, dtype, m, K):
    rng = np.random.default_rng(100 + 10 * m + K)
    Bt, rho = 96, 2.326
    A, b, c, d = _random_programs(rng, Bt, m, K, rho)
    relax_mask = np.zeros(K); relax_mask[0] = 1.0
    w = np.full((Bt, m + 1), 0.33) * rng.uniform(0.5, 2.0, size=(Bt, m + 1))
    r = rng.normal(size=(Bt, m)) * 0.3
    if dtype == torch.float32:      # both sides solve the same (fp32-representable) program
        A, b, c, d, w, r = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (A, b, c, d, w, r))
    cones = ops.pack_cones(dev(A, dtype), dev(b, dtype), dev(c, dtype), dev(d, dtype))
    y, status, iters = ops.socp(dev(w, dtype), dev(r, dtype), cones, dev(relax_mask, dtype), dev(np.full(Bt, rho), dtype))
    assert (status == 0).all(), status.cpu().numpy()
    assert int(iters.max()) <= 30
    yh = host(y)
    for i in range(Bt):
        sol = osocp.clf_cbf_socp(w[i], r[i], [(A[i, k], b[i, k], c[i, k], d[i, k]) for k in range(K)], rho, relax_mask)
        assert sol["status"] == "optimal"
        # fp32 entry point: the iterates are fp64 behind it, measured 1.7e-7 over this family
        all_close(yh[i], sol["x"], 1e-6 if dtype == torch.float64 else 1e-3, 1e-7 if dtype == torch.float64 else 1e-3, what="y vs oracle socp")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_cbc_socp_equals_two_step_path(ops, dtype):
    """bcbf_cbc_socp (terms + cones + solve in one launch) == bcbf_cbc_terms followed by bcbf_socp."""
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    Bt = 70                                  # not a multiple of 64: exercises the shadow quads
    p = make_instances(Bt, 64, 3, 2, dtype=dtype, device=DEV, seed=31)
    t = make_unicycle_task(Bt, dtype=dtype, device=DEV, seed=32)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    Mk, Bk = ops.posterior_step(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], t["x"])
    grad, cst, fhat, ghat = ops.unicycle_constraints(t["x"], t["plan"], t["dot_plan"], t["Kp"], 10.0, t["centers"],
                                                     t["radii"], t["tw"], t["gammas"], 4.0)
    terms, cones, cstatus = ops.cbc_terms(Mk, Bk, p["A"], grad, cst, t["sign"], fhat, ghat)
    y1, st1, it1 = ops.socp(t["w"], t["r"], cones, t["relax_mask"], t["rho"])
    y2, st2, it2, cones2, cstatus2, terms2 = ops.cbc_socp(Mk, Bk, p["A"], grad, cst, t["sign"], fhat, ghat, t["w"],
                                                          t["r"], t["relax_mask"], t["rho"], want_terms=True)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    rel_close(host(terms2), host(terms), tol, what="terms")
    rel_close(host(cones2), host(cones), tol, what="cones")
    assert torch.equal(cstatus, cstatus2) and torch.equal(st1, st2)
    ok = (st1 == 0).cpu().numpy()
    assert ok.sum() >= 10          # (this small-N synthetic task leaves many programs infeasible)
    all_close(host(y2)[ok], host(y1)[ok], 1e-6 if dtype == torch.float64 else 1e-3, 1e-7 if dtype == torch.float64 else 1e-3, what="fused y vs two-step y")


def test_socp_flags_infeasible_instances_without_disturbing_others(ops):
    rng = np.random.default_rng(0)
    A, b, c, d = _random_programs(rng, 8)
    # instance 3: two contradictory half-planes (u0 >= 2 and u0 <= -2), no relaxation on them
    A[3, 1] = A[3, 2] = np.eye(3)[:, 1:]
    b[3, 1] = b[3, 2] = [1.0, 0, 0]
    c[3, 1], c[3, 2] = [1.0, 0.0], [-1.0, 0.0]
    d[3, 1] = d[3, 2] = -1.0
    dt = torch.float64
    cones = ops.pack_cones(dev(A, dt), dev(b, dt), dev(c, dt), dev(d, dt))
    y, status, _ = ops.socp(dev(np.full((8, 3), 0.33), dt), dev(np.zeros((8, 2)), dt), cones,
                            dev(np.array([1.0, 0, 0]), dt), dev(np.full(8, 1.0), dt))
    st = status.cpu().numpy()
    assert st[3] != 0 and (np.delete(st, 3) == 0).all()


def test_coneqp_known_answer_from_reference_tests(ops):
    """tests/test_optimizers.py:6-26 of the reference (cvxopt doc SOCP): x = [-5.02,-5.77,-8.52]."""
    from kat import cvxopt_doc_example
    lin, cons = cvxopt_doc_example()
    _, Gqs, hqs = osocp.convert_socp_to_cvxopt_format(lin, cons)
    G = np.vstack(Gqs); h = np.concatenate([q[:, 0] for q in hqs])
    dt = torch.float64
    x, status, iters = ops.coneqp(dev(np.zeros((1, 3, 3)), dt), dev(lin[None], dt), dev(G[None], dt), dev(h[None], dt),
                                  0, [3, 4])
    assert int(status[0]) == 0
    np.testing.assert_allclose(host(x)[0], [-5.02, -5.77, -8.52], rtol=1e-2, atol=1e-3)
    np.testing.assert_allclose(host(x)[0], osocp.optimizer_socp(lin, cons)["x"], rtol=1e-7, atol=1e-8)
    # QP with linear inequalities (optimizer_qp_cvxpy shape): min |A y + b|^2 s.t. 0 <= c'y + d
    rng = np.random.default_rng(4)
    Aq, bq = rng.normal(size=(3, 2)), rng.normal(size=3)
    lincons = [("a", (np.array([1.0, 0.5]), 0.3)), ("b", (np.array([-0.2, 1.0]), -0.1))]
    sol = osocp.optimizer_qp((Aq, bq), lincons)
    P = 2 * Aq.T @ Aq; q = 2 * Aq.T @ bq
    Gl = np.stack([-cc for _, (cc, _) in lincons]); hl = np.array([dd for _, (_, dd) in lincons])
    x, status, _ = ops.coneqp(dev(P[None], dt), dev(q[None], dt), dev(Gl[None], dt), dev(hl[None], dt), 2, [])
    assert int(status[0]) == 0
    np.testing.assert_allclose(host(x)[0], sol["x"], rtol=1e-7, atol=1e-8)


@pytest.mark.parametrize("name", ["saved_run_mean_cbf_maxrisk0p5", "saved_run_bayes_cbf_maxrisk0p01"])
def test_saved_run_controls_end_to_end(ops, name):
    """All 200 logged states of the reference's committed runs at once: task functions -> terms ->
    cones -> SOCP on the GPU reproduces the logged GUROBI controls, and one Euler step of the
    true plant reproduces the logged next state."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    dt_, T = float(g["dt"]), int(g["numSteps"])
    x0, xg = g["state_start"], g["state_goal"]
    planner = ouni.PiecewiseLinearPlanner(x0, xg, T, dt_, frac_time_to_reach_goal=0.95)
    cbfs = ouni.obstacles_at_mid_from_start_and_goal(x0, xg, tuple(g["term_weights"]))
    dt = torch.float64
    S = T
    x = dev(g["state"].astype(np.float64), dt)
    plan = dev(np.stack([planner.plan(t) for t in range(T)]), dt)
    dplan = dev(np.stack([planner.dot_plan(t) for t in range(T)]), dt)
    centers = dev(np.broadcast_to(np.stack([c.center for c in cbfs]), (S, 2, 2)), dt)
    radii = dev(np.broadcast_to(np.array([c.radius for c in cbfs]), (S, 2)), dt)
    grad, cst, fhat, ghat = ops.unicycle_constraints(x, plan, dplan, dev(np.array([0.9, 1.5, 0.0]), dt),
                                                     float(g["clf_gamma"]), centers, radii, dev(g["term_weights"], dt),
                                                     dev(g["cbf_gammas"], dt), float(g["mean_L"]))
    Mk = torch.zeros(S, 3, 3, dtype=dt, device=DEV)
    Bk = torch.eye(3, dtype=dt, device=DEV).expand(S, 3, 3).contiguous()
    A = dev(np.broadcast_to(np.diag(g["kernel_diag_A"]), (S, 3, 3)), dt)
    terms, cones, cstatus = ops.cbc_terms(Mk, Bk, A, grad, cst, dev(np.array([-1.0, 1, 1]), dt), fhat, ghat)
    assert (cstatus == 0).all()
    rho = ocbc.cbc1_safety_factor(float(g["max_risk"]))
    y, status, iters = ops.socp(dev(np.broadcast_to(g["cost_weights"], (S, 3)), dt), torch.zeros(S, 2, dtype=dt, device=DEV),
                                cones, dev(np.array([1.0, 0, 0]), dt), dev(np.full(S, rho), dt))
    assert (status == 0).all()
    yh = host(y)
    # (fp64 here; the bound is the RECORD's precision: GUROBI's barrier tolerance and the float32 event file it was logged
    #  to -- measured 1.55e-3; the oracle's solver agrees with the device to 1e-7, test_socp_vs_oracle)
    all_close(yh[:, :2], g["uopt"], 2e-3, 2e-3, what="uopt vs GUROBI run")
    value = (g["cost_weights"] * yh ** 2).sum(axis=1)
    np.testing.assert_allclose(value, g["opt_value"], rtol=1e-4, atol=1e-5)
    xs = x.clone()
    ops.unicycle_step(xs, dev(g["uopt"].astype(np.float64), dt), dt_, float(g["true_L"]))
    np.testing.assert_allclose(host(xs)[:-1], g["state"][1:], atol=5e-6)


# --------------------------------------------------------------------------------------------
def test_full_size_properties_config3(ops):
    """BASELINE config 3 at full size (N=512, n=3, m=2, batch=4096, fp32): size-independent
    properties + a sampled comparison with the oracle."""
    from bayesian_cbf_amd.synthetic import make_instances
    Bt, N, n, m = 4096, 512, 3, 2
    dtype = torch.float32
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=1234)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert (info == 0).all()
    Vw, alpha = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    Mk, Bk = ops.posterior_step(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
    assert torch.isfinite(Mk).all() and torch.isfinite(Bk).all()
    prior = p["s2"][:, None, None] * p["Bm"]
    # (1) symmetry, (2) 0 <= B_k <= prior on the diagonal (variance reduction), (3) PSD up to rounding
    assert (Bk - Bk.transpose(1, 2)).abs().max() == 0
    d, dp = torch.diagonal(Bk, dim1=1, dim2=2), torch.diagonal(prior, dim1=1, dim2=2)
    assert (d <= dp * (1 + 1e-5)).all() and (d >= -1e-3 * dp).all()
    ev = torch.linalg.eigvalsh(Bk.double().cpu())
    assert (ev.min(dim=1).values >= -1e-3 * dp.double().cpu().max(dim=1).values).all()
    # (4) a query at a training point reproduces that point's fitted target: Mk [1;u_j] ~ xdot_j
    xq2 = p["X"][:, 17, :].contiguous()
    Mk2, Bk2 = ops.posterior_step(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq2)
    pred = torch.einsum("bnc,bc->bn", Mk2, p["UH"][:, 17, :])
    assert (pred - p["Xdot"][:, 17, :]).abs().max() < 5e-2
    var_at_train = torch.einsum("bc,bcd,bd->b", p["UH"][:, 17, :], Bk2, p["UH"][:, 17, :])
    assert (var_at_train.abs() < 1e-2 * torch.einsum("bc,bcd,bd->b", p["UH"][:, 17, :], prior, p["UH"][:, 17, :])).all()
    # (5) linearity of the mean in the targets: doubling Xdot doubles Mk (M0 = 0)
    Vw2, _ = ops.potrs(Lop, 2 * p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    Mk3, _ = ops.posterior_step(Lop, Vw2, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
    assert (Mk3 - 2 * Mk).abs().max() <= 1e-4 * max(1.0, float(Mk.abs().max()))
    # (6) sampled instances against the oracle
    h = {k: host(v) for k, v in p.items()}
    for i in (0, 1337, 4095):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jitter"][i][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None],
                                        h["ell"][i][None], h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None],
                                        h["xq"][i][None])
        rel_close(host(Mk)[i], Mk_o[0], 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk[%d]" % i)
        rel_close(host(Bk)[i], Bk_o[0], 1e-3, scale=float(h["s2"][i] * np.abs(h["Bm"][i]).max()), what="Bk[%d]" % i)


# --------------------------------------------------------------------------------------------
CBC2_FILES = sorted(glob.glob(os.path.join(GOLDEN, "cbc2_*.npz")))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("path", CBC2_FILES, ids=os.path.basename)
def test_reldeg2_jets_and_terms_vs_reference_golden(ops, path, dtype):
    """Posterior jets + rel-degree-2 terms (cbc2_gp / GradientGP path) against vectors recorded from the
    reference's autograd-based cbc2_quadratic_terms."""
    from oracle import cbc2 as oc2
    g = np.load(path)
    X, U, Xdot = g["X"], g["U"], g["Xdot"]
    N, n = X.shape
    m = U.shape[1]
    S = len(g["xs"])
    UH = ogp.homogeneous_controls(U)
    rep = lambda a: dev(np.broadcast_to(a, (S,) + np.shape(a)), dtype)
    jit = 1e-5 * g["jitter_rand"][0]
    Lop, UHB, info, _ = ops.refit(rep(X), rep(UH), rep(g["B"]), rep(g["ell"]), rep(np.array(float(g["s2"]))), rep(jit))
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, rep(Xdot), rep(UH), rep(g["M0"]), want_alpha=False)
    xs = dev(g["xs"], dtype)
    Mk, Bk, G, Mj = ops.posterior_jets(Lop, Vw, rep(X), UHB, rep(g["ell"]), rep(np.array(float(g["s2"]))), rep(g["B"]),
                                       rep(g["M0"]), xs)
    st = ogp.refit_state(X, U, Xdot, g["B"], g["ell"], float(g["s2"]), g["M0"], g["jitter_rand"])
    C = m + 1
    tol = 1e-8 if dtype == torch.float64 else 1e-3      # (fp32 measured: <= 7e-6 on every golden file)
    for i in range(S):
        jets = oc2.posterior_jets(st["L"], st["Y"], X, st["UHB"], g["ell"], float(g["s2"]), g["B"], g["M0"], g["xs"][i])
        rel_close(host(Mk)[i], jets["Mk"], tol, scale=max(1.0, np.abs(jets["Mk"]).max()), what="Mk")
        Gh, Mjh = host(G)[i], host(Mj)[i]
        gscale = max(np.abs(jets["G11"]).max(), np.abs(jets["G10"]).max(), 1e-3)
        for d in range(n):
            rel_close(Gh[(1 + d) * C:(2 + d) * C, :C], jets["G10"][d], tol, scale=gscale, what="G10")
            rel_close(Mjh[:, (1 + d) * C:(2 + d) * C], jets["dMk"][d], tol, scale=max(1.0, np.abs(jets["dMk"]).max()), what="dMk")
            for e in range(n):
                rel_close(Gh[(1 + d) * C:(2 + d) * C, (1 + e) * C:(2 + e) * C], jets["G11"][d][e], tol, scale=gscale, what="G11")
    out = ops.cbc2_terms(Mk, Bk, G, Mj, rep(g["A"]), rep(g["B"]), rep(g["ell"]), rep(np.array(float(g["s2"]))),
                         dev(g["t_h"].reshape(S), dtype), dev(g["t_gh"], dtype), dev(g["t_hess"], dtype),
                         dev(g["k_alpha"], dtype), dev(g["u0s"], dtype))
    (mA, mb), (Q, p, r), mean, var, status = out
    assert (status == 0).all()
    ttol = 1e-7 if dtype == torch.float64 else 1e-3     # (fp32 measured: <= 3.4e-5)
    for name, val in (("mean_A", mA), ("mean_b", mb), ("Q", Q), ("p", p), ("r", r), ("mean", mean), ("var", var)):
        ref = g["t_" + name].reshape(host(val).shape)
        rel_close(host(val), ref, ttol, scale=max(np.abs(ref).max(), 1e-2), what=name)


# --------------------------------------------------------------------------------------------
# The eigenvalue clean-up of GradientGP.knl (gp_algebra.py:384-392) with the branch FIRING
def _sign_pattern_explains(H, Href, tol):
    import itertools
    n = H.shape[0]
    return any(np.abs(np.diag(d) @ Href @ np.diag(d) - H).max() <= tol for d in itertools.product([1.0, -1.0], repeat=n))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_hessian_cleanup_on_device_vs_executed_reference(ops, dtype):
    """bcbf_clean_hessian (csrc/geev_small.h on the device) on the 96 Hessians GradientGP.knl of the executed reference
    cleaned (tests/golden/hessclean_handmade.npz; the branch fires in 80): status says fired exactly where the reference
    fired; the result is the reference's `eigenvectors.T @ diag(evalz) @ eigenvectors` for every n <= 2 case and for every
    n >= 3 case except those where LAPACK builds themselves disagree about eigenvector signs (then: that sign pattern);
    the non-default projection mode gives a different matrix."""
    g = np.load(os.path.join(GOLDEN, "hessclean_handmade.npz"))
    same = explained = differs_proj = 0
    for n in (1, 2, 3, 4):
        M, ref, fired = g["M_n%d" % n], g["t_knl_n%d" % n], g["branch_fired_n%d" % n]
        H, status = ops.clean_hessian(dev(M, dtype))
        Hp, statusp = ops.clean_hessian(dev(M, dtype), mode="project")
        H, Hp, status = host(H), host(Hp), status.cpu().numpy()
        assert ((status == 4) == fired).all() and (status[~fired] == 0).all(), (n, status, fired)
        assert (statusp.cpu().numpy() == status).all()
        for k in range(len(M)):
            # fp32: the INPUT is rounded to 6e-8 |M|, which moves the eigenvectors by that over the eigenvalue gap (>= 0.05)
            tol = (1e-10 if dtype == torch.float64 else 1e-3) * max(1.0, np.abs(M[k]).max())
            if not fired[k]:
                np.testing.assert_allclose(H[k], M[k], rtol=0, atol=tol)
                continue
            differs_proj += int(n > 1 and np.abs(Hp[k] - ref[k]).max() > 1e-4)
            if np.abs(H[k] - ref[k]).max() <= tol:
                same += 1
            else:
                assert n >= 3 and _sign_pattern_explains(H[k], ref[k], tol), (n, k, H[k], ref[k])
                explained += 1
    assert same >= 76 and same + explained == 80 and differs_proj >= 50, (same, explained, differs_proj)


@pytest.mark.timeout(120)
def test_hessian_cleanup_on_device_non_finite_input_returns(ops):
    """NaN / Inf entries: status 1 (the reference's assert fails on NaN eigenvalues), the matrix handed back as it came -- and
    the kernel RETURNS (the general solver's balancing loop would spin forever on NaN)."""
    for n in (1, 2, 3, 4):
        M = np.tile(np.eye(n) + 0.1, (6, 1, 1))
        M[1, n - 1, 0] = np.nan
        M[3, 0, n - 1] = np.inf
        M[4, 0, 0] = -np.inf
        for dtype in (torch.float64, torch.float32):
            H, status = ops.clean_hessian(dev(M, dtype))
            torch.cuda.synchronize()
            st = status.cpu().numpy()
            assert list(st) == [0, 1, 0, 1, 1, 0], (n, st)
            np.testing.assert_array_equal(host(H)[[0, 2, 5]], M[[0, 2, 5]].astype(np.float32 if dtype == torch.float32 else np.float64))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_hessian_cleanup_on_device_random_vs_general_eigensolver(ops, n):
    """4000 random near-PSD matrices per size against the reference's own statements run on torch.linalg.eig (= the
    `torch.eig` of the harness): n <= 2 identical in every case; n >= 3 identical in >= 93 % and every other case is a
    sign pattern of the same matrix (csrc/geev_small.h: sweep counts depend on rounding residues in any xGEEV)."""
    rng = np.random.RandomState(300 + n)
    Ms = []
    for t in range(4000):
        A = rng.randn(n, n)
        w, V = np.linalg.eigh(A + A.T)
        w = np.abs(w) + 0.02 * (1 + np.arange(n))
        if t % 4:
            w[0] = -rng.uniform(1e-6, 1.8e-3)
        M = (V * w) @ V.T
        M = 0.5 * (M + M.T)
        if t % 5 == 1:
            M = M + 1e-16 * rng.randn(n, n)
        if t % 3 == 0 and n > 1:
            z = rng.randint(n)
            M[z, :] = 0.0
            M[:, z] = 0.0
            w2 = np.linalg.eigvalsh(M)
            if np.min(np.diff(w2)) < 1e-6 or w2[0] <= -2e-3:
                continue
        Ms.append(M)
    Ms = np.stack(Ms)
    H, status = ops.clean_hessian(dev(Ms, torch.float64))
    H, status = host(H), status.cpu().numpy()
    lam, vec = torch.linalg.eig(torch.from_numpy(Ms))
    ev, vec = lam.real.numpy().copy(), vec.real.numpy()
    fired = ((ev > -2e-3) & (ev < 0)).any(axis=1)
    assert ((status == 4) == fired).all() and (status[~fired] == 0).all()
    same = explained = 0
    for k in np.where(fired)[0]:
        e = np.where(ev[k] < 0, 0.0, ev[k])
        ref = vec[k].T @ np.diag(e) @ vec[k]
        tol = 1e-9 * max(1.0, np.abs(Ms[k]).max())
        if np.abs(H[k] - ref).max() <= tol:
            same += 1
        else:
            assert n >= 3 and _sign_pattern_explains(H[k], ref, tol), (n, Ms[k], H[k], ref)
            explained += 1
    np.testing.assert_array_equal(H[~fired], Ms[~fired])
    print("clean_hessian n=%d: %d fired, %d identical to torch.linalg.eig's formula, %d sign patterns" % (n, fired.sum(), same, explained))
    assert fired.sum() > 1500 and (explained == 0 if n <= 2 else same >= 0.93 * fired.sum())


EIGFIRED_FILES = sorted(glob.glob(os.path.join(GOLDEN, "eigfired_*.npz")))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("path", EIGFIRED_FILES, ids=os.path.basename)
def test_reldeg2_terms_with_cleanup_branch_firing_vs_reference_golden(ops, path, dtype):
    """bcbf_posterior_jets + bcbf_cbc2_terms against cbc2_quadratic_terms(cbc2_gp(...)) of the executed reference in the
    state where GradientGP.knl's clean-up FIRES in every record: the factor is the one cached at output scale `s2_L`, the
    query runs at `s2_q[i]` (control_affine_model.py:379-385).  status == 4 (branch ran, reference formula) everywhere,
    terms within 1e-7 (fp64) / 1e-3 (fp32; measured <= 4.1e-5); the projection mode gives different terms."""
    g = np.load(path)
    X, U, Xdot = g["X"], g["U"], g["Xdot"]
    N, n = X.shape
    m = U.shape[1]
    S = len(g["xs"])
    assert g["branch_fired"].all() and g["agree_openblas"].all()
    UH = ogp.homogeneous_controls(U)
    rep = lambda a: dev(np.broadcast_to(a, (S,) + np.shape(a)), dtype)
    jit = 1e-5 * g["jitter_rand"][0]
    Lop, UHB, info, _ = ops.refit(rep(X), rep(UH), rep(g["B"]), rep(g["ell"]), rep(np.array(float(g["s2_L"]))), rep(jit))
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, rep(Xdot), rep(UH), rep(g["M0"]), want_alpha=False)
    s2q = dev(g["s2_q"], dtype)
    Mk, Bk, G, Mj = ops.posterior_jets(Lop, Vw, rep(X), UHB, rep(g["ell"]), s2q, rep(g["B"]), rep(g["M0"]), dev(g["xs"], dtype))
    args = (Mk, Bk, G, Mj, rep(g["A"]), rep(g["B"]), rep(g["ell"]), s2q, dev(g["t_h"].reshape(S), dtype), dev(g["t_gh"], dtype),
            dev(g["t_hess"], dtype), dev(g["k_alpha"], dtype), dev(g["u0s"], dtype))
    (mA, mb), (Q, p, r), mean, var, status = ops.cbc2_terms(*args)
    assert (status == 4).all(), status
    ttol = 1e-7 if dtype == torch.float64 else 1e-3
    for name, val in (("mean_A", mA), ("mean_b", mb), ("Q", Q), ("p", p), ("r", r), ("mean", mean), ("var", var)):
        ref = g["t_" + name].reshape(host(val).shape)
        rel_close(host(val), ref, ttol, scale=max(np.abs(ref).max(), 1e-2), what=name)
    out_p = ops.cbc2_terms(*args, hessian_mode="project")
    assert (out_p[4] == 4).all()
    assert np.abs(host(out_p[3]) - g["t_var"].reshape(S)).max() > 1e-5 * np.abs(g["t_var"]).max()


# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n,m,b,dtype", [(512, 3, 2, 203, torch.float32), (100, 3, 2, 8, torch.float32), (256, 3, 1, 64, torch.float32),
                                           (1024, 3, 3, 37, torch.float32), (64, 3, 1, 5, torch.float32), (1280, 3, 2, 17, torch.float32),
                                           (480, 4, 3, 37, torch.float32), (96, 2, 3, 5, torch.float32), (64, 2, 1, 40, torch.float32), (416, 4, 2, 17, torch.float32),
                                           (512, 3, 2, 203, torch.float64), (100, 3, 2, 9, torch.float64), (256, 2, 1, 64, torch.float64),
                                           (480, 4, 3, 37, torch.float64), (64, 1, 1, 5, torch.float64), (416, 4, 2, 17, torch.float64),
                                           (200, 6, 2, 17, torch.float64), (640, 3, 2, 40, torch.float64)])
def test_shared_gp_matrix_core_queries_vs_oracle(ops, N, n, m, b, dtype):
    """Regime S (custom_predict with b test points, control_affine_model.py:536, 1051): the MFMA kernels (fp32: W slab in
    LDS; fp64: W in registers, N <= 512, n <= 4) against the fp64 oracle, ragged b (not a multiple of the queries a
    wave holds) and ragged N (padding rows).  The last two fp64 cases lie outside the matrix-core kernel's range: the
    direct entry refuses them and the routed query streams them."""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(1, N, n, m, dtype=dtype, device=DEV, seed=3 + N)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert int(info[0]) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    g = torch.Generator(device="cpu").manual_seed(11)
    idx = torch.randint(0, N, (b,), generator=g)
    xq = (p["X"][0, idx.to(DEV)] + 0.3 * torch.randn(b, n, generator=g).to(DEV, dtype)).contiguous()
    j2 = (1e-5 * torch.rand(b, m + 1, generator=g)).to(DEV, dtype)
    direct = not f64 or (N <= 512 and n <= 4)
    if direct:
        Mk, Bk, W = ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, j2, want_W=True)
    else:
        with pytest.raises(ValueError):
            ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, j2, want_W=True)
        Mk, Bk, W = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, j2, shared=True, want_W=True)
    h = {k: host(v) for k, v in p.items()}
    st = ogp.refit_state(h["X"][0], h["U"][0], h["Xdot"][0], h["Bm"][0], h["ell"][0], h["s2"][0], h["M0"][0],
                         h["jitter"][0][None] / 1e-5)
    rep = lambda a: np.broadcast_to(a[None], (b,) + a.shape)
    Mk_o, Bk_o = ogp.posterior_step(rep(st["L"]), rep(st["alpha"]), rep(h["X"][0]), rep(st["UHB"]), rep(h["ell"][0]),
                                    rep(h["s2"][0]), rep(h["Bm"][0]), rep(h["M0"][0]), host(xq), jitter2=host(j2))
    prior = h["s2"][0] * np.abs(h["Bm"][0]).max()
    rel_close(host(Mk), Mk_o, 1e-9 if f64 else 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk")
    rel_close(host(Bk), Bk_o, 1e-9 if f64 else 1e-3, scale=prior, what="Bk")
    # W'W reproduces the Gram the kernel accumulated (and the routed query entry gives the same numbers)
    Wh = host(W)
    G = np.einsum("bic,bid->bcd", Wh, Wh)
    Bk_w = prior * 0 + h["s2"][0] * h["Bm"][0][None] - G + np.stack([np.diag(r) for r in host(j2)])
    rel_close(host(Bk), Bk_w, 1e-12 if f64 else 1e-4, scale=prior, what="Bk from W")
    Mk2, Bk2, _ = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, j2, shared=True)
    rel_close(host(Mk2), Mk_o, 1e-9 if f64 else 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk(query)")
    rel_close(host(Bk2), Bk_o, 1e-9 if f64 else 1e-3, scale=prior, what="Bk(query)")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N,n,m,b,bp,kernel", [(100, 2, 1, 37, 37, "rbf"), (64, 3, 2, 50, 21, "rbf"), (33, 4, 3, 16, 16, "rbf"),
                                               (130, 2, 1, 5, 70, "rbf"), (96, 3, 2, 40, 40, "matern52"),
                                               (96, 3, 2, 40, 40, "rbf_matern52")])
def test_predict_assemble_vs_oracle_formula(ops, dtype, N, n, m, b, bp, kernel):
    """bcbf_predict_assemble (the one-launch tail of _custom_predict_matrix / custom_predict_fullmat, control_affine_model.py:
    1051-1091, 963-980): from the Gram G = W'W', BkXX = k(X*, X*') B - G (+ the make_psd jitter on its diagonal when b == b') and kron(Bk2, A),
    against the oracle's statements of the same lines evaluated in fp64 on the device's own W (ragged tiles, b != b', every
    (n, m) extreme, both data kernels)."""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(1, N, n, m, dtype=dtype, device=DEV, seed=70 + N)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], kernel=kernel)
    assert int(info[0]) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    g = torch.Generator(device="cpu").manual_seed(3)
    mk = lambda k: (p["X"][0, torch.randint(0, N, (k,), generator=g).to(DEV)] + 0.3 * torch.randn(k, n, generator=g).to(DEV, dtype)).contiguous()
    Xq, Xqp = mk(b), mk(bp)
    if b == bp:
        Xqp = Xq
    q = lambda x: ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], x, shared=True, want_W=True, kernel=kernel)[2]
    W, Wp = q(Xq), q(Xqp)
    jit = (1e-5 * torch.rand(b * (m + 1), generator=g)).to(DEV, dtype) if b == bp else None
    A = p["A"][0].contiguous()
    G = torch.einsum("bnc,pnd->bpcd", W[:, :N], Wp[:, :N]).contiguous()
    BkXX, Kron = ops.predict_assemble(G, Xq, Xqp, p["ell"][0].contiguous(), p["s2"], p["Bm"][0].contiguous(), A, jit,
                                      want_BkXX=True, want_kron=True, kernel=kernel)
    h = lambda t: host(t).astype(np.float64)
    knl = ogp.DATA_KERNELS[kernel]
    KB = knl(h(Xq), h(Xqp), h(p["ell"][0]), float(p["s2"][0]))[:, :, None, None] * h(p["Bm"][0])[None, None]
    ref = KB - np.einsum("bic,pid->bpcd", h(W)[:, :N], h(Wp)[:, :N])                    # (:1079-1088 on the device's W)
    if jit is not None:
        C = m + 1
        for i in range(b):
            ref[i, i] += np.diag(h(jit).reshape(b, C)[i])                                # (:1089, first draw)
    scale = float(p["s2"][0]) * float(p["Bm"][0].abs().max())
    rel_close(h(BkXX), ref, 1e-12 if f64 else 2e-5, scale=scale, what="BkXX")
    Bk2 = ref.transpose(0, 2, 1, 3).reshape(b * (m + 1), bp * (m + 1))                    # (:975)
    rel_close(h(Kron), np.kron(Bk2, h(A)), 1e-12 if f64 else 2e-5, scale=scale * float(A.abs().max()), what="kron(Bk2, A)")
    only, _ = ops.predict_assemble(G, Xq, Xqp, p["ell"][0].contiguous(), p["s2"], p["Bm"][0].contiguous(), None, jit, kernel=kernel)
    assert torch.equal(only, BkXX)


@pytest.mark.parametrize("N,n,dtype,mult,m", [(512, 3, torch.float32, 16, 2), (480, 4, torch.float64, 16, 2), (100, 2, torch.float64, 16, 2),
                                              (512, 3, torch.float64, 16, 2), (288, 4, torch.float32, 16, 2), (512, 3, torch.float32, 32, 2),
                                              (200, 2, torch.float32, 32, 2), (320, 3, torch.float64, 32, 2),
                                              (128, 2, torch.float32, 16, 1), (512, 2, torch.float64, 16, 1), (320, 3, torch.float32, 32, 1),
                                              (96, 1, torch.float64, 32, 1)])
def test_shared_gp_five_queries_per_wave_form(ops, N, n, dtype, mult, m):
    """m = 2 / m = 1 (three / two columns per query), more queries than one wave per SIMD holds at four per wave: the launcher packs
    FIVE / EIGHT queries into the 16 matrix-core columns of a wave (posterior_shared_reg.hip, QW = 5 / 8) when that saves a round of waves:
    mult = 16: one wave per SIMD; 32: fp32 two waves per SIMD, fp64 two rounds.  Against the fp64 oracle on a sample of the queries, and against the same batch cut into pieces that take the
    four-per-wave form (same arithmetic per query: only the lane a value sits in differs)."""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(1, N, n, m, dtype=dtype, device=DEV, seed=41 + N)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert int(info[0]) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = mult * cus + 503                                       # ragged: not a multiple of 5, 20 or 4
    g = torch.Generator(device="cpu").manual_seed(7)
    xq = (p["X"][0, torch.randint(0, N, (b,), generator=g).to(DEV)] + 0.3 * torch.randn(b, n, generator=g).to(DEV, dtype)).contiguous()
    j2 = (1e-5 * torch.rand(b, m + 1, generator=g)).to(DEV, dtype)
    Mk, Bk, W = ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, j2, want_W=True)
    scale = float(p["s2"][0]) * float(p["Bm"][0].abs().max())
    for a in range(0, b, 1024):
        Mk1, Bk1, W1 = ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq[a:a + 1024].contiguous(),
                                            j2[a:a + 1024].contiguous(), want_W=True)
        tol = 1e-10 if f64 else 2e-4          # (the two forms are separate instantiations: a multiply-add contracted in one and not
                                              #  in the other moves a kernel value by an ulp, and the triangular solve amplifies it by
                                              #  the factor's condition number -- fp32, n = 2: 1e-5 at N = 128; both forms then sit
                                              #  equally far from the fp64 answer)
        rel_close(host(Mk[a:a + 1024]), host(Mk1), tol, scale=max(1.0, float(Mk1.abs().max())), what="Mk")
        rel_close(host(Bk[a:a + 1024]), host(Bk1), tol, scale=scale, what="Bk")
        rel_close(host(W[a:a + 1024]), host(W1), tol, scale=max(1e-3, float(W1.abs().max())), what="W")
    pick = torch.randint(0, b, (48,), generator=g)
    pick[:3] = torch.tensor([0, b - 1, b - 2])
    h = {k: host(v) for k, v in p.items()}
    st = ogp.refit_state(h["X"][0], h["U"][0], h["Xdot"][0], h["Bm"][0], h["ell"][0], h["s2"][0], h["M0"][0],
                         h["jitter"][0][None] / 1e-5)
    rep = lambda a_: np.broadcast_to(a_[None], (len(pick),) + a_.shape)
    Mk_o, Bk_o = ogp.posterior_step(rep(st["L"]), rep(st["alpha"]), rep(h["X"][0]), rep(st["UHB"]), rep(h["ell"][0]),
                                    rep(h["s2"][0]), rep(h["Bm"][0]), rep(h["M0"][0]), host(xq)[pick.numpy()],
                                    jitter2=host(j2)[pick.numpy()])
    rel_close(host(Mk)[pick.numpy()], Mk_o, 1e-9 if f64 else 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk vs oracle")
    rel_close(host(Bk)[pick.numpy()], Bk_o, 1e-9 if f64 else 1e-3, scale=h["s2"][0] * np.abs(h["Bm"][0]).max(), what="Bk vs oracle")


def test_shared_gp_two_waves_per_simd_form_equals_one_wave_form(ops):
    """fp32, more queries than one wave per SIMD holds (> 16 per compute unit): the launcher takes the 256-register
    instantiation of the register-resident kernel (two workgroups per CU, plain operand loads).  Same arithmetic in the
    same order as the one-wave form: the same answers as the batch cut into pieces that take the one-wave form."""
    from bayesian_cbf_amd.synthetic import make_instances
    dtype, N, n, m = torch.float32, 512, 3, 2
    p = make_instances(1, N, n, m, dtype=dtype, device=DEV, seed=77)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = 16 * cus + 1237                                       # ragged, beyond the switch-over
    g = torch.Generator(device="cpu").manual_seed(5)
    xq = (p["X"][0, torch.randint(0, N, (b,), generator=g).to(DEV)] + 0.3 * torch.randn(b, n, generator=g).to(DEV, dtype)).contiguous()
    Mk, Bk, W = ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, want_W=True)
    for a in range(0, b, 2048):
        Mk1, Bk1, W1 = ops.posterior_shared(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq[a:a + 2048].contiguous(), want_W=True)
        scale = float(p["s2"][0]) * float(p["Bm"][0].abs().max())
        rel_close(host(Mk[a:a + 2048]), host(Mk1), 1e-6, scale=max(1.0, float(Mk1.abs().max())), what="Mk")
        rel_close(host(Bk[a:a + 2048]), host(Bk1), 1e-6, scale=scale, what="Bk")
        rel_close(host(W[a:a + 2048]), host(W1), 1e-6, scale=max(1e-3, float(W1.abs().max())), what="W")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_control_step_shared_model_equals_replicated_model(ops, dtype):
    """bcbf_unicycle_control_step with shared_gp=1 (one learned model, Bt closed loops: BASELINE config 4) gives the
    controls of the per-instance path run on Bt copies of the model, and both equal the composed entry points."""
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    Bt, N = 100, 128
    p = make_instances(1, N, 3, 2, dtype=dtype, device=DEV, seed=41)
    t = make_unicycle_task(Bt, dtype=dtype, device=DEV, seed=42)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    A = (0.01 * p["A"]).contiguous()
    shared = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=A)
    rep = {k: v.expand(Bt, *v.shape[1:]).contiguous() for k, v in shared.items()}
    x1, x2 = t["x"].clone(), t["x"].clone()
    ws1, ws2 = ops.control_workspace(Bt, 2, dtype, DEV), ops.control_workspace(Bt, 2, dtype, DEV)
    ops.unicycle_control_step(shared, t, ws1, x1, dt=0.05, L_true=12.0, L_mean=4.0, max_iters=40)
    ops.unicycle_control_step(rep, t, ws2, x2, dt=0.05, L_true=12.0, L_mean=4.0, max_iters=40)
    tol = 1e-9 if dtype == torch.float64 else 1e-3
    prior = float(p["s2"][0]) * float(p["Bm"][0].abs().max())
    rel_close(host(ws1["Mk"]), host(ws2["Mk"]), tol, scale=max(1.0, float(ws2["Mk"].abs().max())), what="Mk")
    rel_close(host(ws1["Bk"]), host(ws2["Bk"]), tol, scale=prior, what="Bk")
    ok = ((ws1["status"] == 0) & (ws2["status"] == 0)).cpu().numpy()
    assert ok.sum() >= Bt // 2
    ytol = 1e-6 if dtype == torch.float64 else 1e-3      # (fp32 measured: 2.1e-6)
    all_close(host(ws1["y"])[ok], host(ws2["y"])[ok], ytol, ytol, what="shared-vs-instance y")
    all_close(host(x1)[ok], host(x2)[ok], ytol, ytol, what="shared-vs-instance x")
    # composed path on the same inputs
    Mk, Bk, _ = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], t["x"], shared=True)
    grad, cst, fhat, ghat = ops.unicycle_constraints(t["x"], t["plan"], t["dot_plan"], t["Kp"], 10.0, t["centers"],
                                                     t["radii"], t["tw"], t["gammas"], 4.0)
    y, st, it, _, _, _ = ops.cbc_socp(Mk, Bk, rep["A"], grad, cst, t["sign"], fhat, ghat, t["w"], t["r"],
                                      t["relax_mask"], t["rho"], max_iters=40)
    # (the composed path evaluates the task rows in another kernel: same source, but the compiler may contract
    #  multiply-adds differently, so agreement is to rounding, not bitwise)
    assert int((st != ws1["status"]).sum()) <= 1
    ctol = 1e-9 if dtype == torch.float64 else 1e-3      # (fp32 measured: 3.2e-7)
    all_close(host(y)[ok], host(ws1["y"])[ok], ctol, ctol, what="composed y")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_online_gp_append_equals_refit(ops, dtype):
    """bcbf_gp_append (BASELINE configs[4]: growing N without refactorisation) over 40 observations, crossing a
    32-row padding boundary in place and re-packed, against bcbf_refit + bcbf_potrs on all the points -- which is
    what the reference does (it refits from scratch)."""
    from bayesian_cbf_amd.synthetic import make_instances
    Bt, N0, N1, n, m = 5, 50, 90, 3, 2
    p = make_instances(Bt, N1, n, m, dtype=dtype, device=DEV, seed=77)
    cut = lambda t, N: t[:, :N].contiguous()
    Lop, UHB, info, _ = ops.refit(cut(p["X"], N0), cut(p["UH"], N0), p["Bm"], p["ell"], p["s2"], cut(p["jitter"], N0))
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, cut(p["Xdot"], N0), cut(p["UH"], N0), p["M0"], want_alpha=False)
    X = cut(p["X"], N0)
    for N in range(N0, N1):
        Lop, Vw, X, UHB, info = ops.gp_append(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"],
                                              p["X"][:, N].contiguous(), p["UH"][:, N].contiguous(),
                                              p["Xdot"][:, N].contiguous(), p["jitter"][:, N].contiguous())
        assert (info == 0).all()
    Lop_r, UHB_r, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    Vw_r, _ = ops.potrs(Lop_r, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    assert torch.equal(X, p["X"])
    rel_close(host(UHB), host(UHB_r), 1e-12 if dtype == torch.float64 else 1e-6, what="UHB")
    # the reference exposes only posterior outputs: compare those (and, in fp64, the internals too)
    xq = p["xq"]
    Mk, Bk = ops.posterior_step(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq)
    Mk_r, Bk_r = ops.posterior_step(Lop_r, Vw_r, p["X"], UHB_r, p["ell"], p["s2"], p["Bm"], p["M0"], xq)
    tol = 1e-8 if dtype == torch.float64 else 1e-3
    prior = float((p["s2"][:, None, None] * p["Bm"]).abs().max())
    rel_close(host(Mk), host(Mk_r), tol, scale=max(1.0, float(Mk_r.abs().max())), what="Mk")
    rel_close(host(Bk), host(Bk_r), tol, scale=prior, what="Bk")
    if dtype == torch.float64:
        rel_close(host(Lop), host(Lop_r), 1e-8, what="Lop")
        rel_close(host(Vw), host(Vw_r), 1e-8, what="Vw")


@pytest.mark.parametrize("gemm", [False, True], ids=["potri", "trtri+gemm"])
@pytest.mark.parametrize("dtype,N", [(torch.float64, 100), (torch.float64, 256), (torch.float32, 64)])
def test_potri_dense_inverse(ops, dtype, N, gemm):
    """K_b^-1 from the packed factor (ragged N: the last column chunk is partial): bcbf_potri, and bcbf_trtri (dense
    L^-1, checked lower triangular with L L^-1 = I through the dense factor) followed by one GEMM."""
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(3, N, 3, 2, dtype=dtype, device=DEV, seed=21)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert (info == 0).all()
    Kinv = ops.kb_inverse(Lop, N, gemm=gemm)
    Kb = ops.kb_build(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    eye = torch.eye(N, dtype=torch.float64, device=DEV)
    res = (Kb.double() @ Kinv.double() - eye).abs().max()
    # K_b is ill conditioned (cond ~ 1e5..1e8 with the 1e-5 jitter): residual relative to |K_b| |K_b^-1|
    scale = float(Kb.double().abs().max() * Kinv.double().abs().max())
    # (K_b K_b^-1 - I relative to |K_b| |K_b^-1|: the likelihood gradient's intermediate, fit runs it in fp64 -- FIT_DTYPE)
    assert float(res) <= (1e-10 if dtype == torch.float64 else 2e-3) * max(scale, 1.0), (float(res), scale)
    assert float((Kinv - Kinv.transpose(1, 2)).abs().max()) <= (1e-9 if dtype == torch.float64 else 1e-1) * float(Kinv.abs().max())


def test_edge_cases_empty_batch_single_point_and_maximum_size(ops):
    """Empty batch (every entry point returns without launching), N = 1, and the maximum supported N = 2048 (fp64 and
    fp32) against the oracle."""
    from bayesian_cbf_amd.synthetic import make_instances
    # ---- empty batch
    p = make_instances(1, 8, 3, 2, dtype=torch.float64, device=DEV, seed=1)
    e = {k: v[:0].contiguous() for k, v in p.items()}
    Lop, UHB, info, _ = ops.refit(e["X"], e["UH"], e["Bm"], e["ell"], e["s2"], e["jitter"])
    assert Lop.shape[0] == 0 and info.numel() == 0
    Vw, _ = ops.potrs(Lop, e["Xdot"], e["UH"], e["M0"])
    Mk, Bk = ops.posterior_step(Lop, Vw, e["X"], UHB, e["ell"], e["s2"], e["Bm"], e["M0"], e["xq"])
    assert Mk.shape == (0, 3, 3) and Bk.shape == (0, 3, 3)
    # ---- N = 1
    q = make_instances(3, 1, 3, 2, dtype=torch.float64, device=DEV, seed=2)
    Lop, UHB, info, _ = ops.refit(q["X"], q["UH"], q["Bm"], q["ell"], q["s2"], q["jitter"])
    Vw, _ = ops.potrs(Lop, q["Xdot"], q["UH"], q["M0"], want_alpha=False)
    Mk, Bk = ops.posterior_step(Lop, Vw, q["X"], UHB, q["ell"], q["s2"], q["Bm"], q["M0"], q["xq"])
    h = {k: host(v) for k, v in q.items()}
    for i in range(3):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jitter"][i][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None], h["ell"][i][None],
                                        h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None], h["xq"][i][None])
        rel_close(host(Mk)[i], Mk_o[0], 1e-10, scale=max(1.0, np.abs(Mk_o).max()), what="Mk N=1")
        rel_close(host(Bk)[i], Bk_o[0], 1e-10, scale=h["s2"][i] * np.abs(h["Bm"][i]).max(), what="Bk N=1")
    # ---- N = 2048: well-conditioned inputs (wide box) so that fp32 factors too
    for dtype, tol in ((torch.float64, 1e-8), (torch.float32, 1e-3)):      # (fp32 measured: 6e-8)
        r = make_instances(2, 2048, 3, 2, dtype=torch.float64, device=DEV, seed=3)
        r["X"] = (r["X"] * 6.0).contiguous()                 # spread the points: K_b stays positive definite in fp32
        r["xq"] = (r["xq"] * 6.0).contiguous()
        rr = {k: v.to(dtype).contiguous() for k, v in r.items()}
        Lop, UHB, info, _ = ops.refit(rr["X"], rr["UH"], rr["Bm"], rr["ell"], rr["s2"], rr["jitter"])
        assert (info == 0).all()
        Vw, _ = ops.potrs(Lop, rr["Xdot"], rr["UH"], rr["M0"], want_alpha=False)
        Mk, Bk = ops.posterior_step(Lop, Vw, rr["X"], UHB, rr["ell"], rr["s2"], rr["Bm"], rr["M0"], rr["xq"])
        h = {k: host(v) for k, v in r.items()}
        st = ogp.refit_state(h["X"][0], h["U"][0], h["Xdot"][0], h["Bm"][0], h["ell"][0], h["s2"][0], h["M0"][0],
                             h["jitter"][0][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][0][None], st["UHB"][None], h["ell"][0][None],
                                        h["s2"][0][None], h["Bm"][0][None], h["M0"][0][None], h["xq"][0][None])
        rel_close(host(Mk)[0], Mk_o[0], tol, scale=max(1.0, np.abs(Mk_o).max()), what="Mk N=2048")
        rel_close(host(Bk)[0], Bk_o[0], tol, scale=h["s2"][0] * np.abs(h["Bm"][0]).max(), what="Bk N=2048")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_controller_cones_rows_match_oracle(ops, m, dtype):
    """bcbf_controller_cones: every constraint kind of SOCPController / QPController (controllers.py:396-540, 614-629),
    positive-definite and indefinite Asq, a batch of instances, against the numpy restatement."""
    from oracle import controllers as oc
    rng = np.random.default_rng(100 + m)
    Bt, K, ev = 37, 4, 2
    kinds, factors = [1, 2, 0, 1], [1.7, 1.0, 1.0, 0.4]
    T = m + 1 + m * m + m + 1
    terms = np.zeros((Bt, K, T))
    raw = []
    for b in range(Bt):
        row = []
        for k in range(K):
            R = rng.normal(size=(m + 1, m + 1))
            Asq = R @ R.T + 0.05 * np.eye(m + 1)
            if kinds[k] == 1 and b % 3 == 0:          # indefinite: exercises the eigen fallback
                w, Q = np.linalg.eigh(Asq)
                w[0] = -0.3 * abs(w[0]) - 0.01
                Asq = (Q * w) @ Q.T
            bfe, e = rng.normal(size=m), rng.normal()
            V, bfv, v = Asq[1:, 1:], 2 * Asq[1:, 0], Asq[0, 0]
            terms[b, k] = np.concatenate([bfe, [e], V.ravel(), bfv, [v]])
            row.append((bfe, e, V, bfv, v))
        raw.append(row)
    u_ref = rng.normal(size=(Bt, m))
    G, h, qdims, l, cst = ops.controller_cones(dev(terms, dtype), dev(u_ref, dtype), kinds, factors, ctrl_reg=0.7,
                                               relax_weight=30.0, extravars=ev, objective=True)
    assert G.dtype == torch.float64 and l == 1 and qdims == [m + 2] * 4 and int(cst.abs().max()) == 0
    G, h = host(G), host(h)
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    if dtype == torch.float32:                            # the oracle sees the rounded inputs the kernel saw
        terms = host(dev(terms, dtype)); u_ref = host(dev(u_ref, dtype))
    nv = ev + m
    for b in range(Bt):
        tb = [(t_[:m], t_[m], t_[m + 1:m + 1 + m * m].reshape(m, m), t_[m + 1 + m * m:m + 1 + m * m + m], t_[-1]) for t_ in terms[b]]
        # linear row first
        _, _, c, d = oc.convert_cbc_terms_to_socp_terms(*tb[1], ev)
        np.testing.assert_allclose(G[b, 0], -c, rtol=tol, atol=tol)
        np.testing.assert_allclose(h[b, 0], d, rtol=tol, atol=tol)
        Ro, ho, ao, bo = oc.socp_objective(u_ref[b], 0.7, 30.0, extravars=ev)
        np.testing.assert_allclose(G[b, 1:m + 3], np.vstack([-ao, -Ro]), rtol=tol, atol=tol)
        np.testing.assert_allclose(h[b, 1:m + 3], np.concatenate([[bo], ho]), rtol=tol, atol=tol)
        r0 = m + 3
        for k in (0, 2, 3):
            if kinds[k] == 0:
                A, bb, c, d = oc.convert_cbc_terms_to_socp_terms(*tb[k], ev)
            else:
                A, bb, c, d = oc.socp_safety(*tb[k], factors[k], ev)
            Gk, hk = G[b, r0:r0 + m + 2], h[b, r0:r0 + m + 2]
            np.testing.assert_allclose(Gk[0], -c, rtol=tol, atol=tol)
            np.testing.assert_allclose(hk[0], d, rtol=tol, atol=tol)
            Mg, Mr = np.column_stack([hk[1:], -Gk[1:, ev:]]), np.column_stack([bb, A[:, ev:]])
            assert np.all(Gk[1:, :ev] == 0)
            fallback = kinds[k] == 1 and b % 3 == 0
            if fallback:                                   # rows = sqrt(lambda) v', up to the sign of v
                np.testing.assert_allclose(Mg.T @ Mg, Mr.T @ Mr, rtol=50 * tol, atol=50 * tol)
                np.testing.assert_allclose(np.abs(Mg), np.abs(Mr), rtol=200 * tol, atol=200 * tol)
            else:
                np.testing.assert_allclose(Mg, Mr, rtol=10 * tol, atol=10 * tol)
            r0 += m + 2
        assert r0 == G.shape[1]


def test_controller_cones_flags_unfactorable_stability_terms(ops):
    """kind 0 retries once with + 1e-3 I (controllers.py:464-469); a clearly indefinite Asq is reported per instance."""
    m = 1
    good = np.array([0.3, 0.1, 1.0, 0.2, 2.0])          # bfe, e, V, bfv, v
    tiny = np.array([0.3, 0.1, 1.0, 2.0, 1.0 - 5e-4])   # v V - bfv^2/4 slightly negative: fixed by the 1e-3 shift
    bad = np.array([0.3, 0.1, 1.0, 0.2, -2.0])
    terms = dev(np.stack([good, tiny, bad])[:, None, :], torch.float64)
    G, h, qd, l, cst = ops.controller_cones(terms, None, [0], extravars=1, objective=False)
    c = host(cst).ravel()
    assert c[0] == 0 and c[1] == 0 and c[2] != 0
    from oracle import controllers as oc
    A, b, c, d = oc.convert_cbc_terms_to_socp_terms(tiny[:1], tiny[1], tiny[2:3].reshape(1, 1), tiny[3:4], tiny[4], 1)
    np.testing.assert_allclose(-host(G)[1, 1:], A, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(host(h)[1, 1:], b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 2e-4)], ids=["f64", "f32"])
def test_rbf_plus_linear_data_kernel_entry_points(ops, dtype, tol):
    """bcbf_kb_build_rbflin / bcbf_posterior_query_rbflin with independent instances (one `lin` per instance):
    k = s2 (exp(-1/2 |x-x'|^2/ell^2) + lin x'x'), against numpy."""
    rng = np.random.default_rng(7)
    Bt, N, n, C = 5, 70, 2, 4
    X = rng.uniform(-1.5, 1.5, (Bt, N, n)); UH = rng.normal(size=(Bt, N, C)); UH[..., 0] = 1
    R = rng.normal(size=(Bt, C, C)); Bm = R @ R.transpose(0, 2, 1) + 0.2 * np.eye(C)
    ell = np.repeat(rng.uniform(0.5, 1.2, (Bt, 1)), n, axis=1); s2 = rng.uniform(0.5, 1.5, Bt); lin = rng.uniform(0.05, 0.4, Bt)
    jit = 1e-4 * rng.uniform(size=(Bt, N)) + (1e-3 if dtype == torch.float32 else 0.0)
    Y = rng.normal(size=(Bt, N, n)); M0 = 0.1 * rng.normal(size=(Bt, C, n)); xq = rng.uniform(-1, 1, (Bt, n))
    d = lambda a: dev(a, dtype)
    Kb = ops.kb_build(d(X), d(UH), d(Bm), d(ell), d(s2), d(jit), lin=d(lin))
    Lop, info, _ = ops.potrf(Kb)
    assert int(info.abs().max()) == 0
    Vw, _ = ops.potrs(Lop, d(Y), d(UH), d(M0), want_alpha=False)
    UHB = np.einsum("bnc,bcd->bnd", UH, Bm)
    Mk, Bk, W = ops.posterior_query(Lop, Vw, d(X), d(UHB), d(ell), d(s2), d(Bm), d(M0), d(xq), shared=False, want_W=True,
                                    lin=d(lin))
    for b in range(Bt):
        Kref = ogp.rbf_linear_kernel(X[b], X[b], ell[b], s2[b], lin[b]) * (UH[b] @ Bm[b] @ UH[b].T) + np.diag(jit[b])
        rel_close(host(Kb[b]), Kref, tol, what="K_b")
        L = np.linalg.cholesky(Kref)
        Phi = ogp.rbf_linear_kernel(X[b], xq[b:b + 1], ell[b], s2[b], lin[b]) * UHB[b]
        Wr = np.linalg.solve(L, Phi)
        Vr = np.linalg.solve(L, Y[b] - UH[b] @ M0[b])
        rel_close(host(W[b, :N]), Wr, 5 * tol, what="W")                     # (fp32: 1e-3; measured 5.6e-5)
        # (the posterior mean is a weighted sum of the TARGETS, here white noise of scale |Y| ~ 3.5: error relative to that
        #  scale, as B_k's is relative to the prior scale; fp32 measured 1.5e-3 of |Mk| = 4e-4 of |Y|)
        rel_close(host(Mk[b]), M0[b].T + Vr.T @ Wr, 5 * tol, scale=max(1.0, np.abs(Y[b]).max()), what="Mk")
        kss = s2[b] * (1 + lin[b] * xq[b] @ xq[b])
        rel_close(host(Bk[b]), kss * Bm[b] - Wr.T @ Wr, 5 * tol, scale=kss * np.abs(Bm[b]).max(), what="Bk")   # (measured 1.8e-6)


@pytest.mark.parametrize("m", [1, 2])
def test_fp64_shared_queries_two_per_workgroup(ops, m):
    """fp64, one model, many queries: the streaming kernel answers two queries per workgroup (odd query count, W output,
    second jitter).  Checked against the one-query-per-call path of the same kernel and against the oracle."""
    from bayesian_cbf_amd.synthetic import make_instances
    N, n, b = 150, 3, 37
    p = make_instances(1, N, n, m, dtype=torch.float64, device=DEV, seed=5)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert int(info[0]) == 0
    Vw, alpha = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"])
    g = torch.Generator(device=DEV).manual_seed(3)
    xq = (2 * torch.rand(b, n, dtype=torch.float64, device=DEV, generator=g) - 1).contiguous()
    jit2 = (1e-5 * torch.rand(b, 1 + m, dtype=torch.float64, device=DEV, generator=g)).contiguous()
    Mk, Bk, W = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, jit2, shared=True, want_W=True)
    for i in (0, 1, 17, 36):                                   # one query per call: the NQ = 1 instantiation
        Mk1, Bk1, W1 = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq[i:i + 1].contiguous(),
                                           jit2[i:i + 1].contiguous(), shared=True, want_W=True)
        rel_close(host(Mk[i]), host(Mk1[0]), 1e-12, scale=1.0, what="Mk vs single")
        rel_close(host(Bk[i]), host(Bk1[0]), 1e-12, scale=1.0, what="Bk vs single")
        rel_close(host(W[i]), host(W1[0]), 1e-12, scale=1.0, what="W vs single")
    h = {k: host(v) for k, v in p.items()}
    st = ogp.refit_state(h["X"][0], h["U"][0], h["Xdot"][0], h["Bm"][0], h["ell"][0], h["s2"][0], h["M0"][0],
                         h["jitter"][0][None] / 1e-5)
    for i in (0, 36):
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][0][None], st["UHB"][None], h["ell"][0][None],
                                        h["s2"][0][None], h["Bm"][0][None], h["M0"][0][None], host(xq)[i][None],
                                        jitter2=host(jit2)[i][None])
        rel_close(host(Mk[i]), Mk_o[0], 1e-8, scale=max(1.0, np.abs(Mk_o).max()), what="Mk vs oracle")
        rel_close(host(Bk[i]), Bk_o[0], 1e-8, scale=h["s2"][0] * np.abs(h["Bm"][0]).max(), what="Bk vs oracle")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N,n,m", [(1, 2, 1), (31, 3, 2), (33, 3, 2), (100, 2, 1), (256, 2, 1), (512, 3, 2), (700, 3, 3)])
def test_refit_one_wave_per_instance_vs_oracle_and_workgroup_form(ops, N, n, m, dtype):
    """The batch form of the refit (refit_wave64.hip: one wave per instance, 4-column-blocked diagonal tiles; fp64 and fp32;
    a batch of 70 runs one wave per SIMD, the two-waves-per-SIMD fp32 allocation is covered by the C3 test) against
    the oracle's factor and against the workgroup-per-instance form (refit_mfma64.hip / refit_mfma.hip) on the same inputs: dense L,
    packed operator (incl. the inverted diagonal blocks), UH*B, per-instance failure index.  `form=` forces the
    form (the library picks by batch size)."""
    from bayesian_cbf_amd.synthetic import make_instances
    Bt = 70                                    # odd number of workgroups' worth of waves + a ragged tail
    f64 = dtype == torch.float64
    # (fp32 tP: two fp32 factorizations of a K_b with cond ~1e5 compared entry by entry -- an internal representation, forward
    #  bound cond * eps = 6e-3, measured 7.8e-4; every reference-exposed output derived from it is held to 1e-3)
    tL, tW, tP = (1e-8, 1e-9, 1e-8) if f64 else (1e-3, 1e-3, 2e-3)
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=100 + N)
    p["X"] = (p["X"] * 2.0).contiguous()
    jit = p["jitter"].clone()
    X, UH = p["X"].clone(), p["UH"].clone()
    if N >= 31:                                # instance 5: a duplicated point with a negative shift -> pivot 21 fails
        X[5, 20], UH[5, 20] = X[5, 3], UH[5, 3]
        jit[5] = 0.0
        jit[5, 20] = -1e-3 if f64 else -1e-2
    args = (X, UH, p["Bm"], p["ell"], p["s2"], jit)
    Lop_w, UHB_w, info_w, Ld_w = ops.refit(*args, want_dense=True, form=ops.REFIT_WAVE)
    Kb = ops.kb_build(*args)
    Lop_p, info_p, Ld_p = ops.potrf(Kb, want_dense=True, form=ops.REFIT_WAVE)   # the from-dense instantiation of the same kernel
    Lop_g, UHB_g, info_g, Ld_g = ops.refit(*args, want_dense=True, form=ops.REFIT_WORKGROUP)
    torch.cuda.synchronize()
    iw = info_w.cpu().numpy()
    assert np.array_equal(iw, info_g.cpu().numpy()) and np.array_equal(iw, info_p.cpu().numpy())
    good = iw == 0
    assert good.sum() == (Bt - 1 if N >= 31 else Bt) and (N < 31 or iw[5] == 21)
    rel_close(host(UHB_w), host(UHB_g), 1e-14 if f64 else 1e-6, what="UHB")
    h = {k: host(v) for k, v in dict(X=X, U=p["U"], Xdot=p["Xdot"], Bm=p["Bm"], ell=p["ell"], s2=p["s2"], M0=p["M0"], jit=jit).items()}
    for i in (0, 1, 37, Bt - 1):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jit"][i][None] / 1e-5)
        rel_close(host(Ld_w[i]), st["L"], tL, what="L vs oracle [%d]" % i)
        rel_close(host(Ld_p[i]), st["L"], tL, what="L(potrf) vs oracle [%d]" % i)
    g = torch.as_tensor(good, device=DEV)
    rel_close(host(Ld_w[g]), host(Ld_g[g]), tW, what="L vs workgroup form")
    # packed operator: off-diagonal panels and inverted diagonal blocks (inverses of ill-conditioned blocks: relative to
    # the largest entry of the operator, per instance)
    for i in np.nonzero(good)[0][:8]:
        rel_close(host(Lop_w[i]), host(Lop_g[i]), tP, what="Lop vs workgroup form [%d]" % i)
        rel_close(host(Lop_p[i]), host(Lop_g[i]), tP, what="Lop(potrf) vs workgroup form [%d]" % i)
    # and the posterior through the new operator
    Vw, _ = ops.potrs(Lop_w, p["Xdot"], UH, p["M0"], want_alpha=False)
    Mk, Bk = ops.posterior_step(Lop_w, Vw, X, UHB_w, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
    for i in (0, Bt - 1):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jit"][i][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None], h["ell"][i][None],
                                        h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None], host(p["xq"])[i][None])
        rel_close(host(Mk)[i], Mk_o[0], 1e-8 if f64 else 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk")
        rel_close(host(Bk)[i], Bk_o[0], 1e-8 if f64 else 1e-3, scale=float(h["s2"][i] * np.abs(h["Bm"][i]).max()), what="Bk")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,Bt,N,n,m", [("pair", 1, 1, 2, 1), ("pair", 70, 31, 3, 2), ("pair", 70, 33, 3, 2), ("pair", 3, 100, 6, 3),
                                          ("pair", 70, 256, 2, 1), ("pair", 9, 500, 3, 2),
                                          ("team", 1, 1, 2, 1), ("team", 7, 33, 3, 2), ("team", 3, 100, 6, 3), ("team", 9, 500, 3, 2),
                                          ("team", 2, 1000, 3, 3), ("team", 1, 2048, 3, 2),
                                          ("team4", 7, 33, 3, 2), ("team4", 5, 300, 6, 3), ("team4", 2, 500, 3, 2)])
def test_refit_two_waves_per_instance_vs_one_wave_form_and_oracle(ops, form, Bt, N, n, m, dtype):
    """The chain + bulk forms of the refit (refit_wave64.hip: a chain wave that factors and inverts the diagonal tiles on the
    matrix cores; `pair`: one bulk wave a block column behind, N <= 512; `team` / `team4`: seven / three bulk waves sharing a
    column's tiles, hand-offs per block row, N <= 2048) forced by `form=` against the
    one-wave form on the same inputs -- packed operator incl. both copies of the inverted diagonal blocks, UH*B,
    per-instance failure index (a failed pivot in one instance) -- and, through potrs + the posterior kernel, against the
    oracle.  Shapes: one row, a ragged last block, a state wider than the registers hold (n = 6), the largest systems of
    the forms, one instance and odd batches."""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=300 + N)
    p["X"] = (p["X"] * 2.0).contiguous()
    jit = p["jitter"].clone()
    X, UH = p["X"].clone(), p["UH"].clone()
    bad = Bt > 5 and N >= 31
    if bad:                                    # instance 5: a duplicated point with a negative shift -> pivot 21 fails
        X[5, 20], UH[5, 20] = X[5, 3], UH[5, 3]
        jit[5] = 0.0
        jit[5, 20] = -1e-3 if f64 else -1e-2
    args = (X, UH, p["Bm"], p["ell"], p["s2"], jit)
    forced = {"pair": ops.REFIT_PAIR, "team4": ops.REFIT_TEAM4, "team": ops.REFIT_TEAM8}[form]   # (two / four / eight waves per instance)
    Lop_p, UHB_p, info_p, _ = ops.refit(*args, form=forced)
    Lop_w, UHB_w, info_w, _ = ops.refit(*args, form=ops.REFIT_WAVE)
    torch.cuda.synchronize()
    ip = info_p.cpu().numpy()
    assert np.array_equal(ip, info_w.cpu().numpy())
    good = ip == 0
    assert good.sum() == (Bt - 1 if bad else Bt) and (not bad or ip[5] == 21)
    assert torch.equal(UHB_p, UHB_w)
    # (fp32: two factorizations of K_b with cond ~1e5 and the inverses of its diagonal blocks; the forms round K_b's entries
    #  differently since the one-wave form's interior tiles skip the jitter / padding selects: cond x eps = 6e-3)
    for i in np.nonzero(good)[0][:8]:
        rel_close(host(Lop_p[i]), host(Lop_w[i]), 1e-8 if f64 else 1e-3, what="Lop vs one-wave form [%d]" % i)   # (fp32 measured: 2.6e-6)
    Vw, _ = ops.potrs(Lop_p, p["Xdot"], UH, p["M0"], want_alpha=False)
    Mk, Bk = ops.posterior_step(Lop_p, Vw, X, UHB_p, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
    h = {k: host(v) for k, v in dict(X=X, U=p["U"], Xdot=p["Xdot"], Bm=p["Bm"], ell=p["ell"], s2=p["s2"], M0=p["M0"], jit=jit).items()}
    for i in (0, Bt - 1):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                             h["jit"][i][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None], h["ell"][i][None],
                                        h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None], host(p["xq"])[i][None])
        rel_close(host(Mk)[i], Mk_o[0], 1e-8 if f64 else 1e-3, scale=max(1.0, np.abs(Mk_o).max()), what="Mk")
        rel_close(host(Bk)[i], Bk_o[0], 1e-8 if f64 else 1e-3, scale=float(h["s2"][i] * np.abs(h["Bm"][i]).max()), what="Bk")


@pytest.mark.parametrize("dtype,N,n,m", [(torch.float64, 1024, 3, 2), (torch.float64, 1100, 2, 1), (torch.float32, 512, 3, 2),
                                         (torch.float32, 1000, 4, 3), (torch.float32, 576, 3, 1)], ids=["f64-1024", "f64-1100", "f32-512", "f32-1000", "f32-576"])
def test_refit_super_panel_form_equals_plain_form(ops, dtype, N, n, m):
    """One-wave refit: the 64-column super-panel instantiation (2 x 2 tiles per stream pass, lean value pass, in-register second
    update) against the plain instantiation of the same kernel on the same inputs, entry by entry -- incl. a ragged last block
    and an odd number of block columns -- and per-instance failure index.  (The super-panel fp64 instantiation sits at 256 + 256
    registers plus scratch; this is the check that caught a build of it whose last diagonal tile lost its jitter.)"""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(6, N, n, m, dtype=dtype, device=DEV, seed=900 + N)
    args = (p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    sup, plain = ops.REFIT_WAVE | ops.REFIT_SUPER_ON, ops.REFIT_WAVE | ops.REFIT_SUPER_OFF
    Lop_s, UHB_s, info_s, _ = ops.refit(*args, form=sup)
    Lop_p, UHB_p, info_p, _ = ops.refit(*args, form=plain)
    torch.cuda.synchronize()
    assert torch.equal(info_s, info_p) and int((info_s == 0).sum()) >= 4     # (a system that fp32 cannot factor fails in both forms alike)
    assert torch.equal(UHB_s, UHB_p)
    for i in torch.nonzero(info_s == 0).flatten().tolist():
        # (fp64: both forms accumulate the same products in a different order; fp32: cond x eps, as between the other forms)
        # (fp32: two different fp32 factorisations of a K_b with cond ~1e5 -- the factor is an internal representation, not
        #  a reference-exposed output; forward bound cond * eps = 6e-3, measured 4.4e-4; the posterior from it: 1e-3 below)
        rel_close(host(Lop_s[i]), host(Lop_p[i]), 1e-9 if f64 else 2e-3, what="super-panel vs plain form [%d]" % i)
    if not f64:
        # fp32 again with a jitter of order 1 on the diagonal: K_b is then well conditioned, the two forms agree to rounding, and
        # a jitter entry that went missing or to the wrong row would stand out
        big = (p["jitter"] * 5e4).contiguous()
        Lb_s, _, ib_s, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], big, form=sup)
        Lb_p, _, ib_p, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], big, form=plain)
        torch.cuda.synchronize()
        assert int((ib_s != 0).sum()) == 0 and int((ib_p != 0).sum()) == 0
        for i in range(6):
            rel_close(host(Lb_s[i]), host(Lb_p[i]), 2e-5, what="super-panel vs plain form, large jitter [%d]" % i)


_RETRY_FORMS = [("workgroup", "rbf"), ("wave", "rbf"), ("pair", "rbf"), ("team4", "rbf"), ("team8", "rbf"),
                ("team8", "matern52"), ("team8", "rbf_matern52")]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Bt,N,n,m", [(7, 33, 3, 2), (7, 100, 2, 1)])
@pytest.mark.parametrize("form,kernel", _RETRY_FORMS, ids=["%s-%s" % fk for fk in _RETRY_FORMS])
def test_refit_retry_factors_only_failed_instances_in_every_form(ops, form, kernel, Bt, N, n, m, dtype):
    """The retry's prev_info reaches the kernel of EVERY launch form (an explicit launcher argument): after a launch in which
    instance 5 fails at pivot 21, the operators of the six good instances are overwritten with a sentinel, instance 5's
    jitter is repaired and the retry runs under the same form -- info all zero, the sentinel rows bit for bit untouched (a
    launcher that lost prev_info would factor the whole batch again), row 5 equal to a fresh full refit with the repaired
    jitter.  Shapes: the smallest with a ragged second block, and with more than one block row."""
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    forced = {"workgroup": ops.REFIT_WORKGROUP, "wave": ops.REFIT_WAVE, "pair": ops.REFIT_PAIR, "team4": ops.REFIT_TEAM4,
              "team8": ops.REFIT_TEAM8}[form]
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=100 + N)
    X, UH, jit = (p["X"] * 2.0).contiguous(), p["UH"].clone(), p["jitter"].clone()
    X[5, 20], UH[5, 20] = X[5, 3], UH[5, 3]    # instance 5: a duplicated point with a negative shift -> pivot 21 fails
    jit[5] = 0.0
    jit[5, 20] = -1e-3 if f64 else -1e-2
    Lop, UHB, info, _ = ops.refit(X, UH, p["Bm"], p["ell"], p["s2"], jit, kernel=kernel, form=forced)
    want = [0] * Bt
    want[5] = 21
    assert info.tolist() == want
    good = torch.arange(Bt, device=DEV) != 5
    Lop[good] = 7.25                            # the sentinel
    jit[5] = p["jitter"][5]
    jit[5, 20] = 1e-3 if f64 else 1e-2          # repaired: the shift with its sign turned
    info2 = torch.full_like(info, 77)
    ops.refit_retry(X, UH, p["Bm"], p["ell"], p["s2"], jit, Lop, UHB, info, info2, kernel=kernel, form=forced)
    Lref, _, iref, _ = ops.refit(X, UH, p["Bm"], p["ell"], p["s2"], jit, kernel=kernel, form=forced)
    torch.cuda.synchronize()
    assert info2.tolist() == [0] * Bt and iref.tolist() == [0] * Bt
    assert torch.equal(Lop[good], torch.full_like(Lop[good], 7.25))
    rel_close(host(Lop[5]), host(Lref[5]), 1e-8 if f64 else 1e-3, what="retried operator vs fresh refit")


@pytest.mark.timeout(180)
def test_refit_handoff_protocols_soak(ops):
    """The chain / bulk refit kernels hand work over through spin waits on LDS counters; a lost wake-up would be a hang.
    A few hundred synchronised launches over random shapes, precisions, forms (library's choice, two waves, team of eight /
    four, one wave), dense outputs and failed pivots in random places (the long version: tools/stress_refit.py); every
    launch must come back, and the failure index must not depend on the form."""
    from bayesian_cbf_amd.synthetic import make_instances
    rng = np.random.default_rng(7)
    forms = {"default": None, "pair": ops.REFIT_PAIR, "team8": ops.REFIT_TEAM8, "team4": ops.REFIT_TEAM4, "wave": ops.REFIT_WAVE}
    launches = 0
    for _ in range(40):
        dtype = torch.float64 if rng.random() < 0.5 else torch.float32
        N = int(rng.choice([1, 31, 33, 100, 256, 300, 512]))
        Bt = int(rng.choice([1, 2, 7, 64, 300, 513]))
        n, m = [(2, 1), (3, 2), (6, 3)][int(rng.integers(3))]
        p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=int(rng.integers(1000)))
        jit = p["jitter"].clone()
        for _k in range(int(rng.integers(0, 3))):
            jit[int(rng.integers(Bt)), int(rng.integers(N))] = -10.0
        infos = {}
        for name, form in forms.items():
            for _rep in range(2):
                _, _, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit, want_dense=bool(rng.random() < 0.2 and N <= 300),
                                          form=form)
                torch.cuda.synchronize()
                launches += 1
            infos[name] = info.cpu().numpy()
        if dtype == torch.float64:              # (fp32: a pivot at rounding level may fail in one form and not in another)
            for name in forms:
                assert np.array_equal(infos[name], infos["wave"]), (name, N, Bt)
    assert launches == 400


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K", [5, 7])
def test_programs_with_more_than_four_cones_vs_oracle(ops, dtype, K):
    """BCBF_MAX_QUAD_CONSTRAINTS = 4 is the quad kernel's limit, not the library's: programs with up to
    BCBF_MAX_CONSTRAINTS = 8 cones (a third, fourth ... obstacle) go through bcbf_cbc_terms + the wide bcbf_coneqp
    instantiation (`ops.socp` routes).  Random feasible programs + one infeasible, against the oracle."""
    rng = np.random.default_rng(40 + K)
    Bt, m, rho = 48, 2, 2.326
    A, b, c, d = _random_programs(rng, Bt, m, K, rho)
    A[7, 1] = A[7, 2] = np.eye(3)[:, 1:] * 1e-3            # instance 7: two contradictory un-relaxed half planes
    b[7, 1] = b[7, 2] = [1.0, 0, 0]
    c[7, 1], c[7, 2] = [1.0, 0.0], [-1.0, 0.0]
    d[7, 1] = d[7, 2] = -1.0
    relax_mask = np.zeros(K); relax_mask[0] = 1.0
    w = np.full((Bt, m + 1), 0.33) * rng.uniform(0.5, 2.0, size=(Bt, m + 1))
    r = rng.normal(size=(Bt, m)) * 0.3
    if dtype == torch.float32:
        A, b, c, d, w, r = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (A, b, c, d, w, r))
    cones = ops.pack_cones(dev(A, dtype), dev(b, dtype), dev(c, dtype), dev(d, dtype))
    y, status, iters = ops.socp(dev(w, dtype), dev(r, dtype), cones, dev(relax_mask, dtype), dev(np.full(Bt, rho), dtype))
    st = status.cpu().numpy()
    assert st[7] != 0 and (np.delete(st, 7) == 0).all(), st
    yh = host(y)
    for i in range(Bt):
        if i == 7:
            continue
        sol = osocp.clf_cbf_socp(w[i], r[i], [(A[i, k], b[i, k], c[i, k], d[i, k]) for k in range(K)], rho, relax_mask)
        assert sol["status"] == "optimal"
        np.testing.assert_allclose(yh[i], sol["x"], rtol=1e-6 if dtype == torch.float64 else 1e-5,
                                   atol=1e-7 if dtype == torch.float64 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", ["matern52", "rbf_matern52"])
def test_matern52_option_kb_build_and_posterior_vs_oracle(ops, kernel, dtype):
    """The OPT-IN Matern-5/2 data kernel (bcbf_kb_build_matern52 -> bcbf_potrf -> bcbf_potrs ->
    bcbf_posterior_query_matern52) against the oracle's formula (which is checked against scikit-learn's Matern):
    dense K_b, and posterior M_k / B_k / W for per-instance queries and for queries of one shared model."""
    import scipy.linalg as sla
    from bayesian_cbf_amd.synthetic import make_instances
    Bt, N, n, m = 4, 70, 3, 2
    p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=12)
    f64 = dtype == torch.float64
    jit = p["jitter"] if f64 else (p["jitter"] * 100).contiguous()
    Kb = ops.kb_build(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
    Lop, info, _ = ops.potrf(Kb)
    assert (info == 0).all()
    UHB = (p["UH"] @ p["Bm"]).contiguous()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    Mk, Bk, W = ops.posterior_query(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"], shared=False,
                                    want_W=True, kernel=kernel)
    one = lambda t: t[:1].contiguous()
    Mk_s, Bk_s, _ = ops.posterior_query(one(Lop), one(Vw), one(p["X"]), one(UHB), one(p["ell"]), one(p["s2"]), one(p["Bm"]),
                                        one(p["M0"]), p["xq"], shared=True, kernel=kernel)
    h = {k: host(v) for k, v in p.items()}
    hj = host(jit)
    tol = 1e-9 if f64 else 1e-3          # (fp32 measured: 3.6e-7)
    for i in range(Bt):
        UH = h["UH"][i]
        K_o = ogp.DATA_KERNELS[kernel](h["X"][i], h["X"][i], h["ell"][i], h["s2"][i]) * (UH @ h["Bm"][i] @ UH.T) + np.diag(hj[i])
        rel_close(host(Kb)[i], K_o, 1e-12 if f64 else 1e-5, what="Kb")
        L = np.linalg.cholesky(K_o)
        Y = h["Xdot"][i] - UH @ h["M0"][i]
        cases = [(host(Mk)[i], host(Bk)[i])] + ([(host(Mk_s)[j], host(Bk_s)[j]) for j in range(Bt)] if i == 0 else [])
        for qi, (Mk_d, Bk_d) in enumerate(cases):
            xq = h["xq"][i] if qi == 0 else h["xq"][qi - 1]
            Phi = ogp.DATA_KERNELS[kernel](h["X"][i], xq[None], h["ell"][i], h["s2"][i])[:, :1] * (UH @ h["Bm"][i])
            W_o = sla.solve_triangular(L, Phi, lower=True)
            Mk_o = h["M0"][i].T + sla.solve_triangular(L, Y, lower=True).T @ W_o
            Bk_o = h["s2"][i] * h["Bm"][i] - W_o.T @ W_o
            rel_close(Mk_d, Mk_o, tol, scale=max(1.0, np.abs(Mk_o).max()), what="Mk")
            rel_close(Bk_d, Bk_o, tol, scale=float(h["s2"][i] * np.abs(h["Bm"][i]).max()), what="Bk")
            if qi == 0:
                rel_close(host(W)[i, :N], W_o, tol, scale=max(np.abs(W_o).max(), 1e-3), what="W")
    # the Matern posterior differs from the RBF one (the option is not silently ignored)
    Lr, UHBr, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
    Vr, _ = ops.potrs(Lr, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    Mr, Br = ops.posterior_step(Lr, Vr, p["X"], UHBr, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
    assert float((Br - Bk).abs().max()) > 1e-3


@pytest.mark.parametrize("kernel", ["matern52", "rbf_matern52"])
def test_matern52_option_facade_prediction_fit_append_and_derivative_gp(ops, kernel):
    """`ControlAffineRegressor(data_kernel=kernel)` (opt-in; no reference counterpart, formulas pinned in
    tests/test_oracle_formulas.py): custom_predict against the oracle; the likelihood gradient of fit() against central
    differences of the oracle's Matern likelihood; fit() lowers the loss; append_data equals a from-scratch state on all the
    points; the rel-degree-2 terms (derivative GP on the Matern jets) against the oracle's closed form."""
    import scipy.linalg as sla
    from oracle import cbc2 as oc2
    from bayesian_cbf_amd.control_affine_model import ControlAffineRegressor, ControlAffineRegressorExact
    from bayesian_cbf_amd.cbc2 import cbc2_quadratic_terms
    rng = np.random.default_rng(3)
    N, n, m, b = 40, 2, 1, 5
    X, U, Y = rng.normal(size=(N, n)), rng.normal(size=(N, m)), rng.normal(size=(N, n))
    A, B = np.array([[1.0, 0.2], [0.2, 0.5]]), np.array([[0.8, 0.1], [0.1, 0.6]])
    ell, s2, M0 = np.array([0.9, 1.3]), 0.7, rng.normal(size=(1 + m, n)) * 0.1
    f = dict(dtype=torch.float64, device=DEV)
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), **f)
    reg = ControlAffineRegressor(n, m, device=DEV, dtype=torch.float64, data_kernel=kernel)
    reg.set_kernel_params(A=A, B=B, lengthscale=ell, scalefactor=s2, M0=M0)
    reg.fit(T_(X), T_(U), T_(Y), training_iter=0)
    draws = []
    orig = reg.rand_fn
    reg.rand_fn = lambda k: draws.append(orig(k)) or draws[-1]
    Xt, Ut = rng.normal(size=(b, n)), rng.normal(size=(b, m))
    mean, cov = reg.custom_predict(T_(Xt), T_(Ut))
    UH, UHt = np.c_[np.ones(N), U], np.c_[np.ones(b), Ut]
    jit0 = 1e-5 * host(draws[0])
    K = ogp.DATA_KERNELS[kernel](X, X, ell, s2) * (UH @ B @ UH.T) + np.diag(jit0)
    L = np.linalg.cholesky(K)
    ks = ogp.DATA_KERNELS[kernel](X, Xt, ell, s2) * (UH @ B @ UHt.T)
    v = sla.solve_triangular(L, ks, lower=True)
    mean_o = UHt @ M0 + ks.T @ sla.cho_solve((L, True), Y - UH @ M0)
    sv_o = ogp.DATA_KERNELS[kernel](Xt, Xt, ell, s2) * (UHt @ B @ UHt.T) - v.T @ v
    rel_close(host(mean), mean_o, 1e-9, scale=max(1.0, np.abs(mean_o).max()), what="mean")
    rel_close(host(cov)[0], np.kron(sv_o, A), 1e-9, what="cov")
    # ---- rel-degree-2 terms through the facade (bcbf_posterior_jets_matern52 + bcbf_cbc2_terms(kernel_kind = 1))
    Pm = np.array([[1.3, 0.2], [0.2, 0.8]])
    qv = np.array([0.3, -0.4])
    hfun = lambda z: 0.5 * z @ T_(Pm) @ z + T_(qv) @ z - 1.0
    gfun = lambda z: T_(Pm) @ z + T_(qv)
    Hfun = lambda z: T_(Pm)
    x0, u0, ka = Xt[0], rng.random(m), np.array([1.0, 3.0])
    (mA, mb), (Q, pp, r), mean2, var2 = cbc2_quadratic_terms(reg, hfun, gfun, Hfun, T_(x0), T_(u0), ka)
    Yr = Y - UH @ M0
    jets = oc2.posterior_jets(L, Yr, X, UH @ B, ell, s2, B, M0, x0, kernel=kernel)
    (oA, ob), (oQ, op_, or_), omean, ovar = oc2.cbc2_terms(jets, A, B, ell, s2, float(0.5 * x0 @ Pm @ x0 + qv @ x0 - 1.0), Pm @ x0 + qv,
                                                           Pm, ka, u0, kernel=kernel)
    for name, val, ref in (("mean_A", mA, oA), ("mean_b", mb, ob), ("Q", Q, oQ), ("p", pp, op_), ("r", r, or_), ("mean", mean2, omean),
                           ("var", var2, ovar)):
        ref = np.asarray(ref)
        rel_close(host(val).reshape(ref.shape), ref, 1e-7, scale=max(np.abs(ref).max(), abs(float(ovar)), 1e-2), what=name)
    # ---- append_data: the last 6 points enter one by one == a state fitted on all the points (same jitter draws)
    reg2 = ControlAffineRegressor(n, m, device=DEV, dtype=torch.float64, data_kernel=kernel)
    reg2.set_kernel_params(A=A, B=B, lengthscale=ell, scalefactor=s2, M0=M0)
    jall = rng.random(N)
    seq = iter([jall[:N - 6]] + [jall[N - 6 + k:N - 5 + k] for k in range(6)])
    reg2.rand_fn = lambda k: T_(next(seq)[:k])
    reg2.fit(T_(X[:N - 6]), T_(U[:N - 6]), T_(Y[:N - 6]), training_iter=0)
    reg2._state()
    reg2.append_data(T_(X[N - 6:]), T_(U[N - 6:]), T_(Y[N - 6:]))
    assert reg2.Xtrain.shape[0] == N
    reg2.rand_fn = lambda k: T_(np.zeros(k))
    m2, c2 = reg2.custom_predict(T_(Xt), T_(Ut))
    K2 = ogp.DATA_KERNELS[kernel](X, X, ell, s2) * (UH @ B @ UH.T) + np.diag(1e-5 * jall)
    L2 = np.linalg.cholesky(K2)
    v2 = sla.solve_triangular(L2, ks, lower=True)
    rel_close(host(m2), UHt @ M0 + ks.T @ sla.cho_solve((L2, True), Y - UH @ M0), 1e-8, scale=max(1.0, np.abs(mean_o).max()), what="mean after append")
    rel_close(host(c2)[0], np.kron(ogp.DATA_KERNELS[kernel](Xt, Xt, ell, s2) * (UHt @ B @ UHt.T) - v2.T @ v2, A), 1e-7, what="cov after append")
    # ---- the likelihood gradient against central differences of the oracle's Matern likelihood, then a short fit
    jfix = 1e-5 * np.linspace(0.1, 0.9, N)
    reg.rand_fn = lambda k: T_(np.linspace(0.1, 0.9, N)[:k])

    def oracle_loss():
        mm = reg.model
        with torch.no_grad():
            return -ogp.marginal_log_likelihood(X, UH, Y, mm.A.cpu().numpy(), mm.B.cpu().numpy(), mm.lengthscale.cpu().numpy().ravel(),
                                                float(mm.outputscale), mm.M0.cpu().numpy(), jfix, kernel=kernel) / (N * n)
    for p_ in reg.model.parameters():
        p_.grad = None
    loss = reg.neg_mll_backward()
    np.testing.assert_allclose(loss, oracle_loss(), rtol=1e-9, atol=1e-10)
    for name, p_ in reg.model.named_parameters():
        flat, gflat = p_.data.view(-1), p_.grad.view(-1)
        for k in range(min(flat.numel(), 3)):
            old, h = float(flat[k]), 1e-5
            flat[k] = old + h; lp = oracle_loss()
            flat[k] = old - h; lm = oracle_loss()
            flat[k] = old
            np.testing.assert_allclose(float(gflat[k]), (lp - lm) / (2 * h), rtol=3e-5, atol=3e-7, err_msg="%s[%d]" % (name, k))
    reg.rand_fn = orig
    reg.fit(T_(X), T_(U), T_(Y), training_iter=15)
    assert reg.fit_losses[-1] < reg.fit_losses[0]
    with pytest.raises(ValueError):
        ControlAffineRegressorExact(n, m, device=DEV, data_kernel="matern32")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", ["matern52", "rbf_matern52"])
def test_matern52_fused_refit_equals_build_then_factor_and_jets_vs_oracle(ops, kernel, dtype):
    """bcbf_refit_matern52 (fused values + jittered Cholesky + packing, the team form) gives the factor of
    bcbf_kb_build_matern52 -> bcbf_potrf (posterior through either within rounding); bcbf_posterior_jets_matern52 against the
    oracle's Matern jets for batches of instances, two shapes, ragged N."""
    from oracle import cbc2 as oc2
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    for (N, n, m) in ((100, 2, 1), (300, 3, 2)):
        Bt = 3
        p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=40 + N)
        X, xq = (p["X"] * 2.0).contiguous(), (p["xq"] * 2.0).contiguous()
        jit = (p["jitter"] * (1 if f64 else 1e2)).contiguous()
        Lop, UHB, info, _ = ops.refit(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
        assert (info == 0).all()
        Kb = ops.kb_build(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
        Lop2, info2, _ = ops.potrf(Kb)
        assert (info2 == 0).all()
        Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        Vw2, _ = ops.potrs(Lop2, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        q = lambda L_, V_: ops.posterior_query(L_, V_, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, shared=False, kernel=kernel)
        (Mk1, Bk1, _), (Mk2, Bk2, _) = q(Lop, Vw), q(Lop2, Vw2)
        tol = 1e-9 if f64 else 1e-3      # (fp32 measured: 1.9e-7)
        rel_close(host(Mk1), host(Mk2), tol, scale=max(1.0, float(Mk2.abs().max())), what="Mk fused vs build+factor")
        rel_close(host(Bk1), host(Bk2), tol, scale=float((p["s2"][:, None, None] * p["Bm"]).abs().max()), what="Bk fused vs build+factor")
        Mk, Bk, G, Mj = ops.posterior_jets(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, kernel=kernel)
        h = {k: host(v) for k, v in p.items()}
        hX, hxq, hj = host(X), host(xq), host(jit)
        C = m + 1
        jt = 1e-8 if f64 else 1e-3       # (fp32 measured: 3.8e-7)
        for i in range(Bt):
            UH = h["UH"][i]
            K = ogp.DATA_KERNELS[kernel](hX[i], hX[i], h["ell"][i], h["s2"][i]) * (UH @ h["Bm"][i] @ UH.T) + np.diag(hj[i])
            L = np.linalg.cholesky(K)
            jets = oc2.posterior_jets(L, h["Xdot"][i] - UH @ h["M0"][i], hX[i], UH @ h["Bm"][i], h["ell"][i], float(h["s2"][i]), h["Bm"][i],
                                      h["M0"][i], hxq[i], kernel=kernel)
            prior = float(h["s2"][i] * np.abs(h["Bm"][i]).max())
            rel_close(host(Mk)[i], jets["Mk"], jt, scale=max(1.0, np.abs(jets["Mk"]).max()), what="Mk")
            rel_close(host(Bk)[i], jets["Bk"], jt, scale=prior, what="Bk")
            Gh, Mjh = host(G)[i], host(Mj)[i]
            gscale = max(np.abs(jets["G11"]).max(), np.abs(jets["G10"]).max(), prior, 1e-3)
            for d in range(n):
                rel_close(Gh[(1 + d) * C:(2 + d) * C, :C], jets["G10"][d], jt, scale=gscale, what="G10")
                rel_close(Mjh[:, (1 + d) * C:(2 + d) * C], jets["dMk"][d], jt, scale=max(1.0, np.abs(jets["dMk"]).max()), what="dMk")
                for e in range(n):
                    rel_close(Gh[(1 + d) * C:(2 + d) * C, (1 + e) * C:(2 + e) * C], jets["G11"][d][e], jt, scale=gscale, what="G11")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_syrk_kb_inverse_and_deterministic_likelihood_gradient(ops, dtype):
    """Fit path without a BLAS call and without float atomics: K_b^-1 = Linv' Linv on the matrix cores (bcbf_syrk_lt) is the
    inverse of the oracle's K_b (and symmetric bit for bit); bcbf_mll_grad's split form (partial sums through the
    workspace, added in a fixed order) returns BIT-IDENTICAL gradients from repeated launches and agrees with the
    one-workgroup form."""
    from bayesian_cbf_amd.synthetic import make_instances
    from bayesian_cbf_amd import _lib
    f64 = dtype == torch.float64
    for N in (33, 100, 512):
        Bt, n, m = 2, 3, 2
        p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=N)
        X = (p["X"] * 3.0).contiguous()                   # well conditioned: the check is on the arithmetic
        jit = (p["jitter"] * (1 if f64 else 1e3)).contiguous()
        Lop, UHB, info, _ = ops.refit(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit)
        assert (info == 0).all()
        Kinv = ops.kb_inverse(Lop, N)
        assert torch.equal(Kinv, Kinv.transpose(1, 2))
        Kb = ops.kb_build(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit).double()
        res = (Kb @ Kinv.double() - torch.eye(N, dtype=torch.float64, device=DEV)).abs().max()
        cond = float(torch.linalg.cond(Kb).max())
        assert float(res) < (1e-13 if f64 else 1e-5) * cond, (N, float(res), cond)
        np.testing.assert_allclose(host(Kinv), host(ops.kb_inverse(Lop, N, gemm=False)), rtol=0,
                                   atol=(1e-9 if f64 else 1e-2) * float(Kinv.abs().max()))
        R = (p["Xdot"] - p["UH"] @ p["M0"]).contiguous()
        alpha = (Kinv @ R).contiguous()
        Ainv = torch.linalg.inv(p["A"].double()).to(dtype).contiguous()
        args = (Lop, alpha, Kinv, X, p["UH"], R, Ainv, p["Bm"], p["ell"], p["s2"])
        first = ops.mll_grad(*args)
        for _ in range(3):
            again = ops.mll_grad(*args)
            assert all(torch.equal(a, b) for a, b in zip(first, again)), "the split form must be deterministic"
        # workspace: one slot set per workgroup of a model -- the pair form's split (few models) or the row form's row chunks x column
        # slices (round 6), whichever is larger
        g_pairs = min(128, -(-N * N // 8192))
        rc, tiles = -(-N // 256), -(-N // 128)
        g_rows = rc * max(1, min(128 // rc, tiles))
        assert int(_lib.lib.bcbf_mll_grad_work_bytes(Bt, N, m)) == 8 * Bt * max(g_pairs, g_rows) * 26
        saved = ops._mll_work
        ops._mll_work = lambda *a: None                   # no workspace: one workgroup per model
        try:
            single = ops.mll_grad(*args)
        finally:
            ops._mll_work = saved
        for a, b in zip(first, single):
            np.testing.assert_allclose(host(a), host(b), rtol=1e-10 if f64 else 2e-4, atol=(1e-10 if f64 else 2e-4) * float(b.abs().max()))


@pytest.mark.parametrize("kernel", ["rbf", "matern52", "rbf_matern52"])
@pytest.mark.parametrize("n,m", [(3, 2), (2, 1)])
def test_posterior_jets_matrix_core_form_equals_streaming_form(ops, n, m, kernel, monkeypatch):
    """jets_mfma.hip (fp32; residual in MFMA accumulators, operator through an LDS-DMA ring) against the streaming kernel on the same inputs, output by
    output -- one GP per query and ONE shared GP for all queries (`shared`), the opt-in data kernels, sizes with a ragged last block / a half-filled last
    64-row group / the largest the form takes, with and without the W output."""
    from bayesian_cbf_amd.synthetic import make_instances
    for Bt, N, shared in ((5, 512, False), (3, 300, False), (37, 480, True), (4, 33, False), (2, 64, True)):
        p = make_instances(1 if shared else Bt, N, n, m, dtype=torch.float32, device=DEV, seed=31 * n + m + N)
        jit = (p["jitter"] * 1e3).contiguous()
        Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
        assert (info == 0).all()
        Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        g = torch.Generator(device=DEV).manual_seed(N)
        xq = (p["X"][0, :Bt] if shared else p["X"][:, 0]) + 0.3 * torch.randn(Bt, n, device=DEV, generator=g)
        xq = xq.contiguous()
        out = {}
        for form in ("0", "2"):
            monkeypatch.setenv("BCBF_JETS_MFMA", form)
            out[form] = ops.posterior_jets(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, shared=shared, want_W=True, kernel=kernel)
        torch.cuda.synchronize()
        for name, a, b in zip(("Mk", "Bk", "G", "Mj", "Wj"), out["0"], out["2"]):
            sc = max(float(a.abs().max()), 1e-3)
            if name == "Bk":                                   # (B_k = s2 B - W'W cancels: held to the prior's scale, as everywhere)
                sc = max(sc, float((p["s2"].abs().max() * p["Bm"].abs().max())))
            rel_close(host(b), host(a), 2e-4, scale=sc, what="%s %s N=%d shared=%s" % (kernel, name, N, shared))      # (fp32 sums in a different order; measured <= 3e-5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,m,form", [(n_, m_, "default") for n_ in (1, 2, 3, 4) for m_ in (1, 2, 3)] + [(2, 1, "mfma"), (2, 2, "mfma"), (3, 1, "mfma"), (3, 2, "mfma")])
def test_posterior_jets_every_compiled_shape_and_workgroup_size_vs_oracle(ops, n, m, form, dtype, monkeypatch):
    """("mfma": the same with BCBF_JETS_MFMA=2 -- the matrix-core form of jets_mfma.hip, residual in MFMA accumulators and the operator through an
    LDS-DMA ring, forced for every shape it takes (fp32, N <= 512; by default it runs for twelve right-hand-side columns only).)
    The jets instantiations (Gram / mean sums on the matrix-core accumulators of wave 0) for EVERY (n <= 4, m <= 3) --
    wherever the value kernels and the rel-degree-2 terms kernel work (gp_algebra.py:319-402, cbc2.py:26-33 hold for any
    state / control dimension); (3,3), (4,2), (4,3) have more than 16 tile columns and run the 2 x 2 accumulator form --
    and for training sizes that take one wave, several waves and a ragged last block per workgroup, against the oracle's
    jets: M_k, B_k, dM_k/dx, dW_d'W, dW_d'dW_e, the Wj output against the oracle's triangular solves, and the
    rel-degree-2 terms of a random quadratic barrier formed from those jets (bcbf_cbc2_terms) against the oracle's."""
    import scipy.linalg as sla
    from oracle import cbc2 as oc2
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    if form == "mfma":
        if f64:
            pytest.skip("the matrix-core jets form is fp32")
        monkeypatch.setenv("BCBF_JETS_MFMA", "2")
    C = m + 1
    for N in (40, 300, 700):
        Bt = 3
        p = make_instances(Bt, N, n, m, dtype=dtype, device=DEV, seed=100 * n + m + N)
        X = (p["X"] * 2.0).contiguous()
        xq = (p["xq"] * 2.0).contiguous()
        jit = (p["jitter"] * (1 if f64 else 1e3)).contiguous()
        Lop, UHB, info, _ = ops.refit(X, p["UH"], p["Bm"], p["ell"], p["s2"], jit)
        assert (info == 0).all()
        Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        Mk, Bk, G, Mj, Wj = ops.posterior_jets(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq, want_W=True)
        h = {k: host(v) for k, v in p.items()}
        hX, hxq, hj = host(X), host(xq), host(jit)
        tol = 1e-8 if f64 else 1e-3      # (fp32 measured: values 1e-4, d/dx columns 2.6e-4, Gram blocks 1.1e-5)
        for i in range(Bt):
            st = ogp.refit_state(hX[i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i], hj[i][None] / 1e-5)
            jets = oc2.posterior_jets(st["L"], st["Y"], hX[i], st["UHB"], h["ell"][i], float(h["s2"][i]), h["Bm"][i], h["M0"][i], hxq[i])
            prior = float(h["s2"][i] * np.abs(h["Bm"][i]).max())
            rel_close(host(Mk)[i], jets["Mk"], tol, scale=max(1.0, np.abs(jets["Mk"]).max()), what="Mk N=%d" % N)
            rel_close(host(Bk)[i], jets["Bk"], tol, scale=prior, what="Bk N=%d" % N)
            Gh, Mjh = host(G)[i], host(Mj)[i]
            assert np.array_equal(Gh, Gh.T)
            gscale = max(np.abs(jets["G11"]).max(), np.abs(jets["G10"]).max(), prior, 1e-3)
            rel_close(Gh[:C, :C], h["s2"][i] * h["Bm"][i] - jets["Bk"], tol, scale=gscale, what="G00")
            for d in range(n):
                rel_close(Gh[(1 + d) * C:(2 + d) * C, :C], jets["G10"][d], tol, scale=gscale, what="G10")
                rel_close(Mjh[:, (1 + d) * C:(2 + d) * C], jets["dMk"][d], tol, scale=max(1.0, np.abs(jets["dMk"]).max()), what="dMk")
                for e in range(n):
                    rel_close(Gh[(1 + d) * C:(2 + d) * C, (1 + e) * C:(2 + e) * C], jets["G11"][d][e], tol, scale=gscale, what="G11")
            kstar = ogp.rbf_ard_kernel(hX[i], hxq[i][None], h["ell"][i], h["s2"][i])[:, 0]
            W_o = sla.solve_triangular(st["L"], kstar[:, None] * st["UHB"], lower=True)
            rel_close(host(Wj)[i, :N, :C], W_o, tol, scale=max(np.abs(W_o).max(), 1e-3), what="Wj values")
            d0 = -(hxq[i][0] - hX[i][:, 0]) / h["ell"][i][0] ** 2 * kstar
            dW_o = sla.solve_triangular(st["L"], d0[:, None] * st["UHB"], lower=True)
            rel_close(host(Wj)[i, :N, C:2 * C], dW_o, tol, scale=max(np.abs(dW_o).max(), 1e-3), what="Wj d/dx0")
        # rel-degree-2 terms from these jets: h(x) = 1/2 x'Px + q'x - 1 with a random symmetric P
        rng = np.random.RandomState(7 * n + m + N)
        P = rng.randn(n, n)
        P = 0.5 * (P + P.T) + n * np.eye(n)
        qv, u0, ka = rng.randn(n), rng.rand(Bt, m), np.array([1.0, 3.0])
        hv = np.array([0.5 * x_ @ P @ x_ + qv @ x_ - 1.0 for x_ in hxq])
        gh = np.stack([P @ x_ + qv for x_ in hxq])
        Hh = np.broadcast_to(P, (Bt, n, n)).copy()
        (mA, mb), (Q, pp, r), mean, var, status = ops.cbc2_terms(
            Mk, Bk, G, Mj, p["A"], p["Bm"], p["ell"], p["s2"], dev(hv, dtype), dev(gh, dtype), dev(Hh, dtype), dev(ka, dtype),
            dev(u0, dtype))
        assert (status == 0).all()
        ttol = 1e-7 if f64 else 1e-4
        for i in range(Bt):
            st = ogp.refit_state(hX[i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i], hj[i][None] / 1e-5)
            jets = oc2.posterior_jets(st["L"], st["Y"], hX[i], st["UHB"], h["ell"][i], float(h["s2"][i]), h["Bm"][i], h["M0"][i], hxq[i])
            if not f64:
                # fp32: the jets were held to 1e-3 of their scale above; the terms are differences of products of them, so
                # the terms KERNEL is checked on the jets it was given (the device's, widened to fp64)
                Gh, Mjh = host(G)[i], host(Mj)[i]
                blk = lambda d: slice((1 + d) * C, (2 + d) * C)
                jets = dict(Mk=host(Mk)[i], Bk=host(Bk)[i], dMk=np.stack([Mjh[:, blk(d)] for d in range(n)]),
                            G10=np.stack([Gh[blk(d), :C] for d in range(n)]),
                            G11=np.stack([np.stack([Gh[blk(d), blk(e)] for e in range(n)]) for d in range(n)]))
            (oA, ob), (oQ, op_, or_), omean, ovar = oc2.cbc2_terms(jets, h["A"][i], h["Bm"][i], h["ell"][i], float(h["s2"][i]),
                                                                   float(hv[i]), gh[i], Hh[i], ka, u0[i])
            for name, val, ref in (("mean_A", mA, oA), ("mean_b", mb, ob), ("Q", Q, oQ), ("p", pp, op_), ("r", r, or_),
                                   ("mean", mean, omean), ("var", var, ovar)):
                ref = np.asarray(ref)
                # (the variance polynomial's coefficients cancel against one another: one scale for Q, p, r, var)
                vs = max(np.abs(oQ).max(), np.abs(op_).max(), abs(float(or_)), abs(float(ovar)), 1e-2)
                ms = max(np.abs(oA).max(), abs(float(ob)), abs(float(omean)), 1e-2)
                rel_close(host(val)[i].reshape(ref.shape), ref, ttol, scale=ms if name.startswith("mean") else vs, what=name)


# --------------------------------------------------------------------------------------------
# The opt-in Matern-5/2 data kernel in regime S (matrix-core query) and in the fused control step
@pytest.mark.parametrize("N,n,m,b,dtype", [(512, 3, 2, 203, torch.float32), (100, 3, 2, 21, torch.float32), (256, 2, 1, 64, torch.float32),
                                           (1024, 3, 2, 37, torch.float32), (512, 3, 2, 5200, torch.float32),
                                           (512, 3, 2, 203, torch.float64), (100, 2, 1, 19, torch.float64), (480, 4, 3, 37, torch.float64)])
@pytest.mark.parametrize("kernel", ["matern52", "rbf_matern52"])
def test_matern52_shared_gp_matrix_core_queries_vs_oracle(ops, kernel, N, n, m, b, dtype):
    """bcbf_posterior_shared_matern52 (the regime-S matrix-core kernels with the Matern-5/2 value in the prologue; register-
    resident form N <= 512, the fp32 LDS-slab form beyond; 5200 queries: the five-queries-per-wave packing) against the oracle's
    Matern posterior, ragged b and N; `posterior_query(shared=True, kernel=kernel)` routes to the same kernel; the RBF
    result on the same factor differs (the switch is not ignored)."""
    import scipy.linalg as sla
    from bayesian_cbf_amd.synthetic import make_instances
    f64 = dtype == torch.float64
    p = make_instances(1, N, n, m, dtype=dtype, device=DEV, seed=40 + N + m)
    p["X"] = (p["X"] * (1.0 if f64 else 2.0)).contiguous()
    jit = p["jitter"] if f64 else (p["jitter"] * 100).contiguous()
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
    assert int(info[0]) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    g = torch.Generator(device=DEV).manual_seed(5)
    lo, hi = p["X"][0].amin(dim=0), p["X"][0].amax(dim=0)
    xq = (lo + (hi - lo) * torch.rand(b, n, generator=g, dtype=dtype, device=DEV)).contiguous()
    args = (Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], xq)
    Mk, Bk, W = ops.posterior_shared(*args, want_W=True, kernel=kernel)
    Mq, Bq, _ = ops.posterior_query(*args, shared=True, kernel=kernel)
    assert torch.equal(Mk, Mq) and torch.equal(Bk, Bq)
    Mr, Br, _ = ops.posterior_shared(*args)
    assert float((Br - Bk).abs().max()) > 1e-4
    h = {k: host(v)[0] for k, v in p.items()}
    UH = h["UH"]
    K_o = ogp.DATA_KERNELS[kernel](h["X"], h["X"], h["ell"], h["s2"]) * (UH @ h["Bm"] @ UH.T) + np.diag(host(jit)[0])
    L = np.linalg.cholesky(K_o)
    V_o = sla.solve_triangular(L, h["Xdot"] - UH @ h["M0"], lower=True)
    prior = float(h["s2"] * np.abs(h["Bm"]).max())
    tol = 1e-8 if f64 else 1e-3
    hx = host(xq)
    for i in sorted(set(np.linspace(0, b - 1, min(b, 40)).astype(int))):
        Phi = ogp.DATA_KERNELS[kernel](h["X"], hx[i][None], h["ell"], h["s2"])[:, :1] * (UH @ h["Bm"])
        W_o = sla.solve_triangular(L, Phi, lower=True)
        rel_close(host(Mk)[i], h["M0"].T + V_o.T @ W_o, tol, scale=max(1.0, np.abs(V_o.T @ W_o).max()), what="Mk matern shared")
        rel_close(host(Bk)[i], h["s2"] * h["Bm"] - W_o.T @ W_o, tol, scale=prior, what="Bk matern shared")
        rel_close(host(W)[i, :N], W_o, tol, scale=max(np.abs(W_o).max(), 1e-3), what="W matern shared")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shared", [False, True], ids=["instance-gps", "shared-gp"])
@pytest.mark.parametrize("kernel", ["matern52", "rbf_matern52"])
def test_matern52_fused_control_step_vs_composed_path_and_oracle(ops, kernel, dtype, shared):
    """bcbf_unicycle_control_step_matern52 (gp["kernel"] = "matern52"): posterior of a Matern-5/2 model + the fused task rows /
    terms / SOCP / plant step in one host call == the composed entry points on the same model, and the posterior it leaves in the
    workspace is the oracle's Matern posterior; the RBF step on the same tensors gives a different posterior."""
    import scipy.linalg as sla
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    f64 = dtype == torch.float64
    Bt, N, n, m = 70, 96, 3, 2
    p = make_instances(1 if shared else Bt, N, n, m, dtype=dtype, device=DEV, seed=61)
    t = make_unicycle_task(Bt, dtype=dtype, device=DEV, seed=62)
    jit = p["jitter"] if f64 else (p["jitter"] * 100).contiguous()
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit, kernel=kernel)
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"], kernel=kernel)
    x1, x2 = t["x"].clone(), t["x"].clone()
    ws1, ws2 = ops.control_workspace(Bt, 2, dtype, DEV), ops.control_workspace(Bt, 2, dtype, DEV)
    ops.unicycle_control_step(gp, t, ws1, x1, dt=0.01, L_true=1.0, L_mean=4.0, clf_gamma=10.0, max_iters=40)
    ops._unicycle_control_step_composed(gp, t, ws2, x2, 0.01, 1.0, 4.0, 10.0, 40)
    prior = float((p["s2"][:, None, None] * p["Bm"]).abs().max())
    tol = 1e-9 if f64 else 1e-4
    rel_close(host(ws1["Mk"]), host(ws2["Mk"]), tol, scale=max(1.0, float(ws2["Mk"].abs().max())), what="Mk fused vs composed")
    rel_close(host(ws1["Bk"]), host(ws2["Bk"]), tol, scale=prior, what="Bk fused vs composed")
    ok = ((ws1["status"] == 0) & (ws2["status"] == 0)).cpu().numpy()
    assert ok.sum() >= 10, int(ok.sum())          # (this small-N synthetic task leaves many programs infeasible)
    assert int((ws1["status"] != ws2["status"]).sum()) <= 1, (ws1["status"] != ws2["status"]).nonzero().flatten().tolist()
    ytol = 1e-6 if f64 else 1e-3
    all_close(host(ws1["y"])[ok], host(ws2["y"])[ok], ytol, ytol, what="matern control y fused vs composed")
    all_close(host(x1)[ok], host(x2)[ok], ytol, ytol, what="matern control x fused vs composed")
    # posterior vs the oracle's Matern formula
    h = {k: host(v) for k, v in p.items()}
    hx, hj = host(t["x"]), host(jit)
    ptol = 1e-8 if f64 else 1e-3
    for i in (0, 1, 17, 69):
        gi = 0 if shared else i
        UH = h["UH"][gi]
        K_o = ogp.DATA_KERNELS[kernel](h["X"][gi], h["X"][gi], h["ell"][gi], h["s2"][gi]) * (UH @ h["Bm"][gi] @ UH.T) + np.diag(hj[gi])
        L = np.linalg.cholesky(K_o)
        Phi = ogp.DATA_KERNELS[kernel](h["X"][gi], hx[i][None], h["ell"][gi], h["s2"][gi])[:, :1] * (UH @ h["Bm"][gi])
        W_o = sla.solve_triangular(L, Phi, lower=True)
        Mk_o = h["M0"][gi].T + sla.solve_triangular(L, h["Xdot"][gi] - UH @ h["M0"][gi], lower=True).T @ W_o
        rel_close(host(ws1["Mk"])[i], Mk_o, ptol, scale=max(1.0, np.abs(Mk_o).max()), what="Mk matern control step")
        rel_close(host(ws1["Bk"])[i], h["s2"][gi] * h["Bm"][gi] - W_o.T @ W_o, ptol, scale=float(h["s2"][gi] * np.abs(h["Bm"][gi]).max()),
                  what="Bk matern control step")
    ws3, x3 = ops.control_workspace(Bt, 2, dtype, DEV), t["x"].clone()
    ops.unicycle_control_step(dict(gp, kernel="rbf"), t, ws3, x3, dt=0.01, L_true=1.0, L_mean=4.0, clf_gamma=10.0, max_iters=40)
    assert float((ws3["Bk"] - ws1["Bk"]).abs().max()) > 1e-4
