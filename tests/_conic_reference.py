"""Cone-program families and an optimality check that does not trust the reference's `x` (numpy fp64 only, no torch).

A program is  min 1/2 y'P y + q'y  s.t.  h - G y in K = R_+^l x Q^{q_1} x ...   A point y is accepted as optimal when

  feasibility   every cone's margin (h - G y)_0 - |(h - G y)_{1:}| (a linear row: the row itself) is >= -eps_f max(1, |h|),
  objective     f(y) - lb <= eps_g max(1, |f(y)|), where lb = -1/2 (q + G'z)' P^-1 (q + G'z) - h'z is the Lagrangian's
                minimum over y at a multiplier z in K: a lower bound of the optimal value for ANY z in K (weak duality),
                whatever the stationarity residual of the solver that produced z.

With P > 0 the two imply  |y - y*|^2 <= 2 (f(y) - lb + feasibility slop) / lambda_min(P): closeness to the optimum follows
from the program's own data, the numpy port contributes a multiplier and nothing else.

Tolerances (`tolerances`): ten times the worst figure the numpy port's own `x` shows on the family (REF_WORST, asserted by
tests/test_conic_reference_cpu.py on every case the GPU tests run) -- both sides run the same algorithm to the same 1e-9 stop
tolerances in a different operation order -- and never above 1e-7, the solvers' own accept level.
"""
import functools

import numpy as np

from oracle import socp as osocp

ACCEPT = 1e-7                     # the device solvers' best-iterate accept level: no figure above it passes
LEFT_OUT_CAP = 0.02               # share of a case's programs the numpy port may fail to solve
RHOS = (0.0, 0.5, 2.326, 4.0)
MASKS = ("first", "none", "all")
EPS32 = 2.0 ** -23

# worst (feasibility, objective) figure of the numpy port's own x over every case of the family that the GPU tests run
# (fp64 programs and their fp32-rounded twins); test_conic_reference_cpu.py asserts that no case exceeds them
REF_WORST = {
    "clf_cbf": (7e-10, 1.1e-9),     # measured 6.67e-10, 1.00e-9
    "generic": (9e-10, 1.0e-9),     # measured 8.09e-10, 9.92e-10
    "p0": (1e-10, None),            # measured 9.54e-11 (no bound without P > 0)
}


def tolerances(family):
    """(eps_f, eps_g) of the family: ten times the reference's worst, capped at the accept level."""
    f, g = REF_WORST[family]
    return min(10.0 * f, ACCEPT), (None if g is None else min(10.0 * g, ACCEPT))


# ------------------------------------------------------------------------------------------------ generators
def relax_mask(pattern, K):
    mask = np.zeros(K)
    if pattern == "first":
        mask[0] = 1.0
    elif pattern == "all":
        mask[:] = 1.0
    elif pattern != "none":
        raise ValueError(pattern)
    return mask


def clf_cbf_family(seed, Bt, m, K, f32=False):
    """CLF-CBF programs  min sum w_i (u_i - r_i)^2 + w_m relax^2  s.t.  c_k'u + d_k + mask_k relax >= rho |A_k u + b_k|.
    Cones from Cholesky rows, strictly feasible at u_f (relax = 0) by construction; per instance: rho from RHOS (0: every cone
    a half-plane), slack log-uniform in [1e-6, 2], weights 0.33 * 10^U(-3, 3), reference r = u_f + 5 N(0, 1) so that cones are
    active at the optimum.  f32: every array rounded to fp32 (the program the fp32 entry points see)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((Bt, K, m + 1, m)); b = np.zeros((Bt, K, m + 1)); c = np.zeros((Bt, K, m)); d = np.zeros((Bt, K))
    rho = rng.choice(RHOS, size=Bt)
    w = 0.33 * 10.0 ** rng.uniform(-3.0, 3.0, size=(Bt, m + 1))
    r = np.zeros((Bt, m))
    for i in range(Bt):
        u_f = rng.normal(size=m)
        r[i] = u_f + 5.0 * rng.normal(size=m)
        for k in range(K):
            Asq = rng.normal(size=(m + 1, m + 1))
            Asq = Asq @ Asq.T * rng.uniform(0.001, 1) + 1e-4 * np.eye(m + 1)
            Lc = np.linalg.cholesky(Asq)
            A[i, k], b[i, k] = Lc.T[:, 1:], Lc.T[:, 0]
            c[i, k] = rng.normal(size=m) * 3
            slack = 10.0 ** rng.uniform(-6.0, np.log10(2.0))
            d[i, k] = rho[i] * np.linalg.norm(A[i, k] @ u_f + b[i, k]) - c[i, k] @ u_f + slack
    out = dict(A=A, b=b, c=c, d=d, w=w, r=r, rho=rho)
    if f32:
        out = {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}
    return out


def clf_cbf_generic_form(p, mask, i):
    """(P, q, G, h, dims) of instance i of a CLF-CBF batch: rows [-c', -mask; -rho A, 0], h = [d; rho b]."""
    A, b, c, d, w, r, rho = (p[k][i] for k in ("A", "b", "c", "d", "w", "r", "rho"))
    K, D, m = A.shape[0], A.shape[1] + 1, A.shape[2]
    nv = m + 1
    P = 2.0 * np.diag(w)
    q = np.zeros(nv)
    q[:m] = -2.0 * w[:m] * r
    G = np.zeros((K, D, nv)); h = np.zeros((K, D))
    G[:, 0, :m] = -c
    G[:, 0, m] = -np.asarray(mask, dtype=np.float64)
    G[:, 1:, :m] = -rho * A
    h[:, 0] = d
    h[:, 1:] = rho * b
    return P, q, G.reshape(K * D, nv), h.reshape(K * D), dict(l=0, q=[D] * K)


def _interior_point(rng, l, qdims):
    """A point strictly inside K, margins in [0.1, 2]."""
    parts = [rng.uniform(0.1, 2.0, size=l)]
    for dq in qdims:
        v = rng.normal(size=dq - 1)
        parts.append(np.concatenate([[np.linalg.norm(v) + rng.uniform(0.1, 2.0)], v]))
    return np.concatenate(parts)


def generic_family(seed, Bt, nv, l, qdims):
    """G random, h = G x0 + s0 with s0 strictly inside K, P = A A' U(0.01, 1) + 1e-3 I, q = 10 N(0, 1)."""
    rng = np.random.default_rng(seed)
    Kt = l + sum(qdims)
    P = np.zeros((Bt, nv, nv)); q = np.zeros((Bt, nv)); G = np.zeros((Bt, Kt, nv)); h = np.zeros((Bt, Kt))
    for i in range(Bt):
        G[i] = rng.normal(size=(Kt, nv))
        h[i] = G[i] @ rng.normal(size=nv) + _interior_point(rng, l, qdims)
        Aq = rng.normal(size=(nv, nv))
        P[i] = Aq @ Aq.T * rng.uniform(0.01, 1.0) + 1e-3 * np.eye(nv)
        q[i] = 10.0 * rng.normal(size=nv)
    return dict(P=P, q=q, G=G, h=h, dims=dict(l=l, q=list(qdims)))


def p0_family(seed, Bt, nv, l, qdims):
    """P = 0: q = -G'z0 with z0 strictly inside K (the objective is bounded below on the feasible set: q'x = -z0'(Gx) >=
    -z0'h), G of full column rank (redrawn until its smallest singular value is >= 0.1), h = G x0 + s0 as above."""
    rng = np.random.default_rng(seed)
    Kt = l + sum(qdims)
    assert Kt >= nv
    q = np.zeros((Bt, nv)); G = np.zeros((Bt, Kt, nv)); h = np.zeros((Bt, Kt))
    for i in range(Bt):
        while True:
            G[i] = rng.normal(size=(Kt, nv))
            if np.linalg.svd(G[i], compute_uv=False)[-1] >= 0.1:
                break
        h[i] = G[i] @ rng.normal(size=nv) + _interior_point(rng, l, qdims)
        q[i] = -G[i].T @ _interior_point(rng, l, qdims)
    return dict(P=np.zeros((Bt, nv, nv)), q=q, G=G, h=h, dims=dict(l=l, q=list(qdims)))


def instance(p, i):
    """(P, q, G, h, dims) of instance i of a generic / P = 0 batch."""
    return p["P"][i], p["q"][i], p["G"][i], p["h"][i], p["dims"]


# ------------------------------------------------------------------------------------------------ the check
def objective(P, q, y):
    return 0.5 * y @ P @ y + q @ y


def cone_margins(v, dims):
    """Per cone of K (linear rows first): v_i, or v_0 - |v_{1:}|.  v is in K iff every margin is >= 0."""
    l = dims.get("l", 0)
    return np.concatenate([v[:l], [v[a] - np.linalg.norm(v[a + 1:e]) for a, e in osocp._blocks(dims)]])


def lower_bound(P, q, G, h, z):
    """min_y 1/2 y'Py + q'y + z'(G y - h): a lower bound of the optimal value for any z in K (P > 0)."""
    g = q + G.T @ z
    return -0.5 * g @ np.linalg.solve(P, g) - h @ z


def rounding_slack(P, q, G, dims, y, eps=EPS32):
    """What a componentwise relative perturbation |dy_i| <= eps |y_i| (rounding y to fp32: eps = 2^-23) can change:
    (|df| bound, per-cone margin change bound).  df <= |P y + q|'|dy| + 1/2 |dy|'|P||dy|; a cone's margin moves by at most
    |(G dy)_0| + |(G dy)_{1:}| <= (|G| |dy|)_0 + | (|G| |dy|)_{1:} |."""
    dy = eps * np.abs(y)
    df = np.abs(P @ y + q) @ dy + 0.5 * dy @ np.abs(P) @ dy
    gd = np.abs(G) @ dy
    l = dims.get("l", 0)
    dm = np.concatenate([gd[:l], [gd[a] + np.linalg.norm(gd[a + 1:e]) for a, e in osocp._blocks(dims)]])
    return df, dm


def feasibility_figure(G, h, dims, y, slack=None):
    """max over cones of the violation (beyond `slack`, per cone) / max(1, |h|); 0 when feasible."""
    viol = -cone_margins(h - G @ y, dims)
    if slack is not None:
        viol = viol - slack
    return max(0.0, float(viol.max())) / max(1.0, np.linalg.norm(h))


def z_in_cone_figure(z, dims):
    """Distance of z from K in units of |z| (0 inside)."""
    return max(0.0, float(-cone_margins(z, dims).min())) / max(np.linalg.norm(z), 1e-300)


def gap_figure(P, q, G, h, z, y, slack=0.0):
    """(f(y) - lb(z) - slack) / max(1, |f(y)|)."""
    f = objective(P, q, y)
    return (f - lower_bound(P, q, G, h, z) - slack) / max(1.0, abs(f))


def figures(prog, z, y, rounded=False):
    """(feasibility figure, objective figure) of y on prog = (P, q, G, h, dims) with the multiplier z.  rounded: y is an
    fp32 rounding of the point under test; both figures are taken beyond what that rounding can change.  P = 0: the bound
    does not exist, the objective figure is None."""
    P, q, G, h, dims = prog
    df, dm = rounding_slack(P, q, G, dims, y) if rounded else (0.0, None)
    return feasibility_figure(G, h, dims, y, dm), (gap_figure(P, q, G, h, z, y, df) if P.any() else None)


# ------------------------------------------------------------------------------------------------ reference solves
def solve(prog, maxiters=osocp.MAXITERS):
    P, q, G, h, dims = prog
    return osocp.coneqp(P, q, G, h, dims, maxiters=maxiters)


def solve_batch(progs):
    """The numpy port on every program: (sols, kept) with kept[i] = it returned 'optimal'."""
    sols = [solve(pr) for pr in progs]
    return sols, np.array([s["status"] == "optimal" for s in sols])


def p0_reference_is_a_solution(prog, sol):
    """The P = 0 programs have no bound to hold the device to, only the port's x: its own KKT residuals must then be at the
    level of its stop tolerances (1e-9 relative; ten times that is asked for)."""
    P, q, G, h, dims = prog
    k = osocp.kkt_residuals(P, q, G, h, dims, sol)
    return (k["stationarity"] <= 1e-8 * max(1.0, np.linalg.norm(q)) and k["primal"] <= 1e-8 * max(1.0, np.linalg.norm(h))
            and k["complementarity"] <= 1e-8 * max(1.0, abs(q @ sol["x"])) and k["s_cone"] == 0.0 and k["z_cone"] == 0.0)


@functools.lru_cache(maxsize=None)
def clf_cbf_case(seed, Bt, m, K, pattern, f32=False):
    """One CLF-CBF case, solved once and shared: (batch, mask, progs, sols, kept).  Treat as read-only."""
    p = clf_cbf_family(seed, Bt, m, K, f32)
    mask = relax_mask(pattern, K)
    progs = [clf_cbf_generic_form(p, mask, i) for i in range(Bt)]
    sols, kept = solve_batch(progs)
    return p, mask, progs, sols, kept


@functools.lru_cache(maxsize=None)
def generic_case(family, seed, Bt, nv, l, qdims):
    """One generic ('generic') or P = 0 ('p0') case, solved once and shared: (batch, progs, sols, kept).  Read-only."""
    p = (generic_family if family == "generic" else p0_family)(seed, Bt, nv, l, list(qdims))
    progs = [instance(p, i) for i in range(Bt)]
    sols, kept = solve_batch(progs)
    return p, progs, sols, kept


def clf_cbf_seed(m, K):
    return 7000 + 10 * m + K


def generic_seed(nv, l, qdims):
    return 9000 + 100 * nv + 10 * l + len(qdims)


# the cases of tests/test_gpu_conic.py (listed here so that the CPU tests can walk them without a GPU)
QUAD_SHAPES = [(m, K) for m in (1, 2, 3) for K in (1, 2, 3, 4)]
WIDE_SHAPES = [(m, K) for K in (5, 8) for m in (1, 2, 3)]
QUAD_BT, WIDE_BT, CONEQP_BT = 67, 33, 65
GENERIC_SHAPES = [(1, 1, ()), (1, 0, (2,)), (2, 3, (3,)), (3, 8, ()), (6, 0, (6, 6, 6, 6)), (6, 8, (2, 6, 5, 3)),
                  (5, 0, (4, 3, 6, 2, 5)), (4, 2, (2,) * 7), (6, 8, (6,) * 8)]
P0_SHAPES = [(3, 0, (3, 3)), (4, 0, (3, 3, 3, 3)), (6, 8, (6, 2))]
MIXED_SHAPE = (3, 2, (3, 4))      # permutation / max_iters / mixed-status tests of the generic solver
