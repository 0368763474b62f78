"""The CPU yardstick of the unicycle CLF-CBF quadratic program on the mean model (bcbf_clf_cbf_qp2,
bcbf_unicycle_clf_cbf_{control,rollout}): numpy, fp64, no code shared with the device.

  * `rows`: the program's rows.  Cartesian kind: oracle.control_step.constraint_rows (CLFCartesian, ObstacleCBF) times
    oracle.unicycle.ackermann_g; polar kind: CLFPolar on PolarDynamics through oracle.unicycle.cartesian2polar.  Both are held
    to recorded values of the reference's own classes (tests/golden/unicycle_clf_qp_rows.npz).
  * `solve_qp2`: the enumeration rule of the program (projection of p = -(w/2) a_c onto {box} n {hard rows}; candidates p, the
    feet, the pairwise intersections; admissible = every other row >= -tol; nearest wins, ties to the first), with a *decision
    margin* per program: how far the program is from one where rounding could change `status` or `active`.
  * `plan`, `plant_step`, `control`, `rollout`: planner, plant and the closed loop in sample_generator_trajectory's order.
The reference solves the program with GUROBI through cvxpy, neither available where these tests are built: parity with its
iterates is not claimed.  The enumerator is held to oracle.socp.coneqp and to scipy's SLSQP (tests/test_unicycle_qp_cpu.py)."""
import math

import numpy as np

from oracle import control_step as ocs
from oracle import unicycle as ouni

EPS = {np.dtype(np.float64): np.finfo(np.float64).eps, np.dtype(np.float32): float(np.finfo(np.float32).eps)}
LO, HI = np.array([-10.0, -5 * math.pi]), np.array([10.0, 5 * math.pi])
START, GOAL = np.array([-3.0, -1.0, -math.pi / 4]), np.array([0.0, 0.0, math.pi / 4])
TASK = dict(Kp=(0.9, 1.5, 4.0, 0.0), clf_kind=0, clf_gamma=10.0, relax_weight=10.0, lo=LO, hi=HI, tw=(0.5, 0.5), gammas=())
KP_POLAR = (0.6, 1.5, 4.0, 0.0)
KP_TRACK = (0.9, 1.5, 0.0, 0.0)


def task(**over):
    t = dict(TASK)
    t.update(over)
    return t


def mid_obstacles(start=START, goal=GOAL):
    """(centers[2,2], radii[2]) of obstacles_at_mid_from_start_and_goal."""
    obs = ouni.obstacles_at_mid_from_start_and_goal(start, goal)
    return np.array([o.center for o in obs]), np.array([o.radius for o in obs])


def polar_terms(x, goal, Kp):
    """(polar[3], V, gradV[3], g[3,2]) of CLFPolar / PolarDynamics at one state (unicycle_move_to_pose.py:143-167, 442-497)."""
    rho, al, be = ouni.cartesian2polar(x, goal)
    V = 0.5 * Kp[0] * rho ** 2 + Kp[1] * (1 - math.cos(al)) + Kp[2] * (1 - math.cos(be)) + Kp[3] * (1 - math.cos(be - al))
    gV = np.array([Kp[0] * rho, Kp[1] * math.sin(al) - Kp[3] * math.sin(be - al), Kp[2] * math.sin(be) + Kp[3] * math.sin(be - al)])
    with np.errstate(all="ignore"):
        s = -np.sin(al) / np.float64(rho)
    g = np.array([[-math.cos(al), 0.0], [s, 1.0], [s, 0.0]])
    return np.array([rho, al, be]), V, gV, g


def rows(x, plan, dot_plan, L=1.0, centers=None, radii=None, t=TASK):
    """x[B,3], plan[B,3], dot_plan[B,3], L scalar or [B], centers[Kob,2] / [B,Kob,2], radii[Kob] / [B,Kob]
    -> a[B,1+Kob,2], b[B,1+Kob], values[B,1+Kob] = (V, h_k); row 0 the CLF."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    B = x.shape[0]
    plan = np.broadcast_to(np.asarray(plan, dtype=np.float64), (B, 3))
    dot_plan = np.broadcast_to(np.asarray(dot_plan, dtype=np.float64), (B, 3))
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (B,))
    Kob = 0 if centers is None else np.asarray(radii).shape[-1]
    if Kob:
        centers = np.broadcast_to(np.asarray(centers, dtype=np.float64), (B, Kob, 2))
        radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (B, Kob))
    a, b, v = np.zeros((B, 1 + Kob, 2)), np.zeros((B, 1 + Kob)), np.zeros((B, 1 + Kob))
    Kp = t["Kp"]
    with np.errstate(all="ignore"):
        for i in range(B):
            if t["clf_kind"] == 1:
                assert Kob == 0
                polar, V, gV, g = polar_terms(x[i], plan[i], Kp)
                if not polar[0] > 1e-6:                     # the reference asserts: the program is refused
                    a[i, 0], b[i, 0], v[i, 0] = np.nan, np.nan, V
                    continue
                a[i, 0], b[i, 0], v[i, 0] = gV @ g, t["clf_gamma"] * V, V
            else:
                cen = centers[i] if Kob else np.zeros((0, 2))
                rad = radii[i] if Kob else np.zeros(0)
                grad, const, _ = ocs.constraint_rows(x[i], plan[i], dot_plan[i], Kp[:3], t["clf_gamma"], cen, rad, t["tw"],
                                                     t["gammas"])
                a[i] = grad @ ouni.ackermann_g(x[i], L[i])
                b[i] = const
                v[i, 0] = ouni.CLFCartesian(Kp[:3]).clf(x[i], plan[i])
                for k in range(Kob):
                    v[i, 1 + k] = ouni.ObstacleCBF(cen[k], rad[k], tuple(t["tw"])).cbf(x[i])
    return a, b, v


def half_planes(a, b, lo, hi):
    """The M = 4 + Kob rows A_i.u + B_i >= 0 in the order lo0, lo1, hi0, hi1, hard rows."""
    B, K = b.shape
    A, Bv = np.zeros((B, 3 + K, 2)), np.zeros((B, 3 + K))
    A[:, 0, 0] = A[:, 1, 1] = 1.0
    A[:, 2, 0] = A[:, 3, 1] = -1.0
    Bv[:, 0], Bv[:, 1], Bv[:, 2], Bv[:, 3] = -lo[0], -lo[1], hi[0], hi[1]
    A[:, 4:], Bv[:, 4:] = a[:, 1:], b[:, 1:]
    return A, Bv


def solve_qp2(a, b, lo=LO, hi=HI, w=10.0, eps=EPS[np.dtype(np.float64)]):
    """The rule, for a batch: a[B,K,2], b[B,K].  Returns dict(u[B,2], relax[B], active[B], status[B], margin[B]); u, relax are
    NaN and active -1 where status is 1.  `eps`: the machine epsilon of the arithmetic under test (the rule's tolerance
    is stated in it).  margin: the smaller of
      - the relative gap between the best and the second-best admissible candidate's distance to p, and
      - the smallest |a_i.u + b_i + tol_i| / (|a_i0 u0| + |a_i1 u1| + |b_i|) among the admissibility tests that decided: every
        test of the winner, and, of each inadmissible candidate that is nearer than the winner (all of them when there is no
        winner), its most clearly failing test."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, K = b.shape
    M = 3 + K
    A, Bv = half_planes(a, b, np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    p = -(w / 2) * a[:, 0]
    cands = [(p[:, 0], p[:, 1], np.ones(B, dtype=bool), ())]
    with np.errstate(all="ignore"):
        for i in range(M):
            n2 = A[:, i, 0] ** 2 + A[:, i, 1] ** 2
            tt = (A[:, i, 0] * p[:, 0] + A[:, i, 1] * p[:, 1] + Bv[:, i]) / n2
            cands.append((p[:, 0] - A[:, i, 0] * tt, p[:, 1] - A[:, i, 1] * tt, ~((A[:, i, 0] == 0) & (A[:, i, 1] == 0)), (i,)))
        for i in range(M):
            for j in range(i + 1, M):
                det = A[:, i, 0] * A[:, j, 1] - A[:, i, 1] * A[:, j, 0]
                c0 = (Bv[:, j] * A[:, i, 1] - Bv[:, i] * A[:, j, 1]) / det
                c1 = (Bv[:, i] * A[:, j, 0] - Bv[:, j] * A[:, i, 0]) / det
                cands.append((c0, c1, det != 0, (i, j)))
        nc = len(cands)
        D, OK = np.full((B, nc), np.inf), np.zeros((B, nc), dtype=bool)
        PASSMIN, FAILMAX = np.full((B, nc), np.inf), np.full((B, nc), np.inf)
        U = np.zeros((B, nc, 2))
        for c, (c0, c1, valid, act) in enumerate(cands):
            t0, t1 = A[:, :, 0] * c0[:, None], A[:, :, 1] * c1[:, None]
            s = t0 + t1 + Bv
            scale = np.abs(t0) + np.abs(t1) + np.abs(Bv)
            tol = 64 * eps * scale
            passes = s >= -tol
            m = np.where(scale > 0, np.abs(s + tol) / scale, np.where(s + tol == 0, 0.0, np.inf))
            m = np.where(np.isnan(m), 0.0, m)
            others = np.ones(M, dtype=bool)
            others[list(act)] = False
            ok = valid & passes[:, others].all(1)
            d = (c0 - p[:, 0]) ** 2 + (c1 - p[:, 1]) ** 2
            ok &= d < np.inf                                         # a candidate at infinity is never the nearest
            D[:, c] = np.where(ok, d, np.inf)
            OK[:, c] = ok
            U[:, c, 0], U[:, c, 1] = c0, c1
            PASSMIN[:, c] = np.where(passes[:, others], m[:, others], np.inf).min(1) if others.any() else np.inf
            fail = np.where(~passes[:, others], m[:, others], -np.inf).max(1) if others.any() else np.full(B, -np.inf)
            # an invalid candidate is out by an exact test (zero normal / zero determinant): no margin of its own
            FAILMAX[:, c] = np.where(valid & ~ok, np.where(np.isfinite(d), fail, np.inf), np.inf)
            D[:, c] = np.where(ok, d, np.inf)
        win = D.argmin(1)                                              # (argmin: the first among equals)
        found = OK.any(1)
        rowsfinite = np.isfinite(a).all((1, 2)) & np.isfinite(b).all(1)
        idx = np.arange(B)
        u = U[idx, win]
        relax = (a[:, 0] * u).sum(1) + b[:, 0]
        status = (~(found & rowsfinite & np.isfinite(u).all(1) & np.isfinite(relax))).astype(np.int32)
        active = np.array([sum(1 << i for i in cands[c][3]) for c in win], dtype=np.int32)
        dbest = np.sqrt(D[idx, win])
        D2 = D.copy()
        D2[idx, win] = np.inf
        d2 = np.sqrt(D2.min(1))
        gap = np.where(np.isfinite(d2), np.where(d2 > 0, (d2 - dbest) / d2, 0.0), np.inf)
        # inadmissible candidates that would have won
        Dall = np.stack([(c0 - p[:, 0]) ** 2 + (c1 - p[:, 1]) ** 2 for c0, c1, _, _ in cands], 1)
        nearer = ~OK & ~(np.sqrt(Dall) > (dbest * (1 + 1e-6))[:, None])
        nearer |= ~OK & ~found[:, None]
        margin = np.minimum(gap, PASSMIN[idx, win])
        margin = np.where(found, margin, np.inf)
        margin = np.minimum(margin, np.where(nearer, FAILMAX, np.inf).min(1))
        margin = np.where(rowsfinite, margin, np.inf)
    bad = status != 0
    u, relax, active = np.where(bad[:, None], np.nan, u), np.where(bad, np.nan, relax), np.where(bad, -1, active)
    return dict(u=u, relax=relax, active=active, status=status, margin=margin)


def coneqp_form(a, b, lo=LO, hi=HI, w=10.0):
    """One program (a[K,2], b[K]) as oracle.socp.coneqp's (P, q, G, h, dims): y = (u0, u1, relax), G y <= h.  Each hard row
    is divided by its largest entry -- the same half-plane; the interior-point method runs into its iteration limit on rows
    of very different scales."""
    K = b.shape[0]
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    s = np.maximum(np.abs(a[1:]).max(1), np.abs(b[1:]))
    s = np.where(s > 0, s, 1.0)
    a[1:], b[1:] = a[1:] / s[:, None], b[1:] / s
    P = np.diag([2.0, 2.0, 0.0])
    q = np.array([0.0, 0.0, w])
    G, h = np.zeros((4 + K, 3)), np.zeros(4 + K)
    G[0, 0] = G[1, 1] = -1.0
    G[2, 0] = G[3, 1] = 1.0
    h[:4] = [-lo[0], -lo[1], hi[0], hi[1]]
    G[4, :2], G[4, 2], h[4] = a[0], -1.0, -b[0]
    G[5:, :2], h[5:] = -a[1:], b[1:]
    return P, q, G, h, dict(l=4 + K, q=[])


def planner_steps(numStepsPlan, frac=0.7):
    return min(int(numStepsPlan * frac), numStepsPlan - 1), max(int(0.1 * numStepsPlan), 1)


def plan(kind, x0, goal, t, numStepsPlan=0, dt=0.05, frac=0.7):
    """(plan[B,3], dot_plan[B,3]) at step t: kind 0 NoPlanner, kind 1 oracle.unicycle.PiecewiseLinearPlanner per instance."""
    goal = np.atleast_2d(goal)
    if kind == 0:
        return goal.copy(), np.zeros_like(goal)
    pl, dp = np.zeros_like(goal), np.zeros_like(goal)
    x0 = np.broadcast_to(np.asarray(x0, dtype=np.float64), goal.shape)
    with np.errstate(all="ignore"):
        if (x0 == x0[0]).all() and (goal == goal[0]).all():          # one plan for every instance
            P = ouni.PiecewiseLinearPlanner(x0[0], goal[0], numStepsPlan, dt, frac)
            pl[:], dp[:] = P.plan(t), P.dot_plan(t)
            return pl, dp
        for i in range(goal.shape[0]):
            P = ouni.PiecewiseLinearPlanner(x0[i], goal[i], numStepsPlan, dt, frac)
            pl[i], dp[i] = P.plan(t), P.dot_plan(t)
    return pl, dp


def plant_step(x, u, L, dt):
    """AckermannDrive.step: explicit Euler, no angle wrap."""
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (x.shape[0],))
    return np.stack([x[:, 0] + np.cos(x[:, 2]) * u[:, 0] * dt, x[:, 1] + np.sin(x[:, 2]) * u[:, 0] * dt,
                     x[:, 2] + u[:, 1] / L * dt], axis=1)


def control(x, pl, dp, L=1.0, centers=None, radii=None, t=TASK, eps=EPS[np.dtype(np.float64)]):
    """dict(a, b, values, u, relax, active, status, margin) of one control evaluation."""
    a, b, v = rows(x, pl, dp, L, centers, radii, t)
    out = solve_qp2(a, b, t["lo"], t["hi"], t["relax_weight"], eps)
    out.update(a=a, b=b, values=v)
    return out


def rollout(x0, goal, numSteps, dt=0.05, L_ctrl=1.0, L_true=None, centers=None, radii=None, t=TASK, planner=0, x0_plan=None,
            numStepsPlan=0, frac=0.7, stop_rho=0.0, record_every=0):
    """The closed loop of bcbf_unicycle_clf_cbf_rollout from min_h = inf, cost = 0, status = 0, converged_at = -1.
    Returns dict(x, min_h, cost, status, converged_at, rho_at (the distance to the goal at the step an instance stopped),
    traj[nrec,B,3], u[nrec,B,2], actives (set of active masks met))."""
    x = np.array(np.atleast_2d(x0), dtype=np.float64)
    B = x.shape[0]
    goal = np.broadcast_to(np.asarray(goal, dtype=np.float64), (B, 3))
    L_true = L_ctrl if L_true is None else L_true
    min_h, cost = np.full(B, np.inf), np.zeros(B)
    status, conv, rho_at = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32), np.full(B, np.nan)
    traj, us, actives = [], [], set()
    for s in range(numSteps):
        live = (status == 0) & (conv < 0)
        rho = np.hypot(goal[:, 0] - x[:, 0], goal[:, 1] - x[:, 1])
        stop = live & (rho < stop_rho)
        conv[stop], rho_at[stop] = s, rho[stop]
        live &= ~stop
        pl, dp = plan(planner, x0_plan, goal, s, numStepsPlan, dt, frac)
        c = control(x, pl, dp, L_ctrl, centers, radii, t)
        failed = live & (c["status"] != 0)
        status[failed] = s + 1
        go = live & ~failed
        u = np.where(go[:, None], c["u"], 0.0)
        actives |= set(c["active"][go].tolist())
        if record_every and s % record_every == 0:
            traj.append(x.copy())
            us.append(u.copy())
        if c["values"].shape[1] > 1:
            h = c["values"][:, 1:]
            h = np.where(np.isfinite(h), h, -np.inf).min(1)
            min_h = np.where(go, np.minimum(min_h, h), min_h)
        cost = np.where(go, cost + (u ** 2).sum(1), cost)
        x = np.where(go[:, None], plant_step(x, u, L_true, dt), x)
    return dict(x=x, min_h=min_h, cost=cost, status=status, converged_at=conv, rho_at=rho_at,
                traj=np.array(traj).reshape(-1, B, 3), u=np.array(us).reshape(-1, B, 2), actives=actives)


def starts(Bt, noise=(0.3, 0.3, 0.5), seed=0, start=START):
    """The perturbed starts of the GPU tests (numpy's default_rng, so that host and device runs share them exactly)."""
    return start + np.asarray(noise) * np.random.default_rng(seed).standard_normal((Bt, 3))


def random_programs(n, seed=0):
    """n seeded programs with K in 1..4 at mixed scales: list of (a[K,2], b[K])."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        K = 1 + i % 4
        sa, sb = 10.0 ** rng.uniform(-2, 2), 10.0 ** rng.uniform(-2, 2)
        out.append((sa * rng.standard_normal((K, 2)), sb * rng.standard_normal(K)))
    return out


def hand_programs():
    """Hand-made programs (a[K,2], b[K], what)."""
    z = [0.0, 0.0]
    return [(np.array([z]), np.array([1.0]), "a_c = 0: u = 0"),
            (np.array([[1.0, 2.0], z]), np.array([0.5, 2.0]), "zero-normal hard row, b > 0: ignored"),
            (np.array([[1.0, 2.0], z]), np.array([0.5, -2.0]), "zero-normal hard row, b < 0: infeasible"),
            (np.array([[1.0, 0.0], [1.0, 0.0], [2.0, 0.0]]), np.array([0.0, 1.0, 4.0]), "parallel rows: u0 >= -1 and u0 >= -2"),
            (np.array([[1.0, 0.0], [1.0, 0.0], [-1.0, 0.0]]), np.array([0.0, -3.0, 2.0]), "parallel rows, empty strip"),
            (np.array([[-100.0, -100.0]]), np.array([0.0]), "box corner (hi0, hi1)"),
            (np.array([[100.0, -100.0], [1.0, 1.0]]), np.array([3.0, 40.0]), "box corner (lo0, hi1) with a slack hard row"),
            (np.array([[0.3, -0.2], [1.0, 1.0], [1.0, -1.0], [-1.0, 0.5]]), np.array([1.0, -1.0, -1.0, 4.0]), "vertex of two hard rows")]


def pack(programs, K):
    """The programs with K rows as arrays a[n,K,2], b[n,K]."""
    sel = [(a, b) for a, b, *_ in programs if b.shape[0] == K]
    return np.array([a for a, _ in sel]).reshape(-1, K, 2), np.array([b for _, b in sel]).reshape(-1, K)
