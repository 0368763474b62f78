"""The CPU yardstick of the pendulum CLF-CBF quadratic program (bcbf_pendulum_clf_cbf_{control,rollout}): numpy, fp64.

Two things, neither sharing code with the device function:
  * `solve_qp`: a GENERIC active-set enumerator for  minimise 1/2 z'Pz  subject to  G z <= h  with P positive definite --
    every subset of rows is tried as the active set through its dual (Schur) system; the subset whose point is primal
    feasible with multipliers >= 0 is the optimum, unique because the objective is strictly convex.  It knows nothing about
    the two-row shape of the controller's program.
  * `rows`, `control`, `rollout`: the rows of the reference's EnergyCLF / RadialCBFRelDegree2 / RadialCBF (held to recorded
    values of the reference's own classes, tests/golden/pendulum_clf_cbf_rows.npz) and the closed loop in sampling_pendulum's
    order (pendulum.py:199-226).
The reference solves the program with cvxopt, which is not available where these tests are built: parity with cvxopt's
iterates is not claimed.  The enumerator is held to scipy's SLSQP and to the KKT conditions instead
(tests/test_pendulum_qp_cpu.py), and the unique optimum is what the device is held to."""
import itertools
import math

import numpy as np

TASK = dict(clf_c=1.0, k_alpha=(1.0, 3.0), theta_c=math.pi / 4, delta_c=math.pi / 8, cbf_gamma=1.0, cbf_kind=0,
            slack_weight=100.0)


def task(**over):
    t = dict(TASK)
    t.update(over)
    return t


def rows(x, model, t=TASK):
    """x[B,2], model[B,3] or [3] = (m, g, l)  ->  A[B,2], b[B,2], values[B,2] = (V, h); row 0 the CLF, row 1 the barrier."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    m, g, l = np.broadcast_to(np.asarray(model, dtype=np.float64), (x.shape[0], 3)).T
    th, om = x[:, 0], x[:, 1]
    V = l * om ** 2 / 2 + g * (1 - np.cos(th))
    gradV = np.stack([g * np.sin(th), l * om], axis=1)
    f = np.stack([om, -(g / l) * np.sin(th)], axis=1)
    gx = np.stack([np.zeros_like(th), 1 / (m * l)], axis=1)
    a0 = (gradV * gx).sum(1)
    b0 = -t["clf_c"] * V          # (-gradV . f is g sin(th) om - l om (g/l) sin(th): zero up to its own rounding)
    d = th - t["theta_c"]
    gap = math.cos(t["delta_c"]) - np.cos(d)
    if t["cbf_kind"] == 0:
        k0, k1 = t["k_alpha"]
        h = gap
        lfh = om * np.sin(d)
        grad_lfh = np.stack([om * np.cos(d), np.sin(d)], axis=1)
        a1 = -(grad_lfh * gx).sum(1)
        b1 = (grad_lfh * f).sum(1) + k0 * h + k1 * lfh
    else:
        h = gap * (om ** 2 + 1)
        gradh = np.stack([np.sin(d) * (om ** 2 + 1), 2 * om * gap], axis=1)
        a1 = -(gradh * gx).sum(1)
        b1 = (gradh * f).sum(1) + t["cbf_gamma"] * h
    return np.stack([a0, a1], 1), np.stack([b0, b1], 1), np.stack([V, h], 1)


def solve_qp(P, G, h, tol=1e-9):
    """minimise 1/2 z'Pz s.t. G z <= h for a batch: P[nv,nv] (positive definite), G[B,nc,nv], h[B,nc].
    Returns z[B,nv] (NaN where infeasible), lam[B,nc], status[B] (0 optimal, 1 no active set qualifies = infeasible).
    Active set S: z = -P^-1 G_S' lam_S with (G_S P^-1 G_S') lam_S = -h_S; a singular Schur matrix (dependent rows) is skipped.
    Primal feasibility of the inactive rows is tested exactly, the multipliers' sign to `tol` (a tie between two sets leaves one
    of them with a multiplier of -1 ulp); among the qualifying sets (they all describe the same point) the one with the
    smallest sign violation is returned."""
    G, h = np.asarray(G, dtype=np.float64), np.asarray(h, dtype=np.float64)
    B, nc, nv = G.shape
    Pinv = np.linalg.inv(P)
    best = np.full(B, np.inf)
    z_out, lam_out = np.full((B, nv), np.nan), np.zeros((B, nc))
    for k in range(nc + 1):
        for S in itertools.combinations(range(nc), k):
            S = list(S)
            lam = np.zeros((B, nc))
            ok = np.ones(B, dtype=bool)
            if S:
                GS = G[:, S, :]
                M = GS @ Pinv @ GS.transpose(0, 2, 1)
                ok = np.abs(np.linalg.det(M)) > 0
                M = np.where(ok[:, None, None], M, np.eye(k))
                lam[:, S] = np.linalg.solve(M, -h[:, S, None])[:, :, 0]
            z = -(Pinv @ (G.transpose(0, 2, 1) @ lam[:, :, None]))[:, :, 0]
            if S:                                   # one step of iterative refinement on the active rows (M is ill-conditioned
                res = (GS @ z[:, :, None])[:, :, 0] - h[:, S]          # when two rows are nearly dependent)
                lam[:, S] += np.linalg.solve(M, res[:, :, None])[:, :, 0]
                z = -(Pinv @ (G.transpose(0, 2, 1) @ lam[:, :, None]))[:, :, 0]
            slack = (G @ z[:, :, None])[:, :, 0] - h
            slack[:, S] = 0.0                       # the active rows hold by construction
            with np.errstate(invalid="ignore"):
                feasible = (slack <= 0).all(1)      # exact: a row that cannot be met is never waved through
                viol = (-lam / (1 + np.abs(lam).max(1, keepdims=True))).max(1) if nc else np.zeros(B)
                take = ok & feasible & (viol <= tol) & (viol < best)
            best[take] = viol[take]
            z_out[take], lam_out[take] = z[take], lam[take]
    return z_out, lam_out, (~np.isfinite(best)).astype(np.int32)


def program(A, b, w):
    """The controller's program in solve_qp's form: z = (u, rho), P = diag(1, w), rows a0 u - rho <= b0, a1 u <= b1."""
    B = A.shape[0]
    G = np.zeros((B, 2, 2))
    G[:, 0, 0], G[:, 0, 1], G[:, 1, 0] = A[:, 0], -1.0, A[:, 1]
    return np.diag([1.0, w]), G, b


def control(x, model, t=TASK):
    """dict(A, b, values, u, rho, status) of one control evaluation; u, rho are NaN where status != 0."""
    A, b, values = rows(x, model, t)
    z, _, status = solve_qp(*program(A, b, t["slack_weight"]))
    return dict(A=A, b=b, values=values, u=z[:, 0], rho=z[:, 1], status=status)


def plant_step(x, u, model, dt):
    """x + (f + g u) dt on the plant (m, g, l), theta wrapped with the floored modulo (PendulumDynamicsModel.step)."""
    m, g, l = np.broadcast_to(np.asarray(model, dtype=np.float64), (x.shape[0], 3)).T
    th = x[:, 0] + x[:, 1] * dt
    om = x[:, 1] + (-(g / l) * np.sin(x[:, 0]) + 1 / (m * l) * u) * dt
    return np.stack([np.mod(th + math.pi, 2 * math.pi) - math.pi, om], axis=1)


def rollout(x0, ctrl_model, true_model, numSteps, dt=0.002, t=TASK, record_every=0):
    """The closed loop of bcbf_pendulum_clf_cbf_rollout from min_h = inf, damage = 0, status = 0.  An instance whose program
    is infeasible at step s gets status = s + 1 and keeps the state and statistics it had before that step.
    Returns dict(x, min_h, damage, status, traj[nrec,B,2], u[nrec,B])."""
    x = np.array(np.atleast_2d(x0), dtype=np.float64)
    B = x.shape[0]
    ctrl = np.broadcast_to(np.asarray(ctrl_model, dtype=np.float64), (B, 3))
    true = np.broadcast_to(np.asarray(true_model, dtype=np.float64), (B, 3))
    min_h, damage, status = np.full(B, np.inf), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    traj, us = [], []
    for s in range(numSteps):
        live = status == 0
        c = control(x, ctrl, t)
        failed = live & (c["status"] != 0)
        status[failed] = s + 1
        go = live & ~failed
        u = np.where(go, c["u"], 0.0)
        if record_every and s % record_every == 0:
            traj.append(x.copy())
            us.append(u.copy())
        h = np.where(np.isnan(c["values"][:, 1]), -np.inf, c["values"][:, 1])
        min_h = np.where(go, np.minimum(min_h, h), min_h)
        damage += (go & (0 < x[:, 0]) & (x[:, 0] < math.pi / 4)).astype(np.int32)
        x = np.where(go[:, None], plant_step(x, u, true, dt), x)
    return dict(x=x, min_h=min_h, damage=damage, status=status, traj=np.array(traj).reshape(-1, B, 2),
                u=np.array(us).reshape(-1, B))


def starts(Bt, theta0=5 * math.pi / 12, omega0=-0.01, noise=0.05, seed=0):
    """The perturbed starts of the GPU tests (numpy's default_rng, so that host and device runs share them exactly)."""
    return np.array([theta0, omega0]) + noise * np.random.default_rng(seed).standard_normal((Bt, 2))


def loop_starts(Bt=130):
    """The starts of the closed-loop GPU tests: `starts`, the last ten replaced by states below the unsafe wedge that move up
    towards it (0 < theta < pi/4: the ones the damage counter sees)."""
    x0 = starts(Bt)
    x0[-10:, 0] = np.linspace(0.05, 0.35, 10)
    x0[-10:, 1] = 0.3
    return x0
