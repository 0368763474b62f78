"""The numpy yardstick of the obstacle-field working set (bayesian_cbf_amd/csrc/obstacle_field.hip): the select rule, the audit
rule, and the whole select / solve / audit / swap loop on top of oracle.control_step, each with the MARGIN of its decisions so a
test can leave out the ones that rounding may legitimately flip:
    select     the gap between the S-th and the (S+1)-th smallest h
    violator   the distance of every unselected margin_k from its threshold -tol_f scale_k
    eviction   the gap between the best and the second-best slot, and the best slot's distance from the full-set threshold
all relative to max(1, |the values compared|).  Test infrastructure only."""
import math

import numpy as np

from oracle import cbc as ocbc
from oracle import control_step as ostep
from oracle import unicycle as ouni

TOL_F, TOL_A = 1e-7, 1e-6
CERTIFIED, FULL, UNSOLVED, UNCERTIFIED = 1, 2, 3, 6
START, GOAL = np.array([-3.0, -1.0, -math.pi / 4]), np.array([0.0, 0.0, math.pi / 4])
EPS_G, EPS_F = 1.1e-8, 7e-9                       # the project's objective / feasibility bounds (tests/test_gpu_conic.py)


def random_obstacle_field(Kf, start=START, goal=GOAL, seed=0, box=((-3.5, 0.5), (-2.0, 1.0)), radius=(0.1, 0.35),
                          clear_start=0.5, clear_goal=0.4):
    """Kf discs: centres uniform in the box, radii uniform in `radius`; a disc is rejected when its centre is closer than
    radius + clear_start to the start or radius + clear_goal to the goal.  (centers[Kf,2], radii[Kf])"""
    rng = np.random.RandomState(seed)
    cen, rad = [], []
    while len(rad) < Kf:
        c = np.array([rng.uniform(*box[0]), rng.uniform(*box[1])])
        r = rng.uniform(*radius)
        if np.linalg.norm(c - np.asarray(start)[:2]) < r + clear_start or np.linalg.norm(c - np.asarray(goal)[:2]) < r + clear_goal:
            continue
        cen.append(c)
        rad.append(r)
    return np.array(cen), np.array(rad)


def rows(x, centers, radii, tw):
    """(grad h[K,3], h[K]) of ObstacleCBF for every disc (oracle.unicycle.ObstacleCBF, vectorised)."""
    with np.errstate(all="ignore"):
        gh = np.asarray(x, dtype=np.float64)[:2] - np.asarray(centers, dtype=np.float64)
        th = float(x[2])
        r2 = (gh ** 2).sum(1)
        rn = np.sqrt(r2)
        h = tw[0] * (r2 - np.asarray(radii, dtype=np.float64) ** 2) + tw[1] * (math.cos(th) * gh[:, 0] / rn + math.sin(th) * gh[:, 1] / rn)
        al = np.arctan2(gh[:, 1], gh[:, 0])
        g = np.stack([tw[0] * 2 * gh[:, 0] + tw[1] * np.sin(al - th) * gh[:, 1] / r2,
                      tw[0] * 2 * gh[:, 1] - tw[1] * np.sin(al - th) * gh[:, 0] / r2,
                      -tw[1] * np.sin(th - al)], axis=1)
    return g, h


def _lowest(v):
    v = np.array(v, dtype=np.float64)
    v[np.isnan(v)] = -np.inf
    return v


def _rel_gap(a, b):
    if not (np.isfinite(a) and np.isfinite(b)):
        return 0.0 if a == b else np.inf
    return abs(a - b) / max(1.0, abs(a), abs(b))


def select(x, centers, radii, tw, S):
    """dict(idx[S], margin, min_h): the S smallest h (ties to the lower index, NaN lowest)."""
    _, h = rows(x, centers, radii, tw)
    key = _lowest(h)
    order = np.lexsort((np.arange(len(key)), key))
    margin = np.inf if len(key) == S else _rel_gap(key[order[S - 1]], key[order[S]])
    hm = np.where(np.isfinite(h), h, -np.inf)
    # a tie between two copies of one disc is exact on any machine (the same inputs through the same arithmetic): the index rule
    # decides it, and a test may hold the device to it although the margin is zero
    a, b = (order[S - 1], order[S]) if len(key) > S else (0, 0)
    exact_tie = bool(len(key) > S and np.array_equal(np.asarray(centers)[a], np.asarray(centers)[b])
                     and np.asarray(radii)[a] == np.asarray(radii)[b])
    return dict(idx=order[:S].astype(np.int32), margin=margin, min_h=hm.min(), h=h, exact_tie=exact_tie)


def margins(x, u, Mk, Bk, A, fhat, ghat, rho, centers, radii, tw, gamma):
    """(margin_k [NaN -> -inf], E_k, rho s_k, scale_k) of every disc's cone at the control u."""
    g, h = rows(x, centers, radii, tw)
    ub = np.array([1.0, u[0], u[1]])
    with np.errstate(all="ignore"):
        xd = np.asarray(fhat) + np.asarray(ghat) @ ub[1:] + np.asarray(Mk) @ ub
        E = g @ xd + gamma * h
        q = (ub @ np.asarray(Bk) @ ub) * np.einsum("ki,ij,kj->k", g, np.asarray(A), g)
        rs = rho * np.sqrt(np.where(q > 0, q, 0.0))
        scale = np.ones_like(E)
        scale = np.where(np.abs(E) > scale, np.abs(E), scale)
        scale = np.where(rs > scale, rs, scale)
        m = _lowest(E - rs)
    return m, E, rs, scale


def margin_magnitude(x, u, Mk, Bk, A, fhat, ghat, rho, centers, radii, tw, gamma):
    """The magnitudes summed in margin_k, sum_i |grad_i| |xdot_i| + gamma (tw0 (|p - c|^2 + r^2) + tw1) + rho s_k + 1 with the
    gradient's terms taken in absolute value too: what a rounding-error bound on margin_k is relative to."""
    ub = np.array([1.0, u[0], u[1]])
    with np.errstate(all="ignore"):
        gh = np.asarray(x, dtype=np.float64)[:2] - np.asarray(centers, dtype=np.float64)
        r2 = (gh ** 2).sum(1)
        gabs = np.stack([tw[0] * 2 * np.abs(gh[:, 0]) + tw[1] * np.abs(gh[:, 1]) / r2,
                         tw[0] * 2 * np.abs(gh[:, 1]) + tw[1] * np.abs(gh[:, 0]) / r2, np.full(len(r2), tw[1])], axis=1)
        xd = np.abs(np.asarray(fhat)) + np.abs(np.asarray(ghat)) @ np.abs(ub[1:]) + np.abs(np.asarray(Mk)) @ np.abs(ub)
        q = (ub @ np.asarray(Bk) @ ub) * np.einsum("ki,ij,kj->k", gabs, np.abs(np.asarray(A)), gabs)
        return gabs @ xd + abs(gamma) * (tw[0] * (r2 + np.asarray(radii, dtype=np.float64) ** 2) + tw[1]) \
            + rho * np.sqrt(np.where(q > 0, q, 0.0)) + 1.0


def audit(cert, status, idx, m, scale, tol_f=TOL_F, tol_a=TOL_A):
    """The rule on the margins of `margins`.  Returns dict(cert, idx (new), swapped (slot or -1), violator (or -1), rounds_inc,
    worst_margin, worst_idx, nviol, decision): `decision` is the smallest relative margin of the decisions taken."""
    idx = np.array(idx, dtype=np.int32)
    out = dict(cert=cert, idx=idx, swapped=-1, violator=-1, rounds_inc=0, worst_margin=None, worst_idx=None, nviol=None,
               decision=np.inf)
    if cert != 0:
        return out
    if status != 0:
        return dict(out, cert=UNSOLVED, worst_margin=np.nan, worst_idx=-1, nviol=0)
    K = len(m)
    un = np.array([k for k in range(K) if k not in set(idx.tolist())], dtype=int)
    decision = np.inf
    if len(un):
        o = un[np.lexsort((un, m[un]))]
        out.update(worst_margin=m[o[0]], worst_idx=int(o[0]))
        thr = -tol_f * scale[un]
        with np.errstate(invalid="ignore"):
            d = np.abs(m[un] - thr) / scale[un]
        decision = min(decision, float(np.nanmin(np.where(np.isfinite(m[un]), d, np.inf))))
        viol = un[m[un] < thr]
    else:
        out.update(worst_margin=np.inf, worst_idx=-1)
        viol = un
    out["nviol"] = len(viol)
    if len(viol) == 0:
        return dict(out, cert=CERTIFIED, decision=decision)
    sm, sc = m[idx], scale[idx]
    best = int(np.lexsort((np.arange(len(idx)), -sm))[0])
    decision = min(decision, abs(sm[best] - tol_a * sc[best]) / sc[best] if np.isfinite(sm[best]) else np.inf)
    if sm[best] <= tol_a * sc[best]:
        return dict(out, cert=FULL, decision=decision)
    if len(idx) > 1:
        second = np.sort(sm)[-2]
        decision = min(decision, _rel_gap(sm[best], second))
    vo = viol[np.lexsort((viol, m[viol]))]
    if len(vo) > 1:
        decision = min(decision, _rel_gap(m[vo[0]], m[vo[1]]))
    idx = idx.copy()
    idx[best] = vo[0]
    return dict(out, idx=idx, swapped=best, violator=int(vo[0]), rounds_inc=1, decision=decision)


def objective(y, w, r=(0.0, 0.0)):
    y = np.asarray(y, dtype=np.float64)
    rr = np.array([r[0], r[1], 0.0])
    return float((np.asarray(w) * (y - rr) ** 2).sum())


def task_constants(max_risk=0.01):
    """The constants of rollouts.unicycle_task_tensors."""
    return dict(tw=(0.7, 0.3), gamma=5.0, Kp=np.array([0.9, 1.5, 0.0]), w=np.array([0.33, 0.33, 0.33]), r=np.zeros(2),
                rho=ocbc.cbc1_safety_factor(max_risk), clf_gamma=10.0, L_mean=1.0)


def solve_subset(x, plan, dot_plan, Mk, Bk, A, c, centers, radii, idx, maxiters=None):
    kw = {} if maxiters is None else dict(maxiters=maxiters)
    K = len(idx)
    return ostep.control_step(x, plan, dot_plan, Mk, Bk, A, c["Kp"], c["clf_gamma"], centers[idx], radii[idx], c["tw"],
                              [c["gamma"]] * K, c["L_mean"], c["w"], c["r"], c["rho"],
                              relax_mask=np.array([1.0] + [0.0] * K), **kw)


def field_step(x, plan, dot_plan, Mk, Bk, A, c, centers, radii, S=3, rounds=3, tol_f=TOL_F, tol_a=TOL_A):
    """select, then `rounds` times (solve the working set, audit).  dict(y, status, cert, rounds, idx, status_eff, margins)."""
    x = np.asarray(x, dtype=np.float64)
    idx = select(x, centers, radii, c["tw"], S)["idx"]
    cert, nrounds, o, a, m, scale = 0, 0, None, None, None, None
    fhat, ghat = ouni.ackermann_f(x), ouni.ackermann_g(x, c["L_mean"])
    for _ in range(rounds):
        if cert != 0:
            break
        o = solve_subset(x, plan, dot_plan, Mk, Bk, A, c, centers, radii, idx)
        status = 0 if o["status"] == "optimal" else 1
        y = np.concatenate([o["u"], [o["relax"]]])
        if status == 0:
            m, _, _, scale = margins(x, y[:2], Mk, Bk, A, fhat, ghat, c["rho"], centers, radii, c["tw"], c["gamma"])
        a = audit(cert, status, idx, m, scale, tol_f, tol_a)
        cert, idx, nrounds = a["cert"], a["idx"], nrounds + a["rounds_inc"]
    eff = 0 if cert == CERTIFIED else (status if status != 0 else UNCERTIFIED)
    return dict(y=y, status=status, cert=cert, rounds=nrounds, idx=idx, status_eff=eff, margins=m, scale=scale, step=o)


def full_step(x, plan, dot_plan, Mk, Bk, A, c, centers, radii):
    """The program with every disc's cone, through the oracle."""
    return solve_subset(x, plan, dot_plan, Mk, Bk, A, c, centers, radii, np.arange(len(radii)))


def closed_loop(centers, radii, numSteps, planSteps=120, dt=0.05, L_true=12.0, x0=START, goal=GOAL, S=3, rounds=3,
                Mk=None, Bk=None, A=None, full=True):
    """The fixed-kernel loop of the issue on one field.  Per step: dict(x, field_step, full (the oracle's full program))."""
    c = task_constants()
    Mk = np.zeros((3, 3)) if Mk is None else Mk
    Bk = np.eye(3) if Bk is None else Bk
    A = 0.01 * np.eye(3) if A is None else A
    P = ouni.PiecewiseLinearPlanner(x0, goal, planSteps, dt, frac_time_to_reach_goal=0.95)
    x = np.array(x0, dtype=np.float64)
    out = []
    for t in range(numSteps):
        plan, dplan = P.plan(t), P.dot_plan(t)
        fs = field_step(x, plan, dplan, Mk, Bk, A, c, centers, radii, S, rounds)
        fl = full_step(x, plan, dplan, Mk, Bk, A, c, centers, radii) if full else None
        out.append(dict(x=x.copy(), plan=plan, dot_plan=dplan, fs=fs, full=fl))
        if fs["status_eff"] == 0:
            x = ouni.ackermann_step(x, fs["y"][:2], dt, L_true)
    return out, c
