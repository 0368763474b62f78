"""fp64 yardstick of ONE event of the self-triggered loop with the posterior-drawn plant and the held-control audit
(bcbf_unicycle_trigger_step_audit): plain numpy, one instance at a time, built on tests/_trigger_step_reference.py (tau, the clamp
rules, the clock, the planner row) and tests/_posterior_plant_reference.py (the draw, the two sides of the cone).  What the entry
is specified to do, written down without looking at how it does it:

    the audit, where held != 0, before anything else and whatever the status:   ubar_h = (1, u_held), per obstacle row k = 1..Kob
        mean_k = sign_k (grad_k . (fhat + ghat u_held + M_k ubar_h) + cst_k),  std_k = sqrt(max((ubar_h' B_k ubar_h) grad_k' A grad_k, 0)),
        margin_k = mean_k - rho std_k;    audit_n += 1, audit_neg += !(value >= 0), audit_min = min(audit_min, value) (NaN: -inf)
    the event of _trigger_step_reference.event;  with z, a solved instance moves by the draw held for dt_b instead:
        x = x + xdot_s dt_b, cbc_s = sign_k (grad_k . xdot_s + cst_k), solved += 1, viol += (cbc_s_k < 0 or non-finite), min_cbc
    an unsolved instance keeps its state, xdot_s = 0, cbc_s = 0, no counter moves
    at the end u_held = u, held = (status == 0).

Everything is evaluated in fp64 from the values handed in and every output is rounded to `dtype` once; the counters look at the
rounded values, as the entry's do at what it stores."""
import numpy as np

import _posterior_plant_reference as P
import _trigger_step_reference as S


def new_counters(Kob, dtype=np.float64):
    """The counters of one instance as ops.trigger_audit_workspace starts them."""
    return dict(solved=0, viol=np.zeros(Kob, dtype=np.int64), min_cbc=np.full(Kob, np.inf, dtype=dtype), audit_n=0,
                audit_neg=np.zeros((Kob, 2), dtype=np.int64), audit_min=np.full((Kob, 2), np.inf, dtype=dtype))


def held_audit(u_held, fhat, ghat, Mk, Bk, A, grad, cst, sign, rho, dtype=np.float64):
    """mean[Kob], margin[Kob] in `dtype` and their scales (the sums of the absolute terms) for one instance."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    u_held, fhat, ghat, Mk, Bk, A, grad, cst, sign = map(f, (u_held, fhat, ghat, Mk, Bk, A, grad, cst, sign))
    Kob = len(cst) - 1
    y = np.r_[u_held, 0.0][None]
    mean, margin, sc_mean, sc_margin = (np.zeros(Kob) for _ in range(4))
    ub = np.r_[1.0, u_held]
    sc_m = np.abs(fhat) + np.abs(ghat) @ np.abs(u_held) + np.abs(Mk) @ np.abs(ub)
    for k in range(1, 1 + Kob):
        m, sd = P.row_mean_std(y, Mk[None], Bk[None], A[None], grad[None], cst[None], fhat[None], ghat[None], sign, k)
        mean[k - 1], margin[k - 1] = m[0], m[0] - float(rho) * sd[0]
        sc_mean[k - 1] = np.abs(grad[k]) @ sc_m + abs(cst[k])
        sc_margin[k - 1] = sc_mean[k - 1] + abs(float(rho)) * sd[0]
    return dict(held_mean=mean.astype(dtype), held_margin=margin.astype(dtype), scale_mean=sc_mean, scale_margin=sc_margin)


def count_audit(c, held_mean, held_margin):
    """One audited event into the counters `c` (in place): NaN counts as negative and enters the minimum as -inf."""
    c["audit_n"] += 1
    for j, v in enumerate((np.asarray(held_mean), np.asarray(held_margin))):
        c["audit_neg"][:, j] += ~(v >= 0)
        c["audit_min"][:, j] = np.minimum(c["audit_min"][:, j], np.where(np.isnan(v), -np.inf, v).astype(c["audit_min"].dtype))


def count_risk(c, cbc_s):
    """One solved event on a drawn plant into the counters `c` (in place): rollout_risk_kernel's semantics."""
    v = np.asarray(cbc_s)[1:]
    v = np.where(np.isfinite(v), v, -np.inf).astype(c["min_cbc"].dtype)
    c["solved"] += 1
    c["viol"] += v < 0
    c["min_cbc"] = np.minimum(c["min_cbc"], v)


def event(x, u, status, fhat, ghat, Mk, centers, tw, off, r, ls, sf, Adiag, Bhyp, t, events, plan_all, dplan_all, dt_plan, t_end,
          tau_min, tau_max, L_true, Bk=None, A=None, grad=None, cst=None, sign=None, rho=None, z=None, u_held=None, held=0,
          counters=None, dtype=np.float64, dt_used=None, deltaL=1e-4, zeta=1e-2, L_alpha=1.0, Xtest=None):
    """One instance.  Returns None for a finished instance (nothing changes, the counters included), else the dict of
    _trigger_step_reference.event, with
      z given:       x (in `dtype`), xdot_s[3], cbc_s[1+Kob] and scale_x, scale_xdot, scale_cbc replaced / added: the posterior plant
                     held for dt_b -- the yardstick's own, or `dt_used` (the hold as the device's working type holds it);
      u_held given:  audited (bool), and where audited held_mean, held_margin, scale_mean, scale_margin; u_held_next, held_next;
      counters:      a dict of new_counters, updated in place."""
    ev = S.event(x, u, status, fhat, ghat, Mk, centers, tw, off, r, ls, sf, Adiag, Bhyp, t, events, plan_all, dplan_all, dt_plan, t_end,
                 tau_min, tau_max, L_true, deltaL=deltaL, zeta=zeta, L_alpha=L_alpha, Xtest=Xtest)
    if ev is None:
        return None
    solved = int(status) == 0
    if u_held is not None:
        ev["audited"] = int(held) != 0
        if ev["audited"]:
            ev.update(held_audit(u_held, fhat, ghat, Mk, Bk, A, grad, cst, sign, rho, dtype=dtype))
            if counters is not None:
                count_audit(counters, ev["held_mean"], ev["held_margin"])
        ev["u_held_next"], ev["held_next"] = np.asarray(u, dtype=dtype), int(solved)
    if z is not None:
        dt_b = ev["dt_used"] if dt_used is None else float(dt_used)
        one = lambda a: np.asarray(a, dtype=np.float64)[None]
        st = P.step(one(x), one(np.r_[np.asarray(u, dtype=np.float64), 0.0]), np.array([int(status)]), one(Mk), one(Bk), one(A), one(grad),
                    one(cst), one(fhat), one(ghat), sign, one(z), dt_b, dtype=dtype)
        ev.update(x=st["x_next"][0], xdot_s=st["xdot_s"][0], cbc_s=st["cbc_s"][0], scale_x=st["scale_x"][0],
                  scale_xdot=st["scale_xdot"][0], scale_cbc=st["scale_cbc"][0])
        if solved and counters is not None:
            count_risk(counters, ev["cbc_s"])
    return ev
