"""Yardstick of group O of bcbf_unicycle_trigger_step_observe -- the event of the self-triggered loop written as an observation row
for the learner -- in plain numpy, one instance at a time, built on tests/_trigger_step_reference.py (tau, the clamp rules, the
plant, the clock).  What the entry is specified to do, written down without looking at how it does it:

    e = events before the event;  if e % obs_every == 0 and k = obs_row0 + e // obs_every < obs_ld: row k of the instance's stream
        obs_x  = the state before the step, (0, 0, theta) when shift invariant
        obs_uh = (1, u)                                  an unsolved instance: (1, 0, 0) -- it kept its state
        obs_y  = (x_new - x_old) / dt_b - g(theta; L_mean) u,   g = [[cos th, 0], [sin th, 0], [0, 1 / L_mean]]
    xq_next = x_new, (0, 0, theta_new) when shift invariant, at every event of a live instance

evaluated IN THE WORKING TYPE from the values handed in (the stored states, the stored hold), one rounding per operation, as
unicycle_observe (csrc/unicycle_task.h) does.  L_mean crosses the C ABI as a float in both precisions."""
import math

import numpy as np

import _trigger_step_reference as S


def row_index(e, obs_every, obs_row0, obs_ld):
    """The stream row event number e (the count BEFORE the event) is written to, or None: not an observed event, or past the stream."""
    if e < 0 or e % obs_every:
        return None
    k = obs_row0 + e // obs_every
    return k if k < obs_ld else None


def observation(x_old, x_new, u, solved, dt_b, L_mean, shift_invariant=True, dtype=np.float64):
    """dict(obs_x[3], obs_uh[3], obs_y[3], xq_next[3], bound[3]) in `dtype`.  bound: 8 eps (|dx_d / dt_b| + |u_0| + |u_1| / L_mean) --
    the difference and the division are single exact-rounded operations on stored values, so only sin / cos (a few ulp in a device
    library) and the contraction of g u can differ between two evaluations in the working type."""
    T = dtype
    xo, xn = np.asarray(x_old, dtype=T), np.asarray(x_new, dtype=T)
    uu = np.asarray(u, dtype=T) if solved else np.zeros(2, dtype=T)
    dt, L = T(dt_b), T(np.float32(L_mean))
    th = xo[2]
    G = np.array([[np.cos(th), T(0)], [np.sin(th), T(0)], [T(0), T(1) / L]], dtype=T)
    y = np.empty(3, dtype=T)
    for d in range(3):
        y[d] = T(T(xn[d] - xo[d]) / dt) - T(T(G[d, 0] * uu[0]) + T(G[d, 1] * uu[1]))
    z = T(0)
    obs_x = np.array([z, z, th] if shift_invariant else xo, dtype=T)
    xq = np.array([z, z, xn[2]] if shift_invariant else xn, dtype=T)
    eps = float(np.finfo(T).eps)
    dx = np.abs((xn.astype(np.float64) - xo.astype(np.float64)) / float(dt))
    bound = 8 * eps * (dx + abs(float(uu[0])) + abs(float(uu[1])) / abs(float(L)))
    return dict(obs_x=obs_x, obs_uh=np.array([T(1), uu[0], uu[1]], dtype=T), obs_y=y, xq_next=xq, bound=bound)


def event(x, u, status, fhat, ghat, Mk, centers, tw, off, r, ls, sf, Adiag, Bhyp, t, events, plan_all, dplan_all, dt_plan, t_end,
          tau_min, tau_max, L_true, L_mean=1.0, obs_every=1, obs_row0=0, obs_ld=1, shift_invariant=True, dtype=np.float64, **kw):
    """_trigger_step_reference.event (same arguments) with group O: returns None for a finished instance, else that dict with
    obs_row (the stream row, or None) and obs_x, obs_uh, obs_y, xq_next, bound of `observation` on the yardstick's own new state
    and hold."""
    ev = S.event(x, u, status, fhat, ghat, Mk, centers, tw, off, r, ls, sf, Adiag, Bhyp, t, events, plan_all, dplan_all, dt_plan, t_end,
                 tau_min, tau_max, L_true, **kw)
    if ev is None:
        return None
    ev["obs_row"] = row_index(int(events), obs_every, obs_row0, obs_ld)      # (`events`: the count before the event)
    ev.update(observation(x, ev["x"], u, int(status) == 0, ev["dt_used"], L_mean, shift_invariant, dtype))
    return ev


def rest_row(dtype=np.float64):
    """The row ops.trigger_observe_workspace starts every stream row with: the plant at rest."""
    return dict(obs_x=np.zeros(3, dtype=dtype), obs_uh=np.array([1, 0, 0], dtype=dtype), obs_y=np.zeros(3, dtype=dtype))


def hand_event():
    """An event small enough to do by hand, every number a dyadic rational: theta = 0, so g = [[1, 0], [0, 0], [0, 1/4]] at
    L_mean = 4; u = (2, 1/2) held for dt_b = 1/4 on the true plant with L_true = 1 moves (1, 2, 0) to (1.5, 2, 0.125);
    the finite difference is (2, 0, 0.5), the prior mean's velocity (2, 0, 0.125): the residual the learner sees is (0, 0, 0.375)."""
    return dict(x_old=[1.0, 2.0, 0.0], x_new=[1.5, 2.0, 0.125], u=[2.0, 0.5], dt_b=0.25, L_mean=4.0,
                obs_x=[0.0, 0.0, 0.0], obs_x_raw=[1.0, 2.0, 0.0], obs_uh=[1.0, 2.0, 0.5], obs_y=[0.0, 0.0, 0.375], xq_next=[0.0, 0.0, 0.125],
                xq_next_raw=[1.5, 2.0, 0.125], cos=math.cos(0.0))
