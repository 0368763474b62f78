"""The pendulum safety filter composed from the CPU oracle (test infrastructure for bcbf_pendulum_control_step):
oracle.cbc2.posterior_jets -> mean model shift -> oracle.cbc2.cbc2_terms -> oracle.controllers.socp_controller_control,
with the greedy nominal control and the Euler step of the true pendulum.  One instance per call, numpy fp64."""
import math

import numpy as np

from oracle import cbc2 as oc2
from oracle import controllers as oc
from oracle import gp_posterior as ogp


def oracle_state(X, UH, Xdot, Bm, ell, s2, M0, jitter, A, kernel="rbf"):
    """(L, Y, UHB, ...) of one instance: L = chol(K_b + diag(jitter)) with the given data kernel."""
    K = ogp.DATA_KERNELS[kernel](X, X, ell, s2) * (UH @ Bm @ UH.T) + np.diag(jitter)
    return dict(L=np.linalg.cholesky(K), Y=Xdot - UH @ M0, X=X, UHB=UH @ Bm, ell=ell, s2=float(s2), Bm=Bm, M0=M0, A=A,
                kernel=kernel)


def pendulum_fg(x, mass, gravity, length):
    f = np.array([x[1], -(gravity / length) * math.sin(x[0])])
    g = np.array([0.0, 1.0 / (mass * length)])
    J = np.array([[0.0, 1.0], [-(gravity / length) * math.cos(x[0]), 0.0]])
    return f, g, J


def barrier(x, theta_c=math.pi / 4, delta_c=math.pi / 8):
    d = x[0] - theta_c
    return math.cos(delta_c) - math.cos(d), np.array([math.sin(d), 0.0]), np.array([[math.cos(d), 0.0], [0.0, 0.0]])


def greedy(x, fhat, ghat, dt, x_goal=(0.0, 0.0), Q=np.eye(2), R=1.0):
    """controllers.GreedyController.control (lam = 1/2) on the model (fhat, ghat)."""
    G = dt * ghat.reshape(2, 1)
    Qs = 0.5 * R * dt + 0.5 * (G.T @ Q @ G)[0, 0]
    c = 0.5 * (G.T @ Q @ (np.asarray(x_goal) - x - dt * fhat))[0]
    return np.array([c / Qs])


def euler(x, u, mass, gravity, length, dt):
    f, g, _ = pendulum_fg(x, mass, gravity, length)
    xn = x + (f + g * u[0]) * dt
    xn[0] = ((xn[0] + math.pi) % (2 * math.pi)) - math.pi
    return xn


def oracle_step(state, x, dt=0.002, u_ref=None, mean_model=None, true_model=(1.0, 10.0, 1.0), k_alpha=(1.0, 3.0),
                safety_factor=math.sqrt(99.0), ctrl_reg=1.0, relax_weight=100.0, hessian_mode="reference"):
    """One step of one instance.  state: `oracle_state(...)` or None (no-GP mode).  Returns dict(u_ref, terms (bfe, e, V,
    bfv, v), cons (named cones), u, status ('optimal' or the oracle solver's), x_next)."""
    x = np.asarray(x, dtype=np.float64)
    if state is None:
        jets = dict(Mk=np.zeros((2, 2)), dMk=np.zeros((2, 2, 2)), Bk=np.zeros((2, 2)), G10=np.zeros((2, 2, 2)),
                    G11=np.zeros((2, 2, 2, 2)))
        A, Bm, ell, s2, kernel = np.eye(2), np.eye(2), np.ones(2), 0.0, "rbf"
    else:
        jets = oc2.posterior_jets(state["L"], state["Y"], state["X"], state["UHB"], state["ell"], state["s2"],
                                  state["Bm"], state["M0"], x, kernel=state["kernel"])
        A, Bm, ell, s2, kernel = state["A"], state["Bm"], state["ell"], state["s2"], state["kernel"]
    if mean_model is not None:                    # cbc2.reldeg2_quadratic_terms: Mk += [fhat | ghat], dMk_i[:, 0] += J[:, i]
        f, g, J = pendulum_fg(x, *mean_model)
        jets["Mk"] = jets["Mk"] + np.stack([f, g], axis=1)
        jets["dMk"] = jets["dMk"].copy()
        for i in range(2):
            jets["dMk"][i][:, 0] += J[:, i]
    h, gh, Hh = barrier(x)
    if u_ref is None:
        u_ref = greedy(x, jets["Mk"][:, 0], jets["Mk"][:, 1], dt)
    u_ref = np.asarray(u_ref, dtype=np.float64).reshape(1)
    (mA, mb), (Q, p, r), _, _ = oc2.cbc2_terms(jets, A, Bm, ell, s2, h, gh, Hh, np.asarray(k_alpha), u_ref,
                                               hessian_mode=hessian_mode, kernel=kernel)
    terms = (np.atleast_1d(mA), float(mb), np.atleast_2d(Q), np.atleast_1d(p), float(np.ravel(r)[0]))
    cons = oc.named_socp_constraints(u_ref, ctrl_reg, relax_weight, [terms], [safety_factor])
    u, y, sol = oc.socp_controller_control(u_ref, ctrl_reg, relax_weight, [terms], [safety_factor])
    used = u if sol["status"] == "optimal" else u_ref
    return dict(u_ref=u_ref, terms=terms, cons=cons, u=used, y=y, status=sol["status"],
                x_next=euler(x, used, *true_model, dt), h=h)
