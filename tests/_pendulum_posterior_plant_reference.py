"""The pendulum's posterior-drawn plant restated in numpy (test infrastructure for bcbf_pendulum_control_step_sampled_f64).

CBC2(x,u) = grad(L_f h)' (f + g u) + k_alpha[0] h + k_alpha[1] L_f h reads four columns of the posterior jet at x,
s = (f, g, df/dtheta, df/domega), matrix-variate normal with covariance A (x) Sigma4.  `jet_covariance` and `draw` follow the
kernel's Cholesky and order of operations; `exact_moments` is the mean and variance of CBC2 as a quadratic form in s -- the
yardstick the draws are held to (the (mean, var) of oracle.cbc2.cbc2_terms is the reference's approximation of it)."""
import math

import numpy as np

KXX = {"rbf": 1.0, "matern52": 5.0 / 3.0, "rbf_matern52": 8.0 / 3.0}      # as oracle.gp_posterior.KERNEL_KXX
IX = (0, 1, 2, 4)                                                        # rows / columns {0, 1, C, 2C} of the 6 x 6 jet blocks


def workspace_from_jets(jets, s2, Bm):
    """oracle.cbc2.posterior_jets' dict in the layout of the device workspace: Mk[2,2], Bk[2,2], G[6,6] = W6'W6, Mj[2,6]."""
    C = 2
    G = np.zeros((6, 6))
    G[:C, :C] = s2 * Bm - jets["Bk"]
    Mj = np.zeros((2, 6))
    Mj[:, :C] = jets["Mk"]
    for d in range(2):
        G[(1 + d) * C:(2 + d) * C, :C] = jets["G10"][d]
        G[:C, (1 + d) * C:(2 + d) * C] = jets["G10"][d].T
        Mj[:, (1 + d) * C:(2 + d) * C] = jets["dMk"][d]
        for e in range(2):
            G[(1 + d) * C:(2 + d) * C, (1 + e) * C:(2 + e) * C] = jets["G11"][d][e]
    return dict(Mk=np.array(jets["Mk"], dtype=np.float64), Bk=np.array(jets["Bk"], dtype=np.float64), G=G, Mj=Mj)


def jet_mean(Mk, Mj):
    """[f, g, df/dtheta, df/domega] as the columns of a 2 x 4 matrix."""
    return np.stack([Mk[:, 0], Mk[:, 1], Mj[:, 2], Mj[:, 4]], axis=1)


def jet_covariance(Bk, G, ell, s2, B00, kxx, gp=True):
    """Sigma4 = rows / columns {0, 1, C, 2C} of P6 - G, P6 = blockdiag(s2 Bm, kxx s2/ell_0^2 Bm, kxx s2/ell_1^2 Bm); the top-left
    block is the workspace's Bk.  The lower triangle is read and mirrored, as the kernel does.  gp=False: zero."""
    S = np.zeros((4, 4))
    if not gp:
        return S
    for a in range(4):
        for c in range(a + 1):
            if a < 2:
                v = Bk[a, c]
            else:
                v = -G[IX[a], IX[c]]
                if a == c:
                    v += kxx * s2 / (ell[a - 2] * ell[a - 2]) * B00
            S[a, c] = S[c, a] = v
    return S


def psd_chol(S):
    """S = L L' of a positive-semidefinite matrix (lower triangle read); a pivot <= 0 zeroes its column."""
    n = S.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = S[j, j]
        for p in range(j):
            d -= L[j, p] * L[j, p]
        if d > 0.0:
            L[j, j] = math.sqrt(d)
            for i in range(j + 1, n):
                v = S[i, j]
                for p in range(j):
                    v -= L[i, p] * L[j, p]
                L[i, j] = v / L[j, j]
    return L


def draw(mean, A, S4, Z):
    """S = mean + L_A Z L_Sigma' for Z[..., 2, 4] (any leading axes): T[p][k] = sum_{q <= k} Z[p][q] L_S[k][q] summed in that
    order, then S[i][k] = mean[i][k] + sum_{p <= i} L_A[i][p] T[p][k]."""
    LA, LS = psd_chol(np.asarray(A, dtype=np.float64)), psd_chol(S4)
    Z = np.asarray(Z, dtype=np.float64)
    T = np.zeros(Z.shape)
    for p in range(2):
        for k in range(4):
            t = np.zeros(Z.shape[:-2])
            for q in range(k + 1):
                t = t + Z[..., p, q] * LS[k, q]
            T[..., p, k] = t
    S = np.zeros(Z.shape)
    for i in range(2):
        for k in range(4):
            t = np.zeros(Z.shape[:-2])
            for p in range(i + 1):
                t = t + LA[i, p] * T[..., p, k]
            S[..., i, k] = mean[i, k] + t
    return S


def cbc2_on(S, u, h, gh, Hh, k_alpha):
    """(xdot_s[..., 2], L_f h, CBC2) on draws S[..., 2, 4] at the control u."""
    xd = np.stack([S[..., 0, 0] + S[..., 0, 1] * u, S[..., 1, 0] + S[..., 1, 1] * u], axis=-1)
    lfh = gh[0] * S[..., 0, 0] + gh[1] * S[..., 1, 0]
    gr = [(Hh[i, 0] * S[..., 0, 0] + Hh[i, 1] * S[..., 1, 0]) + (S[..., 0, 2 + i] * gh[0] + S[..., 1, 2 + i] * gh[1]) for i in range(2)]
    cbc2 = (gr[0] * xd[..., 0] + gr[1] * xd[..., 1]) + k_alpha[0] * h + k_alpha[1] * lfh
    return xd, lfh, cbc2


def quadratic_form(u, h, gh, Hh, k_alpha):
    """CBC2 = s'Q s + l's + c in s = vec(S) (row-major, index 4 i + k); Q symmetric."""
    Mg, Mx = np.zeros((2, 8)), np.zeros((2, 8))
    for i in range(2):
        Mx[i, 4 * i] = 1.0
        Mx[i, 4 * i + 1] = u
        for j in range(2):
            Mg[i, 4 * j] += Hh[i, j]
            Mg[i, 4 * j + 2 + i] += gh[j]
    Q = 0.5 * (Mg.T @ Mx + Mx.T @ Mg)
    l = np.zeros(8)
    for j in range(2):
        l[4 * j] = k_alpha[1] * gh[j]
    return Q, l, k_alpha[0] * h


def exact_moments(mean, A, S4, u, h, gh, Hh, k_alpha):
    """Mean and variance of CBC2 under s ~ N(vec(mean), A (x) Sigma4): tr(QK) + mu'Q mu + l'mu + c and
    2 tr((QK)^2) + (2 Q mu + l)'K (2 Q mu + l)."""
    Q, l, c = quadratic_form(u, h, gh, Hh, k_alpha)
    K = np.kron(np.asarray(A, dtype=np.float64), S4)
    mu = np.asarray(mean, dtype=np.float64).reshape(8)
    QK = Q @ K
    b = 2.0 * Q @ mu + l
    return float(np.trace(QK) + mu @ Q @ mu + l @ mu + c), float(2.0 * np.trace(QK @ QK) + b @ K @ b)


def wrap(theta):
    return ((theta + math.pi) % (2 * math.pi)) - math.pi


def sampled_step(ws, A, ell, s2, B00, kxx, h, gh, Hh, k_alpha, u, z, x, dt, gp=True):
    """One instance of the sampled plant kernel from the step's workspace ws = dict(Mk, Bk, G, Mj): (xdot_s[2], cbc_s[2], x_next[2])."""
    S4 = jet_covariance(ws["Bk"], ws["G"], ell, s2, B00, kxx, gp)
    S = draw(jet_mean(ws["Mk"], ws["Mj"]), A, S4, z)
    xd, lfh, cbc2 = cbc2_on(S, u, h, gh, Hh, k_alpha)
    return xd, np.array([lfh, cbc2]), np.array([wrap(x[0] + xd[0] * dt), x[1] + xd[1] * dt])


# ---------------------------------------------------------------- the small model the moment checks run on
K_ALPHA = (1.0, 3.0)
U0 = 0.7
STATES = ((0.35, -0.6), (1.25, 0.45), (-0.7, 1.1))


def small_model(kernel="rbf", seed=0):
    """16 training rows of a noisy pendulum, ell = (0.8, 1.1), s2 = 1.5, Bm = [[1, .2], [.2, .8]], A = [[.7, .1], [.1, 1.3]],
    zero prior mean: `_pendulum_oracle.oracle_state`'s dict, with the raw rows (UH, Xdot, jitter) beside it."""
    from _pendulum_oracle import oracle_state
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, 16), rng.uniform(-1.2, 1.2, 16)], axis=1)
    U = rng.normal(size=(16, 1))
    UH = np.concatenate([np.ones((16, 1)), U], axis=1)
    Xdot = np.stack([X[:, 1], -10.0 * np.sin(X[:, 0]) + U[:, 0]], axis=1) + 0.05 * rng.normal(size=(16, 2))
    st = oracle_state(X, UH, Xdot, np.array([[1.0, 0.2], [0.2, 0.8]]), np.array([0.8, 1.1]), 1.5, np.zeros((2, 2)),
                      np.full(16, 1e-5), np.array([[0.7, 0.1], [0.1, 1.3]]), kernel=kernel)
    return dict(st, UH=UH, Xdot=Xdot, jitter=np.full(16, 1e-5))


def model_at(state, x):
    """(jets of oracle.cbc2.posterior_jets, workspace layout, jet mean, Sigma4, barrier (h, gh, Hh)) of `state` at x."""
    from oracle import cbc2 as oc2
    from _pendulum_oracle import barrier
    x = np.asarray(x, dtype=np.float64)
    jets = oc2.posterior_jets(state["L"], state["Y"], state["X"], state["UHB"], state["ell"], state["s2"], state["Bm"],
                              state["M0"], x, kernel=state["kernel"])
    ws = workspace_from_jets(jets, state["s2"], state["Bm"])
    S4 = jet_covariance(ws["Bk"], ws["G"], state["ell"], state["s2"], state["Bm"][0, 0], KXX[state["kernel"]])
    return jets, ws, jet_mean(ws["Mk"], ws["Mj"]), S4, barrier(x)
