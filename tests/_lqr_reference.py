"""The LQR nominal controller restated in numpy fp64 (test infrastructure for bcbf_lqr_nominal_f32 / _f64 and the pendulum
step's nominal = 1): LQRController.control (reference controllers.py:64-115) with the recursion of affine_backpropagation
(reference ilqr.py:43-76) in place of the external `bdlqr` package.  Everything is batched over a leading axis, so a
1000-iteration horizon on a few hundred instances takes a fraction of a second.

    B = g dt, s = -Q x_goal, z = 0;  pass(A): P = Q, o = s, T times
        G = R + B'PB,  K = G^-1 B'PA,  k = G^-1 (z + B'o),  P <- Q + A'PA - A'PB K,  o <- s + A'o - K'(z + B'o)
    and -K x - k of the last iteration;  u0 = pass(I + dt Jf),  u = pass(I + dt (Jf + sum_j Jg_j u0_j)).
"""
import numpy as np


def solve_no_exchange(G, Y):
    """G X = Y for G[..., m, m], Y[..., m, c] by elimination without row exchanges (as the kernel); ok[...] is False where a
    pivot is not > 0."""
    G, Y = np.array(G, dtype=np.float64), np.array(Y, dtype=np.float64)
    m = G.shape[-1]
    ok = np.ones(G.shape[:-2], dtype=bool)
    with np.errstate(all="ignore"):
        for p in range(m):
            piv = G[..., p, p]
            ok &= piv > 0.0
            for r in range(p + 1, m):
                f = G[..., r, p] / piv
                G[..., r, :] = G[..., r, :] - f[..., None] * G[..., p, :]
                Y[..., r, :] = Y[..., r, :] - f[..., None] * Y[..., p, :]
        for p in range(m - 1, -1, -1):
            v = Y[..., p, :]
            for r in range(p + 1, m):
                v = v - G[..., p, r, None] * Y[..., r, :]
            Y[..., p, :] = v / G[..., p, p, None]
    return Y, ok


def recursion(A, B, Q, R, s, T, z=None):
    """T iterations from P = Q, o = s on A[..., n, n], B[..., n, m] (Q, R, s, z shared).  Returns (P, o, K, k, ok): P, o after
    the last iteration, K, k of the last iteration (from the P, o before it)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    lead = A.shape[:-2]
    n, m = B.shape[-2:]
    z = np.zeros(m) if z is None else np.asarray(z, dtype=np.float64)
    P = np.broadcast_to(np.asarray(Q, dtype=np.float64), lead + (n, n)).copy()
    o = np.broadcast_to(np.asarray(s, dtype=np.float64), lead + (n,)).copy()
    At, Bt = np.swapaxes(A, -1, -2), np.swapaxes(B, -1, -2)
    ok = np.ones(lead, dtype=bool)
    K = k = None
    for _ in range(int(T)):
        PB, PA = P @ B, P @ A
        G = R + Bt @ PB
        w = z + (Bt @ o[..., None])[..., 0]
        Kk, good = solve_no_exchange(G, np.concatenate([Bt @ PA, w[..., None]], axis=-1))
        ok &= good
        K, k = Kk[..., :n], Kk[..., n]
        P = Q + At @ PA - (At @ PB) @ K
        o = s + (At @ o[..., None])[..., 0] - (np.swapaxes(K, -1, -2) @ w[..., None])[..., 0]
    return P, o, K, k, ok


def lqr_pass(A, B, Q, R, s, x, T):
    """-K x - k of the last of T iterations; (u[..., m], ok[...])."""
    _, _, K, k, ok = recursion(A, B, Q, R, s, T)
    with np.errstate(all="ignore"):
        u = -(K @ np.asarray(x, dtype=np.float64)[..., None])[..., 0] - k
    return u, ok


def unpack_jets(Mk, Mj, n, m):
    """(g[Bt,n,m], Jf[Bt,n,n], Jg[Bt,m,n,n]) from the jets' layout Mk[Bt,n,C], Mj[Bt,n,C(1+n)]."""
    C = 1 + m
    Mk, Mj = np.asarray(Mk, dtype=np.float64), np.asarray(Mj, dtype=np.float64)
    g = Mk[:, :, 1:]
    J = Mj.reshape(Mj.shape[0], n, 1 + n, C)[:, :, 1:, :]              # [b, i, d, c]
    Jf = J[..., 0]
    Jg = np.moveaxis(J[..., 1:], -1, 1)                                 # [b, j, i, d]
    return g, Jf, Jg


def lqr_nominal(Mk, Mj, x, x_goal, Q, R, dt, numSteps, t=0):
    """bcbf_lqr_nominal_*: (u[Bt,m], u0[Bt,m], status[Bt]) with the horizon max(numSteps - t, 1); u = u0 = 0 where status is 1."""
    x = np.asarray(x, dtype=np.float64)
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    n, m = x.shape[1], R.shape[0]
    g, Jf, Jg = unpack_jets(Mk, Mj, n, m)
    T = max(int(numSteps) - int(t), 1)
    B = g * dt
    s = -Q @ np.asarray(x_goal, dtype=np.float64)
    I = np.eye(n)
    u0, ok0 = lqr_pass(I + dt * Jf, B, Q, R, s, x, T)
    u0s = np.where(ok0[:, None], u0, 0.0)
    u, ok1 = lqr_pass(I + dt * (Jf + np.einsum("bjid,bj->bid", Jg, u0s)), B, Q, R, s, x, T)
    ok = ok0 & ok1
    return np.where(ok[:, None], u, 0.0), np.where(ok[:, None], u0, 0.0), (~ok).astype(np.int32)
