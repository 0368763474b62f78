"""fp64 yardstick of the posterior-plant tests: a plain numpy restatement of what the sampled control step does AFTER its solve
(bcbf_unicycle_control_step_sampled, include/bcbf.h), one instance at a time, loops as the formula has them:

    ubar   = (1, u0, u1)                       u = y as stored
    s      = max(ubar' B_k ubar, 0)
    A      = L L'                              a pivot <= 0 zeroes its column (positive-semidefinite A accepted)
    xdot_s = fhat + ghat u + M_k ubar + sqrt(s) L z
    x_next = x + xdot_s dt
    cbc_s  = sign_k (grad_k . xdot_s + cst_k)

for an instance with status == 0; any other instance keeps its state and gets xdot_s = 0, cbc_s = 0.  Everything is evaluated in
fp64 from the values handed in (fp32 inputs are exact in fp64) and every output is rounded to `dtype` ONCE, which is what the kernel
is specified to do.  The `scale_*` outputs are the sums of the absolute values of the terms of each sum: the magnitudes a rounding
error is relative to (cbc_s cancels, so its own value is no scale)."""
import numpy as np


def chol_psd(A):
    """Lower-triangular L, L L' = A (lower triangle of A read); a pivot <= 0 leaves its column zero."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - sum(L[j, q] * L[j, q] for q in range(j))
        if not d > 0.0:
            continue
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, q] * L[j, q] for q in range(j))) / L[j, j]
    return L


def step(x, y, status, Mk, Bk, A, grad, cst, fhat, ghat, sign, z, dt, dtype=np.float64):
    """x[Bt,3], y[Bt,3] = (u, relax), status[Bt], Mk[Bt,3,3], Bk[Bt,3,3], A[Bt,3,3], grad[Bt,K,3], cst[Bt,K], fhat[Bt,3],
    ghat[Bt,3,2], sign[K], z[Bt,3], dt -> dict(x_next, xdot_s, cbc_s in `dtype`; scale_x, scale_xdot, scale_cbc in fp64)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    x, y, Mk, Bk, A, grad, cst, fhat, ghat, sign, z = map(f, (x, y, Mk, Bk, A, grad, cst, fhat, ghat, sign, z))
    dt = float(dt)
    Bt, K = cst.shape
    x_next, xdot, cbc = x.copy(), np.zeros((Bt, 3)), np.zeros((Bt, K))
    sc_x, sc_xdot, sc_cbc = np.abs(x), np.zeros((Bt, 3)), np.zeros((Bt, K))
    for b in range(Bt):
        if int(status[b]) != 0:
            continue
        ub = np.array([1.0, y[b, 0], y[b, 1]])
        s = max(float(ub @ Bk[b] @ ub), 0.0)
        L = chol_psd(A[b])
        rs = np.sqrt(s)
        for d in range(3):
            terms = [fhat[b, d]] + [ghat[b, d, i] * ub[1 + i] for i in range(2)] + [Mk[b, d, a] * ub[a] for a in range(3)] \
                + [rs * L[d, q] * z[b, q] for q in range(3)]
            xdot[b, d] = sum(terms)
            sc_xdot[b, d] = sum(abs(t) for t in terms)
        x_next[b] = x[b] + xdot[b] * dt
        sc_x[b] = np.abs(x[b]) + sc_xdot[b] * abs(dt)
        for k in range(K):
            cbc[b, k] = sign[k] * (grad[b, k] @ xdot[b] + cst[b, k])
            sc_cbc[b, k] = np.abs(grad[b, k]) @ sc_xdot[b] + abs(cst[b, k])
    r = lambda a: a.astype(dtype)
    return dict(x_next=r(x_next), xdot_s=r(xdot), cbc_s=r(cbc), scale_x=sc_x, scale_xdot=sc_xdot, scale_cbc=sc_cbc)


def row_mean_std(y, Mk, Bk, A, grad, cst, fhat, ghat, sign, k):
    """Mean and standard deviation of row k's condition under the posterior, per instance: sign_k (grad_k . m + cst_k) and
    sqrt((ubar' B_k ubar) grad_k' A grad_k) -- the two sides of the cone  mean >= rho std."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    y, Mk, Bk, A, grad, cst, fhat, ghat, sign = map(f, (y, Mk, Bk, A, grad, cst, fhat, ghat, sign))
    ub = np.concatenate([np.ones((y.shape[0], 1)), y[:, :2]], axis=1)
    m = fhat + np.einsum("bdi,bi->bd", ghat, y[:, :2]) + np.einsum("bda,ba->bd", Mk, ub)
    g = grad[:, k]
    mean = sign[k] * (np.einsum("bd,bd->b", g, m) + cst[:, k])
    var = np.einsum("ba,bac,bc->b", ub, Bk, ub) * np.einsum("bd,bde,be->b", g, A, g)
    return mean, np.sqrt(np.maximum(var, 0.0))
