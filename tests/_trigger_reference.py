"""fp64 yardstick of the trigger-interval tests: a plain numpy restatement of what the reference's
unicycle_trigger_interval_compute executes per step (bayes_cbf/trigger_interval.py:128-167), loops as it has them -- one pass over
the test points, each against all the others, brute force over ordered pairs -- with the quirks kept: sf squared, the third
derivative's first line only, the pairs a == b included, r the norm of the whole difference array, Lh the largest element of grad_cbf with its batch-wide rho.
(The reference repeats the pair loop for every ei; it does not depend on ei and is done once per ej here.)"""
import math

import numpy as np


def grid(E=3, Nte=1e3, lo=(-0.1, -0.1, -np.pi / 100), hi=(0.1, 0.1, np.pi / 100)):
    nd = int(np.floor(np.power(Nte, 1 / E)))
    axes = [np.linspace(lo[j], hi[j], nd) for j in range(E)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, E)


def whole_norm(pts):
    return float(np.linalg.norm(pts[:, None, :] - pts[None, :, :]))


def lkd(Xtest, ls, sf, uBu, chunk=32):
    """Lkd[ej] = max over ordered pairs (a, b) of uBu * (-2 ls_j^-2) * (-(X_a - X_b)_j / ls_j^2) * sf^2 exp(-1/2 |(X_a - X_b) / ls|^2):
    the reference's loop over the points b, each against all points a (`chunk` of them per numpy call, for speed only)."""
    N, E = Xtest.shape
    best = np.full(E, -np.inf)
    for b in range(0, N, chunk):
        diff = Xtest[None, :, :] - Xtest[b:b + chunk, None, :]
        k = sf ** 2 * np.exp(-0.5 * (diff ** 2 @ ls ** (-2.0)))
        d1 = -diff / ls ** 2 * k[..., None]
        best = np.maximum(best, np.max(uBu * (-2.0 * ls ** (-2.0) * d1), axis=(0, 1)))
    return best


def lfh_tau(Lkd, ls, sf, Adiag, uBu, r, Lh, xvel, deltaL=1e-4, zeta=1e-2, L_alpha=1.0):
    E = len(ls)
    Lfs = np.zeros((E, E))
    for ei in range(E):
        for ej in range(E):
            maxk = Adiag[ei] * uBu * (ls[ej] ** (-2) * sf ** 2)           # the second derivative at x = x': the same at every point
            with np.errstate(invalid="ignore"):
                Lfs[ei, ej] = math.sqrt(2 * math.log(2 * E ** 2 / deltaL)) * maxk + 12 * math.sqrt(6 * E) * max(
                    maxk, np.sqrt(r * Adiag[ei] * Lkd[ej]))
    Lfh = np.linalg.norm(Lfs) / E
    with np.errstate(divide="ignore"):
        tau = (1 / Lfh) * np.log(1 + Lfh * zeta / ((Lfh + L_alpha) * Lh * abs(xvel)))
    return Lfh, tau


def step(x, off, ls, sf, Adiag, uBu, r, Lh, xvel, Xtest=None, **kw):
    """One instance: dict(Lkd[E], Lfh, tau).  Xtest overrides off + x (the fp32 tests hand in the fp32-rounded points)."""
    f = lambda v: np.asarray(v, dtype=np.float64)
    Xtest = f(off) + f(x) if Xtest is None else f(Xtest)
    L = lkd(Xtest, f(ls), float(sf), float(uBu))
    Lfh, tau = lfh_tau(L, f(ls), float(sf), f(Adiag), float(uBu), float(r), float(Lh), float(xvel), **kw)
    return dict(Lkd=L, Lfh=Lfh, tau=tau)


# ------------------------------------------------------------------------------------------------ the obstacle barrier
def default_obstacles():
    """(center[2], radius, weights) of the reference's default cbfs (trigger_interval.py:95-100): built from float32 tensors there."""
    x, xg = np.array([-3, -1, -math.pi / 4], dtype=np.float32), np.array([0, 0, math.pi / 4], dtype=np.float32)
    d = x[:2] - xg[:2]
    mid, off = (x[:2] + xg[:2]) / np.float32(2), np.array([-d[1], d[0]], dtype=np.float32) / np.float32(3)
    rad = np.float32(np.sqrt(np.float32(d @ d))) / np.float32(4)
    return [((mid + off).astype(np.float64), float(rad), (0.7, 0.3)), ((mid - off).astype(np.float64), float(rad), (0.7, 0.3))]


def cbf(center, radius, w, s):
    g = s[:2] - center
    gn = g / np.linalg.norm(g)
    return w[0] * ((g ** 2).sum() - radius ** 2) + w[1] * (math.cos(s[2]) * gn[0] + math.sin(s[2]) * gn[1])


def grad_cbf(center, w, X):
    """Rows [N, 3]; rho is the norm of ALL the (x, y) offsets of the batch, as the reference's torch.norm takes it."""
    g = X[:, :2] - center
    rho = np.linalg.norm(g)
    al, th = np.arctan2(g[:, 1], g[:, 0]), X[:, 2]
    out = np.zeros_like(X)
    out[:, 0] = w[0] * 2 * g[:, 0] + w[1] * np.sin(al - th) * g[:, 1] / rho ** 2
    out[:, 1] = w[0] * 2 * g[:, 1] - w[1] * np.sin(al - th) * g[:, 0] / rho ** 2
    out[:, 2] = -w[1] * np.sin(th - al)
    return out


def saved_run(G, steps=None, dt=0.01, **kw):
    """The whole computation on the committed learning run (a loaded saved_run_learning_v1p6p3.npz): dict(Lfh, tau, xvel)[T]."""
    off = grid()
    r = whole_norm(off)
    obs = default_obstacles()
    steps = range(len(G["state"])) if steps is None else steps
    out = dict(Lfh=[], tau=[], xvel=[])
    for t in steps:
        x, ls, sf = G["state"][t].astype(np.float64), G["knl_lengthscale"][t].astype(np.float64), float(G["knl_scalefactor"][t])
        A, B = G["knl_A"][t].astype(np.float64), G["knl_B"][t].astype(np.float64)
        uh = np.r_[1.0, G["uopt"][t].astype(np.float64)]
        uBu = uh @ B @ uh
        Xtest = off + x
        Lh = max(grad_cbf(c, w, Xtest).max() for c, _, w in obs)
        xvel = np.linalg.norm(G["xtp1"][t].astype(np.float64) - x) / dt
        res = step(x, off, ls, sf, np.diag(A), uBu, r, Lh, xvel, **kw)
        out["Lfh"].append(res["Lfh"])
        out["tau"].append(res["tau"])
        out["xvel"].append(xvel)
    return {k: np.array(v) for k, v in out.items()}
