"""Self-triggering interval (bayes_cbf/trigger_interval.py of the reference) on libbcbf: a high-probability Lipschitz
constant L_fh of the learned dynamics over a grid of test points around x_t and the time tau_k for which the last control stays
safe.  The reference walks a log step by step in Python, all Nte x Nte pairs of the grid per step; here every step (or every
instance of a batched loop) is one workgroup of one launch of `bcbf_trigger_interval`.

What is computed, as the reference EXECUTES it (its recorded outputs, tests/golden/trigger_interval_v1p6p3.npz, were made so):
  * k(x, x') = sf^2 exp(-1/2 sum ((x - x') / ls)^2): sf is squared although the logged value is the output scale already (:33);
  * rbf_d3_knl_d_x_xp_i returns its first line only, -2 ls_i^-2 d k / d x_i (the continuation after the `return` is dead, :41-43);
  * maxk[ei,ej] = A[ei,ei] uBu sf^2 / ls[ej]^2 (the second derivative at x = x', :143); Lkd[ej] = max over ORDERED pairs (a, b),
    a == b included, of uBu d3(X_a, X_b, ej) (:144-147; repeated for every ei upstream, it does not depend on it);
  * r = pdist(grid) is the 2-norm of the whole [Nte, Nte, E] difference array, not the largest distance (:45-46, :126);
  * Lfs[ei,ej] = sqrt(2 log(2 E^2 / deltaL)) maxk + 12 sqrt(6 E) max(maxk, sqrt(r A[ei,ei] Lkd[ej])), Lfh = |Lfs|_F / E (:148-151);
  * Ndte = floor(Nte^(1/E)) points per axis: the default Nte = 1e3 gives 9^3 = 729 (:115-116);
  * Lh = the largest single ELEMENT of grad_cbf(Xtest) over the obstacles, grad_cbf with its batch-wide rho (:159);
  * xvel = |xtp1 - x_t| / dt, tau = (1 / Lfh) log(1 + Lfh zeta / ((Lfh + L_alpha) Lh xvel)); inf at xvel = 0 passes through.
The derivation is specific to the RBF data kernel: any other `kernel_kind` is refused."""
import math
from functools import partial

import numpy as np
import torch

from . import ops
from .tblog import load_tensorboard_scalars
from .unicycle_move_to_pose import obstacles_at_mid_from_start_and_goal


# ------------------------------------------------------------------------------------------------ the reference's helpers (numpy)
def rbf_knl(x, xp, sf, ls):
    """:32-33.  x, xp: [N, E] (or [1, E] against [N, E]); returns [N]."""
    z = (x - xp) / ls
    return sf ** 2 * np.exp(-0.5 * np.sum(z * z, 1))


def rbf_d_knl_d_x_xp_i(x, xp, i, sf, ls):
    """d k / d x_i  (:35-36)."""
    return -(x[:, i] - xp[:, i]) / ls[i] ** 2 * rbf_knl(x, xp, sf, ls)


def rbf_d2_knl_d_x_xp_i(x, xp, i, sf, ls):
    """d^2 k / d x_i d x'_i  (:38-39)."""
    return rbf_knl(x, xp, sf, ls) / ls[i] ** 2 + (x[:, i] - xp[:, i]) / ls[i] ** 2 * rbf_d_knl_d_x_xp_i(x, xp, i, sf, ls)


def rbf_d3_knl_d_x_xp_i(x, xp, i, sf, ls):
    """What :41-43 returns when executed: the first line only, -2 ls_i^-2 d k / d x_i."""
    return -2.0 * ls[i] ** (-2) * rbf_d_knl_d_x_xp_i(x, xp, i, sf, ls)


def pdist(Xtest):
    """The 2-norm of the whole [N, N, E] array of pairwise differences (:45-46) -- one scalar."""
    return np.linalg.norm(Xtest[:, None, :] - Xtest[None, :, :])


def ndgridj(grid_min, grid_max, ns):
    """All combinations of a regular grid, [prod(ns), D], first axis slowest (:48-65)."""
    axes = [np.linspace(lo, hi, int(n)) for lo, hi, n in zip(grid_min, grid_max, ns)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(axes))


def numerical_lipschitz_estimate(Xtest, ej, sf, ls, knl_Aii, knl_uBu, w=None):
    """Sampled Lipschitz estimate (:68-84): |w sigma| maximised over the test points, sigma = Aii uBu d2k(X, X), with its
    density weight.  The reference draws w ~ N(0, 1) unseeded; pass `w` [N] to supply the draws."""
    N = Xtest.shape[0]
    sigma = knl_Aii * knl_uBu * rbf_d2_knl_d_x_xp_i(Xtest, Xtest, ej, sf, ls)
    w = np.random.standard_normal(N) if w is None else np.asarray(w, dtype=np.float64)
    norms = np.abs(w * sigma)
    idx = int(np.argmax(norms))
    return [norms[idx], math.exp(-0.5 * w[idx] ** 2) / math.sqrt(2 * math.pi) * 1e-2]


# ------------------------------------------------------------------------------------------------ batched, on the device
def _grid_norm(off):
    """pdist(off) without the [N, N, E] array: sum_ab |x_a - x_b|^2 = 2 N sum_a |x_a - mean|^2."""
    off = np.asarray(off, dtype=np.float64)
    return math.sqrt(2.0 * off.shape[0] * float(((off - off.mean(0)) ** 2).sum()))


def _require_rbf(kernel_kind):
    kind = ops.DATA_KERNELS.index(kernel_kind) if isinstance(kernel_kind, str) and kernel_kind in ops.DATA_KERNELS else kernel_kind
    if kind != 0:
        raise ValueError("trigger_interval: the Lipschitz bound is derived for the RBF data kernel (kernel_kind 0) only, got %r"
                         % (kernel_kind,))


def default_test_grid(E, Nte=1e3, XteMin=(-0.1, -0.1, -np.pi / 100), XteMax=(0.1, 0.1, np.pi / 100)):
    """The reference's test grid around the origin: floor(Nte^(1/E)) points per axis (:114-125)."""
    Ndte = int(np.floor(np.power(Nte, 1 / E)))
    return ndgridj(list(XteMin)[:E], list(XteMax)[:E], Ndte * np.ones(E))


def trigger_interval_batch(x, xtp1, u, ls, sf, A, B, cbfs, dt, Nte=1e3, deltaL=1e-4, zeta=1e-2, L_alpha=1,
                           XteMin=(-0.1, -0.1, -np.pi / 100), XteMax=(0.1, 0.1, np.pi / 100), off=None, r=None, Lh=None,
                           kernel_kind=0):
    """Trigger interval of Bt instances that already live on the device (the batched loops of rollouts.py): x[Bt,n] the states,
    xtp1[Bt,n] the model's one-step predictions, u[Bt,m] the controls; ls[Bt,n] | [n], sf[Bt] | scalar, A[Bt,n,n] | [n,n],
    B[Bt,1+m,1+m] | [1+m,1+m] the kernel parameters per instance or one model for all; cbfs: objects with `grad_cbf` (ObstacleCBF).
    off[Nte,n]: test-point offsets (default: the reference's grid from Nte / XteMin / XteMax), r: pdist(off); Lh[Bt] overrides
    the obstacle term (then cbfs may be None).  Returns dict(Lfh, tau, xvel, Lkd, Lh, uBu) of device tensors; the O(Nte^2) part is
    one launch of bcbf_trigger_interval, the O(Bt Nte) inputs (uBu, xvel, Lh) are torch on the device."""
    _require_rbf(kernel_kind)
    f = dict(dtype=x.dtype, device=x.device)
    Bt, n = x.shape
    if off is None:
        off = default_test_grid(n, Nte, XteMin, XteMax)
    if r is None:
        r = _grid_norm(off.detach().cpu().numpy() if torch.is_tensor(off) else off)
    off = torch.as_tensor(off).to(**f).contiguous()
    ls, sf, A, B = (torch.as_tensor(v).to(**f) for v in (ls, sf, A, B))
    shared = ls.dim() == 1
    ls, sf = ls.reshape(-1, n).contiguous(), sf.reshape(-1).contiguous()
    Adiag = torch.diagonal(A.reshape(-1, n, n), dim1=-2, dim2=-1).contiguous()
    if not (ls.shape[0] == sf.shape[0] == Adiag.shape[0]) or ls.shape[0] not in (1, Bt) or (shared and ls.shape[0] != 1):
        raise ValueError("trigger_interval_batch: ls %s, sf %s, A %s: one model or one per instance (Bt = %d)"
                         % (tuple(ls.shape), tuple(sf.shape), tuple(A.shape), Bt))
    uh = torch.cat([torch.ones(Bt, 1, **f), u.to(**f).reshape(Bt, -1)], dim=1)
    uBu = torch.einsum("bi,bij,bj->b", uh, B.reshape(-1, uh.shape[1], uh.shape[1]).expand(Bt, -1, -1), uh).contiguous()
    xvel = ((xtp1.to(**f) - x).norm(dim=-1) / dt).contiguous()
    if Lh is None:
        Xtest = off[None] + x[:, None, :]
        Lh = torch.stack([h.grad_cbf(Xtest).amax(dim=(-2, -1)) for h in cbfs]).amax(dim=0)
    Lh = torch.as_tensor(Lh).to(**f).expand(Bt).contiguous()
    Lfh, tau, Lkd = ops.trigger_interval(x.contiguous(), off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL=deltaL, zeta=zeta,
                                         L_alpha=L_alpha)
    return dict(Lfh=Lfh, tau=tau, xvel=xvel, Lkd=Lkd, Lh=Lh, uBu=uBu)


_DEFAULT_CBFS = partial(obstacles_at_mid_from_start_and_goal, torch.tensor([-3, -1, -math.pi / 4]),
                        torch.tensor([0, 0, math.pi / 4]), term_weights=[0.7, 0.3])


def unicycle_trigger_interval_compute(events_file, out_data_files, Nte=1e3, deltaL=1e-4, zeta=1e-2, L_alpha=1,
                                      XteMin=[-0.1, -0.1, -np.pi / 100], XteMax=[0.1, 0.1, np.pi / 100], cbfs=_DEFAULT_CBFS,
                                      dt=0.01, device="cuda", dtype=torch.float64, kernel_kind=0):
    """The reference's entry point (:86-177): read a run's event file (tags vis/state, vis/uopt, vis/xtp1, vis/knl_*), compute
    Lfh, tau, xvel and the sampled Lfh_num, tau_num for every logged step and write them with np.savetxt to
    out_data_files['Lfh.np.txt' | 'tau.np.txt' | 'xvel.np.txt' | 'Lfh_num.np.txt' | 'tau_num.np.txt'].  All logged steps run as
    ONE batch through bcbf_trigger_interval.  Returns the five arrays as a dict as well."""
    _require_rbf(kernel_kind)
    by_tag = load_tensorboard_scalars(events_file)
    col = lambda tag: np.asarray([np.asarray(v, dtype=np.float64) for _, v in by_tag[tag]])
    ls, sf = col("vis/knl_lengthscale"), col("vis/knl_scalefactor").reshape(-1)
    A, B = col("vis/knl_A"), col("vis/knl_B")
    x, xtp1, u = col("vis/state"), col("vis/xtp1"), col("vis/uopt")
    nsteps, E = x.shape
    ls, A, B = ls.reshape(nsteps, E), A.reshape(nsteps, E, E), B.reshape(nsteps, u.shape[1] + 1, u.shape[1] + 1)
    grid = default_test_grid(E, Nte, XteMin, XteMax)
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
    out = trigger_interval_batch(t(x), t(xtp1), t(u), t(ls), t(sf), t(A), t(B), cbfs(), dt, deltaL=deltaL, zeta=zeta,
                                 L_alpha=L_alpha, off=grid)                 # (r = pdist(grid), :126, is formed there)
    host = {k: v.detach().cpu().double().numpy() for k, v in out.items()}
    # the sampled estimate (:150-157, :169): the second derivative at x = x' is the same at every test point, so only the
    # draws differ between the points; unseeded, as upstream
    Lfh_num = np.empty(nsteps)
    for s in range(nsteps):
        Xtest = grid + x[s]
        Lfs_num = [[numerical_lipschitz_estimate(Xtest, ej, sf[s], ls[s], A[s, ei, ei], host["uBu"][s])[0] for ej in range(E)]
                   for ei in range(E)]
        Lfh_num[s] = np.linalg.norm(Lfs_num) / E
    with np.errstate(divide="ignore", invalid="ignore"):
        tau_num = (1 / Lfh_num) * np.log(1 + Lfh_num * zeta / ((Lfh_num + L_alpha) * host["Lh"] * np.abs(host["xvel"])))
    res = {"xvel.np.txt": host["xvel"], "Lfh.np.txt": host["Lfh"], "Lfh_num.np.txt": Lfh_num, "tau.np.txt": host["tau"],
           "tau_num.np.txt": tau_num}
    for name, arr in res.items():
        np.savetxt(out_data_files[name], arr)
    return res
