"""Plain torch fp64 references of the batched hyper-parameter fit (`BatchedHyperFit`), written from the documents and not
from the kernels: the header of csrc/mll_grad.hip (the sums of bcbf_mll_grad), the parameter layout of include/bcbf.h /
batched_fit.py (bcbf_fit_derive), the comment block above fit_adam_step_kernel in csrc/fit.hip (loss, chain rule, Adam) and the
kernel definitions of oracle/gp_posterior.py (differentiated by autograd).  Everything is batched over a leading model dimension
and runs on whatever device its inputs live on; tests/test_fit_reference.py pins these functions themselves on the CPU."""
import math

import torch

KINDS = ("rbf", "matern52", "rbf_matern52")
F64 = torch.float64


def _d(t):
    return None if t is None else t.detach().to(F64)


def data_kernel(X, ell, kind="rbf"):
    """k_kind(X, X; ell) / s2  [B,N,N]: oracle.gp_posterior's rbf_ard_kernel / matern52_ard_kernel / their product, in torch.
    (sqrt at distance 0 is clamped so that autograd gives the limit 0 of the diagonal's length-scale derivative, not 0 * inf)"""
    z = (X[:, :, None, :] - X[:, None, :, :]) / ell[:, None, None, :]
    d2 = (z * z).sum(-1)
    if kind == "rbf":
        return torch.exp(-0.5 * d2)
    a = torch.sqrt(5.0 * d2.clamp_min(1e-300))
    mat = (1.0 + a + 5.0 / 3.0 * d2) * torch.exp(-a)
    if kind == "matern52":
        return mat
    if kind == "rbf_matern52":
        return torch.exp(-0.5 * d2) * mat
    raise ValueError(kind)


def kb_matrix(X, UH, Bm, ell, s2, lin=None, kind="rbf"):
    """K_b = s2 (k_kind(X, X; ell) + lin X X')  o  (UH Bm UH')   [B,N,N] (no jitter)."""
    k = data_kernel(X, ell, kind)
    if lin is not None:
        k = k + lin[:, None, None] * (X @ X.transpose(1, 2))
    return s2[:, None, None] * k * (UH @ Bm @ UH.transpose(1, 2))


def g_matrix(alpha, Kinv, Ainv):
    """G = d log p / d K_b = 1/2 (alpha A^-1 alpha' - nt K_b^-1)  for ANY alpha [B,N,nt] and symmetric Kinv [B,N,N]."""
    return 0.5 * (alpha @ Ainv @ alpha.transpose(1, 2) - alpha.shape[2] * Kinv)


def logdet_chol(K):
    """(logdet K, sum_i |2 log L_ii|) by torch.linalg.cholesky in fp64."""
    dl = 2.0 * torch.log(torch.linalg.cholesky(K.to(F64)).diagonal(dim1=1, dim2=2))
    return dl.sum(1), dl.abs().sum(1)


def mll_sums(alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin=None, kind="rbf", jitter=None):
    """The outputs of bcbf_mll_grad from its own inputs, the gradients by torch autograd of sum_ij G_ij K_b,ij with G held
    constant.  dict(g_ell[B,n], g_s2[B], g_B[B,C,C], RtA, UHtA, abs_sum[B] (+ g_lin[B]) (+ logdetK, logdet_abs with `jitter`))."""
    alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin, jitter = map(_d, (alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin, jitter))
    G = g_matrix(alpha, Kinv, Ainv)
    leaves = [t.clone().requires_grad_(True) for t in ((ell, s2, Bm) if lin is None else (ell, s2, Bm, lin))]
    Kb = kb_matrix(X, UH, leaves[2], leaves[0], leaves[1], None if lin is None else leaves[3], kind)
    terms = G * Kb
    grads = torch.autograd.grad(terms.sum(), leaves)
    out = dict(g_ell=grads[0], g_s2=grads[1], g_B=grads[2], RtA=R.transpose(1, 2) @ alpha, UHtA=UH.transpose(1, 2) @ alpha,
               abs_sum=terms.detach().abs().sum((1, 2)))
    if lin is not None:
        out["g_lin"] = grads[3]
    if jitter is not None:
        out["logdetK"], out["logdet_abs"] = logdet_chol(Kb.detach() + torch.diag_embed(jitter))
    return out


def mll_sums_written(alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin=None):
    """The same sums written out (RBF, optional linear part), as the header of csrc/mll_grad.hip states them:
    g_s2 = sum G k u,  g_ell_d = sum G s2 k_rbf u dx_d^2 / ell_d^3,  g_B = s2 UH' (G o k) UH,  g_lin = sum G s2 u x_i'x_j.
    Also each output's own sum of absolute terms (`abs_*`)."""
    alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin = map(_d, (alpha, Kinv, X, UH, R, Ainv, Bm, ell, s2, lin))
    G = g_matrix(alpha, Kinv, Ainv)
    dx = X[:, :, None, :] - X[:, None, :, :]
    krbf = torch.exp(-0.5 * ((dx / ell[:, None, None, :]) ** 2).sum(-1))
    dot = X @ X.transpose(1, 2)
    k = krbf if lin is None else krbf + lin[:, None, None] * dot
    u = UH @ Bm @ UH.transpose(1, 2)
    s2_ = s2[:, None, None]
    Gk = G * k
    out = dict(g_s2=(Gk * u).sum((1, 2)),
               g_ell=((G * s2_ * krbf * u)[..., None] * dx ** 2).sum((1, 2)) / ell ** 3,
               g_B=s2_ * (UH.transpose(1, 2) @ Gk @ UH),
               RtA=R.transpose(1, 2) @ alpha, UHtA=UH.transpose(1, 2) @ alpha,
               abs_sum=(Gk * u * s2_).abs().sum((1, 2)),
               abs_s2=(Gk * u).abs().sum((1, 2)),
               abs_ell=((G * s2_ * krbf * u).abs()[..., None] * dx ** 2).sum((1, 2)) / ell ** 3)
    if lin is not None:
        out["g_lin"] = (G * s2_ * u * dot).sum((1, 2))
    return out


# ---- the raw parameters (include/bcbf.h, bcbf_fit_derive) ------------------------------------------------------------------
def fit_ranks(n, m, rank):
    return (n, 1 + m) if rank is None else (int(rank), int(rank))


def derive(theta, n, m, rank=None):
    """theta[B,P] = [raw ell (n) | raw s2 | Wa (n x rA) | va (n) | Wb (C x rB) | vb (C) | M0 (C x n)] ->
    dict(ell, s2, A, Bm, M0): softplus for ell, s2 and the diagonals, W W' + diag (differentiable in theta)."""
    sp = torch.nn.functional.softplus
    C = 1 + m
    rA, rB = fit_ranks(n, m, rank)
    B_ = theta.shape[0]
    o = 0
    ell = sp(theta[:, o:o + n]); o += n
    s2 = sp(theta[:, o]); o += 1
    Wa = theta[:, o:o + n * rA].reshape(B_, n, rA); o += n * rA
    va = theta[:, o:o + n]; o += n
    Wb = theta[:, o:o + C * rB].reshape(B_, C, rB); o += C * rB
    vb = theta[:, o:o + C]; o += C
    M0 = theta[:, o:o + C * n].reshape(B_, C, n); o += C * n
    assert o == theta.shape[1], "theta has %d columns, the layout %d" % (theta.shape[1], o)
    return dict(ell=ell, s2=s2, A=Wa @ Wa.transpose(1, 2) + torch.diag_embed(sp(va)),
                Bm=Wb @ Wb.transpose(1, 2) + torch.diag_embed(sp(vb)), M0=M0)


def log_gamma_prior(ell, prior):
    """sum_d log Gamma(ell_d; concentration c, rate r)."""
    c, r = prior
    return (c * math.log(r) - math.lgamma(c) + (c - 1.0) * torch.log(ell) - r * ell).sum(-1)


def neg_mll_batch(theta, X, UH, Y, jitter, n, m, rank=None, prior=None, inverse="cholesky"):
    """loss[B] = -log p(Y_b) / (N n)  (- log GammaPrior(ell_b) / (N n)) of B models, differentiable in theta;
    log p = -1/2 tr(A^-1 R' K^-1 R) - n/2 logdet K - N/2 logdet A - N n/2 log 2 pi,  K = K_b + diag jitter,  R = Y - UH M0.
    inverse = "cholesky": torch.linalg.cholesky of K;  "inv": torch.linalg.inv / torch.logdet (the second route that measures the
    reference's own sensitivity)."""
    N = X.shape[1]
    hp = derive(theta, n, m, rank)
    K = kb_matrix(X, UH, hp["Bm"], hp["ell"], hp["s2"]) + torch.diag_embed(jitter)
    R = Y - UH @ hp["M0"]
    Ainv = torch.linalg.inv(hp["A"])
    if inverse == "cholesky":
        L = torch.linalg.cholesky(K)
        W = torch.linalg.solve_triangular(L, R, upper=False)
        quad = (Ainv * (W.transpose(1, 2) @ W)).sum((1, 2))
        logdetK = 2.0 * torch.log(L.diagonal(dim1=1, dim2=2)).sum(1)
    else:
        quad = (Ainv * (R.transpose(1, 2) @ torch.linalg.inv(K) @ R)).sum((1, 2))
        logdetK = torch.logdet(K)
    logp = -0.5 * quad - 0.5 * n * logdetK - 0.5 * N * torch.logdet(hp["A"]) - 0.5 * N * n * math.log(2.0 * math.pi)
    if prior is not None:
        logp = logp + log_gamma_prior(hp["ell"], prior)
    return -logp / (N * n)


def neg_mll(theta_row, X, UH, Y, jitter, n, m, rank=None, prior=None, inverse="cholesky"):
    """One model: theta_row[P], X[N,n], UH[N,C], Y[N,n], jitter[N] -> the scalar loss (fp64, differentiable)."""
    return neg_mll_batch(theta_row[None], X[None], UH[None], Y[None], jitter[None], n, m, rank, prior, inverse)[0]


def neg_mll_value_and_grad(theta, X, UH, Y, jitter, n, m, rank=None, prior=None, inverse="cholesky"):
    th = theta.detach().to(F64).clone().requires_grad_(True)
    loss = neg_mll_batch(th, _d(X), _d(UH), _d(Y), _d(jitter), n, m, rank, prior, inverse)
    (grad,) = torch.autograd.grad(loss.sum(), th)              # (the models are independent: row b is d loss_b / d theta_b)
    return loss.detach(), grad


# ---- bcbf_fit_adam_step (the comment block above fit_adam_step_kernel) -----------------------------------------------------
def loss_and_grad_from_sums(theta, sums, Ainv, logdetA, N, n, m, rank=None, prior=None):
    """loss[B] and d loss / d theta [B,P] from bcbf_mll_grad's sums (g_ell, g_s2, g_B, logdetK, RtA, UHtA), A^-1 and logdet A, all
    taken as given numbers:  d log p / dA = 1/2 A^-1 (R'alpha) A^-1 - N/2 A^-1,  d log p / dM0 = (UH'alpha) A^-1,  d / d ell, s2, B
    given; the chain rule through softplus and W W' + diag is torch autograd's (a linear form in the derived values)."""
    g_ell, g_s2, g_B, logdetK, RtA, UHtA = (_d(t) for t in sums[:6])
    Ainv, logdetA = _d(Ainv), _d(logdetA)
    scale = 1.0 / (N * n)
    logp = (-0.5 * (Ainv * RtA.transpose(1, 2)).sum((1, 2)) - 0.5 * n * logdetK - 0.5 * N * logdetA
            - 0.5 * N * n * math.log(2.0 * math.pi))
    gA = 0.5 * Ainv @ RtA @ Ainv - 0.5 * N * Ainv
    gM0 = UHtA @ Ainv
    th = theta.detach().to(F64).clone().requires_grad_(True)
    hp = derive(th, n, m, rank)
    lin_form = ((g_ell * hp["ell"]).sum(1) + g_s2 * hp["s2"] + (g_B * hp["Bm"]).sum((1, 2)) + (gA * hp["A"]).sum((1, 2))
                + (gM0 * hp["M0"]).sum((1, 2)))
    lp = log_gamma_prior(hp["ell"], prior) if prior is not None else torch.zeros_like(logp)
    (grad,) = torch.autograd.grad((-scale * (lin_form + lp)).sum(), th)
    return (-scale * (logp + lp)).detach(), grad


def adam_step(theta, mom1, mom2, grad, step, lr, dtype, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's update as the kernel's comment states it, in fp64 with the roundings to the parameters' `dtype` where
    the kernel rounds: the gradient, both moments as stored, and the moments as the update reads them back.
      m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  theta -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
    Returns (theta, mom1, mom2) in fp64 holding values representable in `dtype`."""
    rnd = lambda t: t.to(dtype).to(F64)
    g = rnd(grad.to(F64))
    m, v = mom1.to(F64), mom2.to(F64)
    m = rnd(m + (g - m) * (1.0 - beta1))
    v = rnd(v * beta2 + (1.0 - beta2) * g * g)
    denom = torch.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
    return rnd(theta.to(F64) - lr / (1.0 - beta1 ** step) * (m / denom)), m, v
