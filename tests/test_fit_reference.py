"""The references of tests/_fit_reference.py pinned on the CPU, so that the GPU tests that trust them (test_gpu_fit_scale.py) rest
on something checked: the autograd route of the bcbf_mll_grad sums against the written-out sums, and the torch likelihood against
the numpy oracle."""
import math

import numpy as np
import torch

import _fit_reference as ref


def _inputs(B, N, n, m, nt, seed, lin=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    X = torch.rand(B, N, n, generator=g, dtype=torch.float64) * 2.0
    UH = torch.cat([torch.ones(B, N, 1, dtype=torch.float64), r(B, N, m)], dim=2)
    S = r(B, N, N) / math.sqrt(N)
    W = r(B, nt, nt)
    d = dict(alpha=r(B, N, nt), Kinv=S + S.transpose(1, 2), X=X, UH=UH, R=r(B, N, nt),
             Ainv=W @ W.transpose(1, 2) + torch.eye(nt, dtype=torch.float64), Bm=r(B, m + 1, m + 1) + 2.0 * torch.eye(m + 1, dtype=torch.float64),
             ell=0.6 + torch.rand(B, n, generator=g, dtype=torch.float64), s2=0.5 + torch.rand(B, generator=g, dtype=torch.float64))
    if lin:
        d["lin"] = 0.2 + torch.rand(B, generator=g, dtype=torch.float64)
    return d


def test_mll_sums_autograd_route_equals_the_written_out_sums():
    """d/d(ell, s2, Bm, lin) of sum G o K_b by autograd == the sums of csrc/mll_grad.hip's header written out, to 1e-14 of
    abs_sum (N = 512 with a non-symmetric Bm agrees to 3e-17; 1e-14 leaves room for the order of summation and no more), and
    |sum| / abs_sum is not small -- abs_sum is the scale a pair sum is compared on."""
    for (B, N, n, m, nt, lin) in ((2, 200, 3, 2, 3, False), (1, 512, 3, 2, 3, False), (2, 65, 8, 3, 8, False), (2, 90, 3, 5, 1, True)):
        d = _inputs(B, N, n, m, nt, seed=N, lin=lin)
        a, w = ref.mll_sums(**d), ref.mll_sums_written(**d)
        sc = a["abs_sum"]
        assert torch.allclose(sc, w["abs_sum"], rtol=1e-14, atol=0)
        for k in ("g_ell", "g_s2", "g_B", "RtA", "UHtA") + (("g_lin",) if lin else ()):
            scale = sc.reshape((B,) + (1,) * (a[k].dim() - 1)) if k.startswith("g_") else a[k].abs().amax()
            assert float(((a[k] - w[k]).abs() / scale).max()) < 1e-14, (N, k)
        assert float((a["g_s2"].abs() / sc).min()) > 1e-4, "abs_sum is not the scale of the sums here"
        assert float((w["abs_s2"] / sc).min()) > 0.5 and float((w["abs_ell"] / sc[:, None]).min()) > 1e-2


def test_mll_sums_matern_kinds_differentiate_the_oracle_definitions():
    """The Matern and product kernels of the reference are the oracle's (numpy) definitions, and their length-scale gradient by
    autograd equals central differences of those definitions (incl. the diagonal, where sqrt is not differentiable)."""
    from oracle import gp_posterior as ogp
    d = _inputs(1, 40, 3, 2, 3, seed=3)
    for kind in ref.KINDS:
        k = ref.data_kernel(d["X"], d["ell"], kind)[0].numpy()
        np.testing.assert_allclose(k, ogp.DATA_KERNELS[kind](d["X"][0].numpy(), d["X"][0].numpy(), d["ell"][0].numpy(), 1.0), rtol=1e-13, atol=1e-15)
        s = ref.mll_sums(kind=kind, **d)
        G = ref.g_matrix(d["alpha"], d["Kinv"], d["Ainv"])[0].numpy()
        u = (d["UH"] @ d["Bm"] @ d["UH"].transpose(1, 2))[0].numpy()

        def val(ell):
            return float((G * ogp.DATA_KERNELS[kind](d["X"][0].numpy(), d["X"][0].numpy(), ell, float(d["s2"][0])) * u).sum())
        for q in range(3):
            e = d["ell"][0].numpy().copy()
            h = 1e-6
            ep, em = e.copy(), e.copy()
            ep[q] += h
            em[q] -= h
            fd = (val(ep) - val(em)) / (2 * h)
            assert abs(fd - float(s["g_ell"][0, q])) < 1e-7 * float(s["abs_sum"][0]), (kind, q)


def test_neg_mll_equals_the_oracle_likelihood_at_the_derived_values():
    """_fit_reference.neg_mll (torch, from the raw parameters) == -oracle.gp_posterior.marginal_log_likelihood / (N n) (- log Gamma
    prior) at softplus / W W' + diag of the same row, by both routes to K_b^-1, for full-rank, rank-one and diagonal factors."""
    from oracle import gp_posterior as ogp
    rng = np.random.default_rng(7)
    for (n, m, N, rank, prior) in ((3, 2, 60, None, None), (3, 2, 45, 1, (1e-3, 1e-3)), (2, 1, 33, 0, None), (4, 3, 50, None, (2.0, 3.0))):
        rA, rB = ref.fit_ranks(n, m, rank)
        C = 1 + m
        P = n + 1 + n * rA + n + C * rB + C + C * n
        theta = torch.as_tensor(0.4 * rng.normal(size=P))
        X, U, Y = rng.uniform(-2, 2, (N, n)), rng.normal(size=(N, m)), rng.normal(size=(N, n))
        jit = 1e-5 * rng.uniform(0.1, 0.9, N)
        UH = ogp.homogeneous_controls(U)
        hp = {k: v[0].numpy() for k, v in ref.derive(theta[None], n, m, rank).items()}
        o = 0
        np.testing.assert_allclose(hp["ell"], ogp.softplus(theta[:n].numpy()), rtol=1e-14)
        o = n + 1
        np.testing.assert_allclose(hp["A"], ogp.index_kernel_covar(theta[o:o + n * rA].numpy().reshape(n, rA), theta[o + n * rA:o + n * rA + n].numpy()), rtol=1e-13, atol=1e-15)
        want = -ogp.marginal_log_likelihood(X, UH, Y, hp["A"], hp["Bm"], hp["ell"], float(hp["s2"]), hp["M0"], jit) / (N * n)
        if prior is not None:
            c, r = prior
            want -= sum(c * math.log(r) - math.lgamma(c) + (c - 1) * math.log(l) - r * l for l in hp["ell"]) / (N * n)
        for inverse in ("cholesky", "inv"):
            got = float(ref.neg_mll(theta, *(torch.as_tensor(a) for a in (X, UH, Y, jit)), n, m, rank, prior, inverse))
            assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (n, m, rank, inverse, got, want)
