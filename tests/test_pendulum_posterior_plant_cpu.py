"""CPU-side checks of the pendulum's posterior-drawn plant (bcbf_pendulum_control_step_sampled_f64): the numpy restatement of
the draw (_pendulum_posterior_plant_reference) is held to the exact moments of the rel-degree-2 condition as a quadratic
form in the jet posterior; its degenerate cases; the header declares and the library exports the entry, and every bad
argument is refused with BCBF_EINVAL before any HIP call.  Nothing here asserts anything about the gap between the exact
moments and the (mean, var) the program works with (oracle.cbc2.cbc2_terms): that gap is a finding, reported in DESIGN.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _pendulum_posterior_plant_reference as ref
from test_pendulum_cpu import FAKE
from test_pendulum_learning_cpu import _obs_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bcbf_pendulum_control_step_sampled_f64"
DRAWS = 200000


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def model():
    return ref.small_model()


@pytest.fixture(scope="module")
def normals():
    return np.random.default_rng(12345).standard_normal((DRAWS, 2, 4))


# ---------------------------------------------------------------- the draw against the exact quadratic-form moments
@pytest.mark.parametrize("u", [ref.U0, -1.3], ids=["u0", "u_other"])
@pytest.mark.parametrize("x", ref.STATES, ids=lambda x: "x=%g,%g" % x)
def test_draw_statistics_match_exact_moments(model, normals, x, u):
    _, _, mean, S4, (h, gh, Hh) = ref.model_at(model, x)
    m_ex, v_ex = ref.exact_moments(mean, model["A"], S4, u, h, gh, Hh, ref.K_ALPHA)
    _, _, c = ref.cbc2_on(ref.draw(mean, model["A"], S4, normals), u, h, gh, Hh, ref.K_ALPHA)
    se = np.sqrt(v_ex / DRAWS)
    print("x=%s u=%g: draw mean %.4f var %.4f | exact mean %.4f var %.4f" % (x, u, c.mean(), c.var(), m_ex, v_ex))
    assert abs(c.mean() - m_ex) <= 5.0 * se, (c.mean(), m_ex, se)
    assert abs(c.var() - v_ex) <= 0.03 * v_ex, (c.var(), v_ex)


def test_draw_has_the_matrix_variate_covariance(model, normals):
    _, _, mean, S4, _ = ref.model_at(model, ref.STATES[0])
    S = ref.draw(mean, model["A"], S4, normals).reshape(DRAWS, 8)
    K = np.kron(model["A"], S4)
    np.testing.assert_allclose(np.cov(S.T), K, atol=0.02 * np.abs(K).max())


# ---------------------------------------------------------------- degenerate cases
@pytest.mark.parametrize("how", ["no_gp", "s2=0"])
def test_no_variance_gives_exactly_the_programs_mean(model, how):
    """Without a GP (or with s2 = 0) any z gives mean_A u + mean_b of cbc2_terms: Sigma4 = 0 and the cross term tr C = 0."""
    from oracle import cbc2 as oc2
    from _pendulum_oracle import barrier, pendulum_fg
    rng = np.random.default_rng(5)
    for x in ref.STATES:
        x = np.asarray(x)
        f, g, J = pendulum_fg(x, 1.2, 9.0, 0.9)
        jets = dict(Mk=np.stack([f, g], axis=1), dMk=np.zeros((2, 2, 2)), Bk=np.zeros((2, 2)), G10=np.zeros((2, 2, 2)),
                    G11=np.zeros((2, 2, 2, 2)))
        for i in range(2):
            jets["dMk"][i][:, 0] = J[:, i]
        h, gh, Hh = barrier(x)
        (mA, mb), _, _, var = oc2.cbc2_terms(jets, model["A"], model["Bm"], model["ell"], 0.0, h, gh, Hh, np.array(ref.K_ALPHA),
                                             np.array([ref.U0]))
        assert var == 0.0
        ws = ref.workspace_from_jets(jets, 0.0, model["Bm"])
        S4 = ref.jet_covariance(ws["Bk"], ws["G"], model["ell"], 0.0 if how == "s2=0" else 1.5, model["Bm"][0, 0], 1.0,
                                gp=how == "s2=0")
        assert np.all(S4 == 0.0)
        for u in (ref.U0, -2.0):
            S = ref.draw(ref.jet_mean(ws["Mk"], ws["Mj"]), model["A"], S4, rng.standard_normal((7, 2, 4)))
            _, _, c = ref.cbc2_on(S, u, h, gh, Hh, ref.K_ALPHA)
            np.testing.assert_allclose(c, np.full(7, mA[0] * u + mb), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("kernel", sorted(ref.KXX))
def test_prior_mode_covariance_is_the_closed_form(model, normals, kernel):
    """A regressor with no data: Bk = s2 Bm, G = 0, so Sigma4 = blockdiag(s2 Bm, kxx s2 Bm00 diag(1/ell^2))."""
    s2, Bm, ell = model["s2"], model["Bm"], model["ell"]
    S4 = ref.jet_covariance(s2 * Bm, np.zeros((6, 6)), ell, s2, Bm[0, 0], ref.KXX[kernel])
    want = np.zeros((4, 4))
    want[:2, :2] = s2 * Bm
    want[2, 2], want[3, 3] = (ref.KXX[kernel] * s2 * Bm[0, 0] / ell[d] ** 2 for d in range(2))
    np.testing.assert_allclose(S4, want, rtol=1e-15, atol=0)
    from _pendulum_oracle import barrier
    h, gh, Hh = barrier(np.asarray(ref.STATES[1]))
    mean = np.array([[0.45, 0.0, 0.0, 1.0], [-9.0, 1.0, -3.0, 0.0]])
    m_ex, v_ex = ref.exact_moments(mean, model["A"], S4, ref.U0, h, gh, Hh, ref.K_ALPHA)
    _, _, c = ref.cbc2_on(ref.draw(mean, model["A"], S4, normals), ref.U0, h, gh, Hh, ref.K_ALPHA)
    assert abs(c.mean() - m_ex) <= 5.0 * np.sqrt(v_ex / DRAWS) and abs(c.var() - v_ex) <= 0.03 * v_ex


def test_semidefinite_factors_keep_the_draw_finite_and_in_range(normals):
    A = np.array([[4.0, 2.0], [2.0, 1.0]])                     # rank 1: range span{(2, 1)}, null direction (1, -2)
    B = np.array([[1.0, 0.0], [2.0, 1.0], [0.0, 3.0], [1.0, 1.0]])
    S4 = B @ B.T                                               # rank 2, exactly representable
    null = np.linalg.svd(S4)[0][:, 2:]                         # its null space
    assert np.abs(S4 @ null).max() < 1e-13
    LA, LS = ref.psd_chol(A), ref.psd_chol(S4)
    assert LA[1, 1] == 0.0 and np.all(LS[:, 2:] == 0.0), "a pivot <= 0 zeroes its column"
    np.testing.assert_allclose(LA @ LA.T, A, atol=1e-15)
    np.testing.assert_allclose(LS @ LS.T, S4, atol=1e-14)
    mean = np.arange(8.0).reshape(2, 4)
    D = ref.draw(mean, A, S4, normals[:1000]) - mean
    assert np.isfinite(D).all()
    assert np.abs(D[:, 0, :] - 2.0 * D[:, 1, :]).max() < 1e-12, "rows stay in the range of A"
    assert np.abs(D @ null).max() < 1e-12, "columns stay in the range of Sigma4"
    D0 = ref.draw(mean, np.array([[1.0, 0.0], [0.0, 0.0]]), S4, normals[:1000]) - mean
    assert np.all(D0[:, 1, :] == 0.0) and np.abs(D0[:, 0, :]).max() > 0.1, "a null direction of A receives no draw"


# ---------------------------------------------------------------- the C entry
def test_header_declares_and_library_exports_sampled_entry(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert NAME in declared and NAME in exported and NAME in lib.declared_symbols()


def test_sampled_plant_kernel_is_under_the_scratch_guard():
    """The kernel must use no scratch memory: the build reads its resource remark and fails otherwise."""
    from bayesian_cbf_amd import build
    assert any("pendulum_sampled_plant_kernel" in k for k in build.ZERO_SCRATCH_KERNELS["pendulum.hip"])
    assert "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["pendulum.hip"]


def _sampled_args(**over):
    """The observe entry's Bt = 0 argument list with the sampled entry's additions spliced in before Bt: z, xdot_s, cbc_s,
    relaxed, viol_relaxed, rho_tol."""
    extra = dict(z=FAKE, xdot_s=FAKE, cbc_s=FAKE, relaxed=FAKE, viol_relaxed=FAKE, rho_tol=1e-6)
    rest = {k: v for k, v in over.items() if k not in extra}
    extra.update({k: v for k, v in over.items() if k in extra})
    a = _obs_args(**rest)
    return a[:-6] + list(extra.values()) + a[-6:]


def test_sampled_entry_valid_arguments_pass_the_checks(lib):
    fn = getattr(lib.lib, NAME)
    assert fn(*_sampled_args()) == 0
    assert fn(*_sampled_args(xdot_s=None, cbc_s=None, relaxed=None, viol_relaxed=None, rho_tol=0.0)) == 0
    assert fn(*_sampled_args(Lop=None, Vw=None, X=None, UHB=None, N=0, prior=1)) == 0           # prior mode
    assert fn(*_sampled_args(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0, prior=0)) == 0  # no-GP mode
    assert fn(*_sampled_args(explore=None, ctrl_range=None, obs_x=None, obs_uh=None, obs_y=None, obs_ld=0)) == 0


BAD = [dict(z=None), dict(relaxed=None), dict(viol_relaxed=None), dict(rho_tol=-1e-9), dict(rho_tol=float("nan")),
       # everything the observing entry refuses
       dict(obs_x=None), dict(obs_ld=0), dict(ctrl_range=None), dict(u_ref_in=FAKE), dict(eps=float("nan")), dict(eps=1.5),
       dict(ctrl_range=(ctypes.c_double * 2)(2.0, 1.0)), dict(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0, prior=1),
       dict(prior=2), dict(mean_mass=0.0),
       # ... and the plain entry
       dict(n=3), dict(m=2), dict(x=None), dict(A=None), dict(kalpha=None), dict(Mk=None), dict(G=None), dict(y=None),
       dict(min_h=None), dict(Vw=None), dict(shared=2), dict(kernel_kind=3), dict(hessian_mode=2), dict(max_iters=0),
       dict(dt=0.0), dict(R=0.0), dict(true_mass=0.0), dict(safety_factor=-1.0), dict(Bt=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % (k, v if not isinstance(v, ctypes.Array) else list(v))
                                                          for k, v in d.items()))
def test_sampled_entry_refuses_bad_arguments(lib, bad):
    lib.lib.bcbf_pendulum_plant_step_f64(None, None, 1.0, 1.0, 1.0, 1.0, 0, None)        # leaves another call's message behind
    other = lib.lib.bcbf_last_error()
    assert getattr(lib.lib, NAME)(*_sampled_args(**bad)) == -1
    msg = lib.lib.bcbf_last_error()
    assert msg and msg != other and b"pendulum_control_step" in msg
