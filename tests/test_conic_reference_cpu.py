"""The cone-program helper of the GPU solver tests (tests/_conic_reference.py), checked where no GPU is needed: the bound
rejects what it should, the bound is a bound, the generators are deterministic, and on every case the GPU tests run the numpy
port solves at least 98 % of the programs and stays inside the per-family figures the device tolerances are derived from."""
import numpy as np
import pytest

import _conic_reference as cr
from oracle import socp as osocp

CLF_CASES = ([(m, K, pat, cr.QUAD_BT) for m, K in cr.QUAD_SHAPES for pat in cr.MASKS]
             + [(m, K, "first", cr.WIDE_BT) for m, K in cr.WIDE_SHAPES]
             + [(2, 3, "first", 1), (2, 3, "first", 17), (2, 3, "first", 20)])


def _check_case(family, progs, sols, kept):
    """Left-out share within the cap; multipliers in K; the reference's own figures within REF_WORST of the family."""
    assert (~kept).sum() <= cr.LEFT_OUT_CAP * len(kept), (int((~kept).sum()), len(kept))
    worst_f, worst_g = cr.REF_WORST[family]
    for pr, s in [(pr, s) for pr, s, k in zip(progs, sols, kept) if k]:
        assert cr.z_in_cone_figure(s["z"], pr[4]) <= 1e-12
        f, g = cr.figures(pr, s["z"], s["x"])
        assert f <= worst_f, f
        if worst_g is not None:
            assert g <= worst_g, g        # (g >= 0 holds for a feasible x only; this x may be outside by `f`)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("m,K,pattern,Bt", CLF_CASES)
def test_clf_cbf_cases_reference_solves_and_sets_the_figures(m, K, pattern, Bt, f32):
    _, _, progs, sols, kept = cr.clf_cbf_case(cr.clf_cbf_seed(m, K), Bt, m, K, pattern, f32)
    _check_case("clf_cbf", progs, sols, kept)


@pytest.mark.parametrize("shape", cr.GENERIC_SHAPES + [cr.MIXED_SHAPE], ids=str)
def test_generic_cases_reference_solves_and_sets_the_figures(shape):
    _, progs, sols, kept = cr.generic_case("generic", cr.generic_seed(*shape), cr.CONEQP_BT, *shape)
    _check_case("generic", progs, sols, kept)


@pytest.mark.parametrize("shape", cr.P0_SHAPES, ids=str)
def test_p0_cases_reference_solves_to_small_kkt_residuals(shape):
    _, progs, sols, kept = cr.generic_case("p0", cr.generic_seed(*shape), cr.CONEQP_BT, *shape)
    _check_case("p0", progs, sols, kept)
    for pr, s, k in zip(progs, sols, kept):
        assert not k or cr.p0_reference_is_a_solution(pr, s)


def test_tolerances_follow_the_times_ten_rule_and_the_accept_cap():
    for fam, (f, g) in cr.REF_WORST.items():
        ef, eg = cr.tolerances(fam)
        assert ef == min(10 * f, 1e-7) and (eg is None if g is None else eg == min(10 * g, 1e-7))
        assert ef <= cr.ACCEPT and (eg is None or eg <= cr.ACCEPT)


def _active_case():
    """A generic program whose optimum has an active cone (z large) and the reference's solution of it."""
    _, progs, sols, kept = cr.generic_case("generic", cr.generic_seed(*cr.MIXED_SHAPE), cr.CONEQP_BT, *cr.MIXED_SHAPE)
    for pr, s, k in zip(progs, sols, kept):
        P, q, G, h, dims = pr
        marg = cr.cone_margins(h - G @ s["x"], dims)
        a = int(np.argmin(marg))
        if k and a >= dims["l"] and marg[a] < 1e-8 and np.sort(marg)[1] > 1e-2:      # exactly one active constraint: a cone
            return pr, s, a
    raise AssertionError("no program with a single active cone in the case")


def test_the_check_rejects_a_suboptimal_and_an_infeasible_point_and_accepts_the_solution():
    pr, s, a = _active_case()
    P, q, G, h, dims = pr
    eps_f, eps_g = cr.tolerances("generic")
    x = s["x"]
    f, g = cr.figures(pr, s["z"], x)
    assert f <= eps_f and g <= eps_g
    # 1e-5 along a feasible direction: towards the interior of the active cone (increase its margin) -- stays feasible,
    # but leaves the optimum by 1e-5, which costs |grad f| 1e-5 >> eps_g to first order
    o, e = osocp._blocks(dims)[a - dims["l"]]
    v = (h - G @ x)[o:e]
    gm = -G[o].copy() + (v[1:] / np.linalg.norm(v[1:])) @ G[o + 1:e]       # gradient of the margin v_0 - |v_1:| in x
    inward = gm / np.linalg.norm(gm)
    f_in, g_in = cr.figures(pr, s["z"], x + 1e-5 * inward)
    assert f_in <= eps_f and g_in > eps_g, (f_in, g_in)
    # 1e-5 out of the active cone: the feasibility condition fails
    f_out, _ = cr.figures(pr, s["z"], x - 1e-5 * inward)
    assert f_out > eps_f, f_out


def test_lower_bound_is_a_lower_bound_for_any_multiplier_in_the_cone():
    rng = np.random.default_rng(5)
    _, progs, sols, kept = cr.generic_case("generic", cr.generic_seed(*cr.MIXED_SHAPE), cr.CONEQP_BT, *cr.MIXED_SHAPE)
    for pr, s in list(zip(progs, sols))[:20]:
        P, q, G, h, dims = pr
        fstar = cr.objective(P, q, s["x"])
        assert cr.lower_bound(P, q, G, h, s["z"]) <= fstar + 1e-9 * max(1.0, abs(fstar))
        for _ in range(20):
            z = cr._interior_point(rng, dims["l"], dims["q"]) * 10.0 ** rng.uniform(-3, 2)
            if rng.uniform() < 0.3:                       # boundary points of K too
                z[dims["l"]] = np.linalg.norm(z[dims["l"] + 1:dims["l"] + dims["q"][0]])
            assert cr.lower_bound(P, q, G, h, z) <= fstar + 1e-9 * max(1.0, abs(fstar))


def test_rounding_slack_covers_an_fp32_rounding_of_the_solution():
    """figures(rounded=True) of fp32(x*) stay inside the fp64 tolerances: the widening is large enough, on every program."""
    eps_f, eps_g = cr.tolerances("clf_cbf")
    _, _, progs, sols, kept = cr.clf_cbf_case(cr.clf_cbf_seed(3, 4), cr.QUAD_BT, 3, 4, "first", True)
    plain = 0.0
    for pr, s, k in zip(progs, sols, kept):
        if k:
            y32 = s["x"].astype(np.float32).astype(np.float64)
            f, g = cr.figures(pr, s["z"], y32, rounded=True)
            assert f <= eps_f and g <= eps_g, (f, g)
            plain = max(plain, cr.figures(pr, s["z"], y32)[1])
    assert plain > eps_g           # (and it is needed: unwidened, the rounded points miss the fp64 tolerance)


def test_generators_are_deterministic_under_their_seeds():
    a, b = cr.clf_cbf_family(3, 5, 2, 3), cr.clf_cbf_family(3, 5, 2, 3)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["d"], cr.clf_cbf_family(4, 5, 2, 3)["d"])
    assert set(np.unique(cr.clf_cbf_family(3, 200, 2, 3)["rho"])) == set(cr.RHOS)
    for fam in (cr.generic_family, cr.p0_family):
        a, b = fam(3, 4, 3, 2, [3, 4]), fam(3, 4, 3, 2, [3, 4])
        assert all(np.array_equal(a[k], b[k]) for k in ("P", "q", "G", "h"))
    f32 = cr.clf_cbf_family(3, 5, 2, 3, f32=True)
    assert all(np.array_equal(v, v.astype(np.float32)) for v in f32.values())


def test_generic_form_matches_the_oracle_adapter():
    p = cr.clf_cbf_family(11, 3, 2, 3)
    mask = cr.relax_mask("first", 3)
    for i in range(3):
        ref = osocp.clf_cbf_socp(p["w"][i], p["r"][i], [(p["A"][i, k], p["b"][i, k], p["c"][i, k], p["d"][i, k]) for k in range(3)],
                                 p["rho"][i], mask)
        np.testing.assert_array_equal(cr.solve(cr.clf_cbf_generic_form(p, mask, i))["x"], ref["x"])
