#!/usr/bin/env python3
"""Record the rows of the reference's mean-model unicycle controller (ControllerCLF) into a small .npz fixture.

Executes the reference's own cartesian2polar / polar2cartesian, CLFPolar, PolarDynamics and ControllerCLF._clc / _cbcs
(bayes_cbf/unicycle_move_to_pose.py:82-167, 442-497, 731-752) at 64 states: a 4 x 4 position grid x 3 headings around the
standard start / goal pair; states on the boundary of an obstacle and inside it; states near the goal (rho ~ 1e-3 and 1e-2);
8 random states.  Two controllers:
  polar      ControllerCLF(NoPlanner(goal), cartesian2polar, PolarDynamics(), CLFPolar(Kp)), no obstacles;
  cartesian  ControllerCLF(PiecewiseLinearPlanner(start, goal, 200, 0.05), identity, CartesianDynamics(), CLFCartesian(Kp),
             the two mid obstacles with term weights (0.7, 0.3), gammas 5) at t in {0, 7, 150, 195}.
(bfa, b) of every row is stored as the controller returns it.  The gains are float64 tensors (the classes' defaults are
float32 and would round them); the polar gains carry a non-zero fourth one so that its terms are held too.  The quadratic
program itself has no golden: the reference solves it with GUROBI through cvxpy, which the build container does not have
(tests/_unicycle_qp_reference.py).  Only recorded numbers leave this script.
Build-container only:  python tests/golden/extract_unicycle_clf_qp.py
"""
import math
import os

import numpy as np

import _refenv

HERE = os.path.dirname(os.path.abspath(__file__))
START, GOAL = (-3.0, -1.0, -math.pi / 4), (0.0, 0.0, math.pi / 4)
KP_POLAR, KP_CART = (0.6, 1.5, 4.0, 0.3), (0.9, 1.5, 4.0)
TW, GAMMAS, T_STEPS = (0.7, 0.3), (5.0, 5.0), (0, 7, 150, 195)


def states(centers, radii):
    grid = [(x, y, th) for x in np.linspace(-3.5, 0.5, 4) for y in np.linspace(-2.0, 1.0, 4)
            for th in (-math.pi / 4, 0.6, 2.5)]
    c, r = centers[0], radii[0]
    special = [(c[0] + r, c[1], 0.3), (c[0], c[1] - r, -1.0),                       # on the boundary of obstacle 0
               (c[0] + 0.3 * r, c[1] - 0.2 * r, 1.0), (centers[1][0] - 0.5 * radii[1], centers[1][1], -2.0)]   # inside
    near = [(GOAL[0] - 1e-3 * math.cos(0.4), GOAL[1] - 1e-3 * math.sin(0.4), 0.5), (GOAL[0] + 1e-3, GOAL[1], 2.0),
            (GOAL[0] - 1e-2 * math.cos(-1.0), GOAL[1] - 1e-2 * math.sin(-1.0), 0.9), (GOAL[0], GOAL[1] + 1e-2, -0.7)]
    rng = np.random.default_rng(21)
    rand = [(rng.uniform(-4.0, 1.0), rng.uniform(-2.5, 1.5), rng.uniform(-math.pi, math.pi)) for _ in range(8)]
    X = np.array(grid + special + near + rand, dtype=np.float64)
    assert X.shape == (64, 3)
    return X


class _NoLog:
    def add_scalar(self, *a, **k):
        pass


def main():
    torch = _refenv.setup()
    torch.set_default_dtype(torch.float64)
    import bayes_cbf.unicycle_move_to_pose as ref
    from bayes_cbf.planner import PiecewiseLinearPlanner
    ref.TBLOG = _NoLog()
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)
    start, goal = t64(START), t64(GOAL)
    obs = ref.obstacles_at_mid_from_start_and_goal(start, goal, term_weights=list(TW))
    centers = np.array([o.center.numpy() for o in obs])
    radii = np.array([float(o.radius) for o in obs])
    X = states(centers, radii)
    out = dict(x=X, start=np.array(START), goal=np.array(GOAL), Kp_polar=np.array(KP_POLAR), Kp_cart=np.array(KP_CART),
               tw=np.array(TW), gammas=np.array(GAMMAS), t_steps=np.array(T_STEPS), centers=centers, radii=radii,
               numStepsPlan=np.int64(200), dt=np.float64(0.05))

    clf = ref.CLFPolar(Kp=t64(KP_POLAR))
    dyn = ref.PolarDynamics()
    ctrl = ref.ControllerCLF(ref.NoPlanner(goal), coordinate_converter=ref.cartesian2polar, dynamics=dyn, clf=clf)
    out["clf_gamma"], out["clf_relax_weight"] = np.float64(ctrl.clf_gamma), np.float64(ctrl.clf_relax_weight)
    rec = {k: [] for k in ("polar", "polar_back", "polar_terms", "polar_grad", "polar_g", "polar_bfa", "polar_b")}
    for row in X:
        x = t64(row)
        pol = ref.cartesian2polar(x, goal)
        rec["polar"].append(pol.numpy())
        rec["polar_back"].append(ref.polar2cartesian(pol, goal).numpy())
        rec["polar_terms"].append(clf.clf_terms(pol, goal).numpy())
        rec["polar_grad"].append(clf.grad_clf(pol, goal).numpy())
        rec["polar_g"].append(dyn.g_func(pol).numpy())
        bfa, b = ctrl._clc(x, goal, 0)
        rec["polar_bfa"].append(np.asarray(bfa))
        rec["polar_b"].append(float(b))
    out.update({k: np.array(v, dtype=np.float64) for k, v in rec.items()})

    planner = PiecewiseLinearPlanner(start, goal, 200, 0.05)
    ctrl = ref.ControllerCLF(planner, coordinate_converter=lambda x, xg: x, dynamics=ref.CartesianDynamics(),
                             clf=ref.CLFCartesian(Kp=t64(KP_CART)), cbfs=obs, cbf_gammas=list(GAMMAS))
    plan, dplan, bfa_all, b_all = [], [], [], []
    for t in T_STEPS:
        sg = planner.plan(t)
        plan.append(sg.numpy())
        dplan.append(planner.dot_plan(t).numpy())
        bfa_t, b_t = [], []
        for row in X:
            x = t64(row)
            rows = [ctrl._clc(x, sg, t)] + list(ctrl._cbcs(x, sg, t))
            bfa_t.append([np.asarray(r[0]) for r in rows])
            b_t.append([float(r[1]) for r in rows])
        bfa_all.append(bfa_t)
        b_all.append(b_t)
    out.update(cart_plan=np.array(plan), cart_dot_plan=np.array(dplan), cart_bfa=np.array(bfa_all, dtype=np.float64),
               cart_b=np.array(b_all, dtype=np.float64))                       # [4,64,3,2], [4,64,3]
    np.savez_compressed(os.path.join(HERE, "unicycle_clf_qp_rows.npz"), **out)
    print("unicycle_clf_qp_rows", {k: (np.shape(v), float(np.min(v)), float(np.max(v))) for k, v in out.items()})


if __name__ == "__main__":
    main()
