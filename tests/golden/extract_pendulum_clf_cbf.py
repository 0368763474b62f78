#!/usr/bin/env python3
"""Record the rows of the reference's pendulum CLF-CBF controller into a small .npz fixture.

Executes the reference's own EnergyCLF, RadialCBFRelDegree2 and RadialCBF (bayes_cbf/pendulum.py:530-746) on its
PendulumDynamicsModel with m = l = 1, g = 10 (for another m l the reference's own `direct` vs `abstract` asserts fire) and
stores A(x), b(x), value(x) of each at 64 states: a 6 x 6 grid over theta in [-pi, pi), omega in [-3, 3]; theta = theta_c
exactly (the hard row's coefficient is then 0: once with b < 0, the infeasible program, once with b > 0); theta = 3 pi / 8,
the boundary of the safe set the nominal run settles on; omega = 0; 20 random states.  The quadratic program itself has no
golden: the reference solves it with cvxopt, which the build container does not have (tests/_pendulum_qp_reference.py).
Only recorded numbers leave this script.
Build-container only:  python tests/golden/extract_pendulum_clf_cbf.py
"""
import math
import os

import numpy as np

import _refenv

HERE = os.path.dirname(os.path.abspath(__file__))


def states():
    th_c = math.pi / 4
    grid = [(th, om) for th in np.linspace(-math.pi, math.pi, 6, endpoint=False) for om in np.linspace(-3.0, 3.0, 6)]
    special = [(th_c, 0.0), (th_c, 1.5), (3 * math.pi / 8, 0.0), (3 * math.pi / 8, -0.5), (3 * math.pi / 8, 0.7),
               (-1.0, 0.0), (0.3, 0.0), (2.0, 0.0)]
    rng = np.random.default_rng(20)
    rand = [(rng.uniform(-math.pi, math.pi), rng.uniform(-3.0, 3.0)) for _ in range(20)]
    X = np.array(grid + special + rand, dtype=np.float64)
    assert X.shape == (64, 2)
    return X


def main():
    torch = _refenv.setup()
    torch.set_default_dtype(torch.float64)
    from bayes_cbf.pendulum import EnergyCLF, PendulumDynamicsModel, RadialCBF, RadialCBFRelDegree2
    mass, gravity, length = 1.0, 10.0, 1.0
    model = PendulumDynamicsModel(m=1, n=2, mass=mass, gravity=gravity, length=length, dtype=torch.float64)
    funcs = dict(clf=EnergyCLF(model), cbf2=RadialCBFRelDegree2(model, dtype=torch.float64),
                 # (RadialCBF hands its angles to torch.cos: they have to be tensors; the values are its defaults)
                 cbf1=RadialCBF(model, cbf_col_delta=torch.tensor(math.pi / 8), cbf_col_theta=torch.tensor(math.pi / 4)))
    X = states()
    out = dict(x=X, model=np.array([mass, gravity, length]), clf_c=np.float64(funcs["clf"].clf_c),
               k_alpha=np.array(funcs["cbf2"].k_alpha, dtype=np.float64), cbf_gamma=np.float64(funcs["cbf1"].cbf_col_gamma),
               theta_c=np.float64(funcs["cbf2"].cbf_col_theta), delta_c=np.float64(funcs["cbf2"].cbf_col_delta))
    assert out["theta_c"] == float(funcs["cbf1"].cbf_col_theta) and out["delta_c"] == float(funcs["cbf1"].cbf_col_delta)
    for name, f in funcs.items():
        A, b, v = [], [], []
        for row in X:
            x = torch.tensor(row, dtype=torch.float64)
            A.append(float(f.A(x).reshape(-1)[0]))
            b.append(float(f.b(x).reshape(-1)[0]))
            v.append(float(f.value(x)))
        out[name + "_A"], out[name + "_b"], out[name + "_value"] = (np.array(a, dtype=np.float64) for a in (A, b, v))
    np.savez_compressed(os.path.join(HERE, "pendulum_clf_cbf_rows.npz"), **out)
    print("pendulum_clf_cbf_rows", {k: (np.shape(v), float(np.min(v)), float(np.max(v))) for k, v in out.items()})


if __name__ == "__main__":
    main()
