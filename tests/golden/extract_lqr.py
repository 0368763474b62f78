#!/usr/bin/env python3
"""Record the reference's LQR nominal controller into a small .npz fixture (tests/golden/lqr_nominal.npz).

The reference's LQRController.control (bayes_cbf/controllers.py:64-115) needs two things the build container does not have:
`torch.solve` (removed from torch) and the external package `bdlqr`.  This script installs its own stand-ins for both --
torch.solve(B, A) -> (torch.linalg.solve(A, B), None), and a `bdlqr.lqr.LinearSystem` whose solve() iterates the
reference's OWN affine_backpropagation (bayes_cbf/ilqr.py:43-76) T times from (Q_T, s_T) and returns -K x - k -- then runs
the reference's code unchanged.  No parity with bdlqr's own iterates is claimed.  Recorded:
  (a) the recursion alone: random (A, B, Q, R, s) at (n, m) in {(2,1), (3,2), (4,3)}, T in {1, 2, 3, 64} -> P, o, K, k;
  (b) LQRController.control on PendulumDynamicsModel(mass 1, gravity 10, length 1) at 32 states, (numSteps, t, dt) in
      {(1,0,.01), (2,0,.01), (250,3,.002), (1000,0,.001)}: u and the (A, B, T) handed to the stand-in in BOTH passes;
  (c) the same through a control-affine model whose g depends on x (g = [0.1 sin theta, 1 + 0.2 omega]'), so that the second
      linearisation differs from the first.
Only recorded numbers leave this script.
Build-container only:  python tests/golden/extract_lqr.py
"""
import math
import os
import sys
import types

import numpy as np

import _refenv

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [(1, 0, 0.01), (2, 0, 0.01), (250, 3, 0.002), (1000, 0, 0.001)]
X_GOAL = [0.3, -0.2]
Q_COST = [[2.0, 0.3], [0.3, 1.0]]
R_COST = [[0.5]]


def states():
    X = np.array([(th, om) for th in np.linspace(-math.pi, math.pi, 8, endpoint=False) for om in np.linspace(-3.0, 3.0, 4)])
    assert X.shape == (32, 2)
    return X


def main():
    torch = _refenv.setup()
    torch.set_default_dtype(torch.float64)
    torch.solve = lambda B, A: (torch.linalg.solve(A, B), None)
    from bayes_cbf.ilqr import affine_backpropagation
    calls = []

    class LinearSystem:
        def __init__(self, A, B, Q, R, s, Q_T, s_T, z, T):
            self.a = [torch.as_tensor(np.asarray(v, dtype=np.float64)) for v in (Q, s, R, z, A, B)]
            self.P, self.o, self.T = torch.as_tensor(np.asarray(Q_T, dtype=np.float64)), torch.as_tensor(np.asarray(s_T, dtype=np.float64)), int(T)
            calls.append((np.array(A, dtype=np.float64), np.array(B, dtype=np.float64), int(T)))

        def solve(self, x, steps):
            assert steps == 1 and self.T >= 1
            P, o = self.P, self.o
            for _ in range(self.T):
                P, o, K, k = affine_backpropagation(*self.a, P, o)
            return None, [(-K @ torch.as_tensor(x) - k).numpy()]

    lqr_mod = types.ModuleType("bdlqr.lqr")
    lqr_mod.LinearSystem = LinearSystem
    pkg = types.ModuleType("bdlqr")
    pkg.lqr = lqr_mod
    sys.modules["bdlqr"], sys.modules["bdlqr.lqr"] = pkg, lqr_mod
    from bayes_cbf.controllers import LQRController
    from bayes_cbf.pendulum import PendulumDynamicsModel

    out = {}
    # (a) the recursion alone
    rng = np.random.default_rng(64115)
    for n, m in ((2, 1), (3, 2), (4, 3)):
        A = np.eye(n) + 0.2 * rng.standard_normal((n, n))
        B = 0.5 * rng.standard_normal((n, m))
        Mq, Mr = rng.standard_normal((n, n)), rng.standard_normal((m, m))
        Q, R, s = Mq @ Mq.T + np.eye(n), Mr @ Mr.T + np.eye(m), rng.standard_normal(n)
        tag = "a_%d%d_" % (n, m)
        out.update({tag + "A": A, tag + "B": B, tag + "Q": Q, tag + "R": R, tag + "s": s})
        tt = [torch.as_tensor(v) for v in (Q, s, R, np.zeros(m), A, B)]
        for T in (1, 2, 3, 64):
            P, o = tt[0], tt[1]
            for _ in range(T):
                P, o, K, k = affine_backpropagation(*tt, P, o)
            out.update({"%sT%d_%s" % (tag, T, nm): v.numpy() for nm, v in (("P", P), ("o", o), ("K", K), ("k", k))})

    # (b), (c) LQRController.control
    class XDependentG:
        """the pendulum's f with an input matrix that depends on the state"""
        def f_func(self, X):
            return torch.cat([X[..., 1:2], -10.0 * torch.sin(X[..., 0:1])], axis=-1)

        def g_func(self, X):
            return torch.stack([0.1 * torch.sin(X[..., 0]), 1.0 + 0.2 * X[..., 1]], dim=-1).unsqueeze(-1)

    X = states()
    out.update(x=X, x_goal=np.array(X_GOAL), Q=np.array(Q_COST), R=np.array(R_COST), configs=np.array(CONFIGS, dtype=np.float64),
               b_model=np.array([1.0, 10.0, 1.0]))
    models = dict(b=PendulumDynamicsModel(m=1, n=2, mass=1.0, gravity=10.0, length=1.0, dtype=torch.float64), c=XDependentG())
    for tag, model in models.items():
        for ci, (numSteps, t, dt) in enumerate(CONFIGS):
            ctrl = LQRController(model, torch.tensor(Q_COST), torch.tensor(R_COST), torch.tensor(X_GOAL), numSteps, dt, None)
            U, A1, A2, Bs = [], [], [], []
            for row in X:
                del calls[:]
                U.append(ctrl.control(torch.tensor(row), t=t).numpy())
                assert len(calls) == 2 and calls[0][2] == calls[1][2] == numSteps - t
                A1.append(calls[0][0]); A2.append(calls[1][0]); Bs.append(calls[0][1])
                assert np.array_equal(calls[0][1], calls[1][1])
            pre = "%s_c%d_" % (tag, ci)
            out.update({pre + "u": np.array(U), pre + "A1": np.array(A1), pre + "A2": np.array(A2), pre + "B": np.array(Bs),
                        pre + "T": np.int64(numSteps - t)})
    np.savez_compressed(os.path.join(HERE, "lqr_nominal.npz"), **out)
    print("lqr_nominal: %d arrays; |u| <= %.3g" % (len(out), max(np.abs(v).max() for k, v in out.items() if k.endswith("_u"))))


if __name__ == "__main__":
    main()
