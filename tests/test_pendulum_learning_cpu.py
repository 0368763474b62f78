"""CPU-side checks of the pendulum's online-learning loop (bcbf_pendulum_control_step_observe_f64,
rollouts.pendulum_learning_rollouts): the header declares and the library exports the entry, every bad combination of its
new arguments is refused with BCBF_EINVAL before any HIP call, and the loop's refit schedule is the one the host façade's
learner (OnlineLearner.observe under MeanAdjustedModel) follows."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from test_pendulum_cpu import FAKE, _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bcbf_pendulum_control_step_observe_f64"


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_header_declares_and_library_exports_observe_entry(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert NAME in declared and NAME in exported and NAME in lib.declared_symbols()


RANGE = (ctypes.c_double * 2)(-15.0, 15.0)


def _obs_args(**over):
    """The plain entry's Bt = 0 argument list (test_pendulum_cpu._args) with the observe entry's additions spliced in
    before Bt: prior, explore, eps, ctrl_range, obs_x, obs_uh, obs_y, obs_ld."""
    extra = dict(prior=0, explore=FAKE, eps=0.5, ctrl_range=RANGE, obs_x=FAKE, obs_uh=FAKE, obs_y=FAKE, obs_ld=250)
    plain = {k: v for k, v in over.items() if k not in extra}
    for k, v in over.items():
        if k in extra:
            extra[k] = v
    a = _args(**plain)
    # _args returns [... fails, Bt, n, m, ev_start, ev_stop, stream]
    return a[:-6] + list(extra.values()) + a[-6:]


def test_observe_entry_valid_arguments_pass_the_checks(lib):
    fn = lib.lib.bcbf_pendulum_control_step_observe_f64
    assert fn(*_obs_args()) == 0
    assert fn(*_obs_args(Lop=None, Vw=None, X=None, UHB=None, N=0, prior=1)) == 0           # prior mode
    assert fn(*_obs_args(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0, prior=0)) == 0  # no-GP mode
    assert fn(*_obs_args(explore=None, ctrl_range=None, obs_x=None, obs_uh=None, obs_y=None, obs_ld=0)) == 0
    assert fn(*_obs_args(explore=None, u_ref_in=FAKE)) == 0                                 # clip a caller's u_ref
    assert fn(*_obs_args(eps=0.0)) == 0 and fn(*_obs_args(eps=1.0)) == 0


BAD = [dict(obs_x=None), dict(obs_uh=None), dict(obs_y=None), dict(obs_x=None, obs_uh=None), dict(obs_ld=0),
       dict(obs_ld=-3), dict(ctrl_range=None), dict(u_ref_in=FAKE), dict(eps=float("nan")), dict(eps=-0.1),
       dict(eps=1.5), dict(ctrl_range=(ctypes.c_double * 2)(2.0, 1.0)),
       dict(ctrl_range=(ctypes.c_double * 2)(float("nan"), 1.0)),
       dict(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0, prior=1), dict(prior=2), dict(dt=0.0), dict(dt=-1.0),
       dict(mean_mass=0.0), dict(Bt=-1), dict(x=None)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % (k, v if not isinstance(v, ctypes.Array) else list(v))
                                                          for k, v in d.items()))
def test_observe_entry_refuses_bad_arguments(lib, bad):
    assert lib.lib.bcbf_pendulum_control_step_observe_f64(*_obs_args(**bad)) == -1
    assert lib.lib.bcbf_last_error()


class _StubRegressor:
    def __init__(self, log, learner_ref, state):
        self.log, self.learner_ref, self.state = log, learner_ref, state

    def fit(self, X, U, Y, training_iter=0):
        ln = self.learner_ref[0]
        self.log.append((self.state["t"], len(ln.Xtrain) - 1, self.state.pop("wr", False)))
        assert X.shape[0] == min(len(ln.Xtrain) - 1, ln.max_train)


def _facade_schedule(numSteps, train_every, max_train):
    """OnlineLearner.observe as MeanAdjustedModel drives it (subsample = randint WITH replacement), one call per step."""
    from bayesian_cbf_amd.online import OnlineLearner
    log, ref, state = [], [None], {}

    def subsample(count, k):
        state["wr"] = True
        return torch.randint(count, (k,))
    ln = OnlineLearner(_StubRegressor(log, ref, state), lambda X, U, Xd: Xd, 0.002, train_every, max_train, 0, subsample,
                       enable_learning=True)
    ref[0] = ln
    for t in range(numSteps):
        state["t"] = t
        ln.observe(torch.tensor([0.1 * t, -0.2 * t], dtype=torch.float64), torch.tensor([0.3 * t], dtype=torch.float64))
    return log


@pytest.mark.parametrize("cfg", [(250, 10, 200), (40, 10, 24), (12, 1, 5)])
def test_refit_schedule_equals_facade_learner(lib, cfg):
    from bayesian_cbf_amd.rollouts import pendulum_learning_schedule
    got = pendulum_learning_schedule(*cfg)
    want = _facade_schedule(*cfg)
    assert got == want
    numSteps, train_every, max_train = cfg
    assert got and any(wr for _, _, wr in got) and not all(wr for _, _, wr in got)
    sizes = [min(c, max_train) for _, c, _ in got]
    assert sizes == sorted(sizes) and sizes[-1] == max_train
