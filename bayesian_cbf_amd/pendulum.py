"""Mirror of the hot-path pieces of bayes_cbf/pendulum.py: the ground-truth pendulum model (:82-130) and the
rel-degree-2 radial barrier (:643-696) whose condition `cbc(u)` goes through the jet kernel + closed-form terms
(`cbc2.RelDeg2Safety`).  Controllers / plotting of the reference module are out of scope."""
import math

import torch

from .cbc2 import RelDeg2Safety


class PendulumDynamicsModel:
    """theta'' = -(g/l) sin(theta) + u / (m l):  f(x) = [omega, -(g/l) sin theta],  g(x) = [0, 1/(m l)]'  (:106-130)."""
    ground_truth = True

    def __init__(self, m=1, n=2, mass=1, gravity=10, length=1, deterministic=True, model_noise=0,
                 dtype=torch.get_default_dtype()):
        self.m, self.n, self.mass, self.gravity, self.length, self.dtype = m, n, mass, gravity, length, dtype

    def to(self, dtype):
        self.dtype = dtype

    @property
    def ctrl_size(self):
        return self.m

    @property
    def state_size(self):
        return self.n

    def f_func(self, X):
        theta, omega = X[..., 0:1], X[..., 1:2]
        return torch.cat([omega, -(self.gravity / self.length) * torch.sin(theta)], dim=-1)

    def g_func(self, x):
        gx = torch.tensor([[0.0], [1.0 / (self.mass * self.length)]], dtype=x.dtype, device=x.device)
        return gx.expand(*x.shape[:-1], 2, 1).clone() if x.ndim >= 2 else gx

    def F_func(self, X):
        return torch.cat([self.f_func(X).unsqueeze(-1), self.g_func(X)], dim=-1)

    # the plant protocol of sampling.DynamicsModel (sampling.py:32-47); the reference's pendulum loop
    # (`sampling_pendulum`, :164-233) inlines the same Euler update and theta wrap
    def set_init_state(self, x0):
        self.current_state = x0.clone()

    def step(self, u, dt):
        x = self.current_state
        xdot = self.f_func(x) + (self.g_func(x) @ u.to(x).unsqueeze(-1)).squeeze(-1)
        xn = x + xdot * dt
        xn[..., 0] = ((xn[..., 0] + math.pi) % (2 * math.pi)) - math.pi
        self.current_state = xn
        return dict(xdot=xdot, x=xn)


class RadialCBFRelDegree2(RelDeg2Safety):
    """h(x) = cos(delta_col) - cos(theta - theta_c)  (:675-696): keep the pendulum out of a cone around theta_c."""

    def __init__(self, model, cbf_col_gamma=1, _k_alpha=(1.0, 3.0), cbf_col_delta=math.pi / 8,
                 cbf_col_theta=math.pi / 4, theta_c=math.pi / 4, gamma_col=1, max_unsafe_prob=0.01,
                 delta_col=math.pi / 8, name="cbf-r2", dtype=torch.get_default_dtype()):
        self._model, self._max_unsafe_prob, self._k_alpha = model, max_unsafe_prob, list(_k_alpha)
        self.cbf_col_delta, self.cbf_col_theta, self.name, self.dtype = cbf_col_delta, cbf_col_theta, name, dtype

    k_alpha = property(lambda self: self._k_alpha)
    model = property(lambda self: self._model)
    max_unsafe_prob = property(lambda self: self._max_unsafe_prob)

    def cbf(self, x):
        return math.cos(self.cbf_col_delta) - torch.cos(x[..., 0] - self.cbf_col_theta)

    value = cbf

    def grad_cbf(self, X_in):
        X = X_in.unsqueeze(0) if X_in.ndim == 1 else X_in
        g = torch.cat((torch.sin(X[:, 0:1] - self.cbf_col_theta), X.new_zeros(X.shape[0], 1)), dim=-1)
        return g.squeeze(0) if X_in.ndim == 1 else g

    def hess_cbf(self, x):
        """d grad_cbf / dx (what GradientGP differentiates through, gp_algebra.py:340-345)."""
        H = x.new_zeros(2, 2)
        H[0, 0] = torch.cos(x[0] - self.cbf_col_theta)
        return H


# ----------------------------------------------------------------------------------------------------------------
# The learning demo of BASELINE configs[0]: pendulum.learn_dynamics_matrix_vector (pendulum.py:1052-1271).  Data come
# from one simulated trajectory under a randomised controller; both regressors are fitted on a random subset, evaluated
# on a 20 x 20 (theta, omega) grid with `custom_predict_fullmat`, logged in the reference's tags, and compared with the
# variance-weighted error of `measure_batch_error`.  Plotting is out of scope.
class ControlTrivial:
    """u = m g sin(theta)  (pendulum.py:55-66)."""
    needs_ground_truth = True

    def __init__(self, m=1, mass=None, length=None, gravity=None, dt=None, true_model=None):
        self.m, self.mass, self.length, self.gravity = m, mass, length, gravity

    def control(self, xi, t=None):
        return (self.mass * self.gravity * torch.sin(xi[0])).reshape(1)


class ControlRandom:
    """ControlTrivial scaled by U[0.6, 1.4)  (pendulum.py:69-78)."""
    needs_ground_truth = True

    def __init__(self, **kwargs):
        self.control_trivial = ControlTrivial(**kwargs)

    def control(self, xi, t=None):
        return self.control_trivial.control(xi, t=t) * (torch.rand(1) * 0.8 + 0.60).to(xi)


def sampling_pendulum(dynamics_model, numSteps, controller=None, x0=None, dt=0.01, plot_every_n_steps=20, axs=None,
                      visualizer=None, visualizer_class=None, plotfile=None):
    """pendulum.py:164-233: numSteps controller calls along one explicit-Euler trajectory (theta wrapped to [-pi, pi) by
    the plant's `step`), through the rollout harness of `sampling.sample_generator_trajectory`.  Returns
    (damage %, time[numSteps], theta[numSteps], omega[numSteps], u[numSteps]); damage = share of steps with
    0 < theta < pi/4.  Plotting visualizers are out of scope: the default shows nothing."""
    from .sampling import sample_generator_trajectory, VisualizerZ
    assert controller is not None, "Surprise !! Changed interface to make controller a required argument"
    if visualizer is None:
        visualizer = visualizer_class(plotfile=plotfile, plot_every_n_steps=plot_every_n_steps) if visualizer_class else VisualizerZ()
    x0 = torch.as_tensor(x0, dtype=torch.float64)
    _, X, U = sample_generator_trajectory(dynamics_model, numSteps, dt=dt, x0=x0, controller=controller, visualizer=visualizer)
    theta_vec, omega_vec, u_vec = X[:numSteps, 0], X[:numSteps, 1], U[:, 0]
    assert torch.all((theta_vec <= math.pi) & (-math.pi <= theta_vec))
    damage = ((0 < theta_vec) & (theta_vec < math.pi / 4)).double().sum() * 100 / numSteps
    return damage, dt * torch.arange(numSteps, dtype=torch.float64), theta_vec, omega_vec, u_vec


def sampling_pendulum_data(dynamics_model, D=100, dt=0.01, **kwargs):
    """(dX[D,2], X[D+1,2], U[D+1,1]) with dX the finite differences of the (wrapped) states, pendulum.py:236-252."""
    _, _, theta_vec, omega_vec, u_vec = sampling_pendulum(dynamics_model, numSteps=D + 1, dt=dt, **kwargs)
    X = torch.stack((theta_vec, omega_vec), dim=1)
    U = u_vec.reshape(-1, 1)
    dX = (X[1:] - X[:-1]) / dt
    return dX, X, U


def get_grid_from_Xtrain(Xtrain):
    """20 x 20 grid over the training range (pendulum.py:421-428); [2, 20, 20] like np.mgrid."""
    import numpy as np
    th = slice(Xtrain[:, 0].min(), Xtrain[:, 0].max(), (Xtrain[:, 0].max() - Xtrain[:, 0].min()) / 20)
    om = slice(Xtrain[:, 1].min(), Xtrain[:, 1].max(), (Xtrain[:, 1].max() - Xtrain[:, 1].min()) / 20)
    return np.mgrid[th, om]


def measure_batch_error(FX_learned, var_FX, FX_true):
    """sqrt(mean_b (F - F^)' var_b^-1 (F - F^))  (pendulum.py:1091-1103)."""
    N, D = FX_learned.shape
    assert FX_true.shape == (N, D) and var_FX.shape == (N, D, D)
    diff = (FX_true - FX_learned).unsqueeze(-1).double().cpu()           # an evaluation metric: tiny systems, host side
    errors = diff.transpose(-2, -1) @ torch.linalg.solve(var_FX.double().cpu(), diff)
    assert bool((errors > 0).all())
    return float(torch.sqrt(errors.sum() / N))


def log_learned_model(Xtrain, model, true_f_func, key="Fx", logger=None):
    """Evaluate the model on the grid and log (Xtrain, grid, FX_learned, var_FX, FX_true) (pendulum.py:450-475);
    returns the logged arrays."""
    import numpy as np
    grid = get_grid_from_Xtrain(Xtrain)
    _, N_, M_ = grid.shape
    n, m = model.x_dim, model.u_dim
    Xtest = torch.as_tensor(grid.transpose(1, 2, 0).reshape(-1, 2), dtype=model.dtype, device=model.device)
    FX_learned, var_FX = model.custom_predict_fullmat(Xtest)
    assert FX_learned.shape == (N_ * M_ * (1 + m) * n,)
    assert not torch.isnan(FX_learned).any() and not torch.isnan(var_FX).any()
    FX_true = true_f_func(Xtest).transpose(-1, -2)                       # (b, 1+m, n)
    out = dict(Xtrain=np.asarray(Xtrain), theta_omega_grid=grid,
               FX_learned=FX_learned.reshape(N_, M_, 1 + m, n).cpu().numpy(),
               var_FX=var_FX.reshape(N_, M_, 1 + m, n, N_, M_, 1 + m, n).cpu().numpy(),
               FX_true=FX_true.reshape(N_, M_, 1 + m, n).cpu().numpy())
    if logger is not None:
        logger.add_tensors("/".join(("log_learned_model", key)), out, 0)
    return out


def learn_dynamics_from_data(dX, X, U, pend_env, regressor_class, logger, max_train, tags=(), training_iter=50,
                             device="cuda", dtype=torch.float32):
    """Random subset of the trajectory, fit (50 Adam steps), log the learned model (pendulum.py:345-371)."""
    numSteps = X.shape[0]
    N = min(numSteps - 1, max_train)
    idx = torch.randint(numSteps - 1, size=(N,))
    f = dict(dtype=dtype, device=device)
    Xtrain, Utrain, XdotTrain = X[idx].to(**f), U[idx].to(**f), dX[idx].to(**f)
    dgp = regressor_class(Xtrain.shape[-1], Utrain.shape[-1], device=device, dtype=dtype)
    dgp.fit(Xtrain, Utrain, XdotTrain, training_iter=training_iter)
    if logger is not None:
        logger.add_tensors("train", dict(Xtrain=Xtrain, Utrain=Utrain), 0)
    logged = log_learned_model(Xtrain.cpu().numpy(), dgp, pend_env.F_func, key="/".join(list(tags) + ["Fx"]), logger=logger)
    return dgp, logged


def learned_model_error(logged, n=2, m=1):
    """The number learn_dynamics_matrix_vector_vis writes to vector_matrix_learning_error.txt (pendulum.py:1121-1139):
    measure_batch_error with the per-point (1+m)n x (1+m)n covariance blocks."""
    FXl = torch.as_tensor(logged["FX_learned"]).double()
    b = int(FXl.shape[0] * FXl.shape[1])
    T_ = (1 + m) * n
    var = torch.as_tensor(logged["var_FX"]).double().reshape(b, T_, b, T_)
    blocks = torch.stack([var[i, :, i, :] for i in range(b)])
    return measure_batch_error(FXl.reshape(b, T_), blocks, torch.as_tensor(logged["FX_true"]).double().reshape(b, T_))


def learn_dynamics_matrix_vector_exp(exps=None, theta0=5 * math.pi / 6, omega0=-0.01, tau=0.01, mass=1, gravity=10,
                                     length=1, max_train=200, numSteps=1000, logger=None, device="cuda",
                                     dtype=torch.float32, training_iter=50):
    """pendulum.py:1052-1088: returns {name: (regressor, logged arrays, error)}."""
    from .control_affine_model import ControlAffineRegressorExact, ControlAffineRegressorVector
    exps = exps or dict(matrix=dict(regressor_class=ControlAffineRegressorExact),
                        vector=dict(regressor_class=ControlAffineRegressorVector))
    pend_env = PendulumDynamicsModel(m=1, n=2, mass=mass, gravity=gravity, length=length)
    dX, X, U = sampling_pendulum_data(pend_env, D=numSteps, x0=torch.tensor([theta0, omega0]), dt=tau,
                                      controller=ControlRandom(mass=mass, gravity=gravity, length=length).control)
    if logger is not None:
        for t, (dx, x, u) in enumerate(zip(dX, X, U)):
            logger.add_tensors("traj", dict(dx=dx, x=x, u=u), t)
    out = dict()
    for name, kw in exps.items():
        dgp, logged = learn_dynamics_from_data(dX, X, U, pend_env, kw["regressor_class"], logger, max_train=max_train,
                                               tags=[name], training_iter=training_iter, device=device, dtype=dtype)
        out[name] = (dgp, logged, learned_model_error(logged))
    return out


def compute_errors(regressor_class, sampling_callable, pend_env, ntries=5, max_train=200, test_on_grid=False, ntest=400,
                   device="cuda", dtype=torch.float32):
    """pendulum.py:1248-1303: `ntries` variance-weighted errors (`measure_batch_error`) of `regressor_class` on fresh
    trajectories.  As upstream, the regressor of a sample is constructed and queried WITHOUT being fitted (there is no
    fit call between `regressor_class(...)` and `custom_predict_fullmat`, :1279-1283): the figure is the error of the
    prior model."""
    import numpy as np
    errors = []
    for _ in range(ntries):
        dX, X, U = sampling_callable()
        order = np.arange(X.shape[0] - 1)
        np.random.shuffle(order)
        order_t = torch.from_numpy(order)
        Xtrain = X[order_t[:max_train]]
        if test_on_grid:
            grid = get_grid_from_Xtrain(Xtrain.cpu().numpy())
            Xtest = torch.from_numpy(grid.reshape(-1, Xtrain.shape[-1]))
        else:
            Xtest = X[order_t[-ntest:]]
        Xtest = Xtest.to(device=device, dtype=dtype)
        FX_true = pend_env.F_func(Xtest).transpose(-2, -1)                       # (b, 1+m, n)
        dgp = regressor_class(Xtrain.shape[-1], U.shape[-1], device=device, dtype=dtype)
        FX_learned, var_FX = dgp.custom_predict_fullmat(Xtest.reshape(-1, Xtest.shape[-1]))
        b, T_ = Xtest.shape[0], (1 + pend_env.ctrl_size) * pend_env.state_size
        idx = torch.arange(b, device=var_FX.device)
        blocks = var_FX.reshape(b, T_, b, T_)[idx, :, idx, :]
        errors.append(measure_batch_error(FX_learned.reshape(-1, T_), blocks, FX_true.reshape(-1, T_).to(FX_learned)))
    return errors


def speed_test_matrix_vector_exp(max_train_variations=(256, 256 + 64, 256 + 128, 256 + 256), ntimes=50, repeat=5,
                                 errorbartries=30, logger=None, exps=None, theta0=5 * math.pi / 6, omega0=-0.01, tau=0.01,
                                 mass=1, gravity=10, length=1, numSteps=2000, pendulum_dynamics_class=PendulumDynamicsModel,
                                 training_iter=50, device="cuda", dtype=torch.float32):
    """The reference's published speed test (pendulum.py:1305-1394, the only path of the repository with published
    numbers): one randomised pendulum trajectory; per training-set size a random subset, and per regressor
    (MVGP full / diag, CoGP full / diag) `fit(training_iter=50)`, then
    min(timeit.repeat('dgp.custom_predict_fullmat(Xtest); dgp.clear_cache()', repeat, number=ntimes)) on the 20 x 20
    (theta, omega) grid of the training range, and `errorbartries` prior-model errors (`compute_errors`).  Every timed call
    ends with a device synchronize (the reference's timing is host side).  Logged under the reference's tags when a
    logger is given (`<name>/elapsed` is seconds PER CALL, as upstream logs it); returns
    {name: {max_train: dict(elapsed=s per call, errors=[...], fit_s=...)}}."""
    import time
    import timeit
    from functools import partial
    import numpy as np
    from .control_affine_model import (ControlAffineRegressorExact, ControlAffineRegMatrixDiag,
                                       ControlAffineRegressorVector, ControlAffineRegVectorDiag)
    exps = exps or dict(matrix=dict(regressor_class=ControlAffineRegressorExact),
                        vector=dict(regressor_class=ControlAffineRegressorVector),
                        matrixdiag=dict(regressor_class=ControlAffineRegMatrixDiag),
                        vectordiag=dict(regressor_class=ControlAffineRegVectorDiag))
    pend_env = pendulum_dynamics_class(m=1, n=2, mass=mass, gravity=gravity, length=length)
    sample = partial(sampling_pendulum_data, dynamics_model=pend_env, D=numSteps, x0=torch.tensor([theta0, omega0]), dt=tau,
                     controller=ControlRandom(mass=mass, gravity=gravity, length=length).control)
    dX, X, U = sample()
    if logger is not None:
        for t, (dx, x, u) in enumerate(zip(dX, X, U)):
            logger.add_tensors("traj", dict(dx=dx, x=x, u=u), t)
    order = np.arange(X.shape[0] - 1)
    f = dict(device=device, dtype=dtype)
    out = {name: {} for name in exps}
    for max_train in max_train_variations:
        np.random.shuffle(order)
        idx = torch.from_numpy(order[:max_train].copy())
        Xtrain, Utrain, XdotTrain = X[idx].to(**f), U[idx].to(**f), dX[idx].to(**f)
        grid = get_grid_from_Xtrain(X[idx].numpy())
        Xtest = torch.from_numpy(grid.reshape(-1, 2)).to(**f)           # raw reshape of the [2, 20, 20] mgrid, as upstream (:1351-1355)
        for name, kw in exps.items():
            dgp = kw["regressor_class"](2, 1, device=device, dtype=dtype)
            t0 = time.perf_counter()
            dgp.fit(Xtrain, Utrain, XdotTrain, training_iter=training_iter)
            torch.cuda.synchronize()
            fit_s = time.perf_counter() - t0

            def call():
                dgp.custom_predict_fullmat(Xtest)
                dgp.clear_cache()
                torch.cuda.synchronize()
            call()
            elapsed = min(timeit.repeat(call, repeat=repeat, number=ntimes)) / ntimes
            errors = compute_errors(kw["regressor_class"], sample, pend_env, max_train=max_train, ntries=errorbartries,
                                    device=device, dtype=dtype)
            out[name][max_train] = dict(elapsed=elapsed, errors=errors, fit_s=fit_s,
                                        fit_loss_first_last=[dgp.fit_losses[0], dgp.fit_losses[-1]] if training_iter else None)
            if logger is not None:
                logger.add_scalars(name, dict(elapsed=elapsed), max_train)
                logger.add_tensors(name, dict(errors=np.asarray(errors)), max_train)
    return out


# ------------------------------------------------------------------------------------------------
# The run-script entry points (`run.sh:17-21` calls them by name): experiment half + the NUMBERS half of the reference's
# `_vis` functions (what they read back from the event file and write next to it).  The plotting half (matplotlib figures,
# LaTeX labels, xdg-open) is out of scope (SURVEY 2 / DESIGN 8).
def _newest_events_file(logs_dir):
    import glob
    import os
    return max(glob.glob(os.path.join(logs_dir, "*.tfevents*")), key=lambda f: os.stat(f).st_mtime)


def learn_dynamics_matrix_vector_vis(exps=("matrix", "vector"), events_file=None):
    """pendulum.py:1215-1242 without the figure: reads the logged grids back from the event file, computes the
    variance-weighted error of every experiment (`measure_batch_error` on the per-point covariance blocks, :1121-1139) and
    writes them to `vector_matrix_learning_error.txt` beside the event file in the reference's format (one row, %.03f,
    header = names).  Returns (error_file, {name: error})."""
    import os.path as osp
    import numpy as np
    from .tblog import load_tensorboard_scalars
    logdata = load_tensorboard_scalars(events_file)
    errors = dict()
    for exp in exps:
        key = "log_learned_model/" + exp + "/Fx/"
        logged = dict(FX_learned=logdata[key + "FX_learned"][0][1], var_FX=logdata[key + "var_FX"][0][1],
                      FX_true=logdata[key + "FX_true"][0][1])
        errors[exp] = float(learned_model_error(logged))
    error_file = osp.join(osp.dirname(events_file), "vector_matrix_learning_error.txt")
    np.savetxt(error_file, [[errors[e] for e in exps]], fmt="%.03f", header=" ".join(exps))
    return error_file, errors


def learn_dynamics_matrix_vector(logger_class=None, **kw):
    """pendulum.py:1244-1246: the experiment (`learn_dynamics_matrix_vector_exp`, logged under `data/runs/
    learn_matrix_vector_<version>` unless `logger_class` says otherwise), then the numbers of `_vis`.  Returns the event
    file, as the reference's `_exp` does."""
    from functools import partial
    from .tblog import TBLogger
    logger = (logger_class or partial(TBLogger, exp_tags=["learn_matrix_vector"], runs_dir="data/runs"))()
    res = learn_dynamics_matrix_vector_exp(logger=logger, **kw)
    events_file = _newest_events_file(logger.experiment_logs_dir)
    learn_dynamics_matrix_vector_vis(exps=tuple(res), events_file=events_file)
    return events_file


def speed_test_matrix_vector_vis(events_file, exp_conf=("vectordiag", "matrixdiag", "vector", "matrix")):
    """pendulum.py:1396-1430 without the figure: {name: dict(training_samples, elapsed [s per call], errors)} read back
    from the event file (tags `<name>/elapsed`, `<name>/errors`)."""
    from .tblog import load_tensorboard_scalars
    logdata = load_tensorboard_scalars(events_file)
    out = dict()
    for gp in exp_conf:
        if gp + "/elapsed" not in logdata:
            continue
        training_samples, elapsed = zip(*logdata[gp + "/elapsed"])
        _, errors = zip(*logdata[gp + "/errors"])
        out[gp] = dict(training_samples=list(training_samples), elapsed=list(elapsed), errors=list(errors))
    return out


def speed_test_matrix_vector(logger_class=None, **kw):
    """pendulum.py:1433-1435: the published speed test (`speed_test_matrix_vector_exp`, logged under `data/runs/
    speed_test_matrix_vector_<version>`), then the read-back of `_vis`.  Returns the event file."""
    from functools import partial
    from .tblog import TBLogger
    logger = (logger_class or partial(TBLogger, exp_tags=["speed_test_matrix_vector"], runs_dir="data/runs"))()
    speed_test_matrix_vector_exp(logger=logger, **kw)
    events_file = _newest_events_file(logger.experiment_logs_dir)
    speed_test_matrix_vector_vis(events_file)
    return events_file


# ------------------------------------------------------------------------------------------------
# The safety filter of ControlPendulumCBFLearned (pendulum.py:909-961) run as a batch of closed loops: upstream's own
# learned pendulum controller cannot be constructed (ControlCBFLearned calls clf_class=None), so the working definition is
# SOCPController(cbfs=[RadialCBFRelDegree2], clf=None) with the greedy nominal controller (bcbf_pendulum_control_step).
def pendulum_bayes_cbf_safe_rollouts(Bt=4096, numSteps=250, D=400, max_train=200, training_iter=50, theta0=7 * math.pi / 12,
                                     omega0=-0.01, tau=0.01, mass=1, gravity=10, length=1, seed=0, device="cuda", **kw):
    """Fit a ControlAffineRegressor on one randomised pendulum trajectory (`sampling_pendulum_data` under ControlRandom, a
    random subset of `max_train` rows, `training_iter` Adam steps: learn_dynamics_from_data, pendulum.py:345-371), then run
    `rollouts.pendulum_safety_rollouts` with that ONE model shared by all Bt instances (regime S).  Returns
    (regressor, rollout result).  Keywords go through to the rollouts: plant="posterior" steps every instance on plants drawn
    from the fitted model's own posterior and adds `risk`, the empirical rate of CBC2 < 0 on the draw, to hold against
    max_unsafe_prob (rho_tol separates the steps that bought slack)."""
    from .control_affine_model import ControlAffineRegressorExact
    from .rollouts import pendulum_safety_rollouts
    torch.manual_seed(seed)
    pend_env = PendulumDynamicsModel(m=1, n=2, mass=mass, gravity=gravity, length=length)
    dX, X, U = sampling_pendulum_data(pend_env, D=D, x0=torch.tensor([theta0, omega0]), dt=tau,
                                      controller=ControlRandom(mass=mass, gravity=gravity, length=length).control)
    # (the Exact regressor: learn_dynamics_from_data evaluates the fit on a grid with custom_predict_fullmat, which the base class lacks)
    dgp, _ = learn_dynamics_from_data(dX, X, U, pend_env, ControlAffineRegressorExact, None, max_train=max_train,
                                      training_iter=training_iter, device=device, dtype=torch.float64)
    gp = dict(dgp._state(), kernel=getattr(dgp, "data_kernel", "rbf"))
    kw.setdefault("true_model", (mass, gravity, length))
    return dgp, pendulum_safety_rollouts(Bt, numSteps=numSteps, gp=gp, shared=True, theta0=theta0, omega0=omega0,
                                         device=device, seed=seed, **kw)


# ------------------------------------------------------------------------------------------------
# The learning controller of run_pendulum_control_online_learning (pendulum.py:909-961, 1041-1048).
class ControlPendulumCBFLearned:
    """One-instance façade of upstream's ControlPendulumCBFLearned, same signature: a `ControlCBFLearned` with
    `controller_class=SOCPController` and `cbfs=[RadialCBFRelDegree2(model)]` (the barrier on the learned regressor, as
    upstream builds it), the greedy nominal controller inside the epsilon-greedy explorer, the regressor refit every
    `train_every_n_steps` steps on at most `max_train` rows (`MeanAdjustedModel`, `iterations` Adam steps per refit).
    Deviations: upstream's class cannot run (its ControlCBFLearned defaults to QPController with clf=None) and never sets
    `enable_learning`, so as written it never learns; `enable_learning=False` stays the default here, `True` learns.
    The plotting arguments are accepted and ignored.  `rollouts.pendulum_learning_rollouts` is the batched form."""

    def __init__(self, theta_goal=0., omega_goal=0., quad_goal_cost=((1.0, 0), (0, 1.0)), x_dim=2, u_dim=1, gamma_sr=1,
                 delta_sr=10, train_every_n_steps=10, mean_dynamics_model_class=None, egreedy_scheme=(1, 0.01),
                 iterations=100, dt=0.001, max_train=200, gamma_length_scale_prior=(math.pi / 100, math.pi / 100),
                 constraint_plotter_class=None, true_model=None, plotfile=None, dtype=torch.float64,
                 use_ground_truth_model=False, numSteps=1000, ctrl_range=(-15., 15.), u_quad_cost=((1.,),),
                 enable_learning=False, model=None, exploration_controller_class=None, device=None,
                 unsafe_controller_class=None):
        """mean_dynamics_model_class None = partial(ZeroDynamicsModel, m=1, n=2), upstream's default.  model: the regressor
        (default a fresh ControlAffineRegressor(x_dim, u_dim, gamma_length_scale_prior=...) in `dtype`);
        exploration_controller_class: default `EpsilonGreedyController` (tests pass a replaying subclass);
        unsafe_controller_class: default `GreedyController`; `controllers.LQRController` is upstream's."""
        from .control_affine_model import ControlAffineRegressor
        from .controllers import ControlCBFLearned, EpsilonGreedyController, SOCPController
        from .unicycle_move_to_pose import ZeroDynamicsModel
        if use_ground_truth_model:
            raise NotImplementedError("use_ground_truth_model: ControlCBFCLFGroundTruth / the no-GP mode of the batched step")
        if mean_dynamics_model_class is None:
            mean_dynamics_model_class = lambda: ZeroDynamicsModel(m=u_dim, n=x_dim)
        if model is None:
            model = ControlAffineRegressor(x_dim, u_dim, device=device, dtype=dtype,
                                           gamma_length_scale_prior=gamma_length_scale_prior)
        self.model, self.true_model = model, true_model
        self.cbf2 = RadialCBFRelDegree2(self.model, dtype=dtype)
        self.controller = ControlCBFLearned(
            x_dim=x_dim, u_dim=u_dim, model=model, train_every_n_steps=train_every_n_steps, dt=dt, ctrl_range=ctrl_range,
            x_goal=[theta_goal, omega_goal], x_quad_goal_cost=[list(r) for r in quad_goal_cost],
            u_quad_cost=[list(r) for r in u_quad_cost], numSteps=numSteps, cbfs=[self.cbf2],
            exploration_controller_class=exploration_controller_class or EpsilonGreedyController,
            egreedy_scheme=list(egreedy_scheme), enable_learning=enable_learning,
            mean_dynamics_model_class=mean_dynamics_model_class, max_train=max_train, controller_class=SOCPController,
            training_iter=iterations, **({} if unsafe_controller_class is None else dict(unsafe_controller_class=unsafe_controller_class)))
        self.net_model = self.controller.net_model

    @property
    def last_status(self):
        return self.controller._controller.last_status

    def control(self, xi, t=None):
        """u for the state xi ([n]: raises on an unsolved program, as upstream; [1, n]: keeps u_ref, status in
        `last_status`), and the observation handed to the learner."""
        return self.controller.control(xi, t=t)


def pendulum_online_learning_rollouts(Bt=4096, numSteps=250, tau=0.002, theta0=7 * math.pi / 12, omega0=-0.01,
                                      fit_iters=100, **kw):
    """run_pendulum_control_online_learning (pendulum.py:1041-1048: 250 steps, tau = 0.002, theta0 = 7 pi / 12, float64)
    with ControlPendulumCBFLearned's settings (train every 10 steps, max_train 200, egreedy (1, 0.01), ctrl_range (-15,
    15), `iterations` = 100 Adam steps per refit) and learning ON, for Bt perturbed starts at once
    (`rollouts.pendulum_learning_rollouts`).  Keywords go through: plant="posterior" draws every step's plant from the model the
    instance holds at that step (the rows it learns from then record the drawn plant) and adds `risk`."""
    from .rollouts import pendulum_learning_rollouts
    return pendulum_learning_rollouts(Bt, numSteps=numSteps, dt=tau, theta0=theta0, omega0=omega0, fit_iters=fit_iters,
                                      learning=True, **kw)


# ------------------------------------------------------------------------------------------------
# The CLF-CBF quadratic program on the KNOWN model: PendulumCBFCLFDirect / run_pendulum_control_cbf_clf
# (pendulum.py:530-640, 770-906, 1019-1024), the controller the Bayesian one is measured against.  Rows and program are
# evaluated by the library (bcbf_pendulum_clf_cbf_control / _rollout); `rollouts.pendulum_clf_cbf_rollouts` is the batched form.
def _clf_cbf_eval(x, model, **task):
    """ops.pendulum_clf_cbf_control for ONE state x[2] (any device / float dtype; evaluated on the GPU in float64, the
    precision upstream's program is solved in whatever the torch dtype)."""
    from . import ops
    dev = x.device if x.is_cuda else torch.device("cuda")
    xd = x.detach().reshape(1, 2).to(device=dev, dtype=torch.float64).contiguous()
    return ops.pendulum_clf_cbf_control(xd, ctrl_model=(model.mass, model.gravity, model.length), **task)


class _PendulumAffine:
    """A(x) u - b(x) <= 0, upstream's NamedAffineFunc protocol: value(x), A(x) [1], b(x) (0-d), __call__(x, u)."""
    _row = None

    def _task(self):
        raise NotImplementedError

    def _eval(self, x):
        return _clf_cbf_eval(x, self.model, **self._task())

    def value(self, x):
        return self._eval(x)["values"][0, self._row].to(x)

    def A(self, x):
        return self._eval(x)["A"][0, self._row].reshape(1).to(x)

    def b(self, x):
        return self._eval(x)["b"][0, self._row].to(x)

    def __call__(self, x, u):
        return self.A(x) @ u.reshape(1).to(x) - self.b(x)

    def __getattr__(self, name):          # upstream forwards unknown attributes to its model (mass, gravity, f_func ...)
        if name == "model":
            raise AttributeError(name)
        return getattr(self.model, name)


class EnergyCLF(_PendulumAffine):
    """V = l omega^2 / 2 + g (1 - cos theta);  A = grad V . g(x) = omega / m,  b = -grad V . f(x) - c V = -c V  (:530-579).
    These are the values upstream RETURNS; its hand-written `direct = l omega` agrees with them only when m l = 1, and its
    own assert trips for another model."""
    _row = 0

    def __init__(self, model, clf_c=1, name="clf"):
        self.model, self.clf_c, self.name = model, clf_c, name

    V_clf = _PendulumAffine.value

    def _task(self):
        return dict(clf_c=float(self.clf_c))


class RadialCBF(_PendulumAffine):
    """h = (cos Delta_c - cos(theta - theta_c)) (omega^2 + 1), relative degree 1  (:582-640):  A = -grad h . g(x),
    b = grad h . f(x) + gamma h."""
    _row = 1

    def __init__(self, model, cbf_col_gamma=1, k_alpha=(1., 1.), cbf_col_delta=math.pi / 8, cbf_col_theta=math.pi / 4,
                 theta_c=math.pi / 4, gamma_col=1, delta_col=math.pi / 8, name="cbf"):
        self.model, self.cbf_col_gamma, self.k_alpha, self.name = model, cbf_col_gamma, list(k_alpha), name
        self.cbf_col_delta, self.cbf_col_theta = cbf_col_delta, cbf_col_theta

    h_col = _PendulumAffine.value

    def _task(self):
        return dict(cbf_kind="radial", cbf_gamma=float(self.cbf_col_gamma), theta_c=float(self.cbf_col_theta),
                    delta_c=float(self.cbf_col_delta))


def _clf_cbf_task(ctrl_aff_constraints, constraint_margin_weights):
    """(model, task keywords of ops.pendulum_clf_cbf_*) of the one program shape upstream builds: [EnergyCLF, barrier] on one
    pendulum model, one control, one slack on the first row."""
    cons = list(ctrl_aff_constraints)
    if (len(cons) != 2 or len(constraint_margin_weights) != 1 or not isinstance(cons[0], EnergyCLF)
            or not isinstance(cons[1], (RadialCBFRelDegree2, RadialCBF)) or cons[0].model is not cons[1].model):
        raise NotImplementedError(
            "control_QP_cbf_clf is built for upstream's program: [EnergyCLF, RadialCBFRelDegree2 or RadialCBF] on one "
            "pendulum model with constraint_margin_weights = [w]")
    clf, cbf = cons
    task = dict(clf_c=float(clf.clf_c), theta_c=float(cbf.cbf_col_theta), delta_c=float(cbf.cbf_col_delta),
                slack_weight=float(constraint_margin_weights[0]))
    if isinstance(cbf, RadialCBF):
        task.update(cbf_kind="radial", cbf_gamma=float(cbf.cbf_col_gamma))
    else:
        task.update(cbf_kind="reldeg2", k_alpha=tuple(float(k) for k in cbf.k_alpha))
    return clf.model, task


def control_QP_cbf_clf(x, ctrl_aff_constraints, constraint_margin_weights=[]):
    """pendulum.py:800-864: minimise 1/2 (u^2 + w rho^2) s.t. A_clf u - rho <= b_clf, A_cbf u <= b_cbf; returns u[1] in x's
    dtype.  Upstream iterates with cvxopt; here the unique optimum comes in closed form from the library (parity with
    cvxopt's iterates is not claimed).  Raises RuntimeError("QP is infeasible ...") as upstream does, NotImplementedError
    for any other shape than upstream's own (two rows, one control, one slack on the first row)."""
    model, task = _clf_cbf_task(ctrl_aff_constraints, constraint_margin_weights)
    out = _clf_cbf_eval(x, model, **task)
    if int(out["status"][0]) != 0:
        raise RuntimeError("QP is infeasible\n        minimize 1/2 (u^2 + %g rho^2)\n        s.t.\n        %s [u, rho] <= %s"
                           % (task["slack_weight"], [[float(out["A"][0, 0]), -1.0], [float(out["A"][0, 1]), 0.0]],
                              out["b"][0].tolist()))
    return out["u"].to(device=x.device, dtype=x.dtype)


class PendulumCBFCLFDirect:
    """Upstream's PendulumCBFCLFDirect (:867-906), same signature: EnergyCLF (slack weight 100) and RadialCBFRelDegree2 on
    the known pendulum (mass, gravity, length).  The plotting arguments are accepted and ignored."""
    needs_ground_truth = True

    def __init__(self, mass=None, length=None, gravity=None, dt=None, constraint_plotter_class=None,
                 pendulum_dynamics_class=PendulumDynamicsModel, true_model=None, plotfile=None,
                 dtype=torch.get_default_dtype(), **ignored):
        self.dt, self.true_model, self.dtype, self.pendulum_dynamics_class = dt, true_model, dtype, pendulum_dynamics_class
        self.set_model_params(mass=mass, length=length, gravity=gravity)

    def set_model_params(self, **kwargs):
        self.model = self.pendulum_dynamics_class(m=1, n=2, **kwargs)
        self.cbf2 = RadialCBFRelDegree2(self.model, dtype=self.dtype)
        self.aff_constraints = [EnergyCLF(self.model), self.cbf2]

    def f_func(self, x):
        return self.model.f_func(torch.as_tensor(x))

    def g_func(self, x):
        return self.model.g_func(torch.as_tensor(x))

    def control(self, xi, i=None, t=None):
        return control_QP_cbf_clf(xi, ctrl_aff_constraints=self.aff_constraints, constraint_margin_weights=[100])


def run_pendulum_control_cbf_clf(theta0=5 * math.pi / 12, omega0=-0.01, tau=0.002, mass=1, gravity=10, length=1,
                                 numSteps=15000, controller_class=PendulumCBFCLFDirect,
                                 pendulum_dynamics_class=PendulumDynamicsModel, plotfile=None, dtype=torch.float64,
                                 device="cuda"):
    """run_pendulum_control_cbf_clf (pendulum.py:1019-1024 through run_pendulum_experiment, :299-338): the closed loop of
    PendulumCBFCLFDirect on the true pendulum from (theta0, omega0), numSteps steps of tau -- ONE instance, every step
    recorded, all steps in one launch of the library's rollout kernel.  Returns upstream's
    (damge_perc, time_vec, theta_vec, omega_vec, u_vec), each of length numSteps.
    dtype: float64 by default.  Upstream's default run is float32 states around a float64 solve (its program goes to cvxopt
    in float64 whatever the torch dtype); dtype=torch.float32 runs rows, program and plant in float32.
    Raises RuntimeError("QP is infeasible ...") when a step's program is, as upstream's loop does.  plotfile is ignored."""
    from . import ops
    ctrl = controller_class(mass=mass, gravity=gravity, length=length, dt=tau, dtype=dtype,
                            true_model=pendulum_dynamics_class(m=1, n=2, mass=mass, gravity=gravity, length=length, dtype=dtype))
    if not isinstance(ctrl, PendulumCBFCLFDirect):
        raise NotImplementedError("run_pendulum_control_cbf_clf runs PendulumCBFCLFDirect")
    model, task = _clf_cbf_task(ctrl.aff_constraints, [100])
    f = dict(dtype=dtype, device=device)
    x = torch.tensor([[theta0, omega0]], **f)
    min_h = torch.full((1,), float("inf"), **f)
    damage = torch.zeros(1, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    traj, us = torch.empty(numSteps, 1, 2, **f), torch.empty(numSteps, 1, **f)
    ops.pendulum_clf_cbf_rollout(x, min_h, damage, status, numSteps, dt=tau, ctrl_model=(model.mass, model.gravity, model.length),
                                 true_model=(mass, gravity, length), traj=traj, u_rec=us, record_every=1, **task)
    if int(status[0]) != 0:
        raise RuntimeError("QP is infeasible at step %d (state %s)" % (int(status[0]) - 1, x[0].tolist()))
    theta_vec, omega_vec, u_vec = traj[:, 0, 0], traj[:, 0, 1], us[:, 0]
    assert torch.all((theta_vec <= math.pi) & (-math.pi <= theta_vec))
    damge_perc = damage[0].to(dtype) * 100 / numSteps
    return damge_perc, tau * torch.arange(numSteps, **f), theta_vec, omega_vec, u_vec
