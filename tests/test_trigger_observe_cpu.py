"""CPU-side checks of the self-triggered event that observes itself for a learner (bcbf_unicycle_trigger_step_observe): the numpy
yardstick tests/_trigger_observe_reference.py against an event done by hand and against the yardstick it is built on, the row-index
rule, the entry's argument checks (refused before any HIP call, with a reason), the workspace and the ValueErrors of the `ops`
binding and of the loop."""
import ctypes
import math
import os

import numpy as np
import pytest

import _trigger_observe_reference as TO
import _trigger_step_reference as S
import test_trigger_audit_cpu as TC                       # the made-up instance and the audit entry's refusals, which this entry keeps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_against_an_event_done_by_hand(dtype):
    h = TO.hand_event()
    for si in (True, False):
        o = TO.observation(h["x_old"], h["x_new"], h["u"], True, h["dt_b"], h["L_mean"], shift_invariant=si, dtype=dtype)
        assert all(o[k].dtype == dtype for k in ("obs_x", "obs_uh", "obs_y", "xq_next"))
        assert o["obs_x"].tolist() == (h["obs_x"] if si else h["obs_x_raw"])
        assert o["obs_uh"].tolist() == h["obs_uh"] and o["obs_y"].tolist() == h["obs_y"]
        assert o["xq_next"].tolist() == (h["xq_next"] if si else h["xq_next_raw"])
        # 8 eps (|dx / dt| + |u0| + |u1| / L) = 8 eps ((2, 0, 0.5) + 2 + 0.125)
        np.testing.assert_allclose(o["bound"], 8 * np.finfo(dtype).eps * np.array([4.125, 2.125, 2.625]), rtol=1e-15)
    # an unsolved instance kept its state and applied nothing: the plant at rest, whatever y holds
    o = TO.observation(h["x_old"], h["x_old"], h["u"], False, h["dt_b"], h["L_mean"], dtype=dtype)
    rest = TO.rest_row(dtype)
    assert o["obs_uh"].tolist() == rest["obs_uh"].tolist() == [1, 0, 0] and o["obs_y"].tolist() == rest["obs_y"].tolist() == [0, 0, 0]
    assert o["obs_x"].tolist() == [0, 0, 0] and o["xq_next"].tolist() == [0, 0, 0] and not o["bound"].any()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("status", [0, 2])
def test_reference_event_is_the_trigger_step_yardstick_with_the_row_of_its_own_hold(seed, status):
    base, _ = TC.random_instance(seed)
    want = S.event(status=status, **base)
    ev = TO.event(status=status, **base, L_mean=4.0, obs_every=3, obs_row0=5, obs_ld=9)
    for k, v in want.items():
        assert np.array_equal(np.asarray(ev[k]), np.asarray(v)), k
    assert ev["obs_row"] == 6                                                     # events = 3: 5 + 3 // 3
    th, u = base["x"][2], (base["u"] if status == 0 else np.zeros(2))
    fd = (want["x"] - base["x"]) / want["dt_used"]
    np.testing.assert_allclose(ev["obs_y"], fd - np.array([math.cos(th) * u[0], math.sin(th) * u[0], u[1] / 4.0]), rtol=0, atol=1e-12)
    if status == 0:
        # the true plant turns at u1 / L_true, the prior mean at u1 / L_mean: that residual is what there is to learn
        np.testing.assert_allclose(ev["obs_y"], [0, 0, u[1] / base["L_true"] - u[1] / 4.0], rtol=0, atol=1e-8)   # (ulp(x) / dt_b of the stored state)
    else:
        assert not ev["obs_y"].any() and ev["obs_uh"].tolist() == [1, 0, 0]
    assert ev["obs_x"].tolist() == [0, 0, th] and ev["xq_next"].tolist() == [0, 0, want["x"][2]]
    assert TO.event(status=status, **dict(base, t=1.0)) is None                  # finished: nothing, the row included


def test_row_index_rule():
    # every event observed: row0 + e, until the stream ends
    assert [TO.row_index(e, 1, 0, 4) for e in range(6)] == [0, 1, 2, 3, None, None]
    assert [TO.row_index(e, 1, 48, 50) for e in range(4)] == [48, 49, None, None]
    # every third event: e = 0, 3, 6 ... -> row0, row0 + 1, ...; the events between write nothing
    assert [TO.row_index(e, 3, 2, 5) for e in range(10)] == [2, None, None, 3, None, None, 4, None, None, None]
    # after iteration e of a lockstep loop a live instance has written 1 + e // obs_every rows
    for every in (1, 3):
        for e in range(12):
            assert sum(TO.row_index(j, every, 0, 100) is not None for j in range(e + 1)) == 1 + e // every
    assert TO.row_index(-3, 3, 0, 10) is None


# ------------------------------------------------------------------------------------------------ the entry's argument checks
NPTR = TC.NPTR + 4
OBSX, OBSUH, OBSY, XQN = TC.NPTR, TC.NPTR + 1, TC.NPTR + 2, TC.NPTR + 3
ROWS = (OBSX, OBSUH, OBSY)
GOOD = dict(TC.GOOD, L_mean=4.0, ld=8, row0=2, every=3, flags=1)
BAD = list(TC.BAD) + [(dict(null=n), "given together or not at all") for n in ((OBSX,), (OBSUH,), (OBSY,), (OBSX, OBSUH), (OBSX, OBSY), (OBSUH, OBSY))] \
    + [(dict(ld=0), "obs_ld < 1"), (dict(ld=-4), "obs_ld < 1"), (dict(row0=-1), "obs_row0 < 0"), (dict(every=0), "obs_every < 1"),
       (dict(every=-2), "obs_every < 1"), (dict(L_mean=0.0), "L_mean"), (dict(L_mean=-0.0), "L_mean"), (dict(L_mean=math.nan), "L_mean"),
       (dict(flags=2), "only bit 0"), (dict(flags=3, null=ROWS), "only bit 0")]


def _call(lib, suf, a):
    """The entry on fake pointers: positions 0-44 as bcbf_unicycle_trigger_step_audit takes them (tests/test_trigger_audit_cpu.py),
    45-47 obs_x / obs_uh / obs_y, 48 xq_next."""
    ptr = [ctypes.c_void_p(4096 * (k + 1)) for k in range(NPTR)]
    for k in a["null"]:
        ptr[k] = None
    fn = getattr(lib.lib, "bcbf_unicycle_trigger_step_observe" + suf)
    return fn(*ptr[:9], 96.4, *ptr[9:13], 1e-4, 1e-2, 1.0, a["tau_min"], a["tau_max"], 10.0, 12.0, ptr[13], ptr[14], a["dt_plan"],
              *ptr[15:TC.NPTR], a["L_mean"], ptr[OBSX], ptr[OBSUH], ptr[OBSY], a["ld"], a["row0"], a["every"], ptr[XQN], a["flags"],
              a["Bt"], a["Bh"], a["Kob"], a["Nte"], a["P"], None)


def _id(i, c):
    return "%d-%s" % (i, "-".join("%s%s" % (k, "_".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in c.items()))


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change,why", BAD, ids=[_id(i, c) for i, (c, w) in enumerate(BAD)])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, change, why):
    """Every refusal of the audit entry, and the new ones: a partial row set; obs_ld < 1, obs_row0 < 0, obs_every < 1, L_mean 0 or
    NaN with rows; an undefined flag.  Every case fails the host check, so the fake pointers are never used and no GPU is touched."""
    rc = _call(lib, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_unicycle_trigger_step_observe" + suf) and why in msg, msg


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change", [dict(), dict(null=ROWS), dict(null=(XQN,)), dict(null=ROWS + (XQN,)), dict(null=TC.GROUP_P + TC.GROUP_H),
                                    dict(null=ROWS, ld=0, row0=-1, every=0, L_mean=0.0), dict(flags=0), dict(L_mean=-1.0)],
                         ids=["all", "no-rows", "no-xq_next", "no-O", "O-alone", "no-rows-their-scalars-unread", "raw-inputs", "negative-L_mean"])
def test_a_valid_call_passes_the_checks_and_fails_at_the_launch_without_a_gpu(lib, suf, change):
    """With every group complete or absent the host check passes (the rows' scalars are only looked at with rows); without a device
    the launch then fails: BCBF_ELAUNCH and HIP's message.  Not run where a GPU is present: a launch on these made-up pointers must
    never reach one."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the valid call on made-up pointers is only made where the launch cannot happen")
    rc = _call(lib, suf, dict(GOOD, **change))
    assert rc == -2, (rc, lib.lib.bcbf_last_error().decode())                      # BCBF_ELAUNCH
    assert lib.lib.bcbf_last_error().decode().startswith("bcbf_unicycle_trigger_step_observe" + suf)


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bcbf.h")).read()
    for name in ("bcbf_unicycle_trigger_step_observe_f32", "bcbf_unicycle_trigger_step_observe_f64"):
        assert name + "(" in header and name in lib.declared_symbols() and hasattr(lib.lib, name)


# ------------------------------------------------------------------------------------------------ the ops binding and the loop
def test_workspace_rows_start_as_the_plant_at_rest(lib):
    import torch
    from bayesian_cbf_amd import ops
    ow = ops.trigger_observe_workspace(3, 5, torch.float32, "cpu")
    assert sorted(ow) == sorted(["obs", "ld", "row0", "every", "xq_next", "shift_invariant", "L_mean"])
    X, UH, Y = ow["obs"]
    for v in (X, UH, Y):
        assert tuple(v.shape) == (3, 5, 3) and v.dtype == torch.float32 and v.is_contiguous()
    rest = TO.rest_row(np.float32)
    assert np.array_equal(X.numpy(), np.broadcast_to(rest["obs_x"], (3, 5, 3)))
    assert np.array_equal(UH.numpy(), np.broadcast_to(rest["obs_uh"], (3, 5, 3)))
    assert np.array_equal(Y.numpy(), np.broadcast_to(rest["obs_y"], (3, 5, 3)))
    assert (ow["ld"], ow["row0"], ow["every"], ow["shift_invariant"], ow["L_mean"]) == (5, 0, 1, True, 1.0)
    assert tuple(ow["xq_next"].shape) == (3, 3) and not ow["xq_next"].any()


def test_binding_refuses_wrong_buffers_with_value_errors(lib):
    """The checks of the new arguments come before the device check, so they run on host tensors; a call that passes them then meets
    the refusal of host tensors (there is no CPU path)."""
    import torch
    from bayesian_cbf_amd import ops
    pos, aws, A = TC._binding_inputs()
    prep = ops.unicycle_trigger_step_prepare
    ow = ops.trigger_observe_workspace(4, 6, torch.float64, "cpu")
    with pytest.raises(ValueError, match="gp_A"):
        prep(*pos, observe=ow)
    with pytest.raises(ValueError, match="no key"):
        prep(*pos, gp_A=A, observe=dict(ow, rows=3))
    with pytest.raises(ValueError, match="three stream buffers"):
        prep(*pos, gp_A=A, observe=dict(ow, obs=ow["obs"][:2]))
    with pytest.raises(ValueError, match="three stream buffers"):
        prep(*pos, gp_A=A, observe=dict(ow, obs=(ow["obs"][0], None, ow["obs"][2])))
    with pytest.raises(ValueError, match="obs_uh"):
        prep(*pos, gp_A=A, observe=dict(ow, obs=(ow["obs"][0], ow["obs"][1][:, :5], ow["obs"][2])))
    with pytest.raises(ValueError, match="obs_y"):
        prep(*pos, gp_A=A, observe=dict(ow, obs=(ow["obs"][0], ow["obs"][1], ow["obs"][2].float())))
    with pytest.raises(ValueError, match="obs_x"):
        prep(*pos, gp_A=A, observe=dict(ow, ld=5))                                 # ld must be the buffers' own
    for bad in (dict(ld=0), dict(row0=-1), dict(every=0)):
        with pytest.raises(ValueError, match="ld >= 1, row0 >= 0, every >= 1"):
            prep(*pos, gp_A=A, observe=dict(ow, **bad))
    for L in (0.0, math.nan):
        with pytest.raises(ValueError, match="L_mean"):
            prep(*pos, gp_A=A, observe=dict(ow, L_mean=L))
    with pytest.raises(ValueError, match="xq_next"):
        prep(*pos, gp_A=A, observe=dict(ow, xq_next=torch.zeros(4, 2, dtype=torch.float64)))
    for kw in (dict(observe=ow), dict(observe=dict(ow, obs=None)), dict(observe=dict(ow, xq_next=None)),
               dict(observe=ow, sampled=aws["sampled"], audit=aws["audit"])):
        with pytest.raises(RuntimeError, match="ROCm device tensors"):
            prep(*pos, gp_A=A, **kw)


def test_loop_refuses_the_posterior_plant_and_bad_schedules(lib):
    from bayesian_cbf_amd import rollouts
    with pytest.raises(ValueError, match="teaches nothing"):
        rollouts.self_triggered_learning_rollouts(4, horizon=1.0, plant="posterior", device="cpu")
    for bad in (dict(max_train=0), dict(refit_every=0), dict(obs_every=0)):
        with pytest.raises(ValueError, match="max_train >= 1"):
            rollouts.self_triggered_learning_rollouts(4, horizon=1.0, device="cpu", **bad)
    with pytest.raises(ValueError, match="tau_min"):
        rollouts.self_triggered_learning_rollouts(4, horizon=1.0, tau_min=0.1, tau_max=0.05, device="cpu")
