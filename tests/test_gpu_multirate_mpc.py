"""GPU: the multi-rate closed loops on the device (i7m_mpc_run_multirate, csrc/i7m_mpc_multirate.h;
MPC_GATO_Batch.run_mpc and MPC_GATO.run_mpc of the reference, src/gato_mpc_batch.py:76-217 and
src/gato_mpc.py:53-150) against the same loop in numpy on the C++ port (tests/multirate_mpc_ref.py).

The goal switch and the stop are discrete results, so every parity case first asserts, on the
reference alone, that every recorded distance is at least 1e-3 from the radius; then the NaN
patterns must be identical.  Distances, q and the path use the project's closed-loop tolerances for
the two modes (tests/test_gpu_sampled_mpc.py: 2e-6 direct, 1e-8 ADMM).
"""
import ctypes as C

import numpy as np
import pytest

from multirate_mpc_ref import make_case, run_multirate_ref

pytestmark = pytest.mark.gpu
TOL = {"direct": 2e-6, "admm": 1e-8}
GAP = 1e-3
PIN = [1.0] * 6 + [0.0] * 6
# (N, steps, dt, sim_dt, radius, control): no shift for nine steps then one; a split sub-step;
# MPC_GATO's constants; shifts of 2 and 3; a carried accumulator with dt != 0.01; PREV at radius 0.1
CASES = [(8, 12, .01, .001, .1, "new"), (16, 8, .01, .004, .1, "new"), (16, 6, .01, .02, .01, "prev"),
         (8, 6, .01, .025, .1, "new"), (8, 6, .015, .02, .1, "new"), (8, 6, .01, .02, .1, "prev")]


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


@pytest.fixture(scope="module")
def case():
    return make_case()


def _handle(lib, model, N, rows, mode, dt=0.01):
    return lib.Handle(model, N=N, dt=dt, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def _equal(a, b, keys=("dist", "q", "u", "xpath", "xcur", "xu")):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("N,steps,dt,sim_dt,radius,control", CASES)
def test_parity_with_the_numpy_loop(lib, model, case, N, steps, dt, sim_dt, radius, control, mode):
    """dist, q and xpath within the closed-loop tolerance of the numpy loop, the NaN patterns
    identical, u of step 0 the initial solve's control, and the final state consistent with the
    histories.  Measured on an MI355X, max |q - ref| over the case: direct <= 4.7e-13; ADMM 4.4e-12,
    2.0e-11, 9.1e-10, 1.2e-9, 2.7e-10 and 4.7e-9 in the order of CASES (the largest where sim_dt >=
    0.02: a 1e-9 perturbation of the warm start moves q by up to 6e-9 on the CPU over these runs),
    all inside the closed-loop tolerance 1e-8, which therefore stays the ADMM bound."""
    xs, ends = case
    ref = run_multirate_ref(N, xs, ends, steps, dt=dt, sim_dt=sim_dt, radius=radius, control=control, qp_mode=mode)
    got = _handle(lib, model, N, 4, mode, dt).mpc_run_multirate(xs, ends, steps, sim_dt=sim_dt, goal_radius=radius,
                                                                control_from=control)
    tag = f"{(N, steps, dt, sim_dt, radius, control)} {mode}"
    # the reference alone: every distance clear of the radius, and the events the cases were built for
    assert np.nanmin(ref["margin"]) >= GAP, (tag, np.nanmin(ref["margin"]))
    if radius == 1e-2:
        assert np.isfinite(ref["dist"]).all() and (ref["dist"] > radius).all()
    else:
        assert ref["dist"][0, 0] < radius and ref["dist"][1, 0] < radius and np.isnan(ref["dist"][2:, 0]).all()
        assert np.isfinite(ref["dist"][:, 1:]).all()
    err = {k: np.nanmax(np.abs(got[k] - ref[k])) for k in ("dist", "q", "xpath", "u")}
    print(f"{tag}: min margin {np.nanmin(ref['margin']):.3g}, max |got - ref| " +
          ", ".join(f"{k} {v:.3g}" for k, v in err.items()))
    for key in ("dist", "q", "xpath"):
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(ref[key]), err_msg=key)
    # u of step 0 is the initial solve's control (a run of 0 steps returns that XU), bit for bit
    start = _handle(lib, model, N, 4, mode, dt).mpc_run_multirate(xs, ends, 0)["xu"]
    np.testing.assert_array_equal(got["u"][0], start[:, 12:18])
    for key in ("dist", "q", "xpath"):
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL[mode], err_msg=key)
    # the final state
    last = np.array([np.flatnonzero(np.isfinite(got["q"][:, b, 0]))[-1] for b in range(4)])
    np.testing.assert_array_equal(got["xcur"][:, :6], got["q"][last, np.arange(4)])
    np.testing.assert_array_equal(got["xu"][:, :12], got["xcur"])
    np.testing.assert_array_equal(got["xu"][:, -12:], np.tile(PIN, (4, 1)))
    # the schedule: the library's count of sub-steps after every step is the binding's offset
    np.testing.assert_array_equal(got["sub_start"], ref["sub_start"])
    np.testing.assert_array_equal(got["shift"], ref["shift"])
    n_sub = C.c_int32(-1)
    for i in range(steps + 1):
        assert lib.load().i7m_multirate_substeps(dt, sim_dt, N, i, C.byref(n_sub)) == 0
        assert n_sub.value == got["sub_start"][i]
    # q is the path's entry after each step's last sub-step
    np.testing.assert_array_equal(got["q"], got["xpath"][got["sub_start"][1:] - 1])


def test_step0_control_is_the_initial_solves(lib, model, case):
    """u[0] is XU[12:18] of the initial solve bit for bit: a run of 0 steps returns that XU."""
    xs, ends = case
    for mode in ("direct", "admm"):
        h = _handle(lib, model, 8, 4, mode)
        zero = h.mpc_run_multirate(xs, ends, 0)
        assert zero["dist"].shape == (0, 4) and zero["xpath"].shape == (0, 4, 6) and zero["sub_start"].tolist() == [0]
        np.testing.assert_array_equal(zero["xcur"], xs)  # (XU[:12] is the solve's x_0: pinned only by a step)
        assert np.isfinite(zero["xu"]).all() and np.abs(zero["xu"][:, 12:18]).max() > 0
        one = h.mpc_run_multirate(xs, ends, 1)
        np.testing.assert_array_equal(one["u"][0], zero["xu"][:, 12:18])


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_instances_are_independent(lib, model, case, mode):
    """Sixteen rows of two distinct states give bitwise-equal copies, and a B = 1 run equals its row."""
    xs, ends = case
    kw = dict(sim_dt=0.004, goal_radius=0.1, control_from="new")
    h = _handle(lib, model, 8, 16, mode)
    full = h.mpc_run_multirate(np.tile(xs[:2], (8, 1)), ends, 5, **kw)
    assert np.isnan(full["dist"][2:, 0]).all() and np.isfinite(full["dist"][:, 1]).all()
    for key in ("dist", "q", "u", "xpath"):
        for r in range(2):
            a = full[key][:, r::2]
            np.testing.assert_array_equal(a, np.repeat(a[:, :1], 8, axis=1), err_msg=key)
    for key in ("xcur", "xu"):
        for r in range(2):
            np.testing.assert_array_equal(full[key][r::2], np.tile(full[key][r], (8, 1)), err_msg=key)
    for r in range(2):
        one = h.mpc_run_multirate(xs[r:r + 1], ends, 5, **kw)
        for key in ("dist", "q", "u", "xpath"):
            np.testing.assert_array_equal(one[key][:, 0], full[key][:, r], err_msg=key)
        np.testing.assert_array_equal(one["xcur"][0], full["xcur"][r])
        np.testing.assert_array_equal(one["xu"][0], full["xu"][r])


def test_staggered_ranges(lib, model, case):
    """B = 3072 ADMM instances run as two staggered ranges (i7m_plan.h admm_stagger_min_b): every
    copy of a state is bitwise equal across both ranges, and equals the B = 4 run to the ADMM
    tolerance."""
    xs, ends = case
    kw = dict(sim_dt=0.004, goal_radius=0.1, control_from="new")
    big = _handle(lib, model, 8, 3072, "admm").mpc_run_multirate(np.tile(xs, (768, 1)), ends, 3, **kw)
    small = _handle(lib, model, 8, 4, "admm").mpc_run_multirate(xs, ends, 3, **kw)
    assert np.isnan(big["dist"][2, 0]) and np.isfinite(big["dist"][:, 1:4]).all()
    for key in ("dist", "q", "u", "xpath"):
        a = big[key].reshape(big[key].shape[0], 768, 4, -1)
        np.testing.assert_array_equal(a, np.repeat(a[:, :1], 768, axis=1), err_msg=key)
        np.testing.assert_array_equal(np.isnan(a[:, 0]), np.isnan(small[key].reshape(a[:, 0].shape)), err_msg=key)
    for key in ("dist", "q", "xpath"):
        np.testing.assert_allclose(big[key][:, :4], small[key], rtol=0, atol=TOL["admm"], err_msg=key)
    for key in ("xcur", "xu"):
        a = big[key].reshape(768, 4, -1)
        np.testing.assert_array_equal(a, np.repeat(a[:1], 768, axis=0), err_msg=key)


def test_drop_in_mpc_gato_batch(lib, model, case):
    """MPC_GATO_Batch.run_mpc: row 0's path (one q per sub-step up to the stop) and the reference's
    stats keys, logged at the reference's steps; other batch sizes than the solver map's raise."""
    from indy7_mpc_amd.gato_mpc_batch import GATO_Batch, MPC_GATO_Batch, logged_steps

    xs, ends = case
    ctrl = MPC_GATO_Batch(model, N=8, batch_size=4)
    xpath, stats = ctrl.run_mpc(xs[1], ends, sim_dt=0.004, sim_time=0.032)
    r = ctrl.last
    assert r["dist"].shape == (8, 4) and np.isfinite(r["dist"]).all()
    for key in ("dist", "q", "u", "xpath"):  # identical rows, bitwise
        np.testing.assert_array_equal(r[key], np.repeat(r[key][:, :1], 4, axis=1), err_msg=key)
    assert len(xpath) == r["sub_start"][-1] == 10 and all(np.shape(q) == (6,) for q in xpath)
    np.testing.assert_array_equal(np.array(xpath), r["xpath"][:, 0])
    assert set(stats) == {"solve_times", "goal_distances", "control_inputs"}
    # the reference's float test, literally: abs((i * sim_dt) % 0.05) < 1e-10
    log = [i for i in range(8) if abs((i * 0.004) % 0.05) < 1e-10]
    assert log == [0] and logged_steps(8, 0.004).tolist() == log
    assert stats["goal_distances"] == [float(round(r["dist"][0, 0], 5))]
    np.testing.assert_array_equal(stats["control_inputs"], np.round(r["u"][:1, 0], 5))
    assert len(stats["solve_times"]) == 1 and stats["solve_times"][0] >= 0
    # a row that stops: the path ends with the last step that ran its plant
    xpath0, stats0 = MPC_GATO_Batch(model, N=8, batch_size=4).run_mpc(xs[0], ends, sim_dt=0.004, sim_time=0.032)
    assert len(xpath0) == 1 and len(stats0["goal_distances"]) == 1
    with pytest.raises(ValueError, match="Batch size 3 not supported"):
        MPC_GATO_Batch(model, N=8, batch_size=3)
    with pytest.raises(ValueError, match="Batch size 3 not supported"):
        GATO_Batch(N=8, batch_size=3)


def test_drop_in_gato_batch_solver(lib, model, case):
    """GATO_Batch.solve is the batched solve with the reference's stats keys appended to."""
    from indy7_mpc_amd.gato_mpc_batch import GATO_Batch

    xs, ends = case
    N = 8
    s = GATO_Batch(N=N, batch_size=4, model=model)
    XU = np.zeros((4, 18 * N - 6))
    XU[:, :12] = xs
    out = s.solve(xs, np.tile(ends[0], (4, N)), XU)
    s.reset()
    np.testing.assert_array_equal(out, _handle(lib, model, N, 4, "admm").mpc_run_multirate(xs, ends, 0)["xu"])
    st = s.get_stats()
    assert set(st) == {"solve_time", "sqp_iters", "pcg_iters", "step_size"}
    assert len(st["solve_time"]["values"]) == 1 and len(st["sqp_iters"]["values"]) == 1 and st["pcg_iters"]["values"]


def test_drop_in_mpc_gato(lib, model, case):
    """MPC_GATO.run_mpc is mpc_run_multirate with the reference's constants (0.02, 1e-2, PREV)."""
    from indy7_mpc_amd.gato_mpc import MPC_GATO

    xs, ends = case
    ctrl = MPC_GATO(model, N=16)
    xpath, stats = ctrl.run_mpc(xs[1], ends, sim_time=0.12)
    want = _handle(lib, model, 16, 1, "admm").mpc_run_multirate(xs[1:2], ends, 6, sim_dt=0.02, goal_radius=1e-2,
                                                                control_from="prev")
    assert want["shift"].tolist() == [2] * 6 and len(xpath) == 12
    np.testing.assert_array_equal(np.array(xpath), want["xpath"][:, 0])
    log = [i for i in range(6) if abs((i * 0.02) % 0.05) < 1e-10]
    np.testing.assert_array_equal(stats["goal_distances"], np.round(want["dist"][log, 0], 5))
    np.testing.assert_array_equal(stats["control_inputs"], np.round(want["u"][log, 0], 5))
    # and PREV differs from NEW on the same inputs
    new = _handle(lib, model, 16, 1, "admm").mpc_run_multirate(xs[1:2], ends, 6, sim_dt=0.02, goal_radius=1e-2)
    assert not np.array_equal(new["q"], want["q"])


def test_refusals(lib, model, case):
    """I7M_EINVAL with a message naming the argument, before any device work."""
    xs, ends = case
    N = 8
    with pytest.raises(lib.I7MError, match="I7M_QP_BOX"):
        lib.Handle(model, N=N, max_batch=4, qp_mode=lib.QP_BOX).mpc_run_multirate(xs, ends, 2)
    h = _handle(lib, model, N, 4, "direct")
    h.set_external_wrench(np.ones((4, 6)))
    with pytest.raises(lib.I7MError, match="external wrench"):
        h.mpc_run_multirate(xs, ends, 2)
    h.set_external_wrench(None)
    h.ctrl_begin(np.tile(ends[0], (4, 1)), np.zeros((4, 6)), x0=xs[:1])
    with pytest.raises(lib.I7MError, match="controller session open"):
        h.mpc_run_multirate(xs, ends, 2)
    h.ctrl_end()
    h.set_external_wrench(None)
    for bad in (0.0, -0.001, float("nan")):
        with pytest.raises(lib.I7MError, match="sim_dt must be finite and > 0"):
            h.mpc_run_multirate(xs, ends, 2, sim_dt=bad)
    with pytest.raises(lib.I7MError, match="N - 1 = 7 knots in step 0"):
        h.mpc_run_multirate(xs, ends, 2, sim_dt=0.2)
    with pytest.raises(lib.I7MError, match="max_batch"):
        h.mpc_run_multirate(np.tile(xs, (2, 1)), ends, 2)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = h._lib.i7m_mpc_run_multirate(h._h, 4, dp(xs), dp(ends), 2, 2, None, None, None, None, None, None, None)
    assert rc == -1 and b"dist_out" in h._lib.i7m_last_error()
    # the binding asks i7m_multirate_substeps first; the run itself refuses the same way
    d1 = np.empty((2, 4))
    for sim_dt, msg in ((0.0, b"mpc_run_multirate: sim_dt must be finite"), (float("nan"), b"mpc_run_multirate: sim_dt must"),
                        (0.2, b"mpc_run_multirate: sim_dt = 0.200000 completes more than N - 1 = 7 knots in step 0")):
        o = lib.i7m_multirate_opts()
        assert h._lib.i7m_multirate_opts_default(C.byref(o)) == 0
        assert (o.sim_dt, o.goal_radius, o.control_from, o.reset_what) == (0.001, 0.1, lib.CONTROL_NEW, lib.ADMM_RESET_ALL)
        o.sim_dt = sim_dt
        rc = h._lib.i7m_mpc_run_multirate(h._h, 4, dp(xs), dp(ends), 2, 2, C.byref(o), dp(d1), None, None, None, None, None)
        assert rc == -1 and msg in h._lib.i7m_last_error(), h._lib.i7m_last_error()
    n_sub = C.c_int32(-1)
    assert h._lib.i7m_multirate_substeps(0.01, 0.2, N, 2, C.byref(n_sub)) == -1 and b"N - 1 = 7" in h._lib.i7m_last_error()
    # nothing ran and nothing was left behind: num_steps = 0 is accepted and is the initial solve,
    # with every optional output null too
    d = np.empty((1, 4))  # (not written with 0 steps, but a real pointer)
    xu = np.empty((4, 18 * N - 6))
    assert h._lib.i7m_mpc_run_multirate(h._h, 4, dp(xs), dp(ends), 2, 0, None, dp(d), None, None, None, None, dp(xu)) == 0
    np.testing.assert_array_equal(xu, h.mpc_run_multirate(xs, ends, 0)["xu"])
    assert np.isfinite(xu).all()
