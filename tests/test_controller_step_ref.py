"""CPU: tests/controller_step_ref.py (the controller session in numpy on the port) pinned to
tests/tracking_mpc_ref.py.  With x0 given, a constant elapsed = sim_dt = 0.01, the offsets i + 1 and
oracle.rbd.rk4 under f_actual as the plant, a session is i7m_mpc_run_tracking's loop with the plant
moved outside: best and fbest must be identical, err, q and ee agree to 1e-12."""
import numpy as np
import pytest

from controller_step_ref import HostPlant, run_ctrl_ref, schedule
from indy7_mpc_amd.utils import figure8
from tracking_mpc_ref import make_tracking_case, run_tracking_ref

REF = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
REF.setflags(write=False)


@pytest.mark.parametrize("mode,noisy", [("direct", False), ("admm", False), ("admm", True)])
def test_session_with_the_plant_outside_is_the_tracking_loop(mode, noisy):
    G, H, N, steps = 2, 4, 8, 5
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3)) if noisy else None
    kw = dict(noise=noise, keep_best=noisy, decay=0.97 if noisy else 1.0, qp_mode=mode)
    off = np.arange(1, steps + 1)
    trk = run_tracking_ref(N, G, H, xs, REF, off, fhyp, fact, ref_phase=[0, 17], sim_dt=0.01, **kw)
    el = np.full(steps, 0.01)
    got = run_ctrl_ref(N, G, H, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs, ref_phase=[0, 17], **kw)
    np.testing.assert_array_equal(got["best"], trk["best"])
    np.testing.assert_array_equal(got["fbest"], trk["fbest"])
    if not noisy:
        np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))
    for a, b in ((got["err"], trk["err"]), (got["x_meas"][:, :, :6], trk["q"]), (got["ee"], trk["ee"]),
                 (got["err2"], trk["err2"]), (got["xu_best"], trk["xu_best"]), (got["fhyp"], trk["fhyp"])):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got["u"][-1], got["xu_best"][:, 12:18])


def test_constructor_form_selects_row_zero_first_then_the_true_hypothesis():
    """x0 = None: the first step has x_last = x_meas and u_last = 0, so each hypothesis's error is the
    change of state it predicts over the elapsed time under zero torque; here that is smallest for
    row 0, the zero wrench, and far from a tie.  From the second step on the true hypothesis k wins."""
    G, H, N, steps = 3, 4, 8, 6
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    el, off = schedule(steps)
    assert off.tolist() == [1, 1, 3, 4, 4, 6]
    got = run_ctrl_ref(N, G, H, REF, fhyp, el, off, HostPlant(xs, fact, el, hold_first=True), qp_mode="direct")
    np.testing.assert_array_equal(got["x_meas"][0], xs)
    assert not got["best"][0].any()
    np.testing.assert_array_equal(got["best"][1:], np.tile(k, (steps - 1, 1)))
    assert ((got["err2"][:, :, 1] - got["err2"][:, :, 0]) >= 1e-3).all()
