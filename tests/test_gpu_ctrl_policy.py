"""GPU: the controller session hands out the winner's feedback policy (i7m_ctrl_set_policy /
i7m_ctrl_get_policy / i7m_ctrl_set_applied; csrc/i7m_mpc_sampled_policy.h k_ctrl_policy_copy) at
(G, H, N) = (2, 4, 8), direct.  The policy of a step is compared bit for bit with i7m_qp_policy run on
all G H rows of a twin handle that composes the step from the library's hooks (the same rows, so the
same sweep variant), row `best` taken; x_ref / u_ref are XU_best.  With the policy off a session is the
one it was.  i7m_ctrl_set_applied is checked on a case built for it: the applied torque is one that
hypothesis A explains and the nominal one that hypothesis B explains, the two scoring errors at least
1e-3 apart on the numpy helper."""
import ctypes as C

import numpy as np
import pytest

from oracle import rbd
from sampled_mpc_ref import score
from sampled_policy_ref import REF
from tracking_mpc_ref import make_tracking_case, window

pytestmark = pytest.mark.gpu
G, H, N = 2, 4, 8
T = 18 * N - 6
PHASES = (3, 40)
GAP = 1e-3


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, rows=G * H, mode="direct"):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def _measurements(steps, xs, seed=2):
    """states near the start, as a plant under some torque would deliver them"""
    rng = np.random.default_rng(seed)
    return [xs + 0.02 * (i + 1) * rng.standard_normal(xs.shape) for i in range(steps)]


def test_policy_is_qp_policy_of_the_winning_row(lib, model):
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    el, off = [0.011, 0.012], [1, 2]
    h, twin = _handle(lib, model), _handle(lib, model)
    u, x = h.ctrl_begin(REF, fhyp, x0=xs, ref_phase=PHASES), xs
    h.ctrl_set_policy(N - 1)
    with pytest.raises(lib.I7MError, match="ctrl_get_policy: no i7m_ctrl_step has run since the policy was turned on"):
        h.ctrl_get_policy()
    # the twin: begin's solve, then each step composed from the hooks
    twin.set_external_wrench(fhyp, "world")
    rows = np.repeat(xs, H, axis=0)
    goals = np.repeat(np.stack([window(REF, PHASES[g], 0, N) for g in range(G)]), H, axis=0)
    XU = np.zeros((G * H, T))
    XU[:, :12] = rows
    xu_best = twin.solve(rows, goals, XU)[0][::H].copy()
    for i in range(2):
        # the measurement: the host plant under the group's true wrench, so the winner is row k[g], not row 0
        x = np.array([np.concatenate(rbd.rk4(x[g, :6], x[g, 6:], u[g], el[i], fext6_world=fact[g])) for g in range(G)])
        r = h.ctrl_step(x, el[i], off[i])
        u = r["u"]
        np.testing.assert_array_equal(r["best"], k)
        K, xu_ref = h.ctrl_get_policy()
        assert K.shape == (G, N - 1, 6, 13) and xu_ref.shape == (G, N - 1, 18)
        rows = np.repeat(x, H, axis=0)
        goals = np.repeat(np.stack([window(REF, PHASES[g], off[i], N) for g in range(G)]), H, axis=0)
        XU = np.repeat(xu_best, H, axis=0)
        XU[:, :12] = rows
        xu_new = twin.solve(rows, goals, XU)[0]
        Kt = twin.qp_policy(xu_new, rows, goals, N - 1)
        pick = np.arange(G) * H + r["best"]
        xu_best = xu_new[pick].copy()
        np.testing.assert_array_equal(r["u"], xu_best[:, 12:18])  # the twin composes the session's step
        np.testing.assert_array_equal(K, Kt[pick], err_msg=f"step {i}")
        np.testing.assert_array_equal(xu_ref, xu_best[:, :18 * (N - 1)].reshape(G, N - 1, 18), err_msg=f"step {i}")
        assert all(not np.array_equal(Kt[pick[g]], Kt[g * H]) for g in range(G))  # not row 0's gains
    # fewer stages: the first ones, the same values
    h.ctrl_set_policy(3)
    r = h.ctrl_step(x, 0.01, 3)
    K3, xu3 = h.ctrl_get_policy()
    assert K3.shape == (G, 3, 6, 13) and xu3.shape == (G, 3, 18) and np.isfinite(K3).all()
    end = h.ctrl_end()
    np.testing.assert_array_equal(xu3, end["xu_best"][:, :54].reshape(G, 3, 18))
    twin.close()
    h.close()


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_policy_off_is_the_session_it_was(lib, model, mode):
    """Three steps with resampling: a session whose policy was turned on and off again before its steps,
    and one with the policy on, give the outputs of a session that never heard of it."""
    xs, fhyp, _, _ = make_tracking_case(G, H, seed=11)
    meas = _measurements(3, xs)
    noise = np.random.default_rng(6).normal(0, 2.0, (3, G * H, 3))
    runs = {}
    for kind in ("plain", "off", "on"):
        h = _handle(lib, model, mode=mode)
        rows = [h.ctrl_begin(REF, fhyp, x0=xs, ref_phase=PHASES, keep_best=True, decay=0.97)]
        if kind != "plain":
            h.ctrl_set_policy(N - 1)
        if kind == "off":
            h.ctrl_set_policy(0)
        for i in range(3):
            r = h.ctrl_step(meas[i], 0.011, i + 1, noise=noise[i])
            rows += [r[k] for k in ("u", "best", "fbest", "err", "ee")]
        if kind == "off":
            with pytest.raises(lib.I7MError, match="ctrl_get_policy: the session's policy is off"):
                h.ctrl_get_policy()
        end = h.ctrl_end()
        runs[kind] = rows + [end["xu_best"], end["fhyp"]]
        h.close()
    for kind in ("off", "on"):
        for a, b in zip(runs[kind], runs["plain"]):
            np.testing.assert_array_equal(a, b, err_msg=kind)


def _applied_case():
    """One group, H = 4, at rest.  Rows 1 (A) and 2 (B) are two wrenches; the torque applied is the
    nominal u0 plus the joint torque that turns B's pull into A's: under A it moves the arm as u0 does
    under B.  Returns the inputs and a function of u0 giving (u_applied, x_meas)."""
    x0 = np.zeros((1, 12))
    x0[0, :6] = [0.3, -0.4, 0.5, 0.2, -0.3, 0.1]
    fhyp = np.zeros((4, 6))
    fhyp[1, :3] = [9.0, -4.0, 6.0]   # A
    fhyp[2, :3] = [-7.0, 8.0, -5.0]  # B
    fhyp[3, :3] = [20.0, 20.0, 20.0]
    el = 0.01

    def after(u0):
        q, v = x0[0, :6], x0[0, 6:]
        P = rbd.params()
        tau = lambda f: rbd.crba(q, P) @ (rbd.aba(q, v, u0, P, rbd.fext_list(q, f, "world")) - rbd.aba(q, v, u0, P))  # noqa: E731
        u_app = u0 + tau(fhyp[2]) - tau(fhyp[1])
        qn, vn = rbd.rk4(q, v, u_app, el, fext6_world=fhyp[1])
        return u_app, np.concatenate([qn, vn])[None]
    return x0, fhyp, el, after


def test_set_applied_changes_the_next_best(lib, model):
    x0, fhyp, el, after = _applied_case()
    best = {}
    for applied in (False, True):
        h = _handle(lib, model, rows=4)
        u0 = h.ctrl_begin(REF, fhyp, x0=x0)
        u_app, x_meas = after(u0[0])
        # on the numpy helper: B explains the measurement under the nominal control, A under the applied
        # one, each clear of the other rows by 1e-3
        for u_last, want in ((u0[0], 2), (u_app, 1)):
            err, b = score(x0[0], u_last, x_meas[0], fhyp, el, "world")
            e = np.sort(err)
            assert b == want and e[1] - e[0] >= GAP, (want, err)
        if applied:
            h.ctrl_set_applied(u_app[None])
        r1 = h.ctrl_step(x_meas, el, 1)
        best[applied] = int(r1["best"][0])
        # the report holds for one step only: the next one scores against the control the step returned
        q, v = rbd.rk4(x_meas[0, :6], x_meas[0, 6:], r1["u"][0], el, fext6_world=fhyp[3])
        r2 = h.ctrl_step(np.concatenate([q, v])[None], el, 2)
        assert int(r2["best"][0]) == 3
        h.ctrl_end()
        h.close()
    assert best == {False: 2, True: 1}


def test_refusals(lib, model):
    """All three calls: I7M_EINVAL with the argument named, without a session and on a bad argument."""
    xs, fhyp, _, _ = make_tracking_case(G, H, seed=11)
    h = _handle(lib, model)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    u = np.zeros((G, 6))
    for call, args in (("ctrl_set_policy", (3,)), ("ctrl_get_policy", (None, None)), ("ctrl_set_applied", (dp(u),))):
        assert getattr(h._lib, "i7m_" + call)(h._h, *args) == -1
        assert f"{call}: no controller session is open".encode() in h._lib.i7m_last_error()
        assert getattr(h._lib, "i7m_" + call)(None, *args) == -1
    h.ctrl_begin(REF, fhyp, x0=None, groups=G)
    for bad in (-1, N, 64):
        with pytest.raises(lib.I7MError, match=rf"ctrl_set_policy: n_k = {bad} outside \[0, N - 1 = 7\]"):
            h.ctrl_set_policy(bad)
    with pytest.raises(lib.I7MError, match="ctrl_get_policy: the session's policy is off"):
        h.ctrl_get_policy()
    # no x0 and no step yet: there is no x_last to score an applied torque against
    with pytest.raises(lib.I7MError, match="ctrl_set_applied: no x_last yet"):
        h.ctrl_set_applied(u)
    h.ctrl_step(xs, 0.01, 1)
    assert h._lib.i7m_ctrl_set_applied(h._h, None) == -1 and b"ctrl_set_applied: null u_applied" in h._lib.i7m_last_error()
    for v in (np.nan, np.inf):
        u[1, 2] = v
        with pytest.raises(lib.I7MError, match=r"ctrl_set_applied: u_applied\[8\] is not finite"):
            h.ctrl_set_applied(u)
    u[1, 2] = 0.0
    h.ctrl_set_applied(u)
    h.ctrl_set_policy(2)
    with pytest.raises(lib.I7MError, match="no i7m_ctrl_step has run since the policy was turned on"):
        h.ctrl_get_policy()
    h.ctrl_step(xs, 0.01, 2)
    K, xu = h.ctrl_get_policy()
    assert np.isfinite(K).all() and np.isfinite(xu).all()
    # either output may be NULL
    assert h._lib.i7m_ctrl_get_policy(h._h, None, None) == 0
    # the session still refuses what would overwrite it, and ends as before; the next one starts with the policy off
    with pytest.raises(lib.I7MError, match="controller session open"):
        h.qp_policy(np.zeros((1, T)), xs[:1], np.zeros((1, 3 * N)), 2)
    h.ctrl_end()
    h.ctrl_begin(REF, fhyp, x0=xs)
    with pytest.raises(lib.I7MError, match="the session's policy is off"):
        h.ctrl_get_policy()
    h.close()  # i7m_destroy with a session open frees it


def test_gato_controller_policy(lib, model):
    """GATO_Controller(policy_knots=n): policy() has the documented shapes, control() at the nominal state
    of knot j, j dt after the measurement, is u_ref[j] exactly, and step takes u_applied."""
    from indy7_mpc_amd.gato_controller import GATO_Controller

    n_k = N - 1
    ctrl = GATO_Controller(REF.reshape(-1), batch_size=H, N=N, dt=0.01, f_ext_std=10.0, seed=4, model=model, qp_mode="direct",
                           policy_knots=n_k)
    x = np.zeros(12)
    u = ctrl.step(x, elapsed_time=0.01)
    p = ctrl.policy()
    assert p["K"].shape == (1, n_k, 6, 12) and p["kff"].shape == (1, n_k, 6)
    assert p["x_ref"].shape == (1, n_k, 12) and p["u_ref"].shape == (1, n_k, 6)
    np.testing.assert_array_equal(p["u_ref"][0, 0], u)
    np.testing.assert_array_equal(p["x_ref"][0, 0], x)
    for j in range(n_k):
        np.testing.assert_array_equal(ctrl.control(p["x_ref"][0, j], j * 0.01), p["u_ref"][0, j])
    np.testing.assert_array_equal(ctrl.control(p["x_ref"][0, n_k - 1], 1.0), p["u_ref"][0, n_k - 1])  # held past the last knot
    dx = 1e-3 * np.arange(12)
    np.testing.assert_allclose(ctrl.control(x + dx, 0.0), u + p["K"][0, 0] @ dx, rtol=1e-12, atol=1e-9)
    u2 = ctrl.step(x, elapsed_time=0.01, u_applied=ctrl.control(x, 0.005))
    assert np.isfinite(u2).all() and not np.array_equal(ctrl.policy()["u_ref"], p["u_ref"])
    ctrl.close()
    plain = GATO_Controller(REF.reshape(-1), batch_size=H, N=N, dt=0.01, f_ext_std=10.0, seed=4, model=model, qp_mode="direct")
    assert plain.policy_knots == 0
    np.testing.assert_array_equal(plain.step(x, elapsed_time=0.01), u)  # the default is the controller it was
    with pytest.raises(lib.I7MError, match="policy is off"):
        plain.policy()
    plain.close()
