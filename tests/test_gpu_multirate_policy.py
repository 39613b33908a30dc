"""GPU: the multi-rate closed loop with the plant under the solve's own feedback policy
(i7m_mpc_run_multirate with I7M_CONTROL_POLICY; csrc/i7m_mpc_policy.h k_mpc_multirate_policy_step),
B = 3 instances at N = 8 in both QP modes, against a host loop composed from the library's own hooks:
per step solve, qp_policy, the schedule with its knot index, the rk4 hook per plant sub-step with
u = u_j + K_j (x - x_j) formed in numpy in the kernel's order, then the shift and the pins.

The bound is measured, not chosen: the same composition with control_from="new" against the device
loop that existed before gives the hook-vs-kernel noise of the loop itself (the rk4 and eepos hooks are
other kernels than the step kernel's inlined plant), and the policy run must stay within 8 x that,
for the one 12-term product per sub-step it adds.  The goal switch and the stop are discrete, so
every case first asserts that they occur and that every distance is clear of the radius.
"""
import ctypes as C

import numpy as np
import pytest

from multirate_mpc_ref import make_case, run_multirate_ref

pytestmark = pytest.mark.gpu
N, B = 8, 3
GAP = 1e-3
KEYS = ("dist", "q", "u", "xpath")
# (sim_dt, steps): 2 to 3 knots per solve, j up to 2 within a step (and the 3-knot shift); ten solves
# per knot with the residue sub-step [0.001, 8.67e-19] of step 9, which runs in knot 1
SHAPES = [(0.025, 6), (0.001, 12)]


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


@pytest.fixture(scope="module")
def case():
    """make_case's first three rows and its two endpoints: row 0 starts within the radius of endpoint
    0 and of endpoint 1, so it switches at step 0 and stops at step 1."""
    xs, ends = make_case()
    return xs[:B], ends


def _handle(lib, model, mode, rows=B):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def kdx(K, dx):
    """K dx in the kernel's order (csrc/i7m_mpc_policy.h): t_c = K_c dx_c (+ K_{c+8} dx_{c+8}, c < 4),
    every product and sum rounded on its own, then ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7))."""
    p = K * dx[:, None, :]
    t = p[..., :8].copy()
    t[..., :4] = t[..., :4] + p[..., 8:]
    return ((t[..., 0] + t[..., 4]) + (t[..., 2] + t[..., 6])) + ((t[..., 1] + t[..., 5]) + (t[..., 3] + t[..., 7]))


def host_loop(lib, h, xs, ends, steps, sim_dt, radius, control):
    """i7m_mpc_run_multirate from the library's hooks, one launch per hook and step."""
    T = 18 * N - 6
    sub_start, sub_dt, shift, knot = lib.multirate_schedule(h.cfg.dt, sim_dt, steps, N, knots=True)
    admm = h.cfg.qp_mode == lib.QP_ADMM
    goal_idx, alive = np.zeros(B, int), np.ones(B, bool)
    goals = np.tile(ends[0], (B, N))
    xcur = xs.copy()
    XU = np.zeros((B, T))
    XU[:, :12] = xcur
    if admm:
        h.admm_reset(B)
    XU = h.solve(xcur, goals, XU)[0]
    out = dict(dist=np.full((steps, B), np.nan), q=np.full((steps, B, 6), np.nan), u=np.full((steps, B, 6), np.nan),
               xpath=np.full((sub_start[-1], B, 6), np.nan), jmax=0)
    for i in range(steps):
        if admm:
            h.admm_reset(B)
        xu_new = h.solve(xcur, goals, XU)[0]
        K = h.qp_policy(xu_new, xcur, goals, N - 1) if control == "policy" else None
        d = np.linalg.norm(h.eepos(xcur[:, :6]) - goals[:, :3], axis=1)
        run = []
        for b in np.flatnonzero(alive):
            out["dist"][i, b] = d[b]
            out["u"][i, b] = XU[b, 12:18]
            if d[b] < radius:
                if goal_idx[b] < len(ends) - 1:
                    goal_idx[b] += 1
                    goals[b] = np.tile(ends[goal_idx[b]], N)
                else:
                    alive[b] = False
                    continue
            run.append(b)
        run = np.array(run, int)
        q, v = xcur[run, :6].copy(), xcur[run, 6:].copy()
        for s in range(sub_start[i], sub_start[i + 1]):
            j = knot[s] if control == "policy" else 0
            u = xu_new[run, 18 * j + 12:18 * j + 18]
            if control == "policy":
                du = kdx(K[run, j, :, :12], np.hstack([q, v]) - xu_new[run, 18 * j:18 * j + 12])
                if s == sub_start[i] and not admm:
                    # the exact QP's x_0 is xcur, so a step begins at the nominal state: K dx is an exact
                    # zero and the first sub-step's control is control_from="new"'s, bit for bit.  (OSQP's
                    # iterate meets the x_0 rows only to its tolerance, and there the first sub-step
                    # already corrects for the difference.)
                    assert not du.any()
                u = u + du
                out["jmax"] = max(out["jmax"], int(j))
            q, v = h.rk4(q, v, u, sub_dt[s])
            out["xpath"][s, run] = q
        xcur[run] = np.hstack([q, v])
        out["q"][i, run] = q
        if shift[i] > 0:
            XU[run, :T - 18 * shift[i]] = xu_new[run, 18 * shift[i]:]
        XU[run, :12] = xcur[run]
        XU[run, -12:] = [1.0] * 6 + [0.0] * 6
    out.update(xcur=xcur, xu=XU)
    return out


def test_events_on_the_cpu_port(case):
    """The start and the endpoints give a goal switch and a stop: on the C++ port (control "new", whose
    plant differs from the policy's only from a step's second sub-step on) row 0 switches at step 0 and
    stops at step 1, rows 1 and 2 run on, and every distance is clear of the radius."""
    xs, ends = case
    for sim_dt, steps in SHAPES:
        ref = run_multirate_ref(N, xs, ends, min(steps, 3), sim_dt=sim_dt, radius=0.1, control="new")
        assert ref["dist"][0, 0] < 0.1 and ref["dist"][1, 0] < 0.1 and np.isnan(ref["dist"][2:, 0]).all()
        assert (ref["dist"][:, 1:] > 0.1).all()
        assert np.nanmin(ref["margin"]) >= GAP


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("sim_dt,steps", SHAPES)
def test_against_the_host_composed_loop(lib, model, case, sim_dt, steps, mode):
    """Structure identical, values within 8 x the NEW loop's own hook-vs-kernel noise.  Measured on an
    MI355X, max |device - host| over dist, q, u, xpath, xcur, xu: NEW 1.5e-11 / 4.9e-7
    (direct / ADMM) at sim_dt = 0.025 and 4.8e-13 / 4.9e-7 at 0.001; POLICY 1.7e-12 / 1.9e-7 and 4.8e-13 /
    4.2e-7: at or below the noise itself."""
    xs, ends = case
    h = _handle(lib, model, mode)
    res = {}
    for control in ("new", "policy"):
        host = host_loop(lib, h, xs, ends, steps, sim_dt, 0.1, control)
        dev = h.mpc_run_multirate(xs, ends, steps, sim_dt=sim_dt, goal_radius=0.1, control_from=control)
        # the events the shapes were chosen for, and clear of the radius
        assert host["dist"][0, 0] < 0.1 and host["dist"][1, 0] < 0.1 and np.isnan(host["dist"][2:, 0]).all()
        assert np.isfinite(host["dist"][:, 1:]).all()
        assert np.nanmin(np.abs(host["dist"] - 0.1)) >= GAP
        for key in KEYS:
            np.testing.assert_array_equal(np.isnan(dev[key]), np.isnan(host[key]), err_msg=f"{control} {key}")
        res[control] = {k: float(np.nanmax(np.abs(dev[k] - host[k]))) for k in KEYS + ("xcur", "xu")}
        res[control]["dev"], res[control]["host"] = dev, host
        # the final state and the pins, as the existing loop leaves them
        np.testing.assert_array_equal(dev["xu"][:, :12], dev["xcur"])
        np.testing.assert_array_equal(dev["xu"][1:, -12:], np.tile([1.0] * 6 + [0.0] * 6, (B - 1, 1)))
        np.testing.assert_array_equal(dev["q"], dev["xpath"][dev["sub_start"][1:] - 1])
    h.close()
    noise = max(res["new"][k] for k in KEYS + ("xcur", "xu"))
    for control in ("new", "policy"):
        print(f"sim_dt={sim_dt} {mode} {control}: max |device - host| " +
              ", ".join(f"{k} {res[control][k]:.3g}" for k in KEYS + ("xcur", "xu")))
    # j reaches 3 at sim_dt = 0.025 (a float residue sub-step after a step's third knot), 1 at 0.001
    assert res["policy"]["host"]["jmax"] == (3 if sim_dt == 0.025 else 1)
    # the feedback is not a no-op: from a step's second sub-step on the policy's plant leaves NEW's
    # (with one sub-step per solve every sub-step begins at the nominal state and the runs coincide but
    # for step 9's residue)
    if sim_dt == 0.025:
        assert not np.array_equal(res["policy"]["dev"]["xpath"], res["new"]["dev"]["xpath"])
    for k in KEYS + ("xcur", "xu"):
        assert res["policy"][k] <= 8 * noise, (k, res["policy"][k], noise)


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_zero_gains_reduce_to_new(lib, model, case, monkeypatch, mode):
    """I7M_POLICY_ZERO_K=1 at handle creation zeroes the policy pass's gains, so sub-step s is driven by
    xu_new.u_j + 0 with j = its knot index.  Where every sub-step begins in knot 0 that is
    control_from="new"'s control and the run must equal NEW's bit for bit, through the other kernel:
    sim_dt = 0.001, steps 0 .. 8, with the goal switch at step 0 and the stop at step 1.  (Once a
    sub-step begins past knot 0 the zero-gain control is knot j's, not knot 0's, and the two runs part
    by construction: sim_dt = 0.025 has no such stretch beyond a step's first sub-step.)

    Measured on an MI355X: every difference is 0 in both modes.  That rests on the sub-step loop's shape:
    rk4_step is inlined into each kernel and the compiler contracts its products by the loop around it;
    k_mpc_multirate_policy_step's loop has no barrier and no lane-conditional plant, and the same fma, mul
    and add counts per sub-step as k_mpc_multirate_step's."""
    xs, ends = case
    new = _handle(lib, model, mode).mpc_run_multirate(xs, ends, 9, sim_dt=0.001, goal_radius=0.1, control_from="new")
    monkeypatch.setenv("I7M_POLICY_ZERO_K", "1")
    hz = _handle(lib, model, mode)
    monkeypatch.delenv("I7M_POLICY_ZERO_K")
    got = hz.mpc_run_multirate(xs, ends, 9, sim_dt=0.001, goal_radius=0.1, control_from="policy")
    hz.close()
    assert new["dist"][0, 0] < 0.1 and new["dist"][1, 0] < 0.1 and np.isnan(new["dist"][2:, 0]).all()
    print(f"zero gains {mode}: max |policy - new| " +
          ", ".join(f"{k} {np.nanmax(np.abs(got[k] - new[k])):.3g}" for k in KEYS + ("xcur", "xu")))
    for key in KEYS + ("xcur", "xu"):
        np.testing.assert_array_equal(got[key], new[key], err_msg=key)


def test_refusals(lib, model, case):
    xs, ends = case
    with pytest.raises(lib.I7MError, match="I7M_QP_BOX"):
        lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_BOX).mpc_run_multirate(xs, ends, 2, control_from="policy")
    h = _handle(lib, model, "direct")
    # a step of N - 1 = 7 knots: NEW runs it, POLICY has no control for knot 7
    assert np.isfinite(h.mpc_run_multirate(xs, ends, 1, sim_dt=0.07, control_from="new")["xpath"][:, 1:]).all()
    with pytest.raises(lib.I7MError, match="mpc_run_multirate: sim_dt = 0.070000 completes more than N - 2 = 6 knots in step 0"):
        h.mpc_run_multirate(xs, ends, 1, sim_dt=0.07, control_from="policy")
    assert np.isfinite(h.mpc_run_multirate(xs, ends, 1, sim_dt=0.06, control_from="policy")["xpath"][:, 1:]).all()
    o = lib.i7m_multirate_opts()
    h._lib.i7m_multirate_opts_default(C.byref(o))
    o.control_from = 3
    d = np.empty((1, B))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert h._lib.i7m_mpc_run_multirate(h._h, B, dp(xs), dp(ends), 2, 1, C.byref(o), dp(d), None, None, None, None, None) == -1
    assert b"control_from must be I7M_CONTROL_NEW, I7M_CONTROL_PREV or I7M_CONTROL_POLICY" in h._lib.i7m_last_error()
    h.close()


def test_drivers_with_feedback(lib, model, case):
    """MPC_GATO(feedback=True) and MPC_GATO_Batch(feedback=True): ten steps at N = 8, finite paths of the
    reference's shapes, the library's POLICY run row for row, and not the feedback=False run."""
    from indy7_mpc_amd.gato_mpc import MPC_GATO
    from indy7_mpc_amd.gato_mpc_batch import MPC_GATO_Batch

    xs, ends = case
    x1 = xs[1]
    for fb in (True, False):
        m = MPC_GATO(model, N=N, qp_mode="direct", feedback=fb)
        xpath, stats = m.run_mpc(x1, ends, sim_time=0.2)
        want = _handle(lib, model, "direct", 1).mpc_run_multirate(x1[None], ends, 10, sim_dt=0.02, goal_radius=1e-2,
                                                                  control_from="policy" if fb else "prev")
        assert len(xpath) == 20 and all(q.shape == (6,) for q in xpath) and np.isfinite(np.array(xpath)).all()
        np.testing.assert_array_equal(np.array(xpath), want["xpath"][:, 0])
        assert set(stats) == {"solve_times", "goal_distances", "control_inputs"}
        mb = MPC_GATO_Batch(model, N=N, batch_size=4, qp_mode="admm", feedback=fb)
        xpath, stats = mb.run_mpc(x1, ends, sim_dt=0.001, sim_time=0.01)
        want = _handle(lib, model, "admm", 4).mpc_run_multirate(np.tile(x1, (4, 1)), ends, 10, sim_dt=0.001,
                                                                control_from="policy" if fb else "new")
        assert len(xpath) == 11 and np.isfinite(np.array(xpath)).all()
        np.testing.assert_array_equal(np.array(xpath), want["xpath"][:, 0])
        for key in ("q", "xpath"):
            np.testing.assert_array_equal(mb.last[key], np.repeat(mb.last[key][:, :1], 4, axis=1), err_msg=key)
    assert MPC_GATO(model, N=N).feedback is False and MPC_GATO_Batch(model, N=N).feedback is False
