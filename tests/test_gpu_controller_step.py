"""GPU: the controller session (i7m_ctrl_begin / i7m_ctrl_step / i7m_ctrl_end, csrc/i7m_ctrl.h: one
controller step per call on a state measured outside the device; the deployed controller's
joint_callback, reference gato_controller.py:201-250) against the same steps in numpy on the C++
port (tests/controller_step_ref.py).

The selected hypothesis is a discrete result, so every parity case first asserts, on the reference
alone, that at every step the two smallest scoring errors are at least 1e-3 apart; then best and
fbest must be identical.  Closed-loop comparisons use the project's closed-loop tolerances
(tests/test_gpu_tracking_mpc.py: 2e-6 direct, 1e-8 ADMM).  Every case runs in both forms of
i7m_ctrl_begin: x0 given, and x0 = NULL (the controller's constructor) with the first measurement
equal to the start state.  The clock is uneven (controller_step_ref.ELAPSED), so the window moves by
0, 1 or 2 points a step.

The control itself (replay parity): u reaches 1.2e3 N m on these random starts.  With the same
measurements at every step, the largest |u - u_ref| / (1 + |u_ref|) measured on an MI355X over all
cases and both forms is 1.9e-12 in direct mode (4.8e-12 in the closed loop) and 1.494e-8 in ADMM
mode (the resampling case with x0 given; 8.2e-9 at (3, 4, 8), 7.6e-9 at the deployed shape; 1.0e-8
in the closed loop).  Direct mode is asserted against TOL["direct"].  The ADMM figure exceeds
TOL["admm"] = 1e-8 while the closed-loop parity holds at TOL, so, as the issue that asked for this
test prescribes, its bound is twice the measured value, 2.99e-8 (U_TOL).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from controller_step_ref import HostPlant, run_ctrl_ref, schedule
from indy7_mpc_amd.utils import figure8
from sampled_mpc_ref import make_case
from tracking_mpc_ref import make_tracking_case

pytestmark = pytest.mark.gpu
TOL = {"direct": 2e-6, "admm": 1e-8}
U_TOL = {"direct": TOL["direct"], "admm": 2 * 1.494e-8}  # the control's bound: the module docstring
GAP = 1e-3
REF = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
REF.setflags(write=False)

# name: (G, H, N), seed, mode, steps, resampling
CASES = {
    "groups-direct": ((3, 4, 8), 11, "direct", 6, False),  # groups, a partial wave, the window moving unevenly
    "groups-admm": ((3, 4, 8), 11, "admm", 6, False),
    "deployed": ((1, 16, 64), 12, "admm", 3, False),       # the deployed shape, reset ALL
    "two-waves": ((1, 128, 8), 14, "direct", 6, False),    # the cross-wave argmin
    "resample": ((2, 8, 16), 11, "admm", 5, True),
}
FORMS = ["x0", "null"]


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, N, rows, mode):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def _inputs(name):
    (G, H, N), seed, mode, steps, noisy = CASES[name]
    xs, fhyp, fact, k = make_tracking_case(G, H, seed)
    el, off = schedule(steps)
    noise = np.random.default_rng(5).normal(0, 2.0, (5, 16, 3)) if noisy else None
    kw = dict(keep_best=True, decay=0.97) if noisy else {}
    return G, H, N, mode, steps, xs, fhyp, fact, k, el, off, noise, kw


@functools.lru_cache(maxsize=None)
def _reference(name, form):
    """The helper closing the loop with its own control and the host plant: computed once per case
    and form, shared (read only) by the closed-loop and the replay tests."""
    G, H, N, mode, steps, xs, fhyp, fact, k, el, off, noise, kw = _inputs(name)
    ref = run_ctrl_ref(N, G, H, REF, fhyp, el, off, HostPlant(xs, fact, el, hold_first=form == "null"),
                       x0=xs if form == "x0" else None, noise=noise, qp_mode=mode, **kw)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _run_session(h, G, ref, fhyp, el, off, measure, x0=None, noise=None, phases=None, between=None, **kw):
    """begin, one step per entry of el, end.  measure: (steps, G, 12) or measure(i, u_prev)."""
    out = dict(u0=h.ctrl_begin(ref, fhyp, x0=x0, groups=G, ref_phase=phases, **kw))
    u_prev, rows = out["u0"], []
    for i in range(len(el)):
        xm = np.array(measure(i, u_prev) if callable(measure) else measure[i])
        r = h.ctrl_step(xm, el[i], off[i], noise=None if noise is None else noise[i])
        r["x_meas"] = xm
        rows.append(r)
        u_prev = r["u"]
        if between:
            between(i)
    out.update({key: np.stack([r[key] for r in rows]) for key in rows[0]})
    out.update(h.ctrl_end())
    return out


def _check_condition(tag, ref, form, k, noisy):
    gap = ref["err2"][:, :, 1] - ref["err2"][:, :, 0]
    assert (gap >= GAP).all(), (tag, gap.min())
    first = 1 if form == "null" else 0
    if form == "null":  # x_last = x_meas, u_last = 0: the first step selects row 0 in every case
        assert not ref["best"][0].any()
    if not noisy:  # the hypotheses stay as drawn: from then on every group names its true one
        np.testing.assert_array_equal(ref["best"][first:], np.tile(k, (len(ref["best"]) - first, 1)))
    return gap.min()


def _rel_u(got, ref):
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_closed_loop_parity(lib, model, name, form):
    """The plant on the host (oracle.rbd.rk4 under f_actual) fed the device's control, against the
    helper closing the same loop with its own."""
    G, H, N, mode, steps, xs, fhyp, fact, k, el, off, noise, kw = _inputs(name)
    ref = _reference(name, form)
    gap = _check_condition(name, ref, form, k, noise is not None)
    got = _run_session(_handle(lib, model, N, G * H, mode), G, REF, fhyp, el, off,
                       HostPlant(xs, fact, el, hold_first=form == "null"), x0=xs if form == "x0" else None, noise=noise, **kw)
    d = {key: np.abs(got[key] - ref[key]).max() for key in ("x_meas", "err", "ee")}
    print(f"closed loop {name} {form}: min gap {gap:.3g}, max |device - reference| " +
          ", ".join(f"{key} {v:.3g}" for key, v in d.items()) + f", u (relative) {_rel_u(got['u'], ref['u']):.3g}")
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    for key in ("x_meas", "err", "ee"):
        assert np.isfinite(got[key]).all(), key
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL[mode], err_msg=key)
    np.testing.assert_array_equal(got["u"][-1], got["xu_best"][:, 12:18])
    if noise is None:
        np.testing.assert_array_equal(got["fhyp"], fhyp)
    else:
        assert np.abs(got["fhyp"] - ref["fhyp"]).max() <= 1e-12
        assert not got["fhyp"][::H].any() and not got["fhyp"][:, 3:].any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_replay_parity(lib, model, name, form):
    """The helper's recorded measurements fed to the device: the same inputs at every step, so err
    and ee agree to 1e-12 and the control is compared directly, as |du| / (1 + |u_ref|) <= U_TOL[mode]
    (measured: the module docstring)."""
    G, H, N, mode, steps, xs, fhyp, fact, k, el, off, noise, kw = _inputs(name)
    ref = _reference(name, form)
    _check_condition(name, ref, form, k, noise is not None)
    got = _run_session(_handle(lib, model, N, G * H, mode), G, REF, fhyp, el, off, ref["x_meas"],
                       x0=xs if form == "x0" else None, noise=noise, **kw)
    du = max(_rel_u(got["u"], ref["u"]), _rel_u(got["u0"], ref["u0"]))
    print(f"replay {name} {form} ({mode}): max |du| / (1 + |u_ref|) {du:.3g}, max |u_ref| {np.abs(ref['u']).max():.3g}, "
          f"err {np.abs(got['err'] - ref['err']).max():.3g}, ee {np.abs(got['ee'] - ref['ee']).max():.3g}")
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    for key in ("err", "ee"):
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=1e-12, err_msg=key)
    assert np.isfinite(got["u"]).all()
    assert du <= U_TOL[mode]


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_against_the_merged_loop(lib, model, mode):
    """x0 given, a constant elapsed of 0.01, offsets i + 1 and a second handle's i7m_rk4 under
    f_actual as the plant: the session is i7m_mpc_run_tracking's loop with the plant outside.  The
    two rk4 call sites need not round alike, so this is within TOL, not bit for bit."""
    G, H, N, steps = 3, 4, 8, 6
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    off = np.arange(1, steps + 1)
    trk = _handle(lib, model, N, G * H, mode).mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=0.01)
    plant, state = _handle(lib, model, N, G, mode), [xs.copy()]

    def measure(i, u):
        q, v = plant.rk4(state[0][:, :6], state[0][:, 6:], u, 0.01, fext=fact, frame="world")
        state[0] = np.concatenate([q, v], axis=1)
        return state[0]

    got = _run_session(_handle(lib, model, N, G * H, mode), G, REF, fhyp, np.full(steps, 0.01), off, measure, x0=xs)
    np.testing.assert_array_equal(got["best"], trk["best"])
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))
    np.testing.assert_array_equal(got["fbest"], trk["fbest"])
    for a, b, key in ((got["err"], trk["err"], "err"), (got["x_meas"][:, :, :6], trk["q"], "q"), (got["ee"], trk["ee"], "ee")):
        print(f"merged loop {mode}: max |session - mpc_run_tracking| {key} {np.abs(a - b).max():.3g}")
        np.testing.assert_allclose(a, b, rtol=0, atol=TOL[mode], err_msg=key)


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_groups_are_independent(lib, model, mode):
    """G = 3 with phases (0, 17, 50) and resampling equals, bit for bit, three G = 1 sessions on the
    reference cut at those phases (as test_ref_phase_is_a_cut_of_the_reference)."""
    G, H, N, steps = 3, 4, 8, 4
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    noise = np.random.default_rng(6).normal(0, 2.0, (steps, G * H, 3))
    el, off = schedule(steps)
    phases = [0, 17, 50]
    kw = dict(keep_best=True, decay=0.97)
    h = _handle(lib, model, N, G * H, mode)
    full = _run_session(h, G, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs, noise=noise, phases=phases, **kw)
    assert np.abs(full["err"][:, 1] - full["err"][:, 0]).min() > 1e-6
    for g in range(G):
        r = slice(g * H, (g + 1) * H)
        one = _run_session(h, 1, REF[phases[g]:], fhyp[r], el, off, full["x_meas"][:, g:g + 1], x0=xs[g:g + 1],
                           noise=noise[:, r], **kw)
        np.testing.assert_array_equal(one["u0"][0], full["u0"][g])
        for key in ("u", "best", "fbest", "err", "ee"):
            np.testing.assert_array_equal(one[key][:, 0], full[key][:, g], err_msg=f"{key} group {g}")
        np.testing.assert_array_equal(one["xu_best"][0], full["xu_best"][g])
        np.testing.assert_array_equal(one["fhyp"], full["fhyp"][r])


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_no_residue(lib, model, mode):
    """A second session on the same handle equals the first bit for bit, a query between two steps
    changes nothing, and after i7m_ctrl_end the handle runs i7m_mpc_run_tracking as a fresh one does
    (and keeps the final hypotheses as its wrench)."""
    G, H, N, steps = 2, 4, 8, 4
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    noise = np.random.default_rng(9).normal(0, 2.0, (steps, G * H, 3))
    el, off = schedule(steps)
    kw = dict(noise=noise, keep_best=True, decay=0.97)
    h = _handle(lib, model, N, G * H, mode)
    first = _run_session(h, G, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs, **kw)
    qs = np.random.default_rng(1).uniform(-1, 1, (37, 6))
    ee = []
    again = _run_session(h, G, REF, fhyp, el, off, first["x_meas"], x0=xs, between=lambda i: ee.append(h.eepos(qs)), **kw)
    for key in first:
        np.testing.assert_array_equal(again[key], first[key], err_msg=key)
    assert len(ee) == steps and np.isfinite(ee[0]).all()
    null = _run_session(h, G, REF, fhyp, el, off, first["x_meas"], **kw)  # and the other form after it
    assert np.isfinite(null["u"]).all() and not null["best"][0].any()
    trk_kw = dict(noise=noise, sim_dt=0.01, keep_best=True, decay=0.97)
    after = h.mpc_run_tracking(xs, REF, off, fhyp, fact, **trk_kw)
    fresh = _handle(lib, model, N, G * H, mode).mpc_run_tracking(xs, REF, off, fhyp, fact, **trk_kw)
    for key in fresh:
        np.testing.assert_array_equal(after[key], fresh[key], err_msg=key)
    h2 = _handle(lib, model, N, G * H, mode)
    _run_session(h2, G, REF, fhyp, el[:1], off[:1], first["x_meas"], x0=xs)
    with pytest.raises(lib.I7MError, match="external wrench"):  # the final hypotheses stay on the handle
        h2.mpc_run(xs, make_case(G, H, seed=1)[1], 1)


def _raw_begin(lib, h, G, H, x0, ref, fhyp, L=None, stride=None, phase=None, frame=None, reset_what=None):
    """i7m_ctrl_begin through ctypes with arguments the binding would not pass."""
    dp = lambda a: None if a is None else np.ascontiguousarray(a, float).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    o = lib.i7m_sampled_opts()
    assert h._lib.i7m_sampled_opts_default(C.byref(o)) == 0
    if frame is not None:
        o.frame = frame
    if reset_what is not None:
        o.reset_what = reset_what
    ph = None if phase is None else np.asarray(phase, np.int32)
    keep = [np.ascontiguousarray(a, float) if a is not None else None for a in (x0, ref, fhyp)]
    rc = h._lib.i7m_ctrl_begin(h._h, G, H, dp(keep[0]), dp(keep[1]), 300 if L is None else L, 6 if stride is None else stride,
                               None if ph is None else ph.ctypes.data_as(C.POINTER(C.c_int32)), dp(keep[2]), C.byref(o),
                               None)
    if rc:
        raise lib.I7MError(h._lib.i7m_last_error().decode())


def _raw_step(lib, h, x_meas, u_out=True, elapsed=0.01, off=0):
    xm = None if x_meas is None else np.ascontiguousarray(x_meas, float)
    u = np.empty((64, 6))
    dp = C.POINTER(C.c_double)
    rc = h._lib.i7m_ctrl_step(h._h, None if xm is None else xm.ctypes.data_as(dp), elapsed, off, None,
                              u.ctypes.data_as(dp) if u_out else None, None, None, None, None)
    if rc:
        raise lib.I7MError(h._lib.i7m_last_error().decode())


def test_refusals_of_begin(lib, model):
    """I7M_EINVAL with a message naming the argument, before any device work."""
    G, H, N = 2, 4, 8
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    hb = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_BOX)
    with pytest.raises(lib.I7MError, match="I7M_QP_BOX"):
        hb.ctrl_begin(REF, fhyp, x0=xs)
    h = _handle(lib, model, N, G * H, "direct")
    with pytest.raises(lib.I7MError, match="H = 3"):
        h.ctrl_begin(REF, np.zeros((3, 6)), x0=xs[:1])
    with pytest.raises(lib.I7MError, match="max_batch"):
        h.ctrl_begin(REF, np.tile(fhyp, (2, 1)), x0=np.tile(xs, (2, 1)))
    with pytest.raises(lib.I7MError, match="max_batch"):
        _raw_begin(lib, h, -1, H, None, REF, fhyp)
    with pytest.raises(lib.I7MError, match="L = 0"):
        h.ctrl_begin(REF[:0], fhyp, x0=xs)
    for cols in (4, 2):
        with pytest.raises(lib.I7MError, match=f"ref_stride = {cols}"):
            h.ctrl_begin(np.zeros((50, cols)), fhyp, x0=xs)
    with pytest.raises(lib.I7MError, match=r"ref_phase\[1\]"):
        h.ctrl_begin(REF, fhyp, x0=xs, ref_phase=[0, -1])
    with pytest.raises(lib.I7MError, match="frame"):
        _raw_begin(lib, h, G, H, xs, REF, fhyp, frame=5)
    with pytest.raises(lib.I7MError, match="RESET"):
        h.ctrl_begin(REF, fhyp, x0=xs, reset_what=8)
    with pytest.raises(lib.I7MError, match="null ref"):
        _raw_begin(lib, h, G, H, xs, None, fhyp)
    with pytest.raises(lib.I7MError, match="null fhyp"):
        _raw_begin(lib, h, G, H, xs, REF, None)
    # without a session
    with pytest.raises(lib.I7MError, match="no controller session"):
        h.ctrl_step(xs, 0.01, 0)
    with pytest.raises(lib.I7MError, match="no controller session"):
        h.ctrl_end()
    # nothing ran: no wrench was left on the handle, so the plain closed loop still accepts it
    d, _, _, _ = h.mpc_run(xs, make_case(G, H, seed=1)[1], 1)
    assert np.isfinite(d).all()
    h.ctrl_begin(REF, fhyp, x0=xs)
    with pytest.raises(lib.I7MError, match="already open"):
        h.ctrl_begin(REF, fhyp, x0=xs)
    h.close()  # i7m_destroy with the session open frees it


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_refusals_while_a_session_is_open(lib, model, mode):
    """The entry points that would overwrite what the session carries are refused, the others still
    work, and none of it changes the session: its next step equals, bit for bit, that of a session
    that saw none of these calls."""
    G, H, N = 2, 4, 8
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    el, off = schedule(3)
    B, T = G * H, 18 * N - 6
    xu, goals = np.zeros((B, T)), np.zeros((B, 3 * N))
    xrows = np.repeat(xs, H, axis=0)
    clean = _run_session(_handle(lib, model, N, B, mode), G, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs)
    h = _handle(lib, model, N, B, mode)
    h.ctrl_begin(REF, fhyp, x0=xs)
    steps = [h.ctrl_step(clean["x_meas"][0], el[0], off[0])]
    ends = make_case(G, H, seed=1)[1]
    refused = [
        lambda: h.solve(xrows, goals, xu), lambda: h.qp(xu, xrows, goals), lambda: h.qp_value(xu, xrows, goals),
        lambda: h.linearize(xu, goals), lambda: h.merit(xu, xu, goals), lambda: h.linesearch(xu, xu, goals),
        lambda: h.mpc_run(xs, ends, 1), lambda: h.mpc_run_sampled(xs, ends, 1, fhyp, fact),
        lambda: h.mpc_run_tracking(xs, REF, [1], fhyp, fact), lambda: h.set_external_wrench(fhyp),
        lambda: h.set_external_wrench(None), lambda: h.reset(), lambda: h.admm_reset(B), lambda: h.set_stream(0),
    ]
    for call in refused:
        with pytest.raises(lib.I7MError, match="controller session open"):
            call()
    # i7m_solve_device: refused before it looks at its (here null) device pointers
    assert h._lib.i7m_solve_device(h._h, B, None, None, None, 3, None, None) == -1
    assert b"controller session open" in h._lib.i7m_last_error()
    # still allowed: the queries, the getters, the timing calls, i7m_synchronize
    q = xs[:, :6]
    assert np.isfinite(h.eepos(q)).all() and np.isfinite(h.aba(q, q, q)).all()
    assert np.isfinite(h.aba_derivatives(q, q, q)[0]).all() and np.isfinite(h.rk4(q, q, q, 0.01)[0]).all()
    h.synchronize()
    h.kernel_times()
    if mode == "admm":
        h.admm_stats(B)
    # refused steps
    bad = clean["x_meas"][1].copy()
    bad[1, 1] = np.nan
    with pytest.raises(lib.I7MError, match=r"x_meas\[13\]"):
        h.ctrl_step(bad, el[1], off[1])
    bad[1, 1] = np.inf
    with pytest.raises(lib.I7MError, match=r"x_meas\[13\]"):
        h.ctrl_step(bad, el[1], off[1])
    for e in (0.0, -0.01, np.nan, np.inf):
        with pytest.raises(lib.I7MError, match="elapsed"):
            h.ctrl_step(clean["x_meas"][1], e, off[1])
    with pytest.raises(lib.I7MError, match="ref_offset = -1"):
        h.ctrl_step(clean["x_meas"][1], el[1], -1)
    with pytest.raises(lib.I7MError, match="null x_meas"):
        _raw_step(lib, h, None)
    with pytest.raises(lib.I7MError, match="null u_out"):
        _raw_step(lib, h, clean["x_meas"][1], u_out=False)
    steps += [h.ctrl_step(clean["x_meas"][i], el[i], off[i]) for i in (1, 2)]
    for i, r in enumerate(steps):
        for key in ("u", "best", "fbest", "err", "ee"):
            np.testing.assert_array_equal(r[key], clean[key][i], err_msg=f"{key} step {i}")
    end = h.ctrl_end()
    np.testing.assert_array_equal(end["xu_best"], clean["xu_best"])
    np.testing.assert_array_equal(end["fhyp"], clean["fhyp"])
    h.solve(xrows, goals, xu)  # the session is closed: the handle solves again


def test_gato_controller(lib, model):
    """GATO_Controller without ROS: the stats lists, the offset rule int(sum of elapsed / dt), and with
    a constant actual force equal to a drawn hypothesis and no resampling, best_ids[1:] names it."""
    from indy7_mpc_amd.gato_controller import GATO_Controller

    flat = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3)
    ctrl = GATO_Controller(flat, batch_size=4, N=8, dt=0.01, f_ext_std=10.0, f_ext_resample_std=0.0, model=model, seed=3,
                           qp_mode="direct")
    f = ctrl.f_ext_batch[2].copy()
    assert f[:3].any() and not f[3:].any() and not ctrl.f_ext_batch[0].any()
    xs = make_tracking_case(1, 4, seed=11)[0]
    el, off = schedule(6)
    plant = HostPlant(xs, f[None], el, hold_first=True)
    u = np.zeros((1, 6))
    for i in range(6):
        u = ctrl.step(plant(i, u.reshape(1, 6))[0], elapsed_time=el[i])
        assert u.shape == (6,) and np.isfinite(u).all()
    assert ctrl.dts == el.tolist() and len(ctrl.solve_times) == 6
    assert np.shape(ctrl.tracking_errors) == (6,) and np.shape(ctrl.ee_positions) == (6, 3)
    assert np.shape(ctrl.joint_positions) == (6, 6) and np.shape(ctrl.f_ext_best) == (6, 6)
    np.testing.assert_array_equal(ctrl.ee_ref_positions, REF[off, :3])  # offset = int(sum of elapsed / dt)
    assert ctrl.ref_traj_offset == pytest.approx(np.sum(el) / 0.01)
    np.testing.assert_allclose(ctrl.tracking_errors,
                               np.linalg.norm(np.array(ctrl.ee_positions) - np.array(ctrl.ee_ref_positions), axis=1),
                               rtol=0, atol=1e-15)
    assert ctrl.best_ids[0] == 0
    np.testing.assert_array_equal(ctrl.best_ids[1:], np.full(5, 2))
    np.testing.assert_array_equal(np.array(ctrl.f_ext_best)[1:], np.tile(f, (5, 1)))
    # None = wall clock since the previous call
    ctrl.step(plant.x[0])
    assert len(ctrl.dts) == 7 and 0 < ctrl.dts[-1] < 60
    ctrl.close()
    with pytest.raises(lib.I7MError, match="no controller session"):
        ctrl.step(plant.x[0], elapsed_time=0.01)
