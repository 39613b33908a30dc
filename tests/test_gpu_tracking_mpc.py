"""GPU: the reference-tracking closed loop on the device (i7m_mpc_run_tracking, the goal phase of
csrc/i7m_mpc_sampled.h; the deployed controller's loop, reference gato_controller.py:201-250)
against the same loop in numpy on the C++ port (tests/tracking_mpc_ref.py).

As in tests/test_gpu_sampled_mpc.py the selected hypothesis is a discrete result, so every parity
case first asserts, on the reference alone, that at every step the two smallest scoring errors are
at least 1e-3 apart; then best and fbest must be identical.  err, q and ee use the project's
closed-loop tolerances (tests/test_gpu_mpc.py: 2e-6 direct, 1e-8 ADMM).

The reference trajectory is the controller's figure 8 at 100 points per cycle (2-5 cm per knot), so
every window differs from the last.
"""
import ctypes as C

import numpy as np
import pytest

from indy7_mpc_amd.utils import figure8
from oracle import rbd
from sampled_mpc_ref import make_case
from tracking_mpc_ref import make_tracking_case, run_tracking_ref

pytestmark = pytest.mark.gpu
TOL = {"direct": 2e-6, "admm": 1e-8}
GAP = 1e-3
REF = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
REF.setflags(write=False)


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, N, rows, mode):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def _check_parity(tag, got, ref, mode):
    gap = ref["err2"][:, :, 1] - ref["err2"][:, :, 0]
    assert (gap >= GAP).all(), (tag, gap.min())
    d = {k: np.abs(got[k] - ref[k]).max() for k in ("err", "q", "ee")}
    print(f"{tag}: min gap {gap.min():.3g}, max |device - reference| " + ", ".join(f"{k} {v:.3g}" for k, v in d.items()))
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    for k in ("err", "q", "ee"):
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=TOL[mode], err_msg=k)
    np.testing.assert_array_equal(got["xcur"][:, :6], got["q"][-1])


@pytest.mark.parametrize("G,H,N,steps,sim_dt,mode", [
    (3, 4, 8, 6, 0.01, "direct"), (3, 4, 8, 6, 0.01, "admm"),      # the window advances every step
    (2, 4, 8, 25, 0.001, "direct"), (2, 4, 8, 25, 0.001, "admm"),  # ... at steps 9 and 19 only
])
def test_parity_without_resampling(lib, model, G, H, N, steps, sim_dt, mode):
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    off = (np.arange(steps) + 1) // (1 if sim_dt == 0.01 else 10)
    assert len(set(off.tolist())) == (steps if sim_dt == 0.01 else 3)
    ref = run_tracking_ref(N, G, H, xs, REF, off, fhyp, fact, sim_dt=sim_dt, qp_mode=mode)
    got = _handle(lib, model, N, G * H, mode).mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=sim_dt)
    _check_parity(f"tracking {(G, H, N)} sim_dt {sim_dt} {mode}", got, ref, mode)
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))
    np.testing.assert_array_equal(got["fhyp"], fhyp)


def test_parity_with_resampling(lib, model):
    G, H, N, steps = 2, 8, 16, 5
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    off = np.arange(1, steps + 1)
    kw = dict(noise=noise, sim_dt=0.01, keep_best=True, decay=0.97)
    ref = run_tracking_ref(N, G, H, xs, REF, off, fhyp, fact, qp_mode="admm", **kw)
    got = _handle(lib, model, N, G * H, "admm").mpc_run_tracking(xs, REF, off, fhyp, fact, **kw)
    _check_parity("tracking resample admm", got, ref, "admm")
    df = np.abs(got["fhyp"] - ref["fhyp"]).max()
    print(f"  max |fhyp - ref| {df:.3g}")
    assert df <= 1e-12
    assert np.abs(got["fhyp"] - fhyp).max() > 0.1 and not got["fhyp"][::H].any() and not got["fhyp"][:, 3:].any()


def test_parity_at_the_deployed_shape(lib, model):
    """16 hypotheses at N = 64, the OSQP state reset before every solve: gato_controller.py:221-223,339."""
    G, H, N, steps = 1, 16, 64, 3
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=12)
    off = np.arange(1, steps + 1)
    ref = run_tracking_ref(N, G, H, xs, REF, off, fhyp, fact, sim_dt=0.01, qp_mode="admm", reset_all=True)
    got = _handle(lib, model, N, G * H, "admm").mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=0.01,
                                                                reset_what=lib.ADMM_RESET_ALL)
    _check_parity("tracking deployed shape (1, 16, 64) admm", got, ref, "admm")
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_run_past_the_end_of_the_reference(lib, model, mode):
    """L = N + 2 and offsets up to 6: from step 2 on the windows hold the last point, and at the
    end the whole window is that point."""
    G, H, N, steps = 2, 4, 8, 6
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    short = REF[:N + 2]
    off = np.arange(1, steps + 1)
    ref = run_tracking_ref(N, G, H, xs, short, off, fhyp, fact, sim_dt=0.01, qp_mode=mode)
    got = _handle(lib, model, N, G * H, mode).mpc_run_tracking(xs, short, off, fhyp, fact, sim_dt=0.01)
    for k in ("err", "q", "ee", "xcur", "xu_best"):
        assert np.isfinite(got[k]).all(), k
    _check_parity(f"tracking past the end {mode}", got, ref, mode)
    # far past the end: the error is measured against the last point
    far = _handle(lib, model, N, G * H, mode).mpc_run_tracking(xs, short, [10 ** 9], fhyp, fact, sim_dt=0.01)
    np.testing.assert_allclose(far["err"][0], np.linalg.norm(far["ee"][0] - short[-1, :3], axis=1), rtol=0, atol=1e-15)


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_ref_phase_is_a_cut_of_the_reference(lib, model, mode):
    """G = 3 with phases (0, 17, 50) equals, bit for bit, three G = 1 runs on the reference cut at
    those phases (resampling on, so the wrench rows are written too)."""
    G, H, N, steps = 3, 4, 8, 4
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    noise = np.random.default_rng(6).normal(0, 2.0, (steps, G * H, 3))
    off = np.arange(1, steps + 1)
    phases = [0, 17, 50]
    h = _handle(lib, model, N, G * H, mode)
    kw = dict(sim_dt=0.01, keep_best=True, decay=0.97)
    full = h.mpc_run_tracking(xs, REF, off, fhyp, fact, ref_phase=phases, noise=noise, **kw)
    assert np.abs(full["err"][:, 1] - full["err"][:, 0]).min() > 1e-6
    for g in range(G):
        r = slice(g * H, (g + 1) * H)
        one = h.mpc_run_tracking(xs[g:g + 1], REF[phases[g]:], off, fhyp[r], fact[g:g + 1], noise=noise[:, r], **kw)
        for key in ("err", "best", "q", "ee", "fbest"):
            np.testing.assert_array_equal(one[key][:, 0], full[key][:, g], err_msg=f"{key} group {g}")
        np.testing.assert_array_equal(one["xcur"][0], full["xcur"][g])
        np.testing.assert_array_equal(one["xu_best"][0], full["xu_best"][g])
        np.testing.assert_array_equal(one["fhyp"], full["fhyp"][r])


def test_stride_six_equals_stride_three(lib, model):
    G, H, N, steps = 2, 4, 8, 4
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    off = np.arange(1, steps + 1)
    h = _handle(lib, model, N, G * H, "direct")
    six = REF.copy()
    six[:, 3:] = 7.0  # the last three of each point are never read
    a = h.mpc_run_tracking(xs, six, off, fhyp, fact, ref_phase=[3, 40], sim_dt=0.01)
    b = h.mpc_run_tracking(xs, np.ascontiguousarray(REF[:, :3]), off, fhyp, fact, ref_phase=[3, 40], sim_dt=0.01)
    assert np.isfinite(a["err"]).all()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_one_point_reference_is_the_endpoint_loop(lib, model, mode):
    """L = 1 far from the start: the tracking loop equals, bit for bit, mpc_run_sampled with that
    single endpoint on the same handle — the new goal phase against the merged loop."""
    G, H, N, steps = 2, 4, 8, 4
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    end = rbd.eepos(np.full(6, 0.9))
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    h = _handle(lib, model, N, G * H, mode)
    kw = dict(noise=noise, sim_dt=0.01, keep_best=True, decay=0.97)
    ends = h.mpc_run_sampled(xs, end[None], steps, fhyp, fact, **kw)
    assert (ends["dist"] > 0.095).all()
    trk = h.mpc_run_tracking(xs, end[None], [0, 1, 5, 1000], fhyp, fact, ref_phase=[0, 3], **kw)
    np.testing.assert_array_equal(trk["err"], ends["dist"])
    for key in ("q", "best", "fbest", "xcur", "xu_best", "fhyp"):
        np.testing.assert_array_equal(trk[key], ends[key], err_msg=key)


def test_stagger_cut_splits_no_group(lib, model, monkeypatch):
    """As tests/test_gpu_sampled_mpc.py's: G = 7, H = 4 as two staggered ranges equals the one-range
    run bit for bit (the window of every group is written by its own range)."""
    G, H, N = 7, 4, 8
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=13)
    noise = np.random.default_rng(7).normal(0, 2.0, (2, G * H, 3))
    phases = np.arange(G) * 9
    runs = []
    for min_b in ("8", None):
        if min_b:
            monkeypatch.setenv("I7M_ADMM_STAGGER_MIN_B", min_b)
            monkeypatch.setenv("I7M_ADMM_STAGGER", "1")
        else:
            monkeypatch.delenv("I7M_ADMM_STAGGER_MIN_B")
            monkeypatch.delenv("I7M_ADMM_STAGGER")
        h = _handle(lib, model, N, G * H, "admm")
        runs.append(h.mpc_run_tracking(xs, REF, [1, 2], fhyp, fact, ref_phase=phases, noise=noise, sim_dt=0.01))
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg=key)
    assert np.isfinite(runs[0]["err"]).all()


def test_refusals(lib, model):
    """I7M_EINVAL with a message naming the argument, before any work."""
    G, H, N = 2, 4, 8
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=11)
    off = [1, 2]
    hb = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_BOX)
    with pytest.raises(lib.I7MError, match="I7M_QP_BOX"):
        hb.mpc_run_tracking(xs, REF, off, fhyp, fact)
    h = _handle(lib, model, N, G * H, "direct")
    with pytest.raises(lib.I7MError, match="H = 3"):
        h.mpc_run_tracking(xs[:1], REF, off, np.zeros((3, 6)), fact[:1])
    with pytest.raises(lib.I7MError, match="max_batch"):
        h.mpc_run_tracking(np.tile(xs, (2, 1)), REF, off, np.tile(fhyp, (2, 1)), np.tile(fact, (2, 1)))
    with pytest.raises(lib.I7MError, match="L = 0"):
        h.mpc_run_tracking(xs, REF[:0], off, fhyp, fact)
    for cols in (4, 2):
        with pytest.raises(lib.I7MError, match=f"ref_stride = {cols}"):
            h.mpc_run_tracking(xs, np.zeros((50, cols)), off, fhyp, fact)
    with pytest.raises(lib.I7MError, match=r"ref_offset\[1\]"):
        h.mpc_run_tracking(xs, REF, [1, -2], fhyp, fact)
    with pytest.raises(lib.I7MError, match=r"ref_phase\[0\]"):
        h.mpc_run_tracking(xs, REF, off, fhyp, fact, ref_phase=[-1, 0])
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=0.0)
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=0.011)
    with pytest.raises(lib.I7MError, match="frame"):
        _raw(lib, h, xs, REF, off, fhyp, fact, frame=5)
    with pytest.raises(lib.I7MError, match="RESET"):
        h.mpc_run_tracking(xs, REF, off, fhyp, fact, reset_what=8)
    with pytest.raises(lib.I7MError, match="n_actual"):
        _raw(lib, h, xs, REF, off, fhyp, fact, n_actual=3)
    # null pointers, through the C-ABI itself
    with pytest.raises(lib.I7MError, match="null .*ref"):
        _raw(lib, h, xs, None, off, fhyp, fact)
    with pytest.raises(lib.I7MError, match="ref_offset"):
        _raw(lib, h, xs, REF, None, fhyp, fact, num_steps=2)
    with pytest.raises(lib.I7MError, match="err_out"):
        _raw(lib, h, xs, REF, off, fhyp, fact, err=False)
    # nothing ran: no wrench was left on the handle, so the plain closed loop still accepts it
    d, _, _, _ = h.mpc_run(xs, make_case(G, H, seed=1)[1], 1)
    assert np.isfinite(d).all()


def _raw(lib, h, xs, ref, off, fhyp, fact, num_steps=None, err=True, frame=None, n_actual=None):
    """i7m_mpc_run_tracking through ctypes with arguments the binding would not pass; raises the
    binding's error for a nonzero status."""
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    off = None if off is None else np.asarray(off, np.int32)
    n = len(off) if num_steps is None else num_steps
    ref = None if ref is None else np.ascontiguousarray(ref, float)
    o = lib.i7m_sampled_opts()
    assert h._lib.i7m_sampled_opts_default(C.byref(o)) == 0
    o.sim_dt = 0.01
    if frame is not None:
        o.frame = frame
    if n_actual is not None:
        o.n_actual = n_actual
    out = np.empty((max(n, 1), len(xs)))
    rc = h._lib.i7m_mpc_run_tracking(h._h, len(xs), len(fhyp) // len(xs), dp(xs), dp(ref), 300 if ref is None else len(ref),
                                     6 if ref is None else ref.shape[1], None, ip(off), n, dp(fhyp), dp(fact), None,
                                     C.byref(o), dp(out) if err else None, None, None, None, None, None, None, None)
    if rc:
        raise lib.I7MError(h._lib.i7m_last_error().decode())
    return out


def test_handle_reuse(lib, model):
    """mpc_run_sampled -> mpc_run_tracking -> mpc_run_sampled on one handle: the first and third
    results are equal bit for bit, and so is a repeated tracking run."""
    G, H, N, steps = 2, 4, 8, 3
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=8)
    noise = np.random.default_rng(9).normal(0, 2.0, (steps, G * H, 3))
    for mode in ("direct", "admm"):
        h = _handle(lib, model, N, G * H, mode)
        first = h.mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01)
        trk = h.mpc_run_tracking(xs, REF, [1, 2, 3], fhyp, fact, ref_phase=[5, 60], noise=noise, sim_dt=0.01)
        third = h.mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01)
        again = h.mpc_run_tracking(xs, REF, [1, 2, 3], fhyp, fact, ref_phase=[5, 60], noise=noise, sim_dt=0.01)
        assert np.isfinite(first["dist"]).all() and np.isfinite(trk["err"]).all()
        for key in first:
            np.testing.assert_array_equal(third[key], first[key], err_msg=key)
        for key in trk:
            np.testing.assert_array_equal(again[key], trk[key], err_msg=key)
        with pytest.raises(lib.I7MError, match="external wrench"):  # the final hypotheses stay on the handle
            h.mpc_run(xs, ends, 1)


def test_drop_in_class_names_the_true_hypothesis(lib, model):
    """MPC_GATO_Batch_Sample.run_tracking: the controller's stats keys with one entry per control
    step, and with a constant actual force equal to a drawn hypothesis best_ids names it."""
    from indy7_mpc_amd.gato_mpc_batch_sample import MPC_GATO_Batch_Sample

    probe = MPC_GATO_Batch_Sample(model, N=8, dt=0.01, batch_size=4, f_ext_std=10.0, seed=3, qp_mode="direct")
    f = probe.f_ext_batch[2].copy()
    ctrl = MPC_GATO_Batch_Sample(model, N=8, dt=0.01, batch_size=4, constant_f_ext=f, resample_f_ext=False, f_ext_std=10.0,
                                 seed=3, qp_mode="direct")
    xs = make_tracking_case(1, 4, seed=11)[0]
    flat = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3)
    stats = ctrl.run_tracking(xs[0], flat, sim_dt=0.01, sim_time=0.06)
    assert {"tracking_errors", "ee_positions", "ee_ref_positions", "joint_positions", "solve_times"} <= set(stats)
    assert stats["tracking_errors"].shape == (6,) and len(stats["solve_times"]) == 6
    assert stats["ee_positions"].shape == (6, 3) and stats["joint_positions"].shape == (6, 6)
    np.testing.assert_array_equal(stats["ee_ref_positions"], REF[1:7, :3])  # sim_dt = dt: one point per step
    np.testing.assert_allclose(stats["tracking_errors"],
                               np.linalg.norm(stats["ee_positions"] - stats["ee_ref_positions"], axis=1), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(stats["best_ids"], np.full(6, 2))
    np.testing.assert_array_equal(stats["f_ext_best"], np.tile(f, (6, 1)))
    # (L, 3) and (L, 6) are the same reference; ten control steps per knot move the window once
    st3 = ctrl.run_tracking(xs[0], REF[:, :3], sim_dt=0.01, sim_time=0.06)
    np.testing.assert_array_equal(st3["tracking_errors"], stats["tracking_errors"])
    slow = ctrl.run_tracking(xs[0], REF, sim_dt=0.001, sim_time=0.012)
    np.testing.assert_array_equal(slow["ee_ref_positions"], REF[[0] * 9 + [1] * 3, :3])


# ---- the estimator earns its keep -------------------------------------------------------------------

EST_STEPS, EST_N = 120, 16
EST_F = np.array([-60.0, 20.0, -40.0, 0.0, 0.0, 0.0])


def _estimator_case():
    """One controller from q0 at rest on a small figure 8 through eepos(q0), under a constant
    unmodelled force; H = 8 hypotheses N(0, 20) with row 0 zero, resampled with sigma 2."""
    q0 = np.array([0.3, -0.4, -1.2, 0.2, 0.6, 0.1])
    x0 = np.concatenate([q0, np.zeros(6)])[None]
    ref = figure8(0.15, 0.15, 0, period=2.0, dt=0.01, cycles=2, angle=0.0).reshape(-1, 6)[:, :3].copy()
    ref += rbd.eepos(q0) - ref[0]
    rng = np.random.default_rng(0)
    fhyp = np.zeros((8, 6))
    fhyp[:, :3] = rng.normal(0, 20.0, (8, 3))
    fhyp[0] = 0.0
    noise = rng.normal(0, 2.0, (EST_STEPS, 8, 3))
    return x0, ref, fhyp, noise, np.arange(1, EST_STEPS + 1)


def _estimator_means(run):
    """Mean tracking error over steps 40-119 of the H = 1 (zero hypothesis) and the H = 8 run."""
    x0, ref, fhyp, noise, off = _estimator_case()
    one = run(1, x0, ref, off, np.zeros((1, 6)), EST_F[None], {})
    eight = run(8, x0, ref, off, fhyp, EST_F[None], dict(noise=noise, keep_best=True, decay=0.97))
    return one["err"][40:, 0].mean(), eight["err"][40:, 0].mean()


def test_the_estimator_earns_its_keep(lib, model):
    """The reference's headline behaviour: under f_ext = [-60, 20, -40] N the controller with 8
    resampled hypotheses tracks better than the one that assumes no force.  The port loop's ratio of
    mean tracking errors must be <= 0.6; the device's, whose 120 discrete selections need not follow
    the port's path, <= 0.75."""
    m1, m8 = _estimator_means(lambda H, x0, ref, off, fh, fa, kw: run_tracking_ref(
        EST_N, 1, H, x0, ref, off, fh, fa, sim_dt=0.01, qp_mode="direct", **kw))
    print(f"port: mean tracking error H = 1 {m1:.4f} m, H = 8 {m8:.4f} m, ratio {m8 / m1:.3f}")
    assert m8 / m1 <= 0.6
    d1, d8 = _estimator_means(lambda H, x0, ref, off, fh, fa, kw: _handle(lib, model, EST_N, H, "direct").mpc_run_tracking(
        x0, ref, off, fh, fa, sim_dt=0.01, **kw))
    print(f"device: mean tracking error H = 1 {d1:.4f} m, H = 8 {d8:.4f} m, ratio {d8 / d1:.3f}")
    assert d8 / d1 <= 0.75
