"""GPU: the sampled-wrench closed loop on the device (i7m_mpc_run_sampled, csrc/i7m_mpc_sampled.h;
MPC_GATO_Batch_Sample.run_mpc of the reference, src/gato_mpc_batch_sample.py:106-300) against the
same loop in numpy on the C++ port (tests/sampled_mpc_ref.py).

The selected hypothesis is a discrete result, so every parity case first asserts, on the
reference alone, that at every step the two smallest scoring errors are at least 1e-3 apart; then
best must be identical.  Goal distances and q use the project's closed-loop tolerances for the two
modes (tests/test_gpu_mpc.py: 2e-6 direct, 1e-8 ADMM).
"""
import numpy as np
import pytest

from oracle import rbd
from sampled_mpc_ref import make_case, run_sampled_ref

pytestmark = pytest.mark.gpu
TOL = {"direct": 2e-6, "admm": 1e-8}
GAP = 1e-3


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, N, rows, mode):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def _check_parity(tag, got, ref, mode, steps, G):
    gap = ref["err2"][:, :, 1] - ref["err2"][:, :, 0]
    ran = ref["best"] >= 0
    assert (gap[ran] >= GAP).all(), (tag, gap[ran].min())
    dd = np.nanmax(np.abs(got["dist"] - ref["dist"]))
    dq = np.nanmax(np.abs(got["q"] - ref["q"]))
    print(f"{tag}: min gap {gap[ran].min():.3g}, max |dist - ref| {dd:.3g}, max |q - ref| {dq:.3g}")
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(np.isnan(got["dist"]), np.isnan(ref["dist"]))
    np.testing.assert_array_equal(np.isnan(got["q"]), np.isnan(ref["q"]))
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    np.testing.assert_allclose(got["dist"], ref["dist"], rtol=0, atol=TOL[mode])
    np.testing.assert_allclose(got["q"], ref["q"], rtol=0, atol=TOL[mode])
    last = np.array([np.flatnonzero(np.isfinite(got["q"][:, g, 0]))[-1] for g in range(G)])
    np.testing.assert_array_equal(got["xcur"][:, :6], got["q"][last, np.arange(G)])


@pytest.mark.parametrize("G,H,N,steps,sim_dt,mode", [
    (3, 4, 8, 6, 0.01, "direct"), (3, 4, 8, 6, 0.01, "admm"),
    (3, 4, 8, 6, 0.001, "direct"), (3, 4, 8, 6, 0.001, "admm"),
    (2, 8, 16, 5, 0.01, "admm"),
])
def test_parity_without_resampling(lib, model, G, H, N, steps, sim_dt, mode):
    """Hypotheses N(0, 10) N on the force, the actual wrench = hypothesis (g + 1) mod H, world frame:
    best identical to the reference loop's (and = that hypothesis), dist and q to the closed-loop
    tolerance, the hypotheses untouched."""
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1 if N == 8 else 2)
    ref = run_sampled_ref(N, G, H, xs, ends, steps, fhyp, fact, sim_dt=sim_dt, qp_mode=mode)
    got = _handle(lib, model, N, G * H, mode).mpc_run_sampled(xs, ends, steps, fhyp, fact, sim_dt=sim_dt)
    _check_parity(f"parity {(G, H, N)} sim_dt {sim_dt} {mode}", got, ref, mode, steps, G)
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))
    np.testing.assert_array_equal(got["fhyp"], fhyp)
    rel = np.abs(got["xu_best"] - ref["xu_best"]).max() / np.abs(ref["xu_best"]).max()
    print(f"  xu_best rel {rel:.3g}")  # (reported only: the issue sets no bound for it)


def test_true_hypothesis_scores_zero(lib, model):
    """The plant and the scoring convert the world wrench at the same configuration with the same
    code: the device's winning error, recovered as |rk4(x_last, u_last, winner's wrench) - xcur|
    through Handle.rk4, is <= 1e-12, the winner is the true hypothesis and fbest is its wrench
    bit for bit."""
    G, H, N = 3, 4, 8
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1)
    h = _handle(lib, model, N, G * H, "direct")
    for sim_dt in (0.01, 0.001):
        u_last = h.mpc_run_sampled(xs, ends, 0, fhyp, fact, sim_dt=sim_dt)["xu_best"][:, 12:18]  # the initial solve's
        r = h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=sim_dt)
        np.testing.assert_array_equal(r["best"][0], k)
        np.testing.assert_array_equal(r["fbest"][0], fact)
        qn, vn = h.rk4(xs[:, :6], xs[:, 6:], u_last, sim_dt, fext=r["fbest"][0], frame="world")
        err = np.linalg.norm(np.hstack([qn, vn]) - r["xcur"], axis=1)
        print(f"sim_dt {sim_dt}: recovered winning errors {err}")
        assert (err <= 1e-12).all()
        # and a wrong hypothesis is far from it
        qn, vn = h.rk4(xs[:, :6], xs[:, 6:], u_last, sim_dt, fext=np.zeros((G, 6)), frame="world")
        assert (np.linalg.norm(np.hstack([qn, vn]) - r["xcur"], axis=1) > 1e-3).all()


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("keep_best,decay", [(True, 0.97), (False, 1.0)])
def test_parity_with_resampling(lib, model, keep_best, decay, mode):
    G, H, N, steps = 2, 8, 16, 5
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=2)
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    ref = run_sampled_ref(N, G, H, xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01, qp_mode=mode,
                          keep_best=keep_best, decay=decay)
    got = _handle(lib, model, N, G * H, mode).mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01,
                                                             keep_best=keep_best, decay=decay)
    _check_parity(f"resample keep {keep_best} decay {decay} {mode}", got, ref, mode, steps, G)
    df = np.abs(got["fhyp"] - ref["fhyp"]).max()
    print(f"  max |fhyp - ref| {df:.3g}")
    assert df <= 1e-12
    assert np.abs(got["fhyp"] - fhyp).max() > 0.1 and not got["fhyp"][::H].any() and not got["fhyp"][:, 3:].any()


def test_four_waves_and_tie_break(lib, model):
    """H = 256 (four waves per group: the argmin crosses waves through LDS).  Group 0 holds the true
    wrench three times, rows 70, 75 (same wave) and 200 (a later wave): inputs equal bit for bit give
    errors equal bit for bit on either side, an exact tie, and the lowest index wins.  Group 1's
    true hypothesis is the last lane of the last wave."""
    G, H, N, steps = 2, 256, 8, 2
    xs, ends, fhyp, _, _ = make_case(G, H, seed=4)
    fhyp[70] = fhyp[75] = fhyp[200]
    fact = np.stack([fhyp[200], fhyp[H + 255]])
    ref = run_sampled_ref(N, G, H, xs, ends, steps, fhyp, fact, sim_dt=0.01)
    assert (ref["err2"][:, 0] == 0.0).all()                               # the exact tie
    assert (ref["err2"][:, 1, 1] - ref["err2"][:, 1, 0] >= GAP).all()
    got = _handle(lib, model, N, G * H, "direct").mpc_run_sampled(xs, ends, steps, fhyp, fact, sim_dt=0.01)
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["best"], np.tile([70, 255], (steps, 1)))
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    np.testing.assert_allclose(got["dist"], ref["dist"], rtol=0, atol=TOL["direct"])
    np.testing.assert_allclose(got["q"], ref["q"], rtol=0, atol=TOL["direct"])


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_single_hypothesis(lib, model, mode):
    """H = 1: one lane per group, the zero hypothesis always selected; the loop is then a plain
    closed loop under an unmodelled actual force."""
    G, H, N, steps = 3, 1, 8, 3
    xs, ends, _, _, _ = make_case(G, 2, seed=1)
    fact = np.zeros((G, 6))
    fact[:, :3] = [[5.0, 0, 0], [0, -5.0, 0], [0, 0, 5.0]]
    ref = run_sampled_ref(N, G, H, xs, ends, steps, np.zeros((G, 6)), fact, sim_dt=0.01, qp_mode=mode)
    got = _handle(lib, model, N, G, mode).mpc_run_sampled(xs, ends, steps, np.zeros((G, 6)), fact, sim_dt=0.01)
    assert (got["best"] == 0).all() and not got["fbest"].any()
    np.testing.assert_allclose(got["dist"], ref["dist"], rtol=0, atol=TOL[mode])
    np.testing.assert_allclose(got["q"], ref["q"], rtol=0, atol=TOL[mode])


def _goal_case(single):
    q0 = np.full(6, 0.3)
    ends = np.array([rbd.eepos(q0)] if single else [rbd.eepos(q0), rbd.eepos(np.full(6, 0.9))])
    xs = np.zeros((2, 12))
    xs[0, :6] = q0 + 0.01
    xs[1, :6] = -0.4
    return xs, ends


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("single", [False, True])
def test_goal_switch_and_stop(lib, model, single, mode):
    """A group that starts within 0.095 of endpoint 0 switches to endpoint 1, or with one endpoint
    stops at step 0 and reads NaN / -1 afterwards, at the reference's step indices."""
    G, H, N, steps = 2, 2, 8, 3
    xs, ends = _goal_case(single)
    z = np.zeros((G * H, 6))
    ref = run_sampled_ref(N, G, H, xs, ends, steps, z, np.zeros((G, 6)), sim_dt=0.01, qp_mode=mode)
    got = _handle(lib, model, N, G * H, mode).mpc_run_sampled(xs, ends, steps, z, np.zeros((G, 6)), sim_dt=0.01)
    np.testing.assert_array_equal(got["best"], ref["best"])
    for key in ("dist", "q", "fbest"):
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(ref[key]), err_msg=key)
    np.testing.assert_allclose(got["dist"], ref["dist"], rtol=0, atol=TOL[mode])
    np.testing.assert_allclose(got["q"], ref["q"], rtol=0, atol=TOL[mode])
    assert got["dist"][0, 0] < 0.095
    if single:
        assert np.isnan(got["dist"][1:, 0]).all() and (got["best"][:, 0] == -1).all()
    else:
        assert got["dist"][1, 0] > 0.095 and (got["best"] == 0).all()


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_groups_are_independent(lib, model, mode):
    """The run at G = 3 equals, bit for bit, three runs at G = 1 of each group alone (resampling
    on, so the wrench rows are written too); duplicated groups evolve identically."""
    G, H, N, steps = 3, 4, 8, 4
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=1)
    noise = np.random.default_rng(6).normal(0, 2.0, (steps, G * H, 3))
    h = _handle(lib, model, N, G * H, mode)
    kw = dict(sim_dt=0.01, keep_best=True, decay=0.97)
    full = h.mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, **kw)
    for g in range(G):
        r = slice(g * H, (g + 1) * H)
        one = h.mpc_run_sampled(xs[g:g + 1], ends, steps, fhyp[r], fact[g:g + 1], noise=noise[:, r], **kw)
        for key in ("dist", "best", "q", "fbest"):
            np.testing.assert_array_equal(one[key][:, 0], full[key][:, g], err_msg=f"{key} group {g}")
        np.testing.assert_array_equal(one["xcur"][0], full["xcur"][g])
        np.testing.assert_array_equal(one["xu_best"][0], full["xu_best"][g])
        np.testing.assert_array_equal(one["fhyp"], full["fhyp"][r])
    dup = h.mpc_run_sampled(np.tile(xs[1], (2, 1)), ends, steps, np.tile(fhyp[H:2 * H], (2, 1)), np.tile(fact[1], (2, 1)),
                            noise=np.tile(noise[:, H:2 * H], (1, 2, 1)), **kw)
    for key in ("dist", "best", "q", "fbest"):
        np.testing.assert_array_equal(dup[key][:, 0], dup[key][:, 1], err_msg=key)
    for key in ("xcur", "xu_best"):
        np.testing.assert_array_equal(dup[key][0], dup[key][1], err_msg=key)
    np.testing.assert_array_equal(dup["fhyp"][:H], dup["fhyp"][H:])


def test_stagger_cut_splits_no_group(lib, model, monkeypatch):
    """ADMM batches from I7M_ADMM_STAGGER_MIN_B rows run as two staggered ranges; with G = 7 groups
    of H = 4 the cut must fall on a group boundary, so the staggered run equals the one-range run
    bit for bit.  (The tuning variables are read when the handle is created.)"""
    G, H, N = 7, 4, 8
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=3)
    noise = np.random.default_rng(7).normal(0, 2.0, (1, G * H, 3))
    runs = []
    for min_b in ("8", None):
        if min_b:
            monkeypatch.setenv("I7M_ADMM_STAGGER_MIN_B", min_b)
            monkeypatch.setenv("I7M_ADMM_STAGGER", "1")
        else:
            monkeypatch.delenv("I7M_ADMM_STAGGER_MIN_B")
            monkeypatch.delenv("I7M_ADMM_STAGGER")
        h = _handle(lib, model, N, G * H, "admm")
        runs.append(h.mpc_run_sampled(xs, ends, 1, fhyp, fact, noise=noise, sim_dt=0.01))
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg=key)
    assert np.isfinite(runs[0]["dist"]).all()


def test_refusals(lib, model):
    """I7M_EINVAL with a message, before any work: box mode, H = 3, G H > max_batch, sim_dt = 0,
    sim_dt > dt, null dist_out."""
    import ctypes as C

    G, H, N = 2, 4, 8
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=1)
    hb = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_BOX)
    with pytest.raises(lib.I7MError, match="I7M_QP_BOX"):
        hb.mpc_run_sampled(xs, ends, 1, fhyp, fact)
    h = _handle(lib, model, N, G * H, "direct")
    with pytest.raises(lib.I7MError, match="H = 3"):
        h.mpc_run_sampled(xs[:1], ends, 1, np.zeros((3, 6)), fact[:1])
    with pytest.raises(lib.I7MError, match="max_batch"):
        h.mpc_run_sampled(np.tile(xs, (2, 1)), ends, 1, np.tile(fhyp, (2, 1)), np.tile(fact, (2, 1)))
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=0.0)
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=0.011)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = h._lib.i7m_mpc_run_sampled(h._h, G, H, dp(xs), dp(ends), len(ends), 1, dp(fhyp), dp(fact), None, None, None, None,
                                    None, None, None, None, None)
    assert rc == -1 and b"dist_out" in h._lib.i7m_last_error()
    # nothing ran: no wrench was left on the handle, so the plain closed loop still accepts it
    d, _, _, _ = h.mpc_run(xs, ends, 1)
    assert np.isfinite(d).all()


def test_mpc_run_still_refuses_the_handle_after_a_sampled_run(lib, model):
    """The sampled run leaves its final hypotheses set as the handle's wrench; i7m_mpc_run's
    contract (no wrench, tests/test_gpu_mpc.py) holds until it is cleared."""
    G, H, N = 1, 4, 8
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=1)
    h = _handle(lib, model, N, G * H, "direct")
    h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=0.01)
    with pytest.raises(lib.I7MError, match="external wrench"):
        h.mpc_run(xs, ends, 1)
    h.set_external_wrench(None)
    assert np.isfinite(h.mpc_run(xs, ends, 1)[0]).all()


def test_drop_in_class_names_the_true_hypothesis(lib, model):
    """MPC_GATO_Batch_Sample.run_mpc (the reference's src/gato_mpc_batch_sample.py surface): one q
    per step, the reference's stats keys, and with a constant actual force equal to a drawn
    hypothesis the estimator names it at every step."""
    from indy7_mpc_amd.gato_mpc_batch_sample import MPC_GATO_Batch_Sample

    probe = MPC_GATO_Batch_Sample(model, N=8, dt=0.01, batch_size=4, f_ext_std=10.0, seed=3, qp_mode="direct")
    f = probe.f_ext_batch[2].copy()
    assert f[:3].any() and not f[3:].any() and not probe.f_ext_batch[0].any()
    ctrl = MPC_GATO_Batch_Sample(model, N=8, dt=0.01, batch_size=4, constant_f_ext=f, resample_f_ext=False, f_ext_std=10.0,
                                 f_ext_resample_std=2.0, seed=3, qp_mode="direct")
    np.testing.assert_array_equal(ctrl.f_ext_batch, probe.f_ext_batch)
    xs, ends, _, _, _ = make_case(1, 4, seed=1)
    xpath, stats = ctrl.run_mpc(xs[0], ends, sim_dt=0.01, sim_time=0.065)
    assert len(xpath) == 6 and all(np.shape(q) == (6,) for q in xpath)
    assert {"solve_times", "goal_distances", "control_inputs"} <= set(stats)
    assert len(stats["goal_distances"]) == 2  # logged every 0.05 s: steps 0 and 5
    np.testing.assert_array_equal(stats["best_ids"], np.full(6, 2))
    np.testing.assert_array_equal(stats["f_ext_best"], np.tile(f, (6, 1)))


def test_repeated_closed_loop_calls_on_one_handle(lib, model):
    """One handle serves mpc_run and mpc_run_sampled calls of different shapes in turn: a repeated
    call returns the same arrays bit for bit, whatever ran between (per-call device state does not
    leak from one call into the next)."""
    N, steps = 8, 3
    h = _handle(lib, model, N, 8, "direct")
    xs3, ends, _, _, _ = make_case(3, 2, seed=1)
    plain = h.mpc_run(xs3, ends, 4)
    for a, b in zip(h.mpc_run(xs3, ends, 4), plain):
        np.testing.assert_array_equal(a, b)

    def sampled(hh, G, H, **kw):
        xs, _, fhyp, fact, _ = make_case(G, H, seed=8)
        noise = np.random.default_rng(9).normal(0, 2.0, (steps, G * H, 3))
        return hh.mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01, **kw)

    first = sampled(h, 2, 4)
    sampled(h, 1, 8)
    third = sampled(h, 2, 4)
    assert np.isfinite(first["dist"]).all()
    for key in first:
        np.testing.assert_array_equal(third[key], first[key], err_msg=key)
    with pytest.raises(lib.I7MError, match="external wrench"):
        h.mpc_run(xs3, ends, 4)
    h.set_external_wrench(None)
    for a, b in zip(h.mpc_run(xs3, ends, 4), plain):
        np.testing.assert_array_equal(a, b)
    ha = _handle(lib, model, N, 8, "admm")
    one = sampled(ha, 2, 4, reset_what=lib.ADMM_RESET_ALL)
    two = sampled(ha, 2, 4, reset_what=lib.ADMM_RESET_ALL)
    for key in one:
        np.testing.assert_array_equal(two[key], one[key], err_msg=key)
