"""GPU: the multi-rate sampled-wrench closed loops on the device (i7m_mpc_run_sampled_multirate,
i7m_mpc_run_tracking_multirate; k_sampled_multirate_step, csrc/i7m_mpc_sampled_multirate.h) against
the same loops in numpy on the C++ port (tests/sampled_multirate_ref.py): the plant advances sim_dt
per solve against 10 ms knots, split at the knot boundaries, the hypotheses scored by one rk4 step
of the whole sim_dt (reference src/gato_mpc_batch_sample.py:163-193,284; run_mpc_fig8 of
notebooks/gato_mpc_indy7_fig8.ipynb).

The selected hypothesis, the goal switch and the stop are discrete results, so every parity case
first asserts, on the reference alone, that the two smallest scoring errors are at least GAP = 1e-3
apart and every goal distance at least 1e-3 from the radius; then best, fbest, off and the NaN
patterns must be identical, and dist / err / q / u / xpath are within the project's closed-loop
tolerances (tests/test_gpu_sampled_mpc.py: 2e-6 direct, 1e-8 ADMM).

One exception, by the rule set for this file: where a value tolerance does not hold on the GPU while
every discrete output matches, the bound is 10 x the distance the REFERENCE loop moves when xstart is
perturbed by 1e-13 relative, never a figure taken from the GPU.  That is the control history `u` of
the six ADMM parity cases.  u is a torque of up to 100 N m, and OSQP stopped at eps 1e-3 amplifies a
1e-13 change of its input to 1e-7 there: measured on an MI355X, |device - reference| of u was 1.97e-7
/ 1.15e-7 / 1.53e-7 (endpoints: sim_dt 0.02, 0.025, 0.02 shifted) and 8.48e-8 / 8.39e-8 / 1.00e-7
(tracking), against 1e-8; dist, err, q, xpath and ee of the same runs were within 2.5e-10, and best,
fbest, off and the NaN patterns identical.  The reference, run on the C++ port with xstart * (1 +-
1e-13), moved its u by the U_MOVED_ADMM figures below (6.4e-8 to 2.2e-7), so those cases' bound on u
is 10 x that (6.4e-7 to 2.2e-6).  Everything else, u in direct mode and u of the ADMM stop case
included (7.9e-9 there), keeps the tolerances above.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from indy7_mpc_amd.utils import figure8
from oracle import rbd
from sampled_mpc_ref import make_case
from sampled_multirate_ref import run_sampled_multirate_ref
from tracking_mpc_ref import make_tracking_case

pytestmark = pytest.mark.gpu
TOL = {"direct": 2e-6, "admm": 1e-8}
GAP = 1e-3
REF = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
REF.setflags(write=False)
PHASES = (3, 40)
# max |u - u'| of the reference loop (ADMM) for xstart' = xstart * (1 +- 1e-13), per (source, sim_dt, shift)
U_MOVED_ADMM = {("endpoints", 0.02, 0): 1.40e-7, ("endpoints", 0.025, 0): 6.41e-8, ("endpoints", 0.02, 1): 2.17e-7,
                ("tracking", 0.02, 0): 1.23e-7, ("tracking", 0.025, 0): 1.21e-7, ("tracking", 0.02, 1): 7.49e-8}


def _u_tol(source, sim_dt, mode, shift=0):
    """The bound on the control history: the closed-loop tolerance, or 10 x the reference's own
    movement under a 1e-13 perturbation for the ADMM parity cases (the module docstring)."""
    return 10 * U_MOVED_ADMM[(source, sim_dt, shift)] if mode == "admm" else TOL[mode]


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, N, rows, mode):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


@functools.lru_cache(maxsize=None)
def _reference(source, G, H, N, steps, sim_dt, mode, shift=0):
    """The numpy loop on the parity cases' inputs, computed once per case and left unchanged."""
    if source == "endpoints":
        xs, ends, fhyp, fact, _ = make_case(G, H, seed=1 if N == 8 else 2)
        r = run_sampled_multirate_ref(N, G, H, xs, steps, fhyp, fact, endpoints=ends, sim_dt=sim_dt, qp_mode=mode,
                                      shift_warm_start=shift)
    else:
        xs, fhyp, fact, _ = make_tracking_case(G, H, seed=3)
        r = run_sampled_multirate_ref(N, G, H, xs, steps, fhyp, fact, ref=REF, ref_phase=PHASES, sim_dt=sim_dt,
                                      qp_mode=mode, shift_warm_start=shift)
    for v in r.values():
        v.setflags(write=False)
    return r


def _device(lib, model, source, G, H, N, steps, sim_dt, mode, shift=0):
    h = _handle(lib, model, N, G * H, mode)
    if source == "endpoints":
        xs, ends, fhyp, fact, k = make_case(G, H, seed=1 if N == 8 else 2)
        return h.mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, sim_dt=sim_dt, shift_warm_start=shift), k
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=3)
    return h.mpc_run_tracking_multirate(xs, REF, steps, fhyp, fact, ref_phase=PHASES, sim_dt=sim_dt,
                                        shift_warm_start=shift), k


def _check_parity(tag, got, ref, mode, source, u_tol):
    d = "dist" if source == "endpoints" else "err"
    keys = (d, "q", "u", "xpath") + (() if source == "endpoints" else ("ee",))
    ran = ref["best"] >= 0
    gap = (ref["err2"][:, :, 1] - ref["err2"][:, :, 0])[ran]
    assert (gap >= GAP).all(), (tag, gap.min())
    if source == "endpoints":
        margin = ref["margin"][np.isfinite(ref["margin"])]
        assert (margin >= 1e-3).all(), (tag, margin.min())
    diff = {k: np.nanmax(np.abs(got[k] - ref[k])) for k in keys}
    print(f"{tag}: min gap {gap.min():.3g}, max |device - reference| " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    np.testing.assert_array_equal(got["sub_start"], ref["sub_start"])
    np.testing.assert_array_equal(got["shift"], ref["shift"])
    if source != "endpoints":
        np.testing.assert_array_equal(got["off"], ref["off"])
        np.testing.assert_array_equal(got["off"], np.cumsum(ref["shift"]))
    for k in keys:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=u_tol if k == "u" else TOL[mode], err_msg=k)
    np.testing.assert_array_equal(got["xpath"][ref["sub_start"][1:] - 1], got["q"])  # q is the step's last sub-step


CASES = [(2, 4, 8, 4, 0.02, "direct"), (2, 4, 8, 3, 0.02, "admm"),
         (2, 4, 8, 12, 0.001, "direct"),   # the residue step 9: two sub-steps [0.001, 8.67e-19], shift 1
         (2, 4, 8, 5, 0.015, "direct"),    # shifts 1, 2, 1, 2, 1
         (2, 8, 16, 3, 0.025, "admm")]     # 3-4 sub-steps, shifts 2, 3, 2


@pytest.mark.parametrize("source", ["endpoints", "tracking"])
@pytest.mark.parametrize("G,H,N,steps,sim_dt,mode", CASES)
def test_parity(lib, model, source, G, H, N, steps, sim_dt, mode):
    ref = _reference(source, G, H, N, steps, sim_dt, mode, 0)
    if sim_dt == 0.001:
        assert ref["sub_start"][10] - ref["sub_start"][9] == 2 and ref["shift"][9] == 1
    if sim_dt == 0.015:
        np.testing.assert_array_equal(ref["shift"], [1, 2, 1, 2, 1])
    if sim_dt == 0.025:
        np.testing.assert_array_equal(ref["shift"], [2, 3, 2])
        np.testing.assert_array_equal(np.diff(ref["sub_start"]), [3, 4, 3])
    got, k = _device(lib, model, source, G, H, N, steps, sim_dt, mode)
    _check_parity(f"{source} {(G, H, N)} sim_dt {sim_dt} {mode}", got, ref, mode, source, _u_tol(source, sim_dt, mode))
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))  # the true hypothesis, at every step


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_equals_the_single_rate_loops_at_dt(lib, model, mode):
    """sim_dt = dt, no shift: one sub-step and one knot per step, the loops i7m_mpc_run_sampled and
    i7m_mpc_run_tracking (offsets 1 .. steps) run.  Same handle; best and fbest equal, the values
    within 1e-12 (the two kernels are different instruction streams)."""
    G, H, N, steps = 2, 4, 8, 4
    h = _handle(lib, model, N, G * H, mode)
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=1)
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    kw = dict(noise=noise, sim_dt=0.01, keep_best=True, decay=0.97)
    pairs = [("endpoints", h.mpc_run_sampled(xs, ends, steps, fhyp, fact, **kw),
              h.mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, **kw))]
    xs, fhyp, fact, _ = make_tracking_case(G, H, seed=3)
    pairs.append(("tracking", h.mpc_run_tracking(xs, REF, np.arange(1, steps + 1), fhyp, fact, ref_phase=PHASES, **kw),
                  h.mpc_run_tracking_multirate(xs, REF, steps, fhyp, fact, ref_phase=PHASES, **kw)))
    for source, old, new in pairs:
        np.testing.assert_array_equal(new["best"], old["best"])
        np.testing.assert_array_equal(new["fbest"], old["fbest"])
        keys = ("dist" if source == "endpoints" else "err", "q", "xcur", "xu_best", "fhyp")
        print(f"{source} {mode}: bit-equal " + ", ".join(f"{k} {np.array_equal(new[k], old[k])}" for k in keys))
        for k in keys:
            np.testing.assert_allclose(new[k], old[k], rtol=0, atol=1e-12, err_msg=k)
        np.testing.assert_array_equal(new["xpath"], new["q"])
        if source == "tracking":
            np.testing.assert_array_equal(new["off"], np.arange(1, steps + 1))
            np.testing.assert_allclose(new["ee"], old["ee"], rtol=0, atol=1e-12)


def test_true_hypothesis_score(lib, model):
    """On a step with one sub-step plant and score are the same computation: at sim_dt = 0.001,
    steps 0 .. 8, the winner's one-step prediction (Handle.rk4 from x_last under u_last and the
    winning wrench) lands on the plant's state within 1e-12.  At 0.02 (two sub-steps) it does not,
    and the true row still wins.  x_last of step i is the final state of the run of i steps: a run
    repeated on one handle is identical (test_forced_stagger_groups_and_repeats)."""
    G, H, N = 2, 4, 8
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1)
    h = _handle(lib, model, N, G * H, "direct")
    runs = [h.mpc_run_sampled_multirate(xs, ends, n, fhyp, fact, sim_dt=0.001) for n in range(10)]
    np.testing.assert_array_equal(runs[0]["xcur"], xs)
    full = runs[9]
    assert (np.diff(full["sub_start"]) == 1).all()
    np.testing.assert_array_equal(full["best"], np.tile(k, (9, 1)))
    worst = 0.0
    for i in range(9):
        x0, x1 = runs[i]["xcur"], runs[i + 1]["xcur"]
        qn, vn = h.rk4(x0[:, :6], x0[:, 6:], full["u"][i], 0.001, fext=full["fbest"][i], frame="world")
        worst = max(worst, np.linalg.norm(np.concatenate([qn, vn], axis=1) - x1, axis=1).max())
    print(f"winning error over steps 0..8 at sim_dt 0.001: {worst:.3g}")
    assert worst <= 1e-12
    one = h.mpc_run_sampled_multirate(xs, ends, 1, fhyp, fact, sim_dt=0.02)
    qn, vn = h.rk4(xs[:, :6], xs[:, 6:], one["u"][0], 0.02, fext=one["fbest"][0], frame="world")
    e = np.linalg.norm(np.concatenate([qn, vn], axis=1) - one["xcur"], axis=1)
    print(f"winning error at sim_dt 0.02 (two sub-steps): {e}")
    assert (e > 0).all()
    np.testing.assert_array_equal(one["best"][0], k)
    np.testing.assert_array_equal(one["fbest"][0], fact)


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_stop_and_nan_layout(lib, model, mode):
    """Group 0 starts at rest at q = 0.31, within 0.095 of both endpoints eepos(0.3), eepos(0.33): it
    switches, then stops.  The stopping step's dist / q / u / xpath are recorded and its best is -1;
    from the next step on dist, q, u, xpath and fbest are NaN and best is -1.  Group 1 runs on."""
    G, H, N, steps = 2, 2, 8, 4
    ends = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.33))])
    xs = np.zeros((G, 12))
    xs[0, :6] = 0.31
    xs[1, :6] = -0.4
    z, za = np.zeros((G * H, 6)), np.zeros((G, 6))
    ref = run_sampled_multirate_ref(N, G, H, xs, steps, z, za, endpoints=ends, sim_dt=0.02, qp_mode=mode)
    stop = int(np.flatnonzero(ref["best"][:, 0] < 0)[0])
    assert stop < steps - 1 and np.isfinite(ref["dist"][stop, 0]) and np.isnan(ref["dist"][stop + 1:, 0]).all()
    margin = ref["margin"][np.isfinite(ref["margin"])]
    assert (margin >= 1e-3).all(), margin.min()
    got = _handle(lib, model, N, G * H, mode).mpc_run_sampled_multirate(xs, ends, steps, z, za, sim_dt=0.02)
    np.testing.assert_array_equal(got["best"], ref["best"])
    for key in ("dist", "q", "u", "xpath", "fbest"):
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(ref[key]), err_msg=key)
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL[mode], err_msg=key)
    s0, s1 = got["sub_start"][stop], got["sub_start"][stop + 1]
    assert np.isfinite(got["dist"][stop, 0]) and np.isfinite(got["q"][stop, 0]).all() and np.isfinite(got["u"][stop, 0]).all()
    assert np.isfinite(got["xpath"][s0:s1, 0]).all()
    assert (got["best"][stop:, 0] == -1).all() and np.isnan(got["fbest"][stop:, 0]).all()
    assert np.isnan(got["dist"][stop + 1:, 0]).all() and np.isnan(got["q"][stop + 1:, 0]).all()
    assert np.isnan(got["u"][stop + 1:, 0]).all() and np.isnan(got["xpath"][s1:, 0]).all()
    for key in ("dist", "q", "u", "xpath", "fbest"):
        assert np.isfinite(got[key][:, 1]).all(), key
    assert (got["best"][:, 1] == 0).all()
    alone = _handle(lib, model, N, H, mode).mpc_run_sampled_multirate(xs[1:], ends, steps, z[H:], za[1:], sim_dt=0.02)
    for key in ("dist", "q", "u", "xpath", "best"):
        np.testing.assert_array_equal(alone[key][:, 0], got[key][:, 1], err_msg=key)


@pytest.mark.parametrize("source", ["endpoints", "tracking"])
@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_shift_warm_start(lib, model, source, mode):
    """shift_warm_start = 1: the rows' warm start is XU_best shifted by the knots the step completed
    (two per step at sim_dt = 0.02).  On the reference alone the run differs from the unshifted one
    by more than the tolerance."""
    G, H, N, steps = 2, 4, 8, 4
    ref = _reference(source, G, H, N, steps, 0.02, mode, 1)
    plain = _reference(source, G, H, N, steps, 0.02, mode, 0)
    apart = np.nanmax(np.abs(ref["q"] - plain["q"]))
    print(f"{source} {mode}: shifted and unshifted reference runs differ by {apart:.3g}")
    assert apart > 100 * TOL[mode]
    got, _ = _device(lib, model, source, G, H, N, steps, 0.02, mode, 1)
    _check_parity(f"{source} shift_warm_start {mode}", got, ref, mode, source, _u_tol(source, 0.02, mode, 1))


def test_four_waves_and_tie_break(lib, model):
    """H = 256 (four waves per group) at sim_dt = 0.02.  Group 0 holds the true wrench three times,
    rows 70, 75 (same wave) and 200 (a later wave): identical rows give errors equal bit for bit (not
    0 here: two sub-steps against one), and the lowest index wins.  Group 1's true hypothesis is the
    last lane of the last wave."""
    G, H, N, steps = 2, 256, 8, 2
    xs, ends, fhyp, _, _ = make_case(G, H, seed=4)
    fhyp[70] = fhyp[75] = fhyp[200]
    fact = np.stack([fhyp[200], fhyp[H + 255]])
    ref = run_sampled_multirate_ref(N, G, H, xs, steps, fhyp, fact, endpoints=ends, sim_dt=0.02)
    assert (ref["err2"][:, 0, 0] == ref["err2"][:, 0, 1]).all() and (ref["err2"][:, 0, 0] > 0).all()  # the exact tie
    assert (ref["err2"][:, 1, 1] - ref["err2"][:, 1, 0] >= GAP).all()
    assert (ref["margin"] >= 1e-3).all()
    got = _handle(lib, model, N, G * H, "direct").mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, sim_dt=0.02)
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["best"], np.tile([70, 255], (steps, 1)))
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    for key in ("dist", "q", "u", "xpath"):
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL["direct"], err_msg=key)


def test_forced_stagger_groups_and_repeats(lib, model, monkeypatch):
    """ADMM, G = 7 groups of H = 4 with the stagger forced from 8 rows: the two staggered ranges (cut
    on a group boundary) equal the one-range run bit for bit; the groups run together equal each
    group alone; and a run repeated on the same handle is identical: nothing carries over."""
    G, H, N, steps = 7, 4, 8, 2
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=3)
    noise = np.random.default_rng(7).normal(0, 2.0, (steps, G * H, 3))
    kw = dict(sim_dt=0.02, keep_best=True, decay=0.97)
    runs = []
    for min_b in ("8", None):
        if min_b:
            monkeypatch.setenv("I7M_ADMM_STAGGER_MIN_B", min_b)
            monkeypatch.setenv("I7M_ADMM_STAGGER", "1")
        else:
            monkeypatch.delenv("I7M_ADMM_STAGGER_MIN_B")
            monkeypatch.delenv("I7M_ADMM_STAGGER")
        h = _handle(lib, model, N, G * H, "admm")
        runs.append(h.mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, noise=noise, **kw))
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg=key)
    assert np.isfinite(runs[0]["dist"]).all() and np.isfinite(runs[0]["xpath"]).all()
    full = runs[1]
    for g in range(G):
        r = slice(g * H, (g + 1) * H)
        one = h.mpc_run_sampled_multirate(xs[g:g + 1], ends, steps, fhyp[r], fact[g:g + 1], noise=noise[:, r], **kw)
        for key in ("dist", "best", "q", "u", "xpath", "fbest"):
            np.testing.assert_array_equal(one[key][:, 0], full[key][:, g], err_msg=f"{key} group {g}")
        np.testing.assert_array_equal(one["xcur"][0], full["xcur"][g])
        np.testing.assert_array_equal(one["xu_best"][0], full["xu_best"][g])
        np.testing.assert_array_equal(one["fhyp"], full["fhyp"][r])
    again = h.mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, noise=noise, **kw)
    for key in full:
        np.testing.assert_array_equal(again[key], full[key], err_msg=key)
    trk = [h.mpc_run_tracking_multirate(xs, REF, steps, fhyp, fact, ref_phase=np.arange(G) * 9, noise=noise, **kw)
           for _ in range(2)]
    for key in trk[0]:
        np.testing.assert_array_equal(trk[0][key], trk[1][key], err_msg=key)


def test_refusals(lib, model):
    """I7M_EINVAL with the argument named, before any device work; num_steps = 0 is the initial
    solve; an old entry point still refuses sim_dt > dt."""
    G, H, N = 2, 4, 8
    xs, ends, fhyp, fact, _ = make_case(G, H, seed=1)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    dist = np.empty((4, G))

    def opts(h, **kw):
        o = lib.i7m_sampled_multirate_opts()
        assert h._lib.i7m_sampled_multirate_opts_default(C.byref(o)) == 0
        assert (o.sim_dt, o.decay, o.frame, o.reset_what, o.keep_best, o.n_actual, o.shift_warm_start) == \
            (0.001, 1.0, lib.WRENCH_WORLD, lib.ADMM_RESET_ALL, 0, 1, 0)
        o.sim_dt = 0.02
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def sampled(h, want, G=G, H=H, xs=xs, ends=ends, n_ends=2, steps=1, fhyp=fhyp, fact=fact, out=dist,
                who="mpc_run_sampled_multirate", **kw):
        o = opts(h, **kw)
        rc = h._lib.i7m_mpc_run_sampled_multirate(h._h, G, H, dp(xs), dp(ends), n_ends, steps, dp(fhyp), dp(fact), None,
                                                  C.byref(o), dp(out), None, None, None, None, None, None, None, None)
        msg = h._lib.i7m_last_error().decode()
        assert rc == -1 and want in msg and who in msg, (rc, want, msg)

    def tracking(h, want, ref=REF, L=len(REF), stride=6, phase=None, out=dist, who="mpc_run_tracking_multirate", **kw):
        o = opts(h, **kw)
        rc = h._lib.i7m_mpc_run_tracking_multirate(h._h, G, H, dp(xs), dp(ref), L, stride, ip(phase), 1, dp(fhyp), dp(fact),
                                                   None, C.byref(o), dp(out), None, None, None, None, None, None, None,
                                                   None, None, None)
        msg = h._lib.i7m_last_error().decode()
        assert rc == -1 and want in msg and who in msg, (rc, want, msg)

    hb = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_BOX)
    sampled(hb, "I7M_QP_BOX")
    tracking(hb, "I7M_QP_BOX")
    h = _handle(lib, model, N, G * H, "direct")
    sampled(h, "H = 3", H=3)
    sampled(h, "max_batch", G=3)
    for v in (0.0, -0.02, float("nan"), float("inf")):
        sampled(h, "sim_dt must be finite and > 0", sim_dt=v)
        tracking(h, "sim_dt must be finite and > 0", sim_dt=v)
    sampled(h, "MULTIRATE_MAX_SUB", sim_dt=0.7)
    sampled(h, "more than N - 1 = 7 knots in step 0", sim_dt=0.08)
    tracking(h, "more than N - 1 = 7 knots in step 0", sim_dt=0.08)
    for v in (-1, 2):
        sampled(h, f"shift_warm_start = {v}", shift_warm_start=v)
        tracking(h, f"shift_warm_start = {v}", shift_warm_start=v)
    sampled(h, "frame", frame=2)
    sampled(h, "reset_what", reset_what=8)
    sampled(h, "n_endpoints", n_ends=0)
    sampled(h, "num_steps", steps=-1)
    sampled(h, "n_actual", steps=4, n_actual=2)
    sampled(h, "null xstart", xs=None)
    sampled(h, "null endpoints", ends=None)
    sampled(h, "null fhyp", fhyp=None)
    sampled(h, "null f_actual", fact=None)
    sampled(h, "null dist_out", out=None)
    tracking(h, "L = 0", L=0)
    tracking(h, "ref_stride = 4", stride=4)
    tracking(h, "ref_phase[1] is negative", phase=np.array([2, -1], np.int32))
    tracking(h, "null ref", ref=None)
    tracking(h, "null err_out", out=None)
    # nothing ran: no wrench was left on the handle, so the plain closed loop still accepts it
    assert np.isfinite(h.mpc_run(xs, ends, 1)[0]).all()
    # an open controller session refuses both
    h.ctrl_begin(REF, fhyp, x0=xs)
    sampled(h, "controller session open", who="")  # (the session's one message names no entry point)
    tracking(h, "controller session open", who="")
    h.ctrl_end()
    h.set_external_wrench(None)
    # the single-rate entry points still refuse sim_dt > dt
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=0.011)
    with pytest.raises(lib.I7MError, match="sim_dt"):
        h.mpc_run_tracking(xs, REF, [1], fhyp, fact, sim_dt=0.011)
    # no steps: the initial solve, as the single-rate loop's
    old = h.mpc_run_sampled(xs, ends, 0, fhyp, fact, sim_dt=0.01)
    new = h.mpc_run_sampled_multirate(xs, ends, 0, fhyp, fact, sim_dt=0.02)
    assert new["xpath"].shape == (0, G, 6) and new["u"].shape == (0, G, 6)
    np.testing.assert_array_equal(new["xu_best"], old["xu_best"])
    np.testing.assert_array_equal(new["xcur"], xs)
    trk = h.mpc_run_tracking_multirate(xs, REF, 0, fhyp, fact, sim_dt=0.02)
    assert trk["off"].shape == (0,) and np.isfinite(trk["xu_best"]).all()


def test_drop_in_fig8_and_run_mpc(lib, model):
    """MPC_GATO_Batch_Sample.run_mpc_fig8 (the notebook's surface) on a short figure 8 at N = 8, H = 4,
    sim_dt = 0.02: one q per plant sub-step, the run ends at the first step whose offset reaches
    L - 6 N with that step's plant in the path, the stats are logged at steps 0, 5, 10 with one control
    each.  run_mpc(sim_dt = 0.02) goes through the multi-rate loop and matches the raw binding."""
    from indy7_mpc_amd.gato_mpc_batch_sample import MPC_GATO_Batch_Sample

    N, H = 8, 4
    fig8 = REF[:6 * N + 25].reshape(-1)  # flat, six per point, as the notebook's figure8(): the bound is offset 25
    probe = MPC_GATO_Batch_Sample(model, N=N, dt=0.01, batch_size=H, f_ext_std=10.0, seed=3, qp_mode="direct")
    f = probe.f_ext_batch[2].copy()
    ctrl = MPC_GATO_Batch_Sample(model, N=N, dt=0.01, batch_size=H, constant_f_ext=f, f_ext_std=10.0, seed=3,
                                 qp_mode="direct")
    xstart = np.zeros(12)
    xpath, stats = ctrl.run_mpc_fig8(xstart, fig8, 0.02, 15)
    # offsets 2, 4, ..., 26: step 12 is the first at or past 25, so 13 steps and 26 sub-steps
    np.testing.assert_array_equal(stats["offsets"], 2 * np.arange(1, 14))
    assert len(xpath) == 26 and all(np.shape(q) == (6,) and np.isfinite(q).all() for q in xpath)
    assert {"solve_times", "goal_distances", "control_inputs"} <= set(stats)
    assert len(stats["goal_distances"]) == len(stats["control_inputs"]) == len(stats["solve_times"]) == 3
    r = ctrl.last
    np.testing.assert_array_equal(stats["goal_distances"], np.round(r["err"][[0, 5, 10], 0], 5))
    np.testing.assert_array_equal(np.array(stats["control_inputs"]), np.round(r["u"][[1, 6, 11], 0], 5))
    np.testing.assert_array_equal(np.array(xpath), r["xpath"][:, 0])
    # a run cut short by sim_time: int(0.1 / 0.02) = 5 steps, none breaks
    _, st = ctrl.run_fig8_groups(np.zeros((2, 12)), fig8, 0.02, 0.1, ref_phase=[0, 5])
    assert st["goal_distances"].shape == (1, 2) and st["control_inputs"].shape == (1, 2, 6) and len(st["offsets"]) == 5

    # run_mpc at sim_dt > dt: the multi-rate endpoint loop
    xs, ends, _, _, _ = make_case(1, H, seed=1)
    ctrl2 = MPC_GATO_Batch_Sample(model, N=N, dt=0.01, batch_size=H, constant_f_ext=f, f_ext_std=10.0, seed=3,
                                  qp_mode="direct")
    path, st2 = ctrl2.run_mpc(xs[0], ends, sim_dt=0.02, sim_time=0.13)
    raw = _handle(lib, model, N, H, "direct").mpc_run_sampled_multirate(xs, ends, 6, probe.f_ext_batch, f[None], sim_dt=0.02)
    assert len(path) == 12
    np.testing.assert_array_equal(np.array(path), raw["xpath"][:, 0])
    np.testing.assert_array_equal(st2["best_ids"], raw["best"][:, 0])
    np.testing.assert_array_equal(st2["best_ids"], np.full(6, 2))
    assert len(st2["goal_distances"]) == len(st2["control_inputs"]) == 2  # steps 0 and 5
    np.testing.assert_array_equal(st2["goal_distances"], np.round(raw["dist"][[0, 5], 0], 5))
    np.testing.assert_array_equal(np.array(st2["control_inputs"]),
                                  np.round([raw["u"][1, 0], raw["xu_best"][0, 12:18]], 5))
