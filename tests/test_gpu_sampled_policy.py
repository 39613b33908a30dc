"""GPU: the multi-rate sampled-wrench loops with the plant under the winner's feedback policy
(i7m_sampled_multirate_opts.control_from = I7M_CONTROL_POLICY; csrc/i7m_mpc_sampled_policy.h
k_sampled_multirate_policy_step) at (G, H, N) = (2, 4, 8), against a host loop composed from the
library's own hooks: per step set_external_wrench, solve, qp_policy on every row, the schedule with its
knot index, the rk4 hook per plant sub-step under the actual wrench converted once at x_last's q, with
u = u_j + K_j (x - x_j) formed in numpy in the kernel's order; the replay score, the resample, the
spread and the window come from the numpy helpers.

The selected hypothesis, the goal switch and the stop are discrete: the inputs are those
tests/test_sampled_policy_ref_self.py vetted (two smallest scoring errors >= 1e-3 apart, distances
>= 1e-3 from the radius), and best, off and the NaN / -1 patterns must be identical.  The bound on the
values is measured, not chosen: the same composition with control_from="new" and the one-step score
against the device loop that existed before gives the hook-vs-kernel noise, and the policy run must
stay within 8 x that, for the one 12-term product per sub-step it adds.
"""
import ctypes as C

import numpy as np
import pytest

import policy_ref as pr
from oracle import rbd
from sampled_mpc_ref import GOAL_RADIUS, make_case, resample, score
from sampled_policy_ref import (G, H, N, PHASES, REF, SHAPES, loop_kwargs, policy_case, qp_blocks_wrench, replay_score)
from tracking_mpc_ref import make_tracking_case, window

pytestmark = pytest.mark.gpu
GAP = 1e-3
GATE = 16.0  # tests/test_gpu_policy.py's gate on the gains
T = 18 * N - 6


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def _handle(lib, model, mode, rows=G * H):
    return lib.Handle(model, N=N, max_batch=rows, qp_mode=lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT)


def kdx(K, dx):
    """K dx in the kernel's order: t_c = K_c dx_c (+ K_{c+8} dx_{c+8}, c < 4), every product and sum
    rounded on its own, then ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7))."""
    p = K * dx[..., None, :]
    t = p[..., :8].copy()
    t[..., :4] = t[..., :4] + p[..., 8:]
    return ((t[..., 0] + t[..., 4]) + (t[..., 2] + t[..., 6])) + ((t[..., 1] + t[..., 5]) + (t[..., 3] + t[..., 7]))


def host_loop(lib, h, control, xstart, num_steps, fhyp, f_actual, sim_dt, endpoints=None, ref=None, ref_phase=None,
              noise=None, keep_best=False, decay=1.0):
    """i7m_mpc_run_sampled_multirate / _tracking_multirate from the library's hooks; control "new" (the
    one-step score) or "policy" (the replay score).  Returns the entry point's outputs plus err2."""
    g_n = xstart.shape[0]
    h_n = len(fhyp) // g_n
    B = g_n * h_n
    track = ref is not None
    sub_start, sub_dt, shift, knot = lib.multirate_schedule(h.cfg.dt, sim_dt, num_steps, N, knots=True)
    off = np.cumsum(shift)
    admm = h.cfg.qp_mode == lib.QP_ADMM
    fh = np.array(fhyp, float).reshape(B, 6)
    fa = np.asarray(f_actual, float).reshape(g_n, 6)

    def sqp(xs, goals, XU):
        if admm:
            h.admm_reset(B)
        h.set_external_wrench(fh, "world")
        out = h.solve(xs, goals, XU)[0]
        Kall = h.qp_policy(out, xs, goals, N - 1)[..., :12] if control == "policy" else None
        h.set_external_wrench(None)  # (the query hooks below take their wrench as an argument)
        return out, Kall

    if track:
        phase = np.zeros(g_n, int) if ref_phase is None else np.asarray(ref_phase, int)
        goals = np.repeat(np.stack([window(ref, phase[g], 0, N) for g in range(g_n)]), h_n, axis=0)
    else:
        goals = np.tile(endpoints[0], (B, N))
    goal_idx, alive = np.zeros(g_n, int), np.ones(g_n, bool)
    xcur = np.array(xstart, float)
    xs = np.repeat(xcur, h_n, axis=0)
    XU = np.zeros((B, T))
    XU[:, :12] = xs
    XU_new, Kall = sqp(xs, goals, XU)
    xu_best = XU_new[::h_n].copy()
    K = None if Kall is None else Kall[::h_n].copy()
    d = "err" if track else "dist"
    out = {d: np.full((num_steps, g_n), np.nan), "best": np.full((num_steps, g_n), -1, np.int32),
           "q": np.full((num_steps, g_n, 6), np.nan), "u": np.full((num_steps, g_n, 6), np.nan),
           "xpath": np.full((sub_start[-1], g_n, 6), np.nan), "fbest": np.full((num_steps, g_n, 6), np.nan),
           "err2": np.full((num_steps, g_n, 2), np.nan), "jmax": 0}
    if track:
        out["ee"] = np.full((num_steps, g_n, 3), np.nan)
        out["off"] = np.asarray(off, np.int32)
    for i in range(num_steps):
        x_last, u_last = xcur.copy(), xu_best[:, 12:18].copy()
        run = np.flatnonzero(alive)
        sel = alive.copy()
        out["u"][i, run] = u_last[run]
        held = np.array([rbd.wrench_world_to_local(x_last[g, :6], fa[g]) for g in run])  # once, at x_last's q
        q, v = x_last[run, :6].copy(), x_last[run, 6:].copy()
        us = []
        for s in range(sub_start[i], sub_start[i + 1]):
            if control == "policy":
                j = int(knot[s])
                out["jmax"] = max(out["jmax"], j)
                u = xu_best[run, 18 * j + 12:18 * j + 18] + kdx(K[run, j], np.hstack([q, v]) - xu_best[run, 18 * j:18 * j + 12])
            else:
                u = u_last[run]
            us.append(u)
            q, v = h.rk4(q, v, u, sub_dt[s], fext=held, frame="local")
            out["xpath"][s, run] = q
        xcur[run] = np.hstack([q, v])
        out["q"][i, run] = q
        ee = h.eepos(q)
        for n, g in enumerate(run):
            r = slice(g * h_n, (g + 1) * h_n)
            xs[r] = xcur[g]
            XU[r, :12] = xcur[g]
            XU[r, 12:] = xu_best[g, 12:]
            if track:
                goals[r] = window(ref, phase[g], off[i], N)
                out["ee"][i, g] = ee[n]
                out[d][i, g] = np.linalg.norm(ee[n] - goals[g * h_n, :3])
                continue
            dist = np.linalg.norm(ee[n] - goals[g * h_n, :3])
            out[d][i, g] = dist
            assert abs(dist - GOAL_RADIUS) >= GAP
            if dist < GOAL_RADIUS:
                if goal_idx[g] < len(endpoints) - 1:
                    goal_idx[g] += 1
                    goals[r] = np.tile(endpoints[goal_idx[g]], N)
                else:
                    alive[g] = sel[g] = False
        XU_new, Kall = sqp(xs, goals, XU)
        for n, g in enumerate(run):
            if not sel[g]:
                continue
            r = slice(g * h_n, (g + 1) * h_n)
            if control == "policy":
                err, best = replay_score(x_last[g], [u[n] for u in us], sub_dt[sub_start[i]:sub_start[i + 1]], xcur[g],
                                         fh[r], "world")
            else:
                err, best = score(x_last[g], u_last[g], xcur[g], fh[r], sim_dt, "world")
            e = np.sort(np.where(np.isnan(err), np.inf, err))
            out["err2"][i, g] = [e[0], e[1] if h_n > 1 else np.inf]
            out["best"][i, g] = best
            out["fbest"][i, g] = fh[g * h_n + best]
            xu_best[g] = XU_new[g * h_n + best]
            if K is not None:
                K[g] = Kall[g * h_n + best]
            if noise is not None:
                fh[r] = resample(fh[r], best, noise[i, r], keep_best, decay)
    out.update(xcur=xcur, xu_best=xu_best, fhyp=fh)
    return out


def device_loop(h, control, xstart, num_steps, fhyp, f_actual, sim_dt, endpoints=None, ref=None, ref_phase=None, **kw):
    if ref is not None:
        return h.mpc_run_tracking_multirate(xstart, ref, num_steps, fhyp, f_actual, ref_phase=ref_phase, sim_dt=sim_dt,
                                            control_from=control, **kw)
    return h.mpc_run_sampled_multirate(xstart, endpoints, num_steps, fhyp, f_actual, sim_dt=sim_dt, control_from=control, **kw)


def compare(tag, dev, host, source):
    """best, off and the NaN / -1 patterns identical; returns max |device - host| over the values."""
    keys = ("dist" if source == "endpoints" else "err", "q", "u", "xpath", "fbest", "xcur", "xu_best", "fhyp") + \
        (() if source == "endpoints" else ("ee",))
    np.testing.assert_array_equal(dev["best"], host["best"], err_msg=tag)
    if source != "endpoints":
        np.testing.assert_array_equal(dev["off"], host["off"], err_msg=tag)
    diff = {}
    for k in keys:
        np.testing.assert_array_equal(np.isnan(dev[k]), np.isnan(host[k]), err_msg=f"{tag} {k}")
        diff[k] = float(np.nanmax(np.abs(dev[k] - host[k])))
    print(f"{tag}: max |device - host| " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    return diff


# ---- the gains under a wrench --------------------------------------------------------------------------

def test_gains_under_a_world_wrench(lib, model):
    """i7m_qp_policy on a handle with a world-frame wrench per row, N = 8, B = 5: the gains against the
    longdouble recursion on the wrench-aware blocks, gated at 16 x the float64 restatement's largest error
    on the same problems (tests/test_gpu_policy.py's gate), and sol_out = i7m_qp's buffer bit for bit."""
    from oracle.osqp_ref import synthetic_batch
    B = 5
    xc, g, XU = synthetic_batch(B, N, seed=100 + N)
    XU = XU + 0.05 * np.random.default_rng(N).standard_normal(XU.shape)
    XU[:, :12] = xc
    f = np.zeros((B, 6))
    f[:, :3] = np.random.default_rng(21).normal(0, 10.0, (B, 3))
    f[0] = 0.0
    h = _handle(lib, model, "direct", B)
    plain = h.qp_policy(XU, xc, g, N - 1)
    h.set_external_wrench(f, "world")
    sol = h.qp(XU, xc, g)
    K, psol = h.qp_policy(XU, xc, g, N - 1, want_sol=True)
    h.close()
    np.testing.assert_array_equal(psol, sol)
    np.testing.assert_array_equal(K[0], plain[0])  # the zero wrench is no wrench
    assert not np.array_equal(K[1:], plain[1:])
    blk = [qp_blocks_wrench(XU[b], xc[b], g[b], N, f[b], "world") for b in range(B)]
    ref64 = np.array([pr.riccati_gains(b) for b in blk])
    refL = np.array([pr.riccati_gains(b, np.longdouble) for b in blk])
    floor, got = pr.stage_rel_err(ref64, refL), pr.stage_rel_err(K, refL)
    moved = pr.stage_rel_err(plain[1:], refL[1:]).max()
    print(f"gains under a wrench: float64 restatement max {floor.max():.3g}, device max {got.max():.3g}, ratio "
          f"{got.max() / floor.max():.3g}; the wrench-free gains are {moved:.3g} away")
    assert floor.max() > 0 and moved > 1e3 * GATE * floor.max()  # the wrench is in the gains
    assert got.max() <= GATE * floor.max(), got.max() / floor.max()


# ---- loop parity ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("sim_dt,steps", SHAPES)
@pytest.mark.parametrize("source", ["endpoints", "tracking"])
def test_against_the_host_composed_loop(lib, model, source, sim_dt, steps, mode):
    """Structure identical, values within 8 x the NEW loop's own hook-vs-kernel noise.  Measured on an
    MI355X, max |device - host| over every output, NEW / POLICY: endpoints 3.5e-9 /
    9.8e-12 (direct) and 1.4e-5 / 9.1e-8 (ADMM) at sim_dt = 0.025, 2.3e-12 / 2.3e-12 and 1.2e-7 / 1.3e-7 at
    0.001; tracking 1.9e-10 / 3.7e-12 and 5.6e-7 / 1.4e-7 at 0.025, 9.3e-12 / 9.3e-12 and 1.3e-7 / 1.3e-7 at
    0.001.  The open-loop plant of NEW amplifies a rounding difference over a step's later sub-steps; the
    feedback damps it."""
    c = policy_case(source, sim_dt)
    kw = loop_kwargs(c)
    kw.pop("sim_dt")
    h = _handle(lib, model, mode)
    res = {}
    for control in ("new", "policy"):
        host = host_loop(lib, h, control, c["xstart"], steps, c["fhyp"], c["f_actual"], sim_dt, **kw)
        dev = device_loop(h, control, c["xstart"], steps, c["fhyp"], c["f_actual"], sim_dt, **kw)
        ran = host["best"] >= 0
        gap = (host["err2"][:, :, 1] - host["err2"][:, :, 0])[ran]
        assert (gap >= GAP).all(), (control, gap.min())
        res[control] = compare(f"{source} sim_dt={sim_dt} {mode} {control}", dev, host, source)
        res[control + "_dev"], res[control + "_host"] = dev, host
    h.close()
    d = "dist" if source == "endpoints" else "err"
    pol = res["policy_host"]
    if source == "endpoints":  # the switch at step 0 and the stop at step 1 of group 0; group 1 runs on
        assert pol[d][0, 0] < GOAL_RADIUS and pol[d][1, 0] < GOAL_RADIUS and np.isnan(pol[d][2:, 0]).all()
        assert (pol["best"][1:, 0] == -1).all() and (pol["best"][:, 1] >= 0).all()
    assert pol["jmax"] == (3 if sim_dt == 0.025 else 1)
    assert len(set(pol["best"][:, 1].tolist())) > 1  # more than one row's gains were selected
    # the feedback is not a no-op: from a step's second sub-step on the policy's plant leaves NEW's
    if sim_dt == 0.025:
        assert not np.array_equal(res["policy_dev"]["xpath"], res["new_dev"]["xpath"])
    noise = max(res["new"].values())
    worst = max(res["policy"].values())
    print(f"{source} sim_dt={sim_dt} {mode}: NEW noise {noise:.3g}, POLICY {worst:.3g}, ratio {worst / noise:.3g}")
    for k, v in res["policy"].items():
        assert v <= 8 * noise, (k, v, noise)


def test_four_waves(lib, model):
    """(G, H, N) = (1, 256, 8), direct, two steps at sim_dt = 0.025: every wave forms K dx for itself, the
    argmin crosses the waves.  Against the same host loop."""
    xs, fhyp, _, _ = make_tracking_case(1, 256, seed=4)
    fact = fhyp[200][None].copy()  # a hypothesis of the last wave
    h = _handle(lib, model, "direct", 256)
    res = {}
    for control in ("new", "policy"):
        host = host_loop(lib, h, control, xs, 2, fhyp, fact, 0.025, ref=REF, ref_phase=PHASES[:1])
        dev = device_loop(h, control, xs, 2, fhyp, fact, 0.025, ref=REF, ref_phase=PHASES[:1])
        gap = host["err2"][:, :, 1] - host["err2"][:, :, 0]
        assert (gap >= GAP).all(), gap.min()
        res[control] = compare(f"four waves {control}", dev, host, "tracking")
        if control == "policy":  # the exact 0 of the true row, in the last wave
            np.testing.assert_array_equal(dev["best"], [[200], [200]])
    h.close()
    noise, worst = max(res["new"].values()), max(res["policy"].values())
    print(f"four waves: NEW noise {noise:.3g}, POLICY {worst:.3g}")
    assert worst <= 8 * noise


# ---- the score ---------------------------------------------------------------------------------------

def test_true_hypothesis_scores_exactly_zero(lib, model):
    """One group, H = 4, sim_dt = 0.025 (three or four sub-steps a step), no resampling: hypothesis 2 is
    the actual wrench, hypothesis 1 differs from it by 1e-6 N.  best == 2 at every step: only an exact 0
    beats the near twin at the lower index.  (Under control_from="new" the one-step score cannot tell them
    apart that way: its true hypothesis scores small but not 0.)"""
    xs, fhyp, _, _ = make_tracking_case(1, 4, seed=3)
    fhyp = fhyp.copy()
    fhyp[1] = fhyp[2]
    fhyp[1, 0] += 1e-6
    fact = fhyp[2][None].copy()
    h = _handle(lib, model, "direct", 4)
    got = h.mpc_run_tracking_multirate(xs, REF, 6, fhyp, fact, ref_phase=PHASES[:1], sim_dt=0.025, control_from="policy")
    assert (np.diff(got["sub_start"]) >= 3).all() and np.isfinite(got["err"]).all()
    np.testing.assert_array_equal(got["best"], np.full((6, 1), 2))
    np.testing.assert_array_equal(got["fbest"], np.tile(fact, (6, 1, 1)))
    h.close()


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("source", ["endpoints", "tracking"])
def test_zero_gains_reduce_to_new(lib, model, monkeypatch, source, mode):
    """I7M_POLICY_ZERO_K=1 at handle creation zeroes the policy pass's gains.  At sim_dt = 0.001 every
    sub-step of steps 0 .. 8 is alone in knot 0, so the control is control_from="new"'s and the replay is
    the one-step score: best, off and the NaN patterns must be identical.  Measured on an MI355X
    (DESIGN.md §4.12): every value is equal bit for bit as well, through the other kernel, so that is
    asserted.  It rests on how the compiler contracts rk4_step in the two kernels' loops (§4.11)."""
    c = policy_case(source, 0.001)
    kw = loop_kwargs(c)
    kw.pop("sim_dt")
    kw["noise"] = c["noise"][:9]
    new = device_loop(_handle(lib, model, mode), "new", c["xstart"], 9, c["fhyp"], c["f_actual"], 0.001, **kw)
    monkeypatch.setenv("I7M_POLICY_ZERO_K", "1")
    hz = _handle(lib, model, mode)
    monkeypatch.delenv("I7M_POLICY_ZERO_K")
    got = device_loop(hz, "policy", c["xstart"], 9, c["fhyp"], c["f_actual"], 0.001, **kw)
    hz.close()
    assert (np.diff(new["sub_start"]) == 1).all()
    diff = compare(f"zero gains {source} {mode} (policy vs new)", got, new, source)
    np.testing.assert_array_equal(got["fbest"], new["fbest"])
    for k in diff:  # measured on an MI355X: every value equal bit for bit, both sources and modes
        np.testing.assert_array_equal(got[k], new[k], err_msg=k)


# ---- refusals and drivers ------------------------------------------------------------------------------

def test_refusals(lib, model):
    """I7M_EINVAL with the argument named, before any device work."""
    c = policy_case("endpoints", 0.025)
    xs, ends, fhyp, fact = c["xstart"], c["endpoints"], c["fhyp"], c["f_actual"]
    h = _handle(lib, model, "direct")
    for bad in ("prev", 3, -1):
        with pytest.raises(lib.I7MError, match=r"mpc_run_sampled_multirate: control_from = -?\d is not I7M_CONTROL_NEW"):
            h.mpc_run_sampled_multirate(xs, ends, 1, fhyp, fact, sim_dt=0.02, control_from=bad)
        with pytest.raises(lib.I7MError, match=r"mpc_run_tracking_multirate: control_from = -?\d is not I7M_CONTROL_NEW"):
            h.mpc_run_tracking_multirate(xs, c.get("ref", np.zeros((4, 3))), 1, fhyp, fact, sim_dt=0.02, control_from=bad)
    # a step of N - 1 = 7 knots: NEW runs it, POLICY has no control for knot 7
    assert np.isfinite(h.mpc_run_sampled_multirate(xs, ends, 1, fhyp, fact, sim_dt=0.07)["xpath"][:, 1]).all()
    with pytest.raises(lib.I7MError,
                       match="mpc_run_sampled_multirate: sim_dt = 0.070000 completes more than N - 2 = 6 knots in step 0"):
        h.mpc_run_sampled_multirate(xs, ends, 1, fhyp, fact, sim_dt=0.07, control_from="policy")
    assert np.isfinite(h.mpc_run_sampled_multirate(xs, ends, 1, fhyp, fact, sim_dt=0.06, control_from="policy")["xpath"][:, 1]).all()
    # the defaults struct carries I7M_CONTROL_NEW where it carried the pad
    o = lib.i7m_sampled_multirate_opts()
    assert h._lib.i7m_sampled_multirate_opts_default(C.byref(o)) == 0 and o.control_from == lib.CONTROL_NEW
    assert h._lib.i7m_abi_version() == 12 == lib.ABI_VERSION
    h.close()


def test_drivers_with_feedback(lib, model):
    """MPC_GATO_Batch_Sample.run_mpc_fig8 / run_mpc with feedback=True: the raw policy call row for row,
    not the feedback=False run, whatever sim_dt is; the defaults are the runs they were."""
    from indy7_mpc_amd.gato_mpc_batch_sample import MPC_GATO_Batch_Sample
    fig8 = REF[:6 * N + 25].reshape(-1)
    mk = lambda f=None: MPC_GATO_Batch_Sample(model, N=N, dt=0.01, batch_size=H, constant_f_ext=f, f_ext_std=10.0,  # noqa: E731
                                              seed=3, qp_mode="direct")
    probe = mk()
    f = probe.f_ext_batch[2].copy()
    paths = {}
    for fb in (True, False, None):
        ctrl = mk(f)
        kw = {} if fb is None else dict(feedback=fb)
        xpath, stats = ctrl.run_mpc_fig8(np.zeros(12), fig8, 0.02, 15, **kw)
        raw = _handle(lib, model, "direct", H).mpc_run_tracking_multirate(
            np.zeros((1, 12)), REF[:6 * N + 25], 13, probe.f_ext_batch, np.concatenate([f[:3], np.zeros(3)])[None],
            sim_dt=0.02, control_from="policy" if fb else "new")
        assert len(xpath) == 26 and np.isfinite(np.array(xpath)).all()
        np.testing.assert_array_equal(np.array(xpath), raw["xpath"][:, 0])
        np.testing.assert_array_equal(stats["best_ids"], raw["best"][:, 0])
        paths[fb] = np.array(xpath)
    np.testing.assert_array_equal(paths[None], paths[False])
    assert not np.array_equal(paths[True], paths[False])
    # run_mpc: feedback=True goes through the multi-rate loop at sim_dt <= dt too
    xs, ends, _, _, _ = make_case(1, H, seed=1)
    for sim_dt, steps in ((0.02, 6), (0.005, 6)):
        ctrl = mk(f)
        path, st = ctrl.run_mpc(xs[0], ends, sim_dt=sim_dt, sim_time=steps * sim_dt + 1e-9, feedback=True)
        raw = _handle(lib, model, "direct", H).mpc_run_sampled_multirate(xs, ends, steps, probe.f_ext_batch, f[None],
                                                                        sim_dt=sim_dt, control_from="policy")
        np.testing.assert_array_equal(np.array(path), raw["xpath"][:, 0])
        np.testing.assert_array_equal(st["best_ids"], raw["best"][:, 0])
    ctrl = mk(f)
    path, _ = ctrl.run_mpc(xs[0], ends, sim_dt=0.005, sim_time=0.03 + 1e-9)  # the default: the single-rate loop
    raw = _handle(lib, model, "direct", H).mpc_run_sampled(xs, ends, 6, probe.f_ext_batch, f[None], sim_dt=0.005)
    np.testing.assert_array_equal(np.array(path), raw["q"][:, 0])
