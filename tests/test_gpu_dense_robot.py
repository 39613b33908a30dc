"""GPU: the runtime-model kernels on a robot that is not Indy7 (tests/golden/dense6.json,
tests/dense_robot.py), through the C-ABI, against the oracle on the same robot.

A model that is not bit-identical to the baked-in Indy7 runs the SPEC = false instantiations of
k_linearize, k_linesearch and k_sqp_fused, and every other kernel reads the model from device
memory; Indy7's zeros, identity rotations and symmetric limits hide a wrong index or sign in any of
those reads.  On the dense robot every model number moves a checked output
(tests/test_dense_robot_host.py).  Every handle here is made from dense_model(); the references run
under the dense_oracle fixture, which points oracle.rbd (and through it the C++ port and the loop
references) at the same file.

Tolerances are the project's own, from its tests of the same quantity on Indy7 (test_gpu_parity,
test_gpu_wrench, test_gpu_admm, test_gpu_box, test_gpu_riccati_value and the closed-loop modules);
the references alone stay inside them on this robot (tests/test_dense_robot_host.py).

Measured on an MI355X: every test passes and no kernel needed a change.  Full SQP against the port
2.1e-14 at (N, B) = (16, 300), 2.8e-14 at (32, 64); closed loops in direct mode within 7e-15 of
their references on q (the ADMM multi-rate case 9.3e-12, against 1e-8; its reference moves q by
9.5e-12 when the start state is perturbed by 1e-13 relative).  That the tests can fail was checked
with four builds carrying one wrong model read each: g[0] with the wrong sign in rnea (26 of the 38
tests fail), g[0] and g[1] swapped in k_linearize's seed (25), q's lower bound taken as -q_upper in
box_tab_fill (the box QP test and mask 1) and t[1] for t[2] in crba's composite centre of mass (27).
On Indy7 the first three compute the same numbers as the correct code.

Kernel -> test:
  k_eepos                     test_eepos_and_jacobian_every_query
  k_aba                       test_aba_every_query
  k_abad                      test_aba_derivatives_every_query, test_linearisation_equals_dual_number_path
  k_rk4                       test_rk4_every_query
  k_linearize<false>          test_linearisation_and_cost_match_oracle, test_linearisation_equals_dual_number_path
  k_merit                     test_merit_every_column
  k_linesearch<false>         test_full_sqp_matches_numpy_oracle, test_full_sqp_every_problem_matches_port (1, 2, 4 waves)
  k_sqp_fused<false>          test_full_sqp_every_problem_matches_port (FUSED, FUSED_ITER)
  k_ipm_*                     test_box_qp_binds_on_both_sides, test_box_sqp_matches_oracle, test_box_mask_leaves_the_other_rows_free
  k_mpc_goal, k_mpc_advance   test_closed_loop_mpc_run
  k_mpc_multirate_step        test_closed_loop_multirate
  k_sampled_step              test_closed_loop_sampled, test_closed_loop_tracking
  k_sampled_multirate_step    test_closed_loop_sampled_multirate
  k_ctrl_measure              test_controller_session
"""
import numpy as np
import pytest

from dense_robot import dense_model, dense_oracle  # noqa: F401  (dense_oracle: fixture)
from oracle import box_ipm, cpu, rbd
from oracle.osqp_ref import OSQPSolverRef, SQPRef, synthetic_batch

pytestmark = pytest.mark.gpu
DT = 0.01


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


@pytest.fixture(scope="module")
def dense():
    return dense_model()


def _close(got, ref, tol):
    assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


def _rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-300)


def _knots(XU, N):
    """q, v, u (B (N - 1), 6) of every knot that has a control."""
    K = XU[:, :18 * (N - 1)].reshape(-1, 18)
    return K[:, :6], K[:, 6:12], K[:, 12:]


def _wrench(rng, n):
    return np.hstack([rng.normal(0, 10, (n, 3)), rng.normal(0, 2, (n, 3))])


# ---- the query hooks, every element --------------------------------------------------------------
def test_eepos_and_jacobian_every_query(lib, dense, dense_oracle):
    """257 queries: one past a 256-thread block."""
    q = np.random.default_rng(1).uniform(-3, 3, (257, 6))
    p, J = lib.Handle(dense, N=8, max_batch=1).eepos(q, jacobian=True)
    for i in range(257):
        pe, Je = rbd.d_eepos(q[i], dense_oracle)
        np.testing.assert_allclose(p[i], pe, rtol=0, atol=1e-13, err_msg=str(i))
        np.testing.assert_allclose(J[i], Je, rtol=0, atol=1e-13, err_msg=str(i))


@pytest.mark.parametrize("frame", [None, "local", "world"])
def test_aba_every_query(lib, dense, dense_oracle, frame):
    rng = np.random.default_rng(2)
    n = 70
    q, v, t = rng.uniform(-3, 3, (n, 6)), rng.uniform(-2, 2, (n, 6)), rng.uniform(-50, 50, (n, 6))
    f = _wrench(rng, n)
    h = lib.Handle(dense, N=8, max_batch=1)
    a = h.aba(q, v, t) if frame is None else h.aba(q, v, t, fext=f, frame=frame)
    for i in range(n):
        fl = None if frame is None else rbd.fext_list(q[i], f[i], frame, dense_oracle)
        np.testing.assert_allclose(a[i], rbd.aba(q[i], v[i], t[i], dense_oracle, fl), rtol=1e-10, atol=1e-9, err_msg=str(i))
    if frame is not None:
        assert not np.allclose(a, h.aba(q, v, t))


def test_aba_derivatives_every_query(lib, dense, dense_oracle):
    """43 queries of six lanes each: not a multiple of a block."""
    rng = np.random.default_rng(3)
    n = 43
    q, v, t = rng.uniform(-3, 3, (n, 6)), rng.uniform(-2, 2, (n, 6)), rng.uniform(-50, 50, (n, 6))
    dq, dv, Mi, a = lib.Handle(dense, N=8, max_batch=1).aba_derivatives(q, v, t)
    for i in range(n):
        rdq, rdv, rMi, ra = rbd.aba_derivatives(q[i], v[i], t[i], dense_oracle)
        for got, ref in ((dq[i], rdq), (dv[i], rdv), (Mi[i], rMi)):
            assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), i
        np.testing.assert_allclose(a[i], ra, rtol=1e-10, atol=1e-9)
        assert np.array_equal(Mi[i], Mi[i].T)


@pytest.mark.parametrize("dt", [0.01, 0.02])
@pytest.mark.parametrize("frame", [None, "local", "world"])
def test_rk4_every_query(lib, dense, dense_oracle, frame, dt):
    rng = np.random.default_rng(4)
    n = 33
    q, v, u = rng.uniform(-3, 3, (n, 6)), rng.uniform(-1, 1, (n, 6)), rng.uniform(-20, 20, (n, 6))
    f = _wrench(rng, n)
    h = lib.Handle(dense, N=8, max_batch=1)
    qo, vo = h.rk4(q, v, u, dt) if frame is None else h.rk4(q, v, u, dt, fext=f, frame=frame)
    for i in range(n):
        if frame == "world":  # converted once at the start q (tests/test_gpu_wrench.py)
            rq, rv = rbd.rk4(q[i], v[i], u[i], dt, P=dense_oracle, fext6_world=f[i])
            _close(qo[i], rq, 1e-12)
            _close(vo[i], rv, 1e-10)
        else:
            fl = None if frame is None else [np.zeros(6)] * 5 + [f[i]]
            rq, rv = rbd.rk4(q[i], v[i], u[i], dt, fext=fl, P=dense_oracle)
            np.testing.assert_allclose(qo[i], rq, rtol=1e-12, atol=1e-12, err_msg=str(i))
            np.testing.assert_allclose(vo[i], rv, rtol=1e-10, atol=1e-10, err_msg=str(i))


# ---- k_linearize<false>, k_merit -----------------------------------------------------------------
def _lin_inputs(P, N, B, seed, sigma):
    """A non-trivial linearisation point: the synthetic start, every entry perturbed by N(0, sigma)."""
    xcur, goals, XU = synthetic_batch(B, N, seed, P=P)
    return xcur, goals, XU + np.random.default_rng(seed + 1).normal(0, sigma, XU.shape)


@pytest.mark.parametrize("frame", [None, "local", "world"])
def test_linearisation_and_cost_match_oracle(lib, dense, dense_oracle, frame):
    """Every knot of every problem: all 114 lin entries against the complex-step oracle (with a
    wrench: including d(actInv(oMi6(q)) f)/dq), all 10 cost entries against what OSQPSolverRef
    writes into its g and P for the same XU."""
    N, B = 8, 3
    xcur, goals, XU = _lin_inputs(dense_oracle, N, B, 14, 0.3)
    fw = _wrench(np.random.default_rng(6), B)
    h = lib.Handle(dense, N=N, max_batch=B)
    if frame is not None:
        h.set_external_wrench(fw, frame)
    lin, cost = h.linearize(XU, goals)
    for b in range(B):
        for k in range(N - 1):
            q, v, u = XU[b, 18 * k:18 * k + 6], XU[b, 18 * k + 6:18 * k + 12], XU[b, 18 * k + 12:18 * k + 18]
            dq, dv, Mi, a = rbd.aba_derivatives(q, v, u, dense_oracle, fext6=None if frame is None else fw[b],
                                                frame=frame or "local")
            _close(lin[b, k, 108:], a, 1e-10)
            _close(lin[b, k, :36].reshape(6, 6), DT * dq, 1e-9)
            _close(lin[b, k, 36:72].reshape(6, 6), np.eye(6) + DT * dv, 1e-9)
            _close(lin[b, k, 72:108].reshape(6, 6), DT * Mi, 1e-9)
        s = OSQPSolverRef(N=N, P=dense_oracle)
        s.update_cost_matrix(XU[b], goals[b])
        for k in range(N):
            Qm = s.QN_cost if k == N - 1 else 1.0
            pe, _ = rbd.d_eepos(XU[b, 18 * k:18 * k + 6], dense_oracle)
            ref = np.concatenate([s.g[18 * k:18 * k + 6] / Qm,                       # j = J'e
                                  [Qm, s.Pdata[33 * k + 21], s.R_cost / s.dQ_cost * s.Pdata[33 * k + 21],
                                   np.linalg.norm(pe - goals[b, 3 * k:3 * k + 3])]])
            if k < N - 1:
                assert ref[8] == pytest.approx(s.Pdata[33 * k + 27], rel=1e-14)     # Rm as the oracle stores it
            assert np.abs(cost[b, k, :6] - ref[:6]).max() <= 1e-10 * np.abs(ref[:6]).max(), (b, k)
            assert (np.abs(cost[b, k, 6:] - ref[6:]) <= 1e-10 * np.abs(ref[6:])).all(), (b, k, cost[b, k, 6:], ref[6:])
    if frame is not None:
        h.set_external_wrench(None)
        assert not np.allclose(h.linearize(XU, goals)[0], lin)


def test_linearisation_equals_dual_number_path(lib, dense, dense_oracle):
    """Two device derivative algorithms on the same knots: k_linearize<false> (analytic) and
    k_abad (forward-mode dual-number RNEA), as test_gpu_parity does for Indy7."""
    N, B = 8, 3
    xcur, goals, XU = _lin_inputs(dense_oracle, N, B, 17, 0.8)
    h = lib.Handle(dense, N=N, max_batch=B)
    lin, _ = h.linearize(XU, goals)
    dq, dv, Mi, a = h.aba_derivatives(*_knots(XU, N))
    L = lin.reshape(-1, 114)
    assert len(L) == len(a) == B * (N - 1)
    for n in range(len(L)):
        np.testing.assert_allclose(L[n, :36].reshape(6, 6), DT * dq[n], rtol=1e-9, atol=1e-10 * max(1, DT * np.abs(dq[n]).max()))
        np.testing.assert_allclose(L[n, 36:72].reshape(6, 6), np.eye(6) + DT * dv[n], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(L[n, 72:108].reshape(6, 6), DT * Mi[n], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(L[n, 108:], a[n], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("wrench", [False, True])
def test_merit_every_column(lib, dense, dense_oracle, wrench):
    """qcost, vcost, ucost, the integrator error and |XU[:12] - XU_ref[:12]|, 1e-10 relative."""
    N, B = 8, 3
    xcur, goals, XU = _lin_inputs(dense_oracle, N, B, 6, 0.2)
    ref_xu = XU + np.random.default_rng(8).normal(0, 0.1, XU.shape)
    fw = _wrench(np.random.default_rng(9), B)
    h = lib.Handle(dense, N=N, max_batch=B)
    if wrench:
        h.set_external_wrench(fw, "world")
    m = h.merit(XU, ref_xu, goals)
    for b in range(B):
        sq = SQPRef(OSQPSolverRef(N=N, P=dense_oracle, fext6=fw[b] if wrench else None, fext_frame="world"))
        ref = np.array([*sq.eepos_cost(goals[b], XU[b]), sq.integrator_err(XU[b]), np.linalg.norm(XU[b, :12] - ref_xu[b, :12])])
        assert (ref > 0).all()
        assert (np.abs(m[b] - ref) <= 1e-10 * ref).all(), (b, m[b], ref)


# ---- the exact QP --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 16])
def test_qp_matches_exact_kkt(lib, dense, dense_oracle, N):
    B = 3
    xcur, goals, XU = _lin_inputs(dense_oracle, N, B, 7, 0.3)
    sol = lib.Handle(dense, N=N, max_batch=B).qp(XU, xcur, goals)
    for b in range(B):
        ref = OSQPSolverRef(N=N, P=dense_oracle).setup_and_solve_qp(XU[b], xcur[b], goals[b]).x
        assert _rel(sol[b], ref) < 1e-8, (b, _rel(sol[b], ref))


def test_qp_value_matches_kkt(lib, dense, dense_oracle):
    """i7m_qp_value at N = 10 against the KKT reference of tests/test_gpu_riccati_value.py."""
    from test_gpu_riccati_value import _rel as rel_max, kkt_reference
    N, B = 10, 4
    xcur, goals, XU = synthetic_batch(B, N, 61, P=dense_oracle)
    s = OSQPSolverRef(N=N, P=dense_oracle)
    XU[2:] += 0.25 * (np.stack([s.setup_and_solve_qp(XU[b], xcur[b], goals[b]).x for b in range(2, B)]) - XU[2:])
    h = lib.Handle(dense, N=N, max_batch=B)
    sol, V0 = h.qp(XU, xcur, goals), h.qp_value(XU, xcur, goals)
    for b in range(B):
        x, y0, Vxx = kkt_reference(s, XU[b], xcur[b], goals[b])
        V = V0[b]
        assert rel_max(sol[b], x) <= 1e-8, (b, rel_max(sol[b], x))
        assert rel_max(V[:12, :12], Vxx) <= 1e-8, (b, rel_max(V[:12, :12], Vxx))
        assert rel_max(V[:12, 12], y0 - Vxx @ xcur[b]) <= 1e-8, b
        assert np.abs(V[:12, :12] - V[:12, :12].T).max() / np.abs(V[:12, :12]).max() <= 1e-10, b


# ---- full SQP, direct mode -----------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", [(8, 6, 5), (16, 6, 7)])
def test_full_sqp_matches_numpy_oracle(lib, dense, dense_oracle, N, B, seed):
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    out, st = lib.Handle(dense, N=N, max_batch=B).solve(xcur, goals, XU)
    seen = set()
    for b in range(B):
        sq = SQPRef(OSQPSolverRef(N=N, P=dense_oracle))
        ref = sq.sqp(xcur[b], goals[b], XU[b].copy())
        s = sq.get_stats()
        seen |= set(s["linesearch_alphas"]["values"])
        assert st["qp_iters"][b] == s["qp_iters"]["values"][0]
        np.testing.assert_array_equal(st["alphas"][b][:st["n_alphas"][b]], s["linesearch_alphas"]["values"])
        assert _rel(out[b], ref) < 1e-6, (b, _rel(out[b], ref))
    assert len(seen) >= 3, seen  # (the oracle's: not an all-ones line search)


@pytest.mark.parametrize("N,B,seed", [(16, 300, 5), (32, 64, 7)])
def test_full_sqp_every_problem_matches_port(lib, dense, dense_oracle, N, B, seed, monkeypatch):
    """Every problem against the C++ port; then every line-search wave count (I7M_LS_WAVES 1, 2, 4)
    and every pipeline bit-identical to the three-kernel path, as test_gpu_edges asserts for Indy7."""
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    ref, qp, al, _ = cpu.solve(xcur, goals, XU, N, nthreads=8)
    assert len(np.unique(al[~np.isnan(al)])) >= 3
    outs = {}
    for nw in ("1", "2", "4"):
        monkeypatch.setenv("I7M_LS_WAVES", nw)
        h = lib.Handle(dense, N=N, max_batch=B, pipeline=lib.PIPE_SPLIT)
        outs["waves " + nw] = h.solve(xcur, goals, XU)
        h.close()
    monkeypatch.delenv("I7M_LS_WAVES")
    for pipe in (lib.PIPE_SPLIT, lib.PIPE_FUSED, lib.PIPE_FUSED_ITER, lib.PIPE_AUTO):
        h = lib.Handle(dense, N=N, max_batch=B, pipeline=pipe)
        outs[f"pipeline {pipe}"] = h.solve(xcur, goals, XU)
        h.close()
    out, st = outs[f"pipeline {lib.PIPE_SPLIT}"]
    np.testing.assert_array_equal(st["qp_iters"], qp)
    ran = np.arange(8)[None, :] < st["n_alphas"][:, None]
    np.testing.assert_array_equal(st["n_alphas"], qp)
    np.testing.assert_array_equal(st["alphas"][ran], al[ran])
    print(f"N={N} B={B}: max relative XU error against the port {_rel(out, ref).max():.3g}")
    assert _rel(out, ref).max() < 1e-6
    for name, (o, s) in outs.items():
        np.testing.assert_array_equal(o, out, err_msg=name)
        for key in ("qp_iters", "n_alphas", "alphas", "n_steps", "stepsizes"):
            np.testing.assert_array_equal(s[key], st[key], err_msg=f"{name} {key}")


# ---- ADMM mode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", [(8, 13, 5), (16, 64, 7)])
def test_admm_solves_match_port(lib, dense, dense_oracle, N, B, seed):
    """test_gpu_admm.py::test_admm_solves_match_port's assertions on the dense robot."""
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    h = lib.Handle(dense, N=N, max_batch=B, qp_mode=lib.QP_ADMM)
    st = cpu.AdmmState(B, N)
    xin = XU
    for call in range(2):
        out, s = h.solve(xcur, goals, xin)
        it, rho = h.admm_stats(B)
        ref, qp, al, _, it_r = cpu.solve_admm(xcur, goals, xin, N, st)
        np.testing.assert_array_equal(s["qp_iters"], qp)
        for b in range(B):
            n = qp[b]
            np.testing.assert_array_equal(it[b, :n], it_r[b, :n], err_msg=f"call {call} problem {b}")
            np.testing.assert_array_equal(s["alphas"][b, :s["n_alphas"][b]], al[b, :n])
        assert _rel(out, ref).max() < 5e-8, _rel(out, ref).max()
        x, z, y, q, r = h.admm_state(B)
        np.testing.assert_allclose(r, st.rho, rtol=0, atol=0)
        for a, b_ in ((x, st.x), (z, st.z), (y, st.y), (q, st.q)):
            assert _rel(a, b_).max() < 5e-8
        xin = out


# ---- box mode ------------------------------------------------------------------------------------
def _box_relerr(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _box_points(P, N=16, B=3, seed=5, margin=0.03, speed=0.3):
    """tests/test_gpu_box.py::_qp_inputs's linearisation points (the start, and a quarter step
    towards the equality-only minimiser) from start states that make the q rows bind as well: every
    joint within `margin` of its range of one of its limits (the side drawn per joint), moving
    towards it at `speed` of its velocity limit."""
    _, goals, XU = synthetic_batch(B, N, seed, P=P)
    side = np.random.default_rng(seed + 1000).choice([-1.0, 1.0], (B, 6))
    w = P.q_upper - P.q_lower
    xcur = np.hstack([np.where(side > 0, P.q_upper - margin * w, P.q_lower + margin * w), side * speed * P.v_limit])
    XU[:, :12] = xcur
    s = OSQPSolverRef(N=N, P=P)
    XU2 = XU.copy()
    for b in range(B):
        XU2[b] += 0.25 * (s.setup_and_solve_qp(XU[b], xcur[b], goals[b]).x - XU[b])
    return np.vstack([xcur, xcur]), np.vstack([goals, goals]), np.vstack([XU, XU2])


def test_box_qp_binds_on_both_sides(lib, dense, dense_oracle):
    """One box QP per point at N = 16: iterations and convergence identical, the minimiser to 1e-6
    and strictly inside.  The limits of the dense robot are asymmetric and differ per joint, and the
    oracle alone shows active rows (slack < 1e-3) on a lower and on an upper bound of each of q, v
    and u (measured: q 7 / 15, v 94 / 65, u 3 / 4 rows, 6 to 12 interior-point iterations)."""
    N = 16
    xcur, goals, XU = _box_points(dense_oracle)
    B = XU.shape[0]
    h = lib.Handle(dense, N=N, max_batch=B, qp_mode=lib.QP_BOX)
    sol = h.qp(XU, xcur, goals)
    it, conv, mu = h.box_stats(B)
    ref = OSQPSolverRef(N=N, qp="box", P=dense_oracle)
    lo, hi, bm = box_ipm.box_bounds(dense_oracle, N)
    cls = np.concatenate([np.repeat([box_ipm.MASK_Q, box_ipm.MASK_V, box_ipm.MASK_U], 6)] * N)[:18 * N - 6]
    active = {(c, side): 0 for c in (box_ipm.MASK_Q, box_ipm.MASK_V, box_ipm.MASK_U) for side in ("lower", "upper")}
    for b in range(B):
        x = ref.setup_and_solve_qp(XU[b], xcur[b], goals[b]).x
        r = ref.last_ipm
        for c in (box_ipm.MASK_Q, box_ipm.MASK_V, box_ipm.MASK_U):
            active[c, "lower"] += int((bm & (cls == c) & (x - lo < 1e-3)).sum())
            active[c, "upper"] += int((bm & (cls == c) & (hi - x < 1e-3)).sum())
        assert r.converged and conv[b] and it[b] == r.iters, (b, it[b], r.iters)
        assert _box_relerr(sol[b], x) <= 1e-6, (b, _box_relerr(sol[b], x))
        assert (sol[b][bm] > lo[bm]).all() and (sol[b][bm] < hi[bm]).all()
    print("active rows (class, side):", active)
    assert all(n > 0 for n in active.values()), active


def test_box_sqp_matches_oracle(lib, dense, dense_oracle):
    N, B = 16, 4
    xcur, goals, XU = synthetic_batch(B, N, 5, P=dense_oracle)
    out, st = lib.Handle(dense, N=N, max_batch=B, qp_mode=lib.QP_BOX).solve(xcur, goals, XU)
    s = OSQPSolverRef(N=N, qp="box", P=dense_oracle)
    for b in range(B):
        sq = SQPRef(s)
        ref = sq.sqp(xcur[b], goals[b], XU[b].copy())
        al = list(st["alphas"][b][: st["n_alphas"][b]])
        assert al == sq.stats["linesearch_alphas"]["values"], (b, al, sq.stats["linesearch_alphas"]["values"])
        assert _box_relerr(out[b], ref) <= 1e-5, (b, _box_relerr(out[b], ref))


@pytest.mark.parametrize("mask", [1, 2, 4])
def test_box_mask_leaves_the_other_rows_free(lib, dense, dense_oracle, mask):
    """test_gpu_settings.py's test of the same name, on the dense robot's points."""
    N = 16
    xcur, goals, xu = _box_points(dense_oracle)
    B = xu.shape[0]
    h = lib.Handle(dense, N=N, max_batch=B, qp_mode=lib.QP_BOX, box_mask=mask)
    sol = h.qp(xu, xcur, goals)
    it, conv, mu = h.box_stats(B)
    h.close()
    ref = OSQPSolverRef(N=N, qp="box", box_mask=mask, P=dense_oracle)
    lo, hi, bm = box_ipm.box_bounds(dense_oracle, N, mask)
    lo7, hi7, bm7 = box_ipm.box_bounds(dense_oracle, N)
    free = bm7 & ~bm
    assert bm.any() and free.any()
    outside = 0
    for b in range(B):
        x = ref.setup_and_solve_qp(xu[b], xcur[b], goals[b]).x
        r = ref.last_ipm
        assert conv[b] == r.converged and it[b] == r.iters, (b, it[b], r.iters)
        assert _box_relerr(sol[b], x) <= 1e-6, (b, _box_relerr(sol[b], x))
        assert (sol[b][bm] > lo[bm]).all() and (sol[b][bm] < hi[bm]).all()
        outside += int(((sol[b][free] < lo7[free]) | (sol[b][free] > hi7[free])).sum())
    assert (mu > 0).all(), mu
    assert outside > 0


# ---- closed loops: each loop's own reference and comparison, under the patched model ---------------
def _mode(lib, mode):
    return lib.QP_ADMM if mode == "admm" else lib.QP_DIRECT


def test_closed_loop_mpc_run(lib, dense, dense_oracle):
    """i7m_mpc_run (k_mpc_goal, k_mpc_advance): B = 3, N = 16, 5 steps, each instance against its own
    oracle run (oracle/mpc_ref.py), test_gpu_mpc.py's tolerance."""
    from multirate_mpc_ref import make_case
    from oracle.mpc_ref import run_mpc_ref
    xs, ends = make_case()
    xs, N, steps = xs[1:], 16, 5
    d, q, xc, xu = lib.Handle(dense, N=N, max_batch=3).mpc_run(xs, ends, steps)
    for b in range(3):
        xpath, dists = run_mpc_ref(SQPRef(OSQPSolverRef(N=N, P=dense_oracle)), xs[b], ends, num_steps=steps)
        assert len(dists) == len(xpath) == steps and min(abs(x - 0.1) for x in dists) >= 1e-3  # no stop, clear of the radius
        np.testing.assert_allclose(d[:, b], dists, rtol=0, atol=2e-6)
        np.testing.assert_allclose(q[:, b], np.array(xpath), rtol=0, atol=2e-6)
    np.testing.assert_array_equal(xc[:, :6], q[-1])


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_closed_loop_multirate(lib, dense, dense_oracle, mode):
    """i7m_mpc_run_multirate (k_mpc_multirate_step): B = 2, N = 8, 6 steps at sim_dt 0.004, so a
    plant step splits at a knot (steps 2 and 4); test_gpu_multirate_mpc.py's comparison."""
    from multirate_mpc_ref import make_case, run_multirate_ref
    from test_gpu_multirate_mpc import GAP, TOL
    xs, ends = make_case()
    xs, N, steps = xs[[1, 3]], 8, 6
    ref = run_multirate_ref(N, xs, ends, steps, sim_dt=0.004, qp_mode=mode)
    assert np.nanmin(ref["margin"]) >= GAP and np.isfinite(ref["dist"]).all()
    assert (np.diff(ref["sub_start"]) == 2).any() and ref["shift"].sum() == 2
    got = lib.Handle(dense, N=N, max_batch=2, qp_mode=_mode(lib, mode)).mpc_run_multirate(xs, ends, steps, sim_dt=0.004)
    err = {k: np.nanmax(np.abs(got[k] - ref[k])) for k in ("dist", "q", "xpath", "u")}
    print(f"multirate {mode}: max |got - ref| " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()))
    for key in ("dist", "q", "xpath"):
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(ref[key]), err_msg=key)
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL[mode], err_msg=key)
    np.testing.assert_array_equal(got["sub_start"], ref["sub_start"])
    np.testing.assert_array_equal(got["shift"], ref["shift"])
    np.testing.assert_array_equal(got["q"], got["xpath"][got["sub_start"][1:] - 1])
    np.testing.assert_array_equal(got["xu"][:, :12], got["xcur"])


def test_closed_loop_sampled(lib, dense, dense_oracle):
    """i7m_mpc_run_sampled (k_sampled_step): G = 2, H = 4, N = 8, 4 steps, world frame, resampling
    noise with the best kept, so the true hypothesis stays among the rows: it scores exactly 0 in the
    reference (plant and score are the same computation) and is selected at every step."""
    from sampled_mpc_ref import make_case, run_sampled_ref
    from test_gpu_sampled_mpc import _check_parity
    G, H, N, steps = 2, 4, 8, 4
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1)
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    kw = dict(noise=noise, sim_dt=0.01, keep_best=True, decay=1.0)
    ref = run_sampled_ref(N, G, H, xs, ends, steps, fhyp, fact, qp_mode="direct", **kw)
    assert (ref["err2"][:, :, 0] == 0.0).all()
    np.testing.assert_array_equal(ref["best"], np.tile(k, (steps, 1)))
    h = lib.Handle(dense, N=N, max_batch=G * H)
    got = h.mpc_run_sampled(xs, ends, steps, fhyp, fact, **kw)
    _check_parity("dense sampled direct", got, ref, "direct", steps, G)
    np.testing.assert_array_equal(got["fbest"], np.tile(fact, (steps, 1, 1)))
    assert np.abs(got["fhyp"] - ref["fhyp"]).max() <= 1e-12 and np.abs(got["fhyp"] - fhyp).max() > 0.1
    # the device's winning error of step 0, recovered through the rk4 hook: the plant's own computation
    u0 = h.mpc_run_sampled(xs, ends, 0, fhyp, fact, sim_dt=0.01)["xu_best"][:, 12:18]
    one = h.mpc_run_sampled(xs, ends, 1, fhyp, fact, sim_dt=0.01)
    qn, vn = h.rk4(xs[:, :6], xs[:, 6:], u0, 0.01, fext=one["fbest"][0], frame="world")
    assert (np.linalg.norm(np.hstack([qn, vn]) - one["xcur"], axis=1) <= 1e-12).all()


def test_closed_loop_tracking(lib, dense, dense_oracle):
    """i7m_mpc_run_tracking (k_sampled_step's goal phase): G = 2, H = 4, N = 8, 4 steps."""
    from test_gpu_tracking_mpc import REF, _check_parity
    from tracking_mpc_ref import make_tracking_case, run_tracking_ref
    G, H, N, steps = 2, 4, 8, 4
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    off = np.arange(1, steps + 1)
    ref = run_tracking_ref(N, G, H, xs, REF, off, fhyp, fact, sim_dt=0.01, qp_mode="direct")
    assert (ref["err2"][:, :, 0] == 0.0).all()
    got = lib.Handle(dense, N=N, max_batch=G * H).mpc_run_tracking(xs, REF, off, fhyp, fact, sim_dt=0.01)
    _check_parity("dense tracking direct", got, ref, "direct")
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))
    np.testing.assert_array_equal(got["fhyp"], fhyp)


def test_closed_loop_sampled_multirate(lib, dense, dense_oracle):
    """i7m_mpc_run_sampled_multirate (k_sampled_multirate_step): G = 2, H = 4, N = 8, 3 steps at
    sim_dt 0.02, two knots a step.  (The plant takes two 10 ms sub-steps and the hypotheses are scored
    by one rk4 step of 20 ms: not the same computation, so the true hypothesis scores small, not 0.)"""
    from sampled_mpc_ref import make_case
    from sampled_multirate_ref import run_sampled_multirate_ref
    from test_gpu_sampled_multirate import TOL, _check_parity
    G, H, N, steps = 2, 4, 8, 3
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1)
    ref = run_sampled_multirate_ref(N, G, H, xs, steps, fhyp, fact, endpoints=ends, sim_dt=0.02, qp_mode="direct")
    assert ref["shift"].tolist() == [2, 2, 2] and np.diff(ref["sub_start"]).tolist() == [2, 2, 2]
    got = lib.Handle(dense, N=N, max_batch=G * H).mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, sim_dt=0.02)
    _check_parity("dense sampled multirate direct", got, ref, "direct", "endpoints", TOL["direct"])
    np.testing.assert_array_equal(got["best"], np.tile(k, (steps, 1)))


def test_controller_session(lib, dense, dense_oracle):
    """i7m_ctrl_begin / _step / _end (k_ctrl_measure): 3 steps on states measured from the host
    plant, x0 given; test_gpu_controller_step.py::test_closed_loop_parity's comparison."""
    from controller_step_ref import HostPlant, run_ctrl_ref, schedule
    from test_gpu_controller_step import GAP, REF, TOL, _rel_u, _run_session
    from tracking_mpc_ref import make_tracking_case
    G, H, N, steps = 2, 4, 8, 3
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    el, off = schedule(steps)
    ref = run_ctrl_ref(N, G, H, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs, qp_mode="direct")
    assert (ref["err2"][:, :, 1] - ref["err2"][:, :, 0] >= GAP).all()
    np.testing.assert_array_equal(ref["best"], np.tile(k, (steps, 1)))
    got = _run_session(lib.Handle(dense, N=N, max_batch=G * H), G, REF, fhyp, el, off, HostPlant(xs, fact, el), x0=xs)
    print(f"controller session: u (relative) {_rel_u(got['u'], ref['u']):.3g}, x_meas {np.abs(got['x_meas'] - ref['x_meas']).max():.3g}")
    np.testing.assert_array_equal(got["best"], ref["best"])
    np.testing.assert_array_equal(got["fbest"], ref["fbest"])
    for key in ("x_meas", "err", "ee"):
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL["direct"], err_msg=key)
    assert _rel_u(got["u"], ref["u"]) <= TOL["direct"] and _rel_u(got["u0"], ref["u0"]) <= TOL["direct"]
    np.testing.assert_array_equal(got["u"][-1], got["xu_best"][:, 12:18])
    np.testing.assert_array_equal(got["fhyp"], fhyp)
