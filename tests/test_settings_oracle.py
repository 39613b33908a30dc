"""The C++ port (oracle/cpp/i7m_cpu.cpp) against the numpy restatement (oracle/osqp_ref.py SQPRef on
OSQPSolverRef) at solver settings off their defaults: the OSQP settings, max_sqp_iters / mu /
step_tol, and the box mode's mask, iteration cap and tolerance.  tests/test_gpu_settings.py
compares the device with the port at the same settings (tests/settings_cases.py holds the cases);
this file is what makes the port a reference there.

Every discrete outcome (SQP iterations, OSQP / interior-point iterations per QP, statuses,
line-search steps, converged flags) is identical; XU to 1e-8 relative in ADMM and direct mode
(tests/test_admm_oracle.py's tolerance for these two restatements) and 1e-5 in box mode
(tests/test_box_oracle.py's).  Each case also asserts that its setting changes something against the
default-settings run of the same inputs, so a setting that is silently ignored fails.
"""
import numpy as np
import pytest

from oracle import cpu
from oracle.osqp_ref import synthetic_batch
from settings_cases import (BOX_CASES, OSQP_CASES, SQP_CASES, box_relerr, choose_step_tol, ids, numpy_solves, rel,
                            step_gap)

N = 16


def _port_admm(batch, admm_kw, sqp_kw, calls):
    """`calls` consecutive port solves in ADMM mode: per call (xu, qp_iters, alphas, steps, its,
    status, rho)."""
    xcur, goals, xu = batch
    st = cpu.AdmmState(xu.shape[0], N, rho=admm_kw.get("rho", 0.1))
    res = []
    for _ in range(calls):
        xu, qp, al, ss, it = cpu.solve_admm(xcur, goals, xu, N, st, admm=cpu.admm_cfg(**admm_kw), **sqp_kw)
        res.append((xu, qp, al, ss, it, st.status.copy(), st.rho.copy()))
    return res


def _assert_admm_equal(port, ref, tol=1e-8):
    """One call of _port_admm against one call of numpy_solves (qp "osqp")."""
    xu, qp, al, _, it, status, rho = port
    np.testing.assert_array_equal(qp, ref["qp_iters"])
    for b in range(len(qp)):
        n = qp[b]
        assert list(it[b, :n]) == ref["its"][b] and (it[b, n:] == -1).all(), (b, it[b], ref["its"][b])
        assert list(status[b, :n]) == ref["status"][b] and (status[b, n:] == -1).all(), (b, status[b], ref["status"][b])
        assert list(al[b, :n]) == ref["alphas"][b] and np.isnan(al[b, n:]).all(), (b, al[b], ref["alphas"][b])
    assert rel(xu, ref["xu"]).max() <= tol, rel(xu, ref["xu"])
    np.testing.assert_allclose(rho, ref["rho"], rtol=1e-8)


@pytest.fixture(scope="module")
def batch41():
    return synthetic_batch(4, N, 41)


@pytest.fixture(scope="module")
def default41(batch41):
    """The default-settings port run each case must differ from: two consecutive solves."""
    return _port_admm(batch41, {}, {}, 2)


@pytest.mark.parametrize("name,kw", OSQP_CASES, ids=ids(OSQP_CASES))
def test_port_osqp_settings_match_numpy(batch41, default41, name, kw):
    """Two consecutive solves (the second from the first's output and OSQP state) of four problems
    with one group of OSQP settings off its default.  The setting is seen to act: the OSQP iteration
    counts differ from the default run's (scaling 3 leaves them at 25 / 50 on these four problems
    and moves XU by 3.6e-5, 4000 x the tolerance, instead); check_termination 0 runs exactly
    max_iter iterations and is "solved" by the closing test; the adaptive case moves rho."""
    port = _port_admm(batch41, kw, {}, 2)
    ref = numpy_solves(*batch41, N, dict(qp="osqp", osqp_settings=dict(kw)), {}, calls=2)
    for p, r in zip(port, ref):
        _assert_admm_equal(p, r)
    if name == "scaling3":
        assert rel(port[1][0], default41[1][0]).max() > 1e-6
    else:
        assert any((p[4] != d[4]).any() for p, d in zip(port, default41)), port[0][4]
    if name == "check0":
        ran = port[0][4] >= 0
        assert (port[0][4][ran] == 60).all() and (port[0][5][ran] == 1).all()
    if name == "adapt":
        assert (port[1][6] != kw["rho"]).any(), port[1][6]
    else:
        assert (port[1][6] == kw.get("rho", 0.1)).all()


@pytest.mark.parametrize("name,kw", SQP_CASES, ids=ids(SQP_CASES))
def test_port_sqp_settings_match_numpy(batch41, name, kw):
    """max_sqp_iters 1, 5 and 8 and mu 1 and 1000 in ADMM mode (so that the OSQP record of every
    SQP iteration is compared too).  Every problem runs max_iters QPs; mu moves the line search:
    the alphas differ from those of mu = 10 with the same four iterations."""
    port = _port_admm(batch41, {}, kw, 1)[0]
    ref = numpy_solves(*batch41, N, dict(qp="osqp"), kw)[0]
    _assert_admm_equal(port, ref)
    assert (port[1] == kw["max_iters"]).all(), port[1]
    if "mu" in kw:
        mu10 = _port_admm(batch41, {}, dict(max_iters=kw["max_iters"]), 1)[0]
        assert not np.array_equal(port[2], mu10[2], equal_nan=True)


def _ragged(mode, xcur, goals, xu, rows, kw):
    """Port against numpy on `rows` of a batch with the SQP settings kw; returns the port's
    (qp_iters, alphas) of those rows."""
    xcur, goals, xu = xcur[rows], goals[rows], xu[rows]
    if mode == "direct":
        out, qp, al, _ = cpu.solve(xcur, goals, xu, N, **kw)
        ref = numpy_solves(xcur, goals, xu, N, {}, kw)[0]
        np.testing.assert_array_equal(qp, ref["qp_iters"])
        for b in range(len(qp)):
            assert list(al[b, :qp[b]]) == ref["alphas"][b] and np.isnan(al[b, qp[b]:]).all(), (b, al[b])
        assert rel(out, ref["xu"]).max() <= 1e-8
        return qp, al
    port = _port_admm((xcur, goals, xu), {}, kw, 1)[0]
    _assert_admm_equal(port, numpy_solves(xcur, goals, xu, N, dict(qp="osqp"), kw)[0])
    return port[1], port[2]


def _steps_without_stop(mode, xcur, goals, xu, **kw):
    """(alphas, step lengths) of the port's run with step_tol = 0."""
    if mode == "direct":
        return cpu.solve(xcur, goals, xu, N, step_tol=0.0, nthreads=4, **kw)[2:4]
    return cpu.solve_admm(xcur, goals, xu, N, cpu.AdmmState(xu.shape[0], N), step_tol=0.0, nthreads=4, **kw)[2:4]


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_port_ragged_termination_matches_numpy(mode):
    """Problems that stop after different numbers of SQP iterations (max_sqp_iters 8, a step_tol
    chosen from the port's own step lengths by settings_cases.choose_step_tol, 118.7): twelve
    problems of seed 61 stop after at least five different counts.  Problem 9 draws alpha = 0 at
    iteration 1 when nothing stops it (asserted on the step_tol = 0 run), but its first step, 19.9,
    is below the chosen tolerance, so under that tolerance it stops before: alpha = 0 at an
    iteration >= 1 of a run that has a step_tol is test_port_alpha_zero_rows_match_numpy's."""
    B = 12
    xcur, goals, xu = synthetic_batch(B, N, 61)
    kw = dict(max_iters=8)
    al0, steps0 = _steps_without_stop(mode, xcur, goals, xu, **kw)
    kw["step_tol"] = choose_step_tol(steps0)
    assert step_gap(steps0, kw["step_tol"]) >= 0.01
    qp, al = _ragged(mode, xcur, goals, xu, np.arange(B), kw)
    assert len(set(qp.tolist())) >= 5, np.bincount(qp)
    assert (al0[:, 1:] == 0.0).any(), al0


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_port_alpha_zero_rows_match_numpy(mode):
    """The 64 problems of seed 41 that tests/test_gpu_settings.py runs ragged (max_sqp_iters 8, the
    step_tol chosen from all 64): the port against numpy on the five problems that draw alpha = 0
    when nothing stops them (22 and 56 at iteration 1 with a first step above the tolerance, so they
    go on under it; 34 at iteration 0; 28 and 29 stop before theirs) and on the first three.  In
    direct mode a problem that draws alpha = 0 at iteration k reports zeros from k to the end."""
    B = 64
    xcur, goals, xu = synthetic_batch(B, N, 41)
    kw = dict(max_iters=8)
    al0, steps0 = _steps_without_stop(mode, xcur, goals, xu, **kw)
    kw["step_tol"] = choose_step_tol(steps0)
    assert step_gap(steps0, kw["step_tol"]) >= 0.01
    rows = np.flatnonzero((al0 == 0.0).any(axis=1))
    assert rows.tolist() == [22, 28, 29, 34, 56]
    qp, al = _ragged(mode, xcur, goals, xu, np.concatenate([[0, 1, 2], rows]), kw)
    late = [b for b in range(len(qp)) if (al[b, 1:] == 0.0).any() and al[b, 0] != 0.0]
    assert len(late) >= 2, al
    if mode == "direct":
        for b in late:
            k = int(np.flatnonzero(al[b] == 0.0)[0])
            assert qp[b] == 8 and (al[b, k:] == 0.0).all(), (b, al[b])


@pytest.fixture(scope="module")
def batch46():
    return synthetic_batch(4, N, 46)


@pytest.fixture(scope="module")
def default46(batch46):
    return cpu.solve_box(*batch46, N)


@pytest.mark.parametrize("name,kw", BOX_CASES, ids=ids(BOX_CASES))
def test_port_box_settings_match_numpy(batch46, default46, name, kw):
    """The box mode's mask (1..6: only some of q, v, u bounded), iteration cap and tolerance: the
    interior point's iterations of every QP, the last QP's converged flag and the alphas equal the
    numpy oracle's, XU to 1e-5; the iteration counts differ from the default's (mask 7, 30
    iterations, 1e-8), and a cap of 4 or 1 ends every QP unconverged at the cap."""
    xcur, goals, xu = batch46
    out, qp, al, _, it, conv, mu = cpu.solve_box(xcur, goals, xu, N, box=cpu.box_cfg(**kw))
    ref = numpy_solves(xcur, goals, xu, N, dict(qp="box", box_mask=kw.get("mask", 7), box_tol=kw.get("tol", 1e-8),
                                                 box_max_iters=kw.get("max_iters", 30)), {})[0]
    np.testing.assert_array_equal(qp, ref["qp_iters"])
    for b in range(len(qp)):
        n = qp[b]
        assert list(it[b, :n]) == [i for i, _ in ref["ipm"][b]], (b, it[b], ref["ipm"][b])
        assert bool(conv[b]) == ref["ipm"][b][-1][1], b
        assert list(al[b, :n]) == ref["alphas"][b], (b, al[b], ref["alphas"][b])
        assert box_relerr(out[b], ref["xu"][b]) <= 1e-5, (b, box_relerr(out[b], ref["xu"][b]))
    assert (mu > 0).all()
    assert (it != default46[4]).any()
    if "max_iters" in kw:
        ran = it >= 0
        assert (conv == 0).all() and (it[ran] == kw["max_iters"]).all(), (conv, it)
    else:
        assert (conv == 1).all()
