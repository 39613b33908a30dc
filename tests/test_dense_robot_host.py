"""CPU: the dense second robot (tests/golden/dense6.json, tests/dense_robot.py) is what it claims to
be, and the references agree with each other on it, before any GPU kernel is compared with them.

  validity       every property that makes the robot "dense" (no zero, no two numbers of a block
                 alike, no symmetric limit), asserted on the committed file, and the committed file
                 is what the seeded generator writes
  observability  every model number the dynamics kernels read moves a checked output
  references     the C++ port against the numpy oracle on the dense robot, in all three QP modes
  identities     rnea(aba) = tau, Minv M = I, J = d eepos / dq by complex step: a third opinion
                 should GPU and oracle ever disagree

Reference against reference, measured here (max over the problems of both shapes, the quantity
each test asserts and prints; every alpha sequence identical, alphas seen 0.5, 0.25, 0.125 and,
at N = 8, 0.0625):

  direct  (N, B) = (8, 6) 4.6e-13, (16, 6) 9.2e-14   relative 2-norm of XU, bound 1e-6
  ADMM    (8, 6) 8.8e-10, (16, 6) 7.0e-10            relative 2-norm of XU, bound 5e-8
          OSQP iterations per QP identical (25 or 50), both calls
  box     (8, 6) 2.3e-7, (16, 6) 3.3e-8              max |d XU| / max(1, |XU|), bound 1e-5
          interior-point iterations identical (5 to 7), every QP converged

Observability, measured: exactly the six exempt numbers move nothing; the weakest observed one,
mass[0], moves an output by 7.5e-4 (bound 1e-7).
"""
import copy
import json

import numpy as np
import pytest

import dense_robot as dr
from dense_robot import dense_oracle  # noqa: F401  (fixture)
from oracle import cpu, rbd
from oracle.osqp_ref import OSQPSolverRef, SQPRef, synthetic_batch

SHAPES = [(8, 6, 5), (16, 6, 7)]  # N, B, seed


@pytest.fixture(scope="module")
def raw():
    with open(dr.PATH) as f:
        return json.load(f)


# ---- validity ------------------------------------------------------------------------------------
def test_committed_file_is_the_generators(raw):
    """Same keys as the Indy7 block, and bit for bit what generate() writes."""
    from indy7_mpc_amd.model import load_params
    assert set(raw) == set(load_params())
    assert raw == json.loads(json.dumps(dr.generate()))
    packed = dr.dense_model().packed()
    assert packed.shape == (159,) and np.abs(packed).min() > 0  # i7m_model: no zero anywhere
    np.testing.assert_array_equal(packed[-27:-24], dr.GRAVITY)


def test_rotations_are_proper_and_dense(raw):
    for R in np.array(raw["placement_R"]):
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
        assert abs(np.linalg.det(R) - 1.0) <= 1e-15
        assert np.abs(R).min() >= 0.05 and np.abs(R).max() <= 0.99
        assert dr.distinct(R)


def test_vectors_have_no_zero_and_no_coincidence(raw):
    for key in ("placement_t", "com"):
        for x in np.array(raw[key]):
            assert np.abs(x).min() >= 1e-3 and dr.distinct(x), (key, x)
    g = np.array(raw["gravity"])
    assert np.abs(g).min() >= 1e-3 and dr.distinct(g)
    assert np.abs(g - [1.3, -0.8, -9.6]).max() <= 0.1


def test_inertias_are_physical_and_dense(raw):
    for I in np.array(raw["inertia_com"]):
        np.testing.assert_array_equal(I, I.T)
        w = np.linalg.eigvalsh(I)
        assert w[0] > 0 and w[0] + w[1] > w[2]  # positive definite, principal moments of a real body
        e = dr.sym6(I)
        assert np.abs(e).min() > 0 and dr.distinct(e)  # the six numbers the kernels read
    m = np.array(raw["mass"])
    assert (m > 0).all() and (np.diff(m) < 0).all()


def test_limits_are_asymmetric_and_differ_per_joint(raw):
    lo, hi = np.array(raw["q_lower"]), np.array(raw["q_upper"])
    assert (lo < 0).all() and (hi > 0).all() and (hi - lo >= 3.0).all()
    assert (np.abs(lo + hi) > 0.1).all()                       # q_lower != -q_upper
    assert len(set(np.round(np.concatenate([lo, -lo, hi, -hi]), 6))) == 24  # no bound like another, nor its mirror
    for key in ("v_limit", "effort_limit"):
        x = np.array(raw[key])
        assert (x > 0).all() and len(set(x)) == 6, key


# ---- observability -------------------------------------------------------------------------------
def _outputs(P, states):
    out = []
    for q, v, tau, fw in states:
        p, J = rbd.d_eepos(q, P)
        dq, dv, Mi, a = rbd.aba_derivatives(q, v, tau, P)
        aw = rbd.aba(q, v, tau, P, rbd.fext_list(q, fw, "world", P))
        out.append(np.concatenate([p, J.ravel(), dq.ravel(), dv.ravel(), Mi.ravel(), a, aw]))
    return np.array(out)


def _model_numbers():
    """(name, setter) of the 135 numbers the dynamics read: 54 rotation entries, 18 translations,
    6 masses, 18 centre-of-mass entries, 36 inertia entries (6 per link, both mirror images moved
    together), 3 of gravity.  (The limits enter only the box rows: tests/test_gpu_dense_robot.py.)"""
    out = []
    for j in range(6):
        for r in range(3):
            for c in range(3):
                out.append((f"placement_R[{j}][{r}][{c}]", lambda P, d, j=j, r=r, c=c: P.Rp[j].__setitem__((r, c), P.Rp[j][r, c] + d)))
            out.append((f"placement_t[{j}][{r}]", lambda P, d, j=j, r=r: P.tp[j].__setitem__(r, P.tp[j][r] + d)))
            out.append((f"com[{j}][{r}]", lambda P, d, j=j, r=r: P.com[j].__setitem__(r, P.com[j][r] + d)))
        out.append((f"mass[{j}]", lambda P, d, j=j: P.mass.__setitem__(j, P.mass[j] + d)))
        for name, (r, c) in zip(("Ixx", "Ixy", "Ixz", "Iyy", "Iyz", "Izz"), ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            def set_inertia(P, d, j=j, r=r, c=c):
                P.Ic[j][r, c] += d
                if r != c:
                    P.Ic[j][c, r] += d
            out.append((f"{name}[{j}]", set_inertia))
    for r in range(3):
        out.append((f"gravity[{r}]", lambda P, d, r=r: P.gravity.__setitem__(r, P.gravity[r] + d)))
    return out


# structurally unobservable on a fixed base: link 0 only turns about its own z axis, so of its
# inertia only Izz and of its centre of mass only x and y (through gravity and Izz's parallel axis) act
EXEMPT = {"com[0][2]", "Ixx[0]", "Ixy[0]", "Ixz[0]", "Iyy[0]", "Iyz[0]"}


def test_every_model_number_moves_a_checked_output():
    """Six states (q in U(-3, 3), v in U(-2, 2), tau in U(-50, 50), a world wrench from N(0, 10));
    the outputs the GPU tests check: eepos, J, da/dq, da/dv, Minv, a, and a under the world wrench.
    Each model number, changed by 1e-3, moves at least one of them by more than 1e-7 (scaled by
    max(1, |output|)) — so a kernel that reads the wrong number, or none, for it cannot pass.  The
    six exempt numbers are exactly the ones that move nothing."""
    rng = np.random.default_rng(11)
    states = [(rng.uniform(-3, 3, 6), rng.uniform(-2, 2, 6), rng.uniform(-50, 50, 6), rng.normal(0, 10, 6))
              for _ in range(6)]
    P = dr.dense_params()
    base = _outputs(P, states)
    numbers = _model_numbers()
    assert len(numbers) == 135
    unobserved, weakest = set(), (np.inf, None)
    for name, change in numbers:
        Pc = copy.deepcopy(P)
        change(Pc, 1e-3)
        moved = (np.abs(_outputs(Pc, states) - base) / np.maximum(1.0, np.abs(base))).max()
        if not moved > 1e-7:
            unobserved.add(name)
        elif moved < weakest[0]:
            weakest = (moved, name)
    print(f"weakest observed number: {weakest[1]} moves an output by {weakest[0]:.3g}; unobserved: {sorted(unobserved)}")
    assert unobserved == EXEMPT, sorted(unobserved ^ EXEMPT)


# ---- reference against reference -----------------------------------------------------------------
def _numpy_sqp(s, xcur, goals, XU):
    sq = SQPRef(s)
    ref = sq.sqp(xcur, goals, XU.copy())
    return ref, sq.stats["linesearch_alphas"]["values"], sq.stats["qp_iters"]["values"][0]


@pytest.mark.parametrize("N,B,seed", SHAPES)
def test_port_direct_matches_numpy_oracle_on_the_dense_robot(dense_oracle, N, B, seed):
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    out, qp, al, _ = cpu.solve(xcur, goals, XU, N)
    worst, seen = 0.0, set()
    for b in range(B):
        ref, alphas, iters = _numpy_sqp(OSQPSolverRef(N=N, P=dense_oracle), xcur[b], goals[b], XU[b])
        assert qp[b] == iters
        np.testing.assert_array_equal(al[b, :qp[b]], alphas)
        seen |= set(alphas)
        worst = max(worst, np.linalg.norm(out[b] - ref) / np.linalg.norm(ref))
    print(f"direct N={N} B={B}: XU {worst:.3g} relative, alphas seen {sorted(seen)}")
    assert worst < 1e-6
    assert len(seen) >= 3


@pytest.mark.parametrize("N,B,seed", SHAPES)
def test_port_admm_matches_numpy_osqp_on_the_dense_robot(dense_oracle, N, B, seed):
    """Two consecutive solves, the OSQP state carried."""
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    st = cpu.AdmmState(B, N)
    out, qp, al, _, it = cpu.solve_admm(xcur, goals, XU, N, st)
    out2, qp2, al2, _, it2 = cpu.solve_admm(xcur, goals, out, N, st)
    worst = 0.0
    for b in range(B):
        s = OSQPSolverRef(N=N, qp="osqp", P=dense_oracle)
        sq = SQPRef(s)
        x = sq.sqp(xcur[b], goals[b], XU[b].copy())
        its = [h[0] for h in s.osqp.history]
        assert its == list(it[b, :qp[b]]), (b, its, it[b])
        np.testing.assert_array_equal(sq.stats["linesearch_alphas"]["values"], al[b, :qp[b]])
        x2 = sq.sqp(xcur[b], goals[b], x.copy())
        assert [h[0] for h in s.osqp.history][len(its):] == list(it2[b, :qp2[b]])
        np.testing.assert_array_equal(sq.stats["linesearch_alphas"]["values"][qp[b]:], al2[b, :qp2[b]])
        worst = max(worst, np.linalg.norm(x - out[b]) / np.linalg.norm(x), np.linalg.norm(x2 - out2[b]) / np.linalg.norm(x2))
    print(f"admm N={N} B={B}: XU {worst:.3g} relative, OSQP iterations {sorted(set(it[it > 0]) | set(it2[it2 > 0]))}")
    assert worst < 5e-8


@pytest.mark.parametrize("N,B,seed", SHAPES)
def test_port_box_matches_numpy_oracle_on_the_dense_robot(dense_oracle, N, B, seed):
    xcur, goals, XU = synthetic_batch(B, N, seed, P=dense_oracle)
    out, qp, al, _, it, conv, mu = cpu.solve_box(xcur, goals, XU, N)
    s = OSQPSolverRef(N=N, qp="box", P=dense_oracle)
    orig = s.setup_and_solve_qp
    worst, seen = 0.0, set()
    for b in range(B):
        its = []

        def rec(*a):
            r = orig(*a)
            its.append((s.last_ipm.iters, s.last_ipm.converged))
            return r

        s.setup_and_solve_qp = rec
        ref, alphas, iters = _numpy_sqp(s, xcur[b], goals[b], XU[b])
        s.setup_and_solve_qp = orig
        assert qp[b] == len(its) == iters
        assert list(it[b, :qp[b]]) == [i for i, _ in its], (b, it[b], its)
        assert all(c for _, c in its) and conv[b]
        seen |= {i for i, _ in its}
        np.testing.assert_array_equal(al[b, :qp[b]], alphas)
        worst = max(worst, np.abs(out[b] - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"box N={N} B={B}: XU {worst:.3g}, interior-point iterations {sorted(seen)}")
    assert worst <= 1e-5


# ---- physical identities -------------------------------------------------------------------------
def _close(got, ref, tol=1e-10):
    assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


def test_physical_identities_on_the_dense_robot():
    """Three algorithms of the oracle that share no code path beyond the joint transforms (RNEA,
    the articulated-body ABA, forward kinematics) agree with each other on the dense robot."""
    P = dr.dense_params()
    rng = np.random.default_rng(12)
    for _ in range(8):
        q, v, tau = rng.uniform(-3, 3, 6), rng.uniform(-2, 2, 6), rng.uniform(-50, 50, 6)
        # inverse of forward dynamics
        _close(rbd.rnea(q, v, rbd.aba(q, v, tau, P), P), tau)
        f = rng.normal(0, 10, 6)
        fl = rbd.fext_list(q, f, "world", P)
        _close(rbd.rnea(q, v, rbd.aba(q, v, tau, P, fl), P, fext=fl), tau)
        # Minv M = I, Minv column by column from ABA (a(tau + e_j) - a(tau)), M from RNEA columns
        a0 = rbd.aba(q, v, tau, P)
        Minv = np.stack([rbd.aba(q, v, tau + e, P) - a0 for e in np.eye(6)], axis=1)
        M = rbd.crba(q, P)
        _close(Minv @ M, np.eye(6))
        _close(rbd.aba_derivatives(q, v, tau, P)[2] @ M, np.eye(6))
        # the Jacobian is the derivative of the position
        p, J = rbd.d_eepos(q, P)
        Jc = np.stack([np.imag(rbd.eepos(q + 1j * rbd.H_CS * e, P)) / rbd.H_CS for e in np.eye(6)], axis=1)
        _close(J, Jc)
        _close(p, rbd.eepos(q, P))
