"""GPU: i7m_qp_policy, the QP's Riccati feedback gains (csrc/i7m_mpc_policy.h k_policy_gather behind
the unchanged exact sweep), at (N, B) = (4, 5), (32, 130), (64, 16) and (8, 2048): the two-wave sweep
(B <= 128) and the one-wave one, the large-batch DPP / priority variant, the controller's N = 64.

The reference for the gains is tests/policy_ref.py, the backward recursion in np.longdouble on the
oracle's QP blocks, pinned to the exact KKT solve by tests/test_policy_oracle.py.  Its float64 run
against its longdouble run, per stage relative to max |K~_k|, is the reference's own noise floor on
the same problems; the device is gated against a multiple of the largest such error of the case.
The oracle's blocks cost N - 1 numpy linearisations per problem, so the gains are compared on six rows
spread over the batch (first, last and around each quarter); every other check runs on every row.
"""
import ctypes as C

import numpy as np
import pytest

import policy_ref as pr
from oracle.osqp_ref import synthetic_batch

pytestmark = pytest.mark.gpu
CASES = [(4, 5), (32, 130), (64, 16), (8, 2048)]
# the gate on the gains: GATE x the float64 restatement's error.  The device eliminates [H | -G~] by
# Gauss-Jordan with reciprocal + Newton pivots on MFMA sums, another order than the restatement's, on
# an H that carries R = 1e-5 (cond ~ 4e7).
GATE = 16.0
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


def inputs(N, B):
    xc, g, XU = synthetic_batch(B, N, seed=100 + N)
    XU = XU + 0.05 * np.random.default_rng(N).standard_normal(XU.shape)
    XU[:, :12] = xc
    return XU, xc, g


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"N{c[0]}-B{c[1]}")
def case(request, lib, model):
    """One case's inputs, the DIRECT handle's i7m_qp and i7m_qp_policy outputs, and the reference's
    gains on the compared rows: computed once, read by every test."""
    N, B = request.param
    XU, xc, g = inputs(N, B)
    h = lib.Handle(model, N=N, max_batch=B)
    sol = h.qp(XU, xc, g)
    K, psol = h.qp_policy(XU, xc, g, N - 1, want_sol=True)
    K2 = h.qp_policy(XU, xc, g, 2) if N > 3 else None
    h.close()
    rows = sorted({0, 1, B // 4, B // 2, (3 * B) // 4, B - 1})
    ref64, refL = [], []
    for b in rows:
        blk = pr.qp_blocks(XU[b], xc[b], g[b], N)
        ref64.append(pr.riccati_gains(blk))
        refL.append(pr.riccati_gains(blk, np.longdouble))
    return dict(N=N, B=B, XU=XU, xc=xc, g=g, sol=sol, K=K, psol=psol, K2=K2, rows=rows, ref64=np.array(ref64),
                refL=np.array(refL))


def test_minimiser_is_i7m_qps(case):
    """sol_out is the buffer i7m_qp returns, bit for bit: the policy pass is the unchanged exact solve."""
    np.testing.assert_array_equal(case["psol"], case["sol"])
    assert np.isfinite(case["K"]).all() and case["K"].shape == (case["B"], case["N"] - 1, 6, 13)
    if case["K2"] is not None:  # n_k < N - 1: the first stages, the same values
        np.testing.assert_array_equal(case["K2"], case["K"][:, :2])


def test_gains_against_the_longdouble_recursion(case):
    """Per stage, relative to max |K~_k|.  Measured on an MI355X, device error over the
    float64 restatement's: 0.92 at (4, 5), 5.7 at (32, 130), 7.4 at (64, 16), 0.77 at (8, 2048)."""
    floor = pr.stage_rel_err(case["ref64"], case["refL"])
    got = pr.stage_rel_err(case["K"][case["rows"]], case["refL"])
    ratio = got.max() / floor.max()
    print(f"N={case['N']} B={case['B']}: float64 restatement max {floor.max():.3g} (median {np.median(floor):.3g}), "
          f"device max {got.max():.3g} (median {np.median(got):.3g}), at stage {np.unravel_index(got.argmax(), got.shape)}; "
          f"ratio {ratio:.3g}; max |K| {np.abs(case['K'][..., :12]).max():.3g}, max |kff| {np.abs(case['K'][..., 12]).max():.3g}")
    assert floor.max() > 0
    assert got.max() <= GATE * floor.max(), ratio


def test_gains_reproduce_the_controls(case):
    """u_k = K~_k [x_k; 1] on the minimiser, every row and stage.  The rollout forms u from the stored
    gains and the stored x_k (both exact in fp64) as a 13-term dot product in two partial sums, so its
    error against the exact product is at most gamma_13 S <= 13 eps S / (1 - 13 eps) with S = sum_j
    |K~_kj| |x~_j|; the exact product is taken in longdouble, whose own error (13 x 2^-64 S) and
    rounding to float64 (eps/2 |u| <= eps/2 S) are inside the 14 eps S asserted.  Reported relative to
    max(1, |u_k|) as well."""
    N, B, K, sol = case["N"], case["B"], case["K"], case["sol"]
    idx = 18 * np.arange(N - 1)[:, None]
    x = sol[:, idx + np.arange(12)]                       # (B, N-1, 12)
    u = sol[:, idx + 12 + np.arange(6)]                   # (B, N-1, 6)
    xt = np.concatenate([x, np.ones((B, N - 1, 1))], axis=2).astype(np.longdouble)
    KL = K.astype(np.longdouble)
    exact = np.einsum("bkij,bkj->bki", KL, xt)
    S = np.einsum("bkij,bkj->bki", np.abs(KL), np.abs(xt)).astype(np.float64)
    err = np.abs((exact - u.astype(np.longdouble)).astype(np.float64))
    rel = err / np.maximum(1.0, np.abs(u))
    print(f"N={N} B={B}: max |K~ x~ - u| {err.max():.3g}, relative to max(1, |u|) {rel.max():.3g}, "
          f"in units of eps S {np.max(err / (EPS * S)):.3g}; max S {S.max():.3g}, max |u| {np.abs(u).max():.3g}")
    assert (err <= 14 * EPS * S).all()


def test_admm_handle(case, lib, model):
    """On an I7M_QP_ADMM handle: the DIRECT handle's gains bit for bit, the carried OSQP state left as
    it was, and the next solve the one of a twin handle that never asked for the policy."""
    N, B, XU, xc, g = (case[k] for k in ("N", "B", "XU", "xc", "g"))
    h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_ADMM)
    twin = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_ADMM)
    first, _ = h.solve(xc, g, XU)
    first_t, _ = twin.solve(xc, g, XU)
    np.testing.assert_array_equal(first, first_t)
    before = h.admm_state(B)
    K, sol = h.qp_policy(XU, xc, g, N - 1, want_sol=True)
    after = h.admm_state(B)
    np.testing.assert_array_equal(K, case["K"])
    np.testing.assert_array_equal(sol, case["sol"])
    for a, b, name in zip(before, after, ("x", "z", "y", "q", "rho")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    nxt, st = h.solve(xc, g, first)
    nxt_t, st_t = twin.solve(xc, g, first)
    np.testing.assert_array_equal(nxt, nxt_t)
    np.testing.assert_array_equal(h.admm_stats(B)[0], twin.admm_stats(B)[0])
    h.close()
    twin.close()


def test_refusals(lib, model):
    """I7M_EINVAL with a message naming the argument, before any device work."""
    N, B = 8, 4
    XU, xc, g = inputs(N, B)
    with pytest.raises(lib.I7MError, match="i7m_qp_policy: I7M_QP_BOX"):
        lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_BOX).qp_policy(XU, xc, g, 2)
    h = lib.Handle(model, N=N, max_batch=B)
    for bad in (0, N, -1):
        with pytest.raises(lib.I7MError, match=rf"n_k = {bad} outside \[1, N - 1 = 7\]"):
            h.qp_policy(XU, xc, g, bad)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert h._lib.i7m_qp_policy(h._h, B, dp(XU), dp(xc), dp(g), 3, 2, None, None) == -1
    assert b"i7m_qp_policy: null K_out" in h._lib.i7m_last_error()
    Kb = np.empty((B, 2, 6, 13))
    assert h._lib.i7m_qp_policy(h._h, B, None, dp(xc), dp(g), 3, 2, dp(Kb), None) == -1
    assert b"null xu" in h._lib.i7m_last_error()
    assert h._lib.i7m_qp_policy(h._h, B + 1, dp(XU), dp(xc), dp(g), 3, 2, dp(Kb), None) == -1
    assert b"max_batch" in h._lib.i7m_last_error()
    h.ctrl_begin(np.tile(g[0, :3], (4, 1)), np.zeros((4, 6)), x0=xc[:1])
    with pytest.raises(lib.I7MError, match="controller session open"):
        h.qp_policy(XU, xc, g, 2)
    h.ctrl_end()
    K = h.qp_policy(XU, xc, g, 2)  # and it still works afterwards
    assert np.isfinite(K).all()
    h.close()
