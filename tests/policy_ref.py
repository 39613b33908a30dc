"""Helper (not collected): the backward Riccati recursion of the SQP subproblem QP restated in numpy,
on the blocks of oracle.osqp_ref.OSQPSolverRef.matrices() — the reference for i7m_qp_policy's gains.

The QP is  min 1/2 z' P z + g' z  s.t.  A z = l  over z = XU = [x_0 u_0 x_1 u_1 ... x_{N-1}]
(src/osqp_solver.py:83-143): row block 0 of A is -x_0 = -xs, row block k + 1 is
A_k x_k + B_k u_k - x_{k+1} = -c_k.  In homogeneous coordinates x~ = [x; 1]:
    A~ = [[A, c], [0, 1]],  B~ = [B; 0],  Q~ = [[Q, q], [q', 0]],  N~ = [0 | r]
    H = B~' V~ B~ + R,  G~ = B~' V~ A~ + N~,  K~ = -H^-1 G~ (6 x 13: [K | kff]),
    V~ <- A~' V~ A~ + Q~ + K~' G~,   V~_{N-1} = Q~_{N-1}
and the minimiser is u_k = K~_k [x_k; 1].  Every operation runs in the dtype asked for (float64 or
np.longdouble); the 6 x 6 solve is a Gauss-Jordan elimination with partial pivoting written out
here, because numpy's LAPACK calls have no extended-precision form.
"""
import numpy as np
from scipy.sparse import diags

from oracle.osqp_ref import OSQPSolverRef

NX, NU = 12, 6


def qp_blocks(xu, xs, goals, N, dt=0.01):
    """The stage blocks of the QP linearised at xu with x_0 row xs: dict of float64 arrays A (N-1, 12,
    12), B (N-1, 12, 6), c (N-1, 12), Q (N, 12, 12), q (N, 12), R (N-1, 6, 6), r (N-1, 6), and the
    solver (its l[:12] may be changed and solve_qp_exact() called again)."""
    s = OSQPSolverRef(N=N, dt=dt)
    s.update_constraint_matrix(np.asarray(xu, float), np.asarray(xs, float))
    s.update_cost_matrix(np.asarray(xu, float), np.asarray(goals, float).reshape(3 * N))
    P, Am = s.matrices()
    Pf = (P + P.T - diags(P.diagonal())).toarray()
    Ad = Am.toarray()
    out = dict(A=np.zeros((N - 1, NX, NX)), B=np.zeros((N - 1, NX, NU)), c=np.zeros((N - 1, NX)), Q=np.zeros((N, NX, NX)),
               q=np.zeros((N, NX)), R=np.zeros((N - 1, NU, NU)), r=np.zeros((N - 1, NU)), solver=s)
    for k in range(N):
        o = 18 * k
        out["Q"][k] = Pf[o:o + NX, o:o + NX]
        out["q"][k] = s.g[o:o + NX]
        if k < N - 1:
            rows = slice(NX * (k + 1), NX * (k + 2))
            out["A"][k] = Ad[rows, o:o + NX]
            out["B"][k] = Ad[rows, o + NX:o + 18]
            out["c"][k] = -s.l[rows]
            out["R"][k] = Pf[o + NX:o + 18, o + NX:o + 18]
            out["r"][k] = s.g[o + NX:o + 18]
            assert not Pf[o:o + NX, o + NX:o + 18].any()  # no state-control cross term
    return out


def _solve(H, G):
    """H^-1 G by Gauss-Jordan with partial pivoting, in H's dtype."""
    n = H.shape[0]
    M = np.concatenate([H.copy(), G.copy()], axis=1)
    for p in range(n):
        i = p + int(np.argmax(np.abs(M[p:, p])))
        if i != p:
            M[[p, i]] = M[[i, p]]
        M[p] = M[p] / M[p, p]
        for r in range(n):
            if r != p:
                M[r] = M[r] - M[r, p] * M[p]
    return M[:, n:]


def riccati_gains(blk, dtype=np.float64):
    """K~ (N-1, 6, 13) of every stage, the recursion run in `dtype`."""
    A, B, c, Q, q, R, r = (blk[k].astype(dtype) for k in ("A", "B", "c", "Q", "q", "R", "r"))
    N = Q.shape[0]
    one = dtype(1)

    def hom_q(k):
        Qt = np.zeros((13, 13), dtype=dtype)
        Qt[:12, :12] = Q[k]
        Qt[:12, 12] = q[k]
        Qt[12, :12] = q[k]
        return Qt

    V = hom_q(N - 1)
    K = np.zeros((N - 1, NU, 13), dtype=dtype)
    for k in range(N - 2, -1, -1):
        At = np.zeros((13, 13), dtype=dtype)
        At[:12, :12] = A[k]
        At[:12, 12] = c[k]
        At[12, 12] = one
        Bt = np.zeros((13, NU), dtype=dtype)
        Bt[:12] = B[k]
        Nt = np.zeros((NU, 13), dtype=dtype)
        Nt[:, 12] = r[k]
        W0 = V @ At
        H = Bt.T @ (V @ Bt) + R[k]
        G = Bt.T @ W0 + Nt
        K[k] = -_solve(H, G)
        V = At.T @ W0 + hom_q(k) + K[k].T @ G
    return K


def closed_loop_maps(blk, K):
    """Phi_k = prod_{j < k} (A_j + B_j K_j) (N-1, 12, 12), Phi_0 = I: dx_k / dx_0 under the policy."""
    n = K.shape[0]
    Phi = np.zeros((n, NX, NX), dtype=K.dtype)
    Phi[0] = np.eye(NX)
    for k in range(1, n):
        Phi[k] = (blk["A"][k - 1].astype(K.dtype) + blk["B"][k - 1].astype(K.dtype) @ K[k - 1][:, :12]) @ Phi[k - 1]
    return Phi


def stage_rel_err(K, Kref):
    """max |K_k - Kref_k| / max |Kref_k| per stage: (..., n_k)."""
    K, Kref = np.asarray(K, np.longdouble), np.asarray(Kref, np.longdouble)
    num = np.abs(K - Kref).max(axis=(-1, -2))
    den = np.abs(Kref).max(axis=(-1, -2))
    return (num / den).astype(np.float64)
