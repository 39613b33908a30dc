"""GPU: every numeric setting of i7m_config off its default, against the C++ port (ADMM mode; the
port is pinned to the numpy restatement at the same settings by tests/test_settings_oracle.py) and
against the numpy oracle (direct and box mode).  Each setting reaches a kernel as a runtime
argument with a code path of its own: a kernel that ignored one, baked in its default, or
mishandled the rows of a wave that have stopped while their neighbours iterate on would pass the
rest of the suite, which runs the defaults.  The cases are tests/settings_cases.py's.

Small shapes: N = 16 with B = 13 (the last four-problem wave of the ADMM iteration kernels has
empty rows) or B = 64, and one N = 5 case.

Tolerances:
  every discrete outcome (SQP iterations, OSQP / interior-point iterations, statuses, alphas,
  converged flags)                                   : identical
  ADMM mode vs the port, XU and the carried state    : 5e-8 relative (tests/test_gpu_admm.py).  The
      carried x, z, y are the last QP's iterate, of which XU takes only the fraction alpha, so they
      carry the x-update's rounding in full.  Two cases read above 5e-8 there (5.2e-8 and 9.5e-8 on
      x); for these the port was measured against the numpy restatement on the same inputs on the
      CPU, the two references are themselves 4.5e-8 and 6.9e-8 apart, and the state's bound is
      10 x that spread (STATE_TOL, and the ragged case's docstring).  XU's bound stays 5e-8
      everywhere (largest reading 1.7e-8)
  rho under adaptation                               : rtol 1e-6, else identical
  direct mode vs numpy (and vs the port)             : 1e-6 relative (tests/test_gpu_edges.py)
  box mode vs its oracle                             : 1e-5 SQP, 1e-6 QP (tests/test_gpu_box.py)
  closed loop                                        : tests/test_gpu_mpc.py's: 2e-6 absolute in
      direct mode, 1e-8 in ADMM mode
A step_tol that stops problems early is chosen from the port's own step lengths, 1 % away from
every one of them (settings_cases.choose_step_tol), so the device's rounding cannot flip a stop.
"""
import functools

import numpy as np
import pytest

from oracle import box_ipm, cpu, rbd
from oracle.mpc_ref import run_mpc_ref
from oracle.osqp_ref import OSQPSolverRef, SQPRef, synthetic_batch
from settings_cases import (BOX_CASES, OSQP_CASES, SQP_CASES, box_relerr, choose_step_tol, handle_kw, ids, numpy_solves,
                            rel, step_gap)

pytestmark = pytest.mark.gpu
N = 16
# Carried-state bounds above 5e-8: 10 x the largest relative difference between the port's and the
# numpy restatement's x, z, y over the case's two solves of these 13 problems (CPU, measured 3.5e-8
# on x after the first solve, 4.5e-8 on z after the second; the default settings read 6.8e-9 and
# 1.3e-8: rho = 1 makes the equality rows' rho 1e3 and the reduced system ten times stiffer).
STATE_TOL = {"sigma_alpha_rho": 4.5e-7}
STAT_KEYS = ("qp_iters", "n_alphas", "alphas", "n_steps", "stepsizes")


@pytest.fixture(scope="module")
def lib():
    from indy7_mpc_amd import _lib
    _lib.load()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible but the gpu tests were requested")
    return _lib


@functools.lru_cache(maxsize=None)
def _batch(B, n, seed):
    return synthetic_batch(B, n, seed)


def _ran(qp):
    return np.arange(8)[None, :] < np.asarray(qp)[:, None]


def _alphas_equal(s, al, qp):
    """The device's alpha record (stats) against the port's (B, 8) NaN-padded one."""
    np.testing.assert_array_equal(s["n_alphas"], qp)
    ran = _ran(qp)
    assert np.array_equal(ran, ~np.isnan(al))
    np.testing.assert_array_equal(s["alphas"][ran], al[ran])


def _admm_solves_vs_port(lib, model, batch, n, admm_kw, sqp_kw, calls=2, state_tol=5e-8):
    """`calls` consecutive ADMM solves on a fresh handle and on the port (each from the previous
    one's output and OSQP state), compared after every call: SQP iterations, OSQP iterations and
    status per QP (-1 for the SQP iterations that were not run), alphas, XU, the carried state.
    Returns the port's (qp_iters, its, status, rho, alphas, steps) per call."""
    xcur, goals, xin = batch
    B = xin.shape[0]
    h = lib.Handle(model, N=n, max_batch=B, qp_mode=lib.QP_ADMM, admm=admm_kw or None, **handle_kw(sqp_kw))
    st = cpu.AdmmState(B, n, rho=admm_kw.get("rho", 0.1))
    adaptive = admm_kw.get("adaptive_rho_interval", 0) > 0
    port = []
    for call in range(calls):
        out, s = h.solve(xcur, goals, xin)
        it, rho, stat = h.admm_stats(B, with_status=True)
        ref, qp, al, steps, it_r = cpu.solve_admm(xcur, goals, xin, n, st, admm=cpu.admm_cfg(**admm_kw), **sqp_kw)
        port.append((qp, it_r, st.status.copy(), st.rho.copy(), al, steps))
        np.testing.assert_array_equal(s["qp_iters"], qp, err_msg=f"call {call}")
        ran = _ran(qp)
        assert (it_r[~ran] == -1).all() and (st.status[~ran] == -1).all()
        np.testing.assert_array_equal(it, it_r, err_msg=f"call {call}")
        np.testing.assert_array_equal(stat, st.status, err_msg=f"call {call}")
        _alphas_equal(s, al, qp)
        x, z, y, q, r = h.admm_state(B)
        errs = {"XU": rel(out, ref).max(), "x": rel(x, st.x).max(), "z": rel(z, st.z).max(), "y": rel(y, st.y).max(),
                "q": rel(q, st.q).max()}
        print(f"call {call}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        np.testing.assert_allclose(r, st.rho, rtol=1e-6 if adaptive else 0, atol=0)
        for k, v in errs.items():
            assert v < (5e-8 if k == "XU" else state_tol), (call, k, v)
        xin = out
    h.close()
    return port


@functools.lru_cache(maxsize=None)
def _default_port_its(B, n, seed):
    """OSQP iterations per QP of the port's two default-settings solves of a batch."""
    xcur, goals, xin = _batch(B, n, seed)
    st = cpu.AdmmState(B, n)
    its = []
    for _ in range(2):
        xin, _, _, _, it = cpu.solve_admm(xcur, goals, xin, n, st)
        its.append(it)
    return its


@pytest.mark.parametrize("name,kw", OSQP_CASES, ids=ids(OSQP_CASES))
def test_admm_osqp_settings_match_port(lib, model, name, kw):
    """One group of OSQP settings off its default (sigma / alpha / rho, the scaling passes, the
    check interval 1, 7 and 0 = never, no duality-gap test, eps_abs != eps_rel, rho adaptation at
    an interval that is no multiple of the check interval), 13 problems, two consecutive solves.
    Each setting is seen to act: the port's OSQP iteration counts differ from its default run's on
    these problems (so a device that ignored the setting would not meet them); check_termination 0
    runs max_iter = 60 iterations and is "solved" by the closing test; the adaptive case moves
    rho."""
    B = 13
    port = _admm_solves_vs_port(lib, model, _batch(B, N, 41), N, kw, {}, state_tol=STATE_TOL.get(name, 5e-8))
    assert any((p[1] != d).any() for p, d in zip(port, _default_port_its(B, N, 41)))
    if name == "check0":
        ran = _ran(port[0][0])
        assert (port[0][1][ran] == 60).all() and (port[0][2][ran] == 1).all()
    if name == "adapt":
        assert (port[1][3] != kw["rho"]).sum() >= B // 2, port[1][3]


@pytest.mark.parametrize("name,kw,n", [c + (N,) for c in SQP_CASES] + [("sqp5", dict(max_iters=5), 5)],
                         ids=ids(SQP_CASES) + ["sqp5-N5"])
def test_admm_sqp_settings_match_port(lib, model, name, kw, n):
    """max_sqp_iters 1, 5 and 8, and mu 1 and 1000 with four iterations, in ADMM mode: 13 problems,
    two consecutive solves; the OSQP records of the SQP iterations that were not run are -1
    (_admm_solves_vs_port).  Every problem runs max_sqp_iters QPs (the default step_tol stops
    nothing here), and mu moves the line search: the port's alphas differ from mu = 10's.
    XU and state meet 5e-8 (largest readings: XU 6.7e-9, x 2.2e-8, both max_sqp_iters 8).  Every SQP
    iteration amplifies the x-update's rounding: on these inputs the port and the numpy restatement
    are themselves 1.7e-8 (5 iterations) and 2.4e-8 (8) apart on XU and 3.2e-7 / 2.8e-7 on the
    carried x (CPU), and a build whose iteration kernels differed only in instruction selection
    read 7.5e-8 on XU at 8 iterations.  Should a value-neutral kernel change pass 5e-8 here, the
    bound that spread supports is 10 x it: 2.4e-7 on XU, 3.2e-6 on the state."""
    B = 13
    batch = _batch(B, n, 41)
    port = _admm_solves_vs_port(lib, model, batch, n, {}, kw)
    assert (port[0][0] == kw["max_iters"]).all(), port[0][0]
    if "mu" in kw:
        al10 = cpu.solve_admm(*batch, n, cpu.AdmmState(B, n), max_iters=kw["max_iters"])[2]
        assert not np.array_equal(port[0][4], al10, equal_nan=True)


def _admm_results(lib, model, batch, sqp_kw, device):
    """Two consecutive ADMM solves on a fresh handle through i7m_solve or i7m_solve_device: the
    outputs, stats, carried state, OSQP records with statuses, and duals."""
    xcur, goals, xu = batch
    B = xu.shape[0]
    h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_ADMM, **handle_kw(sqp_kw))
    outs = []
    if device:
        import torch
        dev = torch.device("cuda", 0)
        t_xu, t_xs, t_g = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (xu, xcur, goals))
        for call in range(2):
            t_out = torch.empty_like(t_xu)
            torch.cuda.synchronize()
            h.solve_device(B, t_xu.data_ptr(), t_xs.data_ptr(), t_g.data_ptr(), 3, t_out.data_ptr())
            h.synchronize()
            outs.append(t_out.cpu().numpy())
            t_xu = t_out
    else:
        xin = xu
        for call in range(2):
            xin, s = h.solve(xcur, goals, xin)
            outs += [xin] + [s[k] for k in STAT_KEYS]
    res = tuple(outs) + h.admm_state(B) + h.admm_stats(B, with_status=True) + (h.admm_dual(B),)
    h.close()
    return res


def test_admm_ragged_termination_matches_port_and_staggered_ranges(lib, model, monkeypatch):
    """64 problems that stop after every count from 1 to 8 SQP iterations (max_sqp_iters 8, a
    step_tol chosen from the port's step lengths; three problems draw alpha = 0, two of them at
    iteration 1, and go on with OSQP's warm start): the waves of the iteration kernels hold rows
    that have stopped next to rows that run, with another idle set at every launch.  Two consecutive
    solves against the port (the second is ragged too, and leaves the first's records of later
    iterations stale where it stops earlier: they must read -1), with the automatic kernel choice;
    then with the staggered ranges forced at this size (I7M_ADMM_STAGGER_MIN_B = 2), through
    i7m_solve (two chunks) and i7m_solve_device (two ranges): bit for bit the automatic run's.
    XU to 5e-8.  The carried state to 6.9e-7: after up to eight SQP iterations the port's and the
    numpy restatement's x are 6.9e-8 apart on these 64 problems (5.2e-8 after the second solve, y
    3.4e-8, z 1.8e-8; CPU), and the bound is 10 x that spread."""
    B = 64
    batch = _batch(B, N, 41)
    steps0 = cpu.solve_admm(*batch, N, cpu.AdmmState(B, N), max_iters=8, step_tol=0.0)[3]
    kw = dict(max_iters=8, step_tol=choose_step_tol(steps0))
    assert step_gap(steps0, kw["step_tol"]) >= 0.01
    port = _admm_solves_vs_port(lib, model, batch, N, {}, kw, state_tol=6.9e-7)
    for qp, _, _, _, al, steps in port:
        assert step_gap(steps, kw["step_tol"]) >= 0.01  # also in the second solve, whose inputs the first made
        assert len(set(qp.tolist())) >= 5, np.bincount(qp)
    assert sorted(set(port[0][0].tolist())) == list(range(1, 9))
    al = port[0][4]
    assert ((al[:, 1] == 0.0) & (al[:, 0] != 0.0)).sum() >= 2
    stale = port[1][0] < port[0][0]
    assert stale.sum() >= B // 4
    res = {}
    for device in (False, True):
        monkeypatch.delenv("I7M_ADMM_STAGGER_MIN_B", raising=False)
        monkeypatch.delenv("I7M_ADMM_STAGGER", raising=False)
        res["auto"] = _admm_results(lib, model, batch, kw, device)
        monkeypatch.setenv("I7M_ADMM_STAGGER_MIN_B", "2")
        monkeypatch.setenv("I7M_ADMM_STAGGER", "1")
        res["stagger"] = _admm_results(lib, model, batch, kw, device)
        for i, (a, b) in enumerate(zip(res["auto"], res["stagger"])):
            np.testing.assert_array_equal(a, b, err_msg=f"device {device} item {i}")
        if not device:
            np.testing.assert_array_equal(res["auto"][1], port[0][0])  # the run the port was compared with


# ---- direct mode ---------------------------------------------------------------------------------

DIRECT_CASES = [
    ("sqp1", dict(max_iters=1), {}),
    ("sqp5", dict(max_iters=5, step_tol="chosen"), {}),
    ("sqp8", dict(max_iters=8, step_tol="chosen"), {}),
    ("mu1", dict(mu=1.0, max_iters=4), {}),
    ("mu1000", dict(mu=1000.0, max_iters=4), {}),
    ("eps0.1", {}, dict(eps=0.1, regularize=True)),
    ("eps10", {}, dict(eps=10.0, regularize=True)),
]


def _with_chosen_step_tol(batch, sqp_kw, solver_kw=None):
    """sqp_kw with step_tol "chosen" replaced by choose_step_tol of the port's direct-mode run."""
    kw = dict(sqp_kw)
    if kw.get("step_tol") == "chosen":
        kw["step_tol"] = 0.0
        steps0 = cpu.solve(*batch, N, nthreads=4, **kw, **(solver_kw or {}))[3]
        kw["step_tol"] = choose_step_tol(steps0)
        assert step_gap(steps0, kw["step_tol"]) >= 0.01
    return kw


def _tail_fill(s, max_iters):
    """Direct mode repeats an alpha = 0 to the end (the exact QP solve is deterministic, so
    src/osqp_sqp.py:81-82's `continue` re-solves the same QP): a problem whose alpha is 0 at
    iteration k reports n_alphas = qp_iters = max_sqp_iters and zeros from k on.  Returns the
    first-zero iteration of every such problem."""
    first = []
    for b in range(len(s)):
        a = s["alphas"][b][:s["n_alphas"][b]]
        z = np.flatnonzero(a == 0.0)
        if z.size:
            k = int(z[0])
            assert s["n_alphas"][b] == max_iters and s["qp_iters"][b] == max_iters and (a[k:] == 0.0).all(), (b, a)
            first.append(k)
    return first


def _direct_pipelines(lib, model, batch, hkw):
    """One solve of the batch under every way the direct mode runs: the three-kernel path, the
    fused kernel, the fused kernel launched per SQP iteration, and i7m_solve in three chunks.  All
    equal the three-kernel path bit for bit (include/indy7_mpc.h i7m_config.pipeline)."""
    xcur, goals, xu = batch
    B = xu.shape[0]
    runs = {}
    for name, kw in (("split", dict(pipeline=lib.PIPE_SPLIT)), ("fused", dict(pipeline=lib.PIPE_FUSED)),
                     ("fused_iter", dict(pipeline=lib.PIPE_FUSED_ITER)), ("chunks3", dict(h2h_chunks=3))):
        h = lib.Handle(model, N=N, max_batch=B, **kw, **hkw)
        runs[name] = h.solve(xcur, goals, xu)
        h.close()
    for name in ("fused", "fused_iter", "chunks3"):
        np.testing.assert_array_equal(runs[name][0], runs["split"][0], err_msg=name)
        for key in STAT_KEYS:
            np.testing.assert_array_equal(runs[name][1][key], runs["split"][1][key], err_msg=f"{name} {key}")
    return runs["split"]


@pytest.mark.parametrize("name,sqp_kw,solver_kw", DIRECT_CASES, ids=ids(DIRECT_CASES))
def test_direct_settings_match_numpy_under_every_pipeline(lib, model, name, sqp_kw, solver_kw):
    """max_sqp_iters 1, 5 and 8 (5 and 8 with a step_tol that stops problems after 2, 4, 5 and 7, 8
    iterations), mu 1 and 1000 with four iterations, and the regularisation's eps 0.1 and 10, in
    direct mode: 13 problems against SQPRef on the exact KKT solve, under the three pipelines and
    the chunked host-to-host path, which are equal bit for bit.  mu = 1 holds problems whose alpha
    is 0 from iteration 1 on: the line search's tail fill.  Each setting is seen to act on the
    port: more than two iterations run, or the alphas / XU differ from the default's."""
    B = 13
    batch = _batch(B, N, 41)
    xcur, goals, xu = batch
    kw = _with_chosen_step_tol(batch, sqp_kw, solver_kw)
    ref = numpy_solves(xcur, goals, xu, N, solver_kw, kw)[0]
    out, s = _direct_pipelines(lib, model, batch, dict(handle_kw(kw), **solver_kw))
    np.testing.assert_array_equal(s["qp_iters"], ref["qp_iters"])
    for b in range(B):
        assert list(s["alphas"][b][:s["n_alphas"][b]]) == ref["alphas"][b], (b, s["alphas"][b], ref["alphas"][b])
    err = rel(out, ref["xu"]).max()
    print(f"XU rel {err:.2e}")
    assert err < 1e-6, err
    max_iters = kw.get("max_iters", 2)
    first = _tail_fill(s, max_iters)
    if name == "mu1":
        assert any(k >= 1 for k in first), first
    if "step_tol" in kw:
        assert len(set(ref["qp_iters"].tolist())) >= 3, ref["qp_iters"]
    elif name.startswith("sqp"):
        assert (ref["qp_iters"] == max_iters).all()
    else:
        base_kw = {k: v for k, v in kw.items() if k != "mu"}
        d_out, _, d_al, _ = cpu.solve(xcur, goals, xu, N, **base_kw)
        p_out, _, p_al, _ = cpu.solve(xcur, goals, xu, N, **kw, **solver_kw)
        assert not np.array_equal(p_al, d_al, equal_nan=True) and rel(p_out, d_out).max() > 1e-4


def test_direct_ragged_termination_matches_port(lib, model):
    """The 64 problems of the ADMM ragged case in direct mode (max_sqp_iters 8, step_tol from the
    port's direct-mode steps) against the port, under every pipeline: stops after every count from
    1 to 8, three problems with alpha = 0 (two from iteration 1 on) that the tail fill completes
    while their neighbours iterate.  (The port is pinned to numpy on these draws by
    tests/test_settings_oracle.py::test_port_alpha_zero_rows_match_numpy.)"""
    B = 64
    batch = _batch(B, N, 41)
    kw = _with_chosen_step_tol(batch, dict(max_iters=8, step_tol="chosen"))
    ref, qp, al, steps = cpu.solve(*batch, N, nthreads=4, **kw)
    assert step_gap(steps, kw["step_tol"]) >= 0.01
    out, s = _direct_pipelines(lib, model, batch, handle_kw(kw))
    np.testing.assert_array_equal(s["qp_iters"], qp)
    _alphas_equal(s, al, qp)
    err = rel(out, ref).max()
    print(f"XU rel {err:.2e}")
    assert err < 1e-6, err
    assert sorted(set(qp.tolist())) == list(range(1, 9))
    assert sum(k >= 1 for k in _tail_fill(s, 8)) >= 2


# ---- box mode ------------------------------------------------------------------------------------

GPU_BOX_CASES = [c for c in BOX_CASES if c[0] in ("mask1", "mask2", "mask4", "mask5", "max_iters4", "tol1e-4")]


def _box_kw(kw):
    """box_cfg's names as (Handle keywords, OSQPSolverRef keywords)."""
    hk = {{"mask": "box_mask", "max_iters": "box_max_iters", "tol": "box_tol"}[k]: v for k, v in kw.items()}
    return hk, dict(qp="box", **hk)


@pytest.mark.parametrize("name,kw", GPU_BOX_CASES, ids=ids(GPU_BOX_CASES))
def test_box_settings_match_oracle(lib, model, name, kw):
    """The box mode with only some of q, v, u bounded (masks 1, 2, 4, 5), an iteration cap of 4 and
    a tolerance of 1e-4, four problems through the whole SQP against SQPRef on the interior-point
    oracle: SQP iterations and alphas, the last QP's interior-point iterations and converged flag
    identical, mu positive, XU to 1e-5, the bounded entries inside their bounds.  The cap leaves
    every problem unconverged at 4 iterations; the tolerance and the masks change the iteration
    counts against the default's."""
    B = 4
    xcur, goals, xu = _batch(B, N, 46)
    hk, sk = _box_kw(kw)
    h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_BOX, **hk)
    out, s = h.solve(xcur, goals, xu)
    it, conv, mu = h.box_stats(B)
    h.close()
    ref = numpy_solves(xcur, goals, xu, N, sk, {})[0]
    np.testing.assert_array_equal(s["qp_iters"], ref["qp_iters"])
    lo, hi, bm = box_ipm.box_bounds(rbd.params(), N, kw.get("mask", 7))
    for b in range(B):
        assert list(s["alphas"][b][:s["n_alphas"][b]]) == ref["alphas"][b], (b, s["alphas"][b], ref["alphas"][b])
        assert (it[b], bool(conv[b])) == ref["ipm"][b][-1], (b, it[b], conv[b], ref["ipm"][b])
        assert box_relerr(out[b], ref["xu"][b]) <= 1e-5, (b, box_relerr(out[b], ref["xu"][b]))
        assert (out[b][bm] >= lo[bm]).all() and (out[b][bm] <= hi[bm]).all()
    assert (mu > 0).all(), mu
    last = np.array([r[-1][0] for r in ref["ipm"]])
    if "max_iters" in kw:
        assert not conv.any() and (last == kw["max_iters"]).all()
    else:
        assert conv.all()
        default = cpu.solve_box(xcur, goals, xu, N)
        assert (last != default[4][np.arange(B), default[1] - 1]).any()


@pytest.mark.parametrize("mask", [1, 2, 4, 5])
def test_box_mask_leaves_the_other_rows_free(lib, model, mask):
    """One QP with box rows on only some of q, v, u, at linearisation points that make the rows
    bind (tests/test_gpu_box.py::_qp_inputs): the minimiser and the interior point's iterations
    equal the oracle's with the same mask, the bounded entries lie strictly inside their bounds,
    and the entries outside the mask are free: some of them lie outside the bounds that the full
    mask would have enforced on them."""
    from test_gpu_box import _qp_inputs
    xcur, goals, xu = _qp_inputs(N, 3)
    B = xu.shape[0]
    h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_BOX, box_mask=mask)
    sol = h.qp(xu, xcur, goals)
    it, conv, mu = h.box_stats(B)
    h.close()
    ref = OSQPSolverRef(N=N, qp="box", box_mask=mask)
    lo, hi, bm = box_ipm.box_bounds(ref.P_, N, mask)
    lo7, hi7, bm7 = box_ipm.box_bounds(ref.P_, N)
    free = bm7 & ~bm
    assert bm.any() and free.any()
    outside = 0
    for b in range(B):
        x = ref.setup_and_solve_qp(xu[b], xcur[b], goals[b]).x
        r = ref.last_ipm
        assert conv[b] == r.converged and it[b] == r.iters, (b, it[b], r.iters)
        assert box_relerr(sol[b], x) <= 1e-6, (b, box_relerr(sol[b], x))
        assert (sol[b][bm] > lo[bm]).all() and (sol[b][bm] < hi[bm]).all()
        outside += int(((sol[b][free] < lo7[free]) | (sol[b][free] > hi7[free])).sum())
    assert (mu > 0).all(), mu
    assert outside > 0


# ---- one closed loop -----------------------------------------------------------------------------

class _PortDirectSQP:
    """run_mpc_ref's `sqp` with every solve by the port's direct mode: the step lengths of a loop,
    from which the loop's step_tol is chosen."""

    def __init__(self, n, **cfg):
        self.solver, self.N, self.cfg = OSQPSolverRef(N=n), n, cfg
        self.qp_iters, self.steps = [], []

    def sqp(self, xcur, goal, XU):
        out, qp, _, steps = cpu.solve(np.asarray(xcur, float)[None], np.asarray(goal, float)[None],
                                      np.asarray(XU, float)[None], self.N, **self.cfg)
        self.qp_iters.append(int(qp[0]))
        self.steps.append(steps[0])
        return out[0]


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_closed_loop_with_four_iterations_and_early_stops(lib, model, mode):
    """i7m_mpc_run with max_sqp_iters = 4 and a step_tol that stops some of the loop's solves after
    1 or 2 iterations: three instances (one leaves the 1.1 radius at once and stops), 6 MPC steps.
    Direct mode against oracle/mpc_ref.py's loop on SQPRef with the same settings; ADMM mode
    against the same loop with every solve by the port and its carried OSQP state
    (tests/test_gpu_mpc.py::_PortAdmmSQP).  step_tol: the median of the port loop's step lengths
    of iterations 2-3 with step_tol = 0, moved up until the port loop that runs with it has no
    step length within 1 % of it."""
    from test_gpu_mpc import _PortAdmmSQP
    steps_n, B = 6, 3
    xs = _batch(B, N, 63)[0]
    ends = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.9))])
    port_sqp = (lambda **kw: _PortDirectSQP(N, **kw)) if mode == "direct" else (lambda **kw: _PortAdmmSQP(N, **kw))

    def port_loops(step_tol):
        loops, runs = [], []
        for b in range(B):
            loops.append(port_sqp(max_iters=4, step_tol=step_tol))
            runs.append(run_mpc_ref(loops[-1], xs[b], ends, num_steps=steps_n))
        return loops, runs, np.array([s for lp in loops for s in lp.steps])

    tol = float(np.nanmedian(port_loops(0.0)[2][:, 2:6]))
    for _ in range(100):
        loops, runs, steps = port_loops(tol)
        if step_gap(steps, tol) >= 0.01:
            break
        tol *= 1.003
    assert step_gap(steps, tol) >= 0.01
    counts = [c for lp in loops for c in lp.qp_iters]
    assert min(counts) < 4 and max(counts) == 4 and len(set(counts)) >= 3, counts
    if mode == "direct":
        runs = [run_mpc_ref(SQPRef(OSQPSolverRef(N=N), max_iters=4, step_tol=tol), xs[b], ends, num_steps=steps_n)
                for b in range(B)]
    h = lib.Handle(model, N=N, max_batch=B, max_sqp_iters=4, step_tol=tol,
                   qp_mode=lib.QP_DIRECT if mode == "direct" else lib.QP_ADMM)
    d, q, _, _ = h.mpc_run(xs, ends, steps_n)
    h.close()
    atol = 2e-6 if mode == "direct" else 1e-8
    stopped = 0
    for b in range(B):
        xpath, dists = runs[b]
        n, n_plant = len(dists), len(xpath)
        np.testing.assert_allclose(d[:n, b], dists, rtol=0, atol=atol, err_msg=f"instance {b}")
        assert np.isnan(d[n:, b]).all()
        np.testing.assert_allclose(q[:n_plant, b], np.array(xpath).reshape(n_plant, 6), rtol=0, atol=atol)
        assert np.isnan(q[n_plant:, b]).all()
        stopped += n < steps_n
    assert stopped == 1


# ---- refusals ------------------------------------------------------------------------------------

REFUSED = [
    ("direct", dict(max_sqp_iters=0), "max_sqp_iters"),
    ("direct", dict(max_sqp_iters=9), "max_sqp_iters"),
    ("admm", dict(admm=dict(alpha=0.0)), "admm_alpha"),
    ("admm", dict(admm=dict(alpha=2.0)), "admm_alpha"),
    ("admm", dict(admm=dict(rho=0.0)), "admm_rho"),
    ("admm", dict(admm=dict(sigma=0.0)), "admm_sigma"),
    ("admm", dict(admm=dict(eps_abs=-1.0)), "admm eps"),
    ("admm", dict(admm=dict(scaling=101)), "admm_scaling"),
    ("admm", dict(admm=dict(check_termination=-1)), "admm_check_termination"),
    ("admm", dict(admm=dict(adaptive_rho_tolerance=0.5)), "admm_adaptive_rho_tolerance"),
    ("box", dict(box_max_iters=0), "box_max_iters"),
    ("box", dict(box_max_iters=201), "box_max_iters"),
]
ACCEPTED = [
    ("direct", dict(max_sqp_iters=1)),
    ("direct", dict(max_sqp_iters=8)),
    ("admm", dict(admm=dict(scaling=0))),
    ("admm", dict(admm=dict(scaling=100))),
    ("admm", dict(admm=dict(check_termination=0))),
]


def _case_id(c):
    (k, v), = c[1].items()
    if isinstance(v, dict):
        (k, v), = v.items()
    return f"{k}={v}"


@pytest.mark.parametrize("mode,kw,names", REFUSED, ids=[_case_id(c) for c in REFUSED])
def test_create_refuses_setting(lib, model, mode, kw, names):
    """i7m_create returns I7M_EINVAL (-1) with a message that names the setting for a value outside
    its range: no handle comes back (the range checks precede i7m_create's first allocation)."""
    qp_mode = {"direct": lib.QP_DIRECT, "admm": lib.QP_ADMM, "box": lib.QP_BOX}[mode]
    with pytest.raises(lib.I7MError, match=f"error -1: .*{names}"):
        lib.Handle(model, N=N, max_batch=1, qp_mode=qp_mode, **kw)


@pytest.mark.parametrize("mode,kw", ACCEPTED, ids=[_case_id(c) for c in ACCEPTED])
def test_create_accepts_the_range_ends(lib, model, mode, kw):
    """The values next to the refused ones create a handle."""
    h = lib.Handle(model, N=N, max_batch=1, qp_mode={"direct": lib.QP_DIRECT, "admm": lib.QP_ADMM}[mode], **kw)
    assert h._h
    h.close()
