"""Latency record of one controller step at the deployed shape, (G, H, N) = (1, 16, 64), ADMM, the
OSQP state reset before every solve (gato_controller.py:221-223): p50 / p99 of

  fused     Handle.ctrl_step (i7m_ctrl_step), numpy in, u out;
  composed  the same step from the public surface as gato_controller.py:213-228 composes it:
            batch_sqp.SQPSolverfloat_16 reset + resetRho + resetLambda + solve + sim_forward + a
            host argmin + the resample + set_external_wrench_batch.

Each variant runs one session of --warmup + --steps steps, twice (two repetitions of the same
measurement give the spread to read the difference against).  The plant is a recorded state
sequence near the reference (the latency does not depend on it beyond the OSQP iteration counts,
which both variants share).  Writes profiles/ctrl_step_latency.json and prints the same.

    python tools/ctrl_step_latency.py [--steps 200] [--warmup 10] [--out profiles/ctrl_step_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, H, N, DT = 1, 16, 64, 0.01


def case(steps):
    from indy7_mpc_amd.utils import figure8

    ref = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=DT, cycles=4 + steps // 100).reshape(-1, 6)
    rng = np.random.default_rng(12)
    x0 = np.concatenate([rng.uniform(-1, 1, 6), rng.uniform(-0.5, 0.5, 6)])
    fhyp = np.zeros((H, 6))
    fhyp[:, :3] = rng.normal(0, 10.0, (H, 3))
    fhyp[0] = 0.0
    # the measured states: a slow random walk from x0 (finite, bounded), the same for both variants
    xm = x0 + np.cumsum(rng.normal(0, 2e-3, (steps, 12)), axis=0)
    noise = rng.normal(0, 2.0, (steps, H, 3))
    return ref, fhyp, xm, noise


def pct(ts):
    ts = np.asarray(ts) * 1e3
    return dict(p50_ms=round(float(np.percentile(ts, 50)), 4), p99_ms=round(float(np.percentile(ts, 99)), 4),
                mean_ms=round(float(ts.mean()), 4), max_ms=round(float(ts.max()), 4))


def run_fused(model, lib, ref, fhyp, xm, noise, warmup):
    h = lib.Handle(model, N=N, dt=DT, max_batch=H, qp_mode=lib.QP_ADMM)
    h.ctrl_begin(ref, fhyp, x0=None, groups=G, reset_what=lib.ADMM_RESET_ALL, keep_best=True, decay=0.97)
    ts = []
    for i in range(len(xm)):
        t0 = time.perf_counter()
        u = h.ctrl_step(xm[i], DT, i + 1, noise=noise[i])["u"]
        ts.append(time.perf_counter() - t0)
    assert np.isfinite(u).all()
    h.ctrl_end()
    h.close()
    return ts[warmup:]


def run_composed(model, ref, fhyp, xm, noise, warmup):
    from indy7_mpc_amd.bindings import batch_sqp

    s = batch_sqp.SQPSolverfloat_16(model=model, qp_mode="admm")
    f = fhyp.copy()
    s.set_external_wrench_batch(f)
    T = 18 * N - 6
    goals = np.tile(ref[:N].reshape(-1), (H, 1))
    xs = np.zeros((H, 12))
    XU = s.solve(np.zeros((H, T)), DT, xs, goals)["xu_trajectory"]
    XU[:] = XU[0]
    x_last, u_last = None, None
    ts = []
    for i in range(len(xm)):
        t0 = time.perf_counter()
        x = xm[i]
        if x_last is None:
            x_last, u_last = x, np.zeros(6)
        off = min(i + 1, len(ref) - N)
        goals[:, :] = ref[off:off + N].reshape(-1)
        xs[:, :] = x
        XU[:, :12] = x
        s.reset()
        s.resetRho()
        s.resetLambda()
        new = s.solve(XU, DT, xs, goals)["xu_trajectory"]
        pred = s.sim_forward(x_last, u_last, DT)
        best = int(np.argmin(np.linalg.norm(pred - x, axis=1)))
        fb = f[best].copy()
        f[:] = fb
        f[:, :3] += noise[i]
        f[best] = fb
        f[:, 3:] = 0.0
        f[0] = 0.0
        f *= 0.97
        s.set_external_wrench_batch(f)
        XU[:] = new[best]
        u = XU[0, 12:18].copy()
        x_last, u_last = x, u
        ts.append(time.perf_counter() - t0)
    assert np.isfinite(u).all()
    return ts[warmup:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctrl_step_latency.json"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model

    model = default_model()
    ref, fhyp, xm, noise = case(a.steps + a.warmup)
    rec = dict(shape=dict(G=G, H=H, N=N), qp_mode="admm", reset_what="ALL", steps=a.steps, warmup=a.warmup,
               period_ms=DT * 1e3, library=lib.version(), fused=[], composed=[])
    for rep in range(2):
        rec["fused"].append(pct(run_fused(model, lib, ref, fhyp, xm, noise, a.warmup)))
        rec["composed"].append(pct(run_composed(model, ref, fhyp, xm, noise, a.warmup)))
    for k in ("p50_ms", "p99_ms"):
        fu, co = [r[k] for r in rec["fused"]], [r[k] for r in rec["composed"]]
        rec[k + "_summary"] = dict(fused=min(fu), composed=min(co), fused_spread=round(max(fu) - min(fu), 4),
                                   composed_spread=round(max(co) - min(co), 4))
    rec["p99_within_period"] = max(r["p99_ms"] for r in rec["fused"]) <= DT * 1e3
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
