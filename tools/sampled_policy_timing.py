#!/usr/bin/env python3
"""GPU: what the feedback policy costs and what it does in the sampled-wrench loops and the
controller session.  Three parts, each a process of its own (`--part`), so that
each runs under its own time limit:

cost      i7m_mpc_run_tracking_multirate at (G, H, N) = (256, 16, 32) and (1, 16, 64), sim_dt = 0.02,
          I7M_QP_ADMM, reset ALL before every solve: ms per MPC step with control_from "new" and
          "policy" in alternating repetitions (a call of warm + steps minus a call of warm, over steps,
          so allocation, copies and the initial solve cancel); the median and the spread (max - min).
session   i7m_ctrl_step at (1, 16, 64), ADMM, as tools/ctrl_step_latency.py measures it: p50 / p99 of
          the step with the policy off and on (n_k = N - 1; the step then also runs the policy pass,
          the copy kernel and a second device-to-host copy), two repetitions each, alternating.
tracking  the notebook's two figure-8 runs (N = 32, 0.02 s per solve, force [10, 15, -6], one
          hypothesis and 64) through MPC_GATO_Batch_Sample.run_mpc_fig8 with feedback off and on: the
          mean logged tracking error over the second half of the run.

Prints and writes (--out, one file per part: NAME.<part>.json) one JSON object per part.  Not a test,
and nothing is asserted: it reports, whatever the sign.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def per_step(run, warm, steps):
    t = []
    for n in (warm + steps, warm):
        t0 = time.perf_counter()
        run(n)
        t.append(time.perf_counter() - t0)
    return 1e3 * (t[0] - t[1]) / steps


def cost(lib, model, shapes, warm, steps, reps):
    from indy7_mpc_amd.utils import figure8

    ref = figure8(0.5, 0.55, [0, 0.4, 0.45], period=10.0, dt=0.01, cycles=2).reshape(-1, 6)
    res = []
    for G, H, N in shapes:
        rng = np.random.default_rng(11)
        xs = np.concatenate([rng.uniform(-0.3, 0.3, (G, 6)), rng.uniform(-0.2, 0.2, (G, 6))], axis=1)
        fhyp = np.zeros((G, H, 6))
        fhyp[:, :, :3] = rng.normal(0, 5.0, (G, H, 3))
        fhyp[:, 0] = 0.0
        fact = fhyp[:, 1 % H].copy()
        fhyp = fhyp.reshape(G * H, 6)
        phase = (np.arange(G) * 7) % 900
        h = lib.Handle(model, N=N, max_batch=G * H, qp_mode=lib.QP_ADMM)
        runs = {c: (lambda n, c=c: h.mpc_run_tracking_multirate(xs, ref, n, fhyp, fact, ref_phase=phase, sim_dt=0.02,
                                                                control_from=c)) for c in ("new", "policy")}
        for run in runs.values():
            run(2)  # first-use costs out of the way
        ms = {c: [] for c in runs}
        for _ in range(reps):  # alternating
            for c, run in runs.items():
                ms[c].append(per_step(run, warm, steps))
        med = {c: float(np.median(v)) for c, v in ms.items()}
        last = {c: run(warm + steps) for c, run in runs.items()}
        res.append({"G": G, "H": H, "N": N, "qp_mode": "admm", "sim_dt": 0.02, "warm": warm, "steps": steps,
                    "ms_per_step": ms, "median_ms_per_step": med,
                    "spread_ms": {c: float(max(v) - min(v)) for c, v in ms.items()},
                    "policy_minus_new_ms": med["policy"] - med["new"],
                    "mean_tracking_error": {c: float(np.mean(r["err"])) for c, r in last.items()},
                    "true_row_wins": {c: float(np.mean(r["best"] == 1 % H)) for c, r in last.items()}})
        print(json.dumps(res[-1]), flush=True)
        h.close()
    return res


def session(lib, model, steps, warmup):
    from ctrl_step_latency import DT, G, H, N, case, pct

    ref, fhyp, xm, noise = case(steps + warmup)

    def run(n_k):
        h = lib.Handle(model, N=N, dt=DT, max_batch=H, qp_mode=lib.QP_ADMM)
        h.ctrl_begin(ref, fhyp, x0=None, groups=G, reset_what=lib.ADMM_RESET_ALL, keep_best=True, decay=0.97)
        if n_k:
            h.ctrl_set_policy(n_k)
        ts = []
        for i in range(len(xm)):
            t0 = time.perf_counter()
            u = h.ctrl_step(xm[i], DT, i + 1, noise=noise[i])["u"]
            ts.append(time.perf_counter() - t0)
        assert np.isfinite(u).all()
        h.ctrl_end()
        h.close()
        return pct(ts[warmup:])

    rec = dict(shape=dict(G=G, H=H, N=N), qp_mode="admm", reset_what="ALL", steps=steps, warmup=warmup, n_k=N - 1,
               policy_off=[], policy_on=[])
    for _ in range(2):
        rec["policy_off"].append(run(0))
        rec["policy_on"].append(run(N - 1))
    for k in ("p50_ms", "p99_ms"):
        off, on = [r[k] for r in rec["policy_off"]], [r[k] for r in rec["policy_on"]]
        rec[k + "_summary"] = dict(off=min(off), on=min(on), on_minus_off=round(min(on) - min(off), 4),
                                   off_spread=round(max(off) - min(off), 4), on_spread=round(max(on) - min(on), 4))
    print(json.dumps(rec), flush=True)
    return rec


def tracking(model, sim_time):
    from indy7_mpc_amd.gato_mpc_batch_sample import MPC_GATO_Batch_Sample
    from indy7_mpc_amd.utils import figure8

    # the notebook's figure8(): x = 0.4 sin t, y = 0.5, z = 0.75 + 0.4 sin(2 t) / 2 + 0.2, 5 s per cycle, five cycles
    fig8 = figure8(0.4, 0.4, [0.0, 0.5, 0.75], period=5, dt=0.01, cycles=5, angle=0.0)
    f_ext = np.array([10.0, 15.0, -6.0, 0.0, 0.0, 0.0])
    res = []
    for H, kw in ((1, dict(f_ext_std=0.0)), (64, dict(f_ext_std=1.0, seed=42))):
        rec = {"batch_size": H, "N": 32, "sim_dt": 0.02, "sim_time": sim_time, "force": f_ext[:3].tolist()}
        for fb in (False, True):
            ctrl = MPC_GATO_Batch_Sample(model, N=32, dt=0.01, batch_size=H, constant_f_ext=f_ext, resample_f_ext=False,
                                         f_ext_resample_std=0.0, **kw)
            t0 = time.perf_counter()
            xpath, st = ctrl.run_mpc_fig8(np.zeros(12), fig8, 0.02, sim_time, feedback=fb)
            d = np.asarray(st["goal_distances"], float)
            err = ctrl.last["err"][:, 0]
            rec["feedback" if fb else "open_loop"] = {
                "seconds": time.perf_counter() - t0, "steps": int(len(err)), "path_entries": len(xpath), "logged": int(len(d)),
                "mean_logged_error_second_half": float(d[len(d) // 2:].mean()),
                "mean_error_every_step_second_half": float(err[len(err) // 2:].mean()),
                "max_logged_error_second_half": float(d[len(d) // 2:].max()), "finite": bool(np.isfinite(err).all())}
        res.append(rec)
        print(json.dumps(rec), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("cost", "session", "tracking"), required=True)
    ap.add_argument("--shapes", default="256x16x32,1x16x64", help="GxHxN of the cost part, comma separated")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--session-steps", type=int, default=200)
    ap.add_argument("--sim-time", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_policy_timing"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model

    model = default_model()
    out = {"tool": "tools/sampled_policy_timing.py", "part": a.part, "version": lib.version()}
    if a.part == "cost":
        out["cost"] = cost(lib, model, [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")], a.warm, a.steps,
                           a.reps)
    elif a.part == "session":
        out["session"] = session(lib, model, a.session_steps, 10)
    else:
        out["tracking"] = tracking(model, a.sim_time)
    path = f"{a.out}.{a.part}.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
