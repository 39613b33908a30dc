#!/usr/bin/env python3
"""GPU: the per-step time of the multi-rate closed loop (i7m_mpc_run_multirate, one launch after
each solve) against i7m_mpc_run (a goal launch before and an advance launch after each solve) on
the same handle, ADMM mode, the OSQP state carried from step to step in both (reset_what = 0: the
solve is the same code path in both; i7m_mpc_run has no per-step reset).  The drop-ins' default,
reset ALL before every solve, is timed too and reported beside it.

Per shape and sim_dt, `--reps` alternating repetitions; a repetition times a call of warm + steps
MPC steps and a call of warm steps and reports their difference / steps, so allocation, copies
and the initial solve cancel.  The start states are at least 0.3 from both endpoints, so no
instance switches or stops within the timed steps, and at most 0.9 from both, so i7m_mpc_run's
stop above 1.1 does not turn its instances into no-ops (the record counts the instances either
loop stopped).

Prints and writes (--out) one JSON object.  One process; run it under `timeout`.  Not a test, and
no ratio is asserted: it reports.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(B, seed, eepos, ends):
    rng = np.random.default_rng(seed)
    xs = np.concatenate([rng.uniform(-1, 1, (B, 6)), rng.uniform(-0.5, 0.5, (B, 6))], axis=1)
    for _ in range(100):
        d = np.linalg.norm(eepos(xs[:, :6])[:, None] - ends[None], axis=2)
        near = (d.min(axis=1) < 0.3) | (d.max(axis=1) > 0.9)  # (i7m_mpc_run stops an instance above 1.1)
        if not near.any():
            break
        xs[near, :6] = rng.uniform(-1, 1, (int(near.sum()), 6))
    return xs


def per_step(run, h, warm, steps):
    """ms per MPC step of run(num_steps): (a call of warm + steps) - (a call of warm), over steps."""
    t = []
    for n in (warm + steps, warm):
        h.reset()
        t0 = time.perf_counter()
        run(n)
        t.append(time.perf_counter() - t0)
    return 1e3 * (t[0] - t[1]) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="4096x32,1x32", help="BxN, comma separated")
    ap.add_argument("--sim-dts", default="0.001,0.02")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multirate_loop_timing.json"))
    a = ap.parse_args()
    from indy7_mpc_amd import _lib as lib
    from indy7_mpc_amd.model import default_model

    model = default_model()
    q = lib.Handle(model, N=2, max_batch=2)
    ends = q.eepos(np.array([np.full(6, 0.3), np.full(6, 0.9)]))
    res = []
    for shape in a.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        xs = case(B, 11, q.eepos, ends)
        h = lib.Handle(model, N=N, max_batch=B, qp_mode=lib.QP_ADMM)
        h.mpc_run(xs, ends, 2)  # first-use costs out of the way
        for sim_dt in (float(v) for v in a.sim_dts.split(",")):
            runs = {
                "mpc_run": lambda n: h.mpc_run(xs, ends, n),
                "multirate": lambda n: h.mpc_run_multirate(xs, ends, n, sim_dt=sim_dt, reset_what=0),
                "multirate_reset_all": lambda n: h.mpc_run_multirate(xs, ends, n, sim_dt=sim_dt),
            }
            runs["multirate"](2)
            ms = {k: [] for k in runs}
            for _ in range(a.reps):  # alternating
                for k, run in runs.items():
                    ms[k].append(per_step(run, h, a.warm, a.steps))
            # where a difference comes from: the solve's own kernels (HIP events on their dispatches),
            # per MPC step of a run of warm + steps; the loops' own kernels are the remainder.  The two
            # loops do not solve the same QPs (another plant step, another warm start), so OSQP may
            # take another number of sweeps.
            kern = {}
            for k, run in runs.items():
                h.reset()
                h.set_timing(True)
                h.reset_kernel_times()
                run(a.warm + a.steps)
                kt = h.kernel_times()
                h.set_timing(False)
                kern[k] = {name: {"ms_per_step": ms_sum / (a.warm + a.steps + 1), "launches": int(cnt)}
                           for name, (ms_sum, cnt) in kt.items()}
                kern[k]["solve_kernels_ms_per_step"] = sum(v[0] for v in kt.values()) / (a.warm + a.steps + 1)
            r = h.mpc_run_multirate(xs, ends, a.warm + a.steps, sim_dt=sim_dt, reset_what=0)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res.append({
                "B": B, "N": N, "qp_mode": "admm", "sim_dt": sim_dt, "steps": a.steps, "warm": a.warm,
                "ms_per_step": ms, "median_ms_per_step": med,
                "spread_ms": {k: float(max(v) - min(v)) for k, v in ms.items()},
                "multirate_minus_mpc_run_ms": med["multirate"] - med["mpc_run"],
                "solve_kernels": kern,
                "multirate_minus_mpc_run_solve_kernels_ms": kern["multirate"]["solve_kernels_ms_per_step"]
                - kern["mpc_run"]["solve_kernels_ms_per_step"],
                "sub_steps": int(r["sub_start"][-1]), "knots_shifted": int(r["shift"].sum()),
                "mpc_run_instances_stopped": int(np.isnan(h.mpc_run(xs, ends, a.warm + a.steps)[0]).any(axis=0).sum()),
                "instances_that_met_a_goal": int((~np.isfinite(r["dist"])).any(axis=0).sum() + (r["dist"] < 0.1).any(axis=0).sum()),
                "note": "mpc_run: its own loop (one 0.01 s plant step per solve) on the same handle, state carried; "
                        "multirate: reset_what = 0; multirate_reset_all: the drop-ins' default",
            })
            print(json.dumps(res[-1]), flush=True)
        h.close()
    out = {"tool": "tools/multirate_loop_timing.py", "version": lib.version(), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
