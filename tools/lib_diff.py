"""Bitwise comparison of two library builds on the same inputs (tools/ only).

    I7M_LIB=<a.so> python tools/lib_diff.py dump A.npz    (one process per build)
    python tools/lib_diff.py cmp A.npz B.npz

dump: one config-3 solve (B = 4096, N = 32, bench.py's draws), one config-4 solve (B = 256,
N = 64, box rows), the notebook's 500-step closed loop (B = 1, N = 32), and the ADMM mode: config
3, N = 64, odd batches, adaptive rho, the closing tests after max_iter, each streaming kernel forced;
and the sampled-wrench family at (G, H, N) = (2, 4, 8), 3 steps, direct and ADMM: mpc_run_sampled with
noise, mpc_run_tracking with phases and noise, a controller session in both x0 forms with noise and
its ctrl_end, the multi-rate loops (shifted warm start, the residue sub-step, tracking), a group that
stops with either plant, H = 256 (direct) and mpc_run_multirate (ADMM) (every array of the returned
dicts, keys fam_*).
cmp: per output, how many problems differ at all, the largest relative difference, for the
closed loop the first step at which the goal distances differ, and per key of the family how many
entries differ.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(path):
    from indy7_mpc_amd import _lib
    from indy7_mpc_amd.model import default_model
    from oracle.osqp_ref import synthetic_batch  # goals by the CPU FK: identical inputs for both builds
    m = default_model()
    out = {}
    xc, g, xu = synthetic_batch(4096, 32, 45)
    h = _lib.Handle(m, N=32, max_batch=4096)
    out["c3"] = h.solve(xc, g, xu)[0]
    h.close()
    xc, g, xu = synthetic_batch(256, 64, 48)
    h = _lib.Handle(m, N=64, max_batch=256, qp_mode=_lib.QP_BOX)
    out["c4"] = h.solve(xc, g, xu)[0]
    h.close()
    tr = json.load(open(os.path.join(ROOT, "tests", "golden", "notebook_kats.json")))["mpc_trace"]
    h = _lib.Handle(m, N=32, max_batch=1)
    ends = h.eepos(np.array(tr["endpoint_q"]))
    out["mpc"] = h.mpc_run(np.array([tr["xstart"]]), ends, 500)[0][:, 0]
    h.close()
    # ADMM mode (the drop-in default): config 3 twice (cold, then warm from the carried state), the
    # carried state after it, N = 64 and an odd batch (empty rows of the 3- and 4-problem waves)
    for key, (B, N, seed) in {"a3": (4096, 32, 45), "a64": (24, 64, 48), "a13": (13, 32, 50)}.items():
        xc, g, xu = synthetic_batch(B, N, seed)
        h = _lib.Handle(m, N=N, max_batch=B, qp_mode=_lib.QP_ADMM)
        o1 = h.solve(xc, g, xu)[0]
        o2 = h.solve(xc, g, o1)[0]
        out[key] = np.concatenate([o1, o2], axis=1)
        out[key + "_state"] = np.concatenate(h.admm_state(B)[:4], axis=1)
        out[key + "_iters"] = h.admm_stats(B)[0]
        h.close()
    h = _lib.Handle(m, N=32, max_batch=1, qp_mode=_lib.QP_ADMM)
    out["mpca"] = h.mpc_run(np.array([tr["xstart"]]), ends, 40)[0][:, 0]
    h.close()
    # the iteration kernels' other paths, B = 13 (idle rows in the streaming kernels' last wave): the
    # adaptive-rho kernel with its in-kernel re-factor, the closing tests after max_iter, and each
    # streaming kernel forced at N = 32 (and with the closing tests: `close` alone runs the resident
    # kernel); outputs, carried state, rho, OSQP iterations and statuses
    it2, it4 = {"I7M_ADMM_RES": "0", "I7M_ADMM_ITER2": "1"}, {"I7M_ADMM_RES": "0", "I7M_ADMM_ITER2": "0"}
    closing = dict(max_iter=20, eps_abs=1e-3, eps_rel=1e-3)
    for key, N, admm, env in (("adapt", 16, dict(rho=0.005, adaptive_rho_interval=25), {}),
                              ("close", 16, closing, {}), ("it2", 32, None, it2), ("it4", 32, None, it4),
                              ("close2", 16, closing, it2), ("close4", 16, closing, it4)):
        xc, g, xu = synthetic_batch(13, N, 54)
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:  # (the handle reads the forced kernel choice when it is created)
            h = _lib.Handle(m, N=N, max_batch=13, qp_mode=_lib.QP_ADMM, **({"admm": admm} if admm else {}))
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        o1 = h.solve(xc, g, xu)[0]
        o2 = h.solve(xc, g, o1)[0]
        state, (its, rho, stat) = h.admm_state(13), h.admm_stats(13, with_status=True)
        out[key] = np.concatenate([o1, o2], axis=1)
        out[key + "_state"] = np.concatenate(state[:4] + (state[4][:, None], rho[:, None]), axis=1)
        out[key + "_stats"] = np.concatenate([its, stat], axis=1)
        h.close()
    out.update(family(_lib, m, ends))
    out["ver"] = np.array(_lib.version())
    np.savez(path, **out)


def family(_lib, m, ends):
    """The sampled-wrench entry points on fixed inputs: {fam_<mode>_<call>_<key>: array}."""
    from indy7_mpc_amd.utils import figure8
    from oracle import rbd
    G, H, N, steps = 2, 4, 8, 3
    rng = np.random.default_rng(61)
    xs = np.concatenate([rng.uniform(-1, 1, (G, 6)), rng.uniform(-0.5, 0.5, (G, 6))], axis=1)
    fhyp = np.zeros((G, H, 6))
    fhyp[:, :, :3] = rng.normal(0, 10.0, (G, H, 3))
    fhyp[:, 0] = 0.0
    fact, fhyp = fhyp[np.arange(G), (np.arange(G) + 1) % H].copy(), fhyp.reshape(G * H, 6)
    noise = rng.normal(0, 2.0, (steps, G * H, 3))
    ref = figure8(0.5, 0.55, [0, 0.4, 0.45], period=1.0, dt=0.01, cycles=3).reshape(-1, 6)
    kw = dict(keep_best=True, decay=0.97)
    # (drawn after the inputs above, which stay what they were)
    noise12 = rng.normal(0, 2.0, (12, G * H, 3))
    fhyp256 = np.zeros((G, 256, 6))
    fhyp256[:, :, :3] = rng.normal(0, 10.0, (G, 256, 3))
    fhyp256[:, 0] = 0.0
    fhyp256[np.arange(G), (np.arange(G) + 1) % H] = fact  # the actual wrench is among them
    fhyp256 = fhyp256.reshape(G * 256, 6)
    noise256 = rng.normal(0, 2.0, (2, G * 256, 3))
    xs3 = np.concatenate([rng.uniform(-1, 1, (3, 6)), rng.uniform(-0.5, 0.5, (3, 6))], axis=1)
    xs_stop = np.zeros((G, 12))
    xs_stop[0, :6], xs_stop[1, :6] = 0.31, -0.4
    ends_stop = np.array([rbd.eepos(np.full(6, 0.3)), rbd.eepos(np.full(6, 0.33))])
    out = {}
    for mode, qp in (("direct", _lib.QP_DIRECT), ("admm", _lib.QP_ADMM)):
        def handle():
            return _lib.Handle(m, N=N, max_batch=G * H, qp_mode=qp)
        calls = {}
        h = handle()
        calls["sampled"] = h.mpc_run_sampled(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.01, **kw)
        h.close()
        h = handle()
        calls["tracking"] = h.mpc_run_tracking(xs, ref, [1, 2, 4], fhyp, fact, ref_phase=[0, 17], noise=noise, sim_dt=0.01, **kw)
        h.close()
        for form, x0 in (("x0", xs), ("null", None)):
            h = handle()
            r = {"u0": h.ctrl_begin(ref, fhyp, x0=x0, groups=G, ref_phase=[0, 17], **kw)}
            x = xs.copy()
            for i, (el, off) in enumerate(((0.01, 1), (0.008, 1), (0.012, 3))):
                x[:, :6] += el * x[:, 6:]  # any finite measurement serves: both builds get the same
                for k, v in h.ctrl_step(x, el, off, noise=noise[i]).items():
                    r[f"step{i}_{k}"] = v
            r.update(h.ctrl_end())
            h.close()
            calls["ctrl_" + form] = r
        # the multi-rate plant: two knots a step with the warm start shifted, the residue sub-step of
        # sim_dt = 0.001 (step 9 is [0.001, 8.67e-19]), and tracking with 2.5 knots a step
        h = handle()
        calls["sampled_mr"] = h.mpc_run_sampled_multirate(xs, ends, steps, fhyp, fact, noise=noise, sim_dt=0.02,
                                                          shift_warm_start=1, **kw)
        h.close()
        h = handle()
        calls["sampled_mr_residue"] = h.mpc_run_sampled_multirate(xs, ends, 12, fhyp, fact, noise=noise12, sim_dt=0.001,
                                                                  shift_warm_start=1, **kw)
        h.close()
        h = handle()
        calls["tracking_mr"] = h.mpc_run_tracking_multirate(xs, ref, steps, fhyp, fact, ref_phase=[0, 17], noise=noise,
                                                            sim_dt=0.025, **kw)
        h.close()
        # a group that stops mid-run (at rest within the radius of both endpoints: it switches, then
        # stops), so the NaN / -1 layout is compared, with either plant
        for call, run, sim_dt in (("sampled_stop", "mpc_run_sampled", 0.01), ("sampled_mr_stop", "mpc_run_sampled_multirate", 0.02)):
            h = handle()
            calls[call] = getattr(h, run)(xs_stop, ends_stop, 4, np.zeros((G * H, 6)), np.zeros((G, 6)), sim_dt=sim_dt)
            h.close()
        if mode == "direct":  # H = 256: the merge of four waves (H = 4 above: one partial wave)
            h = _lib.Handle(m, N=N, max_batch=G * 256, qp_mode=qp)
            calls["sampled_w4"] = h.mpc_run_sampled(xs, ends, 2, fhyp256, fact, noise=noise256, sim_dt=0.01, **kw)
            h.close()
            h = _lib.Handle(m, N=N, max_batch=G * 256, qp_mode=qp)
            calls["sampled_mr_w4"] = h.mpc_run_sampled_multirate(xs, ends, 2, fhyp256, fact, noise=noise256, sim_dt=0.02,
                                                                 shift_warm_start=1, **kw)
            h.close()
        else:  # the closed loops' shared reset: the multi-rate loop of whole instances
            h = _lib.Handle(m, N=N, max_batch=3, qp_mode=qp)
            calls["multirate"] = h.mpc_run_multirate(xs3, ends, 3, sim_dt=0.02)
            h.close()
        for call, r in calls.items():
            for k, v in r.items():
                out[f"fam_{mode}_{call}_{k}"] = np.asarray(v)
    return out


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    print("A:", str(A["ver"]), "\nB:", str(B["ver"]))
    for k in ("c3", "c4", "a3", "a3_state", "a3_iters", "a64", "a64_state", "a13", "a13_state") + tuple(
            k + s for k in ("adapt", "close", "it2", "it4", "close2", "close4") for s in ("", "_state", "_stats")):
        if k not in A or k not in B:
            continue
        x, y = A[k].astype(float), B[k].astype(float)
        diff = (x != y).any(axis=1)
        rel = np.linalg.norm(x - y, axis=1) / np.maximum(np.linalg.norm(x, axis=1), 1e-300)
        print(f"{k}: {int(diff.sum())} of {len(x)} problems differ; max rel {rel.max():.2e}")
    for k in ("mpc", "mpca"):
        if k not in A or k not in B:
            continue
        x, y = A[k], B[k]
        nz = np.nonzero((x != y) & ~(np.isnan(x) & np.isnan(y)))[0]
        print(f"{k}: first differing step {nz[0] if len(nz) else None}; max |diff| {np.nanmax(np.abs(x - y)):.3e}")
    fam = sorted(k for k in set(A.files) | set(B.files) if k.startswith("fam_"))
    total = 0
    for k in fam:
        if k not in A.files or k not in B.files:
            print(f"{k}: only in {'A' if k in A.files else 'B'}")
            total += 1
            continue
        x, y = A[k], B[k]
        n = x.size if x.shape != y.shape else int(((x != y) & ~((x != x) & (y != y))).sum())
        total += n
        print(f"{k}: {n} of {x.size} entries differ")
    if fam:
        print(f"family: {len(fam)} keys, {total} differing entries in all")


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        cmp(sys.argv[2], sys.argv[3])
