"""CPU, the C++ port only: the tracking reference loop (tests/tracking_mpc_ref.py) with a one-point
reference is the sampled reference loop (tests/sampled_mpc_ref.py) with that single endpoint, bit
for bit, as long as the endpoint is not reached — the tie between the new helper and the one the
merged loop is tested against."""
import numpy as np
import pytest

from oracle import rbd
from sampled_mpc_ref import GOAL_RADIUS, run_sampled_ref
from tracking_mpc_ref import make_tracking_case, run_tracking_ref, window


def test_window_clamps():
    ref = np.arange(30, dtype=float).reshape(5, 6)
    np.testing.assert_array_equal(window(ref, 0, 0, 3), ref[[0, 1, 2], :3].reshape(-1))
    np.testing.assert_array_equal(window(ref, 1, 2, 4), ref[[3, 4, 4, 4], :3].reshape(-1))
    np.testing.assert_array_equal(window(ref, 2, 100, 2), ref[[4, 4], :3].reshape(-1))
    np.testing.assert_array_equal(window(ref[:1], 0, 7, 2), ref[[0, 0], :3].reshape(-1))


@pytest.mark.parametrize("mode", ["direct", "admm"])
def test_one_point_reference_is_the_endpoint_loop(mode):
    G, H, N, steps = 2, 4, 8, 4
    xs, fhyp, fact, k = make_tracking_case(G, H, seed=11)
    end = rbd.eepos(np.full(6, 0.9))
    noise = np.random.default_rng(5).normal(0, 2.0, (steps, G * H, 3))
    kw = dict(noise=noise, sim_dt=0.01, qp_mode=mode, keep_best=True, decay=0.97)
    ends = run_sampled_ref(N, G, H, xs, end[None], steps, fhyp, fact, **kw)
    assert (ends["dist"] > GOAL_RADIUS).all()  # never reached: the endpoint loop neither switches nor stops
    for stride in (3, 6):
        ref = np.zeros((1, stride))
        ref[0, :3] = end
        trk = run_tracking_ref(N, G, H, xs, ref, [0, 1, 5, 1000], fhyp, fact, ref_phase=[0, 3], **kw)
        np.testing.assert_array_equal(trk["err"], ends["dist"])
        for key in ("best", "q", "fbest", "xcur", "xu_best", "fhyp", "err2"):
            np.testing.assert_array_equal(trk[key], ends[key], err_msg=key)
        np.testing.assert_array_equal(trk["ee"], np.array([[rbd.eepos(q) for q in row] for row in trk["q"]]))
    np.testing.assert_array_equal(ends["best"][0], k)
