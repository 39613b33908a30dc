"""CPU: the numpy statement of the sampled-wrench closed loop (tests/sampled_mpc_ref.py, the
reference of tests/test_gpu_sampled_mpc.py) against the contract in include/indy7_mpc.h
(i7m_mpc_run_sampled): the estimator names the true hypothesis with an error of exactly 0, the
resampling order, the goal switch and the stop."""
import numpy as np
import pytest

from oracle import rbd
from sampled_mpc_ref import make_case, resample, run_sampled_ref


@pytest.mark.parametrize("sim_dt", [0.01, 0.001])
def test_true_hypothesis_wins_with_zero_error(sim_dt):
    G, H, N, steps = 3, 4, 8, 6
    xs, ends, fhyp, fact, k = make_case(G, H, seed=1)
    r = run_sampled_ref(N, G, H, xs, ends, steps, fhyp, fact, sim_dt=sim_dt)
    assert np.isfinite(r["dist"]).all()
    np.testing.assert_array_equal(r["best"], np.tile(k, (steps, 1)))
    assert (r["err2"][:, :, 0] == 0.0).all()
    assert (r["err2"][:, :, 1] > 1e-3).all()
    np.testing.assert_array_equal(r["fbest"], np.tile(fact, (steps, 1, 1)))
    np.testing.assert_array_equal(r["fhyp"], fhyp)  # no noise table: the hypotheses stay


def test_resample_order_on_a_hand_made_case():
    rows = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 0, 0, 0], [4, 5, 6, 7, 8, 9], [-1, -2, -3, 0, 0, 0]], float)
    noise = np.array([[10, 10, 10], [0.5, 0.25, 0.125], [1, 1, 1], [2, 4, 8]], float)
    # the controller's rule: the winner (row 2, with torques) keeps its force, torques go, row 0 is 0
    got = resample(rows, 2, noise, keep_best=True, decay=0.97)
    want = np.array([[0, 0, 0, 0, 0, 0], [4.5, 5.25, 6.125, 0, 0, 0], [4, 5, 6, 0, 0, 0], [6, 9, 14, 0, 0, 0]]) * 0.97
    np.testing.assert_array_equal(got, want)
    # src/gato_mpc_batch_sample.py:291-298: the winner's row is perturbed like the others
    got = resample(rows, 2, noise, keep_best=False, decay=1.0)
    want = np.array([[0, 0, 0, 0, 0, 0], [4.5, 5.25, 6.125, 0, 0, 0], [5, 6, 7, 0, 0, 0], [6, 9, 14, 0, 0, 0]], float)
    np.testing.assert_array_equal(got, want)
    # winner 0: everything collapses onto the zero hypothesis plus noise
    got = resample(rows, 0, noise, keep_best=True, decay=1.0)
    np.testing.assert_array_equal(got[1:, :3], noise[1:])
    assert not got[0].any() and not got[:, 3:].any()
    np.testing.assert_array_equal(rows[2], [4, 5, 6, 7, 8, 9])  # the input is not modified


def _near(q_end):
    x = np.zeros(12)
    x[:6] = np.asarray(q_end) + 0.01
    return x


def test_group_near_endpoint_0_switches_goals():
    G, H, N, steps = 2, 2, 8, 3
    q0 = np.full(6, 0.3)
    ends = np.array([rbd.eepos(q0), rbd.eepos(np.full(6, 0.9))])
    xs = np.stack([_near(q0), np.concatenate([np.full(6, -0.4), np.zeros(6)])])
    r = run_sampled_ref(N, G, H, xs, ends, steps, np.zeros((G * H, 6)), np.zeros((G, 6)), sim_dt=0.01)
    assert r["dist"][0, 0] < 0.095            # recorded against the goal before the switch
    assert r["dist"][1, 0] > 0.095            # then measured against endpoint 1
    assert abs(r["dist"][1, 0] - np.linalg.norm(rbd.eepos(r["q"][1, 0]) - ends[1])) < 1e-15
    assert abs(r["dist"][1, 1] - np.linalg.norm(rbd.eepos(r["q"][1, 1]) - ends[0])) < 1e-15  # group 1 did not switch
    assert np.isfinite(r["dist"]).all() and (r["best"] >= 0).all()


def test_single_endpoint_group_stops_at_step_0():
    G, H, N, steps = 2, 2, 8, 3
    q0 = np.full(6, 0.3)
    ends = np.array([rbd.eepos(q0)])
    xs = np.stack([_near(q0), np.concatenate([np.full(6, -0.4), np.zeros(6)])])
    r = run_sampled_ref(N, G, H, xs, ends, steps, np.zeros((G * H, 6)), np.zeros((G, 6)), sim_dt=0.01)
    assert r["dist"][0, 0] < 0.095 and np.isfinite(r["q"][0, 0]).all()   # the stopping step's plant is recorded
    assert np.isnan(r["dist"][1:, 0]).all() and np.isnan(r["q"][1:, 0]).all()
    assert (r["best"][:, 0] == -1).all() and np.isnan(r["fbest"][:, 0]).all()  # it never selected
    assert np.isfinite(r["dist"][:, 1]).all() and (r["best"][:, 1] == 0).all()
