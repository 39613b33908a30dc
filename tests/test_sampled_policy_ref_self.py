"""CPU: tests/sampled_policy_ref.py, the numpy restatement of the multi-rate sampled-wrench loops
under the winner's feedback policy, checked on itself, and the conditions its cases
(policy_case: the inputs of tests/test_gpu_sampled_policy.py's parity tests) have to meet before a
GPU is involved: the selected hypothesis, the goal switch and the stop are discrete, so a parity
test must know how far from a tie they are.  The device-vs-host noise of these loops is at most 5e-7
(DESIGN.md §4.11); 1e-3 is three orders clear of it."""
import numpy as np
import pytest

from oracle import rbd
from sampled_multirate_ref import run_sampled_multirate_ref
from sampled_policy_ref import (G, H, N, SHAPES, loop_kwargs, policy_case, policy_reference, replay_score,
                                run_sampled_policy_ref)

GAP = 1e-3
OUT = ("best", "q", "u", "xpath", "fbest", "xcur", "xu_best", "fhyp", "err2", "sub_start", "shift")


@pytest.mark.parametrize("source", ["endpoints", "tracking"])
def test_zero_gains_and_one_substep_is_the_multirate_loop(source):
    """K = 0 and one sub-step per step (sim_dt = 0.001, steps 0 .. 8: every sub-step alone in knot 0):
    the control is XU_best's first and the replay is the one rk4 step of sim_dt, so the loop is
    run_sampled_multirate_ref's, value for value."""
    c = policy_case(source, 0.001)
    args = (N, G, H, c["xstart"], 9, c["fhyp"], c["f_actual"])
    kw = loop_kwargs(c)
    kw["noise"] = c["noise"][:9]
    for mode in ("direct", "admm"):
        got = run_sampled_policy_ref(*args, qp_mode=mode, gains="zero", **kw)
        want = run_sampled_multirate_ref(*args, qp_mode=mode, **kw)
        assert (np.diff(got["sub_start"]) == 1).all() and int(got["jmax"]) == 0
        for key in OUT + (("dist", "margin") if source == "endpoints" else ("err", "ee", "off")):
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{mode} {key}")


def test_the_true_hypothesis_replays_to_zero():
    """A hypothesis equal to the actual wrench replays the plant's own arithmetic: error exactly 0 on a
    step of three sub-steps, where the one-step score of the multi-rate loop is small but not 0."""
    c = policy_case("tracking", 0.025)
    r = run_sampled_policy_ref(N, G, H, c["xstart"], 1, c["fhyp"], c["f_actual"], ref=c["ref"], ref_phase=c["ref_phase"],
                               sim_dt=0.025)
    assert r["sub_start"][1] == 3
    np.testing.assert_array_equal(r["best"][0], c["k"])
    np.testing.assert_array_equal(r["err2"][0, :, 0], 0.0)
    one = run_sampled_multirate_ref(N, G, H, c["xstart"], 1, c["fhyp"], c["f_actual"], ref=c["ref"],
                                    ref_phase=c["ref_phase"], sim_dt=0.025)
    assert (one["err2"][0, :, 0] > 0).all()
    # replay_score's tie rule: the lowest index among equal minima, a NaN never wins
    x = c["xstart"][0]
    rows = np.array([[np.nan] * 6, c["fhyp"][1], c["fhyp"][1]])
    us, dts = [np.zeros(6)], [0.01]
    q, v = rbd.rk4(x[:6], x[6:], us[0], dts[0], fext6_world=c["fhyp"][1])
    err, best = replay_score(x, us, dts, np.concatenate([q, v]), rows, "world")
    assert np.isnan(err[0]) and err[1] == err[2] == 0.0 and best == 1


@pytest.mark.parametrize("mode", ["direct", "admm"])
@pytest.mark.parametrize("sim_dt,steps", SHAPES)
@pytest.mark.parametrize("source", ["endpoints", "tracking"])
def test_the_cases_are_clear_of_every_tie(source, sim_dt, steps, mode):
    """In the chosen cases the two smallest scoring errors of every step and group are at least 1e-3
    apart, every goal distance is at least GAP from the radius, and the events the cases were chosen
    for occur: the goal switch and the stop (endpoints, group 0), j reaching 2 within a step
    (sim_dt = 0.025) and the residue sub-step of step 9 (sim_dt = 0.001)."""
    r = policy_reference(source, sim_dt, mode)
    ran = r["best"] >= 0
    gap = (r["err2"][:, :, 1] - r["err2"][:, :, 0])[ran]
    print(f"{source} sim_dt {sim_dt} {mode}: min gap {gap.min():.3g}, best {r['best'].T.tolist()}")
    assert np.isfinite(gap).all() and (gap >= 1e-3).all(), gap.min()
    d = r["dist" if source == "endpoints" else "err"]
    if source == "endpoints":
        margin = r["margin"][np.isfinite(r["margin"])]
        assert (margin >= GAP).all(), margin.min()
        # group 0: inside the radius of endpoint 0 at step 0 (the switch) and of endpoint 1 at step 1
        # (the stop); group 1 runs on
        assert d[0, 0] < 0.095 and d[1, 0] < 0.095 and np.isnan(d[2:, 0]).all()
        assert r["best"][0, 0] >= 0 and (r["best"][1:, 0] == -1).all() and np.isnan(r["fbest"][1:, 0]).all()
        assert np.isfinite(d[:, 1]).all() and (d[:, 1] > 0.095).all() and (r["best"][:, 1] >= 0).all()
    else:
        assert np.isfinite(d).all() and ran.all()
    if sim_dt == 0.025:
        assert int(r["jmax"]) >= 2 and (np.diff(r["sub_start"]) >= 3).all()
    else:
        assert r["sub_start"][10] - r["sub_start"][9] == 2 and r["shift"][9] == 1 and int(r["jmax"]) == 1
    # more than one row is selected over the run: kbuf is read at row `best`, not at a fixed row
    assert len(set(r["best"][:, 1].tolist())) > 1
