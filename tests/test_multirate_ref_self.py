"""CPU: the multi-rate loop's Python schedule (indy7_mpc_amd._lib.multirate_schedule) against a
literal transcription of the reference's while-loop (src/gato_mpc_batch.py:171-199), and the numpy
loop the GPU parity tests compare against (tests/multirate_mpc_ref.py) on the events those tests
rely on: instance 0 switches its goal at step 0 and stops at step 1."""
import numpy as np
import pytest

from indy7_mpc_amd._lib import MULTIRATE_MAX_SUB, multirate_schedule
from multirate_mpc_ref import make_case, run_multirate_ref


def _literal(solver_dt, sim_dt, num_steps):
    """The reference's loop with its names: per MPC step the timesteps and sim_steps."""
    time_accumulated = 0.0
    steps = []
    for _ in range(num_steps):
        sim_time_step = sim_dt
        sim_steps = 0
        timesteps = []
        while sim_time_step > 0:
            timestep = min(sim_time_step, solver_dt - time_accumulated)
            assert int(time_accumulated / solver_dt) == 0  # current_interval: always knot 0
            time_accumulated += timestep
            sim_time_step -= timestep
            timesteps.append(timestep)
            if abs(time_accumulated - solver_dt) < 1e-10:
                sim_steps += 1
                time_accumulated = 0.0
        steps.append((timesteps, sim_steps))
    return steps


@pytest.mark.parametrize("dt,sim_dt,num_steps", [(0.01, 0.001, 50), (0.01, 0.004, 20), (0.01, 0.02, 10), (0.01, 0.025, 10),
                                                 (0.015, 0.02, 12), (0.01, 0.0123, 30)])
def test_schedule_equals_the_literal_loop(dt, sim_dt, num_steps):
    sub_start, sub_dt, shift = multirate_schedule(dt, sim_dt, num_steps)
    lit = _literal(dt, sim_dt, num_steps)
    assert sub_start[0] == 0 and len(sub_start) == num_steps + 1 and len(shift) == num_steps
    for i, (timesteps, sim_steps) in enumerate(lit):
        assert sub_dt[sub_start[i]:sub_start[i + 1]].tolist() == timesteps  # bit for bit, residues included
        assert shift[i] == sim_steps
    assert sub_start[-1] == len(sub_dt) == sum(len(t) for t, _ in lit)


def test_schedule_residues_and_refusals():
    ss, sd, sh = multirate_schedule(0.01, 0.001, 10)
    assert ss.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11] and sh.tolist() == [0] * 9 + [1]
    assert sd[9] == 0.0009999999999999992 and sd[10] == 8.673617379884035e-19
    assert multirate_schedule(0.01, 0.025, 2)[2].tolist() == [2, 3]
    assert multirate_schedule(0.015, 0.02, 5)[2].tolist() == [1, 1, 2, 1, 1]
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sim_dt"):
            multirate_schedule(0.01, bad, 3)
    with pytest.raises(ValueError, match="N - 1 = 7"):
        multirate_schedule(0.01, 0.2, 3, N=8)
    with pytest.raises(ValueError, match=f"more than {MULTIRATE_MAX_SUB}"):
        multirate_schedule(0.01, 0.661, 2, N=64)


def test_reference_loop_switches_at_step_0_and_stops_at_step_1():
    """(N, steps, dt, sim_dt, radius, control) = (8, 6, .01, .02, .1, PREV), direct: instance 0
    records d < 0.1 at step 0 (switch; the plant runs) and at step 1 (the last endpoint: stop, no
    plant), and NaN from step 2 on; the others run to the end."""
    xs, ends = make_case()
    r = run_multirate_ref(8, xs, ends, 6, dt=0.01, sim_dt=0.02, radius=0.1, control="prev")
    assert r["dist"][0, 0] < 0.1 and r["dist"][1, 0] < 0.1
    assert np.isfinite(r["q"][0, 0]).all() and np.isnan(r["q"][1:, 0]).all()
    assert np.isnan(r["dist"][2:, 0]).all() and np.isnan(r["u"][2:, 0]).all()
    assert np.isfinite(r["xpath"][:2, 0]).all() and np.isnan(r["xpath"][2:, 0]).all()
    assert np.isfinite(r["dist"][:, 1:]).all() and np.isfinite(r["xpath"][:, 1:]).all()
    assert np.nanmin(r["margin"]) >= 1e-3
    np.testing.assert_array_equal(r["u"][0], r["u0"])
    np.testing.assert_array_equal(r["xcur"][0, :6], r["q"][0, 0])
    np.testing.assert_array_equal(r["xu"][:, :12], r["xcur"])
    np.testing.assert_array_equal(r["xu"][:, -12:], np.tile([1.0] * 6 + [0.0] * 6, (4, 1)))
