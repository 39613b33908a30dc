"""CPU: utils.figure8 / figure_8, the controller's figure-8 reference trajectory
(gato_controller.py:316-320), against its definition: t = linspace(0, 2 pi, int(period / dt)),
the point (o_x + A_x sin t, o_y, o_z + A_z sin(2 t) / 2 + A_z / 2) rotated about z, rows
[x y z 0 0 0], flattened, tiled `cycles` times.  Also the default window schedule of
MPC_GATO_Batch_Sample.run_tracking."""
import numpy as np
import pytest

from indy7_mpc_amd.gato_mpc_batch_sample import tracking_schedule
from indy7_mpc_amd.utils import figure8, figure_8

A_X, A_Z, OFF = 0.5, 0.55, [0.1, 0.4, 0.45]


def _rz(a, p):
    c, s = np.cos(a), np.sin(a)
    return np.array([c * p[0] - s * p[1], s * p[0] + c * p[1], p[2]])


@pytest.mark.parametrize("period,dt,cycles", [(1.0, 0.01, 3), (10, 0.01, 1), (0.07, 0.01, 2)])
def test_length_and_zero_columns(period, dt, cycles):
    n = int(period / dt)
    tr = figure8(A_X, A_Z, OFF, period, dt, cycles)
    assert tr.shape == (6 * n * cycles,)
    pts = tr.reshape(-1, 6)
    assert not pts[:, 3:].any()
    # periodic tiling: every cycle is the first
    for c in range(cycles):
        np.testing.assert_array_equal(pts[c * n:(c + 1) * n], pts[:n])


def test_points_against_the_closed_form():
    """Five points per cycle: t = 0, pi/2, pi, 3 pi/2, 2 pi."""
    pts = figure8(A_X, A_Z, OFF, period=1.25, dt=0.25, cycles=2).reshape(-1, 6)[:, :3]
    assert pts.shape == (10, 3)
    a = np.pi / 4
    np.testing.assert_allclose(pts[0], _rz(a, [OFF[0], OFF[1], OFF[2] + A_Z / 2]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(pts[1], _rz(a, [OFF[0] + A_X, OFF[1], OFF[2] + A_Z / 2]), rtol=0, atol=1e-15)  # t = pi/2
    np.testing.assert_allclose(pts[2], _rz(a, [OFF[0], OFF[1], OFF[2] + A_Z / 2]), rtol=0, atol=1e-15)        # t = pi
    np.testing.assert_allclose(pts[3], _rz(a, [OFF[0] - A_X, OFF[1], OFF[2] + A_Z / 2]), rtol=0, atol=1e-15)
    # t = pi / 4: the top of the upper lobe
    p = figure8(A_X, A_Z, OFF, period=2.25, dt=0.25, cycles=1).reshape(-1, 6)[1, :3]
    np.testing.assert_allclose(p, _rz(a, [OFF[0] + A_X * np.sqrt(0.5), OFF[1], OFF[2] + A_Z]), rtol=0, atol=1e-15)


def test_angle_and_scalar_offset():
    """angle = 0 leaves the curve in the x-z plane through y = o_y; a scalar offset is all three."""
    pts = figure8(0.15, 0.15, 0, period=2.0, dt=0.01, cycles=2, angle=0.0).reshape(-1, 6)
    assert pts.shape == (400, 6) and not pts[:, 1].any()
    np.testing.assert_array_equal(pts[0, :3], [0.0, 0.0, 0.075])
    assert abs(pts[:, 0]).max() <= 0.15 and pts[:, 2].min() >= 0.0 and pts[:, 2].max() <= 0.15 + 1e-15


def test_ros_spelling_is_the_same_function():
    a = figure8(A_X, A_Z, OFF, period=1.0, dt=0.01, cycles=3)
    b = figure_8(A_X, A_Z, OFF, 0.01, 1.0, 3)
    np.testing.assert_array_equal(a, b)
    c = figure_8(x_amplitude=A_X, z_amplitude=A_Z, offset=OFF, timestep=0.01, period=1.0, num_periods=3, angle_offset=0.3)
    np.testing.assert_array_equal(c, figure8(A_X, A_Z, OFF, 1.0, 0.01, 3, angle=0.3))
    assert np.abs(c - a).max() > 0.01


def test_default_window_schedule_is_exact():
    """floor((i + 1) sim_dt / dt) in rational arithmetic: at sim_dt = dt / 10 the window moves at
    steps 9, 19, ... (accumulated floats reach 0.999... there); at sim_dt = dt every step."""
    n, off = tracking_schedule(0.001, 0.025, 0.01)
    assert n == 25 and off.dtype == np.int32
    np.testing.assert_array_equal(off, (np.arange(25) + 1) // 10)
    assert [i for i in range(1, 25) if off[i] != off[i - 1]] == [9, 19]
    n, off = tracking_schedule(0.01, 0.06, 0.01)
    assert n == 6
    np.testing.assert_array_equal(off, np.arange(1, 7))
    n, off = tracking_schedule(0.01, 0.29, 0.01)  # 0.29 / 0.01 is 28.999... in floats
    assert n == 29 and off[-1] == 29
    n, off = tracking_schedule(0.003, 0.03, 0.01)
    np.testing.assert_array_equal(off, [0, 0, 0, 1, 1, 1, 2, 2, 2, 3])
