"""The dense second robot of the test suite (helper, no tests): tests/golden/dense6.json.

Indy7 is a forgiving input for the runtime-model kernels: its gravity is (0, 0, -9.81), two of its
six joint rotations are the identity and the other four signed permutations, 7 of its 18 placement
translations are exactly 0 and every limit is symmetric, so a wrong index, a transposed entry or a
swapped bound in a model read can multiply a zero and never show.  dense6.json is a 6-joint
revolute-z chain with the same keys as indy7_mpc_amd/params/indy7.json in which every number the
kernels read is non-zero and differs in magnitude from its neighbours (validity:
tests/test_dense_robot_host.py).

The committed JSON is what the tests read.  generate() is the seeded generator it came from, so the
file can be regenerated and audited:  python tests/dense_robot.py  rewrites it, bit for bit.

    dense_model()   RobotModel of the dense robot (what lib.Handle takes)
    dense_params()  rbd.Params of it (the oracle's P)
    dense_oracle    function-scoped fixture: oracle.rbd.PARAMS_PATH and oracle.rbd._P point at the
                    dense robot, so every reference that takes its model from rbd.params() (or, the
                    C++ port, from rbd.PARAMS_PATH through cpu.model_packed) runs on it unchanged;
                    restored after the test.  Import it into the test module that uses it.
"""
import json
import os

import numpy as np
import pytest

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense6.json")
SEED = 20260611
GRAVITY = [1.3, -0.8, -9.6]  # tilted: g[0] and g[1] are read with a non-zero value


def dense_model():
    from indy7_mpc_amd.model import RobotModel, load_params
    return RobotModel(load_params(PATH))


def dense_params():
    from oracle import rbd
    return rbd.Params(PATH)


@pytest.fixture
def dense_oracle(monkeypatch):
    """The oracle's default model is the dense robot for this test; returns its rbd.Params."""
    from oracle import rbd
    P = rbd.Params(PATH)
    monkeypatch.setattr(rbd, "PARAMS_PATH", PATH)
    monkeypatch.setattr(rbd, "_P", P)
    return P


# ---- what "dense" means (asserted on the committed file by tests/test_dense_robot_host.py) ---------
def distinct(x, rel=0.01):
    """No two entries of x equal in magnitude to within rel (of the larger)."""
    a = np.sort(np.abs(np.asarray(x, float).ravel()))
    return bool(np.all(a[1:] - a[:-1] > rel * a[1:]))


def sym6(I):
    """The six distinct entries of a symmetric 3x3: xx, xy, xz, yy, yz, zz (i7m_model's order)."""
    I = np.asarray(I, float)
    return np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


def _rotation(rng):
    """A proper rotation with every entry's magnitude in [0.05, 0.99] and no two alike."""
    while True:
        Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 2] = -Q[:, 2]
        a = np.abs(Q)
        # margins (0.06, 0.98, 2 %) inside the asserted ones, so rounding cannot cross them
        if a.min() >= 0.06 and a.max() <= 0.98 and distinct(Q, 0.02):
            return Q


def _vector(rng, lo, hi, digits):
    """Three signed numbers with magnitudes in [lo, hi], rounded, no two alike."""
    while True:
        x = np.round(rng.uniform(lo, hi, 3) * rng.choice([-1.0, 1.0], 3), digits)
        if np.abs(x).min() >= lo and distinct(x, 0.02):
            return x


def _inertia(rng, m, r):
    """A symmetric positive-definite rotational inertia of a body of mass m and size about r:
    principal moments of a box (so they satisfy the triangle inequality), axes turned by a dense
    rotation, all six entries non-zero and no two alike."""
    while True:
        a, b, c = r * rng.uniform(0.6, 1.6, 3)  # half-extents
        p = m / 3.0 * np.array([b * b + c * c, a * a + c * c, a * a + b * b])
        Q = _rotation(rng)
        I = Q @ np.diag(p) @ Q.T
        I = np.round(0.5 * (I + I.T), 8)
        e = sym6(I)
        w = np.linalg.eigvalsh(I)
        if np.abs(e).min() >= 1e-5 and distinct(e, 0.02) and w[0] > 0 and w[0] + w[1] > 1.02 * w[2]:
            return I


def generate(seed=SEED):
    """The parameter dict of dense6.json from a fixed seed."""
    rng = np.random.default_rng(seed)
    mass = [9.4, 6.1, 3.7, 2.3, 1.45, 0.62]  # decreasing down the chain, like a real arm
    size = [0.12, 0.11, 0.09, 0.07, 0.055, 0.04]
    out = dict(joint_names=[f"joint{j}" for j in range(6)], placement_R=[], placement_t=[], mass=[], com=[],
               inertia_com=[])
    for j in range(6):
        out["placement_R"].append(_rotation(rng).tolist())
        out["placement_t"].append(_vector(rng, 0.03, 0.32, 4).tolist())
        out["mass"].append(float(np.round(mass[j] * rng.uniform(0.97, 1.03), 4)))
        out["com"].append(_vector(rng, 0.008, 1.2 * size[j], 5).tolist())
        out["inertia_com"].append(_inertia(rng, out["mass"][j], size[j]).tolist())
    # limits: no interval symmetric about 0, none like another, each at least 3 rad wide
    # (synthetic_batch draws from half of it)
    out["q_lower"] = [-2.9, -1.7, -3.3, -2.2, -1.45, -3.6]
    out["q_upper"] = [2.1, 2.6, 1.9, 3.1, 2.75, 2.4]
    out["v_limit"] = [2.3, 2.6, 2.9, 3.1, 3.4, 3.7]
    # (efforts a few times the torque that holds the arm against gravity, low enough that the u
    # rows of the box QP bind at the tests' linearisation points)
    out["effort_limit"] = [160.0, 185.0, 58.0, 44.0, 31.0, 7.5]
    out["gravity"] = list(GRAVITY)
    out["name"] = "dense6"
    out["source"] = f"generated by tests/dense_robot.py generate(seed={seed}); a test fixture, not a real arm"
    return out


def write(path=PATH):
    with open(path, "w") as f:
        json.dump(generate(), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    write()
