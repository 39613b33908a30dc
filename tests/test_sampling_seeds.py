"""CPU: the random draws of the two sampled-wrench drop-ins (indy7_mpc_amd/_sampling.py) are part of
their behaviour: seed 3, batch_size 4, groups 2 must hand the library the hypotheses and the noise
recorded in tests/golden/sampling_seed3.npz (hyp (8, 6): the (4, 6) draw tiled over the groups; noise
(2, 8, 3): the first two steps), which were captured from the classes as they stood before the draws
moved into the shared module.  The draws are pure numpy, so a recording stand-in replaces the handle."""
import os

import numpy as np
import pytest

from indy7_mpc_amd import _lib, gato_controller, gato_mpc_batch_sample

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_seed3.npz"))
G, H, N = 2, 4, 8


class _Recorder:
    """What the classes call on a _lib.Handle, recording the hypotheses and the noise they pass."""
    seen = {}

    def __init__(self, model, N=32, **kw):
        self.T = 18 * N - 6

    def ctrl_begin(self, ref, fhyp, **kw):
        self.seen["hyp"] = np.array(fhyp)
        return np.zeros((kw["groups"], 6))

    def ctrl_step(self, x, elapsed, offset, noise=None):
        self.seen.setdefault("noise", []).append(np.array(noise))
        g = x.shape[0]
        return dict(u=np.zeros((g, 6)), best=np.zeros(g, np.int32), fbest=np.zeros((g, 6)), err=np.zeros(g),
                    ee=np.zeros((g, 3)))

    def mpc_run_sampled(self, xs, ends, num_steps, fhyp, fa, noise=None, **kw):
        self.seen["hyp"], self.seen["noise"] = np.array(fhyp), np.array(noise)
        g = xs.shape[0]
        return dict(dist=np.zeros((num_steps, g)), best=np.zeros((num_steps, g), np.int32), q=np.zeros((num_steps, g, 6)),
                    fbest=np.zeros((num_steps, g, 6)), xcur=np.zeros((g, 12)), xu_best=np.zeros((g, self.T)),
                    fhyp=np.array(fhyp))


@pytest.fixture
def seen(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _Recorder)
    monkeypatch.setattr(_Recorder, "seen", {})
    return _Recorder.seen


def test_controller_draws(seen):
    c = gato_controller.GATO_Controller(np.zeros((50, 3)), batch_size=H, N=N, f_ext_std=10.0, f_ext_resample_std=2.0, seed=3,
                                        groups=G, model=object())
    for _ in range(2):
        c.step(np.zeros((G, 12)), 0.01)
    np.testing.assert_array_equal(seen["hyp"], GOLD["hyp"])
    np.testing.assert_array_equal(np.array(seen["noise"]), GOLD["noise"])
    np.testing.assert_array_equal(c.f_ext_batch, GOLD["hyp"][:H])


def test_closed_loop_draws(seen):
    m = gato_mpc_batch_sample.MPC_GATO_Batch_Sample(model=object(), N=N, batch_size=H, resample_f_ext=True, f_ext_std=10.0,
                                                    f_ext_resample_std=2.0, seed=3)
    m.run_mpc_groups(np.zeros((G, 12)), np.zeros((1, 3)), sim_dt=0.01, sim_time=0.02)
    np.testing.assert_array_equal(seen["hyp"], GOLD["hyp"])
    np.testing.assert_array_equal(seen["noise"], GOLD["noise"])


def test_no_draw_without_a_spread():
    """f_ext_std = 0 draws nothing: the generator is where the seed left it."""
    rng = np.random.default_rng(3)
    from indy7_mpc_amd import _sampling
    assert not _sampling.initial_hypotheses(rng, H, 0.0).any()
    assert rng.normal() == np.random.default_rng(3).normal()
