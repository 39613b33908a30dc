"""What the two sampled-wrench drop-ins (``MPC_GATO_Batch_Sample``, ``GATO_Controller``) check, parse
and draw the same way.  The draws keep their order and shapes: a given seed yields the same
hypotheses and the same noise in both classes."""
from __future__ import annotations

import numpy as np

from . import _lib

SIZES = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def qp_mode_of(batch_size, qp_mode):
    """The library's QP mode for 'direct' / 'admm', after the constructors' checks."""
    if batch_size not in SIZES:
        raise ValueError(f"Batch size {batch_size} not supported")
    if qp_mode not in ("direct", "admm"):
        raise ValueError("qp_mode must be 'direct' or 'admm'")
    return _lib.QP_ADMM if qp_mode == "admm" else _lib.QP_DIRECT


def initial_hypotheses(rng, batch_size, f_ext_std):
    """(batch_size, 6) world-frame wrench hypotheses: normal forces, torques 0, row 0 zero
    (src/gato_mpc_batch_sample.py:37-40, gato_controller.py:77-83); nothing is drawn for std 0."""
    if f_ext_std == 0.0:
        return np.zeros((batch_size, 6))
    f = rng.normal(0, f_ext_std, (batch_size, 6))
    f[:, 3:] = 0.0
    f[0] = 0.0
    return f


def resampling_noise(rng, std, *shape):
    """(*shape, 3) force perturbations: (*shape, 6) normals as the reference draws them per step,
    the torques dropped (src/gato_mpc_batch_sample.py:294-296)."""
    return rng.normal(0, std, (*shape, 6))[..., :3]


def reference_points(ref_traj):
    """ref_traj as (L, 3) or (L, 6): flat input has six entries per point (as utils.figure8 builds it)."""
    ref = np.asarray(ref_traj, float)
    if ref.ndim == 1:
        ref = ref.reshape(-1, 6)
    if ref.ndim != 2 or ref.shape[1] not in (3, 6) or ref.shape[0] < 1:
        raise ValueError("ref_traj must be flat with 6 entries per point, (L, 3) or (L, 6)")
    return ref
