#!/usr/bin/env python3
"""Generate tests/golden/filter3d_caller.npz: the REFERENCE's own GaussianModel.compute_3D_filter (wildgaussians/method.py:1140-1190),
called unbound on CPU tensors with a stub that has `xyz`, `filter_3D` and `register_buffer`, on cameras built with
wildgaussians.types.new_cameras -- for tests/test_filter3d.py.

Run where the reference checkout lies (tests/real_caller/reference_caller.py), on the CPU; the four inert stand-ins of make_golden.py
cover the packages the module imports and does not exercise here:

    python tests/golden/make_filter3d_golden.py

Stored: the inputs (xyz, poses, intrinsics, image_sizes), the per-camera R, T the reference formed (every float32 tensor it made
from a numpy array, in order: R, T, R, T, ...) and its filter_3D.  The scene: 8192 points, 12 cameras of mixed sizes with off-centre
principal points, four of them inside the cloud (part of it lies behind them), narrow enough that some points are seen by nobody.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "real_caller"))
P, C, SEED = 8192, 12, 20


def look_at(pos, target, rng):
    z = target - pos
    z /= np.linalg.norm(z)
    a = rng.standard_normal(3)
    x = np.cross(a, z)
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], axis=1), pos[:, None]], axis=1)


def scene():
    rng = np.random.default_rng(SEED)
    xyz = (rng.standard_normal((P, 3)) * np.array([3.0, 2.0, 3.0])).astype(np.float32)
    poses, intr, sizes = [], [], []
    for k in range(C):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        radius = rng.uniform(0.5, 2.0) if k % 3 == 2 else rng.uniform(3.0, 9.0)
        poses.append(look_at(d * radius, rng.normal(0.0, 0.1, 3), rng))
        w, h = int(rng.choice([640, 800, 1024])), int(rng.choice([480, 600, 768]))
        fx = rng.uniform(700.0, 1200.0)
        intr.append([fx, fx * rng.uniform(0.95, 1.05), w / 2 + rng.normal(0.0, 20.0), h / 2 + rng.normal(0.0, 20.0)])
        sizes.append([w, h])
    return xyz, np.asarray(poses, np.float32), np.asarray(intr, np.float32), np.asarray(sizes, np.int32)


def main():
    import make_golden
    import reference_caller as rc
    make_golden._install_shims()
    sys.path.insert(0, rc.PARENT)
    from wildgaussians import method as ref
    from wildgaussians.types import camera_model_to_int, new_cameras
    xyz, poses, intr, sizes = scene()
    cams = new_cameras(poses=poses, intrinsics=intr, camera_models=np.full((C,), camera_model_to_int("pinhole"), dtype=np.int32),
                       distortion_parameters=np.zeros((C, 0), dtype=np.float32), image_sizes=sizes, nears_fars=None)
    stub = types.SimpleNamespace(xyz=torch.from_numpy(xyz), filter_3D=torch.zeros(P, 1))
    stub.register_buffer = lambda name, t: setattr(stub, name, t)
    formed, real = [], torch.tensor

    def spy(data, *a, **k):
        t = real(data, *a, **k)
        if isinstance(data, np.ndarray):
            formed.append(t.numpy().copy())
        return t
    torch.tensor = spy
    try:
        ref.GaussianModel.compute_3D_filter(stub, cams)
    finally:
        torch.tensor = real
    assert len(formed) == 2 * C and stub.filter_3D.shape == (P, 1) and stub.filter_3D.dtype == torch.float32
    f = stub.filter_3D.numpy()
    unseen = float((f == f.max()).mean())
    assert unseen >= 0.01, unseen
    np.savez(os.path.join(HERE, "filter3d_caller.npz"), xyz=xyz, poses=poses, intrinsics=intr, image_sizes=sizes,
             R=np.stack(formed[0::2]), T=np.stack(formed[1::2]), filter_3D=f)
    print("filter3d_caller.npz:", {"P": P, "C": C, "share at the fill value": unseen})


if __name__ == "__main__":
    main()
