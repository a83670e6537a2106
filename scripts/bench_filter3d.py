#!/usr/bin/env python3
"""compute_3D_filter on one MI355X: (a) a float32 PyTorch restatement of the reference's loop over the cameras
(wildgaussians/method.py:1140-1190), host parts included -- what a caller runs without the opt-in --, (b) the fused call with a prebuilt
CameraTable, (c) the fused call including the table's construction; the variants alternate inside ONE process.

usage: python scripts/bench_filter3d.py [--shapes 1000000x200,3000000x1000,100000x1000] [--rounds 3] [--out FILE] [--fused-only]

Times are host clock around work that ends in a device synchronise; (b) also by device events.  Every shape is warmed up; (b) is
repeated until its timed window is at least half a second, per round; (a) is slow, so `--rounds` (3) repeats of it suffice.  Reported
per shape: median and range of each variant, the pair rate P * C / t of (b), and how the two results compare (points whose values
differ by more than 1e-5 relative are visibility decisions at a limit falling the other way: tests/test_filter3d.py bounds them).
--fused-only: (b) alone, a few calls, for a `rocprofv3 --kernel-trace --stats` run of its own.  No GPU: an error, no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
import torch  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402

VALU_PER_PAIR = {"skip_path": 8, "full_path": 66}   # wave64 VALU instructions per camera in filter3d_distance_kernel's loop
ISSUE_CEILING = 538e9                                # wave-instructions / s measured on this part (profiles/r4/pk_probe.txt)


def scene(P, n_cams, seed=0):
    """The tests' recipe, vectorised: cloud N(0, diag(4, 2, 4)), cameras on radius 3 - 9 looking at the origin."""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((P, 3), dtype=np.float32) * np.sqrt([4.0, 2.0, 4.0]).astype(np.float32))
    d = rng.standard_normal((n_cams, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * rng.uniform(3.0, 9.0, (n_cams, 1))
    z = rng.normal(0.0, 0.1, (n_cams, 3)) - pos
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    x = np.cross(rng.standard_normal((n_cams, 3)), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    poses = np.stack([x, np.cross(z, x), z, pos], axis=2).astype(np.float32)
    w, h = rng.choice([640, 800, 1024], n_cams), rng.choice([480, 600, 768], n_cams)
    fx = rng.uniform(400.0, 1200.0, n_cams)
    intr = np.stack([fx, fx, w / 2 + rng.normal(size=n_cams), h / 2 + rng.normal(size=n_cams)], axis=1).astype(np.float32)
    return xyz, poses, intr, np.stack([w, h], axis=1).astype(np.int32)


@torch.no_grad()
def torch_loop(xyz, poses, intrinsics, image_sizes):
    """The reference's statements, in order, on the GPU in float32."""
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.
    for k in range(poses.shape[0]):
        fx, fy, _, _ = intrinsics[k]
        width, height = image_sizes[k]
        pose = np.copy(poses[k])
        pose = np.concatenate([pose, np.array([[0, 0, 0, 1]], dtype=pose.dtype)], axis=0)
        pose = np.linalg.inv(pose)
        R = np.transpose(pose[:3, :3])
        T = pose[:3, 3]
        R = torch.tensor(R, device=xyz.device, dtype=torch.float32)
        T = torch.tensor(T, device=xyz.device, dtype=torch.float32)
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + width / 2.0
        y = y / z * fy + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < fx:
            focal_length = fx
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (0.2 ** 0.5))[..., None]


def host_ms(fn, n=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x200,3000000x1000,100000x1000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter3d.py needs a HIP device")
    dev = torch.device("cuda", 0)
    rows = []
    for shape in a.shapes.split(","):
        P, n_cams = (int(s) for s in shape.split("x"))
        xyz_h, poses, intr, sizes = scene(P, n_cams)
        xyz = torch.from_numpy(xyz_h).to(dev)
        table = FG.CameraTable((poses, intr, sizes), device=dev)
        out = torch.empty(P, 1, device=dev)
        fused = lambda: FG.compute_3D_filter(xyz, table, out=out)  # noqa: E731
        fused_with_table = lambda: FG.compute_3D_filter(xyz, (poses, intr, sizes), out=out)  # noqa: E731
        for _ in range(3):
            fused()
        if a.fused_only:
            host_ms(fused, 10)
            continue
        fused_with_table()
        ref = torch_loop(xyz, poses, intr, sizes)   # warm-up of (a) and the comparison
        got = fused().clone()
        rel = ((got - ref).abs() / ref).reshape(-1)
        n_b = max(3, int(500.0 / max(host_ms(fused, 3), 1e-3)) + 1)   # (b): a window of at least half a second
        ta, tb, tb_ev, tc = [], [], [], []
        for _ in range(a.rounds):
            ta.append(host_ms(lambda: torch_loop(xyz, poses, intr, sizes)))
            tb.append(host_ms(fused, n_b))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_b):
                fused()
            e1.record()
            torch.cuda.synchronize()
            tb_ev.append(e0.elapsed_time(e1) / n_b)
            tc.append(host_ms(fused_with_table))
        b = stats(tb)
        rate = P * n_cams / (b["median_ms"] * 1e-3)
        rows.append({"P": P, "cameras": n_cams, "a_torch_loop": stats(ta), "b_fused_prebuilt_table": b, "b_fused_device_events": stats(tb_ev),
                     "b_calls_per_window": n_b, "c_fused_with_table_construction": stats(tc),
                     "speedup_b_over_a": round(stats(ta)["median_ms"] / b["median_ms"], 1),
                     "pair_rate_G_per_s": round(rate / 1e9, 2),
                     "valu_wave_instr_G_per_s_if_every_camera_skipped": round(rate / 64 * VALU_PER_PAIR["skip_path"] / 1e9, 2),
                     "share_of_issue_ceiling_at_skip_path_count": round(rate / 64 * VALU_PER_PAIR["skip_path"] / ISSUE_CEILING, 3),
                     "vs_torch": {"max_rel_diff": float(rel.max()), "points_over_1e-5": int((rel > 1e-5).sum())}})
        del xyz, out, ref, got
    line = {"metric": "compute_3D_filter", "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
            "valu_wave_instr_per_camera_from_isa": VALU_PER_PAIR, "issue_ceiling_wave_instr_per_s": ISSUE_CEILING,
            "note": "(a) is the behaviour without the opt-in; it is slow, so %d repeats" % a.rounds, "shapes": rows}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
