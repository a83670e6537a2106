#!/usr/bin/env python3
"""The projection-only pass (GaussianRasterizer.project_radii / wg_project_radii) on one MI355X, and the appearance path it exists for, in
ONE process, the legs alternating call by call.

usage: python scripts/bench_project_radii.py [--configs 1000000x1920x1080,3000000x1600x1200] [--views 8] [--samples 30] [--out FILE] [--commit ID]

Frames: wg_scenes.make_cloud(P, W, H, sh_degree=3, seed=0) through the cameras of bench.py's sequence (the base camera yawed by k * 5 degrees,
k = 0 .. views - 1); the visible fraction (radii > 0).mean() of each frame is recorded.  Per frame:
    pass       project_radii alone, beside the SAME frame's preprocess stage time (wg_profile_read over forward calls with plain SH colours,
               forward only; the stage's own device events)
    A          dense appearance MLP (3 + 24 wide inputs, shared 32-wide embedding) + ONE two-tone call (sh_second=True): today's single-call path
    B          raw call with precomputed colours + geometry_reuse + VisibleRows.from_radii + the MLP over the rows + toned call with precomputed
               colours (fused eval_sh for both colour sets): today's row path
    C          VisibleRows.from_camera + the MLP over the rows + ONE two-tone call
A, B and C are forward + backward of a sum loss over both images, gradients to features, embeddings, weights and geometry.  Every call is timed
by its own pair of device events after a warm-up of all legs; one round visits every leg once; median, p10 and p90 over --samples rounds.
No speed gate.  No GPU: an error, no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import appearance_mlp_lib as L  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402
import wg_scenes as S  # noqa: E402
import wg_viewparallel as VP  # noqa: E402
from bench_appearance_mlp import one_ms, stats  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _C  # noqa: E402
from wg_testlib import make_settings, to_dev  # noqa: E402

G, E, DEG = 24, 32, 3
C0 = 0.28209479177387814


def bench_frame(cloud_dev, cam, samples, yaw):
    P = cloud_dev["means3D"].shape[0]
    rs = make_settings(cam, DEG)
    rast = GaussianRasterizer(rs)
    g = torch.Generator().manual_seed(P)
    geom = {k: cloud_dev[k].detach().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    geom["means2D"] = torch.zeros_like(geom["means3D"], requires_grad=True)
    feats = cloud_dev["shs"].reshape(P, 48).detach().clone().requires_grad_(True)
    gemb = (torch.rand(P, G, generator=g) * 2 - 1).cuda().requires_grad_(True)
    aemb = (torch.randn(E, generator=g) * 0.3).cuda().requires_grad_(True)
    Wt = [w.cuda().requires_grad_(True) for w in L.draw_weights(3 + G + E, 1)]
    leaves = [feats, gemb, aemb] + Wt + list(geom.values())

    def tone(rows):
        return torch.split(FG.appearance_mlp((feats[:, :3], gemb), Wt, shared=aemb, rows=rows), [3, 3], dim=-1)

    def two_tone(rows):
        offset, mul = tone(rows)
        toned, _, _, plain = rast(shs=feats.view(P, 16, 3), sh_mul=mul, sh_offset=offset / C0, sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0,
                                  sh_second=True, sh_pre_clamp_max2=1.0, **geom)
        return toned.sum() + plain.sum()

    def colours(f48):
        dirs = torch.nn.functional.normalize(geom["means3D"].detach() - rs.campos[None], dim=-1)
        return (FG.eval_sh(DEG, f48.view(P, 16, 3).transpose(1, 2), dirs) + 0.5).clamp_min(0.0)

    def leg_a():
        return two_tone(None)

    def leg_b():
        plain, radii, _ = rast(colors_precomp=colours(feats.clamp_max(1.0)), **geom)
        offset, mul = tone(FG.VisibleRows.from_radii(radii))
        toned48 = (feats * mul.repeat(1, 16) + torch.cat((offset / C0, torch.zeros_like(feats[:, 3:])), dim=-1)).clamp_max(1.0)
        toned, _, _ = rast(colors_precomp=colours(toned48), **geom)
        return toned.sum() + plain.sum()

    def leg_c():
        return two_tone(FG.VisibleRows.from_camera(rast, geom["means3D"], geom["scales"], geom["rotations"]))

    def fb(fn, reuse):
        def run():
            _C.set_option("geometry_reuse", reuse)
            return torch.autograd.grad(fn(), leaves, allow_unused=True)
        return run

    def the_pass():
        return rast.project_radii(geom["means3D"], geom["scales"], geom["rotations"])
    calls = {"pass": the_pass, "A": fb(leg_a, 0), "B": fb(leg_b, 1), "C": fb(leg_c, 0)}
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    hits = _C.geometry_reuse_hits()
    times = {k: [] for k in calls}
    for _ in range(samples):
        for k, fn in calls.items():
            times[k].append(one_ms(fn))
    hits = _C.geometry_reuse_hits() - hits
    _C.set_option("geometry_reuse", 0)
    # the same frame's preprocess stage, by the library's own per-stage device events
    radii = the_pass()
    _C.profile_enable(True)
    _C.profile_reset()
    with torch.no_grad():
        for _ in range(samples):
            fwd_radii = rast(shs=feats.view(P, 16, 3), **{k: v.detach() for k, v in geom.items()})[1]
    torch.cuda.synchronize()
    prof = _C.profile_read()
    _C.profile_enable(False)
    pre_ms, pre_n = prof["preprocess"]
    res = {k: stats(v) for k, v in times.items()}
    return {"yaw_deg": yaw, "visible_fraction": round(float((radii > 0).float().mean()), 4), "radii_equal_the_forward_calls": bool(torch.equal(radii, fwd_radii)),
            "pass": res["pass"],
            "preprocess_stage_of_the_same_frame": {"mean_ms_per_frame": round(pre_ms / samples, 4), "launches_per_frame": round(pre_n / samples, 2)},
            "A_dense_mlp_two_tone_call": res["A"], "B_two_calls_geometry_reuse_rows": dict(res["B"], geometry_reuse_hits_per_call=round(hits / samples, 2)),
            "C_from_camera_rows_two_tone_call": res["C"],
            "A_over_C_median": round(res["A"]["median_ms"] / res["C"]["median_ms"], 3), "B_over_C_median": round(res["B"]["median_ms"] / res["C"]["median_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000000x1920x1080,3000000x1600x1200")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_project_radii.py needs a HIP device")
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    configs = []
    for spec in (s for s in a.configs.split(",") if s):
        P, W, H = (int(x) for x in spec.split("x"))
        cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=DEG, seed=0).items()}
        frames = []
        for k, cam in enumerate(VP.view_cameras(a.views, W, H)):
            frames.append(bench_frame(cloud, cam, a.samples, 5.0 * k))
            print(json.dumps({"P": P, "W": W, "H": H, **frames[-1]}), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        configs.append({"P": P, "width": W, "height": H, "scene": f"wg_scenes.make_cloud({P}, {W}, {H}, sh_degree=3, seed=0)", "frames": frames})
        del cloud
        torch.cuda.empty_cache()
    line = {"device": torch.cuda.get_device_name(0), "commit": commit, "arguments": {"configs": a.configs, "views": a.views, "samples": a.samples},
            "metric": "project_radii", "widths": "3 + 24 + 32 -> 128 -> 128 -> 6",
            "timing": "one pair of device events per call after a warm-up; one round visits every leg once; median / p10 / p90 over the rounds; "
                      "the preprocess stage: the library's per-stage device events, mean over the same number of forward calls",
            "legs": {"pass": "GaussianRasterizer.project_radii alone",
                     "A": "dense appearance MLP + one two-tone call (sh_second=True), forward + backward",
                     "B": "raw call (precomputed colours) + geometry_reuse + VisibleRows.from_radii + MLP over rows + toned call, forward + backward",
                     "C": "VisibleRows.from_camera + MLP over rows + one two-tone call, forward + backward"},
            "gate": "none: recorded, not gated", "configs": configs}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
