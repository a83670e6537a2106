#!/usr/bin/env python3
"""What a frame's depth image costs on one MI355X, three ways, in ONE process, the legs alternating call by call.

usage: python scripts/bench_render_depth.py [--configs 1000000x1920x1080,3000000x1600x1200] [--samples 30] [--out FILE] [--commit ID]

Frames: wg_scenes.make_cloud(P, W, H, sh_degree=None, seed=0) through the base camera, precomputed colours, forward only (torch.no_grad()).
    plain   the colour call alone: what every leg below contains
    A       the caller's way (method.py:1621-1631): the colour call, torch.norm(means3D - campos) repeated to [P, 3], a second full call through
            the same rasterizer (an all-zero background) with those as colours, one channel kept
    B       the same with geometry_reuse = 1: the second call is a recolouring of the first frame (no projection, binning or sort)
    C       ONE call with return_depth="distance"
The cost of depth is each leg's time minus the plain call's.  Every call is timed by its own pair of device events after a warm-up of all legs;
one round visits every leg once; median, p10 and p90 over --samples rounds.  Launches: the library's per-stage launch counts over one call of
each leg (wg_profile_read; torch's own kernels -- norm, repeat -- are not in them and are listed apart).  Peak memory: the allocator's peak above what is
allocated before the call (the inputs).  The three depth images are compared: C against A's and B's within the distance mode's bound.
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
import wg_scenes as S  # noqa: E402
from bench_appearance_mlp import one_ms, peak_above_inputs, stats  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _C  # noqa: E402
from wg_testlib import make_settings, to_dev  # noqa: E402


def bench_config(P, W, H, samples):
    cam = S.make_camera(W, H)
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=0).items()}
    rs = make_settings(cam, 0)   # an all-zero background, the caller's: its depth call goes through the SAME rasterizer object as its colour call
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"])
    rast = GaussianRasterizer(rs)

    def plain():
        return rast(colors_precomp=cloud["colors_precomp"], **geo)

    def two_calls():
        out = rast(colors_precomp=cloud["colors_precomp"], **geo)
        dist = torch.norm(cloud["means3D"] - rs.campos[None], dim=-1).unsqueeze(-1).repeat(1, 3)
        return out, rast(colors_precomp=dist, **geo)[0][0]

    def leg(fn, reuse):
        def run():
            _C.set_option("geometry_reuse", reuse)
            with torch.no_grad():
                return fn()
        return run
    calls = {"plain": leg(plain, 0), "A": leg(two_calls, 0), "B": leg(two_calls, 1),
             "C": leg(lambda: rast(colors_precomp=cloud["colors_precomp"], return_depth="distance", **geo), 0)}
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
    res = {k: stats(v) for k, v in times.items()}
    # launches of the library per call, and the allocator's peak above the inputs
    launches, peaks = {}, {}
    for k, fn in calls.items():
        _C.profile_enable(True)
        _C.profile_reset()
        fn()
        torch.cuda.synchronize()
        launches[k] = {s: n for s, (_ms, n) in _C.profile_read().items() if n}
        _C.profile_enable(False)
        peaks[k] = int(peak_above_inputs(fn))
    # the three depth images
    d_a, d_b, d_c = calls["A"]()[1], calls["B"]()[1], calls["C"]()[-1]
    _C.set_option("geometry_reuse", 0)
    R, _c, _r, _g, _b, ib = _C.rasterize_gaussians(rs.bg, cloud["means3D"], cloud["colors_precomp"], cloud["opacities"], cloud["scales"], cloud["rotations"], 1.0,
                                                   torch.Tensor([]), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset,
                                                   H, W, torch.Tensor([]), 0, rs.campos, False, False)
    n = int(_C.view_image(ib, H, W)["tile_last"].max())
    bound = (2 * n + 7) * 2.0 ** -24 * d_a.double()
    med = {k: v["median_ms"] for k, v in res.items()}
    out = {"P": P, "width": W, "height": H, "scene": f"wg_scenes.make_cloud({P}, {W}, {H}, sh_degree=None, seed=0)", "num_rendered": int(R),
           "longest_walked_list": n, "plain_call": res["plain"], "A_norm_repeat_second_full_call": res["A"],
           "B_same_with_geometry_reuse": dict(res["B"], geometry_reuse_hits_per_call=round(hits / samples, 2)), "C_one_call_return_depth": res["C"],
           "cost_of_depth_median_ms": {k: round(med[k] - med["plain"], 4) for k in ("A", "B", "C")},
           "library_launches_per_call": launches,
           "torch_kernels_beside_them": {"A": "sub, norm, repeat", "B": "sub, norm, repeat", "C": "none", "plain": "none"},
           "peak_bytes_above_inputs": peaks,
           "depth_images": {"A_equals_B": bool(torch.equal(d_a, d_b)), "C_within_the_distance_bound_of_A": bool(((d_c.double() - d_a.double()).abs() <= bound).all()),
                            "largest_relative_difference_C_to_A": float(((d_c.double() - d_a.double()).abs() / d_a.double().clamp_min(1e-30))[d_a > 0].max())}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000000x1920x1080,3000000x1600x1200")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_depth.py needs a HIP device")
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    configs = []
    for spec in (s for s in a.configs.split(",") if s):
        P, W, H = (int(x) for x in spec.split("x"))
        configs.append(bench_config(P, W, H, a.samples))
        print(json.dumps(configs[-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    line = {"device": torch.cuda.get_device_name(0), "commit": commit, "binding": _C.binding_name(), "arguments": {"configs": a.configs, "samples": a.samples},
            "metric": "render_depth",
            "timing": "forward only (torch.no_grad()); one pair of device events per call after a warm-up of all legs; one round visits every leg once; "
                      "median / p10 / p90 over the rounds",
            "legs": {"plain": "the colour call alone", "A": "colour call + torch.norm + repeat(1, 3) + a second full call over a zero background, one channel kept",
                     "B": "A with geometry_reuse = 1: the second call recolours the first frame", "C": 'one call with return_depth="distance"'},
            "gate": "none: recorded, not gated", "configs": configs}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
