#!/usr/bin/env python3
"""What a distortion loss on a frame costs on one MI355X, forward + backward, three ways, in ONE process, the legs alternating call by call.

usage: python scripts/bench_distortion.py [--configs 1000000x1920x1080,3000000x1600x1200] [--samples 30] [--out FILE] [--commit ID]

Frames: wg_scenes.make_cloud(P, W, H, sh_degree=None, seed=0) through the base camera, precomputed colours; every geometry input and the colours
require grad; the step is forward + backward of <cot, image> (+ dist.mean()).  bench_render_depth_grad.py's protocol.
    plain   the step without the loss: what every leg below contains
    A       the only route there was, and the yardstick: the plain step's forward, v = torch.norm(means3D - campos), a second full three-channel
            call (an all-zero background) with colors_precomp = (1, v, v^2), A * Q - D * D formed in torch, and ONE backward over both calls
    B       the same with geometry_reuse = 1: the second call is a recolouring of the first frame
    C       ONE call with return_distortion="distance", distortion_grad=True: one more forward walk, one more backward walk into the same record
The cost of the loss is each leg's time minus the plain step's.  Every step is timed by its own pair of device events after a warm-up of all
legs; one round visits every leg once; median, p10 and p90 over --samples rounds.  Launches: the library's per-stage launch counts over one step
of each leg (wg_profile_read; torch's own kernels are not in them and are listed apart).  Peak memory: the allocator's peak above what is
allocated before the step (the inputs).  C's gradients are compared with A's (max-rel-err per input).
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
from wg_testlib import make_settings, rel_err, to_dev  # noqa: E402

LEAVES = ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp")


def bench_config(P, W, H, samples):
    cam = S.make_camera(W, H)
    t = {k: to_dev(v).requires_grad_(True) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=0).items()}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    rs = make_settings(cam, 0)   # an all-zero background: the moment call needs one, and both calls go through the SAME rasterizer object
    geo = dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    rast = GaussianRasterizer(rs)
    cot = to_dev(S.make_cotangent(W, H))

    def plain():
        rast(colors_precomp=t["colors_precomp"], **geo)[0].backward(cot)

    def two_calls():
        img = rast(colors_precomp=t["colors_precomp"], **geo)[0]
        v = torch.norm(t["means3D"] - rs.campos[None], dim=-1)
        m = rast(colors_precomp=torch.stack([torch.ones_like(v), v, v * v], dim=1), **geo)[0]
        dist = m[0] * m[2] - m[1] * m[1]
        ((img * cot).sum() + dist.mean()).backward()

    def one_call():
        out = rast(colors_precomp=t["colors_precomp"], return_distortion="distance", distortion_grad=True, **geo)
        ((out[0] * cot).sum() + out[-1].mean()).backward()

    def leg(fn, reuse):
        def run():
            _C.set_option("geometry_reuse", reuse)
            for k in LEAVES:
                t[k].grad = None
            fn()
        return run
    calls = {"plain": leg(plain, 0), "A": leg(two_calls, 0), "B": leg(two_calls, 1), "C": leg(one_call, 0)}
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    hits, walks = _C.geometry_reuse_hits(), _C.get_option("distortion_grad_calls")
    times = {k: [] for k in calls}
    for _ in range(samples):
        for k, fn in calls.items():
            times[k].append(one_ms(fn))
    hits, walks = _C.geometry_reuse_hits() - hits, _C.get_option("distortion_grad_calls") - walks
    res = {k: stats(v) for k, v in times.items()}
    launches, peaks, grads = {}, {}, {}
    for k, fn in calls.items():
        _C.profile_enable(True)
        _C.profile_reset()
        fn()
        torch.cuda.synchronize()
        launches[k] = {s: n for s, (_ms, n) in _C.profile_read().items() if n}
        _C.profile_enable(False)
        grads[k] = {n: t[n].grad.detach().cpu().numpy() for n in LEAVES}
        peaks[k] = int(peak_above_inputs(fn))
    _C.set_option("geometry_reuse", 0)
    med = {k: v["median_ms"] for k, v in res.items()}
    cost = {k: med[k] - med["plain"] for k in ("A", "B", "C")}
    geometry = [n for n in LEAVES if n != "colors_precomp"]
    return {"P": P, "width": W, "height": H, "scene": f"wg_scenes.make_cloud({P}, {W}, {H}, sh_degree=None, seed=0)",
            "plain_step": res["plain"], "A_second_three_channel_call_and_its_backward": res["A"],
            "B_same_with_geometry_reuse": dict(res["B"], geometry_reuse_hits_per_step=round(hits / samples, 2)),
            "C_one_call_distortion_grad": dict(res["C"], distortion_grad_walks_per_step=round(walks / samples, 2)),
            "cost_of_the_loss_median_ms": {k: round(c, 4) for k, c in cost.items()},
            "C_cost_ratio_to": {k: round(cost["C"] / cost[k], 4) if cost[k] > 0 else None for k in ("A", "B")},
            "library_launches_per_step": launches,
            "torch_kernels_beside_them": {"A": "sub, norm, ones_like, mul, stack, the composition A * Q - D * D, mean; their backward; the accumulation of two "
                                               "gradients per geometry input", "B": "as A", "C": "mean and its backward", "plain": "none"},
            "peak_bytes_above_inputs": peaks,
            "gradients_C_against_A_max_rel_err": {n: rel_err(grads["C"][n], grads["A"][n]) for n in geometry},
            "gradients_B_against_A_max_rel_err": {n: rel_err(grads["B"][n], grads["A"][n]) for n in geometry}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000000x1920x1080,3000000x1600x1200")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distortion.py needs a HIP device")
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
            "metric": "distortion_loss",
            "timing": "forward + backward; one pair of device events per step after a warm-up of all legs; one round visits every leg once; "
                      "median / p10 / p90 over the rounds",
            "legs": {"plain": "the step without the loss", "A": "plain forward + torch.norm + a second full three-channel call with colors_precomp = (1, v, v^2) over "
                     "a zero background + A * Q - D * D in torch, one backward over both (the yardstick: the parent commit's only route)",
                     "B": "A with geometry_reuse = 1: the second call recolours the first frame",
                     "C": 'one call with return_distortion="distance", distortion_grad=True'},
            "gate": "none: recorded, not gated", "configs": configs}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
