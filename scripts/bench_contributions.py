#!/usr/bin/env python3
"""What a frame's per-Gaussian contribution statistics cost on one MI355X, in ONE process, the legs alternating call by call.

usage: python scripts/bench_contributions.py [--configs 1000000x1920x1080,3000000x1600x1200] [--samples 30] [--out FILE] [--commit ID]

Frames: wg_scenes.make_cloud(P, W, H, sh_degree=None, seed=0) through the base camera, precomputed colours.
    A       the plain forward call (torch.no_grad())
    B       the same with contributions=stats: the contribution pass behind the frame (max_weight, hits, weight_sum_q32)
    A_grad  the forward call in grad mode with colour_gradients_only=True (what C's forward half is: the frame keeps what a backward call needs)
    C       the parent commit's only route to ANY of the three numbers: A_grad plus the colour-only backward pass under an all-ones cotangent
            -- dL_dcolor[:, c] is then the summed weight alone, through float atomics (no maximum, no hit count, not reproducible)
    depth   the forward call with return_depth="distance": the cost of a bare walk over the finished frame (one per-pixel sum, no atomics)
Reported: B - A, C - A (and C - A_grad, the backward walk alone) and depth - A.  Every call is timed by its own pair of device events after a
warm-up of all legs; one round visits every leg once; median, p10 and p90 over --samples rounds.  B's statistics are compared with C's summed
weight (float32 atomics: a relative figure, not a gate) and two B calls bit for bit.  No speed gate.  No GPU: an error, no fallback."""
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
from bench_appearance_mlp import one_ms, stats  # noqa: E402
from diff_gaussian_rasterization import ContributionStats, GaussianRasterizer, _C  # noqa: E402
from wg_testlib import make_settings, to_dev  # noqa: E402


def bench_config(P, W, H, samples):
    cam = S.make_camera(W, H)
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=0).items()}
    rs = make_settings(cam, 0)
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"])
    rast = GaussianRasterizer(rs)
    st = ContributionStats(P, "cuda")
    colours = cloud["colors_precomp"].clone().requires_grad_(True)
    ones = torch.ones(3, H, W, device="cuda")

    def quiet(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def grad_forward():
        return rast(colors_precomp=colours, colour_gradients_only=True, **geo)

    def colour_backward():
        colours.grad = None
        grad_forward()[0].backward(ones)
        return colours.grad
    calls = {"A": quiet(lambda: rast(colors_precomp=cloud["colors_precomp"], **geo)),
             "B": quiet(lambda: rast(colors_precomp=cloud["colors_precomp"], contributions=st, **geo)),
             "A_grad": grad_forward, "C": colour_backward,
             "depth": quiet(lambda: rast(colors_precomp=cloud["colors_precomp"], return_depth="distance", **geo))}
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(samples):
        for k, fn in calls.items():
            times[k].append(one_ms(fn))
    res = {k: stats(v) for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    # the library's launches and stage times over one call of each leg
    launches = {}
    for k, fn in calls.items():
        _C.profile_enable(True)
        _C.profile_reset()
        fn()
        torch.cuda.synchronize()
        launches[k] = {s: dict(launches=n, ms=round(ms, 4)) for s, (ms, n) in _C.profile_read().items() if n}
        _C.profile_enable(False)
    # what was computed
    st.reset()
    calls["B"]()
    first = (st.max_weight.clone(), st.hits.clone(), st.weight_sum_q32.clone())
    st.reset()
    calls["B"]()
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(first, (st.max_weight, st.hits, st.weight_sum_q32)))
    atomic_sum = calls["C"]()[:, 0].double()
    ws = st.weight_sum
    R = _C.rasterize_gaussians(rs.bg, cloud["means3D"], cloud["colors_precomp"], cloud["opacities"], cloud["scales"], cloud["rotations"], 1.0,
                               torch.Tensor([]), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset,
                               H, W, torch.Tensor([]), 0, rs.campos, False, False)[0]
    return {"P": P, "width": W, "height": H, "scene": f"wg_scenes.make_cloud({P}, {W}, {H}, sh_degree=None, seed=0)", "num_rendered": int(R),
            "A_plain_forward": res["A"], "B_forward_with_contributions": res["B"], "A_grad_forward_in_grad_mode": res["A_grad"],
            "C_forward_plus_colour_only_backward_all_ones": res["C"], "depth_forward_with_return_depth": res["depth"],
            "cost_median_ms": {"B_minus_A": round(med["B"] - med["A"], 4), "C_minus_A": round(med["C"] - med["A"], 4),
                               "C_minus_A_grad": round(med["C"] - med["A_grad"], 4), "depth_minus_A": round(med["depth"] - med["A"], 4)},
            "library_stages_per_call": launches,
            "statistics": {"gaussians_hit": int((st.hits > 0).sum()), "pairs": int(st.hits.sum()), "largest_max_weight": float(st.max_weight.max()),
                           "two_B_calls_bit_equal": bool(same),
                           "largest_relative_difference_of_weight_sum_to_C": float(((ws - atomic_sum).abs() / ws.clamp_min(1e-30))[st.hits > 0].max())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000000x1920x1080,3000000x1600x1200")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contributions", "bench.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contributions.py needs a HIP device")
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
            "metric": "render_contributions",
            "timing": "one pair of device events per call after a warm-up of all legs; one round visits every leg once; median / p10 / p90 over the rounds",
            "legs": {"A": "the plain forward call (no_grad)", "B": "A with contributions=stats",
                     "A_grad": "the forward call in grad mode, colour_gradients_only=True",
                     "C": "A_grad + the colour-only backward pass under an all-ones cotangent: the summed weight alone, float atomics",
                     "depth": 'A with return_depth="distance": a bare walk over the finished frame'},
            "gate": "none: recorded, not gated", "configs": configs}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
