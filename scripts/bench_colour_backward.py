#!/usr/bin/env python3
"""The colour-only backward pass (colour_gradients_only=True) against the full backward pass of the SAME build on the SAME frame: bench.py's
headline scene with precomputed colours (1 M Gaussians, 1920x1080) and one 3 M frame.  Per frame: the backward call alone (the native call on
a kept frame, HIP events) and forward + backward through the operator, each with and without the flag, interleaved in rounds inside one
process; medians of the timed calls with their spread, and the library's own stage times (wg_profile_read) per call.
The stage times are NOT like for like: the colour-only pass books its tile-ordering launch (which also clears dL_dcolor) under "render_backward",
the full pass books the same launch (which clears the gradient records) under "tile_ranges" -- compare the sums of the backward stages, or the
event-timed calls.
--fixed-order: the fixed-order leg instead -- on 1 M / 1920x1080 and 3 M / 1600x1200 frames, the backward call alone (device events per call,
legs alternating in one process, medians of the timed calls with p10 / p90) of (a) the atomic colour-only pass, (b) colour_gradients_only=
"fixed_order", (c) the full backward pass with deterministic_backward=1 on the same frame (what reproducibility costs without (b)); the
scratch (b) leases; whether (b)'s and (c)'s p10 / p90 bands order them.  Written to profiles/colour_backward/bench_fixed_order.json.
usage: bench_colour_backward.py [--calls 30] [--warmup 5] [--out profiles/colour_backward/bench.json] [--fixed-order]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd")); sys.path.insert(0, ROOT)
import torch  # noqa: E402
import wg_scenes as S  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _C  # noqa: E402
from tests.wg_testlib import make_settings, to_dev  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--fixed-order", action="store_true")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "colour_backward", "bench_fixed_order.json" if args.fixed_order else "bench.json")
assert args.calls >= 20 and args.warmup >= 5
dev = torch.device("cuda", 0)
e = torch.Tensor([])


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), p25_ms=round(q[0], 4), p75_ms=round(q[2], 4), max_ms=round(max(ms), 4),
                calls=len(ms))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def band(ms):
    d = statistics.quantiles(ms, n=10)
    return dict(median_ms=round(statistics.median(ms), 4), p10_ms=round(d[0], 4), p90_ms=round(d[8], 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                calls=len(ms))


def stages(fn, calls):
    """The library's stage times per call (HIP events around each stage, accumulated by wg_profile_*)."""
    _C.profile_enable(True)
    _C.profile_reset()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    st = _C.profile_read()
    _C.profile_enable(False)
    return {k: round(ms / calls, 4) for k, (ms, launches) in st.items() if launches}


def frame(P, W, H):
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=0)
    rs = make_settings(S.make_camera(W, H), 0, device=dev)
    t = {k: to_dev(v, dev) for k, v in cloud.items()}
    cot = to_dev(S.make_cotangent(W, H), dev)
    R, _color, radii, gb, bb, ib = _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix,
                                                         rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, H, W, e, 0, rs.campos, False, False)

    def backward(flag):
        return lambda: _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                       rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, cot, e, 0, rs.campos, gb, R, bb, ib, False,
                                                       colour_gradients_only=flag)

    g = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
    rast = GaussianRasterizer(rs)

    def step(flag):
        def run():
            for v in list(g.values()) + [m2d]:
                v.grad = None
            img = rast(means3D=g["means3D"], means2D=m2d, opacities=g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"],
                       colour_gradients_only=flag)[0]
            img.backward(cot)
        return run

    out = {"workload": f"{P} Gaussians, {W}x{H}, precomputed colours", "num_rendered": int(R),
           "stage_note": "colour_only books the tile-ordering launch under render_backward, full books it under tile_ranges: stage rows are not like for like"}
    for what, make in (("backward_call", backward), ("forward_backward", step)):
        fns = {"full": make(False), "colour_only": make(True)}
        ms = {k: [] for k in fns}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(args.calls):   # interleaved: both variants see the same clocks
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        out[what] = {k: spread(v) for k, v in ms.items()}
        out[what]["speedup_of_medians"] = round(out[what]["full"]["median_ms"] / out[what]["colour_only"]["median_ms"], 3)
        out[what + "_stage_ms_per_call"] = {k: stages(fn, args.calls) for k, fn in fns.items()}
    a, b = backward(False)()[1], backward(True)()[1]
    out["max_abs_difference_over_max_abs"] = float((a - b).abs().max() / a.abs().max())
    return out


def frame_fixed_order(P, W, H):
    """Legs (a), (b), (c) of the module docstring on one kept frame."""
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=0)
    rs = make_settings(S.make_camera(W, H), 0, device=dev)
    t = {k: to_dev(v, dev) for k, v in cloud.items()}
    cot = to_dev(S.make_cotangent(W, H), dev)
    R, _color, radii, gb, bb, ib = _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix,
                                                         rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, H, W, e, 0, rs.campos, False, False)

    def backward(**kw):
        return lambda: _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                       rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, cot, e, 0, rs.campos, gb, R, bb, ib, False, **kw)
    fns = {"a_atomic_colour_only": backward(colour_gradients_only=True), "b_fixed_order": backward(colour_gradients_only="fixed_order"),
           "c_full_deterministic": backward(colour_gradients_only=False, options=dict(deterministic_backward=1))}
    ms = {k: [] for k in fns}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.calls):   # alternating: every leg sees the same clocks
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    out = {"workload": f"{P} Gaussians, {W}x{H}, precomputed colours", "num_rendered": int(R), "backward_call": {k: band(v) for k, v in ms.items()}}
    bc = out["backward_call"]
    out["fixed_order_over_atomic_medians"] = round(bc["b_fixed_order"]["median_ms"] / bc["a_atomic_colour_only"]["median_ms"], 3)
    out["fixed_order_over_full_deterministic_medians"] = round(bc["b_fixed_order"]["median_ms"] / bc["c_full_deterministic"]["median_ms"], 3)
    # (b) is slower than (c) only if its whole p10 / p90 band lies above (c)'s
    out["fixed_order_slower_than_full_deterministic_beyond_bands"] = bool(bc["b_fixed_order"]["p10_ms"] > bc["c_full_deterministic"]["p90_ms"])
    # what (b) leases (api.hip: backward_colour_impl): 16 bytes per instance rounded up to 256 + a flag byte per instance rounded up to 16; (c): 40 + 1
    out["fixed_order_scratch_bytes"] = ((16 * int(R) + 255) & ~255) + ((int(R) + 15) & ~15)
    out["full_deterministic_scratch_bytes"] = ((40 * int(R) + 255) & ~255) + ((int(R) + 15) & ~15)
    fx = [backward(colour_gradients_only="fixed_order")()[1] for _ in range(2)]
    at = backward(colour_gradients_only=True)()[1]
    out["two_fixed_order_calls_equal"] = bool(torch.equal(fx[0], fx[1]))
    out["max_abs_difference_to_atomic_over_max_abs"] = float((fx[0] - at).abs().max() / at.abs().max())
    return out


if args.fixed_order:
    res = {"device": torch.cuda.get_device_name(0), "library": _C.version(), "binding": _C.binding_name(), "calls": args.calls, "warmup": args.warmup,
           "frames": [frame_fixed_order(1_000_000, 1920, 1080), frame_fixed_order(3_000_000, 1600, 1200)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    sys.exit(0)

res = {"device": torch.cuda.get_device_name(0), "library": _C.version(), "binding": _C.binding_name(), "calls": args.calls, "warmup": args.warmup,
       "frames": [frame(1_000_000, 1920, 1080), frame(3_000_000, 1920, 1080)]}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
