#!/usr/bin/env python3
"""The appearance MLP over the visible rows only, on one MI355X: wg_fused_gaussians.appearance_mlp(rows=VisibleRows.from_radii(radii))
against today's dense operator over all P rows and against the no-new-kernel alternative, in ONE process, the legs alternating call by call.

usage: python scripts/bench_appearance_mlp_rows.py [--rows 1000000,3000000] [--fractions 1.0,0.5,0.3,0.1] [--samples 30] [--out FILE] [--commit ID]

Per size (widths 3 + 24 + 32; colour a stride-48 view of the features), per form of the appearance embedding (shared [32] / per row
[P, 32]) and per pattern (forward alone under no_grad; forward + backward with a fixed cotangent that is zero at culled rows, as the
rasterizer's is, and gradients to all inputs and weights):
    dense     appearance_mlp over all P rows: the yardstick, measured in the same run
    rows      VisibleRows.from_radii(radii) -- the compaction is INSIDE the timed region -- and appearance_mlp(rows=), per visible fraction
    gathered  (radii > 0).nonzero(), index_select of every per-row input, the dense operator on the gathered copies, the result scattered into
              zeros and the gradients scattered back by autograd: what a caller can do without a new kernel, per visible fraction
`radii` is a seeded random pattern with the given share of positive entries (a chosen mask, not a training view).  Every call is timed by its
own pair of device events after a warm-up of all legs; one round visits every leg once; median, p10 and p90 over --samples rounds.  Launches
are counted by torch.profiler over one call; peak memory is torch.cuda.max_memory_allocated over one call above what is allocated before it
(inputs, weights, radii).  For orientation the line also records (radii > 0).float().mean() of the headline frame of bench.py (wg_scenes,
1 000 000 Gaussians, 1920x1080, seed 0).  No speed gate.  No GPU: an error, no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import appearance_mlp_lib as L  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402
from bench_appearance_mlp import launches, one_ms, peak_above_inputs, stats  # noqa: E402

G, E = 24, 32


def headline_visible_fraction(dev):
    import wg_scenes as S
    from diff_gaussian_rasterization import GaussianRasterizer
    from wg_testlib import make_settings, to_dev
    W, H, P = 1920, 1080, 1_000_000
    cam = S.make_camera(W, H)
    cloud = S.make_cloud(P, W, H, sh_degree=3, seed=0)
    t = {k: to_dev(v) for k, v in cloud.items()}
    with torch.no_grad():
        _, radii, _ = GaussianRasterizer(make_settings(cam, 3))(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
                                                                shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    return {"scene": f"wg_scenes.make_cloud({P}, {W}, {H}, sh_degree=3, seed=0)", "visible_fraction": round(float((radii > 0).float().mean()), 4)}


def bench_size(P, shared, fractions, samples, dev):
    g = torch.Generator().manual_seed(P + shared)
    feats = torch.rand(P, 48, generator=g).to(dev).requires_grad_(True)
    gemb = (torch.rand(P, G, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    avec = (torch.randn(E, generator=g) * 0.3).to(dev)
    arow = avec[None].repeat(P, 1).requires_grad_(True)
    avec.requires_grad_(True)
    W = [w.to(dev).requires_grad_(True) for w in L.draw_weights(3 + G + E, 1)]
    cot_full = torch.randn(P, 6, generator=g).to(dev)
    u = torch.rand(P, generator=g).to(dev)
    leaves = [feats, gemb, avec if shared else arow] + W

    def mlp(colour, ge, ar, rows=None):
        if shared:
            return FG.appearance_mlp((colour, ge), W, shared=avec, rows=rows)
        return FG.appearance_mlp((colour, ge, ar), W, rows=rows)

    legs = {}   # name -> (forward, cotangent)

    def add(fraction):
        radii = torch.where(u < fraction, 5, 0).to(torch.int32)
        cot = cot_full * (radii > 0)[:, None]

        def rows_fwd():
            return mlp(feats[..., :3], gemb, arow, rows=FG.VisibleRows.from_radii(radii))

        def gathered_fwd():
            idx = (radii > 0).nonzero().reshape(-1)
            out = mlp(feats[..., :3].index_select(0, idx), gemb.index_select(0, idx), None if shared else arow.index_select(0, idx))
            return torch.zeros(P, 6, device=dev).index_copy(0, idx, out)
        legs[f"rows@{fraction:g}"] = (rows_fwd, cot)
        legs[f"gathered@{fraction:g}"] = (gathered_fwd, cot)
        return float((radii > 0).float().mean())
    legs["dense"] = (lambda: mlp(feats[..., :3], gemb, arow), cot_full)
    measured = {f"{f:g}": round(add(f), 4) for f in fractions}

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def fb(fn, cot):
        return lambda: torch.autograd.grad(fn(), leaves, cot)
    row = {"P": P, "aembedding": "shared [32]" if shared else "per row [P, 32]", "visible_fraction_of_the_mask": measured, "patterns": {}}
    for name in ("forward", "forward_backward"):
        calls = {k: (nograd(f) if name == "forward" else fb(f, c)) for k, (f, c) in legs.items()}
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(samples):
            for k, fn in calls.items():
                times[k].append(one_ms(fn))
        res = {k: dict(stats(v), launches=launches(calls[k]), peak_bytes_above_inputs=peak_above_inputs(calls[k])) for k, v in times.items()}
        dense = res["dense"]["median_ms"]
        for k, v in res.items():
            v["dense_over_this_median"] = round(dense / v["median_ms"], 3)
        row["patterns"][name] = res
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,3000000")
    ap.add_argument("--fractions", default="1.0,0.5,0.3,0.1")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_appearance_mlp_rows.py needs a HIP device")
    dev = torch.device("cuda", 0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    fractions = [float(s) for s in a.fractions.split(",") if s]
    sizes = []
    for P in (int(s) for s in a.rows.split(",") if s):
        for shared in (True, False):
            sizes.append(bench_size(P, shared, fractions, a.samples, dev))
            torch.cuda.empty_cache()
    line = {"device": torch.cuda.get_device_name(0), "commit": commit, "arguments": {"rows": a.rows, "fractions": a.fractions, "samples": a.samples},
            "metric": "appearance_mlp_rows", "widths": "3 + 24 + 32 -> 128 -> 128 -> 6",
            "timing": "one pair of device events per call after a warm-up; one round visits every leg once; median / p10 / p90 over the rounds",
            "legs": {"dense": "appearance_mlp over all P rows (the yardstick)",
                     "rows@f": "VisibleRows.from_radii (timed) + appearance_mlp(rows=) at visible fraction f",
                     "gathered@f": "nonzero + index_select + the dense operator + scatter by torch at visible fraction f"},
            "gate": "none: recorded, not gated", "headline_frame": headline_visible_fraction(dev), "sizes": sizes}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
