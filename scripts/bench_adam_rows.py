#!/usr/bin/env python3
"""The optimizer step over the visible rows only, on one MI355X: wg_fused_gaussians.VisibleRowsAdam.step(rows=radii) against today's
FusedAdam.step() over all P rows and against the no-new-kernel alternative, in ONE process, the legs alternating step by step.

usage: python scripts/bench_adam_rows.py [--rows 1000000,3000000] [--fractions 1.0,0.87,0.67,0.41,0.1] [--samples 30] [--out FILE] [--commit ID]

Per size, the reference's seven per-Gaussian tensors (xyz 3, features_dc 3, opacities 1, scales 3, rotations 4, embeddings 24,
features_rest 45 floats per row: 83 in all), each with a gradient and both moments:
    dense            FusedAdam.step() over everything: the yardstick (the parent commit's code), measured in the same run
    rows@f/random    VisibleRows.from_radii(radii) -- the compaction is INSIDE the timed region -- and the rows step, at visible share f of a
                     seeded random mask
    rows@f/runs      the same share as contiguous runs of 4096 rows (whole runs drawn by the same seed): what cache-line sharing costs the
                     narrow tensors under the random mask is the difference
    gathered@f       (radii > 0).nonzero(), index_select of param / grad / both moments of every tensor, the dense kernel on the copies,
                     index_copy_ of param and moments back: what a caller can do without a new kernel (random mask)
`radii` is a chosen mask, not a training view.  Every call is timed by its own pair of device events after a warm-up of all legs; one round
visits every leg once; median, p10 and p90 over --samples rounds.  All legs step the same tensors (the values move, the traffic does not).
No speed gate.  No GPU: an error, no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
import torch  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402

WIDTHS = {"xyz": 3, "features_dc": 3, "opacities": 1, "scales": 3, "rotations": 4, "embeddings": 24, "features_rest": 45}
RUN = 4096


def one_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(round(p * (len(v) - 1))))]   # noqa: E731
    return {"median_ms": round(q(0.5), 4), "p10_ms": round(q(0.1), 4), "p90_ms": round(q(0.9), 4), "samples": len(v)}


def bench_size(P, fractions, samples, dev):
    g = torch.Generator().manual_seed(P)
    params = {n: torch.nn.Parameter(torch.randn(P, w, generator=g).to(dev)) for n, w in WIDTHS.items()}
    groups = [{"params": [p], "lr": 1e-3, "name": n} for n, p in params.items()]
    dense = FG.FusedAdam(groups, lr=1e-3, eps=1e-15)
    for p in params.values():
        p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
    dense.step()   # creates the moments
    rows_opt = FG.VisibleRowsAdam.adopt(dense)   # the same parameters and state tensors
    u = torch.rand(P, generator=g).to(dev)
    u_runs = torch.rand((P + RUN - 1) // RUN, generator=g).to(dev).repeat_interleave(RUN)[:P]
    legs = {"dense": dense.step}
    measured = {}

    def add(fraction):
        for pattern, draw in (("random", u), ("runs", u_runs)):
            radii = torch.where(draw < fraction, 5, 0).to(torch.int32)
            legs[f"rows@{fraction:g}/{pattern}"] = lambda radii=radii: rows_opt.step(rows=radii)
            measured[f"{fraction:g}/{pattern}"] = round(float((radii > 0).float().mean()), 4)
        radii = torch.where(u < fraction, 5, 0).to(torch.int32)

        def gathered():
            idx = (radii > 0).nonzero().reshape(-1)
            copies, descs = [], []
            for p in params.values():
                st = dense.state[p]
                c = [t.index_select(0, idx) for t in (p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"])]
                copies.append(c)
                descs.append(FG._AdamTensor(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), c[0].numel(), 0.999, 0.1, 0.001,
                                            1e-3, 1.0, 1e-15, 0.0))
            arr = (FG._AdamTensor * len(descs))(*descs)
            FG._native._check(FG._lib.wg_fused_adam(len(descs), arr, torch.cuda.current_stream().cuda_stream), "wg_fused_adam")
            for p, c in zip(params.values(), copies):
                st = dense.state[p]
                p.detach().index_copy_(0, idx, c[0])
                st["exp_avg"].index_copy_(0, idx, c[2])
                st["exp_avg_sq"].index_copy_(0, idx, c[3])
        legs[f"gathered@{fraction:g}"] = gathered
    for f in fractions:
        add(f)
    for _ in range(3):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(samples):
        for k, fn in legs.items():
            times[k].append(one_ms(fn))
    res = {k: stats(v) for k, v in times.items()}
    for v in res.values():
        v["dense_over_this_median"] = round(res["dense"]["median_ms"] / v["median_ms"], 3)
    floats = sum(WIDTHS.values())
    return {"P": P, "floats_per_row": floats, "dense_bytes_per_step": 28 * floats * P, "visible_fraction_of_the_mask": measured, "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,3000000")
    ap.add_argument("--fractions", default="1.0,0.87,0.67,0.41,0.1")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_rows", "bench.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam_rows.py needs a HIP device")
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
        sizes.append(bench_size(P, fractions, a.samples, dev))
        torch.cuda.empty_cache()
    line = {"device": torch.cuda.get_device_name(0), "commit": commit, "arguments": {"rows": a.rows, "fractions": a.fractions, "samples": a.samples},
            "metric": "adam_rows", "widths": WIDTHS,
            "timing": "one pair of device events per call after a warm-up; one round visits every leg once; median / p10 / p90 over the rounds",
            "legs": {"dense": "FusedAdam.step() over all P rows of the seven tensors (the yardstick)",
                     "rows@f/random": "VisibleRows.from_radii (timed) + wg_adam_rows_step at visible share f, seeded random mask",
                     "rows@f/runs": f"the same with the share drawn as contiguous runs of {RUN} rows",
                     "gathered@f": "nonzero + index_select + wg_fused_adam on the copies + index_copy_ by torch at visible share f (random mask)"},
            "gate": "none: recorded, not gated", "sizes": sizes}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
