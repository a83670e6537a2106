#!/usr/bin/env python3
"""densify_and_prune on one MI355X: (a) a float32 PyTorch restatement of the reference's sequence (wildgaussians/method.py:1280-1468:
quantile, clone + postfix, split + postfix + prune of the parents, prune) on plain tensors and Adam moments -- what a caller runs without the
opt-in --, (b) wg_fused_gaussians.densify_and_prune on the same tensors, the same Adam state, in the same process, alternating.

usage: python scripts/bench_densify.py [--sizes 1000000,3000000] [--big 20000000] [--reps 10] [--out profiles/densify/bench.json] [--fused-only]

Every repetition works on FRESH copies of the inputs (made before the clock starts); times are host clock around work that ends in a
device synchronise.  Per size: median, minimum and maximum of either path; torch.cuda.max_memory_allocated above the inputs; the host
synchronisations of either path (torch.cuda sync debug mode "warn": one warning per synchronising torch call; the fused call's explicit
stream synchronise is counted by hand); the gather kernel's time (device events around the apply call, which is the origin kernel + the
gather) with the bytes it moves, beside the copy ceiling VERDICT.md quotes.  --big: one run of the fused path alone at a size
torch.quantile refuses (> 2^24), skipped with a printed reason when the card's free memory does not allow it.  SH degree 3, 24 embedding
floats: 83 floats per Gaussian, x 3 with the moments, + 6 buffers.  About 5 % cloned, 5 % split, 5 % pruned.  No GPU: an error.
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
import torch  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402

COPY_CEILING = 6.29e12   # bytes / s read + written, measured on this part
PRM = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01, enable_size_pruning=True, use_abs_gradient=True)
SHAPES = {"xyz": 3, "features_dc": 3, "features_rest": 45, "scales": 3, "rotations": 4, "opacities": 1, "embeddings": 24}
BUFFERS = ("xyz_grad", "denom", "filter_3D", "max_radii2D", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max")


def make(P, dev, seed=0):
    """Generated on the device: ~5 % hot by g or ga on either side of percent_dense * extent, ~5 % faint or too large."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    t = {k: r(P, c) for k, c in SHAPES.items()}
    t["scales"] = torch.log(torch.tensor(0.05, device=dev)) + 0.9 * r(P, 1) + 0.2 * r(P, 3)
    o = torch.where(u(P, 1) < 0.04, 0.001 + 0.003 * u(P, 1), 0.02 + 0.9 * u(P, 1))
    t["opacities"] = torch.log(o / (1 - o))
    denom = torch.randint(0, 9, (P, 1), device=dev, generator=g).float()
    stats = {"denom": denom, "xyz_grad": 0.0002 * torch.exp(r(P, 1) - 1.65) * denom, "xyz_gradient_accum_abs": 0.0004 * torch.exp(r(P, 1)) * denom,
             "xyz_gradient_accum_abs_max": 1e-3 * u(P, 1), "filter_3D": 0.001 + 0.01 * u(P, 1), "max_radii2D": 40 * u(P)}
    adam = {k: (1e-3 * r(*v.shape), 1e-6 * u(*v.shape)) for k, v in t.items()}
    return t, adam, stats


def clone_all(x):
    t, adam, stats = x
    return {k: v.clone() for k, v in t.items()}, {k: (m.clone(), v.clone()) for k, (m, v) in adam.items()}, {k: v.clone() for k, v in stats.items()}


def build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)   # noqa: E702
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)   # noqa: E702
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)   # noqa: E702
    return R


@torch.no_grad()
def torch_path(t, adam, stats):
    """The reference's statements on plain tensors, in its order, with its intermediates."""
    def postfix(ext):
        for k in t:
            adam[k] = (torch.cat((adam[k][0], torch.zeros_like(ext[k])), dim=0), torch.cat((adam[k][1], torch.zeros_like(ext[k])), dim=0))
            t[k] = torch.cat((t[k], ext[k]), dim=0)
        n = t["xyz"].shape[0]
        for k in stats:
            stats[k] = torch.cat((stats[k], torch.zeros((n - len(stats[k]), *stats[k].shape[1:]), device=stats[k].device)), dim=0)

    def prune(mask):
        valid = ~mask
        for k in t:
            adam[k] = (adam[k][0][valid], adam[k][1][valid])
            t[k] = t[k][valid]
        for k in stats:
            stats[k] = stats[k][valid]

    grads = stats["xyz_grad"] / stats["denom"]
    grads[grads.isnan()] = 0.0
    ratio = (torch.norm(grads, dim=-1) >= PRM["max_grad"]).float().mean()
    grads_abs = stats["xyz_gradient_accum_abs"] / stats["denom"]
    grads_abs[grads_abs.isnan()] = 0.0
    Q = torch.quantile(grads_abs.reshape(-1), 1 - ratio)
    before = t["xyz"].shape[0]
    thr = PRM["percent_dense"] * PRM["extent"]
    # clone
    scales = torch.exp(t["scales"])
    sel = torch.logical_or(torch.norm(grads, dim=-1) >= PRM["max_grad"], torch.norm(grads_abs, dim=-1) >= Q)
    sel = torch.logical_and(sel, torch.max(scales, dim=1).values <= thr)
    postfix({k: v[sel] for k, v in t.items()})
    clone = t["xyz"].shape[0]
    # split
    scales = torch.exp(t["scales"])
    n_init = t["xyz"].shape[0]
    padded = torch.zeros((n_init), device=scales.device)
    padded[:grads.shape[0]] = grads.squeeze()
    padded_abs = torch.zeros((n_init), device=scales.device)
    padded_abs[:grads_abs.shape[0]] = grads_abs.squeeze()
    sel = torch.logical_or(padded >= PRM["max_grad"], padded_abs >= Q)
    sel = torch.logical_and(sel, torch.max(scales, dim=1).values > thr)
    stds = scales[sel].repeat(2, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=stds.device), std=stds)
    rots = build_rotation(torch.nn.functional.normalize(t["rotations"])[sel]).repeat(2, 1, 1)
    ext = {k: v[sel].repeat(2, 1) for k, v in t.items()}
    ext["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(2, 1)
    ext["scales"] = torch.log(scales[sel].repeat(2, 1) / (0.8 * 2))
    postfix(ext)
    prune(torch.cat((sel, torch.zeros(2 * int(sel.sum().detach().cpu().item()), device=sel.device, dtype=torch.bool))))
    split = t["xyz"].shape[0]
    # prune
    mask = (torch.sigmoid(t["opacities"]) < PRM["min_opacity"]).squeeze()
    mask = torch.logical_or(mask, torch.exp(t["scales"]).max(dim=1).values > 0.1 * PRM["extent"])
    prune(mask)
    return clone - before, split - clone, split - t["xyz"].shape[0]


def fused_path(t, adam, stats):
    return FG.densify_and_prune(t, adam, stats, **PRM)


def count_syncs(fn, x):
    """Synchronising torch calls in one run (sync debug mode 'warn')."""
    args = clone_all(x)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(*args)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(m.message) for m in w)


def timed(fn, x, reps):
    times, peaks, out = [], [], None
    for _ in range(reps):
        args = clone_all(x)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del args
    return times, max(peaks), out


def stats_of(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3), "spread_ms": round(v[-1] - v[0], 3),
            "repeats": len(v)}


def apply_time(x, reps):
    """Device events around wg_densify_apply (origin + gather), by wrapping the library entry for the measurement."""
    real = FG._lib.wg_densify_apply
    ev = []

    class Timed:
        def __call__(self, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(*a)
            e1.record()
            ev.append((e0, e1))
            return r
    FG._lib.wg_densify_apply = Timed()
    try:
        outs = []
        for _ in range(reps):
            args = clone_all(x)
            outs.append(fused_path(*args).n_out)
            del args
        torch.cuda.synchronize()
    finally:
        FG._lib.wg_densify_apply = real
    return [a.elapsed_time(b) for a, b in ev], outs[-1]


def gather_bytes(P, n_out):
    """Bytes the apply step reads and writes: every output row written once and its source read once (moments and buffers of new rows are
    written without a read), the 8-byte origin written and read, the decision byte and block offsets."""
    n_new, n_orig = sum(n_out), n_out[0]
    floats = sum(SHAPES.values())
    wr = n_new * (3 * floats + len(BUFFERS)) * 4
    rd = n_new * floats * 4 + n_orig * (2 * floats + len(BUFFERS)) * 4
    return wr + rd + n_new * 8 * 2 + P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--big", type=int, default=20000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify.py needs a HIP device")
    dev = torch.device("cuda", 0)
    per_gaussian = (3 * sum(SHAPES.values()) + len(BUFFERS)) * 4
    rows = []
    for P in [int(s) for s in a.sizes.split(",") if s]:
        x = make(P, dev)
        fused_path(*clone_all(x))   # warm-up
        if a.fused_only:
            timed(fused_path, x, 5)
            continue
        torch_path(*clone_all(x))
        tb, tf = [], []
        peak_t = peak_f = 0
        for _ in range(a.reps):   # alternate, one repetition each
            t1, p1, ref = timed(torch_path, x, 1)
            t2, p2, res = timed(fused_path, x, 1)
            tb += t1
            tf += t2
            peak_t, peak_f = max(peak_t, p1), max(peak_f, p2)
        ev, n_out = apply_time(x, a.reps)
        sb, sf = stats_of(tb), stats_of(tf)
        ap_ms = sorted(ev)[len(ev) // 2]
        nbytes = gather_bytes(P, n_out)
        rows.append({"P": P, "input_bytes": P * per_gaussian, "torch_restatement": sb, "fused": sf,
                     "speedup_median": round(sb["median_ms"] / sf["median_ms"], 2),
                     "median_gap_ms": round(sb["median_ms"] - sf["median_ms"], 3), "combined_spread_ms": round(sb["spread_ms"] + sf["spread_ms"], 3),
                     "fused_below_torch_by_more_than_combined_spread": sb["median_ms"] - sf["median_ms"] > sb["spread_ms"] + sf["spread_ms"],
                     "peak_bytes_above_inputs": {"torch_restatement": peak_t, "fused": peak_f, "fused_no_higher": peak_f <= peak_t},
                     "host_synchronisations": {"torch_restatement": count_syncs(torch_path, x), "fused_torch_calls": count_syncs(fused_path, x),
                                               "fused_explicit_stream_synchronize": 1},
                     "counts": {"torch_restatement": [int(c) for c in ref], "fused": list(res.counts), "n_out": list(n_out)},
                     "apply": {"median_ms_device_events": round(ap_ms, 4), "bytes_moved": nbytes, "TB_per_s": round(nbytes / (ap_ms * 1e-3) / 1e12, 3),
                               "copy_ceiling_TB_per_s": COPY_CEILING / 1e12, "share_of_copy_ceiling": round(nbytes / (ap_ms * 1e-3) / COPY_CEILING, 3)}})
        del x, ref, res
        torch.cuda.empty_cache()
    big = None
    if a.big and not a.fused_only:
        P = a.big
        need = int(P * per_gaussian * 2.3)   # inputs, outputs (~1.05 x), the generator's temporaries
        free, _ = torch.cuda.mem_get_info()
        if free < need:
            big = {"P": P, "skipped": f"needs about {need / 2 ** 30:.1f} GiB, {free / 2 ** 30:.1f} GiB free"}
            print("20 M run skipped:", big["skipped"])
        else:
            x = make(P, dev)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            res = fused_path(*x)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            try:
                torch.quantile(x[2]["denom"].reshape(-1), 0.5)
                refuses = False
            except RuntimeError:
                refuses = True
            big = {"P": P, "input_bytes": P * per_gaussian, "memory_needed_bytes_estimate": need, "fused_ms_single_run_cold": round(ms, 3),
                   "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base, "counts": list(res.counts), "Q": res.Q, "ratio": res.ratio,
                   "torch_quantile_refuses_this_size": refuses}
            del x, res
    line = {"metric": "densify_and_prune", "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv), "floats_per_gaussian": sum(SHAPES.values()),
            "bytes_per_gaussian_with_moments_and_buffers": per_gaussian, "sizes": rows, "beyond_torch_quantile_limit": big}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
