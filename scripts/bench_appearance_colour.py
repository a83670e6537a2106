#!/usr/bin/env python3
"""The toned-colour step of WildGaussians.optimize_embedding on one MI355X: from the [E] appearance embedding to the [P, 3] precomputed
colours and back to the embedding's gradient, three ways in ONE process, the legs alternating:

  fused     wg_fused_gaussians.toned_colours, over the visible rows only (rows = a RowList built once from the mask)
  chain     the project's existing opt-in operators: appearance_mlp(shared=), the tone in PyTorch, wg_fused_gaussians.eval_sh; only the
            embedding requires a gradient.  It cannot use the mask: it evaluates all P rows.
  torch     plain PyTorch with the caller's requires_grad pattern (wildgaussians/method.py:1755-1830): the MLP's parameters, the features and
            the per-Gaussian embeddings all require a gradient, so autograd computes every weight and input gradient.  All P rows.

usage: python scripts/bench_appearance_colour.py [--rows 1000000,3000000] [--fractions 1.0,0.3] [--samples 30] [--out FILE] [--commit ID]
                                                 [--accuracy FILE]

Widths 3 + 24 + 32, degree 3.  Per size and visible fraction (the same random mask for every leg): forward alone (no_grad) and forward +
backward with a fixed cotangent that is zero on invisible rows.  Every call is timed by its own pair of device events after a warm-up of all
legs; legs alternate in blocks of five calls; median, p10 and p90 over --samples calls.  Launches are counted by torch.profiler over one call;
peak memory is torch.cuda.max_memory_allocated over one forward + backward above what is allocated before it.  --accuracy: per tensor
max(err / bound) against the float64 oracle of tests/appearance_colour_lib.py for the fused operator and for PyTorch's float32 on the same
device, and their ratio (recorded, not gated).  No GPU: an error, no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import appearance_colour_lib as L  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402
from bench_appearance_mlp import launches, one_ms, peak_above_inputs, stats  # noqa: E402

G, E, DEG = 24, 32, 3


def bench_size(P, fraction, samples, dev):
    g = torch.Generator().manual_seed(P + int(100 * fraction))
    feats = (torch.rand(P, 48, generator=g) * 1.75 - 0.25).to(dev)
    gemb = (torch.rand(P, G, generator=g) * 2 - 1).to(dev)
    xyz = (torch.randn(P, 3, generator=g) * 2).to(dev)
    campos = torch.tensor(L.CAMPOS, device=dev)
    emb = (torch.randn(E, generator=g) * 0.3).to(dev).requires_grad_(True)
    W = [w.to(dev) for w in L.draw_weights(3 + G + E, 1)]
    mask = (torch.rand(P, generator=g) < fraction).to(dev) if fraction < 1.0 else torch.ones(P, dtype=torch.bool, device=dev)
    rows = FG.RowList(mask)   # once, as fit_appearance_embedding does
    cot = torch.randn(P, 3, generator=g).to(dev) * mask[:, None]
    # the caller's pattern: everything is a parameter of the model
    feats_p, gemb_p = feats.clone().requires_grad_(True), gemb.clone().requires_grad_(True)
    W_p = [w.clone().requires_grad_(True) for w in W]

    def fused_fwd():
        return FG.toned_colours(feats, gemb, emb, xyz, campos, W, DEG, rows=rows)

    def chain_fwd():
        return L.operator_chain(FG, feats, gemb, emb, xyz, campos, W, DEG)

    def torch_fwd():
        return L.torch_chain(feats_p, gemb_p, emb, xyz, campos, W_p, DEG)

    def fb(fwd):
        def run():
            emb.grad = None
            fwd().backward(cot)
            for t in [feats_p, gemb_p] + W_p:
                t.grad = None
            return emb.grad
        return run

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    legs = {"fused": fused_fwd, "chain": chain_fwd, "torch": torch_fwd}
    row = {"P": P, "visible_fraction": fraction, "visible_rows": rows.M, "patterns": {}}
    for name, wrap in (("forward", nograd), ("forward_backward", fb)):
        fns = {k: wrap(f) for k, f in legs.items()}
        outs = {}
        for _ in range(3):
            outs = {k: f() for k, f in fns.items()}
        torch.cuda.synchronize()
        sel = mask[:, None] if name == "forward" else 1   # forward: the fused leg leaves invisible rows at 0
        diff = {k: float(((outs[k] - outs["torch"]) * sel).abs().max()) for k in ("fused", "chain")}
        del outs
        times = {k: [] for k in fns}
        while len(times["fused"]) < samples:
            for k, f in fns.items():
                times[k] += [one_ms(f) for _ in range(5)]
        res = {k: dict(stats(v), launches=launches(fns[k])) for k, v in times.items()}
        res["chain_over_fused_median"] = round(res["chain"]["median_ms"] / res["fused"]["median_ms"], 3)
        res["torch_over_fused_median"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 3)
        res["max_abs_diff_from_torch"] = diff
        row["patterns"][name] = res
    row["peak_bytes_above_inputs"] = {k: peak_above_inputs(fb(f)) for k, f in legs.items()}
    return row


def accuracy(dev):
    """max(err / bound) per tensor: the fused operator and PyTorch's float32 on this device, against the float64 oracle."""
    out = []
    for P, listed in ((357, False), (714, True), (33000, False)):
        c = L.make_case(P, G, E, 77 + P)
        rows = L.scattered_rows(P, P // 2, 77 + P) if listed else None
        cot = L.dense_cotangent(P, 77 + P)
        if rows is not None:   # PyTorch's leg evaluates every row: give it the cotangent the list implies
            m = torch.zeros(P, 1)
            m[rows] = 1
            cot = cot * m
        o = L.oracle(c, cot, DEG, rows)
        t = dict(features=c["features"].to(dev), gembedding=c["gemb"].to(dev), xyz=c["xyz"].to(dev), campos=c["campos"].to(dev),
                 weights=[w.to(dev) for w in c["weights"]])
        res = {}
        for leg in ("fused", "torch"):
            emb = c["emb"].to(dev).requires_grad_(True)
            if leg == "fused":
                col = FG.toned_colours(embedding=emb, deg=DEG, rows=None if rows is None else rows.to(dev), **t)
            else:
                col = L.torch_chain(t["features"], t["gembedding"], emb, t["xyz"], t["campos"], t["weights"], DEG)
            col.backward(cot.to(dev))
            col = col.detach().cpu()
            if rows is not None:
                col = col * m
            res[leg] = {"colours": L.ratio(col, o["colours"], o["e_colours"]), "grad_embedding": L.ratio(emb.grad, o["grad"], o["e_grad"])}
        out.append({"P": P, "listed_rows": P if rows is None else len(rows), "discarded_candidates": round(c["discarded"], 4),
                    "clamped_coefficients": round(o["clamped"], 4), "floored_colours": round(o["floored"], 4),
                    "fused_err_over_bound": {k: round(v, 5) for k, v in res["fused"].items()},
                    "torch_float32_err_over_bound": {k: round(v, 5) for k, v in res["torch"].items()},
                    "fused_over_torch": {k: (round(res["fused"][k] / res["torch"][k], 3) if res["torch"][k] > 0 else None) for k in res["fused"]}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,3000000")
    ap.add_argument("--fractions", default="1.0,0.3")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--accuracy", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_appearance_colour.py needs a HIP device")
    dev = torch.device("cuda", 0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    head = {"device": torch.cuda.get_device_name(0), "commit": commit,
            "arguments": {"rows": a.rows, "fractions": a.fractions, "samples": a.samples}}
    if a.accuracy:
        acc = dict(head, metric="appearance_colour_accuracy", yardstick="max over elements of |result - float64| / a-priori float32 rounding "
                   "bound (tests/appearance_colour_lib.py); recorded, not gated", cases=accuracy(dev))
        os.makedirs(os.path.dirname(os.path.abspath(a.accuracy)), exist_ok=True)
        with open(a.accuracy, "w") as f:
            json.dump(acc, f, indent=1)
        print(json.dumps(acc))
    sizes = []
    for P in (int(s) for s in a.rows.split(",") if s):
        for fraction in (float(s) for s in a.fractions.split(",") if s):
            sizes.append(bench_size(P, fraction, a.samples, dev))
            torch.cuda.empty_cache()
    line = dict(head, metric="appearance_colour", widths="3 + 24 + 32 -> 128 -> 128 -> 6, degree 3",
                timing="one pair of device events per call after a warm-up; legs alternate in blocks of five calls; median / p10 / p90",
                legs={"fused": "toned_colours over the visible rows", "chain": "appearance_mlp(shared=) + PyTorch tone + eval_sh, all rows, "
                      "only the embedding requires a gradient", "torch": "plain PyTorch, all rows, the caller's requires_grad pattern"},
                sizes=sizes)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
