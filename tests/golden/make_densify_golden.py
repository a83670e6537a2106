#!/usr/bin/env python3
"""Generate tests/golden/densify_caller.npz: the REFERENCE's own GaussianModel.densify_and_prune (wildgaussians/method.py:1420-1468, with
_densify_and_clone, _densify_and_split, _densification_postfix, _prune_points) and reset_opacity (:1249-1278), run on the CPU on a real
GaussianModel (small config: SH degree 1, one Fourier frequency) with a torch.optim.Adam whose moments are non-zero -- for
tests/test_densify_prune.py.

Run where the reference checkout lies (tests/real_caller/reference_caller.py), on the CPU; the four inert stand-ins of make_golden.py
cover the packages the module imports and does not exercise here:

    python tests/golden/make_densify_golden.py

Two things are done to the running reference, neither to its files:
  * method.py:1361 allocates `padded_grad_abs` with a hard-coded device="cuda"; torch.zeros is wrapped for the duration of the call so that
    this one request goes to the CPU;
  * torch.normal(mean=0, std=s) is replaced by torch.randn(...) * s + mean, which is bit-equal to it on the CPU under the same generator
    state (asserted below before it is relied on), so that the standard-normal draw itself can be recorded.

Stored -- recorded data only; the inputs are regenerated from the seed by tests/densify_prune_lib.make_inputs on both sides: the seed and
sizes, the recorded noise, ratio and Q as the reference formed them (torch.quantile is wrapped to see them), its three counts, the origin of
every output row (features_dc[:, 0] holds the input row index; the kind follows from the segment), the children's xyz and scales, the buffers
and the opacity moments after the call, and reset_opacity's result on the densified model.  Parameters that are pure copies are checked
through the origin, not stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "real_caller"))
P, SEED = 4096, 7


def main():
    import densify_prune_lib as L
    import make_golden
    import reference_caller as rc
    make_golden._install_shims()
    sys.path.insert(0, rc.PARENT)
    from wildgaussians import method as ref
    from wildgaussians.config import Config
    prm = dict(L.DEFAULTS)
    d = L.make_inputs(P, SEED, sh_degree=1, n_embed=6, ga_mode="grid")
    cfg = Config(source_path="", model_path="", sh_degree=1, appearance_n_fourier_freqs=1, uncertainty_mode="disabled",
                 percent_dense=prm["percent_dense"], use_gof_abs_gradient=True)
    model = ref.GaussianModel(cfg, training_setup=True)
    assert type(model.optimizer) is torch.optim.Adam
    for group in model.optimizer.param_groups:
        name = group["name"]
        if name not in d:
            continue
        p = torch.nn.Parameter(torch.from_numpy(d[name].copy()))
        group["params"][0] = p
        model.register_parameter(name, p)
        model.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.from_numpy(d[name + ".exp_avg"].copy()),
                                    "exp_avg_sq": torch.from_numpy(d[name + ".exp_avg_sq"].copy())}
    for name in L.BUFFERS:
        model.register_buffer(name, torch.from_numpy(d[name].copy()))
    assert all(getattr(model, n).shape[0] == P for n in model._dynamically_sized_props)

    # torch.normal == randn * std + mean, bit for bit, under the same generator state
    std = torch.rand(1000, 3) + 0.01
    torch.manual_seed(5)
    a = torch.normal(mean=torch.zeros_like(std), std=std)
    torch.manual_seed(5)
    assert torch.equal(a, torch.randn(std.shape) * std + torch.zeros_like(std))

    seen = {}
    real_zeros, real_normal, real_quantile = torch.zeros, torch.normal, torch.quantile

    def zeros(*a, **k):
        if k.get("device") == "cuda":
            k["device"] = "cpu"
        return real_zeros(*a, **k)

    def normal(mean, std):
        z = torch.randn(std.shape)
        seen["noise"] = z.numpy().copy()
        return z * std + mean

    def quantile(x, q, *a, **k):
        r = real_quantile(x, q, *a, **k)
        seen["ratio"], seen["Q"] = np.float32(1.0) - q.numpy(), r.numpy().copy()
        return r
    torch.zeros, torch.normal, torch.quantile = zeros, normal, quantile
    torch.manual_seed(SEED)
    try:
        counts = model.densify_and_prune(prm["max_grad"], prm["min_opacity"], prm["extent"], prm["enable_size_pruning"])
    finally:
        torch.zeros, torch.normal, torch.quantile = real_zeros, real_normal, real_quantile
    counts = tuple(int(c) for c in counts)
    n_new = model.xyz.shape[0]
    src = model.features_dc[:, 0].detach().numpy().astype(np.int64)
    # kinds from the segments: originals ascend, then clones ascend, then the two copies of the surviving children
    brk = [0] + [i + 1 for i in range(n_new - 1) if src[i + 1] <= src[i]] + [n_new]
    assert len(brk) == 5, brk
    kind = np.concatenate([np.full(brk[k + 1] - brk[k], k) for k in range(4)])
    origin = np.stack([src, kind], axis=1).astype(np.int32)
    child = kind >= 2

    # the restatement, and the guarantees the test relies on: no decision inside the gap, every class populated
    r = L.restate(d, prm, seen["noise"])
    assert np.array_equal(r["origin"], origin) and r["counts"] == counts, (r["counts"], counts)
    assert r["n_out"][1] > 50 and r["n_out"][2] > 50 and r["pruned_originals"] > 50 and r["pruned_children"] > 10, r["n_out"]
    assert r["nan_stats"] > 50 and r["ties_at_Q"] > 1 and (~r["child_kept"]).sum() > 10
    assert abs(float(seen["Q"]) - r["Q"]) <= r["Q_bound"] and float(seen["ratio"]) == r["ratio"]

    st = model.optimizer.state[model.opacities]
    out = dict(P=P, seed=SEED, noise=seen["noise"], ratio=seen["ratio"], Q=seen["Q"], counts=np.asarray(counts), origin=origin,
               child_xyz=model.xyz.detach().numpy()[child], child_scales=model.scales.detach().numpy()[child],
               opacities_exp_avg=st["exp_avg"].numpy(), **{"buf_" + n: getattr(model, n).numpy() for n in L.BUFFERS})
    model.reset_opacity()
    out["reset_opacities"] = model.opacities.detach().numpy()
    assert np.isfinite(out["reset_opacities"]).all()
    np.savez_compressed(os.path.join(HERE, "densify_caller.npz"), **out)
    print("densify_caller.npz:", {"P": P, "P_new": n_new, "counts": counts, "n_out": r["n_out"], "ratio": r["ratio"], "Q": r["Q"],
                                  "ties at Q": r["ties_at_Q"], "pruned children": r["pruned_children"], "NaN statistics": r["nan_stats"]})


if __name__ == "__main__":
    main()
