#!/usr/bin/env python3
"""Writes tests/golden/dino_ref.npz: what the REFERENCE's own DinoVisionTransformer (wildgaussians/dinov2.py) returns from
`get_intermediate_layers(x, n=[block], reshape=True)[-1]` on the cases of tests/dino_lib.py, on the CPU, in float32 and in float64.

    python tests/golden/make_dino_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies: dinov2.py is imported by its path, `dinov2_vits14_reg(pretrained=False)` builds the model, and
tests/dino_lib.make_weights() is loaded into it (strictly: every name of the state dict is generated).  The case with `offset` / `antialias`
sets the two attributes the non-`reg` constructor passes (interpolate_offset = 0.1, interpolate_antialias = False) on that model.

The fixture holds recorded data only.  Per case: the float64 output on every 8th channel at all tokens, ref32_dev = max |float32 - float64|
over the WHOLE tensor, and the largest magnitude of the float64 output.  Inputs and weights are regenerated from seeds by tests/dino_lib.py.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dino_lib as L  # noqa: E402


def reference_module(checkout):
    spec = importlib.util.spec_from_file_location("wg_reference_dinov2", os.path.join(checkout, "wildgaussians", "dinov2.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod   # the model factory looks its architectures up in sys.modules[__name__]
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, c, dtype):
    model = mod.dinov2_vits14_reg(pretrained=False)
    model.load_state_dict(L.state_dict(L.make_weights(c["peaked"])), strict=True)
    model.interpolate_offset, model.interpolate_antialias = c["offset"], c["antialias"]
    model = model.to(dtype).eval()
    with torch.no_grad():
        out = model.get_intermediate_layers(L.make_image(c).to(dtype), n=[c["block"]], reshape=True)[-1]
    return out.double().numpy()


def main(checkout):
    torch.manual_seed(0)
    mod = reference_module(checkout)
    arrays = {}
    for c in L.CASES:
        o32, o64 = run_reference(mod, c, torch.float32), run_reference(mod, c, torch.float64)
        assert o64.shape == (1, L.EMBED, c["h"], c["w"])
        dev = np.abs(o32 - o64).max()
        arrays[c["name"] + "/out64"] = np.ascontiguousarray(o64[:, ::L.CHANNEL_STRIDE])
        arrays[c["name"] + "/ref32_dev"] = np.float64(dev)
        arrays[c["name"] + "/max_abs"] = np.float64(np.abs(o64).max())
        mine = L.run_oracle_case(c)
        print(f"{c['name']}: ref32_dev = {dev:.3e}, max|out| = {np.abs(o64).max():.3f}, max|oracle - reference float64| = {np.abs(mine - o64).max():.3e}")
    np.savez_compressed(L.GOLDEN, **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")
    assert os.path.getsize(L.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main(sys.argv[1])
