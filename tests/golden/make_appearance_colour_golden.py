#!/usr/bin/env python3
"""Writes tests/golden/appearance_colour_ref.npz: what the REFERENCE's own statements give for the toned colours on the cases of
tests/appearance_colour_lib.GOLDEN_CASES, on the CPU.

    python tests/golden/make_appearance_colour_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies.  As make_appearance_mlp_golden.py does, EmbeddingModel and eval_sh are executed out of
method.py (the module itself needs packages a test machine may lack); appearance_colour_lib.run_reference joins them with the caller's inline
statements (method.py:1555, :1557, :1592-1598).  The fixture holds recorded data only: per case the [P, 3] colours and the gradient of
sum(colours * cot) to the [E] embedding, in float32 and in float64.  Inputs, weights and cotangents are regenerated from the seeds by
tests/appearance_colour_lib.
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import appearance_colour_lib as L  # noqa: E402
import appearance_mlp_lib as ML  # noqa: E402


def reference_parts(checkout):
    """-> (EmbeddingModel, eval_sh) executed out of the checkout's method.py."""
    src = open(os.path.join(checkout, "wildgaussians", "method.py")).read()
    ns = {"torch": torch, "nn": nn, "Config": object}
    a = src.index("\nC0 = ")
    exec(src[a:src.index("\ndef get_expon_lr_func", a)], ns)  # the SH constants and eval_sh
    a = src.index("class EmbeddingModel(nn.Module):")
    exec(src[a:src.index("\n\n\n", a)], ns)  # the class body
    return ns["EmbeddingModel"], ns["eval_sh"]


def reference_model(cls, c, dtype):
    cfg = ML.StubConfig(c["E"])
    cfg.appearance_n_fourier_freqs = c["G"] // 6   # the class sizes its first layer as E + 3 + 6 * n_fourier_freqs
    assert 6 * cfg.appearance_n_fourier_freqs == c["G"]
    return ML.load_weights(cls(cfg), c["weights"], dtype)


def main():
    checkout = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cls, eval_sh = reference_parts(checkout)
    torch.set_num_threads(1)
    arrays = {}
    for i, (P, G, E, seed, deg) in enumerate(L.GOLDEN_CASES):
        c = L.make_case(P, G, E, seed)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            colours, grad = L.run_reference(reference_model(cls, c, dtype), eval_sh, c, deg, dtype)
            assert colours.dtype == grad.dtype == (np.float32 if tag == "32" else np.float64)
            arrays[f"colours{tag}_{i}"], arrays[f"grad{tag}_{i}"] = colours, grad
        print(f"P {P} G {G} E {E} seed {seed} deg {deg}: discarded {c['discarded']:.3f} {c['lost']}")
    np.savez_compressed(L.GOLDEN, cases=np.array(json.dumps(L.GOLDEN_CASES)), **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
