#!/usr/bin/env python3
"""Writes tests/golden/frame_store_ref.npz: the float32 arrays under the reference's `train_images` / `train_masks` entries
(wildgaussians/method.py:1716-1723: its own convert_image_dtype, then np.moveaxis(..., -1, 0) for an image and [None] for a mask) for the
input frames of tests/frame_store_lib.py.

    python tests/golden/make_frame_store_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies; convert_image_dtype is executed out of its method.py.  Per case the fixture holds the
input, and the result as its dense storage IN MEMORY ORDER with the axis permutation that gives that order (an image's result is a
[3, H, W] view of H x W x 3 storage: its strides are part of what the store has to reproduce).  Recorded data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frame_store_lib as L  # noqa: E402


def main(reference_root):
    convert = L.reference_convert(reference_root)
    out = {}
    for name, img in L.inputs().items():
        result = L.build_array(convert, name, img)
        assert result.dtype == np.float32, (name, result.dtype)
        storage, perm = L.memory_order(result)
        back = L.from_memory_order(storage, perm)
        assert back.shape == result.shape and back.strides == result.strides and np.array_equal(back.view(np.uint32), result.view(np.uint32))
        out[name + "_in"] = img
        out[name + "_storage"] = storage
        out[name + "_perm"] = np.asarray(perm, dtype=np.int64)
    np.savez_compressed(L.GOLDEN, **out)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
