"""Shared pieces of tests/test_frame_store.py and tests/golden/make_frame_store_golden.py: the fixture's input frames (generated, no random
numbers), the two list expressions of the reference's `WildGaussians.setup_train` (wildgaussians/method.py:1716-1723) over a given
`convert_image_dtype`, and the loader of the reference's own function where a checkout lies."""
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_store_ref.npz")

IMAGE_CASES = ("image_u8", "image_u8_all", "image_f32", "image_u16")
MASK_CASES = ("mask_u8", "mask_bool")
CASES = IMAGE_CASES + MASK_CASES
EIGHT_BIT = ("image_u8", "image_u8_all", "mask_u8", "mask_bool")   # every float is exactly k / 255: the store keeps these as uint8


def cycling_bytes(H, W, C):
    """uint8 [H, W, C]: the bytes cycle through 0..255 along the pixels, from a channel-dependent offset, with an odd step (so that 256
    pixels visit all 256 values in every channel)."""
    p = np.arange(H * W, dtype=np.int64).reshape(H, W, 1)
    c = np.arange(C, dtype=np.int64).reshape(1, 1, C)
    return ((p * 37 + c * 85 + 3) % 256).astype(np.uint8)


def inputs():
    """name -> the array a dataset would hold (images H x W x 3, masks H x W)."""
    p = np.arange(35, dtype=np.int64).reshape(5, 7)
    return {
        "image_u8": cycling_bytes(5, 7, 3),                # 35 pixels: a stretch of the cycle per channel
        "image_u8_all": cycling_bytes(16, 16, 3),          # 256 pixels: all 256 values in every channel
        "mask_u8": ((p * 29 + 1) % 256).astype(np.uint8),  # values other than 0 and 255
        "mask_bool": (p % 3 == 0),
        "image_f32": ((cycling_bytes(5, 7, 3).astype(np.float32) + np.float32(0.25)) / np.float32(256.0)).astype(np.float32),
        "image_u16": (cycling_bytes(5, 7, 3).astype(np.uint16) * np.uint16(257) + np.uint16(1)),
    }


def image_array(convert, img):
    """The array under one entry of `train_images` (method.py:1716-1718, before torch.from_numpy)."""
    return np.moveaxis(convert(img, np.float32), -1, 0)


def mask_array(convert, img):
    """The array under one entry of `train_masks` (method.py:1720-1723, before torch.from_numpy)."""
    return convert(img, np.float32)[None]


def build_array(convert, name, img):
    return image_array(convert, img) if name in IMAGE_CASES else mask_array(convert, img)


def restated_convert(image, dtype):
    """What the reference's convert_image_dtype does on the way to float32, as the fixture pins it: ONE division for 8-bit sources."""
    assert dtype == np.float32
    if image.dtype == np.float32:
        return image
    if image.dtype == np.uint8:
        return image.astype(np.float32) / 255.0
    return image.astype(np.float32)


def memory_order(a):
    """(the dense storage of `a` in the order it lies in memory, shaped by that order; the permutation of a's axes that gives that order)."""
    perm = tuple(int(i) for i in np.argsort([-s for s in a.strides], kind="stable"))
    return np.ascontiguousarray(a.transpose(perm)), perm


def from_memory_order(storage, perm):
    """The inverse of memory_order: an array with the recorded shape AND strides."""
    inv = np.argsort(perm)
    return storage.transpose(tuple(int(i) for i in inv))


def reference_convert(reference_root):
    """convert_image_dtype executed out of the reference's method.py (the module itself needs packages a test machine may lack)."""
    path = os.path.join(reference_root, "wildgaussians", "method.py")
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "convert_image_dtype")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["convert_image_dtype"]
