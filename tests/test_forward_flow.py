"""The host FLOW of the forward pass, not only its result: which stages a call enqueues, and how often, in every flow forward_impl
(csrc/api.hip) can take.  The per-stage profiler counts every launch the host makes (wg_profile_read), so a frame's counts are a
fingerprint of the path through the host code: a refactoring of that code must leave them alone."""
import ctypes
import math
import os
import re

import pytest
import torch

import wg_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, P = 128, 96, 4000


def huge_size():
    """The smallest near-square image of more tiles than the LDS histogram holds (wg::BIN_MAX_TILES)."""
    n = int(re.search(r"constexpr int BIN_MAX_TILES = (\d+);", open(os.path.join(ROOT, "wild-gaussians_amd", "csrc", "wg_common.h")).read()).group(1))
    tile = int(re.search(r"#define WG_TILE_X (\d+)", open(os.path.join(ROOT, "include", "wg_rasterizer.h")).read()).group(1))   # (tiles are square)
    gy = math.isqrt(n)
    gx = n // gy + 1
    assert gx * gy > n >= (gx - 1) * gy
    return gx * tile, gy * tile


# case -> (options, forward keywords, image size or None, Gaussians); two frames each, the second one with the first one's history
SPLIT = dict(near_split=1, lazy_min_len=256, lazy_target=100, lazy_cap=256)
CASES = {
    "classic": (dict(speculative_forward=0), {}, None, P),
    "speculative": (dict(speculative_forward=1), {}, None, P),           # frame 2: a hit
    "deferred": (dict(speculative_forward=2), {}, None, P),              # frame 2 returns without its verdict
    "fixed_capacity": ({}, dict(binning_capacity=1 << 20), None, P),
    "global_sort": (dict(force_global_sort=1), {}, None, P),
    "near_split_lazy": (SPLIT, {}, None, P),
    "lazy_colour": (dict(SPLIT, lazy_colour=1, lazy_colour_min_p=1), {}, None, P),
    "huge_frame": ({}, {}, "huge", P),
    "no_gaussians": ({}, {}, None, 0),
}
DEFAULTS = dict(speculative_forward=1, force_global_sort=0, near_split=-1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, lazy_colour=1,
                lazy_colour_min_p=4000000)

# Taken on an MI355X from the parent of the commit that split forward_impl into named steps (2469fb0, "Fused forward-only msssim and
# ssim_down for the uncertainty path"), by printing measure(case) for every case.  {stage: launches} of frame 1 and of frame 2, stages without a launch left out.
CLASSIC = {"preprocess": 1, "scan": 2, "duplicate_keys": 1, "sort": 1, "render_forward": 1}
FIXED = {"preprocess": 1, "scan": 2, "duplicate_keys": 1, "sort": 1, "render_forward": 2, "render_fixup": 1}   # (+ the poisoning launch)
GLOBAL = {"preprocess": 1, "scan": 3, "duplicate_keys": 1, "sort": 1, "render_forward": 1}
SPLIT_LAZY = {"preprocess": 1, "scan": 3, "duplicate_keys": 2, "sort": 1, "render_forward": 1, "render_fixup": 2}
HUGE = {"preprocess": 1, "scan": 2, "duplicate_keys": 1, "sort": 1, "tile_ranges": 2, "render_forward": 1}
EXPECTED = {
    "classic": [CLASSIC, CLASSIC],
    "speculative": [CLASSIC, CLASSIC],                        # (a miss would enqueue the tail twice)
    "deferred": [CLASSIC, dict(CLASSIC, render_forward=2)],   # (frame 2: + the poisoning launch)
    "fixed_capacity": [FIXED, FIXED],
    "global_sort": [GLOBAL, GLOBAL],
    "near_split_lazy": [SPLIT_LAZY, SPLIT_LAZY],
    "lazy_colour": [dict(SPLIT_LAZY, preprocess=3), dict(SPLIT_LAZY, preprocess=3)],
    "huge_frame": [HUGE, HUGE],
    "no_gaussians": [{"render_forward": 1}, {"render_forward": 1}],
}


def forward_without_gaussians(w, h):
    """P = 0 through the C-ABI itself: both bindings answer such a call without asking the library."""
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda")
    geom, binning, img = _C._Scratch(dev), _C._Scratch(dev), _C._Scratch(dev)
    bg, eye, out = torch.zeros(3, device=dev), torch.eye(4, device=dev), torch.empty((3, h, w), device=dev)
    a = _C._forward_args(geom, binning, img, 0, 0, 0, h, w, bg, None, None, None, None, None, 1.0, None, None, eye, eye, None, 1.0, 1.0, 0.1, None,
                         False, False, out, None, dev)
    try:
        assert _C._lib.wg_rasterize_forward_ex(ctypes.byref(a)) == 0
    finally:
        buffers = geom.take(), binning.take(), img.take()   # (alive until the frame is through)
    torch.cuda.synchronize()
    del buffers


def measure(name):
    from diff_gaussian_rasterization import _C
    from tests.wg_testlib import run_hip
    opts, kw, size, n = CASES[name]
    w, h = huge_size() if size == "huge" else (W, H)
    cam = S.make_camera(w, h)
    cloud = S.make_cloud(n, w, h, sh_degree=3, seed=3, scale_mult=7.0)
    frames = []
    try:
        for k, v in dict(DEFAULTS, **opts).items():   # (setting "speculative_forward" also clears the thread's frame history: frame 1 has none)
            _C.set_option(k, v)
        _C.profile_enable(True)
        for _ in range(2):
            _C.profile_reset()
            if n == 0:
                forward_without_gaussians(w, h)
            else:
                with torch.no_grad():
                    run_hip(cloud, cam, sh_degree=3, **kw)
            torch.cuda.synchronize()
            frames.append({stage: launches for stage, (_, launches) in _C.profile_read().items() if launches})
    finally:
        _C.profile_enable(False)
        _C.profile_reset()
        for k, v in DEFAULTS.items():
            _C.set_option(k, v)
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_forward_flow_enqueues_what_it_always_did(name):
    assert measure(name) == EXPECTED[name]

