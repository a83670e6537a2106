"""Helpers of tests/test_contributions.py: scenes, the operator's calls, and the yardstick -- per-Gaussian contribution statistics read off
the operator's OWN forward call with one-hot precomputed colours over a zero background.  Gaussians g0, g1, g2 get the colours e_0, e_1, e_2
and every other row 0: the forward kernel's channel c is then C = fma(1, w, 0) = w at g_c and C = fma(0, w', C) = C at every other instance,
i.e. EXACTLY g_c's blend weight w = alpha * T per pixel (0 where it was not blended: a blended weight is > 0)."""
import numpy as np
import torch

import wg_scenes as S
from wg_testlib import make_settings, to_dev

Q32 = 4294967296.0

# the scenes of tests/test_render_depth.py, restated: name -> P, W, H, scale_mult, random sub-pixel offsets
SCENES = {
    "ragged": (8000, 250, 130, 3.0, True),        # partial tiles
    "saturating": (1500, 320, 200, 12.0, False),  # long lists, pixels that stop early beside pixels nothing reaches
}


def scene(name):
    """-> (cloud as device tensors, camera, sub-pixel offsets or None)"""
    if name == "dense":   # ~1000 instances per tile
        P, W, H, sm, offsets, seed = 30000, 320, 200, 7.0, False, 5
    else:
        (P, W, H, sm, offsets), seed = SCENES[name], 11
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=seed, scale_mult=sm).items()}
    so = np.random.default_rng(3).uniform(-0.5, 0.5, size=(H, W, 2)).astype(np.float32) if offsets else None
    return cloud, S.make_camera(W, H), so


def one_tile(P):
    """tests/test_render_depth.py's recipe: one 16 x 16 tile, P faint Gaussians that all cover it -- every pixel blends every instance and
    nothing saturates, so the walk's batches end exactly where the list does."""
    rng = np.random.default_rng(P)
    z = rng.uniform(2.0, 8.0, size=P)
    means = np.stack([0.02 * z * rng.uniform(-1, 1, size=P), 0.02 * z * rng.uniform(-1, 1, size=P), z], axis=1)
    scales = (1.5 * z)[:, None] * np.ones((P, 3))
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    cloud = dict(means3D=means, scales=scales, rotations=q, opacities=np.full((P, 1), 0.01), colors_precomp=rng.uniform(0, 1, size=(P, 3)))
    return {k: to_dev(np.ascontiguousarray(v, dtype=np.float32)) for k, v in cloud.items()}, S.make_camera(16, 16)


def render(cloud, cam, so=None, colors=None, bg=None, **fwd):
    """One call of the operator with precomputed colours -> its output tuple."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=np.zeros(3, np.float32) if bg is None else np.array(bg, np.float32), subpixel_offset=so)
    return GaussianRasterizer(rs)(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"],
                                  colors_precomp=cloud["colors_precomp"] if colors is None else colors, scales=cloud["scales"],
                                  rotations=cloud["rotations"], **fwd)


def collect(cloud, cam, so=None, mask=None, stats=None, **fwd):
    """One call with contributions= -> (the ContributionStats, the call's outputs)."""
    from diff_gaussian_rasterization import ContributionStats
    if stats is None:
        stats = ContributionStats(cloud["means3D"].shape[0], "cuda")
    out = render(cloud, cam, so, contributions=stats, contribution_mask=mask, **fwd)
    return stats, out


def stats_of_weights(w, mask=None):
    """w: [K, H, W] float32 blend weights of K Gaussians per pixel (0 = not blended) -> (max_weight [K] float32, hits [K] int64,
    weight_sum_q32 [K] int64) as the contribution pass defines them: a NaN weight counts as a hit, adds 0 to the sum and makes the maximum
    NaN.  w * 2^32 is exact in float64 and below 2^53: floor and the int64 sum are exact."""
    if mask is not None:
        w = torch.where(mask.reshape(1, *w.shape[1:]) != 0, w, torch.zeros_like(w))
    flat = w.reshape(w.shape[0], -1)
    nan = torch.isnan(flat)
    mx = flat.max(dim=1).values if flat.shape[1] else torch.zeros(flat.shape[0], device=w.device)   # (torch's max propagates NaN)
    hits = (flat != 0).sum(dim=1)
    q = torch.floor(torch.where(nan, torch.zeros_like(flat), flat).double() * Q32).to(torch.int64).sum(dim=1)
    return mx, hits, q


def yardstick(cloud, cam, so, ids, mask=None, **fwd):
    """The three statistics of the Gaussians `ids` (a list of row numbers) from ceil(len / 3) one-hot calls of the operator
    -> (max_weight, hits, weight_sum_q32), each [len(ids)]."""
    P = cloud["means3D"].shape[0]
    mx, hits, q = [], [], []
    for i in range(0, len(ids), 3):
        group = ids[i:i + 3]
        colors = torch.zeros(P, 3, device="cuda")
        for c, g in enumerate(group):
            colors[g, c] = 1.0
        img = render(cloud, cam, so, colors=colors, **fwd)[0]
        a, b, c_ = stats_of_weights(img[:len(group)], mask)
        mx.append(a), hits.append(b), q.append(c_)
    return torch.cat(mx), torch.cat(hits), torch.cat(q)


def assert_stats_equal(stats, want, ids=None):
    """torch.equal on all three arrays (max_weight compared on its bits where finite, NaN against NaN)."""
    sel = (lambda t: t) if ids is None else (lambda t: t[torch.as_tensor(ids, device=t.device)])
    mw, hits, q = sel(stats.max_weight), sel(stats.hits), sel(stats.weight_sum_q32)
    assert torch.equal(hits, want[1]), (hits, want[1])
    assert torch.equal(q, want[2]), (q, want[2])
    assert torch.equal(torch.isnan(mw), torch.isnan(want[0]))
    assert torch.equal(torch.nan_to_num(mw, nan=-1.0), torch.nan_to_num(want[0], nan=-1.0)), (mw, want[0])


def native_frame(_C, rs, cloud, **fwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians(rs.bg, cloud["means3D"], cloud["colors_precomp"], cloud["opacities"], cloud["scales"], cloud["rotations"], 1.0, e,
                                  rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height,
                                  rs.image_width, e, 0, rs.campos, False, False, **fwd)


def native_contrib(_C, rs, P, frame, max_weight, hits, weight_sum_q32, mask=None, **kw):
    return _C.render_contributions(frame[3], frame[4], frame[5], frame[0], P, rs.image_height, rs.image_width, max_weight, hits, weight_sum_q32,
                                   pixel_mask=mask, subpixel_offset=rs.subpixel_offset, **kw)


def fresh(P, poison=False):
    """Three output arrays: zeros, or poisoned (values an accumulate = 0 call must overwrite)."""
    if poison:
        return (torch.full((P,), 0.5, device="cuda"), torch.full((P,), 77, dtype=torch.int64, device="cuda"),
                torch.full((P,), 1 << 40, dtype=torch.int64, device="cuda"))
    return (torch.zeros(P, device="cuda"), torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(P, dtype=torch.int64, device="cuda"))
