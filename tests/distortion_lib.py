"""Helpers of tests/test_distortion.py: scenes, the operator's calls and the yardsticks of the distortion pass (wg_render_distortion /
wg_distortion_grad).  None of them runs the code under test:

Y-w   the operator's own forward call with one-hot precomputed colours over a zero background (tests/contributions_lib.py: yardstick) gives each
      Gaussian's blend weight w = alpha * T per pixel bit for bit; sum_{j<i} w_i w_j (v_i - v_j)^2 is then formed in float64.
Y-32  the route a caller had before: a call with colors_precomp = (1, v, v^2) over a zero background renders (A, D, Q); dist = A Q - D^2; its
      gradient is that call's backward pass under the cotangent (g Q, -2 g D, g A) formed in float64 from the run's own image;
      dL/dv = dcol[:, 1] + 2 v dcol[:, 2], and in distance mode the direct term dL/dv (x - campos) / v added in float64.  Run through the operator
      (float32) and through oracle.run_scene(precision="f32").
Y-64  the same through the float64 oracle."""
import numpy as np
import torch

import wg_scenes as S
from wg_testlib import make_settings, rel_err, to_dev

EPS = 2.0 ** -24   # float32 unit roundoff
ORDER_BAR = 2e-6   # two orders of the same float32 sums (tests/test_colour_backward.py, docs/OPTIONS.md)
GRAD_BAR = 1e-3    # the project's gradient bar
BG = (0.2, 0.5, 0.8)
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")
# the scenes of tests/test_render_depth_grad.py: name -> P, W, H, scale_mult, random sub-pixel offsets, seed.
# "saturating" is drawn with seed 5 instead of that file's 11: the gradient tests need the float32 oracle's route to lie within 2.5e-4 of the
# float64 oracle's, and with seed 11 it does not (scales 8.7e-4: a threshold decision that differs between the two precisions); with seed 5 the
# largest difference is 2.5e-6 (ragged 1.8e-4, plain 2.2e-5) -- measured on the CPU, no code under test involved.
SCENES = {
    "ragged": (8000, 250, 130, 3.0, True, 11),        # partial tiles
    "saturating": (1500, 320, 200, 12.0, False, 5),   # long lists, pixels that stop early through n_contrib
    "plain": (10000, 256, 256, 1.0, False, 11),
}
ROUTE_BAR = 2.5e-4   # the condition on a scene: the float32 oracle's route against the float64 oracle's

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def with_cotangents(cloud, cam, so=None, v=None):
    """-> dict(cloud: numpy arrays, cam, so, cot: image cotangent [3,H,W], cot_t: distortion cotangent [H,W], v: the float32 scalars -- the
    distances to the camera as torch computes them unless given)"""
    W, H = cam["width"], cam["height"]
    if v is None:
        v = torch.norm(torch.from_numpy(cloud["means3D"]) - torch.from_numpy(np.asarray(cam["campos"], np.float32))[None], dim=-1).numpy()
    return dict(cloud=cloud, cam=cam, so=so, cot=S.make_cotangent(W, H), cot_t=np.ascontiguousarray(3.0 * S.make_cotangent(W, H, seed=7)[0]),
                v=np.ascontiguousarray(v, np.float32))


def make_scene(name):
    if name == "dense":   # ~1000 instances per tile: lists the lazy sort engages on at test thresholds
        P, W, H, sm, offsets, seed = 30000, 320, 200, 7.0, False, 5
    else:
        P, W, H, sm, offsets, seed = SCENES[name]
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=seed, scale_mult=sm)
    so = np.random.default_rng(3).uniform(-0.5, 0.5, size=(H, W, 2)).astype(np.float32) if offsets else None
    return with_cotangents(cloud, S.make_camera(W, H), so)


def scene(name):
    return cached(("scene", name), lambda: make_scene(name))


def one_tile(P, v=None):
    """tests/test_render_depth.py's recipe (contributions_lib.one_tile), as a scene dict: one 16 x 16 tile, P faint Gaussians that all cover it."""
    rng = np.random.default_rng(P)
    z = rng.uniform(2.0, 8.0, size=P)
    means = np.stack([0.02 * z * rng.uniform(-1, 1, size=P), 0.02 * z * rng.uniform(-1, 1, size=P), z], axis=1)
    scales = (1.5 * z)[:, None] * np.ones((P, 3))
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    cloud = dict(means3D=means, scales=scales, rotations=q, opacities=np.full((P, 1), 0.01), colors_precomp=rng.uniform(0, 1, size=(P, 3)))
    return with_cotangents({k: np.ascontiguousarray(a, dtype=np.float32) for k, a in cloud.items()}, S.make_camera(16, 16), v=v)


def leaves(sc):
    t = {k: to_dev(a).requires_grad_(True) for k, a in sc["cloud"].items()}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    return t


def geo(t):
    return dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])


def grads(t, **more):
    g = {k: None if t[k].grad is None else t[k].grad.detach().cpu().numpy().astype(np.float64) for k in GEOMETRY + ("colors_precomp",) if k in t}
    g.update(more)
    return g


def settings(sc, bg=BG):
    return make_settings(sc["cam"], 0, bg=np.array(bg, np.float32), subpixel_offset=sc["so"])


def forward_map(sc, mode, exact=True, v=None, **fwd):
    """The code under test, forward only (under no_grad) -> the distortion map [H, W] as a device tensor."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    source = "distance" if mode == "distance" else to_dev(sc["v"] if v is None else v)
    with torch.no_grad():
        out = GaussianRasterizer(settings(sc))(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"],
                                               rotations=t["rotations"], colors_precomp=t["colors_precomp"], return_distortion=source,
                                               exact_compositing=bool(exact), **fwd)
    return out[-1]


def new_call(sc, mode, image=True, exact=True, **fwd):
    """The code under test: one call with return_distortion= and distortion_grad=True, a loss on the map (and on the image)
    -> dict(grads, dist, color)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = leaves(sc)
    values = to_dev(sc["v"]).requires_grad_(True) if mode == "values" else None
    out = GaussianRasterizer(settings(sc))(**geo(t), colors_precomp=t["colors_precomp"], return_distortion="distance" if values is None else values,
                                           distortion_grad=True, exact_compositing=bool(exact), **fwd)
    dist = out[-1]
    assert dist.requires_grad
    loss = (dist * to_dev(sc["cot_t"])).sum()
    if image:
        loss = loss + (out[0] * to_dev(sc["cot"])).sum()
    loss.backward()
    return dict(grads=grads(t, values=None if values is None else values.grad.detach().cpu().numpy().astype(np.float64)),
                dist=dist.detach().cpu().numpy(), color=out[0].detach().cpu().numpy())


# ---- Y-32 / Y-64: the (1, v, v^2) route ---------------------------------------------------------------------------------------------------
def moment_colours(v):
    """colors_precomp = (1, v, v^2), float32 (v^2 rounded once)"""
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(np.stack([np.ones_like(v), v, v * v], axis=1))


def route_cotangent(image, g):
    """(g Q, -2 g D, g A) in float64 from the route's own image (A, D, Q)"""
    A, D, Q = (np.asarray(image[c], np.float64) for c in range(3))
    g = np.asarray(g, np.float64)
    return np.stack([g * Q, -2.0 * g * D, g * A])


def values_gradient(dcol, v):
    dcol = np.asarray(dcol, np.float64).reshape(-1, 3)
    return dcol[:, 1] + 2.0 * np.asarray(v, np.float64) * dcol[:, 2]


def direct_term(sc, dv):
    """dL/dv (x - campos) / v in float64, 0 where v == 0"""
    d = sc["cloud"]["means3D"].astype(np.float64) - np.asarray(sc["cam"]["campos"], np.float64)[None]
    v = np.linalg.norm(d, axis=1)
    return np.where(v[:, None] > 0, dv[:, None] * d / np.where(v > 0, v, 1.0)[:, None], 0.0)


def sum_routes(sc, one, two, mode, image):
    """The image call's gradients (`one`, or None) and the route's (`two`, with dL/dv under "values") added in float64."""
    out = {}
    for k in GEOMETRY:
        out[k] = np.asarray(two[k], np.float64) + (np.asarray(one[k], np.float64) if image else 0.0)
    out["values"] = np.asarray(two["values"], np.float64)
    if mode == "distance":
        out["means3D"] = out["means3D"] + direct_term(sc, out["values"])
    return out


def operator_image_call(sc, exact=True, **fwd):
    """the same call without the keyword under the image cotangent -> gradients"""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = leaves(sc)
    out = GaussianRasterizer(settings(sc))(**geo(t), colors_precomp=t["colors_precomp"], exact_compositing=bool(exact), **fwd)
    out[0].backward(to_dev(sc["cot"]))
    return grads(t)


def operator_route(sc, exact=True, v=None, backward=True, **fwd):
    """Y-32 through the operator -> dict(image [3,H,W] float32 numpy = (A, D, Q), dist32: the float32 composition A * Q - D * D formed by torch
    on the device, and with backward=True the route's gradients + "values")"""
    from diff_gaussian_rasterization import GaussianRasterizer
    v = sc["v"] if v is None else np.asarray(v, np.float32)
    t = leaves(sc)
    colors = to_dev(moment_colours(v)).requires_grad_(backward)
    rs = make_settings(sc["cam"], 0, subpixel_offset=sc["so"])   # a zero background
    out = GaussianRasterizer(rs)(**geo(t), colors_precomp=colors, exact_compositing=bool(exact), **fwd)
    img = out[0].detach()
    res = dict(image=img.cpu().numpy(), dist32=(img[0] * img[2] - img[1] * img[1]).cpu().numpy())
    if backward:
        cot3 = torch.from_numpy(route_cotangent(res["image"], sc["cot_t"]).astype(np.float32)).cuda()
        out[0].backward(cot3)
        res["grads"] = grads(t, values=values_gradient(colors.grad.detach().cpu().numpy(), v))
    return res


def oracle_image_call(oracle, sc, precision):
    o = oracle.run_scene(sc["cloud"], sc["cam"], sh_degree=0, cotangent=sc["cot"], bg=np.array(BG, np.float32), subpixel_offset=sc["so"], precision=precision)
    P = sc["cloud"]["means3D"].shape[0]
    return {k: np.asarray(o["grads"][k], np.float64).reshape(P, -1) for k in GEOMETRY}


def oracle_route(oracle, sc, precision):
    """Y-32 / Y-64 through the oracle -> the route's gradients + "values", and its own map "dist" = A Q - D^2 formed in float64 from its image"""
    dt = np.float32 if precision == "f32" else np.float64
    cloud = dict(sc["cloud"], colors_precomp=moment_colours(sc["v"]))
    fwd = oracle.run_scene(cloud, sc["cam"], sh_degree=0, subpixel_offset=sc["so"], precision=precision)
    image = np.asarray(fwd["color"], np.float64)
    cot3 = np.ascontiguousarray(route_cotangent(image, sc["cot_t"]).astype(dt))
    o = oracle.run_scene(cloud, sc["cam"], sh_degree=0, cotangent=cot3, subpixel_offset=sc["so"], precision=precision)
    P = sc["cloud"]["means3D"].shape[0]
    g = {k: np.asarray(o["grads"][k], np.float64).reshape(P, -1) for k in GEOMETRY}
    g["values"] = values_gradient(o["grads"]["colors_precomp"], sc["v"])
    g["dist"] = image[0] * image[2] - image[1] * image[1]
    return g


def errors(got, ref, mode):
    """name -> rel_err over the gradients the issue lists (values: values mode only; in distance mode dL/dv reaches means3D)"""
    names = GEOMETRY + (("values",) if mode == "values" else ())
    return {k: rel_err(np.asarray(got[k]).reshape(np.asarray(ref[k]).shape), ref[k]) for k in names}


# ---- Y-w: exact weights ---------------------------------------------------------------------------------------------------------------------
def exact_weights(sc, exact=True, **fwd):
    """w [P, H, W] float32 (device): each Gaussian's blend weight per pixel, bit for bit, from ceil(P / 3) one-hot calls of the operator
    (contributions_lib.yardstick's trick: channel c of the forward kernel is fma(1, w, 0) = w at its Gaussian and fma(0, w', C) = C elsewhere)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    P = t["means3D"].shape[0]
    rs = make_settings(sc["cam"], 0, subpixel_offset=sc["so"])
    w = torch.zeros(P, sc["cam"]["height"], sc["cam"]["width"], device="cuda")
    with torch.no_grad():
        for i in range(0, P, 3):
            n = min(3, P - i)
            colors = torch.zeros(P, 3, device="cuda")
            for c in range(n):
                colors[i + c, c] = 1.0
            img = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"],
                                         rotations=t["rotations"], colors_precomp=colors, exact_compositing=bool(exact), **fwd)[0]
            w[i:i + n] = img[:n]
    return w


def tile_order(sc, exact=True):
    """The Gaussian ids of a one-tile scene's list, front to back (the frame's own sorted list)."""
    from diff_gaussian_rasterization import _C
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    rs = make_settings(sc["cam"], 0, subpixel_offset=sc["so"])
    e = torch.Tensor([])
    f = _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                               rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0, rs.campos, False, False,
                               options=dict(exact_compositing=int(bool(exact))))
    assert rs.image_height <= 16 and rs.image_width <= 16
    return _C.view_binning(f[4], f[0])["point_list"].cpu().numpy().astype(np.int64)


def exact_distortion(w, v, order):
    """Y-w in float64 from the weights [P, H, W], the float32 scalars [P] and the list order -> dict(dist, and the magnitudes of the centred bound:
    A, S1 = sum w |u|, S2 = sum w u^2 with u = v - c, c the v of each pixel's first blended instance in list order; n = the list's length)."""
    w = w.double().cpu().numpy()[order]                 # [n, H, W] front to back
    v = np.asarray(v, np.float64)[order]
    blended = w > 0
    first = np.argmax(blended, axis=0)                  # the first blended instance per pixel (0 where none: its weights are 0 anyway)
    c = v[first]
    u = v[:, None, None] - c[None]
    A = w.sum(axis=0)
    S1 = (w * np.abs(u)).sum(axis=0)
    S2 = (w * u * u).sum(axis=0)
    D = (w * u).sum(axis=0)
    # the pair sum itself, not the moments: sum_{j<i} w_i w_j (v_i - v_j)^2 = 1/2 sum_{i,j}
    pair = np.zeros_like(A)
    for i in range(w.shape[0]):
        pair += w[i] * (w[:i] * (v[i] - v[:i])[:, None, None] ** 2).sum(axis=0)
    assert np.abs(pair - (A * S2 - D * D)).max() <= 1e-9 * max(1.0, float(np.abs(pair).max()))   # (the identity, in float64)
    return dict(dist=pair, A=A, S1=S1, S2=S2, n=int(w.shape[0]))


def centred_bound(y, extra_n=0):
    """The a-priori bound of |computed - exact| per pixel for distortion.hip's arithmetic, eps = 2^-24, n = the list's length:
      u^ = fl(v - c): one rounding;  A^: n - 1 additions -> (n - 1) eps A;
      D'^: the first term is 0, every other passes at most n - 1 fused multiply-adds, + u^'s rounding -> n eps S1;
      Q'^: u^ * u^ carries 2 eps from u^ and 1 from its own rounding, + n - 1 fused multiply-adds -> (n + 2) eps S2;
      A^ Q'^: (2n + 1) eps A S2;  fl(D'^ D'^): 2 n eps S1^2 + 1 eps S1^2;  the final fused multiply-add: eps |dist| <= eps A S2;
    first order in total (2n + 2) eps A S2 + (2n + 1) eps S1^2 <= (2n + 2) eps (A S2 + S1^2); one more unit covers the second-order terms
    ((2n + 2)^2 eps < 1 for every n here):  k(n) = 2n + 3."""
    n = y["n"] + extra_n
    return (2 * n + 3) * EPS * (y["A"] * y["S2"] + y["S1"] ** 2)
