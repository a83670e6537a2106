"""The projection-only pass (include/wg_rasterizer.h: wg_project_radii; csrc/project/project.hip; GaussianRasterizer.project_radii;
wg_fused_gaussians.VisibleRows.from_camera): a frame's radii before, and without, rendering it.

The gate has no tolerance: the pass restates the per-Gaussian kernel's geometry under that kernel's compiler flags, so every radius must be
the integer the forward call writes for the same inputs and camera (and, where the CPU oracle supports the mode, the oracle's).  Shapes are
the smallest at which the kernel can go wrong: a hand-built cloud that sits on every cull decision, clouds around the wave (63, 64, 65), inside
one 256-lane workgroup, across two (357) and across twenty (5000), on a 4 x 3 and a 10 x 8 tile grid."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import appearance_mlp_lib as L
import wg_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0 = 0.28209479177387814


def FG():
    import wg_fused_gaussians
    return wg_fused_gaussians


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cov3d(scales, rotations, scale_modifier):
    """cov3D_precomp of a scales / rotations cloud (float64 arithmetic, rounded once): another route to the same frame, not the same bits."""
    s, q = scales.astype(np.float64), rotations.astype(np.float64)
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                   2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    M = Rm * (s * scale_modifier)[:, None, :]
    Sg = M @ M.transpose(0, 2, 1)
    return np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).astype(np.float32)


def _as_mode(cloud, mode, scale_modifier=1.0):
    """The geometry arguments of one call mode from an activated scales / rotations cloud -> (dict for project_radii / forward, filter or None).
    "raw": log-scales, unnormalised quaternions, a 3-D filter value per Gaussian and logit opacities, as the caller's parameters are."""
    P = cloud["means3D"].shape[0]
    if mode == "precomp":
        return dict(means3D=cloud["means3D"], cov3D_precomp=_cov3d(cloud["scales"], cloud["rotations"], scale_modifier)), None
    if mode == "raw":
        stretch = (0.5 + (np.arange(P) % 5) * 0.75).astype(np.float32)[:, None]
        filt = (0.004 * (1 + np.arange(P) % 3)).astype(np.float32)[:, None]
        return dict(means3D=cloud["means3D"], scales=np.log(np.maximum(cloud["scales"], 1e-4)).astype(np.float32),
                    rotations=(cloud["rotations"] * stretch).astype(np.float32)), filt
    return dict(means3D=cloud["means3D"], scales=cloud["scales"], rotations=cloud["rotations"]), None


def _settings(cam, kernel_size=0.1, scale_modifier=1.0, degree=0):
    from wg_testlib import make_settings
    return make_settings(cam, degree, kernel_size=kernel_size, scale_modifier=scale_modifier)


def _forward_radii(rs, geom, filt, opacities):
    """radii of the forward call on the same inputs (precomputed colours: no radius depends on a colour)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: _dev(v) for k, v in geom.items()}
    P = t["means3D"].shape[0]
    with torch.no_grad():
        out = GaussianRasterizer(rs)(means2D=torch.zeros_like(t["means3D"]), opacities=_dev(opacities), colors_precomp=torch.full((P, 3), 0.5, device="cuda"),
                                     **t, **({} if filt is None else {"filter_3D": _dev(filt)}))
    return out[1]


def _project(rs, geom, filt):
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: _dev(v) for k, v in geom.items()}
    return GaussianRasterizer(rs).project_radii(**t, **({} if filt is None else {"filter_3D": _dev(filt)}))


def _oracle_radii(oracle, cam, geom, opacities, kernel_size, scale_modifier):
    e = np.zeros((0,), np.float32)
    P, H, W = geom["means3D"].shape[0], cam["height"], cam["width"]
    return oracle.rasterize_gaussians(np.zeros(3, np.float32), geom["means3D"], np.full((P, 3), 0.5, np.float32), opacities, geom.get("scales", e),
                                      geom.get("rotations", e), scale_modifier, geom.get("cov3D_precomp", e), cam["viewmatrix"], cam["projmatrix"],
                                      cam["tanfovx"], cam["tanfovy"], kernel_size, np.zeros((H, W, 2), np.float32), H, W, e, 0, cam["campos"])[2]


# ---- 1. the decision edges ----------------------------------------------------------------------------------------------------------------
EW, EH = 64, 48   # 4 x 3 tiles; focal length 55.4 pixels


@functools.lru_cache(maxsize=None)
def edge_cloud():
    """Each row is (x, y, z, isotropic scale).  The camera of S.make_camera(64, 48) has identity rotation at the origin, so vz == z exactly."""
    near = np.float32(0.2)
    rows = [
        (0.0, 0.0, near, 0.01),                                   # vz <= 0.2f: culled
        (0.0, 0.0, np.nextafter(near, np.float32(1)), 0.01),      # the next float: kept
        (0.02, -0.01, near, 1.0), (0.02, -0.01, np.nextafter(near, np.float32(1)), 1.0),
        (0.0, 0.0, -1.0, 0.05), (0.3, 0.2, -0.2, 2.0), (0.0, 0.0, 0.0, 0.05),   # behind the camera, and in its plane
        (0.0, 0.0, 2.0, 5.0), (0.4, -0.3, 3.0, 9.0),              # rectangle clamps to the whole grid
        (0.0, 0.0, 2.0, 0.0), (0.5, 0.3, 2.0, 0.0),               # zero scales: det == 0 without the mip filter, radius 2 with it
        (0.0, 0.0, 2.0, 0.02), (-1.0, 0.7, 2.0, 0.03), (1.1, -0.8, 2.0, 0.01), (0.3, 0.3, 9.5, 0.2),   # ordinary, on screen
        (1.155, 0.0, 2.0, 0.02), (-1.155, 0.0, 2.0, 0.02), (0.0, 0.866, 2.0, 0.02), (0.0, -0.866, 2.0, 0.02),   # centres at the frame's borders
    ]
    for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1)):             # centre ~72 pixels beyond each side of the frame
        x, y = sx * 2.6 * 1.0, sy * 2.31 * 1.0
        rows.append((x, y, 2.0, 0.01))                            # radius ~2: the rectangle misses the grid (ntiles == 0)
        rows.append((x, y, 2.0, 1.0))                             # radius ~85: it reaches the grid
        rows.append((x, y, 2.0, 0.85))                            # around the reach of the first tile column / row
        rows.append((x, y, 2.0, 0.7))
    a = np.asarray(rows, np.float32)
    P = a.shape[0]
    rng = np.random.default_rng(11)
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    aniso = np.ones((P, 3), np.float32)
    aniso[11:15] = np.asarray([[1.0, 0.4, 2.5]], np.float32)   # the ordinary ones: anisotropic, so that the rotation matters
    return dict(means3D=np.ascontiguousarray(a[:, :3]), scales=np.ascontiguousarray(a[:, 3:4] * aniso), rotations=q.astype(np.float32),
                opacities=np.full((P, 1), 0.7, np.float32))


@pytest.mark.parametrize("mode", ["scales_rotations", "precomp", "raw"])
@pytest.mark.parametrize("kernel_size", [0.0, 0.1])
@pytest.mark.parametrize("scale_modifier", [0.5, 1.0, 2.0])
def test_radii_equal_the_forward_calls_at_every_cull_decision(oracle, scale_modifier, kernel_size, mode):
    cloud, cam = edge_cloud(), S.make_camera(EW, EH)
    assert np.array_equal(cam["viewmatrix"], np.eye(4, dtype=np.float32))   # vz == z
    P = cloud["means3D"].shape[0]
    geom, filt = _as_mode(cloud, mode, scale_modifier)
    rs = _settings(cam, kernel_size, scale_modifier)
    got, want = _project(rs, geom, filt), _forward_radii(rs, geom, filt, cloud["opacities"])
    assert got.dtype == torch.int32 and got.shape == (P,) and got.device == want.device
    assert torch.equal(got, want), (got.cpu().numpy(), want.cpu().numpy())
    r = got.cpu().numpy()
    assert 0 < int((r > 0).sum()) < P
    assert r[0] == 0 and r[2] == 0 and not r[4:7].any()            # z = 0.2f, and behind
    assert r[1] > 0 and r[3] > 0                                    # nextafter(0.2f)
    assert r[7] > 0 and r[8] > 0
    if mode != "raw":   # (raw parameters cannot express a zero scale: exp() is positive and the filter adds to it)
        assert (r[9] > 0) == (kernel_size > 0) and (r[10] > 0) == (kernel_size > 0)
        assert not r[19::4].any()                                   # beyond each side, small: culled by ntiles == 0
        if scale_modifier >= 1.0:
            assert r[20::4].all()                                   # beyond each side, large: kept
        o = _oracle_radii(oracle, cam, geom, cloud["opacities"], kernel_size, scale_modifier)
        assert np.array_equal(r, o), (r, o)


# ---- 2. in bulk ---------------------------------------------------------------------------------------------------------------------------
YAWS = (0.0, 35.0, 75.0)   # the cloud fills a 66-degree wedge around +z: at 75 degrees part of it is behind the camera, the rest mostly off screen


@pytest.mark.parametrize("size", [(64, 48), (160, 120)], ids=["64x48", "160x120"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 357, 5000])
def test_radii_equal_the_forward_calls_in_bulk(oracle, P, size):
    W, H = size
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=40 + P, scale_mult=4.0)
    for yaw in YAWS:
        cam = S.make_camera(W, H, yaw_deg=yaw)
        rs = _settings(cam)
        for mode in ("scales_rotations", "precomp", "raw"):
            geom, filt = _as_mode(cloud, mode)
            got, want = _project(rs, geom, filt), _forward_radii(rs, geom, filt, cloud["opacities"])
            assert got.shape == (P,) and torch.equal(got, want), (yaw, mode)
            if mode != "raw" and P <= 357:
                assert np.array_equal(got.cpu().numpy(), _oracle_radii(oracle, cam, geom, cloud["opacities"], 0.1, 1.0)), (yaw, mode)
            if P >= 63:   # the frontal frame may keep everything and the turned-away one nothing; 35 degrees has both outcomes
                n = int((got > 0).sum())
                assert (yaw == 75.0 or n > 0) and (yaw == 0.0 or n < P), (yaw, mode, n)
        if P >= 63 and yaw == 75.0:
            vz = cloud["means3D"] @ cam["viewmatrix"][:3, 2] + cam["viewmatrix"][3, 2]
            assert 0 < int((vz <= 0.2).sum()) < P


def test_no_gaussians_give_an_empty_tensor():
    from diff_gaussian_rasterization import GaussianRasterizer
    rast = GaussianRasterizer(_settings(S.make_camera(64, 48)))
    z = lambda *s: torch.zeros(*s, device="cuda")
    for kw in (dict(scales=z(0, 3), rotations=z(0, 4)), dict(cov3D_precomp=z(0, 6)), dict(scales=z(0, 3), rotations=z(0, 4), filter_3D=z(0, 1))):
        r = rast.project_radii(z(0, 3), **kw)
        assert r.shape == (0,) and r.dtype == torch.int32 and r.is_cuda


# ---- 3. nothing else is written -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 65, 357])
def test_only_the_radii_are_written(P):
    from diff_gaussian_rasterization import _C
    GUARD = 300
    W, H = 64, 48
    cloud, cam = S.make_cloud(P, W, H, sh_degree=None, seed=7, scale_mult=4.0), S.make_camera(W, H, yaw_deg=35.0)
    rs = _settings(cam)
    t = {k: _dev(cloud[k]) for k in ("means3D", "scales", "rotations")}
    buf = torch.full((GUARD + P + GUARD,), -7, dtype=torch.int32, device="cuda")
    inputs_before = {k: v.clone() for k, v in t.items()}
    a = _C._ProjectArgs()
    a.struct_size = C.sizeof(a)
    a.P, a.width, a.height = P, W, H
    a.means3D, a.scales, a.rotations = (t[k].data_ptr() for k in ("means3D", "scales", "rotations"))
    a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, rs.tanfovx, rs.tanfovy, rs.kernel_size
    a.viewmatrix, a.projmatrix = rs.viewmatrix.data_ptr(), rs.projmatrix.data_ptr()
    a.radii = buf.data_ptr() + 4 * GUARD
    a.stream = torch.cuda.current_stream().cuda_stream
    assert _C._lib.wg_project_radii(C.byref(a)) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -7).all()) and bool((buf[GUARD + P:] == -7).all())
    assert bool((buf[GUARD:GUARD + P] >= 0).all())
    assert torch.equal(buf[GUARD:GUARD + P], _project(rs, {k: cloud[k] for k in t}, None))
    assert all(torch.equal(t[k], inputs_before[k]) for k in t)


# ---- 4. the list ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["scales_rotations", "precomp", "raw"])
def test_from_camera_builds_the_list_of_the_forward_calls_radii(mode):
    from diff_gaussian_rasterization import GaussianRasterizer
    fg = FG()
    W, H, P = 64, 48, 5000
    cloud, cam = S.make_cloud(P, W, H, sh_degree=None, seed=9, scale_mult=4.0), S.make_camera(W, H, yaw_deg=35.0)
    geom, filt = _as_mode(cloud, mode)
    rs = _settings(cam)
    want_radii = _forward_radii(rs, geom, filt, cloud["opacities"])
    want = fg.VisibleRows.from_radii(want_radii)
    t = {k: _dev(v) for k, v in geom.items()}
    extra = {} if filt is None else dict(filter_3D=_dev(filt), opacities=_dev(cloud["opacities"]))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")   # (where this torch build honours it: a host synchronisation inside from_camera raises)
    try:
        got = fg.VisibleRows.from_camera(GaussianRasterizer(rs), **t, **extra)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert isinstance(got, fg.VisibleRows) and got.P == want.P == P and got.M == want.M == P
    assert got.count.is_cuda and got.count.dtype == torch.int32 and got.count.shape == (1,)
    n = int(want.count)
    assert 0 < n < P and int(got.count) == n
    assert torch.equal(got.index[:n], want.index[:n])
    assert torch.equal(got.radii, want_radii) and want.radii is None


def test_the_pass_is_captured_and_replayed_on_other_positions():
    """No allocation, no host wait, no atomics: the launch is captured in a graph, and a replay follows the positions of the replay."""
    from diff_gaussian_rasterization import _C
    W, H, P = 64, 48, 357
    cloud, cam = S.make_cloud(P, W, H, sh_degree=None, seed=5, scale_mult=4.0), S.make_camera(W, H)
    rs = _settings(cam)
    t = {k: _dev(cloud[k]) for k in ("means3D", "scales", "rotations")}
    args = lambda: (t["means3D"], t["scales"], t["rotations"], None, None, 1.0, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, H, W)
    moved = t["means3D"].clone()
    moved[:, 0] += 0.8 * moved[:, 2]   # towards, and beyond, the right border
    first = _C.project_radii(*args())
    here = t["means3D"].clone()
    t["means3D"].copy_(moved)
    second = _C.project_radii(*args())
    t["means3D"].copy_(here)
    assert not torch.equal(first, second)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _C.project_radii(*args())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    t["means3D"].copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, second)


# ---- 5. the step it exists for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw-parameters"])
@pytest.mark.parametrize("max_workgroups", [1, 0])
def test_rows_from_the_camera_in_front_of_one_two_tone_call(max_workgroups, raw):
    """"Dense MLP, then ONE sh_second=True call" against "from_camera, then the MLP over the listed rows, then the same call": both images,
    radii, the loss and every per-row gradient (features, per-Gaussian embedding, geometry) bit for bit -- an unlisted row's tone is never
    read and its cotangent is zero.  The weight gradients and the shared embedding's are sums over rows and are compared at
    max_workgroups = 1 only, for the reason tests/test_appearance_rows.py::test_consistency_with_the_rasterizer gives: one workgroup's
    partial is one chain over its rows in order and zero cotangents add exact zeros, while several workgroups group the rows differently in
    the dense walk and in the list."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from wg_testlib import to_dev
    fg = FG()
    Wd, Hd, P, G, E, DEG = 64, 48, 357, 24, 32, 3
    cam = S.make_camera(Wd, Hd)
    cot, cot2 = to_dev(S.make_cotangent(Wd, Hd)), to_dev(S.make_cotangent(Wd, Hd, seed=2))
    cloud = S.make_cloud(P, Wd, Hd, sh_degree=DEG, seed=3, scale_mult=4.0)
    geom_np, filt = _as_mode(cloud, "raw" if raw else "scales_rotations")
    opac = np.log(cloud["opacities"] / (1 - cloud["opacities"])).astype(np.float32) if raw else cloud["opacities"]
    rs = _settings(cam, degree=DEG)
    g = torch.Generator().manual_seed(5)
    gemb0, aemb0 = torch.rand(P, G, generator=g) * 2 - 1, torch.randn(E, generator=g) * 0.3
    weights = L.draw_weights(3 + G + E, 77)
    names = ["W1", "b1", "W2", "b2", "W3", "b3"]
    results, frames, counts = [], [], []
    for use_rows in (False, True):
        geom = {k: to_dev(v).requires_grad_(True) for k, v in geom_np.items()}
        geom["opacities"] = to_dev(opac).requires_grad_(True)
        geom["means2D"] = torch.zeros_like(geom["means3D"], requires_grad=True)
        feats = to_dev(cloud["shs"]).reshape(P, 48).requires_grad_(True)
        gemb, aemb = gemb0.cuda().requires_grad_(True), aemb0.cuda().requires_grad_(True)
        Wt = [w.cuda().requires_grad_(True) for w in weights]
        extra = {} if filt is None else dict(filter_3D=to_dev(filt))
        rast = GaussianRasterizer(rs)
        rows = None
        if use_rows:   # BEFORE the frame is rendered: no raw call, no second projection
            rows = fg.VisibleRows.from_camera(rast, geom["means3D"], geom["scales"], geom["rotations"], **extra)
            counts.append(int(rows.count))
        offset, mul = torch.split(fg.appearance_mlp((feats[:, :3], gemb), Wt, shared=aemb, max_workgroups=max_workgroups, rows=rows), [3, 3], dim=-1)
        toned, radii, _, plain = rast(shs=feats.view(P, 16, 3), sh_mul=mul, sh_offset=offset / C0, sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0,
                                      sh_second=True, sh_pre_clamp_max2=1.0, deterministic_backward=True, **geom, **extra)
        loss = (toned * cot).sum() + (plain * cot2).sum()
        loss.backward()
        if use_rows:
            assert torch.equal(rows.radii, radii)
        frames.append((toned.detach(), plain.detach(), radii))
        per_row = dict(loss=loss.detach(), features=feats.grad, gemb=gemb.grad, **{k: v.grad for k, v in geom.items()})
        summed = dict(aemb=aemb.grad, **{n: w.grad for n, w in zip(names, Wt)})
        results.append((per_row, summed))
    n = int((frames[0][2] > 0).sum())
    assert 0 < n < P and counts == [n]   # the frame culls some rows and keeps some
    for a, b in zip(*frames):
        assert torch.equal(a, b)
    (dr, ds), (rr, rsum) = results
    assert len(dr) == 8
    for k in dr:
        assert dr[k] is not None and torch.equal(dr[k], rr[k]), k
    assert bool(dr["features"].any()) and bool(dr["gemb"].any()) and bool(dr["means3D"].any())
    if max_workgroups == 1:
        assert len(ds) == 7
        for k in ds:
            assert ds[k] is not None and torch.equal(ds[k], rsum[k]), k


# ---- 6. both bindings ------------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [{root!r}, {pkg!r}]
import wg_scenes as S
from diff_gaussian_rasterization import _C
assert _C.binding_name() == {name!r}, _C.binding_name()
W, H, P = 160, 120, 5000
cloud, cam = S.make_cloud(P, W, H, sh_degree=None, seed=13, scale_mult=4.0), S.make_camera(W, H, yaw_deg=35.0)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
r = _C.project_radii(d(cloud["means3D"]), d(cloud["scales"]), d(cloud["rotations"]), None, None, 1.0, d(cam["viewmatrix"]), d(cam["projmatrix"]),
                     cam["tanfovx"], cam["tanfovy"], 0.1, H, W)
f = _C.project_radii(d(cloud["means3D"]), d(np.log(cloud["scales"])), d(cloud["rotations"] * 3), None, torch.full((P, 1), 0.01, device="cuda"), 1.0,
                     d(cam["viewmatrix"]), d(cam["projmatrix"]), cam["tanfovx"], cam["tanfovy"], 0.1, H, W)
np.save({out!r}, np.stack([r.cpu().numpy(), f.cpu().numpy()]))
"""


def test_both_bindings_give_the_same_radii(tmp_path):
    """WG_BINDING=ctypes and the compiled binding, each in a fresh child process whose import picks the binding from the environment."""
    import glob
    assert glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")), "the compiled binding has not been built"
    got = {}
    for name in ("ctypes", "torch"):
        out = str(tmp_path / f"{name}.npy")
        code = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "wild-gaussians_amd"), name=name, out=out)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, WG_BINDING=name), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[name] = np.load(out)
    assert got["ctypes"].shape == (2, 5000) and np.array_equal(got["ctypes"], got["torch"])
    assert 0 < int((got["ctypes"][0] > 0).sum()) < 5000 and not np.array_equal(got["ctypes"][0], got["ctypes"][1])
