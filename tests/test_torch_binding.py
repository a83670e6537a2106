"""The compiled torch binding of the C-ABI (wild-gaussians_amd/csrc/torch_binding.cpp -> diff_gaussian_rasterization/_C_torch*.so; INTEGRATION.md
section 2 as a file that builds): the reference's pybind11 surface (ext.cpp:15-19, rasterize_points.h:18-71) on top of libwg_rasterizer.so.
Held to the ctypes binding, which is the default and carries the opt-ins beyond that surface."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
import wg_scenes as S  # noqa: E402

built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
needs_binding = pytest.mark.skipif(not built, reason="compiled binding not built (python wild-gaussians_amd/build.py --torch-binding)")


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)   # (what the process was started with: WG_BINDING, or the default)


@needs_binding
def test_compiled_binding_has_the_reference_modules_surface_and_errors(binding):
    _C = binding
    from diff_gaussian_rasterization import _C_torch as m
    assert {"rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible", "rasterize_gaussians_ex", "rasterize_gaussians_backward_ex"} <= set(dir(m))
    e = torch.Tensor([])
    args = lambda m3: (torch.zeros(3), m3, e, torch.zeros(5, 1), e, e, 1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, 0.1, e, 8, 8, e, 0, torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="num_points, 3"):      # rasterize_points.cu:59-61
        m.rasterize_gaussians(*args(torch.zeros(5, 2)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.rasterize_gaussians(*args(torch.zeros(5, 3)))
    assert _C.binding_name() == "torch"          # the default when it has been built (round 5)
    assert _C.use_binding("ctypes") == "torch" and _C.binding_name() == "ctypes" and _C.use_binding("torch") == "ctypes" and _C.binding_name() == "torch"
    with pytest.raises(ValueError):
        _C.use_binding("pybind")


@pytest.mark.gpu
@needs_binding
@pytest.mark.parametrize("colors", ["sh", "precomp"])
def test_compiled_binding_gives_the_ctypes_bindings_results(binding, colors):
    """Same library underneath: images, radii, accumulation and the image state bit-identical; gradients to the atomics' run-to-run
    rounding; markVisible equal; through the native functions and through the autograd operator."""
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.wg_testlib import make_settings, run_hip, run_hip_native, to_dev
    P, W, H = 120_000, 800, 450
    deg = 2 if colors == "sh" else None
    cloud = S.make_cloud(P, W, H, sh_degree=deg, seed=21, scale_mult=2.0)
    cam = S.make_camera(W, H, yaw_deg=-4.0)
    cot = S.make_cotangent(W, H, seed=8)
    d = deg if deg is not None else 0
    out = {}
    for name in ("ctypes", "torch"):
        _C.use_binding(name)
        assert _C.binding_name() == name
        h = run_hip(cloud, cam, sh_degree=d, cotangent=cot)
        n = run_hip_native(cloud, cam, sh_degree=d)
        vis = _C.mark_visible(to_dev(cloud["means3D"]), to_dev(cam["viewmatrix"]), to_dev(cam["projmatrix"]))
        out[name] = dict(h=h, n_contrib=n["views"]["image"]["n_contrib"].cpu().numpy(), final_T=n["views"]["image"]["final_T"].cpu().numpy(),
                         R=int(n["num_rendered"]), vis=vis.cpu().numpy())
    a, b = out["ctypes"], out["torch"]
    assert a["R"] == b["R"] > 0 and np.array_equal(a["vis"], b["vis"]) and a["vis"].dtype == np.bool_
    for k in ("color", "radii", "accumulation"):
        assert np.array_equal(a["h"][k], b["h"][k]), k
    assert np.array_equal(a["n_contrib"], b["n_contrib"]) and np.array_equal(a["final_T"], b["final_T"])
    assert set(a["h"]["grads"]) == set(b["h"]["grads"])
    for k, g in a["h"]["grads"].items():
        assert float(np.abs(g - b["h"]["grads"][k]).max()) <= 4e-6 * float(np.abs(g).max()) + 1e-30, k
    # no Gaussians: zero image, empty radii, nothing launched (rasterize_points.cu:83)
    _C.use_binding("torch")
    rs = make_settings(cam, 0)
    z = lambda *s: torch.zeros(*s, device="cuda")
    img, radii, acc = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    assert img.shape == (3, H, W) and not img.any() and radii.numel() == 0 and acc.shape == (H, W)


@pytest.mark.gpu
@needs_binding
@pytest.mark.parametrize("name", ["torch", "ctypes"])
def test_wrong_size_tensors_raise_instead_of_reading_out_of_bounds(binding, name):
    """the compiled binding is the default and its fast path skips the Python-side checks, so it repeats them itself -- a
    filter_3D / colors_precomp2 / raw tuple of the wrong length, or filter_3D combined with colors_precomp2, must raise under BOTH
    bindings (the preprocess kernels would otherwise index P entries of a shorter tensor)."""
    _C = binding
    _C.use_binding(name)
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.wg_testlib import make_settings, to_dev
    P, W, H = 2000, 160, 96
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=3)
    rast = GaussianRasterizer(make_settings(S.make_camera(W, H), 0))
    t = {k: to_dev(v) for k, v in cloud.items()}
    base = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    col = t["colors_precomp"]
    with pytest.raises((RuntimeError, Exception), match="filter_3D"):
        rast(**base, colors_precomp=col, filter_3D=torch.ones(P - 7, device="cuda"))
    with pytest.raises((RuntimeError, Exception), match="colors2|colors_precomp2"):
        rast(**base, colors_precomp=col, colors_precomp2=col[: P - 1])
    with pytest.raises((RuntimeError, Exception), match="colors2|colors_precomp2"):
        rast(**base, colors_precomp=col[: P - 1].contiguous(), colors_precomp2=col)
    with pytest.raises((RuntimeError, Exception), match="filter_3D"):
        rast(**base, colors_precomp=col, colors_precomp2=col, filter_3D=torch.ones(P, device="cuda"))
    # the reference-shaped arguments too (the reference's own binding checks none of them)
    with pytest.raises(RuntimeError, match="scales"):
        rast(**{**base, "scales": t["scales"][: P - 3].contiguous()}, colors_precomp=col)
    with pytest.raises(RuntimeError, match="opacities"):
        rast(**{**base, "opacities": t["opacities"][: P - 3].contiguous()}, colors_precomp=col)
    # the raw tuple of the backward call
    e = torch.Tensor([])
    rs = rast.raster_settings
    R, color, radii, gb, bb, ib = _C.rasterize_gaussians(rs.bg, t["means3D"], col, t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                         rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, H, W, e, 0, rs.campos, False, False)[:6]
    with pytest.raises(RuntimeError, match="raw"):
        _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, col, t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
                                        rs.kernel_size, rs.subpixel_offset, torch.zeros(3, H, W, device="cuda"), e, 0, rs.campos, gb, R, bb, ib, False,
                                        raw=(torch.ones(P - 5, device="cuda"), t["opacities"]))
    # and a well-formed call still works afterwards
    img = rast(**base, colors_precomp=col)[0]
    assert torch.isfinite(img).all()


# ---- one table of calls for both bindings' argument checks -----------------------------------------------------------------------------
# A call mode is a well-formed argument set (_mode_arguments); a case is a mode, the call it is made through ("fwd" / "bwd"), one edit
# that breaks exactly one check, and that check's message (None, None: the well-formed call of the mode, which must pass).
FILTER_MSG = "filter_3D (raw-parameter mode) needs scales and rotations, P filter values, and neither colors2 nor binning_capacity"
COLORS2_MSG = "colors2 needs precomputed colours of P x 3 in both sets (no SH, no sh_tone, no binning_capacity)"
ROWS_MSG = "a per-Gaussian argument of the backward call does not have P rows"
OPTIONS = (1, 0, 1)   # CALL_OPTION_DEFAULTS, given per call: the table does not depend on the thread's defaults


def _mode_arguments(mode, P, H, W, device):
    e = torch.Tensor([])
    sh_mode = mode in ("sh", "sh_tone", "sh_second")
    cloud = {k: torch.from_numpy(v).to(device) for k, v in S.make_cloud(P, W, H, sh_degree=2 if sh_mode else None, seed=5, scale_mult=4.0).items()}
    g = torch.Generator().manual_seed(7)
    rand = lambda *shape: torch.rand(*shape, generator=g).to(device)
    A = dict(means3D=cloud["means3D"], colors=cloud.get("colors_precomp", e), opacity=cloud["opacities"], scales=cloud["scales"],
             rotations=cloud["rotations"], cov3D_precomp=e, sh=cloud.get("shs", e), degree=2 if sh_mode else 0, debug=False, fwd={}, bwd={},
             radii=torch.ones(P, dtype=torch.int32, device=device), dL=rand(3, H, W) / (3 * H * W))
    if mode in ("sh_tone", "sh_second"):
        A["fwd"]["sh_tone"] = A["bwd"]["sh_tone"] = (0.5 + rand(P, 3), 0.1 * rand(P, 3), 1.0, 1.0)
    if mode == "sh_second":
        A["fwd"]["sh_second"] = A["bwd"]["sh_second"] = (None, None, 1.0, None)
    if mode == "colors2":
        A["fwd"]["colors2"] = rand(P, 3)
    if mode in ("sh_second", "colors2"):
        A["bwd"]["dL_dout_color2"] = rand(3, H, W) / (3 * H * W)
    if mode == "raw":   # opacity / scales / rotations are the raw parameters
        A["opacity"], A["scales"] = torch.logit(A["opacity"]), torch.log(A["scales"])
        A["fwd"]["filter_3D"] = 0.001 * rand(P, 1)
        A["bwd"]["raw"] = (A["fwd"]["filter_3D"], A["opacity"])
    if mode == "fixed":
        A["fwd"]["binning_capacity"] = 4096   # (64 Gaussians on four tiles: at most 256 instances)
    return A


def _set(key, value, sub=None):
    """An edit of the argument set: value(A, P) -> A[key], or A[sub][key]."""
    def edit(A, P):
        (A if sub is None else A[sub])[key] = value(A, P)
    return edit


def _short(key, rows):
    return _set(key, lambda A, P: A[key][: P - rows])


CASES = [(f"{call}-{mode}-well-formed", call, mode, None, None) for call, modes in
         (("fwd", ("precomp", "sh", "sh_tone", "sh_second", "colors2", "raw", "fixed")), ("bwd", ("precomp", "sh", "sh_tone", "sh_second", "colors2", "raw")))
         for mode in modes] + [
    ("colors_precomp", "fwd", "precomp", _short("colors", 3), "colors_precomp must have 3 * P elements"),
    ("opacities-short", "fwd", "precomp", _short("opacity", 3), "opacities must have 1 * P elements"),
    ("opacities-absent", "fwd", "precomp", _set("opacity", lambda A, P: torch.Tensor([])), "opacities must have P elements"),
    ("scales", "fwd", "precomp", _short("scales", 3), "scales must have 3 * P elements"),
    ("rotations", "fwd", "sh", _short("rotations", 1), "rotations must have 4 * P elements"),
    ("cov3D_precomp", "fwd", "precomp", _set("cov3D_precomp", lambda A, P: torch.ones(P - 2, 6, device=A["means3D"].device)), "cov3D_precomp must have 6 * P elements"),
    ("sh-not-P-M-3", "fwd", "sh", _set("sh", lambda A, P: A["sh"].transpose(1, 2).contiguous()), "sh must have dimensions (P, M, 3)"),
    ("filter_3D-length", "fwd", "raw", _set("filter_3D", lambda A, P: A["fwd"]["filter_3D"][: P - 7], "fwd"), FILTER_MSG),
    ("filter_3D-with-colors2", "fwd", "raw", _set("colors2", lambda A, P: A["colors"].clone(), "fwd"), FILTER_MSG),
    ("filter_3D-without-scales", "fwd", "raw", _set("scales", lambda A, P: torch.Tensor([])), FILTER_MSG),
    ("colors2-with-sh", "fwd", "sh", _set("colors2", lambda A, P: torch.ones(P, 3, device=A["means3D"].device), "fwd"), COLORS2_MSG),
    ("colors2-with-sh_tone", "fwd", "colors2", _set("sh_tone", lambda A, P: (None, None, 1.0, 1.0), "fwd"), COLORS2_MSG),
    ("colors2-rows", "fwd", "colors2", _set("colors2", lambda A, P: A["fwd"]["colors2"][: P - 1], "fwd"), COLORS2_MSG),
    ("sh_second-without-sh", "fwd", "precomp", _set("sh_second", lambda A, P: (None, None, None, None), "fwd"),
     "sh_second (two tones of one SH block) needs SH colours and neither colors2 nor binning_capacity"),
    ("binning_capacity-with-debug", "fwd", "fixed", _set("debug", lambda A, P: True), "binning_capacity (the fixed-capacity forward) has no debug mode"),
    ("binning_capacity-zero", "fwd", "fixed", _set("binning_capacity", lambda A, P: 0, "fwd"), "binning_capacity must be positive"),
    ("sh_mul-rows", "fwd", "sh_tone", _set("sh_tone", lambda A, P: (A["fwd"]["sh_tone"][0][: P - 1],) + A["fwd"]["sh_tone"][1:], "fwd"),
     "sh_mul must have 3 * P elements"),
    ("tone-length", "fwd", "sh_tone", _set("sh_tone", lambda A, P: A["fwd"]["sh_tone"][:3], "fwd"), "a tone is (mul, offset, pre_clamp_max, post_clamp_max)"),
    ("bwd-radii", "bwd", "precomp", _short("radii", 1), ROWS_MSG),
    ("bwd-scales", "bwd", "sh", _short("scales", 3), ROWS_MSG),
    ("bwd-dL_dout_color", "bwd", "precomp", _set("dL", lambda A, P: A["dL"].permute(1, 2, 0).contiguous()), "dL_dout_color must have dimensions (3, H, W)"),
    ("bwd-dL_dout_color2", "bwd", "colors2", _set("dL_dout_color2", lambda A, P: A["dL"][:, :, :-1].contiguous(), "bwd"),
     "dL_dout_color2 must have the first image's dimensions"),
    ("bwd-raw-length", "bwd", "raw", _set("raw", lambda A, P: A["bwd"]["raw"] + (A["opacity"],), "bwd"), "raw is (filter_3D, raw_opacities)"),
    ("bwd-raw-rows", "bwd", "raw", _set("raw", lambda A, P: (A["bwd"]["raw"][0][: P - 5], A["opacity"]), "bwd"),
     "raw = (filter_3D, raw_opacities) must have P elements each"),
    ("bwd-sh_offset-rows", "bwd", "sh_tone", _set("sh_tone", lambda A, P: (None, A["bwd"]["sh_tone"][1][: P - 1], 1.0, 1.0), "bwd"),
     "sh_offset must have 3 * P elements"),
]
case_table = pytest.mark.parametrize("call,mode,edit,message", [pytest.param(*c[1:], id=c[0]) for c in CASES])


def _case_arguments(mode, edit, P, H, W, device):
    A = _mode_arguments(mode, P, H, W, device)
    if edit is not None:
        edit(A, P)
    return A


@case_table
def test_argument_checks_refuse_each_malformed_call_with_its_message(call, mode, edit, message):
    """_check_forward_arguments / _check_backward_arguments (what the ctypes binding calls, and what csrc/torch_binding.cpp repeats in C++)
    on CPU tensors: pure functions of shapes -- one case per check with the exact message, and the well-formed call of every mode."""
    from diff_gaussian_rasterization import _C
    A = _case_arguments(mode, edit, 8, 16, 16, "cpu")
    if call == "fwd":
        run = lambda: _C._check_forward_arguments(A["means3D"], A["colors"], A["opacity"], A["scales"], A["rotations"], A["cov3D_precomp"], A["sh"], A["debug"],
                                                  *(A["fwd"].get(k) for k in ("sh_tone", "binning_capacity", "colors2", "filter_3D", "sh_second")))
    else:
        run = lambda: _C._check_backward_arguments(A["means3D"], A["radii"], A["colors"], A["scales"], A["rotations"], A["cov3D_precomp"], A["sh"], A["dL"],
                                                   *(A["bwd"].get(k) for k in ("sh_tone", "dL_dout_color2", "raw", "sh_second")))
    if message is None:
        assert run() is None
    else:
        with pytest.raises(RuntimeError) as info:
            run()
        assert str(info.value) == message


def _native_forward(_C, rs, A):
    return _C.rasterize_gaussians(rs.bg, A["means3D"], A["colors"], A["opacity"], A["scales"], A["rotations"], 1.0, A["cov3D_precomp"], rs.viewmatrix,
                                  rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, A["sh"],
                                  A["degree"], rs.campos, False, A["debug"], options=OPTIONS, **A["fwd"])


def _native_backward(_C, rs, A, frame):
    return _C.rasterize_gaussians_backward(rs.bg, A["means3D"], A["radii"], A["colors"], A["scales"], A["rotations"], 1.0, A["cov3D_precomp"], rs.viewmatrix,
                                           rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, A["dL"], A["sh"], A["degree"], rs.campos,
                                           frame[3], frame[0], frame[4], frame[5], A["debug"], options=OPTIONS, **A["bwd"])


@pytest.mark.gpu
@needs_binding
@case_table
def test_both_bindings_refuse_the_same_calls_with_the_same_messages(binding, call, mode, edit, message):
    """The table above through _C.rasterize_gaussians / _C.rasterize_gaussians_backward under each binding: a malformed call raises the
    same RuntimeError in both, in the binding, before the library is called (a backward case gets the buffers of its mode's well-formed
    forward call); a well-formed one runs in both.  Then a well-formed forward and backward call: a refused call leaves nothing behind."""
    _C = binding
    from tests.wg_testlib import make_settings
    P, H, W = 64, 32, 32
    rs = make_settings(S.make_camera(W, H), 0)
    good, A = _mode_arguments(mode, P, H, W, "cuda"), _case_arguments(mode, edit, P, H, W, "cuda")
    said = {}
    for name in ("ctypes", "torch"):
        _C.use_binding(name)
        if call == "bwd":
            frame = _native_forward(_C, rs, good)
            A["radii"] = frame[2][: A["radii"].numel()]
        try:
            res = _native_forward(_C, rs, A) if call == "fwd" else _native_backward(_C, rs, A, frame)
            said[name] = None
            assert all(torch.isfinite(t).all() for t in (res[1:2] + res[6:] if call == "fwd" else res) if t is not None)
        except RuntimeError as err:
            said[name] = str(err)
    assert said["ctypes"] == said["torch"] == message
    well = _mode_arguments("precomp", P, H, W, "cuda")
    frame = _native_forward(_C, rs, well)
    well["radii"] = frame[2]
    grads = _native_backward(_C, rs, well, frame)
    assert torch.isfinite(frame[1]).all() and frame[0] > 0 and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.gpu
@needs_binding
@pytest.mark.parametrize("colors", ["sh", "precomp"])
def test_reference_shaped_entry_points_are_the_ex_ones_without_blocks(binding, colors):
    """The compiled module called directly: rasterize_gaussians / rasterize_gaussians_backward are the `_ex` routines with no optional block
    and the default options (1, 0, 1) -- same frame bit for bit, same gradients to the atomics' run-to-run rounding (the `_ex` pair's
    deterministic mode, twice, bit for bit), same shapes and dtypes, also for no Gaussians.  ("precomp" passes no sub-pixel offsets: a
    zero-sized tensor to the one, None to the other.)"""
    _C = binding
    from diff_gaussian_rasterization import _C_torch as m
    from tests.wg_testlib import make_settings, to_dev
    P, W, H = 2000, 160, 96
    deg = 2 if colors == "sh" else 0
    rs = make_settings(S.make_camera(W, H, yaw_deg=3.0), deg)
    e = torch.Tensor([])
    dL = to_dev(S.make_cotangent(W, H, seed=4))

    def calls(P):
        t = {k: to_dev(v)[:P] for k, v in S.make_cloud(max(P, 1), W, H, sh_degree=deg if colors == "sh" else None, seed=11, scale_mult=2.0).items()}
        so_ref, so_ex = (rs.subpixel_offset, rs.subpixel_offset) if colors == "sh" else (e, None)
        fw = lambda so: (rs.bg, t["means3D"], t.get("colors_precomp", e), t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                         rs.tanfovx, rs.tanfovy, rs.kernel_size, so, H, W, t.get("shs", e), deg, rs.campos, False, False)
        bw = lambda so, f: (rs.bg, t["means3D"], f[2], t.get("colors_precomp", e), t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                            rs.tanfovx, rs.tanfovy, rs.kernel_size, so, dL, t.get("shs", e), deg, rs.campos, f[3], f[0], f[4], f[5], False)
        ref_frame = m.rasterize_gaussians(*fw(so_ref))
        ref_grads = m.rasterize_gaussians_backward(*bw(so_ref, ref_frame))

        def ex(options):
            frame = m.rasterize_gaussians_ex(*fw(so_ex), None, None, None, None, None, options)
            return frame, m.rasterize_gaussians_backward_ex(*bw(so_ex, frame), None, None, None, None, options)
        return ref_frame, ref_grads, ex

    ref_frame, ref_grads, ex = calls(P)
    ex_frame, ex_grads = ex((1, 0, 1))
    assert len(ref_frame) == len(ex_frame) == 6 and ref_frame[0] == ex_frame[0] > 0
    assert torch.equal(ref_frame[1], ex_frame[1]) and torch.equal(ref_frame[2], ex_frame[2])
    va, vb = _C.view_image(ref_frame[5], H, W), _C.view_image(ex_frame[5], H, W)
    assert torch.equal(va["n_contrib"], vb["n_contrib"]) and torch.equal(va["final_T"], vb["final_T"])
    assert len(ref_grads) == len(ex_grads) == 8
    for g, h in zip(ref_grads, ex_grads):
        assert g.shape == h.shape and g.dtype == h.dtype
        assert g.numel() == 0 or float((g - h).abs().max()) <= 4e-6 * float(g.abs().max()) + 1e-30
    (_, det1), (_, det2) = ex((1, 1, 1)), ex((1, 1, 1))
    assert all(torch.equal(g, h) for g, h in zip(det1, det2))
    # no Gaussians: nothing launched, the same eight shapes and dtypes
    ref_frame, ref_grads, ex = calls(0)
    ex_frame, ex_grads = ex((1, 0, 1))
    assert ref_frame[0] == ex_frame[0] == 0 and not ref_frame[1].any() and ref_frame[1].shape == ex_frame[1].shape == (3, H, W)
    assert all(a.numel() == b.numel() == 0 and a.dtype == b.dtype for a, b in zip(ref_frame[2:], ex_frame[2:]))
    assert len(ref_grads) == len(ex_grads) == 8 and all(g.shape == h.shape and g.dtype == h.dtype for g, h in zip(ref_grads, ex_grads))


def test_binding_follows_the_environment():
    """WG_BINDING=ctypes|torch selects the binding at import; without it the compiled one is the default when it has been built."""
    from diff_gaussian_rasterization import _C
    want = os.environ.get("WG_BINDING") or ("torch" if built and not os.environ.get("WG_RASTERIZER_LIB") else "ctypes")
    assert _C.binding_name() == want


@pytest.mark.gpu
@needs_binding
def test_cross_section_of_the_suite_passes_under_the_ctypes_binding():
    """The ctypes binding (`WG_BINDING=ctypes`: what serves a variant library, and the fallback where the compiled module has not been
    built) is a supported path, so a cross-section of the GPU suite runs under it INSIDE the driver-run suite:
    the four parity cases forward and backward, the operator surface, the thirty-case argument sweep, the deterministic mode, and every call
    mode beyond the reference's surface (two colour sets, two tones, one tone, raw parameters: twelve cases) against the reference's own
    kernels -- in a subprocess whose import picks the binding from the environment."""
    import re
    import subprocess
    sel = ("binding_follows_the_environment or forward_rgb_parity or backward_gradient_parity or operator_surface_semantics or "
           "argument_sweep_against_the_oracle or deterministic_backward_mode_is_bit_reproducible or "
           "(two_colour_sets_in_one_call and (0 or 5 or 11)) or (two_tones_of_one_sh_block and (1 or 6 or 12)) or "
           "(one_tone_beside and (2 or 7)) or (raw_parameter_mode_beside and 0) or wrong_size_tensors")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu or not gpu", "-p", "no:cacheprovider", "tests/test_parity_gpu.py",
                        "tests/test_reference_modes.py", "tests/test_torch_binding.py", "-k", sel],
                       cwd=ROOT, env=dict(os.environ, WG_BINDING="ctypes"), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 40, tail
