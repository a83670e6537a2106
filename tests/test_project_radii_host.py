"""The projection-only pass without a device (include/wg_rasterizer.h: wg_project_radii): what both bindings refuse, with which message, and
what the library refuses before any device work.

The bindings check shapes, modes and dtypes first and the device last, so every malformed call of the table below is refused on host
tensors; the well-formed call on host tensors is refused by the last check (the pass has no CPU path)."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wg_rasterizer.h")
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
P = 8
NO_CPU = " must live on a HIP device, the one of means3D: this pass has no CPU path"


def _good():
    return dict(means3D=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4), cov3D_precomp=None, filter_3D=None,
                scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), tan_fovx=0.5, tan_fovy=0.5, kernel_size=0.1,
                image_height=48, image_width=64)


def _precomp():
    return dict(_good(), scales=None, rotations=None, cov3D_precomp=torch.ones(P, 6))


ONE_SOURCE = "project_radii needs exactly one of a scales / rotations pair or cov3D_precomp"
FILTER = "filter_3D (raw-parameter mode) needs scales and rotations, and P filter values"
CASES = [
    ("host-tensors", _good, {}, "means3D" + NO_CPU),
    ("host-tensors-precomp", _precomp, {}, "means3D" + NO_CPU),
    ("host-tensors-raw", _good, dict(filter_3D=torch.ones(P, 1)), "means3D" + NO_CPU),
    ("means3D-shape", _good, dict(means3D=torch.zeros(P, 2)), "means3D must have dimensions (num_points, 3)"),
    ("means3D-1d", _good, dict(means3D=torch.zeros(3 * P)), "means3D must have dimensions (num_points, 3)"),
    ("both-sources", _good, dict(cov3D_precomp=torch.ones(P, 6)), ONE_SOURCE),
    ("neither-source", _good, dict(scales=None, rotations=None), ONE_SOURCE),
    ("half-a-pair", _good, dict(rotations=None), ONE_SOURCE),
    ("half-a-pair-with-precomp", _precomp, dict(scales=torch.ones(P, 3)), ONE_SOURCE),
    ("filter-with-precomp", _precomp, dict(filter_3D=torch.ones(P, 1)), FILTER),
    ("filter-size", _good, dict(filter_3D=torch.ones(P - 1, 1)), FILTER),
    ("means3D-dtype", _good, dict(means3D=torch.zeros(P, 3, dtype=torch.float64)), "means3D must be float32"),
    ("scales-dtype", _good, dict(scales=torch.ones(P, 3, dtype=torch.float16)), "scales must be float32"),
    ("filter-dtype", _good, dict(filter_3D=torch.ones(P, 1, dtype=torch.float64)), "filter_3D must be float32"),
    ("viewmatrix-dtype", _good, dict(viewmatrix=torch.eye(4, dtype=torch.float64)), "viewmatrix must be float32"),
    ("scales-rows", _good, dict(scales=torch.ones(P - 1, 3)), "scales must have 3 * P elements"),
    ("rotations-rows", _good, dict(rotations=torch.ones(P, 3)), "rotations must have 4 * P elements"),
    ("cov3D-rows", _precomp, dict(cov3D_precomp=torch.ones(P + 1, 6)), "cov3D_precomp must have 6 * P elements"),
    ("viewmatrix-shape", _good, dict(viewmatrix=torch.eye(3)), "viewmatrix must have dimensions (4, 4)"),
    ("viewmatrix-flat", _good, dict(viewmatrix=torch.eye(4).reshape(16)), "viewmatrix must have dimensions (4, 4)"),
    ("projmatrix-shape", _good, dict(projmatrix=torch.zeros(4, 3)), "projmatrix must have dimensions (4, 4)"),
    ("height", _good, dict(image_height=0), "image_height and image_width must be positive"),
    ("width", _good, dict(image_width=-64), "image_height and image_width must be positive"),
]
case_table = pytest.mark.parametrize("base,edit,message", [pytest.param(*c[1:], id=c[0]) for c in CASES])
ORDER = ("means3D", "scales", "rotations", "cov3D_precomp", "filter_3D", "scale_modifier", "viewmatrix", "projmatrix", "tan_fovx", "tan_fovy",
         "kernel_size", "image_height", "image_width")


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)


@case_table
def test_each_malformed_call_is_refused_with_its_message_under_either_binding(binding, base, edit, message):
    _C = binding
    A = dict(base(), **edit)
    names = ("ctypes", "torch") if built else ("ctypes",)
    said = {}
    for name in names:
        _C.use_binding(name)
        assert _C.binding_name() == name
        with pytest.raises(RuntimeError) as info:
            _C.project_radii(*(A[k] for k in ORDER))
        said[name] = str(info.value)
    assert all(v == message for v in said.values()), said


def test_the_compiled_binding_is_part_of_the_comparison():
    assert built, "the compiled binding has not been built: the table above compared the ctypes binding with nothing"


def test_the_public_method_refuses_before_the_binding_does():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.5, kernel_size=0.1, subpixel_offset=torch.zeros(48, 64, 2),
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False, return_accumulation=False)
    rast = GaussianRasterizer(rs)
    g = _good()
    for kw in (dict(), dict(scales=g["scales"]), dict(scales=g["scales"], rotations=g["rotations"], cov3D_precomp=torch.ones(P, 6))):
        with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
            rast.project_radii(g["means3D"], **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):   # well-formed, on the host
        rast.project_radii(g["means3D"], g["scales"], g["rotations"], filter_3D=torch.ones(P, 1), opacities=torch.zeros(P, 1))
    import wg_fused_gaussians as fg
    with pytest.raises(RuntimeError, match="no CPU path"):
        fg.VisibleRows.from_camera(rast, g["means3D"], g["scales"], g["rotations"])
    assert "radii" in fg.VisibleRows.__slots__ and fg.VisibleRows(torch.zeros(1, dtype=torch.int32), 1).radii is None


# ---- the C-ABI, over FAKE device addresses: every call below must be refused (or be a no-op) before any device work ----------------------------
def _args(_C, **kw):
    a = _C._ProjectArgs()
    a.struct_size = C.sizeof(a)
    a.P, a.width, a.height = 100, 64, 48
    a.means3D, a.scales, a.rotations, a.viewmatrix, a.projmatrix, a.radii = (0x10000,) * 6
    a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, 0.5, 0.5, 0.1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_library_refuses_malformed_calls_before_any_device_work():
    from diff_gaussian_rasterization import _C
    f = _C._lib.wg_project_radii
    INVALID = -1
    assert C.sizeof(_C._ProjectArgs) == 112   # 8 + 3 * 4 (+ 4 padding) + 5 * 8 + 4 * 4 + 4 * 8
    assert f(None) == INVALID
    assert f(C.byref(_args(_C, struct_size=C.sizeof(_C._ProjectArgs) - 8))) == INVALID   # does not cover the fields
    assert f(C.byref(_args(_C, struct_size=0))) == INVALID
    for name in ("means3D", "viewmatrix", "projmatrix", "radii"):                          # a null mandatory pointer with P > 0
        assert f(C.byref(_args(_C, **{name: None}))) == INVALID, name
    assert f(C.byref(_args(_C, cov3D_precomp=0x10000))) == INVALID                         # both covariance sources
    assert f(C.byref(_args(_C, scales=None, rotations=None))) == INVALID                   # neither
    assert f(C.byref(_args(_C, rotations=None))) == INVALID and f(C.byref(_args(_C, scales=None))) == INVALID   # half a pair
    assert f(C.byref(_args(_C, scales=None, cov3D_precomp=0x10000))) == INVALID
    assert f(C.byref(_args(_C, scales=None, rotations=None, cov3D_precomp=0x10000, filter_3D=0x10000))) == INVALID   # raw parameters are pairs
    assert f(C.byref(_args(_C, P=0, scales=None, rotations=None, cov3D_precomp=0x10000, filter_3D=0x10000))) == INVALID
    for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(height=-48), dict(P=-1), dict(P=0, width=0)):   # sizes
        assert f(C.byref(_args(_C, **kw))) == INVALID, kw
    # P = 0: WG_OK, nothing launched, no pointer looked at
    assert f(C.byref(_args(_C, P=0))) == 0
    assert f(C.byref(_args(_C, P=0, means3D=None, scales=None, rotations=None, viewmatrix=None, projmatrix=None, radii=None))) == 0
    assert f(C.byref(_args(_C, P=0, filter_3D=0x10000))) == 0


def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    from diff_gaussian_rasterization import _C
    text = open(HEADER).read()
    assert re.search(r"\bint wg_project_radii\(const wg_project_args\* args\);", text)
    fields = re.search(r"typedef struct wg_project_args \{(.*?)\} wg_project_args;", text, re.S).group(1)
    assert "raw_opacities" not in fields and "filter_3D" in fields   # the radius depends on no opacity: the header says why
    declared = [n for n, _ in _C._ProjectArgs._fields_]
    assert declared == ["struct_size", "P", "width", "height", "means3D", "scales", "rotations", "cov3D_precomp", "filter_3D", "scale_modifier", "tan_fovx",
                        "tan_fovy", "kernel_size", "viewmatrix", "projmatrix", "radii", "stream"]
    order = [fields.index(n) for n in declared]
    assert order == sorted(order)   # the ctypes struct lists the header's fields in the header's order
    out = subprocess.run(["nm", "-D", "--defined-only", _C._lib._name], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "wg_project_radii" for ln in out.splitlines() if ln.split())
