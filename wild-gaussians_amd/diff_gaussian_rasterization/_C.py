"""``diff_gaussian_rasterization._C`` -- binding of the MI355X rasterizer's C-ABI library.

Stands where the reference's pybind11 module of the same name stands
(submodules/diff-gaussian-rasterization/ext.cpp:15-19, rasterize_points.{h,cu}) and exports the same
three functions with the same argument order and return tuples:

    rasterize_gaussians(...)          -> (num_rendered, out_color, radii, geomBuffer, binningBuffer, imgBuffer)
    rasterize_gaussians_backward(...) -> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                                          dL_dscales, dL_drotations)
    mark_visible(means3D, viewmatrix, projmatrix) -> bool[P]

It is the one Python door to ``libwg_rasterizer.so`` (include/wg_rasterizer.h).  Each call is dispatched to the compiled torch binding
(csrc/torch_binding.cpp, the default when built) or to the ctypes binding below (``_forward_ctypes`` / ``_backward_ctypes``: a variant library,
the counting tools, a tree without the compiled module).  Both take the same arguments, refuse the same malformed calls with the same messages
(``_check_forward_arguments`` / ``_check_backward_arguments`` here, the same checks in C++ there) and return the same tuples.  Per-call option
resolution, the opt-in geometry reuse, the library's options, stage timing and the views into the scratch buffers live here for both.  There
is NO fallback: if the HIP library has not been built, importing this module raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("WG_RASTERIZER_LIB") or os.path.join(_HERE, "libwg_rasterizer.so")  # override: another build of the same C-ABI

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} is missing: build the HIP library first "
        "(python wild-gaussians_amd/build.py, or __graft_entry__.build()).  There is no CPU fallback.")

_lib = C.CDLL(_LIB_PATH)

# The compiled torch binding of the same C-ABI (csrc/torch_binding.cpp -> _C_torch*.so, built by build.py --torch-binding; INTEGRATION.md
# section 2): the reference's three functions with the reference's signatures + the `_ex` pair carrying every optional block.  It is the
# DEFAULT whenever it has been built (end of this file); WG_BINDING=ctypes (or use_binding("ctypes")) selects the ctypes code below, which
# covers the same surface and is what serves a variant library (WG_RASTERIZER_LIB).
_torch_ext = None


def use_binding(name: str) -> str:
    """"torch" (the default when built) or "ctypes": which binding serves the calls.  Returns the previous name."""
    global _torch_ext
    prev = "ctypes" if _torch_ext is None else "torch"
    if name == "torch":
        if _LIB_PATH != os.path.join(_HERE, "libwg_rasterizer.so"):
            raise ImportError("the compiled binding links the in-tree libwg_rasterizer.so; WG_RASTERIZER_LIB points elsewhere")
        from . import _C_torch  # noqa: F401  (ImportError when it has not been built: python wild-gaussians_amd/build.py --torch-binding)
        _torch_ext = _C_torch
    elif name == "ctypes":
        _torch_ext = None
    else:
        raise ValueError(name)
    return prev


def binding_name() -> str:
    return "ctypes" if _torch_ext is None else "torch"


from ._abi import (_ALLOC_FN, _vp, _i, _f, _ShTone, _SecondImage, _RawGaussians, _RecolorParent, _CallOptions, _ForwardArgs,  # noqa: E402
                    _BackwardArgs, _ProjectArgs, _DepthArgs, _DepthGrad, _ContribArgs, _DistortionArgs, _DistortionGrad,
                    _BackwardExtras)   # (pure ctypes)

_lib.wg_rasterize_forward.restype = _i
_lib.wg_rasterize_forward.argtypes = [_ALLOC_FN, _vp, _ALLOC_FN, _vp, _ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                      _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _i, _vp, _vp, _i, _vp]
_lib.wg_rasterize_backward.restype = _i
_lib.wg_rasterize_backward.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _f,
                                       _vp, _vp, _vp, _vp, _vp, _vp] + [_vp] * 9 + [_i, _vp]
_lib.wg_rasterize_forward_ex.restype = _i
_lib.wg_rasterize_forward_ex.argtypes = [C.POINTER(_ForwardArgs)]
_lib.wg_rasterize_backward_ex.restype = _i
_lib.wg_rasterize_backward_ex.argtypes = [C.POINTER(_BackwardArgs)]
_lib.wg_forward_status.restype = _i
_lib.wg_forward_status.argtypes = [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]
_lib.wg_mark_visible.restype = _i
_lib.wg_mark_visible.argtypes = [_i, _vp, _vp, _vp, _vp, _vp]
_lib.wg_project_radii.restype = _i
_lib.wg_project_radii.argtypes = [C.POINTER(_ProjectArgs)]
_lib.wg_render_depth.restype = _i
_lib.wg_render_depth.argtypes = [C.POINTER(_DepthArgs)]
_lib.wg_render_contributions.restype = _i
_lib.wg_render_contributions.argtypes = [C.POINTER(_ContribArgs)]
_lib.wg_render_distortion.restype = _i
_lib.wg_render_distortion.argtypes = [C.POINTER(_DistortionArgs)]
_lib.wg_rasterize_backward_with.restype = _i
_lib.wg_rasterize_backward_with.argtypes = [C.POINTER(_BackwardArgs), C.POINTER(_BackwardExtras)]
for _name in ("wg_geometry_buffer_size", "wg_geometry_buffer_size_rows", "wg_binning_buffer_size"):
    getattr(_lib, _name).restype = C.c_size_t
    getattr(_lib, _name).argtypes = [_i]
_lib.wg_image_buffer_size.restype = C.c_size_t
_lib.wg_image_buffer_size.argtypes = [_i, _i]
_lib.wg_image_accumulation_offset.restype = C.c_size_t
_lib.wg_image_accumulation_offset.argtypes = [_i, _i]
for _name, _args in (("wg_status_string", [_i]), ("wg_last_hip_error", []), ("wg_version", [])):
    getattr(_lib, _name).restype = C.c_char_p
    getattr(_lib, _name).argtypes = _args
_lib.wg_get_option.restype = _i
_lib.wg_get_option.argtypes = [C.c_char_p]
_lib.wg_set_option.restype = _i
_lib.wg_set_option.argtypes = [C.c_char_p, _i]


class _GeometryView(C.Structure):
    _fields_ = [(n, _vp) for n in ("depths", "radii", "splats", "cov3D", "clamped", "tiles_touched", "point_offsets")]


class _BinningView(C.Structure):
    _fields_ = [(n, _vp) for n in ("point_list",)]


class _ImageView(C.Structure):
    _fields_ = [(n, _vp) for n in ("final_T", "accumulation", "n_contrib", "ranges", "tile_last", "tile_near", "split", "order_fwd", "order_key", "order_bwd")]


_lib.wg_view_geometry.restype = _i
_lib.wg_view_geometry.argtypes = [_vp, _i, C.POINTER(_GeometryView)]
_lib.wg_view_backward_rows.restype = _i
_lib.wg_view_backward_rows.argtypes = [_vp, _i, C.c_size_t, C.POINTER(_vp)]
_lib.wg_view_binning.restype = _i
_lib.wg_view_binning.argtypes = [_vp, _i, C.POINTER(_BinningView)]
_lib.wg_view_image.restype = _i
_lib.wg_view_image.argtypes = [_vp, _i, _i, C.POINTER(_ImageView)]

IMAGE_STATE_ALIGNMENT = 256  # final_T sits at the first 256-byte aligned address of imgBuffer (wg_rasterizer.h)
_acc_offsets = {}


def accumulation_offset(height: int, width: int) -> int:
    """Bytes from final_T to the accumulation array inside imgBuffer (wg_image_accumulation_offset; cached per frame size)."""
    k = (height, width)
    if k not in _acc_offsets:
        _acc_offsets[k] = int(_lib.wg_image_accumulation_offset(int(width), int(height)))
    return _acc_offsets[k]


def _check(status: int, what: str) -> int:
    if status < 0:
        msg = _lib.wg_status_string(status).decode()
        if status == -3:
            msg += ": " + _lib.wg_last_hip_error().decode()
        raise RuntimeError(f"{what} failed: {msg}")
    return status


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    """float32, contiguous, on `device`; zero-sized tensors are the reference's "absent" sentinel."""
    if t.numel() == 0:
        return t
    if t.device != device or t.dtype != torch.float32:
        t = t.to(device=device, dtype=torch.float32)
    return t if t.is_contiguous() else t.contiguous()


def _f32s(device, *tensors):
    return [None if t is None else _f32(t, device) for t in tensors]


def _ptr(t: torch.Tensor):
    return t.data_ptr() if t.numel() != 0 else None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _Scratch:
    """One resizable byte tensor per scratch buffer: the role of resizeFunctional (rasterize_points.cu:27-33)."""

    def __init__(self, device):
        self.device = device
        self.tensor = torch.empty(0, dtype=torch.uint8, device=device)
        self.callback = _ALLOC_FN(self._alloc)

    def _alloc(self, nbytes, _user):
        self.tensor = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self.tensor.data_ptr()

    def take(self) -> torch.Tensor:
        """Hand the tensor over and break the self -> callback -> bound method -> self cycle: with the cycle left in place the
        buffer would stay allocated until Python's cyclic collector runs, some tens of steps later -- hundreds of MB of dead
        scratch per step for the caching allocator to cover with fresh (slow, synchronising) device allocations."""
        t, self.tensor, self.callback = self.tensor, None, None
        return t


def _tone_block(sh_tone, device, P, grads=None):
    """sh_tone = (mul [P,3] or None, offset [P,3] or None, pre_clamp_max or None, post_clamp_max or None) -> (_ShTone, keep-alive).
    Beyond the reference: see wg_sh_tone in include/wg_rasterizer.h."""
    mul, offset, pre, post = sh_tone
    keep = _f32s(device, mul, offset)
    t = _ShTone(*(None if v is None else v.data_ptr() for v in keep), float("inf") if pre is None else float(pre),
                float("inf") if post is None else float(post), *(None if g is None else g.data_ptr() for g in grads or ()))
    return t, keep


def _second_block(device, colors2=None, out_color2=None, dL_dpix2=None, dL_dcolor2=None):
    """wg_second_image from whichever of its four tensors the call has -> (_SecondImage, keep-alive)."""
    keep = _f32s(device, colors2, out_color2, dL_dpix2, dL_dcolor2)
    return _SecondImage(*(None if t is None else t.data_ptr() for t in keep)), keep


def _raw_block(device, filter_3D, raw_opacities=None):
    """wg_raw_gaussians (raw_opacities: the backward call's) -> (_RawGaussians, keep-alive)."""
    keep = _f32s(device, filter_3D, raw_opacities)
    return _RawGaussians(*(None if t is None else t.data_ptr() for t in keep)), keep


def _attach_blocks(a, opts, tone=None, tone2=None, second=None, raw=None):
    """Hang the optional blocks, each a (struct, keep-alive) pair or None, and the per-call options on an args struct -> keep-alive list."""
    keep = []
    for name, block in (("tone", tone), ("tone2", tone2), ("second", second), ("raw", raw), ("options", (_CallOptions(*opts), None))):
        if block is not None:
            keep += block
            setattr(a, name, C.pointer(block[0]))
    a.sh_second = int(tone2 is not None)
    return keep


# ----------------------------------------------------------------------------------------------------------
# The argument checks of both calls: a wrong-size tensor must raise, not send a kernel out of bounds.  Pure functions of shapes,
# numel() values and which optional arguments are given.  The ctypes binding calls them; the compiled one, a module of its own whose fast
# path pays for no Python-side check, makes the same checks in the same order with the same messages (csrc/torch_binding.cpp).
def _rows(t, per, P):
    return t.numel() in (0, per * P)


def _sh_rows(sh, P):
    return sh.numel() == 0 or (sh.dim() == 3 and sh.size(0) == P and sh.size(2) == 3)


def _check_tone(tone, P):
    if tone is not None and len(tone) != 4:
        raise RuntimeError("a tone is (mul, offset, pre_clamp_max, post_clamp_max)")
    for name, v in zip(("mul", "offset"), tone or ()):
        if v is not None and v.numel() != 3 * P:
            raise RuntimeError(f"sh_{name} must have 3 * P elements")


def _check_forward_arguments(means3D, colors, opacity, scales, rotations, cov3D_precomp, sh, debug, sh_tone, binning_capacity, colors2, filter_3D, sh_second):
    """What rasterize_gaussians refuses, after its two leading checks (means3D is (P, 3), on a HIP device)."""
    P = means3D.size(0)
    fixed = binning_capacity is not None
    if filter_3D is not None and (colors2 is not None or fixed or scales.numel() == 0 or filter_3D.numel() != P):
        raise RuntimeError("filter_3D (raw-parameter mode) needs scales and rotations, P filter values, and neither colors2 nor binning_capacity")
    if sh_second is not None and (colors2 is not None or fixed or sh.numel() == 0 or colors.numel() != 0):
        raise RuntimeError("sh_second (two tones of one SH block) needs SH colours and neither colors2 nor binning_capacity")
    if colors2 is not None and (sh_tone is not None or fixed or sh.numel() != 0 or colors.numel() != 3 * P or colors2.numel() != 3 * P):
        raise RuntimeError("colors2 needs precomputed colours of P x 3 in both sets (no SH, no sh_tone, no binning_capacity)")
    if fixed and debug:
        raise RuntimeError("binning_capacity (the fixed-capacity forward) has no debug mode")
    for t, per, name in ((colors, 3, "colors_precomp"), (opacity, 1, "opacities"), (scales, 3, "scales"), (rotations, 4, "rotations"),
                         (cov3D_precomp, 6, "cov3D_precomp")):
        if not _rows(t, per, P):
            raise RuntimeError(f"{name} must have {per} * P elements")
    if not _sh_rows(sh, P):
        raise RuntimeError("sh must have dimensions (P, M, 3)")
    if opacity.numel() != P:
        raise RuntimeError("opacities must have P elements")
    _check_tone(sh_tone, P)
    _check_tone(sh_second, P)
    if fixed and int(binning_capacity) <= 0:
        raise RuntimeError("binning_capacity must be positive")


def _check_backward_arguments(means3D, radii, colors, scales, rotations, cov3D_precomp, sh, dL_dout_color, sh_tone, dL_dout_color2, raw, sh_second):
    """What rasterize_gaussians_backward refuses, after the three mode checks it makes in front of both bindings."""
    P = means3D.size(0)
    if dL_dout_color.dim() != 3 or dL_dout_color.size(0) != 3:
        raise RuntimeError("dL_dout_color must have dimensions (3, H, W)")
    if dL_dout_color2 is not None and dL_dout_color2.numel() != dL_dout_color.numel():
        raise RuntimeError("dL_dout_color2 must have the first image's dimensions")
    if P != 0 and not (radii.numel() == P and _rows(colors, 3, P) and _rows(scales, 3, P) and _rows(rotations, 4, P) and _rows(cov3D_precomp, 6, P)
                       and _sh_rows(sh, P)):
        raise RuntimeError("a per-Gaussian argument of the backward call does not have P rows")
    _check_tone(sh_tone, P)
    _check_tone(sh_second, P)
    if raw is not None and len(raw) != 2:
        raise RuntimeError("raw is (filter_3D, raw_opacities)")
    if raw is not None and (raw[0].numel() != P or raw[1].numel() != P):
        raise RuntimeError("raw = (filter_3D, raw_opacities) must have P elements each")


# ----------------------------------------------------------------------------------------------------------
# Geometry reuse across consecutive calls (option "geometry_reuse", OPT-IN since round 4: default off).  WildGaussians rasterizes the
# same Gaussians through the same camera twice per step -- raw colours, then toned colours (method.py:1573-1611), a third time for
# depth -- and the reference projects, bins and sorts each time.  With the option on the binding remembers the LAST full forward call
# of the calling thread: when the next call hands over the very same geometry tensors (same Python objects, same autograd versions,
# same data pointers: nothing wrote to them that autograd knows of), the same camera tensors and scalars and only other precomputed
# colours, it takes wg_forward_args::recolor -- a copy of the projected state with the new colours and the compositing along the
# parent's sorted lists; binning and image-state buffers are shared with the parent call's (the per-pixel values are identical).
# Identity is by object (weak references), never by address alone: a freed tensor's address can be handed to a new one.
# WHY OPT-IN: a write through `tensor.data` (or `set_()` to equal-shaped storage at the same address) moves no version counter, and the
# binding cannot see it without reading the data back.  The remembered call ends with the first BACKWARD call of the process after it
# (`_reuse_epoch`; on whatever thread autograd runs it), so a training step -- forward calls, backward, optimiser -- is safe; a
# forward-only loop that edits geometry through `.data` between two renders of one camera is not, and a drop-in must not depend on its
# caller never doing that.  Callers that switch it on (wg_integration.apply_optins does) make that promise, or call forget_geometry().
# A parent call whose frame may turn out not to have fit (binning_capacity=, speculative_forward = 2) is never remembered: its child
# would composite along empty lists and return a clean background image where the contract says NaN.
GEOMETRY_REUSE_DEFAULT = 0


class _ReuseState:
    def __init__(self):
        self.last = None        # the remembered forward call (strong references to its scratch buffers)
        self.hits = 0
        self.last_fixed = None


class _PerThread:
    """`_reuse.<attr>` = the calling thread's _ReuseState.  A plain registry instead of threading.local, so that a backward call
    (usually on autograd's thread) can drop EVERY thread's stale entry -- and with it the references that keep a frame's scratch
    buffers alive until that thread's next forward call."""
    _states = {}

    @classmethod
    def state(cls):
        ident = threading.get_ident()
        s = cls._states.get(ident)
        if s is None:
            s = cls._states[ident] = _ReuseState()
        return s

    def __getattr__(self, name):
        return getattr(self.state(), name)

    def __setattr__(self, name, value):
        setattr(self.state(), name, value)


_reuse = _PerThread()
_reuse_epoch = 0   # bumped by every backward call (any thread; the GIL orders it)


def _tensor_token(t):
    """What must be unchanged for a tensor argument to count as 'the same': the object and its version counter (zero-sized
    'absent' sentinels are fresh objects on every call: they match each other)."""
    if t is None or t.numel() == 0:
        return None
    try:
        version = t._version
    except RuntimeError:   # inference-mode tensors track no version: nothing can vouch for "unchanged", so they never match
        return (lambda: None, object(), tuple(t.shape), t.dtype)
    return (weakref.ref(t), version, tuple(t.shape), t.dtype, t.data_ptr(), tuple(t.stride()))


def _same_token(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a[0]() is not None and a[0]() is b[0]() and a[1:] == b[1:]


def _reuse_key(background, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
               kernel_size, subpixel_offset, H, W, prefiltered, device):
    tensors = tuple(_tensor_token(t) for t in (means3D, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, background,
                                               subpixel_offset))
    scalars = (float(scale_modifier), float(tan_fovx), float(tan_fovy), float(kernel_size), H, W, bool(prefiltered), str(device),
               _stream(device))
    return tensors, scalars


def _reuse_lookup(key):
    last = _reuse.last
    if last is None or last.get("epoch") != _reuse_epoch or last["scalars"] != key[1] or last.get("opts") != key[2] or len(last["tensors"]) != len(key[0]):
        return None
    if not all(_same_token(a, b) for a, b in zip(last["tensors"], key[0])):
        return None
    return last


def forget_geometry():
    """Drop the calling thread's remembered forward call (and the scratch buffers it keeps alive)."""
    _reuse.last = None


# ----------------------------------------------------------------------------------------------------------
# Per-call options (wg_call_options in include/wg_rasterizer.h): the three switches that AFFECT RESULTS travel with every call; the
# library has no process-wide state for them.  A call's values: the `options=` argument (a dict, or the resolved 3-tuple the autograd
# layer keeps on its ctx so that a frame's backward call carries its forward call's values), else the CALLING THREAD's defaults --
# which `call_options(...)` overrides for a `with` block and `set_option(name, value)` sets for the thread (what the tests' and
# bench.py's `--option deterministic_backward=1` use; other threads, and other callers in the process, are not affected).
CALL_OPTION_DEFAULTS = dict(exact_compositing=1, deterministic_backward=0, grad_record=1)
_tls = threading.local()


def _thread_call_options() -> dict:
    d = getattr(_tls, "call_options", None)
    if d is None:
        d = _tls.call_options = dict(CALL_OPTION_DEFAULTS)
    return d


def resolve_call_options(options=None):
    """-> (exact_compositing, deterministic_backward, grad_record) as ints: `options` (dict with any of the three names, None values = not
    given; or an already resolved 3-tuple) over the calling thread's defaults."""
    if isinstance(options, tuple):
        return options
    d = _thread_call_options()
    if options:
        unknown = set(options) - set(CALL_OPTION_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown call option(s) {sorted(unknown)}")
        d = dict(d, **{k: int(v) for k, v in options.items() if v is not None})
    return (int(bool(d["exact_compositing"])), int(bool(d["deterministic_backward"])), int(bool(d["grad_record"])))


@contextlib.contextmanager
def call_options(**kw):
    """`with _C.call_options(deterministic_backward=1): ...` -- the calling thread's defaults for the block (for callers that cannot pass
    keywords, e.g. the reference's unedited method.py)."""
    unknown = set(kw) - set(CALL_OPTION_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown call option(s) {sorted(unknown)}")
    d = _thread_call_options()
    saved = dict(d)
    d.update({k: int(v) for k, v in kw.items()})
    try:
        yield
    finally:
        d.clear()
        d.update(saved)


# The colour-only backward pass (wg_backward_args::colour_gradients_only): a frame whose geometry is frozen and whose precomputed colours alone
# take a gradient gets dL_dcolors from one cheap walk and nothing else.  The flag travels BESIDE the three per-call options (it selects what
# is computed, not how): the `colour_gradients_only=` keyword of rasterize_gaussians_backward, else the calling thread's default, which
# `colour_gradients_only(True)` sets for a `with` block (for callers that cannot pass keywords).
COLOUR_ONLY_MSG = ("colour_gradients_only needs precomputed colours and nothing that has per-Gaussian work behind them "
                   "(no SH colours, sh_tone, sh_second, second colour set or raw parameters) and deterministic_backward = 0")


# "fixed_order" in place of True asks for the same gradient without float atomics (wg_backward_args::colour_gradients_only =
# WG_COLOUR_GRADIENTS_FIXED_ORDER: per-instance slots + an ordered per-Gaussian sum, bit-identical run to run).  Same calls served, same calls refused.
COLOUR_FIXED_ORDER = "fixed_order"
_COLOUR_MODE_ABI = {True: 1, COLOUR_FIXED_ORDER: 2}   # the C-ABI's values


def _colour_mode(value):
    """True / False / "fixed_order" from what a caller passed; any other string is a ValueError (checked before any device work)."""
    if isinstance(value, str):
        if value != COLOUR_FIXED_ORDER:
            raise ValueError(f"colour_gradients_only is True, False, None or '{COLOUR_FIXED_ORDER}', not {value!r}")
        return COLOUR_FIXED_ORDER
    return bool(value)


def resolve_colour_gradients_only(value=None):
    """`value` (the keyword; None = not given) over the calling thread's default -> False, True or "fixed_order"."""
    return getattr(_tls, "colour_gradients_only", False) if value is None else _colour_mode(value)


@contextlib.contextmanager
def colour_gradients_only(on=True):
    """`with _C.colour_gradients_only(True): ...` -- the calling thread's default for the block (True, False or "fixed_order")."""
    on = _colour_mode(on)   # (an unknown string raises here, with nothing changed)
    saved = getattr(_tls, "colour_gradients_only", False)
    _tls.colour_gradients_only = on
    try:
        yield
    finally:
        _tls.colour_gradients_only = saved


def colour_only_refused(has_sh, toned, second, raw, sh_second, opts) -> bool:
    """What the colour-only backward pass refuses, each argument a bool but the resolved options (the library returns
    WG_ERR_INVALID_ARGUMENT for the same calls)."""
    return bool(has_sh or toned or second or raw or sh_second or opts[1])


# The depth pass's gradient (wg_depth_grad): one more walk of the frame's backward call that adds into the ATOMIC gradient record, so it is refused
# wherever there is no such record (the library returns WG_ERR_INVALID_ARGUMENT for the same calls) -- by the operator at forward time, by
# rasterize_gaussians_backward in front of both bindings, with this one message.
DEPTH_GRAD_MSG = ("depth_grad adds the depth loss's gradient into the frame's gradient record: it cannot be combined with colour_gradients_only, "
                  "deterministic_backward = 1, grad_record = 0 or binning_capacity")
DEPTH_GRAD_BLOCK_MSG = "depth is (dL_ddepth, source): the depth cotangent [H, W] and the frame's return_depth source"
DEPTH_GRAD_COTANGENT_MSG = "dL_ddepth must be a float32 tensor of H * W elements on the frame's HIP device"


def depth_grad_refused(colour_only, opts, fixed_capacity=False) -> bool:
    """What a depth gradient cannot be combined with: the colour-only backward pass, deterministic_backward = 1, grad_record = 0 (opts = the
    resolved per-call options) and, at forward time, binning_capacity (refused for depth already)."""
    return bool(colour_only or opts[1] or not opts[2] or fixed_capacity)


def _check_depth_grad_arguments(depth, P, dL_dout_color):
    """What rasterize_gaussians_backward refuses of its `depth` block, after the mode check in front of both bindings.  The compiled binding
    makes the same checks in the same order with the same messages (csrc/torch_binding.cpp: DepthGrad)."""
    if not isinstance(depth, (tuple, list)) or len(depth) != 2:
        raise RuntimeError(DEPTH_GRAD_BLOCK_MSG)
    dL_ddepth, source = depth
    device = dL_dout_color.device
    if (not isinstance(dL_ddepth, torch.Tensor) or dL_ddepth.dtype != torch.float32 or dL_ddepth.numel() * 3 != dL_dout_color.numel()
            or dL_ddepth.device != device):
        raise RuntimeError(DEPTH_GRAD_COTANGENT_MSG)
    check_depth_source(source, P)
    if isinstance(source, torch.Tensor) and (not source.is_cuda or source.device != device):
        raise RuntimeError(DEPTH_SOURCE_MSG)


# The distortion pass's gradient (wg_distortion_grad): the same kind of walk into the same record, refused in the same places with one message.
DISTORTION_GRAD_MSG = ("distortion_grad adds the distortion loss's gradient into the frame's gradient record: it cannot be combined with "
                       "colour_gradients_only, deterministic_backward = 1, grad_record = 0 or binning_capacity")
DISTORTION_GRAD_BLOCK_MSG = ("distortion is (dL_ddistortion, moments, source): the distortion cotangent [H, W], the forward pass's moments [4, H, W] "
                             "and the frame's return_distortion source")
DISTORTION_GRAD_COTANGENT_MSG = "dL_ddistortion must be a float32 tensor of H * W elements on the frame's HIP device"
DISTORTION_GRAD_MOMENTS_MSG = "moments must be a float32 tensor of 4 * H * W elements on the frame's HIP device"
DISTORTION_SOURCE_MSG = 'return_distortion must be "distance" or a float32 [P] tensor of per-Gaussian scalars on the frame\'s HIP device'
DISTORTION_CAPACITY_MSG = ("return_distortion cannot be combined with binning_capacity: a fixed-capacity frame that did not fit has no lists to walk, "
                           "and its verdict is not known when the distortion pass is queued")


def distortion_grad_refused(colour_only, opts, fixed_capacity=False) -> bool:
    """What a distortion gradient cannot be combined with: what a depth gradient cannot (depth_grad_refused)."""
    return depth_grad_refused(colour_only, opts, fixed_capacity)


def check_distortion_source(source, P=None):
    """What `return_distortion` / `source` may be, as far as no device is needed (P = None: the size is checked later).  An unknown string is a
    ValueError, like colour_gradients_only's.  The compiled binding makes the same checks in the same order with the same messages."""
    if isinstance(source, str):
        if source != "distance":
            raise ValueError(DISTORTION_SOURCE_MSG)
        return
    if not isinstance(source, torch.Tensor) or source.dtype != torch.float32:
        raise RuntimeError(DISTORTION_SOURCE_MSG)
    if P is not None and source.numel() != P:
        raise RuntimeError("distortion values must have P elements")


def _check_distortion_grad_arguments(distortion, P, dL_dout_color):
    """What rasterize_gaussians_backward refuses of its `distortion` block, after the mode check in front of both bindings.  The compiled binding
    makes the same checks in the same order with the same messages (csrc/torch_binding.cpp: DistortionBlock)."""
    if not isinstance(distortion, (tuple, list)) or len(distortion) != 3:
        raise RuntimeError(DISTORTION_GRAD_BLOCK_MSG)
    dL_ddist, moments, source = distortion
    device = dL_dout_color.device
    if (not isinstance(dL_ddist, torch.Tensor) or dL_ddist.dtype != torch.float32 or dL_ddist.numel() * 3 != dL_dout_color.numel()
            or dL_ddist.device != device):
        raise RuntimeError(DISTORTION_GRAD_COTANGENT_MSG)
    if (not isinstance(moments, torch.Tensor) or moments.dtype != torch.float32 or moments.numel() * 3 != 4 * dL_dout_color.numel()
            or moments.device != device):
        raise RuntimeError(DISTORTION_GRAD_MOMENTS_MSG)
    check_distortion_source(source, P)
    if isinstance(source, torch.Tensor) and (not source.is_cuda or source.device != device):
        raise RuntimeError(DISTORTION_SOURCE_MSG)


def _fill(a, device, P, degree, M, H, W, debug, scale_modifier, tan_fovx, tan_fovy, kernel_size, **tensors):
    """The fields wg_forward_args and wg_backward_args share; every other pointer field by name (None or zero-sized = NULL)."""
    a.struct_size = C.sizeof(a)
    a.P, a.D, a.M, a.width, a.height, a.debug = P, int(degree), M, W, H, int(bool(debug))
    a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = float(scale_modifier), float(tan_fovx), float(tan_fovy), float(kernel_size)
    for name, t in tensors.items():
        setattr(a, name, None if t is None else _ptr(t))
    a.stream = _stream(device)


def _forward_args(geom, binning, img, P, degree, M, H, W, background, means3D, sh, colors, opacity, scales, scale_modifier, rotations, cov3D_precomp,
                  viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, kernel_size, subpixel_offset, prefiltered, debug, out_color, radii, device):
    a = _ForwardArgs()
    _fill(a, device, P, degree, M, H, W, debug, scale_modifier, tan_fovx, tan_fovy, kernel_size, background=background, means3D=means3D, shs=sh,
          colors_precomp=colors, opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix,
          projmatrix=projmatrix, cam_pos=campos, subpixel_offset=subpixel_offset, out_color=out_color, radii=radii)
    a.geometry_alloc, a.prefiltered = geom.callback, int(bool(prefiltered))
    if binning is not None:
        a.binning_alloc, a.image_alloc = binning.callback, img.callback
    return a


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, tan_fovx, tan_fovy, kernel_size, subpixel_offset, image_height, image_width, sh, degree,
                        campos, prefiltered, debug, sh_tone=None, binning_capacity=None, colors2=None, filter_3D=None, sh_second=None, options=None,
                        forward_only=False):
    """The reference's `rasterize_gaussians` (rasterize_points.h:18-40) plus, by keyword, everything beyond it (include/wg_rasterizer.h:
    the optional blocks of wg_rasterize_forward_ex):
    sh_tone: (mul [P,3] | None, offset [P,3] | None, pre_clamp_max | None, post_clamp_max | None) on the SH coefficients (wg_sh_tone).
    sh_second: a 4-tuple like sh_tone (all four may be None): a SECOND image from the same SH coefficients through this tone, composited in
      the same walk; the result then ends with a seventh element, the second image.  Composes with sh_tone and filter_3D.
    colors2: a second [P,3] set of precomputed colours composited in the same walk (wg_second_image); seventh element likewise.
    filter_3D: opacity / scales / rotations are the caller's RAW parameters, get_gaussians() (method.py:1060-1086) runs in-kernel.
    binning_capacity: an int = no host rendezvous at all (capturable in a hipGraph); `rendered` is then the capacity, and
      forward_status(imgBuffer, H, W) tells the real count and whether the frame fit.
    options: per-call options (see resolve_call_options).
    forward_only: the caller expects no backward call for this frame (wg_forward_args::forward_only; a hint: results are the same either way)."""
    opts = resolve_call_options(options)
    H, W = int(image_height), int(image_width)
    key = None
    if _torch_ext is not None and not _geometry_reuse_on:
        _reuse.last = None   # the usual path: the compiled binding checks its arguments itself (same messages), nothing is remembered
    else:
        if means3D.dim() != 2 or means3D.size(1) != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:59-61
        if not means3D.is_cuda:
            raise RuntimeError("means3D must live on a HIP device: this rasterizer has no CPU path")
        _check_forward_arguments(means3D, colors, opacity, scales, rotations, cov3D_precomp, sh, debug, sh_tone, binning_capacity, colors2, filter_3D,
                                 sh_second)
        device, P = means3D.device, means3D.size(0)
        # precomputed colours over remembered geometry: no projection, no binning
        reusable = (P != 0 and sh_tone is None and not debug and colors.numel() == 3 * P and sh.numel() == 0 and colors2 is None
                    and filter_3D is None and sh_second is None and _geometry_reuse_on)
        if reusable:
            key = _reuse_key(background, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                             tan_fovy, kernel_size, subpixel_offset, H, W, prefiltered, device) + (opts,)
            last = _reuse_lookup(key)
            if last is not None:
                geom = _Scratch(device)
                out_color = torch.empty((3, H, W), dtype=torch.float32, device=device)
                colors_f, bg_f, so = _f32s(device, colors, background, subpixel_offset)
                a = _forward_args(geom, None, None, P, 0, 0, H, W, bg_f, None, None, colors_f, None, None, 1.0, None, None, None, None, None, 1.0, 1.0, 0.0,
                                  so, False, False, out_color, None, device)
                parent = _RecolorParent(last["geom"].data_ptr(), last["binning"].data_ptr(), last["img"].data_ptr(), int(last["R"]))
                ob = _CallOptions(*opts)
                a.recolor, a.options = C.pointer(parent), C.pointer(ob)
                try:
                    with torch.cuda.device(device):
                        rendered = _lib.wg_rasterize_forward_ex(C.byref(a))
                finally:
                    child = geom.take()
                _check(rendered, "wg_rasterize_forward_ex (recolor)")
                _reuse.hits += 1
                # (a fresh radii tensor, as every call of the reference returns: 4 bytes per Gaussian)
                return (rendered, out_color, last["radii"].clone(), child, last["binning"], last["img"])
        else:
            _reuse.last = None   # any other kind of call ends the remembered one's reach

    if _torch_ext is not None:   # the compiled binding (csrc/torch_binding.cpp): the whole surface but the recolouring above
        res = _torch_ext.rasterize_gaussians_ex(background, means3D, colors, opacity, scales, rotations, float(scale_modifier), cov3D_precomp, viewmatrix,
                                                projmatrix, float(tan_fovx), float(tan_fovy), float(kernel_size), subpixel_offset, H, W, sh, int(degree),
                                                campos, bool(prefiltered), bool(debug), sh_tone, binning_capacity, colors2, filter_3D, sh_second, opts, bool(forward_only))
    else:
        res = _forward_ctypes(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                              tan_fovy, kernel_size, subpixel_offset, H, W, sh, degree, campos, prefiltered, debug, sh_tone, binning_capacity, colors2,
                              filter_3D, sh_second, opts, device, P, forward_only)
    if binning_capacity is not None:
        _reuse.last_fixed = (res[5], H, W)
    # (never a parent whose verdict is not in yet: see "Geometry reuse" above)
    if key is not None and binning_capacity is None and _lib.wg_get_option(b"speculative_forward") != 2:
        _reuse.last = dict(tensors=key[0], scalars=key[1], opts=key[2], R=res[0], radii=res[2], geom=res[3], binning=res[4], img=res[5],
                           epoch=_reuse_epoch)
    return res


def _forward_ctypes(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                    kernel_size, subpixel_offset, H, W, sh, degree, campos, prefiltered, debug, sh_tone, binning_capacity, colors2, filter_3D, sh_second,
                    opts, device, P, forward_only=False):
    """The checked forward call through ctypes -> the reference's six, + the second image with colors2 / sh_second."""
    geom, binning, img = _Scratch(device), _Scratch(device), _Scratch(device)
    two = colors2 is not None or sh_second is not None
    if P == 0:  # rasterize_points.cu:83: nothing is launched, the image stays zero
        return (0, torch.zeros((3, H, W), dtype=torch.float32, device=device), torch.zeros((0,), dtype=torch.int32, device=device),
                geom.take(), binning.take(), img.take()) + ((torch.zeros((3, H, W), dtype=torch.float32, device=device),) if two else ())
    # both outputs are fully written by the kernels (every pixel, every Gaussian): no need for the reference's zero fill
    out_color = torch.empty((3, H, W), dtype=torch.float32, device=device)
    radii = torch.empty((P,), dtype=torch.int32, device=device)
    out_color2 = torch.empty((3, H, W), dtype=torch.float32, device=device) if two else None
    means3D, background, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, subpixel_offset, sh = _f32s(
        device, means3D, background, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, subpixel_offset, sh)
    M = sh.size(1) if sh.numel() != 0 else 0  # rasterize_points.cu:85-89
    a = _forward_args(geom, binning, img, P, degree, M, H, W, background, means3D, sh, colors, opacity, scales, scale_modifier, rotations, cov3D_precomp,
                      viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, kernel_size, subpixel_offset, prefiltered, debug, out_color, radii, device)
    keep = _attach_blocks(a, opts,  # noqa: F841  (alive until the call has returned)
                          tone=None if sh_tone is None else _tone_block(sh_tone, device, P),
                          tone2=None if sh_second is None else _tone_block(sh_second, device, P),
                          second=_second_block(device, colors2=colors2, out_color2=out_color2) if two else None,
                          raw=None if filter_3D is None else _raw_block(device, filter_3D))
    a.binning_capacity = int(binning_capacity or 0)
    a.forward_only = int(bool(forward_only))
    try:
        with torch.cuda.device(device):
            rendered = _lib.wg_rasterize_forward_ex(C.byref(a))
    finally:
        buffers = (geom.take(), binning.take(), img.take())
    _check(rendered, "wg_rasterize_forward")
    return (rendered, out_color, radii) + buffers + (() if out_color2 is None else (out_color2,))


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size, subpixel_offset, dL_dout_color, sh,
                                 degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, sh_tone=None, dL_dout_color2=None, raw=None,
                                 sh_second=None, options=None, colour_gradients_only=None, want=None, depth=None, distortion=None):
    """The reference's `rasterize_gaussians_backward` (rasterize_points.h:42-66) -> the eight tensors, plus by keyword:
    distortion = (dL_ddistortion [H, W], moments [4, H, W], source): the cotangent of the frame's distortion output (render_distortion), the
      moments that call returned and its source -- "distance" or the float32 [P] tensor of scalars.  One more per-tile walk adds the distortion
      loss's gradient into the gradient record (wg_distortion_grad through wg_rasterize_backward_with), behind the depth block's when both are
      given.  The result carries one more tensor, dL_dvalues [P] of the distortion's scalars: last, or IN FRONT of depth's dL_dvalues when
      `depth` is given too (which stays last).  Refused where `depth` is.  None: today's call, nothing new runs.
    depth = (dL_ddepth [H, W], source): the cotangent of the frame's depth output (render_depth) and its source -- "distance" or the float32 [P]
      tensor of scalars.  One more per-tile walk adds the depth loss's gradient into the gradient record (wg_depth_grad), so the geometry
      gradients returned are those of the image loss plus the depth loss; in distance mode dL_dmeans3D also carries the direct term.  The result
      ends with one more tensor, dL_dvalues [P] (the gradient of the scalars).  Needs the atomic gradient record: refused with
      colour_gradients_only, deterministic_backward = 1 and grad_record = 0.  None: today's call, nothing new runs.
    want = (dL_dcolors, dL_dcov3D) booleans (None = both): whether the caller reads them.  One it does not want comes back as None wherever the
      library treats it as an intermediate (dL_dcolors with SH colours and the gradient record, dL_dcov3D without cov3D_precomp): it is then
      neither allocated nor stored (wg_backward_args: NULL).  The autograd function passes its needs_input_grad.
    sh_tone: two more tensors are appended, dL_dsh_mul, dL_dsh_offset (None where the input was None); dL_dsh is then the gradient of the raw
      coefficients.
    sh_second (a frame rasterized with sh_second; needs dL_dout_color2): the eight + (dL_dsh_mul, dL_dsh_offset, dL_dsh_mul2, dL_dsh_offset2).
    dL_dout_color2 (a frame rasterized with colors2): the second image's cotangent; the result ends with dL_dcolors2 [P,3].
    raw = (filter_3D, raw_opacities) of a raw-parameter forward call: dL_dopacity / dL_dscales / dL_drotations are the RAW parameters' gradients.
    options: the frame's forward call's per-call options (resolve_call_options).
    colour_gradients_only (None = the calling thread's default, off unless inside `with colour_gradients_only(True)`): only dL_dcolors [P,3]
      is computed and allocated; the eight-tuple has None in the other seven places.  Precomputed colours only, no optional block, no
      deterministic_backward.  "fixed_order": the same without float atomics, bit-identical run to run (any other string: ValueError)."""
    global _reuse_epoch
    colour_only = resolve_colour_gradients_only(colour_gradients_only)   # (first: an unknown string is a ValueError before anything else happens)
    opts = resolve_call_options(options)
    want_colors, want_cov3D = (True, True) if want is None else (bool(want[0]), bool(want[1]))
    _reuse_epoch += 1   # what the forward calls remembered ends here (see "Geometry reuse" above) ...
    states = _PerThread._states
    for st in list(states.values()):                     # ... and so do the references that kept those frames' scratch alive (any thread's)
        st.last = None
    if len(states) > 8:                                  # (threads that have ended: their states go with them)
        alive = {t.ident for t in threading.enumerate()}
        for ident in [i for i in states if i not in alive]:
            states.pop(ident, None)
    if depth is not None and depth_grad_refused(colour_only, opts):   # the mode checks, in front of both bindings
        raise RuntimeError(DEPTH_GRAD_MSG)
    if distortion is not None and distortion_grad_refused(colour_only, opts):
        raise RuntimeError(DISTORTION_GRAD_MSG)
    if colour_only and colour_only_refused(sh.numel() != 0, sh_tone is not None, dL_dout_color2 is not None, raw is not None,
                                           sh_second is not None, opts):
        raise RuntimeError(COLOUR_ONLY_MSG)
    if sh_second is not None and dL_dout_color2 is None:
        raise RuntimeError("sh_second needs the second image's cotangent (dL_dout_color2)")
    record = bool(opts[2] or opts[1])
    dual = dL_dout_color2 is not None and sh_second is None
    if raw is not None and (not record or dual):
        raise RuntimeError("the raw-parameter backward pass needs grad_record = 1 and cannot be combined with the two-colour call")
    if (dual or sh_second is not None) and ((dual and sh_tone is not None) or (not record and means3D.size(0) != 0)):
        raise RuntimeError("the two-colour backward pass needs the gradient record (grad_record = 1 or deterministic_backward = 1) and no sh_tone")
    if colour_only:
        if _torch_ext is not None:
            return _torch_ext.rasterize_gaussians_backward_colour(background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                                                                  viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), float(kernel_size),
                                                                  subpixel_offset, dL_dout_color, sh, int(degree), campos, geomBuffer, int(R), binningBuffer,
                                                                  imageBuffer, bool(debug), opts, _COLOUR_MODE_ABI[colour_only])
        _check_backward_arguments(means3D, radii, colors, scales, rotations, cov3D_precomp, sh, dL_dout_color, None, None, None, None)
        return _backward_colour_ctypes(background, means3D, colors, subpixel_offset, dL_dout_color, geomBuffer, R, binningBuffer, imageBuffer, debug, opts,
                                       _COLOUR_MODE_ABI[colour_only])
    if _torch_ext is not None and distortion is not None:
        return _torch_ext.rasterize_gaussians_backward_distortion(background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                                                                  viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), float(kernel_size),
                                                                  subpixel_offset, dL_dout_color, sh, int(degree), campos, geomBuffer, int(R), binningBuffer,
                                                                  imageBuffer, bool(debug), sh_tone, dL_dout_color2, raw, sh_second, opts, want_colors,
                                                                  want_cov3D, depth, distortion)
    if _torch_ext is not None and depth is not None:
        return _torch_ext.rasterize_gaussians_backward_depth(background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                                                             viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), float(kernel_size), subpixel_offset,
                                                             dL_dout_color, sh, int(degree), campos, geomBuffer, int(R), binningBuffer, imageBuffer,
                                                             bool(debug), sh_tone, dL_dout_color2, raw, sh_second, opts, want_colors, want_cov3D, depth)
    if _torch_ext is not None:
        return _torch_ext.rasterize_gaussians_backward_ex(background, means3D, radii, colors, scales, rotations, float(scale_modifier), cov3D_precomp,
                                                          viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), float(kernel_size), subpixel_offset,
                                                          dL_dout_color, sh, int(degree), campos, geomBuffer, int(R), binningBuffer, imageBuffer,
                                                          bool(debug), sh_tone, dL_dout_color2, raw, sh_second, opts, want_colors, want_cov3D)
    _check_backward_arguments(means3D, radii, colors, scales, rotations, cov3D_precomp, sh, dL_dout_color, sh_tone, dL_dout_color2, raw, sh_second)
    if depth is not None:
        _check_depth_grad_arguments(depth, means3D.size(0), dL_dout_color)
    if distortion is not None:
        _check_distortion_grad_arguments(distortion, means3D.size(0), dL_dout_color)
    return _backward_ctypes(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                            tan_fovy, kernel_size, subpixel_offset, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug,
                            sh_tone, dL_dout_color2, raw, sh_second, opts, want_colors, want_cov3D, depth, distortion)


def _backward_ctypes(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     kernel_size, subpixel_offset, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, sh_tone,
                     dL_dout_color2, raw, sh_second, opts, want_colors=True, want_cov3D=True, depth=None, distortion=None):
    """The checked backward call through ctypes -> the reference's eight, + what the optional blocks add (+ the distortion's dL_dvalues [P] with
    `distortion`, + depth's dL_dvalues [P] last with `depth`)."""
    device, P, H, W = means3D.device, means3D.size(0), dL_dout_color.size(1), dL_dout_color.size(2)
    sh = _f32(sh, device)
    M = sh.size(1) if sh.numel() != 0 else 0
    dual = dL_dout_color2 is not None and sh_second is None
    # The reference zero-fills nine gradient tensors per call (rasterize_points.cu:157-165).  With the gradient record (the default,
    # include/wg_rasterizer.h) the library clears its own accumulator and every output is fully written by the per-Gaussian kernel
    # (zeros for culled Gaussians); without it the four accumulation targets of the per-tile pass share one zeroed allocation.
    f = dict(dtype=torch.float32, device=device)
    if P != 0 and (opts[2] or opts[1]):
        dL_dconic = None   # the reference's intermediate: not returned (rasterize_points.cu:201), so not requested
        dL_dmeans2D, dL_dopacity = torch.empty((P, 3), **f), torch.empty((P, 1), **f)
        # (with SH colours an intermediate too: a caller that does not want it gets None, the kernel skips the store)
        dL_dcolors = torch.empty((P, 3), **f) if want_colors or M == 0 else None
    else:
        acc = torch.zeros((P * 11,), **f)
        dL_dconic, dL_dmeans2D = acc[0:4 * P].view(P, 2, 2), acc[4 * P:7 * P].view(P, 3)
        dL_dcolors, dL_dopacity = acc[7 * P:10 * P].view(P, 3), acc[10 * P:11 * P].view(P, 1)
    alloc = torch.empty if P != 0 else torch.zeros
    dL_dmeans3D, dL_dsh = alloc((P, 3), **f), alloc((P, M, 3), **f)
    dL_dcov3D = alloc((P, 6), **f) if want_cov3D or cov3D_precomp.numel() != 0 else None   # (from scales and rotations: an intermediate)
    alloc_sr = alloc if scales.numel() != 0 else torch.zeros
    dL_dscales, dL_drotations = alloc_sr((P, 3), **f), alloc_sr((P, 4), **f)
    dL_dcolors2 = alloc((P, 3), **f) if dual else None
    tone_grads, tone2_grads = (None if t is None else tuple(None if v is None else alloc((P, 3), **f) for v in t[:2]) for t in (sh_tone, sh_second))
    dL_dvalues = None if depth is None else alloc((P,), **f)   # (the library fills it)
    dL_dvalues_t = None if distortion is None else alloc((P,), **f)   # (likewise)
    if P != 0:
        means3D, background, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, subpixel_offset, dL_dout_color = _f32s(
            device, means3D, background, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, subpixel_offset, dL_dout_color)
        radii = radii.contiguous()
        a = _BackwardArgs()
        _fill(a, device, P, degree, M, H, W, debug, scale_modifier, tan_fovx, tan_fovy, kernel_size, background=background, means3D=means3D, shs=sh,
              colors_precomp=colors, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix,
              campos=campos, subpixel_offset=subpixel_offset, radii=radii, dL_dpix=dL_dout_color,
              geom_buffer=geomBuffer, binning_buffer=binningBuffer, image_buffer=imageBuffer, dL_dmean2D=dL_dmeans2D, dL_dconic=dL_dconic,
              dL_dopacity=dL_dopacity, dL_dcolor=dL_dcolors, dL_dmean3D=dL_dmeans3D, dL_dcov3D=dL_dcov3D, dL_dsh=dL_dsh, dL_dscale=dL_dscales,
              dL_drot=dL_drotations)
        a.R = int(R)
        keep = _attach_blocks(a, opts,  # noqa: F841  (alive until the call has returned)
                              tone=None if sh_tone is None else _tone_block(sh_tone, device, P, tone_grads),
                              tone2=None if sh_second is None else _tone_block(sh_second, device, P, tone2_grads),
                              second=None if dL_dout_color2 is None else _second_block(device, dL_dpix2=dL_dout_color2, dL_dcolor2=dL_dcolors2),
                              raw=None if raw is None else _raw_block(device, *raw))
        if depth is not None:   # wg_depth_grad: the cotangent, the scalars (NULL = distance: the call's means3D and campos) and their gradient
            dL_ddepth, source = depth
            dL_ddepth = dL_ddepth.contiguous()
            values = None if isinstance(source, str) else source.contiguous()
            block = _DepthGrad(C.sizeof(_DepthGrad), dL_ddepth.data_ptr(), None if values is None else values.data_ptr(), dL_dvalues.data_ptr())
            keep += [dL_ddepth, values, block]
            a.depth = C.pointer(block)
        extras = None
        if distortion is not None:   # wg_distortion_grad, carried by wg_backward_extras: wg_backward_args' size is pinned
            dL_ddist, moments, source = distortion
            dL_ddist, moments = dL_ddist.contiguous(), moments.contiguous()
            values = None if isinstance(source, str) else source.contiguous()
            block = _DistortionGrad(C.sizeof(_DistortionGrad), dL_ddist.data_ptr(), moments.data_ptr(), None if values is None else values.data_ptr(),
                                    dL_dvalues_t.data_ptr())
            extras = _BackwardExtras(C.sizeof(_BackwardExtras), C.pointer(block))
            keep += [dL_ddist, moments, values, block]
        with torch.cuda.device(device):
            status = _lib.wg_rasterize_backward_ex(C.byref(a)) if extras is None else _lib.wg_rasterize_backward_with(C.byref(a), C.byref(extras))
        _check(status, "wg_rasterize_backward")
    out = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    last = (() if distortion is None else (dL_dvalues_t,)) + (() if depth is None else (dL_dvalues,))
    if sh_second is not None:
        return out + (tone_grads or (None, None)) + tone2_grads + last
    if dual:
        return out + (dL_dcolors2,) + last
    return (out if sh_tone is None else out + tone_grads) + last   # (raw-parameter mode: same tuple, slots 2, 6, 7 are gradients of the raw parameters)


def _backward_colour_ctypes(background, means3D, colors, subpixel_offset, dL_dout_color, geomBuffer, R, binningBuffer, imageBuffer, debug, opts, mode=1):
    """The checked colour-only backward call through ctypes -> the reference's eight places, dL_dcolors alone filled."""
    device, P, H, W = means3D.device, means3D.size(0), dL_dout_color.size(1), dL_dout_color.size(2)
    dL_dcolors = (torch.empty if P != 0 else torch.zeros)((P, 3), dtype=torch.float32, device=device)   # the library fills it
    if P != 0:
        background, colors, subpixel_offset, dL_dout_color = _f32s(device, background, colors, subpixel_offset, dL_dout_color)
        a = _BackwardArgs()
        _fill(a, device, P, 0, 0, H, W, debug, 1.0, 1.0, 1.0, 0.0, background=background, colors_precomp=colors, subpixel_offset=subpixel_offset,
              dL_dpix=dL_dout_color, geom_buffer=geomBuffer, binning_buffer=binningBuffer, image_buffer=imageBuffer, dL_dcolor=dL_dcolors)
        a.R, a.colour_gradients_only = int(R), int(mode)   # 1: atomics; 2: fixed order
        keep = _attach_blocks(a, opts)  # noqa: F841  (alive until the call has returned)
        with torch.cuda.device(device):
            status = _lib.wg_rasterize_backward_ex(C.byref(a))
        _check(status, "wg_rasterize_backward")
    return (None, dL_dcolors, None, None, None, None, None, None)


def forward_status(imageBuffer, H, W):
    """(num_rendered, fits) of the forward call that produced imageBuffer (wg_forward_status: synchronises the current stream)."""
    n, f = _i(0), _i(0)
    with torch.cuda.device(imageBuffer.device):
        _check(_lib.wg_forward_status(imageBuffer.data_ptr(), int(W), int(H), C.byref(n), C.byref(f), _stream(imageBuffer.device)), "wg_forward_status")
    return int(n.value), bool(f.value)


def last_forward_status():
    """forward_status of the calling thread's latest binning_capacity= (fixed-capacity) forward call; None if there was none."""
    last = _reuse.last_fixed
    return None if last is None else forward_status(*last)


def mark_visible(means3D, viewmatrix, projmatrix):
    if _torch_ext is not None:
        return _torch_ext.mark_visible(means3D, viewmatrix, projmatrix)
    device = means3D.device
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=device)
    if P != 0:
        means3D, viewmatrix, projmatrix = _f32(means3D, device), _f32(viewmatrix, device), _f32(projmatrix, device)
        with torch.cuda.device(device):
            _check(_lib.wg_mark_visible(P, _ptr(means3D), _ptr(viewmatrix), _ptr(projmatrix), present.data_ptr(),
                                        _stream(device)), "wg_mark_visible")
    return present


# ----------------------------------------------------------------------------------------------------------
# The projection-only pass (wg_project_radii): a frame's radii -- the forward call's bits -- before it is rendered.
def _check_project_arguments(means3D, scales, rotations, cov3D_precomp, filter_3D, viewmatrix, projmatrix, image_height, image_width):
    """What project_radii refuses (None = not given).  Shapes, modes and dtypes first -- pure functions of the tensors' metadata --, the
    device last.  The compiled binding makes the same checks in the same order with the same messages (csrc/torch_binding.cpp)."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P = means3D.size(0)
    if (scales is None) != (rotations is None) or (scales is None) == (cov3D_precomp is None):
        raise RuntimeError("project_radii needs exactly one of a scales / rotations pair or cov3D_precomp")
    if filter_3D is not None and (cov3D_precomp is not None or filter_3D.numel() != P):
        raise RuntimeError("filter_3D (raw-parameter mode) needs scales and rotations, and P filter values")
    named = (("means3D", means3D), ("scales", scales), ("rotations", rotations), ("cov3D_precomp", cov3D_precomp), ("filter_3D", filter_3D),
             ("viewmatrix", viewmatrix), ("projmatrix", projmatrix))
    for name, t in named:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
    for t, per, name in ((scales, 3, "scales"), (rotations, 4, "rotations"), (cov3D_precomp, 6, "cov3D_precomp")):
        if t is not None and t.numel() != per * P:
            raise RuntimeError(f"{name} must have {per} * P elements")
    for name, t in (("viewmatrix", viewmatrix), ("projmatrix", projmatrix)):
        if t.dim() != 2 or t.size(0) != 4 or t.size(1) != 4:
            raise RuntimeError(f"{name} must have dimensions (4, 4)")
    if int(image_height) <= 0 or int(image_width) <= 0:
        raise RuntimeError("image_height and image_width must be positive")
    for name, t in named:
        if t is not None and (not t.is_cuda or t.device != means3D.device):
            raise RuntimeError(f"{name} must live on a HIP device, the one of means3D: this pass has no CPU path")


def project_radii(means3D, scales, rotations, cov3D_precomp, filter_3D, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  image_height, image_width):
    """radii (int32 [P]) of the frame a forward call with these geometry inputs and this camera would render -- the same bits -- from one
    launch on torch's current stream: no colours, no scratch buffers, no host synchronisation (wg_project_radii).  `scales` + `rotations` or
    `cov3D_precomp`, the other(s) None; with `filter_3D` the pair is the caller's RAW parameters.  float32 tensors on one HIP device."""
    if _torch_ext is not None:
        return _torch_ext.project_radii(means3D, scales, rotations, cov3D_precomp, filter_3D, float(scale_modifier), viewmatrix, projmatrix,
                                        float(tan_fovx), float(tan_fovy), float(kernel_size), int(image_height), int(image_width))
    _check_project_arguments(means3D, scales, rotations, cov3D_precomp, filter_3D, viewmatrix, projmatrix, image_height, image_width)
    device, P = means3D.device, means3D.size(0)
    radii = torch.empty((P,), dtype=torch.int32, device=device)   # fully written by the kernel
    if P != 0:
        keep = [None if t is None else t.contiguous() for t in (means3D, scales, rotations, cov3D_precomp, filter_3D, viewmatrix, projmatrix)]
        a = _ProjectArgs()
        a.struct_size = C.sizeof(a)
        a.P, a.width, a.height = P, int(image_width), int(image_height)
        a.means3D, a.scales, a.rotations, a.cov3D_precomp, a.filter_3D, a.viewmatrix, a.projmatrix = (None if t is None else t.data_ptr() for t in keep)
        a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = float(scale_modifier), float(tan_fovx), float(tan_fovy), float(kernel_size)
        a.radii, a.stream = radii.data_ptr(), _stream(device)
        with torch.cuda.device(device):
            _check(_lib.wg_project_radii(C.byref(a)), "wg_project_radii")
    return radii


# ----------------------------------------------------------------------------------------------------------
# The depth pass (wg_render_depth): one scalar per Gaussian composited over a finished frame like a colour channel.
DEPTH_SOURCE_MSG = 'return_depth must be "distance" or a float32 [P] tensor of per-Gaussian scalars on the frame\'s HIP device'
DEPTH_CAPACITY_MSG = ("return_depth cannot be combined with binning_capacity: a fixed-capacity frame that did not fit has no lists to walk, "
                      "and its verdict is not known when the depth pass is queued")


def check_depth_source(source, P=None):
    """What `return_depth` / `source` may be, as far as no device is needed (P = None: the size is checked later).  The compiled binding makes
    the same checks in the same order with the same messages (csrc/torch_binding.cpp: RenderDepth)."""
    if isinstance(source, str):
        if source != "distance":
            raise RuntimeError(DEPTH_SOURCE_MSG)
        return
    if not isinstance(source, torch.Tensor) or source.dtype != torch.float32:
        raise RuntimeError(DEPTH_SOURCE_MSG)
    if P is not None and source.numel() != P:
        raise RuntimeError("depth values must have P elements")


def _check_depth_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, source, means3D, campos,
                           subpixel_offset, out):
    """What render_depth refuses: the source first (type, dtype, size, device), then the distance mode's inputs, the frame's size, the
    sub-pixel offsets and the output."""
    device = imageBuffer.device
    check_depth_source(source, P)
    if isinstance(source, torch.Tensor):
        if not source.is_cuda or source.device != device:
            raise RuntimeError(DEPTH_SOURCE_MSG)
    else:
        if means3D is None or campos is None:
            raise RuntimeError('depth source "distance" needs means3D and campos')
        if means3D.dtype != torch.float32 or means3D.numel() != 3 * P or campos.dtype != torch.float32 or campos.numel() != 3:
            raise RuntimeError("means3D must be float32 with 3 * P elements, campos float32 with 3")
        if not means3D.is_cuda or means3D.device != device or not campos.is_cuda or campos.device != device:
            raise RuntimeError("means3D and campos must live on the frame's HIP device")
    if int(P) < 0 or int(num_rendered) < 0 or int(image_height) <= 0 or int(image_width) <= 0:
        raise RuntimeError("P and num_rendered must not be negative, image_height and image_width must be positive")
    if subpixel_offset is not None and subpixel_offset.numel() != 0 and (
            subpixel_offset.dtype != torch.float32 or subpixel_offset.numel() != 2 * int(image_height) * int(image_width) or subpixel_offset.device != device):
        raise RuntimeError("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device")
    if out is not None and (out.dtype != torch.float32 or out.numel() != int(image_height) * int(image_width) or not out.is_contiguous()
                            or out.device != device):
        raise RuntimeError("out must be a contiguous float32 tensor of H * W elements on the frame's HIP device")
    if not (geomBuffer.is_cuda and binningBuffer.is_cuda and imageBuffer.is_cuda):
        raise RuntimeError("the frame's buffers must live on a HIP device")


def render_depth(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, source, means3D=None, campos=None,
                 subpixel_offset=None, options=None, out=None, debug=False):
    """depth (float32 [H, W]) of the finished frame these three buffers belong to (what rasterize_gaussians returned; num_rendered = its first
    element): sum over the pairs the frame blended of v * alpha * T, no background, no normalisation (wg_render_depth) -- one launch on torch's
    current stream that only reads the frame.  source: "distance" (v = |means3D - campos|, both then required) or a float32 [P] device tensor.
    subpixel_offset / options: the frame's.  out: a contiguous float32 tensor of H * W elements to write into (returned viewed as [H, W])."""
    opts = resolve_call_options(options)
    H, W = int(image_height), int(image_width)
    if _torch_ext is not None:
        return _torch_ext.render_depth(geomBuffer, binningBuffer, imageBuffer, int(num_rendered), int(P), H, W, source, means3D, campos,
                                       subpixel_offset, opts, out, bool(debug))
    _check_depth_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, H, W, source, means3D, campos, subpixel_offset, out)
    device = imageBuffer.device
    depth = torch.empty((H, W), dtype=torch.float32, device=device) if out is None else out.view(H, W)   # fully written by the library
    distance = isinstance(source, str)
    keep = [t.contiguous() if t is not None and t.numel() != 0 else None
            for t in ((means3D if distance else None), (campos if distance else None), (None if distance else source), subpixel_offset)]
    a = _DepthArgs()
    a.struct_size = C.sizeof(a)
    a.P, a.R, a.width, a.height, a.debug = int(P), int(num_rendered), W, H, int(bool(debug))
    if int(P) != 0:
        a.geom_buffer, a.binning_buffer, a.image_buffer = geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr()
    a.means3D, a.campos, a.values, a.subpixel_offset = (None if t is None else t.data_ptr() for t in keep)
    ob = _CallOptions(*opts)
    a.options = C.pointer(ob)
    a.out_depth, a.stream = depth.data_ptr(), _stream(device)
    with torch.cuda.device(device):
        _check(_lib.wg_render_depth(C.byref(a)), "wg_render_depth")
    return depth


# ----------------------------------------------------------------------------------------------------------
# The distortion pass (wg_render_distortion): the distortion term of a finished frame from the blend weights' centred moments.
def _check_distortion_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, source, means3D, campos,
                                subpixel_offset):
    """What render_distortion refuses: _check_depth_arguments' list with the distortion's own source messages."""
    device = imageBuffer.device
    check_distortion_source(source, P)
    if isinstance(source, torch.Tensor):
        if not source.is_cuda or source.device != device:
            raise RuntimeError(DISTORTION_SOURCE_MSG)
    else:
        if means3D is None or campos is None:
            raise RuntimeError('distortion source "distance" needs means3D and campos')
        if means3D.dtype != torch.float32 or means3D.numel() != 3 * P or campos.dtype != torch.float32 or campos.numel() != 3:
            raise RuntimeError("means3D must be float32 with 3 * P elements, campos float32 with 3")
        if not means3D.is_cuda or means3D.device != device or not campos.is_cuda or campos.device != device:
            raise RuntimeError("means3D and campos must live on the frame's HIP device")
    if int(P) < 0 or int(num_rendered) < 0 or int(image_height) <= 0 or int(image_width) <= 0:
        raise RuntimeError("P and num_rendered must not be negative, image_height and image_width must be positive")
    if subpixel_offset is not None and subpixel_offset.numel() != 0 and (
            subpixel_offset.dtype != torch.float32 or subpixel_offset.numel() != 2 * int(image_height) * int(image_width) or subpixel_offset.device != device):
        raise RuntimeError("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device")
    if not (geomBuffer.is_cuda and binningBuffer.is_cuda and imageBuffer.is_cuda):
        raise RuntimeError("the frame's buffers must live on a HIP device")


def render_distortion(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, source, means3D=None, campos=None,
                      subpixel_offset=None, options=None, moments=False, debug=False):
    """distortion (float32 [H, W]) of the finished frame these three buffers belong to: sum_{j<i} w_i w_j (v_i - v_j)^2 over the pairs the frame
    blended, w = alpha * T, as A Q' - D'^2 of the moments centred on each pixel's first blended v (wg_render_distortion) -- one launch on torch's
    current stream that only reads the frame.  source: "distance" (v = |means3D - campos|, both then required) or a float32 [P] device tensor.
    moments=True: -> (distortion, moments [4, H, W] = the planes A, D', Q', c), what the frame's backward call takes with the distortion's
    cotangent (rasterize_gaussians_backward(distortion=)).  subpixel_offset / options: the frame's."""
    opts = resolve_call_options(options)
    H, W = int(image_height), int(image_width)
    if _torch_ext is not None:
        return _torch_ext.render_distortion(geomBuffer, binningBuffer, imageBuffer, int(num_rendered), int(P), H, W, source, means3D, campos,
                                            subpixel_offset, opts, bool(moments), bool(debug))
    _check_distortion_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, H, W, source, means3D, campos, subpixel_offset)
    device = imageBuffer.device
    dist = torch.empty((H, W), dtype=torch.float32, device=device)   # both fully written by the library
    mom = torch.empty((4, H, W), dtype=torch.float32, device=device) if moments else None
    distance = isinstance(source, str)
    keep = [t.contiguous() if t is not None and t.numel() != 0 else None
            for t in ((means3D if distance else None), (campos if distance else None), (None if distance else source), subpixel_offset)]
    a = _DistortionArgs()
    a.struct_size = C.sizeof(a)
    a.P, a.R, a.width, a.height, a.debug = int(P), int(num_rendered), W, H, int(bool(debug))
    if int(P) != 0:
        a.geom_buffer, a.binning_buffer, a.image_buffer = geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr()
    a.means3D, a.campos, a.values, a.subpixel_offset = (None if t is None else t.data_ptr() for t in keep)
    ob = _CallOptions(*opts)
    a.options = C.pointer(ob)
    a.out_distortion, a.out_moments, a.stream = dist.data_ptr(), None if mom is None else mom.data_ptr(), _stream(device)
    with torch.cuda.device(device):
        _check(_lib.wg_render_distortion(C.byref(a)), "wg_render_distortion")
    return (dist, mom) if moments else dist


# ----------------------------------------------------------------------------------------------------------
# The contribution pass (wg_render_contributions): per Gaussian the largest blend weight, the number of blended pairs and their fixed-point
# sum over a finished frame, combined into caller-owned [P] arrays with integer atomics.
CONTRIB_CAPACITY_MSG = ("contributions cannot be combined with binning_capacity: a fixed-capacity frame that did not fit has no lists to walk, "
                        "and its verdict is not known when the contribution pass is queued")
CONTRIB_NONE_MSG = "at least one of max_weight, hits and weight_sum_q32 must be given"
CONTRIB_MASK_MSG = "contribution_mask must be a float32 tensor of H * W elements on the frame's HIP device"


def _contrib_output_msg(name, dtype):
    return f"{name} must be a contiguous {dtype} tensor of P elements on the frame's HIP device"


def _check_contrib_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, max_weight, hits, weight_sum_q32,
                             pixel_mask, subpixel_offset):
    """What render_contributions refuses: the outputs first (none at all; type, dtype, size, layout, device of each), then the frame's size, the
    mask, the sub-pixel offsets and the buffers.  The compiled binding makes the same checks in the same order with the same messages
    (csrc/torch_binding.cpp: RenderContributions)."""
    device = imageBuffer.device
    if max_weight is None and hits is None and weight_sum_q32 is None:
        raise RuntimeError(CONTRIB_NONE_MSG)
    for name, t, dtype, dname in (("max_weight", max_weight, torch.float32, "float32"), ("hits", hits, torch.int64, "int64"),
                                  ("weight_sum_q32", weight_sum_q32, torch.int64, "int64")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != int(P) or not t.is_contiguous()
                              or t.device != device):
            raise RuntimeError(_contrib_output_msg(name, dname))
    if int(P) < 0 or int(num_rendered) < 0 or int(image_height) <= 0 or int(image_width) <= 0:
        raise RuntimeError("P and num_rendered must not be negative, image_height and image_width must be positive")
    N = int(image_height) * int(image_width)
    if pixel_mask is not None and (not isinstance(pixel_mask, torch.Tensor) or pixel_mask.dtype != torch.float32 or pixel_mask.numel() != N
                                   or pixel_mask.device != device):
        raise RuntimeError(CONTRIB_MASK_MSG)
    if subpixel_offset is not None and subpixel_offset.numel() != 0 and (
            subpixel_offset.dtype != torch.float32 or subpixel_offset.numel() != 2 * N or subpixel_offset.device != device):
        raise RuntimeError("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device")
    if not (geomBuffer.is_cuda and binningBuffer.is_cuda and imageBuffer.is_cuda):
        raise RuntimeError("the frame's buffers must live on a HIP device")


def render_contributions(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, image_height, image_width, max_weight, hits, weight_sum_q32,
                         pixel_mask=None, subpixel_offset=None, options=None, accumulate=True, debug=False):
    """Combine what each Gaussian contributed to the finished frame these three buffers belong to (what rasterize_gaussians returned;
    num_rendered = its first element) into max_weight (float32 [P]), hits (int64 [P]) and weight_sum_q32 (int64 [P]; the sum of
    floor(w * 2^32)), any of which may be None (wg_render_contributions) -- one launch on torch's current stream that only reads the frame
    and uses integer atomics, so two calls give the same bits.  pixel_mask: float32, H * W elements; a pixel whose entry is 0 takes no part.
    accumulate=False zero-fills the given arrays under the same call first.  subpixel_offset / options: the frame's.  Returns None."""
    opts = resolve_call_options(options)
    H, W = int(image_height), int(image_width)
    if _torch_ext is not None:
        return _torch_ext.render_contributions(geomBuffer, binningBuffer, imageBuffer, int(num_rendered), int(P), H, W, max_weight, hits,
                                               weight_sum_q32, pixel_mask, subpixel_offset, opts, bool(accumulate), bool(debug))
    _check_contrib_arguments(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, H, W, max_weight, hits, weight_sum_q32, pixel_mask,
                             subpixel_offset)
    if int(P) == 0:   # no Gaussian: nothing to fill, nothing to walk (an empty tensor has no address to hand to the library)
        return None
    device = imageBuffer.device
    keep = [t.contiguous() if t is not None and t.numel() != 0 else None for t in (pixel_mask, subpixel_offset)]
    a = _ContribArgs()
    a.struct_size = C.sizeof(a)
    a.P, a.R, a.width, a.height, a.debug = int(P), int(num_rendered), W, H, int(bool(debug))
    a.geom_buffer, a.binning_buffer, a.image_buffer = geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr()
    a.pixel_mask, a.subpixel_offset = (None if t is None else t.data_ptr() for t in keep)
    ob = _CallOptions(*opts)
    a.options = C.pointer(ob)
    a.max_weight, a.hits, a.weight_sum_q32 = (None if t is None else t.data_ptr() for t in (max_weight, hits, weight_sum_q32))
    a.accumulate, a.stream = int(bool(accumulate)), _stream(device)
    with torch.cuda.device(device):
        _check(_lib.wg_render_contributions(C.byref(a)), "wg_render_contributions")
    return None


# ----------------------------------------------------------------------------------------------------------
# Introspection for the parity tests: typed views into the opaque scratch buffers (device tensors, no copy).
def _from_ptr(ptr, shape, dtype, owner):
    # torch.frombuffer cannot wrap device memory; the CUDA array interface can
    class _Holder:
        pass

    h = _Holder()
    n = 1
    for s in shape:
        n *= s
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1", torch.int64: "<i8"}[dtype]
    h.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    t = torch.as_tensor(h, device=owner.device) if n else torch.empty(shape, dtype=dtype, device=owner.device)
    t._wg_owner = owner  # keep the scratch buffer alive
    return t


def view_geometry(geomBuffer, P):
    v = _GeometryView()
    _check(_lib.wg_view_geometry(geomBuffer.data_ptr(), int(P), C.byref(v)), "wg_view_geometry")
    rows = _vp()   # (None for a frame that left no backward rows: its buffer does not hold the array)
    _check(_lib.wg_view_backward_rows(geomBuffer.data_ptr(), int(P), geomBuffer.numel(), C.byref(rows)), "wg_view_backward_rows")
    return dict(depths=_from_ptr(v.depths, (P,), torch.float32, geomBuffer), radii=_from_ptr(v.radii, (P,), torch.int32, geomBuffer),
                splats=_from_ptr(v.splats, (P, 12), torch.float32, geomBuffer), cov3D=_from_ptr(v.cov3D, (P, 6), torch.float32, geomBuffer),
                clamped=_from_ptr(v.clamped, (P,), torch.uint8, geomBuffer), bwd_row=_from_ptr(rows.value, (P, 10), torch.float32, geomBuffer) if rows.value else None,
                tiles_touched=_from_ptr(v.tiles_touched, (P,), torch.int32, geomBuffer),
                point_offsets=_from_ptr(v.point_offsets, (P,), torch.int32, geomBuffer))


def view_binning(binningBuffer, R):
    v = _BinningView()
    _check(_lib.wg_view_binning(binningBuffer.data_ptr(), int(R), C.byref(v)), "wg_view_binning")
    return dict(point_list=_from_ptr(v.point_list, (R,), torch.int32, binningBuffer))


def view_image(imageBuffer, H, W):
    v = _ImageView()
    _check(_lib.wg_view_image(imageBuffer.data_ptr(), int(W), int(H), C.byref(v)), "wg_view_image")
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return dict(final_T=_from_ptr(v.final_T, (H, W), torch.float32, imageBuffer),
                accumulation=_from_ptr(v.accumulation, (H, W), torch.float32, imageBuffer),
                n_contrib=_from_ptr(v.n_contrib, (H, W), torch.int32, imageBuffer),
                ranges=_from_ptr(v.ranges, (tiles, 2), torch.int32, imageBuffer),
                tile_last=_from_ptr(v.tile_last, (tiles,), torch.int32, imageBuffer),
                tile_near=_from_ptr(v.tile_near, (tiles,), torch.int32, imageBuffer),
                split=_from_ptr(v.split, (2,), torch.int32, imageBuffer),
                order_fwd=_from_ptr(v.order_fwd, (tiles,), torch.int32, imageBuffer),
                order_key=_from_ptr(v.order_key, (4,), torch.int32, imageBuffer),
                order_bwd=_from_ptr(v.order_bwd, (tiles,), torch.int32, imageBuffer))


_geometry_reuse_on = False   # the option "geometry_reuse" is read by this binding only: kept here too, so that no call has to ask the library


def set_option(name: str, value: int) -> None:
    """wg_set_option: a tuning switch of the library (process-wide; every setting gives identical results: docs/OPTIONS.md), e.g.
    set_option("force_global_sort", 1).  For the three RESULT-AFFECTING names (exact_compositing, deterministic_backward, grad_record), which
    the library takes per call, it sets the CALLING THREAD's default instead (see call_options)."""
    global _geometry_reuse_on
    if name in CALL_OPTION_DEFAULTS:
        _thread_call_options()[name] = int(bool(int(value)))
    else:
        _check(_lib.wg_set_option(name.encode(), int(value)), f"wg_set_option({name})")
        if name == "geometry_reuse":
            _geometry_reuse_on = bool(int(value))
    forget_geometry()   # a remembered forward call was made under the old options


def geometry_reuse_hits() -> int:
    """How many calls of this thread took the geometry-reuse path so far."""
    return _reuse.hits


def get_option(name: str) -> int:
    """wg_get_option: current value of a library option (-1: unknown name); for the three per-call names, the calling thread's default."""
    if name in CALL_OPTION_DEFAULTS:
        return int(_thread_call_options()[name])
    return int(_lib.wg_get_option(name.encode()))


def version() -> str:
    return _lib.wg_version().decode()


# ----------------------------------------------------------------------------------------------------------
# Per-stage HIP-event timing (wg_profile_* in wg_rasterizer.h); used by bench.py for the roofline object.
STAGE_COUNT = 12  # WG_STAGE_COUNT (include/wg_rasterizer.h)


class _StageTimes(C.Structure):
    _fields_ = [("total_ms", C.c_double * STAGE_COUNT), ("launches", C.c_longlong * STAGE_COUNT)]


_lib.wg_profile_enable.restype = _i
_lib.wg_profile_enable.argtypes = [_i]
_lib.wg_profile_reset.restype = _i
_lib.wg_profile_reset.argtypes = []
_lib.wg_profile_read.restype = _i
_lib.wg_profile_read.argtypes = [C.POINTER(_StageTimes)]
_lib.wg_stage_name.restype = C.c_char_p
_lib.wg_stage_name.argtypes = [_i]


def profile_enable(on: bool) -> None:
    _check(_lib.wg_profile_enable(int(bool(on))), "wg_profile_enable")


def profile_reset() -> None:
    _check(_lib.wg_profile_reset(), "wg_profile_reset")


def profile_read() -> dict:
    """{stage name: (total_ms, launches)} accumulated since the last profile_reset()."""
    st = _StageTimes()
    _check(_lib.wg_profile_read(C.byref(st)), "wg_profile_read")
    return {_lib.wg_stage_name(i).decode(): (float(st.total_ms[i]), int(st.launches[i])) for i in range(STAGE_COUNT)}

# WG_OPTIONS="name=value,name=value": library options applied at import (e.g. WG_OPTIONS=force_global_sort=1).  One of the three per-call
# names sets the PROCESS default (CALL_OPTION_DEFAULTS: what every thread starts from, also threads created later), not only the importing
# thread's -- WG_OPTIONS=deterministic_backward=1 has to reach worker and view-parallel threads too.
for _kv in filter(None, os.environ.get("WG_OPTIONS", "").split(",")):
    _k, _, _v = _kv.partition("=")
    _k = _k.strip()
    if _k in CALL_OPTION_DEFAULTS:
        CALL_OPTION_DEFAULTS[_k] = int(bool(int(_v or "1")))
        _thread_call_options()[_k] = CALL_OPTION_DEFAULTS[_k]
    else:
        set_option(_k, int(_v or "1"))


def set_default_call_option(name: str, value: int) -> None:
    """The PROCESS-wide default of a per-call option: what threads that have not set their own start from (set_option / call_options stay
    per thread).  Threads that already resolved their defaults keep them; the calling thread takes the new value."""
    if name not in CALL_OPTION_DEFAULTS:
        raise ValueError(name)
    CALL_OPTION_DEFAULTS[name] = int(bool(int(value)))
    _thread_call_options()[name] = CALL_OPTION_DEFAULTS[name]


# Which binding serves the calls: the compiled module (csrc/torch_binding.cpp -> _C_torch*.so) when it has been built and links this very
# library -- it carries the whole surface and costs less host time per call --, the ctypes code above otherwise.  WG_BINDING=ctypes|torch
# forces one (torch: ImportError if it has not been built).
_want = os.environ.get("WG_BINDING", "")
if _want:
    use_binding(_want)
elif _LIB_PATH == os.path.join(_HERE, "libwg_rasterizer.so"):
    try:
        use_binding("torch")
    except ImportError:
        pass
