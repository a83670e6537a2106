// diff_gaussian_rasterization._C_torch -- the compiled torch binding of the C-ABI (include/wg_rasterizer.h), standing where the
// reference's pybind11 module stands (submodules/diff-gaussian-rasterization/ext.cpp:15-19, rasterize_points.{h,cu}): the same three
// functions, the same argument order and return tuples (rasterize_points.h:18-71) -- INTEGRATION.md section 2 as a file that builds and
// is tested: what a maintainer of the reference would write to keep `rasterize_points.cu`'s surface on top of libwg_rasterizer.so --
// plus `rasterize_gaussians_ex` / `rasterize_gaussians_backward_ex`: the same two calls with everything beyond the reference by
// argument (the optional blocks and per-call options of wg_rasterize_forward_ex / _backward_ex).  Each direction is written ONCE
// (`forward` / `backward` below); the four entry points at the end only pack tuples, the reference-shaped pair being the `_ex` pair with
// no optional block and the default options.  It is the DEFAULT binding when built (diff_gaussian_rasterization/_C.py loads it; the
// ctypes code there is the fallback and keeps the Python-side geometry reuse).
// Host-side C++ only (no kernels here): torch supplies device memory, the device guard and the current HIP stream.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>   // torch on ROCm calls its device type "cuda": the stream getter of that name
#include <c10/core/DeviceGuard.h>

#include <limits>
#include <tuple>
#include <vector>

#include "wg_rasterizer.h"

namespace {

namespace py = pybind11;
using OptTensor = c10::optional<torch::Tensor>;

// the role of resizeFunctional (rasterize_points.cu:27-33); the binning allocator may be called twice in one forward call
// (speculative forward): the tensor is simply resized again, the pointer returned last is the one in use
char* resize_cb(size_t n, void* user) {
    auto& t = *static_cast<torch::Tensor*>(user);
    t.resize_({static_cast<int64_t>(n)});
    return reinterpret_cast<char*>(t.data_ptr());
}

torch::Tensor f32(const torch::Tensor& t, const torch::Device& dev) {   // float32, contiguous, on dev; zero-sized = "absent"
    if (t.numel() == 0) return t;
    return t.to(dev, torch::kFloat32).contiguous();
}
const float* ptr(const torch::Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }
char* bytes_of(const torch::Tensor& t) { return reinterpret_cast<char*>(t.data_ptr()); }

void check(int status, const char* what) {
    if (status >= 0) return;
    std::string msg = std::string(what) + " failed: " + wg_status_string(status);
    if (status == -3) msg += std::string(": ") + wg_last_hip_error();
    throw std::runtime_error(msg);   // -> RuntimeError, as AT_ERROR / std::runtime_error in the reference
}

wg_call_options call_options(const std::tuple<int, int, int>& o) {
    wg_call_options c;
    c.exact_compositing = std::get<0>(o); c.deterministic_backward = std::get<1>(o); c.grad_record = std::get<2>(o);
    return c;
}
const wg_call_options kDefaultOptions = WG_CALL_OPTIONS_DEFAULT;

// What both directions take, in the reference's order.  A zero-sized tensor is "absent"; so is a null subpixel_offset.
struct Scene {
    const torch::Tensor &background, &means3D, &colors, &scales, &rotations;
    float scale_modifier;
    const torch::Tensor &cov3D_precomp, &viewmatrix, &projmatrix;
    float tan_fovx, tan_fovy, kernel_size;
    const torch::Tensor* subpixel_offset;
    const torch::Tensor& sh;
    int degree;
    const torch::Tensor& campos;
    bool debug;
};
const torch::Tensor* opt(const OptTensor& t) { return t.has_value() ? &*t : nullptr; }

// The Scene as float32 device tensors, alive for the call, and the fields of wg_forward_args / wg_backward_args they fill.
struct Inputs {
    torch::Tensor bg, m3, shs, col, sc, rot, cov, vm, pm, cam, so;
    int M;
    Inputs(const Scene& s, const torch::Device& dev)
        : bg(f32(s.background, dev)), m3(f32(s.means3D, dev)), shs(f32(s.sh, dev)), col(f32(s.colors, dev)), sc(f32(s.scales, dev)),
          rot(f32(s.rotations, dev)), cov(f32(s.cov3D_precomp, dev)), vm(f32(s.viewmatrix, dev)), pm(f32(s.projmatrix, dev)),
          cam(f32(s.campos, dev)), so(s.subpixel_offset ? f32(*s.subpixel_offset, dev) : torch::Tensor()),
          M(shs.numel() ? static_cast<int>(shs.size(1)) : 0) {}   // rasterize_points.cu:85-89
    template <class Args>
    void fill(Args& a, const Scene& s, int H, int W, const float* Args::*campos, const wg_call_options& co, const torch::Device& dev) const {
        a.struct_size = sizeof(a);
        a.P = static_cast<int>(s.means3D.size(0)); a.D = s.degree; a.M = M; a.width = W; a.height = H; a.debug = s.debug;
        a.scale_modifier = s.scale_modifier; a.tan_fovx = s.tan_fovx; a.tan_fovy = s.tan_fovy; a.kernel_size = s.kernel_size;
        a.background = ptr(bg); a.means3D = ptr(m3); a.shs = ptr(shs); a.colors_precomp = ptr(col); a.scales = ptr(sc); a.rotations = ptr(rot);
        a.cov3D_precomp = ptr(cov); a.viewmatrix = ptr(vm); a.projmatrix = ptr(pm); a.*campos = ptr(cam); a.subpixel_offset = ptr(so);
        a.stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
        a.options = &co;
    }
};

// sh_tone = None | (mul [P,3] | None, offset [P,3] | None, pre_clamp_max | None, post_clamp_max | None)   (wg_sh_tone)
struct Tone {
    wg_sh_tone t{};
    torch::Tensor mul, offset;
    bool given = false;
    void parse(const py::object& o, const torch::Device& dev, int P) {
        if (o.is_none()) return;
        const py::tuple tu = o.cast<py::tuple>();
        if (tu.size() != 4) throw std::runtime_error("a tone is (mul, offset, pre_clamp_max, post_clamp_max)");
        given = true;
        const float inf = std::numeric_limits<float>::infinity();
        auto take = [&](int i, torch::Tensor& dst, const float*& p, const char* name) {
            if (tu[i].is_none()) return;
            dst = f32(tu[i].cast<torch::Tensor>(), dev);
            if (dst.numel() != 3 * (int64_t)P) throw std::runtime_error(std::string("sh_") + name + " must have 3 * P elements");
            p = dst.data_ptr<float>();
        };
        take(0, mul, t.mul, "mul");
        take(1, offset, t.offset, "offset");
        t.pre_clamp_max = tu[2].is_none() ? inf : tu[2].cast<float>();
        t.post_clamp_max = tu[3].is_none() ? inf : tu[3].cast<float>();
    }
};

// The per-Gaussian sizes both directions check: a wrong-size tensor must raise, not send a kernel out of bounds (the
// reference's binding checks none of them, rasterize_points.cu:59-61 is all there is).  _C.py makes the same checks, same messages,
// for the ctypes binding (_check_forward_arguments / _check_backward_arguments).
bool rows(const torch::Tensor& t, int64_t per, int64_t P) { return t.numel() == 0 || t.numel() == per * P; }
bool sh_rows(const torch::Tensor& sh, int64_t P) { return sh.numel() == 0 || (sh.ndimension() == 3 && sh.size(0) == P && sh.size(2) == 3); }

struct ForwardResult {
    int rendered = 0;
    torch::Tensor color, radii, geom, binning, img, color2;   // color2: defined with colors2 / sh_second only
};

ForwardResult forward(const Scene& s, const torch::Tensor& opacity, const int H, const int W, const bool prefiltered, const py::object& sh_tone,
                      const py::object& binning_capacity, const OptTensor& colors2, const OptTensor& filter_3D, const py::object& sh_second,
                      const wg_call_options& co, const bool forward_only = false) {
    if (s.means3D.ndimension() != 2 || s.means3D.size(1) != 3) AT_ERROR("means3D must have dimensions (num_points, 3)");   // rasterize_points.cu:59-61
    if (!s.means3D.is_cuda()) throw std::runtime_error("means3D must live on a HIP device: this rasterizer has no CPU path");
    const auto dev = s.means3D.device();
    const c10::DeviceGuard guard(dev);
    const int P = static_cast<int>(s.means3D.size(0));
    const int64_t P64 = P;
    const auto f = s.means3D.options().dtype(torch::kFloat32), i32 = s.means3D.options().dtype(torch::kInt32);
    const bool two = colors2.has_value() || !sh_second.is_none(), fixed = !binning_capacity.is_none();
    if (filter_3D.has_value() && (colors2.has_value() || fixed || s.scales.numel() == 0 || filter_3D->numel() != P64))
        throw std::runtime_error("filter_3D (raw-parameter mode) needs scales and rotations, P filter values, and neither colors2 nor binning_capacity");
    if (!sh_second.is_none() && (colors2.has_value() || fixed || s.sh.numel() == 0 || s.colors.numel() != 0))
        throw std::runtime_error("sh_second (two tones of one SH block) needs SH colours and neither colors2 nor binning_capacity");
    if (colors2.has_value() && (!sh_tone.is_none() || fixed || s.sh.numel() != 0 || s.colors.numel() != 3 * P64 || colors2->numel() != 3 * P64))
        throw std::runtime_error("colors2 needs precomputed colours of P x 3 in both sets (no SH, no sh_tone, no binning_capacity)");
    if (fixed && s.debug) throw std::runtime_error("binning_capacity (the fixed-capacity forward) has no debug mode");
    auto sized = [&](const torch::Tensor& t, int64_t per, const char* name) {
        if (!rows(t, per, P64)) throw std::runtime_error(std::string(name) + " must have " + std::to_string(per) + " * P elements");
    };
    sized(s.colors, 3, "colors_precomp"); sized(opacity, 1, "opacities"); sized(s.scales, 3, "scales"); sized(s.rotations, 4, "rotations");
    sized(s.cov3D_precomp, 6, "cov3D_precomp");
    if (!sh_rows(s.sh, P64)) throw std::runtime_error("sh must have dimensions (P, M, 3)");
    if (opacity.numel() != P64) throw std::runtime_error("opacities must have P elements");
    Tone tone, tone2;
    tone.parse(sh_tone, dev, P);
    tone2.parse(sh_second, dev, P);
    const int capacity = fixed ? binning_capacity.cast<int>() : 0;
    if (fixed && capacity <= 0) throw std::runtime_error("binning_capacity must be positive");

    ForwardResult r;
    const auto bytes = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
    r.geom = torch::empty({0}, bytes); r.binning = torch::empty({0}, bytes); r.img = torch::empty({0}, bytes);
    if (P == 0) {   // :83: nothing is launched, the image stays zero
        r.color = torch::zeros({3, H, W}, f); r.radii = torch::zeros({0}, i32);
        if (two) r.color2 = torch::zeros({3, H, W}, f);
        return r;
    }
    r.color = torch::empty({3, H, W}, f); r.radii = torch::empty({P}, i32);   // both fully written by the kernels: no zero fill
    const Inputs in(s, dev);
    const auto op = f32(opacity, dev);
    wg_forward_args a{};
    in.fill(a, s, H, W, &wg_forward_args::cam_pos, co, dev);
    a.geometry_alloc = resize_cb; a.geometry_user = &r.geom; a.binning_alloc = resize_cb; a.binning_user = &r.binning;
    a.image_alloc = resize_cb; a.image_user = &r.img;
    a.prefiltered = prefiltered; a.opacities = ptr(op); a.out_color = r.color.data_ptr<float>(); a.radii = r.radii.data_ptr<int>();
    a.binning_capacity = capacity;
    a.forward_only = forward_only ? 1 : 0;
    if (tone.given) a.tone = &tone.t;
    wg_second_image second{};
    torch::Tensor c2;
    if (two) {
        r.color2 = torch::empty({3, H, W}, f);
        second.out_color2 = r.color2.data_ptr<float>();
        if (tone2.given) {
            a.tone2 = &tone2.t; a.sh_second = 1;
        } else {
            c2 = f32(*colors2, dev);
            second.colors_precomp2 = ptr(c2);
        }
        a.second = &second;
    }
    wg_raw_gaussians raw{};
    torch::Tensor f3d;
    if (filter_3D.has_value()) {
        f3d = f32(*filter_3D, dev);
        raw.filter_3D = ptr(f3d);
        a.raw = &raw;
    }
    {
        py::gil_scoped_release nogil;   // (the call may wait for the frame's instance count: other Python threads run meanwhile)
        r.rendered = wg_rasterize_forward_ex(&a);
    }
    check(r.rendered, "wg_rasterize_forward");
    return r;
}

// The reference's eight (rasterize_points.cu:201) and what the optional blocks add (undefined = not asked for).
struct Gradients {
    torch::Tensor means2D, colors, opacity, means3D, cov3D, sh, scales, rotations, colors2, mul, offset, mul2, offset2, values, values_t;   // values: with `depth` only; values_t: with `distortion` only
    std::vector<torch::Tensor> eight() const { return {means2D, colors, opacity, means3D, cov3D, sh, scales, rotations}; }
};

Gradients backward(const Scene& s, const torch::Tensor& radii, const torch::Tensor& dL_dout_color, const torch::Tensor& geomBuffer, const int R,
                   const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const py::object& sh_tone, const OptTensor& dL_dout_color2,
                   const py::object& raw_in, const py::object& sh_second, const wg_call_options& co, const int colour_only = 0,   // (wg_backward_args::colour_gradients_only)
                   const bool want_colors = true, const bool want_cov3D = true, const py::object& depth = py::none(),   // depth: wg_depth_grad
                   const py::object& distortion = py::none()) {   // distortion: wg_distortion_grad (through wg_backward_extras)
    const auto dev = s.means3D.device();
    const c10::DeviceGuard guard(dev);
    const int P = static_cast<int>(s.means3D.size(0));
    const int64_t P64 = P;
    const bool two_tone = !sh_second.is_none(), dual = dL_dout_color2.has_value() && !two_tone;
    if (dL_dout_color.ndimension() != 3 || dL_dout_color.size(0) != 3) throw std::runtime_error("dL_dout_color must have dimensions (3, H, W)");
    if (dL_dout_color2.has_value() && dL_dout_color2->numel() != dL_dout_color.numel()) throw std::runtime_error("dL_dout_color2 must have the first image's dimensions");
    if (P != 0 && (radii.numel() != P64 || !rows(s.colors, 3, P64) || !rows(s.scales, 3, P64) || !rows(s.rotations, 4, P64) ||
                   !rows(s.cov3D_precomp, 6, P64) || !sh_rows(s.sh, P64)))
        throw std::runtime_error("a per-Gaussian argument of the backward call does not have P rows");
    Tone tone, tone2;
    tone.parse(sh_tone, dev, P);
    tone2.parse(sh_second, dev, P);
    if (two_tone && !dL_dout_color2.has_value()) throw std::runtime_error("sh_second needs the second image's cotangent (dL_dout_color2)");
    wg_raw_gaussians raw{};
    torch::Tensor f3d, rop;
    if (!raw_in.is_none()) {
        const py::tuple tu = raw_in.cast<py::tuple>();
        if (tu.size() != 2) throw std::runtime_error("raw is (filter_3D, raw_opacities)");
        f3d = f32(tu[0].cast<torch::Tensor>(), dev);
        rop = f32(tu[1].cast<torch::Tensor>(), dev);
        if (f3d.numel() != P64 || rop.numel() != P64) throw std::runtime_error("raw = (filter_3D, raw_opacities) must have P elements each");
        raw.filter_3D = ptr(f3d); raw.raw_opacities = ptr(rop);
    }
    // depth = None | (dL_ddepth [H, W], source): the checks of _C.py's _check_depth_grad_arguments, in its order, with its messages
    torch::Tensor dLd, dvalues;
    bool depth_distance = false;
    if (!depth.is_none()) {
        const char* source_msg = "return_depth must be \"distance\" or a float32 [P] tensor of per-Gaussian scalars on the frame's HIP device";
        const char* block_msg = "depth is (dL_ddepth, source): the depth cotangent [H, W] and the frame's return_depth source";
        const char* cot_msg = "dL_ddepth must be a float32 tensor of H * W elements on the frame's HIP device";
        if (!(py::isinstance<py::tuple>(depth) || py::isinstance<py::list>(depth)) || py::len(depth) != 2) throw std::runtime_error(block_msg);
        const py::sequence sq = depth.cast<py::sequence>();
        const py::object cot = sq[0], source = sq[1];
        if (!THPVariable_Check(cot.ptr())) throw std::runtime_error(cot_msg);
        dLd = cot.cast<torch::Tensor>();
        if (dLd.scalar_type() != torch::kFloat32 || dLd.numel() * 3 != dL_dout_color.numel() || dLd.device() != dL_dout_color.device()) throw std::runtime_error(cot_msg);
        depth_distance = py::isinstance<py::str>(source);
        if (depth_distance) {
            if (source.cast<std::string>() != "distance") throw std::runtime_error(source_msg);
        } else {
            if (!THPVariable_Check(source.ptr())) throw std::runtime_error(source_msg);
            dvalues = source.cast<torch::Tensor>();
            if (dvalues.scalar_type() != torch::kFloat32) throw std::runtime_error(source_msg);
            if (dvalues.numel() != P64) throw std::runtime_error("depth values must have P elements");
            if (!dvalues.is_cuda() || dvalues.device() != dL_dout_color.device()) throw std::runtime_error(source_msg);
            dvalues = dvalues.contiguous();
        }
        dLd = dLd.contiguous();
    }
    // distortion = None | (dL_ddistortion [H, W], moments [4, H, W], source): the checks of _C.py's _check_distortion_grad_arguments, in its order,
    // with its messages (an unknown string is a ValueError there and here)
    torch::Tensor dLt, mom, tvalues;
    bool dist_distance = false;
    if (!distortion.is_none()) {
        const char* source_msg = "return_distortion must be \"distance\" or a float32 [P] tensor of per-Gaussian scalars on the frame's HIP device";
        const char* block_msg = "distortion is (dL_ddistortion, moments, source): the distortion cotangent [H, W], the forward pass's moments [4, H, W] "
                                "and the frame's return_distortion source";
        const char* cot_msg = "dL_ddistortion must be a float32 tensor of H * W elements on the frame's HIP device";
        const char* mom_msg = "moments must be a float32 tensor of 4 * H * W elements on the frame's HIP device";
        if (!(py::isinstance<py::tuple>(distortion) || py::isinstance<py::list>(distortion)) || py::len(distortion) != 3) throw std::runtime_error(block_msg);
        const py::sequence sq = distortion.cast<py::sequence>();
        const py::object cot = sq[0], mo = sq[1], source = sq[2];
        if (!THPVariable_Check(cot.ptr())) throw std::runtime_error(cot_msg);
        dLt = cot.cast<torch::Tensor>();
        if (dLt.scalar_type() != torch::kFloat32 || dLt.numel() * 3 != dL_dout_color.numel() || dLt.device() != dL_dout_color.device()) throw std::runtime_error(cot_msg);
        if (!THPVariable_Check(mo.ptr())) throw std::runtime_error(mom_msg);
        mom = mo.cast<torch::Tensor>();
        if (mom.scalar_type() != torch::kFloat32 || mom.numel() * 3 != 4 * dL_dout_color.numel() || mom.device() != dL_dout_color.device()) throw std::runtime_error(mom_msg);
        dist_distance = py::isinstance<py::str>(source);
        if (dist_distance) {
            if (source.cast<std::string>() != "distance") throw py::value_error(source_msg);
        } else {
            if (!THPVariable_Check(source.ptr())) throw std::runtime_error(source_msg);
            tvalues = source.cast<torch::Tensor>();
            if (tvalues.scalar_type() != torch::kFloat32) throw std::runtime_error(source_msg);
            if (tvalues.numel() != P64) throw std::runtime_error("distortion values must have P elements");
            if (!tvalues.is_cuda() || tvalues.device() != dL_dout_color.device()) throw std::runtime_error(source_msg);
            tvalues = tvalues.contiguous();
        }
        dLt = dLt.contiguous();
        mom = mom.contiguous();
    }

    const int H = static_cast<int>(dL_dout_color.size(1)), W = static_cast<int>(dL_dout_color.size(2));
    const Inputs in(s, dev);
    const int M = in.M;
    // Every gradient tensor, allocated here and nowhere else.  The reference zero-fills nine tensors (:157-165); with the gradient record
    // every one of them is fully written by the library (zeros for culled Gaussians), without it the four accumulation targets (one of
    // them dL_dconic, the reference's intermediate: not returned, so not requested with the record) must arrive zeroed.
    const auto f = s.means3D.options().dtype(torch::kFloat32);
    if (colour_only) {   // wg_backward_args::colour_gradients_only: dL_dcolors alone exists, and the library fills it
        Gradients g;
        g.colors = P != 0 ? torch::empty({P, 3}, f) : torch::zeros({P, 3}, f);
        if (P == 0) return g;
        const auto dL = f32(dL_dout_color, dev);
        wg_backward_args a{};
        in.fill(a, s, H, W, &wg_backward_args::campos, co, dev);
        a.R = R;
        a.geom_buffer = bytes_of(geomBuffer); a.binning_buffer = bytes_of(binningBuffer); a.image_buffer = bytes_of(imageBuffer);
        a.dL_dpix = ptr(dL);
        a.dL_dcolor = g.colors.data_ptr<float>();
        a.colour_gradients_only = colour_only;   // 1: atomics; WG_COLOUR_GRADIENTS_FIXED_ORDER: slots + an ordered sum
        int status;
        {
            py::gil_scoped_release nogil;
            status = wg_rasterize_backward_ex(&a);
        }
        check(status, "wg_rasterize_backward");
        return g;
    }
    const bool record = P != 0 && (co.grad_record != 0 || co.deterministic_backward != 0), have_scales = s.scales.numel() != 0;
    auto alloc = [&](std::initializer_list<int64_t> shape, bool written) {
        return (P != 0 && written) ? torch::empty(shape, f) : torch::zeros(shape, f);
    };
    // want_colors / want_cov3D = false: the caller reads neither (the autograd function, for inputs that take no gradient).  Where the library
    // treats them as intermediates -- dL_dcolor with SH colours and the record, dL_dcov3D without cov3D_precomp -- they are then neither
    // allocated nor handed over (the per-Gaussian kernel skips the stores) and stay undefined; anywhere else they exist as ever.
    const bool colors_out = want_colors || !record || s.sh.numel() == 0, cov3D_out = want_cov3D || s.cov3D_precomp.numel() != 0;
    Gradients g;
    g.means3D = alloc({P, 3}, true); g.means2D = alloc({P, 3}, record); g.opacity = alloc({P, 1}, record);
    if (colors_out) g.colors = alloc({P, 3}, record);
    if (cov3D_out) g.cov3D = alloc({P, 6}, true); g.sh = alloc({P, M, 3}, true); g.scales = alloc({P, 3}, have_scales); g.rotations = alloc({P, 4}, have_scales);
    const torch::Tensor dL_dconic = record ? torch::Tensor() : torch::zeros({P, 2, 2}, f);
    if (dual) g.colors2 = alloc({P, 3}, true);
    if (tone.t.mul) g.mul = alloc({P, 3}, true);
    if (tone.t.offset) g.offset = alloc({P, 3}, true);
    if (tone2.t.mul) g.mul2 = alloc({P, 3}, true);
    if (tone2.t.offset) g.offset2 = alloc({P, 3}, true);
    if (!depth.is_none()) g.values = alloc({P}, true);   // (the library fills it)
    if (!distortion.is_none()) g.values_t = alloc({P}, true);   // (likewise)
    if (P == 0) return g;

    tone.t.dL_dmul = const_cast<float*>(ptr(g.mul)); tone.t.dL_doffset = const_cast<float*>(ptr(g.offset));
    tone2.t.dL_dmul = const_cast<float*>(ptr(g.mul2)); tone2.t.dL_doffset = const_cast<float*>(ptr(g.offset2));
    const auto dL = f32(dL_dout_color, dev);
    const auto rad = radii.contiguous();
    wg_backward_args a{};
    in.fill(a, s, H, W, &wg_backward_args::campos, co, dev);
    a.R = R;
    a.radii = rad.data_ptr<int>();
    a.geom_buffer = bytes_of(geomBuffer); a.binning_buffer = bytes_of(binningBuffer); a.image_buffer = bytes_of(imageBuffer);
    a.dL_dpix = ptr(dL);
    a.dL_dmean2D = g.means2D.data_ptr<float>(); a.dL_dconic = const_cast<float*>(ptr(dL_dconic));
    a.dL_dopacity = g.opacity.data_ptr<float>(); a.dL_dcolor = const_cast<float*>(ptr(g.colors)); a.dL_dmean3D = g.means3D.data_ptr<float>();
    a.dL_dcov3D = const_cast<float*>(ptr(g.cov3D)); a.dL_dsh = M ? g.sh.data_ptr<float>() : nullptr; a.dL_dscale = g.scales.data_ptr<float>();
    a.dL_drot = g.rotations.data_ptr<float>();
    if (tone.given) a.tone = &tone.t;
    wg_second_image second{};
    torch::Tensor dL2;
    if (two_tone || dual) {
        dL2 = f32(*dL_dout_color2, dev);
        second.dL_dpix2 = ptr(dL2);
        if (two_tone) { a.tone2 = &tone2.t; a.sh_second = 1; } else second.dL_dcolor2 = g.colors2.data_ptr<float>();
        a.second = &second;
    }
    if (!raw_in.is_none()) a.raw = &raw;
    wg_depth_grad dgrad{};
    if (!depth.is_none()) {   // the cotangent, the scalars (NULL = distance: the call's means3D and campos) and their gradient
        dgrad.struct_size = sizeof(dgrad);
        dgrad.dL_ddepth = dLd.data_ptr<float>(); dgrad.values = depth_distance ? nullptr : dvalues.data_ptr<float>(); dgrad.dL_dvalues = g.values.data_ptr<float>();
        a.depth = &dgrad;
    }
    wg_distortion_grad tgrad{};
    wg_backward_extras extras{};
    if (!distortion.is_none()) {   // wg_backward_args' size is pinned: the block travels in wg_backward_extras
        tgrad.struct_size = sizeof(tgrad);
        tgrad.dL_ddistortion = dLt.data_ptr<float>(); tgrad.moments = mom.data_ptr<float>();
        tgrad.values = dist_distance ? nullptr : tvalues.data_ptr<float>(); tgrad.dL_dvalues = g.values_t.data_ptr<float>();
        extras.struct_size = sizeof(extras);
        extras.distortion = &tgrad;
    }
    int status;
    {
        py::gil_scoped_release nogil;   // (as the forward call: a deferred frame's verdict may be waited for here)
        status = distortion.is_none() ? wg_rasterize_backward_ex(&a) : wg_rasterize_backward_with(&a, &extras);
    }
    check(status, "wg_rasterize_backward");
    return g;
}

py::object or_none(const torch::Tensor& t) { return t.defined() ? py::cast(t) : py::none(); }

}  // namespace

// rasterize_points.cu:35-119: `forward` with no optional block and the default options
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> RasterizeGaussiansHIP(
    const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
    const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy, const float kernel_size,
    const torch::Tensor& subpixel_offset, const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
    const torch::Tensor& campos, const bool prefiltered, const bool debug) {
    const py::object none = py::none();
    const Scene s{background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  &subpixel_offset, sh, degree, campos, debug};
    const ForwardResult r = forward(s, opacity, image_height, image_width, prefiltered, none, none, c10::nullopt, c10::nullopt, none, kDefaultOptions);
    return std::make_tuple(r.rendered, r.color, r.radii, r.geom, r.binning, r.img);
}

// rasterize_points.cu:121-204: `backward` likewise
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardHIP(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                              const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                              const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                              const float tan_fovx, const float tan_fovy, const float kernel_size, const torch::Tensor& subpixel_offset,
                              const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                              const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                              const bool debug) {
    const py::object none = py::none();
    const Scene s{background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  &subpixel_offset, sh, degree, campos, debug};
    const Gradients g = backward(s, radii, dL_dout_color, geomBuffer, R, binningBuffer, imageBuffer, none, c10::nullopt, none, none, kDefaultOptions);
    return std::make_tuple(g.means2D, g.colors, g.opacity, g.means3D, g.cov3D, g.sh, g.scales, g.rotations);   // :201
}

// rasterize_points.cu:206-225
torch::Tensor markVisible(torch::Tensor& means3D, torch::Tensor& viewmatrix, torch::Tensor& projmatrix) {
    const auto dev = means3D.device();
    const int P = static_cast<int>(means3D.size(0));
    torch::Tensor present = torch::zeros({P}, means3D.options().dtype(torch::kBool));
    if (P != 0) {
        const c10::DeviceGuard guard(dev);
        const auto m3 = f32(means3D, dev), vm = f32(viewmatrix, dev), pm = f32(projmatrix, dev);
        check(wg_mark_visible(P, ptr(m3), ptr(vm), ptr(pm), reinterpret_cast<unsigned char*>(present.data_ptr()),
                              c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream()), "wg_mark_visible");
    }
    return present;
}

// The projection-only pass (wg_project_radii): radii of the frame a forward call with these geometry inputs and this camera would render, from
// one launch on torch's current stream.  The checks of _C.py's _check_project_arguments, in its order, with its messages: shapes, modes and
// dtypes first, the device last.
torch::Tensor ProjectRadii(const torch::Tensor& means3D, const OptTensor& scales, const OptTensor& rotations, const OptTensor& cov3D_precomp,
                           const OptTensor& filter_3D, const float scale_modifier, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                           const float tan_fovx, const float tan_fovy, const float kernel_size, const int image_height, const int image_width) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3) throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    const int64_t P64 = means3D.size(0);
    if (scales.has_value() != rotations.has_value() || scales.has_value() == cov3D_precomp.has_value())
        throw std::runtime_error("project_radii needs exactly one of a scales / rotations pair or cov3D_precomp");
    if (filter_3D.has_value() && (cov3D_precomp.has_value() || filter_3D->numel() != P64))
        throw std::runtime_error("filter_3D (raw-parameter mode) needs scales and rotations, and P filter values");
    const std::pair<const char*, const torch::Tensor*> named[] = {
        {"means3D", &means3D}, {"scales", opt(scales)}, {"rotations", opt(rotations)}, {"cov3D_precomp", opt(cov3D_precomp)},
        {"filter_3D", opt(filter_3D)}, {"viewmatrix", &viewmatrix}, {"projmatrix", &projmatrix}};
    for (const auto& n : named)
        if (n.second && n.second->scalar_type() != torch::kFloat32) throw std::runtime_error(std::string(n.first) + " must be float32");
    auto sized = [&](const OptTensor& t, int64_t per, const char* name) {
        if (t.has_value() && t->numel() != per * P64) throw std::runtime_error(std::string(name) + " must have " + std::to_string(per) + " * P elements");
    };
    sized(scales, 3, "scales"); sized(rotations, 4, "rotations"); sized(cov3D_precomp, 6, "cov3D_precomp");
    for (const auto& n : {named[5], named[6]})
        if (n.second->ndimension() != 2 || n.second->size(0) != 4 || n.second->size(1) != 4)
            throw std::runtime_error(std::string(n.first) + " must have dimensions (4, 4)");
    if (image_height <= 0 || image_width <= 0) throw std::runtime_error("image_height and image_width must be positive");
    for (const auto& n : named)
        if (n.second && (!n.second->is_cuda() || n.second->device() != means3D.device()))
            throw std::runtime_error(std::string(n.first) + " must live on a HIP device, the one of means3D: this pass has no CPU path");

    const auto dev = means3D.device();
    const c10::DeviceGuard guard(dev);
    torch::Tensor radii = torch::empty({P64}, means3D.options().dtype(torch::kInt32));   // fully written by the kernel
    if (P64 == 0) return radii;
    auto cont = [](const OptTensor& t) { return t.has_value() ? t->contiguous() : torch::Tensor(); };
    const auto m3 = means3D.contiguous(), sc = cont(scales), rot = cont(rotations), cov = cont(cov3D_precomp), f3d = cont(filter_3D),
               vm = viewmatrix.contiguous(), pm = projmatrix.contiguous();
    wg_project_args a{};
    a.struct_size = sizeof(a);
    a.P = static_cast<int>(P64); a.width = image_width; a.height = image_height;
    a.means3D = ptr(m3); a.scales = ptr(sc); a.rotations = ptr(rot); a.cov3D_precomp = ptr(cov); a.filter_3D = ptr(f3d);
    a.scale_modifier = scale_modifier; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy; a.kernel_size = kernel_size;
    a.viewmatrix = ptr(vm); a.projmatrix = ptr(pm);
    a.radii = radii.data_ptr<int>();
    a.stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    int status;
    {
        py::gil_scoped_release nogil;
        status = wg_project_radii(&a);
    }
    check(status, "wg_project_radii");
    return radii;
}

// The depth pass (wg_render_depth): one scalar per Gaussian composited over the finished frame these three buffers belong to -> depth [H, W].
// The checks of _C.py's _check_depth_arguments, in its order, with its messages.
torch::Tensor RenderDepth(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const int R, const int P,
                          const int image_height, const int image_width, const py::object& source, const OptTensor& means3D, const OptTensor& campos,
                          const OptTensor& subpixel_offset, const std::tuple<int, int, int>& options, const OptTensor& out, const bool debug) {
    const char* source_msg = "return_depth must be \"distance\" or a float32 [P] tensor of per-Gaussian scalars on the frame's HIP device";
    const auto dev = imageBuffer.device();
    const bool distance = py::isinstance<py::str>(source);
    torch::Tensor values;
    if (distance) {
        if (source.cast<std::string>() != "distance") throw std::runtime_error(source_msg);
    } else {
        if (!THPVariable_Check(source.ptr())) throw std::runtime_error(source_msg);
        values = source.cast<torch::Tensor>();
        if (values.scalar_type() != torch::kFloat32) throw std::runtime_error(source_msg);
        if (values.numel() != P) throw std::runtime_error("depth values must have P elements");
        if (!values.is_cuda() || values.device() != dev) throw std::runtime_error(source_msg);
    }
    if (distance) {
        if (!means3D.has_value() || !campos.has_value()) throw std::runtime_error("depth source \"distance\" needs means3D and campos");
        if (means3D->scalar_type() != torch::kFloat32 || means3D->numel() != 3 * (int64_t)P || campos->scalar_type() != torch::kFloat32 || campos->numel() != 3)
            throw std::runtime_error("means3D must be float32 with 3 * P elements, campos float32 with 3");
        if (!means3D->is_cuda() || means3D->device() != dev || !campos->is_cuda() || campos->device() != dev)
            throw std::runtime_error("means3D and campos must live on the frame's HIP device");
    }
    if (P < 0 || R < 0 || image_height <= 0 || image_width <= 0)
        throw std::runtime_error("P and num_rendered must not be negative, image_height and image_width must be positive");
    const int64_t N = (int64_t)image_height * image_width;
    if (subpixel_offset.has_value() && subpixel_offset->numel() != 0 &&
        (subpixel_offset->scalar_type() != torch::kFloat32 || subpixel_offset->numel() != 2 * N || subpixel_offset->device() != dev))
        throw std::runtime_error("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device");
    if (out.has_value() && (out->scalar_type() != torch::kFloat32 || out->numel() != N || !out->is_contiguous() || out->device() != dev))
        throw std::runtime_error("out must be a contiguous float32 tensor of H * W elements on the frame's HIP device");
    if (!(geomBuffer.is_cuda() && binningBuffer.is_cuda() && imageBuffer.is_cuda())) throw std::runtime_error("the frame's buffers must live on a HIP device");

    const c10::DeviceGuard guard(dev);
    torch::Tensor depth = out.has_value() ? out->view({image_height, image_width})
                                          : torch::empty({image_height, image_width}, imageBuffer.options().dtype(torch::kFloat32));   // fully written by the library
    const auto m3 = distance ? means3D->contiguous() : torch::Tensor(), cam = distance ? campos->contiguous() : torch::Tensor(),
               val = distance ? torch::Tensor() : values.contiguous(),
               so = subpixel_offset.has_value() ? subpixel_offset->contiguous() : torch::Tensor();
    const wg_call_options co = call_options(options);
    wg_depth_args a{};
    a.struct_size = sizeof(a);
    a.P = P; a.R = R; a.width = image_width; a.height = image_height; a.debug = debug;
    if (P != 0) { a.geom_buffer = bytes_of(geomBuffer); a.binning_buffer = bytes_of(binningBuffer); a.image_buffer = bytes_of(imageBuffer); }
    a.subpixel_offset = ptr(so); a.values = ptr(val); a.means3D = ptr(m3); a.campos = ptr(cam);
    a.options = &co;
    a.out_depth = depth.data_ptr<float>();
    a.stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    int status;
    {
        py::gil_scoped_release nogil;
        status = wg_render_depth(&a);
    }
    check(status, "wg_render_depth");
    return depth;
}

// The contribution pass (wg_render_contributions): per Gaussian the largest blend weight, the number of blended pairs and their fixed-point sum
// over the finished frame these three buffers belong to, combined into the caller's [P] tensors (any may be None).
// The checks of _C.py's _check_contrib_arguments, in its order, with its messages.
void RenderContributions(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const int R, const int P,
                         const int image_height, const int image_width, const py::object& max_weight, const py::object& hits,
                         const py::object& weight_sum_q32, const py::object& pixel_mask, const OptTensor& subpixel_offset,
                         const std::tuple<int, int, int>& options, const bool accumulate, const bool debug) {
    const auto dev = imageBuffer.device();
    if (max_weight.is_none() && hits.is_none() && weight_sum_q32.is_none())
        throw std::runtime_error("at least one of max_weight, hits and weight_sum_q32 must be given");
    const auto output = [&](const py::object& o, const char* name, const torch::ScalarType dtype, const char* dname) {
        torch::Tensor t;
        if (o.is_none()) return t;
        const std::string msg = std::string(name) + " must be a contiguous " + dname + " tensor of P elements on the frame's HIP device";
        if (!THPVariable_Check(o.ptr())) throw std::runtime_error(msg);
        t = o.cast<torch::Tensor>();
        if (t.scalar_type() != dtype || t.numel() != P || !t.is_contiguous() || t.device() != dev) throw std::runtime_error(msg);
        return t;
    };
    const torch::Tensor mw = output(max_weight, "max_weight", torch::kFloat32, "float32"), hi = output(hits, "hits", torch::kInt64, "int64"),
                        ws = output(weight_sum_q32, "weight_sum_q32", torch::kInt64, "int64");
    if (P < 0 || R < 0 || image_height <= 0 || image_width <= 0)
        throw std::runtime_error("P and num_rendered must not be negative, image_height and image_width must be positive");
    const int64_t N = (int64_t)image_height * image_width;
    torch::Tensor mask;
    if (!pixel_mask.is_none()) {
        const char* mask_msg = "contribution_mask must be a float32 tensor of H * W elements on the frame's HIP device";
        if (!THPVariable_Check(pixel_mask.ptr())) throw std::runtime_error(mask_msg);
        mask = pixel_mask.cast<torch::Tensor>();
        if (mask.scalar_type() != torch::kFloat32 || mask.numel() != N || mask.device() != dev) throw std::runtime_error(mask_msg);
    }
    if (subpixel_offset.has_value() && subpixel_offset->numel() != 0 &&
        (subpixel_offset->scalar_type() != torch::kFloat32 || subpixel_offset->numel() != 2 * N || subpixel_offset->device() != dev))
        throw std::runtime_error("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device");
    if (!(geomBuffer.is_cuda() && binningBuffer.is_cuda() && imageBuffer.is_cuda())) throw std::runtime_error("the frame's buffers must live on a HIP device");
    if (P == 0) return;   // no Gaussian: nothing to fill, nothing to walk (an empty tensor has no address to hand to the library)

    const c10::DeviceGuard guard(dev);
    const auto mk = mask.defined() ? mask.contiguous() : torch::Tensor(), so = subpixel_offset.has_value() ? subpixel_offset->contiguous() : torch::Tensor();
    const wg_call_options co = call_options(options);
    wg_contrib_args a{};
    a.struct_size = sizeof(a);
    a.P = P; a.R = R; a.width = image_width; a.height = image_height; a.debug = debug;
    a.geom_buffer = bytes_of(geomBuffer); a.binning_buffer = bytes_of(binningBuffer); a.image_buffer = bytes_of(imageBuffer);
    a.subpixel_offset = ptr(so); a.pixel_mask = ptr(mk);
    a.options = &co;
    a.max_weight = mw.defined() ? mw.data_ptr<float>() : nullptr;
    a.hits = hi.defined() ? reinterpret_cast<unsigned long long*>(hi.data_ptr<int64_t>()) : nullptr;
    a.weight_sum_q32 = ws.defined() ? reinterpret_cast<unsigned long long*>(ws.data_ptr<int64_t>()) : nullptr;
    a.accumulate = accumulate ? 1 : 0;
    a.stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    int status;
    {
        py::gil_scoped_release nogil;
        status = wg_render_contributions(&a);
    }
    check(status, "wg_render_contributions");
}

// ---- everything beyond the reference, by argument (the blocks of wg_forward_args / wg_backward_args) -------------------------------------
// -> the reference's six, + the second image with colors2 / sh_second
py::tuple RasterizeGaussiansEx(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
                               const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
                               const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                               const float kernel_size, const OptTensor& subpixel_offset, const int image_height, const int image_width,
                               const torch::Tensor& sh, const int degree, const torch::Tensor& campos, const bool prefiltered, const bool debug,
                               const py::object& sh_tone, const py::object& binning_capacity, const OptTensor& colors2, const OptTensor& filter_3D,
                               const py::object& sh_second, const std::tuple<int, int, int>& options, const bool forward_only) {
    const Scene s{background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  opt(subpixel_offset), sh, degree, campos, debug};
    const ForwardResult r = forward(s, opacity, image_height, image_width, prefiltered, sh_tone, binning_capacity, colors2, filter_3D, sh_second,
                                    call_options(options), forward_only);
    if (r.color2.defined()) return py::make_tuple(r.rendered, r.color, r.radii, r.geom, r.binning, r.img, r.color2);
    return py::make_tuple(r.rendered, r.color, r.radii, r.geom, r.binning, r.img);
}
// (callers from before wg_forward_args::forward_only: a backward call may follow)
py::tuple RasterizeGaussiansExNoHint(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
                                     const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
                                     const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                     const float kernel_size, const OptTensor& subpixel_offset, const int image_height, const int image_width,
                                     const torch::Tensor& sh, const int degree, const torch::Tensor& campos, const bool prefiltered, const bool debug,
                                     const py::object& sh_tone, const py::object& binning_capacity, const OptTensor& colors2, const OptTensor& filter_3D,
                                     const py::object& sh_second, const std::tuple<int, int, int>& options) {
    return RasterizeGaussiansEx(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                kernel_size, subpixel_offset, image_height, image_width, sh, degree, campos, prefiltered, debug, sh_tone, binning_capacity,
                                colors2, filter_3D, sh_second, options, false);
}

// The distortion pass (wg_render_distortion): the distortion term of the finished frame these three buffers belong to -> distortion [H, W], or
// with moments = true (distortion, moments [4, H, W]).  The checks of _C.py's _check_distortion_arguments, in its order, with its messages.
py::object RenderDistortion(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const int R, const int P,
                            const int image_height, const int image_width, const py::object& source, const OptTensor& means3D, const OptTensor& campos,
                            const OptTensor& subpixel_offset, const std::tuple<int, int, int>& options, const bool want_moments, const bool debug) {
    const char* source_msg = "return_distortion must be \"distance\" or a float32 [P] tensor of per-Gaussian scalars on the frame's HIP device";
    const auto dev = imageBuffer.device();
    const bool distance = py::isinstance<py::str>(source);
    torch::Tensor values;
    if (distance) {
        if (source.cast<std::string>() != "distance") throw py::value_error(source_msg);
    } else {
        if (!THPVariable_Check(source.ptr())) throw std::runtime_error(source_msg);
        values = source.cast<torch::Tensor>();
        if (values.scalar_type() != torch::kFloat32) throw std::runtime_error(source_msg);
        if (values.numel() != P) throw std::runtime_error("distortion values must have P elements");
        if (!values.is_cuda() || values.device() != dev) throw std::runtime_error(source_msg);
    }
    if (distance) {
        if (!means3D.has_value() || !campos.has_value()) throw std::runtime_error("distortion source \"distance\" needs means3D and campos");
        if (means3D->scalar_type() != torch::kFloat32 || means3D->numel() != 3 * (int64_t)P || campos->scalar_type() != torch::kFloat32 || campos->numel() != 3)
            throw std::runtime_error("means3D must be float32 with 3 * P elements, campos float32 with 3");
        if (!means3D->is_cuda() || means3D->device() != dev || !campos->is_cuda() || campos->device() != dev)
            throw std::runtime_error("means3D and campos must live on the frame's HIP device");
    }
    if (P < 0 || R < 0 || image_height <= 0 || image_width <= 0)
        throw std::runtime_error("P and num_rendered must not be negative, image_height and image_width must be positive");
    const int64_t N = (int64_t)image_height * image_width;
    if (subpixel_offset.has_value() && subpixel_offset->numel() != 0 &&
        (subpixel_offset->scalar_type() != torch::kFloat32 || subpixel_offset->numel() != 2 * N || subpixel_offset->device() != dev))
        throw std::runtime_error("subpixel_offset must be float32 with H * W * 2 elements on the frame's HIP device");
    if (!(geomBuffer.is_cuda() && binningBuffer.is_cuda() && imageBuffer.is_cuda())) throw std::runtime_error("the frame's buffers must live on a HIP device");

    const c10::DeviceGuard guard(dev);
    const auto f = imageBuffer.options().dtype(torch::kFloat32);
    torch::Tensor dist = torch::empty({image_height, image_width}, f), mom;   // both fully written by the library
    if (want_moments) mom = torch::empty({4, image_height, image_width}, f);
    const auto m3 = distance ? means3D->contiguous() : torch::Tensor(), cam = distance ? campos->contiguous() : torch::Tensor(),
               val = distance ? torch::Tensor() : values.contiguous(),
               so = subpixel_offset.has_value() ? subpixel_offset->contiguous() : torch::Tensor();
    const wg_call_options co = call_options(options);
    wg_distortion_args a{};
    a.struct_size = sizeof(a);
    a.P = P; a.R = R; a.width = image_width; a.height = image_height; a.debug = debug;
    if (P != 0) { a.geom_buffer = bytes_of(geomBuffer); a.binning_buffer = bytes_of(binningBuffer); a.image_buffer = bytes_of(imageBuffer); }
    a.subpixel_offset = ptr(so); a.values = ptr(val); a.means3D = ptr(m3); a.campos = ptr(cam);
    a.options = &co;
    a.out_distortion = dist.data_ptr<float>();
    a.out_moments = want_moments ? mom.data_ptr<float>() : nullptr;
    a.stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    int status;
    {
        py::gil_scoped_release nogil;
        status = wg_render_distortion(&a);
    }
    check(status, "wg_render_distortion");
    if (want_moments) return py::make_tuple(dist, mom);
    return py::cast(dist);
}

// -> the reference's eight, + (mul, offset, mul2, offset2) with sh_second, + dL_dcolors2 with a second colour set, + (mul, offset) with sh_tone,
//    + the distortion's dL_dvalues [P] with the distortion block, + dL_dvalues [P] last with the depth block (None: absent)
py::tuple RasterizeGaussiansBackwardDistortion(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                       const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                                       const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                       const float tan_fovx, const float tan_fovy, const float kernel_size, const OptTensor& subpixel_offset,
                                       const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                                       const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                       const bool debug, const py::object& sh_tone, const OptTensor& dL_dout_color2, const py::object& raw_in,
                                       const py::object& sh_second, const std::tuple<int, int, int>& options, const bool want_colors,
                                       const bool want_cov3D, const py::object& depth, const py::object& distortion) {
    const Scene s{background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  opt(subpixel_offset), sh, degree, campos, debug};
    const Gradients g = backward(s, radii, dL_dout_color, geomBuffer, R, binningBuffer, imageBuffer, sh_tone, dL_dout_color2, raw_in, sh_second,
                                 call_options(options), 0, want_colors, want_cov3D, depth, distortion);
    py::list out;
    for (const auto& t : g.eight()) out.append(or_none(t));   // (None: dL_dcolors / dL_dcov3D that the caller did not want)
    if (!sh_second.is_none()) {
        for (const auto& t : {g.mul, g.offset, g.mul2, g.offset2}) out.append(or_none(t));
    } else if (dL_dout_color2.has_value()) {
        out.append(g.colors2);
    } else if (!sh_tone.is_none()) {
        out.append(or_none(g.mul)); out.append(or_none(g.offset));
    }
    if (!distortion.is_none()) out.append(g.values_t);   // + the distortion's dL_dvalues [P], in front of depth's
    if (!depth.is_none()) out.append(g.values);          // + dL_dvalues [P], last
    return py::tuple(out);
}

// (without the distortion block)
py::tuple RasterizeGaussiansBackwardDepth(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                       const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                                       const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                       const float tan_fovx, const float tan_fovy, const float kernel_size, const OptTensor& subpixel_offset,
                                       const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                                       const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                       const bool debug, const py::object& sh_tone, const OptTensor& dL_dout_color2, const py::object& raw_in,
                                       const py::object& sh_second, const std::tuple<int, int, int>& options, const bool want_colors,
                                       const bool want_cov3D, const py::object& depth) {
    return RasterizeGaussiansBackwardDistortion(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                                tan_fovx, tan_fovy, kernel_size, subpixel_offset, dL_dout_color, sh, degree, campos, geomBuffer, R,
                                                binningBuffer, imageBuffer, debug, sh_tone, dL_dout_color2, raw_in, sh_second, options, want_colors,
                                                want_cov3D, depth, py::none());
}

// (without the depth block: today's call)
py::tuple RasterizeGaussiansBackwardEx(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                       const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                                       const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                       const float tan_fovx, const float tan_fovy, const float kernel_size, const OptTensor& subpixel_offset,
                                       const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                                       const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                       const bool debug, const py::object& sh_tone, const OptTensor& dL_dout_color2, const py::object& raw_in,
                                       const py::object& sh_second, const std::tuple<int, int, int>& options, const bool want_colors,
                                       const bool want_cov3D) {
    return RasterizeGaussiansBackwardDepth(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                           tan_fovy, kernel_size, subpixel_offset, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                           debug, sh_tone, dL_dout_color2, raw_in, sh_second, options, want_colors, want_cov3D, py::none());
}

// (callers from before the two "wanted" flags: all eight)
py::tuple RasterizeGaussiansBackwardExAll(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                          const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                                          const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                          const float tan_fovx, const float tan_fovy, const float kernel_size, const OptTensor& subpixel_offset,
                                          const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                                          const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                          const bool debug, const py::object& sh_tone, const OptTensor& dL_dout_color2, const py::object& raw_in,
                                          const py::object& sh_second, const std::tuple<int, int, int>& options) {
    return RasterizeGaussiansBackwardEx(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                        tan_fovy, kernel_size, subpixel_offset, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                        debug, sh_tone, dL_dout_color2, raw_in, sh_second, options, true, true);
}

// the colour-only backward pass (wg_backward_args::colour_gradients_only; _C.py refuses the calls it does not serve in front of both
// bindings) -> the reference's eight places, dL_dcolors alone filled
py::tuple RasterizeGaussiansBackwardColour(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                           const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                                           const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                           const float tan_fovx, const float tan_fovy, const float kernel_size, const OptTensor& subpixel_offset,
                                           const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                                           const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                           const bool debug, const std::tuple<int, int, int>& options, const int mode) {
    if (mode != WG_COLOUR_GRADIENTS_ATOMIC && mode != WG_COLOUR_GRADIENTS_FIXED_ORDER) throw std::runtime_error("colour-only backward: mode is 1 (atomic) or 2 (fixed order)");
    const py::object none = py::none();
    const Scene s{background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                  opt(subpixel_offset), sh, degree, campos, debug};
    const Gradients g = backward(s, radii, dL_dout_color, geomBuffer, R, binningBuffer, imageBuffer, none, c10::nullopt, none, none, call_options(options), mode);
    return py::make_tuple(py::none(), g.colors, py::none(), py::none(), py::none(), py::none(), py::none(), py::none());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {   // ext.cpp:15-19
    m.def("rasterize_gaussians", &RasterizeGaussiansHIP);
    m.def("rasterize_gaussians_backward", &RasterizeGaussiansBackwardHIP);
    m.def("mark_visible", &markVisible);
    m.def("project_radii", &ProjectRadii);                                     // wg_project_radii: a frame's radii before it is rendered
    m.def("render_depth", &RenderDepth);                                       // wg_render_depth: a scalar per Gaussian composited over a finished frame
    m.def("render_distortion", &RenderDistortion);                             // wg_render_distortion: the distortion term of a finished frame (+ its moments)
    m.def("render_contributions", &RenderContributions);                       // wg_render_contributions: per-Gaussian contribution statistics of a finished frame
    m.def("rasterize_gaussians_ex", &RasterizeGaussiansEx);                    // + the blocks of wg_forward_args, + the forward_only hint
    m.def("rasterize_gaussians_ex", &RasterizeGaussiansExNoHint);              //   (overload without the hint)
    m.def("rasterize_gaussians_backward_ex", &RasterizeGaussiansBackwardEx);   // + the blocks of wg_backward_args, + which of dL_dcolors / dL_dcov3D the caller wants
    m.def("rasterize_gaussians_backward_ex", &RasterizeGaussiansBackwardExAll);   //   (overload without the two flags: all eight)
    m.def("rasterize_gaussians_backward_colour", &RasterizeGaussiansBackwardColour);   // wg_backward_args::colour_gradients_only
    m.def("rasterize_gaussians_backward_depth", &RasterizeGaussiansBackwardDepth);     // + wg_backward_args::depth: (dL_ddepth, source) -> ..., dL_dvalues
    m.def("rasterize_gaussians_backward_distortion", &RasterizeGaussiansBackwardDistortion);   // + wg_backward_extras::distortion: (dL_ddistortion, moments, source)
}
