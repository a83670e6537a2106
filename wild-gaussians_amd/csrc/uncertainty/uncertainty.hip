// Fused uncertainty head and DINO loss for gfx950 (include/wg_uncertainty.h): what UncertaintyModel._compute_losses does around the frozen
// backbone in its default mode (wildgaussians/method.py:363-433, :190-201, :267-323), restated.
//
// Everything here is streaming or reduction work:
//   * the feature maps [C, N] are read coalesced along the N positions; head_stats and head_backward give one 256-thread workgroup to a
//     channel, head_forward and cosine give one to 64 positions (its four waves take every fourth channel; the folded coefficient of a
//     channel is wave-uniform, so it is a scalar load) and add the four wave sums in a fixed order in LDS;
//   * maps_forward is one pass over H x W (36 B read, 4 B written per pixel); the 4 taps of s per pixel come from a map of a few KB;
//   * maps_backward gathers, per cell of s, over the at most (2 P + 1)^2 full-resolution pixels and the downsampled pixels that touch it.
// No atomics; every sum is a butterfly within the wave, then wave 0..3 in order, then workgroup partials in order (finish, in double).
#include <hip/hip_runtime.h>
#include <cmath>
#include <stddef.h>
#include "wg_uncertainty.h"
#include "wg_rasterizer.h"

namespace wgu {

constexpr int TPB = 256;          // every kernel: 4 waves
constexpr int MAP_TW = 64, MAP_TH = 16;   // maps_forward's tile: a wave per row, four rows per thread
constexpr int DINO_TW = 64, DINO_TH = 4;  // dino_loss: one pixel per thread

// One axis of F.interpolate(mode="bilinear", align_corners=False): src = (dst + 0.5) * in / out - 0.5, clamped at 0, in integers:
// i0 = floor(src), i1 = min(i0 + 1, in - 1), l = src - i0 (one rounding).  in == out gives i0 = dst, l = 0.
struct Tap {
    int i0, i1;
    float l;
};

__host__ __device__ inline Tap make_tap(int dst, int in, int out) {
    int num = (2 * dst + 1) * in - out;
    const int den = 2 * out;
    if (num < 0) num = 0;
    Tap t;
    t.i0 = num / den;
    t.l = (float)(num - t.i0 * den) / (float)den;
    t.i1 = t.i0 + 1 < in ? t.i0 + 1 : in - 1;
    return t;
}

// torch's order: h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
__device__ inline float bilerp(const float* __restrict__ m, int stride, const Tap& ty, const Tap& tx) {
    const float w1 = tx.l, w0 = 1.f - tx.l, h1 = ty.l, h0 = 1.f - ty.l;
    const float* r0 = m + (size_t)ty.i0 * stride;
    const float* r1 = m + (size_t)ty.i1 * stride;
    return h0 * (w0 * r0[tx.i0] + w1 * r0[tx.i1]) + h1 * (w0 * r1[tx.i0] + w1 * r1[tx.i1]);
}

// the weight of cell i in the tap (both taps name the same cell at the clamped last row / column)
__device__ inline float tap_weight(const Tap& t, int i) { return (t.i0 == i ? 1.f - t.l : 0.f) + (t.i1 == i ? t.l : 0.f); }

// Sum of K values per thread over the 256 threads, the same bits in every thread: butterfly in the wave, then waves 0..3 in order.
template <int K>
__device__ inline void block_sum(float (&v)[K], float* red /* [4 * K] */) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // a previous use of `red` is over
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ void __launch_bounds__(TPB) prepare_kernel(int H, int W, int h, int w, int pad_top, int pad_left, int hP, int wP,
                                                      const float* __restrict__ img, const float* __restrict__ mean,
                                                      const float* __restrict__ stdv, float* __restrict__ out) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), c = blockIdx.z;
    if (X >= wP || Y >= hP) return;
    const int y = Y - pad_top, x = X - pad_left;
    float v = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {
        const Tap ty = make_tap(y, H, h), tx = make_tap(x, W, w);
        v = (bilerp(img + (size_t)c * H * W, W, ty, tx) - mean[c]) / stdv[c];
    }
    out[((size_t)c * hP + Y) * wP + X] = v;
}

// ------------------------------------------------------------------------------------------------ head
// Welford per thread, Chan's merge across lanes and waves: one pass, no cancellation.
struct Moments {
    float n, mean, m2;
};
__device__ inline Moments merge(const Moments& a, const Moments& b) {
    Moments r;
    r.n = a.n + b.n;
    if (r.n == 0.f) return Moments{0.f, 0.f, 0.f};
    const float d = b.mean - a.mean, f = b.n / r.n;
    r.mean = a.mean + d * f;
    r.m2 = a.m2 + b.m2 + d * d * a.n * f;
    return r;
}

__global__ void __launch_bounds__(TPB) head_stats_kernel(int C, int N, int training, const float* __restrict__ x, const float* __restrict__ kdrop,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ w, float eps, float momentum, float* __restrict__ running_mean,
                                                         float* __restrict__ running_var, float* __restrict__ coef, float* __restrict__ stats) {
    __shared__ Moments red[4];
    const int c = blockIdx.x;
    float m, v;
    const float k = kdrop[c];
    if (training) {
        const float* xc = x + (size_t)c * N;
        Moments a{0.f, 0.f, 0.f};
        for (int p = threadIdx.x; p < N; p += TPB) {
            const float val = xc[p];
            a.n += 1.f;
            const float d = val - a.mean;
            a.mean += d / a.n;
            a.m2 += d * (val - a.mean);
        }
        for (int d = 32; d >= 1; d >>= 1) {
            Moments o{__shfl_xor(a.n, d), __shfl_xor(a.mean, d), __shfl_xor(a.m2, d)};
            // both partners must get the same bits: merge (lower lane, upper lane) in that order on both sides
            a = (threadIdx.x & d) ? merge(o, a) : merge(a, o);
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x != 0) return;
        a = merge(merge(merge(red[0], red[1]), red[2]), red[3]);
        const float var = a.m2 / (float)N;
        m = k * a.mean;
        v = k * k * var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (k * k * (a.m2 / (float)(N - 1)));
    } else {
        if (threadIdx.x != 0) return;
        m = running_mean[c];
        v = running_var[c];
    }
    const float inv = 1.f / sqrtf(v + eps);
    coef[c] = w[c] * gamma[c] * k * inv;
    coef[C + c] = w[c] * (beta[c] - gamma[c] * m * inv);
    stats[c] = m;
    stats[C + c] = inv;
}

__global__ void __launch_bounds__(TPB) head_forward_kernel(int C, int N, const float* __restrict__ x, const float* __restrict__ coef,
                                                           const float* __restrict__ conv_bias, float* __restrict__ s, float* __restrict__ dsdl) {
    __shared__ float red[4], part[4][64];
    float q[1] = {0.f};
    for (int c = threadIdx.x; c < C; c += TPB) q[0] += coef[C + c];
    block_sum<1>(q, red);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (p < N) {
        const float* xp = x + p;
        int c = wave;
        for (; c + 12 < C; c += 16) {   // four loads in flight; coef[c] is wave-uniform
            const float x0 = xp[(size_t)c * N], x1 = xp[(size_t)(c + 4) * N], x2 = xp[(size_t)(c + 8) * N], x3 = xp[(size_t)(c + 12) * N];
            acc += coef[c] * x0;
            acc += coef[c + 4] * x1;
            acc += coef[c + 8] * x2;
            acc += coef[c + 12] * x3;
        }
        for (; c < C; c += 4) acc += coef[c] * xp[(size_t)c * N];
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || p >= N) return;
    const float z = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) + (q[0] + conv_bias[0] + 0.5413248546129181f);  // log(e - 1)
    float sp, d;
    if (z > 20.f) {
        sp = z;
        d = 1.f;
    } else {
        const float e = expf(z);
        sp = log1pf(e);
        d = e / (e + 1.f);
    }
    s[p] = sp;
    dsdl[p] = d;
}

__global__ void __launch_bounds__(TPB) head_backward_kernel(int C, int N, const float* __restrict__ x, const float* __restrict__ ds,
                                                            const float* __restrict__ dsdl, const float* __restrict__ kdrop,
                                                            const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ w,
                                                            float* __restrict__ d_gamma, float* __restrict__ d_beta, float* __restrict__ d_w,
                                                            float* __restrict__ d_b) {
    __shared__ float red[8];
    const int c = blockIdx.x;
    const float* xc = x + (size_t)c * N;
    float g[2] = {0.f, 0.f};
    for (int p = threadIdx.x; p < N; p += TPB) {
        const float dl = ds[p] * dsdl[p];
        g[0] += dl;
        g[1] += dl * xc[p];
    }
    block_sum<2>(g, red);
    if (threadIdx.x != 0) return;
    const float xs = stats[C + c] * (kdrop[c] * g[1] - stats[c] * g[0]);   // sum_p dlogit_p * xhat_cp
    d_w[c] = gamma[c] * xs + beta[c] * g[0];
    d_gamma[c] = w[c] * xs;
    d_beta[c] = w[c] * g[0];
    if (c == 0) d_b[0] = g[0];
}

// ------------------------------------------------------------------------------------------------ maps
struct MapGeom {
    int H, W, P, hp, wp, pad_top, pad_left;
    float clip_min;
};

// bilinear(s) at full-resolution pixel (y, x) of the cropped frame, BEFORE the clamp
__device__ inline float s_at(const float* __restrict__ s, const MapGeom& g, int y, int x) {
    return bilerp(s, g.wp, make_tap(y + g.pad_top, g.hp, g.hp * g.P), make_tap(x + g.pad_left, g.wp, g.wp * g.P));
}

__global__ void __launch_bounds__(TPB) maps_forward_kernel(MapGeom g, int C, const float* __restrict__ s, const float* __restrict__ gt,
                                                           const float* __restrict__ pred, const float* __restrict__ ssim,
                                                           const float* __restrict__ msssim, float* __restrict__ loss_mult,
                                                           float* __restrict__ partials) {
    __shared__ float red[24];
    const int x = blockIdx.x * MAP_TW + (threadIdx.x & 63);
    const int ybase = blockIdx.y * MAP_TH + (threadIdx.x >> 6);
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (x < g.W) {
        const Tap tx = make_tap(x + g.pad_left, g.wp, g.wp * g.P);
        const size_t plane = (size_t)g.H * g.W;
#pragma unroll
        for (int r = 0; r < MAP_TH / 4; ++r) {
            const int y = ybase + 4 * r;
            if (y >= g.H) break;
            const Tap ty = make_tap(y + g.pad_top, g.hp, g.hp * g.P);
            const float u = fmaxf(bilerp(s, g.wp, ty, tx), g.clip_min);
            const float lm = fminf(1.f / (2.f * (u * u)), 3.f);
            const size_t i = (size_t)y * g.W + x;
            float mse = 0.f;
            for (int c = 0; c < C; ++c) {
                const float d = gt[c * plane + i] - pred[c * plane + i];
                mse += d * d;
            }
            const float ss = ssim[i], ms = msssim[i];
            loss_mult[i] = lm;
            acc[0] += logf(u);
            acc[1] += lm;
            acc[2] += ss * lm;
            acc[3] += mse * lm;
            acc[4] += ss;
            acc[5] += ms;
        }
    }
    block_sum<6>(acc, red);
    if (threadIdx.x == 0) {
        float* o = partials + 6 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        for (int k = 0; k < 6; ++k) o[k] = acc[k];
    }
}

// ------------------------------------------------------------------------------------------------ dino
__global__ void __launch_bounds__(TPB) cosine_kernel(int C, int N, float eps, const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ out) {
    __shared__ float part[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    if (p < N)
        for (int c = wave; c < C; c += 4) {
            const float va = a[(size_t)c * N + p], vb = b[(size_t)c * N + p];
            ab += va * vb;
            aa += va * va;
            bb += vb * vb;
        }
    part[0][wave][lane] = ab;
    part[1][wave][lane] = aa;
    part[2][wave][lane] = bb;
    __syncthreads();
    if (wave != 0 || p >= N) return;
    ab = ((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane];
    aa = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
    bb = ((part[2][0][lane] + part[2][1][lane]) + part[2][2][lane]) + part[2][3][lane];
    out[p] = ab / (fmaxf(sqrtf(aa), eps) * fmaxf(sqrtf(bb), eps));   // each norm is clamped on its own
}

struct DinoGeom {
    int nh, nw, hd, wd, dpad_top, dpad_left;
};

// 1 / (2 u^2) at full-resolution pixel (y, x)
__device__ inline float lm_at(const float* __restrict__ s, const MapGeom& g, int y, int x) {
    const float u = fmaxf(s_at(s, g, y, x), g.clip_min);
    return 1.f / (2.f * (u * u));
}

__global__ void __launch_bounds__(TPB) dino_loss_kernel(MapGeom g, DinoGeom q, const float* __restrict__ s, const float* __restrict__ cosm,
                                                        float* __restrict__ dino_part, float* __restrict__ partials) {
    __shared__ float red[4];
    const int x = blockIdx.x * DINO_TW + (threadIdx.x & 63), y = blockIdx.y * DINO_TH + (threadIdx.x >> 6);
    float acc[1] = {0.f};
    if (x < q.nw && y < q.nh) {
        const float c = bilerp(cosm, q.wd, make_tap(y + q.dpad_top, q.hd, q.hd * g.P), make_tap(x + q.dpad_left, q.wd, q.wd * g.P));
        const float dp = fminf(fmaxf(1.f - (c - 0.5f) / 0.5f, 0.f), 1.f);
        dino_part[(size_t)y * q.nw + x] = dp;
        float lm;
        if (q.nh == g.H && q.nw == g.W) {
            lm = lm_at(s, g, y, x);
        } else {
            const Tap ty = make_tap(y, g.H, q.nh), tx = make_tap(x, g.W, q.nw);
            const float w1 = tx.l, w0 = 1.f - tx.l, h1 = ty.l, h0 = 1.f - ty.l;
            lm = h0 * (w0 * lm_at(s, g, ty.i0, tx.i0) + w1 * lm_at(s, g, ty.i0, tx.i1)) +
                 h1 * (w0 * lm_at(s, g, ty.i1, tx.i0) + w1 * lm_at(s, g, ty.i1, tx.i1));
        }
        acc[0] = dp * lm;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// ------------------------------------------------------------------------------------------------ finish
__global__ void __launch_bounds__(TPB) finish_kernel(int H, int W, int nh, int nw, float reg_weight, int n_maps, int n_dino,
                                                     const float* __restrict__ maps_partials, const float* __restrict__ dino_partials,
                                                     float* __restrict__ result) {
    __shared__ double red[7][TPB];
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_maps; i += TPB)
        for (int k = 0; k < 6; ++k) a[k] += (double)maps_partials[6 * (size_t)i + k];
    for (int i = threadIdx.x; i < n_dino; i += TPB) a[6] += (double)dino_partials[i];
    for (int k = 0; k < 7; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int d = TPB / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int k = 0; k < 7; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double px = (double)H * W;
    const double beta = red[0][0] / px, uloss = red[6][0] / ((double)nh * nw);
    const double mse_d = red[3][0] / red[1][0];
    result[0] = (float)(uloss + (double)reg_weight * beta);
    result[1] = (float)(red[4][0] / px);
    result[2] = (float)(red[5][0] / px);
    result[3] = (float)(red[2][0] / red[1][0]);
    result[4] = (float)mse_d;
    result[5] = (float)(10.0 * log10(1.0 / mse_d));
    result[6] = (float)beta;
    result[7] = (float)uloss;
}

// ------------------------------------------------------------------------------------------------ maps backward
// One workgroup per cell (i, j) of s.  A full-resolution pixel reaches the cell through the upsampling's taps; its padded row lies in
// [P i - (P + 1) / 2, P i + P + (P + 1) / 2] (for any P; the exact membership is the tap weight, which is 0 outside).  With downsampling, a
// downsampled pixel reaches the cell through those of its four full-resolution taps that lie in that window.
__global__ void __launch_bounds__(TPB) maps_backward_kernel(MapGeom g, int nh, int nw, float reg_weight, const float* __restrict__ s,
                                                            const float* __restrict__ dino_part, const float* __restrict__ grad_loss,
                                                            float* __restrict__ ds) {
    __shared__ float red[4];
    const int i = blockIdx.x / g.wp, j = blockIdx.x % g.wp;
    const int half = (g.P + 1) / 2;
    const int Hp = g.hp * g.P, Wp = g.wp * g.P;
    // window in cropped coordinates, clipped to the frame
    const int ya = max(g.P * i - half - g.pad_top, 0), yb = min(g.P * i + g.P + half - g.pad_top, g.H - 1);
    const int xa = max(g.P * j - half - g.pad_left, 0), xb = min(g.P * j + g.P + half - g.pad_left, g.W - 1);
    const int ny = yb - ya + 1, nx = xb - xa + 1;
    const bool same = nh == g.H && nw == g.W;
    const float cb = reg_weight / ((float)g.H * (float)g.W), cd = 1.f / ((float)nh * (float)nw);
    float acc[1] = {0.f};
    if (ny > 0 && nx > 0) {
        for (int t = threadIdx.x; t < ny * nx; t += TPB) {
            const int y = ya + t / nx, x = xa + t % nx;
            const Tap ty = make_tap(y + g.pad_top, g.hp, Hp), tx = make_tap(x + g.pad_left, g.wp, Wp);
            const float wc = tap_weight(ty, i) * tap_weight(tx, j);
            const float u = bilerp(s, g.wp, ty, tx);
            if (wc != 0.f && u >= g.clip_min) {
                float gu = cb / u;                                                        // d beta / du
                if (same) gu -= cd * dino_part[(size_t)y * nw + x] / (u * u * u);         // d (dino_part / (2 u^2)) / du
                acc[0] += gu * wc;
            }
        }
        if (!same) {
            // resized pixels whose first tap row lies in [ya - 1, yb]: a conservative range for any scale factor (an axis that is
            // enlarged clamps its source index at 0, which only moves pixels INTO the range's first rows); the tap weights decide
            const float fy = (float)nh / (float)g.H, fx = (float)nw / (float)g.W;
            const int qya = max((int)floorf((ya - 0.5f) * fy - 0.5f) - 1, 0), qyb = min((int)ceilf((yb + 1.5f) * fy - 0.5f) + 1, nh - 1);
            const int qxa = max((int)floorf((xa - 0.5f) * fx - 0.5f) - 1, 0), qxb = min((int)ceilf((xb + 1.5f) * fx - 0.5f) + 1, nw - 1);
            const int qny = qyb - qya + 1, qnx = qxb - qxa + 1;
            for (int t = threadIdx.x; t < qny * qnx; t += TPB) {
                const int qy = qya + t / qnx, qx = qxa + t % qnx;
                const float dp = dino_part[(size_t)qy * nw + qx];
                if (dp == 0.f) continue;
                const Tap dy = make_tap(qy, g.H, nh), dx = make_tap(qx, g.W, nw);
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int y = (k & 2) ? dy.i1 : dy.i0, x = (k & 1) ? dx.i1 : dx.i0;
                    const float wq = ((k & 2) ? dy.l : 1.f - dy.l) * ((k & 1) ? dx.l : 1.f - dx.l);
                    if (y < ya || y > yb || x < xa || x > xb) continue;
                    const Tap ty = make_tap(y + g.pad_top, g.hp, Hp), tx = make_tap(x + g.pad_left, g.wp, Wp);
                    const float wc = tap_weight(ty, i) * tap_weight(tx, j);
                    const float u = bilerp(s, g.wp, ty, tx);
                    if (wc != 0.f && u >= g.clip_min) sum -= wq * wc / (u * u * u);
                }
                acc[0] += cd * dp * sum;
            }
        }
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) ds[blockIdx.x] = acc[0] * grad_loss[0];
}

// ------------------------------------------------------------------------------------------------ host checks
inline bool tap_fits(long in, long out) { return in >= 1 && out >= 1 && 2 * in * out + in < (1L << 31); }

inline bool geom_ok(int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min) {
    if (H < 1 || W < 1 || P < 1 || hp < 1 || wp < 1 || !(clip_min > 0.f)) return false;
    if ((long)hp * P >= (1L << 20) || (long)wp * P >= (1L << 20) || (long)hp * wp >= (1L << 31)) return false;
    if (!tap_fits(hp, (long)hp * P) || !tap_fits(wp, (long)wp * P)) return false;
    if (pad_top < 0 || pad_left < 0 || (long)pad_top + H > (long)hp * P || (long)pad_left + W > (long)wp * P) return false;
    return true;
}

inline int done() { return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP; }

}  // namespace wgu

using namespace wgu;

extern "C" {

int wg_uncertainty_prepare(int C, int H, int W, int h, int w, int pad_top, int pad_left, int hP, int wP, const float* img, const float* mean,
                           const float* std, float* out, void* stream) {
    if (C < 1 || H < 1 || W < 1 || h < 1 || w < 1 || hP < 1 || wP < 1 || !img || !mean || !std || !out) return WG_ERR_INVALID_ARGUMENT;
    if (pad_top < 0 || pad_left < 0 || (long)pad_top + h > hP || (long)pad_left + w > wP) return WG_ERR_INVALID_ARGUMENT;
    if (!tap_fits(H, h) || !tap_fits(W, w) || C > 65535 || (hP + 3) / 4 > 65535) return WG_ERR_INVALID_ARGUMENT;
    dim3 grid((wP + 63) / 64, (hP + 3) / 4, C);
    hipLaunchKernelGGL(prepare_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, H, W, h, w, pad_top, pad_left, hP, wP, img, mean, std, out);
    return done();
}

int wg_uncertainty_head_stats(int C, int N, int training, const float* x, const float* kdrop, const float* bn_weight, const float* bn_bias,
                              const float* conv_weight, float eps, float momentum, float* running_mean, float* running_var, float* coef,
                              float* stats, void* stream) {
    if (C < 1 || N < 1 || (training && N < 2) || !x || !kdrop || !bn_weight || !bn_bias || !conv_weight || !running_mean || !running_var ||
        !coef || !stats || !(eps >= 0.f))
        return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(head_stats_kernel, dim3(C), dim3(TPB), 0, (hipStream_t)stream, C, N, training, x, kdrop, bn_weight, bn_bias, conv_weight,
                       eps, momentum, running_mean, running_var, coef, stats);
    return done();
}

int wg_uncertainty_head_forward(int C, int N, const float* x, const float* coef, const float* conv_bias, float* s, float* dsdl, void* stream) {
    if (C < 1 || N < 1 || !x || !coef || !conv_bias || !s || !dsdl) return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(head_forward_kernel, dim3((N + 63) / 64), dim3(TPB), 0, (hipStream_t)stream, C, N, x, coef, conv_bias, s, dsdl);
    return done();
}

int wg_uncertainty_head_backward(int C, int N, const float* x, const float* ds, const float* dsdl, const float* kdrop, const float* stats,
                                 const float* bn_weight, const float* bn_bias, const float* conv_weight, float* d_bn_weight, float* d_bn_bias,
                                 float* d_conv_weight, float* d_conv_bias, void* stream) {
    if (C < 1 || N < 1 || !x || !ds || !dsdl || !kdrop || !stats || !bn_weight || !bn_bias || !conv_weight || !d_bn_weight || !d_bn_bias ||
        !d_conv_weight || !d_conv_bias)
        return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(head_backward_kernel, dim3(C), dim3(TPB), 0, (hipStream_t)stream, C, N, x, ds, dsdl, kdrop, stats, bn_weight, bn_bias,
                       conv_weight, d_bn_weight, d_bn_bias, d_conv_weight, d_conv_bias);
    return done();
}

size_t wg_uncertainty_maps_scratch_floats(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return 6 * (size_t)((W + MAP_TW - 1) / MAP_TW) * (size_t)((H + MAP_TH - 1) / MAP_TH);
}

int wg_uncertainty_maps_forward(int C, int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, const float* s,
                                const float* gt, const float* pred, const float* ssim, const float* msssim, float* loss_mult, float* partials,
                                void* stream) {
    if (C < 1 || !geom_ok(H, W, P, hp, wp, pad_top, pad_left, clip_min) || !s || !gt || !pred || !ssim || !msssim || !loss_mult || !partials)
        return WG_ERR_INVALID_ARGUMENT;
    dim3 grid((W + MAP_TW - 1) / MAP_TW, (H + MAP_TH - 1) / MAP_TH);
    hipLaunchKernelGGL(maps_forward_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, MapGeom{H, W, P, hp, wp, pad_top, pad_left, clip_min}, C, s,
                       gt, pred, ssim, msssim, loss_mult, partials);
    return done();
}

int wg_uncertainty_cosine(int C, int N, float eps, const float* a, const float* b, float* cos, void* stream) {
    if (C < 1 || N < 1 || !a || !b || !cos || !(eps >= 0.f)) return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(cosine_kernel, dim3((N + 63) / 64), dim3(TPB), 0, (hipStream_t)stream, C, N, eps, a, b, cos);
    return done();
}

size_t wg_uncertainty_dino_scratch_floats(int nh, int nw) {
    if (nh < 1 || nw < 1) return 0;
    return (size_t)((nw + DINO_TW - 1) / DINO_TW) * (size_t)((nh + DINO_TH - 1) / DINO_TH);
}

static bool dino_ok(int H, int W, int P, int nh, int nw) {
    if (nh < 1 || nw < 1) return false;   // a side may be LARGER than the frame's: dino_downsample rounds up to a multiple of 14
    return tap_fits(H, nh) && tap_fits(W, nw) && (nh + DINO_TH - 1) / DINO_TH <= 65535;
}

int wg_uncertainty_dino_loss(int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, const float* s, int nh, int nw,
                             int hd, int wd, int dpad_top, int dpad_left, const float* cos, float* dino_part, float* partials, void* stream) {
    if (!geom_ok(H, W, P, hp, wp, pad_top, pad_left, clip_min) || !dino_ok(H, W, P, nh, nw) ||
        !geom_ok(nh, nw, P, hd, wd, dpad_top, dpad_left, clip_min) || !s || !cos || !dino_part || !partials)
        return WG_ERR_INVALID_ARGUMENT;
    dim3 grid((nw + DINO_TW - 1) / DINO_TW, (nh + DINO_TH - 1) / DINO_TH);
    hipLaunchKernelGGL(dino_loss_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, MapGeom{H, W, P, hp, wp, pad_top, pad_left, clip_min},
                       DinoGeom{nh, nw, hd, wd, dpad_top, dpad_left}, s, cos, dino_part, partials);
    return done();
}

int wg_uncertainty_finish(int H, int W, int nh, int nw, float regularizer_weight, const float* maps_partials, const float* dino_partials,
                          float* result, void* stream) {
    const size_t nm = wg_uncertainty_maps_scratch_floats(H, W) / 6, nd = wg_uncertainty_dino_scratch_floats(nh, nw);
    if (nm == 0 || nd == 0 || nm >= (1UL << 31) || nd >= (1UL << 31) || !maps_partials || !dino_partials || !result) return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, H, W, nh, nw, regularizer_weight, (int)nm, (int)nd,
                       maps_partials, dino_partials, result);
    return done();
}

int wg_uncertainty_maps_backward(int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, float regularizer_weight,
                                 const float* s, int nh, int nw, const float* dino_part, const float* grad_loss, float* ds, void* stream) {
    if (!geom_ok(H, W, P, hp, wp, pad_top, pad_left, clip_min) || !dino_ok(H, W, P, nh, nw) || !s || !dino_part || !grad_loss || !ds)
        return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(maps_backward_kernel, dim3(hp * wp), dim3(TPB), 0, (hipStream_t)stream, MapGeom{H, W, P, hp, wp, pad_top, pad_left, clip_min},
                       nh, nw, regularizer_weight, s, dino_part, grad_loss, ds);
    return done();
}

}  // extern "C"
