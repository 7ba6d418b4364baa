// patchify.hip -- the reference cuda_corr extension's functions that are off
// the tracker's hot path (gfx950): the correlation backward (autograd;
// correlation_kernel.cu:236-286) and patchify forward / backward (:288-333;
// the torch-encoder fallback).  One thread per element, atomics into fp32 /
// fp64 gradients.  Built with -ffp-contract=off like altcorr.hip, which these
// kernels were part of: the backward's tap sum would contract otherwise.
// The kernels spell corr.hpp's window-pixel rule out (wrap_add(floor, offset - radius), then the bounds):
// through corr::window_px / in_map, in any of four forms, they compile to other instructions than before.
#include "corr.hpp"

namespace dpvo {
namespace {

// ---------------------------------------------------------------------------
// backward (training surface): atomics into fp32/fp64 grads
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void corr_backward_kernel(const T* gmap, int N1, int C, int PH, int PW,
                                                            const T* fmap, int N2, int H2, int W2,
                                                            const float* coords, const int64_t* ii,
                                                            const int64_t* jj, const float* grad, int B, int E,
                                                            int radius, T* g1, T* g2, int64_t total)
{
    const int D = 2 * radius + 2, Do = D - 1;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t n = idx;
        const int j0 = n % PW; n /= PW;
        const int i0 = n % PH; n /= PH;
        const int c = n % D; n /= D;   // x offset in the raw window
        const int a = n % D; n /= D;   // y offset
        const int e = n % E; n /= E;
        const int b = (int)n;
        const float* cb = coords + (((int64_t)b * E + e) * 2) * PH * PW + i0 * PW + j0;
        const float x = cb[0], y = cb[PH * PW];
        const float dx = x - floorf(x), dy = y - floorf(y);
        // raw-window gradient = sum of the bilinear taps that read (a, c)
        float g = 0.f;
        auto G = [&](int aa, int cc) -> float {
            if (aa < 0 || aa >= Do || cc < 0 || cc >= Do) return 0.f;
            // grad layout: [B][E][x][y][PH][PW]
            return grad[((((int64_t)b * E + e) * Do + cc) * Do + aa) * PH * PW + i0 * PW + j0];
        };
        g += (1 - dx) * (1 - dy) * G(a, c);
        g += dx * (1 - dy) * G(a, c - 1);
        g += (1 - dx) * dy * G(a - 1, c);
        g += dx * dy * G(a - 1, c - 1);
        if (g == 0.f) continue;
        const int ix = (int)ii[e], jx = (int)jj[e];
        if (ix < 0 || ix >= N1 || jx < 0 || jx >= N2) continue;
        const int i1 = wrap_add(floor_to_int_sat(y), a - radius), j1 = wrap_add(floor_to_int_sat(x), c - radius);
        if (!(i1 >= 0 && i1 < H2 && j1 >= 0 && j1 < W2)) continue;
        const T* f1 = gmap + (((int64_t)b * N1 + ix) * C) * PH * PW + i0 * PW + j0;
        const T* f2 = fmap + (((int64_t)b * N2 + jx) * C) * H2 * W2 + (int64_t)i1 * W2 + j1;
        T* d1 = g1 + (((int64_t)b * N1 + ix) * C) * PH * PW + i0 * PW + j0;
        T* d2 = g2 + (((int64_t)b * N2 + jx) * C) * H2 * W2 + (int64_t)i1 * W2 + j1;
        for (int k = 0; k < C; k++) {
            atomicAdd(d1 + (int64_t)k * PH * PW, (T)g * f2[(int64_t)k * H2 * W2]);
            atomicAdd(d2 + (int64_t)k * H2 * W2, (T)g * f1[(int64_t)k * PH * PW]);
        }
    }
}

// ---------------------------------------------------------------------------
// patchify
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void patchify_forward_kernel(const T* net, int64_t s0, int64_t s1, int64_t s2,
                                                               int64_t s3, int B, int C, int H, int W,
                                                               const float* coords, int M, int radius, T* out,
                                                               int64_t total)
{
    const int D = 2 * radius + 2;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t n = idx;
        const int bb = n % D; n /= D;
        const int a = n % D; n /= D;
        const int k = n % C; n /= C;
        const int m = n % M; n /= M;
        const int b = (int)n;
        const float x = coords[((int64_t)b * M + m) * 2 + 0], y = coords[((int64_t)b * M + m) * 2 + 1];
        const int i = wrap_add(floor_to_int_sat(y), a - radius), j = wrap_add(floor_to_int_sat(x), bb - radius);
        T v = (T)0;
        if (i >= 0 && i < H && j >= 0 && j < W) v = net[b * s0 + k * s1 + (int64_t)i * s2 + (int64_t)j * s3];
        out[idx] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void patchify_backward_kernel(int B, int C, int H, int W, const float* coords,
                                                                int M, int radius, const T* grad, T* net_grad,
                                                                int64_t total)
{
    const int D = 2 * radius + 2;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t n = idx;
        const int bb = n % D; n /= D;
        const int a = n % D; n /= D;
        const int k = n % C; n /= C;
        const int m = n % M; n /= M;
        const int b = (int)n;
        const float x = coords[((int64_t)b * M + m) * 2 + 0], y = coords[((int64_t)b * M + m) * 2 + 1];
        const int i = wrap_add(floor_to_int_sat(y), a - radius), j = wrap_add(floor_to_int_sat(x), bb - radius);
        if (i >= 0 && i < H && j >= 0 && j < W)
            atomicAdd(net_grad + (((int64_t)b * C + k) * H + i) * W + j, grad[idx]);
    }
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" int dpvo_corr_backward(int dtype, const void* gmap, const int64_t* gsz, const void* fmap,
                                  const int64_t* fsz, const float* coords, const int64_t* csz, const int64_t* ii,
                                  const int64_t* jj, const float* grad, int radius, void* gmap_grad, void* fmap_grad,
                                  void* stream)
{
    DPVO_CHECK_ARG(dtype == DPVO_F32 || dtype == DPVO_F64, "backward supports float32/float64 feature maps");
    DPVO_CHECK_ARG(csz[2] == 2 && radius >= 0, "bad coords / radius");
    const int D = 2 * radius + 2;
    const int64_t total = csz[0] * csz[1] * D * D * csz[3] * csz[4];
    if (total == 0) return 0;
    const unsigned grid = grid_for(total, 256, 65536);
    corr::dispatch_dtype<false>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(corr_backward_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T*)gmap,
                           (int)gsz[1], (int)gsz[2], (int)csz[3], (int)csz[4], (const T*)fmap, (int)fsz[1],
                           (int)fsz[3], (int)fsz[4], coords, ii, jj, grad, (int)csz[0], (int)csz[1], radius,
                           (T*)gmap_grad, (T*)fmap_grad, total);
    });
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_patchify_forward(int dtype, const void* net, const int64_t* nsz, const int64_t* nst,
                                     const float* coords, int64_t M, int radius, void* out, void* stream)
{
    DPVO_CHECK_ARG(radius >= 0 && radius <= 64, "bad radius");
    const int D = 2 * radius + 2;
    const int64_t total = nsz[0] * M * nsz[1] * D * D;
    if (total == 0) return 0;
    const unsigned grid = grid_for(total, 256, 65536);
    const bool known = corr::dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(patchify_forward_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T*)net,
                           nst[0], nst[1], nst[2], nst[3], (int)nsz[0], (int)nsz[1], (int)nsz[2], (int)nsz[3], coords,
                           (int)M, radius, (T*)out, total);
    });
    DPVO_CHECK_ARG(known, "unsupported dtype");
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_patchify_backward(int dtype, const int64_t* nsz, const float* coords, int64_t M, int radius,
                                      const void* grad, void* net_grad, void* stream)
{
    DPVO_CHECK_ARG(dtype == DPVO_F32 || dtype == DPVO_F64, "patchify backward supports float32/float64");
    const int D = 2 * radius + 2;
    const int64_t total = nsz[0] * M * nsz[1] * D * D;
    if (total == 0) return 0;
    const unsigned grid = grid_for(total, 256, 65536);
    corr::dispatch_dtype<false>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(patchify_backward_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (int)nsz[0],
                           (int)nsz[1], (int)nsz[2], (int)nsz[3], coords, (int)M, radius, (const T*)grad,
                           (T*)net_grad, total);
    });
    DPVO_CHECK_LAUNCH();
    return 0;
}
