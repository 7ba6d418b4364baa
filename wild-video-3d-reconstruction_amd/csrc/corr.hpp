// corr.hpp -- what the correlation units share (altcorr.hip: the exact fp16
// chain and the generic kernel; corrmfma.hip: the matrix-core kernel;
// patchify.hip: the backward and patchify): DPVO's window geometry, the one
// copy of the out-of-map rule, of the shared-box rule, of the reference's
// bilinear rounding sequence and of the stacked row's index decode.
#pragma once

#include "common.hpp"

namespace dpvo {
namespace corr {

// radius 3: an 8x8 raw window per patch pixel, bilinearly reduced to 7x7; 3x3 patches, 128 channels
constexpr int R = 3, D = 8, DO = 7, PS = 3, NP = 9, C = 128;
// The shared box: floor spreads up to 4 px (12 x 12).  At level 1 about 1 edge
// in 9 of the C3 workload spreads by 3 px (perspective scale ~1.4 between
// frames up to 35 apart); per-pixel windows would cost it 4x the common pass.
constexpr int BOX = 12;
// DPVO's stacked row [x][y][P][P][level] of the two-level pyramid (dpvo.py:333)
constexpr int ROW = DO * DO * NP * 2;
static_assert(ROW == 882, "the update operator's correlation input width");

// ---------------------------------------------------------------------------
// window pixels: offset (0 .. 2 radius + 1) of the window around floor(coordinate),
// in the reference's wrapping int arithmetic; a pixel outside the map reads as 0
// ---------------------------------------------------------------------------
__device__ __forceinline__ int window_px(int floor, int offset, int radius) { return wrap_add(floor, offset - radius); }
__device__ __forceinline__ bool in_map(int y, int x, int H, int W)
{
    // (an if, not `return a && b && ..`: that form changes the matrix-core kernel's branch code)
    if (y >= 0 && y < H && x >= 0 && x < W) return true;
    return false;
}

// ---------------------------------------------------------------------------
// The nine 8x8 windows of a patch overlap: when their floors spread by at most
// BOX - D pixels each way ("fast") they lie in one bh x bw box with origin
// (oy, ox), whose pixels are then read once for all nine.  Otherwise each patch
// pixel keeps its own D x D window (bw = bh = D; the origin is still min - R).
// The spread is taken in int64: saturated floors can lie 2^32 apart.
// Written into the caller's level record (any struct with fast, oy, ox, bh, bw), one field after the
// other: returned as a value of its own, the exact kernel's LDS stores were scheduled differently.
// ---------------------------------------------------------------------------
template <typename M>
__device__ __forceinline__ void patch_box(M& m, int ymin, int ymax, int xmin, int xmax)
{
    m.fast = ((int64_t)ymax - ymin) <= BOX - D && ((int64_t)xmax - xmin) <= BOX - D;
    m.oy = wrap_add(ymin, -R);
    m.ox = wrap_add(xmin, -R);
    m.bh = m.fast ? (ymax - ymin) + D : D;
    m.bw = m.fast ? (xmax - xmin) + D : D;
}

// ---------------------------------------------------------------------------
// The bilinear 8x8 -> 7x7 step in the reference's rounding sequence
// (correlation_kernel.cu:221-232, an ATen expression: every elementwise op
// rounded to T): the fractions converted to T, 1 - d in T, each weight one
// product in T; then w00 c00, + w01 c01, + w10 c10, + w11 c11, each product
// and each sum rounded to T.  T: half_t, half2_t (two levels at once, each lane
// rounding like the scalar), float, double.  Exact only in units built with
// -ffp-contract=off: a contracted multiply-add rounds once instead of twice.
// ---------------------------------------------------------------------------
template <typename T>
struct Bilinear { T w00, w01, w10, w11; };

template <typename T>
__device__ __forceinline__ Bilinear<T> bilinear_weights(float x, float y)
{
    const T dx = (T)(x - floorf(x)), dy = (T)(y - floorf(y));
    const T one = (T)1;
    const T omdx = one - dx, omdy = one - dy;
    return {omdx * omdy, dx * omdy, omdx * dy, dx * dy};
}

template <typename T>
__device__ __forceinline__ T bilinear(const Bilinear<T>& w, T c00, T c01, T c10, T c11)
{
    T v = w.w00 * c00;
    v = v + w.w01 * c01;
    v = v + w.w10 * c10;
    v = v + w.w11 * c11;
    return v;
}

// The matrix-core kernel's step (w0 .. w3 = bilinear_weights<float>) is deliberately another arithmetic: fp32, one
// explicit fma per term (one rounding, not two), so that it rounds alike whatever the compiler would contract.
__device__ __forceinline__ float cm_bilinear(float w0, float w1, float w2, float w3, float r00, float r01, float r10,
                                             float r11)
{
    float v = __builtin_fmaf(w3, r11, __builtin_fmaf(w2, r10, __builtin_fmaf(w1, r01, w0 * r00)));
    // an fp32 value, rounded to fp16 by the caller's conversion: without this
    // the compiler may fuse the last fma into the conversion (v_fma_mix*_f16:
    // one rounding instead of two)
    asm volatile("" : "+v"(v));
    return v;
}

// ---------------------------------------------------------------------------
// index decodes: window position pos = bx * DO + a (x offset, y offset), and
// element pair t = pos * NP + q of the stacked row (q: patch pixel; the pair
// is the two levels)
// ---------------------------------------------------------------------------
struct WindowPos { int bx, a; };
__device__ __forceinline__ WindowPos window_pos(int pos)
{
    const int bx = pos / DO;
    return {bx, pos - bx * DO};
}
// (spells window_pos out: calling it here changed the two-level exact kernel's instructions)
struct StackedPos { int q, bx, a; };
__device__ __forceinline__ StackedPos stacked_pos(int t)
{
    const int pos = t / NP, q = t - pos * NP;
    const int bx = pos / DO, a = pos - bx * DO;
    return {q, bx, a};
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// a feature map [.][N][C][H][W] stored channel-last with 16-byte aligned fp16 pixels
// (what a 16-byte load per lane needs; the batch stride and the base pointer are the caller's)
static inline bool channel_last_16b(const int64_t* st) { return st[2] == 1 && st[1] % 8 == 0 && st[3] % 8 == 0 && st[4] % 8 == 0; }

// dtype code -> f(T{}) with the element type (fp16 only where HALF); false for any other code
template <bool HALF = true, typename F>
bool dispatch_dtype(int dtype, F&& f)
{
    if constexpr (HALF)
        if (dtype == DPVO_F16) { f(half_t{}); return true; }
    if (dtype == DPVO_F32) { f(float{}); return true; }
    if (dtype == DPVO_F64) { f(double{}); return true; }
    return false;
}

}  // namespace corr
}  // namespace dpvo
