// geometry.hip -- fused projective ops of dpvo/projective_ops.py for gfx950,
// and the tracker's two single-pose kernels.
//
// The reference composes transform() from ~30 ATen/lietorch launches and
// materialises E*9 broadcast pose copies (lietorch/broadcasting.py:21-29);
// here one thread handles one edge: Gij = poses[jj] * poses[ii]^-1 once, then
// the P*P patch pixels, with lietorch's normalise-on-load semantics.
#include <algorithm>

#include "common.hpp"
#include "liegroups.hpp"

namespace dpvo {
namespace {

using lie::SE3;
using G3 = SE3<float>;

// ---------------------------------------------------------------------------
// The per-pixel rules, each written once.  A kernel's bits depend on the order
// of operations inside these expressions (and on how the compiler contracts
// them): tests/geometry_ref.py counts its bars from exactly this text.
// ---------------------------------------------------------------------------
// iproj (projective_ops.py:19-29): pixel (px, py) with inverse depth pd of a
// frame with intrinsics ki -> the homogeneous ray X0
__device__ __forceinline__ void backproject(const float* ki, float px, float py, float pd, float (&X0)[4])
{
    X0[0] = (px - ki[2]) / ki[0];
    X0[1] = (py - ki[3]) / ki[1];
    X0[2] = 1.0f;
    X0[3] = pd;
}

// proj of g * X0 with the target's intrinsics kj, Z clamped to >= 0.1
// (projective_ops.py:32-50); Z is the unclamped depth (the validity test)
struct Px {
    float x, y, d, Z;
};
__device__ __forceinline__ Px project(const G3& g, const float* kj, const float (&X0)[4])
{
    float X1[4];
    g.act4(X0, X1);
    const float d = 1.0f / fmaxf(X1[2], 0.1f);
    return {kj[0] * (d * X1[0]) + kj[2], kj[1] * (d * X1[1]) + kj[3], d, X1[2]};
}

// g with its rotation reset to the identity (transform's tonly, projective_ops.py:61-62)
__device__ __forceinline__ G3 translation_only(G3 g)
{
    g.so3.q.x = 0.f; g.so3.q.y = 0.f; g.so3.q.z = 0.f; g.so3.q.w = 1.f;
    return g;
}

// flow_mag of one pixel (projective_ops.py:111-121): p0 under Gii, p1 under
// Gij, p2 under the translation-only Gij
__device__ __forceinline__ float flow_term(const Px& p0, const Px& p1, const Px& p2, float beta)
{
    const float f1 = sqrtf((p1.x - p0.x) * (p1.x - p0.x) + (p1.y - p0.y) * (p1.y - p0.y));
    const float f2 = sqrtf((p2.x - p0.x) * (p2.x - p0.x) + (p2.y - p0.y) * (p2.y - p0.y));
    return beta * f1 + (1.0f - beta) * f2;
}

// PC: the patch size as a compile-time constant (3, every tracker preset) or
// 0 for a run-time P.  The operands are __restrict__ (coords / valid never
// alias the inputs) and, with PC, every patch value and both intrinsics are
// loaded before the first store: the previous loop, with possible aliasing,
// reloaded them after each pixel's stores -- a dependent L2 round trip per
// pixel (17 us at C3).
template <int PC>
__global__ __launch_bounds__(256) void transform_kernel(const float* __restrict__ poses,
                                                       const float* __restrict__ patches, int P,
                                                       const float* __restrict__ intr, const int64_t* __restrict__ ii,
                                                       const int64_t* __restrict__ jj, const int64_t* __restrict__ kk,
                                                       int64_t E, int flags, float* __restrict__ coords,
                                                       float* __restrict__ valid)
{
    const bool depth = flags & DPVO_TF_DEPTH, tonly = flags & DPVO_TF_TONLY, chw = flags & DPVO_TF_CHW;
    const int od = depth ? 3 : 2;
    const int64_t PP = PC ? PC * PC : (int64_t)P * P;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = ii[e], j = jj[e], k = kk[e];   // (the three index loads together)
        __builtin_amdgcn_sched_barrier(0);
        const float* pa = patches + k * 3 * PP;
        // Gij = poses[jj] * poses[ii].inv()   (projective_ops.py:60); raw pose
        // words first (G3::load normalizes: arithmetic on the loaded values)
        float rj[7], ri[7];
#pragma unroll
        for (int t = 0; t < 7; t++) {
            rj[t] = poses[j * 7 + t];
            ri[t] = poses[i * 7 + t];
        }
        float ki[4], kj[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            ki[t] = intr[i * 4 + t];
            kj[t] = intr[j * 4 + t];
        }
        float pv[3][PC ? PC * PC : 1];
        if constexpr (PC > 0) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int q = 0; q < PC * PC; q++) pv[c][q] = pa[c * PC * PC + q];
        }
        __builtin_amdgcn_sched_barrier(0);   // (every operand load issued before the arithmetic)
        G3 g = G3::load(rj).mul(G3::load(ri).inv());
        if (tonly) g = translation_only(g);
        auto pixel = [&](int64_t q, float px, float py, float pd) __attribute__((always_inline)) {
            float X0[4];
            backproject(ki, px, py, pd, X0);
            const Px p = project(g, kj, X0);
            if (chw) {
                coords[(e * od + 0) * PP + q] = p.x;
                coords[(e * od + 1) * PP + q] = p.y;
                if (depth) coords[(e * od + 2) * PP + q] = p.d;
            } else {
                coords[(e * PP + q) * od + 0] = p.x;
                coords[(e * PP + q) * od + 1] = p.y;
                if (depth) coords[(e * PP + q) * od + 2] = p.d;
            }
            if (valid) valid[e * PP + q] = p.Z > 0.2f ? 1.0f : 0.0f;
        };
        if constexpr (PC > 0) {
#pragma unroll
            for (int q = 0; q < PC * PC; q++) pixel(q, pv[0][q], pv[1][q], pv[2][q]);
        } else {
            for (int64_t q = 0; q < PP; q++) pixel(q, pa[q], pa[PP + q], pa[2 * PP + q]);
        }
    }
}

__global__ __launch_bounds__(256) void point_cloud_kernel(const float* __restrict__ poses,
                                                         const float* __restrict__ patches, int P,
                                                         const float* __restrict__ intr,
                                                         const int64_t* __restrict__ ix, int64_t m, int centre_only,
                                                         float* __restrict__ out)
{
    const int64_t PP = (int64_t)P * P, centre = (P / 2) * P + P / 2;
    // centre_only is the pixel range [centre, centre + 1) of the same loop, and
    // the loop is kept as one instance (no unrolling): the centre is then the
    // full cloud's pixel before its division by w.  Two copies of the body were
    // contracted into different FMAs, 10 ulp apart where the sum cancels.
    const int64_t q0 = centre_only ? centre : 0, q1 = centre_only ? centre + 1 : PP;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = ix[k];
        const float* pa = patches + k * 3 * PP;
        // every operand load of the first pixel issued before the arithmetic (G3::load normalizes)
        float rp[7], kv[4], c[3];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 7; t++) rp[t] = poses[f * 7 + t];
#pragma unroll
        for (int t = 0; t < 4; t++) kv[t] = intr[f * 4 + t];
#pragma unroll
        for (int t = 0; t < 3; t++) c[t] = pa[t * PP + q0];
        __builtin_amdgcn_sched_barrier(0);
        const G3 g = G3::load(rp).inv();
        int64_t q = q0;
#pragma unroll 1
        for (;;) {
            float X0[4], X1[4];
            backproject(kv, c[0], c[1], c[2], X0);
            g.act4(X0, X1);
            if (centre_only) {
                out[k * 3 + 0] = X1[0] / X1[3];
                out[k * 3 + 1] = X1[1] / X1[3];
                out[k * 3 + 2] = X1[2] / X1[3];
            } else {
                float* o = out + (k * PP + q) * 4;
                o[0] = X1[0]; o[1] = X1[1]; o[2] = X1[2]; o[3] = X1[3];
            }
            if (++q >= q1) break;
#pragma unroll
            for (int t = 0; t < 3; t++) c[t] = pa[t * PP + q];
        }
    }
}

// ---------------------------------------------------------------------------
// DPVO.motionmag (dpvo.py:507-514) for the two directions keyframe() reads
// (i -> j and j -> i, :609): mean over the matching edges and their P*P
// pixels of flow_mag = beta |x(Gij) - x(Gii)| + (1 - beta) |x(t-only Gij) -
// x(Gii)|.  out[d] = NaN when direction d has no edge (torch's mean of an
// empty tensor).
// ---------------------------------------------------------------------------
// direction of edge (a, b) for the frame pair (fi, fj): 0 for fi -> fj, 1 for
// fj -> fi, -1 for any other edge
__device__ __forceinline__ int edge_dir(int64_t a, int64_t b, int64_t fi, int64_t fj)
{
    return (a == fi && b == fj) ? 0 : (a == fj && b == fi) ? 1 : -1;
}

// adds the flow_mag of edge (a -> b, patch k)'s P*P pixels to acc, in pixel
// order (the loop unrolls where the kernel knows PP at compile time)
__device__ __forceinline__ void edge_flow(const float* poses, const float* patches, const float* intr, int64_t a,
                                          int64_t b, int64_t k, int64_t PP, float beta, float& acc)
{
    const G3 Pa = G3::load(poses + a * 7), Pb = G3::load(poses + b * 7);
    const G3 g0 = Pa.mul(Pa.inv());
    const G3 g1 = Pb.mul(Pa.inv());
    const G3 g2 = translation_only(g1);
    const float *ka = intr + a * 4, *kb = intr + b * 4;
    const float* pa = patches + k * 3 * PP;
    for (int64_t q = 0; q < PP; q++) {
        float X0[4];
        backproject(ka, pa[q], pa[PP + q], pa[2 * PP + q], X0);
        acc += flow_term(project(g0, ka, X0), project(g1, kb, X0), project(g2, kb, X0), beta);
    }
}

// Every thread's (sum, count) of the two directions -> the block's, in
// s_sum[d][0] / s_cnt[d][0], by a fixed tree: w = NT / 2 and halving, element
// t takes t + w.  That order is the one the tests' bars count, and it makes
// the result deterministic.
template <int NT>
__device__ __forceinline__ void tree_reduce(float (&s_sum)[2][NT], int (&s_cnt)[2][NT], const float (&sum)[2],
                                            const int (&cnt)[2])
{
    const int t = threadIdx.x;
    for (int d = 0; d < 2; d++) { s_sum[d][t] = sum[d]; s_cnt[d][t] = cnt[d]; }
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int d = 0; d < 2; d++) { s_sum[d][t] += s_sum[d][t + w]; s_cnt[d][t] += s_cnt[d][t + w]; }
        __syncthreads();
    }
}

__device__ __forceinline__ float mean_or_nan(float sum, int edges, int64_t PP)
{
    return edges ? sum / (float)((int64_t)edges * PP) : __builtin_nanf("");
}

// One workgroup scans the edge list (no mask -> index -> gather round trip, no
// host sync for the match count).
constexpr int MM_THREADS = 1024;
__global__ __launch_bounds__(MM_THREADS) void motion_mag_kernel(const float* poses, const float* patches, int P,
                                                               const float* intr, const int64_t* ii,
                                                               const int64_t* jj, const int64_t* kk, int64_t E,
                                                               int64_t fi, int64_t fj, float beta, float* out)
{
    __shared__ float s_sum[2][MM_THREADS];
    __shared__ int s_cnt[2][MM_THREADS];
    const int t = threadIdx.x;
    const int64_t PP = (int64_t)P * P;
    float sum[2] = {0.f, 0.f};
    int cnt[2] = {0, 0};
    for (int64_t e = t; e < E; e += MM_THREADS) {
        const int64_t a = ii[e], b = jj[e];
        const int dir = edge_dir(a, b, fi, fj);
        if (dir < 0) continue;
        edge_flow(poses, patches, intr, a, b, kk[e], PP, beta, sum[dir]);
        cnt[dir]++;
    }
    tree_reduce(s_sum, s_cnt, sum, cnt);
    if (t < 2) out[t] = mean_or_nan(s_sum[t][0], s_cnt[t][0], PP);
}

// The same two means over many workgroups (the single-workgroup scan of the
// ~95k-edge list takes ~80 us, a latency chain of dependent index loads per
// thread): one edge per thread (grid-stride past MM2_MAXBLK blocks), each
// workgroup reduces its threads into part[block] = (sum, count) per direction,
// and motion_mag_final_kernel adds the partials in a fixed order too.
constexpr int MM2_THREADS = 256, MM2_MAXBLK = 4096;
template <int PT>   // PT = P * P when known at compile time (the P*P pixel loop unrolls), else 0
__global__ __launch_bounds__(MM2_THREADS) void motion_mag_part_kernel(const float* poses, const float* patches, int P,
                                                                     const float* intr, const int64_t* ii,
                                                                     const int64_t* jj, const int64_t* kk, int64_t E,
                                                                     int64_t fi, int64_t fj, float beta, float* part)
{
    __shared__ float s_sum[2][MM2_THREADS];
    __shared__ int s_cnt[2][MM2_THREADS];
    const int t = threadIdx.x;
    const int64_t PP = PT ? PT : (int64_t)P * P;
    float sum[2] = {0.f, 0.f};
    int cnt[2] = {0, 0};
    for (int64_t e = blockIdx.x * (int64_t)MM2_THREADS + t; e < E; e += (int64_t)gridDim.x * MM2_THREADS) {
        const int64_t a = ii[e], b = jj[e];
        const int dir = edge_dir(a, b, fi, fj);
        if (dir < 0) continue;
        float s = 0.f;   // (the edge's own sum first: not the single-workgroup kernel's order)
        edge_flow(poses, patches, intr, a, b, kk[e], PP, beta, s);
        sum[dir] += s;
        cnt[dir]++;
    }
    tree_reduce(s_sum, s_cnt, sum, cnt);
    if (t < 2) {
        part[blockIdx.x * 4 + 2 * t] = s_sum[t][0];
        part[blockIdx.x * 4 + 2 * t + 1] = __int_as_float(s_cnt[t][0]);
    }
}

// partials of nblk workgroups -> the two means; 256 threads take strided
// partials, then the tree (deterministic for a given nblk)
__global__ __launch_bounds__(MM2_THREADS) void motion_mag_final_kernel(const float* part, int nblk, int64_t PP, float* out)
{
    __shared__ float s_sum[2][MM2_THREADS];
    __shared__ int s_cnt[2][MM2_THREADS];
    const int t = threadIdx.x;
    float sm[2] = {0.f, 0.f};
    int c[2] = {0, 0};
    for (int b = t; b < nblk; b += MM2_THREADS)
        for (int d = 0; d < 2; d++) {
            sm[d] += part[b * 4 + 2 * d];
            c[d] += __float_as_int(part[b * 4 + 2 * d + 1]);
        }
    tree_reduce(s_sum, s_cnt, sm, c);
    if (t < 2) out[t] = mean_or_nan(s_sum[t][0], s_cnt[t][0], PP);
}

// Keyframe distance matrix for the global BA's distance-based edges
// (dpvo.py:383-429 compute_keyframe_distance / get_distance_based_edges, which
// call flow_mag twice and .item() once per frame pair -- O(n^2) host syncs).
// dist[a][b] = mean over frame a's M patches and P*P pixels of flow_mag(a -> b),
// the same per-pixel arithmetic as edge_flow.  One workgroup per (a, block of
// KF_TB targets): frame a's back-projected pixels and their Gaa projection are
// staged in LDS once, each target's sum is reduced in a fixed tree order
// (deterministic).
constexpr int KF_THREADS = 256, KF_TB = 16;
__global__ __launch_bounds__(KF_THREADS) void keyframe_flow_kernel(const float* poses, const float* patches, int P,
                                                                  const float* intr, int64_t n, int64_t M,
                                                                  float beta, float* dist)
{
    extern __shared__ float kf_sh[];
    __shared__ float red[KF_THREADS];
    const int t = threadIdx.x;
    const int64_t a = blockIdx.x, b0 = (int64_t)blockIdx.y * KF_TB;
    const int64_t PP = (int64_t)P * P, NPX = M * PP;
    float* X0s = kf_sh;            // [4][NPX]
    float* c0s = kf_sh + 4 * NPX;  // [2][NPX]
    const G3 Pa = G3::load(poses + a * 7);
    const G3 Pai = Pa.inv();
    const G3 g0 = Pa.mul(Pai);     // transform(ii, ii): Gaa, as the reference composes it
    const float* ka = intr + a * 4;
    for (int64_t px = t; px < NPX; px += KF_THREADS) {
        const int64_t k = px / PP, q = px - k * PP;
        const float* pa = patches + (M * a + k) * 3 * PP;
        float X0[4];
        backproject(ka, pa[q], pa[PP + q], pa[2 * PP + q], X0);
        const Px p0 = project(g0, ka, X0);
#pragma unroll
        for (int c = 0; c < 4; c++) X0s[c * NPX + px] = X0[c];
        c0s[px] = p0.x;
        c0s[NPX + px] = p0.y;
    }
    __syncthreads();
    for (int bi = 0; bi < KF_TB; bi++) {
        const int64_t b = b0 + bi;
        if (b >= n) break;
        const G3 g1 = G3::load(poses + b * 7).mul(Pai);
        const G3 g2 = translation_only(g1);
        const float* kb = intr + b * 4;
        float sum = 0.f;
        for (int64_t px = t; px < NPX; px += KF_THREADS) {
            const float X0[4] = {X0s[px], X0s[NPX + px], X0s[2 * NPX + px], X0s[3 * NPX + px]};
            const Px p0 = {c0s[px], c0s[NPX + px], 0.f, 0.f};
            sum += flow_term(p0, project(g1, kb, X0), project(g2, kb, X0), beta);
        }
        red[t] = sum;
        __syncthreads();
        for (int w = KF_THREADS / 2; w > 0; w >>= 1) {   // (one float: not tree_reduce's two pairs)
            if (t < w) red[t] += red[t + w];
            __syncthreads();
        }
        if (t == 0) dist[a * n + b] = red[0] / (float)NPX;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// DPVO.__call__'s DAMPED_LINEAR motion model (dpvo.py:816-825) in one
// launch instead of five lietorch calls from Python (inv, mul, log, the scalar
// product, exp, mul): poses[n] = Exp(s Log(poses[n-1] poses[n-2]^-1)) poses[n-1],
// s = MOTION_DAMPING * dt ratio rounded to fp32 (as torch rounds the scalar).
// The same SE3 functions the lietorch kernels use, values kept in registers
// between them (fp32 either way).
__global__ void pose_extrapolate_kernel(float* poses, int64_t n, float s)
{
    const SE3<float> P1 = SE3<float>::load(poses + (n - 1) * 7), P2 = SE3<float>::load(poses + (n - 2) * 7);
    float xi[6];
    P1.mul(P2.inv()).Log(xi);
    for (int k = 0; k < 6; k++) xi[k] = xi[k] * s;
    SE3<float>::Exp(xi).mul(P1).store(poses + n * 7);
}

// keyframe()'s relative pose of a dropped frame (dpvo.py:613): out = a b^-1
__global__ void pose_relative_kernel(const float* a, const float* b, float* out)
{
    SE3<float>::load(a).mul(SE3<float>::load(b).inv()).store(out);
}

// K3 where the patch size is the tracker's 3 (the kernel instance with it as a
// compile-time constant), K0 for any other P
template <typename... A, typename... B>
void launch_by_patch(int P, void (*K3)(A...), void (*K0)(A...), unsigned grid, unsigned block, void* stream, B... args)
{
    hipLaunchKernelGGL(P == 3 ? K3 : K0, dim3(grid), dim3(block), 0, as_stream(stream), args...);
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" int dpvo_transform(const float* poses, const float* patches, int P, const float* intrinsics,
                              const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t num_edges, int flags,
                              float* coords, float* valid, void* stream)
{
    DPVO_CHECK_ARG(P >= 1, "bad patch size");
    if (num_edges == 0) return 0;
    DPVO_CHECK_ARG(poses && patches && intrinsics && ii && jj && kk && coords, "null operand");
    launch_by_patch(P, transform_kernel<3>, transform_kernel<0>, grid_for(num_edges, 256), 256, stream, poses, patches,
                    P, intrinsics, ii, jj, kk, num_edges, flags, coords, valid);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_point_cloud(const float* poses, const float* patches, int P, const float* intrinsics,
                                const int64_t* ix, int64_t m, int centre_only, float* out, void* stream)
{
    DPVO_CHECK_ARG(P >= 1, "bad patch size");
    if (m == 0) return 0;
    DPVO_CHECK_ARG(poses && patches && intrinsics && ix && out, "null operand");
    hipLaunchKernelGGL(point_cloud_kernel, dim3(grid_for(m, 256)), dim3(256), 0, as_stream(stream), poses, patches,
                       P, intrinsics, ix, m, centre_only, out);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_motion_mag(const float* poses, const float* patches, int P, const float* intrinsics,
                               const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t num_edges, int64_t i,
                               int64_t j, float beta, float* out, void* stream)
{
    DPVO_CHECK_ARG(P >= 1, "bad patch size");
    DPVO_CHECK_ARG(num_edges >= 0, "negative edge count");
    DPVO_CHECK_ARG(out && (num_edges == 0 || (poses && patches && intrinsics && ii && jj && kk)), "null operand");
    hipLaunchKernelGGL(motion_mag_kernel, dim3(1), dim3(MM_THREADS), 0, as_stream(stream), poses, patches, P,
                       intrinsics, ii, jj, kk, num_edges, i, j, beta, out);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_motion_mag_workspace_bytes(int64_t num_edges)
{
    (void)num_edges;
    return (size_t)MM2_MAXBLK * 4 * sizeof(float);
}

extern "C" int dpvo_motion_mag_ws(const float* poses, const float* patches, int P, const float* intrinsics,
                                  const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t num_edges, int64_t i,
                                  int64_t j, float beta, float* out, void* workspace, size_t workspace_bytes,
                                  void* stream)
{
    DPVO_CHECK_ARG(P >= 1, "bad patch size");
    DPVO_CHECK_ARG(num_edges >= 0, "negative edge count");
    DPVO_CHECK_ARG(out && (num_edges == 0 || (poses && patches && intrinsics && ii && jj && kk)), "null operand");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_motion_mag_workspace_bytes(num_edges), "workspace too small");
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>((num_edges + MM2_THREADS - 1) / MM2_THREADS,
                                                                  MM2_MAXBLK));
    launch_by_patch(P, motion_mag_part_kernel<9>, motion_mag_part_kernel<0>, nblk, MM2_THREADS, stream, poses, patches,
                    P, intrinsics, ii, jj, kk, num_edges, i, j, beta, (float*)workspace);
    hipLaunchKernelGGL(motion_mag_final_kernel, dim3(1), dim3(MM2_THREADS), 0, as_stream(stream),
                       (const float*)workspace, nblk, (int64_t)P * P, out);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_keyframe_flow_lds_bytes(int P, int64_t patches_per_frame)
{
    return (size_t)6 * P * P * patches_per_frame * sizeof(float);
}

extern "C" int dpvo_keyframe_flow(const float* poses, const float* patches, int P, const float* intrinsics,
                                  int64_t num_frames, int64_t patches_per_frame, float beta, float* dist, void* stream)
{
    DPVO_CHECK_ARG(P >= 1 && num_frames >= 0 && patches_per_frame >= 1, "bad sizes");
    DPVO_CHECK_ARG(num_frames < 65536 * (int64_t)KF_TB, "too many frames");
    if (num_frames == 0) return 0;
    DPVO_CHECK_ARG(poses && patches && intrinsics && dist, "null operand");
    const size_t lds = dpvo_keyframe_flow_lds_bytes(P, patches_per_frame);
    DPVO_CHECK_ARG(lds + KF_THREADS * sizeof(float) <= 160 * 1024, "one frame's patches do not fit in LDS");
    const dim3 grid((unsigned)num_frames, (unsigned)((num_frames + KF_TB - 1) / KF_TB));
    hipLaunchKernelGGL(keyframe_flow_kernel, grid, dim3(KF_THREADS), lds, as_stream(stream), poses, patches, P,
                       intrinsics, num_frames, patches_per_frame, beta, dist);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_pose_extrapolate(float* poses, int64_t n, float s, void* stream)
{
    DPVO_CHECK_ARG(poses != nullptr && n >= 2, "poses[n-2], poses[n-1] needed (n >= 2)");
    hipLaunchKernelGGL(pose_extrapolate_kernel, dim3(1), dim3(1), 0, as_stream(stream), poses, n, s);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_pose_relative(const float* a, const float* b, float* out, void* stream)
{
    DPVO_CHECK_ARG(a && b && out, "null operand");
    hipLaunchKernelGGL(pose_relative_kernel, dim3(1), dim3(1), 0, as_stream(stream), a, b, out);
    DPVO_CHECK_LAUNCH();
    return 0;
}
