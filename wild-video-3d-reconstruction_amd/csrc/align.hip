// align.hip -- Sim(3) between two matched point clouds for loop closure:
// RANSAC over 3-point Umeyama models and the least-squares refit on the
// winner's inliers, device-resident and in fp64 (the reference:
// dpvo/loop_closure/optim_utils.py:64-150, numba on the host after a
// device->host copy).
//
// The hypothesis samples come from the caller (int32 [H][3]); the device draws
// no random numbers, so the result is a pure function of the inputs and can be
// compared hypothesis by hypothesis with a host restatement.
//
// score kernel: one wave per hypothesis, four waves per workgroup.  Every lane
// computes the same 3-point model (wave-uniform values, no divergence), the
// lanes stride over the N points, the wave sums its counts with lane swaps.
// select kernel: one workgroup.  Winner = the first hypothesis whose count
// exceeds early_exit, else the first with the largest count -- what the
// reference's sequential loop (break at inliers > 100, strict improvement)
// returns on the same samples.  It recomputes the winner's model, writes the
// inlier mask and refits over it: means first, then centred sums, each a
// fixed-order reduction (per-thread strided sums, then an LDS tree), bitwise
// repeatable.
//
// Umeyama's SVD is a one-sided Jacobi iteration on the 3x3 covariance itself
// (column rotations; cov^T cov is never formed, so small singular values keep
// their relative accuracy and the reference's absolute rank rule at 2^-52 is
// testable).  A 3-point covariance has rank <= 2: the third left singular
// vector is always completed as u1 x u2, the third singular value carries its
// sign (b3 . u3), and the reflection fix det(U) det(V) < 0 then reduces to
// R = u1 v1^T + u2 v2^T + sign(det V) u3 v3^T, tr(D S) = d1 + d2 + sign(det V) d3.
//
// This file is compiled without FMA contraction (Makefile): both kernels then
// evaluate the model and the threshold test with the same roundings, which
// are those of the reference's expression order.
#include <float.h>

#include "common.hpp"

namespace dpvo {
namespace align {

enum { CODE_OK = 0, CODE_NO_HYPOTHESIS = 1, CODE_DEGENERATE_REFIT = 2 };
enum { JACOBI_SWEEPS = 12, BLOCK = 256, WAVES = BLOCK / 64 };

struct Model {
    double M[9];   // c R, row-major
    double R[9];
    double t[3];
    double c;
};

// the workspace: the refit's moments, written by the first pass and read by the second
struct Moments {
    double mx[3], my[3];
    long long n;
};

__host__ __device__ __forceinline__ void rotate_columns(double* a, int p, int q, double cs, double sn)
{
    for (int r = 0; r < 3; r++) {
        const double ap = a[r * 3 + p], aq = a[r * 3 + q];
        a[r * 3 + p] = cs * ap - sn * aq;
        a[r * 3 + q] = sn * ap + cs * aq;
    }
}

__host__ __device__ __forceinline__ void swap_columns(double* a, int p, int q)
{
    for (int r = 0; r < 3; r++) {
        const double v = a[r * 3 + p];
        a[r * 3 + p] = a[r * 3 + q];
        a[r * 3 + q] = v;
    }
}

__host__ __device__ __forceinline__ double column_dot(const double* a, int p, int q)
{
    return a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];
}

// Umeyama (IEEE PAMI 1991) from the moments: y ~ c R x + t.  cov = sum of
// (y - my)(x - mx)^T / n, sigma_x = sum |x - mx|^2 / n.  false: the covariance
// has fewer than 2 singular values above DBL_EPSILON (the reference's rule).
__host__ __device__ static bool umeyama_solve(const double* mx, const double* my, const double* cov, double sigma_x, Model& m)
{
    double B[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; i++) B[i] = cov[i];
    // one-sided Jacobi: rotate column pairs of B (and of V) until they are orthogonal: B = cov V
    for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = column_dot(B, p, p), beta = column_dot(B, q, q), gamma = column_dot(B, p, q);
            if (!(fabs(gamma) > DBL_EPSILON * sqrt(alpha * beta)) || gamma == 0.0) continue;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
            rotate_columns(B, p, q, cs, sn);
            rotate_columns(V, p, q, cs, sn);
        }
    }
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = sqrt(column_dot(B, k, k));
    // descending order (the reflection fix belongs to the smallest singular value)
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
        const int p = pq == 1 ? 1 : 0, q = pq == 1 ? 2 : 1;   // (0,1) (1,2) (0,1)
        if (d[p] < d[q]) {
            const double v = d[p];
            d[p] = d[q];
            d[q] = v;
            swap_columns(B, p, q);
            swap_columns(V, p, q);
        }
    }
    int rank = 0;
    for (int k = 0; k < 3; k++) rank += d[k] > DBL_EPSILON ? 1 : 0;
    if (rank < 2) return false;
    double u1[3], u2[3], u3[3];
    for (int r = 0; r < 3; r++) u1[r] = B[r * 3] / d[0];
    for (int r = 0; r < 3; r++) u2[r] = B[r * 3 + 1] / d[1];
    // the columns are orthogonal to rounding; one Gram-Schmidt step keeps U orthonormal when d2 << d1
    const double o = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int r = 0; r < 3; r++) u2[r] -= o * u1[r];
    const double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int r = 0; r < 3; r++) u2[r] /= n2;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double d3 = B[2] * u3[0] + B[5] * u3[1] + B[8] * u3[2];   // signed
    const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) +
                        V[2] * (V[3] * V[7] - V[4] * V[6]);
    const double sg = detV < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            m.R[i * 3 + j] = u1[i] * V[j * 3] + u2[i] * V[j * 3 + 1] + sg * (u3[i] * V[j * 3 + 2]);
    m.c = (d[0] + d[1] + sg * d3) / sigma_x;
    for (int i = 0; i < 9; i++) m.M[i] = m.R[i] * m.c;
    for (int i = 0; i < 3; i++)
        m.t[i] = my[i] - m.c * (m.R[i * 3] * mx[0] + m.R[i * 3 + 1] * mx[1] + m.R[i * 3 + 2] * mx[2]);
    return true;
}

// the model of one 3-point sample; false: an index outside [0, N), a repeated
// index, or a degenerate covariance
__host__ __device__ static bool sample_model(const double* __restrict__ src, const double* __restrict__ dst, int N,
                                    const int* __restrict__ s, Model& m)
{
    const int a = s[0], b = s[1], c = s[2];
    if (a < 0 || a >= N || b < 0 || b >= N || c < 0 || c >= N || a == b || a == c || b == c) return false;
    const int idx[3] = {a, b, c};
    double x[3][3], y[3][3], mx[3], my[3];
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++) {
            x[k][r] = src[(size_t)idx[k] * 3 + r];
            y[k][r] = dst[(size_t)idx[k] * 3 + r];
        }
    for (int r = 0; r < 3; r++) {
        mx[r] = (x[0][r] + x[1][r] + x[2][r]) / 3.0;
        my[r] = (y[0][r] + y[1][r] + y[2][r]) / 3.0;
    }
    double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var = 0;
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 3; i++) {
            const double xi = x[k][i] - mx[i];
            var += xi * xi;
            for (int j = 0; j < 3; j++) cov[j * 3 + i] += (y[k][j] - my[j]) * xi;
        }
    for (int i = 0; i < 9; i++) cov[i] /= 3.0;
    return umeyama_solve(mx, my, cov, var / 3.0, m);
}

// |c R x + t - y| < threshold, in the reference's order: (x @ (c R)^T + t) - y, sqrt of the sum of squares
__host__ __device__ __forceinline__ bool inlier(const Model& m, const double* __restrict__ x, const double* __restrict__ y,
                                       double threshold)
{
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    const double d0 = (((x0 * m.M[0] + x1 * m.M[1]) + x2 * m.M[2]) + m.t[0]) - y[0];
    const double d1 = (((x0 * m.M[3] + x1 * m.M[4]) + x2 * m.M[5]) + m.t[1]) - y[1];
    const double d2 = (((x0 * m.M[6] + x1 * m.M[7]) + x2 * m.M[8]) + m.t[2]) - y[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2) < threshold;
}

__global__ __launch_bounds__(BLOCK) void score_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                      int N, const int* __restrict__ samples, int H,
                                                      double threshold, int* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (h >= H) return;   // the whole wave
    Model m;
    const bool ok = sample_model(src, dst, N, samples + (size_t)h * 3, m);
    int cnt = 0;
    if (ok)
        for (int p = lane; p < N; p += 64) cnt += inlier(m, src + (size_t)p * 3, dst + (size_t)p * 3, threshold) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) counts[h] = ok ? cnt : -1;
}

// sum of every v[k] over the workgroup in a fixed order; every thread gets the sums
template <int K>
__device__ static void block_sum(double (&v)[K], double* sh)
{
    const int t = threadIdx.x;
    for (int k = 0; k < K; k++) sh[k * BLOCK + t] = v[k];
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int k = 0; k < K; k++) sh[k * BLOCK + t] += sh[k * BLOCK + t + w];
        __syncthreads();
    }
    for (int k = 0; k < K; k++) v[k] = sh[k * BLOCK];
    __syncthreads();
}

__host__ __device__ static void quaternion_of(const double* R, double* q)   // [x y z w], w >= 0 branch first
{
    const double tr = R[0] + R[4] + R[8];
    double x, y, z, w;
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
    }
    const double nrm = sqrt(x * x + y * y + z * z + w * w);
    q[0] = x / nrm; q[1] = y / nrm; q[2] = z / nrm; q[3] = w / nrm;
}

// Umeyama over the points with mask[p] != 0 (mask NULL: all), the whole
// workgroup.  Thread t owns the points t, t + 256, ...: it reads only mask
// bytes it wrote itself when the mask comes from this kernel.  Writes
// out_sim3 [8] (NaN when there is no fit); returns the code and the point
// count to thread 0's caller (uniform across the workgroup).
__device__ static int block_umeyama(const double* __restrict__ src, const double* __restrict__ dst, int N,
                                    const unsigned char* mask, double* __restrict__ out_sim3, Moments* ws, double* sh,
                                    long long* npoints)
{
    const int t = threadIdx.x;
    double s1[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int p = t; p < N; p += BLOCK) {
        if (mask && !mask[p]) continue;
        for (int r = 0; r < 3; r++) {
            s1[r] += src[(size_t)p * 3 + r];
            s1[3 + r] += dst[(size_t)p * 3 + r];
        }
        s1[6] += 1.0;
    }
    block_sum<7>(s1, sh);
    if (t == 0) {
        for (int r = 0; r < 3; r++) {
            ws->mx[r] = s1[r] / s1[6];
            ws->my[r] = s1[3 + r] / s1[6];
        }
        ws->n = (long long)s1[6];
    }
    __syncthreads();
    const long long n = ws->n;
    *npoints = n;
    int code = CODE_DEGENERATE_REFIT;
    Model m;
    if (n > 0) {   // uniform
        double mx[3], my[3];
        for (int r = 0; r < 3; r++) { mx[r] = ws->mx[r]; my[r] = ws->my[r]; }
        double s2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int p = t; p < N; p += BLOCK) {
            if (mask && !mask[p]) continue;
            for (int i = 0; i < 3; i++) {
                const double xi = src[(size_t)p * 3 + i] - mx[i];
                s2[9] += xi * xi;
                for (int j = 0; j < 3; j++) s2[j * 3 + i] += (dst[(size_t)p * 3 + j] - my[j]) * xi;
            }
        }
        block_sum<10>(s2, sh);
        for (int i = 0; i < 10; i++) s2[i] /= (double)n;
        if (umeyama_solve(mx, my, s2, s2[9], m)) code = CODE_OK;
    }
    if (t == 0) {
        if (code == CODE_OK) {
            for (int r = 0; r < 3; r++) out_sim3[r] = m.t[r];
            quaternion_of(m.R, out_sim3 + 3);
            out_sim3[7] = m.c;
        } else {
            for (int r = 0; r < 8; r++) out_sim3[r] = __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    return code;
}

__global__ __launch_bounds__(BLOCK) void select_refit_kernel(const double* __restrict__ src,
                                                             const double* __restrict__ dst, int N,
                                                             const int* __restrict__ samples, int H, double threshold,
                                                             int early_exit, const int* __restrict__ counts,
                                                             double* __restrict__ out_sim3,
                                                             unsigned char* __restrict__ out_mask,
                                                             int* __restrict__ out_info, Moments* ws)
{
    __shared__ double sh[10 * BLOCK];
    __shared__ int s_exit[BLOCK], s_cnt[BLOCK], s_arg[BLOCK];
    const int t = threadIdx.x;
    // the first hypothesis above early_exit; the first hypothesis with the largest count
    int first_exit = H, best = 0, arg = H;
    for (int h = t; h < H; h += BLOCK) {
        const int c = counts[h];
        if (early_exit >= 0 && c > early_exit && h < first_exit) first_exit = h;
        if (c > best) { best = c; arg = h; }   // ascending h: ties keep the earlier one
    }
    s_exit[t] = first_exit; s_cnt[t] = best; s_arg[t] = arg;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_exit[t] = min(s_exit[t], s_exit[t + w]);
            const int c = s_cnt[t + w], a = s_arg[t + w];
            if (c > s_cnt[t] || (c == s_cnt[t] && a < s_arg[t])) { s_cnt[t] = c; s_arg[t] = a; }
        }
        __syncthreads();
    }
    const int winner = s_exit[0] < H ? s_exit[0] : s_arg[0];
    if (winner >= H) {   // every sample invalid or degenerate (or without a single inlier)
        for (int p = t; p < N; p += BLOCK) out_mask[p] = 0;
        if (t < 8) out_sim3[t] = __longlong_as_double(0x7ff8000000000000ll);
        if (t == 0) { out_info[0] = CODE_NO_HYPOTHESIS; out_info[1] = -1; out_info[2] = 0; out_info[3] = 0; }
        return;
    }
    Model m;
    sample_model(src, dst, N, samples + (size_t)winner * 3, m);   // valid: its count is >= 1
    for (int p = t; p < N; p += BLOCK)
        out_mask[p] = inlier(m, src + (size_t)p * 3, dst + (size_t)p * 3, threshold) ? 1 : 0;
    __syncthreads();
    long long n = 0;
    const int code = block_umeyama(src, dst, N, out_mask, out_sim3, ws, sh, &n);
    if (t == 0) { out_info[0] = code; out_info[1] = winner; out_info[2] = counts[winner]; out_info[3] = (int)n; }
}

__global__ __launch_bounds__(BLOCK) void umeyama_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                        int N, const unsigned char* __restrict__ mask,
                                                        double* __restrict__ out_sim3, int* __restrict__ out_info,
                                                        Moments* ws)
{
    __shared__ double sh[10 * BLOCK];
    long long n = 0;
    const int code = block_umeyama(src, dst, N, mask, out_sim3, ws, sh, &n);
    if (threadIdx.x == 0) { out_info[0] = code; out_info[1] = -1; out_info[2] = 0; out_info[3] = (int)n; }
}

enum : int64_t { MAX_POINTS = 1 << 24, MAX_HYPOTHESES = 1 << 20 };

}  // namespace align
}  // namespace dpvo

using namespace dpvo;
using namespace dpvo::align;

extern "C" size_t dpvo_sim3_workspace_bytes(int64_t N, int64_t H)
{
    if (N < 3 || N > MAX_POINTS || H < 0 || H > MAX_HYPOTHESES) return 0;
    return (sizeof(Moments) + 255) & ~(size_t)255;
}

extern "C" int dpvo_sim3_ransac(const double* src, const double* dst, int64_t N, const int* samples, int64_t H,
                                double threshold, int early_exit, double* out_sim3, int* out_counts,
                                unsigned char* out_mask, int* out_info, void* workspace, size_t workspace_bytes,
                                void* stream)
{
    DPVO_CHECK_ARG(N >= 3 && N <= MAX_POINTS, "need 3 <= N <= 2^24 points");
    DPVO_CHECK_ARG(H >= 1 && H <= MAX_HYPOTHESES, "need 1 <= H <= 2^20 hypotheses");
    DPVO_CHECK_ARG(threshold > 0.0 && threshold <= DBL_MAX, "threshold must be finite and > 0");
    DPVO_CHECK_ARG(src && dst && samples, "src / dst / samples missing");
    DPVO_CHECK_ARG(out_sim3 && out_counts && out_mask && out_info, "outputs missing");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_sim3_workspace_bytes(N, H),
                   "workspace too small (dpvo_sim3_workspace_bytes)");
    DPVO_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((H + WAVES - 1) / WAVES)), dim3(BLOCK), 0, s, src, dst, (int)N,
                       samples, (int)H, threshold, out_counts);
    hipLaunchKernelGGL(select_refit_kernel, dim3(1), dim3(BLOCK), 0, s, src, dst, (int)N, samples, (int)H, threshold,
                       early_exit, out_counts, out_sim3, out_mask, out_info, (Moments*)workspace);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_sim3_umeyama(const double* src, const double* dst, int64_t N, const unsigned char* mask,
                                 double* out_sim3, int* out_info, void* workspace, size_t workspace_bytes,
                                 void* stream)
{
    DPVO_CHECK_ARG(N >= 3 && N <= MAX_POINTS, "need 3 <= N <= 2^24 points");
    DPVO_CHECK_ARG(src && dst, "src / dst missing");
    DPVO_CHECK_ARG(out_sim3 && out_info, "outputs missing");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_sim3_workspace_bytes(N, 0),
                   "workspace too small (dpvo_sim3_workspace_bytes)");
    DPVO_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    hipLaunchKernelGGL(umeyama_kernel, dim3(1), dim3(BLOCK), 0, as_stream(stream), src, dst, (int)N, mask, out_sim3,
                       out_info, (Moments*)workspace);
    DPVO_CHECK_LAUNCH();
    return 0;
}
