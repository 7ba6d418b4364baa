// fastba.hip -- sparse Gauss-Newton bundle adjustment over SE(3) poses and
// patch inverse depths, for gfx950.
//
// Replaces the reference's cuda_ba extension (dpvo/fastba/ba.cpp:236-241,
// ba_cuda.cu).  Same normal equations and update as ba_cuda.cu:214-540:
//   per edge (patch centre only): residual, mask, Jacobians Ji, Jj, Jz;
//   B (6N x 6N pose block), E (6N x Mu), C, v, u; Q = 1/(C + lmbda);
//   S = B - E Q E^T, y = v - E Q u, S += diag(1e-4 S + 1);
//   dX = chol_solve(S, y); dZ = Q (u - E^T dX); left retraction of the poses,
//   clamped additive update of the depths.
//
// MI355X structure (no host synchronisation inside the call):
//   mark    -- bitmap of the referenced patches                (grid over E)
//   scan    -- popcount prefix -> sorted unique ids kx, counts  (1 workgroup)
//   zero    -- clear the Mu-sized accumulators                  (grid)
//   per iteration:
//     hessian -- per edge; B and v reduced in LDS (ds_add_f32), flushed
//                once per workgroup; E/C/u with device atomics   (grid over E)
//     schur   -- E Q E^T and E Q u over patch chunks             (grid over Mu)
//     solve   -- Cholesky (fp64, LDS) + solve + pose retraction  (1 workgroup)
//     patch   -- dZ, depth retraction, re-zero accumulators      (grid over Mu)
// The unique-id inverse (the reference's torch::_unique, ba_cuda.cu:435) is
// recomputed per edge from the bitmap instead of being stored.
#include <algorithm>
#include <cfloat>
#include <stdlib.h>

#include <hipcub/hipcub.hpp>

#include <cstdlib>

#include "common.hpp"

#include <type_traits>

namespace dpvo {

// ---------------------------------------------------------------------------
// device SE3 helpers, float (restating ba_cuda.cu:18-156)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void actSO3(const float* q, const float* X, float* Y)
{
    float uv[3];
    uv[0] = 2.0f * (q[1] * X[2] - q[2] * X[1]);
    uv[1] = 2.0f * (q[2] * X[0] - q[0] * X[2]);
    uv[2] = 2.0f * (q[0] * X[1] - q[1] * X[0]);
    Y[0] = X[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    Y[1] = X[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    Y[2] = X[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}
__device__ __forceinline__ void actSE3(const float* t, const float* q, const float* X, float* Y)
{
    actSO3(q, X, Y);
    Y[3] = X[3];
    Y[0] += X[3] * t[0];
    Y[1] += X[3] * t[1];
    Y[2] += X[3] * t[2];
}
__device__ __forceinline__ void adjSE3(const float* t, const float* q, const float* X, float* Y)
{
    const float qinv[4] = {-q[0], -q[1], -q[2], q[3]};
    actSO3(qinv, &X[0], &Y[0]);
    actSO3(qinv, &X[3], &Y[3]);
    float u[3], v[3];
    u[0] = t[2] * X[1] - t[1] * X[2];
    u[1] = t[0] * X[2] - t[2] * X[0];
    u[2] = t[1] * X[0] - t[0] * X[1];
    actSO3(qinv, u, v);
    Y[3] += v[0];
    Y[4] += v[1];
    Y[5] += v[2];
}
__device__ __forceinline__ void relSE3(const float* ti, const float* qi, const float* tj, const float* qj,
                                       float* tij, float* qij)
{
    qij[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];
    qij[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
    qij[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
    qij[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
    actSO3(qij, ti, tij);
    tij[0] = tj[0] - tij[0];
    tij[1] = tj[1] - tij[1];
    tij[2] = tj[2] - tij[2];
}
__device__ __forceinline__ void expSO3(const float* phi, float* q)
{
    const float theta_sq = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    const float theta_p4 = theta_sq * theta_sq;
    const float theta = sqrtf(theta_sq);
    float imag, real;
    if (theta_sq < 1e-8f) {
        imag = 0.5f - (1.0f / 48.0f) * theta_sq + (1.0f / 3840.0f) * theta_p4;
        real = 1.0f - (1.0f / 8.0f) * theta_sq + (1.0f / 384.0f) * theta_p4;
    } else {
        imag = sinf(0.5f * theta) / theta;
        real = cosf(0.5f * theta);
    }
    q[0] = imag * phi[0];
    q[1] = imag * phi[1];
    q[2] = imag * phi[2];
    q[3] = real;
}
__device__ __forceinline__ void cross_inplace(const float* a, float* b)
{
    const float x0 = a[1] * b[2] - a[2] * b[1], x1 = a[2] * b[0] - a[0] * b[2], x2 = a[0] * b[1] - a[1] * b[0];
    b[0] = x0;
    b[1] = x1;
    b[2] = x2;
}
__device__ __forceinline__ void expSE3(const float* xi, float* t, float* q)
{
    expSO3(xi + 3, q);
    float tau[3] = {xi[0], xi[1], xi[2]};
    const float phi[3] = {xi[3], xi[4], xi[5]};
    const float theta_sq = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    const float theta = sqrtf(theta_sq);
    t[0] = tau[0];
    t[1] = tau[1];
    t[2] = tau[2];
    if (theta > 1e-4f) {
        const float a = (1.0f - cosf(theta)) / theta_sq;
        cross_inplace(phi, tau);
        t[0] += a * tau[0];
        t[1] += a * tau[1];
        t[2] += a * tau[2];
        const float b = (theta - sinf(theta)) / (theta * theta_sq);
        cross_inplace(phi, tau);
        t[0] += b * tau[0];
        t[1] += b * tau[1];
        t[2] += b * tau[2];
    }
}
__device__ __forceinline__ void retrSE3(const float* xi, const float* t, const float* q, float* t1, float* q1)
{
    float dt[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 1};
    expSE3(xi, dt, dq);
    q1[0] = dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1];
    q1[1] = dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2];
    q1[2] = dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0];
    q1[3] = dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2];
    actSO3(dq, t, t1);
    t1[0] += dt[0];
    t1[1] += dt[1];
    t1[2] += dt[2];
}

// ---------------------------------------------------------------------------
// workspace layout
// ---------------------------------------------------------------------------
constexpr int BA_LDS_NMAX = 12;  // optimised poses whose B fits in LDS (72x72 fp32)
constexpr int BA_SOLVE_NMAX = 64;  // up to 384 x 384 (fp64 Cholesky in global scratch beyond BA_LDS_NMAX)
constexpr int HDR_MU = 0, HDR_STATUS = 1, HDR_BW = 2, HDR_WORDS = 16;
constexpr int BS_TILE = 64;            // tile edge of the banded reduced camera system
constexpr int BS_NMAX = 32767;         // pose keys are packed as 16-bit pairs in the Schur reduction

struct BaLayout {
    size_t hdr, bits, wordbase, kx, B, v, C, u, E, S, y, dX, Sd, yd, Bpart, total;
    int nbH;   // Hessian workgroups (each leaves one partial B / v in Bpart)
    int64_t nwords, mu_max;
    int n6;
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static BaLayout ba_layout(int64_t E, int64_t num_patches, int N)
{
    BaLayout L{};
    L.nwords = (num_patches + 31) / 32;
    L.mu_max = E < num_patches ? E : num_patches;
    if (L.mu_max < 1) L.mu_max = 1;
    L.n6 = 6 * N;
    const size_t n6 = (size_t)(L.n6 > 0 ? L.n6 : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
    L.hdr = take(HDR_WORDS * 4);
    L.bits = take((size_t)L.nwords * 4);
    L.wordbase = take((size_t)L.nwords * 4);
    L.kx = take((size_t)L.mu_max * 4);
    L.B = take(n6 * n6 * 4);
    L.v = take(n6 * 4);
    L.C = take((size_t)L.mu_max * 4);
    L.u = take((size_t)L.mu_max * 4);
    L.E = take((size_t)L.mu_max * n6 * 4);
    L.S = take(n6 * n6 * 4);
    L.y = take(n6 * 4);
    L.dX = take(n6 * 4);
    // fp64 Cholesky scratch, only for systems too large for the LDS solver
    const bool big = L.n6 > 6 * 12;
    L.Sd = take(big ? n6 * (n6 + 1) * 8 : 8);
    L.yd = take(big ? n6 * 8 : 8);
    // per-workgroup partial B / v of the LDS Hessian path, reduced by ba_breduce_kernel
    L.nbH = (int)grid_for(E > 0 ? E : 1, 256, 1024);
    L.Bpart = take(N <= BA_LDS_NMAX ? (size_t)L.nbH * (n6 * n6 + n6) * 4 : 8);
    L.total = off;
    return L;
}

struct BaParams {
    float* poses;
    float* patches;
    const float* intrinsics;
    const float* target;
    const float* weight;
    const float* lmbda;
    const int64_t* ii;
    const int64_t* jj;
    const int64_t* kk;
    int64_t E, num_patches;
    int P, t0, N, n6;
    int* hdr;
    int* status;
    uint32_t* bits;
    int* wordbase;
    int* kx;
    float *B, *v, *C, *u, *Em, *S, *y, *dX;
    double* Sd;
    double* yd;
    int red_iters;   // wave reductions of the pose-block terms per wave (0 = per-lane atomics only)
    float* Bpart;    // [nbH][n6 * n6 + n6] per-workgroup partial B / v (LDS Hessian path)
    int nbH;
    // sparse (band) path only -- see "large pose windows" below
    float* ent;      // [E][16] per-edge Schur entries: E_i row (6), E_j row (6), C, u
    const int* kptr; // [Mu + 1] CSR of the edges of each unique patch (into eord)
    const int* eord; // [E] edge ids sorted by unique-patch rank
    float* Qk;       // [Mu] 1 / (C + lmbda)
    float* uk;       // [Mu]
    double* St;      // band tiles of the reduced camera system, lower triangle (fp64)
    double* ys;      // [T * 64] right-hand side, then the solution dX (fp64)
    int T, bt;       // 64-wide tiles per side, tile bandwidth
    // depth prior (dpvo_ba_forward_prior): nullptr = the plain call
    const float* est; // [num_patches][3][P][P], channel 2 at the centre pixel
    float mu;
};

__device__ __forceinline__ bool failed(const BaParams& p) { return *(volatile int*)p.status != 0; }

// Depth prior of the reference's Python BA (dpvo/ba.py:151-159): a patch with
// a prior inverse depth est adds mu to C and -mu (d - est) to u before
// Q = 1 / (C + lmbda) is formed.  Valid is 0 < est < +inf: the reference's
// est > 0 alone lets 1 / median(depth) = inf through, and the depth turns NaN.
__device__ __forceinline__ bool prior_valid(float est) { return est > 0.f && est < __builtin_inff(); }

// atomic dense path: the prior enters C / u once, as the value the
// accumulators of unique patch k start an iteration from (0 without a prior)
__device__ __forceinline__ void prior_seed(const BaParams& p, int64_t k, float& C0, float& u0)
{
    C0 = 0.f;
    u0 = 0.f;
    if (p.est == nullptr) return;
    const int64_t PP = (int64_t)p.P * p.P, at = ((int64_t)p.kx[k] * 3 + 2) * PP + (p.P / 2) * p.P + p.P / 2;
    const float est = p.est[at];
    if (prior_valid(est)) {
        C0 = p.mu;
        u0 = -p.mu * (p.patches[at] - est);
    }
}

// ---------------------------------------------------------------------------
// unique(kk): bitmap + popcount prefix
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ba_mark_kernel(BaParams p)
{
    // Consecutive edges mostly reference consecutive patches, so a wave's
    // lanes hit 1-3 bitmap words: OR-reduce per word across the wave and issue
    // one atomic per distinct word (same-address atomics serialise in L2).
    const int lane = threadIdx.x & 63;
    for (int64_t e0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~int64_t(63); e0 < p.E;
         e0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = e0 + lane;
        int64_t word = -1;
        uint32_t bit = 0;
        if (e < p.E) {
            const int64_t k = p.kk[e];
            if (k < 0 || k >= p.num_patches) {
                atomicExch(p.status, -1);  // patch index out of range
            } else {
                word = k >> 5;
                bit = 1u << (k & 31);
            }
        }
        uint64_t pending = __ballot(word >= 0);
        while (pending) {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int64_t lw = __shfl(word, leader);
            const bool mine = word == lw;
            uint32_t b = mine ? bit : 0u;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) b |= __shfl_xor(b, o);
            if (lane == leader) atomicOr(&p.bits[lw], b);
            pending &= ~__ballot(mine);
        }

    }
}

constexpr int SCAN_LDS_WORDS = 16384;   // 64 KB: the bitmap of up to 524,288 patches

__global__ __launch_bounds__(1024) void ba_scan_kernel(BaParams p, int64_t nwords)
{
    __shared__ int part[1024];
    __shared__ uint32_t sbits[SCAN_LDS_WORDS];
    const int tid = threadIdx.x;
    const int64_t per = (nwords + 1023) / 1024;
    const int64_t w0 = tid * per, w1 = min(nwords, w0 + per);
    // Each thread owns a contiguous run of words; reading them in place is a
    // chain of dependent-latency loads per thread, so the bitmap is first
    // staged through LDS with coalesced, independent loads.
    const bool staged = nwords <= SCAN_LDS_WORDS;
    if (staged) {
        for (int64_t w = tid; w < nwords; w += 1024) sbits[w] = p.bits[w];
        __syncthreads();
    }
    auto word = [&](int64_t w) { return staged ? sbits[w] : p.bits[w]; };
    int cnt = 0;
    for (int64_t w = w0; w < w1; w++) cnt += __popc(word(w));
    part[tid] = cnt;
    __syncthreads();
    // inclusive Hillis-Steele scan over 1024 partials
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int base = part[tid] - cnt;
    for (int64_t w = w0; w < w1; w++) {
        uint32_t m = word(w);
        p.wordbase[w] = base;
        while (m) {
            const int bit = __ffs(m) - 1;
            m &= m - 1;
            p.kx[base++] = (int)(w * 32 + bit);
        }
    }
    if (tid == 1023) p.hdr[HDR_MU] = part[1023];
}

__device__ __forceinline__ int unique_rank(const BaParams& p, int64_t k)
{
    const uint32_t w = p.bits[k >> 5];
    return p.wordbase[k >> 5] + __popc(w & ((1u << (k & 31)) - 1u));
}

// element (A, B), A >= B, of the banded lower-triangle tile storage: tile
// (r, c), 0 <= r - c <= bt, lives at index c * (bt + 1) + (r - c), row-major 64 x 64
__device__ __forceinline__ double* bs_tile(const BaParams& p, int r, int c)
{
    return p.St + (((int64_t)c * (p.bt + 1) + (r - c)) << 12);
}
__device__ __forceinline__ double* bs_elem(const BaParams& p, int A, int B)
{
    return bs_tile(p, A >> 6, B >> 6) + ((A & 63) << 6) + (B & 63);
}

__global__ __launch_bounds__(256) void ba_zero_kernel(BaParams p)
{
    const int Mu = p.hdr[HDR_MU];
    const int64_t nE = (int64_t)Mu * p.n6, nB = (int64_t)p.n6 * p.n6;
    const int64_t total = nE + (int64_t)Mu + nB + p.n6 + nB + p.n6;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t j = i;
        if (j < nE) { p.Em[j] = 0.f; continue; } j -= nE;
        if (j < Mu) {   // C and u of patch j together (the depth prior's seed, else 0)
            float C0, u0;
            prior_seed(p, j, C0, u0);
            p.C[j] = C0;
            p.u[j] = u0;
            continue;
        }
        j -= Mu;
        if (j < nB) { p.B[j] = 0.f; continue; } j -= nB;
        if (j < p.n6) { p.v[j] = 0.f; continue; } j -= p.n6;
        if (j < nB) { p.S[j] = 0.f; continue; } j -= nB;
        p.y[j] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// residuals + normal equations (ba_cuda.cu:214-365)
// ---------------------------------------------------------------------------
// SPARSE: the large-window path -- B goes straight into the band tiles of S,
// v into y, and the patch terms are stored per edge (no dense E).
template <bool LDS_B, bool SPARSE>
__global__ __launch_bounds__(256) void ba_hessian_kernel(BaParams p)
{
    extern __shared__ __attribute__((aligned(16))) float sB[];  // [n6*n6] B upper triangle + [n6] v
    const int n6 = p.n6;
    if (failed(p)) return;
    float* Bacc = LDS_B ? sB : p.B;
    float* vacc = LDS_B ? sB + n6 * n6 : p.v;
    // pose-block element (r, c), r <= c: upper triangle of the dense B, or
    // its mirror in the lower-triangle fp64 band tiles; v -> the fp64 y there
    auto bptr = [&](int r, int c) {
        if constexpr (SPARSE) return bs_elem(p, c, r);
        else return &Bacc[r * n6 + c];
    };
    auto vptr = [&](int r) {
        if constexpr (SPARSE) return p.ys + r;
        else return vacc + r;
    };
    if (LDS_B) {
        for (int i = threadIdx.x; i < n6 * n6 + n6; i += blockDim.x) sB[i] = 0.f;
        __syncthreads();
    }
    const float fx = p.intrinsics[0], fy = p.intrinsics[1], cx = p.intrinsics[2], cy = p.intrinsics[3];
    const int64_t PP = (int64_t)p.P * p.P, centre = (p.P / 2) * p.P + p.P / 2;

    const int lane = threadIdx.x & 63;
    // whole waves walk the edges together (the pose-block reduction below is per wave)
    for (int64_t n0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~int64_t(63); n0 < p.E;
         n0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = n0 + lane;
        const int64_t kxn = n < p.E ? p.kk[n] : -1;
        const bool valid = kxn >= 0 && kxn < p.num_patches;
        const int64_t ne = valid ? n : n0;                // a valid edge index for the (discarded) loads
        const int64_t kc = valid ? kxn : 0;
        const int k = unique_rank(p, kc);
        const int64_t i_abs = p.ii[ne], j_abs = p.jj[ne];
        const float* Pi = p.poses + i_abs * 7;
        const float* Pj = p.poses + j_abs * 7;
        const float ti[3] = {Pi[0], Pi[1], Pi[2]}, tj[3] = {Pj[0], Pj[1], Pj[2]};
        const float qi[4] = {Pi[3], Pi[4], Pi[5], Pi[6]}, qj[4] = {Pj[3], Pj[4], Pj[5], Pj[6]};
        const float* pa = p.patches + kc * 3 * PP + centre;
        float Xi[4], Xj[4], tij[3], qij[4];
        Xi[0] = (pa[0] - cx) / fx;
        Xi[1] = (pa[PP] - cy) / fy;
        Xi[2] = 1.0f;
        Xi[3] = pa[2 * PP];
        relSE3(ti, qi, tj, qj, tij, qij);
        actSE3(tij, qij, Xi, Xj);
        const float X = Xj[0], Y = Xj[1], Z = Xj[2], W = Xj[3];
        const float d = (Z >= 0.2f) ? 1.0f / Z : 0.0f;
        const float d2 = d * d;
        const float x1 = fx * (X / Z) + cx, y1 = fy * (Y / Z) + cy;
        const float rx = p.target[ne * 2 + 0] - x1, ry = p.target[ne * 2 + 1] - y1;
        const bool in_bounds = (sqrtf(rx * rx + ry * ry) < 128.f) && (Z > 0.2f) && (x1 > -64.f) && (y1 > -64.f) &&
                               (x1 < 2.f * cx + 64.f) && (y1 < 2.f * cy + 64.f);
        const float mask = (in_bounds && valid) ? 1.0f : 0.0f;
        const int ix = (int)(i_abs - p.t0), jx = (int)(j_abs - p.t0);
        const bool iv = valid && ix >= 0 && ix < p.N, jv = valid && jx >= 0 && jx < p.N;

        // both residual rows, summed per destination
        float Ji[2][6], Jj[2][6], Jz[2], w[2], r[2];
        w[0] = mask * p.weight[ne * 2 + 0];
        w[1] = mask * p.weight[ne * 2 + 1];
        r[0] = rx;
        r[1] = ry;
        Jz[0] = fx * (tij[0] * d - tij[2] * (X * d2));
        Jz[1] = fy * (tij[1] * d - tij[2] * (Y * d2));
        {
            const float a[6] = {fx * W * d, 0.f, fx * -X * W * d2, fx * -X * Y * d2, fx * (1.f + X * X * d2), fx * -Y * d};
            const float b[6] = {0.f, fy * W * d, fy * -Y * W * d2, fy * (-1.f - Y * Y * d2), fy * (X * Y * d2), fy * X * d};
#pragma unroll
            for (int t = 0; t < 6; t++) { Jj[0][t] = a[t]; Jj[1][t] = b[t]; }
        }
        adjSE3(tij, qij, Jj[0], Ji[0]);
        adjSE3(tij, qij, Jj[1], Ji[1]);

        // patch terms: E rows (device atomics; a wave's lanes mostly hold different patches), C, u
        if constexpr (SPARSE) {
            if (n < p.E) {
                float Ei[6], Ej[6], Ck = 0.f, uk = 0.f;
#pragma unroll
                for (int t = 0; t < 6; t++) { Ei[t] = 0.f; Ej[t] = 0.f; }
#pragma unroll
                for (int row = 0; row < 2; row++) {
#pragma unroll
                    for (int t = 0; t < 6; t++) {
                        Ei[t] += -w[row] * Jz[row] * Ji[row][t];
                        Ej[t] += w[row] * Jz[row] * Jj[row][t];
                    }
                    Ck += w[row] * Jz[row] * Jz[row];
                    uk += w[row] * r[row] * Jz[row];
                }
                const float z = 0.f;
                float4* o = reinterpret_cast<float4*>(p.ent + n * 16);
                o[0] = make_float4(iv ? Ei[0] : z, iv ? Ei[1] : z, iv ? Ei[2] : z, iv ? Ei[3] : z);
                o[1] = make_float4(iv ? Ei[4] : z, iv ? Ei[5] : z, jv ? Ej[0] : z, jv ? Ej[1] : z);
                o[2] = make_float4(jv ? Ej[2] : z, jv ? Ej[3] : z, jv ? Ej[4] : z, jv ? Ej[5] : z);
                o[3] = make_float4(valid ? Ck : z, valid ? uk : z, z, z);
            }
        } else if (valid) {
            float Ei[6], Ej[6], Ck = 0.f, uk = 0.f;
#pragma unroll
            for (int t = 0; t < 6; t++) { Ei[t] = 0.f; Ej[t] = 0.f; }
#pragma unroll
            for (int row = 0; row < 2; row++) {
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    Ei[t] += -w[row] * Jz[row] * Ji[row][t];
                    Ej[t] += w[row] * Jz[row] * Jj[row][t];
                }
                Ck += w[row] * Jz[row] * Jz[row];
                uk += w[row] * r[row] * Jz[row];
            }
            atomicAdd(&p.C[k], Ck);
            atomicAdd(&p.u[k], uk);
            float* Erow = p.Em + (int64_t)k * n6;
            if (iv) {
#pragma unroll
                for (int t = 0; t < 6; t++) atomicAdd(&Erow[6 * ix + t], Ei[t]);
            }
            if (jv) {
#pragma unroll
                for (int t = 0; t < 6; t++) atomicAdd(&Erow[6 * jx + t], Ej[t]);
            }
        }

        // pose terms: v_i, v_j and the B blocks (ii, jj upper triangles; ij off-diagonal,
        // stored once in the upper triangle; a self edge folds into ii).  Lanes with the
        // same (ix, jx) -- runs of consecutive edges share a frame pair -- are summed
        // across the wave first: one LDS / device atomic per value instead of 64.
        const bool self = iv && jv && ix == jx;
        const bool up = ix < jx;
        float vi[6], vj[6], bii[21], bjj[21], bij[36];
#pragma unroll
        for (int t = 0; t < 6; t++) {
            vi[t] = iv ? -w[0] * r[0] * Ji[0][t] - w[1] * r[1] * Ji[1][t] : 0.f;
            vj[t] = jv ? w[0] * r[0] * Jj[0][t] + w[1] * r[1] * Jj[1][t] : 0.f;
        }
        {
            int u = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++, u++) {
                    float sii = 0.f, sjj = 0.f;
                    if (self) {
#pragma unroll
                        for (int row = 0; row < 2; row++)
                            sii += w[row] * (Ji[row][a] * Ji[row][b] + Jj[row][a] * Jj[row][b] - Ji[row][a] * Jj[row][b] -
                                             Jj[row][a] * Ji[row][b]);
                    } else {
                        if (iv) sii = w[0] * Ji[0][a] * Ji[0][b] + w[1] * Ji[1][a] * Ji[1][b];
                        if (jv) sjj = w[0] * Jj[0][a] * Jj[0][b] + w[1] * Jj[1][a] * Jj[1][b];
                    }
                    bii[u] = sii;
                    bjj[u] = sjj;
                }
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) {
                float s = 0.f;
                if (iv && jv && !self)
                    s = up ? -(w[0] * Ji[0][a] * Jj[0][b] + w[1] * Ji[1][a] * Jj[1][b])
                           : -(w[0] * Jj[0][a] * Ji[0][b] + w[1] * Jj[1][a] * Ji[1][b]);
                bij[a * 6 + b] = s;
            }
        const bool has = iv || jv;
        // (ix, jx) < 2^15 (BS_NMAX); an index outside the window is not used, so it keys as 0x7fff
        const uint32_t key = has ? ((uint32_t)(iv ? ix : 0x7fff) << 17 | (uint32_t)(jv ? jx : 0x7fff) << 2 |
                                    (iv ? 2u : 0u) | (jv ? 1u : 0u))
                                 : 0xffffffffu;
        uint64_t pending = __ballot(has);
        for (int iter = 0; pending && iter < p.red_iters; iter++) {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const uint32_t lkey = __shfl(key, leader);
            const bool mine = key == lkey;
            const int lix = __shfl(ix, leader), ljx = __shfl(jx, leader);
            const bool liv = (lkey & 2) != 0, ljv = (lkey & 1) != 0;
            const bool lself = liv && ljv && lix == ljx;
            const bool lup = lix < ljx;
            auto red = [&](float v) { return wave64_sum(mine ? v : 0.f); };
            if (liv) {
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    const float s = red(vi[t]);
                    if (lane == leader) atomicAdd(vptr(6 * lix + t), s);
                }
                int u = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, u++) {
                        const float s = red(bii[u]);
                        if (lane == leader) atomicAdd(bptr(6 * lix + a, 6 * lix + b), s);
                    }
            }
            if (ljv) {
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    const float s = red(vj[t]);
                    if (lane == leader) atomicAdd(vptr(6 * ljx + t), s);
                }
            }
            if (ljv && !lself) {
                int u = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, u++) {
                        const float s = red(bjj[u]);
                        if (lane == leader) atomicAdd(bptr(6 * ljx + a, 6 * ljx + b), s);
                    }
            }
            if (liv && ljv && !lself) {
                const int r0 = lup ? lix : ljx, c0 = lup ? ljx : lix;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b < 6; b++) {
                        const float s = red(bij[a * 6 + b]);
                        if (lane == leader) atomicAdd(bptr(6 * r0 + a, 6 * c0 + b), s);
                    }
            }
            pending &= ~__ballot(mine);
        }
        // many distinct frame pairs in this wave (kk-major backward edges): plain
        // per-lane atomics for the lanes not reduced above
        if ((pending >> lane) & 1) {
            if (iv) {
#pragma unroll
                for (int t = 0; t < 6; t++) atomicAdd(vptr(6 * ix + t), vi[t]);
                int u = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, u++) atomicAdd(bptr(6 * ix + a, 6 * ix + b), bii[u]);
            }
            if (jv) {
#pragma unroll
                for (int t = 0; t < 6; t++) atomicAdd(vptr(6 * jx + t), vj[t]);
            }
            if (jv && !self) {
                int u = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, u++) atomicAdd(bptr(6 * jx + a, 6 * jx + b), bjj[u]);
            }
            if (iv && jv && !self) {
                const int r0 = up ? ix : jx, c0 = up ? jx : ix;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b < 6; b++) atomicAdd(bptr(6 * r0 + a, 6 * c0 + b), bij[a * 6 + b]);
            }
        }
    }
    if (LDS_B) {
        // one partial per workgroup, summed by ba_breduce_kernel: every workgroup
        // adding into the same ~3.7k floats is the slow case of float atomics
        // (MI355X_MICROARCH.md: every workgroup into one 2.3 KB row, 14x slower)
        __syncthreads();
        float* dst = p.Bpart + (int64_t)blockIdx.x * (n6 * n6 + n6);
        for (int i = threadIdx.x; i < n6 * n6 + n6; i += blockDim.x) dst[i] = sB[i];
    }
}

// B / v = sum of the Hessian workgroups' partials.  A workgroup owns 64
// consecutive entries; its 16 waves stride over the partials (coalesced
// 256-byte rows) and combine through LDS.  Fixed order: deterministic.
__global__ __launch_bounds__(1024) void ba_breduce_kernel(BaParams p)
{
    __shared__ float red[16][64];
    if (failed(p)) return;
    const int n6 = p.n6, ne = n6 * n6 + n6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (i < ne) {
#pragma unroll 8
        for (int b = wave; b < p.nbH; b += 16) s += p.Bpart[(int64_t)b * ne + i];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && i < ne) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; w++) t += red[w][lane];
        if (i < n6 * n6) p.B[i] = t;
        else p.v[i - n6 * n6] = t;
    }
}

// ---------------------------------------------------------------------------
// Schur complement terms: S_acc += Q_k e_k e_k^T (upper), y_acc += Q_k u_k e_k
// ---------------------------------------------------------------------------
constexpr int SCHUR_CHUNK = 64;


__device__ __forceinline__ int schur_chunk(int n6) { return n6 <= 96 ? SCHUR_CHUNK : 16; }
static inline size_t schur_lds_bytes(int n6)
{
    const int ch = n6 <= 96 ? SCHUR_CHUNK : 16;
    return ((size_t)2 * n6 * (ch + 4) + ch) * 4;
}

// The chunk's E rows are staged TRANSPOSED (pose coordinate major, patch
// minor, 4-float padded pitch), once as E Q and once as E, so an entry's
// k-sum runs over float4 LDS reads with independent accumulators per entry.
// (Patch-major staging made every k step a dependent ds_read_b32 round trip:
// 40 us per call, 65 % parked on s_waitcnt.)
__global__ __launch_bounds__(256) void ba_schur_kernel(BaParams p)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];  // sEQ [n6][pitch], sEt [n6][pitch], sU [ch]
    if (failed(p)) return;
    const int Mu = p.hdr[HDR_MU];
    const int n6 = p.n6;
    const int nup = n6 * (n6 + 1) / 2;
    const float lm = p.lmbda[0];
    const int ch = schur_chunk(n6), pitch = ch + 4;
    float* sEQ = sm;
    float* sEt = sm + n6 * pitch;
    float* sU = sm + 2 * n6 * pitch;
    for (int64_t k0 = (int64_t)blockIdx.x * ch; k0 < Mu; k0 += (int64_t)gridDim.x * ch) {
        const int cnt = (int)min((int64_t)ch, Mu - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < ch * n6; i += blockDim.x) {
            const int kk = i / n6, a = i - kk * n6;
            float e = 0.f, q = 0.f;
            if (kk < cnt) {
                e = p.Em[(k0 + kk) * n6 + a];
                q = 1.0f / (p.C[k0 + kk] + lm);
            }
            sEQ[a * pitch + kk] = e * q;
            sEt[a * pitch + kk] = e;
        }
        for (int kk = threadIdx.x; kk < ch; kk += blockDim.x) sU[kk] = kk < cnt ? p.u[k0 + kk] : 0.f;
        __syncthreads();
        // upper triangle of sum_k (E_ak Q_k) E_bk, i.e. the reference's matmul(E*Q, E^T)
        for (int idx = threadIdx.x; idx < nup; idx += blockDim.x) {
            // row a of the upper-triangle entry idx (row a holds n6 - a entries)
            const float t = (float)(2 * n6 + 1);
            int a = (int)((t - sqrtf(t * t - 8.f * (float)idx)) * 0.5f);
            a = max(0, min(a, n6 - 1));
            while (a > 0 && a * (2 * n6 - a + 1) / 2 > idx) a--;
            while ((a + 1) * (2 * n6 - a) / 2 <= idx) a++;
            const int b = a + (idx - a * (2 * n6 - a + 1) / 2);
            const float4* ea = reinterpret_cast<const float4*>(sEQ + a * pitch);
            const float4* eb = reinterpret_cast<const float4*>(sEt + b * pitch);
            float s0 = 0.f, s1 = 0.f;
            for (int q = 0; q < ch / 4; q++) {
                const float4 x = ea[q], y = eb[q];
                s0 += x.x * y.x + x.z * y.z;
                s1 += x.y * y.y + x.w * y.w;
            }
            const float s = s0 + s1;
            if (s != 0.f) atomicAdd(&p.S[a * n6 + b], s);
        }
        for (int a = threadIdx.x; a < n6; a += blockDim.x) {
            float s = 0.f;
            for (int kk = 0; kk < cnt; kk++) s += sEQ[a * pitch + kk] * sU[kk];
            if (s != 0.f) atomicAdd(&p.y[a], s);
        }
    }
}

// ---------------------------------------------------------------------------
// dense solve (fp64 Cholesky) + pose retraction; one workgroup
// ---------------------------------------------------------------------------
// retraction of the N optimised poses by dX (ba_cuda.cu:160-188) and reset of
// the pose accumulators; shared by both solve kernels
__device__ void ba_retract_and_reset(BaParams& p, const double* yv, int tid, int nthreads)
{
    const int n = p.n6;
    for (int i = tid; i < n; i += nthreads) p.dX[i] = (float)yv[i];
    for (int i = tid; i < p.N; i += nthreads) {
        float* P = p.poses + (int64_t)(p.t0 + i) * 7;
        const float t0v[3] = {P[0], P[1], P[2]}, q0v[4] = {P[3], P[4], P[5], P[6]};
        float xi[6], t1v[3], q1v[4];
        for (int k = 0; k < 6; k++) xi[k] = (float)yv[6 * i + k];
        retrSE3(xi, t0v, q0v, t1v, q1v);
        P[0] = t1v[0]; P[1] = t1v[1]; P[2] = t1v[2];
        P[3] = q1v[0]; P[4] = q1v[1]; P[5] = q1v[2]; P[6] = q1v[3];
    }
    for (int i = tid; i < n * n; i += nthreads) { p.B[i] = 0.f; p.S[i] = 0.f; }
    for (int i = tid; i < n; i += nthreads) { p.v[i] = 0.f; p.y[i] = 0.f; }
}

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double a_diag_lds(const double* L, int j) { return L[j * 65 + j]; }

__device__ __forceinline__ double readlane_d(double v, int lane)
{
    const int64_t u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffff), lane);
    const int hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
    return __longlong_as_double(((int64_t)hi << 32) | (uint32_t)lo);
}

// n6 <= 64: one wave, lane r holds row r of the system in registers (fully
// unrolled, compile-time column indices).  Column j of L is broadcast through
// LDS (one ds_write per lane, broadcast reads of the column): no readlane
// round trips and no per-element branches.  Right-looking Cholesky and
// forward / backward substitution in fp32 -- the precision of the reference,
// which factors the float32 S with torch::linalg::cholesky (ba_cuda.cu:518-521).
// A single wave has no partner to hide latency behind, so the short fp32
// sqrt / div chains (vs fp64) are what sets this kernel's time.  (Measured
// alternatives, both no faster: v_readlane broadcasts instead of LDS -- no
// waits, but ~14k instructions through one wave's issue slot; four waves with
// 4 x 4 register blocks -- two barriers per column cost what they save.)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64) void ba_solve_wave_kernel(BaParams p)
{
    typedef float RT;
    __shared__ RT col[64];
    __shared__ RT Lsh[64 * 65];
    __shared__ double yv[64];
    if (failed(p)) return;
    const int n = p.n6, r = threadIdx.x;
    RT a[64];
    // unconditional loads from clamped (valid) indices, then select: a load
    // under a per-element condition makes hipcc wait vmcnt(0) per element
    const int rc = r < n ? r : n - 1;
    float bv[64], sv[64];
#pragma unroll
    for (int c = 0; c < 64; c++) {
        const int cc = c < n ? c : n - 1;
        const int r0 = rc < cc ? rc : cc, c0 = rc < cc ? cc : rc;
        bv[c] = p.B[r0 * n + c0];
        sv[c] = p.S[r0 * n + c0];
    }
#pragma unroll
    for (int c = 0; c < 64; c++) {
        RT s = bv[c] - sv[c];
        if (r == c) s += (RT)1e-4 * s + (RT)1.0;
        a[c] = (r < n && c < n) ? s : (RT)0;
    }
    const float v_r = p.v[rc], y_r = p.y[rc];
    RT y = r < n ? (RT)(v_r - y_r) : (RT)0;
    int fail = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        if (j >= n || fail) break;
        col[r] = a[j];
        wave_lds_fence();
        const RT djj = col[j];
        if (!(djj > (RT)0)) {
            fail = j + 1;
            break;
        }
        const RT ljj = sqrt(djj);
        const RT l = r > j ? a[j] / ljj : (r == j ? ljj : (RT)0);
        a[j] = l;
        wave_lds_fence();
        col[r] = l;
        wave_lds_fence();
#pragma unroll
        for (int c = j + 1; c < 64; c++) a[c] -= l * col[c];   // rows r >= c kept (lower triangle)
        wave_lds_fence();
    }
    if (fail) {
        if (r == 0) atomicExch(p.status, fail);
        return;
    }
    // L to LDS (row r), then L z = y and L^T x = z with one broadcast per step
#pragma unroll
    for (int c = 0; c < 64; c++) Lsh[r * 65 + c] = a[c];
    wave_lds_fence();
    for (int j = 0; j < n; j++) {
        if (r == j) col[0] = y / Lsh[j * 65 + j];
        wave_lds_fence();
        const RT zj = col[0];
        if (r == j) y = zj;
        else if (r > j) y -= Lsh[r * 65 + j] * zj;
        wave_lds_fence();
    }
    for (int j = n - 1; j >= 0; j--) {
        if (r == j) col[0] = y / Lsh[j * 65 + j];
        wave_lds_fence();
        const RT xj = col[0];
        if (r == j) y = xj;
        else if (r < j) y -= Lsh[j * 65 + r] * xj;
        wave_lds_fence();
    }
    if (r < n) yv[r] = (double)y;
    wave_lds_fence();
    ba_retract_and_reset(p, yv, r, 64);
}

__global__ __launch_bounds__(256) void ba_solve_kernel(BaParams p)
{
    extern __shared__ __attribute__((aligned(16))) double sA[];  // [n6][n6+1] + [n6]
    __shared__ int s_fail;
    if (failed(p)) return;
    const int n = p.n6, ld = n + 1;
    const bool in_lds = n <= 6 * BA_LDS_NMAX;
    double* A = in_lds ? sA : p.Sd;
    double* yv = in_lds ? sA + n * ld : p.yd;
    const int tid = threadIdx.x;
    if (tid == 0) s_fail = 0;
    // S = B - E Q E^T (upper, mirrored), y = v - E Q u; damping S += diag(1e-4 S + 1)
    for (int i = tid; i < n * n; i += blockDim.x) {
        const int a = i / n, b = i - a * n;
        const int r0 = a < b ? a : b, c0 = a < b ? b : a;
        double s = (double)(p.B[r0 * n + c0] - p.S[r0 * n + c0]);
        if (a == b) s += 1e-4 * s + 1.0;
        A[a * ld + b] = s;
    }
    for (int i = tid; i < n; i += blockDim.x) yv[i] = (double)(p.v[i] - p.y[i]);
    __syncthreads();
    // right-looking Cholesky, lower triangle in place
    for (int j = 0; j < n; j++) {
        const double djj = A[j * ld + j];
        if (!(djj > 0.0)) {
            if (tid == 0) s_fail = j + 1;
            break;
        }
        const double ljj = sqrt(djj);
        __syncthreads();
        for (int i = j + 1 + tid; i < n; i += blockDim.x) A[i * ld + j] /= ljj;
        __syncthreads();
        if (tid == 0) A[j * ld + j] = ljj;
        const int m = n - j - 1;
        for (int t = tid; t < m * m; t += blockDim.x) {
            const int r = j + 1 + t / m, c = j + 1 + t % m;
            if (c <= r) A[r * ld + c] -= A[r * ld + j] * A[c * ld + j];
        }
        __syncthreads();
    }
    __syncthreads();
    if (s_fail) {
        if (tid == 0) atomicExch(p.status, s_fail);
        return;
    }
    // forward then backward substitution: L z = y, L^T x = z
    for (int j = 0; j < n; j++) {
        const double yj = yv[j] / A[j * ld + j];
        __syncthreads();
        if (tid == 0) yv[j] = yj;
        for (int i = j + 1 + tid; i < n; i += blockDim.x) yv[i] -= A[i * ld + j] * yj;
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; j--) {
        const double yj = yv[j] / A[j * ld + j];
        __syncthreads();
        if (tid == 0) yv[j] = yj;
        for (int i = tid; i < j; i += blockDim.x) yv[i] -= A[j * ld + i] * yj;
        __syncthreads();
    }
    __syncthreads();
    ba_retract_and_reset(p, yv, tid, blockDim.x);
}

// ---------------------------------------------------------------------------
// depth update (ba_cuda.cu:191-211, :523) and accumulator reset
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ba_patch_kernel(BaParams p, int structure_only, int reset)
{
    if (failed(p)) return;
    const int Mu = p.hdr[HDR_MU];
    const int n6 = p.n6;
    const float lm = p.lmbda[0];
    const int64_t PP = (int64_t)p.P * p.P;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < Mu; k += (int64_t)gridDim.x * blockDim.x) {
        const float Q = 1.0f / (p.C[k] + lm);
        float dZ;
        float* Erow = p.Em + k * n6;
        if (structure_only) {
            dZ = Q * p.u[k];
        } else {
            float s = 0.f;
            for (int a = 0; a < n6; a++) s += Erow[a] * p.dX[a];
            dZ = Q * (p.u[k] - s);
        }
        float* pd = p.patches + ((int64_t)p.kx[k] * 3 + 2) * PP;
        float d = pd[0] + dZ;
        d = (d > 20.f) ? 1.0f : d;
        d = fmaxf(d, 1e-4f);
        for (int64_t q = 0; q < PP; q++) pd[q] = d;
        if (reset) {
            float C0, u0;
            prior_seed(p, k, C0, u0);   // (reads the depth stored above)
            p.C[k] = C0;
            p.u[k] = u0;
            for (int a = 0; a < n6; a++) Erow[a] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Large pose windows: global BA (dpvo.py:436-505 calls fastba.BA with t0 = 1,
// t1 = n, i.e. thousands of poses).  The reference's dense E (6N x Mu: 77 GB
// at 4096 keyframes, past its int32 accessors) and dense E Q E^T GEMM are
// replaced by the same algebra on the graph's structure:
//   * per-edge Schur entries (E_i row, E_j row, C and u terms) instead of E,
//     with the edges of each unique patch found through a radix-sorted CSR;
//   * S = B - sum_k Q_k E_k E_k^T accumulated directly into 64 x 64 tiles of
//     its lower band -- the bandwidth is the widest pose span of one patch's
//     edges (19 poses for the reference's fixed global edge pattern) --
//     with keyed per-wave reductions ahead of the atomics;
//   * a tiled band Cholesky (one launch each of potrf / trsm / syrk per tile
//     column) and one-workgroup band triangular solves.
// fp32 throughout, like the reference's float S and cholesky (ba_cuda.cu:
// 510-523); only the summation order differs from the dense path.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bs_keys_kernel(BaParams p, uint32_t* keys, int* vals)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < p.E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = p.kk[e];
        keys[e] = (k >= 0 && k < p.num_patches) ? (uint32_t)unique_rank(p, k) : 0u;
        vals[e] = (int)e;
    }
}

// kptr[rank] = first sorted position of the rank (every rank has an edge)
__global__ __launch_bounds__(256) void bs_ptr_kernel(const uint32_t* keys, int64_t E, int* kptr)
{
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < E; s += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t key = keys[s];
        if (s == 0 || keys[s - 1] != key) kptr[key] = (int)s;
        if (s == E - 1) kptr[key + 1] = (int)E;
    }
}

// bandwidth of S in poses: the widest span of optimised poses one patch's edges touch
__global__ __launch_bounds__(256) void bs_span_kernel(BaParams p)
{
    const int Mu = p.hdr[HDR_MU];
    int best = 0;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < Mu; k += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0x7fffffff, hi = -1;
        for (int q = p.kptr[k]; q < p.kptr[k + 1]; q++) {
            const int e = p.eord[q];
            const int64_t a = p.ii[e] - p.t0, b = p.jj[e] - p.t0;
            if (a >= 0 && a < p.N) { lo = min(lo, (int)a); hi = max(hi, (int)a); }
            if (b >= 0 && b < p.N) { lo = min(lo, (int)b); hi = max(hi, (int)b); }
        }
        if (hi > lo) best = max(best, hi - lo);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(&p.hdr[HDR_BW], best);
}

__global__ __launch_bounds__(256) void bs_zero_kernel(BaParams p)
{
    const int64_t nS = (int64_t)p.T * (p.bt + 1) * (BS_TILE * BS_TILE / 2), ny = (int64_t)p.T * (BS_TILE / 2);
    const double2 z = make_double2(0.0, 0.0);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nS + ny; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nS) reinterpret_cast<double2*>(p.St)[i] = z;
        else reinterpret_cast<double2*>(p.ys)[i - nS] = z;
    }
}

// Per unique patch k (one lane each; consecutive patches share their pose
// structure, so a wave's lanes mostly hold the same pose pairs):
//   Q_k = 1 / (C_k + lmbda);  y -= Q_k u_k E_k;  S -= Q_k E_k E_k^T.
// E_k's entries are the host row summed over the patch's edges (when they
// share ii, as DPVO's do) plus one E_j row per edge; the pair products are
// accumulated without merging equal poses (the sum is the same).
__global__ __launch_bounds__(256) void bs_schur_kernel(BaParams p)
{
    if (failed(p)) return;
    const int Mu = p.hdr[HDR_MU];
    const float lm = p.lmbda[0];
    const int lane = threadIdx.x & 63;
    for (int64_t k0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) & ~int64_t(63); k0 < Mu;
         k0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = k0 + lane;
        const bool live = k < Mu;
        const int s0 = live ? p.kptr[k] : 0, s1 = live ? p.kptr[k + 1] : 0;
        const int64_t hpose = live ? p.ii[p.eord[s0]] : 0;
        float C = 0.f, u = 0.f, H[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool uniform = true;
        for (int q = s0; q < s1; q++) {
            const int e = p.eord[q];
            const float4* en = reinterpret_cast<const float4*>(p.ent + (int64_t)e * 16);
            const float4 a = en[0], b = en[1], d = en[3];
            H[0] += a.x; H[1] += a.y; H[2] += a.z; H[3] += a.w; H[4] += b.x; H[5] += b.y;
            C += d.x;
            u += d.y;
            uniform = uniform && p.ii[e] == hpose;
        }
        if (p.est != nullptr && live) {   // depth prior, before Q, Qk and uk are formed
            const int64_t PP = (int64_t)p.P * p.P, at = ((int64_t)p.kx[k] * 3 + 2) * PP + (p.P / 2) * p.P + p.P / 2;
            const float est = p.est[at];
            if (prior_valid(est)) {
                C += p.mu;
                u -= p.mu * (p.patches[at] - est);
            }
        }
        const float Q = 1.0f / (C + lm);
        if (live) {
            p.Qk[k] = Q;
            p.uk[k] = u;
        }
        const int deg = s1 - s0;
        const int nent = live ? (uniform ? 1 + deg : 2 * deg) : 0;
        // entry t -> (window pose or -1, row)
        auto entry = [&](int t, float* v) -> int {
            int64_t pose;
            if (uniform && t == 0) {
#pragma unroll
                for (int x = 0; x < 6; x++) v[x] = H[x];
                pose = hpose;
            } else {
                const int q = uniform ? t - 1 : (t >> 1);
                const bool jside = uniform || (t & 1);
                const int e = p.eord[s0 + q];
                const float* src = p.ent + (int64_t)e * 16 + (jside ? 6 : 0);
#pragma unroll
                for (int x = 0; x < 6; x++) v[x] = src[x];
                pose = jside ? p.jj[e] : p.ii[e];
            }
            pose -= p.t0;
            return (pose >= 0 && pose < p.N) ? (int)pose : -1;
        };
        int maxn = nent, maxp = nent * (nent + 1) / 2;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            maxn = max(maxn, __shfl_xor(maxn, o));
            maxp = max(maxp, __shfl_xor(maxp, o));
        }
        // y -= Q u E_k, one entry per lane per round
        const float qu = Q * u;
        for (int t = 0; t < maxn; t++) {
            float ev[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int pose = t < nent ? entry(t, ev) : -1;
            uint64_t pending = __ballot(pose >= 0);
            while (pending) {
                const int leader = __ffsll((unsigned long long)pending) - 1;
                const int lpose = __shfl(pose, leader);
                const bool mine = pose == lpose;
#pragma unroll
                for (int x = 0; x < 6; x++) {
                    const float s = wave64_sum(mine ? qu * ev[x] : 0.f);
                    if (lane == leader) atomicAdd(&p.ys[6 * lpose + x], -(double)s);
                }
                pending &= ~__ballot(mine);
            }
        }
        // S -= Q E_k E_k^T over entry pairs ta <= tb, one pair per lane per round
        int ta = 0, tb = 0;
        for (int it = 0; it < maxp; it++) {
            float ea[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, eb[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int pa = -1, pb = -1;
            if (ta < nent) {
                pa = entry(ta, ea);
                pb = entry(tb, eb);
            }
            uint32_t key = 0xffffffffu;
            if (pa >= 0 && pb >= 0) {
                if (pa < pb) {
                    const int t = pa; pa = pb; pb = t;
#pragma unroll
                    for (int x = 0; x < 6; x++) { const float v = ea[x]; ea[x] = eb[x]; eb[x] = v; }
                }
                key = (uint32_t)pa << 16 | (uint32_t)pb;
            }
            const bool same = ta == tb;
            uint64_t pending = __ballot(key != 0xffffffffu);
            while (pending) {
                const int leader = __ffsll((unsigned long long)pending) - 1;
                const uint32_t lkey = __shfl(key, leader);
                const bool mine = key == lkey;
                const int hi = (int)(lkey >> 16), lo = (int)(lkey & 0xffff);
                if (hi != lo) {
#pragma unroll
                    for (int x = 0; x < 6; x++)
#pragma unroll
                        for (int z = 0; z < 6; z++) {
                            const float s = wave64_sum(mine ? -Q * ea[x] * eb[z] : 0.f);
                            if (lane == leader) atomicAdd(bs_elem(p, 6 * hi + x, 6 * lo + z), (double)s);
                        }
                } else {
#pragma unroll
                    for (int x = 0; x < 6; x++)
#pragma unroll
                        for (int z = 0; z <= x; z++) {
                            const float v = same ? ea[x] * ea[z] : ea[x] * eb[z] + eb[x] * ea[z];
                            const float s = wave64_sum(mine ? -Q * v : 0.f);
                            if (lane == leader) atomicAdd(bs_elem(p, 6 * hi + x, 6 * hi + z), (double)s);
                        }
                }
                pending &= ~__ballot(mine);
            }
            if (ta < nent && ++tb == nent) {
                ta++;
                tb = ta;
            }
        }
    }
}

// S += diag(1e-4 S + 1) (ba_cuda.cu:517-518); identity on the padding past 6N
__global__ __launch_bounds__(256) void bs_damp_kernel(BaParams p)
{
    if (failed(p)) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.T * BS_TILE; i += gridDim.x * blockDim.x) {
        double* d = bs_elem(p, i, i);
        *d = i < p.n6 ? *d + (1e-4 * *d + 1.0) : 1.0;
    }
}

// Cholesky of diagonal tile c, one wave: lane r holds row r, column j of L is
// broadcast through LDS (as ba_solve_wave_kernel).  Upper entries written 0.
__global__ __launch_bounds__(64) void bs_potrf_kernel(BaParams p, int c)
{
    __shared__ double col[64];
    if (failed(p)) return;
    const int r = threadIdx.x;
    double* A = bs_tile(p, c, c) + r * 64;
    double a[64];
#pragma unroll
    for (int j = 0; j < 64; j += 2) {
        const double2 v = *reinterpret_cast<const double2*>(A + j);
        a[j] = v.x; a[j + 1] = v.y;
    }
    int fail = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        col[r] = a[j];
        wave_lds_fence();
        const double djj = col[j];
        if (!(djj > 0.0)) {
            fail = j + 1;
            break;
        }
        const double ljj = sqrt(djj);
        const double l = r > j ? a[j] / ljj : (r == j ? ljj : 0.0);
        a[j] = l;
        wave_lds_fence();
        col[r] = l;
        wave_lds_fence();
#pragma unroll
        for (int cc = j + 1; cc < 64; cc++) a[cc] -= l * col[cc];
        wave_lds_fence();
    }
    if (fail) {
        if (r == 0) atomicExch(p.status, c * BS_TILE + fail);
        return;
    }
#pragma unroll
    for (int j = 0; j < 64; j += 2)
        *reinterpret_cast<double2*>(A + j) = make_double2(j <= r ? a[j] : 0.0, j + 1 <= r ? a[j + 1] : 0.0);
}

// panel: A_rc <- A_rc L_cc^{-T} for r = c + 1 + blockIdx.x; lane i solves row i
__global__ __launch_bounds__(64) void bs_trsm_kernel(BaParams p, int c)
{
    __shared__ double Ls[64 * 65];
    if (failed(p)) return;
    const int r = c + 1 + blockIdx.x, i = threadIdx.x;
    const double* L = bs_tile(p, c, c);
    for (int q = i; q < 4096; q += 64) Ls[(q >> 6) * 65 + (q & 63)] = L[q];
    double* A = bs_tile(p, r, c) + i * 64;
    double x[64];
#pragma unroll
    for (int j = 0; j < 64; j += 2) {
        const double2 v = *reinterpret_cast<const double2*>(A + j);
        x[j] = v.x; x[j + 1] = v.y;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 64; j++) {
        x[j] = x[j] / Ls[j * 65 + j];
#pragma unroll
        for (int t = j + 1; t < 64; t++) x[t] -= x[j] * Ls[t * 65 + j];
    }
#pragma unroll
    for (int j = 0; j < 64; j += 2) *reinterpret_cast<double2*>(A + j) = make_double2(x[j], x[j + 1]);
}

// trailing update inside the band: A_rq -= A_rc A_qc^T for c < q <= r <= c + nb
__global__ __launch_bounds__(256) void bs_syrk_kernel(BaParams p, int c)
{
    __shared__ double Xs[64 * 65], Ys[64 * 65];
    if (failed(p)) return;
    const int idx = blockIdx.x;
    int i = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= idx) i++;
    while (i * (i + 1) / 2 > idx) i--;
    const int k = idx - i * (i + 1) / 2;
    const int r = c + 1 + i, q = c + 1 + k;
    const double* X = bs_tile(p, r, c);
    const double* Y = bs_tile(p, q, c);
    for (int t = threadIdx.x; t < 4096; t += 256) {
        Xs[(t >> 6) * 65 + (t & 63)] = X[t];
        Ys[(t >> 6) * 65 + (t & 63)] = Y[t];
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4] = {};
#pragma unroll 4
    for (int t = 0; t < 64; t++) {
        double xa[4], yb[4];
#pragma unroll
        for (int a = 0; a < 4; a++) xa[a] = Xs[(ty * 4 + a) * 65 + t];
#pragma unroll
        for (int b = 0; b < 4; b++) yb[b] = Ys[(tx * 4 + b) * 65 + t];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) acc[a][b] += xa[a] * yb[b];
    }
    double* O = bs_tile(p, r, q);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double2* o = reinterpret_cast<double2*>(O + (ty * 4 + a) * 64 + tx * 4);
        double2 v0 = o[0], v1 = o[1];
        v0.x -= acc[a][0]; v0.y -= acc[a][1]; v1.x -= acc[a][2]; v1.y -= acc[a][3];
        o[0] = v0;
        o[1] = v1;
    }
}

// L L^T x = y in place on ys, band-aware forward / backward substitution (one workgroup)
__global__ __launch_bounds__(256) void bs_trsv_kernel(BaParams p)
{
    __shared__ double Ls[64 * 65];
    __shared__ double zs[64];
    __shared__ double part[256];
    if (failed(p)) return;
    const int tid = threadIdx.x, T = p.T, bt = p.bt;
    double* y = p.ys;
    for (int c = 0; c < T; c++) {
        const double* Lcc = bs_tile(p, c, c);
        for (int q = tid; q < 4096; q += 256) Ls[(q >> 6) * 65 + (q & 63)] = Lcc[q];
        __syncthreads();
        if (tid < 64) {
            double yi = y[c * 64 + tid];
            for (int j = 0; j < 64; j++) {
                const double zj = __shfl(yi / Ls[j * 65 + j], j);
                if (tid == j) yi = zj;
                else if (tid > j) yi -= Ls[tid * 65 + j] * zj;
            }
            zs[tid] = yi;
            y[c * 64 + tid] = yi;
        }
        __syncthreads();
        const int rows = (min(T - 1, c + bt) - c) * 64;
        for (int q = tid; q < rows; q += 256) {
            const int r = c + 1 + (q >> 6), a = q & 63;
            const double* Lrc = bs_tile(p, r, c) + a * 64;
            double s = 0.0;
            for (int t = 0; t < 64; t++) s += Lrc[t] * zs[t];
            y[r * 64 + a] -= s;
        }
        __syncthreads();
    }
    for (int c = T - 1; c >= 0; c--) {
        const int rows = (min(T - 1, c + bt) - c) * 64;
        const int t = tid & 63;
        double s = 0.0;
        for (int q = tid >> 6; q < rows; q += 4) {
            const int r = c + 1 + (q >> 6), a = q & 63;
            s += bs_tile(p, r, c)[a * 64 + t] * y[r * 64 + a];
        }
        part[tid] = s;
        const double* Lcc = bs_tile(p, c, c);
        for (int q = tid; q < 4096; q += 256) Ls[(q >> 6) * 65 + (q & 63)] = Lcc[q];
        __syncthreads();
        if (tid < 64) {
            double xi = y[c * 64 + tid] - (part[tid] + part[tid + 64] + part[tid + 128] + part[tid + 192]);
            for (int j = 63; j >= 0; j--) {
                const double xj = __shfl(xi / Ls[j * 65 + j], j);
                if (tid == j) xi = xj;
                else if (tid < j) xi -= Ls[j * 65 + tid] * xj;
            }
            y[c * 64 + tid] = xi;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void bs_retract_kernel(BaParams p)
{
    if (failed(p)) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.N; i += gridDim.x * blockDim.x) {
        float* P = p.poses + (int64_t)(p.t0 + i) * 7;
        const float t0v[3] = {P[0], P[1], P[2]}, q0v[4] = {P[3], P[4], P[5], P[6]};
        float xi[6], t1v[3], q1v[4];
        for (int k = 0; k < 6; k++) xi[k] = (float)p.ys[6 * i + k];
        retrSE3(xi, t0v, q0v, t1v, q1v);
        P[0] = t1v[0]; P[1] = t1v[1]; P[2] = t1v[2];
        P[3] = q1v[0]; P[4] = q1v[1]; P[5] = q1v[2]; P[6] = q1v[3];
    }
}

// dZ_k = Q_k (u_k - E_k^T dX) over the patch's edge entries; depth retraction (ba_cuda.cu:191-211)
__global__ __launch_bounds__(256) void bs_patch_kernel(BaParams p)
{
    if (failed(p)) return;
    const int Mu = p.hdr[HDR_MU];
    const int64_t PP = (int64_t)p.P * p.P;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < Mu; k += (int64_t)gridDim.x * blockDim.x) {
        // the reference rounds dX to float before E^T dX (ba_cuda.cu:523)
        float s = 0.f;
        for (int q = p.kptr[k]; q < p.kptr[k + 1]; q++) {
            const int e = p.eord[q];
            const float* en = p.ent + (int64_t)e * 16;
            const int64_t a = p.ii[e] - p.t0, b = p.jj[e] - p.t0;
            if (a >= 0 && a < p.N)
                for (int t = 0; t < 6; t++) s += en[t] * (float)p.ys[6 * a + t];
            if (b >= 0 && b < p.N)
                for (int t = 0; t < 6; t++) s += en[6 + t] * (float)p.ys[6 * b + t];
        }
        const float dZ = p.Qk[k] * (p.uk[k] - s);
        float* pd = p.patches + ((int64_t)p.kx[k] * 3 + 2) * PP;
        float d = pd[0] + dZ;
        d = (d > 20.f) ? 1.0f : d;
        d = fmaxf(d, 1e-4f);
        for (int64_t q = 0; q < PP; q++) pd[q] = d;
    }
}

struct BsLayout {
    size_t hdr, bits, wordbase, kx, kin, kout, vin, vout, tmp, tmp_bytes, kptr, ent, Qk, uk, y, St, total;
    int64_t nwords, mu_max;
    int n6, T;
};

static size_t bs_sort_temp_bytes(int64_t E)
{
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr,
                                             (int*)nullptr, (int)E);
    return bytes;
}

static BsLayout bs_layout(int64_t E, int64_t num_patches, int N)
{
    BsLayout L{};
    L.nwords = (num_patches + 31) / 32;
    L.mu_max = std::max<int64_t>(1, std::min(E, num_patches));
    L.n6 = 6 * N;
    L.T = std::max(1, (L.n6 + BS_TILE - 1) / BS_TILE);
    const size_t e = (size_t)std::max<int64_t>(E, 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
    L.hdr = take(HDR_WORDS * 4);
    L.bits = take((size_t)L.nwords * 4);
    L.wordbase = take((size_t)L.nwords * 4);
    L.kx = take((size_t)L.mu_max * 4);
    L.kin = take(e * 4);
    L.kout = take(e * 4);
    L.vin = take(e * 4);
    L.vout = take(e * 4);
    L.tmp_bytes = bs_sort_temp_bytes((int64_t)e);
    L.tmp = take(L.tmp_bytes);
    L.kptr = take((size_t)(L.mu_max + 1) * 4);
    L.ent = take(e * 64);
    L.Qk = take((size_t)L.mu_max * 4);
    L.uk = take((size_t)L.mu_max * 4);
    L.y = take((size_t)L.T * BS_TILE * 8);
    L.St = take((size_t)L.T * L.T * BS_TILE * BS_TILE * 8);   // the band can be the whole matrix
    L.total = off;
    return L;
}

// one call of the sparse path; p carries the operands, status and sizes
static int ba_forward_sparse(BaParams p, char* ws, const BsLayout& L, int iterations, hipStream_t s)
{
    p.hdr = (int*)(ws + L.hdr);
    if (!p.status) p.status = p.hdr + HDR_STATUS;
    p.bits = (uint32_t*)(ws + L.bits);
    p.wordbase = (int*)(ws + L.wordbase);
    p.kx = (int*)(ws + L.kx);
    int* kptr = (int*)(ws + L.kptr);
    p.kptr = kptr;
    p.eord = (const int*)(ws + L.vout);
    p.ent = (float*)(ws + L.ent);
    p.Qk = (float*)(ws + L.Qk);
    p.uk = (float*)(ws + L.uk);
    p.ys = (double*)(ws + L.y);
    p.St = (double*)(ws + L.St);
    p.T = L.T;
    p.red_iters = 2;
    DPVO_CHECK_HIP(hipMemsetAsync(ws + L.hdr, 0, L.wordbase - L.hdr, s));  // header + bitmap
    DPVO_CHECK_HIP(hipMemsetAsync(p.status, 0, sizeof(int), s));
    const unsigned gE = grid_for(p.E, 256, 2048);
    const unsigned gM = grid_for(L.mu_max, 256, 2048);
    hipLaunchKernelGGL(ba_mark_kernel, dim3(gE), dim3(256), 0, s, p);
    hipLaunchKernelGGL(ba_scan_kernel, dim3(1), dim3(1024), 0, s, p, L.nwords);
    hipLaunchKernelGGL(bs_keys_kernel, dim3(gE), dim3(256), 0, s, p, (uint32_t*)(ws + L.kin), (int*)(ws + L.vin));
    DPVO_CHECK_LAUNCH();
    int bits = 1;
    while (bits < 32 && (int64_t(1) << bits) < L.mu_max) bits++;
    size_t tmp_bytes = L.tmp_bytes;
    DPVO_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + L.tmp, tmp_bytes, (uint32_t*)(ws + L.kin),
                                                      (uint32_t*)(ws + L.kout), (int*)(ws + L.vin),
                                                      (int*)(ws + L.vout), (int)p.E, 0, bits, s));
    hipLaunchKernelGGL(bs_ptr_kernel, dim3(gE), dim3(256), 0, s, (const uint32_t*)(ws + L.kout), p.E, kptr);
    hipLaunchKernelGGL(bs_span_kernel, dim3(gM), dim3(256), 0, s, p);
    DPVO_CHECK_LAUNCH();
    // the band decides the factorisation's launch shapes: one host read per call
    int hdr[HDR_WORDS], st = 0;
    DPVO_CHECK_HIP(hipMemcpyAsync(hdr, p.hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
    DPVO_CHECK_HIP(hipMemcpyAsync(&st, p.status, sizeof st, hipMemcpyDeviceToHost, s));
    DPVO_CHECK_HIP(hipStreamSynchronize(s));
    if (st != 0) return 0;   // bad patch index: reported through status, state untouched
    const int bw = hdr[HDR_BW];
    p.bt = std::min(L.T - 1, (6 * bw + 5 + BS_TILE - 1) / BS_TILE);
    const unsigned gH = grid_for(p.E, 256, 1024);
    const unsigned gZ = grid_for((int64_t)L.T * (p.bt + 1) * (BS_TILE * BS_TILE / 2), 256, 8192);
    for (int it = 0; it < iterations; it++) {
        hipLaunchKernelGGL(bs_zero_kernel, dim3(gZ), dim3(256), 0, s, p);
        hipLaunchKernelGGL((ba_hessian_kernel<false, true>), dim3(gH), dim3(256), 0, s, p);
        hipLaunchKernelGGL(bs_schur_kernel, dim3(gM), dim3(256), 0, s, p);
        hipLaunchKernelGGL(bs_damp_kernel, dim3(grid_for((int64_t)L.T * BS_TILE, 256, 1024)), dim3(256), 0, s, p);
        DPVO_CHECK_LAUNCH();
        for (int c = 0; c < L.T; c++) {
            hipLaunchKernelGGL(bs_potrf_kernel, dim3(1), dim3(64), 0, s, p, c);
            const int nb = std::min(p.bt, L.T - 1 - c);
            if (nb > 0) {
                hipLaunchKernelGGL(bs_trsm_kernel, dim3(nb), dim3(64), 0, s, p, c);
                hipLaunchKernelGGL(bs_syrk_kernel, dim3(nb * (nb + 1) / 2), dim3(256), 0, s, p, c);
            }
        }
        DPVO_CHECK_LAUNCH();
        hipLaunchKernelGGL(bs_trsv_kernel, dim3(1), dim3(256), 0, s, p);
        hipLaunchKernelGGL(bs_retract_kernel, dim3(grid_for(p.N, 256)), dim3(256), 0, s, p);
        hipLaunchKernelGGL(bs_patch_kernel, dim3(gM), dim3(256), 0, s, p);
        DPVO_CHECK_LAUNCH();
    }
    return 0;
}

// ---------------------------------------------------------------------------
// fastba.reproject (ba_cuda.cu:368-418)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reproject_kernel(const float* poses, const float* patches, int P,
                                                       const float* intrinsics, const int64_t* ii, const int64_t* jj,
                                                       const int64_t* kk, int64_t E, float* coords)
{
    const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
    const int64_t PP = (int64_t)P * P;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < E; n += (int64_t)gridDim.x * blockDim.x) {
        const float* Pi = poses + ii[n] * 7;
        const float* Pj = poses + jj[n] * 7;
        const float ti[3] = {Pi[0], Pi[1], Pi[2]}, tj[3] = {Pj[0], Pj[1], Pj[2]};
        const float qi[4] = {Pi[3], Pi[4], Pi[5], Pi[6]}, qj[4] = {Pj[3], Pj[4], Pj[5], Pj[6]};
        float tij[3], qij[4], Xi[4], Xj[4];
        relSE3(ti, qi, tj, qj, tij, qij);
        const float* pa = patches + kk[n] * 3 * PP;
        for (int64_t q = 0; q < PP; q++) {
            Xi[0] = (pa[q] - cx) / fx;
            Xi[1] = (pa[PP + q] - cy) / fy;
            Xi[2] = 1.0f;
            Xi[3] = pa[2 * PP + q];
            actSE3(tij, qij, Xi, Xj);
            coords[(n * 2 + 0) * PP + q] = fx * (Xj[0] / Xj[2]) + cx;
            coords[(n * 2 + 1) * PP + q] = fy * (Xj[1] / Xj[2]) + cy;
        }
    }
}

// ---------------------------------------------------------------------------
// neighbors on the device: stable sort by (ii, jj, edge), then prev/next
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nb_keys_kernel(const int64_t* ii, const int64_t* jj, int64_t E, uint64_t* keys,
                                                     int* vals)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        // order-preserving map of signed 32-bit values to unsigned
        const uint32_t hi = (uint32_t)(int32_t)ii[e] ^ 0x80000000u, lo = (uint32_t)(int32_t)jj[e] ^ 0x80000000u;
        keys[e] = ((uint64_t)hi << 32) | lo;
        vals[e] = (int)e;
    }
}

__global__ __launch_bounds__(256) void nb_link_kernel(const uint64_t* keys, const int* vals, int64_t E, int64_t* ix,
                                                     int64_t* jx)
{
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < E; s += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t g = (uint32_t)(keys[s] >> 32);
        const bool first = s == 0 || (uint32_t)(keys[s - 1] >> 32) != g;
        const bool last = s == E - 1 || (uint32_t)(keys[s + 1] >> 32) != g;
        const int e = vals[s];
        ix[e] = first ? -1 : vals[s - 1];
        jx[e] = last ? -1 : vals[s + 1];
    }
}

static size_t nb_sort_temp_bytes(int64_t E)
{
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int*)nullptr,
                                       (int*)nullptr, (int)E);
    return bytes;
}

// ---------------------------------------------------------------------------
// Deterministic dense path: DPVO's sliding window (N <= 12 optimised poses).
//
// One wave per unique patch (the groups of the kk group-by CSR, members in
// ascending edge order), lanes = the patch's edges:
//   * C, u and the patch's E row are wave sums of its edges -- no atomics;
//   * the pose-block terms go into a per-wave LDS partial of H = B - E Q E^T
//     (upper triangle) and g = v - E Q u: the shared-frame (i, i) block by wave
//     sums, each edge's own (j, j) / (i, j) blocks by one ds_add per value
//     (the edges of one patch have distinct target frames, so a ds_add never
//     sees two lanes on one address; otherwise the patch runs lane by lane),
//     and the patch's Schur term -Q e e^T over the poses it touches;
//   * the next iteration's launch first applies this one's depth update
//     dZ = Q (u - e . dX) to its patches (ba_cuda.cu:191-211, :523).
// Per-wave partials are summed in a fixed order (workgroup, then a reduce
// kernel), so every run gives the same bits.  The 6N x 6N (N <= 12) system
// is factored by one workgroup, one barrier per column, the augmented row g
// carried along (forward substitution for free), then one wave back-
// substitutes and the poses are retracted.
// ---------------------------------------------------------------------------
typedef float bd_f4v __attribute__((ext_vector_type(4)));
typedef int bd_i4v __attribute__((ext_vector_type(4)));
constexpr int BD_NMAX = 12;
constexpr int BD_N6MAX = 6 * BD_NMAX;     // 72
// 4 waves per workgroup at ~235 VGPRs (2 per SIMD: the 512 workgroups are all
// resident).  6 waves -- all of C2's ~2,100 kk groups in one pass -- measured
// 45.8 -> 54.8 us per iteration as is, 69 with the VGPRs capped for 3 per SIMD
// (spills).
constexpr int BD_WAVES = 4;
constexpr int BD_HD_LD = 64;   // row pitch of the dense lower-triangle system the wave solver loads
static_assert(6 * 10 + 1 <= 64 && 6 * 10 < BD_HD_LD, "Hd (64 rows x BD_HD_LD) holds the wave solver's n6 + 1 rows");
// 4 waves each.  Measured over 256-2048 (round 3) and again with this round's
// reduce and solve: 768 / 1024 workgroups 54-56 us per iteration at C2
// against 46 at 512 (the reduce reads every workgroup's partial)
constexpr int BD_GRID = 512;
static_assert(BD_GRID % 16 == 0, "bd_reduce_kernel: 16 waves split the partials evenly");
static int bd_grid() { return BD_GRID; }

struct BdLayout {
    size_t hdr, gid, offs, perm, groups, gbws, gbws_bytes, erec, grec, Em, Cg, ug, Hpart, H, Hd, dX, total;
    int64_t mu_max;
    int n6, nup, ent;
};

static BdLayout bd_layout(int64_t E, int64_t num_patches, int N)
{
    BdLayout L{};
    L.n6 = 6 * N;
    L.nup = L.n6 * (L.n6 + 1) / 2;
    L.ent = L.nup + L.n6;
    L.mu_max = std::max<int64_t>(1, std::min(E, num_patches));
    const size_t e = (size_t)std::max<int64_t>(E, 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return o; };
    L.hdr = take(HDR_WORDS * 4);
    L.gid = take(e * 8);
    L.offs = take((e + 1) * 4);
    L.perm = take(e * 4);
    L.groups = take(8);
    L.gbws_bytes = dpvo_group_by_workspace_bytes((int64_t)e);
    L.gbws = take(L.gbws_bytes);
    L.erec = take(e * 32);
    L.grec = take((size_t)L.mu_max * 16);
    L.Em = take((size_t)L.mu_max * std::max(L.n6, 1) * 4);
    L.Cg = take((size_t)L.mu_max * 4);
    L.ug = take((size_t)L.mu_max * 4);
    L.Hpart = take((size_t)BD_GRID * std::max(L.ent, 1) * 4);
    L.H = take((size_t)std::max(L.ent, 1) * 4);
    L.Hd = take((size_t)64 * BD_HD_LD * 4);
    L.dX = take((size_t)std::max(L.n6, 1) * 4);
    L.total = off;
    return L;
}

struct BdParams {
    float* poses;
    float* patches;
    const float* intrinsics;
    const float* target;
    const float* weight;
    const float* lmbda;
    const int64_t* ii;
    const int64_t* jj;
    const int64_t* kk;
    int64_t num_patches, mu_max;
    int P, t0, N, n6, nup, ent;
    const int* offs;       // kk group-by CSR
    const int* perm;
    const int64_t* groups;
    int64_t E;
    // per-call gathers in CSR order (bd_prep_kernel): edge q = (i, j, target)
    // and (weight, -, -); group g = (start, count, patch k or -1, -)
    bd_f4v* erec;
    bd_i4v* grec;
    int* status;
    float *Em, *Cg, *ug, *Hpart, *H, *Hd, *dX;
    // depth prior (dpvo_ba_forward_prior): nullptr = the plain call
    const float* est;      // [num_patches][3][P][P], channel 2 at the centre pixel
    float mu;
};

// row-major upper triangle of the n6 x n6 system, a <= b
__device__ __forceinline__ int tri_up(int a, int b, int n6) { return a * (2 * n6 - a + 1) / 2 + (b - a); }

// all-lane sum kept in VGPRs (no readlanes: 33 sums in flight would not fit
// in SGPRs); (r0 + r1) + (r2 + r3) of the four DPP-row sums, the same bits in
// every lane since a + b == b + a
__device__ __forceinline__ float wave64_allsum(float s)
{
    s = row16_sum(s);
    // gfx950 lane swaps (VALU, no LDS round trip): rows 0+1 / 2+3, then halves
    auto h = __builtin_amdgcn_permlane16_swap(__float_as_int(s), __float_as_int(s), false, false);
    s = __int_as_float(h[0]) + __int_as_float(h[1]);
    auto w = __builtin_amdgcn_permlane32_swap(__float_as_int(s), __float_as_int(s), false, false);
    return __int_as_float(w[0]) + __int_as_float(w[1]);
}

// 33 per-lane values summed over the wave, total of value L left in lane L
// (lanes 33..63: don't care) -- a reduce-scatter butterfly: each exchange
// step halves the values a lane carries (33 + 16 + 8 + 4 + 2 + 1 exchanges
// instead of 33 all-lane reductions of 6 each).  A fixed tree: every run
// gives the same bits.
__device__ __forceinline__ float wave64_sum33(const float (&v)[33], int lane)
{
    float y[32];
    {
        // slot 0 pairs with slot 32 (lanes >= 32 keep slot 32), the others with
        // themselves: y[j] = total over lanes L, L ^ 32 of slot j (+ 32 b5)
        // (v_permlane32_swap exchanges the first operand's upper 32 lanes with
        // the second's lower 32: the two results summed are the pair's total)
        auto h0 = __builtin_amdgcn_permlane32_swap(__float_as_int(v[0]), __float_as_int(v[32]), false, false);
        y[0] = __int_as_float(h0[0]) + __int_as_float(h0[1]);
#pragma unroll
        for (int j = 1; j < 32; j++) {
            auto h = __builtin_amdgcn_permlane32_swap(__float_as_int(v[j]), __float_as_int(v[j]), false, false);
            y[j] = __int_as_float(h[0]) + __int_as_float(h[1]);
        }
    }
    float z[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {   // bit 4: keep slot j (0) or j + 16 (1); permlane16_swap
        // exchanges the first operand's odd 16-lane rows with the second's even rows
        auto h = __builtin_amdgcn_permlane16_swap(__float_as_int(y[j]), __float_as_int(y[j + 16]), false, false);
        z[j] = __int_as_float(h[0]) + __int_as_float(h[1]);
    }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {   // bit 3, partner lane ^ 8 (row rotate by 8)
        const float send = b3 ? z[j] : z[j + 8], keep = b3 ? z[j + 8] : z[j];
        q[j] = keep + dpp_rot<0x128>(send);
    }
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {   // bit 2, partner lane ^ 4 (swizzle xor 4)
        const float send = b2 ? q[j] : q[j + 4], keep = b2 ? q[j + 4] : q[j];
        r[j] = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x101F));
    }
    float t2[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {   // bit 1, quad_perm [2, 3, 0, 1]
        const float send = b1 ? r[j] : r[j + 2], keep = b1 ? r[j + 2] : r[j];
        t2[j] = keep + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0x4E, 0xF, 0xF, false));
    }
    // bit 0, quad_perm [1, 0, 3, 2]
    const float send = b0 ? t2[0] : t2[1], keep = b0 ? t2[1] : t2[0];
    return keep + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0xB1, 0xF, 0xF, false));
}

__device__ __forceinline__ unsigned wave_or(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// per-edge Jacobians of one residual pair (ba_cuda.cu:254-290, 326-330)
struct BdEdge {
    float Ji[2][6], Jj[2][6], Jz[2], w[2], r[2];
    int ix, jx;
    bool iv, jv, self;
};

__device__ __forceinline__ void bd_edge(const BdParams& p, const bd_f4v r0, const bd_f4v r1, float px, float py,
                                        float dk, float fx, float fy, float cx, float cy, BdEdge& o)
{
    const int64_t i_abs = __float_as_int(r0[0]), j_abs = __float_as_int(r0[1]);
    const float* Pi = p.poses + i_abs * 7;
    const float* Pj = p.poses + j_abs * 7;
    const float ti[3] = {Pi[0], Pi[1], Pi[2]}, tj[3] = {Pj[0], Pj[1], Pj[2]};
    const float qi[4] = {Pi[3], Pi[4], Pi[5], Pi[6]}, qj[4] = {Pj[3], Pj[4], Pj[5], Pj[6]};
    float Xi[4], Xj[4], tij[3], qij[4];
    Xi[0] = (px - cx) / fx;
    Xi[1] = (py - cy) / fy;
    Xi[2] = 1.0f;
    Xi[3] = dk;
    relSE3(ti, qi, tj, qj, tij, qij);
    actSE3(tij, qij, Xi, Xj);
    const float X = Xj[0], Y = Xj[1], Z = Xj[2], W = Xj[3];
    const float d = (Z >= 0.2f) ? 1.0f / Z : 0.0f;
    const float d2 = d * d;
    const float x1 = fx * (X / Z) + cx, y1 = fy * (Y / Z) + cy;
    const float rx = r0[2] - x1, ry = r0[3] - y1;
    const bool in_bounds = (sqrtf(rx * rx + ry * ry) < 128.f) && (Z > 0.2f) && (x1 > -64.f) && (y1 > -64.f) &&
                           (x1 < 2.f * cx + 64.f) && (y1 < 2.f * cy + 64.f);
    const float mask = in_bounds ? 1.0f : 0.0f;
    o.w[0] = mask * r1[0];
    o.w[1] = mask * r1[1];
    o.r[0] = rx;
    o.r[1] = ry;
    o.Jz[0] = fx * (tij[0] * d - tij[2] * (X * d2));
    o.Jz[1] = fy * (tij[1] * d - tij[2] * (Y * d2));
    const float a[6] = {fx * W * d, 0.f, fx * -X * W * d2, fx * -X * Y * d2, fx * (1.f + X * X * d2), fx * -Y * d};
    const float b[6] = {0.f, fy * W * d, fy * -Y * W * d2, fy * (-1.f - Y * Y * d2), fy * (X * Y * d2), fy * X * d};
#pragma unroll
    for (int t = 0; t < 6; t++) {
        o.Jj[0][t] = a[t];
        o.Jj[1][t] = b[t];
    }
    adjSE3(tij, qij, o.Jj[0], o.Ji[0]);
    adjSE3(tij, qij, o.Jj[1], o.Ji[1]);
    o.ix = (int)(i_abs - p.t0);
    o.jx = (int)(j_abs - p.t0);
    o.iv = o.ix >= 0 && o.ix < p.N;
    o.jv = o.jx >= 0 && o.jx < p.N;
    o.self = o.iv && o.jv && o.ix == o.jx;
}

// the terms of one edge on the patch's own frame i (a self edge folds its
// j terms in, ba_cuda.cu:294-322): (i, i) upper block, v_i, E_i
__device__ __forceinline__ void bd_iterms(const BdEdge& o, float bii[21], float vi[6], float Ei[6])
{
    int u = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++, u++) {
            float s = 0.f;
#pragma unroll
            for (int row = 0; row < 2; row++) {
                if (o.self)
                    s += o.w[row] * (o.Ji[row][a] * o.Ji[row][b] + o.Jj[row][a] * o.Jj[row][b] -
                                     o.Ji[row][a] * o.Jj[row][b] - o.Jj[row][a] * o.Ji[row][b]);
                else
                    s += o.w[row] * o.Ji[row][a] * o.Ji[row][b];
            }
            bii[u] = o.iv ? s : 0.f;
        }
#pragma unroll
    for (int t = 0; t < 6; t++) {
        float v = -o.w[0] * o.r[0] * o.Ji[0][t] - o.w[1] * o.r[1] * o.Ji[1][t];
        float e = -o.w[0] * o.Jz[0] * o.Ji[0][t] - o.w[1] * o.Jz[1] * o.Ji[1][t];
        if (o.self) {
            v += o.w[0] * o.r[0] * o.Jj[0][t] + o.w[1] * o.r[1] * o.Jj[1][t];
            e += o.w[0] * o.Jz[0] * o.Jj[0][t] + o.w[1] * o.Jz[1] * o.Jj[1][t];
        }
        vi[t] = o.iv ? v : 0.f;
        Ei[t] = o.iv ? e : 0.f;
    }
}

// the edge's own target-frame terms, added to the wave's partial and E row
__device__ __forceinline__ void bd_jterms_add(const BdEdge& o, float* part, float* ev, int n6, int nup)
{
    if (!o.jv || o.self) return;
    const int j6 = 6 * o.jx;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++)
            atomicAdd(&part[tri_up(j6 + a, j6 + b, n6)], o.w[0] * o.Jj[0][a] * o.Jj[0][b] + o.w[1] * o.Jj[1][a] * o.Jj[1][b]);
        atomicAdd(&part[nup + j6 + a], o.w[0] * o.r[0] * o.Jj[0][a] + o.w[1] * o.r[1] * o.Jj[1][a]);
        atomicAdd(&ev[j6 + a], o.w[0] * o.Jz[0] * o.Jj[0][a] + o.w[1] * o.Jz[1] * o.Jj[1][a]);
    }
    if (o.iv) {
        const int i6 = 6 * o.ix;
        const bool up = o.ix < o.jx;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const float s = up ? -(o.w[0] * o.Ji[0][a] * o.Jj[0][b] + o.w[1] * o.Ji[1][a] * o.Jj[1][b])
                                   : -(o.w[0] * o.Jj[0][a] * o.Ji[0][b] + o.w[1] * o.Jj[1][a] * o.Ji[1][b]);
                atomicAdd(&part[up ? tri_up(i6 + a, j6 + b, n6) : tri_up(j6 + a, i6 + b, n6)], s);
            }
    }
}

// The Schur term  H -= sum_k Q_k e_k e_k^T,  g -= sum_k Q_k u_k e_k  over a
// workgroup's patches: every wave parks its patch's E row, Q_k E row and
// Q_k u_k in a slot of the workgroup's list (slot = wave + BD_WAVES * its
// local iteration: a fixed order), and at a flush every thread owns
// upper-triangle entries of the partial and sums the listed patches' products
// into them in slot order -- a rank-BD_SLOTS update with plain LDS reads, no
// atomics.  Every entry is a sum of a[s] * b[s] over the slots (Hessian entry
// (r, c): (Q e)[r] * e[c]; gradient entry r: (Q u) * e[r]), so a thread takes
// its entries BD_FLUSH_J at a time, two LDS reads per entry and slot with the
// reads of the BD_FLUSH_J independent sums in flight together (one entry at a
// time, the sum's dependence left the reads' latency exposed: ~14k cycles per
// flush at C2, 6k now).
constexpr int BD_SLOT_IT = 8;                     // wave iterations per flush
constexpr int BD_SLOTS = BD_SLOT_IT * BD_WAVES;   // listed patches per flush
constexpr int BD_SLOT_LD = 2 * BD_N6MAX + 2;      // E row, Q E row, Q u, pad
constexpr int BD_SLOT_QE = BD_N6MAX, BD_SLOT_QU = 2 * BD_N6MAX;
constexpr int BD_FLUSH_J = 4;
static_assert(BD_SLOTS * BD_SLOT_LD % 4 == 0, "slot list zeroed in 16-byte stores");

// Once per call: the edge data the patch kernel needs, gathered into CSR
// order (one coalesced 32-byte record per edge instead of perm -> ii / jj /
// target / weight), and each group's (start, count, patch), so every BA
// iteration's per-patch chain of dependent loads is group -> edges -> poses.
__global__ __launch_bounds__(256) void bd_prep_kernel(BdParams p)
{
    const int64_t G = min(*p.groups, p.mu_max);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < p.E; q += stride) {
        const int64_t e = p.perm[q];
        p.erec[2 * q] = bd_f4v{__int_as_float((int)p.ii[e]), __int_as_float((int)p.jj[e]), p.target[2 * e],
                               p.target[2 * e + 1]};
        p.erec[2 * q + 1] = bd_f4v{p.weight[2 * e], p.weight[2 * e + 1], 0.f, 0.f};
    }
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < G; g += stride) {
        const int start = p.offs[g];
        const int64_t k = p.kk[p.perm[start]];
        p.grec[g] = bd_i4v{start, p.offs[g + 1] - start, (k < 0 || k >= p.num_patches) ? -1 : (int)k, 0};
    }
}

#ifdef DPVO_STAMPS
// Diagnostic build only (never the product library): per-wave cycle sums of
// the patch kernel's phases, s_memtime stamps.  dpvo_bd_stamps[block][wave][seg].
__device__ unsigned long long dpvo_bd_stamps[BD_GRID * BD_WAVES * 16];
#define BD_STAMP(v)                                                                            \
    unsigned long long v;                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");                  \
    __builtin_amdgcn_sched_barrier(0);
#define BD_ACC(seg, a, b) bst[seg] += (b) - (a);
#else
#define BD_STAMP(v)
#define BD_ACC(seg, a, b)
#endif

template <bool APPLY, bool HESS>
__global__ __launch_bounds__(64 * BD_WAVES) void bd_patch_kernel(BdParams p)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    if (*(volatile int*)p.status != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n6 = p.n6, nup = p.nup, ent = p.ent, N = p.N;
    const int entp = (ent + 3) & ~3;   // per-wave partial pitch (16-byte aligned)
#ifdef DPVO_STAMPS
    unsigned long long bst[16] = {};
#endif
    BD_STAMP(t_begin)
    const bool pose_terms = HESS && N > 0;
    float* part = sm + wave * entp;
    float* ev = sm + BD_WAVES * entp + wave * BD_N6MAX;
    // (row, column) of every upper-triangle entry k = tri_up(r, c): r | c << 8
    uint16_t* tri_rc = reinterpret_cast<uint16_t*>(sm + BD_WAVES * entp + BD_WAVES * BD_N6MAX);
    float* slots = sm + BD_WAVES * entp + BD_WAVES * BD_N6MAX + (pose_terms ? (nup + 7) / 8 * 4 : 0);   // 16-B aligned
    if (pose_terms) {
        // (16-byte stores: BD_WAVES * entp and BD_SLOTS * BD_SLOT_LD are multiples of 4)
        for (int i = threadIdx.x; i < BD_WAVES * entp / 4; i += blockDim.x) ((bd_f4v*)sm)[i] = bd_f4v{0.f, 0.f, 0.f, 0.f};
        for (int i = threadIdx.x; i < BD_SLOTS * BD_SLOT_LD / 4; i += blockDim.x)
            ((bd_f4v*)slots)[i] = bd_f4v{0.f, 0.f, 0.f, 0.f};
        // (row, column) of packed entry k, one entry per thread and pass: the row
        // from the closed form of tri_up, corrected by one step either way
        const float nn = (float)(2 * n6 + 1);
        for (int k = threadIdx.x; k < nup; k += blockDim.x) {
            int r = (int)((nn - sqrtf(nn * nn - 8.f * (float)k)) * 0.5f);
            r = min(max(r, 0), n6 - 1);
            if (r + 1 < n6 && tri_up(r + 1, r + 1, n6) <= k) r++;
            if (tri_up(r, r, n6) > k) r--;
            tri_rc[k] = (uint16_t)(r | (r + k - tri_up(r, r, n6)) << 8);
        }
    }
    __syncthreads();
    BD_STAMP(t_init)
    BD_ACC(0, t_begin, t_init)
    const int64_t G = min(*p.groups, p.mu_max);
    const float lm = p.lmbda[0];
    const float fx = p.intrinsics[0], fy = p.intrinsics[1], cx = p.intrinsics[2], cy = p.intrinsics[3];
    const int64_t PP = (int64_t)p.P * p.P, centre = (p.P / 2) * p.P + p.P / 2;
    const float dx0 = (APPLY && lane < n6) ? p.dX[lane] : 0.f;
    const float dx1 = (APPLY && lane + 64 < n6) ? p.dX[lane + 64] : 0.f;

    // every wave of every workgroup runs the same number of iterations (the
    // flushes are workgroup barriers); g >= G leaves the wave's slot empty
    const int64_t stride = (int64_t)gridDim.x * BD_WAVES;
    const int64_t niter = (G + stride - 1) / stride;
    for (int64_t it = 0; it < niter; it++) {
        const int64_t g = it * stride + (int64_t)blockIdx.x * BD_WAVES + wave;
        const int sit = (int)(it % BD_SLOT_IT);
        float* slot = slots + (sit * BD_WAVES + wave) * BD_SLOT_LD;
        if (pose_terms) {   // empty until filled (Q e = 0, Q u = 0)
            if (lane < n6) slot[BD_SLOT_QE + lane] = 0.f;
            if (lane + 64 < n6) slot[BD_SLOT_QE + 64 + lane] = 0.f;
            if (lane == 0) slot[BD_SLOT_QU] = 0.f;
        }
        BD_STAMP(ti0)
        if (g < G) do {
        const bd_i4v gr = p.grec[g];
        const int start = gr[0], cnt = gr[1];
        const int64_t k = gr[2];
        if (k < 0) {
            if (lane == 0) atomicExch(p.status, -1);  // patch index out of range
            continue;
        }
        float* pd = p.patches + (k * 3 + 2) * PP;
        float dk;
        if (APPLY) {
            // this patch's depth update from the previous iteration's solve
            const float Q = 1.0f / (p.Cg[g] + lm);
            float s = 0.f;
            if (N > 0) {
                const float* Er = p.Em + g * n6;
                s = wave64_sum((lane < n6 ? Er[lane] * dx0 : 0.f) + (lane + 64 < n6 ? Er[lane + 64] * dx1 : 0.f));
            }
            float d = pd[0] + Q * (p.ug[g] - s);
            d = (d > 20.f) ? 1.0f : d;
            d = fmaxf(d, 1e-4f);
            if (lane < PP) pd[lane] = d;
            dk = d;
        } else {
            dk = pd[centre];
        }
        if (!HESS) continue;   // (leaves the do-while: the next iteration)
        const float px = p.patches[(k * 3 + 0) * PP + centre], py = p.patches[(k * 3 + 1) * PP + centre];
        // depth prior: one centre-pixel load per patch, in flight with px / py;
        // p.est is a kernel argument, so the test is wave-uniform and the plain
        // call (nullptr) issues nothing
        float est = 0.f;
        if (p.est != nullptr) {
            float e0 = 0.f;
            if (lane == 0) e0 = p.est[(k * 3 + 2) * PP + centre];
            est = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e0)));
        }

        if (pose_terms) {
            if (lane < n6) ev[lane] = 0.f;
            if (lane + 64 < n6) ev[lane + 64] = 0.f;
        }
        float Ck = 0.f, uk = 0.f;
        wave_lds_fence();
        BD_STAMP(ti1)
        BD_ACC(1, ti0, ti1)
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const bool on = lane < cnt - c0;
            const int q = on ? start + c0 + lane : start;
            BdEdge o;
            bd_edge(p, p.erec[2 * q], p.erec[2 * q + 1], px, py, dk, fx, fy, cx, cy, o);
#ifdef DPVO_STAMPS
            asm volatile("" ::"v"(o.Ji[0][0]), "v"(o.Jj[1][5]), "v"(o.w[0]), "v"(o.r[1]));
#endif
            BD_STAMP(tc0)
            BD_ACC(2, ti1, tc0)
            if (!on) { o.w[0] = o.w[1] = 0.f; o.iv = o.jv = o.self = false; }
            float cl = 0.f, ul = 0.f;
#pragma unroll
            for (int row = 0; row < 2; row++) {
                cl += o.w[row] * o.Jz[row] * o.Jz[row];
                ul += o.w[row] * o.r[row] * o.Jz[row];
            }
            Ck += wave64_sum(cl);
            uk += wave64_sum(ul);
            if (!pose_terms) continue;
            // one pass when every edge of the patch has the same frame i (DPVO:
            // the patch's own frame) and distinct target frames; otherwise one
            // lane per pass, in edge order
            const uint64_t ivm0 = __ballot(o.iv);
            const int ix0 = __shfl(o.ix, ivm0 ? __ffsll((unsigned long long)ivm0) - 1 : 0);
            bool mixed = __ballot(o.iv && o.ix != ix0) != 0;
            const bool jt = o.jv && !o.self;
            for (int q = 0; q < N && !mixed; q++)
                mixed = __popcll(__ballot(jt && o.jx == q)) > 1;
            const int passes = mixed ? 64 : 1;
            BD_STAMP(tc1)
            BD_ACC(3, tc0, tc1)
            for (int ps = 0; ps < passes; ps++) {
                const bool act = !mixed || lane == ps;
                const uint64_t ivm = __ballot(act && o.iv);
                if (ivm) {
                    // the shared-frame terms: wave sums, entry t added by lane t
                    const int i6 = 6 * __shfl(o.ix, __ffsll((unsigned long long)ivm) - 1);
                    float bii[21], vi[6], Ei[6];
                    bd_iterms(o, bii, vi, Ei);
                    // lane u < 21: the (i, i) entry u; 21 + t: v_i[t]; 27 + t: E_i[t]
                    float x33[33];
#pragma unroll
                    for (int u = 0; u < 21; u++) x33[u] = act ? bii[u] : 0.f;
#pragma unroll
                    for (int t = 0; t < 6; t++) {
                        x33[21 + t] = act ? vi[t] : 0.f;
                        x33[27 + t] = act ? Ei[t] : 0.f;
                    }
                    const float val = wave64_sum33(x33, lane);
                    int addr = -1;
                    float* base = part;
                    if (lane < 21) {
                        int a = 0, r = lane;
                        while (r >= 6 - a) { r -= 6 - a; a++; }
                        addr = tri_up(i6 + a, i6 + a + r, n6);
                    } else if (lane < 27) {
                        addr = nup + i6 + lane - 21;
                    } else if (lane < 33) {
                        addr = i6 + lane - 27;
                        base = ev;
                    }
                    if (addr >= 0) atomicAdd(&base[addr], val);
                }
                BD_STAMP(tc2)
                if (act) bd_jterms_add(o, part, ev, n6, nup);
                wave_lds_fence();
                BD_STAMP(tc3)
                BD_ACC(4, tc1, tc2)
                BD_ACC(5, tc2, tc3)
            }
        }
        BD_STAMP(ti2)
        // dk is this iteration's depth (post-APPLY).  Added after the edge sums,
        // in this fixed place: the path stays bitwise repeatable.  The stored
        // Cg / ug carry the term, so the next launch's APPLY needs nothing new.
        if (prior_valid(est)) {
            Ck += p.mu;
            uk -= p.mu * (dk - est);
        }
        if (!pose_terms) {
            if (lane == 0) { p.Cg[g] = Ck; p.ug[g] = uk; }
            continue;
        }
        wave_lds_fence();
        // the patch's E row, C, u (the next launch's depth update reads them)
        const float e0 = lane < n6 ? ev[lane] : 0.f, e1 = lane + 64 < n6 ? ev[lane + 64] : 0.f;
        float* Er = p.Em + g * n6;
        if (lane < n6) Er[lane] = e0;
        if (lane + 64 < n6) Er[lane + 64] = e1;
        if (lane == 0) { p.Cg[g] = Ck; p.ug[g] = uk; }
        // the Schur term goes through the workgroup's slot list (flushed below)
        const float Q = 1.0f / (Ck + lm);
        if (lane < n6) {
            slot[lane] = e0;
            slot[BD_SLOT_QE + lane] = Q * e0;
        }
        if (lane + 64 < n6) {
            slot[lane + 64] = e1;
            slot[BD_SLOT_QE + 64 + lane] = Q * e1;
        }
        if (lane == 0) slot[BD_SLOT_QU] = Q * uk;
        wave_lds_fence();
        BD_STAMP(ti3)
        BD_ACC(6, ti2, ti3)
        } while (false);
        BD_STAMP(tf0)
        if (pose_terms && (sit == BD_SLOT_IT - 1 || it == niter - 1)) {
            // flush: H_k -= sum_s (Q_s e_s[r]) e_s[c], g_r -= sum_s (Q u)_s e_s[r],
            // slots in order, into wave 0's partial
            __syncthreads();
            const int ns = (sit + 1) * BD_WAVES;
            for (int k0 = threadIdx.x; k0 < ent; k0 += BD_FLUSH_J * (int)blockDim.x) {
                float acc[BD_FLUSH_J];
                int oa[BD_FLUSH_J], ob[BD_FLUSH_J];
#pragma unroll
                for (int j = 0; j < BD_FLUSH_J; j++) {
                    const int kx = k0 + j * (int)blockDim.x;
                    const int rc = kx < nup ? tri_rc[kx] : 0;
                    oa[j] = kx < nup ? BD_SLOT_QE + (rc & 255) : BD_SLOT_QU;
                    ob[j] = kx < nup ? rc >> 8 : kx - nup;
                    if (kx >= ent) oa[j] = ob[j] = 0;   // (a pass past the end: read, never stored)
                    acc[j] = kx < ent ? sm[kx] : 0.f;
                }
                for (int q = 0; q < ns; q++) {
                    const float* sl = slots + q * BD_SLOT_LD;
#pragma unroll
                    for (int j = 0; j < BD_FLUSH_J; j++) acc[j] -= sl[oa[j]] * sl[ob[j]];
                }
#pragma unroll
                for (int j = 0; j < BD_FLUSH_J; j++)
                    if (k0 + j * (int)blockDim.x < ent) sm[k0 + j * (int)blockDim.x] = acc[j];
            }
            __syncthreads();
        }
        BD_STAMP(tf1)
        BD_ACC(7, tf0, tf1)
        BD_ACC(8, ti0, tf0)
    }
    if (!pose_terms) return;
    // the workgroup's partial: its waves' partials summed in wave order
    __syncthreads();
    BD_STAMP(tw0)
    float* dst = p.Hpart + (int64_t)blockIdx.x * ent;
    for (int i = threadIdx.x; i < ent; i += blockDim.x) {
        float s = sm[i];
#pragma unroll
        for (int w = 1; w < BD_WAVES; w++) s += sm[w * entp + i];
        dst[i] = s;
    }
#ifdef DPVO_STAMPS
    BD_STAMP(t_end)
    BD_ACC(9, tw0, t_end)
    BD_ACC(10, t_begin, t_end)
    if (lane == 0 && APPLY)
        for (int k = 0; k < 16; k++) dpvo_bd_stamps[((int64_t)blockIdx.x * BD_WAVES + wave) * 16 + k] = bst[k];
#endif
}

// H = sum of the patch kernel's workgroup partials, fixed order.  Also stored
// as dense rows for the wave solver: Hd[b][a] = H(a, b) (a <= b, the lower
// triangle, row pitch BD_HD_LD) and row n6 = g.
// 32 entries per workgroup (twice the workgroups of a 64-entry split: the
// reduce is bound by how fast few CUs pull the 512 partials, 3.9 MB at C2/C3):
// half h = lane / 32 of each wave reads partial rows 2 (wave + 16 j) + h, every
// row segment a full 128-byte line; the halves' sums are added by a lane swap,
// the waves' in wave order -- a fixed order, so the same bits every call.
constexpr int BR_E = 32;
__global__ __launch_bounds__(1024) void bd_reduce_kernel(BdParams p)
{
    __shared__ float red[16][BR_E];
    if (*(volatile int*)p.status != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, e = lane & 31;
    const int i = blockIdx.x * BR_E + e;
    // all of this lane's partials in flight at once (one HBM round trip),
    // then summed in row order
    constexpr int PER = BD_GRID / 32;
    static_assert(BD_GRID % 32 == 0, "16 waves x 2 halves split the partials evenly");
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; j++)
        v[j] = i < p.ent ? p.Hpart[(int64_t)(2 * (wave + 16 * j) + h) * p.ent + i] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; j++) s += v[j];
    {
        auto w2 = __builtin_amdgcn_permlane32_swap(__float_as_int(s), __float_as_int(s), false, false);
        const float o = __int_as_float(h ? w2[0] : w2[1]);   // the other half's sum
        s = h ? o + s : s + o;                              // (half 0's + half 1's in both)
    }
    if (h == 0) red[wave][e] = s;
    __syncthreads();
    if (wave == 0 && h == 0 && i < p.ent) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; w++) t += red[w][e];
        p.H[i] = t;
        const int n = p.n6;
        int a = 0, b;
        if (i < p.nup) {   // (a, b) of the packed upper entry i
            int k = i;
            while (k >= n - a) { k -= n - a; a++; }
            b = a + k;
        } else {
            a = i - p.nup;
            b = n;
        }
        // the wave solver's rows: the damped lower triangle (S += diag(1e-4 S
        // + 1), ba_cuda.cu:517-518), zeros above it, the g row.  Only for the
        // windows it solves (n6 + 1 rows of BD_HD_LD): 11-12 poses go to
        // bd_solve_kernel, which reads H, and would overrun Hd's 64 rows
        if (n < BD_HD_LD) {
            p.Hd[b * BD_HD_LD + a] = a == b ? t + (1e-4f * t + 1.0f) : t;
            if (a < b && b < n) p.Hd[a * BD_HD_LD + b] = 0.f;
        }
    }
}

// damping S += diag(1e-4 S + 1) (ba_cuda.cu:517-518), fp32 Cholesky of the
// augmented [S; g^T], back substitution, retraction.  The factor is blocked by
// pose (6 x 6 blocks): per block column one thread factors the diagonal block,
// one thread per remaining row solves its panel row, and the trailing update
// (a 6-term dot product per entry) is spread over the workgroup -- three
// barriers per pose instead of one per column.  The augmented row n rides
// along as an extra panel row, so it ends as z = L^-1 g.
constexpr int BS_LD = BD_N6MAX + 4;   // 76: quad-aligned rows (the trailing update reads float4s)
typedef float bs_f4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void bd_solve_kernel(BdParams p)
{
    __shared__ __attribute__((aligned(16))) float A[(BD_N6MAX + 1) * BS_LD];   // lower triangle, rows 0..n (row n = g^T)
    __shared__ __attribute__((aligned(16))) float PT[6][BS_LD];                // the current panel, transposed
    __shared__ float xs[BD_N6MAX];
    __shared__ float dinv[BD_N6MAX];
    __shared__ int sfail;
    if (*(volatile int*)p.status != 0) return;
    const int n = p.n6, tid = threadIdx.x, N = p.N;
    // every load issued before any is used: one L2 round trip, not one per entry
    constexpr int NLD = ((BD_N6MAX + 1) * BD_N6MAX + 255) / 256;
    float hv[NLD];
#pragma unroll
    for (int s2 = 0; s2 < NLD; s2++) {
        const int t = tid + 256 * s2;
        const int r = t / max(n, 1), c = t - r * n;
        int src = -1;
        if (t < (n + 1) * n) src = r == n ? p.nup + c : (c <= r ? tri_up(c, r, n) : -1);
        hv[s2] = p.H[src < 0 ? 0 : src];
        if (src < 0) hv[s2] = 0.f;
    }
#pragma unroll
    for (int s2 = 0; s2 < NLD; s2++) {
        const int t = tid + 256 * s2;
        if (t < (n + 1) * n) {
            const int r = t / n, c = t - r * n;
            float v = hv[s2];
            if (r == c) v += 1e-4f * v + 1.0f;
            A[r * BS_LD + c] = v;
        }
    }
    if (tid == 0) sfail = 0;
    __syncthreads();
    for (int kb = 0; kb < N; kb++) {
        const int k0 = 6 * kb;
        // 1. the diagonal block, in place (one thread; the pivots in column order)
        if (tid == 0) {
            float L[6][6];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j <= i; j++) L[i][j] = A[(k0 + i) * BS_LD + k0 + j];
            int fail = 0;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                float d = L[j][j];
#pragma unroll
                for (int t = 0; t < j; t++) d -= L[j][t] * L[j][t];
                if (!(d > 0.f) && !fail) fail = k0 + j + 1;
                const float l = sqrtf(d), il = 1.0f / l;
                L[j][j] = l;
                dinv[k0 + j] = il;
#pragma unroll
                for (int i = j + 1; i < 6; i++) {
                    float v = L[i][j];
#pragma unroll
                    for (int t = 0; t < j; t++) v -= L[i][t] * L[j][t];
                    L[i][j] = v * il;
                }
            }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j <= i; j++) A[(k0 + i) * BS_LD + k0 + j] = L[i][j];
            sfail = fail;
        }
        __syncthreads();
        if (sfail) break;
        // 2. panel rows below the block (and the augmented row n): x L_kk^T = a
        const int c1 = k0 + 6;   // first trailing column
        const int rows = n + 1 - c1;
        if (tid < rows) {
            const int r = c1 + tid;
            float x[6];
#pragma unroll
            for (int t = 0; t < 6; t++) {
                float v = A[r * BS_LD + k0 + t];
#pragma unroll
                for (int s2 = 0; s2 < t; s2++) v -= A[(k0 + t) * BS_LD + k0 + s2] * x[s2];
                x[t] = v * dinv[k0 + t];
            }
#pragma unroll
            for (int t = 0; t < 6; t++) {
                A[r * BS_LD + k0 + t] = x[t];
                PT[t][r] = x[t];
            }
        }
        __syncthreads();
        // 3. trailing update A[r][c] -= L[r][k0:k0+6] . L[c][k0:k0+6] for c1 <= c <= r
        // (row n: every c < n), four columns per item from the transposed panel
        const int q0 = c1 >> 2, nq = ((n + 3) >> 2) - q0;
        for (int it = tid; it < rows * nq; it += 256) {
            const int ri = it / nq;
            const int r = c1 + ri, c0 = 4 * (q0 + it - ri * nq);
            if (r < n && c0 > r) continue;
            float lr[6];
#pragma unroll
            for (int t = 0; t < 6; t++) lr[t] = PT[t][r];
            bs_f4 v = *(const bs_f4*)(A + r * BS_LD + c0);
            bs_f4 u = v;
#pragma unroll
            for (int t = 0; t < 6; t++) {
                const bs_f4 lc = *(const bs_f4*)(&PT[t][c0]);
                u.x -= lr[t] * lc.x;
                u.y -= lr[t] * lc.y;
                u.z -= lr[t] * lc.z;
                u.w -= lr[t] * lc.w;
            }
            // only c1 <= c (and c <= r below row n, c < n on it) change
            const int lim = r < n ? r : n - 1;
            v.x = (c0 + 0 >= c1 && c0 + 0 <= lim) ? u.x : v.x;
            v.y = (c0 + 1 >= c1 && c0 + 1 <= lim) ? u.y : v.y;
            v.z = (c0 + 2 >= c1 && c0 + 2 <= lim) ? u.z : v.z;
            v.w = (c0 + 3 >= c1 && c0 + 3 <= lim) ? u.w : v.w;
            *(bs_f4*)(A + r * BS_LD + c0) = v;
        }
        __syncthreads();
    }
    if (sfail) {
        if (tid == 0) atomicExch(p.status, sfail);
        return;
    }
    // L^T x = z, z = row n of the augmented factor; lane c holds x_c / z_c
    if (tid < 64) {
        float z0 = tid < n ? A[n * BS_LD + tid] : 0.f, z1 = tid + 64 < n ? A[n * BS_LD + tid + 64] : 0.f;
        for (int j = n - 1; j >= 0; j--) {
            const float zj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(j < 64 ? z0 : z1), j & 63));
            const float xj = zj * dinv[j];
            if (tid < j) z0 -= A[j * BS_LD + tid] * xj;
            if (tid + 64 < j) z1 -= A[j * BS_LD + tid + 64] * xj;
            if (tid == (j & 63)) {
                if (j < 64) z0 = xj;
                else z1 = xj;
            }
        }
        if (tid < n) xs[tid] = z0;
        if (tid + 64 < n) xs[tid + 64] = z1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) p.dX[i] = xs[i];
    if (tid < p.N) {
        float* P = p.poses + (int64_t)(p.t0 + tid) * 7;
        const float t0v[3] = {P[0], P[1], P[2]}, q0v[4] = {P[3], P[4], P[5], P[6]};
        float xi[6], t1v[3], q1v[4];
        for (int k = 0; k < 6; k++) xi[k] = xs[6 * tid + k];
        retrSE3(xi, t0v, q0v, t1v, q1v);
        P[0] = t1v[0]; P[1] = t1v[1]; P[2] = t1v[2];
        P[3] = q1v[0]; P[4] = q1v[1]; P[5] = q1v[2]; P[6] = q1v[3];
    }
}

// The same damping / factor / solve / retraction in ONE wave, for windows of
// up to 10 poses (DPVO's OPTIMIZATION_WINDOW; n = 6 NN <= 60), NN compile-time
// so every loop unrolls onto registers.  Lane i holds row i of the lower
// triangle of the augmented [S; g^T] (lane n holds g^T), loaded as 16-byte
// vectors from the reduce kernel's dense rows.
// Right-looking Cholesky, per column k: the pivot by readlane, lane k's
// sqrt and the column scaled by 1/L[k][k]; the next column's entries updated
// through a readlane of L[k+1][k] (the critical path: no LDS round trip),
// every later column through the broadcast of column k from LDS (one
// ds_write per lane, 16-byte broadcast reads, packed FMAs).  The g row rides
// along as row n and ends as z = L^-1 g.  Back substitution L^T x = z on the
// transposed factor (LDS transpose once): lane r then holds column r, and
// every x_j, broadcast by readlane, is one FMA into the running sums --
// no cross-lane reduction per unknown.  Status: the first failing leading
// minor, as torch::linalg::cholesky reports it.
__device__ __forceinline__ float rdl(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

typedef float bd_f2 __attribute__((ext_vector_type(2)));
// f(integral_constant<int, K>) for K = B .. E-1, expanded at compile time
template <int B, int E>
struct bd_unroll {
    template <class F>
    __device__ __forceinline__ static void run(F&& f)
    {
        if constexpr (B < E) {
            f(std::integral_constant<int, B>{});
            bd_unroll<B + 1, E>::run(f);
        }
    }
};
typedef float bd_f4 __attribute__((ext_vector_type(4)));
constexpr int BD_T_LD = 68;   // transpose rows: 272 B, 16-byte aligned, column reads conflict-free

template <int NN>
__global__ __launch_bounds__(64) void bd_solve_wave_kernel(BdParams p)
{
    constexpr int n = 6 * NN;
    constexpr int NV = (n + 3) / 4;   // 16-byte vectors per row
    static_assert(n < 64 && n % 2 == 0, "one lane per row plus the g row; columns in pairs");
    __shared__ __attribute__((aligned(16))) float col[n][64];              // column k of the factor, by row
    __shared__ __attribute__((aligned(16))) float tr[(n + 1) * BD_T_LD];   // the factor, row-major, for the transpose
    __shared__ float xs[64];
    const int status = *(volatile int*)p.status;   // checked once the system loads below are in flight
    const int lane = threadIdx.x;
    // rows 0 .. n (lanes past n load row 0: a harmless copy, never read)
    const float* src = p.Hd + (lane <= n ? lane : 0) * BD_HD_LD;
    float a[4 * NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const bd_f4 x = __builtin_nontemporal_load((const bd_f4*)src + v);
        a[4 * v + 0] = x[0]; a[4 * v + 1] = x[1]; a[4 * v + 2] = x[2]; a[4 * v + 3] = x[3];
    }
    if (status != 0) return;
    // broadcast reads of col[k][c] address LDS as (zero VGPR) + constant offset
    // (otherwise every read materialises its constant address in a VGPR)
    int zoff;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zoff));
    const float(*colz)[64] = reinterpret_cast<const float(*)[64]>(reinterpret_cast<const char*>(col) + zoff);
    // lane k keeps pivot k (one writelane per column); the first failing
    // leading minor is read off a ballot after the factor
    float piv = 1.f;
    // one column step per k, k a compile-time constant (bd_unroll): every a[]
    // index is static, so the system stays in registers at any NN
    bd_unroll<0, n>::run([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const float d = rdl(a[k], k);
        asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(piv) : "s"(d), "n"(k));
        // lane k: d / sqrt(d) = L[k][k]; lanes below it: L[r][k]; lane n: z_k
        a[k] *= __builtin_amdgcn_rsqf(d);
        if constexpr (k + 1 < n) {
            col[k][lane] = a[k];
            a[k + 1] -= a[k] * rdl(a[k], k + 1);   // the next pivot's column: no LDS latency
            // columns k + 2 .. n - 1 from the LDS broadcast of column k: the
            // leading ones alone up to a multiple of 4, then 16-byte broadcast
            // reads (constant offsets on a zero address) and packed FMAs
#pragma unroll
            for (int c = k + 2; c < ((k + 5) & ~3) && c < n; c++) a[c] -= a[k] * colz[k][c];
#pragma unroll
            for (int c = (k + 5) & ~3; c < n; c += 4) {
                if (c + 4 <= n) {
                    const bd_f4 lc = *(const bd_f4*)&colz[k][c];
                    const bd_f2 r0 = __builtin_elementwise_fma(-bd_f2{a[k], a[k]}, bd_f2{lc[0], lc[1]},
                                                               bd_f2{a[c], a[c + 1]});
                    const bd_f2 r1 = __builtin_elementwise_fma(-bd_f2{a[k], a[k]}, bd_f2{lc[2], lc[3]},
                                                               bd_f2{a[c + 2], a[c + 3]});
                    a[c] = r0[0];
                    a[c + 1] = r0[1];
                    a[c + 2] = r1[0];
                    a[c + 3] = r1[1];
                } else {
                    const bd_f2 lc = *(const bd_f2*)&colz[k][c];
                    const bd_f2 r = __builtin_elementwise_fma(-bd_f2{a[k], a[k]}, lc, bd_f2{a[c], a[c + 1]});
                    a[c] = r[0];
                    a[c + 1] = r[1];
                }
            }
        }
    });
    const uint64_t bad = __ballot(lane < n && !(piv > 0.f));
    if (bad) {
        if (lane == 0) atomicExch(p.status, __ffsll((unsigned long long)bad));
        return;
    }
    // transpose through LDS: lane r reads column r -- L[i][r] for i > r, z_r
    // from row n; the diagonal and the entries above it (which the
    // right-looking updates leave as garbage) read as zero
#pragma unroll
    for (int v = 0; v < NV; v++)
        *(bd_f4*)&tr[lane * BD_T_LD + 4 * v] = bd_f4{a[4 * v], a[4 * v + 1], a[4 * v + 2], a[4 * v + 3]};
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0); one wave: its LDS accesses stay in order
    const int rc = lane < n ? lane : 0;
    float lt[n + 1];
#pragma unroll
    for (int i = 0; i <= n; i++) {
        const float v = tr[i * BD_T_LD + rc];
        lt[i] = (i > lane || i == n) ? v : 0.f;   // L[i][r], i > r (the diagonal: rinv)
    }
    const float rinv = 1.0f / tr[rc * BD_T_LD + rc];
    // L^T x = z, j = n-1 .. 0: x_j = (z_j - s_j) / L[j][j], s_r = sum_{i > r} L[i][r] x_i.
    // Lanes r >= j add lt[j] = 0, so after the loop every lane's s is final and
    // (z - s) / L[r][r] is x_r, the value broadcast at step r.
    float sacc = 0.f;
#pragma unroll
    for (int j = n - 1; j >= 0; j--) {
        const float xj = rdl((lt[n] - sacc) * rinv, j);
        sacc += lt[j] * xj;
    }
    const float x = (lt[n] - sacc) * rinv;
    if (lane < n) {
        xs[lane] = x;
        p.dX[lane] = x;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (lane < NN) {
        float* P = p.poses + (int64_t)(p.t0 + lane) * 7;
        const float t0v[3] = {P[0], P[1], P[2]}, q0v[4] = {P[3], P[4], P[5], P[6]};
        float xi[6], t1v[3], q1v[4];
#pragma unroll
        for (int k = 0; k < 6; k++) xi[k] = xs[6 * lane + k];
        retrSE3(xi, t0v, q0v, t1v, q1v);
        P[0] = t1v[0]; P[1] = t1v[1]; P[2] = t1v[2];
        P[3] = q1v[0]; P[4] = q1v[1]; P[5] = q1v[2]; P[6] = q1v[3];
    }
}

static void bd_solve_launch(const BdParams& p, hipStream_t s)
{
    if (p.N > 10) {   // 11-12 poses: the workgroup solver
        hipLaunchKernelGGL(bd_solve_kernel, dim3(1), dim3(256), 0, s, p);
        return;
    }
    switch (p.N) {
#define BW_CASE(K) \
    case K: hipLaunchKernelGGL(bd_solve_wave_kernel<K>, dim3(1), dim3(64), 0, s, p); break;
        BW_CASE(1) BW_CASE(2) BW_CASE(3) BW_CASE(4) BW_CASE(5) BW_CASE(6) BW_CASE(7) BW_CASE(8) BW_CASE(9) BW_CASE(10)
#undef BW_CASE
    default: break;
    }
}

static int ba_forward_det(BdParams p, char* ws, const BdLayout& L, int64_t E, const int* csr_offs,
                          const int* csr_perm, const int64_t* csr_groups, int iterations, hipStream_t s)
{
    if (csr_offs && csr_perm && csr_groups) {
        p.offs = csr_offs;
        p.perm = csr_perm;
        p.groups = csr_groups;
    } else {
        int bits = 1;
        while (bits < 64 && (int64_t(1) << bits) < p.num_patches) bits++;
        if (dpvo_group_by(p.kk, E, bits, (int64_t*)(ws + L.gid), (int*)(ws + L.offs), (int*)(ws + L.perm),
                          (int64_t*)(ws + L.groups), ws + L.gbws, L.gbws_bytes, s) != 0)
            return -2;
        p.offs = (const int*)(ws + L.offs);
        p.perm = (const int*)(ws + L.perm);
        p.groups = (const int64_t*)(ws + L.groups);
    }
    p.E = E;
    p.erec = (bd_f4v*)(ws + L.erec);
    p.grec = (bd_i4v*)(ws + L.grec);
    hipLaunchKernelGGL(bd_prep_kernel, dim3(grid_for(E, 256, 2048)), dim3(256), 0, s, p);
    p.Em = (float*)(ws + L.Em);
    p.Cg = (float*)(ws + L.Cg);
    p.ug = (float*)(ws + L.ug);
    p.Hpart = (float*)(ws + L.Hpart);
    p.H = (float*)(ws + L.H);
    p.Hd = (float*)(ws + L.Hd);
    p.dX = (float*)(ws + L.dX);
    const size_t lds = (size_t)(BD_WAVES * (p.N > 0 ? (L.ent + 3) / 4 * 4 : 0) + BD_WAVES * BD_N6MAX) * 4 +
                       (size_t)(p.N > 0 ? (L.nup + 7) / 8 * 4 : 0) * 4 +
                       (size_t)(p.N > 0 ? BD_SLOTS * BD_SLOT_LD : 0) * 4;
    const unsigned gR = (unsigned)((L.ent + BR_E - 1) / BR_E);
    for (int it = 0; it < iterations; it++) {
        if (it == 0)
            hipLaunchKernelGGL((bd_patch_kernel<false, true>), dim3(bd_grid()), dim3(64 * BD_WAVES), lds, s, p);
        else
            hipLaunchKernelGGL((bd_patch_kernel<true, true>), dim3(bd_grid()), dim3(64 * BD_WAVES), lds, s, p);
        if (p.N > 0) {
            hipLaunchKernelGGL(bd_reduce_kernel, dim3(gR), dim3(1024), 0, s, p);   // (BD_GRID partials)
            bd_solve_launch(p, s);
        }
        DPVO_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((bd_patch_kernel<true, false>), dim3(bd_grid()), dim3(64 * BD_WAVES), 0, s, p);
    DPVO_CHECK_LAUNCH();
    return 0;
}

}  // namespace dpvo

using namespace dpvo;

static bool ba_sparse(int N, int flags) { return N > 0 && ((flags & DPVO_BA_SPARSE) || N > BA_SOLVE_NMAX); }
static bool ba_det(int N, int flags) { return !ba_sparse(N, flags) && N <= BD_NMAX && !(flags & DPVO_BA_ATOMIC); }

extern "C" size_t dpvo_ba_workspace_bytes_ex(int64_t num_edges, int64_t num_patches, int num_opt_poses, int flags)
{
    const int N = num_opt_poses < 0 ? 0 : num_opt_poses;
    if (ba_sparse(N, flags)) return bs_layout(num_edges, num_patches, N).total;
    if (ba_det(N, flags)) return bd_layout(num_edges, num_patches, N).total;
    return ba_layout(num_edges, num_patches, N).total;
}

extern "C" size_t dpvo_ba_workspace_bytes(int64_t num_edges, int64_t num_patches, int num_opt_poses)
{
    return dpvo_ba_workspace_bytes_ex(num_edges, num_patches, num_opt_poses, 0);
}

#ifdef DPVO_STAMPS
extern "C" int dpvo_diag_bd_stamps(void* host, size_t bytes)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dpvo_bd_stamps), std::min(bytes, sizeof(dpvo_bd_stamps)), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

// The one implementation behind the four dpvo_ba_forward* exports: the
// deterministic per-patch path, else the sparse band path, else the atomic
// dense path.  patches_est == NULL or prior_mu == 0: no depth prior.
extern "C" int dpvo_ba_forward_prior(float* poses, float* patches, int64_t num_patches, int P,
                                     const float* intrinsics, const float* target, const float* weight,
                                     const float* lmbda, const float* patches_est, float prior_mu, const int64_t* ii,
                                     const int64_t* jj, const int64_t* kk, int64_t num_edges, int t0, int t1,
                                     int iterations, int flags, const int* csr_offs, const int* csr_perm,
                                     const int64_t* csr_groups, void* workspace, size_t workspace_bytes, int* status,
                                     void* stream)
{
    const int N = t1 - t0;
    DPVO_CHECK_ARG(N >= 0, "t1 must be >= t0");
    DPVO_CHECK_ARG(N <= BS_NMAX, "more than 32767 optimised poses");
    DPVO_CHECK_ARG(P >= 1 && num_patches >= 0 && iterations >= 0, "bad sizes");
    DPVO_CHECK_ARG(prior_mu >= 0.f && prior_mu <= FLT_MAX, "prior_mu must be finite and >= 0");
    const float* est = prior_mu > 0.f ? patches_est : nullptr;
    hipStream_t s = as_stream(stream);
    char* ws = (char*)workspace;
    if (ba_det(N, flags)) {
        const BdLayout L = bd_layout(num_edges, num_patches, N);
        DPVO_CHECK_ARG(workspace && workspace_bytes >= L.total, "workspace too small");
        DPVO_CHECK_ARG(P * P <= 64, "patch size above 8");
        DPVO_CHECK_ARG(num_edges < 0x7fffffff, "too many edges");
        BdParams p{};
        p.poses = poses; p.patches = patches; p.intrinsics = intrinsics; p.target = target; p.weight = weight;
        p.lmbda = lmbda; p.ii = ii; p.jj = jj; p.kk = kk; p.num_patches = num_patches; p.mu_max = L.mu_max;
        p.P = P; p.t0 = t0; p.N = N; p.n6 = L.n6; p.nup = L.nup; p.ent = L.ent;
        p.est = est; p.mu = prior_mu;
        p.status = status ? status : (int*)(ws + L.hdr) + HDR_STATUS;
        // KEEP_STATUS: the caller's word may already hold a failure (the
        // tracker's window-key check); every bd_* kernel returns on entry when
        // it is non-zero, so the call then leaves poses and patches untouched
        if (!(status && (flags & DPVO_BA_KEEP_STATUS))) DPVO_CHECK_HIP(hipMemsetAsync(p.status, 0, sizeof(int), s));
        if (num_edges == 0 || iterations == 0) return 0;
        return ba_forward_det(p, ws, L, num_edges, csr_offs, csr_perm, csr_groups, iterations, s);
    }
    BaParams p{};
    p.poses = poses; p.patches = patches; p.intrinsics = intrinsics; p.target = target; p.weight = weight;
    p.lmbda = lmbda; p.ii = ii; p.jj = jj; p.kk = kk; p.E = num_edges; p.num_patches = num_patches;
    p.P = P; p.t0 = t0; p.N = N; p.n6 = 6 * N;
    p.est = est; p.mu = prior_mu;
    if (ba_sparse(N, flags)) {
        const BsLayout L = bs_layout(num_edges, num_patches, N);
        DPVO_CHECK_ARG(workspace && workspace_bytes >= L.total, "workspace too small");
        DPVO_CHECK_ARG(num_edges < 0x7fffffff, "too many edges");
        if (num_edges == 0 || iterations == 0) {
            if (status) DPVO_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
            return 0;
        }
        p.status = status;
        return ba_forward_sparse(p, ws, L, iterations, s);
    }
    const BaLayout L = ba_layout(num_edges, num_patches, N);
    DPVO_CHECK_ARG(workspace && workspace_bytes >= L.total, "workspace too small");
    p.hdr = (int*)(ws + L.hdr);
    p.status = status ? status : p.hdr + HDR_STATUS;
    p.red_iters = 2;   // wave-reduction rounds of the atomic path's Hessian (measured best)
    p.bits = (uint32_t*)(ws + L.bits);
    p.wordbase = (int*)(ws + L.wordbase);
    p.kx = (int*)(ws + L.kx);
    p.B = (float*)(ws + L.B); p.v = (float*)(ws + L.v); p.C = (float*)(ws + L.C); p.u = (float*)(ws + L.u);
    p.Em = (float*)(ws + L.E); p.S = (float*)(ws + L.S); p.y = (float*)(ws + L.y); p.dX = (float*)(ws + L.dX);
    p.Sd = (double*)(ws + L.Sd);
    p.yd = (double*)(ws + L.yd);
    p.Bpart = (float*)(ws + L.Bpart);
    p.nbH = L.nbH;
    if (num_edges == 0 || iterations == 0) {
        if (status) DPVO_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
        return 0;
    }
    DPVO_CHECK_HIP(hipMemsetAsync(ws + L.hdr, 0, L.wordbase - L.hdr, s));  // header + bitmap
    if (status) DPVO_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    const unsigned gE = grid_for(num_edges, 256, 2048);
    hipLaunchKernelGGL(ba_mark_kernel, dim3(gE), dim3(256), 0, s, p);
    hipLaunchKernelGGL(ba_scan_kernel, dim3(1), dim3(1024), 0, s, p, L.nwords);
    hipLaunchKernelGGL(ba_zero_kernel, dim3(256), dim3(256), 0, s, p);
    DPVO_CHECK_LAUNCH();
    const bool lds_b = N <= BA_LDS_NMAX;
    const size_t lds_h = lds_b ? (size_t)(p.n6 * p.n6 + p.n6) * 4 : 0;
    const unsigned gH = (unsigned)L.nbH;
    const unsigned gP = grid_for(L.mu_max, 256, 1024);
    const int sch = p.n6 <= 96 ? SCHUR_CHUNK : 16;
    const unsigned gS = (unsigned)std::min<int64_t>((L.mu_max + sch - 1) / sch, 512);
    const size_t lds_s = schur_lds_bytes(p.n6);
    const size_t lds_v = lds_b ? (size_t)(p.n6 * (p.n6 + 1) + p.n6) * 8 : 0;
    for (int it = 0; it < iterations; it++) {
        if (lds_b) {
            hipLaunchKernelGGL((ba_hessian_kernel<true, false>), dim3(gH), dim3(256), lds_h, s, p);
            if (p.n6 > 0)
                hipLaunchKernelGGL(ba_breduce_kernel, dim3((p.n6 * p.n6 + p.n6 + 63) / 64), dim3(1024), 0, s, p);
        } else
            hipLaunchKernelGGL((ba_hessian_kernel<false, false>), dim3(gH), dim3(256), 0, s, p);
        if (N > 0) {
            hipLaunchKernelGGL(ba_schur_kernel, dim3(gS), dim3(256), lds_s, s, p);
            if (p.n6 <= 64)
                hipLaunchKernelGGL(ba_solve_wave_kernel, dim3(1), dim3(64), 0, s, p);
            else
                hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(256), lds_v, s, p);
        }
        hipLaunchKernelGGL(ba_patch_kernel, dim3(gP), dim3(256), 0, s, p, N == 0 ? 1 : 0, it + 1 < iterations ? 1 : 0);
        DPVO_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int dpvo_ba_forward_csr(float* poses, float* patches, int64_t num_patches, int P, const float* intrinsics,
                                   const float* target, const float* weight, const float* lmbda, const int64_t* ii,
                                   const int64_t* jj, const int64_t* kk, int64_t num_edges, int t0, int t1,
                                   int iterations, int flags, const int* csr_offs, const int* csr_perm,
                                   const int64_t* csr_groups, void* workspace, size_t workspace_bytes, int* status,
                                   void* stream)
{
    return dpvo_ba_forward_prior(poses, patches, num_patches, P, intrinsics, target, weight, lmbda, nullptr, 0.f, ii,
                                 jj, kk, num_edges, t0, t1, iterations, flags, csr_offs, csr_perm, csr_groups,
                                 workspace, workspace_bytes, status, stream);
}

extern "C" int dpvo_ba_forward_ex(float* poses, float* patches, int64_t num_patches, int P, const float* intrinsics,
                                  const float* target, const float* weight, const float* lmbda, const int64_t* ii,
                                  const int64_t* jj, const int64_t* kk, int64_t num_edges, int t0, int t1,
                                  int iterations, int flags, void* workspace, size_t workspace_bytes, int* status,
                                  void* stream)
{
    return dpvo_ba_forward_prior(poses, patches, num_patches, P, intrinsics, target, weight, lmbda, nullptr, 0.f, ii,
                                 jj, kk, num_edges, t0, t1, iterations, flags, nullptr, nullptr, nullptr, workspace,
                                 workspace_bytes, status, stream);
}

extern "C" int dpvo_ba_forward(float* poses, float* patches, int64_t num_patches, int P, const float* intrinsics,
                               const float* target, const float* weight, const float* lmbda, const int64_t* ii,
                               const int64_t* jj, const int64_t* kk, int64_t num_edges, int t0, int t1,
                               int iterations, void* workspace, size_t workspace_bytes, int* status, void* stream)
{
    return dpvo_ba_forward_ex(poses, patches, num_patches, P, intrinsics, target, weight, lmbda, ii, jj, kk,
                              num_edges, t0, t1, iterations, 0, workspace, workspace_bytes, status, stream);
}

extern "C" int dpvo_reproject(const float* poses, const float* patches, int P, const float* intrinsics,
                              const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t num_edges,
                              float* coords, void* stream)
{
    DPVO_CHECK_ARG(P >= 1, "bad patch size");
    if (num_edges == 0) return 0;
    hipLaunchKernelGGL(reproject_kernel, dim3(grid_for(num_edges, 256)), dim3(256), 0, as_stream(stream), poses,
                       patches, P, intrinsics, ii, jj, kk, num_edges, coords);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_neighbors_workspace_bytes(int64_t num_edges)
{
    const size_t n = (size_t)(num_edges > 0 ? num_edges : 1);
    return align256(n * 8) * 2 + align256(n * 4) * 2 + align256(nb_sort_temp_bytes(num_edges > 0 ? num_edges : 1));
}

extern "C" int dpvo_neighbors(const int64_t* ii, const int64_t* jj, int64_t num_edges, int64_t* ix, int64_t* jx,
                              void* workspace, size_t workspace_bytes, void* stream)
{
    if (num_edges == 0) return 0;
    DPVO_CHECK_ARG(num_edges < 0x7fffffff, "too many edges");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_neighbors_workspace_bytes(num_edges), "workspace too small");
    hipStream_t s = as_stream(stream);
    const size_t n = (size_t)num_edges;
    char* ws = (char*)workspace;
    uint64_t* k_in = (uint64_t*)ws;
    uint64_t* k_out = (uint64_t*)(ws + align256(n * 8));
    int* v_in = (int*)(ws + 2 * align256(n * 8));
    int* v_out = (int*)(ws + 2 * align256(n * 8) + align256(n * 4));
    void* tmp = ws + 2 * align256(n * 8) + 2 * align256(n * 4);
    size_t tmp_bytes = nb_sort_temp_bytes(num_edges);
    const unsigned g = grid_for(num_edges, 256, 2048);
    hipLaunchKernelGGL(nb_keys_kernel, dim3(g), dim3(256), 0, s, ii, jj, num_edges, k_in, v_in);
    DPVO_CHECK_LAUNCH();
    DPVO_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, k_in, k_out, v_in, v_out, (int)num_edges, 0, 64, s));
    hipLaunchKernelGGL(nb_link_kernel, dim3(g), dim3(256), 0, s, k_out, v_out, num_edges, ix, jx);
    DPVO_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// cuda_ba.solve_system (ba.cpp:174-234): loop-closure pose-graph normal
// equations.  J (7r x 7n) has per-edge 7x7 blocks J_i at (x, i) and J_j at
// (x, j); A = J^T J and b = -J^T res in fp64 (the reference's Eigen double
// sparse matrices), diag(A) <- diag(A) (1 + lm) + ep.  Rows / columns >= m
// (= 7 * freen, or 7n) are dropped: the reference solves only the top-left
// block there.  One thread per (edge, 7x7 output entry); fp64 atomics.
// ---------------------------------------------------------------------------
namespace dpvo {
__global__ __launch_bounds__(256) void ss_assemble_kernel(const float* __restrict__ Ji, const float* __restrict__ Jj,
                                                          const int64_t* __restrict__ ii,
                                                          const int64_t* __restrict__ jj,
                                                          const float* __restrict__ res, int64_t r, int64_t m,
                                                          double* __restrict__ A, double* __restrict__ b,
                                                          int* __restrict__ status)
{
    const int64_t total = r * 49;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x = t / 49;
        const int kl = (int)(t - x * 49), k = kl / 7, l = kl - k * 7;   // output entry (row l of block, column k)
        const int64_t i = ii[x], j = jj[x];
        if (i == j) {   // the reference calls exit(1) here (ba.cpp:205-206)
            atomicExch(status, 1);
            continue;
        }
        const float* Ai = Ji + x * 49;
        const float* Aj = Jj + x * 49;
        // (J^T J) entries: sum over the 7 residual rows q of J[q][l] J[q][k]
        double sii = 0, sjj = 0, sij = 0, sji = 0;
#pragma unroll
        for (int q = 0; q < 7; q++) {
            const double il = Ai[q * 7 + l], ik = Ai[q * 7 + k], jl = Aj[q * 7 + l], jk = Aj[q * 7 + k];
            sii += il * ik;
            sjj += jl * jk;
            sij += il * jk;
            sji += jl * ik;
        }
        const int64_t ri = 7 * i + l, rj = 7 * j + l, ci = 7 * i + k, cj = 7 * j + k;
        if (ri < m && ci < m) atomicAdd(&A[ri * m + ci], sii);
        if (rj < m && cj < m) atomicAdd(&A[rj * m + cj], sjj);
        if (ri < m && cj < m) atomicAdd(&A[ri * m + cj], sij);
        if (rj < m && ci < m) atomicAdd(&A[rj * m + ci], sji);
        if (k == 0) {   // b = -J^T res, row l of both blocks
            double bi = 0, bj = 0;
#pragma unroll
            for (int q = 0; q < 7; q++) {
                const double rq = res[x * 7 + q];
                bi += Ai[q * 7 + l] * rq;
                bj += Aj[q * 7 + l] * rq;
            }
            if (ri < m) atomicAdd(&b[ri], -bi);
            if (rj < m) atomicAdd(&b[rj], -bj);
        }
    }
}

__global__ __launch_bounds__(256) void ss_damp_kernel(double* A, int64_t m, double ep, double lm)
{
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < m; d += (int64_t)gridDim.x * blockDim.x) {
        double& a = A[d * m + d];
        a = a + a * lm + ep;
    }
}
}  // namespace dpvo

extern "C" int dpvo_solve_system_assemble(const float* J_i, const float* J_j, const int64_t* ii, const int64_t* jj,
                                          const float* res, int64_t r, int64_t m, float ep, float lm, double* A,
                                          double* b, int* status, void* stream)
{
    DPVO_CHECK_ARG(r >= 0 && m >= 0, "bad sizes");
    DPVO_CHECK_ARG(m == 0 || (A && b), "A / b missing");
    hipStream_t s = as_stream(stream);
    if (m > 0) {
        DPVO_CHECK_HIP(hipMemsetAsync(A, 0, (size_t)(m * m) * sizeof(double), s));
        DPVO_CHECK_HIP(hipMemsetAsync(b, 0, (size_t)m * sizeof(double), s));
    }
    if (status) DPVO_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    if (r > 0 && m > 0) {
        hipLaunchKernelGGL(ss_assemble_kernel, dim3(grid_for(r * 49, 256, 8192)), dim3(256), 0, s, J_i, J_j, ii, jj,
                           res, r, m, A, b, status);
    }
    if (m > 0) hipLaunchKernelGGL(ss_damp_kernel, dim3(grid_for(m, 256, 1024)), dim3(256), 0, s, A, m, (double)ep,
                                  (double)lm);
    DPVO_CHECK_LAUNCH();
    return 0;
}
