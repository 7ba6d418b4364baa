// fastba.hpp -- what the bundle-adjustment translation units share: the call
// record and the three path drivers (fastba.hip dispatches; fastba_det.hip and
// fastba_atomic.hip implement), and the per-edge / per-pose / per-patch
// arithmetic every solver path uses.  The library is built without relocatable
// device code, so the device side is all __forceinline__.  Not liegroups.hpp:
// its SE3<float> is different arithmetic (geometry.hip's).
#pragma once

#include "common.hpp"

namespace dpvo {

constexpr int HDR_MU = 0, HDR_STATUS = 1, HDR_BW = 2, HDR_WORDS = 16;   // workspace header words
constexpr int BA_SOLVE_NMAX = 64;  // atomic path: up to 384 x 384 (fp64 Cholesky in global scratch beyond its LDS)
constexpr int BD_NMAX = 12;        // deterministic path: DPVO's sliding window
constexpr int BS_NMAX = 32767;     // band path: pose keys are packed as 16-bit pairs in the Schur reduction

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline bool ba_sparse(int N, int flags) { return N > 0 && ((flags & DPVO_BA_SPARSE) || N > BA_SOLVE_NMAX); }
static inline bool ba_det(int N, int flags) { return !ba_sparse(N, flags) && N <= BD_NMAX && !(flags & DPVO_BA_ATOMIC); }

// one dpvo_ba_forward* call, as its entry point received it
struct BaCall {
    float *poses, *patches;
    const float *intrinsics, *target, *weight, *lmbda;
    const float* est;   // depth prior [num_patches][3][P][P], channel 2 at the centre pixel; nullptr = the plain call
    float mu;
    const int64_t *ii, *jj, *kk;
    int64_t E, num_patches;
    int P, t0, N;
    int* status;        // the caller's status word or nullptr (then the workspace header's)
    int flags;
    const int *csr_offs, *csr_perm;   // caller's kk group-by (deterministic path), all three or none
    const int64_t* csr_groups;
};

// The drivers check their own preconditions but report under the entry point's name.
#define BA_CHECK_ARG(cond, msg)                                                   \
    do {                                                                          \
        if (!(cond)) {                                                            \
            ::dpvo::set_error(std::string("dpvo_ba_forward_prior: ") + (msg));    \
            return -1;                                                            \
        }                                                                         \
    } while (0)

// det: deterministic per-patch path; atomic: dense atomic path; band: large pose windows
size_t det_workspace_bytes(int64_t E, int64_t num_patches, int N);
size_t atomic_workspace_bytes(int64_t E, int64_t num_patches, int N);
size_t band_workspace_bytes(int64_t E, int64_t num_patches, int N);
int det_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s);
int atomic_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s);
int band_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s);

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

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

// left retraction of one stored pose (t, q) by xi (ba_cuda.cu:160-188)
__device__ __forceinline__ void ba_retract_pose(float* P, const float xi[6])
{
    const float t0v[3] = {P[0], P[1], P[2]}, q0v[4] = {P[3], P[4], P[5], P[6]};
    float t1v[3], q1v[4];
    retrSE3(xi, t0v, q0v, t1v, q1v);
    P[0] = t1v[0]; P[1] = t1v[1]; P[2] = t1v[2];
    P[3] = q1v[0]; P[4] = q1v[1]; P[5] = q1v[2]; P[6] = q1v[3];
}

// clamped additive update of an inverse depth (ba_cuda.cu:191-211)
__device__ __forceinline__ float ba_depth_step(float d, float dZ)
{
    d += dZ;
    d = (d > 20.f) ? 1.0f : d;
    return fmaxf(d, 1e-4f);
}

// Depth prior of the reference's Python BA (dpvo/ba.py:151-159): a patch at
// inverse depth d with a prior est adds mu to C and -mu (d - est) to u before
// Q = 1 / (C + lmbda) is formed.  Valid is 0 < est < +inf: the reference's
// est > 0 alone lets 1 / median(depth) = inf through, and the depth turns NaN.
__device__ __forceinline__ bool prior_valid(float est) { return est > 0.f && est < __builtin_inff(); }
__device__ __forceinline__ void ba_prior_terms(float est, float d, float mu, float& C, float& u)
{
    if (prior_valid(est)) {
        C += mu;
        u -= mu * (d - est);
    }
}

// per-edge residual, validity mask and Jacobians of one residual pair
// (ba_cuda.cu:254-290, 326-330); ix / jx index the window of N poses from t0
struct BaEdge {
    float Ji[2][6], Jj[2][6], Jz[2], w[2], r[2];
    int ix, jx;
    bool iv, jv, self;
};

// Edge (i_abs -> j_abs) of the patch point (px, py, inverse depth dk), target
// (tx, ty), weights (w0, w1).  valid = false (an edge the caller discards)
// clears the mask and iv / jv.
__device__ __forceinline__ void ba_edge(const float* poses, int64_t i_abs, int64_t j_abs, float px, float py,
                                        float dk, float tx, float ty, float w0, float w1, float fx, float fy,
                                        float cx, float cy, int t0, int N, bool valid, BaEdge& o)
{
    const float* Pi = poses + i_abs * 7;
    const float* Pj = poses + j_abs * 7;
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
    const float rx = tx - x1, ry = ty - y1;
    const bool in_bounds = (sqrtf(rx * rx + ry * ry) < 128.f) && (Z > 0.2f) && (x1 > -64.f) && (y1 > -64.f) &&
                           (x1 < 2.f * cx + 64.f) && (y1 < 2.f * cy + 64.f);
    const float mask = (in_bounds && valid) ? 1.0f : 0.0f;
    o.w[0] = mask * w0;
    o.w[1] = mask * w1;
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
    o.ix = (int)(i_abs - t0);
    o.jx = (int)(j_abs - t0);
    o.iv = valid && o.ix >= 0 && o.ix < N;
    o.jv = valid && o.jx >= 0 && o.jx < N;
    o.self = o.iv && o.jv && o.ix == o.jx;
}

// the edge's terms on its patch: E rows of frames i and j, C, u
__device__ __forceinline__ void ba_edge_patch_terms(const BaEdge& o, float Ei[6], float Ej[6], float& Ck, float& uk)
{
    Ck = 0.f;
    uk = 0.f;
#pragma unroll
    for (int t = 0; t < 6; t++) { Ei[t] = 0.f; Ej[t] = 0.f; }
#pragma unroll
    for (int row = 0; row < 2; row++) {
#pragma unroll
        for (int t = 0; t < 6; t++) {
            Ei[t] += -o.w[row] * o.Jz[row] * o.Ji[row][t];
            Ej[t] += o.w[row] * o.Jz[row] * o.Jj[row][t];
        }
        Ck += o.w[row] * o.Jz[row] * o.Jz[row];
        uk += o.w[row] * o.r[row] * o.Jz[row];
    }
}

}  // namespace dpvo
