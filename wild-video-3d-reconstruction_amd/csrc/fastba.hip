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
// This file: the C entry points, their argument checks and the dispatch over
// the three solver paths (the deterministic per-patch path, fastba_det.hip;
// the dense atomic and the band path, fastba_atomic.hip; shared arithmetic in
// fastba.hpp), and reproject, neighbors and the solve_system assembly.
#include <cfloat>

#include <hipcub/hipcub.hpp>

#include "fastba.hpp"

namespace dpvo {
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

}  // namespace dpvo

using namespace dpvo;

extern "C" size_t dpvo_ba_workspace_bytes_ex(int64_t num_edges, int64_t num_patches, int num_opt_poses, int flags)
{
    const int N = num_opt_poses < 0 ? 0 : num_opt_poses;
    if (ba_sparse(N, flags)) return band_workspace_bytes(num_edges, num_patches, N);
    if (ba_det(N, flags)) return det_workspace_bytes(num_edges, num_patches, N);
    return atomic_workspace_bytes(num_edges, num_patches, N);
}

extern "C" size_t dpvo_ba_workspace_bytes(int64_t num_edges, int64_t num_patches, int num_opt_poses)
{
    return dpvo_ba_workspace_bytes_ex(num_edges, num_patches, num_opt_poses, 0);
}

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
    BaCall c{};
    c.poses = poses; c.patches = patches; c.intrinsics = intrinsics; c.target = target; c.weight = weight;
    c.lmbda = lmbda; c.est = prior_mu > 0.f ? patches_est : nullptr; c.mu = prior_mu;
    c.ii = ii; c.jj = jj; c.kk = kk; c.E = num_edges; c.num_patches = num_patches;
    c.P = P; c.t0 = t0; c.N = N; c.status = status; c.flags = flags;
    c.csr_offs = csr_offs; c.csr_perm = csr_perm; c.csr_groups = csr_groups;
    const auto forward = ba_det(N, flags) ? det_forward : ba_sparse(N, flags) ? band_forward : atomic_forward;
    return forward(c, (char*)workspace, workspace_bytes, iterations, as_stream(stream));
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
