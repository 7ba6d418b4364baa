// fastba_atomic.hip -- the two bundle-adjustment paths that sum with device
// atomics (see fastba.hip for the algebra): the dense path (ba_*: windows of up
// to 64 poses, DPVO_BA_ATOMIC) and the band path for global BA (bs_*: large
// pose windows, below).  They share the unique-patch bitmap (mark / scan /
// unique_rank) and ba_hessian_kernel.  Neither is bitwise repeatable.
//
// Dense path (no host synchronisation inside the call):
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

#include <hipcub/hipcub.hpp>

#include "fastba.hpp"

namespace dpvo {

// ---------------------------------------------------------------------------
// workspace layout
// ---------------------------------------------------------------------------
constexpr int BA_LDS_NMAX = 12;  // optimised poses whose B fits in LDS (72x72 fp32)
constexpr int BS_TILE = 64;      // tile edge of the banded reduced camera system

struct BaLayout {
    size_t hdr, bits, wordbase, kx, B, v, C, u, E, S, y, dX, Sd, yd, Bpart, total;
    int nbH;   // Hessian workgroups (each leaves one partial B / v in Bpart)
    int64_t nwords, mu_max;
    int n6;
};

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

// the depth prior's terms of unique patch k, added to its C / u (the plain call: nothing)
__device__ __forceinline__ void prior_add(const BaParams& p, int64_t k, float& C, float& u)
{
    if (p.est == nullptr) return;
    const int64_t PP = (int64_t)p.P * p.P, at = ((int64_t)p.kx[k] * 3 + 2) * PP + (p.P / 2) * p.P + p.P / 2;
    ba_prior_terms(p.est[at], p.patches[at], p.mu, C, u);
}

// dense path: the prior enters C / u once, as the value the accumulators of
// unique patch k start an iteration from (0 without a prior)
__device__ __forceinline__ void prior_seed(const BaParams& p, int64_t k, float& C0, float& u0)
{
    C0 = 0.f;
    u0 = 0.f;
    prior_add(p, k, C0, u0);
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
        const float* pa = p.patches + kc * 3 * PP + centre;
        // both residual rows, summed per destination
        BaEdge o;
        ba_edge(p.poses, p.ii[ne], p.jj[ne], pa[0], pa[PP], pa[2 * PP], p.target[ne * 2 + 0], p.target[ne * 2 + 1],
                p.weight[ne * 2 + 0], p.weight[ne * 2 + 1], fx, fy, cx, cy, p.t0, p.N, valid, o);
        const int ix = o.ix, jx = o.jx;
        const bool iv = o.iv, jv = o.jv, self = o.self;
        const auto &Ji = o.Ji, &Jj = o.Jj;
        const auto &w = o.w, &r = o.r;

        // patch terms: E rows (device atomics; a wave's lanes mostly hold different patches), C, u
        if constexpr (SPARSE) {
            if (n < p.E) {
                float Ei[6], Ej[6], Ck, uk;
                ba_edge_patch_terms(o, Ei, Ej, Ck, uk);
                const float z = 0.f;
                float4* dst = reinterpret_cast<float4*>(p.ent + n * 16);
                dst[0] = make_float4(iv ? Ei[0] : z, iv ? Ei[1] : z, iv ? Ei[2] : z, iv ? Ei[3] : z);
                dst[1] = make_float4(iv ? Ei[4] : z, iv ? Ei[5] : z, jv ? Ej[0] : z, jv ? Ej[1] : z);
                dst[2] = make_float4(jv ? Ej[2] : z, jv ? Ej[3] : z, jv ? Ej[4] : z, jv ? Ej[5] : z);
                dst[3] = make_float4(valid ? Ck : z, valid ? uk : z, z, z);
            }
        } else if (valid) {
            float Ei[6], Ej[6], Ck, uk;
            ba_edge_patch_terms(o, Ei, Ej, Ck, uk);
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
        float xi[6];
        for (int k = 0; k < 6; k++) xi[k] = (float)yv[6 * i + k];
        ba_retract_pose(p.poses + (int64_t)(p.t0 + i) * 7, xi);
    }
    for (int i = tid; i < n * n; i += nthreads) { p.B[i] = 0.f; p.S[i] = 0.f; }
    for (int i = tid; i < n; i += nthreads) { p.v[i] = 0.f; p.y[i] = 0.f; }
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
        const float d = ba_depth_step(pd[0], dZ);
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
        if (live) prior_add(p, k, C, u);   // before Q, Qk and uk are formed
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
        float xi[6];
        for (int k = 0; k < 6; k++) xi[k] = (float)p.ys[6 * i + k];
        ba_retract_pose(p.poses + (int64_t)(p.t0 + i) * 7, xi);
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
        const float d = ba_depth_step(pd[0], dZ);
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

// the call's operands and sizes; the workspace pointers are the driver's to set
static BaParams ba_params(const BaCall& c)
{
    BaParams p{};
    p.poses = c.poses; p.patches = c.patches; p.intrinsics = c.intrinsics; p.target = c.target; p.weight = c.weight;
    p.lmbda = c.lmbda; p.ii = c.ii; p.jj = c.jj; p.kk = c.kk; p.E = c.E; p.num_patches = c.num_patches;
    p.P = c.P; p.t0 = c.t0; p.N = c.N; p.n6 = 6 * c.N;
    p.est = c.est; p.mu = c.mu;
    p.red_iters = 2;   // wave-reduction rounds of the Hessian's pose-block terms (measured best)
    return p;
}

size_t band_workspace_bytes(int64_t E, int64_t num_patches, int N) { return bs_layout(E, num_patches, N).total; }

int band_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s)
{
    const BsLayout L = bs_layout(c.E, c.num_patches, c.N);
    BA_CHECK_ARG(ws && ws_bytes >= L.total, "workspace too small");
    BA_CHECK_ARG(c.E < 0x7fffffff, "too many edges");
    if (c.E == 0 || iterations == 0) {
        if (c.status) DPVO_CHECK_HIP(hipMemsetAsync(c.status, 0, sizeof(int), s));
        return 0;
    }
    BaParams p = ba_params(c);
    p.hdr = (int*)(ws + L.hdr);
    p.status = c.status ? c.status : p.hdr + HDR_STATUS;
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
        for (int tc = 0; tc < L.T; tc++) {   // tile columns
            hipLaunchKernelGGL(bs_potrf_kernel, dim3(1), dim3(64), 0, s, p, tc);
            const int nb = std::min(p.bt, L.T - 1 - tc);
            if (nb > 0) {
                hipLaunchKernelGGL(bs_trsm_kernel, dim3(nb), dim3(64), 0, s, p, tc);
                hipLaunchKernelGGL(bs_syrk_kernel, dim3(nb * (nb + 1) / 2), dim3(256), 0, s, p, tc);
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

size_t atomic_workspace_bytes(int64_t E, int64_t num_patches, int N) { return ba_layout(E, num_patches, N).total; }

int atomic_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s)
{
    const BaLayout L = ba_layout(c.E, c.num_patches, c.N);
    BA_CHECK_ARG(ws && ws_bytes >= L.total, "workspace too small");
    if (c.E == 0 || iterations == 0) {
        if (c.status) DPVO_CHECK_HIP(hipMemsetAsync(c.status, 0, sizeof(int), s));
        return 0;
    }
    BaParams p = ba_params(c);
    const int N = c.N;
    p.hdr = (int*)(ws + L.hdr);
    p.status = c.status ? c.status : p.hdr + HDR_STATUS;
    p.bits = (uint32_t*)(ws + L.bits);
    p.wordbase = (int*)(ws + L.wordbase);
    p.kx = (int*)(ws + L.kx);
    p.B = (float*)(ws + L.B); p.v = (float*)(ws + L.v); p.C = (float*)(ws + L.C); p.u = (float*)(ws + L.u);
    p.Em = (float*)(ws + L.E); p.S = (float*)(ws + L.S); p.y = (float*)(ws + L.y); p.dX = (float*)(ws + L.dX);
    p.Sd = (double*)(ws + L.Sd);
    p.yd = (double*)(ws + L.yd);
    p.Bpart = (float*)(ws + L.Bpart);
    p.nbH = L.nbH;
    DPVO_CHECK_HIP(hipMemsetAsync(ws + L.hdr, 0, L.wordbase - L.hdr, s));  // header + bitmap
    if (c.status) DPVO_CHECK_HIP(hipMemsetAsync(c.status, 0, sizeof(int), s));
    const unsigned gE = grid_for(c.E, 256, 2048);
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

}  // namespace dpvo
