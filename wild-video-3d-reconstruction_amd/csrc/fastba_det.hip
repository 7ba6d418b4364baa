// fastba_det.hip -- the deterministic dense bundle-adjustment path (bd_*):
// DPVO's sliding window (N <= 12 optimised poses), what the tracker runs every
// update.  See fastba.hip for the algebra and the dispatch.
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
#include <algorithm>
#include <type_traits>

#include "fastba.hpp"

namespace dpvo {

typedef float bd_f4v __attribute__((ext_vector_type(4)));
typedef int bd_i4v __attribute__((ext_vector_type(4)));
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

// the edge of CSR record (r0, r1) = ((i, j, target), (weight, -, -)), bd_prep_kernel's gather
__device__ __forceinline__ void bd_edge(const BdParams& p, const bd_f4v r0, const bd_f4v r1, float px, float py,
                                        float dk, float fx, float fy, float cx, float cy, BaEdge& o)
{
    ba_edge(p.poses, __float_as_int(r0[0]), __float_as_int(r0[1]), px, py, dk, r0[2], r0[3], r1[0], r1[1], fx, fy, cx,
            cy, p.t0, p.N, true, o);
}

// the terms of one edge on the patch's own frame i (a self edge folds its
// j terms in, ba_cuda.cu:294-322): (i, i) upper block, v_i, E_i
__device__ __forceinline__ void bd_iterms(const BaEdge& o, float bii[21], float vi[6], float Ei[6])
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
__device__ __forceinline__ void bd_jterms_add(const BaEdge& o, float* part, float* ev, int n6, int nup)
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
        // every edge's patch index, not only each group's first: the group-by
        // keeps the low bits of kk, so an index past the end can share a group
        // with a valid patch
        const int64_t k = p.kk[e];
        if (k < 0 || k >= p.num_patches) atomicExch(p.status, -1);
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
            const float d = ba_depth_step(pd[0], Q * (p.ug[g] - s));
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
            BaEdge o;
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
        ba_prior_terms(est, dk, p.mu, Ck, uk);
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
        float xi[6];
        for (int k = 0; k < 6; k++) xi[k] = xs[6 * tid + k];
        ba_retract_pose(p.poses + (int64_t)(p.t0 + tid) * 7, xi);
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
        float xi[6];
#pragma unroll
        for (int k = 0; k < 6; k++) xi[k] = xs[6 * lane + k];
        ba_retract_pose(p.poses + (int64_t)(p.t0 + lane) * 7, xi);
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

size_t det_workspace_bytes(int64_t E, int64_t num_patches, int N) { return bd_layout(E, num_patches, N).total; }

int det_forward(const BaCall& c, char* ws, size_t ws_bytes, int iterations, hipStream_t s)
{
    const BdLayout L = bd_layout(c.E, c.num_patches, c.N);
    BA_CHECK_ARG(ws && ws_bytes >= L.total, "workspace too small");
    BA_CHECK_ARG(c.P * c.P <= 64, "patch size above 8");
    BA_CHECK_ARG(c.E < 0x7fffffff, "too many edges");
    BdParams p{};
    p.poses = c.poses; p.patches = c.patches; p.intrinsics = c.intrinsics; p.target = c.target; p.weight = c.weight;
    p.lmbda = c.lmbda; p.ii = c.ii; p.jj = c.jj; p.kk = c.kk; p.E = c.E; p.num_patches = c.num_patches;
    p.mu_max = L.mu_max; p.P = c.P; p.t0 = c.t0; p.N = c.N; p.n6 = L.n6; p.nup = L.nup; p.ent = L.ent;
    p.est = c.est; p.mu = c.mu;
    p.status = c.status ? c.status : (int*)(ws + L.hdr) + HDR_STATUS;
    // KEEP_STATUS: the caller's word may already hold a failure (the
    // tracker's window-key check); every bd_* kernel returns on entry when
    // it is non-zero, so the call then leaves poses and patches untouched
    if (!(c.status && (c.flags & DPVO_BA_KEEP_STATUS))) DPVO_CHECK_HIP(hipMemsetAsync(p.status, 0, sizeof(int), s));
    if (c.E == 0 || iterations == 0) return 0;
    if (c.csr_offs && c.csr_perm && c.csr_groups) {
        p.offs = c.csr_offs;
        p.perm = c.csr_perm;
        p.groups = c.csr_groups;
    } else {
        int bits = 1;
        while (bits < 64 && (int64_t(1) << bits) < p.num_patches) bits++;
        if (dpvo_group_by(p.kk, c.E, bits, (int64_t*)(ws + L.gid), (int*)(ws + L.offs), (int*)(ws + L.perm),
                          (int64_t*)(ws + L.groups), ws + L.gbws, L.gbws_bytes, s) != 0)
            return -2;
        p.offs = (const int*)(ws + L.offs);
        p.perm = (const int*)(ws + L.perm);
        p.groups = (const int64_t*)(ws + L.groups);
    }
    p.erec = (bd_f4v*)(ws + L.erec);
    p.grec = (bd_i4v*)(ws + L.grec);
    hipLaunchKernelGGL(bd_prep_kernel, dim3(grid_for(c.E, 256, 2048)), dim3(256), 0, s, p);
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
            hipLaunchKernelGGL((bd_patch_kernel<false, true>), dim3(BD_GRID), dim3(64 * BD_WAVES), lds, s, p);
        else
            hipLaunchKernelGGL((bd_patch_kernel<true, true>), dim3(BD_GRID), dim3(64 * BD_WAVES), lds, s, p);
        if (p.N > 0) {
            hipLaunchKernelGGL(bd_reduce_kernel, dim3(gR), dim3(1024), 0, s, p);   // (BD_GRID partials)
            bd_solve_launch(p, s);
        }
        DPVO_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((bd_patch_kernel<true, false>), dim3(BD_GRID), dim3(64 * BD_WAVES), 0, s, p);
    DPVO_CHECK_LAUNCH();
    return 0;
}

}  // namespace dpvo

#ifdef DPVO_STAMPS
extern "C" int dpvo_diag_bd_stamps(void* host, size_t bytes)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dpvo::dpvo_bd_stamps), std::min(bytes, sizeof(dpvo::dpvo_bd_stamps)), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
