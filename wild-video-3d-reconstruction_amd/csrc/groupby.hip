// groupby.hip -- the tracker's edge bookkeeping (gfx950): the sync-free group-by on its radix and
// counting-sort paths, the per-update window keys and the fused window group-by, the correlation's
// target-frame edge order, the CSR neighbours and the edge append.  The only unit that includes hipcub.
#include <climits>
#include <cstdlib>

#include <hipcub/hipcub.hpp>

#include "updateop.hpp"

namespace dpvo {
namespace {

// ---------------------------------------------------------------------------
// sync-free group-by (torch.unique(key, return_inverse=True) + CSR)
// ---------------------------------------------------------------------------
// keys as unsigned radix-sort keys: 32-bit when the caller's bound fits
// (fewer radix passes), 64-bit otherwise (any int64 key; negative keys sort
// after the non-negative ones but still group by equality)
template <typename K>
__global__ __launch_bounds__(256) void gb_keys_kernel(const int64_t* __restrict__ key, int64_t n,
                                                      K* __restrict__ kout, int* __restrict__ idx)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        kout[e] = (K)key[e];
        idx[e] = (int)e;
    }
}

template <typename K>
__global__ __launch_bounds__(256) void gb_flags_kernel(const K* __restrict__ sk, int64_t n, int* __restrict__ flag)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        flag[i] = (i == 0 || sk[i] != sk[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void gb_finish_kernel(const int* __restrict__ flag, const int* __restrict__ incl,
                                                        const int* __restrict__ perm, int64_t n,
                                                        int64_t* __restrict__ gid, int* __restrict__ offs,
                                                        int64_t* __restrict__ groups)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = incl[i] - 1;
        gid[perm[i]] = r;
        if (flag[i]) offs[r] = (int)i;
        if (i == n - 1) {
            offs[r + 1] = (int)n;
            *groups = r + 1;
        }
    }
}

struct GbLayout {
    int64_t k_in, k_out, v_in, flag, incl, tmp, tmp_bytes, total;
};

size_t gb_tmp_bytes(int64_t n)
{
    size_t a = 0, a64 = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr,
                                             (int*)nullptr, (int)n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a64, (uint64_t*)nullptr, (uint64_t*)nullptr, (int*)nullptr,
                                             (int*)nullptr, (int)n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (int*)nullptr, (int*)nullptr, (int)n);
    return std::max(std::max(a, a64), b);
}

GbLayout gb_layout(int64_t n)
{
    GbLayout L;
    int64_t o = 0;
    L.k_in = o;  o += align256(8 * n);
    L.k_out = o; o += align256(8 * n);
    L.v_in = o;  o += align256(4 * n);
    L.flag = o;  o += align256(4 * n);
    L.incl = o;  o += align256(4 * n);
    L.tmp = o;
    L.tmp_bytes = (int64_t)gb_tmp_bytes(n);
    o += align256(L.tmp_bytes);
    L.total = o;
    return L;
}

// Counting-sort group-by for keys bounded by 2^key_bits <= 2^22 (the tracker's
// kk < N M and its dense (ii, jj) pair key): a histogram with atomic slots, one
// exclusive scan over the bins carrying (start, group index) together, a
// scatter, and a per-group fix-up that restores ascending edge order inside
// each group (the atomic slots are arrival order) -- the same outputs as the
// stable radix sort, in 5 launches instead of ~12 (the radix path's merge
// passes, flags, scan and finish kernels).
constexpr int CB_MAX_BITS = 22;

struct CbLayout {
    int64_t hist, pre, slot, ptmp, tmp, tmp_bytes, total;
};

struct CbCombine {
    __host__ __device__ int64_t operator()(int c) const { return (int64_t)c | ((int64_t)(c > 0) << 32); }
};

CbLayout cb_layout(int64_t n, int key_bits)
{
    const int64_t B = int64_t(1) << key_bits;
    CbLayout L;
    int64_t o = 0;
    L.hist = o; o += align256(4 * B);
    L.pre = o;  o += align256(8 * B);
    L.slot = o; o += align256(4 * n);
    L.ptmp = o; o += align256(4 * n);
    L.tmp = o;
    size_t tb = 0;
    hipcub::TransformInputIterator<int64_t, CbCombine, const int*> it(nullptr, CbCombine());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, it, (int64_t*)nullptr, (int)B);
    L.tmp_bytes = (int64_t)tb;
    o += align256(L.tmp_bytes);
    L.total = o;
    return L;
}

// runs of equal keys inside a wave take one atomic per run (the run head's),
// so bins hit by many consecutive edges do not serialise on one address.
// Called by whole waves (uniform trip counts); valid lanes are a prefix.
__device__ __forceinline__ int cb_run_slot(uint32_t k, bool valid, int lane, int* __restrict__ hist)
{
    const uint32_t prev = __shfl_up(k, 1);
    const bool head = valid && (lane == 0 || prev != k);
    const uint64_t hm = __ballot(head), vm = __ballot(valid);
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
    const int hl = 63 - __clzll(hm & upto);                  // my run's head lane
    const uint64_t above = hm & ~upto;
    const int end = above ? __ffsll((long long)above) - 1 : 64 - __clzll(vm);
    int base = 0;
    if (head) base = atomicAdd(&hist[k], end - lane);
    base = __shfl(base, valid ? hl : 0);
    return base + (lane - hl);
}

__global__ __launch_bounds__(256) void cb_hist_kernel(const int64_t* __restrict__ key, int64_t n, uint32_t mask,
                                                      int* __restrict__ hist, int* __restrict__ slot)
{
    const int lane = threadIdx.x & 63;
    for (int64_t e0 = blockIdx.x * (int64_t)blockDim.x; e0 < n; e0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = e0 + threadIdx.x;   // uniform trip count: whole waves stay converged
        const bool valid = e < n;
        const uint32_t k = valid ? (uint32_t)key[e] & mask : 0xffffffffu;
        const int s = cb_run_slot(k, valid, lane, hist);
        if (valid) slot[e] = s;
    }
}

// The placement step of the counting sort: edge e, the s-th arrival in bin k,
// goes to its bin's start + s; the bin's scanned entry carries (start, group
// index) together, and the first arrival records the group's start.
__device__ __forceinline__ void cb_place(const int64_t* __restrict__ pre, uint32_t k, int s, int64_t e,
                                         int* __restrict__ ptmp, int64_t* __restrict__ gid, int* __restrict__ offs)
{
    const int64_t p = pre[k];
    const int start = (int)(p & 0xffffffff), g = (int)(p >> 32);
    ptmp[start + s] = (int)e;
    gid[e] = g;
    if (s == 0) offs[g] = start;
}

__global__ __launch_bounds__(256) void cb_scatter_kernel(const int64_t* __restrict__ key, int64_t n, uint32_t mask,
                                                         const int* __restrict__ hist, const int64_t* __restrict__ pre,
                                                         const int* __restrict__ slot, int* __restrict__ ptmp,
                                                         int64_t* __restrict__ gid, int* __restrict__ offs,
                                                         int64_t* __restrict__ groups)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        cb_place(pre, (uint32_t)key[e] & mask, slot[e], e, ptmp, gid, offs);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t last = pre[mask] + CbCombine()(hist[mask]);
        const int64_t G = last >> 32;
        *groups = G;
        offs[G] = (int)n;
    }
}

// one wave per group: members back into ascending edge order (ranks by
// comparison; edge ids are distinct, so the ranks are a permutation).  Groups
// of <= 64 rank in registers (readlane broadcasts), up to CB_CAP members
// through the wave's LDS slice (16-byte broadcast reads), larger ones from
// global memory (L2).
constexpr int CB_CAP = 2048;
constexpr int CB_WAVES = 4;

__device__ __forceinline__ void cb_fix_group(int64_t g, const int* __restrict__ ptmp, const int* __restrict__ offs,
                                             const int64_t* __restrict__ gid, int64_t n, int* __restrict__ perm,
                                             int* __restrict__ mine, int lane)
{
    const int b = offs[g], S = offs[g + 1] - b;
    if (S <= 64) {
        const int v = lane < S ? ptmp[b + lane] : INT_MAX;
        int rank = 0;
        for (int j = 0; j < S; j++) rank += __builtin_amdgcn_readlane(v, j) < v;
        if (lane < S) perm[b + rank] = v;
    } else if (S <= CB_CAP) {
        for (int i = lane; i < S; i += 64) mine[i] = ptmp[b + i];
        for (int i = S + lane; i < ((S + 3) & ~3); i += 64) mine[i] = INT_MAX;   // pad the last int4
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < S; i += 64) {
            const int v = mine[i];
            int rank = 0;
            for (int j = 0; j < S; j += 4) {
                const int4 q = *(const int4*)(mine + j);
                rank += (q.x < v) + (q.y < v) + (q.z < v) + (q.w < v);
            }
            perm[b + rank] = v;
        }
        __builtin_amdgcn_wave_barrier();   // every lane's reads before the next group's writes
    } else {
        // more than CB_CAP members: they are the edges e with gid[e] == g, so a
        // scan of gid over [first member, last member] in ascending e emits
        // them in order -- O(span / 64) per group, at most n / CB_CAP such
        // groups (a rank by comparison would be O(S^2))
        int lo = INT_MAX, hi = -1;
        for (int i = lane; i < S; i += 64) {
            const int v = ptmp[b + i];
            lo = min(lo, v);
            hi = max(hi, v);
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o));
            hi = max(hi, __shfl_xor(hi, o));
        }
        int w = b;
        for (int64_t e0 = lo; e0 <= hi; e0 += 64) {
            const int64_t e = e0 + lane;
            const bool m = e <= hi && e < n && gid[e] == g;
            const uint64_t bal = __ballot(m);
            if (m) perm[w + __popcll(bal & ((1ull << lane) - 1))] = (int)e;
            w += __popcll(bal);
        }
    }
}

__global__ __launch_bounds__(64 * CB_WAVES) void cb_fix_kernel(const int* __restrict__ ptmp,
                                                               const int* __restrict__ offs,
                                                               const int64_t* __restrict__ groups,
                                                               const int64_t* __restrict__ gid, int64_t n,
                                                               int* __restrict__ perm)
{
    __shared__ __attribute__((aligned(16))) int buf[CB_WAVES][CB_CAP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t G = *groups;
    for (int64_t g = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; g < G;
         g += ((int64_t)gridDim.x * blockDim.x) >> 6)
        cb_fix_group(g, ptmp, offs, gid, n, perm, buf[w], lane);
}

// The tracker's per-update edge keys (DPVO.update: _kk_groups, _ij_groups and
// the context-row index of dpvo.py:718): key_kk = kk - M base, key_ij =
// (ii - base) * 64 + (jj - base), ctx = kk mod ring (the patch ring slot:
// DPVO.corr's and the context gather's index), jslot = jj mod frames (the
// frame ring slot).  flag (optional): set to -2 (unless already non-zero)
// when an edge lies outside the 64-frame key window, so a violated invariant
// fails loudly at the tracker's next status read instead of mis-grouping
// silently.  The only copy of the rule, for dpvo_window_keys and dpvo_window_group_by.  (ring_slot is
// apart so that the keys are stored before the 64-bit modulo: all in one cost window_keys_kernel 2 VGPRs.)
struct WindowKey { int64_t kk, ij; };

__device__ __forceinline__ WindowKey window_key(int64_t i, int64_t j, int64_t k, int64_t M, int64_t base,
                                                int* __restrict__ flag)
{
    const int64_t a = i - base, b = j - base, kr = k - M * base;
    if (flag && (a < 0 || a >= 64 || b < 0 || b >= 64 || kr < 0 || kr >= 64 * M)) atomicCAS(flag, 0, -2);
    return {kr, a * 64 + b};
}

// Python's modulo (kk, jj >= 0 in the tracker)
__device__ __forceinline__ int64_t ring_slot(int64_t x, int64_t n)
{
    const int64_t r = x % n;
    return r < 0 ? r + n : r;
}

// the keys in one pass, instead of ~6 torch elementwise launches
__global__ __launch_bounds__(256) void window_keys_kernel(const int64_t* __restrict__ ii,
                                                          const int64_t* __restrict__ jj,
                                                          const int64_t* __restrict__ kk, int64_t E, int64_t M,
                                                          int64_t base, int64_t ring, int64_t frames,
                                                          int64_t* __restrict__ key_kk, int64_t* __restrict__ key_ij,
                                                          int64_t* __restrict__ ctx, int64_t* __restrict__ jslot,
                                                          int* __restrict__ flag)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = jj[e], k = kk[e];
        const WindowKey w = window_key(ii[e], j, k, M, base, flag);
        key_kk[e] = w.kk;
        key_ij[e] = w.ij;
        ctx[e] = ring_slot(k, ring);
        jslot[e] = ring_slot(j, frames);
    }
}

// The tracker's whole per-update grouping -- window_keys_kernel's outputs plus
// the counting-sort group-bys of key_kk (2^kk_bits bins) and key_ij (4096
// bins) -- in one memset and four launches instead of thirteen (DPVO.update's
// window keys, then dpvo_group_by twice, each a memset, a histogram, a
// two-kernel device scan, a scatter and a fix-up).  The launches are short
// (~5 us) and back to back, so their count, not their bytes, sets the cost.
// Outputs are dpvo_group_by's exactly (same masking of out-of-window keys).
constexpr int WG_IJ_BITS = 12;

struct WgLayout {
    int64_t hist, pre_kk, pre_ij, pre_j, slot_kk, slot_ij, ptmp_kk, ptmp_ij, key_kk, key_ij, total;
};

WgLayout wg_layout(int64_t n, int kk_bits)
{
    const int64_t Bkk = int64_t(1) << kk_bits, Bij = int64_t(1) << WG_IJ_BITS;
    WgLayout L;
    int64_t o = 0;
    L.hist = o;    o += align256(4 * (Bkk + Bij));   // kk bins then ij bins: one memset
    L.pre_kk = o;  o += align256(8 * Bkk);
    L.pre_ij = o;  o += align256(8 * Bij);
    L.pre_j = o;   o += align256(4 * Bij);           // ij bins' starts in jj-major order
    L.slot_kk = o; o += align256(4 * n);
    L.slot_ij = o; o += align256(4 * n);
    L.ptmp_kk = o; o += align256(4 * n);
    L.ptmp_ij = o; o += align256(4 * n);
    L.key_kk = o;  o += align256(4 * n);
    L.key_ij = o;  o += align256(4 * n);
    L.total = o;
    return L;
}

__global__ __launch_bounds__(256) void wg_hist_kernel(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                      const int64_t* __restrict__ kk, int64_t E, int64_t M,
                                                      int64_t base, int64_t ring, int64_t frames, uint32_t mask_kk,
                                                      int64_t* __restrict__ ctx, int64_t* __restrict__ jslot,
                                                      int* __restrict__ flag, int* __restrict__ hist_kk,
                                                      int* __restrict__ hist_ij, int* __restrict__ slot_kk,
                                                      int* __restrict__ slot_ij, uint32_t* __restrict__ key_kk,
                                                      uint32_t* __restrict__ key_ij)
{
    // the (ii, jj) keys: a patch's edges go to different frame pairs, so a
    // wave's lanes rarely share one and ~500 bins took every edge's atomic; a
    // workgroup ranks its edges in an LDS histogram instead and reserves each
    // touched bin's range with one global atomic (the slots within a bin are
    // ordered by wg_fix afterwards, as before).  The kk keys come in runs (a
    // patch's edges are adjacent): one atomic per run, cb_run_slot.
    constexpr int BIJ = 1 << WG_IJ_BITS;
    __shared__ int lh[BIJ];
    const int lane = threadIdx.x & 63;
    for (int64_t e0 = blockIdx.x * (int64_t)blockDim.x; e0 < E; e0 += (int64_t)gridDim.x * blockDim.x) {
        for (int i = threadIdx.x; i < BIJ; i += blockDim.x) lh[i] = 0;
        __syncthreads();
        const int64_t e = e0 + threadIdx.x;   // uniform trip count: whole waves stay converged
        const bool valid = e < E;
        uint32_t kk_k = 0xffffffffu, ij_k = 0xffffffffu;
        if (valid) {
            const int64_t j = jj[e], k = kk[e];
            const WindowKey w = window_key(ii[e], j, k, M, base, flag);
            kk_k = (uint32_t)w.kk & mask_kk;   // dpvo_group_by's masking
            ij_k = (uint32_t)w.ij & (BIJ - 1);
            ctx[e] = ring_slot(k, ring);
            jslot[e] = ring_slot(j, frames);
            key_kk[e] = kk_k;
            key_ij[e] = ij_k;
        }
        const int s_kk = cb_run_slot(kk_k, valid, lane, hist_kk);
        const int l_ij = valid ? atomicAdd(&lh[ij_k], 1) : 0;   // rank within this workgroup's share
        __syncthreads();
        for (int i = threadIdx.x; i < BIJ; i += blockDim.x) {
            const int c = lh[i];
            if (c) lh[i] = atomicAdd(&hist_ij[i], c);   // the workgroup's base in bin i
        }
        __syncthreads();
        if (valid) {
            slot_kk[e] = s_kk;
            slot_ij[e] = lh[ij_k] + l_ij;
        }
        __syncthreads();   // (lh is cleared for the next round)
    }
}

// block 0 scans the kk bins, block 1 the ij bins: (start, group index) per
// bin, the group count and offs[G] = E.  8192 bins per round: thread t loads
// bins 8t .. 8t+7 (two 16-byte loads, coalesced), scans them in registers,
// one block scan of the thread sums, 64-byte coalesced stores of the results.
// (16 bins per thread, C3's 16384 kk bins in one round: 11.8 vs 11.4 us.)
__global__ __launch_bounds__(1024) void wg_scan_kernel(const int* __restrict__ hist, int Bkk, int64_t* __restrict__ pre_kk,
                                                       int64_t* __restrict__ pre_ij, int* __restrict__ offs_kk,
                                                       int* __restrict__ offs_ij, int64_t* __restrict__ groups_kk,
                                                       int64_t* __restrict__ groups_ij, int n,
                                                       int* __restrict__ pre_j)
{
    __shared__ int64_t wsum[16];
    if (blockIdx.x == 2) {
        // the (ii, jj) bins visited jj-major (bin a * 64 + b at transposed
        // position b * 64 + a): their starts give altcorr's target-frame order
        // from the ij slots, with no histogram of its own
        const int* h = hist + Bkk;
        const int t = threadIdx.x, lane = t & 63, w = t >> 6;
        int c[4], loc[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int tix = 4 * t + j, b = tix >> 6, a = tix & 63;
            c[j] = h[a * 64 + b];
            loc[j] = sum;
            sum += c[j];
        }
        int x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int off = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) off += i < w ? (int)wsum[i] : 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int tix = 4 * t + j, b = tix >> 6, a = tix & 63;
            pre_j[a * 64 + b] = off + x - sum + loc[j];
        }
        return;
    }
    const bool ij = blockIdx.x != 0;
    const int B = ij ? (1 << WG_IJ_BITS) : Bkk;
    const int* h = ij ? hist + Bkk : hist;
    int64_t* pre = ij ? pre_ij : pre_kk;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    constexpr int PT = 8;   // bins per thread
    int64_t carry = 0;
    for (int base = 0; base < B; base += 1024 * PT) {
        const int b0 = base + PT * t;
        int c[PT];
        if (b0 + PT <= B && ((uintptr_t)(h + b0) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < PT / 4; q++) {
                const int4 x = *(const int4*)(h + b0 + 4 * q);
                c[4 * q] = x.x; c[4 * q + 1] = x.y; c[4 * q + 2] = x.z; c[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PT; j++) c[j] = b0 + j < B ? h[b0 + j] : 0;
        }
        int64_t loc[PT], s = 0;
#pragma unroll
        for (int j = 0; j < PT; j++) {
            loc[j] = s;
            s += CbCombine()(c[j]);
        }
        int64_t x = s;   // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int64_t off = carry, tot = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int64_t v = wsum[i];
            off += i < w ? v : 0;
            tot += v;
        }
        const int64_t ex = off + x - s;
#pragma unroll
        for (int j = 0; j < PT; j++)
            if (b0 + j < B) pre[b0 + j] = ex + loc[j];
        carry += tot;
        __syncthreads();   // wsum is rewritten next round
    }
    if (t == 0) {   // carry = the grand total
        const int64_t G = carry >> 32;
        *(ij ? groups_ij : groups_kk) = G;
        (ij ? offs_ij : offs_kk)[G] = n;
    }
}

__global__ __launch_bounds__(256) void wg_scatter_kernel(int64_t E, const uint32_t* __restrict__ key_kk,
                                                         const uint32_t* __restrict__ key_ij,
                                                         const int64_t* __restrict__ pre_kk,
                                                         const int64_t* __restrict__ pre_ij,
                                                         const int* __restrict__ slot_kk,
                                                         const int* __restrict__ slot_ij, int* __restrict__ ptmp_kk,
                                                         int* __restrict__ ptmp_ij, int64_t* __restrict__ gid_kk,
                                                         int64_t* __restrict__ gid_ij, int* __restrict__ offs_kk,
                                                         int* __restrict__ offs_ij, const int* __restrict__ pre_j,
                                                         int* __restrict__ order_j)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        if (order_j) order_j[pre_j[key_ij[e]] + slot_ij[e]] = (int)e;
        cb_place(pre_kk, key_kk[e], slot_kk[e], e, ptmp_kk, gid_kk, offs_kk);
        cb_place(pre_ij, key_ij[e], slot_ij[e], e, ptmp_ij, gid_ij, offs_ij);
    }
}

// one wave per group, the (larger) ij groups first
__global__ __launch_bounds__(64 * CB_WAVES) void wg_fix_kernel(int64_t n, const int* __restrict__ ptmp_kk,
                                                               const int* __restrict__ offs_kk,
                                                               const int64_t* __restrict__ groups_kk,
                                                               const int64_t* __restrict__ gid_kk,
                                                               int* __restrict__ perm_kk,
                                                               const int* __restrict__ ptmp_ij,
                                                               const int* __restrict__ offs_ij,
                                                               const int64_t* __restrict__ groups_ij,
                                                               const int64_t* __restrict__ gid_ij,
                                                               int* __restrict__ perm_ij)
{
    __shared__ __attribute__((aligned(16))) int buf[CB_WAVES][CB_CAP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t Gi = *groups_ij, G = Gi + *groups_kk;
    for (int64_t g = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; g < G;
         g += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        if (g < Gi)
            cb_fix_group(g, ptmp_ij, offs_ij, gid_ij, n, perm_ij, buf[w], lane);
        else
            cb_fix_group(g - Gi, ptmp_kk, offs_kk, gid_kk, n, perm_kk, buf[w], lane);
    }
}

// dpvo_edge_order: the ordering the window group-by emits as jj_order, for callers without one --
// edge visiting order grouped by target frame (counting sort; the order inside
// a frame's group is arbitrary -- it only affects which edges share an L2)
__global__ __launch_bounds__(256) void edge_hist_kernel(const int64_t* __restrict__ jj, int64_t E, int nb,
                                                        int* __restrict__ count)
{
    extern __shared__ int h[];
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = jj[e];
        atomicAdd(&h[(j >= 0 && j < nb) ? (int)j : nb], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= nb; i += blockDim.x)
        if (h[i]) atomicAdd(&count[i], h[i]);
}

// scatter: each workgroup counts its chunk per bucket in LDS, reserves one
// contiguous run per bucket with a single global atomic, then fills it
// (every thread adding to a few shared global cursors serialises: ~0.4 ms)
__global__ __launch_bounds__(256) void edge_scatter_kernel(const int64_t* __restrict__ jj, int64_t E, int nb,
                                                           const int* __restrict__ count, int* __restrict__ cursor,
                                                           int* __restrict__ order)
{
    extern __shared__ int sh[];
    int* base = sh;              // [nb + 1] global start of this workgroup's run per bucket
    int* loc = sh + (nb + 1);    // [nb + 1] local counts, then local cursors
    const int64_t chunk = (E + gridDim.x - 1) / gridDim.x;
    const int64_t e0 = blockIdx.x * chunk, e1 = min(E, e0 + chunk);
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) loc[i] = 0;
    __syncthreads();
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int64_t j = jj[e];
        atomicAdd(&loc[(j >= 0 && j < nb) ? (int)j : nb], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i <= nb; i++) {
            const int c = count[i];
            base[i] = loc[i] ? s + atomicAdd(&cursor[i], loc[i]) : 0;
            s += c;
            loc[i] = 0;
        }
    }
    __syncthreads();
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int64_t j = jj[e];
        const int b = (j >= 0 && j < nb) ? (int)j : nb;
        order[base[b] + atomicAdd(&loc[b], 1)] = (int)e;
    }
}

// neighbors over the kk group-by CSR: one wave per group; member i's
// predecessor / successor in (jj, edge) order by an O(s^2) scan of the group
// (s ~ 25 in DPVO's steady state), 64 members at a time, broadcast by shuffles.
__global__ __launch_bounds__(256) void nb_csr_kernel(const int64_t* __restrict__ jj, const int* __restrict__ offs,
                                                     const int* __restrict__ perm, const int64_t* __restrict__ groups,
                                                     int64_t max_groups, int64_t* __restrict__ ix,
                                                     int64_t* __restrict__ jx)
{
    const int lane = threadIdx.x & 63;
    const int64_t G = min(*groups, max_groups);
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t g = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; g < G; g += nw) {
        const int start = offs[g], s = offs[g + 1] - start;
        for (int i0 = 0; i0 < s; i0 += 64) {
            const bool mine = i0 + lane < s;
            const int ei = mine ? perm[start + i0 + lane] : 0;
            const int64_t ji = mine ? jj[ei] : 0;
            // best predecessor (largest key below mine) / successor (smallest above)
            int64_t pj = INT64_MIN, nj = INT64_MAX;
            int pe = -1, ne = -1;
            for (int t0 = 0; t0 < s; t0 += 64) {
                const int cnt = min(64, s - t0);
                const int et = t0 + lane < s ? perm[start + t0 + lane] : 0;
                const int64_t jt = t0 + lane < s ? jj[et] : 0;
                for (int k = 0; k < cnt; k++) {
                    const int ek = __shfl(et, k);
                    const int64_t jk = __shfl(jt, k);
                    const bool below = jk < ji || (jk == ji && ek < ei);
                    const bool above = jk > ji || (jk == ji && ek > ei);
                    if (below && (jk > pj || (jk == pj && ek > pe))) { pj = jk; pe = ek; }
                    if (above && (jk < nj || (jk == nj && ek < ne))) { nj = jk; ne = ek; }
                }
            }
            if (mine) {
                ix[ei] = pe;
                jx[ei] = ne;
            }
        }
    }
}

// DPVO.__call__'s edge append (dpvo.py:756-769, 799-800): the old edge list
// followed by the forward edges (patches of frames [n - r, n - 1) into frame
// n - 1) and the backward edges (frame n - 1's patches into frames
// [n - r, n), patch-major as flatmeshgrid(indexing="ij") lists them), with
// ii = ix[kk] -- one launch instead of two aranges + meshgrid per direction,
// the concatenations and the ix gather.  n: the frame count after the new
// frame was added.
struct AppendRanges {
    int64_t f0, nf;           // forward: patches f0 .. f0 + nf, all into frame n - 1
    int64_t b0, j0, nj, nb;   // backward: patches from b0, each into frames j0 .. j0 + nj, nb edges in all
    __host__ __device__ AppendRanges(int64_t n, int64_t M, int64_t r)
    {
        j0 = n - r > 0 ? n - r : 0;
        nj = n - j0;
        f0 = M * j0;
        b0 = M * (n - 1 > 0 ? n - 1 : 0);
        nf = b0 - f0;
        nb = (M * n - b0) * nj;
    }
};

__global__ __launch_bounds__(256) void append_edges_kernel(const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                           const int64_t* __restrict__ kk, int64_t E,
                                                           const int64_t* __restrict__ ix, int64_t n, int64_t M,
                                                           int64_t r, int64_t* __restrict__ ii_o,
                                                           int64_t* __restrict__ jj_o, int64_t* __restrict__ kk_o)
{
    const AppendRanges a(n, M, r);
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E + a.nf + a.nb;
         e += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j, k;
        if (e < E) {
            i = ii[e], j = jj[e], k = kk[e];
        } else if (e < E + a.nf) {
            k = a.f0 + (e - E), j = n - 1, i = ix[k];
        } else {
            const int64_t t = e - E - a.nf;
            k = a.b0 + t / a.nj, j = a.j0 + t % a.nj, i = ix[k];
        }
        ii_o[e] = i;
        jj_o[e] = j;
        kk_o[e] = k;
    }
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" size_t dpvo_group_by_workspace_bytes(int64_t n)
{
    return (size_t)gb_layout(n > 0 ? n : 1).total + 256;
}

extern "C" size_t dpvo_group_by_workspace_bytes_for(int64_t n, int key_bits)
{
    size_t r = dpvo_group_by_workspace_bytes(n);
    if (key_bits >= 1 && key_bits <= CB_MAX_BITS) r = std::max(r, (size_t)cb_layout(n > 0 ? n : 1, key_bits).total + 256);
    return r;
}

extern "C" int dpvo_group_by(const int64_t* key, int64_t n, int key_bits, int64_t* gid, int* offs, int* perm,
                             int64_t* groups, void* workspace, size_t workspace_bytes, void* stream)
{
    DPVO_CHECK_ARG(n >= 0 && n < (int64_t(1) << 31), "bad size");
    DPVO_CHECK_ARG(key_bits >= 1 && key_bits <= 64, "key_bits must be 1..64");
    DPVO_CHECK_ARG(groups != nullptr, "groups output missing");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        DPVO_CHECK_HIP(hipMemsetAsync(groups, 0, sizeof(int64_t), st));
        DPVO_CHECK_HIP(hipMemsetAsync(offs, 0, sizeof(int), st));
        return 0;
    }
    char* ws = align256(workspace);
    if (key_bits <= CB_MAX_BITS && workspace != nullptr) {
        const CbLayout C = cb_layout(n, key_bits);
        if (workspace_bytes >= (size_t)C.total + 256) {   // else: the radix path below
            const int64_t B = int64_t(1) << key_bits;
            const uint32_t mask = (uint32_t)(B - 1);
            int* hist = (int*)(ws + C.hist);
            int64_t* pre = (int64_t*)(ws + C.pre);
            int* slot = (int*)(ws + C.slot);
            int* ptmp = (int*)(ws + C.ptmp);
            const unsigned gn = grid_for(n, 256, 2048);
            DPVO_CHECK_HIP(hipMemsetAsync(hist, 0, 4 * B, st));
            hipLaunchKernelGGL(cb_hist_kernel, dim3(gn), dim3(256), 0, st, key, n, mask, hist, slot);
            size_t tb = (size_t)C.tmp_bytes;
            hipcub::TransformInputIterator<int64_t, CbCombine, const int*> it(hist, CbCombine());
            DPVO_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(ws + C.tmp, tb, it, pre, (int)B, st));
            hipLaunchKernelGGL(cb_scatter_kernel, dim3(gn), dim3(256), 0, st, key, n, mask, hist, pre, slot, ptmp, gid,
                               offs, groups);
            const unsigned gf = grid_for(std::min<int64_t>(n, B) * 64, 64 * CB_WAVES, 2048);
            hipLaunchKernelGGL(cb_fix_kernel, dim3(gf), dim3(64 * CB_WAVES), 0, st, ptmp, offs, groups, gid, n, perm);
            DPVO_CHECK_LAUNCH();
            return 0;
        }
    }
    const GbLayout L = gb_layout(n);
    DPVO_CHECK_ARG(workspace != nullptr && workspace_bytes >= (size_t)L.total + 256, "workspace too small");
    int* v_in = (int*)(ws + L.v_in);
    int* flag = (int*)(ws + L.flag);
    int* incl = (int*)(ws + L.incl);
    size_t tmp_bytes = (size_t)L.tmp_bytes;
    const unsigned g = grid_for(n, 256, 2048);
    auto sort = [&](auto* k_in, auto* k_out) -> int {
        using K = std::remove_pointer_t<decltype(k_in)>;
        hipLaunchKernelGGL(gb_keys_kernel<K>, dim3(g), dim3(256), 0, st, key, n, k_in, v_in);
        DPVO_CHECK_LAUNCH();
        DPVO_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + L.tmp, tmp_bytes, k_in, k_out, v_in, perm, (int)n, 0,
                                                          key_bits, st));
        hipLaunchKernelGGL(gb_flags_kernel<K>, dim3(g), dim3(256), 0, st, k_out, n, flag);
        return 0;
    };
    if (key_bits <= 32)
        sort((uint32_t*)(ws + L.k_in), (uint32_t*)(ws + L.k_out));
    else
        sort((uint64_t*)(ws + L.k_in), (uint64_t*)(ws + L.k_out));
    tmp_bytes = (size_t)L.tmp_bytes;
    DPVO_CHECK_HIP(hipcub::DeviceScan::InclusiveSum(ws + L.tmp, tmp_bytes, flag, incl, (int)n, st));
    hipLaunchKernelGGL(gb_finish_kernel, dim3(g), dim3(256), 0, st, flag, incl, perm, n, gid, offs, groups);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_window_keys(const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t E, int64_t M,
                                int64_t base, int64_t ring, int64_t frames, int64_t* key_kk, int64_t* key_ij,
                                int64_t* ctx, int64_t* jslot, int* flag, void* stream)
{
    DPVO_CHECK_ARG(E >= 0 && M > 0 && ring > 0 && frames > 0, "E >= 0, M > 0, ring > 0 and frames > 0 required");
    if (E == 0) return 0;
    DPVO_CHECK_ARG(ii && jj && kk && key_kk && key_ij && ctx && jslot, "null operand");
    hipLaunchKernelGGL(window_keys_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, as_stream(stream), ii, jj, kk,
                       E, M, base, ring, frames, key_kk, key_ij, ctx, jslot, flag);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_window_group_by_workspace_bytes(int64_t E, int kk_bits)
{
    if (kk_bits < 1 || kk_bits > CB_MAX_BITS) return 0;
    return (size_t)wg_layout(E > 0 ? E : 1, kk_bits).total + 256;
}

extern "C" int dpvo_window_group_by(const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t E, int64_t M,
                                    int64_t base, int64_t ring, int64_t frames, int kk_bits, int64_t* ctx,
                                    int64_t* jslot, int* flag, int64_t* kk_gid, int* kk_offs, int* kk_perm,
                                    int64_t* kk_groups, int64_t* ij_gid, int* ij_offs, int* ij_perm,
                                    int64_t* ij_groups, int* jj_order, void* workspace, size_t workspace_bytes,
                                    void* stream)
{
    DPVO_CHECK_ARG(E >= 0 && E < (int64_t(1) << 31), "bad size");
    DPVO_CHECK_ARG(M > 0 && ring > 0 && frames > 0, "M > 0, ring > 0 and frames > 0 required");
    DPVO_CHECK_ARG(kk_bits >= 1 && kk_bits <= CB_MAX_BITS, "kk_bits must be 1..22");
    DPVO_CHECK_ARG(kk_groups && kk_offs && ij_groups && ij_offs, "CSR outputs missing");
    hipStream_t st = as_stream(stream);
    if (E == 0) {
        DPVO_CHECK_HIP(hipMemsetAsync(kk_groups, 0, sizeof(int64_t), st));
        DPVO_CHECK_HIP(hipMemsetAsync(kk_offs, 0, sizeof(int), st));
        DPVO_CHECK_HIP(hipMemsetAsync(ij_groups, 0, sizeof(int64_t), st));
        DPVO_CHECK_HIP(hipMemsetAsync(ij_offs, 0, sizeof(int), st));
        return 0;
    }
    DPVO_CHECK_ARG(ii && jj && kk && ctx && jslot && kk_gid && kk_perm && ij_gid && ij_perm, "null operand");
    const WgLayout L = wg_layout(E, kk_bits);
    DPVO_CHECK_ARG(workspace != nullptr && workspace_bytes >= (size_t)L.total + 256, "workspace too small");
    char* ws = align256(workspace);
    const int Bkk = 1 << kk_bits;
    int* hist = (int*)(ws + L.hist);
    int64_t* pre_kk = (int64_t*)(ws + L.pre_kk);
    int64_t* pre_ij = (int64_t*)(ws + L.pre_ij);
    int* slot_kk = (int*)(ws + L.slot_kk);
    int* slot_ij = (int*)(ws + L.slot_ij);
    int* ptmp_kk = (int*)(ws + L.ptmp_kk);
    int* ptmp_ij = (int*)(ws + L.ptmp_ij);
    uint32_t* key_kk = (uint32_t*)(ws + L.key_kk);
    uint32_t* key_ij = (uint32_t*)(ws + L.key_ij);
    int* pre_j = (int*)(ws + L.pre_j);
    const unsigned gn = grid_for(E, 256, 2048);
    DPVO_CHECK_HIP(hipMemsetAsync(hist, 0, 4 * (size_t)(Bkk + (1 << WG_IJ_BITS)), st));
    hipLaunchKernelGGL(wg_hist_kernel, dim3(gn), dim3(256), 0, st, ii, jj, kk, E, M, base, ring, frames,
                       (uint32_t)(Bkk - 1), ctx, jslot, flag, hist, hist + Bkk, slot_kk, slot_ij, key_kk, key_ij);
    hipLaunchKernelGGL(wg_scan_kernel, dim3(jj_order ? 3 : 2), dim3(1024), 0, st, hist, Bkk, pre_kk, pre_ij, kk_offs,
                       ij_offs, kk_groups, ij_groups, (int)E, pre_j);
    hipLaunchKernelGGL(wg_scatter_kernel, dim3(gn), dim3(256), 0, st, E, key_kk, key_ij, pre_kk, pre_ij, slot_kk,
                       slot_ij, ptmp_kk, ptmp_ij, kk_gid, ij_gid, kk_offs, ij_offs, pre_j, jj_order);
    const int64_t waves = std::min<int64_t>(E, Bkk) + std::min<int64_t>(E, 1 << WG_IJ_BITS);
    const unsigned gf = grid_for(waves * 64, 64 * CB_WAVES, 2048);
    hipLaunchKernelGGL(wg_fix_kernel, dim3(gf), dim3(64 * CB_WAVES), 0, st, E, ptmp_kk, kk_offs, kk_groups, kk_gid,
                       kk_perm, ptmp_ij, ij_offs, ij_groups, ij_gid, ij_perm);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_edge_order_workspace_bytes(int num_buckets) { return (size_t)2 * (num_buckets + 1) * 4; }

extern "C" int dpvo_edge_order(const int64_t* jj, int64_t num_edges, int num_buckets, int* order, void* workspace,
                               size_t workspace_bytes, void* stream)
{
    DPVO_CHECK_ARG(num_buckets >= 1 && num_buckets <= 16384, "num_buckets must be 1..16384");
    DPVO_CHECK_ARG(num_edges >= 0 && num_edges < 0x7fffffff, "bad edge count");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_edge_order_workspace_bytes(num_buckets), "workspace too small");
    if (num_edges == 0) return 0;
    hipStream_t s = as_stream(stream);
    int* count = (int*)workspace;
    int* cursor = count + num_buckets + 1;
    DPVO_CHECK_HIP(hipMemsetAsync(workspace, 0, dpvo_edge_order_workspace_bytes(num_buckets), s));
    const size_t lds = (size_t)(num_buckets + 1) * 4;
    const unsigned g = grid_for(num_edges, 256, 512);
    hipLaunchKernelGGL(edge_hist_kernel, dim3(g), dim3(256), lds, s, jj, num_edges, num_buckets, count);
    const unsigned gs = grid_for(num_edges, 2048, 256);
    hipLaunchKernelGGL(edge_scatter_kernel, dim3(gs), dim3(256), 2 * lds, s, jj, num_edges, num_buckets, count,
                       cursor, order);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_neighbors_csr(const int64_t* jj, const int* offs, const int* perm, const int64_t* groups,
                                  int64_t max_groups, int64_t num_edges, int64_t* ix, int64_t* jx, void* stream)
{
    DPVO_CHECK_ARG(groups != nullptr && offs != nullptr && perm != nullptr, "CSR missing");
    DPVO_CHECK_ARG(num_edges >= 0 && num_edges < (int64_t(1) << 31), "bad size");
    if (num_edges == 0 || max_groups <= 0) return 0;
    const unsigned grid = grid_for(max_groups * 64, 256, 4096);
    hipLaunchKernelGGL(nb_csr_kernel, dim3(grid), dim3(256), 0, as_stream(stream), jj, offs, perm, groups,
                       max_groups, ix, jx);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t dpvo_append_edges_count(int64_t n, int64_t M, int64_t r)
{
    if (n < 1 || M < 1 || r < 1) return -1;
    const AppendRanges a(n, M, r);
    return a.nf + a.nb;
}

extern "C" int dpvo_append_edges(const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t E, const int64_t* ix,
                                 int64_t n, int64_t M, int64_t r, int64_t* ii_out, int64_t* jj_out, int64_t* kk_out,
                                 void* stream)
{
    const int64_t add = dpvo_append_edges_count(n, M, r);
    DPVO_CHECK_ARG(add >= 0 && E >= 0, "n >= 1, M >= 1, PATCH_LIFETIME >= 1 and E >= 0 required");
    DPVO_CHECK_ARG(ix && ii_out && jj_out && kk_out && (E == 0 || (ii && jj && kk)), "null operand");
    if (E + add == 0) return 0;
    hipLaunchKernelGGL(append_edges_kernel, dim3(grid_for(E + add, 256, 4096)), dim3(256), 0, as_stream(stream), ii,
                       jj, kk, E, ix, n, M, r, ii_out, jj_out, kk_out);
    DPVO_CHECK_LAUNCH();
    return 0;
}
