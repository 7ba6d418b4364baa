// updateop.hip -- what the learned update operator itself launches (gfx950):
// SoftAgg in its three forms, the row gather and the edge targets.  The
// tracker's edge bookkeeping (group-by, window keys, CSR neighbours, edge
// append) is groupby.hip, the torch_scatter reductions are scatter.hip.
//
// SoftAgg (reference dpvo/blocks.py:40-48) aggregates edge features over
// groups of edges sharing a key with torch_scatter 2.1.2's scatter_softmax +
// scatter_sum.  torch_scatter is absent on ROCm and ATen's scatter_reduce
// "amax" path is a same-address atomic storm (~2.4 ms per call at C3), so the
// whole softmax-weighted sum is one streaming pass here:
//
//   1. CSR of the group labels: count (atomics on G counters), one-block
//      exclusive scan, fill (atomic cursor per group);
//   2. one wave64 per (group, 128-channel slice): the wave sorts its edge
//      list in LDS (ascending edge index -> deterministic fp32 sums), then
//      streams the f/s rows 8 edges at a time with a batched online softmax
//      (one rescale per 8 edges), and writes y = acc / (l + eps).
//
// Bytes per edge: 2 rows x D x sizeof(T) read once (+12 B of CSR traffic);
// the kernel is HBM-bound like the GEMMs around it.
#include "updateop.hpp"

namespace dpvo {
namespace {

constexpr int SA_WAVES = 4;          // waves per block in the reduce kernel
constexpr int SA_UNROLL = 8;         // edges in flight per online-softmax step
constexpr int SA_CAP = DPVO_SOFTAGG_SORT_CAP;

struct SaLayout {
    int64_t count, offs, cursor, perm, total;
};

SaLayout sa_layout(int64_t E, int64_t G)
{
    SaLayout L;
    int64_t o = 0;
    L.count = o;  o += align256(4 * G);
    L.offs = o;   o += align256(4 * (G + 1));
    L.cursor = o; o += align256(4 * G);
    L.perm = o;   o += align256(4 * E);
    L.total = o;
    return L;
}

__global__ __launch_bounds__(256) void sa_count_kernel(const int64_t* __restrict__ group, int64_t E, int64_t G,
                                                       int* __restrict__ count)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = group[e];
        if (g >= 0 && g < G) atomicAdd(&count[g], 1);
    }
}

// exclusive scan of count[0..G) -> offs[0..G], cursor = offs (single block)
__global__ __launch_bounds__(1024) void sa_scan_kernel(const int* __restrict__ count, int64_t G,
                                                       int* __restrict__ offs, int* __restrict__ cursor)
{
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (G + 1023) / 1024;
    const int64_t g0 = tid * per, g1 = min(G, g0 + per);
    int sum = 0;
    for (int64_t g = g0; g < g1; g++) sum += count[g];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int base = part[tid] - sum;
    for (int64_t g = g0; g < g1; g++) {
        offs[g] = base;
        cursor[g] = base;
        base += count[g];
    }
    if (tid == 1023) offs[G] = part[1023];
}

__global__ __launch_bounds__(256) void sa_fill_kernel(const int64_t* __restrict__ group, int64_t E, int64_t G,
                                                      int* __restrict__ cursor, int* __restrict__ perm)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = group[e];
        if (g < 0 || g >= G) continue;
        perm[atomicAdd(&cursor[g], 1)] = (int)e;
    }
}

template <typename T> struct Pair;
template <> struct Pair<half_t> {
    typedef half2_t V;
    static __device__ __forceinline__ float2_t load(const half_t* p) { V v = *(const V*)p; return {(float)v.x, (float)v.y}; }
    static __device__ __forceinline__ void store(half_t* p, float2_t v) { *(V*)p = V{(half_t)v.x, (half_t)v.y}; }
};
template <> struct Pair<float> {
    static __device__ __forceinline__ float2_t load(const float* p) { return *(const float2_t*)p; }
    static __device__ __forceinline__ void store(float* p, float2_t v) { *(float2_t*)p = v; }
};
template <> struct Pair<double> {
    static __device__ __forceinline__ float2_t load(const double* p) { return {(float)p[0], (float)p[1]}; }
    static __device__ __forceinline__ void store(double* p, float2_t v) { p[0] = v.x; p[1] = v.y; }
};

// Online softmax-weighted sum over rows order[0 .. n) for the lane's two
// channels, in SA_UNROLL batches from order[0].  The only copy of the pass: all three reduce
// kernels run it, so equal row lists give equal bits.  A caller that starts inside a list folds the
// start into the pointer (a start index of its own cost sa_reduce_csr_kernel<half> 3 VGPRs and a wave).
template <typename T>
__device__ __forceinline__ void sa_online(const T* __restrict__ f, int64_t ldf, const T* __restrict__ s, int64_t lds,
                                          const int* order, int n, int cc, float2_t& m, float2_t& l, float2_t& acc)
{
    for (int i0 = 0; i0 < n; i0 += SA_UNROLL) {
        float2_t sv[SA_UNROLL], fv[SA_UNROLL];
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++) {
            const int64_t e = order[min(i0 + u, n - 1)];
            sv[u] = Pair<T>::load(s + e * lds + cc);
            fv[u] = Pair<T>::load(f + e * ldf + cc);
        }
        float2_t mb = m;
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++)
            if (i0 + u < n) {
                mb.x = fmaxf(mb.x, sv[u].x);
                mb.y = fmaxf(mb.y, sv[u].y);
            }
        const float ax = __expf(m.x - mb.x), ay = __expf(m.y - mb.y);
        l.x *= ax; l.y *= ay; acc.x *= ax; acc.y *= ay;
#pragma unroll
        for (int u = 0; u < SA_UNROLL; u++)
            if (i0 + u < n) {
                const float px = __expf(sv[u].x - mb.x), py = __expf(sv[u].y - mb.y);
                l.x += px; l.y += py;
                acc.x += px * fv[u].x; acc.y += py * fv[u].y;
            }
        m = mb;
    }
}

// One wave per (group, 128-channel slice).  Lane owns channels c, c+1.
template <typename T>
__global__ __launch_bounds__(64 * SA_WAVES) void sa_reduce_kernel(const T* __restrict__ f, int64_t ldf,
                                                                  const T* __restrict__ s, int64_t lds,
                                                                  const int* __restrict__ offs,
                                                                  const int* __restrict__ perm, int64_t G, int D,
                                                                  int slices, float eps, T* __restrict__ y)
{
    __shared__ int lst[SA_WAVES][2][SA_CAP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t task = (int64_t)blockIdx.x * SA_WAVES + w;
    if (task >= G * slices) return;
    const int64_t g = task / slices;
    const int c = (int)(task % slices) * 128 + 2 * lane;
    const int b = offs[g], S = offs[g + 1] - b;
    const bool act = c < D;
    const int cc = act ? c : 0;
    float2_t m = {-INFINITY, -INFINITY}, l = {0.f, 0.f}, acc = {0.f, 0.f};

    // ascending edge order within the group (ranks of distinct edge ids).  The
    // online pass is instantiated once per source of the order -- the wave's
    // LDS list or global perm -- never through one pointer that may be either:
    // such a generic pointer compiles to flat loads, and a flat load of the
    // LDS list is not ordered after the ds_write that stored it (another lane's
    // rank), so the pass could read a stale slot of the sorted list -- the
    // round-5 intermittent "csr != dense" SoftAgg mismatch.
    if (S <= SA_CAP) {
        int* raw = lst[w][0];
        int* srt = lst[w][1];
        for (int i = lane; i < S; i += 64) raw[i] = perm[b + i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < S; i += 64) {
            const int v = raw[i];
            int r = 0;
            for (int j = 0; j < S; j++) r += raw[j] < v;
            srt[r] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        sa_online<T>(f, ldf, s, lds, srt, S, cc, m, l, acc);
    } else {
        sa_online<T>(f, ldf, s, lds, perm + b, S, cc, m, l, acc);
    }
    if (act) Pair<T>::store(y + g * (int64_t)D + c, float2_t{acc.x / (l.x + eps), acc.y / (l.y + eps)});
}

// SoftAgg over a prebuilt CSR whose group count lives on the device.  Group
// members are already in ascending edge order (stable sort): no LDS sort.
template <typename T>
__global__ __launch_bounds__(256) void sa_reduce_csr_kernel(const T* __restrict__ f, int64_t ldf,
                                                            const T* __restrict__ s, int64_t lds,
                                                            const int* __restrict__ offs,
                                                            const int* __restrict__ perm,
                                                            const int64_t* __restrict__ groups, int D, int slices,
                                                            float eps, T* __restrict__ y)
{
    const int lane = threadIdx.x & 63;
    const int64_t ntask = *groups * slices;
    for (int64_t task = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; task < ntask;
         task += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t g = task / slices;
        const int c = (int)(task % slices) * 128 + 2 * lane;
        const int b = offs[g], S = offs[g + 1] - b;
        const bool act = c < D;
        const int cc = act ? c : 0;
        float2_t m = {-INFINITY, -INFINITY}, l = {0.f, 0.f}, acc = {0.f, 0.f};
        // (shared for fp64 too, at 89 VGPRs for the 85 of a body of its own, occupancy 5 either way: csr == dense)
        sa_online<T>(f, ldf, s, lds, perm + b, S, cc, m, l, acc);
        if (act) Pair<T>::store(y + g * (int64_t)D + c, float2_t{acc.x / (l.x + eps), acc.y / (l.y + eps)});
    }
}

// sa_reduce_csr_kernel with a workgroup per (group, 128-channel slice): groups
// of at least SA_SPLIT rows are cut into four contiguous row ranges, one per
// wave, whose (max, sum, weighted sum) states are merged in wave order -- the
// long frame-pair groups (~190 rows at C3) run four times shorter chains of
// dependent loads.  Shorter groups run on wave 0 alone with exactly
// sa_reduce_csr_kernel's arithmetic (same bits).  Deterministic either way.
constexpr int SA_SPLIT = 64;
template <typename T>
__global__ __launch_bounds__(256) void sa_reduce_csr_split_kernel(const T* __restrict__ f, int64_t ldf,
                                                                  const T* __restrict__ s, int64_t lds,
                                                                  const int* __restrict__ offs,
                                                                  const int* __restrict__ perm,
                                                                  const int64_t* __restrict__ groups, int D,
                                                                  int slices, float eps, T* __restrict__ y)
{
    __shared__ float2_t st[4][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntask = *groups * slices;
    for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
        const int64_t g = task / slices;
        const int c = (int)(task % slices) * 128 + 2 * lane;
        const int b = offs[g], S = offs[g + 1] - b;
        const int* order = perm + b;
        const bool act = c < D;
        const int cc = act ? c : 0;
        float2_t m = {-INFINITY, -INFINITY}, l = {0.f, 0.f}, acc = {0.f, 0.f};
        if (S < SA_SPLIT) {
            if (wave == 0) {
                sa_online<T>(f, ldf, s, lds, order, S, cc, m, l, acc);
                if (act) Pair<T>::store(y + g * (int64_t)D + c, float2_t{acc.x / (l.x + eps), acc.y / (l.y + eps)});
            }
            continue;   // S is uniform over the workgroup: every wave skips the barriers below together
        }
        const int q = (S + 3) / 4, r0 = min(S, wave * q), r1 = min(S, r0 + q);
        sa_online<T>(f, ldf, s, lds, order + r0, r1 - r0, cc, m, l, acc);
        st[wave][0][lane] = m;
        st[wave][1][lane] = l;
        st[wave][2][lane] = acc;
        __syncthreads();
        if (wave == 0) {
            float2_t M = st[0][0][lane];
#pragma unroll
            for (int w = 1; w < 4; w++) {
                M.x = fmaxf(M.x, st[w][0][lane].x);
                M.y = fmaxf(M.y, st[w][0][lane].y);
            }
            float2_t L = {0.f, 0.f}, A = {0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const float2_t mw = st[w][0][lane];
                if (mw.x != -INFINITY) {
                    const float a = __expf(mw.x - M.x);
                    L.x += st[w][1][lane].x * a;
                    A.x += st[w][2][lane].x * a;
                }
                if (mw.y != -INFINITY) {
                    const float a = __expf(mw.y - M.y);
                    L.y += st[w][1][lane].y * a;
                    A.y += st[w][2][lane].y * a;
                }
            }
            if (act) Pair<T>::store(y + g * (int64_t)D + c, float2_t{A.x / (L.x + eps), A.y / (L.y + eps)});
        }
        __syncthreads();   // the states are read before the next task overwrites them
    }
}

// The SoftAgg entry points' shared checks in their order (true for a check an entry point does not
// make): the failed check's message for the caller to report under its own name, or nullptr.
const char* sa_bad_operands(int D, bool sizes_ok, int64_t ldf, int64_t lds, bool csr_ok)
{
    if (!(D > 0 && D % 2 == 0)) return "feature dim must be even and positive";
    if (!sizes_ok) return "bad sizes";
    if (!(ldf >= D && lds >= D && ldf % 2 == 0 && lds % 2 == 0)) return "row strides must be even and >= D";
    if (!csr_ok) return "CSR missing";
    return nullptr;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void gather_rows_kernel(const TI* __restrict__ x, int64_t ldx, int64_t rows,
                                                          const int64_t* __restrict__ idx, int64_t n, int D,
                                                          TO* __restrict__ out)
{
    // one wave per output row, 2 channels per lane per step
    const int lane = threadIdx.x & 63;
    for (int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; r < n;
         r += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t src = idx[r];
        const bool ok = src >= 0 && src < rows;
        for (int c = 2 * lane; c < D; c += 128) {
            float2_t v = {0.f, 0.f};
            if (ok) v = Pair<TI>::load(x + src * ldx + c);
            Pair<TO>::store(out + r * (int64_t)D + c, v);
        }
    }
}

// target = coords[..., P/2, P/2] + float(delta), weight = float(w) for every
// edge (DPVO.update after the update operator, dpvo.py:724-727), one launch
// instead of three.  delta / w: fp16 rows with their own strides (the fused
// operator's [E][4] head rows); c: the patch centre's x at c + e * cs, y at
// c + e * cs + cc.
__global__ __launch_bounds__(256) void edge_targets_kernel(const half_t* __restrict__ delta, int64_t ds,
                                                           const half_t* __restrict__ w, int64_t ws,
                                                           const float* __restrict__ c, int64_t cs, int64_t cc,
                                                           int64_t E, float* __restrict__ target,
                                                           float* __restrict__ weight)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        target[2 * e] = c[e * cs] + (float)delta[e * ds];
        target[2 * e + 1] = c[e * cs + cc] + (float)delta[e * ds + 1];
        weight[2 * e] = (float)w[e * ws];
        weight[2 * e + 1] = (float)w[e * ws + 1];
    }
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" size_t dpvo_softagg_workspace_bytes(int64_t num_edges, int64_t groups)
{
    return (size_t)sa_layout(num_edges < 0 ? 0 : num_edges, groups < 0 ? 0 : groups).total + 256;
}

extern "C" int dpvo_softagg_forward(int dtype, const void* f, int64_t ldf, const void* s, int64_t lds,
                                    const int64_t* group, int64_t num_edges, int D, int64_t groups, float eps,
                                    void* y, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* bad = sa_bad_operands(D, num_edges >= 0 && groups >= 0 && num_edges < (int64_t(1) << 31), ldf, lds,
                                      true);
    DPVO_CHECK_ARG(!bad, bad);
    DPVO_CHECK_ARG(dtype == DPVO_F16 || dtype == DPVO_F32 || dtype == DPVO_F64, "unsupported dtype");
    if (groups == 0) return 0;
    DPVO_CHECK_ARG(num_edges > 0, "groups without edges");
    const SaLayout L = sa_layout(num_edges, groups);
    DPVO_CHECK_ARG(workspace != nullptr && workspace_bytes >= (size_t)L.total + 256, "workspace too small");
    hipStream_t st = as_stream(stream);
    char* ws = align256(workspace);
    int* count = (int*)(ws + L.count);
    int* offs = (int*)(ws + L.offs);
    int* cursor = (int*)(ws + L.cursor);
    int* perm = (int*)(ws + L.perm);
    DPVO_CHECK_HIP(hipMemsetAsync(count, 0, 4 * groups, st));
    const unsigned gE = grid_for(num_edges, 256, 4096);
    hipLaunchKernelGGL(sa_count_kernel, dim3(gE), dim3(256), 0, st, group, num_edges, groups, count);
    hipLaunchKernelGGL(sa_scan_kernel, dim3(1), dim3(1024), 0, st, count, groups, offs, cursor);
    hipLaunchKernelGGL(sa_fill_kernel, dim3(gE), dim3(256), 0, st, group, num_edges, groups, cursor, perm);
    const int slices = (D + 127) / 128;
    const unsigned gR = (unsigned)((groups * slices + SA_WAVES - 1) / SA_WAVES);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(sa_reduce_kernel<T>, dim3(gR), dim3(64 * SA_WAVES), 0, st, (const T*)f, ldf, (const T*)s,
                           lds, offs, perm, groups, D, slices, eps, (T*)y);
    });
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_softagg_csr(int dtype, const void* f, int64_t ldf, const void* s, int64_t lds, const int* offs,
                                const int* perm, const int64_t* groups, int64_t max_groups, int D, float eps, void* y,
                                void* stream)
{
    const char* bad = sa_bad_operands(D, true, ldf, lds, groups != nullptr && offs != nullptr && perm != nullptr);
    DPVO_CHECK_ARG(!bad, bad);
    if (max_groups <= 0) return 0;
    hipStream_t st = as_stream(stream);
    const int slices = (D + 127) / 128;
    const unsigned grid = grid_for(max_groups * slices * 64, 256, 4096);
    const bool known = dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(sa_reduce_csr_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)f, ldf, (const T*)s, lds,
                           offs, perm, groups, D, slices, eps, (T*)y);
    });
    DPVO_CHECK_ARG(known, "unsupported dtype");
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_softagg_csr_long(int dtype, const void* f, int64_t ldf, const void* s, int64_t lds,
                                     const int* offs, const int* perm, const int64_t* groups, int64_t max_groups,
                                     int D, float eps, void* y, void* stream)
{
    const char* bad = sa_bad_operands(D, true, ldf, lds, groups != nullptr && offs != nullptr && perm != nullptr);
    DPVO_CHECK_ARG(!bad, bad);
    DPVO_CHECK_ARG(dtype == DPVO_F16 || dtype == DPVO_F32, "dtype must be fp16 or fp32");
    if (max_groups <= 0) return 0;
    const int slices = (D + 127) / 128;
    const unsigned grid = grid_for(max_groups * slices, 1, 8192);
    if (dtype == DPVO_F16)
        hipLaunchKernelGGL(sa_reduce_csr_split_kernel<half_t>, dim3(grid), dim3(256), 0, as_stream(stream),
                           (const half_t*)f, ldf, (const half_t*)s, lds, offs, perm, groups, D, slices, eps,
                           (half_t*)y);
    else
        hipLaunchKernelGGL(sa_reduce_csr_split_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream),
                           (const float*)f, ldf, (const float*)s, lds, offs, perm, groups, D, slices, eps, (float*)y);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_gather_rows(int in_dtype, const void* x, int64_t ldx, int64_t rows, const int64_t* idx, int64_t n,
                                int D, int out_dtype, void* out, void* stream)
{
    DPVO_CHECK_ARG(D > 0 && D % 2 == 0 && ldx >= D && ldx % 2 == 0, "feature dim / row stride must be even");
    DPVO_CHECK_ARG(n >= 0 && rows >= 0, "bad sizes");
    if (n == 0) return 0;
    hipStream_t s = as_stream(stream);
    const unsigned grid = grid_for(n * 64, 256, 8192);
    bool out_known = false;
    const bool in_known = dispatch_dtype(in_dtype, [&](auto ti) {
        out_known = dispatch_dtype(out_dtype, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            hipLaunchKernelGGL((gather_rows_kernel<TI, TO>), dim3(grid), dim3(256), 0, s, (const TI*)x, ldx, rows, idx,
                               n, D, (TO*)out);
        });
    });
    DPVO_CHECK_ARG(in_known && out_known, "unsupported dtype");
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_edge_targets(const void* delta, int64_t delta_stride, const void* w, int64_t w_stride,
                                 const float* centre, int64_t centre_stride, int64_t centre_comp, int64_t E,
                                 float* target, float* weight, void* stream)
{
    DPVO_CHECK_ARG(E >= 0, "E >= 0 required");
    if (E == 0) return 0;
    DPVO_CHECK_ARG(delta && w && centre && target && weight, "null operand");
    hipLaunchKernelGGL(edge_targets_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, as_stream(stream),
                       (const half_t*)delta, delta_stride, (const half_t*)w, w_stride, centre, centre_stride,
                       centre_comp, E, target, weight);
    DPVO_CHECK_LAUNCH();
    return 0;
}
