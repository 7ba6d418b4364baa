// retrieval.hip -- descriptor retrieval for loop closure: the reference's
// query_online (dpvo/netvlad_retrieval.py:89-104: torch.matmul of the rows
// before idx - skip_window with the query row, then torch.topk), for Q
// queries in one call, masked on the device and bitwise repeatable.
//
// score kernel: the grid follows the db rows (a wave takes R consecutive rows,
// four waves per workgroup) and the query chunks (QC queries, grid.y), so a
// single query (R = 1, QC = 1) still spreads over the device; a batch runs
// R = 4, QC = 8: per 16 bytes of the feature dimension a wave loads 4 row and
// 8 query pieces for 32 products (the query rows through L1/L2: every wave of
// the chunk reads the same ones).  Lane l owns the elements
// 4 l + 256 i .. 4 l + 256 i + 3 and accumulates them with fmaf in ascending
// order into one fp32; wave64_sum is a fixed tree.  The bits of a score so
// depend on its two rows and D alone: not on Q, on the query's place in the
// batch (both instantiations run the same chain per score), on N or on the
// grid.  Rows that are candidates of no query of the chunk are not read;
// a row that is a candidate of some query but not of another is computed for
// all and discarded by a select, so what it holds (NaN) reaches no output.
//
// top-k kernel: one workgroup per query.  k rounds; round k takes the largest
// score after the previous pick in the total order (score descending, row
// ascending).  A maximum over a total order does not depend on the order the
// reduction visits the candidates in, so ties come out by ascending row.
// NaN scores are never picked.
#include <math.h>

#include "common.hpp"

namespace dpvo {
namespace retrieval {

enum { BLOCK = 256, WAVES = BLOCK / 64, QCHUNK = 8, QROWS = 4, MAX_TOPK = 32 };
enum : int64_t { MAX_ROWS = 1 << 24, MAX_QUERIES = 1 << 16 };

// the end of query row n's candidate range, 0 for a row outside [0, N)
__device__ __forceinline__ int64_t candidate_end(int64_t n, int64_t N, int64_t skip)
{
    const int64_t e = (n >= 0 && n < N) ? n - skip : 0;
    return e > 0 ? e : 0;
}

// U steps of 256 elements from element d on: per step 16 bytes per lane of every row and of every query row,
// R x QC x 4 products.  All loads first, so they are in flight together (the single-query kernel is latency-bound:
// U = 8), then the products in ascending order.  No branch: the query slots past the chunk's last query point at a
// valid row and are discarded by the caller.
template <int R, int QC, int U>
__device__ __forceinline__ void steps(const float* const (&row)[R], const float* const (&qrow)[QC], int d,
                                      float (&acc)[R][QC])
{
    float4 a[U][R], b[U][QC];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int j = 0; j < R; j++) a[u][j] = *reinterpret_cast<const float4*>(row[j] + d + u * 256);
#pragma unroll
        for (int q = 0; q < QC; q++) b[u][q] = *reinterpret_cast<const float4*>(qrow[q] + d + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int q = 0; q < QC; q++)
#pragma unroll
            for (int j = 0; j < R; j++) {
                acc[j][q] = __builtin_fmaf(a[u][j].x, b[u][q].x, acc[j][q]);
                acc[j][q] = __builtin_fmaf(a[u][j].y, b[u][q].y, acc[j][q]);
                acc[j][q] = __builtin_fmaf(a[u][j].z, b[u][q].z, acc[j][q]);
                acc[j][q] = __builtin_fmaf(a[u][j].w, b[u][q].w, acc[j][q]);
            }
}

template <int QC, int R>
__global__ __launch_bounds__(BLOCK) void score_kernel(const float* __restrict__ db, int64_t ld, int64_t N, int D,
                                                      const int64_t* __restrict__ query_rows, int64_t Q, int64_t skip,
                                                      float* __restrict__ ws, float* __restrict__ out_scores)
{
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * R;   // the wave's rows r0 .. r0 + R - 1
    if (r0 >= N) return;   // the whole wave
    const int64_t q0 = (int64_t)blockIdx.y * QC;
    const int nq = (int)(Q - q0 < QC ? Q - q0 : QC);
    int64_t end[QC], last = 0;
    const float* qrow[QC];
#pragma unroll
    for (int q = 0; q < QC; q++) {
        const int64_t n = q < nq ? query_rows[q0 + q] : -1;
        end[q] = candidate_end(n, N, skip);
        qrow[q] = db + (end[q] > 0 ? n : 0) * ld;
        last = end[q] > last ? end[q] : last;
    }
    float acc[R][QC];
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
        for (int q = 0; q < QC; q++) acc[j][q] = 0.f;
    if (r0 < last) {   // wave-uniform: a candidate of at least one query of the chunk
        // rows past the chunk's largest range are not read: their slot re-reads row last - 1 and is discarded below
        const float* row[R];
#pragma unroll
        for (int j = 0; j < R; j++) row[j] = db + (r0 + j < last ? r0 + j : last - 1) * ld;
        // whole 256-element blocks (every lane takes part, a wave-uniform trip count), then the lanes of the last
        // partial block: ascending i for every lane, whatever the unrolling
        constexpr int UNROLL = R * QC == 1 ? 8 : 1;
        const int nfull = D >> 8, tail = D & 255;
        int i = 0;
        for (; i + UNROLL <= nfull; i += UNROLL) steps<R, QC, UNROLL>(row, qrow, lane * 4 + i * 256, acc);
        for (; i < nfull; i++) steps<R, QC, 1>(row, qrow, lane * 4 + i * 256, acc);
        if (lane * 4 < tail) steps<R, QC, 1>(row, qrow, lane * 4 + nfull * 256, acc);
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int64_t r = r0 + j;
        if (r >= N) break;   // wave-uniform
#pragma unroll
        for (int q = 0; q < QC; q++) {
            if (q < nq) {
                const bool cand = r < end[q];
                const float sum = wave64_sum(acc[j][q]);
                const float s = cand ? sum : -INFINITY;
                if (lane == 0) {
                    if (cand) ws[(q0 + q) * N + r] = s;
                    if (out_scores) out_scores[(q0 + q) * N + r] = s;
                }
            }
        }
    }
}

__device__ __forceinline__ bool better(float v, int64_t i, float bv, int64_t bi)
{
    return i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi));
}

__global__ __launch_bounds__(BLOCK) void topk_kernel(const float* __restrict__ ws, int64_t N,
                                                     const int64_t* __restrict__ query_rows, int64_t skip, int top_k,
                                                     float* __restrict__ out_val, int64_t* __restrict__ out_idx)
{
    __shared__ float s_v[WAVES];
    __shared__ long long s_i[WAVES];
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t end = candidate_end(query_rows[q], N, skip);
    const float* __restrict__ s = ws + q * N;
    float pv = INFINITY;   // the previous pick: everything comes after (+inf, -1)
    long long pi = -1;
    for (int k = 0; k < top_k; k++) {
        float bv = -INFINITY;
        long long bi = -1;
        for (int64_t i = t; i < end; i += BLOCK) {
            const float v = s[i];
            const bool after = v < pv || (v == pv && i > pi);   // false for NaN
            if (after && (bi < 0 || v > bv)) { bv = v; bi = i; }   // ascending i: a tie keeps the earlier row
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const long long oi = __shfl_xor(bi, off, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if ((t & 63) == 0) { s_v[t >> 6] = bv; s_i[t >> 6] = bi; }
        __syncthreads();
        bv = s_v[0]; bi = s_i[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++)
            if (better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
        __syncthreads();
        if (t == 0) {
            out_val[q * top_k + k] = bi >= 0 ? bv : -INFINITY;
            out_idx[q * top_k + k] = bi;
        }
        if (bi < 0) {   // uniform: the candidates are used up, the rest is tail
            if (t == 0)
                for (int kk = k + 1; kk < top_k; kk++) { out_val[q * top_k + kk] = -INFINITY; out_idx[q * top_k + kk] = -1; }
            return;
        }
        pv = bv; pi = bi;
    }
}

static bool shape_ok(int64_t Q, int64_t N, int top_k)
{
    return Q >= 1 && Q <= MAX_QUERIES && N >= 1 && N <= MAX_ROWS && top_k >= 1 && top_k <= MAX_TOPK;
}

}  // namespace retrieval
}  // namespace dpvo

using namespace dpvo;
using namespace dpvo::retrieval;

extern "C" size_t dpvo_retrieval_workspace_bytes(int64_t Q, int64_t N, int top_k)
{
    if (!shape_ok(Q, N, top_k)) return 0;
    return ((size_t)Q * (size_t)N * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int dpvo_retrieval_query(const float* db, int64_t ld, int64_t N, int D, const int64_t* query_rows, int64_t Q,
                                    int64_t skip_window, int top_k, float* out_val, int64_t* out_idx, float* out_scores,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    DPVO_CHECK_ARG(top_k >= 1 && top_k <= MAX_TOPK, "need 1 <= top_k <= 32");
    DPVO_CHECK_ARG(N >= 1 && N <= MAX_ROWS, "need 1 <= N <= 2^24 rows");
    DPVO_CHECK_ARG(Q >= 1 && Q <= MAX_QUERIES, "need 1 <= Q <= 2^16 queries");
    DPVO_CHECK_ARG(D >= 4 && D <= (1 << 20) && D % 4 == 0, "D must be a multiple of 4 in [4, 2^20]");
    DPVO_CHECK_ARG(ld >= D && ld % 4 == 0, "need ld >= D and ld % 4 == 0");
    DPVO_CHECK_ARG(skip_window >= 0, "skip_window must be >= 0");
    DPVO_CHECK_ARG(db && query_rows && out_val && out_idx, "db / query_rows / outputs missing");
    DPVO_CHECK_ARG(((uintptr_t)db & 15) == 0, "db must be 16-byte aligned");
    DPVO_CHECK_ARG(workspace && workspace_bytes >= dpvo_retrieval_workspace_bytes(Q, N, top_k),
                   "workspace too small (dpvo_retrieval_workspace_bytes)");
    DPVO_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "workspace must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    float* ws = (float*)workspace;
    if (Q == 1) {
        const unsigned tiles = (unsigned)((N + WAVES - 1) / WAVES);
        hipLaunchKernelGGL((score_kernel<1, 1>), dim3(tiles, 1), dim3(BLOCK), 0, s, db, ld, N, D, query_rows, Q,
                           skip_window, ws, out_scores);
    } else {
        const unsigned tiles = (unsigned)((N + WAVES * QROWS - 1) / (WAVES * QROWS));
        hipLaunchKernelGGL((score_kernel<QCHUNK, QROWS>), dim3(tiles, (unsigned)((Q + QCHUNK - 1) / QCHUNK)),
                           dim3(BLOCK), 0, s, db, ld, N, D, query_rows, Q, skip_window, ws, out_scores);
    }
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)Q), dim3(BLOCK), 0, s, ws, N, query_rows, skip_window, top_k, out_val,
                       out_idx);
    DPVO_CHECK_LAUNCH();
    return 0;
}
