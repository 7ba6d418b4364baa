// select.hip -- the Patchifier's two non-uniform patch-centre selections as
// device code with fixed launch shapes and no host read (gfx950), so that they
// sit inside the captured ingest graph:
//   dpvo_select_gradient  the M of C random candidates with the largest image
//                         gradient (net.py:103-109,129-134), one launch
//   dpvo_select_mask      M cells of a validity mask in uniform random order
//                         (net.py:141-144), two launches
// Both are launch-bound and select in LDS (rank by counting, 64 candidates per
// workgroup; a radix select of the caller's random keys in one workgroup), with
// integer arithmetic and integer LDS atomics only -- the result does not
// depend on which wave arrives first.
#include "common.hpp"

namespace dpvo {
namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int GRAD_MAX_C = 8192;    // candidate scores in LDS (32 KiB); the tracker's C is 3 * 384
constexpr int MASK_MAX_M = 4096;    // selected (key, cell) words in LDS (32 KiB)
constexpr int RADIX_BINS = 2048;
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;   // vkey of a cell that is not valid
// the radix select's digits of u = key << 32 | cell from the top: the 31 key
// bits (62 .. 32), then the cell bits
constexpr int RADIX_LEVELS = 6;
__device__ const int radix_shift[RADIX_LEVELS] = {52, 41, 32, 22, 11, 0};
__device__ const int radix_width[RADIX_LEVELS] = {11, 11, 9, 10, 11, 11};

// ---------------------------------------------------------------------------
// gradient-biased selection
// ---------------------------------------------------------------------------
// mean over the 4x4 block at (4 y, 4 x) of sqrt(dx^2 + dy^2) on gray = R + G + B
// (the reference's ((2 u / 255 - 0.5) + 0.5) * 127.5 summed over channels is that
// integer on 8-bit frames); dx^2 + dy^2 <= 2 * 765^2 < 2^24 is exact in fp32, the
// square root is correctly rounded, the 16 terms are added in row-major order.
// 0 outside the pooled [(H - 1) / 4][(W - 1) / 4] map.  Inside it the 5 x 5 byte
// window ends at row 4 y + 4 <= H - 1 and column 4 x + 4 <= W - 1.
__device__ float gradient_score(const uint8_t* __restrict__ image, int H, int W, int64_t x, int64_t y)
{
    const int ph = (H - 1) / 4, pw = (W - 1) / 4;
    if (x < 0 || x >= pw || y < 0 || y >= ph) return 0.0f;
    const int64_t plane = (int64_t)H * W;
    const uint8_t* p = image + (4 * y) * W + 4 * x;
    int g[5][5];
#pragma unroll
    for (int r = 0; r < 5; r++)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const int64_t o = (int64_t)r * W + c;
            g[r][c] = (int)p[o] + (int)p[plane + o] + (int)p[2 * plane + o];
        }
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int dx = g[r][c + 1] - g[r][c], dy = g[r + 1][c] - g[r][c];
            s += __fsqrt_rn((float)(dx * dx + dy * dy));
        }
    return s * 0.0625f;
}

// One workgroup per 64 candidates.  rank(c) = #{j : (s_j, j) < (s_c, c)} is the
// candidate's place in the stable ascending argsort; ranks C - M .. C - 1 go to
// out[0 .. M).  (One workgroup for all of them took 0.1 ms at C = 1152: 1.3 M
// comparisons on one CU.)
__global__ __launch_bounds__(SEL_THREADS) void select_gradient_kernel(
    const uint8_t* __restrict__ image, int H, int W, const int64_t* __restrict__ cand_x,
    const int64_t* __restrict__ cand_y, int C, int M, int64_t* __restrict__ out_x, int64_t* __restrict__ out_y,
    float* __restrict__ scores)
{
    __shared__ __attribute__((aligned(16))) float sc[GRAD_MAX_C];
    __shared__ int rank[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C4 = (C + 3) & ~3;
    // every workgroup scores all C candidates (a few byte loads each, from L2):
    // cheaper than a second launch, and the C^2 comparisons spread over the grid
    for (int c = tid; c < C4; c += SEL_THREADS) {
        float s = 0.0f;   // (the pad never counts: it is compared only as j < C)
        if (c < C) {
            s = gradient_score(image, H, W, cand_x[c], cand_y[c]);
            if (scores && blockIdx.x == 0) scores[c] = s;
        }
        sc[c] = s;
    }
    if (tid < 64) rank[tid] = 0;
    __syncthreads();
    // this workgroup ranks 64 candidates, one per lane; each of its 16 waves
    // counts over a sixteenth of the scores (integer adds: any order)
    const int c = blockIdx.x * 64 + lane;
    const int per = ((C4 / 4 + SEL_WAVES - 1) / SEL_WAVES) * 4;
    const int j0 = wave * per, j1 = min(j0 + per, C4);
    if (c < C) {
        const float s = sc[c];
        int part = 0;
        // every lane reads the same four scores: one broadcast 16-byte LDS read
        for (int j = j0; j < j1; j += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&sc[j]);
            part += (v.x < s || (v.x == s && j < c)) && j < C;
            part += (v.y < s || (v.y == s && j + 1 < c)) && j + 1 < C;
            part += (v.z < s || (v.z == s && j + 2 < c)) && j + 2 < C;
            part += (v.w < s || (v.w == s && j + 3 < c)) && j + 3 < C;
        }
        atomicAdd(&rank[lane], part);
    }
    __syncthreads();
    if (wave == 0 && c < C) {
        const int m = rank[lane] - (C - M);
        if (m >= 0 && m < M) {
            out_x[m] = cand_x[c];
            out_y[m] = cand_y[c];
        }
    }
}

// ---------------------------------------------------------------------------
// masked selection
// ---------------------------------------------------------------------------
// launch 1: vkey[cy * w + cx] = the caller's key where the cell is valid (some
// mask byte of its 4 x 4 block is set, cx < w - 1, cy < h - 1), NO_CELL elsewhere.
// One thread per four cells of a cell row: four 16-byte loads of the mask rows
// where the rows are 16-byte aligned, bytes elsewhere (frame edges, odd widths).
__global__ __launch_bounds__(256) void mask_cells_kernel(const uint8_t* __restrict__ mask, int H, int W, int h, int w,
                                                         const int* __restrict__ keys, uint32_t* __restrict__ vkey,
                                                         int aligned16)
{
    const int gw = (w + 3) / 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)h * gw) return;
    const int cy = (int)(t / gw), g = (int)(t % gw);
    unsigned any[4] = {0, 0, 0, 0};
    const int c0 = 16 * g;
    for (int dr = 0; dr < 4; dr++) {
        const int r = 4 * cy + dr;
        if (r >= H) break;
        const uint8_t* row = mask + (int64_t)r * W;
        if (aligned16 && c0 + 16 <= W) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + c0);
            any[0] |= v.x;
            any[1] |= v.y;
            any[2] |= v.z;
            any[3] |= v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int c = c0 + 4 * j + q;
                    if (c < W) any[j] |= row[c];
                }
        }
    }
    for (int j = 0; j < 4; j++) {
        const int cx = 4 * g + j;
        if (cx >= w) break;
        const int64_t cell = (int64_t)cy * w + cx;
        const bool valid = any[j] != 0 && cx < w - 1 && cy < h - 1;
        vkey[cell] = valid ? ((uint32_t)keys[cell] & 0x7FFFFFFFu) : NO_CELL;
    }
}

// f(cell, vkey[cell]) over all n cells, 16-byte loads (vkey is 16-byte aligned)
template <typename F>
__device__ __forceinline__ void for_each_vkey(const uint32_t* __restrict__ vkey, int n, F f)
{
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += SEL_THREADS) {
        const uint4 v = reinterpret_cast<const uint4*>(vkey)[i];
        f(4 * i, v.x);
        f(4 * i + 1, v.y);
        f(4 * i + 2, v.z);
        f(4 * i + 3, v.w);
    }
    const int i = 4 * n4 + threadIdx.x;
    if (i < n) f(i, vkey[i]);
}

// launch 2, one workgroup: the min(M, K) smallest of the K valid cells'
// u = key << 32 | cell (distinct words, so their order is the contract's
// (key, cell) order), by a radix select from the top digit down -- it stops at
// the first digit whose boundary bin is taken whole, the second for distinct
// random keys; equal keys go on into the cell bits -- then the survivors are
// ranked by counting and written to out[rank], cyclically repeated when K < M.
__global__ __launch_bounds__(SEL_THREADS) void select_mask_kernel(const uint32_t* __restrict__ vkey, int n, int w,
                                                                  int M, int64_t* __restrict__ out_x,
                                                                  int64_t* __restrict__ out_y, int* __restrict__ count)
{
    __shared__ int hist[RADIX_BINS];
    __shared__ int wave_sum[SEL_WAVES];
    __shared__ int found[3];   // the boundary bin, the count below it, its own count
    __shared__ int nsurv;
    __shared__ uint64_t surv[MASK_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t prefix = 0;   // the selected words are those with (u >> shift) <= prefix
    int shift = 0;
    int need = 0, K = 0;
    for (int level = 0; level < RADIX_LEVELS; level++) {
        const int width = radix_width[level];
        shift = radix_shift[level];
        const int hi = shift + width;
        const uint32_t dmask = (1u << width) - 1;
        for (int b = tid; b < RADIX_BINS; b += SEL_THREADS) hist[b] = 0;
        __syncthreads();
        for_each_vkey(vkey, n, [&](int cell, uint32_t k) {
            if (k == NO_CELL) return;
            const uint64_t u = ((uint64_t)k << 32) | (uint32_t)cell;
            if ((u >> hi) == prefix) atomicAdd(&hist[(uint32_t)(u >> shift) & dmask], 1);
        });
        __syncthreads();
        // inclusive scan over the bins, two per thread
        const int a = hist[2 * tid], b = hist[2 * tid + 1];
        int incl = a + b;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int base = 0, total = 0;
        for (int v = 0; v < SEL_WAVES; v++) {
            const int s = wave_sum[v];
            base += v < wave ? s : 0;
            total += s;
        }
        if (level == 0) {
            K = total;
            need = min(M, K);
            if (K == 0) break;   // (uniform: every thread sees the same total)
        }
        const int excl = base + incl - (a + b);
        if (excl < need && need <= excl + a) {
            found[0] = 2 * tid, found[1] = excl, found[2] = a;
        } else if (excl + a < need && need <= excl + a + b) {
            found[0] = 2 * tid + 1, found[1] = excl + a, found[2] = b;
        }
        __syncthreads();
        prefix = (prefix << width) | (uint32_t)found[0];
        need -= found[1];
        const bool whole = found[2] == need;   // always at shift 0: the words are distinct
        __syncthreads();
        if (whole) break;
    }
    if (tid == 0) {
        count[0] = K;
        nsurv = 0;
    }
    if (K == 0) {
        for (int m = tid; m < M; m += SEL_THREADS) out_x[m] = 1, out_y[m] = 1;
        return;
    }
    __syncthreads();
    const int S = min(M, K);
    for_each_vkey(vkey, n, [&](int cell, uint32_t k) {
        if (k == NO_CELL) return;
        const uint64_t u = ((uint64_t)k << 32) | (uint32_t)cell;
        if ((u >> shift) <= prefix) {
            const int i = atomicAdd(&nsurv, 1);   // (any order: the ranks below restore it)
            if (i < S) surv[i] = u;
        }
    });
    __syncthreads();
    for (int i = tid; i < S; i += SEL_THREADS) {
        const uint64_t u = surv[i];
        int rank = 0;
        for (int j = 0; j < S; j++) rank += surv[j] < u;
        const uint32_t cell = (uint32_t)u;
        const int64_t cx = cell % (uint32_t)w, cy = cell / (uint32_t)w;
        for (int m = rank; m < M; m += K) out_x[m] = cx, out_y[m] = cy;
    }
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" int dpvo_select_gradient(const uint8_t* image, int H, int W, const int64_t* cand_x, const int64_t* cand_y,
                                    int64_t C, int64_t M, int64_t* out_x, int64_t* out_y, float* scores, void* stream)
{
    DPVO_CHECK_ARG(H >= 8 && W >= 8, "the frame must be at least 8 x 8");
    DPVO_CHECK_ARG(C >= 0 && M >= 0, "bad sizes");
    DPVO_CHECK_ARG(M <= C, "M candidates cannot be kept out of fewer (M > C)");
    DPVO_CHECK_ARG(C <= GRAD_MAX_C, "at most 8192 candidates");
    if (C == 0 || (M == 0 && scores == nullptr)) return 0;
    DPVO_CHECK_ARG(image && cand_x && cand_y, "null operand");
    DPVO_CHECK_ARG(M == 0 || (out_x && out_y), "null output");
    hipLaunchKernelGGL(select_gradient_kernel, dim3((unsigned)((C + 63) / 64)), dim3(SEL_THREADS), 0,
                       as_stream(stream), image, H, W, cand_x,
                       cand_y, (int)C, (int)M, out_x, out_y, scores);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpvo_select_mask_workspace_bytes(int h, int w)
{
    if (h <= 0 || w <= 0) return 16;
    return (((size_t)h * (size_t)w * sizeof(uint32_t)) + 15) & ~(size_t)15;
}

extern "C" int dpvo_select_mask(const uint8_t* mask, int H, int W, int h, int w, const int* keys, int64_t M,
                                int64_t* out_x, int64_t* out_y, int* count, void* workspace, void* stream)
{
    DPVO_CHECK_ARG(H >= 1 && W >= 1 && h >= 1 && w >= 1, "bad sizes");
    DPVO_CHECK_ARG((int64_t)h * w < (int64_t(1) << 31), "at most 2^31 - 1 cells");
    DPVO_CHECK_ARG(M >= 0 && M <= MASK_MAX_M, "M must be in [0, 4096]");
    if (M == 0) return 0;
    DPVO_CHECK_ARG(mask && keys && out_x && out_y && count && workspace, "null operand");
    DPVO_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    uint32_t* vkey = (uint32_t*)workspace;
    const int gw = (w + 3) / 4;
    const int aligned16 = ((uintptr_t)mask & 15) == 0 && W % 16 == 0;
    hipLaunchKernelGGL(mask_cells_kernel, dim3(grid_for((int64_t)h * gw, 256, int64_t(1) << 30)), dim3(256), 0, st,
                       mask, H, W, h, w, keys, vkey, aligned16);
    DPVO_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_mask_kernel, dim3(1), dim3(SEL_THREADS), 0, st, (const uint32_t*)vkey, h * w, w, (int)M,
                       out_x, out_y, count);
    DPVO_CHECK_LAUNCH();
    return 0;
}
