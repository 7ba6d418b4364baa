// rowgemm_rowmajor.hip -- rowgemm3_kernel: the full-row GEMM on a ROW-MAJOR W
// ([384][K]) staged by LDS-DMA, with every row epilogue of dpvo_rowgemm.  What
// dpvo_rowgemm runs without DPVO_RG_WKB, and the two-launch form of
// dpvo_rowgemm_pair; nothing in DPVO.update() reaches it (the hot path is the
// k-blocked family, rowgemm_kblocked.hip) -- it is the reference the k-blocked
// kernels are bit-identical to, and what the tests compose them from.
//
// Tiling: 512 threads = 8 waves as 2 (M) x 4 (N); wave tile 64 x 96 =
// 4 x 6 mfma_f32_16x16x32_f16 accumulators.  BK = 64; A (16 KB) and W (48 KB)
// stages are staged global -> LDS by global_load_lds (16 B per lane, source
// pre-swizzled, conflict-free ds_read_b128 fragment reads).  Persistent blocks
// walk a flat (tile, k-stage) sequence, so the next tile's first stage loads
// during the current tile's epilogue.
#include "rowgemm.hpp"

namespace dpvo {
namespace {

// ---------------------------------------------------------------------------
// v3: the v1 tiling (128 x 384, 8 waves, BK = 64) with the A stream prefetched
// TWO stages ahead instead of one.  A (the activations, 73 MB per layer at C3)
// is the HBM stream; W (295 KB) is L2-resident.  In v1 a stage holds A and W
// together, so one stage of lookahead leaves only 16 KB of A in flight per CU
// (4 MB chip-wide, ~2 TB/s at HBM latency).  Here W has 2 slots (48 KB) and A
// a ring of 3 (16 KB), issued in the order W(i+1), A(i+2): the wait for step i
// (vmcnt 10) then leaves A(i+1) and A(i+2) in flight.  The 96 KB y tile no
// longer fits beside the rings, so the epilogue runs in two 64-row halves
// through the consumed W slot.
// ---------------------------------------------------------------------------
constexpr int R3_W_SLOT = RG_W_STAGE;            // 48 KB
constexpr int R3_A_BASE = 2 * R3_W_SLOT;         // A ring after the two W slots
constexpr int R3_LDS = R3_A_BASE + 3 * RG_A_STAGE;   // 144 KB

template <int FLAGS, bool DUAL = false>
__global__ __launch_bounds__(RG_THREADS, 1) void rowgemm3_kernel(dpvo_rowgemm_args p, dpvo_rowgemm_args p2)
{
    __shared__ __attribute__((aligned(16))) char smem[R3_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int K = p.K;
    const int ksteps = K / RG_BK;
    const int64_t Mrows = p.M_dev ? min(*p.M_dev, p.M) : p.M;
    const int64_t ntiles = (Mrows + RG_BM - 1) / RG_BM;
    if ((int64_t)blockIdx.x >= ntiles) return;
    // DUAL: a second GEMM on the same A (p2's W, bias, outputs): every tile runs
    // twice in a row, the second pass's A stream hitting L2
    const int64_t my_tiles = ((ntiles - 1 - blockIdx.x) / gridDim.x + 1) << (DUAL ? 1 : 0);
    const int64_t total = my_tiles * ksteps;
    const int64_t wdelta = DUAL ? (const half_t*)p2.W - (const half_t*)p.W : 0;

    const half_t* __restrict__ Wt = (const half_t*)p.W;
    const half_t* __restrict__ zero = (const half_t*)p.zero_row;
    const int srow = lane >> 3, pch = lane & 7;
    const half_t* wsrc[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const int n = (wave * 6 + j) * 8 + srow;
        wsrc[j] = Wt + (int64_t)n * K + 8 * (pch ^ ((n >> 1) & 7));
    }
    // A rows of the tile a flat step belongs to (two tiles can be in flight)
    auto a_src = [&](int64_t tile, int j) {
        const int r = (wave * 2 + j) * 8 + srow;
        const int64_t m = tile * RG_BM + r;
        const half_t* row = zero;
        if (m < Mrows) {
            const int64_t s = p.a_idx ? p.a_idx[m] : m;
            if (s >= 0 && s < p.a_rows) row = (const half_t*)p.A + s * p.lda;
        }
        return row + 8 * (pch ^ ((r >> 1) & 7));
    };
    // flat step f -> (tile, k-step) of this block
    auto tile_of = [&](int64_t f) { return (int64_t)blockIdx.x + ((f / ksteps) >> (DUAL ? 1 : 0)) * gridDim.x; };
    auto second = [&](int64_t f) { return DUAL && ((f / ksteps) & 1); };
    const half_t* asrc[2];
    int64_t asrc_tile = -1;
    auto issue_a = [&](int64_t f) {
        const int64_t t = tile_of(f);
        if (t != asrc_tile) {
            asrc[0] = a_src(t, 0);
            asrc[1] = a_src(t, 1);
            asrc_tile = t;
        }
        char* sA = smem + R3_A_BASE + (int)(f % 3) * RG_A_STAGE;
        const int k0 = (int)(f % ksteps) * RG_BK;
        glds16(asrc[0] + k0, sA + (wave * 2 + 0) * 1024);
        glds16(asrc[1] + k0, sA + (wave * 2 + 1) * 1024);
    };
    auto issue_w = [&](int64_t f) {
        char* sW = smem + (int)(f & 1) * R3_W_SLOT;
        const int64_t k0 = (f % ksteps) * RG_BK + (second(f) ? wdelta : 0);
#pragma unroll
        for (int j = 0; j < 6; j++) glds16(wsrc[j] + k0, sW + (wave * 6 + j) * 1024);
    };

    f4_t acc[4][6];
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 6; nt++) acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    int a_off[4], w_off[6], a_sw[4], w_sw[6];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        const int row = wm * 64 + mt * 16 + fr;
        a_off[mt] = row * 128;
        a_sw[mt] = (row >> 1) & 7;
    }
#pragma unroll
    for (int nt = 0; nt < 6; nt++) {
        const int n = wn * 96 + nt * 16 + fr;
        w_off[nt] = n * 128;
        w_sw[nt] = (n >> 1) & 7;
    }

    EpiConsts2 kc;
    load_consts2<FLAGS>(p, lane, kc);
    // prologue: A(0), W(0), A(1) -- then every step issues W(i+1), A(i+2)
    issue_a(0);
    issue_w(0);
    if (total > 1) issue_a(1);
    for (int64_t i = 0; i < total; i++) {
        const bool w_next = i + 1 < total, a_next = i + 2 < total;
        if (w_next) issue_w(i + 1);
        if (a_next) issue_a(i + 2);
        // outstanding after W(i): A(i+1) [2], W(i+1) [6], A(i+2) [2]
        if (a_next)
            asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (w_next)
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* sA = smem + R3_A_BASE + (int)(i % 3) * RG_A_STAGE;
        const char* sW = smem + (int)(i & 1) * R3_W_SLOT;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            const int c = kk * 4 + fq;
            h8_t a[4], b[6];
#pragma unroll
            for (int mt = 0; mt < 4; mt++) a[mt] = *(const h8_t*)(sA + a_off[mt] + 16 * (c ^ a_sw[mt]));
#pragma unroll
            for (int nt = 0; nt < 6; nt++) b[nt] = *(const h8_t*)(sW + w_off[nt] + 16 * (c ^ w_sw[nt]));
            // W as the first operand: the accumulator is the transposed tile, lane
            // (fr, fq) holding row fr, columns 4 fq .. 4 fq + 3 of each 16 x 16 block
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < 6; nt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[nt], a[mt], acc[mt][nt], 0, 0, 0);
        }
        __builtin_amdgcn_s_barrier();
        if ((int)(i % ksteps) != ksteps - 1) continue;

        // ---- epilogue of tile t.  y16 = act(fp16(acc + b)): four consecutive
        // columns of one row per (m-tile, n-tile) and lane.
        const int64_t cur_tile = tile_of(i);
        const bool sec = second(i);
        const dpvo_rowgemm_args& pe = sec ? p2 : p;
        h4_t y16[4][6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const h4_t bias = *(const h4_t*)((const half_t*)pe.bias + wn * 96 + nt * 16 + 4 * fq);
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                y16[mt][nt] = rg_y4(acc[mt][nt], bias, (FLAGS & RG_RELU) != 0, (FLAGS & RG_SIGMOID) != 0);
                acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
            }
        }
        // Two 64-row halves through the consumed W slot (whole-row stores are
        // coalesced; 8-byte stores straight from the accumulator layout measured
        // slower even with no row-wise op).  Half h holds tile rows
        // {64 w + 32 h + [0, 32)}, w = 0, 1: every wave writes its m-tiles 2h,
        // 2h+1, so only half of y16 stays live across the first half's row pass.
        const YMapSlot ym{(int)(i & 1) * R3_W_SLOT};
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const int col = wn * 96 + nt * 16 + 4 * fq;
#pragma unroll
                for (int mm = 0; mm < 2; mm++)
                    *(h4_t*)(smem + ym.off(wm * 32 + mm * 16 + fr, col * 2)) = y16[2 * h + mm][nt];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // rows per batch (register budget: half of y16 is still live here)
            constexpr int RB = (FLAGS & (RG_RES | RG_GATE | RG_LN)) ? ((FLAGS & (RG_LN | RG_HEADS)) ? 2 : 4) : 8;
            const int lr = wave * 8;                                             // 8 rows inside one 32-row block
            const int64_t row0 = cur_tile * RG_BM + (lr >> 5) * 64 + h * 32 + (lr & 31);
#pragma unroll
            for (int q0 = 0; q0 < 8; q0 += RB)
                epilogue_rows2<FLAGS, RB>(pe, Mrows, smem, ym, lr + q0, row0 + q0, lane, kc);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
    }
}

template <int FLAGS, bool DUAL = false>
int launch3(const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid, hipStream_t stream)
{
    hipLaunchKernelGGL((rowgemm3_kernel<FLAGS, DUAL>), dim3(grid), dim3(RG_THREADS), 0, stream, a, b);
    return 0;
}

}  // namespace

int launch_rowgemm3(int flags, bool dual, const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid,
                    hipStream_t stream)
{
    if (dual) return flags == 0 ? launch3<0, true>(a, b, grid, stream) : -1;
    switch (flags) {
    case 0: return launch3<0>(a, b, grid, stream);
    case RG_RELU: return launch3<RG_RELU>(a, b, grid, stream);
    case RG_SIGMOID: return launch3<RG_SIGMOID>(a, b, grid, stream);
    case RG_LN | RG_LN_RELU: return launch3<RG_LN | RG_LN_RELU>(a, b, grid, stream);
    case RG_RES: return launch3<RG_RES>(a, b, grid, stream);
    case RG_RES | RG_LN: return launch3<RG_RES | RG_LN>(a, b, grid, stream);
    case RG_GATE | RG_LN: return launch3<RG_GATE | RG_LN>(a, b, grid, stream);
    case RG_GATE | RG_HEADS: return launch3<RG_GATE | RG_HEADS>(a, b, grid, stream);
    case RG_GATE: return launch3<RG_GATE>(a, b, grid, stream);
    default: return -1;
    }
}

}  // namespace dpvo
