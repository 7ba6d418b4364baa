// rowgemm_kblocked.hip -- the row-GEMM kernels on a K-BLOCKED W ([K/32][384][32]),
// streamed from L2 straight into registers: everything DPVO.update() launches.
//   rowgemm5_kernel        plain GEMM (0 / RELU / SIGMOID), optionally two on one A (DUAL)
//   rowpair6_kernel        SoftAgg's f / g pair with the A tile resident in LDS (PRE: A formed on the fly)
//   rowchain5_kernel       Linear -> act -> Linear [-> LN -> Linear | gate GEMM] -> row epilogue
//   rowgemm_narrow_kernel  32-row tiles for device-counted GEMMs
// The first three share the wave frame of rowgemm.hpp and, in the diagnostic
// build, the dpvo_stamps buffer -- hence one translation unit.
#include "rowgemm.hpp"

#include <algorithm>

namespace dpvo {
namespace {

#ifdef DPVO_STAMPS
__device__ unsigned long long dpvo_stamps[1024 * 8 * ST_SEGS];
#endif

// ---------------------------------------------------------------------------
// v5 (round 4): the plain GEMM (flags 0 / RELU / SIGMOID) with a k-blocked W
// and no LDS-DMA:
//   * 8 waves as 1 (M) x 8 (N), wave tile 128 x 48 (8 x 3 accumulators), BK 32:
//     every W fragment is read by one wave only (24 KB per k-step and CU from
//     L2; the 2 x 4 layout read each twice: 93 -> 85 us for the SoftAgg pair);
//   * W ([K/32][384][32]: a fragment = one contiguous 1 KB, whole lines)
//     streams from L2 straight into registers, two k-steps ahead -- no LDS
//     traffic for W;
//   * A (128 rows x 64 B per k-step) goes global -> registers -> a 4-slot LDS
//     ring (register staging, four k-steps ahead; rc_sw chunk swizzle,
//     conflict-free fragment reads);
//   * one barrier per TWO k-steps (in-kernel stamps: with one per k-step the
//     waves of a SIMD met at every step, the younger ~500 cycles behind); every
//     wait is the compiler's exact count of the wave's own loads and stores;
//   * the row epilogue stages y16 through a 96 KB LDS tile and stores whole
//     rows, with the next tile's first loads already in flight ahead of it.
// (Measured and not kept: W / A prefetched three or four k-steps ahead -- the
// vmcnt waits are ~10 % of a k-step, no gain; the next k-step's fragments read
// between this one's MFMAs -- 79 -> 91 us.)
// Persistent blocks walk a flat (tile, pass, k-step) sequence; DUAL runs a
// second GEMM (p2's W, bias, out16) on the same A tile right after the first.
// Per output element the MFMA k order is rowgemm3's: the same bits.
// ---------------------------------------------------------------------------
template <int FLAGS, bool DUAL>
__global__ __launch_bounds__(R5_THREADS, 1) void rowgemm5_kernel(dpvo_rowgemm_args p, dpvo_rowgemm_args p2)
{
    static_assert((FLAGS & ~(RG_RELU | RG_SIGMOID)) == 0, "v5: plain GEMMs only");
    __shared__ __attribute__((aligned(16))) char smem[R5_LDS];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = p.K, nks = K / R5_BK;
    const int64_t Mrows = p.M_dev ? min(*p.M_dev, p.M) : p.M;
    const int64_t ntiles = (Mrows + RG_BM - 1) / RG_BM;
    if ((int64_t)blockIdx.x >= ntiles) return;
    constexpr int NP = DUAL ? 2 : 1;
    const int64_t my_tiles = (ntiles - 1 - blockIdx.x) / gridDim.x + 1;
    const int64_t total = my_tiles * NP * nks;   // flat k-steps of this block
    const R5Lane L(lane, w);

    // ---- A staging: the lane's row of the tile a cursor is on
    int64_t a_tile = -1;
    const half_t* arow = (const half_t*)p.zero_row;
    auto a_row = [&](int64_t t) __attribute__((always_inline)) {
        if (t == a_tile) return;
        a_tile = t;
        arow = r5_a_source(p, Mrows, t * RG_BM + L.ar) + 8 * L.ac;
    };
    h8_t areg[2];
    auto load_a = [&](const R5Cursor& c) __attribute__((always_inline)) -> h8_t {
        a_row(c.t);
        return *(const h8_t*)(arow + c.k * R5_BK);
    };
    // ---- W fragments of the flat stream
    h8_t wreg[2][3];
    const half_t* W1 = (const half_t*)p.W;
    const half_t* W2 = DUAL ? (const half_t*)p2.W : W1;
    auto load_w = [&](const R5Cursor& c, h8_t (&r)[3]) __attribute__((always_inline)) {
        r5_load_w(DUAL && c.q ? W2 : W1, c.k, L.wcol, r);
    };
    // ---- biases of this wave's columns, both passes
    h4_t bias[NP][3];
#pragma unroll
    for (int q = 0; q < NP; q++)
#pragma unroll
        for (int nt = 0; nt < 3; nt++)
            bias[q][nt] = *(const h4_t*)((const half_t*)(q ? p2.bias : p.bias) + 48 * w + 16 * nt + 4 * L.fq);
    f4_t acc[8][3];
#pragma unroll
    for (int mt = 0; mt < 8; mt++)
#pragma unroll
        for (int nt = 0; nt < 3; nt++) acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};

    auto epilogue = [&](int64_t t, auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        const dpvo_rowgemm_args& pe = q ? p2 : p;
        r5_acc_to_y<8, true>(
            acc, 0, [&](int nt, int) { return bias[q][nt]; }, (FLAGS & RG_RELU) != 0, (FLAGS & RG_SIGMOID) != 0, smem, L);
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        // whole rows out: wave w stores rows 16 w .. 16 w + 15
        r5_store_rows<16>(smem, pe, [&](int lr) { return t * RG_BM + lr; }, Mrows, w, lane);
    };

    // ---- prologue: stages 0, 1 into slots 0, 1; stages 2, 3 in registers
    // (stage g: slot g % 4, register set g % 2); W stages 0, 1 (stage f in
    // wreg[f % 2])
    const unsigned G = gridDim.x;
    R5Cursor cur{0, (int64_t)blockIdx.x, 0, 0};   // step f
    R5Cursor cw = cur, ca = cur;                   // W / A prefetch cursors
#pragma unroll
    for (int r = 0; r < 2; r++) {
        load_w(cw, wreg[r]);
        cw.next(total, nks, NP, G);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const h8_t x = load_a(ca);
        *(h8_t*)(smem + R5_Y + r * R5_ASLOT + L.aw_off) = x;
        ca.next(total, nks, NP, G);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        areg[r] = load_a(ca);
        ca.next(total, nks, NP, G);
    }
#ifdef DPVO_STAMPS
    unsigned long long st_sum[ST_SEGS] = {};
    RC_STAMP(t_begin)
#endif
    // one k-step, PH = f mod 4: stage f is read from slot f % 4 and, after
    // the MFMAs, stage f + 2 written into slot (f + 2) % 4.  One barrier per
    // TWO k-steps (even f): it makes stages f, f + 1 visible (written at the
    // ends of f - 2, f - 1) and frees slots (f + 2) % 4, (f + 3) % 4 (stages
    // f - 2, f - 1, read at f - 2, f - 1), so the waves of a SIMD may drift a
    // k-step apart between them.
    auto step = [&](auto ph) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph)::value;
        constexpr int PR = PH & 1;
        RC_STAMP(s0)
        if (PR == 0) {
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_s_barrier();
        }
        RC_STAMP(s1)
#ifdef DPVO_STAMPS
        asm volatile("" ::"v"(wreg[PR][0]), "v"(wreg[PR][1]), "v"(wreg[PR][2]));
#endif
        RC_STAMP(s2)
        r5_mfmas_slot(smem + R5_Y + PH * R5_ASLOT, L, wreg[PR], acc);
        // W(f + 2) is issued BEFORE A(f + 4): the MFMAs' wait on W(f) at step f
        // then never covers an HBM A load; only the ring write (after this
        // step's MFMAs) waits on its A stage
        load_w(cw, wreg[PR]);                                                  // W stage f + 2
        cw.next(total, nks, NP, G);
        __builtin_amdgcn_sched_barrier(0);
        *(h8_t*)(smem + R5_Y + ((PH + 2) & 3) * R5_ASLOT + L.aw_off) = areg[PR];   // stage f + 2
        areg[PR] = load_a(ca);                                                         // stage f + 4
        ca.next(total, nks, NP, G);
        RC_STAMP(s3)
        RC_ACC(0, s0, s1) RC_ACC(1, s1, s2) RC_ACC(2, s2, s3)
        if (cur.k == nks - 1) {
            if (DUAL && cur.q)
                epilogue(cur.t, std::integral_constant<int, DUAL ? 1 : 0>{});
            else
                epilogue(cur.t, std::integral_constant<int, 0>{});
            RC_STAMP(s4)
            RC_ACC(3, s3, s4)
        }
        cur.next(total, nks, NP, G);
    };
    for (int64_t f = 0; f < total; f += 4) {
        bd_steps<0, 4>::run([&](auto pc) __attribute__((always_inline)) {
            if (f + decltype(pc)::value < total) step(pc);
        });
    }
#ifdef DPVO_STAMPS
    RC_STAMP(t_end)
    st_sum[10] += t_end - t_begin;
    if (lane == 0)
        for (int k = 0; k < ST_SEGS; k++) dpvo_stamps[((int64_t)blockIdx.x * 8 + w) * ST_SEGS + k] = st_sum[k];
#endif
}

// ---------------------------------------------------------------------------
// rowpair6 (round 6): SoftAgg's f / g pair (rowgemm5 DUAL, K <= 384) with the
// whole A tile resident in LDS.  rowgemm5 streams A through a 4-slot ring and
// reads it twice, once per pass; the second read comes back from past L2 (the
// round-5 counters: 152 MB fetched for agg_kk's 73 MB operand, 345 MB for
// pair_pre's).  Here pass 0 stages every k-step of the tile into its own 8 KB
// slot (96 KB at K = 384), pass 1 runs on those slots with no loads and no
// barriers, and each pass's row epilogue goes out through half a y tile (48 KB,
// 64 rows at a time).  During pass 1 the next tile's first two A stages load
// into the registers the ring protocol uses; they reach slots 0 / 1 after pass
// 1's epilogue.  Same MFMA operands in the same k order, the same epilogue
// arithmetic: bit-identical to rowgemm5.
//
// PRE (dpvo_rowgemm_pair_pre): the A rows are formed while they are staged,
// A[m] = fp16(pre.a[m] + pre.b16[pre.b_idx[m]]) -- rowadd_ln's fp32 add and
// rounding (net + agg_kk(net), net.py:87 -> the agg_ij SoftAgg's f / g
// operand) without its 73 MB fp16 rows round-tripping HBM.
// ---------------------------------------------------------------------------
struct R5PreRaw {
    f4_t lo, hi;   // 8 fp32 of pre.a
    h8_t b;        // 8 fp16 of the gathered addend, or -0 (a row without one)
};
template <bool PRE>
using r5_areg_t = std::conditional_t<PRE, R5PreRaw, h8_t>;
__device__ __forceinline__ h8_t r5_cvt(const h8_t& x) { return x; }
__device__ __forceinline__ h8_t r5_cvt(const R5PreRaw& x)
{
    h8_t y;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        y[i] = (half_t)(x.lo[i] + (float)x.b[i]);
        y[4 + i] = (half_t)(x.hi[i] + (float)x.b[4 + i]);
    }
    return y;
}

constexpr int P6_YH = P6_MAXK * R5_ASLOT;                        // half y tile after the A tile
constexpr int P6_IDX = P6_YH + 64 * 768;                         // PRE: addend sources
constexpr int P6_BIAS = P6_IDX + R5_PRE_IDX_TILES * RG_BM * 8;   // PRE: both passes' biases
constexpr int P6_LDS = P6_BIAS + 2 * RG_BN * 2;                  // 153.5 KB

template <bool PRE>
__global__ __launch_bounds__(R5_THREADS, 1) void rowpair6_kernel(dpvo_rowgemm_args p, dpvo_rowgemm_args p2,
                                                                 dpvo_rowadd_args pre)
{
    __shared__ __attribute__((aligned(16))) char smem[P6_LDS];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nks = p.K / R5_BK;   // even, 4 .. 12 (host-checked)
    const int64_t Mrows = p.M_dev ? min(*p.M_dev, p.M) : p.M;
    const int64_t ntiles = (Mrows + RG_BM - 1) / RG_BM;
    if ((int64_t)blockIdx.x >= ntiles) return;
    const unsigned G = gridDim.x;
    const int64_t my_tiles = (ntiles - 1 - blockIdx.x) / G + 1;
    const int64_t total_w = my_tiles * 2 * nks;
    const R5Lane L(lane, w);
    int64_t* idx_lds = (int64_t*)(smem + P6_IDX);
    auto pre_src = [&](int64_t m) __attribute__((always_inline)) -> int64_t {
        return (m < Mrows && pre.b16) ? (pre.b_idx ? pre.b_idx[m] : m) : -1;
    };
    // ---- A staging: the lane's row of a tile (PRE: the fp32 row and its addend)
    int64_t a_tile = -1;
    int a_lt = -1;
    const half_t* arow = (const half_t*)p.zero_row;
    const float* arow32 = nullptr;
    auto pre_set = [&](int64_t t, int64_t s) __attribute__((always_inline)) {
        const int64_t m = t * RG_BM + L.ar;
        arow32 = (const float*)pre.a + (m < Mrows ? m : 0) * pre.lda + 8 * L.ac;
        const half_t* b = (const half_t*)g_pre_negzero.v;
        if (s >= 0 && s < pre.b_rows) b = (const half_t*)pre.b16 + s * RG_BN;
        arow = b + 8 * L.ac;
    };
    if constexpr (PRE) {
        a_tile = blockIdx.x;
        a_lt = 0;
        pre_set(a_tile, pre_src(a_tile * RG_BM + L.ar));
    }
    auto a_row = [&](int64_t t) __attribute__((always_inline)) {
        if (t == a_tile) return;
        a_tile = t;
        if constexpr (PRE) {
            a_lt++;
            pre_set(t, idx_lds[a_lt * RG_BM + L.ar]);
        } else {
            arow = r5_a_source(p, Mrows, t * RG_BM + L.ar) + 8 * L.ac;
        }
    };
    r5_areg_t<PRE> areg[2];
    auto load_a = [&](int64_t t, int k) __attribute__((always_inline)) -> r5_areg_t<PRE> {
        a_row(t);
        if constexpr (PRE) {
            R5PreRaw x;
            x.lo = *(const f4_t*)(arow32 + k * R5_BK);
            x.hi = *(const f4_t*)(arow32 + k * R5_BK + 4);
            x.b = *(const h8_t*)(arow + k * R5_BK);
            return x;
        } else {
            return *(const h8_t*)(arow + k * R5_BK);
        }
    };
    auto put_a = [&](int slot, const r5_areg_t<PRE>& x) __attribute__((always_inline)) {
        *(h8_t*)(smem + slot * R5_ASLOT + L.aw_off) = r5_cvt(x);
    };
    // ---- W fragments (rowgemm5's flat (tile, pass, k-step) stream, two ahead)
    h8_t wreg[2][3];
    const half_t* W1 = (const half_t*)p.W;
    const half_t* W2 = (const half_t*)p2.W;
    auto load_w = [&](const R5Cursor& c, h8_t (&r)[3]) __attribute__((always_inline)) {
        r5_load_w(c.q ? W2 : W1, c.k, L.wcol, r);
    };
    h4_t bias[PRE ? 1 : 2][3];
    if constexpr (PRE) {
        if (threadIdx.x < 2 * 96) {
            const int b = threadIdx.x / 96, c = 4 * (threadIdx.x % 96);
            *(h4_t*)(smem + P6_BIAS + b * RG_BN * 2 + 2 * c) = *(const h4_t*)((const half_t*)(b ? p2.bias : p.bias) + c);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int nt = 0; nt < 3; nt++)
                bias[q][nt] = *(const h4_t*)((const half_t*)(q ? p2.bias : p.bias) + 48 * w + 16 * nt + 4 * L.fq);
    }
    f4_t acc[8][3];
#pragma unroll
    for (int mt = 0; mt < 8; mt++)
#pragma unroll
        for (int nt = 0; nt < 3; nt++) acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
    };
    // pass q's rows out, 64 at a time through the half y tile (wave w: rows
    // 8 w .. 8 w + 7 of the half); ends on a barrier
    auto epilogue = [&](int64_t t, auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        const dpvo_rowgemm_args& pe = q ? p2 : p;
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            r5_acc_to_y<4, true>(
                acc, 4 * hh,
                [&](int nt, int col) {
                    if constexpr (PRE)
                        return *(const h4_t*)(smem + P6_BIAS + q * RG_BN * 2 + 2 * col);
                    else
                        return bias[q][nt];
                },
                false, false, smem + P6_YH, L);
            sync();
            const int64_t row0 = t * RG_BM + 64 * hh;
            r5_store_rows<8>(smem + P6_YH, pe, [&](int lr) { return row0 + lr; }, Mrows, w, lane);
            sync();
        }
    };

    // ---- prologue: W steps 0, 1; the first tile's A stages 0, 1 in slots 0, 1, 2, 3 in registers
    R5Cursor cw{0, (int64_t)blockIdx.x, 0, 0};
    auto wnext = [&]() __attribute__((always_inline)) { cw.next(total_w, nks, 2, G); };
    load_w(cw, wreg[0]);
    wnext();
    load_w(cw, wreg[1]);
    wnext();
    put_a(0, load_a(blockIdx.x, 0));
    put_a(1, load_a(blockIdx.x, 1));
    areg[0] = load_a(blockIdx.x, 2);
    areg[1] = load_a(blockIdx.x, 3);
    if constexpr (PRE) {
        for (int i = RG_BM + threadIdx.x; i < (int)my_tiles * RG_BM; i += blockDim.x)
            idx_lds[i] = pre_src(((int64_t)blockIdx.x + (int64_t)(i / RG_BM) * G) * RG_BM + i % RG_BM);
    }
    auto mfmas = [&](int slot, const h8_t (&wr)[3]) __attribute__((always_inline)) {
        r5_mfmas_slot(smem + slot * R5_ASLOT, L, wr, acc);
    };
#ifdef DPVO_STAMPS
    // segments: 0 pass-0 barrier waits, 1 pass-0 k-steps otherwise, 2 pass-0
    // epilogue, 3 pass 1, 4 pass-1 epilogue + next stages, 10 total, 11 tiles
    unsigned long long st_sum[ST_SEGS] = {};
    RC_STAMP(p_begin)
#endif
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += G) {
        const bool more = tile + G < ntiles;
#ifdef DPVO_STAMPS
        st_sum[11] += 1;
        RC_STAMP(q0)
#endif
        // ---- pass 0: k-step ks reads slot ks, then stage ks + 2 goes from its
        // register set into slot ks + 2 and stage ks + 4 is loaded; one barrier
        // per two k-steps makes stages ks, ks + 1 visible (no slot is reused
        // within the tile, so no barrier guards a rewrite)
#pragma unroll 1
        for (int ks = 0; ks < nks; ks += 2) {
            bd_steps<0, 2>::run([&](auto pc) __attribute__((always_inline)) {
                constexpr int PH = decltype(pc)::value;
                const int k = ks + PH;
                RC_STAMP(b0)
                if (PH == 0) sync();
                RC_STAMP(b1)
                RC_ACC(0, b0, b1)
                mfmas(k, wreg[PH]);
                load_w(cw, wreg[PH]);
                wnext();
                __builtin_amdgcn_sched_barrier(0);
                if (k + 2 < nks) {
                    put_a(k + 2, areg[PH]);
                    if (k + 4 < nks) areg[PH] = load_a(tile, k + 4);
                }
            });
        }
#ifdef DPVO_STAMPS
        RC_STAMP(q1)
        st_sum[1] += q1 - q0;
#endif
        epilogue(tile, std::integral_constant<int, 0>{});
#ifdef DPVO_STAMPS
        RC_STAMP(q2)
        RC_ACC(2, q1, q2)
#endif
        // ---- pass 1 on the resident tile; the next tile's stages 0, 1 load meanwhile
#pragma unroll 1
        for (int ks = 0; ks < nks; ks += 2) {
            bd_steps<0, 2>::run([&](auto pc) __attribute__((always_inline)) {
                constexpr int PH = decltype(pc)::value;
                mfmas(ks + PH, wreg[PH]);
                load_w(cw, wreg[PH]);
                wnext();
                if (ks == 0 && more) areg[PH] = load_a(tile + G, PH);
            });
        }
#ifdef DPVO_STAMPS
        RC_STAMP(q3)
        RC_ACC(3, q2, q3)
#endif
        epilogue(tile, std::integral_constant<int, 1>{});
        if (more) {   // (every wave is past its pass-1 reads: the epilogue's barriers)
            put_a(0, areg[0]);
            put_a(1, areg[1]);
            areg[0] = load_a(tile + G, 2);
            areg[1] = load_a(tile + G, 3);
        }
#ifdef DPVO_STAMPS
        RC_STAMP(q4)
        RC_ACC(4, q3, q4)
#endif
    }
#ifdef DPVO_STAMPS
    RC_STAMP(p_end)
    st_sum[1] -= st_sum[0];   // (segment 1 held the whole pass 0)
    st_sum[10] += p_end - p_begin;
    if (lane == 0)
        for (int k = 0; k < ST_SEGS; k++) dpvo_stamps[((int64_t)blockIdx.x * 8 + w) * ST_SEGS + k] = st_sum[k];
#endif
}

// ---------------------------------------------------------------------------
// Chained pair: Y = epi2(act1(A W1^T + b1) W2^T + b2) with the 128 x 384
// intermediate kept in LDS -- the update operator's Linear -> ReLU -> Linear
// pairs (corr0/corr1, c1, c2, the GRU res branches; net.py:53-56,
// blocks.py:27-30), whose 73 MB intermediates otherwise round-trip HBM.  The y
// tile is GEMM2's A operand, then its output for the row epilogue.
//
// v5 chains (round 4): the chain dataflow -- GEMM1 -> y tile -> GEMM2
// [-> LayerNorm -> GEMM3 (TRI) | gate GEMM (GATED)] -> row epilogue -- on
// rowgemm5's machinery: every W (k-blocked) streams from L2 into registers two
// W-steps ahead over one flat per-block sequence (W1, then W2, then W3 / Wg),
// A goes through registers into the 4-slot ring (GEMM1 and the gate pass; one
// barrier per two A-steps), the GEMMs over the y tile read it in place and
// need no barrier at all.  8 waves as 1 (M) x 8 (N), wave tile 128 x 48.
// K1 % 64 == 0 keeps the register-set parities of both sequences equal to the
// k-step's.  The biases sit in LDS (read at the y-tile writes without waiting
// behind the prefetch's vmcnt; in registers the LN chains spilled).
// OVL (residual-only epilogues): tile t's row epilogue runs inside tile
// t + 1's GEMM1 k-loop on every wave (8 batches of 2 rows, each batch's loads
// one k-step ahead of its arithmetic) -- GEMM1 never touches the y tile.
// (Measured at C3 shapes: 151 us with it, 156 without; two batches in flight
// spill.)  Per output element the MFMA k order and the epilogue arithmetic are
// rowgemm3's: bit-identical to the unchained launches.
//
// GATED (the GRU's GatedResidual, blocks.py:27-30): after GEMM2 has put y in
// the y tile, a third GEMM on the same A (re-read from L2) gives
// gate = sigmoid(A Wg^T + bg) in the accumulators, and every lane rewrites its
// own y tile elements as fp16(gate * y) -- the epilogue then adds them to the
// residual like RES, which is bit-for-bit the GATE epilogue's
// x + fp16(gate * y) without the 73 MB gate16 round trip (nor a gate held in
// registers across the GEMMs).
// TRI (the corr MLP of net.py:54-61 and the `norm(net + inp + corr(.))` of
// :78-79 in one launch): pg is then the MIDDLE Linear -- GEMM2 runs with pg's
// W and bias, its y tile gets pg's row epilogue in place (LayerNorm -> ReLU,
// rounded to fp16: the A operand the next Linear casts to under autocast),
// then a third GEMM on that tile with p's W and bias feeds p's epilogue.
// Bit-identical to rowchain (corr0, corr1, LN|LN_RELU) -> fp16 rows ->
// rowgemm (corr2, RES|LN): the same MFMA k order and the same epilogue code.
//
// F1: GEMM1's activation as a compile-time constant (RG_RELU: every chain of
// the update operator), or -1 to read it from p1.flags.  With the runtime
// flags the y-tile conversion evaluates the sigmoid (exp + rcp per element)
// beside the ReLU and selects: ~10k cycles per tile, an eighth of a c1 tile.
// PRELN (the first GRU's gated chain, dpvo_rowchain_gated_pre): the
// residual base is not read from res32 but formed in the row epilogue as
// LayerNorm(pre.a + pre.b16[b_idx] + pre.c16[c_idx]) with rowadd_ln's fp32
// arithmetic in its order (preln_rows) -- the rows rowadd_ln would have
// written as out32 (net.py:90-91: net + agg_kk + agg_ij -> norm), without
// their 147 MB write and re-read.
// ---------------------------------------------------------------------------
// OVL's batch schedule: 16 rows per wave in OVL_NB batches of OVL_R rows, batch
// b's loads after k-step L(b) = b (nk1 - 4) / (OVL_NB - 1) and its arithmetic
// one k-step later.  L must be strictly increasing in b for every batch to be
// issued and finished by k-step nk1 - 3, i.e. (nk1 - 4) >= OVL_NB - 1 with nk1
// even: the kernel defers a tile's epilogue only from OVL_MIN_NK1 k-steps up
// (shorter GEMM1s run the epilogue in place).
constexpr int OVL_R = 2, OVL_NB = 16 / OVL_R;   // (4-row batches: the same time, 248 registers)
constexpr int OVL_MIN_NK1 = 12;
static_assert(OVL_MIN_NK1 % 2 == 0 && OVL_MIN_NK1 - 4 >= OVL_NB - 1,
              "OVL: b (nk1 - 4) / (OVL_NB - 1) must take a new k-step for every batch");

template <int F2, bool GATED = false, int FMID = 0, int F1 = -1, bool PRELN = false>
__global__ __launch_bounds__(R5_THREADS, 1) void rowchain5_kernel(dpvo_rowgemm_args p1, dpvo_rowgemm_args p,
                                                                  dpvo_rowgemm_args pg, dpvo_rowadd_args pre)
{
    static_assert(!PRELN || (GATED && (F2 & RG_NOADD) && (F2 & RG_LN)), "PRELN: the gated LN chain");
    constexpr bool TRI = FMID != 0;
    static_assert(!(TRI && GATED), "a chain is either gated or three GEMMs long");
    // (RES | LN overlapped the same way -- the corr chain, the gated LN chain --
    // measured 188 -> 197 us and 150 -> 150 us: its batches' loads queue ahead
    // of the A stream's in the in-order vmcnt; profiles/r6/experiments/)
    constexpr bool OVL = (F2 & ~RG_NOADD) == RG_RES;
    constexpr int NSEG = (TRI || GATED) ? 3 : 2;
    constexpr int NPA = GATED ? 2 : 1;   // A passes per tile
    constexpr int nk2 = RG_BN / R5_BK;
    constexpr int BIAS_OFF = R5_LDS;   // the three biases, 768 B each, after the A ring
    constexpr int IDX_OFF = BIAS_OFF + 3 * RG_BN * 2;   // the gathered rows' sources, R5_IDX_TILES tiles
    __shared__ __attribute__((aligned(16))) char smem[R5_LDS + 3 * RG_BN * 2 + (!GATED && !TRI ? R5_IDX_TILES * RG_BM * 8 : 0)];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const R5Lane L(lane, w);
    const int nk1 = p1.K / R5_BK;
    const int64_t Mrows = p1.M_dev ? min(*p1.M_dev, p1.M) : p1.M;
    const int64_t ntiles = (Mrows + RG_BM - 1) / RG_BM;
    if ((int64_t)blockIdx.x >= ntiles) return;
    const unsigned G = gridDim.x;
    const int64_t my_tiles = (ntiles - 1 - blockIdx.x) / G + 1;
    const int64_t total_a = my_tiles * NPA * nk1;
    const int n2 = TRI ? nk2 : nk1;
    const int64_t total_w = my_tiles * (nk1 + nk2 + (NSEG == 3 ? n2 : 0));
    const YMapChunk ym;
    // ---- the gathered rows' sources (p1.a_idx): the first tile's read
    // directly in the prologue, the block's later tiles' from an LDS table
    // filled after the prologue's loads are issued (published by GEMM1's first
    // barrier), so crossing into the next tile inside the k-loop waits on LDS,
    // not (vmcnt 0) on every load the wave has in flight -- the W / A prefetch
    // and the OVL epilogue's.  (K1 = 64: the prologue's four A stages already
    // cross, so the whole table is filled first.)  The host sizes the grid so
    // that a block has <= R5_IDX_TILES tiles.  The two-GEMM chains only (c1 /
    // c2 gather); the gated and three-GEMM chains keep the direct read, their
    // registers are full.
    constexpr bool IDX_LDS = !GATED && !TRI;
    int64_t* idx_lds = (int64_t*)(smem + IDX_OFF);
    const bool idx_tab = IDX_LDS && p1.a_idx, idx_early = idx_tab && nk1 < 4;
    auto idx_fill = [&](int i0) __attribute__((always_inline)) {
        for (int i = i0 + threadIdx.x; i < (int)my_tiles * RG_BM; i += blockDim.x) {
            const int64_t m = ((int64_t)blockIdx.x + (int64_t)(i / RG_BM) * G) * RG_BM + i % RG_BM;
            idx_lds[i] = m < Mrows ? p1.a_idx[m] : -1;
        }
    };
    if (idx_early) {
        idx_fill(0);
        __syncthreads();
    }
    // ---- A staging: the lane's row of the tile a cursor is on
    int64_t a_tile = -1;
    int a_lt = -1;   // the block-local index of a_tile (the cursor moves a tile at a time)
    const half_t* arow = (const half_t*)p1.zero_row;
    if (idx_tab && !idx_early) {   // the first tile, from global (the table is filled after the prologue)
        a_tile = blockIdx.x;
        a_lt = 0;
        const int64_t m0 = a_tile * RG_BM + L.ar;
        arow = r5_a_at(p1, Mrows, m0, m0 < Mrows ? p1.a_idx[m0] : -1) + 8 * L.ac;
    }
    auto a_row = [&](int64_t t) __attribute__((always_inline)) {
        if (t == a_tile) return;
        a_tile = t;
        if constexpr (IDX_LDS) a_lt++;
        const int64_t m = t * RG_BM + L.ar;
        // (r5_a_source for the direct read: same registers, but other branches and 12 more scalar instructions)
        if constexpr (IDX_LDS) {
            arow = r5_a_at(p1, Mrows, m, !p1.a_idx ? m : idx_lds[a_lt * RG_BM + L.ar]) + 8 * L.ac;
        } else if (p1.a_idx) {   // (the load's wait stays inside this branch: a wait at
            arow = r5_a_at(p1, Mrows, m, m < Mrows ? p1.a_idx[m] : -1) + 8 * L.ac;   // the join would drain the queue on every path)
        } else {
            arow = r5_a_at(p1, Mrows, m, m) + 8 * L.ac;
        }
    };
    h8_t areg[2];
    auto load_a = [&](const R5Cursor& c) __attribute__((always_inline)) -> h8_t {
        a_row(c.t);
        return *(const h8_t*)(arow + c.k * R5_BK);
    };
    // ---- W: segment 0 = W1, 1 = the middle (TRI) or second Linear, 2 = the
    // last (TRI) or the gate (GATED)
    const half_t* Ws0 = (const half_t*)p1.W;
    const half_t* Ws1 = (const half_t*)(TRI ? pg.W : p.W);
    const half_t* Ws2 = (const half_t*)(TRI ? p.W : pg.W);
    h8_t wreg[2][3];
    auto load_w = [&](const R5WCursor& c, h8_t (&r)[3]) __attribute__((always_inline)) {
        r5_load_w(c.s == 0 ? Ws0 : (c.s == 1 ? Ws1 : Ws2), c.k, L.wcol, r);
    };
    // ---- the biases (GEMM1, GEMM2, GEMM3 / gate) into LDS: read at the
    // y-tile writes without waiting behind the W / A prefetch's vmcnt
    if (threadIdx.x < 3 * 96) {
        const int b = threadIdx.x / 96, c = 4 * (threadIdx.x % 96);
        const void* src = b == 0 ? p1.bias : (b == 1 ? (TRI ? pg.bias : p.bias) : (TRI ? p.bias : pg.bias));
        if (b < NSEG) *(h4_t*)(smem + BIAS_OFF + b * RG_BN * 2 + 2 * c) = *(const h4_t*)((const half_t*)src + c);
    }
    f4_t acc[8][3];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < 8; mt++)
#pragma unroll
            for (int nt = 0; nt < 3; nt++) acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
    };
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
    };
    // acc + bias (LDS copy bi) -> act -> fp16 -> y tile
    // (its own copy: r5_acc_to_y changed the gated and three-GEMM kernels' allocation, +4 .. 6 VGPRs, PRELN spilled)
    auto acc_to_y = [&](int bi, bool relu, bool sigm) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            const int col = 48 * w + 16 * nt + 4 * L.fq;
            const h4_t b = *(const h4_t*)(smem + BIAS_OFF + bi * RG_BN * 2 + 2 * col);
#pragma unroll
            for (int mt = 0; mt < 8; mt++) {
                h4_t y;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    half_t v = (half_t)(acc[mt][nt][r] + (float)b[r]);
                    if (relu) v = v > (half_t)0 ? v : (half_t)0;
                    if (sigm) v = (half_t)fast_sigmoid((float)v);
                    y[r] = v;
                }
                *(h4_t*)(smem + ym.off(16 * mt + L.fr, col * 2)) = y;
            }
        }
    };
    const unsigned bid = blockIdx.x;
    R5Cursor ca{0, (int64_t)bid, 0, 0};
    R5WCursor cw{0, (int64_t)bid, 0, 0};
    auto wnext = [&]() __attribute__((always_inline)) { cw.next(total_w, nk1, nk2, n2, NSEG, G); };
    auto anext = [&]() __attribute__((always_inline)) { ca.next(total_a, nk1, NPA, G); };
    // one A-step g (GEMM1 or the gate pass), PH = g & 1 = the W-step's parity:
    // stage g from slot g % 4; after the MFMAs stage g + 2 (register set PH)
    // into slot (g + 2) % 4 and stage g + 4 loaded into set PH.  One barrier per
    // two A-steps (even g): it makes stages g, g + 1 visible and frees the slots
    // of stages g - 2, g - 1.
    int ga = 0;
    auto step_a = [&](auto ph) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph)::value;
        if (PH == 0) sync();
        // (the A fragments and MFMAs written out, here and in step_y: r5_mfmas
        // changed the gated and three-GEMM kernels' allocation like r5_acc_to_y)
        const char* sa = smem + R5_Y + (ga & 3) * R5_ASLOT;
        h8_t a[8];
#pragma unroll
        for (int mt = 0; mt < 8; mt++) a[mt] = *(const h8_t*)(sa + L.ar_off + 1024 * mt);
#pragma unroll
        for (int nt = 0; nt < 3; nt++)
#pragma unroll
            for (int mt = 0; mt < 8; mt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wreg[PH][nt], a[mt], acc[mt][nt], 0, 0, 0);
        // (W before A, the ring write after the MFMAs: as in rowgemm5)
        load_w(cw, wreg[PH]);
        wnext();
        __builtin_amdgcn_sched_barrier(0);
        *(h8_t*)(smem + R5_Y + ((ga + 2) & 3) * R5_ASLOT + L.aw_off) = areg[PH];
        areg[PH] = load_a(ca);
        anext();
        ga++;
    };
    // one k-step of a GEMM over the y tile (read in place; no barrier)
    auto step_y = [&](auto ph, int ks) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph)::value;
        h8_t a[8];
#pragma unroll
        for (int mt = 0; mt < 8; mt++) a[mt] = *(const h8_t*)(smem + ym.off(16 * mt + L.fr, (ks * 4 + L.fq) * 16));
#pragma unroll
        for (int nt = 0; nt < 3; nt++)
#pragma unroll
            for (int mt = 0; mt < 8; mt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wreg[PH][nt], a[mt], acc[mt][nt], 0, 0, 0);
        load_w(cw, wreg[PH]);
        wnext();
    };
    auto gemm_y = [&]() __attribute__((always_inline)) {
        zero_acc();
#pragma unroll 1
        for (int ks = 0; ks < nk2; ks += 2) {
            step_y(std::integral_constant<int, 0>{}, ks);
            step_y(std::integral_constant<int, 1>{}, ks + 1);
        }
    };
    // TRI: LayerNorm (+ ReLU) of the y tile's rows in place, rounded to fp16
    // (epi2_finish's LN arithmetic)
    auto mid_rows = [&](const dpvo_rowgemm_args& pm) __attribute__((always_inline)) {
        EpiConsts2 km;
        load_consts2<FMID>(pm, lane, km);
        const int h = lane >> 5, s = lane & 31;
#pragma unroll 1
        for (int i = 0; i < 8; i++) {
            const int r = w * 16 + 2 * i + h;
            ep_f4 v[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const ep_h4 y = *(const ep_h4*)(smem + ym.off(r, (128 * j + 4 * s) * 2));
                v[j] = ep_f4{(float)y[0], (float)y[1], (float)y[2], (float)y[3]};
            }
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++) sm += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
            const float mean = half_sum(sm) * (1.f / RG_BN);
            float sq = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const ep_f4 d = v[j] - mean;
                sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
            const float rstd = rsqrtf(half_sum(sq) * (1.f / RG_BN) + pm.ln_eps);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                v[j] = (v[j] - mean) * rstd * km.g[j] + km.b[j];
                if (FMID & RG_LN_RELU)
#pragma unroll
                    for (int t = 0; t < 4; t++) v[j][t] = fmaxf(v[j][t], 0.f);
                *(ep_h4*)(smem + ym.off(r, (128 * j + 4 * s) * 2)) =
                    ep_h4{(half_t)v[j][0], (half_t)v[j][1], (half_t)v[j][2], (half_t)v[j][3]};
            }
        }
    };
    // the row epilogue in batches of R rows: local rows lr .. lr + R - 1 of tile et
    auto epi_issue = [&](int64_t et, int lr, auto& o) __attribute__((always_inline)) {
        constexpr int R = sizeof(o.add) / sizeof(o.add[0][0]) / 3 * 2;
        epi2_load<F2, R>(p, Mrows, et * RG_BM + lr, lane, o);
    };
    auto epi_done = [&](int64_t et, int lr, const EpiConsts2& kc, const auto& o) __attribute__((always_inline)) {
        constexpr int R = sizeof(o.add) / sizeof(o.add[0][0]) / 3 * 2;
        const int hh = lane >> 5, ss = lane & 31;
        epi2_finish<F2, R>(
            p, Mrows,
            [&](int i, int j) { return *(const ep_h4*)(smem + ym.off(lr + 2 * i + hh, (128 * j + 4 * ss) * 2)); },
            et * RG_BM + lr, lane, kc, o);
    };

    // ---- prologue: W-steps 0, 1 in registers; A stages 0, 1 in slots 0, 1,
    // 2 and 3 in register sets 0, 1
    load_w(cw, wreg[0]);
    wnext();
    load_w(cw, wreg[1]);
    wnext();
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const h8_t x = load_a(ca);
        *(h8_t*)(smem + R5_Y + r * R5_ASLOT + L.aw_off) = x;
        anext();
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        areg[r] = load_a(ca);
        anext();
    }
    if (idx_tab && !idx_early) idx_fill(RG_BM);   // (tiles 1.. : read after GEMM1's first barrier)
    int64_t etile = -1;   // OVL: the tile whose row epilogue is still pending
#ifdef DPVO_STAMPS
    // chain segments: 0 GEMM1 k-loop (+ OVL epilogue), 1 GEMM1 -> y tile + sync,
    // 2 GEMM2 (+ TRI: mid rows + GEMM3) + syncs, 3 y-tile write (+ gate pass) + sync,
    // 4 row epilogue (non-OVL / last tile), 10 total, 11 tiles
    unsigned long long st_sum[ST_SEGS] = {};
    RC_STAMP(c_begin)
#endif
    for (int64_t tile = bid; tile < ntiles; tile += G) {
#ifdef DPVO_STAMPS
        RC_STAMP(c0)
        st_sum[11] += 1;
#endif
        const bool more = tile + G < ntiles;
        // ---- GEMM1 (+ OVL: the previous tile's row epilogue, rows 16 w .. 16 w + 15
        // in OVL_NB batches of OVL_R: batch b's loads after k-step L(b) =
        // b (nk1 - 4) / (OVL_NB - 1), its y-tile reads and arithmetic after
        // k-step L(b) + 1 <= nk1 - 3.
        // Barriers come at the even k-steps only, so the last batch must finish
        // before the barrier of k-step nk1 - 2: that barrier is the only one
        // between a wave's last read of tile t's y rows and the other waves'
        // acc_to_y writes of tile t + 1 after k-step nk1 - 1.  (Round 4 to 5
        // scheduled the last batch's reads after k-step nk1 - 2, with no barrier
        // before those writes: a wave running ahead could overwrite y-tile
        // columns a slower wave had not read yet -- the intermittent last-bit
        // differences of the round-5 graph-replay test.)
        {
            EpiOps2<OVL_R> st;
            int bi = 0, bd = 0;
            auto ovl = [&](int ks) __attribute__((always_inline)) {
                if (!OVL || etile < 0) return;
                if (bd < bi) {
                    EpiConsts2 kc;
                    load_consts2<F2>(p, lane, kc);
                    epi_done(etile, 16 * w + OVL_R * bd, kc, st);
                    bd++;
                }
                __builtin_amdgcn_sched_barrier(0);
                // (complete only for nk1 >= OVL_MIN_NK1: etile is set under that condition alone)
                if (bi < OVL_NB && (bi * (nk1 - 4)) / (OVL_NB - 1) == ks) {
                    epi_issue(etile, 16 * w + OVL_R * bi, st);
                    bi++;
                }
            };
            zero_acc();
#pragma unroll 1
            for (int ks = 0; ks < nk1; ks += 2) {
                step_a(std::integral_constant<int, 0>{});
                ovl(ks);
                step_a(std::integral_constant<int, 1>{});
                ovl(ks + 1);
            }
        }
        etile = -1;
#ifdef DPVO_STAMPS
        RC_STAMP(c1)
#endif
        if constexpr (F1 >= 0)
            acc_to_y(0, (F1 & RG_RELU) != 0, (F1 & RG_SIGMOID) != 0);
        else
            acc_to_y(0, p1.flags & RG_RELU, p1.flags & RG_SIGMOID);
        sync();
#ifdef DPVO_STAMPS
        RC_STAMP(c2)
#endif
        gemm_y();
        sync();   // every wave is done reading the y tile
        if (TRI) {
            acc_to_y(1, false, false);
            sync();
            mid_rows(pg);
            sync();
            gemm_y();
            sync();
            acc_to_y(2, F2 & RG_RELU, F2 & RG_SIGMOID);
        } else {
#ifdef DPVO_STAMPS
            RC_STAMP(c3t)
            RC_ACC(2, c2, c3t)
#endif
            acc_to_y(1, F2 & RG_RELU, F2 & RG_SIGMOID);
        }
        if (GATED) {
            // gate = sigmoid(A Wg^T + bg) (rowgemm's SIGMOID rounding); y = fp16(gate * y)
            zero_acc();
#pragma unroll 1
            for (int ks = 0; ks < nk1; ks += 2) {
                step_a(std::integral_constant<int, 0>{});
                step_a(std::integral_constant<int, 1>{});
            }
#pragma unroll
            for (int nt = 0; nt < 3; nt++) {
                const int col = 48 * w + 16 * nt + 4 * L.fq;
                const h4_t b = *(const h4_t*)(smem + BIAS_OFF + 2 * RG_BN * 2 + 2 * col);
#pragma unroll
                for (int mt = 0; mt < 8; mt++) {
                    h4_t* yp = (h4_t*)(smem + ym.off(16 * mt + L.fr, col * 2));
                    h4_t y = *yp;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const half_t g = (half_t)fast_sigmoid((float)(half_t)(acc[mt][nt][r] + (float)b[r]));
                        y[r] = (half_t)((float)g * (float)y[r]);
                    }
                    *yp = y;
                }
            }
        }
        sync();
#ifdef DPVO_STAMPS
        RC_STAMP(c4)
        RC_ACC(0, c0, c1) RC_ACC(1, c1, c2) RC_ACC(3, c2, c4)
#endif
        if (OVL && more && nk1 >= OVL_MIN_NK1) {   // (the batches' schedule fits: see OVL_MIN_NK1)
            etile = tile;   // runs inside the next tile's GEMM1
            continue;
        }
        // the row epilogue now: rows 16 w .. 16 w + 15 (the next tile's y
        // tile writes follow its GEMM1 k-steps' barriers)
        // (the accumulators are dead here: the next batch's loads are issued
        // before this batch's arithmetic, two batches live)
        EpiConsts2 kc;
        load_consts2<F2>(p, lane, kc);
        if constexpr (OVL) {   // (only the last tile: one batch live, no spill beside the deferred state)
#pragma unroll 1
            for (int q0 = 0; q0 < 16; q0 += 4) {
                EpiOps2<4> st;
                epi_issue(tile, 16 * w + q0, st);
                epi_done(tile, 16 * w + q0, kc, st);
            }
        } else if constexpr (PRELN) {
            PreOps<4> st[2];
            preln_issue<4>(pre, Mrows, tile * RG_BM + 16 * w, lane, st[0]);
            bd_steps<0, 4>::run([&](auto bc) __attribute__((always_inline)) {
                constexpr int b = decltype(bc)::value;
                if constexpr (b + 1 < 4) preln_issue<4>(pre, Mrows, tile * RG_BM + 16 * w + 4 * (b + 1), lane, st[(b + 1) & 1]);
                EpiOps2<4> o;
                preln_rows<4>(pre, lane, st[b & 1], o);
                epi_done(tile, 16 * w + 4 * b, kc, o);
            });
        } else {
            EpiOps2<4> st[2];
            epi_issue(tile, 16 * w, st[0]);
            bd_steps<0, 4>::run([&](auto bc) __attribute__((always_inline)) {
                constexpr int b = decltype(bc)::value;
                if constexpr (b + 1 < 4) epi_issue(tile, 16 * w + 4 * (b + 1), st[(b + 1) & 1]);
                epi_done(tile, 16 * w + 4 * b, kc, st[b & 1]);
            });
        }
#ifdef DPVO_STAMPS
        RC_STAMP(c5)
        RC_ACC(4, c4, c5)
#endif
    }
#ifdef DPVO_STAMPS
    RC_STAMP(c_end)
    st_sum[10] += c_end - c_begin;
    if (lane == 0)
        for (int k = 0; k < ST_SEGS; k++) dpvo_stamps[((int64_t)blockIdx.x * 8 + w) * ST_SEGS + k] = st_sum[k];
#endif
}

// ---------------------------------------------------------------------------
// Narrow tiles (round 6) for the device-counted GEMMs -- SoftAgg's h Linear
// on the groups (`rowgemm(y, *ph, M_dev=G)`, net.py): G (~4.4k patch groups,
// a few hundred frame-pair groups at C3) is known only on the device, so
// rowgemm5 launched for the upper bound put it on 35 / 4 busy workgroups of
// 128 rows: 15 us a launch, bound by each workgroup's L1 traffic (the whole
// 288 KB W per tile).  Here a workgroup takes 32 rows x 192 columns (two per
// row tile; 4 waves x 48 columns, 2 x 3 accumulators): the A tile is loaded
// once into LDS (XOR-swizzled 16-byte chunks: conflict-free fragment reads),
// each wave streams its W fragments from L2 two k-steps ahead, and each lane
// stores its 4 columns of each row.  Same 16 x 16 x 32 blocks in the same k
// order, the same epilogue rounding: bit-identical to rowgemm5.
// ---------------------------------------------------------------------------
// (RN_WD: W k-steps in flight; 4 measured the same as 2, 7.17 vs 7.11 us)
constexpr int RN_THREADS = 256, RN_MAXK = 896, RN_WD = 2;

template <int FLAGS, int KC>   // KC = K / 64: the A chunks each thread stages
__global__ __launch_bounds__(RN_THREADS) void rowgemm_narrow_kernel(dpvo_rowgemm_args p)
{
    static_assert((FLAGS & ~(RG_RELU | RG_SIGMOID)) == 0, "narrow: plain GEMMs only");
    __shared__ __attribute__((aligned(16))) char sA[RN_BM * RN_MAXK * 2];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int K = 64 * KC, nks = K / R5_BK, rowb = 2 * K;
    static_assert(K <= RN_MAXK && K % 128 == 0, "narrow: the A tile's swizzle needs K % 128 == 0");
    static_assert(nks % RN_WD == 0, "narrow: whole groups of W k-steps");
    const int64_t Mrows = p.M_dev ? min(*p.M_dev, p.M) : p.M;
    const int64_t ntiles = (Mrows + RN_BM - 1) / RN_BM;
    const int c0 = 192 * (blockIdx.x & 1) + 48 * w;   // this wave's first column
    const half_t* __restrict__ W = (const half_t*)p.W + (c0 + fr) * R5_BK + 8 * fq;
    half_t* out = (half_t*)p.out16;
    auto soff = [&](int r, int c) __attribute__((always_inline)) { return r * rowb + ((c ^ (r & 15)) << 4); };
    h4_t bias[3];
#pragma unroll
    for (int nt = 0; nt < 3; nt++) bias[nt] = *(const h4_t*)((const half_t*)p.bias + c0 + 16 * nt + 4 * fq);
    const int ar = threadIdx.x >> 3, ac = threadIdx.x & 7;   // staging: row ar, chunks ac + 8 j
    for (int64_t t = blockIdx.x >> 1; t < ntiles; t += gridDim.x >> 1) {
        // ---- the A tile into LDS: all KC loads of a thread in flight together
        const int64_t m = t * RN_BM + ar;
        const half_t* row = (const half_t*)p.zero_row;
        if (m < Mrows) {
            const int64_t src = p.a_idx ? p.a_idx[m] : m;
            if (src >= 0 && src < p.a_rows) row = (const half_t*)p.A + src * p.lda;
        }
        h8_t st[KC];
#pragma unroll
        for (int j = 0; j < KC; j++) st[j] = *(const h8_t*)(row + 8 * (ac + 8 * j));
#pragma unroll
        for (int j = 0; j < KC; j++) *(h8_t*)(sA + soff(ar, ac + 8 * j)) = st[j];
        __syncthreads();
        f4_t acc[2][3];
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int nt = 0; nt < 3; nt++) acc[mt][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
        h8_t wf[RN_WD][3];
#pragma unroll
        for (int d = 0; d < RN_WD; d++) r5_load_w(W, d, 0, wf[d]);
#pragma unroll 1
        for (int ks = 0; ks < nks; ks += RN_WD) {
            bd_steps<0, RN_WD>::run([&](auto pc) __attribute__((always_inline)) {
                constexpr int S = decltype(pc)::value;
                r5_mfmas([&](int mt) { return sA + soff(16 * mt + fr, 4 * (ks + S) + fq); }, wf[S], acc);
                r5_load_w(W, min(ks + S + RN_WD, nks - 1), 0, wf[S]);   // (unconditional: exact wait counts)
            });
        }
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            const int col = c0 + 16 * nt + 4 * fq;
#pragma unroll
            for (int mt = 0; mt < 2; mt++) {
                const h4_t y = rg_y4(acc[mt][nt], bias[nt], (FLAGS & RG_RELU) != 0, (FLAGS & RG_SIGMOID) != 0);
                const int64_t row = t * RN_BM + 16 * mt + fr;
                if (row < Mrows) *(h4_t*)(out + row * p.ldo16 + col) = y;
            }
        }
        __syncthreads();   // (every wave's A reads before the next tile's writes)
    }
}

// ---- launchers
template <int FLAGS, bool DUAL>
int launch5(const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid, hipStream_t stream)
{
    hipLaunchKernelGGL((rowgemm5_kernel<FLAGS, DUAL>), dim3(grid), dim3(R5_THREADS), 0, stream, a, b);
    return 0;
}

template <int FLAGS>
int launch_narrow(const dpvo_rowgemm_args& a, unsigned grid, hipStream_t stream)
{
    if (a.K == 384)
        hipLaunchKernelGGL((rowgemm_narrow_kernel<FLAGS, 6>), dim3(grid), dim3(RN_THREADS), 0, stream, a);
    else if (a.K == 896)
        hipLaunchKernelGGL((rowgemm_narrow_kernel<FLAGS, 14>), dim3(grid), dim3(RN_THREADS), 0, stream, a);
    else
        return -1;
    return 0;
}

struct ChainCall {
    const dpvo_rowgemm_args &g1, &p, &pg;
    const dpvo_rowadd_args* pre;
    bool relu1;   // GEMM1's activation is ReLU: the compile-time F1 = RG_RELU kernel, else p1.flags at run time
    unsigned grid;
    hipStream_t stream;
};
template <int F2, bool GATED = false, int FMID = 0, bool PRELN = false>
int launch_chain(const ChainCall& c)
{
    const dpvo_rowadd_args pre = c.pre ? *c.pre : dpvo_rowadd_args{};
    if (c.relu1)
        hipLaunchKernelGGL((rowchain5_kernel<F2, GATED, FMID, RG_RELU, PRELN>), dim3(c.grid), dim3(R5_THREADS), 0,
                           c.stream, c.g1, c.p, c.pg, pre);
    else if constexpr (!PRELN)
        hipLaunchKernelGGL((rowchain5_kernel<F2, GATED, FMID, -1, PRELN>), dim3(c.grid), dim3(R5_THREADS), 0, c.stream,
                           c.g1, c.p, c.pg, pre);
    else
        return -1;
    return 0;
}

}  // namespace

int launch_rowgemm5(int flags, bool dual, const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid,
                    hipStream_t stream)
{
    if (dual) return flags == 0 ? launch5<0, true>(a, b, grid, stream) : -1;
    switch (flags) {
    case 0: return launch5<0, false>(a, b, grid, stream);
    case RG_RELU: return launch5<RG_RELU, false>(a, b, grid, stream);
    case RG_SIGMOID: return launch5<RG_SIGMOID, false>(a, b, grid, stream);
    default: return -1;
    }
}

int launch_rowgemm_narrow(int flags, const dpvo_rowgemm_args& a, unsigned grid, hipStream_t stream)
{
    switch (flags) {
    case 0: return launch_narrow<0>(a, grid, stream);
    case RG_RELU: return launch_narrow<RG_RELU>(a, grid, stream);
    case RG_SIGMOID: return launch_narrow<RG_SIGMOID>(a, grid, stream);
    default: return -1;
    }
}

int launch_rowpair6(const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, const dpvo_rowadd_args* pre, unsigned grid,
                    hipStream_t stream)
{
    const int nks = a.K / R5_BK;
    if (nks < P6_MINK || nks > P6_MAXK) return -1;   // (the A tile must fit LDS)
    if (pre)
        hipLaunchKernelGGL((rowpair6_kernel<true>), dim3(grid), dim3(R5_THREADS), 0, stream, a, b, *pre);
    else
        hipLaunchKernelGGL((rowpair6_kernel<false>), dim3(grid), dim3(R5_THREADS), 0, stream, a, b, dpvo_rowadd_args{});
    return 0;
}

int launch_rowchain5(int f2, bool gated, int fmid, bool relu1, const dpvo_rowgemm_args& g1, const dpvo_rowgemm_args& p,
                     const dpvo_rowgemm_args& pg, const dpvo_rowadd_args* pre, unsigned grid, hipStream_t stream)
{
    constexpr int LNR = RG_LN | RG_LN_RELU, NA = RG_NOADD;
    const ChainCall c{g1, p, pg, pre, relu1, grid, stream};
    if (pre) return gated && !fmid && f2 == (RG_RES | RG_LN | NA) ? launch_chain<RG_RES | RG_LN | NA, true, 0, true>(c) : -1;
    if (gated) {
        if (fmid) return -1;
        switch (f2) {
        case RG_RES | RG_LN | NA: return launch_chain<RG_RES | RG_LN | NA, true>(c);
        case RG_RES | RG_HEADS | NA: return launch_chain<RG_RES | RG_HEADS | NA, true>(c);
        default: return -1;
        }
    }
    if (fmid) return fmid == LNR && f2 == (RG_RES | RG_LN) ? launch_chain<RG_RES | RG_LN, false, LNR>(c) : -1;
    switch (f2) {
    case RG_RES | NA: return launch_chain<RG_RES | NA>(c);   // (c1 / c2: no addend loads, + 0 in their place)
    case LNR: return launch_chain<LNR>(c);
    case RG_RES: return launch_chain<RG_RES>(c);
    case RG_GATE | RG_LN: return launch_chain<RG_GATE | RG_LN>(c);
    case RG_GATE | RG_HEADS: return launch_chain<RG_GATE | RG_HEADS>(c);
    default: return -1;
    }
}

}  // namespace dpvo

#ifdef DPVO_STAMPS
extern "C" int dpvo_diag_stamps(void* host, size_t bytes)
{
    using namespace dpvo;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dpvo_stamps), std::min(bytes, sizeof(dpvo_stamps)), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
