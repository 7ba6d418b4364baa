// rowgemm.hpp -- what the row-GEMM units share (rowgemm.hip, rowgemm_rowmajor.hip,
// rowgemm_kblocked.hip): vector types and constants, the two-rows-per-wave row
// epilogue, the PRELN row operands, the y-tile maps, the wave frame of the
// k-blocked family, and the per-family host launchers (the only cross-file
// surface).  Everything device-side sits in an anonymous namespace: each unit
// gets its own copy, the two __device__ constant rows included (read-only).
#pragma once

#include "common.hpp"

#include <type_traits>

namespace dpvo {

// ---------------------------------------------------------------------------
// host launchers, one per kernel family.  Arguments are validated and the
// grid sized by the caller (rowgemm.hip); a launcher picks the instantiation
// and returns -1 when there is none for the flags it was given.
// ---------------------------------------------------------------------------
// rowgemm_rowmajor.hip: flags = an epilogue set of dpvo_rowgemm (dual: 0 only, b = the second GEMM)
int launch_rowgemm3(int flags, bool dual, const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid,
                    hipStream_t stream);
// rowgemm_kblocked.hip: flags = 0 / RELU / SIGMOID (dual: 0 only)
int launch_rowgemm5(int flags, bool dual, const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, unsigned grid,
                    hipStream_t stream);
int launch_rowgemm_narrow(int flags, const dpvo_rowgemm_args& a, unsigned grid, hipStream_t stream);   // K = 384 / 896
int launch_rowpair6(const dpvo_rowgemm_args& a, const dpvo_rowgemm_args& b, const dpvo_rowadd_args* pre, unsigned grid,
                    hipStream_t stream);
// f2: the last GEMM's epilogue as the kernel takes it (RG_* with RG_NOADD);
// fmid != 0: the three-GEMM chain (pg the middle Linear), gated: pg the gate
// Linear, pre != nullptr: the PRELN gated chain
int launch_rowchain5(int f2, bool gated, int fmid, bool relu1, const dpvo_rowgemm_args& g1, const dpvo_rowgemm_args& p,
                     const dpvo_rowgemm_args& pg, const dpvo_rowadd_args* pre, unsigned grid, hipStream_t stream);

namespace {

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

constexpr int RG_BM = 128, RG_BN = 384, RG_BK = 64, RG_THREADS = 512;
constexpr int RG_A_STAGE = RG_BM * RG_BK * 2;   // 16 KB
constexpr int RG_W_STAGE = RG_BN * RG_BK * 2;   // 48 KB

enum {
    RG_RELU = DPVO_RG_RELU, RG_SIGMOID = DPVO_RG_SIGMOID, RG_RES = DPVO_RG_RES, RG_GATE = DPVO_RG_GATE,
    RG_LN = DPVO_RG_LN, RG_LN_RELU = DPVO_RG_LN_RELU, RG_HEADS = DPVO_RG_HEADS,
    RG_NOADD = 1 << 20   // (device side only) RES without a res16 addend: + 0 in its place, no loads
};

// the k-blocked family: 512 threads, BK = 32, a 96 KB y tile and a 4-slot A ring
constexpr int R5_THREADS = 512, R5_BK = 32;
constexpr int R5_Y = RG_BM * 768;                  // 96 KB
constexpr int R5_ASLOT = RG_BM * R5_BK * 2;        // 8 KB
constexpr int R5_LDS = R5_Y + 4 * R5_ASLOT;        // 128 KB
constexpr int R5_IDX_TILES = 8;       // rowchain5: tiles per block whose row sources sit in LDS
constexpr int R5_PRE_IDX_TILES = 8;   // rowpair6 PRE: tiles per block whose addend sources sit in LDS
constexpr int P6_MINK = 4, P6_MAXK = 12;   // rowpair6: k-steps of a resident A tile (128 <= K <= 384 fits LDS)
constexpr int RN_BM = 32;                  // rowgemm_narrow: rows per tile

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ float hround(float v) { return (float)(half_t)v; }

__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// sum over half a wave (32 lanes): a DPP row reduce plus one gfx950 lane swap,
// VALU only (a + b == b + a, so every lane of the half agrees)
__device__ __forceinline__ float half_sum(float x)
{
    x = row16_sum(x);
    auto h = __builtin_amdgcn_permlane16_swap(__float_as_int(x), __float_as_int(x), false, false);
    return __int_as_float(h[0]) + __int_as_float(h[1]);
}

// one accumulator fragment -> the autocast Linear's output: fp16(acc + b) [-> relu | sigmoid]
__device__ __forceinline__ h4_t rg_y4(const f4_t& acc, const h4_t& b, bool relu, bool sigm)
{
    h4_t y;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        half_t v = (half_t)(acc[r] + (float)b[r]);
        if (relu) v = v > (half_t)0 ? v : (half_t)0;
        if (sigm) v = (half_t)fast_sigmoid((float)v);
        y[r] = v;
    }
    return y;
}

// ---- the row epilogue with two rows per wave: half h = lane/32 takes row
// 2i + h, lane s = lane%32 of the half owns columns 4s + 128j (j < 3), so every
// global access is a 16-byte (fp32) or 8-byte (fp16) vector -- half the store
// instructions of a one-row-per-wave layout, whose completions every next-tile
// k-step wait includes (one vmcnt for loads and stores).  Row sums: half_sum.
typedef float ep_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 ep_h4 __attribute__((ext_vector_type(4)));

struct EpiConsts2 {
    ep_f4 g[3], b[3];     // LayerNorm weight / bias at this lane's columns
    ep_f4 hw[4][3];       // head weights (fp16 values)
    float hb[4];
};

template <int FLAGS>
__device__ __forceinline__ void load_consts2(const dpvo_rowgemm_args& p, int lane, EpiConsts2& k)
{
    const int s = lane & 31;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int c = 128 * j + 4 * s;
        if (FLAGS & RG_LN) {
            k.g[j] = *(const ep_f4*)(p.ln_g + c);
            k.b[j] = *(const ep_f4*)(p.ln_b + c);
        }
        if (FLAGS & RG_HEADS) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const ep_h4 w = *(const ep_h4*)((const half_t*)p.head_w + q * RG_BN + c);
                k.hw[q][j] = ep_f4{(float)w[0], (float)w[1], (float)w[2], (float)w[3]};
            }
        }
    }
    if (FLAGS & RG_HEADS) {
#pragma unroll
        for (int q = 0; q < 4; q++) k.hb[q] = (float)((const half_t*)p.head_b)[q];
    }
}

template <int R>   // R rows = R/2 row pairs
struct EpiOps2 {
    ep_f4 base[R / 2][3];   // res32
    ep_h4 add[R / 2][3];    // res16[idx] or gate16
};

// A row of zeros the epilogue reads in place of an absent res16 row: the add
// registers are then always load destinations (a zero-fill branch beside the
// load made the compiler drain every outstanding load -- the chain's W / A
// prefetch included -- before each OVL batch, to order the zero writes after
// the registers' previous loads).
__device__ half_t g_epi_zero_row[RG_BN];   // (device globals start zeroed)

template <int FLAGS, int R>
__device__ __forceinline__ void epi2_load(const dpvo_rowgemm_args& p, int64_t M, int64_t row0, int lane, EpiOps2<R>& o)
{
    if (!(FLAGS & (RG_RES | RG_GATE))) return;
    const int h = lane >> 5, s = lane & 31;
#pragma unroll
    for (int i = 0; i < R / 2; i++) {
        const int64_t rr = row0 + 2 * i + h;
        const int64_t row = rr < M ? rr : M - 1;   // clamped for loads; stores skip rows >= M
        const float* r32 = (const float*)p.res32 + row * p.ldr;
        const half_t* r16 = g_epi_zero_row;
        if (FLAGS & RG_GATE) {
            r16 = (const half_t*)p.gate16 + row * RG_BN;
        } else if (p.res16) {
            const int64_t src = p.res16_idx ? p.res16_idx[row] : row;
            if (src >= 0) r16 = (const half_t*)p.res16 + src * RG_BN;
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int c = 128 * j + 4 * s;
            o.base[i][j] = *(const ep_f4*)(r32 + c);
            if (!(FLAGS & RG_NOADD)) o.add[i][j] = *(const ep_h4*)(r16 + c);
        }
    }
}

// yget(i, j): the fp16 y of row 2 i + h, columns 128 j + 4 s .. + 3 (from the
// y tile in LDS, or from registers in the warp-specialised chain)
template <int FLAGS, int R, typename YGet>
__device__ __forceinline__ void epi2_finish(const dpvo_rowgemm_args& p, int64_t M, YGet yget, int64_t row0, int lane,
                                            const EpiConsts2& k, const EpiOps2<R>& o)
{
    const int h = lane >> 5, s = lane & 31;
    ep_f4 v[R / 2][3];
#pragma unroll
    for (int i = 0; i < R / 2; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const ep_h4 y = yget(i, j);
            v[i][j] = ep_f4{(float)y[0], (float)y[1], (float)y[2], (float)y[3]};
        }
    }
    if (FLAGS & (RG_RES | RG_GATE)) {
#pragma unroll
        for (int i = 0; i < R / 2; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                // (NOADD: + 0.f as the zero row's addend -- -0 + 0 is +0, kept bit for bit)
                const ep_f4 add = (FLAGS & RG_NOADD) ? ep_f4{0.f, 0.f, 0.f, 0.f}
                                                     : ep_f4{(float)o.add[i][j][0], (float)o.add[i][j][1],
                                                             (float)o.add[i][j][2], (float)o.add[i][j][3]};
                if (FLAGS & RG_GATE) {   // x + fp16(gate * res)   (blocks.py:30, fp16 product)
#pragma unroll
                    for (int t = 0; t < 4; t++) v[i][j][t] = o.base[i][j][t] + hround(add[t] * v[i][j][t]);
                } else {                 // (res32 + res16) + y
                    v[i][j] = (o.base[i][j] + add) + v[i][j];
                }
            }
    }
    if (FLAGS & RG_LN) {
#pragma unroll
        for (int i = 0; i < R / 2; i++) {
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++) sm += (v[i][j][0] + v[i][j][1]) + (v[i][j][2] + v[i][j][3]);
            const float mean = half_sum(sm) * (1.f / RG_BN);
            float sq = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const ep_f4 d = v[i][j] - mean;
                sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
            const float rstd = rsqrtf(half_sum(sq) * (1.f / RG_BN) + p.ln_eps);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                v[i][j] = (v[i][j] - mean) * rstd * k.g[j] + k.b[j];
                if (FLAGS & RG_LN_RELU)
#pragma unroll
                    for (int t = 0; t < 4; t++) v[i][j][t] = fmaxf(v[i][j][t], 0.f);
            }
        }
    }
    if (FLAGS & RG_HEADS) {
        // d = W_d relu(v) + b_d ; w = sigmoid(W_w relu(v) + b_w)   (fp16 operands, fp32 accumulate)
#pragma unroll
        for (int i = 0; i < R / 2; i++) {
            float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float x = hround(fmaxf(v[i][j][t], 0.f));
#pragma unroll
                    for (int q = 0; q < 4; q++) d[q] += x * k.hw[q][j][t];
                }
            half_t ho[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float z = hround(half_sum(d[q]) + k.hb[q]);
                if (q >= 2) z = hround(fast_sigmoid(z));
                ho[q] = (half_t)z;
            }
            const int64_t row = row0 + 2 * i + h;
            if (s == 0 && row < M) *(ep_h4*)((half_t*)p.head_out + row * 4) = ep_h4{ho[0], ho[1], ho[2], ho[3]};
        }
    }
#pragma unroll
    for (int i = 0; i < R / 2; i++) {
        const int64_t row = row0 + 2 * i + h;
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int c = 128 * j + 4 * s;
            if (p.out32) *(ep_f4*)((float*)p.out32 + row * p.ldo32 + c) = v[i][j];
            if (p.out16)
                *(ep_h4*)((half_t*)p.out16 + row * p.ldo16 + c) =
                    ep_h4{(half_t)v[i][j][0], (half_t)v[i][j][1], (half_t)v[i][j][2], (half_t)v[i][j][3]};
        }
    }
}

template <int FLAGS, int R, typename YMap>
__device__ __forceinline__ void epilogue_rows2(const dpvo_rowgemm_args& p, int64_t M, const char* smem, YMap ym,
                                               int lrow0, int64_t row0, int lane, const EpiConsts2& k)
{
    EpiOps2<R> o;
    epi2_load<FLAGS, R>(p, M, row0, lane, o);
    const int h = lane >> 5, s = lane & 31;
    epi2_finish<FLAGS, R>(
        p, M, [&](int i, int j) { return *(const ep_h4*)(smem + ym.off(lrow0 + 2 * i + h, (128 * j + 4 * s) * 2)); },
        row0, lane, k, o);
}

// ---- y-tile maps
struct YMapSlot {   // 64 rows x 768 B in one W slot, 32-B granules XOR (row/4)&3
    int base;
    __device__ int off(int r, int byte) const { return base + r * 768 + (byte ^ (((r >> 2) & 3) << 5)); }
};

struct YMapChunk {   // 128 rows x 768 B, 16-byte chunks XOR (row & 15): conflict-free
    // ds_read_b128 fragment reads down 16 rows and 256-byte row sweeps
    __device__ int off(int r, int byte) const { return r * 768 + (((byte >> 4) ^ (r & 15)) << 4) + (byte & 15); }
};

// chunk swizzle of the BK = 32 stage rows (64 B = four 16-byte chunks): the
// physical chunk p of row r holds logical chunk p ^ rc_sw(r), with rc_sw =
// [0, 2, 3, 1][(r >> 2) & 3].  Each ds_read_b128 lane group ({0-3, 12-15,
// 20-27}, ...) reads rows fr = lane & 15 at chunk fq = lane >> 4; with this
// permutation its 16 lanes hit 16 distinct 16-byte bank slots (the plain
// (r >> 2) & 3 xor put two lanes on each slot: 2-way conflicts on every
// fragment read, 46 % of the chain kernels' LDS cycles).
__device__ __forceinline__ int rc_sw(int r) { return (0x78 >> (((r >> 2) & 3) << 1)) & 3; }

// f(integral_constant<int, K>) for K = B .. E-1, expanded at compile time
template <int B, int E>
struct bd_steps {
    template <class F>
    __device__ __forceinline__ static void run(F&& f)
    {
        if constexpr (B < E) {
            f(std::integral_constant<int, B>{});
            bd_steps<B + 1, E>::run(f);
        }
    }
};

// (tile, pass, k-step) of a flat step, advanced one step at a time (no
// 64-bit divisions); past the end it stays on the last step
struct R5Cursor {
    int64_t f, t;
    int k, q;
    __device__ __forceinline__ void next(int64_t total, int nks, int np, unsigned grid)
    {
        if (f + 1 >= total) return;
        f++;
        if (++k == nks) {
            k = 0;
            if (++q == np) {
                q = 0;
                t += grid;
            }
        }
    }
};

struct R5WCursor {   // (tile, segment, k-step) of the chains' flat W-step sequence
    int64_t f, t;
    int s, k;
    __device__ __forceinline__ void next(int64_t total, int n0, int n1, int n2, int nseg, unsigned grid)
    {
        if (f + 1 >= total) return;
        f++;
        if (++k == (s == 0 ? n0 : s == 1 ? n1 : n2)) {
            k = 0;
            if (++s == nseg) {
                s = 0;
                t += grid;
            }
        }
    }
};

#ifdef DPVO_STAMPS
// Diagnostic build only (never the product library): per-wave cycle sums of
// the k-blocked kernels' k-loop segments, s_memtime stamps (cdna guide,
// In-kernel stamps), written to dpvo_stamps[block][wave][segment]
// (rowgemm_kblocked.hip).
constexpr int ST_SEGS = 16;
#define RC_STAMP(v)                                                                            \
    unsigned long long v;                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");                  \
    __builtin_amdgcn_sched_barrier(0);
#define RC_ACC(seg, a, b) st_sum[seg] += (b) - (a);
#else
#define RC_STAMP(v)
#define RC_ACC(seg, a, b)
#endif

// The addend of a row without one: -0, so that v + b == v for every v (rowadd_ln
// then adds nothing; a +0 would turn -0 into +0)
struct R5NegZeroRow {
    unsigned short v[RG_BN];
    constexpr R5NegZeroRow() : v{}
    {
        for (int i = 0; i < RG_BN; i++) v[i] = 0x8000;
    }
};
// (a non-const __device__ object: global address space, so that a pointer to
// it or to an addend row stays a global pointer -- a constant one made the
// loads through it flat loads)
__device__ R5NegZeroRow g_pre_negzero = R5NegZeroRow{};

// PRELN's row operands: R rows (R / 2 row pairs, half a wave per row, lane s
// of the half at columns 4 s + 128 j: rowadd_ln's and epi2's layout)
template <int R>
struct PreOps {
    ep_f4 a[R / 2][3];
    ep_h4 b[R / 2][3], c[R / 2][3];
};
template <int R>
__device__ __forceinline__ void preln_issue(const dpvo_rowadd_args& pre, int64_t M, int64_t row0, int lane, PreOps<R>& o)
{
    const int h = lane >> 5, s = lane & 31;
    const half_t* negzero = (const half_t*)g_pre_negzero.v;
#pragma unroll
    for (int i = 0; i < R / 2; i++) {
        const int64_t rr = row0 + 2 * i + h;
        const int64_t row = rr < M ? rr : M - 1;   // clamped for loads; stores skip rows >= M
        const int64_t sb = pre.b_idx ? pre.b_idx[row] : row;
        const int64_t sc = pre.c_idx ? pre.c_idx[row] : row;
        const half_t* b = pre.b16 && sb >= 0 && sb < pre.b_rows ? (const half_t*)pre.b16 + sb * RG_BN : negzero;
        const half_t* c = pre.c16 && sc >= 0 && sc < pre.c_rows ? (const half_t*)pre.c16 + sc * RG_BN : negzero;
        const float* a = (const float*)pre.a + row * pre.lda;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int col = 128 * j + 4 * s;
            o.a[i][j] = *(const ep_f4*)(a + col);
            o.b[i][j] = *(const ep_h4*)(b + col);
            o.c[i][j] = *(const ep_h4*)(c + col);
        }
    }
}
// base = rowadd_ln(a, b16, c16, LN)'s out32 rows, operation for operation:
// ((a + b) + c), the 12 values of a lane summed in order, half-wave sums,
// then (v - mean) * rstd * g + beta
template <int R>
__device__ __forceinline__ void preln_rows(const dpvo_rowadd_args& pre, int lane, const PreOps<R>& o, EpiOps2<R>& e)
{
    const int s = lane & 31;
#pragma unroll
    for (int i = 0; i < R / 2; i++) {
        float v[12];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) v[4 * j + t] = o.a[i][j][t];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) v[4 * j + t] += (float)o.b[i][j][t];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) v[4 * j + t] += (float)o.c[i][j][t];
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < 12; j++) sm += v[j];
        const float mean = half_sum(sm) * (1.f / RG_BN);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 12; j++) q += (v[j] - mean) * (v[j] - mean);
        const float rstd = rsqrtf(half_sum(q) * (1.f / RG_BN) + pre.ln_eps);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const ep_f4 g = *(const ep_f4*)(pre.ln_g + 128 * j + 4 * s);
            const ep_f4 bt = *(const ep_f4*)(pre.ln_b + 128 * j + 4 * s);
#pragma unroll
            for (int t = 0; t < 4; t++) e.base[i][j][t] = (v[4 * j + t] - mean) * rstd * g[t] + bt[t];
        }
    }
}

// ---------------------------------------------------------------------------
// The wave frame of the k-blocked family (rowgemm5 / rowpair6 / rowchain5):
// 8 waves as 1 (M) x 8 (N), wave w on all 128 rows x columns 48 w .. 48 w + 47
// (8 x 3 mfma_f32_16x16x32_f16 accumulators).  W is [K/32][384][32]: a fragment
// = one contiguous 1 KB; A stages are 128 rows x 64 B slots with the rc_sw
// chunk swizzle.  Each kernel keeps its own schedule around these pieces.
// ---------------------------------------------------------------------------
struct R5Lane {
    int w;        // the wave (wave-uniform)
    int fr, fq;   // MFMA fragment: row / column lane & 15, k chunk lane >> 4
    int ar, ac;   // A staging: the lane holds row 16 w + (lane >> 2), logical chunk lane & 3
    int aw_off;   // slot image: row r, physical chunk ac ^ rc_sw(r) holds logical chunk ac
    int ar_off;   // fragment read of row 16 mt + fr: + 1024 mt
    int wcol;     // W fragments: column 48 w + 16 nt + fr, k 8 fq .. 8 fq + 7 of the step
    __device__ __forceinline__ R5Lane(int lane, int wave)
        : w(wave), fr(lane & 15), fq(lane >> 4), ar(16 * wave + (lane >> 2)), ac(lane & 3),
          aw_off(ar * 64 + 16 * (ac ^ rc_sw(ar))), ar_off(fr * 64 + 16 * (fq ^ rc_sw(fr))),
          wcol((48 * wave + fr) * R5_BK + 8 * fq)
    {
    }
};

// The A row that output row m reads with gather index src: the zero row past
// Mrows and for a negative or out-of-range index
__device__ __forceinline__ const half_t* r5_a_at(const dpvo_rowgemm_args& p, int64_t Mrows, int64_t m, int64_t src)
{
    const half_t* row = (const half_t*)p.zero_row;
    if (m < Mrows && src >= 0 && src < p.a_rows) row = (const half_t*)p.A + src * p.lda;
    return row;
}
// ... with the index read from p.a_idx (or m itself without one)
__device__ __forceinline__ const half_t* r5_a_source(const dpvo_rowgemm_args& p, int64_t Mrows, int64_t m)
{
    const half_t* row = (const half_t*)p.zero_row;
    if (p.a_idx) {   // (the index load's wait inside the branch, not at the join)
        if (m < Mrows) {
            const int64_t src = p.a_idx[m];
            if (src >= 0 && src < p.a_rows) row = (const half_t*)p.A + src * p.lda;
        }
    } else if (m < Mrows && m < p.a_rows) {
        row = (const half_t*)p.A + m * p.lda;
    }
    return row;
}

// the three W fragments of k-step k (off: the lane's offset inside a k-block)
__device__ __forceinline__ void r5_load_w(const half_t* W, int k, int off, h8_t (&r)[3])
{
    const half_t* src = W + (int64_t)k * (RG_BN * R5_BK) + off;
#pragma unroll
    for (int nt = 0; nt < 3; nt++) r[nt] = *(const h8_t*)(src + nt * 16 * R5_BK);
}

// one k-step: NMT A fragments (a_at(mt): the address of m-tile mt's) against
// the three W fragments.  W as the first operand: the accumulator is the
// transposed tile, lane (fr, fq) holding row fr, columns 4 fq .. 4 fq + 3 of
// each 16 x 16 block
template <int NMT, class AAt>
__device__ __forceinline__ void r5_mfmas(AAt a_at, const h8_t (&wr)[3], f4_t (&acc)[NMT][3])
{
    h8_t a[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) a[mt] = *(const h8_t*)a_at(mt);
#pragma unroll
    for (int nt = 0; nt < 3; nt++)
#pragma unroll
        for (int mt = 0; mt < NMT; mt++)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wr[nt], a[mt], acc[mt][nt], 0, 0, 0);
}
// ... with the A fragments of an A-ring / resident slot
__device__ __forceinline__ void r5_mfmas_slot(const char* slot, const R5Lane& L, const h8_t (&wr)[3], f4_t (&acc)[8][3])
{
    r5_mfmas([&](int mt) { return slot + L.ar_off + 1024 * mt; }, wr, acc);
}

// acc + bias -> act -> fp16 -> y tile: m-tiles mt0 .. mt0 + NMT - 1 of the
// wave's columns into rows 16 m + fr of ytile (YMapChunk).  bias_of(nt, col):
// the four biases at column col; ZERO: the accumulators are cleared behind.
template <int NMT, bool ZERO, class Bias>
__device__ __forceinline__ void r5_acc_to_y(f4_t (&acc)[8][3], int mt0, Bias bias_of, bool relu, bool sigm, char* ytile,
                                            const R5Lane& L)
{
    const YMapChunk ym;
#pragma unroll
    for (int nt = 0; nt < 3; nt++) {
        const int col = 48 * L.w + 16 * nt + 4 * L.fq;
        const h4_t b = bias_of(nt, col);
#pragma unroll
        for (int m = 0; m < NMT; m++) {
            const h4_t y = rg_y4(acc[mt0 + m][nt], b, relu, sigm);
            if (ZERO) acc[mt0 + m][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
            *(h4_t*)(ytile + ym.off(16 * m + L.fr, col * 2)) = y;
        }
    }
}

// whole rows out of a y tile into pe.out16: wave w stores local rows RPW w ..
// RPW w + RPW - 1 (row_of(local): the global row), one 768-byte row per
// instruction (lanes 0-47, 16 bytes each: 16 stores per lane and 128 rows
// instead of 24 of 8 bytes); rows that are only 8-byte aligned go two per
// pass, 8 bytes per lane.  (pe, Mrows, w and lane by reference and the row as
// the caller's own expression: passed by value they changed rowpair6's and
// rowgemm5's allocation.)
template <int RPW, class RowOf>
__device__ __forceinline__ void r5_store_rows(const char* ytile, const dpvo_rowgemm_args& pe, const RowOf& row_of,
                                              const int64_t& Mrows, const int& w, const int& lane)
{
    const YMapChunk ym;
    half_t* out = (half_t*)pe.out16;
    if (((uintptr_t)out & 15) == 0 && (pe.ldo16 & 7) == 0) {
        if (lane < 48) {
#pragma unroll 4
            for (int i = 0; i < RPW; i++) {
                const int lr = RPW * w + i;
                const int64_t row = row_of(lr);
                const h8_t v = *(const h8_t*)(ytile + ym.off(lr, 16 * lane));
                if (row < Mrows) *(h8_t*)(out + row * pe.ldo16 + 8 * lane) = v;
            }
        }
    } else {
        const int h = lane >> 5, s = lane & 31;
#pragma unroll 2
        for (int i = 0; i < RPW / 2; i++) {
            const int lr = RPW * w + 2 * i + h;
            const int64_t row = row_of(lr);
            ep_h4 v[3];
#pragma unroll
            for (int j = 0; j < 3; j++) v[j] = *(const ep_h4*)(ytile + ym.off(lr, (128 * j + 4 * s) * 2));
            if (row < Mrows) {
#pragma unroll
                for (int j = 0; j < 3; j++) *(ep_h4*)(out + row * pe.ldo16 + 128 * j + 4 * s) = v[j];
            }
        }
    }
}

}  // namespace
}  // namespace dpvo
