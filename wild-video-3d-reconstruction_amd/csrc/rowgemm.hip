// rowgemm.hip -- the row-GEMM entry points of the C ABI: full-row MFMA GEMMs
// with fused update-operator epilogues (gfx950).
//
// The learned update operator (reference dpvo/net.py:75-93, blocks.py) is a
// chain of Linear(384 -> 384) layers over E ~ 95k edge rows, glued by
// LayerNorm, ReLU/sigmoid, residual adds, gating and row gathers.  Under the
// reference's autocast every Linear is an fp16 GEMM (fp32 accumulate, fp16
// output) and every glue op is its own elementwise pass over E x 384 fp32.
//
// Here one kernel computes   Y = A W^T + b   for a tile of 128 rows and ALL
// 384 output columns, so any row-wise op can run in the epilogue:
//   y16 = fp16(acc + b)  [-> relu | sigmoid]          (autocast Linear output)
//   v   = y  | res32 + res16[idx] + y | res32 + fp16(gate16 * y)
//   v   = LayerNorm(v) [-> relu]                       (fp32, as autocast)
//   heads: d = W_d relu(v) + b_d, w = sigmoid(W_w relu(v) + b_w)  (fp16 out)
//   out32 = v, out16 = fp16(v)
// A rows may be gathered through an index (idx < 0 -> a zero row), which
// fuses `mask_ix * net[:, ix]` (net.py:82-85) into the GEMM's operand load.
//
// This file validates, sizes the grid and dispatches; the GEMM kernels live in
//   rowgemm_kblocked.hip  W k-blocked [K/32][384][32], streamed L2 -> registers:
//                         EVERY launch of DPVO.update() (the hot path)
//   rowgemm_rowmajor.hip  W row-major [384][K], LDS-DMA: the fallback for a
//                         plain [384][K] weight and the tests' reference
// and share rowgemm.hpp.  Entry point -> kernel (file):
//   dpvo_rowgemm            WKB: rowgemm5_kernel, or rowgemm_narrow_kernel with a
//                           device row count at K = 384 / 896 (kblocked);
//                           otherwise rowgemm3_kernel (rowmajor)
//   dpvo_rowgemm_pair       WKB: rowpair6_kernel at 128 <= K <= 384, else
//                           rowgemm5_kernel DUAL (kblocked); otherwise
//                           rowgemm3_kernel DUAL (rowmajor)
//   dpvo_rowgemm_pair_pre   rowpair6_kernel PRE (kblocked)
//   dpvo_rowchain, dpvo_rowchain3, dpvo_rowchain_gated, dpvo_rowchain_gated_pre
//                           rowchain5_kernel (kblocked)
//   dpvo_rowadd_ln          rowadd_ln_kernel (below)
#include "rowgemm.hpp"

#include <algorithm>

namespace dpvo {
namespace {

// v = a32[row] (+ b16[idx[row]]) -> [LayerNorm] -> out32 / out16
// Half a wave per row: lane l of the half covers columns 4l + 128j (j < 3), so
// every access is a 16-byte (fp32) or 8-byte (fp16) vector and one wave keeps
// two rows' loads in flight.  HBM-bound: 4 B x 384 in, 6 B x 384 out per row.
typedef float rl_f4 __attribute__((ext_vector_type(4)));
typedef half_t rl_h4 __attribute__((ext_vector_type(4)));

// Every load of a row is issued before the first use: the two row-source
// indices together, then the a, b and c rows together (absent addends read a
// row of -0, so v + b == v exactly, as the skipped add; the fp16 / fp32 choice
// of a is a template parameter).  Branching per load had the compiler wait on
// each in turn: ~7 dependent HBM round trips per row, 67 us at C3.
template <bool A16>
__global__ __launch_bounds__(256) void rowadd_ln_kernel(dpvo_rowadd_args p)
{
    const int sub = threadIdx.x & 31;
    float g[12], bt[12];
    if (p.ln_g) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const rl_f4 gg = *(const rl_f4*)((const float*)p.ln_g + 128 * j + 4 * sub);
            const rl_f4 bb = *(const rl_f4*)((const float*)p.ln_b + 128 * j + 4 * sub);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                g[4 * j + t] = gg[t];
                bt[4 * j + t] = bb[t];
            }
        }
    }
    const half_t* negzero = (const half_t*)g_pre_negzero.v;
    for (int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 5; row < p.M;
         row += ((int64_t)gridDim.x * blockDim.x) >> 5) {
        float v[12];
        const int64_t sb = p.b_idx ? p.b_idx[row] : row;
        const int64_t sc = p.c_idx ? p.c_idx[row] : row;
        const half_t* b = p.b16 && sb >= 0 && sb < p.b_rows ? (const half_t*)p.b16 + sb * RG_BN : negzero;
        const half_t* c2 = p.c16 && sc >= 0 && sc < p.c_rows ? (const half_t*)p.c16 + sc * RG_BN : negzero;
        rl_h4 hb[3], hc[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int c = 128 * j + 4 * sub;
            if constexpr (A16) {
                const rl_h4 h = *(const rl_h4*)((const half_t*)p.a + row * p.lda + c);
#pragma unroll
                for (int t = 0; t < 4; t++) v[4 * j + t] = (float)h[t];
            } else {
                const rl_f4 a = *(const rl_f4*)((const float*)p.a + row * p.lda + c);
#pragma unroll
                for (int t = 0; t < 4; t++) v[4 * j + t] = a[t];
            }
            hb[j] = *(const rl_h4*)(b + c);
            hc[j] = *(const rl_h4*)(c2 + c);
        }
        // ((a + b) + c: the two row adds of consecutive rowadd_ln calls, in order)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) v[4 * j + t] += (float)hb[j][t];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) v[4 * j + t] += (float)hc[j][t];
        if (p.ln_g) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 12; j++) s += v[j];
            const float mean = half_sum(s) * (1.f / RG_BN);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 12; j++) q += (v[j] - mean) * (v[j] - mean);
            const float rstd = rsqrtf(half_sum(q) * (1.f / RG_BN) + p.ln_eps);
#pragma unroll
            for (int j = 0; j < 12; j++) v[j] = (v[j] - mean) * rstd * g[j] + bt[j];
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int c = 128 * j + 4 * sub;
            if (p.out32) *(rl_f4*)((float*)p.out32 + row * RG_BN + c) = rl_f4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
            if (p.out16)
                *(rl_h4*)((half_t*)p.out16 + row * RG_BN + c) =
                    rl_h4{(half_t)v[4 * j], (half_t)v[4 * j + 1], (half_t)v[4 * j + 2], (half_t)v[4 * j + 3]};
        }
    }
}

int g_num_cus = 0;

int ensure_num_cus()
{
    if (g_num_cus == 0) {
        int dev = 0;
        DPVO_CHECK_HIP(hipGetDevice(&dev));
        DPVO_CHECK_HIP(hipDeviceGetAttribute(&g_num_cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (g_num_cus <= 0) g_num_cus = 256;
    }
    return 0;
}

// Blocks of a persistent 128-row-tile kernel: one per tile up to one per
// compute unit; cap > 0: at least ntiles / cap, so that no block walks more
// than cap tiles (what its LDS index table holds).  After ensure_num_cus().
unsigned persistent_grid(int64_t M, int cap = 0)
{
    const int64_t ntiles = (M + RG_BM - 1) / RG_BM;
    int64_t grid = std::min<int64_t>(ntiles, g_num_cus);
    if (cap > 0) grid = std::max<int64_t>(grid, (ntiles + cap - 1) / cap);
    return (unsigned)grid;
}

inline bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// What every kernel requires of one GEMM's operands; `who` prefixes the
// message.  reads_a: the GEMM streams A from memory (any K % 64 == 0, A / lda /
// zero_row checked); otherwise it is a later GEMM of a chain and reads the
// 384-wide intermediate.  The epilogue's inputs and outputs are checked with
// epilogue = true (gate_on_chip: the gate comes from a gate GEMM, not gate16).
#define RG_CHECK(cond, msg) DPVO_CHECK_ARG(cond, std::string(who) + ": " + (msg))
int check_gemm(const char* who, const dpvo_rowgemm_args* a, bool reads_a, bool epilogue, bool gate_on_chip = false)
{
    RG_CHECK(a != nullptr, "null args");
    RG_CHECK(a->N == RG_BN, "output width must be 384");
    RG_CHECK(a->W && a->bias, "W and bias are required");
    RG_CHECK(aligned(a->W, 16), "W must be 16-byte aligned");
    RG_CHECK(aligned(a->bias, 8), "bias must be 8-byte aligned");
    if (reads_a) {
        // (the k-blocked kernels step K by 32 with one barrier per TWO k-steps: K a
        // multiple of 64 makes every tile's last k-step odd, so the even step after
        // it separates a tile's y-tile reads from the next tile's writes -- K = 32
        // would race; the row-major kernel stages K in steps of 64)
        RG_CHECK(a->K > 0 && a->K % RG_BK == 0, "K must be a positive multiple of 64 (pad W with zeros)");
        RG_CHECK(a->A && a->zero_row, "A and zero_row are required");
        RG_CHECK(a->lda >= a->K && a->lda % 8 == 0, "lda must be >= K and a multiple of 8");
        RG_CHECK(aligned(a->A, 16) && aligned(a->zero_row, 16), "A and zero_row must be 16-byte aligned");
    } else {
        RG_CHECK(a->K == RG_BN, "a chained GEMM's K must be 384 (the intermediate width)");
    }
    if (!epilogue) return 0;
    const int f = a->flags;
    RG_CHECK(!(f & (DPVO_RG_RES | DPVO_RG_GATE)) || a->res32, "residual input missing");
    RG_CHECK(!(f & DPVO_RG_GATE) || a->gate16 || gate_on_chip, "gate input missing");
    RG_CHECK(!(f & DPVO_RG_LN) || (a->ln_g && a->ln_b), "LayerNorm weights missing");
    RG_CHECK(!(f & DPVO_RG_HEADS) || (a->head_w && a->head_b && a->head_out), "head weights missing");
    RG_CHECK(!a->out16 || (a->ldo16 % 4 == 0 && aligned(a->out16, 8)), "out16 needs 8-byte aligned rows (ldo16 % 4 == 0)");
    RG_CHECK(!a->out32 || (a->ldo32 % 4 == 0 && aligned(a->out32, 16)), "out32 needs 16-byte aligned rows (ldo32 % 4 == 0)");
    return 0;
}

// dpvo_rowgemm's and the pairs' own rule: what a k-blocked W restricts
int check_rowgemm(const dpvo_rowgemm_args* a)
{
    const char* who = "rowgemm";
    if (check_gemm(who, a, true, true)) return -1;
    if (a->flags & DPVO_RG_WKB) {
        RG_CHECK((a->flags & ~(DPVO_RG_WKB | DPVO_RG_RELU | DPVO_RG_SIGMOID)) == 0,
                 "k-blocked W (WKB) takes only RELU / SIGMOID");
        RG_CHECK(a->out16 && !a->out32, "WKB writes out16 only (8-byte aligned rows)");
    }
    return 0;
}

// the first GEMM of a chain: an activation only, its epilogue fields unused
int check_chain_first(const char* who, const dpvo_rowgemm_args* g1)
{
    if (check_gemm(who, g1, true, false)) return -1;
    RG_CHECK((g1->flags & ~(DPVO_RG_RELU | DPVO_RG_SIGMOID)) == 0, "the first GEMM takes only an activation");
    return 0;
}

int chain_status(int rc, const char* who, int flags)
{
    if (rc) {
        set_error(std::string(who) + ": unsupported epilogue flag combination " + std::to_string(flags));
        return -1;
    }
    DPVO_CHECK_LAUNCH();
    return 0;
}

int rowchain_launch(const dpvo_rowgemm_args* g1, const dpvo_rowgemm_args* g2, const dpvo_rowgemm_args* gate, void* stream,
                    const dpvo_rowadd_args* pre = nullptr)
{
    const char* who = pre ? "rowchain_gated_pre" : gate ? "rowchain_gated" : "rowchain";
    if (check_chain_first(who, g1) || check_gemm(who, g2, false, true, gate != nullptr)) return -1;
    const int f = g2->flags;
    if (gate) {
        RG_CHECK(f & DPVO_RG_GATE, "the second GEMM's flags must include DPVO_RG_GATE");
        RG_CHECK(!g2->gate16, "gate16 must be NULL (the gate is computed on chip)");
        RG_CHECK(gate->W && gate->bias && aligned(gate->W, 16) && aligned(gate->bias, 8),
                 "gate W (16-byte aligned) and bias (8-byte aligned) are required");
        RG_CHECK(gate->K == g1->K && gate->N == RG_BN, "gate W must be [384][K1] like W1");
    }
    const bool relu1 = g1->flags == DPVO_RG_RELU;   // (the compile-time activation)
    RG_CHECK(!pre || (f == (DPVO_RG_GATE | DPVO_RG_LN) && relu1), "a gated GATE | LN chain with a ReLU first GEMM");
    if (g1->M <= 0) return 0;
    if (ensure_num_cus()) return -1;
    const unsigned grid = persistent_grid(g1->M, R5_IDX_TILES);   // (a block's row sources fit its LDS table)
    dpvo_rowgemm_args a2 = *g2;
    a2.M = g1->M;
    a2.M_dev = g1->M_dev;
    int kf = f;   // the epilogue as the kernel takes it
    if (gate) {
        // the gated y goes through the RES epilogue (res16 none: the addend
        // loads compiled out, RG_NOADD): x + fp16(gate * y); PRELN forms the
        // residual base LayerNorm(pre rows) in the epilogue
        a2.gate16 = nullptr;
        a2.res16 = nullptr;
        kf = (f & ~DPVO_RG_GATE) | RG_RES | RG_NOADD;
    } else if (f == DPVO_RG_RES && !g2->res16) {   // (c1 / c2: no addend loads, + 0 in their place)
        kf |= RG_NOADD;
    }
    return chain_status(launch_rowchain5(kf, gate != nullptr, 0, relu1, *g1, a2, gate ? *gate : a2, pre, grid, as_stream(stream)),
                        who, f);
}
#undef RG_CHECK

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" int dpvo_rowgemm_pair(const dpvo_rowgemm_args* a, const dpvo_rowgemm_args* b, void* stream)
{
    if (check_rowgemm(a) || check_rowgemm(b)) return -1;
    DPVO_CHECK_ARG((a->flags == 0 && b->flags == 0) || (a->flags == DPVO_RG_WKB && b->flags == DPVO_RG_WKB),
                   "rowgemm_pair: plain GEMMs only (flags 0, or WKB on both)");
    DPVO_CHECK_ARG(a->A == b->A && a->lda == b->lda && a->a_idx == b->a_idx && a->a_rows == b->a_rows &&
                       a->K == b->K && a->M == b->M && a->M_dev == b->M_dev,
                   "rowgemm_pair: both GEMMs must share A, K and M");
    if (a->M <= 0) return 0;
    if (ensure_num_cus()) return -1;
    const unsigned grid = persistent_grid(a->M);
    const int nks = a->K / R5_BK;
    if (!(a->flags & DPVO_RG_WKB))
        launch_rowgemm3(0, true, *a, *b, grid, as_stream(stream));
    else if (nks >= P6_MINK && nks <= P6_MAXK)   // (the A tile fits LDS)
        launch_rowpair6(*a, *b, nullptr, grid, as_stream(stream));
    else
        launch_rowgemm5(0, true, *a, *b, grid, as_stream(stream));
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_rowgemm_pair_pre(const dpvo_rowgemm_args* a, const dpvo_rowgemm_args* b,
                                     const dpvo_rowadd_args* pre, void* stream)
{
    DPVO_CHECK_ARG(pre != nullptr && pre->a != nullptr && !pre->a_f16 && pre->lda >= 384 && pre->lda % 4 == 0 &&
                       ((uintptr_t)pre->a & 15) == 0,
                   "rowgemm_pair_pre: pre.a must be fp32 rows of >= 384 (16-byte aligned)");
    DPVO_CHECK_ARG(!pre->b16 || ((uintptr_t)pre->b16 & 15) == 0, "rowgemm_pair_pre: pre.b16 must be 16-byte aligned");
    DPVO_CHECK_ARG(!pre->ln_g && !pre->c16 && !pre->out32 && !pre->out16,
                   "rowgemm_pair_pre: pre is the row add only (no LayerNorm, second addend or outputs)");
    if (check_rowgemm(a) || check_rowgemm(b)) return -1;
    DPVO_CHECK_ARG(a->flags == DPVO_RG_WKB && b->flags == DPVO_RG_WKB, "rowgemm_pair_pre: k-blocked W on both");
    DPVO_CHECK_ARG(a->K == 384 && b->K == 384 && a->M == b->M && a->M == pre->M && a->M_dev == b->M_dev &&
                       !a->a_idx && !b->a_idx,
                   "rowgemm_pair_pre: K = 384, one M, no row gather (the rows are pre's)");
    if (a->M <= 0) return 0;
    if (ensure_num_cus()) return -1;
    // (a block's addend sources fit its LDS table)
    launch_rowpair6(*a, *b, pre, persistent_grid(a->M, R5_PRE_IDX_TILES), as_stream(stream));
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_rowgemm(const dpvo_rowgemm_args* a, void* stream)
{
    if (check_rowgemm(a)) return -1;
    const int f = a->flags;
    if (a->M <= 0) return 0;
    if (ensure_num_cus()) return -1;
    int rc;
    if (!(f & DPVO_RG_WKB)) {
        rc = launch_rowgemm3(f, false, *a, *a, persistent_grid(a->M), as_stream(stream));
    } else if (a->M_dev && (a->K == 384 || a->K == 896)) {
        // a device row count (the SoftAgg group GEMMs: G rows of an upper bound M,
        // G << M) takes the narrow 32-row tiles, two blocks per tile
        const unsigned grid_n = 2 * (unsigned)std::min<int64_t>((a->M + RN_BM - 1) / RN_BM, 2 * (int64_t)g_num_cus);
        rc = launch_rowgemm_narrow(f & ~DPVO_RG_WKB, *a, grid_n, as_stream(stream));
    } else {
        rc = launch_rowgemm5(f & ~DPVO_RG_WKB, false, *a, *a, persistent_grid(a->M), as_stream(stream));
    }
    if (rc) {
        set_error("dpvo_rowgemm: unsupported epilogue flag combination " + std::to_string(f));
        return -1;
    }
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_rowchain(const dpvo_rowgemm_args* g1, const dpvo_rowgemm_args* g2, void* stream)
{
    return rowchain_launch(g1, g2, nullptr, stream);
}

extern "C" int dpvo_rowchain3(const dpvo_rowgemm_args* g1, const dpvo_rowgemm_args* g2, const dpvo_rowgemm_args* g3,
                              void* stream)
{
    const char* who = "rowchain3";
    if (check_chain_first(who, g1) || check_gemm(who, g2, false, true) || check_gemm(who, g3, false, true)) return -1;
    DPVO_CHECK_ARG(g2->flags == (DPVO_RG_LN | DPVO_RG_LN_RELU) && ((uintptr_t)g2->ln_g & 15) == 0 &&
                       ((uintptr_t)g2->ln_b & 15) == 0,
                   "rowchain3: the middle epilogue must be LN | LN_RELU with 16-byte aligned LayerNorm parameters");
    DPVO_CHECK_ARG(g3->flags == (DPVO_RG_RES | DPVO_RG_LN), "rowchain3: the last epilogue must be RES | LN");
    if (g1->M <= 0) return 0;
    if (ensure_num_cus()) return -1;
    dpvo_rowgemm_args a3 = *g3;
    a3.M = g1->M;
    a3.M_dev = g1->M_dev;
    // (a block's row sources fit its LDS table)
    return chain_status(launch_rowchain5(g3->flags, false, g2->flags, g1->flags == DPVO_RG_RELU, *g1, a3, *g2, nullptr,
                                         persistent_grid(g1->M, R5_IDX_TILES), as_stream(stream)),
                        who, g3->flags);
}

extern "C" int dpvo_rowchain_gated(const dpvo_rowgemm_args* gate, const dpvo_rowgemm_args* g1,
                                   const dpvo_rowgemm_args* g2, void* stream)
{
    DPVO_CHECK_ARG(gate != nullptr, "rowchain_gated: gate args missing");
    return rowchain_launch(g1, g2, gate, stream);
}

extern "C" int dpvo_rowchain_gated_pre(const dpvo_rowgemm_args* gate, const dpvo_rowgemm_args* g1,
                                       const dpvo_rowgemm_args* g2, const dpvo_rowadd_args* pre, void* stream)
{
    DPVO_CHECK_ARG(gate != nullptr && pre != nullptr && g1 != nullptr && g2 != nullptr,
                   "rowchain_gated_pre: gate / pre args missing");
    DPVO_CHECK_ARG(pre->a && !pre->a_f16 && pre->lda >= RG_BN && pre->lda % 4 == 0 && ((uintptr_t)pre->a & 15) == 0,
                   "rowchain_gated_pre: pre.a must be fp32 rows of >= 384 (16-byte aligned)");
    DPVO_CHECK_ARG(pre->ln_g && pre->ln_b && ((uintptr_t)pre->ln_g & 15) == 0 && ((uintptr_t)pre->ln_b & 15) == 0,
                   "rowchain_gated_pre: pre.ln_g / ln_b (16-byte aligned) are required");
    DPVO_CHECK_ARG((!pre->b16 || ((uintptr_t)pre->b16 & 7) == 0) && (!pre->c16 || ((uintptr_t)pre->c16 & 7) == 0),
                   "rowchain_gated_pre: pre.b16 / c16 must be 8-byte aligned");
    DPVO_CHECK_ARG(!pre->c16 || pre->b16, "rowchain_gated_pre: c16 needs b16");
    DPVO_CHECK_ARG(pre->M == g1->M && !g1->M_dev, "rowchain_gated_pre: pre.M must be the chain's row count");
    DPVO_CHECK_ARG(!g2->res32 && !g2->res16, "rowchain_gated_pre: the residual comes from pre (res32 / res16 NULL)");
    dpvo_rowgemm_args b2 = *g2;
    b2.res32 = pre->a;   // (the shared residual check; the kernel reads pre)
    b2.ldr = pre->lda;
    return rowchain_launch(g1, &b2, gate, stream, pre);
}

extern "C" int dpvo_rowadd_ln(const dpvo_rowadd_args* a, void* stream)
{
    DPVO_CHECK_ARG(a != nullptr, "rowadd_ln: args missing");
    if (a->M <= 0) return 0;   // (empty tensors may carry null data pointers)
    DPVO_CHECK_ARG(a->a != nullptr, "rowadd_ln: input missing");
    DPVO_CHECK_ARG(a->lda >= RG_BN && a->lda % 4 == 0, "rowadd_ln: lda must be a multiple of 4 and >= 384");
    DPVO_CHECK_ARG((uintptr_t)a->a % (a->a_f16 ? 8 : 16) == 0, "rowadd_ln: input rows must be vector aligned");
    DPVO_CHECK_ARG(!a->b16 || (uintptr_t)a->b16 % 8 == 0, "rowadd_ln: b16 must be 8-byte aligned");
    DPVO_CHECK_ARG(!a->c16 || (uintptr_t)a->c16 % 8 == 0, "rowadd_ln: c16 must be 8-byte aligned");
    DPVO_CHECK_ARG(!a->c16 || a->b16, "rowadd_ln: c16 needs b16 (the second addend follows the first)");
    DPVO_CHECK_ARG(!a->ln_g || ((uintptr_t)a->ln_g % 16 == 0 && (uintptr_t)a->ln_b % 16 == 0),
                   "rowadd_ln: LayerNorm parameters must be 16-byte aligned");
    DPVO_CHECK_ARG((!a->out32 || (uintptr_t)a->out32 % 16 == 0) && (!a->out16 || (uintptr_t)a->out16 % 8 == 0),
                   "rowadd_ln: outputs must be vector aligned");
    DPVO_CHECK_ARG(a->out32 || a->out16, "rowadd_ln: no output");
    DPVO_CHECK_ARG(!a->ln_g == !a->ln_b, "rowadd_ln: LayerNorm needs both weight and bias");
    const unsigned grid = grid_for(a->M * 32, 256, 16384);
    if (a->a_f16)
        hipLaunchKernelGGL(rowadd_ln_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), *a);
    else
        hipLaunchKernelGGL(rowadd_ln_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), *a);
    DPVO_CHECK_LAUNCH();
    return 0;
}
