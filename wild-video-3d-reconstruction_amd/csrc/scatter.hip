// scatter.hip -- torch_scatter 2.1.2 reductions (scatter_sum / mean / max /
// softmax) over the CSR of dpvo_group_by(index) (gfx950): the reference's
// SoftAgg (blocks.py:42-43), its Python BA (ba.py:40-56) and loop closure
// (long_term.py:134) call them.
// src is viewed as [outer][E][inner] (the scatter dim in the middle) and the
// index is 1-D along it.  One thread per (group, outer x inner column) walks
// the group's members in ascending edge order: deterministic, no atomics.
#include "updateop.hpp"

namespace dpvo {
namespace {

enum { SC_SUM = 0, SC_MEAN = 1, SC_MAX = 2, SC_SOFTMAX = 3 };

template <typename T> struct ScAcc { typedef float type; };
template <> struct ScAcc<double> { typedef double type; };

template <typename T, int OP>
__global__ __launch_bounds__(256) void scatter_csr_kernel(const T* __restrict__ src, int64_t outer, int64_t E,
                                                          int64_t inner, const int64_t* __restrict__ index,
                                                          const int* __restrict__ offs, const int* __restrict__ perm,
                                                          const int64_t* __restrict__ groups, int64_t max_groups,
                                                          float eps, T* __restrict__ out, int64_t out_rows,
                                                          int64_t* __restrict__ arg)
{
    typedef typename ScAcc<T>::type A;
    const int64_t G = min(*groups, max_groups);
    const int64_t cols = outer * inner;
    const int64_t cblocks = (cols + 255) / 256;
    for (int64_t w = blockIdx.x; w < G * cblocks; w += gridDim.x) {
        const int64_t g = w / cblocks;
        const int64_t col = (w % cblocks) * 256 + threadIdx.x;
        if (col >= cols) continue;
        const int64_t o = col / inner, c = col % inner;
        const int b = offs[g], s = offs[g + 1] - b;
        const T* sp = src + o * E * inner + c;
        if (OP == SC_SUM || OP == SC_MEAN) {
            A a = 0;
            for (int i = 0; i < s; i++) a += (A)sp[(int64_t)perm[b + i] * inner];
            const int64_t key = index[perm[b]];
            if (key < 0 || key >= out_rows) continue;
            T* op = out + (o * out_rows + key) * inner + c;
            A v = (A)*op + a;
            if (OP == SC_MEAN) v = v / (A)s;
            *op = (T)v;
        } else if (OP == SC_MAX) {
            A m = 0;
            int64_t am = -1;
            for (int i = 0; i < s; i++) {
                const int e = perm[b + i];
                const A v = (A)sp[(int64_t)e * inner];
                if (am < 0 || v > m) {
                    m = v;
                    am = e;
                }
            }
            const int64_t key = index[perm[b]];
            if (key < 0 || key >= out_rows) continue;
            out[(o * out_rows + key) * inner + c] = (T)m;
            arg[(o * out_rows + key) * inner + c] = am;
        } else {   // SOFTMAX: recentre on the group max, exp, / (sum + eps)   (composite/softmax.py)
            A m = 0;
            for (int i = 0; i < s; i++) {
                const A v = (A)sp[(int64_t)perm[b + i] * inner];
                m = (i == 0 || v > m) ? v : m;
            }
            A den = 0;
            for (int i = 0; i < s; i++) den += exp((A)sp[(int64_t)perm[b + i] * inner] - m);
            den += (A)eps;
            T* op = out + o * E * inner + c;
            for (int i = 0; i < s; i++) {
                const int64_t e = perm[b + i];
                op[e * inner] = (T)(exp((A)sp[e * inner] - m) / den);
            }
        }
    }
}

template <typename T>
void scatter_dispatch(int op, const T* src, int64_t outer, int64_t E, int64_t inner, const int64_t* index,
                      const int* offs, const int* perm, const int64_t* groups, int64_t max_groups, float eps, T* out,
                      int64_t out_rows, int64_t* arg, hipStream_t st)
{
    const int64_t cblocks = (outer * inner + 255) / 256;
    const unsigned grid = grid_for(max_groups * cblocks, 1, 16384);
#define SC_LAUNCH(OPV)                                                                                          \
    hipLaunchKernelGGL((scatter_csr_kernel<T, OPV>), dim3(grid), dim3(256), 0, st, src, outer, E, inner, index, \
                       offs, perm, groups, max_groups, eps, out, out_rows, arg)
    switch (op) {
    case SC_SUM: SC_LAUNCH(SC_SUM); break;
    case SC_MEAN: SC_LAUNCH(SC_MEAN); break;
    case SC_MAX: SC_LAUNCH(SC_MAX); break;
    case SC_SOFTMAX: SC_LAUNCH(SC_SOFTMAX); break;   // (the entry point has checked op)
    }
#undef SC_LAUNCH
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

extern "C" int dpvo_scatter_csr(int op, int dtype, const void* src, int64_t outer, int64_t E, int64_t inner,
                                const int64_t* index, const int* offs, const int* perm, const int64_t* groups,
                                int64_t max_groups, float eps, void* out, int64_t out_rows, int64_t* argmax,
                                void* stream)
{
    DPVO_CHECK_ARG(op >= SC_SUM && op <= SC_SOFTMAX, "op must be 0 (sum), 1 (mean), 2 (max) or 3 (softmax)");
    DPVO_CHECK_ARG(outer >= 0 && E >= 0 && inner >= 0 && out_rows >= 0, "bad sizes");
    DPVO_CHECK_ARG(E < (int64_t(1) << 31), "at most 2^31 - 1 elements along the scatter dim");
    DPVO_CHECK_ARG(op != SC_MAX || argmax != nullptr, "scatter max needs the argmax output");
    if (E == 0 || outer == 0 || inner == 0 || max_groups <= 0) return 0;
    DPVO_CHECK_ARG(src && index && offs && perm && groups && out, "null operand");
    hipStream_t st = as_stream(stream);
    const bool known = dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        scatter_dispatch(op, (const T*)src, outer, E, inner, index, offs, perm, groups, max_groups, eps, (T*)out,
                         out_rows, argmax, st);
    });
    DPVO_CHECK_ARG(known, "unsupported dtype");
    DPVO_CHECK_LAUNCH();
    return 0;
}
