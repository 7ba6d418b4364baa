// pgo.hip -- Sim(3) pose-graph optimisation for loop closure, device-resident
// and in fp64 (the reference: dpvo/loop_closure/optim_utils.py:158-255 with
// pypose autograd Jacobians and an Eigen sparse solve, ba.cpp:174-234).
//
// State g [n][7]: additive tangent coordinates [tau, phi, sigma] of the
// world-to-camera Sim3 of every pose.  Edges: n-1 chain edges (i = k,
// j = k-1, C = T_{k-1} T_k^-1 of the input poses) then L loop edges
// (C = loop_poses[l]); residual r = Log(C Exp(g_i) Exp(g_j)^-1); cost = mean
// of the squares.
//
// Jacobians (exact, with respect to the additive coordinates):
//   J_i =  Jl^-1(r) Ad(C) Jl(g_i),   J_j = -Jl^-1(r) Ad(C Exp(g_i) Exp(g_j)^-1) Jl(g_j)
// Jl is the exact left Jacobian of Sim3, not liegroups.hpp's truncated
// series: series of ad(x / 2^m) where it converges fast, then m doublings
// Jl(2y) = (I + exp(ad y)) Jl(y) / 2, exp(ad 2y) = exp(ad y)^2; Jl^-1(r) by
// Gauss-Jordan with partial pivoting.
//
// Normal equations: A = J^T J + damping is never formed densely.  It has 7x7
// blocks at (k,k), (k,k-1) and one per loop edge; in natural order the
// Cholesky fill stays inside each row's envelope [first[k], k].  The blocks
// are gathered per pose / per block in a fixed edge order (no float atomics:
// bitwise repeatable) into a block skyline, factorised and solved by one
// workgroup that sweeps the columns (pgo_solve_kernel).
//
// The Levenberg-Marquardt loop is enqueued whole: accept / reject, the lm
// update and the stop rule run on the device, a done flag turns the remaining
// iterations into early exits, the host reads one packed status word.
#include "common.hpp"
#include "liegroups.hpp"
#include "pgo_math.hpp"

namespace dpvo {
namespace pgo {

enum { ST_OK = 0, ST_SELF_EDGE = 1, ST_BAD_INDEX = 2, ST_NOT_PD = 3 };

struct State {
    double lm, ep;
    double cost_cur, cost_new;
    int done, code, pivot, iters_run;
    int m;             // optimised poses: rows / columns of the system
    int nhi;           // rows whose envelope reaches past the chain neighbour
    long long total;   // blocks in the skyline
};

struct Layout {
    size_t state, g, cand, delta, bvec, cons, eI, eJ, res, Ji, Jj, sq, jlp, first, rowptr, hil, sky, bytes;
};

static inline size_t up(size_t x) { return (x + 255) & ~(size_t)255; }

static Layout layout(int64_t n, int64_t L)
{
    Layout o;
    const size_t E = (size_t)(n - 1 + L), N = (size_t)n, hi = (size_t)(L < n ? L : n);
    size_t p = 0;
    auto take = [&](size_t bytes) { size_t at = p; p = up(p + bytes); return at; };
    o.state = take(sizeof(State));
    o.g = take(N * 7 * 8);
    o.cand = take(N * 7 * 8);
    o.delta = take(N * 7 * 8);
    o.bvec = take(N * 7 * 8);
    o.cons = take(E * 8 * 8);
    o.eI = take(E * 4);
    o.eJ = take(E * 4);
    o.res = take(E * 7 * 8);
    o.Ji = take(E * 49 * 8);
    o.Jj = take(E * 49 * 8);
    o.sq = take(E * 8);
    o.jlp = take(N * 49 * 8);
    o.first = take(N * 4);
    o.rowptr = take((N + 1) * 8);
    o.hil = take((hi + 1) * 4);
    o.sky = take((2 * N + hi * N) * 49 * 8);
    o.bytes = p;
    return o;
}

// ---------------------------------------------------------------------------
// once per call: state g, edge constants, edge index lists, validation
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pgo_init_kernel(const double* __restrict__ poses, const double* __restrict__ g_in,
                                                      const double* __restrict__ loop_poses,
                                                      const int64_t* __restrict__ lii, const int64_t* __restrict__ ljj,
                                                      int n, int L, double lm, double ep, State* st,
                                                      double* __restrict__ g, double* __restrict__ cons,
                                                      int* __restrict__ eI, int* __restrict__ eJ,
                                                      int* __restrict__ first)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { st->lm = lm; st->ep = ep; }
    if (t < n) {
        const S3 Tk = se3_as_sim3_inv(poses + (size_t)t * 7);
        if (g_in) {
            for (int i = 0; i < 7; i++) g[(size_t)t * 7 + i] = g_in[(size_t)t * 7 + i];
        } else {
            double xi[7];
            Tk.Log(xi);
            for (int i = 0; i < 7; i++) g[(size_t)t * 7 + i] = xi[i];
        }
        first[t] = t > 0 ? t - 1 : 0;
        if (t > 0) {  // chain edge e = t - 1: (i, j) = (t, t - 1), C = T_{t-1} T_t^-1
            const S3 Tp = se3_as_sim3_inv(poses + (size_t)(t - 1) * 7);
            Tp.mul(Tk.inv()).store(cons + (size_t)(t - 1) * 8);
            eI[t - 1] = t;
            eJ[t - 1] = t - 1;
        }
    }
    if (t < L) {
        const int e = n - 1 + t;
        const int64_t a = lii[t], b = ljj[t];
        int ia = 0, ib = 1;
        if (a < 0 || a >= n || b < 0 || b >= n) {
            atomicMax(&st->code, (int)ST_BAD_INDEX);
            st->done = 1;
        } else if (a == b) {
            atomicCAS(&st->code, (int)ST_OK, (int)ST_SELF_EDGE);
            st->done = 1;
        } else {
            ia = (int)a;
            ib = (int)b;
        }
        eI[e] = ia;
        eJ[e] = ib;
        for (int i = 0; i < 8; i++) cons[(size_t)e * 8 + i] = loop_poses[(size_t)t * 8 + i];
    }
}

// once per call, one workgroup: the envelope (first column of every row),
// the skyline row pointers, the rows with a long envelope, the free count m
__global__ __launch_bounds__(256) void pgo_struct_kernel(int n, int L, int freen, const int* __restrict__ eI,
                                                         const int* __restrict__ eJ, int* __restrict__ first,
                                                         long long* __restrict__ rowptr, int* __restrict__ hil,
                                                         State* st)
{
    __shared__ long long part[256];
    __shared__ int smax;
    const int t = threadIdx.x;
    if (st->done) return;
    if (t == 0) smax = 0;
    __syncthreads();
    for (int l = t; l < L; l += 256) {
        const int a = eI[n - 1 + l], b = eJ[n - 1 + l];
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        atomicMin(&first[hi], lo);
        atomicMax(&smax, hi + 1);
    }
    __syncthreads();
    const int chunk = (n + 255) / 256, k0 = t * chunk, k1 = min(n, k0 + chunk);
    long long s = 0;
    for (int k = k0; k < k1; k++) s += k - first[k] + 1;
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int i = 0; i < 256; i++) { const long long v = part[i]; part[i] = run; run += v; }
        rowptr[n] = run;
        st->total = run;
        st->m = freen == -2 ? min(smax, n) : (freen < 0 ? n : min(freen, n));
        // rows with a long envelope, each once, in loop order
        int nhi = 0;
        for (int l = 0; l < L; l++) {
            const int a = eI[n - 1 + l], b = eJ[n - 1 + l];
            const int hi = a > b ? a : b;
            if (first[hi] >= hi - 1) continue;
            bool seen = false;
            for (int q = 0; q < nhi; q++) seen = seen || hil[q] == hi;
            if (!seen) hil[nhi++] = hi;
        }
        st->nhi = nhi;
    }
    __syncthreads();
    s = part[t];
    for (int k = k0; k < k1; k++) { rowptr[k] = s; s += k - first[k] + 1; }
}

// ---------------------------------------------------------------------------
// per pose: Jl(g_k)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pgo_pose_kernel(const double* __restrict__ g, int n, double* __restrict__ jlp,
                                                      const State* st)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (st->done || k >= n) return;
    double J[7][7];
    exact_left_jacobian(g + (size_t)k * 7, J);
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) jlp[(size_t)k * 49 + i * 7 + j] = J[i][j];
}

// per edge: residual, its squared norm and (JAC) both Jacobians
template <bool JAC>
__global__ __launch_bounds__(64) void pgo_edge_kernel(const double* __restrict__ g, const double* __restrict__ cons,
                                                      const int* __restrict__ eI, const int* __restrict__ eJ, int E,
                                                      const double* __restrict__ jlp, double* __restrict__ res,
                                                      double* __restrict__ Ji, double* __restrict__ Jj,
                                                      double* __restrict__ sq, const State* st)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (st->done || e >= E) return;
    const int i = eI[e], j = eJ[e];
    double r[7];
    const S3 C = S3::load(cons + (size_t)e * 8);
    const S3 M = edge_residual(C, g + (size_t)i * 7, g + (size_t)j * 7, r);
    double s = 0;
    for (int q = 0; q < 7; q++) s += r[q] * r[q];
    sq[e] = s;
    if (!JAC) return;
    for (int q = 0; q < 7; q++) res[(size_t)e * 7 + q] = r[q];
    edge_jacobians(C, M, r, jlp + (size_t)i * 49, jlp + (size_t)j * 49, Ji + (size_t)e * 49, Jj + (size_t)e * 49);
}

// sum of sq[0..E) / (7 E) in a fixed order; every thread returns it
__device__ static double block_cost(const double* __restrict__ sq, int E, double* sh)
{
    const int t = threadIdx.x;
    double s = 0;
    for (int e = t; e < E; e += 256) s += sq[e];
    sh[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double c = sh[0] / (7.0 * (double)E);
    __syncthreads();
    return c;
}

// cost of the current state -> state, history[itr] (and *cost_out)
__global__ __launch_bounds__(256) void pgo_cost_kernel(const double* __restrict__ sq, int E, int itr,
                                                       double* __restrict__ hist, double* __restrict__ cost_out,
                                                       State* st)
{
    __shared__ double sh[256];
    if (st->done) return;
    const double c = block_cost(sq, E, sh);
    if (threadIdx.x == 0) {
        st->cost_cur = c;
        if (hist) hist[itr] = c;
        if (cost_out) *cost_out = c;
    }
}

// ---------------------------------------------------------------------------
// block-sparse normal equations
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pgo_zero_kernel(double* __restrict__ sky, const State* st)
{
    if (st->done) return;
    const long long total = st->total * 49;
    for (long long x = blockIdx.x * 256ll + threadIdx.x; x < total; x += (long long)gridDim.x * 256) sky[x] = 0.0;
}

__device__ __forceinline__ size_t blk(const long long* rowptr, const int* first, int k, int c)
{
    return (size_t)(rowptr[k] + (c - first[k])) * 49;
}

// task < n: diagonal block and right-hand side of pose `task`;
// task >= n: the off-diagonal block of edge task - n.  Every sum runs over
// the edges in their list order.
__global__ __launch_bounds__(64) void pgo_assemble_kernel(const double* __restrict__ res, const double* __restrict__ Ji,
                                                          const double* __restrict__ Jj, const int* __restrict__ eI,
                                                          const int* __restrict__ eJ, int n, int L,
                                                          const int* __restrict__ first,
                                                          const long long* __restrict__ rowptr,
                                                          double* __restrict__ sky, double* __restrict__ bvec,
                                                          const State* st)
{
    if (st->done) return;
    const int task = blockIdx.x, t = threadIdx.x, m = st->m, E = n - 1 + L;
    if (task < n) {
        const int k = task;
        if (k >= m || t >= 56) return;
        const bool isb = t >= 49;
        const int a = isb ? t - 49 : t / 7, b = isb ? 0 : t % 7;
        double acc = 0;
        auto add = [&](const double* J, int e) {
            const double* Je = J + (size_t)e * 49;
            if (isb) {
                for (int q = 0; q < 7; q++) acc -= Je[q * 7 + a] * res[(size_t)e * 7 + q];
            } else {
                for (int q = 0; q < 7; q++) acc += Je[q * 7 + a] * Je[q * 7 + b];
            }
        };
        if (k >= 1) add(Ji, k - 1);
        if (k <= n - 2) add(Jj, k);
        for (int e = n - 1; e < E; e++) {
            if (eI[e] == k) add(Ji, e);
            else if (eJ[e] == k) add(Jj, e);
        }
        if (isb) {
            bvec[(size_t)k * 7 + a] = acc;
        } else {
            if (a == b) acc = acc + acc * st->lm + st->ep;
            sky[blk(rowptr, first, k, k) + a * 7 + b] = acc;
        }
        return;
    }
    const int e = task - n;
    if (t >= 49) return;
    const int hi = max(eI[e], eJ[e]), lo = min(eI[e], eJ[e]);
    if (hi >= m) return;
    if (e >= n - 1) {  // a loop edge owns its block unless the chain or an earlier loop has the same pair
        if (hi - lo == 1) return;
        for (int q = n - 1; q < e; q++)
            if (max(eI[q], eJ[q]) == hi && min(eI[q], eJ[q]) == lo) return;
    }
    const int a = t / 7, b = t % 7;
    double acc = 0;
    for (int q = e; q < E; q = (q < n - 1 ? n - 1 : q + 1)) {
        if (max(eI[q], eJ[q]) != hi || min(eI[q], eJ[q]) != lo) continue;
        const double* Jhi = (eI[q] == hi ? Ji : Jj) + (size_t)q * 49;
        const double* Jlo = (eI[q] == hi ? Jj : Ji) + (size_t)q * 49;
        for (int r = 0; r < 7; r++) acc += Jhi[r * 7 + a] * Jlo[r * 7 + b];
    }
    sky[blk(rowptr, first, hi, lo) + a * 7 + b] = acc;
}

// ---------------------------------------------------------------------------
// block skyline Cholesky, forward and backward substitution, candidate state.
// One workgroup sweeps the columns; at column j the rows whose envelope
// covers j (the chain neighbour j + 1 and the active loop rows) are worked on
// side by side, one lane per block entry.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pgo_solve_kernel(int n, const int* __restrict__ first,
                                                        const long long* __restrict__ rowptr,
                                                        const int* __restrict__ hil, double* __restrict__ sky,
                                                        double* __restrict__ bvec, const double* __restrict__ g,
                                                        double* __restrict__ delta, double* __restrict__ cand,
                                                        State* st)
{
    __shared__ double sL[49];
    __shared__ double sv[7];
    __shared__ double spart[32][8];
    __shared__ int sfail;
    if (st->done) return;
    const int t = threadIdx.x, m = st->m, nhi = st->nhi;
    if (t == 0) sfail = 0;
    __syncthreads();

    // ---- factorisation: A = L L^T, in place
    for (int j = 0; j < m; j++) {
        const int fj = first[j];
        const int ntask = (2 + nhi) * 49;
        // S_k = A_kj - sum_p L_kp L_jp^T for the diagonal row and every active row
        for (int x = t; x < ntask; x += 256) {
            const int slot = x / 49, ab = x - slot * 49, a = ab / 7, b = ab - a * 7;
            int k;
            if (slot == 0) k = j;
            else if (slot == 1) k = j + 1;
            else {
                k = hil[slot - 2];
                if (k == j + 1 || k <= j || first[k] > j) continue;
            }
            if (k >= m) continue;
            const int p0 = max(first[k], fj);
            const size_t out = blk(rowptr, first, k, j) + ab;
            double s = sky[out];
            const double* Lk = sky + blk(rowptr, first, k, p0) + a * 7;
            const double* Lj = sky + blk(rowptr, first, j, p0) + b * 7;
            for (int p = p0; p < j; p++, Lk += 49, Lj += 49)
                for (int q = 0; q < 7; q++) s -= Lk[q] * Lj[q];
            sky[out] = s;
        }
        __syncthreads();
        if (t == 0) {  // 7x7 Cholesky of the diagonal block
            double D[7][7];
            const double* d = sky + blk(rowptr, first, j, j);
            for (int a = 0; a < 7; a++)
                for (int b = 0; b < 7; b++) D[a][b] = d[a * 7 + b];
            for (int c = 0; c < 7; c++) {
                double v = D[c][c];
                for (int q = 0; q < c; q++) v -= D[c][q] * D[c][q];
                if (!(v > 0.0) && !sfail) {  // not positive definite: report the leading minor, no clamp
                    sfail = 1;
                    st->code = ST_NOT_PD;
                    st->pivot = j * 7 + c + 1;
                }
                const double l = sqrt(v), il = 1.0 / l;
                D[c][c] = l;
                for (int r = c + 1; r < 7; r++) {
                    double w = D[r][c];
                    for (int q = 0; q < c; q++) w -= D[r][q] * D[c][q];
                    D[r][c] = w * il;
                }
            }
            double* o = sky + blk(rowptr, first, j, j);
            for (int a = 0; a < 7; a++)
                for (int b = 0; b < 7; b++) {
                    const double v = b <= a ? D[a][b] : 0.0;
                    sL[a * 7 + b] = v;
                    o[a * 7 + b] = v;
                }
        }
        __syncthreads();
        // L_kj = S_k L_jj^-T, one lane per block row
        for (int x = t; x < (1 + nhi) * 7; x += 256) {
            const int slot = x / 7 + 1, a = x - (slot - 1) * 7;
            int k;
            if (slot == 1) k = j + 1;
            else {
                k = hil[slot - 2];
                if (k == j + 1 || k <= j || first[k] > j) continue;
            }
            if (k >= m) continue;
            double* row = sky + blk(rowptr, first, k, j) + a * 7;
            double xr[7];
            for (int b = 0; b < 7; b++) {
                double v = row[b];
                for (int q = 0; q < b; q++) v -= xr[q] * sL[b * 7 + q];
                xr[b] = v / sL[b * 7 + b];
            }
            for (int b = 0; b < 7; b++) row[b] = xr[b];
        }
        __syncthreads();
    }

    // ---- forward substitution L y = b (y over b)
    for (int k = 0; k < m; k++) {
        const int f = first[k], w = k - f;
        {
            const int a = t & 7, q = t >> 3;
            double acc = 0;
            if (a < 7)
                for (int c = f + q; c < k; c += 32) {
                    const double* Lb = sky + blk(rowptr, first, k, c) + a * 7;
                    const double* y = bvec + (size_t)c * 7;
                    for (int b = 0; b < 7; b++) acc += Lb[b] * y[b];
                }
            spart[q][a] = acc;
        }
        __syncthreads();
        if (t == 0) {
            const double* Ld = sky + blk(rowptr, first, k, k);
            const int nq = w < 32 ? w : 32;
            double y[7];
            for (int a = 0; a < 7; a++) {
                double v = bvec[(size_t)k * 7 + a];
                for (int q = 0; q < nq; q++) v -= spart[q][a];
                for (int b = 0; b < a; b++) v -= Ld[a * 7 + b] * y[b];
                y[a] = v / Ld[a * 7 + a];
            }
            for (int a = 0; a < 7; a++) bvec[(size_t)k * 7 + a] = y[a];
        }
        __syncthreads();
    }

    // ---- backward substitution L^T x = y (x over y)
    for (int k = m - 1; k >= 0; k--) {
        if (t == 0) {
            const double* Ld = sky + blk(rowptr, first, k, k);
            double x[7];
            for (int a = 6; a >= 0; a--) {
                double v = bvec[(size_t)k * 7 + a];
                for (int b = a + 1; b < 7; b++) v -= Ld[b * 7 + a] * x[b];
                x[a] = v / Ld[a * 7 + a];
            }
            for (int a = 0; a < 7; a++) { bvec[(size_t)k * 7 + a] = x[a]; sv[a] = x[a]; }
        }
        __syncthreads();
        const int f = first[k], w = k - f;
        for (int x = t; x < w * 7; x += 256) {  // y_c -= L_kc^T x_k
            const int c = f + x / 7, b = x % 7;
            const double* Lb = sky + blk(rowptr, first, k, c);
            double v = 0;
            for (int a = 0; a < 7; a++) v += Lb[a * 7 + b] * sv[a];
            bvec[(size_t)c * 7 + b] -= v;
        }
        __syncthreads();
    }

    for (int x = t; x < n * 7; x += 256) {
        const double d = x < m * 7 ? bvec[x] : 0.0;
        delta[x] = d;
        cand[x] = g[x] + d;
    }
    if (t == 0 && sfail) st->done = 1;
}

// accept / reject, lm update, stop rule (optim_utils.py:245-253)
__global__ __launch_bounds__(256) void pgo_update_kernel(const double* __restrict__ sq, int E, int n, int itr,
                                                         const double* __restrict__ hist, double* __restrict__ g,
                                                         const double* __restrict__ cand, State* st)
{
    __shared__ double sh[256];
    if (st->done) return;
    const double cnew = block_cost(sq, E, sh);
    const double ccur = st->cost_cur;
    const bool accept = cnew < ccur;
    if (accept)
        for (int x = threadIdx.x; x < n * 7; x += 256) g[x] = cand[x];
    if (threadIdx.x == 0) {
        st->cost_new = cnew;
        st->lm = accept ? st->lm * 0.5 : st->lm * 2.0;
        st->iters_run = itr + 1;
        if (ccur < 1e-5 && itr >= 4 && hist[itr - 4] / ccur < 1.5) st->done = 1;
    }
}

// Exp(g)^-1 [n][8], NaN in the unused history slots, the packed status word
__global__ __launch_bounds__(64) void pgo_final_kernel(const double* __restrict__ g, int n, int iters,
                                                       double* __restrict__ out, double* __restrict__ hist,
                                                       int* __restrict__ status, const State* st)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && out) S3::Exp(g + (size_t)k * 7).inv().store(out + (size_t)k * 8);
    if (k < iters && hist && k >= st->iters_run) hist[k] = __longlong_as_double(0x7ff8000000000000ll);
    if (k == 0 && status) *status = st->code | (st->iters_run << 4) | (st->pivot << 12);
}

struct Ws {
    State* st;
    double *g, *cand, *delta, *bvec, *cons, *res, *Ji, *Jj, *sq, *jlp, *sky;
    int *eI, *eJ, *first, *hil;
    long long* rowptr;
};

static Ws carve(void* base, const Layout& o)
{
    char* p = (char*)base;
    Ws w;
    w.st = (State*)(p + o.state);
    w.g = (double*)(p + o.g); w.cand = (double*)(p + o.cand); w.delta = (double*)(p + o.delta);
    w.bvec = (double*)(p + o.bvec); w.cons = (double*)(p + o.cons); w.res = (double*)(p + o.res);
    w.Ji = (double*)(p + o.Ji); w.Jj = (double*)(p + o.Jj); w.sq = (double*)(p + o.sq);
    w.jlp = (double*)(p + o.jlp); w.sky = (double*)(p + o.sky);
    w.eI = (int*)(p + o.eI); w.eJ = (int*)(p + o.eJ); w.first = (int*)(p + o.first); w.hil = (int*)(p + o.hil);
    w.rowptr = (long long*)(p + o.rowptr);
    return w;
}

static inline unsigned g64(int64_t n) { return grid_for(n, 64); }

}  // namespace pgo
}  // namespace dpvo

using namespace dpvo;
using namespace dpvo::pgo;

#define PGO_CHECK_COMMON()                                                                          \
    DPVO_CHECK_ARG(n >= 2 && n <= 65536 && L >= 0 && L <= 65536, "need 2 <= n <= 65536, 0 <= L <= 65536"); \
    DPVO_CHECK_ARG(poses && (L == 0 || (loop_poses && loop_ii && loop_jj)), "poses / loop arrays missing"); \
    DPVO_CHECK_ARG(workspace && status, "workspace / status missing");                               \
    const Layout lay = layout(n, L);                                                                 \
    DPVO_CHECK_ARG(workspace_bytes >= lay.bytes, "workspace too small (dpvo_pgo_workspace_bytes)");   \
    DPVO_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");              \
    const Ws w = carve(workspace, lay);                                                              \
    hipStream_t s = as_stream(stream);                                                               \
    const int E = (int)(n - 1 + L);                                                                  \
    DPVO_CHECK_HIP(hipMemsetAsync(w.st, 0, sizeof(State), s))

extern "C" size_t dpvo_pgo_workspace_bytes(int64_t n, int64_t L)
{
    if (n < 2 || L < 0 || n > 65536 || L > 65536) return 0;
    return layout(n, L).bytes;
}

// launches of one linearisation: Jl per pose, residuals and Jacobians, cost
static void enqueue_linearise(const Ws& w, int n, int E, double* res, double* Ji, double* Jj, int itr, double* hist,
                              double* cost_out, hipStream_t s)
{
    hipLaunchKernelGGL(pgo_pose_kernel, dim3(g64(n)), dim3(64), 0, s, w.g, n, w.jlp, w.st);
    hipLaunchKernelGGL(pgo_edge_kernel<true>, dim3(g64(E)), dim3(64), 0, s, w.g, w.cons, w.eI, w.eJ, E, w.jlp, res, Ji,
                       Jj, w.sq, w.st);
    hipLaunchKernelGGL(pgo_cost_kernel, dim3(1), dim3(256), 0, s, w.sq, E, itr, hist, cost_out, w.st);
}

// launches of one damped solve from w.res / w.Ji / w.Jj: -> w.delta, w.cand
static void enqueue_solve(const Ws& w, int n, int L, hipStream_t s)
{
    hipLaunchKernelGGL(pgo_zero_kernel, dim3(256), dim3(256), 0, s, w.sky, w.st);
    hipLaunchKernelGGL(pgo_assemble_kernel, dim3((unsigned)(n + n - 1 + L)), dim3(64), 0, s, w.res, w.Ji, w.Jj, w.eI,
                       w.eJ, n, L, w.first, w.rowptr, w.sky, w.bvec, w.st);
    hipLaunchKernelGGL(pgo_solve_kernel, dim3(1), dim3(256), 0, s, n, w.first, w.rowptr, w.hil, w.sky, w.bvec, w.g,
                       w.delta, w.cand, w.st);
}

extern "C" int dpvo_pgo_residual(const double* g, const double* poses, const double* loop_poses,
                                 const int64_t* loop_ii, const int64_t* loop_jj, int64_t n, int64_t L, double* res,
                                 double* Ji, double* Jj, double* cost, void* workspace, size_t workspace_bytes,
                                 int* status, void* stream)
{
    PGO_CHECK_COMMON();
    DPVO_CHECK_ARG(res && Ji && Jj, "outputs missing");
    hipLaunchKernelGGL(pgo_init_kernel, dim3(g64(n > L ? n : L)), dim3(64), 0, s, poses, g, loop_poses, loop_ii,
                       loop_jj, (int)n, (int)L, 0.0, 0.0, w.st, w.g, w.cons, w.eI, w.eJ, w.first);
    enqueue_linearise(w, (int)n, E, res, Ji, Jj, 0, nullptr, cost, s);
    hipLaunchKernelGGL(pgo_final_kernel, dim3(1), dim3(64), 0, s, w.g, 0, 0, (double*)nullptr, (double*)nullptr, status,
                       w.st);
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_pgo_step(const double* g, const double* poses, const double* loop_poses, const int64_t* loop_ii,
                             const int64_t* loop_jj, int64_t n, int64_t L, double ep, double lm, int64_t freen,
                             double* delta, void* workspace, size_t workspace_bytes, int* status, void* stream)
{
    PGO_CHECK_COMMON();
    DPVO_CHECK_ARG(delta, "delta missing");
    DPVO_CHECK_ARG(freen >= -1, "freen must be >= -1");
    hipLaunchKernelGGL(pgo_init_kernel, dim3(g64(n > L ? n : L)), dim3(64), 0, s, poses, g, loop_poses, loop_ii,
                       loop_jj, (int)n, (int)L, lm, ep, w.st, w.g, w.cons, w.eI, w.eJ, w.first);
    hipLaunchKernelGGL(pgo_struct_kernel, dim3(1), dim3(256), 0, s, (int)n, (int)L,
                       (int)(freen > n ? n : freen), w.eI, w.eJ, w.first, w.rowptr, w.hil, w.st);
    enqueue_linearise(w, (int)n, E, w.res, w.Ji, w.Jj, 0, nullptr, nullptr, s);
    DPVO_CHECK_HIP(hipMemsetAsync(w.delta, 0, (size_t)n * 7 * 8, s));   // a failed call returns zeros
    enqueue_solve(w, (int)n, (int)L, s);
    hipLaunchKernelGGL(pgo_final_kernel, dim3(1), dim3(64), 0, s, w.g, 0, 0, (double*)nullptr, (double*)nullptr, status,
                       w.st);
    DPVO_CHECK_HIP(hipMemcpyAsync(delta, w.delta, (size_t)n * 7 * 8, hipMemcpyDeviceToDevice, s));
    DPVO_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpvo_pgo(const double* poses, const double* loop_poses, const int64_t* loop_ii, const int64_t* loop_jj,
                        int64_t n, int64_t L, int iters, double ep, double lmbda, int64_t freen, double* out_sim3,
                        double* cost_history, void* workspace, size_t workspace_bytes, int* status, void* stream)
{
    PGO_CHECK_COMMON();
    DPVO_CHECK_ARG(out_sim3 && (iters == 0 || cost_history), "outputs missing");
    DPVO_CHECK_ARG(iters >= 0 && iters <= 255, "0 <= iters <= 255");
    DPVO_CHECK_ARG(freen >= -2, "freen: >= 0, -1 (all poses) or -2 (up to the last loop pose)");
    hipLaunchKernelGGL(pgo_init_kernel, dim3(g64(n > L ? n : L)), dim3(64), 0, s, poses, (const double*)nullptr,
                       loop_poses, loop_ii, loop_jj, (int)n, (int)L, lmbda, ep, w.st, w.g, w.cons, w.eI, w.eJ, w.first);
    hipLaunchKernelGGL(pgo_struct_kernel, dim3(1), dim3(256), 0, s, (int)n, (int)L,
                       (int)(freen > n ? n : freen), w.eI, w.eJ, w.first, w.rowptr, w.hil, w.st);
    for (int itr = 0; itr < iters; itr++) {
        enqueue_linearise(w, (int)n, E, w.res, w.Ji, w.Jj, itr, cost_history, nullptr, s);
        enqueue_solve(w, (int)n, (int)L, s);
        hipLaunchKernelGGL(pgo_edge_kernel<false>, dim3(g64(E)), dim3(64), 0, s, w.cand, w.cons, w.eI, w.eJ, E, w.jlp,
                           w.res, w.Ji, w.Jj, w.sq, w.st);
        hipLaunchKernelGGL(pgo_update_kernel, dim3(1), dim3(256), 0, s, w.sq, E, (int)n, itr, cost_history, w.g, w.cand,
                           w.st);
    }
    hipLaunchKernelGGL(pgo_final_kernel, dim3(g64(n > iters ? n : iters)), dim3(64), 0, s, w.g, (int)n, iters, out_sim3,
                       cost_history, status, w.st);
    DPVO_CHECK_LAUNCH();
    return 0;
}
