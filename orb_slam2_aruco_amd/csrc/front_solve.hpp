// front_solve.hpp -- what a workgroup does with one front of an elimination tree (front_plan.hpp), shared by essential_graph.hip
// (7 rows a vertex) and global_ba.hip (6): the children's Schur complements added to it, the partial Cholesky factorisation that
// leaves the boundary's own complement, and the substitution back once the ancestors' unknowns are known.  A front kernel gathers
// its own blocks, calls front_merge_children, runs front_partial_llt on the LDS copy or in place (that branch stays in the kernel's
// own text: DESIGN.md 4k), and substitutes at once when it has no boundary; front_back is the body of a back kernel.  LM_THREADS
// threads.
#pragma once
#include "front_plan.hpp"
#include "lm_dense.hpp"

namespace orbfe {
namespace {

// The first k columns of M = L L^T in place (lower triangle, right-looking, no pivoting) with the trailing update carried over all n
// rows, which leaves the Schur complement of the last n - k; r, the right-hand side, is one more column: r[0, k) becomes L11^-1 r and
// r[k, n) what the parent adds.  PACKED: M is the lower triangle row after row (the LDS copy), else rows of n.  Returns whether every
// pivot was positive.
template <bool PACKED> __device__ __forceinline__ bool front_partial_llt(double* M, int n, int k, double* r, int* fail_s)
{
    const int tid = threadIdx.x;
    auto row = [n](int i) { return PACKED ? (size_t)i * (i + 1) / 2 : (size_t)i * n; };
    for (int kk = 0; kk < k; kk++) {
        if (tid == 0) {
            const double d = M[row(kk) + kk];
            if (!(d > 0) || !isfinite(d)) *fail_s = 1;
            else M[row(kk) + kk] = sqrt(d);
        }
        __syncthreads();
        if (*fail_s) return false;
        const double lkk = M[row(kk) + kk];
        for (int i = kk + 1 + tid; i < n; i += LM_THREADS) M[row(i) + kk] /= lkk;
        if (tid == 0) r[kk] /= lkk;
        __syncthreads();
        const double yk = r[kk];
        for (int i = kk + 1 + (tid >> 4); i < n; i += LM_THREADS / 16) {
            const double lik = M[row(i) + kk];
            for (int j = kk + 1 + (tid & 15); j <= i; j += 16) M[row(i) + j] -= lik * M[row(j) + kk];
            if ((tid & 15) == 0) r[i] -= lik * yk;
        }
        __syncthreads();
    }
    return true;
}

// x_own of a factored front of R rows a vertex: L11^T x = y - L21^T x_boundary, the boundary's x being the ancestors'.  F holds L
// (rows of n), r holds y in [0, k), w is the front's work vector; vtx the front's (own, boundary) vertices, xt the solution, R a vertex.
template <int R> __device__ __forceinline__ void front_substitute_back(const FrontNode& nd, const int32_t* vtx, double* xt, const double* F, const double* r,
                                                                       double* w)
{
    const int tid = threadIdx.x, n = R * (nd.nown + nd.nb), k = R * nd.nown;
    for (int i = tid; i < k; i += LM_THREADS) {
        double s = r[i];
        for (int j = k; j < n; j++) s -= F[(size_t)j * n + i] * xt[(size_t)vtx[j / R] * R + j % R];
        w[i] = s;
    }
    __syncthreads();
    for (int kk = k - 1; kk >= 0; kk--) {
        if (tid == 0) w[kk] /= F[(size_t)kk * n + kk];
        __syncthreads();
        const double xk = w[kk];
        for (int i = tid; i < kk; i += LM_THREADS) w[i] -= F[(size_t)kk * n + i] * xk;
        __syncthreads();
    }
    for (int i = tid; i < k; i += LM_THREADS) xt[(size_t)vtx[i / R] * R + i % R] = w[i];
}

// The children's Schur complements added to front F (rows of n = R (nown + nb), lower triangle) and to its right-hand side r, the
// left child then the right one: the child's boundary vertex b is the front's vertex map[b], and where the map turns two of them
// round the entry goes to the transposed place.  Every entry has one thread; a barrier behind each child.
template <int R> __device__ __forceinline__ void front_merge_children(const FrontNode& nd, const FrontNode* nodes, const int32_t* cmap, const double* fronts,
                                                                      double* F, double* r)
{
    const int tid = threadIdx.x, n = R * (nd.nown + nd.nb);
    for (int ch = 0; ch < 2; ch++) {
        if (nd.child[ch] < 0) continue;
        const FrontNode cn = nodes[nd.child[ch]];
        const int m = R * (cn.nown + cn.nb), ck = R * cn.nown, cb = R * cn.nb;
        const double* G = fronts + cn.front;
        const double* gr = G + (size_t)m * m;
        const int32_t* map = cmap + nd.cmap[ch];
        for (int idx = tid; idx < cb * cb; idx += LM_THREADS) {
            const int bi = idx / cb, bj = idx % cb;
            if (bj > bi) continue;
            int row = R * map[bi / R] + bi % R, col = R * map[bj / R] + bj % R;
            if (row < col) {
                const int t = row; row = col; col = t;
            }
            F[(size_t)row * n + col] += G[(size_t)(ck + bi) * m + ck + bj];
        }
        for (int bi = tid; bi < cb; bi += LM_THREADS) r[R * map[bi / R] + bi % R] += gr[ck + bi];
        __syncthreads();
    }
}

// A back kernel: the unknowns of a front that has a boundary, once its ancestors' are known
template <int R> __device__ __forceinline__ void front_back(const FrontNode& nd, double* fronts, const int32_t* node_vtx, double* xt)
{
    const int n = R * (nd.nown + nd.nb);
    if (nd.nb == 0 || nd.nown == 0) return;
    double* F = fronts + nd.front;
    front_substitute_back<R>(nd, node_vtx + nd.vtx, xt, F, F + (size_t)n * n, F + (size_t)n * n + n);
}

} // namespace
} // namespace orbfe
