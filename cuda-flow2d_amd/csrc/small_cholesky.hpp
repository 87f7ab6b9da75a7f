// The K x K Cholesky factorisation and solve of flow2d_subset_refine_2d (K = 6) and flow2d_node_strain_2d (K = 3, 6), in IEEE
// double, one copy: the pivot test and the order of every sum are part of those definitions (flow2d_c_abi.h).  Every loop is
// unrolled and no array is indexed by a run-time value: the matrices live in registers.
//
// subset_refine.hip takes solve<6> from here but keeps the factorisation written out in refine_node: with factor<6> each of
// its kernels lost one v_mov_b32 (the flat state's constant, set once instead of per pivot test) and changed nothing else,
// and timed against the parent at 4096 x 4096, R = 15, it was 1.2 % slower in every one of five rounds (+228 us against a
// parent spread of 37; profiles/node_grid_headers/README.md).  The local form compiles to the parent's arithmetic.
#pragma once

#include <hip/hip_runtime.h>

// Cholesky M = L L^T and the two solves of the header; false where a pivot test fails.  M's lower triangle comes in L.
template <int K>
__device__ __forceinline__ bool factor(double (&L)[K][K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double mkk = L[k][k];
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < k; ++m) sum += L[k][m] * L[k][m];
        const double d = mkk - sum;
        if (!(d > 1e-10 * mkk)) return false;
        L[k][k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            double inner = 0.0;
#pragma unroll
            for (int m = 0; m < k; ++m) inner += L[i][m] * L[k][m];
            L[i][k] = (L[i][k] - inner) / L[k][k];
        }
    }
    return true;
}

template <int K>
__device__ __forceinline__ void solve(const double (&L)[K][K], const double (&b)[K], double (&x)[K])
{
    double y[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < i; ++m) sum += L[i][m] * y[m];
        y[i] = (b[i] - sum) / L[i][i];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double sum = 0.0;
#pragma unroll
        for (int m = i + 1; m < K; ++m) sum += L[m][i] * x[m];
        x[i] = (y[i] - sum) / L[i][i];
    }
}
