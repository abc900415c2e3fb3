// gs_reduce.h - the fixed LDS halving tree behind every "one fixed sequence of roundings" sum of the small-kernel files, once.
//
// Contract.  A ROW is THREADS consecutive LDS elements, element t written by lane t; a row set is N rows at stride THREADS
// (sh[q * THREADS + t], or T sh[N][THREADS]).  The tree runs the steps w = THREADS / 2, THREADS / 4, ..., 1, and in step w lane
// t < w does row[t] += row[t + w], for every row of the first set in row order, then every row of the second set.  Which two
// elements meet at which step is a function of THREADS alone: neither the grid, nor the wave a lane sits in, nor the other
// lanes' values move an addition, so a float sum has the same bits every run and an integer sum the value any order gives.
// The result of a row is at its element 0.  Both row sets go through ONE barrier sequence: a barrier before the first step (the
// callers' own writes to the rows are visible) and one after every step.  After the call every lane of the workgroup may read
// element 0 of any row; elements 1 .. THREADS - 1 hold partial sums and mean nothing.  The call ends on a barrier that orders
// the tree's last write before the lanes' reads, NOT those reads before a later write: whoever writes the rows again without a
// barrier of its own in between races with a lane still reading (gs_depth_norm.hip adds that barrier, the others read once).
// Every lane of the workgroup must make the call (the barriers are uniform), with THREADS == blockDim.x.
//
// The shuffle trees of the wave sums (gs_loss.hip, gs_eval.hip, ...) are another order and not this file's business.
#pragma once
#include <hip/hip_runtime.h>

// NA rows of a and NB rows of b, already written, through one barrier sequence
template <int THREADS, int NA, int NB = 0, typename A, typename B = A>
__device__ __forceinline__ void gs_block_tree(A* a, int t, B* b = nullptr) {
  static_assert(THREADS > 1 && (THREADS & (THREADS - 1)) == 0, "the halving tree needs a power of two");
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (t < w) {
      for (int q = 0; q < NA; q++) a[q * THREADS + t] += a[q * THREADS + t + w];
      for (int q = 0; q < NB; q++) b[q * THREADS + t] += b[q * THREADS + t + w];
    }
    __syncthreads();
  }
}

// lane t's v[q] -> element t of row q
template <int THREADS, int N, typename T>
__device__ __forceinline__ void gs_rows_put(const T (&v)[N], T* sh, int t) {
  for (int q = 0; q < N; q++) sh[q * THREADS + t] = v[q];
}

// sum of v[q] over the workgroup; every lane's v holds the result.  sh: [N][THREADS]
template <int THREADS, int N, typename T>
__device__ __forceinline__ void gs_block_tree_sum(T (&v)[N], T* sh, int t) {
  gs_rows_put<THREADS>(v, sh, t);
  gs_block_tree<THREADS, N>(sh, t);
  for (int q = 0; q < N; q++) v[q] = sh[q * THREADS];
}

// the finishing kernels' step: part is [count][N]; lane t adds the records t, t + THREADS, ... in index order, then the tree.
// Every lane's v holds the result.
template <int THREADS, int N, typename T>
__device__ __forceinline__ void gs_partials_tree_sum(const T* part, int count, T (&v)[N], T* sh, int t) {
  for (int q = 0; q < N; q++) v[q] = T(0);
  for (int i = t; i < count; i += THREADS)
    for (int q = 0; q < N; q++) v[q] += part[(size_t)i * N + q];
  gs_block_tree_sum<THREADS>(v, sh, t);
}
