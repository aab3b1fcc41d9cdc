// Sort of (64-bit key, row index) pairs on the device, ascending by key and then by row index: every pair is distinct, so any
// correct sort yields the one pinned order (the package's tie rule: equal scores in ascending input row).  Shared by
// metrics.hip (ap_per_class) and tile_merge.h (the tile -> full-image merge).
//
// A bitonic network with every comparator pointing up: rows >= n act as +inf and are never touched, so n needs no padding.
// The steps whose partner lies inside a block of kBitonicBlock rows run in LDS -- one launch for the stages k = 2 .. kBitonicBlock,
// one per later stage for its steps j = kBitonicBlock / 2 .. 1 -- the wider ones one launch each.  No exchange between
// workgroups inside a launch.
#pragma once
#include <hip/hip_runtime.h>

namespace obb {
namespace {

constexpr int kBitonicThreads = 256;
constexpr int kBitonicBlock = 2048;      // 24 KiB of LDS: 2048 x (8-byte key, 4-byte row index)

// one comparator per row i with its partner above it; mirror: the first step of a merge of blocks of k rows
__global__ __launch_bounds__(kBitonicThreads) void k_bitonic(unsigned long long* __restrict__ key, int* __restrict__ idx, unsigned n, unsigned k,
                                                              unsigned j, int mirror) {
  const unsigned i = blockIdx.x * (unsigned)kBitonicThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned p = mirror ? (i ^ (k - 1u)) : (i ^ j);
  if (p <= i || p >= n) return;
  const unsigned long long ka = key[i], kb = key[p];
  const int ia = idx[i], ib = idx[p];
  if (kb < ka || (kb == ka && ib < ia)) {
    key[i] = kb, key[p] = ka;
    idx[i] = ib, idx[p] = ia;
  }
}

__device__ __forceinline__ void bitonic_lds_cmpx(unsigned long long* sk, int* si, int i, int p) {
  const unsigned long long ka = sk[i], kb = sk[p];
  const int ia = si[i], ib = si[p];
  if (kb < ka || (kb == ka && ib < ia)) {
    sk[i] = kb, sk[p] = ka;
    si[i] = ib, si[p] = ia;
  }
}

// merge_only = 0: the stages k = 2 .. kBitonicBlock; 1: the steps j = kBitonicBlock / 2 .. 1 of a later stage.  Rows >= n are +inf here too.
__global__ __launch_bounds__(kBitonicThreads) void k_bitonic_lds(unsigned long long* __restrict__ key, int* __restrict__ idx, unsigned n,
                                                                  int merge_only) {
  __shared__ unsigned long long sk[kBitonicBlock];
  __shared__ int si[kBitonicBlock];
  const int tid = threadIdx.x;
  const unsigned base = blockIdx.x * (unsigned)kBitonicBlock;
  for (int q = tid; q < kBitonicBlock; q += kBitonicThreads) {
    const unsigned g = base + (unsigned)q;
    sk[q] = g < n ? key[g] : ~0ull;
    si[q] = g < n ? idx[g] : 0x7fffffff;
  }
  __syncthreads();
  for (int k = merge_only ? kBitonicBlock : 2; k <= kBitonicBlock; k <<= 1) {
    if (!merge_only) {                                   // mirror step of the merge of blocks of k rows
      const int h = k >> 1;
      for (int t = tid; t < kBitonicBlock / 2; t += kBitonicThreads) {
        const int i = ((t & ~(h - 1)) << 1) | (t & (h - 1));
        bitonic_lds_cmpx(sk, si, i, i ^ (k - 1));
      }
      __syncthreads();
    }
    for (int j = merge_only ? k >> 1 : k >> 2; j > 0; j >>= 1) {
      for (int t = tid; t < kBitonicBlock / 2; t += kBitonicThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        bitonic_lds_cmpx(sk, si, i, i + j);
      }
      __syncthreads();
    }
  }
  for (int q = tid; q < kBitonicBlock; q += kBitonicThreads) {
    const unsigned g = base + (unsigned)q;
    if (g < n) key[g] = sk[q], idx[g] = si[q];
  }
}

// key[0 .. rows), idx[0 .. rows) sorted in place on `st` (rows >= 1)
inline void bitonic_sort_pairs(unsigned long long* key, int* idx, unsigned rows, hipStream_t st) {
  const unsigned grid = (rows + kBitonicThreads - 1) / kBitonicThreads;
  const unsigned sort_blocks = (rows + kBitonicBlock - 1) / kBitonicBlock;
  k_bitonic_lds<<<sort_blocks, kBitonicThreads, 0, st>>>(key, idx, rows, 0);
  for (unsigned long long k = 2ull * kBitonicBlock; (k >> 1) < rows; k <<= 1) {
    k_bitonic<<<grid, kBitonicThreads, 0, st>>>(key, idx, rows, (unsigned)k, 0u, 1);
    for (unsigned j = (unsigned)(k >> 2); j >= (unsigned)kBitonicBlock; j >>= 1)
      k_bitonic<<<grid, kBitonicThreads, 0, st>>>(key, idx, rows, (unsigned)k, j, 0);
    k_bitonic_lds<<<sort_blocks, kBitonicThreads, 0, st>>>(key, idx, rows, 1);
  }
}

}  // namespace
}  // namespace obb
