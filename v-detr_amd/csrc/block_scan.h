// block_scan.h — prefixes over a workgroup, and the tile compaction built on them.  Device only.
//
// One algorithm: a `__shfl_up` ladder inside each wave, then ONE LDS word per wave.  Contract of every block_* function:
// every thread of a workgroup of exactly THREADS threads calls it (uniform control flow); `row` is the caller's
// `__shared__ T row[THREADS / kWave]`; the function ENDS in a barrier, so the row may be reused at once and needs none on entry.
//
// Compaction in two launches, as every caller here does it (nothing waits between the launches):
//   launch 1  one workgroup per tile flags its rows and writes ONE count per tile with an ordinary store
//   launch 2  every workgroup adds up the counts of the tiles before its own (block_sum over a few hundred words), ranks its own
//             flags (block_exclusive_sum / block_rank) and writes its rows; the workgroup of the last tile writes the total
// No "last workgroup adds up" ticket (README round 6: 43-68 us against 6 us for two launches on this chip), no device-wide
// atomics and no memset: every word has one writer and two runs give the same bits.  Where the counts are too many to re-add
// per workgroup, ONE workgroup scans them in between (block_exclusive_sum_array).
#pragma once
#include "wave.h"

namespace vdetr {

// inclusive prefix sum of v over the lanes of the wave
__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive prefix sum of v over the workgroup's threads; `total` is the workgroup's sum (all a count-only launch keeps)
template <int THREADS>
__device__ __forceinline__ int block_exclusive_sum(int v, int (&row)[THREADS / kWave], int& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int inc = wave_inclusive_sum(v);
  if (lane == kWave - 1) row[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / kWave; ++w) {
    const int s = row[w];
    if (w < wave) before += s;
    total += s;
  }
  __syncthreads();
  return before + inc - v;
}

// the same for any value type and associative op(earlier, later) with its identity (no inverse needed: int / plus, double / fmax)
template <int THREADS, typename T, typename Op>
__device__ __forceinline__ T block_exclusive_scan(T v, T identity, Op op, T (&row)[THREADS / kWave], T& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  T inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T o = __shfl_up(inc, d, kWave);
    if (lane >= d) inc = op(o, inc);
  }
  const T below = __shfl_up(inc, 1, kWave);  // the inclusive prefix of the lane before
  if (lane == kWave - 1) row[wave] = inc;
  __syncthreads();
  T before = identity;
  total = identity;
#pragma unroll
  for (int w = 0; w < THREADS / kWave; ++w) {
    const T s = row[w];
    if (w < wave) before = op(before, s);
    total = op(total, s);
  }
  __syncthreads();
  return lane > 0 ? op(before, below) : before;
}

// set flags in the threads below this one (the ballot rank); `total` is the number of set flags in the workgroup
template <int THREADS>
__device__ __forceinline__ int block_rank(bool flag, int (&row)[THREADS / kWave], int& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) row[wave] = __popcll(mask);
  __syncthreads();
  int before = __popcll(mask & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / kWave; ++w) {
    const int s = row[w];
    if (w < wave) before += s;
    total += s;
  }
  __syncthreads();
  return before;
}

// sum of term(i) over i in [0, n), strided over the workgroup (the earlier tiles' counts; flags to count), the same in every thread
template <int THREADS, typename I, typename F>
__device__ __forceinline__ int block_sum(I n, F term, int (&row)[THREADS / kWave]) {
  int s = 0;
  for (I i = threadIdx.x; i < n; i += THREADS) s += term(i);
  int total;
  block_exclusive_sum<THREADS>(s, row, total);
  return total;
}

// out[i] = in[0] + .. + in[i - 1] for i in [0, n) by ONE workgroup, THREADS entries per pass with a carry; out may be in.
// Returns the sum of all n, in every thread.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_sum_array(const int* in, int* out, int n, int (&row)[THREADS / kWave]) {
  int carry = 0;
  for (int base = 0; base < n; base += THREADS) {
    const int i = base + (int)threadIdx.x;
    int total;
    const int before = block_exclusive_sum<THREADS>(i < n ? in[i] : 0, row, total);
    if (i < n) out[i] = carry + before;
    carry += total;
  }
  return carry;
}

}  // namespace vdetr
