// pos_bn.h — what the two kernels of the position MLP (PositionEmbeddingLearned) share around its BatchNorm: pos_mlp_kernel
// (heads.hip) and rb_qkv_pos_kernel (rowblock_pos.hip).  DESIGN.md 4.5, 6.4.3.  Per-thread device code (no LDS, no barrier) and one
// host dispatcher.  Thread tid of a workgroup of kPosThreads = 256 threads is hidden channel tid.
//
// NOT here, on purpose: the coordinates' moments (phase 1) and the channel's mean / variance from them.  Every shape of a shared
// function tried for them moved the digests of the 16 training instantiations; the two files keep them written out,
// the same arithmetic in the same order (tests/test_gpu_rowblock.py: torch.equal), each with a pointer at its twin.
#pragma once
#include <type_traits>

#include "common.h"

namespace vdetr {

constexpr int kPosThreads = 256;
constexpr int pos_nmom(int cin) { return cin + cin * (cin + 1) / 2; }  // sums + upper triangle of the coordinates' second moments

// what ONE workgroup of a training launch (the caller picks it) leaves behind: the saved statistics, the running ones (the mean
// with the convolution's bias, the unbiased variance) and the batch counter.  (The descriptor travels by value: by reference the
// widest instantiations lost an instruction.)
__device__ __forceinline__ void pos_store_stats(vdetr_posmlp_desc M, int T, float meanf, float varf, float invstd, float bias1) {
  const int ch = threadIdx.x;
  M.save_mean[ch] = meanf;
  M.save_invstd[ch] = invstd;
  if (M.running_mean) {
    const float m = M.momentum, n = (float)T;
    M.running_mean[ch] = (1.f - m) * M.running_mean[ch] + m * (meanf + bias1);
    M.running_var[ch] = (1.f - m) * M.running_var[ch] + m * varf * (n / (n > 1.f ? n - 1.f : 1.f));
  }
  if (ch == 0 && M.counter) M.counter[0] += 1;
}

// eval form: relu(((W1 x + b1 - rm) * invstd) * gamma + beta) with the running statistics (torch's eval order)
__device__ __forceinline__ void pos_infer_stats(const vdetr_posmlp_desc& M, float& rm, float& invstd) {
  const int ch = threadIdx.x;
  rm = M.running_mean[ch];
  invstd = rsqrtf(M.running_var[ch] + M.eps);
}

// launch(std::integral_constant<int, CIN>) for the kernel instance of cin coordinates (1 .. 8: the callers check)
template <typename F>
static inline void dispatch_cin(int cin, F launch) {
  switch (cin) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;  // (key positions: pos_for_key)
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;  // (box centre + size: the decoder's query position)
    case 7: launch(std::integral_constant<int, 7>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace vdetr
