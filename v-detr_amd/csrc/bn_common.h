// bn_common.h — what the BatchNorm + ReLU + Dropout blocks (bn_act.hip, heads.hip) share: their dropout stream, keyed by (channel,
// element of the channel's B*N values) so that the fused heads launch and the one-launch-per-block form draw the same masks for
// the same (salt, generator state) and the backward regenerates them; and the activation behind a sparse tensor's BatchNorm.
#pragma once
#include "attn_common.h"

namespace vdetr {

// drop_stream.h's pair form: drop_prefix(g, channel, 1), then word e >> 1 holds the draws of elements e and e ^ 1 (drop_keep_pair)
__device__ __forceinline__ DropStream bn_rng(const vdetr_bnact_desc& d) { return drop_stream(d.dropout_p, d.seed, d.offset, d.rng_state); }

// the activation behind a sparse tensor's BatchNorm (sp_bn.hip, and the eval-mode epilogue of sparse_conv.hip): 0 none, 1 ReLU,
// 2 ELU (alpha 1), on the four channels a thread holds
__device__ __forceinline__ f32x4 bn_act(f32x4 v, int act) {
  if (act == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  } else if (act == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : expm1f(v[e]);
  }
  return v;
}

}  // namespace vdetr
