// train_meter.hip — the training loop's loss meter on the device (vdetr_loss_meter_update_f32).
//
// Reference: engine.py:74,100-102,109.  Every iteration reads `loss_reduced.item()` twice: for `math.isfinite` (a non-finite loss
// ends the run BEFORE backward and the optimizer step) and for `SmoothedValue.update` (utils/misc.py:53-56: the deque of the last
// `window_size` values, their count and their double sum).  Either read drains the queue of a step that the host enqueues about as
// slowly as the device runs it.  This launch takes the loss as the device scalar it is and keeps what the two reads fed in one
// 288-byte block; the host copies the block back where the reference prints (engine.LossMeter.read).  The `bad` word of the block is
// the flag vdetr_adamw_guard_f32 reads: "stop before the step" is decided here, on the device.
// One workgroup, one lane: three loads, at most three stores; the launch is its cost.
#include "common.h"

namespace vdetr {

__global__ __launch_bounds__(kWave) void loss_meter_kernel(const float* __restrict__ loss, vdetr_loss_meter_state* __restrict__ st,
                                                           long iter) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st->bad != 0) return;  // training has stopped: later losses do not enter the window
  const int window = st->window;
  if (window < 1 || window > VDETR_LOSS_METER_MAX_WINDOW) {  // device data: not trusted as an index bound
    st->bad = 2;
    return;
  }
  const float x = *loss;
  if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {  // NaN or +-inf: what math.isfinite refuses
    st->bad = 1;
    st->bad_iter = iter;
    return;
  }
  const long count = st->count;
  const long slot = count >= 0 ? count % window : 0;
  st->ring[slot] = x;
  st->total += (double)x;
  st->count = count + 1;
}

}  // namespace vdetr

using namespace vdetr;

extern "C" int vdetr_loss_meter_update_f32(const vdetr_loss_meter_desc* d, vdetr_stream_t stream) {
  VDETR_REQUIRE(d != nullptr, "loss_meter_update: null descriptor");
  VDETR_REQUIRE(d->loss != nullptr, "loss_meter_update: loss is NULL");
  VDETR_REQUIRE(d->state != nullptr, "loss_meter_update: state is NULL");
  VDETR_REQUIRE(((uintptr_t)d->loss & 3) == 0 && ((uintptr_t)d->state & 7) == 0,
                "loss_meter_update: loss must be 4-B aligned and state 8-B aligned (loss %p, state %p)", (const void*)d->loss,
                (const void*)d->state);
  VDETR_REQUIRE(d->iter >= 0, "loss_meter_update: iter=%lld", (long long)d->iter);
  hipLaunchKernelGGL(loss_meter_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, d->loss, d->state, (long)d->iter);
  return check_launch("loss_meter_update");
}
