// workspace.h — the host layer every file with a caller-provided workspace shares (DESIGN.md 6.4 "Scene-aligned tiles,
// partials and the workspace carver").  A file writes its layout ONCE, as a `lay_out(Carver&, ...)` that returns the region
// pointers: `*_workspace_bytes` measures it on Carver(nullptr), the launch checks the caller's buffer with require_workspace
// and carves it with the same function, so the size and the pointers cannot drift apart.
#pragma once
#include "common.h"

namespace vdetr {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Hands out the regions of a workspace in order, each starting on a multiple of 256 B.  On nullptr it measures (bytes(); the
// *_workspace_bytes functions add 256 for the start's own rounding), on the caller's pointer it yields the regions.
class Carver {
 public:
  explicit Carver(const void* workspace) : raw_((uintptr_t)workspace), start_(align256(raw_)), at_(start_) {}
  template <typename T>
  T* take(size_t count) {
    T* p = take_unpadded<T>(count);
    at_ = align256(at_);
    return p;
  }
  template <typename T>
  T* take_unpadded(size_t count) {                                      // for a last region whose size was never rounded up
    T* p = reinterpret_cast<T*>(at_);
    at_ += count * sizeof(T);
    return p;
  }
  // One T (at most 240 B) on the first multiple of 16 B of the caller's own pointer: it lies inside the 256 B that hold the
  // start's rounding, so alone it costs nothing; regions that follow it start 256 B further on, clear of it.  Call it first.
  template <typename T>
  T* take_head16(bool regions_follow) {
    static_assert(sizeof(T) <= 240, "the head slot must fit the start's rounding");
    if (regions_follow) at_ += 256;
    return reinterpret_cast<T*>((raw_ + 15) & ~(uintptr_t)15);
  }
  size_t bytes() const { return at_ - start_; }

 private:
  uintptr_t raw_, start_, at_;
};

inline int require_workspace(const char* op, const void* workspace, size_t have, size_t need) {
  if (workspace && have >= need) return VDETR_OK;
  set_error("%s: workspace %zu B < required %zu B", op, have, need);
  return VDETR_ERR_WORKSPACE;
}

}  // namespace vdetr
