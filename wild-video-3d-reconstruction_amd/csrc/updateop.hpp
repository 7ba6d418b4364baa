// updateop.hpp -- what the update-operator units (updateop.hip, groupby.hip,
// scatter.hip) share on the host: workspace alignment and the dtype dispatch.
#pragma once

#include "common.hpp"

namespace dpvo {

// workspace regions start on 256-byte boundaries; callers give 256 spare bytes
static inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }
static inline char* align256(void* p) { return (char*)(((uintptr_t)p + 255) & ~uintptr_t(255)); }

// fn(T()) for the element type of a DPVO_F16 / F32 / F64 code; false (and no
// call) for any other code
template <typename F>
static inline bool dispatch_dtype(int dtype, F&& fn)
{
    switch (dtype) {
    case DPVO_F16: fn(half_t()); return true;
    case DPVO_F32: fn(float()); return true;
    case DPVO_F64: fn(double()); return true;
    default: return false;
    }
}

}  // namespace dpvo
