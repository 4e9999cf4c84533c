// Device-side pieces that fdsr_train.hip and fdsr_wgrad.hip both use.  Internal header, HIP sources only.
#pragma once

namespace fdsr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

}  // namespace fdsr
