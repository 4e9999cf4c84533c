// Philox4x32-10 (Salmon et al., SC'11) + Box-Muller: the device side of the engine's pinned noise streams (include/fdsr.h documents
// the counter / key words; tests/philox_reference.py restates them).  Shared by fdsr_kernels.hip and fdsr_nafnet.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace fdsr {

__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
// Tile-addressed noise (include/fdsr.h: fdsr_set_noise_tiles): the counter of pixel `pix` = y * W + x of image n, a W-wide tile whose
// origin in a scene_w-wide scene is origins[n] = (y0, x0): the pixel's index in the scene, (y0 + y) * scene_w + (x0 + x), in 64 bits.
// It addresses a counter, not memory: an origin outside the scene only draws other numbers.
__device__ __forceinline__ size_t tile_counter(const int* __restrict__ origins, int scene_w, int W, size_t n, size_t pix) {
  const long long y = (long long)origins[2 * n] + (long long)(pix / (size_t)W);
  const long long x = (long long)origins[2 * n + 1] + (long long)(pix % (size_t)W);
  return (size_t)(y * (long long)scene_w + x);
}
// three standard normals for pixel `i` of noise plane `plane` under {seed, calls}
__device__ __forceinline__ void randn3(const unsigned long long* rng, int plane, size_t i, float out[3]) {
  const unsigned long long seed = rng[0], calls = rng[1];
  unsigned c0 = (unsigned)i, c1 = (unsigned)(i >> 32), c2 = (unsigned)plane, c3 = (unsigned)calls;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ (unsigned)(calls >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  // 24-bit uniforms in (0,1] (above 2^23 the sum rounds to even: 0xFFFFFF gives 1, radius 0; the smallest, 2^-25, gives |z| <= 5.887);
  // Box-Muller on two pairs (the fourth normal is not used)
  const float u0 = ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-8f, u1 = ((float)(c1 >> 8) + 0.5f) * 5.9604644775390625e-8f;
  const float u2 = ((float)(c2 >> 8) + 0.5f) * 5.9604644775390625e-8f, u3 = ((float)(c3 >> 8) + 0.5f) * 5.9604644775390625e-8f;
  const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
  float s0, cs0, s1, cs1;
  sincospif(2.0f * u1, &s0, &cs0);
  sincospif(2.0f * u3, &s1, &cs1);
  out[0] = r0 * cs0;
  out[1] = r0 * s0;
  out[2] = r1 * cs1;
  (void)s1;
}

}  // namespace fdsr
