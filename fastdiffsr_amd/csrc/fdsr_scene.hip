// Whole-scene tiling on gfx950 (include/fdsr.h: fdsr_scene_gather / _blend / _finish; fastdiffsr_amd/scene.py walks the scene).
//
//   gather   scene-sized arrays -> the tiles' network inputs: cond = ToTensor() * 2 - 1 of the uint8 scene (the arithmetic of
//            u8_to_tensor_kernel, fdsr_val.hip), noise = crops of a [P,3,SH,SW] field in fdsr_sample's [P,B,3,t,t] layout
//   blend    sampled tiles -> acc [3,SH,SW] += w * v, wsum [SH,SW] += w with the plan's separable ramps
//   finish   acc / wsum -> fp32 scene and / or the uint8 scene (the arithmetic of tensor2img_u8_kernel, fdsr_kernels.hip)
//
// All three move bytes and nothing else: a thread owns four consecutive pixels of a row.  Its four fp32 values of a plane move as
// one 16-byte access wherever the address allows it (a tile's x0, or a scene width that is no multiple of 4, shifts the scene side
// off the 16-byte grid: those groups, and the last group of a row whose length is no multiple of 4, go element by element).  Its
// twelve uint8 bytes (gather reads them, finish writes them) move as three dwords where they start on a 4-byte address, else byte
// by byte.
//
// Determinism of blend: one launch per tile, in ascending tile index, on the caller's stream; inside a launch a scene pixel is
// touched by exactly one thread; the product and the sums are separately rounded fp32 operations (__fmul_rn / __fadd_rn: the
// compiler may not contract them).  There are no atomics.  Weights are evaluated in fp64 from small integers and rounded once.
//
// The tile tables live on the device, so the host cannot check them: every kernel skips a tile whose origin would leave the scene.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fdsr_engine_int.h"

using namespace fdsr_int;

namespace {

constexpr int NT = 256;
constexpr size_t MAX_BLOCKS = 8192;     // memory-bound: a few workgroups per CU, the rest of the work by grid stride

unsigned blocks_for(size_t total) {
  const size_t b = (total + NT - 1) / NT;
  return (unsigned)(b < MAX_BLOCKS ? (b ? b : 1) : MAX_BLOCKS);
}

__device__ __forceinline__ bool tile_origin(const int* __restrict__ origins, int b, int t, int SH, int SW, int* y0, int* x0) {
  *y0 = origins[2 * b];
  *x0 = origins[2 * b + 1];
  return *y0 >= 0 && *x0 >= 0 && *y0 <= SH - t && *x0 <= SW - t;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ void load4(const float* __restrict__ p, float v[4], int n) {
  if (n == 4 && aligned16(p)) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ p, const float v[4], int n) {
  if (n == 4 && aligned16(p)) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < n; ++k) p[k] = v[k];
  }
}

// one thread: four pixels of one tile row, the three channels
__global__ void __launch_bounds__(NT) scene_gather_cond_kernel(const unsigned char* __restrict__ scene, const int* __restrict__ origins,
                                                               float* __restrict__ cond, int B, int t, int SH, int SW) {
  const int G = (t + 3) / 4;
  const size_t total = (size_t)B * t * G;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const int g = (int)(i % G), y = (int)((i / G) % t), b = (int)(i / ((size_t)G * t));
    int y0, x0;
    if (!tile_origin(origins, b, t, SH, SW, &y0, &x0)) continue;
    const int x = 4 * g, n = min(4, t - x);
    const unsigned char* src = scene + ((size_t)(y0 + y) * SW + x0 + x) * 3;
    unsigned char px[12];
    if (n == 4 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {      // four whole pixels, inside the tile's row: three dword loads
      const unsigned int* s32 = reinterpret_cast<const unsigned int*>(src);
      for (int q = 0; q < 3; ++q) {
        const unsigned int u = s32[q];
        for (int e = 0; e < 4; ++e) px[4 * q + e] = (unsigned char)(u >> (8 * e));
      }
    } else {
      for (int k = 0; k < 3 * n; ++k) px[k] = src[k];
    }
    for (int c = 0; c < 3; ++c) {
      float v[4];
      for (int k = 0; k < n; ++k)      // ToTensor() (/ 255), * (hi - lo), + lo with (lo, hi) = (-1, 1): fdsr_val.hip, u8_to_tensor_kernel
        v[k] = __fadd_rn(__fmul_rn(__fdiv_rn((float)px[k * 3 + c], 255.0f), 2.0f), -1.0f);
      store4(cond + (((size_t)b * 3 + c) * t + y) * t + x, v, n);
    }
  }
}

// one thread: four pixels of one row of one (plane, tile, channel)
__global__ void __launch_bounds__(NT) scene_gather_noise_kernel(const float* __restrict__ field, const int* __restrict__ origins,
                                                                float* __restrict__ noise, int P, int B, int t, int SH, int SW) {
  const int G = (t + 3) / 4;
  const size_t total = (size_t)P * B * 3 * t * G;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    size_t r = i;
    const int g = (int)(r % G); r /= G;
    const int y = (int)(r % t); r /= t;
    const int c = (int)(r % 3); r /= 3;
    const int b = (int)(r % B);
    const int p = (int)(r / B);
    int y0, x0;
    if (!tile_origin(origins, b, t, SH, SW, &y0, &x0)) continue;
    const int x = 4 * g, n = min(4, t - x);
    float v[4];
    load4(field + (((size_t)p * 3 + c) * SH + y0 + y) * SW + x0 + x, v, n);
    store4(noise + ((((size_t)p * B + b) * 3 + c) * t + y) * t + x, v, n);
  }
}

// the 1-D weight of include/fdsr.h, in fp64: quotients of small integers, at most two of them multiplied
__device__ __forceinline__ double ramp_weight(int i, int t, int lead, int trail) {
  double w = 1.0;
  if (i < lead) w = (double)(i + 1) / (double)(lead + 1);
  if (i >= t - trail) w *= (double)(t - i) / (double)(trail + 1);
  return w;
}

__device__ __forceinline__ int clamp_ramp(int r, int t) { return r < 0 ? 0 : (r > t ? t : r); }

// ONE tile per launch (tile `b` of this call's tables); one thread: four pixels of one tile row
__global__ void __launch_bounds__(NT) scene_blend_kernel(const float* __restrict__ tiles, const int* __restrict__ origins,
                                                         const int* __restrict__ ramps, int b, int t, float* __restrict__ acc,
                                                         float* __restrict__ wsum, int SH, int SW) {
  const int G = (t + 3) / 4;
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= t * G) return;
  int y0, x0;
  if (!tile_origin(origins, b, t, SH, SW, &y0, &x0)) return;
  const int g = i % G, y = i / G;
  const int x = 4 * g, n = min(4, t - x);
  const int top = clamp_ramp(ramps[4 * b], t), left = clamp_ramp(ramps[4 * b + 1], t);
  const int bottom = clamp_ramp(ramps[4 * b + 2], t), right = clamp_ramp(ramps[4 * b + 3], t);
  const double wy = ramp_weight(y, t, top, bottom);
  float w[4];
  for (int k = 0; k < 4; ++k) w[k] = k < n ? (float)(wy * ramp_weight(x + k, t, left, right)) : 0.f;
  const size_t at = (size_t)(y0 + y) * SW + x0 + x;
  for (int c = 0; c < 3; ++c) {
    float v[4], a[4];
    load4(tiles + (((size_t)b * 3 + c) * t + y) * t + x, v, n);
    float* dst = acc + (size_t)c * SH * SW + at;
    load4(dst, a, n);
    for (int k = 0; k < n; ++k) a[k] = __fadd_rn(a[k], __fmul_rn(w[k], v[k]));
    store4(dst, a, n);
  }
  float s[4];
  load4(wsum + at, s, n);
  for (int k = 0; k < n; ++k) s[k] = __fadd_rn(s[k], w[k]);
  store4(wsum + at, s, n);
}

// one thread: four consecutive pixels of the flattened scene
__global__ void __launch_bounds__(NT) scene_finish_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, size_t N,
                                                          unsigned char* __restrict__ dst_u8, float* __restrict__ dst_f32) {
  const size_t groups = (N + 3) / 4;
  for (size_t gi = (size_t)blockIdx.x * NT + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * NT) {
    const size_t i = 4 * gi;
    const int n = (int)(N - i < 4 ? N - i : 4);
    float s[4];
    load4(wsum + i, s, n);
    unsigned char px[12];
    for (int c = 0; c < 3; ++c) {
      float a[4];
      load4(acc + c * N + i, a, n);
      for (int k = 0; k < n; ++k) a[k] = __fdiv_rn(a[k], s[k]);
      if (dst_f32) store4(dst_f32 + c * N + i, a, n);
      for (int k = 0; k < n; ++k) {     // Metrics.tensor2img with min_max = (-1, 1): fdsr_kernels.hip, tensor2img_u8_kernel
        float v = fminf(fmaxf(a[k], -1.0f), 1.0f);
        v = __fdiv_rn(__fsub_rn(v, -1.0f), __fsub_rn(1.0f, -1.0f));
        px[k * 3 + c] = (unsigned char)rintf(__fmul_rn(v, 255.0f));
      }
    }
    if (!dst_u8) continue;
    unsigned char* o = dst_u8 + i * 3;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      unsigned int* o32 = reinterpret_cast<unsigned int*>(o);
      for (int q = 0; q < 3; ++q)
        o32[q] = (unsigned)px[4 * q] | ((unsigned)px[4 * q + 1] << 8) | ((unsigned)px[4 * q + 2] << 16) | ((unsigned)px[4 * q + 3] << 24);
    } else {
      for (int k = 0; k < 3 * n; ++k) o[k] = px[k];
    }
  }
}

bool bad_scene(int SH, int SW, int t) { return t < 1 || SH < t || SW < t; }

}  // namespace

extern "C" {

int fdsr_scene_gather(fdsr_handle h, const uint8_t* scene_u8, const float* field, int planes, int scene_h, int scene_w,
                      const int32_t* origins, int n_tiles, int tile, float* cond, float* noise, void* hip_stream) {
  if (!scene_u8 || !origins || !cond || n_tiles < 1 || bad_scene(scene_h, scene_w, tile) || (field && (!noise || planes < 1)))
    return fail(h, FDSR_E_INVALID, "fdsr_scene_gather: bad arguments (%d tiles of %d in a %dx%d scene, %d planes)", n_tiles, tile,
                scene_h, scene_w, planes);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int G = (tile + 3) / 4;
  hipLaunchKernelGGL(scene_gather_cond_kernel, dim3(blocks_for((size_t)n_tiles * tile * G)), dim3(NT), 0, st, scene_u8, origins, cond,
                     n_tiles, tile, scene_h, scene_w);
  HIPCHK(h, hipGetLastError());
  if (field) {
    hipLaunchKernelGGL(scene_gather_noise_kernel, dim3(blocks_for((size_t)planes * n_tiles * 3 * tile * G)), dim3(NT), 0, st, field,
                       origins, noise, planes, n_tiles, tile, scene_h, scene_w);
    HIPCHK(h, hipGetLastError());
  }
  return FDSR_OK;
}

int fdsr_scene_gather_f32(fdsr_handle h, const float* scene, int scene_h, int scene_w, const int32_t* origins, int n_tiles, int tile,
                          float* tiles, void* hip_stream) {
  if (!scene || !origins || !tiles || n_tiles < 1 || bad_scene(scene_h, scene_w, tile))
    return fail(h, FDSR_E_INVALID, "fdsr_scene_gather_f32: bad arguments (%d tiles of %d in a %dx%d scene)", n_tiles, tile, scene_h,
                scene_w);
  // a [3,SH,SW] image is a noise field of one plane, and [1,n,3,t,t] is [n,3,t,t]
  hipLaunchKernelGGL(scene_gather_noise_kernel, dim3(blocks_for((size_t)n_tiles * 3 * tile * ((tile + 3) / 4))), dim3(NT), 0,
                     reinterpret_cast<hipStream_t>(hip_stream), scene, origins, tiles, 1, n_tiles, tile, scene_h, scene_w);
  HIPCHK(h, hipGetLastError());
  return FDSR_OK;
}

int fdsr_scene_blend(fdsr_handle h, const float* tiles, const int32_t* origins, const int32_t* ramps, int n_tiles, int tile,
                     float* acc, float* wsum, int scene_h, int scene_w, void* hip_stream) {
  if (!tiles || !origins || !ramps || !acc || !wsum || n_tiles < 1 || bad_scene(scene_h, scene_w, tile) || tile > 32768)
    return fail(h, FDSR_E_INVALID, "fdsr_scene_blend: bad arguments (%d tiles of %d in a %dx%d scene)", n_tiles, tile, scene_h, scene_w);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int threads = tile * ((tile + 3) / 4);
  for (int b = 0; b < n_tiles; ++b)      // ascending tile index on one stream: the order every scene pixel sees
    hipLaunchKernelGGL(scene_blend_kernel, dim3((unsigned)((threads + NT - 1) / NT)), dim3(NT), 0, st, tiles, origins, ramps, b, tile,
                       acc, wsum, scene_h, scene_w);
  HIPCHK(h, hipGetLastError());
  return FDSR_OK;
}

int fdsr_scene_finish(fdsr_handle h, const float* acc, const float* wsum, int scene_h, int scene_w, uint8_t* dst_u8, float* dst_f32,
                      void* hip_stream) {
  if (!acc || !wsum || scene_h < 1 || scene_w < 1 || (!dst_u8 && !dst_f32))
    return fail(h, FDSR_E_INVALID, "fdsr_scene_finish: bad arguments (%dx%d scene)", scene_h, scene_w);
  const size_t N = (size_t)scene_h * scene_w;
  hipLaunchKernelGGL(scene_finish_kernel, dim3(blocks_for((N + 3) / 4)), dim3(NT), 0, reinterpret_cast<hipStream_t>(hip_stream), acc,
                     wsum, N, dst_u8, dst_f32);
  HIPCHK(h, hipGetLastError());
  return FDSR_OK;
}

}  // extern "C"
