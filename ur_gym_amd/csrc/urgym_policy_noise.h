// urgym_policy_noise.h — what the forward sampling kernels (urgym_actor.hip) and the policy-loss backward pass
// (urgym_actor_backward.hip) must agree on to the bit: the backward pass promises `action` and `log_prob` bitwise equal to
// urgym_actor_sample_rows', so the words of the policy noise and the constants of the Box-Muller and log-probability expressions are
// stated here once.  The expressions themselves stay in each kernel: their text is the bitwise contract, and each kernel states its own.
// Device code; the including unit provides hip_runtime.h.
#pragma once
#include <stdint.h>

#include "urgym_philox.h"

namespace urgym {

constexpr uint32_t NOISE_TAG = 0x504F4C00u;  // counter word 3 of the policy noise is NOISE_TAG | block (include/urgym.h)
constexpr float TWO_M24 = 1.0f / 16777216.0f;
constexpr float HALF_LOG_2PI = 0.918938533204672742f;

// the six words of (seed, draw, env) as their 24-bit integers m(w) = w >> 8, exact in float32
__device__ __forceinline__ void noise_words(uint64_t seed, uint64_t draw, uint32_t env, float m[6]) {
  uint32_t a[4], b[4];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), d0 = (uint32_t)draw, d1 = (uint32_t)(draw >> 32);
  philox4x32_10(k0, k1, env, d0, d1, NOISE_TAG | 0u, a);
  philox4x32_10(k0, k1, env, d0, d1, NOISE_TAG | 1u, b);
  m[0] = (float)(a[0] >> 8), m[1] = (float)(a[1] >> 8), m[2] = (float)(a[2] >> 8), m[3] = (float)(a[3] >> 8);
  m[4] = (float)(b[0] >> 8), m[5] = (float)(b[1] >> 8);
}

// six floats of a row (an action, its noise, ...) as three 8-byte stores
__device__ __forceinline__ void store6(float* rows, size_t row, const float v[6]) {
  float2* out = reinterpret_cast<float2*>(rows + row * 6);
  out[0] = make_float2(v[0], v[1]);
  out[1] = make_float2(v[2], v[3]);
  out[2] = make_float2(v[4], v[5]);
}

}  // namespace urgym
