// urgym_philox.h — Philox4x32-10 (Salmon et al., SC'11), the one counter-based generator of the library: the reset sampler of the
// step kernels (urgym_hip.hip, through urgym_device.h) and the policy noise of the actor kernels (urgym_actor.hip) both call this
// function.  Integer code only, so it means the same under either translation unit's floating-point flags.  The including file
// provides __device__, __forceinline__ and __umulhi (hip_runtime.h, or the host harness's stand-ins in urgym_device.h).
#pragma once
#include <stdint.h>

namespace urgym {

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace urgym
