// urgym_weights.hip — reloads the packed weights of an actor (urgym_actor.hip) or of the twin critics (urgym_critic.hip) from
// DEVICE tensors in torch's own layout: what a learner that keeps its parameters in torch does after every optimiser step, and, for
// the target critic, SAC's Polyak update (train.py:40-48, SB3 polyak_update with tau = 0.005) while it packs.  One launch per
// reload, on the caller's stream; no host synchronisation, no allocation.
//
// One lane writes one float4 ("quad") of the packed buffer: urgym_pack_map.h says which source tensor the quad comes from and
// which four elements of it (or padding, +0.0f), the inverse of the host packing loops of urgym_pack_host.h.  The packed writes are
// what the buffer is read by later, float4 per lane, consecutive lanes at consecutive addresses.  The source is read as single
// floats, so nothing beyond 4-byte alignment is assumed.  In layer 2 (the bulk) a lane reads four consecutive floats of a row and
// the two lane halves two adjacent such groups; the four waves of a workgroup take four consecutive reads sq of one tile, so a
// workgroup consumes 32 rows x 128 contiguous bytes: every cache line it touches is used completely within the workgroup, and the
// transposition needs no LDS.  The buffers are 0.1 to 2 MB: the launch is bound by latency, not by bandwidth.
//
//
// The unpack kernels run the same map the other way (a checkpoint holds the target critic, which exists only packed, in torch's
// layout): one lane reads its float4 and writes each float that has a source element back to that element as a single float;
// padding writes nothing.  Copies only: every bit pattern goes through unchanged.
//
// This unit may contract a * b + c to fma like urgym_actor.hip; the blend's products are therefore made opaque before the add.
#include <hip/hip_runtime.h>

#include "urgym_pack_map.h"
#include "urgym_weights.h"

namespace urgym {

namespace {

constexpr int PACK_THREADS = 256;

struct ActorPackParams {
  float4* packed;
  const float* src[PACK_ACTOR_TENSORS];
  PackDims d;
  uint32_t quads;  // float4 in the buffer
  int head;        // the log_std head is given
};

struct CriticPackParams {
  float4* packed;
  const float* src[2 * PACK_CRITIC_TENSORS];
  PackDims d;
  uint32_t quads;
  int blend;       // tau != 1
  float tau, omt;  // omt = 1.0f - tau, formed on the host
};

struct ActorUnpackParams {
  const float4* packed;
  float* dst[PACK_ACTOR_TENSORS];
  PackDims d;
  uint32_t quads;
  int head;  // the log_std head's destinations are given
};

struct CriticUnpackParams {
  const float4* packed;
  float* dst[2 * PACK_CRITIC_TENSORS];
  PackDims d;
  uint32_t quads;
};

// the urgym_critic.hip idiom: a value the compiler may not look through, no instruction emitted
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// src[t] without indexing the kernel arguments by a per-lane value (which would put them in scratch)
template <class T, int N>
__device__ __forceinline__ T* pick(T* const (&src)[N], int t) {
  T* p = src[0];
#pragma unroll
  for (int i = 1; i < N; i++) p = t == i ? src[i] : p;
  return p;
}

__device__ __forceinline__ float4 gather(const float* p, const PackQuad& m) {
  float4 v;
  v.x = m.off[0] >= 0 ? p[m.off[0]] : 0.0f;
  v.y = m.off[1] >= 0 ? p[m.off[1]] : 0.0f;
  v.z = m.off[2] >= 0 ? p[m.off[2]] : 0.0f;
  v.w = m.off[3] >= 0 ? p[m.off[3]] : 0.0f;
  return v;
}

// the inverse of gather: the floats that have an element go to it, padding goes nowhere
__device__ __forceinline__ void scatter(float* p, const PackQuad& m, const float4& v) {
  if (m.off[0] >= 0) p[m.off[0]] = v.x;
  if (m.off[1] >= 0) p[m.off[1]] = v.y;
  if (m.off[2] >= 0) p[m.off[2]] = v.z;
  if (m.off[3] >= 0) p[m.off[3]] = v.w;
}

__global__ void __launch_bounds__(PACK_THREADS) actor_pack_kernel(const ActorPackParams P) {
  const uint32_t q = blockIdx.x * PACK_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  const bool head = pack_quad_actor(P.d, q, m);
  if (head && !P.head) return;  // the head's floats stay as they are
  P.packed[q] = gather(pick(P.src, m.tensor), m);
}

// include/urgym.h, urgym_critic_load: packed = (packed * omt) + (tau * src), every operation rounded to float32 on its own
__device__ __forceinline__ float polyak(float old, float src, float tau, float omt) { return rounded(old * omt) + rounded(tau * src); }

__global__ void __launch_bounds__(PACK_THREADS) critic_pack_kernel(const CriticPackParams P) {
  const uint32_t q = blockIdx.x * PACK_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  pack_quad_critic(P.d, q, m);
  float4 v = gather(pick(P.src, m.tensor), m);
  if (P.blend) {  // tau == 1 never reads the old value: a load repairs a buffer that holds NaN
    const float4 o = P.packed[q];
    v.x = polyak(o.x, v.x, P.tau, P.omt);
    v.y = polyak(o.y, v.y, P.tau, P.omt);
    v.z = polyak(o.z, v.z, P.tau, P.omt);
    v.w = polyak(o.w, v.w, P.tau, P.omt);
  }
  P.packed[q] = v;
}

__global__ void __launch_bounds__(PACK_THREADS) actor_unpack_kernel(const ActorUnpackParams P) {
  const uint32_t q = blockIdx.x * PACK_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  const bool head = pack_quad_actor(P.d, q, m);
  if (head && !P.head) return;  // no destination for the head
  scatter(pick(P.dst, m.tensor), m, P.packed[q]);
}

__global__ void __launch_bounds__(PACK_THREADS) critic_unpack_kernel(const CriticUnpackParams P) {
  const uint32_t q = blockIdx.x * PACK_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  pack_quad_critic(P.d, q, m);
  scatter(pick(P.dst, m.tensor), m, P.packed[q]);
}

}  // namespace

void actor_pack_launch(const ActorPacked& a, const float* const* src, hipStream_t s) {
  ActorPackParams P;
  P.packed = reinterpret_cast<float4*>(a.weights);
  for (int i = 0; i < PACK_ACTOR_TENSORS; i++) P.src[i] = src[i];
  P.d = pack_dims_actor(a.in_features, a.hidden);
  P.quads = (uint32_t)(pack_actor_floats(P.d) / 4);
  P.head = src[PACK_W_LS] != nullptr;
  hipLaunchKernelGGL(actor_pack_kernel, dim3((P.quads + PACK_THREADS - 1) / PACK_THREADS), dim3(PACK_THREADS), 0, s, P);
}

void critic_pack_launch(const CriticPacked& c, const float* const* src, float tau, hipStream_t s) {
  CriticPackParams P;
  P.packed = reinterpret_cast<float4*>(c.weights);
  for (int i = 0; i < 2 * PACK_CRITIC_TENSORS; i++) P.src[i] = src[i];
  P.d = pack_dims_critic(c.in_features, c.hidden);
  P.quads = (uint32_t)(pack_critic_floats(P.d) / 4);
  P.blend = tau != 1.0f;
  P.tau = tau, P.omt = 1.0f - tau;
  hipLaunchKernelGGL(critic_pack_kernel, dim3((P.quads + PACK_THREADS - 1) / PACK_THREADS), dim3(PACK_THREADS), 0, s, P);
}

void actor_unpack_launch(const ActorPacked& a, float* const* dst, hipStream_t s) {
  ActorUnpackParams P;
  P.packed = reinterpret_cast<const float4*>(a.weights);
  for (int i = 0; i < PACK_ACTOR_TENSORS; i++) P.dst[i] = dst[i];
  P.d = pack_dims_actor(a.in_features, a.hidden);
  P.quads = (uint32_t)(pack_actor_floats(P.d) / 4);
  P.head = dst[PACK_W_LS] != nullptr;
  hipLaunchKernelGGL(actor_unpack_kernel, dim3((P.quads + PACK_THREADS - 1) / PACK_THREADS), dim3(PACK_THREADS), 0, s, P);
}

void critic_unpack_launch(const CriticPacked& c, float* const* dst, hipStream_t s) {
  CriticUnpackParams P;
  P.packed = reinterpret_cast<const float4*>(c.weights);
  for (int i = 0; i < 2 * PACK_CRITIC_TENSORS; i++) P.dst[i] = dst[i];
  P.d = pack_dims_critic(c.in_features, c.hidden);
  P.quads = (uint32_t)(pack_critic_floats(P.d) / 4);
  hipLaunchKernelGGL(critic_unpack_kernel, dim3((P.quads + PACK_THREADS - 1) / PACK_THREADS), dim3(PACK_THREADS), 0, s, P);
}

}  // namespace urgym
