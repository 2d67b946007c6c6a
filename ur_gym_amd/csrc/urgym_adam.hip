// urgym_adam.hip — Adam on the device (include/urgym.h, urgym_actor_adam_step / urgym_critic_adam_step): one launch steps every
// parameter tensor of an actor, or of the twin critics, in place and writes the packed buffer the kernels read from the stepped
// values -- what a learner that keeps its parameters in torch otherwise does with an optimiser's train of launches followed by a
// reload (urgym_weights.hip), and for the target critic a second, blending reload.
//
// One lane handles one float4 ("quad") of the packed buffer, exactly as in the pack kernels: urgym_pack_map.h names the quad's source
// tensor and four offsets (or padding).  The map is a bijection between the elements of the source tensors and the non-padding floats of
// the buffer (tests/adam_harness.cpp checks that direction), so a lane that steps the elements its quad names steps every element
// exactly once, and no two lanes touch the same element: no ordering between lanes is needed.  For every offset >= 0 the lane loads p,
// g, m, v as single floats (nothing beyond 4-byte alignment is assumed), runs adam_element of urgym_adam.h and stores p', m', v'; then
// it writes the quad as one float4, consecutive lanes at consecutive addresses.  In layer 2 (the bulk) a workgroup consumes 32 rows x
// 128 contiguous bytes of each of the four tensors, as the pack kernels do of one.
//
// This unit is built with -ffp-contract=off: every line of adam_element and of the blend is one operation rounded on its own, with no
// device to keep the compiler from fusing them.  Division and square root are the correctly rounded ones (hipcc's default), and the
// unit's float32 denormal mode keeps subnormals.
//
// The clipped steps (actor_adam_scaled_kernel, critic_adam_scaled_kernel) are the same two bodies with the
// element of urgym_grad_clip.h: separate kernels, so that the device code of the two unclipped ones is what it was without them.
#include <hip/hip_runtime.h>

#include "urgym_adam.h"
#include "urgym_grad_clip.h"
#include "urgym_pack_map.h"

namespace urgym {

namespace {

constexpr int ADAM_THREADS = 256;

struct ActorAdamParams {
  float4* packed;
  AdamTensors<PACK_ACTOR_TENSORS> t;
  PackDims d;
  uint32_t quads;  // float4 in the buffer
  AdamCoef c;
};

struct CriticAdamParams {
  float4* online;
  float4* target;  // or null
  AdamTensors<2 * PACK_CRITIC_TENSORS> t;
  PackDims d;
  uint32_t quads;
  int blend;       // target given and tau != 1
  float tau, omt;  // omt = 1.0f - tau, formed on the host
  AdamCoef c;
};

// src[t] without indexing the kernel arguments by a per-lane value (which would put them in scratch): a chain of selects
template <class T, int N>
__device__ __forceinline__ T* pick(T* const (&src)[N], int t) {
  T* p = src[0];
#pragma unroll
  for (int i = 1; i < N; i++) p = t == i ? src[i] : p;
  return p;
}

// steps the four elements quad `m` names and returns the quad of the packed buffer: p' where an offset is given, +0.0f where not.
// SCALED: the element of urgym_grad_clip.h, gs = g * scale first (the clipped steps); otherwise `scale` is not looked at.
template <int N, bool SCALED = false>
__device__ __forceinline__ float4 step_quad(const AdamTensors<N>& t, const PackQuad& m, const AdamCoef& c, float scale = 1.0f) {
  float* const p = pick(t.param, m.tensor);
  const float* const g = pick(t.grad, m.tensor);
  float* const ea = pick(t.exp_avg, m.tensor);
  float* const es = pick(t.exp_avg_sq, m.tensor);
  float out[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    out[k] = 0.0f;
    const int o = m.off[k];
    if (o >= 0) {
      float pv = p[o], mv = ea[o], vv = es[o];
      if (SCALED)
        adam_element_scaled(c, g[o], scale, pv, mv, vv);
      else
        adam_element(c, g[o], pv, mv, vv);
      p[o] = pv, ea[o] = mv, es[o] = vv;
      out[k] = pv;
    }
  }
  return make_float4(out[0], out[1], out[2], out[3]);
}

__global__ void __launch_bounds__(ADAM_THREADS) actor_adam_kernel(const ActorAdamParams P) {
  const uint32_t q = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  pack_quad_actor(P.d, q, m);  // the head is written like the rest
  P.packed[q] = step_quad(P.t, m, P.c);
}

// include/urgym.h, urgym_critic_load: packed = (packed * omt) + (tau * src), every operation rounded to float32 on its own
__device__ __forceinline__ float polyak(float old, float src, float tau, float omt) {
  const float a = old * omt;
  const float b = tau * src;
  return a + b;
}

__global__ void __launch_bounds__(ADAM_THREADS) critic_adam_kernel(const CriticAdamParams P) {
  const uint32_t q = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  PackQuad m;
  pack_quad_critic(P.d, q, m);
  float4 v = step_quad(P.t, m, P.c);
  P.online[q] = v;
  if (!P.target) return;
  if (P.blend) {  // tau == 1 never reads the old value
    const float4 o = P.target[q];
    v.x = polyak(o.x, v.x, P.tau, P.omt);
    v.y = polyak(o.y, v.y, P.tau, P.omt);
    v.z = polyak(o.z, v.z, P.tau, P.omt);
    v.w = polyak(o.w, v.w, P.tau, P.omt);
  }
  P.target[q] = v;
}

// The clipped steps (include/urgym.h, urgym_actor_adam_step_scaled / urgym_critic_adam_step_scaled): the two kernels above, line for
// line, with the clip coefficient -- a DEVICE scalar a urgym_*_grad_norm launch earlier on the stream wrote -- read once per lane and
// every gradient element multiplied by it as it is read.  Kernels of their own: the two above are not touched by their existence.
struct ActorAdamScaledParams {
  ActorAdamParams p;
  const float* scale;
};

struct CriticAdamScaledParams {
  CriticAdamParams p;
  const float* scale;
};

__global__ void __launch_bounds__(ADAM_THREADS) actor_adam_scaled_kernel(const ActorAdamScaledParams S) {
  const ActorAdamParams& P = S.p;
  const uint32_t q = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  const float scale = S.scale[0];
  PackQuad m;
  pack_quad_actor(P.d, q, m);
  P.packed[q] = step_quad<PACK_ACTOR_TENSORS, true>(P.t, m, P.c, scale);
}

__global__ void __launch_bounds__(ADAM_THREADS) critic_adam_scaled_kernel(const CriticAdamScaledParams S) {
  const CriticAdamParams& P = S.p;
  const uint32_t q = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (q >= P.quads) return;
  const float scale = S.scale[0];
  PackQuad m;
  pack_quad_critic(P.d, q, m);
  float4 v = step_quad<2 * PACK_CRITIC_TENSORS, true>(P.t, m, P.c, scale);
  P.online[q] = v;
  if (!P.target) return;
  if (P.blend) {  // tau == 1 never reads the old value
    const float4 o = P.target[q];
    v.x = polyak(o.x, v.x, P.tau, P.omt);
    v.y = polyak(o.y, v.y, P.tau, P.omt);
    v.z = polyak(o.z, v.z, P.tau, P.omt);
    v.w = polyak(o.w, v.w, P.tau, P.omt);
  }
  P.target[q] = v;
}

}  // namespace

void actor_adam_launch(const ActorPacked& a, const AdamTensors<PACK_ACTOR_TENSORS>& t, const AdamCoef& c, hipStream_t s) {
  ActorAdamParams P;
  P.packed = reinterpret_cast<float4*>(a.weights);
  P.t = t;
  P.d = pack_dims_actor(a.in_features, a.hidden);
  P.quads = (uint32_t)(pack_actor_floats(P.d) / 4);
  P.c = c;
  hipLaunchKernelGGL(actor_adam_kernel, dim3((P.quads + ADAM_THREADS - 1) / ADAM_THREADS), dim3(ADAM_THREADS), 0, s, P);
}

void critic_adam_launch(const CriticPacked& online, const CriticPacked* target, const AdamTensors<2 * PACK_CRITIC_TENSORS>& t, const AdamCoef& c,
                        float tau, hipStream_t s) {
  CriticAdamParams P;
  P.online = reinterpret_cast<float4*>(online.weights);
  P.target = target ? reinterpret_cast<float4*>(target->weights) : nullptr;
  P.t = t;
  P.d = pack_dims_critic(online.in_features, online.hidden);
  P.quads = (uint32_t)(pack_critic_floats(P.d) / 4);
  P.blend = target && tau != 1.0f;
  P.tau = target ? tau : 1.0f, P.omt = 1.0f - P.tau;
  P.c = c;
  hipLaunchKernelGGL(critic_adam_kernel, dim3((P.quads + ADAM_THREADS - 1) / ADAM_THREADS), dim3(ADAM_THREADS), 0, s, P);
}

void actor_adam_scaled_launch(const ActorPacked& a, const AdamTensors<PACK_ACTOR_TENSORS>& t, const AdamCoef& c, const float* scale, hipStream_t s) {
  ActorAdamScaledParams S;
  ActorAdamParams& P = S.p;
  P.packed = reinterpret_cast<float4*>(a.weights);
  P.t = t;
  P.d = pack_dims_actor(a.in_features, a.hidden);
  P.quads = (uint32_t)(pack_actor_floats(P.d) / 4);
  P.c = c;
  S.scale = scale;
  hipLaunchKernelGGL(actor_adam_scaled_kernel, dim3((P.quads + ADAM_THREADS - 1) / ADAM_THREADS), dim3(ADAM_THREADS), 0, s, S);
}

void critic_adam_scaled_launch(const CriticPacked& online, const CriticPacked* target, const AdamTensors<2 * PACK_CRITIC_TENSORS>& t, const AdamCoef& c,
                               float tau, const float* scale, hipStream_t s) {
  CriticAdamScaledParams S;
  CriticAdamParams& P = S.p;
  P.online = reinterpret_cast<float4*>(online.weights);
  P.target = target ? reinterpret_cast<float4*>(target->weights) : nullptr;
  P.t = t;
  P.d = pack_dims_critic(online.in_features, online.hidden);
  P.quads = (uint32_t)(pack_critic_floats(P.d) / 4);
  P.blend = target && tau != 1.0f;
  P.tau = target ? tau : 1.0f, P.omt = 1.0f - P.tau;
  P.c = c;
  S.scale = scale;
  hipLaunchKernelGGL(critic_adam_scaled_kernel, dim3((P.quads + ADAM_THREADS - 1) / ADAM_THREADS), dim3(ADAM_THREADS), 0, s, S);
}

}  // namespace urgym
