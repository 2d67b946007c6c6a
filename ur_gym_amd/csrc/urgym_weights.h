// urgym_weights.h — seam between urgym_weights.hip (the pack kernels that reload an actor's or a critic's packed weights from device
// tensors, and the unpack kernels that write them back, compiled with the flags of urgym_actor.hip) and urgym_policy_abi.hip (the learner's entry points), beside urgym_actor.h / urgym_critic.h.
// Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "urgym_actor.h"
#include "urgym_critic.h"

namespace urgym {

// Rewrites every float of the actor's packed buffer from src[PACK_W0 .. PACK_B_OUT] (DEVICE pointers, float32, torch's [out][in]
// layout, 4-byte aligned), padding as +0.0f, in ONE launch on `s`.  src[PACK_W_LS] / src[PACK_B_LS]: both null = the log_std head's
// floats are not touched; both given = the head is written too.  The caller has validated everything.
void actor_pack_launch(const ActorPacked& a, const float* const* src, hipStream_t s);

// The same for both Q-networks (src[6 net + PACK_*]) in ONE launch.  tau == 1: packed = src, the old value is not read; otherwise
// packed = (packed * (1.0f - tau)) + (tau * src), three float32 operations each rounded on its own.
void critic_pack_launch(const CriticPacked& c, const float* const* src, float tau, hipStream_t s);

// The map the other way: every element of dst[PACK_W0 .. PACK_B_OUT] (DEVICE pointers, float32, torch's [out][in] layout, 4-byte
// aligned) is written from the one packed float that holds it, as a single-float store, in ONE launch on `s`; padding writes nothing,
// and every bit pattern goes through unchanged.  dst[PACK_W_LS] / dst[PACK_B_LS]: both null = the head is skipped; both given = it is
// written too.  No allocation, no synchronisation.  The caller has validated everything.
void actor_unpack_launch(const ActorPacked& a, float* const* dst, hipStream_t s);

// The same for both Q-networks (dst[6 net + PACK_*], all twelve required) in ONE launch.
void critic_unpack_launch(const CriticPacked& c, float* const* dst, hipStream_t s);

}  // namespace urgym
