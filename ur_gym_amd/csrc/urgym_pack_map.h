// urgym_pack_map.h — where every float of a packed weight buffer comes from: the inverse of the host packing loops of
// urgym_pack_host.h (actor_create / actor_set_log_std / critic_create), stated once as __host__ __device__ functions.  The pack
// kernels of urgym_weights.hip run it on the device; tests/pack_harness.cpp runs it on the host, against those loops.
//
// A buffer is addressed in QUADS of 4 floats (one float4, one lane of a pack kernel).  Every region of both layouts starts and ends
// on a multiple of 4 floats, so a quad has ONE source tensor; its four floats sit at four offsets of it, or are padding (+0.0f).
//
//   actor   p1 [HT][6][64][4] | p2 [HT][4 HT][64][4] | small: b0[HP] | b1[HP] | w_mu [HP/4][6][4] | b_mu[8] | w_ls [HP/4][6][4] | b_ls[8]
//   critic  net 0: p1 [HT][7][64][4] | p2 [HT][4 HT][64][4];  net 1: the same;  then per net small: b0[HP] | b1[HP] | w_q[HP] | b_q, 0, 0, 0
//   HP = hidden width padded to a multiple of 128, HT = HP / 32.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define URGYM_HD __host__ __device__
#else
#define URGYM_HD
#endif

namespace urgym {

constexpr int PACK_ACTOR_STEPS4 = 6;   // float4 reads per lane and layer-1 tile of the actor (K padded to 48)
constexpr int PACK_CRITIC_STEPS4 = 7;  // the critic's (K padded to 56)

// source tensors of a network, in the order of the descriptors of include/urgym.h
enum { PACK_W0 = 0, PACK_B0, PACK_W1, PACK_B1, PACK_W_OUT, PACK_B_OUT, PACK_W_LS, PACK_B_LS, PACK_ACTOR_TENSORS };
constexpr int PACK_CRITIC_TENSORS = 6;  // per network: W0 b0 W1 b1 w_q b_q; tensor id = 6 net + PACK_*

struct PackDims {
  int in, H, HT, HP, steps4;
  size_t n1, n2, ns;  // floats of layer 1, layer 2 and small of ONE network
};

URGYM_HD inline PackDims pack_dims_actor(int in, int H) {
  PackDims d;
  d.in = in, d.H = H, d.HP = (H + 127) / 128 * 128, d.HT = d.HP / 32, d.steps4 = PACK_ACTOR_STEPS4;
  d.n1 = (size_t)d.HT * d.steps4 * 64 * 4, d.n2 = (size_t)d.HT * d.HT * 4 * 64 * 4, d.ns = (size_t)d.HP * 14 + 16;
  return d;
}
URGYM_HD inline PackDims pack_dims_critic(int in, int H) {
  PackDims d = pack_dims_actor(in, H);
  d.steps4 = PACK_CRITIC_STEPS4;
  d.n1 = (size_t)d.HT * d.steps4 * 64 * 4, d.ns = (size_t)d.HP * 3 + 4;
  return d;
}
URGYM_HD inline size_t pack_actor_floats(const PackDims& d) { return d.n1 + d.n2 + d.ns; }
URGYM_HD inline size_t pack_critic_floats(const PackDims& d) { return 2 * (d.n1 + d.n2 + d.ns); }
// the log_std head of the actor's small array, in floats from the start of small: [begin, end)
URGYM_HD inline size_t pack_actor_head_begin(const PackDims& d) { return (size_t)d.HP * 8 + 8; }

struct PackQuad {
  int tensor;  // PACK_* (the critic: 6 net + PACK_*); meaningless when all four offsets are negative
  int off[4];  // element of that tensor, or < 0: the float is padding, +0.0f
};

// quad q of a packed layer 1, [HT][steps4][64 lanes][4]: float c of lane l's read sq of tile t = W0[32 t + (l & 31)][2 (4 sq + c) + (l >> 5)]
URGYM_HD inline void pack_quad_layer1(const PackDims& d, uint32_t q, PackQuad& out) {
  const int l = (int)(q & 63u), r = (int)(q >> 6), sq = r % d.steps4, t = r / d.steps4;
  const int n = 32 * t + (l & 31);
  out.tensor = PACK_W0;
  _Pragma("unroll") for (int c = 0; c < 4; c++) {
    const int k = 2 * (4 * sq + c) + (l >> 5);
    out.off[c] = (n < d.H && k < d.in) ? n * d.in + k : -1;
  }
}

// quad q of a packed layer 2, [HT][4 HT][64 lanes][4]: read sq = 4 u + g of tile t pairs, in float c, neuron 32 u + 8 g + 4 (l >> 5) + c
URGYM_HD inline void pack_quad_layer2(const PackDims& d, uint32_t q, PackQuad& out) {
  const int l = (int)(q & 63u), r = (int)(q >> 6), sq = r % (d.HT * 4), t = r / (d.HT * 4);
  const int n = 32 * t + (l & 31), k0 = 32 * (sq / 4) + 8 * (sq % 4) + 4 * (l >> 5);
  out.tensor = PACK_W1;
  _Pragma("unroll") for (int c = 0; c < 4; c++) out.off[c] = (n < d.H && k0 + c < d.H) ? n * d.H + k0 + c : -1;
}

// a head in w_mu's packing, [HP / 4][6][4] then 8 floats of bias; i = first float of the quad within the head
URGYM_HD inline void pack_quad_head(const PackDims& d, int i, int w_tensor, int b_tensor, PackQuad& out) {
  if (i < d.HP * 6) {
    const int r = i >> 2, o = r % 6, n4 = r / 6;
    out.tensor = w_tensor;
    _Pragma("unroll") for (int c = 0; c < 4; c++) out.off[c] = (4 * n4 + c < d.H) ? o * d.H + 4 * n4 + c : -1;
  } else {
    out.tensor = b_tensor;
    _Pragma("unroll") for (int c = 0; c < 4; c++) out.off[c] = (i - d.HP * 6 + c < 6) ? i - d.HP * 6 + c : -1;
  }
}

URGYM_HD inline void pack_quad_bias(const PackDims& d, int n0, int tensor, PackQuad& out) {
  out.tensor = tensor;
  _Pragma("unroll") for (int c = 0; c < 4; c++) out.off[c] = (n0 + c < d.H) ? n0 + c : -1;
}

// Quad q of the actor's buffer.  Returns true where the quad belongs to the log_std head (written only when the head is given).
URGYM_HD inline bool pack_quad_actor(const PackDims& d, uint32_t q, PackQuad& out) {
  const uint32_t q1 = (uint32_t)(d.n1 / 4), q2 = (uint32_t)(d.n2 / 4);
  if (q < q1) return pack_quad_layer1(d, q, out), false;
  if (q < q1 + q2) return pack_quad_layer2(d, q - q1, out), false;
  const int i = (int)(q - q1 - q2) * 4, HP = d.HP;
  if (i < HP) return pack_quad_bias(d, i, PACK_B0, out), false;
  if (i < 2 * HP) return pack_quad_bias(d, i - HP, PACK_B1, out), false;
  if (i < 8 * HP + 8) return pack_quad_head(d, i - 2 * HP, PACK_W_OUT, PACK_B_OUT, out), false;
  return pack_quad_head(d, i - (8 * HP + 8), PACK_W_LS, PACK_B_LS, out), true;
}

// Quad q of the critic's buffer (both networks); out.tensor = 6 net + PACK_*.
URGYM_HD inline void pack_quad_critic(const PackDims& d, uint32_t q, PackQuad& out) {
  const uint32_t q1 = (uint32_t)(d.n1 / 4), q2 = (uint32_t)(d.n2 / 4), qs = (uint32_t)(d.ns / 4);
  int net;
  if (q < 2 * (q1 + q2)) {
    net = q >= q1 + q2;
    q -= (uint32_t)net * (q1 + q2);
    if (q < q1) pack_quad_layer1(d, q, out);
    else pack_quad_layer2(d, q - q1, out);
  } else {
    q -= 2 * (q1 + q2);
    net = q >= qs;
    const int i = (int)(q - (uint32_t)net * qs) * 4, HP = d.HP;
    if (i < HP) pack_quad_bias(d, i, PACK_B0, out);
    else if (i < 2 * HP) pack_quad_bias(d, i - HP, PACK_B1, out);
    else if (i < 3 * HP) pack_quad_bias(d, i - 2 * HP, PACK_W_OUT, out);
    else {
      out.tensor = PACK_B_OUT;
      _Pragma("unroll") for (int c = 0; c < 4; c++) out.off[c] = c == 0 ? 0 : -1;
    }
  }
  out.tensor += PACK_CRITIC_TENSORS * net;
}

}  // namespace urgym
