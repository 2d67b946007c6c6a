// urgym_pack_host.h — the host packing loops of urgym_actor_create, urgym_actor_set_log_std and urgym_critic_create, moved here word
// for word so that a host program (tests/pack_harness.cpp) can call what the library calls.  They are the yardstick the device pack
// kernels (urgym_weights.hip, through the map of urgym_pack_map.h) are checked against, and are deliberately NOT written in terms
// of that map.  Plain C++: no HIP.
#pragma once
#include <stddef.h>
#include <vector>

#include "../../include/urgym.h"

namespace urgym {

// p1 | p2 | small of an actor, the log_std head left zero; returns the offsets of p2 and small in floats
inline std::vector<float> pack_actor_host(const urgym_actor_desc* d, size_t* p2_off, size_t* small_off) {
  constexpr int IN_PAD = 48, L1_STEPS4 = IN_PAD / 8, L1_TILE4 = L1_STEPS4 * 64;
  const int H = d->hidden_width, in = d->in_features;
  const int HP = (H + 127) / 128 * 128, HT = HP / 32;
  const size_t n1 = (size_t)HT * L1_TILE4 * 4, n2 = (size_t)HT * HT * 4 * 64 * 4, ns = (size_t)HP * 14 + 16;
  *p2_off = n1, *small_off = n1 + n2;
  std::vector<float> w(n1 + n2 + ns, 0.0f);
  // layer 1: float c of lane l's read sq of tile t = W0[32 t + (l & 31)][2 (4 sq + c) + (l >> 5)]
  for (int t = 0; t < HT; t++)
    for (int sq = 0; sq < L1_STEPS4; sq++)
      for (int l = 0; l < 64; l++)
        for (int c = 0; c < 4; c++) {
          const int n = 32 * t + (l & 31), k = 2 * (4 * sq + c) + (l >> 5);
          if (n < H && k < in) w[((((size_t)t * L1_STEPS4 + sq) * 64 + l) * 4) + c] = d->w0[(size_t)n * in + k];
        }
  // layer 2: read sq = 4 u + g of tile t pairs, in float c, the neurons 32 u + 8 g + 4 (l >> 5) + c of layer 1
  for (int t = 0; t < HT; t++)
    for (int sq = 0; sq < HT * 4; sq++)
      for (int l = 0; l < 64; l++)
        for (int c = 0; c < 4; c++) {
          const int n = 32 * t + (l & 31), k = 32 * (sq / 4) + 8 * (sq % 4) + 4 * (l >> 5) + c;
          if (n < H && k < H) w[n1 + ((((size_t)t * HT * 4 + sq) * 64 + l) * 4) + c] = d->w1[(size_t)n * H + k];
        }
  float* sm = w.data() + n1 + n2;
  for (int n = 0; n < H; n++) {
    sm[n] = d->b0[n];
    sm[HP + n] = d->b1[n];
    for (int o = 0; o < 6; o++) sm[2 * HP + ((size_t)(n / 4) * 6 + o) * 4 + n % 4] = d->w_mu[(size_t)o * H + n];
  }
  for (int o = 0; o < 6; o++) sm[(size_t)HP * 8 + o] = d->b_mu[o];
  return w;
}

// the log_std head of an actor of width H, HP = its padded width: the 6 HP + 8 floats at small + 8 HP + 8
inline std::vector<float> pack_log_std_host(int H, int HP, const float* w_ls, const float* b_ls) {
  std::vector<float> head((size_t)HP * 6 + 8, 0.0f);  // w_log_std in w_mu's packing [neuron / 4][6][neuron % 4], then the bias
  for (int n = 0; n < H; n++)
    for (int o = 0; o < 6; o++) head[((size_t)(n / 4) * 6 + o) * 4 + n % 4] = w_ls[(size_t)o * H + n];
  for (int o = 0; o < 6; o++) head[(size_t)HP * 6 + o] = b_ls[o];
  return head;
}

// both networks' packed layers, then both networks' small arrays; returns the offset of the small arrays in floats
inline std::vector<float> pack_critic_host(const urgym_critic_desc* d, size_t* small_off) {
  constexpr int CIN_PAD = 56, C1_STEPS4 = CIN_PAD / 8, C1_TILE4 = C1_STEPS4 * 64;
  const int H = d->hidden_width, in = d->in_features;
  const int HP = (H + 127) / 128 * 128, HT = HP / 32;
  const size_t n1 = (size_t)HT * C1_TILE4 * 4, n2 = (size_t)HT * HT * 4 * 64 * 4, ns = (size_t)HP * 3 + 4;
  *small_off = 2 * (n1 + n2);
  std::vector<float> w(2 * (n1 + n2 + ns), 0.0f);
  for (int net = 0; net < 2; net++) {
    const urgym_q_network& q = d->qf[net];
    float* w1 = w.data() + (size_t)net * (n1 + n2);
    float* w2 = w1 + n1;
    // layer 1: float c of lane l's read sq of tile t = W0[32 t + (l & 31)][2 (4 sq + c) + (l >> 5)]
    for (int t = 0; t < HT; t++)
      for (int sq = 0; sq < C1_STEPS4; sq++)
        for (int l = 0; l < 64; l++)
          for (int cc = 0; cc < 4; cc++) {
            const int n = 32 * t + (l & 31), k = 2 * (4 * sq + cc) + (l >> 5);
            if (n < H && k < in) w1[((((size_t)t * C1_STEPS4 + sq) * 64 + l) * 4) + cc] = q.w0[(size_t)n * in + k];
          }
    // layer 2: read sq = 4 u + g of tile t pairs, in float c, the neurons 32 u + 8 g + 4 (l >> 5) + c of layer 1
    for (int t = 0; t < HT; t++)
      for (int sq = 0; sq < HT * 4; sq++)
        for (int l = 0; l < 64; l++)
          for (int cc = 0; cc < 4; cc++) {
            const int n = 32 * t + (l & 31), k = 32 * (sq / 4) + 8 * (sq % 4) + 4 * (l >> 5) + cc;
            if (n < H && k < H) w2[((((size_t)t * HT * 4 + sq) * 64 + l) * 4) + cc] = q.w1[(size_t)n * H + k];
          }
    float* sm = w.data() + *small_off + (size_t)net * ns;
    for (int n = 0; n < H; n++) sm[n] = q.b0[n], sm[HP + n] = q.b1[n], sm[2 * HP + n] = q.w_q[n];
    sm[3 * HP] = q.b_q[0];
  }
  return w;
}

}  // namespace urgym
