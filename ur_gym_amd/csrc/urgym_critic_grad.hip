// urgym_critic_grad.hip — the gradient of the twin Q-networks with respect to the ACTION, d q_i / d a and d min(q_0, q_1) / d a, as one
// HIP kernel for MI355X (gfx950): what the actor loss of SAC needs from the critic (include/urgym.h, urgym_critic_action_gradient).
// Per row and network
//
//   g_i = W0_i[:, action columns]^T  D1_i  W1_i^T  D2_i  w_q,i          D = diag(pre-activation > 0)
//
// -- no sum over the rows of the batch, so a row's result depends on nothing but the row, like everything in urgym_critic.hip.  The
// kernel reads the critic's packed buffer as it is (urgym_pack_map.h) and keeps critic_kernel's conventions (urgym_critic.hip:1-21):
// 4 waves of 32 rows, v_mfma_f32_32x32x2_f32, the SAME wave runs qf0 and then qf1, the inputs are gathered once.  Per network:
//
//   forward    critic_kernel's, operation for operation (q is bitwise urgym_critic_evaluate's); of the two hidden layers only the
//              ReLU masks are kept, as BITS: 16 HT per lane and layer, bit = pre-activation > 0.
//   layer 2    a second pass over the network's layer-2 tiles.  With tile t staged (output neurons 32 t .. 32 t + 31, all inputs j),
//              dh1[j] += sum_n W1[n][j] (mask2[n] ? w_q[n] : 0): the B operand of step (g, r) is rebuilt from the mask bits and w_q
//              and sits on the lane that produced z2 of neuron 32 t + 8 g + 4 h + r, the A operand is the tile TRANSPOSED.  All HT
//              output tiles accumulate at once (16 HT accumulators; affordable because h1 is bits by now).
//   layer 1    only the six action columns of W0 (feature in_features - 6 + c), picked out of the packed layer-1 tiles once per
//              workgroup and network into LDS [6][HP]: da[c] = sum_j W0[j][c] (mask1[j] ? dh1[j] : 0), 6 * 16 HT fma per lane and one
//              cross-lane add.
//
// The staged double buffer, the forward and backward MFMA blocks, the mask words and the transposed A operand with its padded LDS image are
// urgym_mlp_grad.h's, shared with the two parameter-gradient units; what is written out here is what this kernel alone does.
//
// This unit may contract a * b + c to fma, like urgym_critic.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "urgym_critic.h"
#include "urgym_mlp_grad.h"

namespace urgym {

namespace {

using namespace mlp_grad;

// critic_kernel's geometry: urgym_critic.h states it once and both units assert it
constexpr int CRITIC_THREADS = CRITIC_GEOMETRY_THREADS;  // 4 waves
constexpr int CRITIC_ROWS = CRITIC_GEOMETRY_ROWS;        // rows per workgroup (32 per wave)
constexpr int CIN_PAD = CRITIC_GEOMETRY_CIN_PAD;         // layer-1 K, padded with zero weights (in_features <= 53)
constexpr int C1_STEPS4 = CIN_PAD / 8;
constexpr int C1_TILE4 = C1_STEPS4 * 64;
constexpr int C1_CHUNK4 = 4 * C1_TILE4;

struct CriticGradKParams {
  const float4* w;      // the critic's packed layers (CriticKParams of urgym_critic.hip)
  const float4* small;  // per network: b0[HP] | b1[HP] | w_q[HP] | b_q, 0, 0, 0
  int in_features;
  CriticGradCall call;
};

__device__ __forceinline__ float grad_feature(const CriticGradCall& C, size_t m, int k) {
  const int gd = C.goal_dim;
  if (k < gd) return C.achieved_goal[m * gd + k];
  if (k < 2 * gd) return C.desired_goal[m * gd + (k - gd)];
  k -= 2 * gd;
  if (k < C.obs_dim) return C.observation[m * C.obs_dim + k];
  k -= C.obs_dim;
  return k < 6 ? C.action[m * 6 + k] : 0.0f;
}

template <int HT>
__global__ void __launch_bounds__(CRITIC_THREADS, (HT <= 4 ? 2 : 1)) critic_grad_kernel(const CriticGradKParams P) {
  constexpr int HP = HT * 32;
  constexpr int L2_TILE4 = HT * 4 * 64;        // float4 per packed layer-2 tile
  constexpr int L2_IMAGE4 = HT * 4 * L2_ROW4;  // float4 of its staged image
  constexpr int BUF4 = C1_CHUNK4 > L2_IMAGE4 ? C1_CHUNK4 : L2_IMAGE4;
  constexpr int NET4 = HT * C1_TILE4 + HT * L2_TILE4;
  constexpr int SMALL4 = (3 * HP + 4) / 4;
  constexpr int L1_CHUNKS = HT / 4;
  constexpr int PF1 = C1_CHUNK4 / CRITIC_THREADS, PF2 = L2_TILE4 / CRITIC_THREADS;  // float4 per thread and staged chunk (7, HT)
  constexpr int MW = HT / 2;                                                        // mask words per layer: two tiles of 16 bits each
  __shared__ float4 wbuf[2][BUF4];
  __shared__ float4 small4[2 * SMALL4];
  __shared__ float4 wact4[6 * HP / 4];  // the action columns of the network in hand: [6][HP]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CriticGradCall& C = P.call;
  const int M = C.M;
  const size_t row0 = (size_t)blockIdx.x * CRITIC_ROWS;

  for (int i = tid; i < 2 * SMALL4; i += CRITIC_THREADS) small4[i] = P.small[i];
#pragma unroll
  for (int i = 0; i < PF1; i++) wbuf[0][tid + CRITIC_THREADS * i] = P.w[tid + CRITIC_THREADS * i];

  const int h = lane >> 5;
  const size_t row = row0 + wave * 32 + (lane & 31);
  const bool live = row < (size_t)M;
  const size_t m = live ? row : (size_t)M - 1;  // lanes past the end compute on the last row and store nothing
  // this lane in the staged images (urgym_mlp_grad.h: Lane)
  const int ai = lane & 31, jj = 8 * (ai >> 3) + 2 * (ai & 3) + ((ai >> 2) & 1);
  const int abase = (jj >> 1) * L2_ROW4 + (jj & 1) * 33 + 4 * h;
  const int sbase = l2_slot(tid >> 6, tid & 63);
  const Lane L = {tid, lane, h, abase, sbase};

  const float* small = reinterpret_cast<const float*>(small4);
  float* wact = reinterpret_cast<float*>(wact4);
  float qv0 = 0.0f, qv1 = 0.0f;
  float da0[6], da1[6];
#pragma unroll
  for (int c = 0; c < 6; c++) da0[c] = 0.0f, da1[c] = 0.0f;
  int buf = 0;  // the half of wbuf that holds the chunk in use

#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    const float4* p1 = P.w + (size_t)net * NET4;
    const float4* p2 = p1 + HT * C1_TILE4;
    const float4* sm4 = small4 + net * SMALL4;

    // ---- the action columns: W0[n][k], k = in_features - 6 + c, is float (k >> 1) & 3 of read row k >> 3, lane 32 (k & 1) + (n & 31)
    // of layer-1 tile n >> 5.  The first barrier below separates these stores from the other network's reads, the later ones from ours.
    if (net) __syncthreads();
    {
      const float* w1f = reinterpret_cast<const float*>(p1);
      for (int i = tid; i < 6 * HP; i += CRITIC_THREADS) {
        const int c = i / HP, n = i - c * HP, k = P.in_features - 6 + c;
        wact[i] = w1f[((((n >> 5) * C1_STEPS4 + (k >> 3)) * 64 + 32 * (k & 1) + (n & 31)) << 2) + ((k >> 1) & 3)];
      }
    }
    if (!net) __syncthreads();  // small4, the first chunk

    // this lane's B operands of layer 1 (critic_kernel's xb), gathered per network: they are dead after layer 1, and 28 registers that
    // live through both networks are 28 spilled ones at HT = 16.  The row index is made opaque so that the gather stays in the loop.
    uint32_t mrow = (uint32_t)m;
    formed(mrow);
    float xb[CIN_PAD / 2];
#pragma unroll
    for (int s = 0; s < CIN_PAD / 2; s++) xb[s] = grad_feature(C, (size_t)mrow, 2 * s + h);

    uint32_t m1[MW], m2[MW];
#pragma unroll
    for (int i = 0; i < MW; i++) m1[i] = 0, m2[i] = 0;

    // ---- layer 1 forward (critic_kernel's); h1 lives until layer 2 has run forward, its mask beyond
    float h1[HT * 16];
    // chunk c of four tiles; meanwhile the next chunk travels: another of layer 1 or, after the last, layer-2 tile 0
    auto chunk1 = [&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      constexpr bool LAST = c + 1 == L1_CHUNKS;
      constexpr int NPF = LAST ? PF2 : PF1;
      const float4* wb = wbuf[buf];
      staged<CRITIC_THREADS, NPF, LAST, float4>(wbuf, buf, L, (LAST ? p2 : p1 + (c + 1) * C1_CHUNK4) + tid, [&](auto sg) __attribute__((always_inline)) {
        constexpr int tt = decltype(sg)::value;
        layer1_tile<C1_STEPS4, tt, 4 * c + tt, HT>(wb, sm4, L, xb, h1, m1);
      });
    };
    chunk1(std::integral_constant<int, 0>());
    if constexpr (L1_CHUNKS > 1) chunk1(std::integral_constant<int, 1>());
    if constexpr (L1_CHUNKS > 2) chunk1(std::integral_constant<int, 2>());
    if constexpr (L1_CHUNKS > 3) chunk1(std::integral_constant<int, 3>());

    // ---- layer 2 forward tile by tile, each tile straight into layer 3 (critic_kernel's); the tile after it travels meanwhile
    float qsum = 0.0f;
    auto fwd2 = [&](int t, const float4* next) __attribute__((always_inline)) {
      const float4* wb = wbuf[buf] + lane + h;
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 b = sm4[(HP + 32 * t + 8 * g + 4 * h) / 4];
        acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
      }
      staged<CRITIC_THREADS, PF2, true, float4>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
        layer2_forward_quarter<HT, decltype(sg)::value>(wb, h1, acc);
      });
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 w = sm4[(2 * HP + 32 * t + 8 * g + 4 * h) / 4];
        qsum = fmaf(w.x, fmaxf(acc[4 * g + 0], 0.0f), qsum);
        qsum = fmaf(w.y, fmaxf(acc[4 * g + 1], 0.0f), qsum);
        qsum = fmaf(w.z, fmaxf(acc[4 * g + 2], 0.0f), qsum);
        qsum = fmaf(w.w, fmaxf(acc[4 * g + 3], 0.0f), qsum);
      }
      uint32_t bits = relu_bits(acc) << (16 * (t & 1));
      formed(bits);
#pragma unroll
      for (int i = 0; i < MW; i++) m2[i] |= (t >> 1) == i ? bits : 0u;  // (a register array takes no run-time index)
    };
#pragma unroll 1
    for (int t = 0; t < HT; t++)  // after the last tile: tile 0 again, for the way back
      fwd2(t, p2 + (size_t)(t + 1 < HT ? t + 1 : 0) * L2_TILE4 + tid);
    // the two lane halves hold partial sums over different neurons
    const float qn = qsum + __shfl_xor(qsum, 32) + small[net * (SMALL4 * 4) + 3 * HP];
    if (net == 0) qv0 = qn; else qv1 = qn;

    // ---- layer 2 backward: dh1 = W1^T (mask2 ? w_q : 0), tile by tile again; accumulator 4 U + c, register v: neuron 128 U + 8 v + 4 h + c
    f32x16 dacc[HT];
#pragma unroll
    for (int u = 0; u < HT; u++)
#pragma unroll
      for (int v = 0; v < 16; v++) dacc[u][v] = 0.0f;
    auto back2 = [&](int t, const float4* next, auto npf, auto next_is_tile) __attribute__((always_inline)) {
      const uint32_t bits = mask_tile(m2, t);
      const float4* wb = wbuf[buf] + abase;
      staged<CRITIC_THREADS, decltype(npf)::value, decltype(next_is_tile)::value, float4>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
        constexpr int g = decltype(sg)::value;
        const float4 wq = sm4[(2 * HP + 32 * t + 8 * g + 4 * h) / 4];
        const float wqr[4] = {wq.x, wq.y, wq.z, wq.w};
        layer2_backward_quarter<HT, g>(wb, [&](int r) __attribute__((always_inline)) { return (bits >> (4 * g + r)) & 1u ? wqr[r] : 0.0f; }, dacc);
      });
    };
#pragma unroll 1
    for (int t = 0; t + 1 < HT; t++) back2(t, p2 + (size_t)(t + 1) * L2_TILE4 + tid, std::integral_constant<int, PF2>(), std::true_type());
    // The last tile stages the other network's first layer-1 chunk: qf1's for qf0; qf0's again for qf1, which nobody reads (loads and
    // stores without a condition stay in registers, urgym_critic.hip).
    back2(HT - 1, P.w + (net == 0 ? NET4 : 0) + tid, std::integral_constant<int, PF1>(), std::false_type());

    // ---- layer 1 backward on the six action columns; the mask bit of neuron 128 U + 8 v + 4 h + c is bit 4 (v & 3) + c of tile 4 U + (v >> 2)
    float da[6];
#pragma unroll
    for (int c = 0; c < 6; c++) da[c] = 0.0f;
#pragma unroll
    for (int U = 0; U < HT / 4; U++)
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int u = 4 * U + (v >> 2);
        const uint32_t bits = m1[u >> 1] >> (16 * (u & 1) + 4 * (v & 3));
        const float d0 = bits & 1u ? dacc[4 * U + 0][v] : 0.0f, d1 = bits & 2u ? dacc[4 * U + 1][v] : 0.0f;
        const float d2 = bits & 4u ? dacc[4 * U + 2][v] : 0.0f, d3 = bits & 8u ? dacc[4 * U + 3][v] : 0.0f;
#pragma unroll
        for (int c = 0; c < 6; c++) {
          const float4 w = wact4[(c * HP + 128 * U + 8 * v + 4 * h) / 4];
          da[c] = fmaf(w.w, d3, fmaf(w.z, d2, fmaf(w.y, d1, fmaf(w.x, d0, da[c]))));
        }
        asm volatile("" ::: "memory");  // keeps the 6 * 4 HT reads from being hoisted above the accumulators all at once
      }
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const float g = da[c] + __shfl_xor(da[c], 32);
      if (net == 0) da0[c] = g; else da1[c] = g;
    }
  }

  if (live && h == 0) {
    const bool sel = qv1 < qv0;  // a tie takes qf0 (include/urgym.h)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      if (C.dq_da) C.dq_da[m * 6 + c] = da0[c], C.dq_da[((size_t)M + m) * 6 + c] = da1[c];
      if (C.dqmin_da) C.dqmin_da[m * 6 + c] = sel ? da1[c] : da0[c];
    }
    if (C.q) C.q[m] = qv0, C.q[(size_t)M + m] = qv1;
    if (C.q_min) C.q_min[m] = fminf(qv0, qv1);
  }
}

template <int HT>
void launch(const CriticGradKParams& P, hipStream_t s) {
  const unsigned grid = (unsigned)(((size_t)P.call.M + CRITIC_ROWS - 1) / CRITIC_ROWS);
  hipLaunchKernelGGL((critic_grad_kernel<HT>), dim3(grid), dim3(CRITIC_THREADS), 0, s, P);
}

}  // namespace

// Instances HT = 4 and 8 (hidden widths up to 256, the shipped checkpoints' among them) keep everything in registers.  At HT = 12 and 16
// the 16 HT accumulators fill the accumulator file and hipcc spills some 30 to 60 long-lived values to scratch; such instances are not
// built, and the call refuses those widths.
bool critic_grad_supported(Critic* c) { return critic_packed(c).hidden <= CRITIC_GRAD_MAX_HIDDEN; }

void critic_grad_launch(Critic* c, const CriticGradCall& call, hipStream_t s) {
  const CriticPacked buf = critic_packed(c);
  const int HT = (buf.hidden + 127) / 128 * 4;
  CriticGradKParams P;
  P.w = reinterpret_cast<const float4*>(buf.weights);
  P.small = reinterpret_cast<const float4*>(buf.weights + critic_small_offset(buf));
  P.in_features = buf.in_features;
  P.call = call;
  if (HT == 4) launch<4>(P, s);
  else launch<8>(P, s);
}

}  // namespace urgym
