// urgym_actor_backward.hip — the gradient of a loss on the SAC actor with respect to its PARAMETERS: the backward pass of SAC's policy
// loss as HIP kernels for MI355X (gfx950) (include/urgym.h, urgym_actor_parameter_gradients).  The mirror of
// urgym_critic_backward.hip on the actor's packed buffer, whose layer 2 has the critic's layout (urgym_pack_map.h): two stages and a
// workspace (urgym_backward_map.h states every offset once, for host and device, as ActorBackwardMap; urgym_mlp_grad.h holds the blocks
// of all three stages that the critic's gradient units share).
//
//   stage 1   per row, actor_kernel<HT, true>'s forward pass operation for operation (action and log_prob are bitwise
//             urgym_actor_sample_rows'), the ReLU masks kept as bits; the head arithmetic of the SAMPLE form, or the given head
//             gradients; d_h2 = W_mu^T d_mu + W_ls^T dr as twelve fma per neuron on the VALU from the heads as they are packed (one
//             float4 per column and four consecutive neurons); the second pass over the layer-2 tiles with the transposed A operand.
//             It writes h1, h2, d2, d1, the gathered x and the twelve head gradients of its rows into the workspace, and the optional
//             per-row outputs.
//   stage 2   g_W1 = d2^T h1 and g_W0 = d1^T x as v_mfma_f32_32x32x2_f32 GEMMs with the row index as K, one wave per 64 x 64 block; the
//             bias sums g_b1, g_b0 on the VALU from the A operands; g_Wmu and g_Wls as twelve fma chains per neuron against h2 in waves
//             of their own (a 32-wide MFMA block would carry 12 useful columns of 32); g_bmu and g_bls are float64 sums rounded once
//             per split.  Up to BW_SPLIT_ROWS rows it stores the results itself.
//   stage 3   only above BW_SPLIT_ROWS rows: adds the partial results of the splits in ascending order, in float64, and rounds once.
//
// The order of every sum is fixed by the geometry alone: per output element rows ascend within a split (row group by row group; within
// a group of 32 rows the MFMA step (q, c), q = 0 .. 3, c = 0 .. 3, adds rows 8 q + c and 8 q + 4 + c; a head chain adds rows
// 8 q + 4 h + c per lane half h and joins the halves last), then the splits ascend.  No atomics.  This unit may contract a * b + c to
// fma, like urgym_actor.hip; where the header asks for an operation rounded on its own, rounded() stands between.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "urgym_actor.h"
#include "urgym_backward_map.h"
#include "urgym_mlp_grad.h"
#include "urgym_pack_map.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

using namespace mlp_grad;
typedef ActorBackwardMap Map;
enum { AB_G_WMU = BW_G_HEAD, AB_G_BMU, AB_G_WLS, AB_G_BLS };  // the head tensors of the policy

// actor_kernel's geometry
constexpr int ACTOR_THREADS = 256;  // 4 waves
constexpr int ACTOR_ROWS = 128;     // rows per workgroup (32 per wave)
constexpr int IN_PAD = 48;          // layer-1 K, padded with zero weights (in_features <= 47)
static_assert(ACTOR_ROWS == BW_S1_ROWS && IN_PAD == Map::X && IN_PAD == 8 * PACK_ACTOR_STEPS4 && BW_MAX_COUNT == ACTOR_BACKWARD_MAX_COUNT, "urgym_backward_map.h");
constexpr int L1_STEPS4 = IN_PAD / 8;
constexpr int L1_TILE4 = L1_STEPS4 * 64;
constexpr int L1_CHUNK4 = 4 * L1_TILE4;
struct BackwardKParams {
  const float4* p1;     // layer 1, packed [HT][L1_STEPS4][64 lanes] float4
  const float4* p2;     // layer 2, packed [HT][HT * 4][64 lanes] float4
  const float4* small;  // b0[HP] | b1[HP] | w_mu as [HP / 4][6][4] | b_mu[8] | w_log_std as [HP / 4][6][4] | b_log_std[8]
  BwDims d;
  ActorBackwardCall call;
};

__device__ __forceinline__ float row_feature(const ActorBackwardCall& C, size_t m, int k) {
  const int gd = C.goal_dim;
  if (k < gd) return C.achieved_goal[m * gd + k];
  if (k < 2 * gd) return C.desired_goal[m * gd + (k - gd)];
  k -= 2 * gd;
  return k < C.obs_dim ? C.observation[m * C.obs_dim + k] : 0.0f;
}

// ------------------------------------------------------------------------------------------------ stage 1
// One workgroup per CU in both instances: at two (256 registers per lane) the HT = 4 instance spilled 76 registers -- the twelve head
// gradients, the noise and the clamped log_std live across the pass back, which the critic's kernel has no counterpart of.
template <int HT>
__global__ void __launch_bounds__(ACTOR_THREADS, 1) actor_backward_rows_kernel(const BackwardKParams P) {
  constexpr int HP = HT * 32;
  constexpr int L2_TILE4 = HT * 4 * 64;        // float4 per packed layer-2 tile
  constexpr int L2_IMAGE4 = HT * 4 * L2_ROW4;  // float4 of its staged image
  constexpr int BUF4 = L1_CHUNK4 > L2_IMAGE4 ? L1_CHUNK4 : L2_IMAGE4;
  constexpr int HEAD4 = (HP * 6 + 8) / 4;  // float4 per layer-3 head: weights, then the bias
  constexpr int SMALL4 = (HP * 2) / 4 + 2 * HEAD4;
  constexpr int L1_CHUNKS = HT / 4;
  constexpr int PF1 = L1_CHUNK4 / ACTOR_THREADS, PF2 = L2_TILE4 / ACTOR_THREADS;  // float4 per thread and staged chunk (6, HT)
  constexpr int MW = HT / 2;                                                      // mask words per layer: two tiles of 16 bits each
  __shared__ float4 wbuf[2][BUF4];
  __shared__ float4 small4[SMALL4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ActorBackwardCall& C = P.call;
  const BwDims& D = P.d;
  const int M = C.M;

  for (int i = tid; i < SMALL4; i += ACTOR_THREADS) small4[i] = P.small[i];
#pragma unroll
  for (int i = 0; i < PF1; i++) wbuf[0][tid + ACTOR_THREADS * i] = P.p1[tid + ACTOR_THREADS * i];

  const int h = lane >> 5;
  const size_t row = Map::s1_row(blockIdx.x, wave, lane);
  const bool live = row < (size_t)M;
  const bool stores = Map::s1_stores(D, row);     // the same for the whole wave: its row group exists
  const size_t m = live ? row : (size_t)M - 1;  // lanes past the end compute on the last row and store +0
  // the wave's row group, in scalar registers, and this lane's place in a group's [neuron][32 rows]: the neurons of lane half 1 are 4 on
  const size_t group = Map::s1_group(blockIdx.x, __builtin_amdgcn_readfirstlane(wave));
  const uint32_t lane_off = Map::s1_lane_offset(lane, 4);
  // this lane in the staged images (urgym_mlp_grad.h: Lane)
  const int ai = lane & 31, jj = 8 * (ai >> 3) + 2 * (ai & 3) + ((ai >> 2) & 1);
  const int abase = (jj >> 1) * L2_ROW4 + (jj & 1) * 33 + 4 * h;
  const int sbase = l2_slot(tid >> 6, tid & 63);
  const Lane L = {tid, lane, h, abase, sbase};

  const float* small = reinterpret_cast<const float*>(small4);
  int buf = 0;  // the half of wbuf that holds the chunk in use

  // this lane's float of (array, neuron 0); neuron n is 32 n floats on (a wave-uniform base and one 32-bit lane offset)
  float* const ws_h1 = C.workspace + Map::group_offset(D, 0, BW_H1, group) + lane_off;
  float* const ws_h2 = C.workspace + Map::group_offset(D, 0, BW_H2, group) + lane_off;
  float* const ws_d2 = C.workspace + Map::group_offset(D, 0, BW_D2, group) + lane_off;
  float* const ws_d1 = C.workspace + Map::group_offset(D, 0, BW_D1, group) + lane_off;

  // this lane's B operands of layer 1: features 2 s + h of its row
  float xb[IN_PAD / 2];
#pragma unroll
  for (int s = 0; s < IN_PAD / 2; s++) xb[s] = row_feature(C, m, 2 * s + h);
  if (stores) {
#pragma unroll
    for (int s = 0; s < IN_PAD / 2; s++) (C.workspace + Map::x_group_offset(D, group))[32 * (2 * s) + Map::s1_lane_offset(lane, 1)] = live ? xb[s] : 0.0f;
  }
  __syncthreads();  // small4, the first chunk

  uint32_t m1[MW], m2[MW];
#pragma unroll
  for (int i = 0; i < MW; i++) m1[i] = 0, m2[i] = 0;

  // ---- layer 1 forward (actor_kernel's); h1 lives until layer 2 has run forward, its mask beyond
  float h1[HT * 16];
  // chunk c of four tiles; meanwhile the next chunk travels: another of layer 1 or, after the last, layer-2 tile 0
  auto chunk1 = [&](auto cc) __attribute__((always_inline)) {
    constexpr int c = decltype(cc)::value;
    constexpr bool LAST = c + 1 == L1_CHUNKS;
    const float4* wb = wbuf[buf];
    staged<ACTOR_THREADS, (LAST ? PF2 : PF1), LAST>(wbuf, buf, L, (LAST ? P.p2 : P.p1 + (c + 1) * L1_CHUNK4) + tid, [&](auto sg) __attribute__((always_inline)) {
      constexpr int tt = decltype(sg)::value;
      layer1_tile<L1_STEPS4, tt, 4 * c + tt, HT>(wb, small4, L, xb, h1, m1);
    });
  };
  chunk1(std::integral_constant<int, 0>());
  if constexpr (L1_CHUNKS > 1) chunk1(std::integral_constant<int, 1>());
  // (every store to the workspace stands outside `staged`: a branch between the loads and the stores of a travelling chunk sends
  // the chunk through scratch)
  if (stores) {
#pragma unroll
    for (int t = 0; t < HT; t++)
#pragma unroll
      for (int v = 0; v < 16; v++) ws_h1[32 * Map::fwd_neuron(t, v, 0)] = live ? h1[t * 16 + v] : 0.0f;
  }

  // ---- layer 2 forward tile by tile, each tile straight into both heads of layer 3 (actor_kernel<HT, true>'s fma order per output:
  // tiles ascending, within a tile g, then the four neurons of the float4); the tile after it travels meanwhile
  float mu[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float ls[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  auto fwd2 = [&](int t, const float4* next) __attribute__((always_inline)) {
    const float4* wb = wbuf[buf] + lane + h;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 b = small4[(HP + 32 * t + 8 * g + 4 * h) / 4];
      acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
    }
    staged<ACTOR_THREADS, PF2, true>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
      layer2_forward_quarter<HT, decltype(sg)::value>(wb, h1, acc);
    });
    f32x16 r;
#pragma unroll
    for (int v = 0; v < 16; v++) r[v] = fmaxf(acc[v], 0.0f);
    const float4* wm = small4 + (2 * HP) / 4 + (size_t)((32 * t + 4 * h) / 4) * 6;
#pragma unroll
    for (int g = 0; g < 4; g++) {
#pragma unroll
      for (int o = 0; o < 6; o++) {
        const float4 w = wm[2 * g * 6 + o];
        mu[o] = fmaf(w.x, r[4 * g + 0], mu[o]);
        mu[o] = fmaf(w.y, r[4 * g + 1], mu[o]);
        mu[o] = fmaf(w.z, r[4 * g + 2], mu[o]);
        mu[o] = fmaf(w.w, r[4 * g + 3], mu[o]);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; g++) {
#pragma unroll
      for (int o = 0; o < 6; o++) {
        const float4 w = wm[HEAD4 + 2 * g * 6 + o];
        ls[o] = fmaf(w.x, r[4 * g + 0], ls[o]);
        ls[o] = fmaf(w.y, r[4 * g + 1], ls[o]);
        ls[o] = fmaf(w.z, r[4 * g + 2], ls[o]);
        ls[o] = fmaf(w.w, r[4 * g + 3], ls[o]);
      }
    }
    if (stores) {
#pragma unroll
      for (int v = 0; v < 16; v++) ws_h2[32 * Map::fwd_neuron(t, v, 0)] = live ? r[v] : 0.0f;
    }
    uint32_t bits = relu_bits(acc) << (16 * (t & 1));
    formed(bits);
#pragma unroll
    for (int i = 0; i < MW; i++) m2[i] |= (t >> 1) == i ? bits : 0u;  // (a register array takes no run-time index)
  };
#pragma unroll 1
  for (int t = 0; t < HT; t++)  // after the last tile: tile 0 again, for the way back
    fwd2(t, P.p2 + (size_t)(t + 1 < HT ? t + 1 : 0) * L2_TILE4 + tid);

  // ---- the sampling epilogue of actor_kernel<HT, true>, expression for expression; both lane halves hold the row's 12 sums after the
  // cross-lane add and run the same arithmetic
  const bool gauss = C.mode == URGYM_SAMPLE_GAUSSIAN;
  float eps[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (gauss) {
    float w[6];
    noise_words(C.seed, C.draw, (uint32_t)row, w);
#pragma unroll
    for (int p = 0; p < 3; p++) {  // Box-Muller: u1 in (0, 1], u2 in [0, 1), both exact
      const float r = sqrtf(-2.0f * logf((w[2 * p] + 1.0f) * TWO_M24));
      const float turn = 2.0f * (w[2 * p + 1] * TWO_M24);  // angle / pi: exact
      eps[2 * p] = r * cospif(turn);
      eps[2 * p + 1] = r * sinpif(turn);
    }
  }
  float mean[6], raw[6], lstd[6], sd[6], act[6];
  float lp = 0.0f;
#pragma unroll
  for (int o = 0; o < 6; o++) {
    mean[o] = mu[o] + __shfl_xor(mu[o], 32) + small[HP * 8 + o];
    raw[o] = ls[o] + __shfl_xor(ls[o], 32) + small[HP * 14 + 8 + o];
    lstd[o] = fminf(fmaxf(raw[o], -20.0f), 2.0f);
    sd[o] = expf(lstd[o]);
    act[o] = tanhf(gauss ? fmaf(sd[o], eps[o], mean[o]) : mean[o]);
    lp += -0.5f * eps[o] * eps[o] - lstd[o] - HALF_LOG_2PI - logf(1.0f - act[o] * act[o] + 1e-6f);
  }

  // ---- the upstream gradient at the heads: given (HEADS), or formed from d_action and d_log_prob (SAMPLE), each line of the header one
  // float32 operation rounded on its own; dr = d_log_std through the clamp, both edges inclusive (a NaN r compares false: 0)
  float dmu[6], dls[6], dr[6];
#pragma unroll
  for (int o = 0; o < 6; o++) {
    if (C.d_action) {
      const float da = C.d_action[m * 6 + o];
      const float dlp = C.d_log_prob ? C.d_log_prob[m] : 0.0f;
      const float a = rounded(act[o]);  // (a value of its own: a product shared with log_prob's 1 - a a would change how that one contracts)
      const float p = rounded(a * a);
      const float t = rounded(1.0f - p);
      const float c = rounded((2.0f * a) / rounded(t + 1e-6f));
      const float A = rounded(da + rounded(dlp * c));
      const float dpre = rounded(A * t);
      const float e = rounded(sd[o] * eps[o]);
      dmu[o] = dpre;
      dls[o] = rounded(dpre * e) - dlp;
    } else {
      dmu[o] = C.d_mu[m * 6 + o];
      dls[o] = C.d_log_std[m * 6 + o];
    }
    if (!live) dmu[o] = 0.0f, dls[o] = 0.0f;
    dr[o] = (raw[o] >= -20.0f && raw[o] <= 2.0f) ? dls[o] : 0.0f;
  }
  if (h == 0) {
    if (stores) {
      float* ws_heads = C.workspace + Map::heads_group_offset(D, 0, group) + (lane & 31);
#pragma unroll
      for (int o = 0; o < 6; o++) ws_heads[32 * o] = dmu[o], ws_heads[32 * (6 + o)] = dr[o];
    }
    if (live) {
      if (C.action) store6(C.action, row, act);
      if (C.log_prob) C.log_prob[row] = lp;
      if (C.out_d_mu) store6(C.out_d_mu, row, dmu);
    }
  } else if (live) {
    if (C.noise) store6(C.noise, row, eps);
    if (C.log_std) store6(C.log_std, row, lstd);
    if (C.out_d_log_std) store6(C.out_d_log_std, row, dls);
    if (C.std) store6(C.std, row, sd);
  }

  // d_h2 of neurons 32 t + 8 g + 4 h + c, c = 0 .. 3: one float4 per head column, twelve fma per neuron in the order mu 0 .. 5, ls 0 .. 5
  auto head_back = [&](int t, int g) __attribute__((always_inline)) {
    const float4* wm = small4 + (2 * HP) / 4 + (size_t)((32 * t + 4 * h) / 4) * 6 + 2 * g * 6;
    f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int o = 0; o < 6; o++) {
      const float4 w = wm[o];
      d[0] = fmaf(w.x, dmu[o], d[0]), d[1] = fmaf(w.y, dmu[o], d[1]), d[2] = fmaf(w.z, dmu[o], d[2]), d[3] = fmaf(w.w, dmu[o], d[3]);
    }
#pragma unroll
    for (int o = 0; o < 6; o++) {
      const float4 w = wm[HEAD4 + o];
      d[0] = fmaf(w.x, dr[o], d[0]), d[1] = fmaf(w.y, dr[o], d[1]), d[2] = fmaf(w.z, dr[o], d[2]), d[3] = fmaf(w.w, dr[o], d[3]);
    }
    return d;
  };

  // d2 = mask2 ? d_h2 : 0 of this lane's neurons, as the pass below forms its B operands
  if (stores) {
#pragma unroll
    for (int t = 0; t < HT; t++) {
      const uint32_t bits = m2[t >> 1] >> (16 * (t & 1));
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 d = head_back(t, g);
#pragma unroll
        for (int c = 0; c < 4; c++) ws_d2[32 * Map::fwd_neuron(t, 4 * g + c, 0)] = (live && ((bits >> (4 * g + c)) & 1u)) ? d[c] : 0.0f;
      }
    }
  }

  // ---- layer 2 backward: W1^T d2, tile by tile again; accumulator 4 U + c, register v: neuron 128 U + 8 v + 4 h + c
  f32x16 dacc[HT];
#pragma unroll
  for (int u = 0; u < HT; u++)
#pragma unroll
    for (int v = 0; v < 16; v++) dacc[u][v] = 0.0f;
  auto back2 = [&](int t, const float4* next, auto npf) __attribute__((always_inline)) {
    const uint32_t bits = mask_tile(m2, t);
    const float4* wb = wbuf[buf] + abase;
    staged<ACTOR_THREADS, decltype(npf)::value, true>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
      constexpr int g = decltype(sg)::value;
      const f32x4 d = head_back(t, g);
      layer2_backward_quarter<HT, g>(wb, [&](int r) __attribute__((always_inline)) { return (bits >> (4 * g + r)) & 1u ? d[r] : 0.0f; }, dacc);
    });
  };
#pragma unroll 1
  for (int t = 0; t + 1 < HT; t++) back2(t, P.p2 + (size_t)(t + 1) * L2_TILE4 + tid, std::integral_constant<int, PF2>());
  back2(HT - 1, P.p2, std::integral_constant<int, 0>());  // nothing travels behind the last tile

  // ---- d1 = mask1 ? W1^T d2 : 0; the mask bit of neuron 128 U + 8 v + 4 h + c is bit 4 (v & 3) + c of tile 4 U + (v >> 2)
  if (stores) {
#pragma unroll
    for (int U = 0; U < HT / 4; U++)
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int u = 4 * U + (v >> 2);
        const uint32_t bits = m1[u >> 1] >> (16 * (u & 1) + 4 * (v & 3));
#pragma unroll
        for (int c = 0; c < 4; c++) ws_d1[32 * Map::back_neuron(4 * U + c, v, 0)] = (live && ((bits >> c) & 1u)) ? dacc[4 * U + c][v] : 0.0f;
      }
  }
}

// ------------------------------------------------------------------------------------------------ stage 2
struct ReduceKParams {
  const float* ws;
  float* partial;  // the workspace again, for the partial sums (S > 1)
  BwDims d;
  float* grad[Map::NETS][Map::TENSORS];
};

__global__ void __launch_bounds__(256) actor_backward_reduce_kernel(const ReduceKParams P) {
  const BwDims& D = P.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, i = lane & 31;
  int split, net, job0;  // net = 0
  Map::s2_block(D, blockIdx.x, &split, &net, &job0);
  const BwJob job = Map::job(D, job0 + wave);
  if (job.kind == BW_JOB_NONE) return;
  int R0, R1;
  Map::split_groups(D, split, &R0, &R1);
  float* dst[Map::TENSORS];
#pragma unroll
  for (int t = 0; t < Map::TENSORS; t++) dst[t] = D.S > 1 ? P.partial + Map::partial_offset(D, split, 0) + Map::tensor_offset(D, t) : P.grad[0][t];

  if (job.kind == BW_JOB_HEAD) {
    const int n = 32 * job.ab + i;
    float acc[Map::HEADS];
#pragma unroll
    for (int j = 0; j < Map::HEADS; j++) acc[j] = 0.0f;
    for (int R = R0; R < R1; R++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const size_t row = Map::s2_row(R, q, h);
        const float4 a = *reinterpret_cast<const float4*>(P.ws + Map::offset(D, 0, BW_H2, row, n));
#pragma unroll
        for (int j = 0; j < Map::HEADS; j++) {
          const float4 d = *reinterpret_cast<const float4*>(P.ws + Map::heads_offset(D, 0, row, j));
          acc[j] = fmaf(a.x, d.x, acc[j]), acc[j] = fmaf(a.y, d.y, acc[j]), acc[j] = fmaf(a.z, d.z, acc[j]), acc[j] = fmaf(a.w, d.w, acc[j]);
        }
      }
#pragma unroll
    for (int j = 0; j < Map::HEADS; j++) {
      const float g = acc[j] + __shfl_xor(acc[j], 32);
      if (h == 0 && n < D.H) dst[Map::head_tensor(j)][Map::head_element(D, j, n)] = g;
    }
    if (job.ab != 0) return;
    // g_bmu and g_bls of the split: twelve scalars out of up to 1024 terms each, possibly of one sign, so the sums are kept in float64
    // and rounded once.  Lane (h, i) adds row i of every second row group from R0 + h on, ascending; then the 64 lanes are added in
    // a fixed butterfly (lane_sum).
    double dsum[Map::HEADS];
#pragma unroll
    for (int j = 0; j < Map::HEADS; j++) dsum[j] = 0.0;
    for (int R = R0 + h; R < R1; R += 2)
#pragma unroll
      for (int j = 0; j < Map::HEADS; j++) dsum[j] += (double)P.ws[Map::heads_offset(D, 0, Map::s2_bias_row(R, i), j)];
#pragma unroll
    for (int j = 0; j < Map::HEADS; j++) {
      dsum[j] = lane_sum(dsum[j]);
      if (lane == 0) dst[j < 6 ? AB_G_BMU : AB_G_BLS][j % 6] = (float)dsum[j];
    }
    return;
  }

  // a 64 x 64 block: A = d2 (g_W1) or d1 (g_W0), neurons 64 ab + 32 ia + i; B = h1, or x with 48 columns
  const bool w1 = job.kind == BW_JOB_W1;
  const int a_array = w1 ? BW_D2 : BW_D1, b_limit = w1 ? D.HP : Map::X;
  f32x16 acc[2][2];
#pragma unroll
  for (int ia = 0; ia < 2; ia++)
#pragma unroll
    for (int jb = 0; jb < 2; jb++)
#pragma unroll
      for (int v = 0; v < 16; v++) acc[ia][jb][v] = 0.0f;
  float bsum[2] = {0.0f, 0.0f};
  const int an = 64 * job.ab + i, bn = 64 * job.bb + i;
  for (int R = R0; R < R1; R++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const size_t row = Map::s2_row(R, q, h);
      const float* abase = P.ws + Map::offset(D, 0, a_array, row, 0);
      const float* bbase = w1 ? P.ws + Map::offset(D, 0, BW_H1, row, 0) : P.ws + Map::x_offset(D, row, 0);
      float4 a[2], b[2];
      a[0] = operand4(abase, an, D.HP), a[1] = operand4(abase, an + 32, D.HP);
      b[0] = operand4(bbase, bn, b_limit), b[1] = operand4(bbase, bn + 32, b_limit);
      gemm_step(acc, bsum, a, b);
    }
  gemm_store<Map>(D, job, lane, w1 ? D.H : D.in, dst[w1 ? BW_G_W1 : BW_G_W0], dst[w1 ? BW_G_B1 : BW_G_B0], acc, bsum);
}

// ------------------------------------------------------------------------------------------------ stage 3
__global__ void __launch_bounds__(256) actor_backward_combine_kernel(const ReduceKParams P) {
  combine_element<Map>(P.partial, P.d, P.grad, (size_t)blockIdx.x * 256 + threadIdx.x);
}

template <int HT>
void launch_rows(const BackwardKParams& P, hipStream_t s) {
  hipLaunchKernelGGL((actor_backward_rows_kernel<HT>), dim3(Map::s1_grid(P.d)), dim3(ACTOR_THREADS), 0, s, P);
}

}  // namespace

// Instances HT = 4 and 8, like the critic's gradients and for their reason: the 16 HT accumulators of the pass back through layer 2.
bool actor_backward_supported(Actor* a) { return actor_packed(a).hidden <= BW_MAX_HIDDEN; }

uint64_t actor_backward_workspace_bytes(Actor* a, int count) {
  const ActorPacked buf = actor_packed(a);
  return (uint64_t)Map::dims(buf.in_features, buf.hidden, count).floats * sizeof(float);
}

int actor_backward_launches(int count) { return count > BW_SPLIT_ROWS ? 3 : 2; }

void actor_backward_launch(Actor* a, const ActorBackwardCall& call, hipStream_t s) {
  const ActorPacked buf = actor_packed(a);
  const PackDims pd = pack_dims_actor(buf.in_features, buf.hidden);
  BackwardKParams P;
  P.p1 = reinterpret_cast<const float4*>(buf.weights);
  P.p2 = reinterpret_cast<const float4*>(buf.weights + pd.n1);
  P.small = reinterpret_cast<const float4*>(buf.weights + pd.n1 + pd.n2);
  P.d = Map::dims(buf.in_features, buf.hidden, call.M);
  P.call = call;
  if (pd.HT == 4) launch_rows<4>(P, s);
  else launch_rows<8>(P, s);
  ReduceKParams Q;
  Q.ws = call.workspace, Q.partial = call.workspace, Q.d = P.d;
  for (int t = 0; t < Map::TENSORS; t++) Q.grad[0][t] = call.grad[t];
  hipLaunchKernelGGL(actor_backward_reduce_kernel, dim3(Map::s2_grid(P.d)), dim3(256), 0, s, Q);
  if (P.d.S > 1) hipLaunchKernelGGL(actor_backward_combine_kernel, dim3((unsigned)((P.d.P + 255) / 256)), dim3(256), 0, s, Q);
}

}  // namespace urgym
