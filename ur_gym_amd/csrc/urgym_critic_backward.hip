// urgym_critic_backward.hip — the gradient of a loss on the twin Q-networks with respect to their PARAMETERS: the backward pass of
// SAC's critic loss as HIP kernels for MI355X (gfx950) (include/urgym.h, urgym_critic_parameter_gradients).  Unlike everything in
// urgym_critic.hip and urgym_critic_grad.hip the results SUM over the rows of the batch, so the work is two stages and a workspace
// (urgym_backward_map.h states every offset once, for host and device; urgym_mlp_grad.h holds the blocks of all three stages that
// the actor's backward pass and the action gradient share):
//
//   stage 1   per row, critic_grad_kernel's structure on the critic's packed buffer as it is (urgym_critic_grad.hip:1-24, urgym_mlp_grad.h): the forward
//             pass operation for operation (q is bitwise urgym_critic_evaluate's), the ReLU masks kept as bits, the second pass over
//             the layer-2 tiles with the transposed A operand -- now with B = mask2 ? w_q dq[row] : 0.  It stops there: no action
//             columns.  It writes h1, h2, d2 and d1 = mask1 ? W1^T d2 : 0 of its rows, the gathered x and dq into the workspace, and q.
//   stage 2   one launch for both networks: g_W1 = d2^T h1 and g_W0 = d1^T x as v_mfma_f32_32x32x2_f32 GEMMs with the row index as K,
//             one wave per 64 x 64 block of the result, operands read from the workspace as float4 (four rows of one neuron); the
//             bias sums g_b1, g_b0 are added up on the VALU from the A operands the block with column 0 loads anyway; g_wq = sum dq h2
//             is an fma chain of waves of its own, g_bq = sum dq a float64 sum rounded once per split.  Up to BW_SPLIT_ROWS rows it stores the results itself.
//   stage 3   only above BW_SPLIT_ROWS rows: stage 2 ran once per split of 1024 rows into the workspace, and this launch adds the
//             partial results in ascending order of the split, in float64, and rounds once.  A launch of its own rather than a last pass of stage 2, which would
//             need a counter in the workspace and an ordering between workgroups of one grid.
//
// The order of every sum is fixed by the geometry alone: per output element rows ascend within a split (row group by row group; within
// a group of 32 rows the MFMA step (q, c), q = 0 .. 3, c = 0 .. 3, adds rows 8 q + c and 8 q + 4 + c), then the splits ascend.  No
// atomics.  This unit may contract a * b + c to fma, like urgym_critic.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "urgym_backward_map.h"
#include "urgym_critic.h"
#include "urgym_mlp_grad.h"

namespace urgym {

namespace {

using namespace mlp_grad;
typedef CriticBackwardMap Map;
enum { BW_G_WQ = BW_G_HEAD, BW_G_BQ };  // the head tensors of a Q-network

// critic_kernel's geometry: urgym_critic.h states it once and every critic unit asserts it
constexpr int CRITIC_THREADS = CRITIC_GEOMETRY_THREADS;  // 4 waves
constexpr int CRITIC_ROWS = CRITIC_GEOMETRY_ROWS;        // rows per workgroup (32 per wave)
constexpr int CIN_PAD = CRITIC_GEOMETRY_CIN_PAD;         // layer-1 K, padded with zero weights (in_features <= 53)
static_assert(CRITIC_ROWS == BW_S1_ROWS && CIN_PAD == Map::X && CRITIC_THREADS == 256 && CRITIC_GRAD_MAX_HIDDEN == BW_MAX_HIDDEN, "urgym_backward_map.h");
constexpr int C1_STEPS4 = CIN_PAD / 8;
constexpr int C1_TILE4 = C1_STEPS4 * 64;
constexpr int C1_CHUNK4 = 4 * C1_TILE4;

struct BackwardKParams {
  const float4* w;      // the critic's packed layers (CriticKParams of urgym_critic.hip)
  const float4* small;  // per network: b0[HP] | b1[HP] | w_q[HP] | b_q, 0, 0, 0
  BwDims d;
  CriticBackwardCall call;
};

__device__ __forceinline__ float row_feature(const CriticBackwardCall& C, size_t m, int k) {
  const int gd = C.goal_dim;
  if (k < gd) return C.achieved_goal[m * gd + k];
  if (k < 2 * gd) return C.desired_goal[m * gd + (k - gd)];
  k -= 2 * gd;
  if (k < C.obs_dim) return C.observation[m * C.obs_dim + k];
  k -= C.obs_dim;
  return k < 6 ? C.action[m * 6 + k] : 0.0f;
}

// ------------------------------------------------------------------------------------------------ stage 1
template <int HT>
__global__ void __launch_bounds__(CRITIC_THREADS, (HT <= 4 ? 2 : 1)) critic_backward_rows_kernel(const BackwardKParams P) {
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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CriticBackwardCall& C = P.call;
  const BwDims& D = P.d;
  const int M = C.M;

  for (int i = tid; i < 2 * SMALL4; i += CRITIC_THREADS) small4[i] = P.small[i];
#pragma unroll
  for (int i = 0; i < PF1; i++) wbuf[0][tid + CRITIC_THREADS * i] = P.w[tid + CRITIC_THREADS * i];

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

#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    const float4* p1 = P.w + (size_t)net * NET4;
    const float4* p2 = p1 + HT * C1_TILE4;
    const float4* sm4 = small4 + net * SMALL4;
    // this lane's float of (array, neuron 0) of the network in hand; neuron n is 32 n floats on
    // (a wave-uniform base and one 32-bit lane offset: per-lane 64-bit addresses, one per store, do not fit the register file)
    float* const ws_h1 = C.workspace + Map::group_offset(D, net, BW_H1, group) + lane_off;
    float* const ws_h2 = C.workspace + Map::group_offset(D, net, BW_H2, group) + lane_off;
    float* const ws_d2 = C.workspace + Map::group_offset(D, net, BW_D2, group) + lane_off;
    float* const ws_d1 = C.workspace + Map::group_offset(D, net, BW_D1, group) + lane_off;

    if (!net) __syncthreads();  // small4, the first chunk

    // this lane's B operands of layer 1, gathered per network (urgym_critic_grad.hip says why)
    uint32_t mrow = (uint32_t)m;
    formed(mrow);
    float xb[CIN_PAD / 2];
#pragma unroll
    for (int s = 0; s < CIN_PAD / 2; s++) xb[s] = row_feature(C, (size_t)mrow, 2 * s + h);
    if (!net && stores) {
#pragma unroll
      for (int s = 0; s < CIN_PAD / 2; s++) (C.workspace + Map::x_group_offset(D, group))[32 * (2 * s) + Map::s1_lane_offset(lane, 1)] = live ? xb[s] : 0.0f;
    }

    uint32_t m1[MW], m2[MW];
#pragma unroll
    for (int i = 0; i < MW; i++) m1[i] = 0, m2[i] = 0;

    // ---- layer 1 forward (critic_kernel's); h1 lives until layer 2 has run forward, its mask beyond
    float h1[HT * 16];
    // chunk c of four tiles; meanwhile the next chunk travels: another of layer 1 or, after the last, layer-2 tile 0
    auto chunk1 = [&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      constexpr bool LAST = c + 1 == L1_CHUNKS;
      const float4* wb = wbuf[buf];
      staged<CRITIC_THREADS, (LAST ? PF2 : PF1), LAST>(wbuf, buf, L, (LAST ? p2 : p1 + (c + 1) * C1_CHUNK4) + tid, [&](auto sg) __attribute__((always_inline)) {
        constexpr int tt = decltype(sg)::value;
        layer1_tile<C1_STEPS4, tt, 4 * c + tt, HT>(wb, sm4, L, xb, h1, m1);
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
      staged<CRITIC_THREADS, PF2, true>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
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
      if (stores) {
#pragma unroll
        for (int v = 0; v < 16; v++) ws_h2[32 * Map::fwd_neuron(t, v, 0)] = live ? fmaxf(acc[v], 0.0f) : 0.0f;
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

    // ---- the upstream gradient of this row and network: given, or (q - target) * scale in two rounded operations
    float dqv = 0.0f;
    if (live) {
      if (C.dq) dqv = C.dq[(size_t)net * M + m];
      else dqv = rounded(rounded(qn - C.target[m]) * C.scale);
    }
    if (h == 0) {
      if (stores) C.workspace[Map::heads_offset(D, net, row, 0)] = dqv;
      if (live && C.q) C.q[(size_t)net * M + m] = qn;
    }

    // d2 = mask2 ? w_q dq : 0 of this lane's neurons, as the pass below forms its B operands
    if (stores) {
#pragma unroll
      for (int t = 0; t < HT; t++) {
        const uint32_t bits = m2[t >> 1] >> (16 * (t & 1));
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const int n = Map::fwd_neuron(t, v, 0);
          const float d2 = rounded(small[net * (SMALL4 * 4) + 2 * HP + n + 4 * h] * dqv);
          ws_d2[32 * n] = (bits >> v) & 1u ? d2 : 0.0f;
        }
      }
    }

    // ---- layer 2 backward: W1^T d2, d2 = mask2 ? w_q dq : 0, tile by tile again; accumulator 4 U + c, register v: neuron 128 U + 8 v + 4 h + c
    f32x16 dacc[HT];
#pragma unroll
    for (int u = 0; u < HT; u++)
#pragma unroll
      for (int v = 0; v < 16; v++) dacc[u][v] = 0.0f;
    auto back2 = [&](int t, const float4* next, auto npf, auto next_is_tile) __attribute__((always_inline)) {
      const uint32_t bits = mask_tile(m2, t);
      const float4* wb = wbuf[buf] + L.abase;
      staged<CRITIC_THREADS, decltype(npf)::value, decltype(next_is_tile)::value>(wbuf, buf, L, next, [&](auto sg) __attribute__((always_inline)) {
        constexpr int g = decltype(sg)::value;
        const float4 wq = sm4[(2 * HP + 32 * t + 8 * g + 4 * h) / 4];
        const float wqr[4] = {wq.x, wq.y, wq.z, wq.w};
        layer2_backward_quarter<HT, g>(wb, [&](int r) __attribute__((always_inline)) {
          const float d2 = rounded(wqr[r] * dqv);  // (formed whatever the mask says: a product under a condition is a branch)
          return (bits >> (4 * g + r)) & 1u ? d2 : 0.0f;
        }, dacc);
      });
    };
#pragma unroll 1
    for (int t = 0; t + 1 < HT; t++) back2(t, p2 + (size_t)(t + 1) * L2_TILE4 + tid, std::integral_constant<int, PF2>(), std::true_type());
    // the last tile stages the other network's first layer-1 chunk (urgym_critic_grad.hip)
    back2(HT - 1, P.w + (net == 0 ? NET4 : 0) + tid, std::integral_constant<int, PF1>(), std::false_type());

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
}

// ------------------------------------------------------------------------------------------------ stage 2
struct ReduceKParams {
  const float* ws;
  float* partial;  // the workspace again, for the partial sums (S > 1)
  BwDims d;
  float* grad[Map::NETS][Map::TENSORS];
};

__global__ void __launch_bounds__(256) critic_backward_reduce_kernel(const ReduceKParams P) {
  const BwDims& D = P.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, i = lane & 31;
  int split, net, job0;
  Map::s2_block(D, blockIdx.x, &split, &net, &job0);
  const BwJob job = Map::job(D, job0 + wave);
  if (job.kind == BW_JOB_NONE) return;
  int R0, R1;
  Map::split_groups(D, split, &R0, &R1);
  float* dst[Map::TENSORS];
#pragma unroll
  for (int t = 0; t < Map::TENSORS; t++) dst[t] = D.S > 1 ? P.partial + Map::partial_offset(D, split, net) + Map::tensor_offset(D, t) : P.grad[net][t];

  if (job.kind == BW_JOB_HEAD) {
    const int n = 32 * job.ab + i;
    float acc = 0.0f;
    for (int R = R0; R < R1; R++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const size_t row = Map::s2_row(R, q, h);
        const float4 a = *reinterpret_cast<const float4*>(P.ws + Map::offset(D, net, BW_H2, row, n));
        const float4 d = *reinterpret_cast<const float4*>(P.ws + Map::heads_offset(D, net, row, 0));
        acc = fmaf(a.x, d.x, acc), acc = fmaf(a.y, d.y, acc), acc = fmaf(a.z, d.z, acc), acc = fmaf(a.w, d.w, acc);
      }
    const float g = acc + __shfl_xor(acc, 32);
    if (h == 0 && n < D.H) dst[BW_G_WQ][n] = g;
    if (job.ab != 0) return;
    // g_bq of the split: one scalar out of up to 1024 terms of one sign, so its sum is kept in float64 and rounded once.  Lane (h, i)
    // adds row i of every second row group from R0 + h on, ascending; then the 64 lanes are added in a fixed butterfly (lane_sum).
    double dsum = 0.0;
    for (int R = R0 + h; R < R1; R += 2) dsum += (double)P.ws[Map::heads_offset(D, net, Map::s2_bias_row(R, i), 0)];
    dsum = lane_sum(dsum);
    if (lane == 0) dst[BW_G_BQ][0] = (float)dsum;
    return;
  }

  // a 64 x 64 block: A = d2 (g_W1) or d1 (g_W0), neurons 64 ab + 32 ia + i; B = h1, or x with 56 columns
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
      const float* abase = P.ws + Map::offset(D, net, a_array, row, 0);
      const float* bbase = w1 ? P.ws + Map::offset(D, net, BW_H1, row, 0) : P.ws + Map::x_offset(D, row, 0);
      float4 a[2], b[2];
      a[0] = operand4(abase, an, D.HP), a[1] = operand4(abase, an + 32, D.HP);
      b[0] = operand4(bbase, bn, b_limit), b[1] = operand4(bbase, bn + 32, b_limit);
      gemm_step(acc, bsum, a, b);
    }
  gemm_store<Map>(D, job, lane, w1 ? D.H : D.in, dst[w1 ? BW_G_W1 : BW_G_W0], dst[w1 ? BW_G_B1 : BW_G_B0], acc, bsum);
}

// ------------------------------------------------------------------------------------------------ stage 3
__global__ void __launch_bounds__(256) critic_backward_combine_kernel(const ReduceKParams P) {
  combine_element<Map>(P.partial, P.d, P.grad, (size_t)blockIdx.x * 256 + threadIdx.x);
}

template <int HT>
void launch_rows(const BackwardKParams& P, hipStream_t s) {
  hipLaunchKernelGGL((critic_backward_rows_kernel<HT>), dim3(Map::s1_grid(P.d)), dim3(CRITIC_THREADS), 0, s, P);
}

}  // namespace

// Instances HT = 4 and 8, like the action gradient's and for its reason: the 16 HT accumulators of the pass back through layer 2.
bool critic_backward_supported(Critic* c) { return critic_packed(c).hidden <= CRITIC_GRAD_MAX_HIDDEN; }

uint64_t critic_backward_workspace_bytes(Critic* c, int count) {
  const CriticPacked buf = critic_packed(c);
  return (uint64_t)Map::dims(buf.in_features, buf.hidden, count).floats * sizeof(float);
}

int critic_backward_launches(int count) { return count > BW_SPLIT_ROWS ? 3 : 2; }

void critic_backward_launch(Critic* c, const CriticBackwardCall& call, hipStream_t s) {
  const CriticPacked buf = critic_packed(c);
  const int HT = (buf.hidden + 127) / 128 * 4;
  BackwardKParams P;
  P.w = reinterpret_cast<const float4*>(buf.weights);
  P.small = reinterpret_cast<const float4*>(buf.weights + critic_small_offset(buf));
  P.d = Map::dims(buf.in_features, buf.hidden, call.M);
  P.call = call;
  if (HT == 4) launch_rows<4>(P, s);
  else launch_rows<8>(P, s);
  ReduceKParams Q;
  Q.ws = call.workspace, Q.partial = call.workspace, Q.d = P.d;
  for (int net = 0; net < 2; net++)
    for (int t = 0; t < Map::TENSORS; t++) Q.grad[net][t] = call.grad[net][t];
  hipLaunchKernelGGL(critic_backward_reduce_kernel, dim3(Map::s2_grid(P.d)), dim3(256), 0, s, Q);
  if (P.d.S > 1) hipLaunchKernelGGL(critic_backward_combine_kernel, dim3((unsigned)((2 * P.d.P + 255) / 256)), dim3(256), 0, s, Q);
}

}  // namespace urgym
