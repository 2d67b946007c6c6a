// urgym_critic_backward.hip — the gradient of a loss on the twin Q-networks with respect to their PARAMETERS: the backward pass of
// SAC's critic loss as HIP kernels for MI355X (gfx950) (include/urgym.h, urgym_critic_parameter_gradients).  Unlike everything in
// urgym_critic.hip and urgym_critic_grad.hip the results SUM over the rows of the batch, so the work is two stages and a workspace
// (urgym_backward_map.h states every offset once, for host and device):
//
//   stage 1   per row, critic_grad_kernel's structure on the critic's packed buffer as it is (urgym_critic_grad.hip:1-31): the forward
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

namespace urgym {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// critic_kernel's geometry: urgym_critic.h states it once and every critic unit asserts it
constexpr int CRITIC_THREADS = CRITIC_GEOMETRY_THREADS;  // 4 waves
constexpr int CRITIC_ROWS = CRITIC_GEOMETRY_ROWS;        // rows per workgroup (32 per wave)
constexpr int CIN_PAD = CRITIC_GEOMETRY_CIN_PAD;         // layer-1 K, padded with zero weights (in_features <= 53)
static_assert(CRITIC_ROWS == BW_S1_ROWS && CIN_PAD == BW_X && CRITIC_THREADS == 256, "urgym_backward_map.h");
constexpr int C1_STEPS4 = CIN_PAD / 8;
constexpr int C1_TILE4 = C1_STEPS4 * 64;
constexpr int C1_CHUNK4 = 4 * C1_TILE4;
constexpr int L2_ROW4 = 66;  // float4 per read row of a staged layer-2 tile (urgym_critic_grad.hip: the transposed A operand)

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

// where float4 (read row sq, lane l) of a packed layer-2 tile lies in its staged image
__device__ __forceinline__ int l2_slot(int sq, int l) { return sq * L2_ROW4 + l + (l >> 5); }

// bit v = acc[v] > 0: a pre-activation of exactly 0 has derivative 0 (torch's relu), and so has NaN
__device__ __forceinline__ uint32_t relu_bits(const f32x16 acc) {
  uint32_t bits = 0;
#pragma unroll
  for (int v = 0; v < 16; v++) bits |= (acc[v] > 0.0f ? 1u : 0u) << v;
  return bits;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    static_for<I + 1, N>(f);
  }
}

// makes a value opaque to the optimiser where it is complete (urgym_critic_grad.hip: formed)
__device__ __forceinline__ void formed(uint32_t& word) { word = (uint32_t)__builtin_amdgcn_mov_dpp((int)word, 0xE4, 0xF, 0xF, true); }

// a result that must be rounded before it is used (urgym_critic.hip: rounded)
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
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
  const size_t row = bw_s1_row(blockIdx.x, wave, lane);
  const bool live = row < (size_t)M;
  const bool stores = bw_s1_stores(D, row);     // the same for the whole wave: its row group exists
  const size_t m = live ? row : (size_t)M - 1;  // lanes past the end compute on the last row and store +0
  // the wave's row group, in scalar registers, and this lane's place in a group's [neuron][32 rows]: the neurons of lane half 1 are 4 on
  const size_t group = bw_s1_group(blockIdx.x, __builtin_amdgcn_readfirstlane(wave));
  const uint32_t lane_off = bw_s1_lane_offset(lane, 4);
  // this lane as an A lane of the backward pass (urgym_critic_grad.hip)
  const int ai = lane & 31, jj = 8 * (ai >> 3) + 2 * (ai & 3) + ((ai >> 2) & 1);
  const int abase = (jj >> 1) * L2_ROW4 + (jj & 1) * 33 + 4 * h;
  const int sbase = l2_slot(tid >> 6, tid & 63);

  const float* small = reinterpret_cast<const float*>(small4);
  int buf = 0;  // the half of wbuf that holds the chunk in use

#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    const float4* p1 = P.w + (size_t)net * NET4;
    const float4* p2 = p1 + HT * C1_TILE4;
    const float4* sm4 = small4 + net * SMALL4;
    // this lane's float of (array, neuron 0) of the network in hand; neuron n is 32 n floats on
    // (a wave-uniform base and one 32-bit lane offset: per-lane 64-bit addresses, one per store, do not fit the register file)
    float* const ws_h1 = C.workspace + bw_group_offset(D, net, BW_H1, group) + lane_off;
    float* const ws_h2 = C.workspace + bw_group_offset(D, net, BW_H2, group) + lane_off;
    float* const ws_d2 = C.workspace + bw_group_offset(D, net, BW_D2, group) + lane_off;
    float* const ws_d1 = C.workspace + bw_group_offset(D, net, BW_D1, group) + lane_off;

    if (!net) __syncthreads();  // small4, the first chunk

    // this lane's B operands of layer 1, gathered per network (urgym_critic_grad.hip says why)
    uint32_t mrow = (uint32_t)m;
    formed(mrow);
    float xb[CIN_PAD / 2];
#pragma unroll
    for (int s = 0; s < CIN_PAD / 2; s++) xb[s] = row_feature(C, (size_t)mrow, 2 * s + h);
    if (!net && stores) {
#pragma unroll
      for (int s = 0; s < CIN_PAD / 2; s++) (C.workspace + bw_x_group_offset(D, group))[32 * (2 * s) + bw_s1_lane_offset(lane, 1)] = live ? xb[s] : 0.0f;
    }

    uint32_t m1[MW], m2[MW];
#pragma unroll
    for (int i = 0; i < MW; i++) m1[i] = 0, m2[i] = 0;

    // ---- layer 1 forward (critic_kernel's); h1 lives until layer 2 has run forward, its mask beyond
    float h1[HT * 16];
    // the chunk after the one in use travels in four parts (urgym_critic_grad.hip: staged)
    auto staged = [&](const float4* next, auto npf, auto next_is_tile, auto&& quarter) __attribute__((always_inline)) {
      constexpr int NPF = decltype(npf)::value, CH = (NPF + 3) / 4;
      constexpr bool TILE = decltype(next_is_tile)::value;
      float4* wn = wbuf[buf ^ 1];
      static_for<0, 4>([&](auto sg) __attribute__((always_inline)) {
        constexpr int S = decltype(sg)::value, I0 = S * CH, N = I0 + CH <= NPF ? CH : (NPF > I0 ? NPF - I0 : 0);
        f32x4 pf[N > 0 ? N : 1];  // (a native vector: copies of a float4 struct that a rounded() stands between stayed in scratch)
        static_for<0, N>([&](auto i) __attribute__((always_inline)) { pf[i] = *reinterpret_cast<const f32x4*>(next + CRITIC_THREADS * (I0 + i)); });
        quarter(sg);
        static_for<0, N>([&](auto i) __attribute__((always_inline)) {
          *reinterpret_cast<f32x4*>(wn + (TILE ? sbase + 4 * L2_ROW4 * (I0 + i) : tid + CRITIC_THREADS * (I0 + i))) = pf[i];
        });
      });
      __syncthreads();  // everyone has left this chunk (its buffer is the one after next) and the next chunk is in place
      buf ^= 1;
    };
    auto chunk1 = [&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      constexpr bool LAST = c + 1 == L1_CHUNKS;
      constexpr int NPF = LAST ? PF2 : PF1;
      const float4* wb = wbuf[buf];
      staged((LAST ? p2 : p1 + (c + 1) * C1_CHUNK4) + tid, std::integral_constant<int, NPF>(), std::integral_constant<bool, LAST>(), [&](auto sg) __attribute__((always_inline)) {
        constexpr int tt = decltype(sg)::value, t = 4 * c + tt;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const float4 b = sm4[(32 * t + 8 * g + 4 * h) / 4];
          acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
        }
#pragma unroll
        for (int sq = 0; sq < C1_STEPS4; sq++) {
          const float4 a = wb[(tt * C1_STEPS4 + sq) * 64 + lane];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xb[4 * sq + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xb[4 * sq + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xb[4 * sq + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xb[4 * sq + 3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; v++) h1[t * 16 + v] = fmaxf(acc[v], 0.0f);
        m1[t >> 1] |= relu_bits(acc) << (16 * (t & 1));
        if constexpr (tt & 1) formed(m1[t >> 1]);
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
        for (int v = 0; v < 16; v++) ws_h1[32 * bw_fwd_neuron(t, v, 0)] = live ? h1[t * 16 + v] : 0.0f;
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
      staged(next, std::integral_constant<int, PF2>(), std::true_type(), [&](auto sg) __attribute__((always_inline)) {
        constexpr int S = decltype(sg)::value;
#pragma unroll
        for (int sq = S * HT; sq < (S + 1) * HT; sq++) {  // sq = 4 u + g: registers 4 g .. 4 g + 3 of layer-1 tile u
          const float4 a = wb[sq * L2_ROW4];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h1[4 * sq + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h1[4 * sq + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h1[4 * sq + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h1[4 * sq + 3], acc, 0, 0, 0);
        }
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
        for (int v = 0; v < 16; v++) ws_h2[32 * bw_fwd_neuron(t, v, 0)] = live ? fmaxf(acc[v], 0.0f) : 0.0f;
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
      if (stores) C.workspace[bw_dq_offset(D, net, row)] = dqv;
      if (live && C.q) C.q[(size_t)net * M + m] = qn;
    }

    // d2 = mask2 ? w_q dq : 0 of this lane's neurons, as the pass below forms its B operands
    if (stores) {
#pragma unroll
      for (int t = 0; t < HT; t++) {
        const uint32_t bits = m2[t >> 1] >> (16 * (t & 1));
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const int n = bw_fwd_neuron(t, v, 0);
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
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < MW; i++) word = (t >> 1) == i ? m2[i] : word;
      const uint32_t bits = word >> (16 * (t & 1));
      const float4* wb = wbuf[buf] + abase;
      staged(next, npf, next_is_tile, [&](auto sg) __attribute__((always_inline)) {
        constexpr int g = decltype(sg)::value;
        const float4 wq = sm4[(2 * HP + 32 * t + 8 * g + 4 * h) / 4];
        const float wqr[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
        for (int r = 0; r < 4; r++) {  // one MFMA step: k = h is neuron 32 t + 8 g + 4 h + r of layer 2
          const float d2 = rounded(wqr[r] * dqv);  // (formed whatever the mask says: a product under a condition is a branch)
          const float b = (bits >> (4 * g + r)) & 1u ? d2 : 0.0f;
#pragma unroll
          for (int U = 0; U < HT / 4; U++) {
            const float4 a = wb[16 * U * L2_ROW4 + 8 * g + r];  // W1[32 t + 8 g + 4 h + r][128 U + 4 jj + c], c = 0 .. 3
            dacc[4 * U + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b, dacc[4 * U + 0], 0, 0, 0);
            dacc[4 * U + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b, dacc[4 * U + 1], 0, 0, 0);
            dacc[4 * U + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b, dacc[4 * U + 2], 0, 0, 0);
            dacc[4 * U + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b, dacc[4 * U + 3], 0, 0, 0);
          }
        }
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
          for (int c = 0; c < 4; c++) ws_d1[32 * bw_back_neuron(4 * U + c, v, 0)] = (live && ((bits >> c) & 1u)) ? dacc[4 * U + c][v] : 0.0f;
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stage 2
struct ReduceKParams {
  const float* ws;
  float* partial;  // the workspace again, for the partial sums (S > 1)
  BwDims d;
  float* grad[2][BW_TENSORS];
};

// Four consecutive rows of neuron n of an array: one float4.  n < limit, or the operand is +0 (the columns of x past 56).
__device__ __forceinline__ float4 operand4(const float* base, int n, int limit) {
  if (n >= limit) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return *reinterpret_cast<const float4*>(base + 32 * (size_t)n);
}

__global__ void __launch_bounds__(256) critic_backward_reduce_kernel(const ReduceKParams P) {
  const BwDims& D = P.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, i = lane & 31;
  int split, net, job0;
  bw_s2_block(D, blockIdx.x, &split, &net, &job0);
  const BwJob job = bw_job(D, job0 + wave);
  if (job.kind == BW_JOB_NONE) return;
  int R0, R1;
  bw_split_groups(D, split, &R0, &R1);
  float* dst[BW_TENSORS];
#pragma unroll
  for (int t = 0; t < BW_TENSORS; t++) dst[t] = D.S > 1 ? P.partial + bw_partial_offset(D, split, net) + bw_tensor_offset(D, t) : P.grad[net][t];

  if (job.kind == BW_JOB_HEAD) {
    const int n = 32 * job.ab + i;
    float acc = 0.0f;
    for (int R = R0; R < R1; R++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const size_t row = bw_s2_row(R, q, h);
        const float4 a = *reinterpret_cast<const float4*>(P.ws + bw_offset(D, net, BW_H2, row, n));
        const float4 d = *reinterpret_cast<const float4*>(P.ws + bw_dq_offset(D, net, row));
        acc = fmaf(a.x, d.x, acc), acc = fmaf(a.y, d.y, acc), acc = fmaf(a.z, d.z, acc), acc = fmaf(a.w, d.w, acc);
      }
    const float g = acc + __shfl_xor(acc, 32);
    if (h == 0 && n < D.H) dst[BW_G_WQ][n] = g;
    if (job.ab != 0) return;
    // g_bq of the split: one scalar out of up to 1024 terms of one sign, so its sum is kept in float64 and rounded once.  Lane (h, i)
    // adds row i of every second row group from R0 + h on, ascending; then the 64 lanes are added in a fixed butterfly.
    double dsum = 0.0;
    for (int R = R0 + h; R < R1; R += 2) dsum += (double)P.ws[bw_dq_offset(D, net, bw_s2_bq_row(R, i))];
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) dsum += __shfl_xor(dsum, step);
    if (lane == 0) dst[BW_G_BQ][0] = (float)dsum;
    return;
  }

  // a 64 x 64 block: A = d2 (g_W1) or d1 (g_W0), neurons 64 ab + 32 ia + i; B = h1, or x with 56 columns
  const bool w1 = job.kind == BW_JOB_W1;
  const int a_array = w1 ? BW_D2 : BW_D1, b_limit = w1 ? D.HP : BW_X;
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
      const size_t row = bw_s2_row(R, q, h);
      const float* abase = P.ws + bw_offset(D, net, a_array, row, 0);
      const float* bbase = w1 ? P.ws + bw_offset(D, net, BW_H1, row, 0) : P.ws + bw_x_offset(D, row, 0);
      float4 a[2], b[2];
      a[0] = operand4(abase, an, D.HP), a[1] = operand4(abase, an + 32, D.HP);
      b[0] = operand4(bbase, bn, b_limit), b[1] = operand4(bbase, bn + 32, b_limit);
#pragma unroll
      for (int ia = 0; ia < 2; ia++) {
#pragma unroll
        for (int jb = 0; jb < 2; jb++) {
          acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ia].x, b[jb].x, acc[ia][jb], 0, 0, 0);
          acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ia].y, b[jb].y, acc[ia][jb], 0, 0, 0);
          acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ia].z, b[jb].z, acc[ia][jb], 0, 0, 0);
          acc[ia][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ia].w, b[jb].w, acc[ia][jb], 0, 0, 0);
        }
        bsum[ia] = (((bsum[ia] + a[ia].x) + a[ia].y) + a[ia].z) + a[ia].w;
      }
    }
  const int columns = w1 ? D.H : D.in;
  float* gw = dst[w1 ? BW_G_W1 : BW_G_W0];
#pragma unroll
  for (int ia = 0; ia < 2; ia++) {
#pragma unroll
    for (int jb = 0; jb < 2; jb++) {
      const int j = bw_s2_column(job, jb, lane);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int n = bw_s2_neuron(job, ia, v, lane);
        if (n < D.H && j < columns) gw[(size_t)n * columns + j] = acc[ia][jb][v];  // padded rows and columns are never stored
      }
    }
    const float gb = bsum[ia] + __shfl_xor(bsum[ia], 32);
    const int n = an + 32 * ia;
    if (job.bb == 0 && h == 0 && n < D.H) dst[w1 ? BW_G_B1 : BW_G_B0][n] = gb;
  }
}

// ------------------------------------------------------------------------------------------------ stage 3
__global__ void __launch_bounds__(256) critic_backward_combine_kernel(const ReduceKParams P) {
  const BwDims& D = P.d;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * D.P) return;
  const int net = e >= D.P;
  const size_t r = e - (size_t)net * D.P;
  double sum = (double)P.partial[bw_partial_offset(D, 0, net) + r];  // at most 64 float32 terms: float64 adds them without an error of its own
  for (int s = 1; s < D.S; s++) sum += (double)P.partial[bw_partial_offset(D, s, net) + r];
  size_t at;
  const int t = bw_tensor_of(D, r, &at);
  P.grad[net][t][at] = (float)sum;
}

template <int HT>
void launch_rows(const BackwardKParams& P, hipStream_t s) {
  hipLaunchKernelGGL((critic_backward_rows_kernel<HT>), dim3(bw_s1_grid(P.d)), dim3(CRITIC_THREADS), 0, s, P);
}

}  // namespace

// Instances HT = 4 and 8, like the action gradient's and for its reason: the 16 HT accumulators of the pass back through layer 2.
bool critic_backward_supported(Critic* c) { return critic_packed(c).hidden <= CRITIC_GRAD_MAX_HIDDEN; }

uint64_t critic_backward_workspace_bytes(Critic* c, int count) {
  const CriticPacked buf = critic_packed(c);
  return (uint64_t)bw_dims(buf.in_features, buf.hidden, count).floats * sizeof(float);
}

int critic_backward_launches(int count) { return count > BW_SPLIT_ROWS ? 3 : 2; }

void critic_backward_launch(Critic* c, const CriticBackwardCall& call, hipStream_t s) {
  const CriticPacked buf = critic_packed(c);
  const int HT = (buf.hidden + 127) / 128 * 4;
  BackwardKParams P;
  P.w = reinterpret_cast<const float4*>(buf.weights);
  P.small = reinterpret_cast<const float4*>(buf.weights + critic_small_offset(buf));
  P.d = bw_dims(buf.in_features, buf.hidden, call.M);
  P.call = call;
  if (HT == 4) launch_rows<4>(P, s);
  else launch_rows<8>(P, s);
  ReduceKParams Q;
  Q.ws = call.workspace, Q.partial = call.workspace, Q.d = P.d;
  for (int net = 0; net < 2; net++)
    for (int t = 0; t < BW_TENSORS; t++) Q.grad[net][t] = call.grad[net][t];
  hipLaunchKernelGGL(critic_backward_reduce_kernel, dim3(bw_s2_grid(P.d)), dim3(256), 0, s, Q);
  if (P.d.S > 1) hipLaunchKernelGGL(critic_backward_combine_kernel, dim3((unsigned)((2 * P.d.P + 255) / 256)), dim3(256), 0, s, Q);
}

}  // namespace urgym
