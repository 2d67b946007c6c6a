// urgym_critic.hip — the twin Q-networks of the reference's SAC checkpoints (SB3 ContinuousCritic of MultiInputPolicy, train.py:40-48:
// q_i = L4(relu(L2(relu(L0(cat[features, action]))))), i = 0, 1) as one HIP kernel for MI355X (gfx950), with the minimum and the SAC
// target in its epilogue.
//
// The scheme is the actor's (urgym_actor.hip:1-31): float32 on v_mfma_f32_32x32x2_f32, weights as the A operand (32 neurons per tile
// on the lanes' rows), the rows of the batch as the B operand (row m on lane l & 31), layer 2's A packed on the host so that the
// layer-1 activations are consumed from the registers they were produced in, weights that all four waves re-read staged through
// double-buffered LDS chunks.  What differs:
//
//   input      achieved_goal | desired_goal | observation | action (SB3: cat([features, actions])), up to 53 floats: layer-1 K is
//              padded to 56 with zero weights, 28 MFMAs and 7 float4 reads per tile.  Rows come from explicit pointers, M of them;
//              a row's result depends on nothing but the row.
//   two nets   one launch, and the SAME wave runs qf0 and then qf1 on its 32 rows: the 28 input registers are gathered once and stay,
//              the 16 HT registers of h1 are reused.  The packed weights of both networks are one stream of chunks
//              (qf0: layer-1 chunks, layer-2 tiles; qf1: the same), so the double buffering runs across the seam: qf0's last
//              layer-2 tile prefetches qf1's first layer-1 chunk.
//   layer 3    one output per network: 16 fma per tile and lane right after the tile's MFMAs, one cross-lane add, the bias.
//   epilogue   q[2][M], q_min = fminf(q0, q1), target = reward + (gamma * not_done) * (q_min - ent_coef * log_prob): include/urgym.h
//              states the expression; no product of it is fused into the next operation (sac_target).
//
// This unit may contract a * b + c to fma, like urgym_actor.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <vector>

#include "urgym_critic.h"
#include "urgym_pack_host.h"

namespace urgym {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CRITIC_THREADS = 256;  // 4 waves
constexpr int CRITIC_ROWS = 128;     // rows per workgroup (32 per wave)
constexpr int CIN_PAD = 56;          // layer-1 K, padded with zero weights (in_features <= 53)
static_assert(CRITIC_THREADS == CRITIC_GEOMETRY_THREADS && CRITIC_ROWS == CRITIC_GEOMETRY_ROWS && CIN_PAD == CRITIC_GEOMETRY_CIN_PAD, "urgym_critic.h");
constexpr int C1_STEPS4 = CIN_PAD / 8;          // float4 reads per lane and layer-1 tile (4 MFMA steps, 2 k each)
constexpr int C1_TILE4 = C1_STEPS4 * 64;        // float4 per packed layer-1 tile
constexpr int C1_CHUNK4 = 4 * C1_TILE4;         // float4 per staged layer-1 chunk (4 tiles, 28 KB)

struct CriticKParams {
  const float4* w;      // per network: layer 1 packed [HT][C1_STEPS4][64 lanes] float4, then layer 2 packed [HT][HT * 4][64 lanes] float4
  const float4* small;  // per network: b0[HP] | b1[HP] | w_q[HP] | b_q, 0, 0, 0
  CriticCall call;
};

__device__ __forceinline__ float critic_feature(const CriticCall& C, size_t m, int k) {
  const int gd = C.goal_dim;
  if (k < gd) return C.achieved_goal[m * gd + k];
  if (k < 2 * gd) return C.desired_goal[m * gd + (k - gd)];
  k -= 2 * gd;
  if (k < C.obs_dim) return C.observation[m * C.obs_dim + k];
  k -= C.obs_dim;
  return k < 6 ? C.action[m * 6 + k] : 0.0f;
}

// A product that must be rounded before it is used: this unit is compiled with -ffp-contract=fast, under which the back end fuses a
// multiplication into the addition that consumes it whatever a pragma in the source says.  The empty statement makes the value
// opaque to the compiler and emits no instruction.
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// include/urgym.h, urgym_critic_evaluate: every operation rounds to float32 on its own, in this association
__device__ __forceinline__ float sac_target(float reward, float gamma, float not_done, float q_min, float ent_coef, const float* log_prob, size_t m) {
  float v = q_min;
  if (log_prob) v = q_min - rounded(ent_coef * log_prob[m]);
  const float g = rounded(gamma * not_done);
  return reward + rounded(g * v);
}

// HT = tiles of 32 neurons per hidden layer (4, 8, 12, 16), as in actor_kernel: up to HT = 8 two workgroups share a CU.
template <int HT>
__global__ void __launch_bounds__(CRITIC_THREADS, (HT <= 8 ? 2 : 1)) critic_kernel(const CriticKParams P) {
  constexpr int HP = HT * 32;
  constexpr int L2_TILE4 = HT * 4 * 64;  // float4 per packed layer-2 tile
  constexpr int BUF4 = C1_CHUNK4 > L2_TILE4 ? C1_CHUNK4 : L2_TILE4;
  constexpr int NET4 = HT * C1_TILE4 + HT * L2_TILE4;  // float4 per network in P.w
  constexpr int SMALL4 = (3 * HP + 4) / 4;             // float4 per network in P.small
  constexpr int L1_CHUNKS = HT / 4;
  constexpr int PF1 = C1_CHUNK4 / CRITIC_THREADS, PF2 = L2_TILE4 / CRITIC_THREADS;  // float4 per thread and staged chunk (7, HT)
  __shared__ float4 wbuf[2][BUF4];
  __shared__ float4 small4[2 * SMALL4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CriticCall& C = P.call;
  const int M = C.M;
  const size_t row0 = (size_t)blockIdx.x * CRITIC_ROWS;

  for (int i = tid; i < 2 * SMALL4; i += CRITIC_THREADS) small4[i] = P.small[i];
#pragma unroll
  for (int i = 0; i < PF1; i++) wbuf[0][tid + CRITIC_THREADS * i] = P.w[tid + CRITIC_THREADS * i];

  // this lane's B operands of layer 1: features 2 s + h of its row (h = lane >> 5: which of the two k of an MFMA step it supplies);
  // gathered once, used by both networks
  const int h = lane >> 5;
  const size_t row = row0 + wave * 32 + (lane & 31);
  const bool live = row < (size_t)M;
  const size_t m = live ? row : (size_t)M - 1;  // lanes past the end compute on the last row and store nothing
  float xb[CIN_PAD / 2];
#pragma unroll
  for (int s = 0; s < CIN_PAD / 2; s++) xb[s] = critic_feature(C, m, 2 * s + h);
  __syncthreads();

  const float* small = reinterpret_cast<const float*>(small4);
  float h1[HT * 16];
  float qv0 = 0.0f, qv1 = 0.0f;
  int buf = 0;  // the half of wbuf that holds the chunk in use

#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    const float4* p1 = P.w + (size_t)net * NET4;
    const float4* p2 = p1 + HT * C1_TILE4;
    const float4* sm4 = small4 + net * SMALL4;

    // ---- layer 1: h1 = relu(W0 x + b0), chunks of 4 tiles
#pragma unroll
    for (int c = 0; c < L1_CHUNKS; c++) {
      constexpr int PFN = PF1 > PF2 ? PF1 : PF2;
      const int pfn = c + 1 < L1_CHUNKS ? PF1 : PF2;  // (a constant: the loop is unrolled)
      const float4* next = (c + 1 < L1_CHUNKS ? p1 + (c + 1) * C1_CHUNK4 : p2) + tid;
      float4 pf[PFN];
#pragma unroll
      for (int i = 0; i < PFN; i++)
        if (i < pfn) pf[i] = next[CRITIC_THREADS * i];
      const float4* wb = wbuf[buf];
#pragma unroll
      for (int tt = 0; tt < 4; tt++) {
        const int t = 4 * c + tt;
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
      }
      float4* wn = wbuf[buf ^ 1];
#pragma unroll
      for (int i = 0; i < PFN; i++)
        if (i < pfn) wn[tid + CRITIC_THREADS * i] = pf[i];
      __syncthreads();  // everyone has left this chunk (its buffer is the one after next) and the next chunk is in place
      buf ^= 1;
    }

    // ---- layer 2 tile by tile, each tile straight into layer 3 (one output: 16 fma per tile and lane)
    float qsum = 0.0f;
    // one tile; meanwhile the chunk after it (npf float4 per thread at `next`) travels to the other half of wbuf
    auto tile2 = [&](int t, const float4* next, auto npf) __attribute__((always_inline)) {
      constexpr int NPF = decltype(npf)::value;
      float4 pf[NPF];
#pragma unroll
      for (int i = 0; i < NPF; i++) pf[i] = next[CRITIC_THREADS * i];
      const float4* wb = wbuf[buf];
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 b = sm4[(HP + 32 * t + 8 * g + 4 * h) / 4];
        acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
      }
#pragma unroll
      for (int sq = 0; sq < HT * 4; sq++) {  // sq = 4 u + g: registers 4 g .. 4 g + 3 of layer-1 tile u
        const float4 a = wb[sq * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h1[4 * sq + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h1[4 * sq + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h1[4 * sq + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h1[4 * sq + 3], acc, 0, 0, 0);
      }
      // layer 3 on this lane's 16 neurons of the tile, 32 t + 8 g + 4 h + r in register 4 g + r
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 w = sm4[(2 * HP + 32 * t + 8 * g + 4 * h) / 4];
        qsum = fmaf(w.x, fmaxf(acc[4 * g + 0], 0.0f), qsum);
        qsum = fmaf(w.y, fmaxf(acc[4 * g + 1], 0.0f), qsum);
        qsum = fmaf(w.z, fmaxf(acc[4 * g + 2], 0.0f), qsum);
        qsum = fmaf(w.w, fmaxf(acc[4 * g + 3], 0.0f), qsum);
      }
      float4* wn = wbuf[buf ^ 1];
#pragma unroll
      for (int i = 0; i < NPF; i++) wn[tid + CRITIC_THREADS * i] = pf[i];
      __syncthreads();
      buf ^= 1;
    };
#pragma unroll 1
    for (int t = 0; t + 1 < HT; t++) tile2(t, p2 + (size_t)(t + 1) * L2_TILE4 + tid, std::integral_constant<int, PF2>());
    // The last tile stages the other network's first layer-1 chunk: qf1's for qf0; qf0's again for qf1, which nobody reads (loads
    // and stores without a condition stay in registers; under one the compiler kept them in scratch).
    tile2(HT - 1, P.w + (net == 0 ? NET4 : 0) + tid, std::integral_constant<int, PF1>());
    // the two lane halves hold partial sums over different neurons
    const float qn = qsum + __shfl_xor(qsum, 32) + small[net * (SMALL4 * 4) + 3 * HP];
    if (net == 0) qv0 = qn; else qv1 = qn;
  }

  if (live && h == 0) {
    const float qm = fminf(qv0, qv1);
    if (C.q) C.q[m] = qv0, C.q[(size_t)M + m] = qv1;
    if (C.q_min) C.q_min[m] = qm;
    if (C.target) {
      const float not_done = (C.terminated && C.terminated[m]) ? 0.0f : 1.0f;
      C.target[m] = sac_target(C.reward[m], C.gamma, not_done, qm, C.ent_coef, C.log_prob, m);
    }
  }
}

template <int HT>
void launch(const CriticKParams& P, hipStream_t s) {
  const unsigned grid = (unsigned)(((size_t)P.call.M + CRITIC_ROWS - 1) / CRITIC_ROWS);
  hipLaunchKernelGGL((critic_kernel<HT>), dim3(grid), dim3(CRITIC_THREADS), 0, s, P);
}

}  // namespace

struct Critic {
  int in_features = 0, hidden = 0, ht = 0;
  float* d_weights = nullptr;  // both networks' packed layers, then both networks' small arrays
  size_t small_off = 0;        // in floats
};

int critic_create(const urgym_critic_desc* d, int in_features, Critic** out, char* err, size_t err_len) {
  auto refuse = [&](const char* what) {
    snprintf(err, err_len, "urgym_critic_create: %s", what);
    return (int)URGYM_ERR_ARG;
  };
  if (!d || !out) return refuse("null argument");
  if (d->n_critics != 2) return refuse("n_critics must be 2");
  if (d->reserved0 != 0) return refuse("reserved0 must be 0");
  for (const urgym_q_network& q : d->qf)
    if (!q.w0 || !q.b0 || !q.w1 || !q.b1 || !q.w_q || !q.b_q) return refuse("a weight or bias pointer is null");
  if (d->hidden_width <= 0 || d->hidden_width % 32 != 0 || d->hidden_width > 512)
    return refuse("hidden_width must be a multiple of 32 and at most 512");
  if (d->in_features != in_features || in_features > CIN_PAD) {
    char msg[200];
    snprintf(msg, sizeof(msg), "in_features is %d, but this env kind's achieved_goal | desired_goal | observation | action has %d", d->in_features,
             in_features);
    return refuse(msg);
  }
  const int H = d->hidden_width, in = d->in_features;
  const int HP = (H + 127) / 128 * 128, HT = HP / 32;
  Critic* c = new (std::nothrow) Critic();
  if (!c) return refuse("out of memory");
  c->in_features = in, c->hidden = H, c->ht = HT;
  const std::vector<float> w = pack_critic_host(d, &c->small_off);  // the packing loops: urgym_pack_host.h
  hipError_t e = hipMalloc((void**)&c->d_weights, w.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(c->d_weights, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    snprintf(err, err_len, "urgym_critic_create: %s", hipGetErrorString(e));
    critic_destroy(c);
    return URGYM_ERR_HIP;
  }
  *out = c;
  return URGYM_OK;
}

void critic_destroy(Critic* c) {
  if (!c) return;
  if (c->d_weights) hipFree(c->d_weights);
  delete c;
}

int critic_in_features(const Critic* c) { return c->in_features; }
CriticPacked critic_packed(Critic* c) { return CriticPacked{c->d_weights, c->small_off + 2 * ((size_t)c->ht * 32 * 3 + 4), c->in_features, c->hidden}; }

void critic_launch(Critic* c, const CriticCall& call, hipStream_t s) {
  CriticKParams P;
  P.w = reinterpret_cast<const float4*>(c->d_weights);
  P.small = reinterpret_cast<const float4*>(c->d_weights + c->small_off);
  P.call = call;
  switch (c->ht) {
    case 4: launch<4>(P, s); break;
    case 8: launch<8>(P, s); break;
    case 12: launch<12>(P, s); break;
    default: launch<16>(P, s); break;
  }
}

}  // namespace urgym
