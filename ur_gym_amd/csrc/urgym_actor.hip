// urgym_actor.hip — the SAC actor of the reference's checkpoints (SB3 MultiInputPolicy: tanh(mu(relu(L2(relu(L0(x)))))),
// model_test.py:21,41) as one HIP kernel for MI355X (gfx950), and the records of a closed-loop rollout that ride in the same launch.
//
// float32 in, float32 weights, float32 accumulate on the f32-input matrix instruction v_mfma_f32_32x32x2_f32: D[32 x 32] +=
// A[32 x 2] B[2 x 32], bitwise a k-ordered fmaf chain.  Weights are the A operand (rows = neurons), activations the B operand
// (columns = environments), so a result tile has its ENVIRONMENT on the lane (l & 31) and 16 neurons in the lane's registers:
// register v of lane l holds neuron 8 (v >> 2) + 4 (l >> 5) + (v & 3) of the tile.  The next layer sums over exactly that index,
// and which two k an MFMA step pairs is free as long as A is packed to match: step (u, g, r) of layer 2 pairs neurons
// 32 u + 8 g + r (lanes 0..31) and 32 u + 8 g + 4 + r (lanes 32..63), both of which sit in register 4 g + r of the lane that has
// to supply them.  So activations never leave the registers: no LDS round trip, no lane movement between the layers.
//
//   workgroup  4 waves x 32 envs = 128 envs; every wave runs the whole network for its 32 envs.
//   layer 1    48 (= in_features padded with zero weights) x HP, HP = hidden width padded to a multiple of 128: 24 MFMAs per tile of
//              32 neurons; the inputs are gathered straight from the bound observation buffers (24 floats per lane).
//   layer 2    HP x HP, HP / 2 MFMAs per tile.  Its output tile goes through ReLU and at once into
//   layer 3    6 x HP on the vector ALU (96 fma per tile and lane, in the shadow of the next tile's MFMAs): a 6-row A operand would
//              waste 26 of the 32 MFMA rows.  The two lane halves hold partial sums over different neurons; one cross-lane add
//              joins them before bias, tanh and the store.
//   weights    packed on the host (actor_create) into the order the lanes read them, one float4 per lane and 4 MFMA steps.  What
//              all four waves re-read goes through LDS: chunks of 4 layer-1 tiles (24 KB) or one layer-2 tile (HP x 128 B), double
//              buffered -- the next chunk is loaded into registers before the MFMAs of the current one and written to the other
//              buffer after them, one barrier per chunk.  Biases and the layer-3 weights (8 HP + 8 floats) are staged once.
//
// The stochastic half (SB3's SquashedDiagGaussianDistribution; include/urgym.h states the semantics and the noise) is a second set
// of instances of the same kernel, actor_kernel<HT, true>: layer 3 gets a second head, log_std (96 more fma per tile and lane, 12 sums
// per env; its weights sit behind w_mu in the same packing, 14 HP + 16 floats staged once), and the epilogue draws the env's noise
// (Philox4x32-10, urgym_philox.h: the reset sampler's function), squashes and evaluates the log-probability.  The deterministic
// instances actor_kernel<HT, false> are compiled from the same text they were before.  URGYM_SAMPLE_UNIFORM needs no network:
// uniform_kernel draws and records.
//
// This unit may contract a * b + c to fma (the step kernels in urgym_hip.hip may not).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <vector>

#include "urgym_actor.h"
#include "urgym_pack_host.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int ACTOR_THREADS = 256;   // 4 waves
constexpr int ACTOR_ENVS = 128;      // envs per workgroup (32 per wave)
constexpr int IN_PAD = 48;           // layer-1 K, padded with zero weights (in_features <= 47)
constexpr int L1_STEPS4 = IN_PAD / 8;            // float4 reads per lane and layer-1 tile (4 MFMA steps, 2 k each)
constexpr int L1_TILE4 = L1_STEPS4 * 64;         // float4 per packed layer-1 tile
constexpr int L1_CHUNK4 = 4 * L1_TILE4;          // float4 per staged layer-1 chunk (4 tiles)

struct ActorKParams {
  const float4* p1;    // layer 1, packed [HT][L1_STEPS4][64 lanes] float4
  const float4* p2;    // layer 2, packed [HT][HT * 4][64 lanes] float4
  const float4* small; // b0[HP] | b1[HP] | w_mu as [HP / 4][6][4] | b_mu[8] | w_log_std as [HP / 4][6][4] | b_log_std[8]
  ActorEnv env;
  float* actions;      // null: records only
  int record;          // pass is valid
  ActorPass pass;
};
struct ActorSParams : ActorKParams {  // the sampling instances and uniform_kernel
  ActorSample how;
};

// NOISE_TAG, TWO_M24, HALF_LOG_2PI, noise_words, store6: urgym_policy_noise.h, shared with the backward pass
constexpr float SIX_LOG_2 = 4.15888308335967186f;

__device__ __forceinline__ float feature(const ActorEnv& E, size_t e, int k) {
  const int gd = E.goal_dim;
  if (k < gd) return E.achieved_goal[e * gd + k];
  if (k < 2 * gd) return E.desired_goal[e * gd + (k - gd)];
  k -= 2 * gd;
  return k < E.obs_dim ? E.observation[e * E.obs_dim + k] : 0.0f;
}

__device__ __forceinline__ void copy_rows(float* dst, const float* src, size_t first, size_t count, int tid) {
  if (!dst) return;
  for (size_t i = tid; i < count; i += ACTOR_THREADS) dst[first + i] = src[first + i];
}

// The records of envs [env0, env0 + cnt): see ActorPass.  Reads the bound buffers, which hold the result of step k - 1 and the
// observations step k will act on.
__device__ void record_rows(const ActorEnv& E, const ActorPass& R, int env0, int cnt, int tid) {
  const size_t od = E.obs_dim, gd = E.goal_dim;
  if (R.k < R.num_steps) {
    copy_rows(R.obs, E.observation, env0 * od, cnt * od, tid);
    copy_rows(R.ach, E.achieved_goal, env0 * gd, cnt * gd, tid);
    copy_rows(R.des, E.desired_goal, env0 * gd, cnt * gd, tid);
  }
  const bool summary = R.ep_done != nullptr;
  if (R.k == 0) {
    if (summary && tid < cnt) {
      const int e = env0 + tid;
      R.ep_done[e] = 0;
      if (R.ep_return) R.ep_return[e] = 0.0;
      if (R.ep_last) R.ep_last[e] = 0;
      if (R.ep_success) R.ep_success[e] = 0;
    }
    return;
  }
  if (tid < cnt) {
    const int e = env0 + tid;
    const float r = E.reward[e];
    const uint8_t term = E.terminated[e], succ = E.is_success[e];
    if (R.reward) R.reward[e] = r;
    if (R.terminated) R.terminated[e] = term;
    if (R.truncated) R.truncated[e] = E.truncated[e];
    if (R.is_success) R.is_success[e] = succ;
    if (R.collision) R.collision[e] = E.collision[e];
    if (summary && !R.ep_done[e]) {  // model_test.py:42-49: reward summed while the episode runs; closed at `steps == last or terminated`
      if (R.ep_return) R.ep_return[e] += (double)r;
      if (term || R.k == R.num_steps) {
        if (R.ep_success) R.ep_success[e] = succ;
        if (R.ep_last) R.ep_last[e] = R.k - 1;
        R.ep_done[e] = 1;
      }
    }
  }
  if (R.final_obs && E.auto_reset) {
    for (size_t i = tid; i < cnt * od; i += ACTOR_THREADS) {
      const size_t e = env0 + i / od;
      if (E.terminated[e] | E.truncated[e]) R.final_obs[env0 * od + i] = E.final_observation[env0 * od + i];
    }
  }
}

// HT = tiles of 32 neurons per hidden layer (4, 8, 12, 16).  Up to HT = 8 the kernel fits 256 registers and 80 KB of LDS: two
// workgroups per CU, i.e. two waves per SIMD, one of which computes while the other waits at a barrier or for its weights.
// SAMPLE: the log_std head next to mu and the sampling epilogue (MEAN or GAUSSIAN; P.how).
template <int HT, bool SAMPLE>
__global__ void __launch_bounds__(ACTOR_THREADS, (HT <= 8 ? 2 : 1))
actor_kernel(const std::conditional_t<SAMPLE, ActorSParams, ActorKParams> P) {
  constexpr int HP = HT * 32;
  constexpr int L2_TILE4 = HT * 4 * 64;  // float4 per packed layer-2 tile
  constexpr int BUF4 = L1_CHUNK4 > L2_TILE4 ? L1_CHUNK4 : L2_TILE4;
  constexpr int HEAD4 = (HP * 6 + 8) / 4;  // float4 per layer-3 head: weights, then the bias
  constexpr int SMALL4 = (HP * 2) / 4 + (SAMPLE ? 2 : 1) * HEAD4;
  constexpr int L1_CHUNKS = HT / 4;
  constexpr int PF1 = L1_CHUNK4 / ACTOR_THREADS, PF2 = L2_TILE4 / ACTOR_THREADS;  // float4 per thread and staged chunk (6, HT)
  constexpr int PF = PF1 > PF2 ? PF1 : PF2;
  __shared__ float4 wbuf[2][BUF4];
  __shared__ float4 small4[SMALL4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = P.env.N;
  const int env0 = blockIdx.x * ACTOR_ENVS;
  if (P.record) record_rows(P.env, P.pass, env0, min(ACTOR_ENVS, N - env0), tid);
  if (!P.actions) return;

  for (int i = tid; i < SMALL4; i += ACTOR_THREADS) small4[i] = P.small[i];
#pragma unroll
  for (int i = 0; i < PF1; i++) wbuf[0][tid + ACTOR_THREADS * i] = P.p1[tid + ACTOR_THREADS * i];

  // this lane's B operands of layer 1: features 2 s + h of env j (h = lane >> 5: which of the two k of an MFMA step it supplies)
  const int h = lane >> 5;
  const int env = env0 + wave * 32 + (lane & 31);
  const bool live = env < N;
  const size_t e = live ? env : N - 1;  // lanes past the end compute on the last env and store nothing
  float xb[IN_PAD / 2];
#pragma unroll
  for (int s = 0; s < IN_PAD / 2; s++) xb[s] = feature(P.env, e, 2 * s + h);
  __syncthreads();

  const float* small = reinterpret_cast<const float*>(small4);
  float h1[HT * 16];
  float4 pf[PF];

  // ---- layer 1: h1 = relu(W0 x + b0), chunks of 4 tiles
#pragma unroll
  for (int c = 0; c < L1_CHUNKS; c++) {
    if (c + 1 < L1_CHUNKS) {
#pragma unroll
      for (int i = 0; i < PF1; i++) pf[i] = P.p1[(c + 1) * L1_CHUNK4 + tid + ACTOR_THREADS * i];
    } else {
#pragma unroll
      for (int i = 0; i < PF2; i++) pf[i] = P.p2[tid + ACTOR_THREADS * i];
    }
    const float4* wb = wbuf[c & 1];
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      const int t = 4 * c + tt;
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 b = small4[(32 * t + 8 * g + 4 * h) / 4];
        acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
      }
#pragma unroll
      for (int sq = 0; sq < L1_STEPS4; sq++) {
        const float4 a = wb[(tt * L1_STEPS4 + sq) * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xb[4 * sq + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xb[4 * sq + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xb[4 * sq + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xb[4 * sq + 3], acc, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 16; v++) h1[t * 16 + v] = fmaxf(acc[v], 0.0f);
    }
    float4* wn = wbuf[(c + 1) & 1];
    if (c + 1 < L1_CHUNKS) {
#pragma unroll
      for (int i = 0; i < PF1; i++) wn[tid + ACTOR_THREADS * i] = pf[i];
    } else {
#pragma unroll
      for (int i = 0; i < PF2; i++) wn[tid + ACTOR_THREADS * i] = pf[i];
    }
    __syncthreads();  // everyone has left chunk c (its buffer is the one after next) and chunk c + 1 is in place
  }

  // ---- layer 2 tile by tile, each tile straight into layer 3
  float mu[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float ls[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // SAMPLE only
  // layer 3 of tile t on r = this lane's 16 relu'd neurons of the tile: w_mu packed [neuron / 4][6][neuron % 4]; the log_std head
  // (SAMPLE) has the same packing, one head further
  auto layer3 = [&](const f32x16& r, int t) {
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
  };
  f32x16 prev;  // SAMPLE only: the tile before, through ReLU
#pragma unroll 1
  for (int t = 0; t < HT; t++) {
    const int cur = (L1_CHUNKS + t) & 1;
    const float4* next = P.p2 + (size_t)(t + 1 < HT ? t + 1 : t) * L2_TILE4 + tid;  // (the last trip re-stages its own tile: unread)
#pragma unroll
    for (int i = 0; i < PF2; i++) pf[i] = next[ACTOR_THREADS * i];
    const float4* wb = wbuf[cur];
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 b = small4[(HP + 32 * t + 8 * g + 4 * h) / 4];
      acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
    }
    if constexpr (SAMPLE) {
      // Twice the layer-3 work does not fit behind the other wave's MFMAs any more (measured: none of it hid), so it is software
      // pipelined: tile t - 1 goes through layer 3 next to the MFMAs of tile t, which do not depend on it -- each MFMA waits 64
      // cycles for the one before, and the vector ALU fills those gaps.  Same fma order per output as the deterministic instance.
      if (t > 0) layer3(prev, t - 1);
    }
#pragma unroll
    for (int sq = 0; sq < HT * 4; sq++) {  // sq = 4 u + g: registers 4 g .. 4 g + 3 of layer-1 tile u
      const float4 a = wb[sq * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h1[4 * sq + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h1[4 * sq + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h1[4 * sq + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h1[4 * sq + 3], acc, 0, 0, 0);
    }
    if constexpr (SAMPLE) {
#pragma unroll
      for (int v = 0; v < 16; v++) prev[v] = fmaxf(acc[v], 0.0f);
    } else {
      // layer 3, this lane's 16 neurons of the tile: w_mu packed [neuron / 4][6][neuron % 4]
      const float4* wm = small4 + (2 * HP) / 4 + (size_t)((32 * t + 4 * h) / 4) * 6;
#pragma unroll
      for (int g = 0; g < 4; g++) {
#pragma unroll
        for (int o = 0; o < 6; o++) {
          const float4 w = wm[2 * g * 6 + o];
          mu[o] = fmaf(w.x, fmaxf(acc[4 * g + 0], 0.0f), mu[o]);
          mu[o] = fmaf(w.y, fmaxf(acc[4 * g + 1], 0.0f), mu[o]);
          mu[o] = fmaf(w.z, fmaxf(acc[4 * g + 2], 0.0f), mu[o]);
          mu[o] = fmaf(w.w, fmaxf(acc[4 * g + 3], 0.0f), mu[o]);
        }
      }
    }
    float4* wn = wbuf[cur ^ 1];
#pragma unroll
    for (int i = 0; i < PF2; i++) wn[tid + ACTOR_THREADS * i] = pf[i];
    __syncthreads();
  }
  if constexpr (SAMPLE) layer3(prev, HT - 1);

  if constexpr (!SAMPLE) {
    float act[6];
#pragma unroll
    for (int o = 0; o < 6; o++) act[o] = tanhf(mu[o] + __shfl_xor(mu[o], 32) + small[HP * 8 + o]);
    if (live && h == 0) {
      float2* out = reinterpret_cast<float2*>(P.actions + (size_t)env * 6);
      out[0] = make_float2(act[0], act[1]);
      out[1] = make_float2(act[2], act[3]);
      out[2] = make_float2(act[4], act[5]);
    }
  } else {
    // Both lane halves hold the env's 12 sums after the cross-lane add and run the same epilogue; half 0 stores the action and the
    // log-probability, half 1 the three optional records.
    const ActorSample& S = P.how;
    const bool gauss = S.mode == URGYM_SAMPLE_GAUSSIAN;
    float eps[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (gauss) {
      float m[6];
      noise_words(S.seed, S.draw, (uint32_t)env, m);
#pragma unroll
      for (int p = 0; p < 3; p++) {  // Box-Muller: u1 in (0, 1], u2 in [0, 1), both exact
        const float r = sqrtf(-2.0f * logf((m[2 * p] + 1.0f) * TWO_M24));
        const float turn = 2.0f * (m[2 * p + 1] * TWO_M24);  // angle / pi: exact
        eps[2 * p] = r * cospif(turn);
        eps[2 * p + 1] = r * sinpif(turn);
      }
    }
    float mean[6], lstd[6], act[6];
    float lp = 0.0f;
#pragma unroll
    for (int o = 0; o < 6; o++) {
      mean[o] = mu[o] + __shfl_xor(mu[o], 32) + small[HP * 8 + o];  // the deterministic instance's expression: MEAN is bitwise that path
      lstd[o] = fminf(fmaxf(ls[o] + __shfl_xor(ls[o], 32) + small[HP * 14 + 8 + o], -20.0f), 2.0f);
      act[o] = tanhf(gauss ? fmaf(expf(lstd[o]), eps[o], mean[o]) : mean[o]);
      lp += -0.5f * eps[o] * eps[o] - lstd[o] - HALF_LOG_2PI - logf(1.0f - act[o] * act[o] + 1e-6f);
    }
    if (live && h == 0) {
      store6(P.actions, (size_t)env, act);
      if (S.log_prob) S.log_prob[env] = lp;
    }
    if (live && h == 1) {
      if (S.noise) store6(S.noise, (size_t)env, eps);
      if (S.log_std) store6(S.log_std, (size_t)env, lstd);
      if (S.mean_action) {
#pragma unroll
        for (int o = 0; o < 6; o++) mean[o] = tanhf(mean[o]);
        store6(S.mean_action, (size_t)env, mean);
      }
    }
  }
}

// URGYM_SAMPLE_UNIFORM: SAC's warm-up before learning_starts.  No forward pass; the records ride here as they do in actor_kernel,
// with the same geometry (128 envs per workgroup).
__global__ void __launch_bounds__(ACTOR_THREADS) uniform_kernel(const ActorSParams P) {
  const int tid = threadIdx.x;
  const int N = P.env.N;
  const int env0 = blockIdx.x * ACTOR_ENVS;
  if (P.record) record_rows(P.env, P.pass, env0, min(ACTOR_ENVS, N - env0), tid);
  const int env = env0 + tid;
  if (!P.actions || tid >= ACTOR_ENVS || env >= N) return;
  const ActorSample& S = P.how;
  float u[6], act[6];
  noise_words(S.seed, S.draw, (uint32_t)env, u);
#pragma unroll
  for (int o = 0; o < 6; o++) {
    u[o] *= TWO_M24;             // exact
    act[o] = 2.0f * u[o] - 1.0f;  // exact: a multiple of 2^-23 in [-1, 1)
  }
  store6(P.actions, (size_t)env, act);
  if (S.log_prob) S.log_prob[env] = -SIX_LOG_2;
  if (S.noise) store6(S.noise, (size_t)env, u);
}

template <int HT, bool SAMPLE, class Params>
void launch(const Params& P, hipStream_t s) {
  const unsigned grid = (unsigned)((P.env.N + ACTOR_ENVS - 1) / ACTOR_ENVS);
  hipLaunchKernelGGL((actor_kernel<HT, SAMPLE>), dim3(grid), dim3(ACTOR_THREADS), 0, s, P);
}

}  // namespace

struct Actor {
  int in_features = 0, hidden = 0, ht = 0, num_envs = 0;
  float* d_weights = nullptr;  // p1 | p2 | small
  size_t p2_off = 0, small_off = 0;  // in floats
  bool has_log_std = false;    // the second head of `small` is filled (actor_set_log_std); zeros until then
  float* d_actions = nullptr;  // [N][6]
  uint8_t* d_done = nullptr;   // [N]
};

int actor_create(const urgym_actor_desc* d, int in_features, int num_envs, Actor** out, char* err, size_t err_len) {
  auto refuse = [&](const char* what) {
    snprintf(err, err_len, "urgym_actor_create: %s", what);
    return (int)URGYM_ERR_ARG;
  };
  if (!d || !out) return refuse("null argument");
  if (!d->w0 || !d->b0 || !d->w1 || !d->b1 || !d->w_mu || !d->b_mu) return refuse("a weight or bias pointer is null");
  if (d->reserved0 != 0) return refuse("reserved0 must be 0");
  if (d->action_dim != 6) return refuse("action_dim must be 6");
  if (d->hidden_width <= 0 || d->hidden_width % 32 != 0 || d->hidden_width > 512)
    return refuse("hidden_width must be a multiple of 32 and at most 512");
  if (d->in_features != in_features || in_features > IN_PAD) {
    char msg[160];
    snprintf(msg, sizeof(msg), "in_features is %d, but this env kind's achieved_goal | desired_goal | observation has %d", d->in_features, in_features);
    return refuse(msg);
  }
  const int H = d->hidden_width, in = d->in_features;
  const int HP = (H + 127) / 128 * 128, HT = HP / 32;
  Actor* a = new (std::nothrow) Actor();
  if (!a) return refuse("out of memory");
  a->in_features = in, a->hidden = H, a->ht = HT, a->num_envs = num_envs;
  const std::vector<float> w = pack_actor_host(d, &a->p2_off, &a->small_off);  // the packing loops: urgym_pack_host.h

  hipError_t e = hipMalloc((void**)&a->d_weights, w.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(a->d_weights, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&a->d_actions, sizeof(float) * 6 * (size_t)num_envs);
  if (e == hipSuccess) e = hipMalloc((void**)&a->d_done, (size_t)num_envs);
  if (e != hipSuccess) {
    snprintf(err, err_len, "urgym_actor_create: %s", hipGetErrorString(e));
    actor_destroy(a);
    return URGYM_ERR_HIP;
  }
  *out = a;
  return URGYM_OK;
}

int actor_set_log_std(Actor* a, const float* w_ls, const float* b_ls, char* err, size_t err_len) {
  const int H = a->hidden, HP = a->ht * 32;
  const std::vector<float> head = pack_log_std_host(H, HP, w_ls, b_ls);
  const hipError_t e = hipMemcpy(a->d_weights + a->small_off + (size_t)HP * 8 + 8, head.data(), head.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    snprintf(err, err_len, "urgym_actor_set_log_std: %s", hipGetErrorString(e));
    return URGYM_ERR_HIP;
  }
  a->has_log_std = true;
  return URGYM_OK;
}

void actor_destroy(Actor* a) {
  if (!a) return;
  for (void* p : {(void*)a->d_weights, (void*)a->d_actions, (void*)a->d_done})
    if (p) hipFree(p);
  delete a;
}

int actor_in_features(const Actor* a) { return a->in_features; }
bool actor_has_log_std(const Actor* a) { return a->has_log_std; }
void actor_mark_log_std(Actor* a) { a->has_log_std = true; }
ActorPacked actor_packed(Actor* a) { return ActorPacked{a->d_weights, a->small_off + (size_t)a->ht * 32 * 14 + 16, a->in_features, a->hidden}; }
float* actor_action_scratch(Actor* a) { return a->d_actions; }
uint8_t* actor_done_scratch(Actor* a) { return a->d_done; }

namespace {

void fill_params(ActorKParams& P, Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass) {
  P.p1 = reinterpret_cast<const float4*>(a->d_weights);
  P.p2 = reinterpret_cast<const float4*>(a->d_weights + a->p2_off);
  P.small = reinterpret_cast<const float4*>(a->d_weights + a->small_off);
  P.env = env;
  P.actions = actions;
  P.record = pass != nullptr;
  if (pass) P.pass = *pass; else memset(&P.pass, 0, sizeof(P.pass));
}

}  // namespace

void actor_launch(Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass, hipStream_t s) {
  ActorKParams P;
  fill_params(P, a, env, actions, pass);
  switch (a->ht) {
    case 4: launch<4, false>(P, s); break;
    case 8: launch<8, false>(P, s); break;
    case 12: launch<12, false>(P, s); break;
    default: launch<16, false>(P, s); break;
  }
}

void actor_launch_sampled(Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass, const ActorSample& how, hipStream_t s) {
  ActorSParams P;
  fill_params(P, a, env, actions, pass);
  P.how = how;
  if (how.mode == URGYM_SAMPLE_UNIFORM) {
    const unsigned grid = (unsigned)((env.N + ACTOR_ENVS - 1) / ACTOR_ENVS);
    hipLaunchKernelGGL(uniform_kernel, dim3(grid), dim3(ACTOR_THREADS), 0, s, P);
    return;
  }
  switch (a->ht) {
    case 4: launch<4, true>(P, s); break;
    case 8: launch<8, true>(P, s); break;
    case 12: launch<12, true>(P, s); break;
    default: launch<16, true>(P, s); break;
  }
}

}  // namespace urgym
