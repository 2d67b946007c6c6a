// urgym_mlp_grad.h — the device code the three gradient units share: urgym_critic_grad.hip (d min Q / da), urgym_critic_backward.hip
// (the Q-loss parameter gradients) and urgym_actor_backward.hip (the policy-loss parameter gradients).  All three run a two-hidden-layer
// MLP forward on its packed buffer (urgym_pack_map.h: the actor's and the critic's layers 1 and 2 have one layout), keep the ReLU masks
// as bits and pass back through layer 2 with the transposed A operand; the two parameter-gradient units then sum over the rows in a
// stage 2 and a stage 3 of one shape (urgym_backward_map.h).  Device code only: __device__ __forceinline__ function templates over
// compile-time parameters, which take the LDS buffers, the lane constants and the register arrays by reference, so that each kernel's
// text is what it was with the blocks written out in its unit.
//
// Shared, stage 1 (4 waves of 32 rows, v_mfma_f32_32x32x2_f32):
//   staged                     the double-buffered step: the next chunk travels in four parts around four quarters of the work
//   layer1_tile                bias, MFMA, ReLU into h1, the mask word of one layer-1 tile
//   layer2_forward_quarter     a quarter of z2 of one staged tile from h1
//   mask_tile                  the mask bits of a tile that is named at run time
//   layer2_backward_quarter    W1^T against the four B values of an MFMA step, which the caller forms
// Shared, stages 2 and 3 (over the BackwardMap of the unit): operand4, gemm_step and gemm_store (the 64 x 64 block: a step of the K loop with
// the bias sums, the guarded stores), lane_sum (the float64 butterfly of the head biases), combine_element.
//
// Deliberately per unit, because it is what tells the three apart: the feature gather (the critic's has the action columns); layer 3 (one
// w_q chain against twelve head chains); the upstream gradient and how B is formed from it (w_q alone, w_q dq, or head_back); the
// sampling epilogue; the action-column pass of critic_grad; the head jobs of stage 2; each kernel's __launch_bounds__ and parameter
// struct (a kernel's symbol names its parameter type); what the last pass back stages (the other network's first chunk, or nothing);
// the two-network loop.  Nothing here branches at run time on which unit calls it.
//
// Still written out in each unit although the text is the same, because as a function here each changed the kernels' machine code
// (compiled and compared kernel by kernel against the units with everything written out; profiles/r6/device_code_identity.txt):
//   the bias load that opens a layer-2 tile    as a function: another instruction order in the layer-2 loop of the HT = 8 instances
//   the mask word put after a layer-2 tile     as a function: two registers of the HT = 4 instance change places
//   the d1 store loop                          with `live` as an argument, or the store as a callable: the condition comes out of the
//                                              optimiser inverted and the register allocation of the whole kernel with it
//   the lane arithmetic of abase and sbase     as a function: the address of the staging store is put together in another order
//   the loop over the layer-1 chunks           as a function that is handed the layer pointers: other scalar registers throughout the
//                                              actor's kernels, which read the pointers from the kernel arguments where they use them
//   the K loop of the 64 x 64 block            the whole block as one function, however its arguments were passed, cost the critic's
//                                              reduce kernel 2 to 10 VGPRs and with them a wave of occupancy (64 -> 66 .. 74, 4 -> 3);
//                                              with the loop and its operand addresses in the unit the registers are the parent's
// They are three, four, nine, three, ten and fourteen lines.  layer2_backward_quarter takes its B values through a callable it evaluates
// inside the step loop for the same reason: four values formed ahead of the loop moved the rounded() products and changed both instances.
//
// The transposed A operand.  A packed layer-2 tile holds W1[32 t + n][j] in float (j & 3) of the float4 of read row sq = j >> 3 and
// lane 32 ((j >> 2) & 1) + n: four CONSECUTIVE j of one neuron n are one float4.  So one ds_read_b128 feeds FOUR MFMAs if the output
// rows are dealt out accordingly: accumulator 4 U + c, register v, lane half h holds dh1 of neuron j = 128 U + 8 v + 4 h + c -- which
// is exactly where the forward pass left the mask bit of that neuron (tile 4 U + (v >> 2), register 4 (v & 3) + c, the same lane), so
// the masks need no lane movement either.  In the forward layout [sq][64 lanes] the 16 lanes of a ds_read_b128 group would then sit
// 128 floats apart on the same four banks; the staged tile is therefore laid out with rows of 66 float4 and lane l at l + (l >> 5):
// the float4 slot (address mod 16) of A-lane i becomes jj(i) mod 16 + const, jj(i) = 8 (i >> 3) + 2 (i & 3) + ((i >> 2) & 1), which
// is distinct over each of the four lane groups of ds_read_b128, and the forward read (slot = lane + (lane >> 5) + const) stays
// conflict-free as well.  Only the LDS image is padded; the packed buffer in memory is untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "urgym_backward_map.h"

namespace urgym {
namespace mlp_grad {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int L2_ROW4 = 66;  // float4 per read row of a staged layer-2 tile: 64 lanes, one slot between the halves, one of padding

// where float4 (read row sq, lane l) of a packed layer-2 tile lies in its staged image
__device__ __forceinline__ int l2_slot(int sq, int l) { return sq * L2_ROW4 + l + (l >> 5); }

// bit v = acc[v] > 0: a pre-activation of exactly 0 has derivative 0 (torch's relu), and so has NaN
__device__ __forceinline__ uint32_t relu_bits(const f32x16 acc) {
  uint32_t bits = 0;
#pragma unroll
  for (int v = 0; v < 16; v++) bits |= (acc[v] > 0.0f ? 1u : 0u) << v;
  return bits;
}

// f(0), ..., f(N - 1) with the index a constant from the start: a prefetch array indexed so is registers in every pass
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    static_for<I + 1, N>(f);
  }
}

// Makes a value opaque to the optimiser where it is complete (an identity quad permutation, one v_mov_dpp).  The mask words need it:
// left to itself the compiler keeps the 16 floats of a tile alive and compares where a bit is used, a pass later, and spills them.
__device__ __forceinline__ void formed(uint32_t& word) { word = (uint32_t)__builtin_amdgcn_mov_dpp((int)word, 0xE4, 0xF, 0xF, true); }

// a result that must be rounded before it is used (urgym_critic.hip: rounded)
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// What a thread is in stage 1, besides its row.  Each kernel fills it in its own text (see above):
//   const int ai = lane & 31, jj = 8 * (ai >> 3) + 2 * (ai & 3) + ((ai >> 2) & 1);
//   const int abase = (jj >> 1) * L2_ROW4 + (jj & 1) * 33 + 4 * h;
//   const int sbase = l2_slot(tid >> 6, tid & 63);
struct Lane {
  int tid, lane, h;  // h: the lane half, k of the MFMA step
  int abase;         // this lane as an A lane of the backward pass: output row i = lane & 31 is input neuron 4 jj + c of its group of 128, k = h
  int sbase;         // the staging slot of float4 tid + 256 i of a layer-2 tile: read row (tid >> 6) + 4 i, lane tid & 63
};

// ------------------------------------------------------------------------------------------------ stage 1
// The chunk after the one in use (NPF float4 per thread at `next`, a layer-2 tile for its padded image or a layer-1 chunk as it is)
// travels in FOUR parts, each loaded before and stored after a quarter of the work on the chunk in use: a quarter of the prefetch
// registers.  Nobody reads the other half of wbuf before the barrier that ends the work.  `buf` is the half that holds the chunk in use.
// Every store to global memory stands outside: a branch between the loads and the stores of a travelling chunk sends it through scratch.
// V, the type of the prefetch registers: a native vector in the two parameter-gradient units (copies of a float4 struct that a rounded()
// stands between stayed in scratch); critic_grad, which has no rounded(), keeps float4 -- with the native vector its HT = 4 instance takes
// one VGPR more (177 -> 178).
template <int THREADS, int NPF, bool TILE, class V = f32x4, int BUF4, class Q>
__device__ __forceinline__ void staged(float4 (&wbuf)[2][BUF4], int& buf, const Lane& L, const float4* next, Q&& quarter) {
  constexpr int CH = (NPF + 3) / 4;
  float4* wn = wbuf[buf ^ 1];
  static_for<0, 4>([&](auto sg) __attribute__((always_inline)) {
    constexpr int S = decltype(sg)::value, I0 = S * CH, N = I0 + CH <= NPF ? CH : (NPF > I0 ? NPF - I0 : 0);
    V pf[N > 0 ? N : 1];
    static_for<0, N>([&](auto i) __attribute__((always_inline)) { pf[i] = *reinterpret_cast<const V*>(next + THREADS * (I0 + i)); });
    quarter(sg);
    static_for<0, N>([&](auto i) __attribute__((always_inline)) {
      *reinterpret_cast<V*>(wn + (TILE ? L.sbase + 4 * L2_ROW4 * (I0 + i) : L.tid + THREADS * (I0 + i))) = pf[i];
    });
  });
  __syncthreads();  // everyone has left this chunk (its buffer is the one after next) and the next chunk is in place
  buf ^= 1;
}

// Layer-1 tile T, tile TT of the staged chunk `wb`: STEPS4 float4 reads per lane against the row's features xb (this lane's B operands:
// features 2 s + h); leaves h1 and the mask bits of the tile (two tiles to a word, formed when the word is complete).
template <int STEPS4, int TT, int T, int HT>
__device__ __forceinline__ void layer1_tile(const float4* wb, const float4* small4, const Lane& L, const float (&xb)[4 * STEPS4], float (&h1)[HT * 16],
                                            uint32_t (&m1)[HT / 2]) {
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 b = small4[(32 * T + 8 * g + 4 * L.h) / 4];
    acc[4 * g + 0] = b.x, acc[4 * g + 1] = b.y, acc[4 * g + 2] = b.z, acc[4 * g + 3] = b.w;
  }
#pragma unroll
  for (int sq = 0; sq < STEPS4; sq++) {
    const float4 a = wb[(TT * STEPS4 + sq) * 64 + L.lane];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xb[4 * sq + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xb[4 * sq + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xb[4 * sq + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xb[4 * sq + 3], acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 16; v++) h1[T * 16 + v] = fmaxf(acc[v], 0.0f);
  m1[T >> 1] |= relu_bits(acc) << (16 * (T & 1));
  if constexpr (TT & 1) formed(m1[T >> 1]);
}

// quarter S of layer 2 forward on a staged tile (wb: its image at this lane's forward slot): read rows sq = 4 u + g take registers
// 4 g .. 4 g + 3 of layer-1 tile u
template <int HT, int S>
__device__ __forceinline__ void layer2_forward_quarter(const float4* wb, const float (&h1)[HT * 16], f32x16& acc) {
#pragma unroll
  for (int sq = S * HT; sq < (S + 1) * HT; sq++) {
    const float4 a = wb[sq * L2_ROW4];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h1[4 * sq + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h1[4 * sq + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h1[4 * sq + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h1[4 * sq + 3], acc, 0, 0, 0);
  }
}

// the mask bits of tile t out of their word, two tiles of 16 bits each (a register array takes no run-time index): bit v of the result is
// register v of the tile
template <int MW>
__device__ __forceinline__ uint32_t mask_tile(const uint32_t (&m)[MW], int t) {
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < MW; i++) word = (t >> 1) == i ? m[i] : word;
  return word >> (16 * (t & 1));
}

// Quarter G of the pass back through staged layer-2 tile t (wb: its image at this lane's A slot): four MFMA steps, step r with k = h
// neuron 32 t + 8 G + 4 h + r of layer 2 and b(r) its masked gradient, formed by the caller.  Accumulator 4 U + c, register v: neuron
// 128 U + 8 v + 4 h + c.
template <int HT, int G, class B>
__device__ __forceinline__ void layer2_backward_quarter(const float4* wb, B&& b, f32x16 (&dacc)[HT]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float br = b(r);
#pragma unroll
    for (int U = 0; U < HT / 4; U++) {
      const float4 a = wb[16 * U * L2_ROW4 + 8 * G + r];  // W1[32 t + 8 G + 4 h + r][128 U + 4 jj + c], c = 0 .. 3
      dacc[4 * U + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, br, dacc[4 * U + 0], 0, 0, 0);
      dacc[4 * U + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, br, dacc[4 * U + 1], 0, 0, 0);
      dacc[4 * U + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, br, dacc[4 * U + 2], 0, 0, 0);
      dacc[4 * U + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, br, dacc[4 * U + 3], 0, 0, 0);
    }
  }
}

// ------------------------------------------------------------------------------------------------ stages 2 and 3
// Four consecutive rows of neuron n of an array: one float4.  n < limit, or the operand is +0 (the columns of x past Map::X).
__device__ __forceinline__ float4 operand4(const float* base, int n, int limit) {
  if (n >= limit) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return *reinterpret_cast<const float4*>(base + 32 * (size_t)n);
}

// The 64 x 64 block job of stage 2, one wave: A = d2 (g_W1) or d1 (g_W0), neurons 64 ab + 32 ia + i; B = h1, or x with Map::X columns.
// One step of its K loop: four consecutive rows of two A and two B neurons; the bias sums g_b1, g_b0 are added up on the VALU from the
// A operands.
__device__ __forceinline__ void gemm_step(f32x16 (&acc)[2][2], float (&bsum)[2], const float4 (&a)[2], const float4 (&b)[2]) {
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
// ... and its results: the block of g_W (H rows of `columns`) and, from the job with column 0, the bias gradients of its 64 neurons
template <class Map>
__device__ __forceinline__ void gemm_store(const BwDims& D, const BwJob& job, int lane, int columns, float* gw, float* gb, const f32x16 (&acc)[2][2],
                                           const float (&bsum)[2]) {
#pragma unroll
  for (int ia = 0; ia < 2; ia++) {
#pragma unroll
    for (int jb = 0; jb < 2; jb++) {
      const int j = Map::s2_column(job, jb, lane);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int n = Map::s2_neuron(job, ia, v, lane);
        if (n < D.H && j < columns) gw[(size_t)n * columns + j] = acc[ia][jb][v];  // padded rows and columns are never stored
      }
    }
    const float sum = bsum[ia] + __shfl_xor(bsum[ia], 32);
    const int n = 64 * job.ab + (lane & 31) + 32 * ia;
    if (job.bb == 0 && (lane >> 5) == 0 && n < D.H) gb[n] = sum;
  }
}

// the 64 lanes' float64 partial sums of a head bias, added in a fixed butterfly
__device__ __forceinline__ double lane_sum(double dsum) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) dsum += __shfl_xor(dsum, step);
  return dsum;
}

// Stage 3, element e of the NETS x P outputs: the partial results of the splits in ascending order, in float64 (at most 64 float32
// terms: float64 adds them without an error of its own), rounded once.
template <class Map>
__device__ __forceinline__ void combine_element(const float* partial, const BwDims& D, float* const (&grad)[Map::NETS][Map::TENSORS], size_t e) {
  static_assert(Map::NETS <= 2, "the network of an element is a comparison");
  if (e >= Map::NETS * D.P) return;
  const int net = Map::NETS == 2 && e >= D.P;
  const size_t r = e - (size_t)net * D.P;
  double sum = (double)partial[Map::partial_offset(D, 0, net) + r];
  for (int s = 1; s < D.S; s++) sum += (double)partial[Map::partial_offset(D, s, net) + r];
  size_t at;
  const int t = Map::tensor_of(D, r, &at);
  grad[net][t][at] = (float)sum;
}

}  // namespace mlp_grad
}  // namespace urgym
