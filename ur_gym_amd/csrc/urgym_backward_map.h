// urgym_backward_map.h — the index arithmetic of the parameter gradients of the critic (urgym_critic_backward.hip) and of the actor
// (urgym_actor_backward.hip), stated once as __host__ __device__ functions: where stage 1 puts what it computes per row, what stage 2
// reads and where its sums go.  The kernels run it on the device (urgym_mlp_grad.h, and what each unit keeps of its own);
// tests/backward_harness.cpp enumerates it on the host (bounds, bijection, every output written once).  One map, BackwardMap, over
// three facts that tell the two apart:
//
//                          NETS   X (features kept of x: the forward kernel's padded layer-1 K)   HEADS (columns of the upstream gradient)
//   CriticBackwardMap       2     56                                                               1   dq
//   ActorBackwardMap        1     48                                                              12   d_mu[6] | dr[6]
//
// The workspace, in floats (HP = hidden width padded to a multiple of 128, RG = ceil(count / 32) row GROUPS of 32 rows):
//
//   per network and array (h1, h2, d2, d1)   [NETS][4][RG][HP][32]   element (row m, neuron n) at ((m >> 5) HP + n) 32 + (m & 31)
//   x  (the gathered input rows, once)       [RG][X][32]             feature k < X (zero from in_features on)
//   heads (the upstream gradient as used)    [NETS][RG][HEADS][32]   the critic's dq; the actor's column j < 6: d_mu[j], 6 + j: dr[j],
//                                                                    d_log_std through the clamp
//   partial sums, only where S > 1           [S][NETS][P]            S = ceil(count / 1024) splits of the rows; P floats per network
//                                                                    laid out as its output tensors one after the other (tensor_offset)
//
// 32 rows of one neuron are 128 contiguous bytes: a half-wave of stage 1 (32 rows, one neuron per register) stores one full line, and
// a lane of stage 2 (one neuron, MFMA operand A or B) reads four consecutive rows as one float4.  Rows count .. 32 RG - 1 of the last
// group are written as +0 by stage 1 and read by stage 2 (they add +0), so every float read was written in the same call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define URGYM_BW_HD __host__ __device__
#else
#define URGYM_BW_HD
#endif

namespace urgym {

constexpr int BW_MAX_COUNT = 65536;  // rows per call (include/urgym.h states it)
constexpr int BW_SPLIT_ROWS = 1024;  // rows per split of stage 2: up to this count stage 2 stores the results itself
constexpr int BW_GROUP = 32;         // rows per row group
constexpr int BW_S1_ROWS = 128;      // rows per workgroup of stage 1 (4 waves of 32): the forward kernels' geometry
constexpr int BW_MAX_HIDDEN = 256;   // the widths stage 1 is built for (instances HT = 4 and 8)

enum { BW_H1 = 0, BW_H2, BW_D2, BW_D1, BW_ARRAYS };
// The output tensors of a network, in the order of urgym_q_network_dev and urgym_actor_params_dev: the two hidden layers, then per head
// tensor its weights and its bias -- BW_G_HEAD + 2 g and + 2 g + 1: w_q, b_q of the critic; w_mu, b_mu, w_log_std, b_log_std of the actor.
enum { BW_G_W0 = 0, BW_G_B0, BW_G_W1, BW_G_B1, BW_G_HEAD };

struct BwDims {
  int in, H, HP, count, RG, S;
  size_t P;                                      // floats of one network's gradient tensors
  size_t x_off, heads_off, partial_off, floats;  // in floats from the start of the workspace; floats = its size
};

// ---- stage 2: one WAVE per job; the jobs of one (split, network) pair, four to a workgroup
//   BW_JOB_W1    g_W1 block [64 ab .. + 64][64 bb .. + 64] = d2^T h1; with bb == 0 also g_b1 of those 64 neurons
//   BW_JOB_W0    g_W0 block [64 ab .. + 64][0 .. 64)      = d1^T x;  also g_b0 of those 64 neurons
//   BW_JOB_HEAD  the head weights of neurons 32 ab .. + 32 = sum (heads) h2^T; with ab == 0 also the head biases
enum { BW_JOB_NONE = -1, BW_JOB_W1 = 0, BW_JOB_W0, BW_JOB_HEAD };
struct BwJob {
  int kind, ab, bb;
};

template <int NETS_, int X_, int HEADS_>
struct BackwardMap {
  static constexpr int NETS = NETS_, X = X_, HEADS = HEADS_;
  static constexpr int HEAD_COLS = HEADS == 1 ? 1 : 6;  // columns per head tensor: the one of w_q, or one per action dimension
  static constexpr int TENSORS = BW_G_HEAD + 2 * (HEADS / HEAD_COLS);
  static_assert(HEADS % HEAD_COLS == 0, "whole head tensors");

  static URGYM_BW_HD inline BwDims dims(int in, int H, int count) {
    BwDims d;
    d.in = in, d.H = H, d.HP = (H + 127) / 128 * 128, d.count = count;
    d.RG = (count + BW_GROUP - 1) / BW_GROUP, d.S = (count + BW_SPLIT_ROWS - 1) / BW_SPLIT_ROWS;
    d.P = (size_t)H * in + (size_t)H * H + 2 * (size_t)H + HEADS * (size_t)H + HEADS;
    d.x_off = (size_t)NETS * BW_ARRAYS * d.RG * d.HP * BW_GROUP;
    d.heads_off = d.x_off + (size_t)d.RG * X * BW_GROUP;
    d.partial_off = d.heads_off + (size_t)NETS * d.RG * HEADS * BW_GROUP;
    d.floats = d.partial_off + (d.S > 1 ? (size_t)d.S * NETS * d.P : 0);
    return d;
  }

  // ---- the map from (network, array, row, neuron) to a workspace offset
  static URGYM_BW_HD inline size_t offset(const BwDims& d, int net, int array, size_t row, int neuron) {
    return ((((size_t)(net * BW_ARRAYS + array) * d.RG + (row >> 5)) * d.HP + neuron) << 5) + (row & 31);
  }
  static URGYM_BW_HD inline size_t x_offset(const BwDims& d, size_t row, int k) { return d.x_off + ((((row >> 5) * X) + k) << 5) + (row & 31); }
  static URGYM_BW_HD inline size_t heads_offset(const BwDims& d, int net, size_t row, int j) {
    return d.heads_off + (((((size_t)net * d.RG) + (row >> 5)) * HEADS + j) << 5) + (row & 31);
  }

  // ---- the outputs: tensor t of a network within its P floats, and the partial sums of (split, network)
  static URGYM_BW_HD inline size_t tensor_floats(const BwDims& d, int t) {
    return t == BW_G_W0 ? (size_t)d.H * d.in : t == BW_G_W1 ? (size_t)d.H * d.H : t < BW_G_HEAD ? (size_t)d.H
           : ((t - BW_G_HEAD) & 1) ? HEAD_COLS : HEAD_COLS * (size_t)d.H;
  }
  static URGYM_BW_HD inline size_t tensor_offset(const BwDims& d, int t) {
    size_t off = 0;
    for (int u = 0; u < t; u++) off += tensor_floats(d, u);
    return off;
  }
  static URGYM_BW_HD inline size_t partial_offset(const BwDims& d, int split, int net) { return d.partial_off + ((size_t)split * NETS + net) * d.P; }
  // which tensor holds float r < P of a network's gradients, and where in it
  static URGYM_BW_HD inline int tensor_of(const BwDims& d, size_t r, size_t* at) {
    int t = TENSORS - 1;
    size_t off = d.P - tensor_floats(d, t);
    while (off > r) off -= tensor_floats(d, --t);
    *at = r - off;
    return t;
  }
  // column j < HEADS of neuron n goes to element (j % HEAD_COLS) H + n of the weights of head tensor j / HEAD_COLS, its bias to element
  // j % HEAD_COLS of the tensor after
  static URGYM_BW_HD inline int head_tensor(int j) { return BW_G_HEAD + 2 * (j / HEAD_COLS); }
  static URGYM_BW_HD inline size_t head_element(const BwDims& d, int j, int n) { return (size_t)(j % HEAD_COLS) * d.H + n; }

  // ---- stage 1: workgroup b, wave w, lane l works on one row; a wave stores where its first row exists (its lanes past the end store +0)
  static URGYM_BW_HD inline size_t s1_row(unsigned block, int wave, int lane) { return (size_t)block * BW_S1_ROWS + wave * 32 + (lane & 31); }
  static URGYM_BW_HD inline bool s1_stores(const BwDims& d, size_t row) { return (row & ~(size_t)31) < (size_t)d.count; }
  static URGYM_BW_HD inline unsigned s1_grid(const BwDims& d) { return (unsigned)((d.count + BW_S1_ROWS - 1) / BW_S1_ROWS); }
  // The same offsets as stage 1 forms them: a part that is one for the wave (its row group) plus a part that is one for the lane, plus
  // 32 x the neuron of lane half 0.  The neurons of lane half 1 are `apart` further on (4 for the arrays, 1 for the features of x; the
  // head columns are stored by lane half 0 alone).
  static URGYM_BW_HD inline size_t s1_group(unsigned block, int wave) { return (size_t)block * (BW_S1_ROWS / BW_GROUP) + wave; }
  static URGYM_BW_HD inline size_t group_offset(const BwDims& d, int net, int array, size_t group) {
    return (((size_t)(net * BW_ARRAYS + array) * d.RG + group) * d.HP) << 5;
  }
  static URGYM_BW_HD inline size_t x_group_offset(const BwDims& d, size_t group) { return d.x_off + ((group * X) << 5); }
  static URGYM_BW_HD inline size_t heads_group_offset(const BwDims& d, int net, size_t group) {
    return d.heads_off + ((((size_t)net * d.RG + group) * HEADS) << 5);
  }
  static URGYM_BW_HD inline uint32_t s1_lane_offset(int lane, int apart) { return 32u * (uint32_t)apart * (uint32_t)(lane >> 5) + (uint32_t)(lane & 31); }
  // h1, h2, d2: register v of forward tile t on lane half h
  static URGYM_BW_HD inline int fwd_neuron(int t, int v, int h) { return 32 * t + 8 * (v >> 2) + 4 * h + (v & 3); }
  // d1: register v of backward accumulator a on lane half h
  static URGYM_BW_HD inline int back_neuron(int a, int v, int h) { return 128 * (a >> 2) + 8 * v + 4 * h + (a & 3); }

  // ---- stage 2 (the jobs: BwJob above)
  static URGYM_BW_HD inline int jobs(const BwDims& d) { const int nb = d.HP / 64; return nb * nb + nb + d.HP / 32; }
  static URGYM_BW_HD inline int job_wgs(const BwDims& d) { return (jobs(d) + 3) / 4; }
  static URGYM_BW_HD inline unsigned s2_grid(const BwDims& d) { return (unsigned)(d.S * NETS * job_wgs(d)); }
  static URGYM_BW_HD inline BwJob job(const BwDims& d, int j) {
    const int nb = d.HP / 64;
    BwJob job = {BW_JOB_NONE, 0, 0};
    if (j < nb * nb) job.kind = BW_JOB_W1, job.ab = j / nb, job.bb = j % nb;
    else if (j < nb * nb + nb) job.kind = BW_JOB_W0, job.ab = j - nb * nb;
    else if (j < jobs(d)) job.kind = BW_JOB_HEAD, job.ab = j - nb * nb - nb;
    return job;
  }
  // workgroup b of stage 2 -> (split, network, first job)
  static URGYM_BW_HD inline void s2_block(const BwDims& d, unsigned b, int* split, int* net, int* job0) {
    const unsigned w = (unsigned)job_wgs(d), pair = b / w;
    *split = (int)(pair / NETS), *net = (int)(pair % NETS), *job0 = (int)(b % w) * 4;
  }
  // the row groups of a split: [first, end)
  static URGYM_BW_HD inline void split_groups(const BwDims& d, int split, int* first, int* end) {
    const int per = BW_SPLIT_ROWS / BW_GROUP, e = (split + 1) * per;
    *first = split * per, *end = e < d.RG ? e : d.RG;
  }
  // the first of the four consecutive rows lane half h reads in step q (0 .. 3) of row group R: MFMA step (q, c) pairs row + c of h = 0 with
  // row + c of h = 1; the fma chains of a head job add rows row .. row + 3 in this order, and join the two halves at the end
  static URGYM_BW_HD inline size_t s2_row(int R, int q, int h) { return (size_t)R * 32 + 8 * q + 4 * h; }
  // the row lane (h, i) of the wave that sums the head biases reads of row group R (it takes every second group from the split's first + h on)
  static URGYM_BW_HD inline size_t s2_bias_row(int R, int i) { return (size_t)R * 32 + i; }
  // the output element of accumulator (ia, jb), register v, lane l of a 64 x 64 block job: neuron n (the row of the gradient), column j
  static URGYM_BW_HD inline int s2_neuron(const BwJob& job, int ia, int v, int lane) { return 64 * job.ab + 32 * ia + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
  static URGYM_BW_HD inline int s2_column(const BwJob& job, int jb, int lane) { return 64 * job.bb + 32 * jb + (lane & 31); }
};

typedef BackwardMap<2, 56, 1> CriticBackwardMap;  // twin Q-networks, critic_kernel's layer-1 K, dq
typedef BackwardMap<1, 48, 12> ActorBackwardMap;  // one policy network, actor_kernel's layer-1 K, d_mu | dr

}  // namespace urgym
