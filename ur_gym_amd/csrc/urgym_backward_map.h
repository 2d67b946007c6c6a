// urgym_backward_map.h — the index arithmetic of the critic's parameter gradients (urgym_critic_backward.hip), stated once as
// __host__ __device__ functions: where stage 1 puts what it computes per row, what stage 2 reads and where its sums go.  The kernels run
// it on the device; tests/backward_harness.cpp enumerates it on the host (bounds, bijection, every output written once).
//
// The workspace, in floats (HP = hidden width padded to a multiple of 128, RG = ceil(count / 32) row GROUPS of 32 rows):
//
//   per network and array (h1, h2, d2, d1)   [RG][HP][32]   element (row m, neuron n) at ((m >> 5) HP + n) 32 + (m & 31)
//   x  (the gathered input rows, once)       [RG][56][32]   feature k < 56 (zero from in_features on)
//   dq (the upstream gradient as used)       [2][RG][32]
//   partial sums, only where S > 1           [S][2][P]      S = ceil(count / 1024) splits of the rows; P floats per network laid out
//                                                           as the six output tensors one after the other (bw_tensor_offset)
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
constexpr int BW_X = 56;             // features kept of x: critic_kernel's padded layer-1 K
constexpr int BW_S1_ROWS = 128;      // rows per workgroup of stage 1 (4 waves of 32): critic_kernel's geometry

enum { BW_H1 = 0, BW_H2, BW_D2, BW_D1, BW_ARRAYS };
// the six output tensors of a network, in the order of urgym_q_network_dev
enum { BW_G_W0 = 0, BW_G_B0, BW_G_W1, BW_G_B1, BW_G_WQ, BW_G_BQ, BW_TENSORS };

struct BwDims {
  int in, H, HP, count, RG, S;
  size_t P;                                   // floats of one network's six gradient tensors
  size_t x_off, dq_off, partial_off, floats;  // in floats from the start of the workspace; floats = its size
};

URGYM_BW_HD inline BwDims bw_dims(int in, int H, int count) {
  BwDims d;
  d.in = in, d.H = H, d.HP = (H + 127) / 128 * 128, d.count = count;
  d.RG = (count + BW_GROUP - 1) / BW_GROUP, d.S = (count + BW_SPLIT_ROWS - 1) / BW_SPLIT_ROWS;
  d.P = (size_t)H * in + (size_t)H * H + 3 * (size_t)H + 1;
  d.x_off = (size_t)2 * BW_ARRAYS * d.RG * d.HP * BW_GROUP;
  d.dq_off = d.x_off + (size_t)d.RG * BW_X * BW_GROUP;
  d.partial_off = d.dq_off + (size_t)2 * d.RG * BW_GROUP;
  d.floats = d.partial_off + (d.S > 1 ? (size_t)d.S * 2 * d.P : 0);
  return d;
}

// ---- the map from (network, array, row, neuron) to a workspace offset
URGYM_BW_HD inline size_t bw_offset(const BwDims& d, int net, int array, size_t row, int neuron) {
  return ((((size_t)(net * BW_ARRAYS + array) * d.RG + (row >> 5)) * d.HP + neuron) << 5) + (row & 31);
}
URGYM_BW_HD inline size_t bw_x_offset(const BwDims& d, size_t row, int k) { return d.x_off + ((((row >> 5) * BW_X) + k) << 5) + (row & 31); }
URGYM_BW_HD inline size_t bw_dq_offset(const BwDims& d, int net, size_t row) { return d.dq_off + ((((size_t)net * d.RG) + (row >> 5)) << 5) + (row & 31); }

// ---- the outputs: tensor t of a network within its P floats, and the partial sums of (split, network)
URGYM_BW_HD inline size_t bw_tensor_offset(const BwDims& d, int t) {
  const size_t H = d.H, w0 = H * d.in, w1 = H * H;
  return t == BW_G_W0 ? 0 : t == BW_G_B0 ? w0 : t == BW_G_W1 ? w0 + H : t == BW_G_B1 ? w0 + H + w1 : t == BW_G_WQ ? w0 + 2 * H + w1 : w0 + 3 * H + w1;
}
URGYM_BW_HD inline size_t bw_tensor_floats(const BwDims& d, int t) {
  return t == BW_G_W0 ? (size_t)d.H * d.in : t == BW_G_W1 ? (size_t)d.H * d.H : t == BW_G_BQ ? 1 : (size_t)d.H;
}
URGYM_BW_HD inline size_t bw_partial_offset(const BwDims& d, int split, int net) { return d.partial_off + ((size_t)split * 2 + net) * d.P; }
// which tensor holds float r < P of a network's gradients, and where in it
URGYM_BW_HD inline int bw_tensor_of(const BwDims& d, size_t r, size_t* at) {
  int t = BW_G_BQ;
  while (bw_tensor_offset(d, t) > r) t--;
  *at = r - bw_tensor_offset(d, t);
  return t;
}

// ---- stage 1: workgroup b, wave w, lane l works on one row; a wave stores where its first row exists (its lanes past the end store +0)
URGYM_BW_HD inline size_t bw_s1_row(unsigned block, int wave, int lane) { return (size_t)block * BW_S1_ROWS + wave * 32 + (lane & 31); }
URGYM_BW_HD inline bool bw_s1_stores(const BwDims& d, size_t row) { return (row & ~(size_t)31) < (size_t)d.count; }
URGYM_BW_HD inline unsigned bw_s1_grid(const BwDims& d) { return (unsigned)((d.count + BW_S1_ROWS - 1) / BW_S1_ROWS); }
// The same offsets as stage 1 forms them: a part that is one for the wave (its row group) plus a part that is one for the lane, plus
// 32 x the neuron of lane half 0.  The neurons of lane half 1 are `apart` further on (4 for the arrays, 1 for the features of x).
URGYM_BW_HD inline size_t bw_s1_group(unsigned block, int wave) { return (size_t)block * (BW_S1_ROWS / BW_GROUP) + wave; }
URGYM_BW_HD inline size_t bw_group_offset(const BwDims& d, int net, int array, size_t group) { return (((size_t)(net * BW_ARRAYS + array) * d.RG + group) * d.HP) << 5; }
URGYM_BW_HD inline size_t bw_x_group_offset(const BwDims& d, size_t group) { return d.x_off + ((group * BW_X) << 5); }
URGYM_BW_HD inline uint32_t bw_s1_lane_offset(int lane, int apart) { return 32u * (uint32_t)apart * (uint32_t)(lane >> 5) + (uint32_t)(lane & 31); }
// h1, h2, d2: register v of forward tile t on lane half h
URGYM_BW_HD inline int bw_fwd_neuron(int t, int v, int h) { return 32 * t + 8 * (v >> 2) + 4 * h + (v & 3); }
// d1: register v of backward accumulator a on lane half h
URGYM_BW_HD inline int bw_back_neuron(int a, int v, int h) { return 128 * (a >> 2) + 8 * v + 4 * h + (a & 3); }

// ---- stage 2: one WAVE per job; the jobs of one (split, network) pair, four to a workgroup
//   BW_JOB_W1    g_W1 block [64 ab .. + 64][64 bb .. + 64] = d2^T h1; with bb == 0 also g_b1 of those 64 neurons
//   BW_JOB_W0    g_W0 block [64 ab .. + 64][0 .. 64)      = d1^T x;  also g_b0 of those 64 neurons
//   BW_JOB_HEAD  g_wq of neurons 32 ab .. + 32 = sum dq h2; with ab == 0 also g_bq
enum { BW_JOB_NONE = -1, BW_JOB_W1 = 0, BW_JOB_W0, BW_JOB_HEAD };
struct BwJob {
  int kind, ab, bb;
};
URGYM_BW_HD inline int bw_jobs(const BwDims& d) { const int nb = d.HP / 64; return nb * nb + nb + d.HP / 32; }
URGYM_BW_HD inline int bw_job_wgs(const BwDims& d) { return (bw_jobs(d) + 3) / 4; }
URGYM_BW_HD inline unsigned bw_s2_grid(const BwDims& d) { return (unsigned)(d.S * 2 * bw_job_wgs(d)); }
URGYM_BW_HD inline BwJob bw_job(const BwDims& d, int j) {
  const int nb = d.HP / 64;
  BwJob job = {BW_JOB_NONE, 0, 0};
  if (j < nb * nb) job.kind = BW_JOB_W1, job.ab = j / nb, job.bb = j % nb;
  else if (j < nb * nb + nb) job.kind = BW_JOB_W0, job.ab = j - nb * nb;
  else if (j < bw_jobs(d)) job.kind = BW_JOB_HEAD, job.ab = j - nb * nb - nb;
  return job;
}
// workgroup b of stage 2 -> (split, network, first job)
URGYM_BW_HD inline void bw_s2_block(const BwDims& d, unsigned b, int* split, int* net, int* job0) {
  const unsigned w = (unsigned)bw_job_wgs(d), pair = b / w;
  *split = (int)(pair >> 1), *net = (int)(pair & 1), *job0 = (int)(b % w) * 4;
}
// the row groups of a split: [first, end)
URGYM_BW_HD inline void bw_split_groups(const BwDims& d, int split, int* first, int* end) {
  const int per = BW_SPLIT_ROWS / BW_GROUP, e = (split + 1) * per;
  *first = split * per, *end = e < d.RG ? e : d.RG;
}
// the first of the four consecutive rows lane half h reads in step q (0 .. 3) of row group R: MFMA step (q, c) pairs row + c of h = 0 with
// row + c of h = 1
URGYM_BW_HD inline size_t bw_s2_row(int R, int q, int h) { return (size_t)R * 32 + 8 * q + 4 * h; }
// the row lane (h, i) of the wave that sums g_bq reads of row group R (it takes every second group from the split's first + h on)
URGYM_BW_HD inline size_t bw_s2_bq_row(int R, int i) { return (size_t)R * 32 + i; }
// the output element of accumulator (ia, jb), register v, lane l of a 64 x 64 block job: neuron n (the row of the gradient), column j
URGYM_BW_HD inline int bw_s2_neuron(const BwJob& job, int ia, int v, int lane) { return 64 * job.ab + 32 * ia + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
URGYM_BW_HD inline int bw_s2_column(const BwJob& job, int jb, int lane) { return 64 * job.bb + 32 * jb + (lane & 31); }

}  // namespace urgym
