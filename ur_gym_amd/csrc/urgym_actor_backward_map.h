// urgym_actor_backward_map.h — the index arithmetic of the actor's parameter gradients (urgym_actor_backward.hip), stated once as
// __host__ __device__ functions: where stage 1 puts what it computes per row, what stage 2 reads and where its sums go.  The kernels run
// it on the device; tests/actor_backward_harness.cpp enumerates it on the host (bounds, bijection, every output written once).  The
// structure is urgym_backward_map.h's with one network, 48 features and twelve head columns where the critic has one.
//
// The workspace, in floats (HP = hidden width padded to a multiple of 128, RG = ceil(count / 32) row GROUPS of 32 rows):
//
//   per array (h1, h2, d2, d1)               [RG][HP][32]   element (row m, neuron n) at ((m >> 5) HP + n) 32 + (m & 31)
//   x  (the gathered input rows)             [RG][48][32]   feature k < 48 (zero from in_features on)
//   heads (d_mu | dr, the upstream as used)  [RG][12][32]   column j < 6: d_mu[j]; 6 + j: dr[j], d_log_std through the clamp
//   partial sums, only where S > 1           [S][P]         S = ceil(count / 1024) splits of the rows; P floats laid out as the eight
//                                                           output tensors one after the other (ab_tensor_offset)
//
// 32 rows of one neuron are 128 contiguous bytes: a half-wave of stage 1 (32 rows, one neuron per register) stores one full line, and
// a lane of stage 2 (one neuron, MFMA operand A or B) reads four consecutive rows as one float4.  Rows count .. 32 RG - 1 of the last
// group are written as +0 by stage 1 and read by stage 2 (they add +0), so every float read was written in the same call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define URGYM_AB_HD __host__ __device__
#else
#define URGYM_AB_HD
#endif

namespace urgym {

constexpr int AB_MAX_COUNT = 65536;  // rows per call (include/urgym.h states it)
constexpr int AB_SPLIT_ROWS = 1024;  // rows per split of stage 2: up to this count stage 2 stores the results itself
constexpr int AB_GROUP = 32;         // rows per row group
constexpr int AB_X = 48;             // features kept of x: actor_kernel's padded layer-1 K
constexpr int AB_HEADS = 12;         // head columns: d_mu[6] | dr[6]
constexpr int AB_S1_ROWS = 128;      // rows per workgroup of stage 1 (4 waves of 32): actor_kernel's geometry
constexpr int AB_MAX_HIDDEN = 256;   // the widths stage 1 is built for (instances HT = 4 and 8)

enum { AB_H1 = 0, AB_H2, AB_D2, AB_D1, AB_ARRAYS };
// the eight output tensors, in the order of urgym_actor_params_dev
enum { AB_G_W0 = 0, AB_G_B0, AB_G_W1, AB_G_B1, AB_G_WMU, AB_G_BMU, AB_G_WLS, AB_G_BLS, AB_TENSORS };

struct AbDims {
  int in, H, HP, count, RG, S;
  size_t P;                                      // floats of the eight gradient tensors
  size_t x_off, heads_off, partial_off, floats;  // in floats from the start of the workspace; floats = its size
};

URGYM_AB_HD inline AbDims ab_dims(int in, int H, int count) {
  AbDims d;
  d.in = in, d.H = H, d.HP = (H + 127) / 128 * 128, d.count = count;
  d.RG = (count + AB_GROUP - 1) / AB_GROUP, d.S = (count + AB_SPLIT_ROWS - 1) / AB_SPLIT_ROWS;
  d.P = (size_t)H * in + (size_t)H * H + 2 * (size_t)H + 12 * (size_t)H + 12;
  d.x_off = (size_t)AB_ARRAYS * d.RG * d.HP * AB_GROUP;
  d.heads_off = d.x_off + (size_t)d.RG * AB_X * AB_GROUP;
  d.partial_off = d.heads_off + (size_t)d.RG * AB_HEADS * AB_GROUP;
  d.floats = d.partial_off + (d.S > 1 ? (size_t)d.S * d.P : 0);
  return d;
}

// ---- the map from (array, row, neuron) to a workspace offset
URGYM_AB_HD inline size_t ab_offset(const AbDims& d, int array, size_t row, int neuron) {
  return ((((size_t)array * d.RG + (row >> 5)) * d.HP + neuron) << 5) + (row & 31);
}
URGYM_AB_HD inline size_t ab_x_offset(const AbDims& d, size_t row, int k) { return d.x_off + ((((row >> 5) * AB_X) + k) << 5) + (row & 31); }
URGYM_AB_HD inline size_t ab_heads_offset(const AbDims& d, size_t row, int j) { return d.heads_off + ((((row >> 5) * AB_HEADS) + j) << 5) + (row & 31); }

// ---- the outputs: tensor t within the P floats, and the partial sums of a split
URGYM_AB_HD inline size_t ab_tensor_floats(const AbDims& d, int t) {
  return t == AB_G_W0 ? (size_t)d.H * d.in : t == AB_G_W1 ? (size_t)d.H * d.H : (t == AB_G_WMU || t == AB_G_WLS) ? 6 * (size_t)d.H
         : (t == AB_G_BMU || t == AB_G_BLS) ? 6 : (size_t)d.H;
}
URGYM_AB_HD inline size_t ab_tensor_offset(const AbDims& d, int t) {
  size_t off = 0;
  for (int u = 0; u < t; u++) off += ab_tensor_floats(d, u);
  return off;
}
URGYM_AB_HD inline size_t ab_partial_offset(const AbDims& d, int split) { return d.partial_off + (size_t)split * d.P; }
// which tensor holds float r < P of the gradients, and where in it
URGYM_AB_HD inline int ab_tensor_of(const AbDims& d, size_t r, size_t* at) {
  int t = 0;
  size_t off = 0;
  while (t + 1 < AB_TENSORS && off + ab_tensor_floats(d, t) <= r) off += ab_tensor_floats(d, t), t++;
  *at = r - off;
  return t;
}

// ---- stage 1: workgroup b, wave w, lane l works on one row; a wave stores where its first row exists (its lanes past the end store +0)
URGYM_AB_HD inline size_t ab_s1_row(unsigned block, int wave, int lane) { return (size_t)block * AB_S1_ROWS + wave * 32 + (lane & 31); }
URGYM_AB_HD inline bool ab_s1_stores(const AbDims& d, size_t row) { return (row & ~(size_t)31) < (size_t)d.count; }
URGYM_AB_HD inline unsigned ab_s1_grid(const AbDims& d) { return (unsigned)((d.count + AB_S1_ROWS - 1) / AB_S1_ROWS); }
// The same offsets as stage 1 forms them: a part that is one for the wave (its row group) plus a part that is one for the lane, plus
// 32 x the neuron of lane half 0.  The neurons of lane half 1 are `apart` further on (4 for the arrays, 1 for the features of x; the
// head columns are stored by lane half 0 alone).
URGYM_AB_HD inline size_t ab_s1_group(unsigned block, int wave) { return (size_t)block * (AB_S1_ROWS / AB_GROUP) + wave; }
URGYM_AB_HD inline size_t ab_group_offset(const AbDims& d, int array, size_t group) { return (((size_t)array * d.RG + group) * d.HP) << 5; }
URGYM_AB_HD inline size_t ab_x_group_offset(const AbDims& d, size_t group) { return d.x_off + ((group * AB_X) << 5); }
URGYM_AB_HD inline size_t ab_heads_group_offset(const AbDims& d, size_t group) { return d.heads_off + ((group * AB_HEADS) << 5); }
URGYM_AB_HD inline uint32_t ab_s1_lane_offset(int lane, int apart) { return 32u * (uint32_t)apart * (uint32_t)(lane >> 5) + (uint32_t)(lane & 31); }
// h1, h2, d2: register v of forward tile t on lane half h
URGYM_AB_HD inline int ab_fwd_neuron(int t, int v, int h) { return 32 * t + 8 * (v >> 2) + 4 * h + (v & 3); }
// d1: register v of backward accumulator a on lane half h
URGYM_AB_HD inline int ab_back_neuron(int a, int v, int h) { return 128 * (a >> 2) + 8 * v + 4 * h + (a & 3); }

// ---- stage 2: one WAVE per job; the jobs of one split, four to a workgroup
//   AB_JOB_W1    g_W1 block [64 ab .. + 64][64 bb .. + 64] = d2^T h1; with bb == 0 also g_b1 of those 64 neurons
//   AB_JOB_W0    g_W0 block [64 ab .. + 64][0 .. 64)      = d1^T x;  also g_b0 of those 64 neurons
//   AB_JOB_HEAD  g_Wmu and g_Wls of neurons 32 ab .. + 32 = sum (d_mu | dr) h2^T; with ab == 0 also g_bmu and g_bls
enum { AB_JOB_NONE = -1, AB_JOB_W1 = 0, AB_JOB_W0, AB_JOB_HEAD };
struct AbJob {
  int kind, ab, bb;
};
URGYM_AB_HD inline int ab_jobs(const AbDims& d) { const int nb = d.HP / 64; return nb * nb + nb + d.HP / 32; }
URGYM_AB_HD inline int ab_job_wgs(const AbDims& d) { return (ab_jobs(d) + 3) / 4; }
URGYM_AB_HD inline unsigned ab_s2_grid(const AbDims& d) { return (unsigned)(d.S * ab_job_wgs(d)); }
URGYM_AB_HD inline AbJob ab_job(const AbDims& d, int j) {
  const int nb = d.HP / 64;
  AbJob job = {AB_JOB_NONE, 0, 0};
  if (j < nb * nb) job.kind = AB_JOB_W1, job.ab = j / nb, job.bb = j % nb;
  else if (j < nb * nb + nb) job.kind = AB_JOB_W0, job.ab = j - nb * nb;
  else if (j < ab_jobs(d)) job.kind = AB_JOB_HEAD, job.ab = j - nb * nb - nb;
  return job;
}
// workgroup b of stage 2 -> (split, first job)
URGYM_AB_HD inline void ab_s2_block(const AbDims& d, unsigned b, int* split, int* job0) {
  const unsigned w = (unsigned)ab_job_wgs(d);
  *split = (int)(b / w), *job0 = (int)(b % w) * 4;
}
// the row groups of a split: [first, end)
URGYM_AB_HD inline void ab_split_groups(const AbDims& d, int split, int* first, int* end) {
  const int per = AB_SPLIT_ROWS / AB_GROUP, e = (split + 1) * per;
  *first = split * per, *end = e < d.RG ? e : d.RG;
}
// the first of the four consecutive rows lane half h reads in step q (0 .. 3) of row group R: MFMA step (q, c) pairs row + c of h = 0 with
// row + c of h = 1; the fma chains of a head job add rows row .. row + 3 in this order, and join the two halves at the end
URGYM_AB_HD inline size_t ab_s2_row(int R, int q, int h) { return (size_t)R * 32 + 8 * q + 4 * h; }
// the row lane (h, i) of the wave that sums the head biases reads of row group R (it takes every second group from the split's first + h on)
URGYM_AB_HD inline size_t ab_s2_bias_row(int R, int i) { return (size_t)R * 32 + i; }
// the output element of accumulator (ia, jb), register v, lane l of a 64 x 64 block job: neuron n (the row of the gradient), column j
URGYM_AB_HD inline int ab_s2_neuron(const AbJob& job, int ia, int v, int lane) { return 64 * job.ab + 32 * ia + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
URGYM_AB_HD inline int ab_s2_column(const AbJob& job, int jb, int lane) { return 64 * job.bb + 32 * jb + (lane & 31); }
// a head job: column j < 12 of neuron n goes to element (j % 6) H + n of g_Wmu (j < 6) or g_Wls
URGYM_AB_HD inline int ab_head_tensor(int j) { return j < 6 ? AB_G_WMU : AB_G_WLS; }
URGYM_AB_HD inline size_t ab_head_element(const AbDims& d, int j, int n) { return (size_t)(j % 6) * d.H + n; }

}  // namespace urgym
