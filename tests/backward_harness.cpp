// backward_harness.cpp — stand-alone host program (tests/test_critic_backward.py and tests/test_actor_backward.py build and run it
// under the address and undefined-behaviour sanitizers, with the argument `critic` or `actor`): the index arithmetic of the parameter
// gradients (ur_gym_amd/csrc/urgym_backward_map.h), enumerated workgroup by workgroup, wave by wave, lane by lane as the kernels of
// urgym_critic_backward.hip and urgym_actor_backward.hip run it.  One enumeration, instantiated for either map:
//
//   * every workspace offset stage 1 writes and stage 2 / 3 read lies inside the size the query reports;
//   * stage 1's writes are a bijection onto what stage 2 reads (each float written once, each written float read, nothing else read);
//   * stage 2's partial sums (count > 1024) are written once each and are exactly what stage 3 reads;
//   * every element of the output tensors (twelve of the critic, eight of the actor) is written exactly once, and nothing outside them.
// An out-of-range store found here is one that never reaches a GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_backward_map.h"

using namespace urgym;

static std::atomic<int> failures{0};  // the cases run on several threads: one printf per message
#define CHECK(cond, ...)                            \
  do {                                              \
    if (!(cond)) {                                  \
      if (failures++ < 20) {                        \
        char msg[256];                              \
        snprintf(msg, sizeof msg, __VA_ARGS__);     \
        printf("FAIL %s: %s\n", #cond, msg);        \
      }                                             \
    }                                               \
  } while (0)

struct Marks {
  std::vector<unsigned char> n;
  size_t limit;
  explicit Marks(size_t size) : n(size, 0), limit(size) {}
  void hit(size_t off, const char* what) {
    CHECK(off < limit, "%s offset %zu of %zu", what, off, limit);
    if (off < limit && n[off] < 255) n[off]++;
  }
};

template <class Map>
static std::string run_case(const char* name, int in, int H, int count) {
  const BwDims d = Map::dims(in, H, count);
  const int HT = d.HP / 32;
  CHECK(d.x_off % 4 == 0 && d.heads_off % 4 == 0 && d.partial_off % 4 == 0, "float4 alignment");
  CHECK(Map::tensor_offset(d, Map::TENSORS - 1) + Map::tensor_floats(d, Map::TENSORS - 1) == d.P, "P = %zu", d.P);
  Marks written(d.floats), read(d.floats);
  // the outputs as the caller's tensors: per network P floats in the order of tensor_offset
  std::vector<Marks> out(Map::NETS, Marks(d.P));

  // ---- stage 1
  for (unsigned b = 0; b < Map::s1_grid(d); b++)
    for (int wave = 0; wave < 4; wave++)
      for (int lane = 0; lane < 64; lane++) {
        const size_t row = Map::s1_row(b, wave, lane), group = Map::s1_group(b, wave);
        const int h = lane >> 5;
        if (!Map::s1_stores(d, row)) continue;
        CHECK(group == row >> 5 && group < (size_t)d.RG, "group %zu row %zu", group, row);
        for (int net = 0; net < Map::NETS; net++) {
          for (int array = BW_H1; array <= BW_D2; array++)
            for (int t = 0; t < HT; t++)
              for (int v = 0; v < 16; v++) {
                const size_t off = Map::group_offset(d, net, array, group) + 32 * (size_t)Map::fwd_neuron(t, v, 0) + Map::s1_lane_offset(lane, 4);
                CHECK(off == Map::offset(d, net, array, row, Map::fwd_neuron(t, v, h)), "forward map");
                written.hit(off, "stage 1 array");
              }
          for (int a = 0; a < HT; a++)
            for (int v = 0; v < 16; v++) {
              const size_t off = Map::group_offset(d, net, BW_D1, group) + 32 * (size_t)Map::back_neuron(a, v, 0) + Map::s1_lane_offset(lane, 4);
              CHECK(off == Map::offset(d, net, BW_D1, row, Map::back_neuron(a, v, h)), "backward map");
              written.hit(off, "stage 1 d1");
            }
          if (h == 0)
            for (int j = 0; j < Map::HEADS; j++) {
              const size_t off = Map::heads_group_offset(d, net, group) + (lane & 31) + 32 * (size_t)j;
              CHECK(off == Map::heads_offset(d, net, row, j), "heads map");
              written.hit(off, "stage 1 heads");
            }
        }
        for (int s = 0; s < Map::X / 2; s++) {
          const size_t off = Map::x_group_offset(d, group) + 32 * (size_t)(2 * s) + Map::s1_lane_offset(lane, 1);
          CHECK(off == Map::x_offset(d, row, 2 * s + h), "x map");
          written.hit(off, "stage 1 x");
        }
      }
  for (size_t i = 0; i < d.partial_off; i++) CHECK(written.n[i] == 1, "workspace float %zu written %d times by stage 1", i, written.n[i]);

  // ---- stage 2
  auto dst = [&](int split, int net, int tensor, size_t at) {
    CHECK(at < Map::tensor_floats(d, tensor), "tensor %d element %zu", tensor, at);
    if (d.S > 1) written.hit(Map::partial_offset(d, split, net) + Map::tensor_offset(d, tensor) + at, "partial");
    else out[net].hit(Map::tensor_offset(d, tensor) + at, "output");
  };
  auto read4 = [&](size_t off) {
    CHECK(off % 4 == 0 && off + 3 < d.partial_off, "float4 read at %zu", off);
    for (int c = 0; c < 4; c++) read.hit(off + c, "stage 2 read");
  };
  std::vector<int> groups_seen(d.RG, 0);
  std::vector<int> bias_reads(d.partial_off - d.heads_off, 0);  // every head gradient enters its float64 bias sum exactly once
  for (unsigned b = 0; b < Map::s2_grid(d); b++) {
    int split, net, job0, R0, R1;
    Map::s2_block(d, b, &split, &net, &job0);
    CHECK(split < d.S && net < Map::NETS, "block %u", b);
    Map::split_groups(d, split, &R0, &R1);
    CHECK(R0 < R1 && R1 <= d.RG, "split %d groups %d %d", split, R0, R1);
    if (net == 0 && job0 == 0)
      for (int R = R0; R < R1; R++) groups_seen[R]++;
    for (int wave = 0; wave < 4; wave++) {
      const BwJob job = Map::job(d, job0 + wave);
      if (job.kind == BW_JOB_NONE) continue;
      for (int lane = 0; lane < 64; lane++) {
        const int h = lane >> 5, i = lane & 31;
        if (job.kind == BW_JOB_HEAD) {
          const int n = 32 * job.ab + i;
          CHECK(n < d.HP, "head neuron %d", n);
          for (int R = R0; R < R1; R++)
            for (int q = 0; q < 4; q++) {
              read4(Map::offset(d, net, BW_H2, Map::s2_row(R, q, h), n));
              for (int j = 0; j < Map::HEADS; j++) read4(Map::heads_offset(d, net, Map::s2_row(R, q, h), j));
            }
          if (h == 0 && n < d.H)
            for (int j = 0; j < Map::HEADS; j++) dst(split, net, Map::head_tensor(j), Map::head_element(d, j, n));
          if (job.ab == 0) {
            for (int R = R0 + h; R < R1; R += 2)
              for (int j = 0; j < Map::HEADS; j++) {
                const size_t off = Map::heads_offset(d, net, Map::s2_bias_row(R, i), j);
                CHECK(off >= d.heads_off && off < d.partial_off, "bias read at %zu", off);
                bias_reads[off - d.heads_off]++;
              }
            if (lane == 0)
              for (int j = 0; j < Map::HEADS; j++) dst(split, net, Map::head_tensor(j) + 1, j % Map::HEAD_COLS);
          }
          continue;
        }
        const bool w1 = job.kind == BW_JOB_W1;
        const int a_array = w1 ? BW_D2 : BW_D1, b_limit = w1 ? d.HP : Map::X, an = 64 * job.ab + i, bn = 64 * job.bb + i;
        for (int R = R0; R < R1; R++)
          for (int q = 0; q < 4; q++) {
            const size_t row = Map::s2_row(R, q, h);
            for (int sub = 0; sub < 2; sub++) {
              CHECK(an + 32 * sub < d.HP, "A neuron");
              read4(Map::offset(d, net, a_array, row, an + 32 * sub));
              if (bn + 32 * sub < b_limit) read4(w1 ? Map::offset(d, net, BW_H1, row, bn + 32 * sub) : Map::x_offset(d, row, bn + 32 * sub));
            }
          }
        const int columns = w1 ? d.H : d.in;
        for (int ia = 0; ia < 2; ia++) {
          for (int jb = 0; jb < 2; jb++)
            for (int v = 0; v < 16; v++) {
              const int n = Map::s2_neuron(job, ia, v, lane), j = Map::s2_column(job, jb, lane);
              if (n < d.H && j < columns) dst(split, net, w1 ? BW_G_W1 : BW_G_W0, (size_t)n * columns + j);
            }
          if (job.bb == 0 && h == 0 && an + 32 * ia < d.H) dst(split, net, w1 ? BW_G_B1 : BW_G_B0, an + 32 * ia);
        }
      }
    }
  }
  for (int R = 0; R < d.RG; R++) CHECK(groups_seen[R] == 1, "row group %d belongs to %d splits", R, groups_seen[R]);
  for (size_t i = 0; i < bias_reads.size(); i++) CHECK(bias_reads[i] == 1, "head float %zu enters its bias sum %d times", i, bias_reads[i]);
  // the bijection: what stage 2 reads is what stage 1 wrote, all of it
  for (size_t i = 0; i < d.partial_off; i++) CHECK(read.n[i] > 0, "workspace float %zu written by stage 1, never read", i);
  for (size_t i = d.partial_off; i < d.floats; i++) CHECK(read.n[i] == 0, "stage 2 reads partial %zu", i);

  // ---- stage 3
  if (d.S > 1) {
    for (size_t i = d.partial_off; i < d.floats; i++) CHECK(written.n[i] == 1, "partial %zu written %d times", i, written.n[i]);
    for (size_t e = 0; e < Map::NETS * d.P; e++) {
      const int net = (int)(e / d.P);
      const size_t r = e - (size_t)net * d.P;
      for (int s = 0; s < d.S; s++) {
        const size_t off = Map::partial_offset(d, s, net) + r;
        CHECK(off >= d.partial_off && off < d.floats && written.n[off] == 1, "stage 3 reads %zu", off);
      }
      size_t at;
      const int t = Map::tensor_of(d, r, &at);
      CHECK(at < Map::tensor_floats(d, t) && Map::tensor_offset(d, t) + at == r, "tensor of %zu", r);
      out[net].hit(Map::tensor_offset(d, t) + at, "output");
    }
  } else {
    CHECK(d.floats == d.partial_off, "no partial sums up to one split");
  }
  for (int net = 0; net < Map::NETS; net++)
    for (size_t i = 0; i < d.P; i++) CHECK(out[net].n[i] == 1, "output float %zu of network %d written %d times", i, net, out[net].n[i]);
  char line[160];
  snprintf(line, sizeof line, "%s in=%d H=%d count=%d floats=%zu splits=%d launches=%d\n", name, in, H, count, d.floats, d.S, d.S > 1 ? 3 : 2);
  return line;
}

// one family: the lines of its cases, its workspace line and its `ok N`; `ins` are the input widths of the four envs, the last the widest
template <class Map>
static int run_family(const char* name, const int (&ins)[4]) {
  const int widths[4] = {32, 128, 160, 256}, counts[11] = {1, 33, 128, 129, 417, 1023, 1024, 1025, 2049, 3072, 4513};
  struct Case {
    int in, H, count;
  };
  std::vector<Case> todo;
  for (int in : ins)
    for (int H : widths)
      for (int count : counts) todo.push_back({in, H, count});
  // 64 splits, with a last split of one row and at the largest count: at H = 32 only.  The enumeration visits every float of the
  // workspace several times; at H = 256 these two cases alone take half a minute under the sanitizers.
  for (int count : {63 * BW_SPLIT_ROWS + 1, BW_MAX_COUNT}) todo.push_back({ins[3], 32, count});
  // the cases are independent: a few threads take them from one list, the two longest (the last two) first; the lines are printed in the list's order
  const int cases = (int)todo.size();
  std::vector<std::string> lines(cases);
  std::atomic<int> next{0};
  auto worker = [&] {
    for (int k; (k = next++) < cases;) {
      const int c = k < 2 ? cases - 2 + k : k - 2;
      lines[c] = run_case<Map>(name, todo[c].in, todo[c].H, todo[c].count);
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool.emplace_back(worker);
  for (auto& t : pool) t.join();
  for (const auto& l : lines) fputs(l.c_str(), stdout);
  // the size include/urgym.h states, and the largest offsets in size_t (no enumeration at this size)
  const BwDims big = Map::dims(ins[3], 256, BW_MAX_COUNT);
  printf("workspace in=%d H=256 count=%d bytes=%zu\n", ins[3], BW_MAX_COUNT, big.floats * sizeof(float));
  CHECK(Map::offset(big, Map::NETS - 1, BW_D1, BW_MAX_COUNT - 1, big.HP - 1) + 1 == big.x_off, "last array float");
  CHECK(Map::heads_offset(big, Map::NETS - 1, BW_MAX_COUNT - 1, Map::HEADS - 1) + 1 == big.partial_off, "last head float");
  CHECK(Map::partial_offset(big, big.S - 1, Map::NETS - 1) + big.P == big.floats, "last partial float");
  if (failures) {
    printf("FAIL %d checks\n", failures.load());
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "critic")) return run_family<CriticBackwardMap>("backward", {36, 38, 47, 53});
  if (argc == 2 && !strcmp(argv[1], "actor")) return run_family<ActorBackwardMap>("actor backward", {30, 32, 41, 47});
  fprintf(stderr, "usage: %s critic|actor\n", argv[0]);
  return 2;
}
