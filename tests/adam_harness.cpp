// Stand-alone host program (tests/test_adam_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// two things the Adam step kernels of ur_gym_amd/csrc/urgym_adam.hip rely on, run on the host.
//
//   adam_harness             the quad map of urgym_pack_map.h, run as a kernel runs it -- one "lane" per quad of the packed buffer --
//                            for every env kind x hidden width in {32, 160, 256, 288, 512}, actor and critic: every element of every
//                            source tensor is named by exactly ONE (quad, slot), and no slot names an element outside its tensor.
//                            (tests/pack_harness.cpp checks the other direction: every packed float is written once.)  A lane that
//                            steps the elements its quad names therefore steps every parameter exactly once.  Prints one line per
//                            case and "ok <cases>".
//   adam_harness IN OUT      the per-element arithmetic, adam_element of urgym_adam.h -- the very function the kernels compile --
//                            on the elements of file IN, results to file OUT, for a bitwise comparison with evaluation.adam_step.
//                            IN:  double lr, beta1, beta2, eps; int64 step; int64 n; float p[n], g[n], m[n], v[n]
//                            OUT: float coef[7] (adam_coefficients of urgym_adam.h); float p'[n], m'[n], v'[n]
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_adam.h"
#include "../ur_gym_amd/csrc/urgym_pack_map.h"

using namespace urgym;

namespace {

int failures = 0;

void fail(const char* what, int in, int H, long tensor, long where) {
  printf("FAIL %s in=%d H=%d tensor=%ld at %ld\n", what, in, H, tensor, where);
  failures++;
}

// names[t][e] = how many (quad, slot) pairs name element e of tensor t; every one must end as 1
template <class Map>
void map_case(const char* label, int in, int H, const std::vector<size_t>& sizes, uint32_t quads, Map map) {
  std::vector<std::vector<int>> names;
  for (size_t n : sizes) names.emplace_back(n, 0);
  size_t padding = 0;
  for (uint32_t q = 0; q < quads; q++) {  // the kernel's body, one lane per quad
    PackQuad m;
    map(q, m);
    for (int c = 0; c < 4; c++) {
      if (m.off[c] < 0) {
        padding++;
        continue;
      }
      if (m.tensor < 0 || (size_t)m.tensor >= sizes.size() || (size_t)m.off[c] >= sizes[m.tensor]) return fail("element out of bounds", in, H, m.tensor, q);
      names[m.tensor][m.off[c]]++;
    }
  }
  size_t elements = 0;
  for (size_t t = 0; t < sizes.size(); t++) {
    elements += sizes[t];
    for (size_t e = 0; e < sizes[t]; e++)
      if (names[t][e] != 1) return fail(names[t][e] ? "element named more than once" : "element named by no quad", in, H, (long)t, (long)e);
  }
  if (elements + padding != (size_t)quads * 4) return fail("elements + padding != floats", in, H, -1, 0);
  printf("%s in=%d H=%d elements=%zu padding=%zu\n", label, in, H, elements, padding);
}

int map_cases() {
  const int actor_in[4] = {30, 32, 41, 47}, widths[5] = {32, 160, 256, 288, 512};
  int cases = 0;
  for (int k = 0; k < 4; k++)
    for (int H : widths) {
      const size_t h = (size_t)H;
      {
        const int in = actor_in[k];
        const PackDims D = pack_dims_actor(in, H);
        map_case("actor", in, H, {h * in, h, h * h, h, 6 * h, 6, 6 * h, 6}, (uint32_t)(pack_actor_floats(D) / 4),
                 [&](uint32_t q, PackQuad& m) { pack_quad_actor(D, q, m); });
      }
      {
        const int in = actor_in[k] + 6;
        const PackDims D = pack_dims_critic(in, H);
        std::vector<size_t> sizes;
        for (int net = 0; net < 2; net++)
          for (size_t n : {h * in, h, h * h, h, h, (size_t)1}) sizes.push_back(n);
        map_case("critic", in, H, sizes, (uint32_t)(pack_critic_floats(D) / 4), [&](uint32_t q, PackQuad& m) { pack_quad_critic(D, q, m); });
      }
      cases += 2;
    }
  if (failures) {
    printf("FAILED %d\n", failures);
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}

int arithmetic(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) return printf("cannot open %s\n", in_path), 2;
  double hyper[4];
  int64_t step = 0, n = 0;
  bool ok = fread(hyper, sizeof(double), 4, f) == 4 && fread(&step, sizeof(step), 1, f) == 1 && fread(&n, sizeof(n), 1, f) == 1 && n >= 0 && n <= (1 << 26);
  std::vector<float> p, g, m, v;
  if (ok) {
    p.resize(n), g.resize(n), m.resize(n), v.resize(n);
    for (std::vector<float>* x : {&p, &g, &m, &v}) ok = ok && fread(x->data(), sizeof(float), (size_t)n, f) == (size_t)n;
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in_path), 2;
  const AdamCoef c = adam_coefficients(hyper[0], hyper[1], hyper[2], hyper[3], step);
  for (int64_t i = 0; i < n; i++) adam_element(c, g[i], p[i], m[i], v[i]);
  f = fopen(out_path, "wb");
  if (!f) return printf("cannot open %s\n", out_path), 2;
  const float coef[7] = {c.b1, c.omb1, c.b2, c.omb2, c.step_size, c.bc2_sqrt, c.eps};
  ok = fwrite(coef, sizeof(float), 7, f) == 7;
  for (std::vector<float>* x : {&p, &m, &v}) ok = ok && fwrite(x->data(), sizeof(float), (size_t)n, f) == (size_t)n;
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out_path), 2;
  printf("stepped %lld\n", (long long)n);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return map_cases();
  if (argc == 3) return arithmetic(argv[1], argv[2]);
  printf("usage: adam_harness [IN OUT]\n");
  return 2;
}
