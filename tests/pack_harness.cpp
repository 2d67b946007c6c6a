// Stand-alone host program (tests/test_weights_host.py builds and runs it; it may also be built with -fsanitize=address,undefined):
// the packing map the device pack kernels use (ur_gym_amd/csrc/urgym_pack_map.h), run on the host exactly as a kernel runs it -- one
// "lane" per quad of the packed buffer -- against the host packing loops the library creates actors and critics with
// (urgym_pack_host.h).  For every env kind and hidden width: word-for-word equality over the whole buffer, padding included; every
// packed float written exactly once; every source offset inside its tensor; the log_std head untouched when it is not given; and
// the blend against the three-operation float32 formula at tau = 0.005 and tau = 1.  Prints one line per case and "ok <cases>".
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_pack_host.h"
#include "../ur_gym_amd/csrc/urgym_pack_map.h"

using namespace urgym;

namespace {

const uint32_t NAN_WORD = 0x7FC00ABCu;
int failures = 0;

void fail(const char* what, int in, int H, long where) {
  printf("FAIL %s in=%d H=%d at %ld\n", what, in, H, where);
  failures++;
}

uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

bool same_words(const std::vector<float>& a, const std::vector<float>& b, long* where) {
  if (a.size() != b.size()) return *where = -1, false;
  for (size_t i = 0; i < a.size(); i++)
    if (bits(a[i]) != bits(b[i])) return *where = (long)i, false;
  return true;
}

// distinct values, exact in float32: consecutive integers from `first` (all below 2^24), alternating in sign
struct Tensors {
  std::vector<std::vector<float>> t;
  float next;
  explicit Tensors(float first) : next(first) {}
  const float* add(size_t n) {
    t.emplace_back(n);
    for (float& v : t.back()) v = ((int)next & 1) ? -next : next, next += 1.0f;
    return t.back().data();
  }
};

// packed = (packed * omt) + (tau * src): three float32 operations, each rounded on its own (volatile keeps them apart)
float polyak(float old, float src, float tau, float omt) {
  volatile float a = old * omt;
  volatile float b = tau * src;
  return a + b;
}

void actor_case(int in, int H) {
  Tensors T(1.0f);
  urgym_actor_desc d;
  memset(&d, 0, sizeof(d));
  d.in_features = in, d.hidden_width = H, d.action_dim = 6;
  d.w0 = T.add((size_t)H * in), d.b0 = T.add(H), d.w1 = T.add((size_t)H * H), d.b1 = T.add(H), d.w_mu = T.add(6 * (size_t)H), d.b_mu = T.add(6);
  const float* w_ls = T.add(6 * (size_t)H);
  const float* b_ls = T.add(6);
  const size_t sizes[PACK_ACTOR_TENSORS] = {(size_t)H * in, (size_t)H, (size_t)H * H, (size_t)H, 6 * (size_t)H, 6, 6 * (size_t)H, 6};
  const float* src[PACK_ACTOR_TENSORS] = {d.w0, d.b0, d.w1, d.b1, d.w_mu, d.b_mu, w_ls, b_ls};

  size_t p2_off, small_off;
  std::vector<float> want = pack_actor_host(&d, &p2_off, &small_off);
  const PackDims D = pack_dims_actor(in, H);
  if (want.size() != pack_actor_floats(D) || p2_off != D.n1 || small_off != D.n1 + D.n2) return fail("actor sizes", in, H, 0);
  const size_t head0 = small_off + pack_actor_head_begin(D), head_len = (size_t)D.HP * 6 + 8;
  if (head0 + head_len != want.size()) return fail("actor head extent", in, H, 0);
  const std::vector<float> head = pack_log_std_host(H, D.HP, w_ls, b_ls);

  for (int with_head = 0; with_head < 2; with_head++) {
    float nan;
    memcpy(&nan, &NAN_WORD, 4);
    std::vector<float> got(want.size(), nan);
    std::vector<int> written(want.size(), 0);
    const uint32_t quads = (uint32_t)(want.size() / 4);
    for (uint32_t q = 0; q < quads; q++) {  // the kernel's body, one lane per quad
      PackQuad m;
      const bool is_head = pack_quad_actor(D, q, m);
      if (is_head != ((size_t)q * 4 >= head0)) return fail("actor head flag", in, H, q);
      if (is_head && !with_head) continue;
      for (int c = 0; c < 4; c++) {
        if (m.off[c] >= 0 && (m.tensor < 0 || m.tensor >= PACK_ACTOR_TENSORS || (size_t)m.off[c] >= sizes[m.tensor])) return fail("actor source out of bounds", in, H, q);
        got[(size_t)q * 4 + c] = m.off[c] >= 0 ? src[m.tensor][m.off[c]] : 0.0f;
        written[(size_t)q * 4 + c]++;
      }
    }
    std::vector<float> expect = want;  // host loops: zero head, or set_log_std's head
    for (size_t i = 0; i < head_len; i++) expect[head0 + i] = with_head ? head[i] : nan;
    long where;
    if (!same_words(got, expect, &where)) return fail(with_head ? "actor words (with head)" : "actor words (head untouched)", in, H, where);
    for (size_t i = 0; i < written.size(); i++)
      if (written[i] != ((i >= head0 && !with_head) ? 0 : 1)) return fail("actor write count", in, H, (long)i);
  }
  printf("actor in=%d H=%d floats=%zu\n", in, H, want.size());
}

void critic_case(int in, int H) {
  const PackDims D = pack_dims_critic(in, H);
  const size_t sizes[PACK_CRITIC_TENSORS] = {(size_t)H * in, (size_t)H, (size_t)H * H, (size_t)H, (size_t)H, 1};
  Tensors Told(1.0f), Tnew(5.0f);
  urgym_critic_desc d_old, d_new;
  const float* src_new[2 * PACK_CRITIC_TENSORS];
  for (int which = 0; which < 2; which++) {
    urgym_critic_desc& d = which ? d_new : d_old;
    Tensors& T = which ? Tnew : Told;
    memset(&d, 0, sizeof(d));
    d.in_features = in, d.hidden_width = H, d.n_critics = 2;
    for (int net = 0; net < 2; net++) {
      urgym_q_network& q = d.qf[net];
      q.w0 = T.add(sizes[0]), q.b0 = T.add(sizes[1]), q.w1 = T.add(sizes[2]), q.b1 = T.add(sizes[3]), q.w_q = T.add(sizes[4]), q.b_q = T.add(sizes[5]);
      if (which) {
        const float* p[PACK_CRITIC_TENSORS] = {q.w0, q.b0, q.w1, q.b1, q.w_q, q.b_q};
        for (int i = 0; i < PACK_CRITIC_TENSORS; i++) src_new[PACK_CRITIC_TENSORS * net + i] = p[i];
      }
    }
  }
  size_t small_off, small_off2;
  const std::vector<float> old_packed = pack_critic_host(&d_old, &small_off);
  const std::vector<float> new_packed = pack_critic_host(&d_new, &small_off2);
  if (new_packed.size() != pack_critic_floats(D) || small_off != 2 * (D.n1 + D.n2) || small_off2 != small_off) return fail("critic sizes", in, H, 0);

  float nan;
  memcpy(&nan, &NAN_WORD, 4);
  const float taus[2] = {1.0f, 0.005f};
  for (float tau : taus) {
    const float omt = 1.0f - tau;
    const bool blend = tau != 1.0f;
    std::vector<float> got = blend ? old_packed : std::vector<float>(new_packed.size(), nan);  // tau = 1 must repair a NaN buffer
    std::vector<int> written(got.size(), 0);
    const uint32_t quads = (uint32_t)(got.size() / 4);
    for (uint32_t q = 0; q < quads; q++) {  // the kernel's body, one lane per quad
      PackQuad m;
      pack_quad_critic(D, q, m);
      for (int c = 0; c < 4; c++) {
        if (m.off[c] >= 0 && (m.tensor < 0 || m.tensor >= 2 * PACK_CRITIC_TENSORS || (size_t)m.off[c] >= sizes[m.tensor % PACK_CRITIC_TENSORS]))
          return fail("critic source out of bounds", in, H, q);
        float v = m.off[c] >= 0 ? src_new[m.tensor][m.off[c]] : 0.0f;
        if (blend) v = polyak(got[(size_t)q * 4 + c], v, tau, omt);
        got[(size_t)q * 4 + c] = v;
        written[(size_t)q * 4 + c]++;
      }
    }
    std::vector<float> expect = new_packed;
    if (blend)
      for (size_t i = 0; i < expect.size(); i++) expect[i] = polyak(old_packed[i], new_packed[i], tau, omt);
    long where;
    if (!same_words(got, expect, &where)) return fail(blend ? "critic words (tau 0.005)" : "critic words (tau 1)", in, H, where);
    for (size_t i = 0; i < got.size(); i++) {
      if (written[i] != 1) return fail("critic write count", in, H, (long)i);
      if (bits(new_packed[i]) == 0 && bits(old_packed[i]) == 0 && bits(got[i]) != 0) return fail("critic padding is not +0", in, H, (long)i);
    }
  }
  printf("critic in=%d H=%d floats=%zu\n", in, H, new_packed.size());
}

}  // namespace

int main() {
  const int actor_in[4] = {30, 32, 41, 47}, critic_in[4] = {36, 38, 47, 53}, widths[5] = {32, 160, 256, 288, 512};
  int cases = 0;
  for (int k = 0; k < 4; k++)
    for (int H : widths) {
      actor_case(actor_in[k], H);
      critic_case(critic_in[k], H);
      cases += 2;
    }
  if (failures) {
    printf("FAILED %d\n", failures);
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}
