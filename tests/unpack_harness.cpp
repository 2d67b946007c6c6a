// Stand-alone host program (tests/test_checkpoint_host.py builds and runs it, once plainly and once with
// -fsanitize=address,undefined): the packing map (ur_gym_amd/csrc/urgym_pack_map.h) run the OTHER way, as the unpack kernels of
// urgym_weights.hip run it -- one "lane" per quad, each float that has an element written to that element -- on the output of the host
// packing loops the library creates actors and critics with (urgym_pack_host.h).  For every env kind and hidden width:
//   * walking all quads, every element of every tensor is the destination of exactly one packed float, every destination lies inside
//     its tensor, and no padding float (one the host loops left +0.0f without a source) has a destination;
//   * unpack of the host-packed buffer returns the source tensors word for word -- the sources hold NaN payloads, -0.0f, denormals and
//     infinities -- and with the head skipped the head's destinations keep their canary;
//   * pack (the map's gather) after unpack reproduces the buffer word for word.
// Prints one line per case and "ok <cases>".
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_pack_host.h"
#include "../ur_gym_amd/csrc/urgym_pack_map.h"

using namespace urgym;

namespace {

const uint32_t CANARY = 0x7FC0C0DEu;
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
float from_bits(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// Distinct words that never equal +0.0f or the canary: a counter in the low 20 bits under a cycle of exponent / sign patterns that
// makes NaNs with payloads (quiet and signalling), infinities' neighbours, denormals, -0.0f's neighbours and ordinary numbers; every
// 97th word is exactly -0.0f, every 101st an infinity (those repeat: the destination counts, not the values, tell elements apart).
struct Words {
  uint32_t n = 1;
  std::vector<std::vector<float>> t;
  float* add(size_t count) {
    static const uint32_t top[8] = {0x7FC00000u, 0x7F800000u, 0xFFC00000u, 0x00000000u, 0x80000000u, 0x3F800000u, 0xC1200000u, 0x7F000000u};
    t.emplace_back(count);
    for (float& v : t.back()) {
      uint32_t w = top[n & 7] | ((n >> 3) & 0xFFFFFu) | 1u;  // | 1: a NaN keeps a payload, a denormal is not zero
      if (n % 97 == 0) w = 0x80000000u;
      if (n % 101 == 0) w = (n & 1) ? 0xFF800000u : 0x7F800000u;
      v = from_bits(w), n++;
    }
    return t.back().data();
  }
};

bool same_words(const float* a, const float* b, size_t n, long* where) {
  for (size_t i = 0; i < n; i++)
    if (bits(a[i]) != bits(b[i])) return *where = (long)i, false;
  return true;
}

// the unpack kernel's body for one quad: the floats that have an element go to it
void scatter(float* const* dst, const PackQuad& m, const float* quad) {
  for (int c = 0; c < 4; c++)
    if (m.off[c] >= 0) dst[m.tensor][m.off[c]] = quad[c];
}

template <int T, class Map>
bool run_case(const char* who, int in, int H, const std::vector<float>& packed, const float* const* src, const size_t* sizes, size_t skip_from, int first_skipped,
              Map map) {
  const uint32_t quads = (uint32_t)(packed.size() / 4);
  // destinations: one heap allocation per tensor, exactly its size, filled with a canary (a store outside one is the sanitizer's to see)
  std::vector<std::vector<float>> out(T);
  std::vector<std::vector<int>> hits(T);
  float* dst[T];
  for (int i = 0; i < T; i++) {
    out[i].assign(sizes[i], from_bits(CANARY));
    hits[i].assign(sizes[i], 0);
    dst[i] = i >= first_skipped ? nullptr : out[i].data();
  }
  for (uint32_t q = 0; q < quads; q++) {
    PackQuad m;
    const bool head = map(q, m);
    if (head != ((size_t)q * 4 >= skip_from)) return fail("head flag", in, H, q), false;
    for (int c = 0; c < 4; c++) {
      const size_t at = (size_t)q * 4 + c;
      if (m.off[c] < 0) {  // padding: the host loops wrote nothing there
        if (bits(packed[at]) != 0) return fail("a float without a destination is not padding", in, H, (long)at), false;
        continue;
      }
      if (m.tensor < 0 || m.tensor >= T || (size_t)m.off[c] >= sizes[m.tensor]) return fail("destination out of bounds", in, H, (long)at), false;
      if (head != (m.tensor >= first_skipped) && first_skipped < T) return fail("head quad outside the head tensors", in, H, (long)at), false;
      hits[m.tensor][m.off[c]]++;
    }
    if (head && first_skipped < T) continue;  // the head is skipped
    scatter(dst, m, packed.data() + (size_t)q * 4);
  }
  for (int i = 0; i < T; i++) {
    for (size_t e = 0; e < sizes[i]; e++)
      if (hits[i][e] != 1) return fail("an element is not the destination of exactly one float", in, H, (long)(i * 100000000L + (long)e)), false;
    long where;
    if (i >= first_skipped) {
      for (size_t e = 0; e < sizes[i]; e++)
        if (bits(out[i][e]) != CANARY) return fail("a skipped tensor was written", in, H, (long)e), false;
    } else if (!same_words(out[i].data(), src[i], sizes[i], &where)) {
      return fail("unpack differs from the source", in, H, i * 100000000L + where), false;
    }
  }
  // pack after unpack: the map's gather from what unpack wrote (the skipped head: from the sources, which is what the buffer holds)
  std::vector<float> again(packed.size(), from_bits(CANARY));
  for (uint32_t q = 0; q < quads; q++) {
    PackQuad m;
    map(q, m);
    for (int c = 0; c < 4; c++) {
      const float* from = m.off[c] < 0 ? nullptr : (m.tensor >= first_skipped ? src[m.tensor] : out[m.tensor].data());
      again[(size_t)q * 4 + c] = from ? from[m.off[c]] : 0.0f;
    }
  }
  long where;
  if (!same_words(again.data(), packed.data(), packed.size(), &where)) return fail("pack after unpack differs from the buffer", in, H, where), false;
  printf("%s in=%d H=%d floats=%zu\n", who, in, H, packed.size());
  return true;
}

void actor_case(int in, int H) {
  Words W;
  urgym_actor_desc d;
  memset(&d, 0, sizeof(d));
  d.in_features = in, d.hidden_width = H, d.action_dim = 6;
  d.w0 = W.add((size_t)H * in), d.b0 = W.add(H), d.w1 = W.add((size_t)H * H), d.b1 = W.add(H), d.w_mu = W.add(6 * (size_t)H), d.b_mu = W.add(6);
  const float* w_ls = W.add(6 * (size_t)H);
  const float* b_ls = W.add(6);
  const size_t sizes[PACK_ACTOR_TENSORS] = {(size_t)H * in, (size_t)H, (size_t)H * H, (size_t)H, 6 * (size_t)H, 6, 6 * (size_t)H, 6};
  const float* src[PACK_ACTOR_TENSORS] = {d.w0, d.b0, d.w1, d.b1, d.w_mu, d.b_mu, w_ls, b_ls};
  size_t p2_off, small_off;
  std::vector<float> packed = pack_actor_host(&d, &p2_off, &small_off);
  const PackDims D = pack_dims_actor(in, H);
  if (packed.size() != pack_actor_floats(D)) return fail("actor sizes", in, H, 0);
  const size_t head0 = small_off + pack_actor_head_begin(D);
  const std::vector<float> head = pack_log_std_host(H, D.HP, w_ls, b_ls);
  if (head0 + head.size() != packed.size()) return fail("actor head extent", in, H, 0);
  memcpy(packed.data() + head0, head.data(), head.size() * sizeof(float));
  auto map = [&](uint32_t q, PackQuad& m) { return pack_quad_actor(D, q, m); };
  if (!run_case<PACK_ACTOR_TENSORS>("actor", in, H, packed, src, sizes, head0, PACK_ACTOR_TENSORS, map)) return;
  run_case<PACK_ACTOR_TENSORS>("actor-no-head", in, H, packed, src, sizes, head0, PACK_W_LS, map);
}

void critic_case(int in, int H) {
  Words W;
  const PackDims D = pack_dims_critic(in, H);
  const size_t one[PACK_CRITIC_TENSORS] = {(size_t)H * in, (size_t)H, (size_t)H * H, (size_t)H, (size_t)H, 1};
  size_t sizes[2 * PACK_CRITIC_TENSORS];
  const float* src[2 * PACK_CRITIC_TENSORS];
  urgym_critic_desc d;
  memset(&d, 0, sizeof(d));
  d.in_features = in, d.hidden_width = H, d.n_critics = 2;
  for (int net = 0; net < 2; net++) {
    urgym_q_network& q = d.qf[net];
    q.w0 = W.add(one[0]), q.b0 = W.add(one[1]), q.w1 = W.add(one[2]), q.b1 = W.add(one[3]), q.w_q = W.add(one[4]), q.b_q = W.add(one[5]);
    const float* p[PACK_CRITIC_TENSORS] = {q.w0, q.b0, q.w1, q.b1, q.w_q, q.b_q};
    for (int i = 0; i < PACK_CRITIC_TENSORS; i++) src[PACK_CRITIC_TENSORS * net + i] = p[i], sizes[PACK_CRITIC_TENSORS * net + i] = one[i];
  }
  size_t small_off;
  const std::vector<float> packed = pack_critic_host(&d, &small_off);
  if (packed.size() != pack_critic_floats(D)) return fail("critic sizes", in, H, 0);
  auto map = [&](uint32_t q, PackQuad& m) { return pack_quad_critic(D, q, m), false; };
  run_case<2 * PACK_CRITIC_TENSORS>("critic", in, H, packed, src, sizes, packed.size(), 2 * PACK_CRITIC_TENSORS, map);
}

}  // namespace

// "layout": the C compiler's sizes and offsets of the three output structs, as JSON (the ctypes mirrors are compared with them)
int print_layout() {
#define FIELD(S, f) printf(", \"" #f "\": %zu", offsetof(S, f))
  printf("{\"urgym_actor_params_out\": {\"sizeof\": %zu", sizeof(urgym_actor_params_out));
  FIELD(urgym_actor_params_out, in_features), FIELD(urgym_actor_params_out, hidden_width), FIELD(urgym_actor_params_out, reserved0);
  FIELD(urgym_actor_params_out, w0), FIELD(urgym_actor_params_out, b0), FIELD(urgym_actor_params_out, w1), FIELD(urgym_actor_params_out, b1);
  FIELD(urgym_actor_params_out, w_mu), FIELD(urgym_actor_params_out, b_mu), FIELD(urgym_actor_params_out, w_log_std), FIELD(urgym_actor_params_out, b_log_std);
  printf("}, \"urgym_q_network_out\": {\"sizeof\": %zu", sizeof(urgym_q_network_out));
  FIELD(urgym_q_network_out, w0), FIELD(urgym_q_network_out, b0), FIELD(urgym_q_network_out, w1), FIELD(urgym_q_network_out, b1);
  FIELD(urgym_q_network_out, w_q), FIELD(urgym_q_network_out, b_q);
  printf("}, \"urgym_critic_params_out\": {\"sizeof\": %zu", sizeof(urgym_critic_params_out));
  FIELD(urgym_critic_params_out, in_features), FIELD(urgym_critic_params_out, hidden_width), FIELD(urgym_critic_params_out, reserved0);
  FIELD(urgym_critic_params_out, qf);
  printf("}}\n");
#undef FIELD
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "layout")) return print_layout();
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
