// mppi_noise_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_noise.h, the header the kernel of
// urgym_mppi_noise.hip compiles: tests/test_mppi_noise_host.py compares what it writes with evaluation.mppi_colored_noise, and runs it a
// second time built with -fsanitize=address,undefined.  Arrays travel as raw bytes: FILE in, FILE.out out.
//
//   mppi_noise_harness layout                    sizeof and every offsetof of urgym_mppi_noise as the C compiler lays it out, JSON
//   mppi_noise_harness scale beta_bits           the bits of mppi_noise_scale(beta), JSON
//   mppi_noise_harness color FILE H WIDTH beta_bits
//                                                in: xi f32 [H][WIDTH]; out: eps f32 [H][WIDTH], the recurrence with the host's scale
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_noise.h"

using namespace urgym;

static float from_bits(const char* text) {
  const uint32_t bits = (uint32_t)strtoul(text, nullptr, 10);
  float x;
  memcpy(&x, &bits, sizeof(x));
  return x;
}

static uint32_t to_bits(float x) {
  uint32_t bits;
  memcpy(&bits, &x, sizeof(x));
  return bits;
}

static std::vector<char> slurp(const char* path, size_t bytes) {
  std::vector<char> data(bytes);
  FILE* f = fopen(path, "rb");
  const bool ok = f && fread(data.data(), 1, bytes, f) == bytes && fgetc(f) == EOF;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "%s: expected exactly %zu bytes\n", path, bytes), exit(4);
  return data;
}

static int layout() {
  printf("{\"sizeof\": %zu, \"alignof\": %zu, \"beta\": %zu, \"reserved0\": %zu}\n", sizeof(urgym_mppi_noise), alignof(urgym_mppi_noise),
         offsetof(urgym_mppi_noise, beta), offsetof(urgym_mppi_noise, reserved0));
  return 0;
}

static int scale(char** v) {
  printf("{\"scale\": %u}\n", to_bits(mppi_noise_scale(from_bits(v[0]))));
  return 0;
}

static int color(char** v) {
  const int H = atoi(v[1]);
  const size_t width = strtoull(v[2], nullptr, 10);
  const float beta = from_bits(v[3]);
  const std::vector<char> in = slurp(v[0], (size_t)H * width * 4);
  std::vector<float> xi((size_t)H * width), eps((size_t)H * width, -7.0f);  // every element must be written
  memcpy(xi.data(), in.data(), in.size());
  mppi_noise_host(xi.data(), H, width, beta, mppi_noise_scale(beta), eps.data());
  FILE* f = fopen((std::string(v[0]) + ".out").c_str(), "wb");
  if (!f || fwrite(eps.data(), 4, eps.size(), f) != eps.size()) exit(5);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 3 && !strcmp(argv[1], "scale")) return scale(argv + 2);
  if (argc == 6 && !strcmp(argv[1], "color")) return color(argv + 2);
  fprintf(stderr, "usage: %s layout | scale beta_bits | color FILE H WIDTH beta_bits\n", argv[0]);
  return 2;
}
