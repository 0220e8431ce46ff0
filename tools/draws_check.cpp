// Stand-alone host print-out of the draw conventions (csrc/draws.h over csrc/tok_hash.h); no HIP, no library:
//
//   g++ -std=c++17 tools/draws_check.cpp -o draws_check && ./draws_check
//
// It includes the headers the kernels include, so what it prints is what they compute: tests/test_draws_cpu.py holds
// isaacgyminsertion_amd/draws.py to it line for line, and the pinned hashes of tests/test_oracle_token_dropout.py are
// its `hash` lines (the triples below are that list's; regenerate the values from here).  Lines:
//   hash <seed> <site> <element> <tok_hash>
//   threshold <p> <draw_threshold(p)>
//   unit <h> <bits of draw_u(h)> <bits of draw_unit(h)>        (fp32 bit patterns, in hex)
//   index <h> <n> <draw_index(h, n)>
//   plane <name> <number>  /  site <name> <number>
#include <stdio.h>
#include <string.h>

#include "../isaacgyminsertion_amd/csrc/draws.h"

namespace {
using namespace igi;

const unsigned long long SEEDS[] = {0ull, 12345ull, 0x123456789ABCDEFull, 0x3FFFFFFF00000001ull, 0x1234567890ABCDEFull,
                                    0x7FFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull};
const unsigned int SITES[] = {0, 1, 3, 6, 7, 14, 22, 30};
const unsigned int ELEMENTS[] = {0u, 1u, 31u, 70001u, 393215u, 4294967295u};
const double PROBS[] = {0.0, 0.1, 0.3, 0.5, 0.75, 1.0};
const unsigned int HASHES[] = {0u, 1u, 255u, 256u, 0x7FFFFFFFu, 0x80000000u, 0x800000FFu, 0x9E3779B1u, 0xFFFFFF00u, 0xFFFFFFFFu};
const unsigned long long COUNTS[] = {1, 3, 37, 4096};

unsigned int bits(float v) {
  unsigned int b;
  memcpy(&b, &v, sizeof b);
  return b;
}
}  // namespace

int main() {
  for (unsigned long long seed : SEEDS)
    for (unsigned int site : SITES)
      for (unsigned int e : ELEMENTS) printf("hash %llu %u %u %u\n", seed, site, e, tok_hash(seed, site, e));
  for (double p : PROBS) printf("threshold %.17g %llu\n", p, draw_threshold(p));
  for (unsigned int h : HASHES) printf("unit %u %08x %08x\n", h, bits(draw_u(h)), bits(draw_unit(h)));
  for (unsigned int h : HASHES)
    for (unsigned long long n : COUNTS) printf("index %u %llu %u\n", h, n, draw_index(h, n));
  for (const DrawName& r : DRAW_PLANES) printf("plane %s %u\n", r.name, r.number);
  for (const DrawName& r : DRAW_SITES) printf("site %s %u\n", r.name, r.number);
  return 0;
}
