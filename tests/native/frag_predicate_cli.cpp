// frag_ranges_ok (csrc/svr_device.h, the region tests/test_frag_setup.py cuts out) over records given on stdin, one per
// line: q0 dq1 dq2 as fp32 bit patterns (hex), A1 B1 A2 B2 as decimal integers, inv_area and the six uv as bit patterns.
// Prints one line of 0 / 1 per record.  tests/test_frag_setup_gpu.py asks it which side of the predicate each of its
// adversarial triangles falls on.
#include <cstdint>
#include <cstdio>
#include <cstring>

#define __host__
#define __device__
#include "frag_setup_under_test.h"

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

int main() {
  unsigned q[3], inv, uvb[6];
  double e[4];
  while (std::scanf("%x %x %x %lf %lf %lf %lf %x %x %x %x %x %x %x", &q[0], &q[1], &q[2], &e[0], &e[1], &e[2], &e[3], &inv, &uvb[0], &uvb[1],
                    &uvb[2], &uvb[3], &uvb[4], &uvb[5]) == 14) {
    float uv[6];
    for (int i = 0; i < 6; i++) uv[i] = from_bits(uvb[i]);
    std::printf("%d\n", svr_layout::frag_ranges_ok(from_bits(q[0]), from_bits(q[1]), from_bits(q[2]), e[0], e[1], e[2], e[3], from_bits(inv), uv) ? 1 : 0);
  }
  return 0;
}
