// column_span (csrc/svr_span.h, the header itself) against the row-by-row predicate it replaces in phase A's column scan:
// for a column of h rows, 1 <= h <= 32, with integer edge values f_i at its first row and integer steps B_i per row, the
// rows k in [0, h) with f_i + k * B_i >= 0 for all three edges -- walked here row by row in fp64 exactly as the scan
// did (f += B: exact, integers below 2^53) -- must be the interval column_span returns.  The brute-force set must be
// contiguous in every case.  Every case runs with the header's fp32 reciprocal pushed by -2 .. +2 ulp (SVR_SPAN_RCP,
// the hook the header offers): whatever the device's v_rcp_f32 rounds to within its documented 1 ulp is covered.
//  random:       seeded cases, h in 1..32, |B_i| up to 2^30 (zero included), |f_i| up to 2^52, in families that make
//                crossings inside the column likely (f near -k * B) as well as anywhere
//  constructed:  ties f = -k * B for k in -1..33, f = -k * B +- 1, |B| = 1 with f across the range, B = 0 with f in
//                {-1, 0, 1}, huge |f| with tiny |B| and the reverse, empty below / above, single rows at both ends,
//                the full column, and the three edges combined so that each in turn sets each end
// Prints "random N constructed M runs R ok", or the first difference and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static int g_ulps = 0;  // what the reciprocal is pushed by
static inline float rcp_under_test(float x) {
  float r = 1.0f / x;
  if (g_ulps == 0 || !std::isfinite(r) || r == 0.0f) return r;
  int32_t b;
  std::memcpy(&b, &r, 4);
  b += (b < 0) ? -g_ulps : g_ulps;  // sign-magnitude: away from / towards zero by whole ulps
  std::memcpy(&r, &b, 4);
  return r;
}
#define SVR_SPAN_RCP(x) rcp_under_test(x)
#define __host__
#define __device__
#include "svr_span.h"

static uint64_t rng_state = 0x53505A41u;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0xbf58476d1ce4e5b9ull;
  return z ^ (z >> 31);
}
static int64_t rnd_mag(int bits) {  // signed, magnitude of up to `bits` bits, every width as likely as another, zero included
  const int w = (int)(rnd64() % (uint64_t)(bits + 1));
  const int64_t m = w ? (int64_t)(rnd64() >> (64 - w)) : 0;
  return (rnd64() & 1u) ? -m : m;
}

static unsigned long long n_runs = 0;

// one case under all five reciprocals; 0 when the span is the brute-force set
static int check(const int64_t fi[3], const int64_t Bi[3], int h) {
  double f[3] = {(double)fi[0], (double)fi[1], (double)fi[2]};
  const double B[3] = {(double)Bi[0], (double)Bi[1], (double)Bi[2]};
  int first = -1, count = 0, last = -1;
  double w0 = f[0], w1 = f[1], w2 = f[2];
  for (int k = 0; k < h; k++) {  // the loop as phase A walked it
    if (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) {
      if (first < 0) first = k;
      last = k;
      count++;
    }
    w0 += B[0];
    w1 += B[1];
    w2 += B[2];
  }
  if (count && last - first + 1 != count) {
    std::printf("not contiguous: f %lld %lld %lld B %lld %lld %lld h %d\n", (long long)fi[0], (long long)fi[1], (long long)fi[2],
                (long long)Bi[0], (long long)Bi[1], (long long)Bi[2], h);
    return 1;
  }
  for (g_ulps = -2; g_ulps <= 2; g_ulps++) {
    int k_first = -99, k_count = -99;
    svr_span::column_span(f[0], f[1], f[2], B[0], B[1], B[2], h, k_first, k_count);
    n_runs++;
    if (k_count != count || (count && k_first != first) || k_first < 0) {
      std::printf("f %lld %lld %lld B %lld %lld %lld h %d rcp %+d ulp: span (%d, %d), rows say (%d, %d)\n", (long long)fi[0], (long long)fi[1],
                  (long long)fi[2], (long long)Bi[0], (long long)Bi[1], (long long)Bi[2], h, g_ulps, k_first, k_count, first, count);
      return 1;
    }
  }
  return 0;
}

static const int64_t F_MAX = (int64_t)1 << 52, B_MAX = (int64_t)1 << 30;
static int64_t clampf(int64_t f) { return f > F_MAX ? F_MAX : (f < -F_MAX ? -F_MAX : f); }

// an edge that passes on every row of any column
static void pass_all(int64_t& f, int64_t& B) { f = F_MAX; B = 0; }

static int random_cases(unsigned long long n, unsigned long long* done) {
  for (unsigned long long c = 0; c < n; c++) {
    int64_t f[3], B[3];
    const int h = 1 + (int)(rnd64() % 32u);
    const unsigned family = (unsigned)(rnd64() % 4u);
    for (int i = 0; i < 3; i++) {
      B[i] = rnd_mag(30);
      if (family == 0) {  // anywhere
        f[i] = rnd_mag(52);
      } else if (family == 1) {  // a crossing in or next to the column, a little off a tie
        const int64_t k = (int64_t)(rnd64() % 36u) - 2;
        f[i] = clampf(-k * B[i] + rnd_mag(family + 1));
      } else if (family == 2) {  // a crossing anywhere in the column, between two rows
        const int64_t k = (int64_t)(rnd64() % 34u) - 1;
        const int64_t a = B[i] < 0 ? -B[i] : B[i];
        f[i] = clampf(-k * B[i] + (a ? (int64_t)(rnd64() % (uint64_t)a) : rnd_mag(3)));
      } else {  // as a triangle has them: two edges hold over most of the column, any may cut it
        f[i] = (rnd64() & 3u) ? clampf(((int64_t)(rnd64() % 40u)) * (B[i] < 0 ? -B[i] : B[i]) + rnd_mag(20)) : rnd_mag(40);
      }
    }
    if (check(f, B, h)) return 1;
    ++*done;
  }
  return 0;
}

static int constructed_cases(unsigned long long* done) {
#define CASE()                      \
  do {                              \
    if (check(f, B, h)) return 1;   \
    ++*done;                        \
  } while (0)
  static const int64_t steps[] = {1, 2, 3, 5, 7, 255, 256, 257, 65535, 65536, 1000003, ((int64_t)1 << 24) - 1, (int64_t)1 << 24, ((int64_t)1 << 24) + 1,
                                  ((int64_t)1 << 29) + 12345, B_MAX - 1, B_MAX};
  int64_t f[3], B[3];
  for (int h = 1; h <= 32; h++) {
    // ties on the boundary row, and one off them, for each edge in turn with the other two passing everywhere
    for (int e = 0; e < 3; e++)
      for (int64_t s : steps)
        for (int sign = -1; sign <= 1; sign += 2)
          for (int64_t k = -1; k <= 33; k++)
            for (int64_t d = -1; d <= 1; d++) {
              for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
              B[e] = sign * s;
              f[e] = -k * B[e] + d;
              CASE();
            }
    // |B| = 1 with f across the whole range
    for (int sign = -1; sign <= 1; sign += 2) {
      for (int64_t v = -40; v <= 40; v++) {
        for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
        B[1] = sign;
        f[1] = v;
        CASE();
      }
      for (int w = 6; w <= 52; w++)
        for (int64_t d = -1; d <= 1; d++)
          for (int fs = -1; fs <= 1; fs += 2) {
            for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
            B[2] = sign;
            f[2] = clampf(fs * (((int64_t)1 << w) + d));
            CASE();
          }
    }
    // B = 0: all rows or none
    for (int e = 0; e < 3; e++)
      for (int64_t v = -1; v <= 1; v++) {
        for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
        B[e] = 0;
        f[e] = v;
        CASE();
      }
    for (int64_t v0 = -1; v0 <= 1; v0++)
      for (int64_t v1 = -1; v1 <= 1; v1++)
        for (int64_t v2 = -1; v2 <= 1; v2++) {
          B[0] = B[1] = B[2] = 0;
          f[0] = v0; f[1] = v1; f[2] = v2;
          CASE();
        }
    // huge |f| with tiny |B|, and the reverse
    for (int e = 0; e < 3; e++)
      for (int fs = -1; fs <= 1; fs += 2)
        for (int bs = -1; bs <= 1; bs += 2) {
          for (int64_t tiny = 1; tiny <= 3; tiny++)
            for (int64_t d = 0; d <= 2; d++) {
              for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
              f[e] = fs * (F_MAX - d);
              B[e] = bs * tiny;
              CASE();
            }
          for (int64_t small = 0; small <= 3; small++)
            for (int64_t d = 0; d <= 2; d++) {
              for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
              f[e] = fs * small;
              B[e] = bs * (B_MAX - d);
              CASE();
            }
        }
    // empty below (crossing before row 0 of a falling edge), empty above (a rising edge crossing at or after row h),
    // a single row at k = 0 and at k = h - 1, the full column
    for (int64_t s : steps) {
      for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
      B[0] = -s; f[0] = -1;                      CASE();  // falls from below zero: none
      B[0] = -s; f[0] = 0;                       CASE();  // row 0 alone (s >= 1)
      B[0] = s;  f[0] = -s * (int64_t)h;         CASE();  // crosses at row h: none
      B[0] = s;  f[0] = -s * (int64_t)h - 1;     CASE();
      B[0] = s;  f[0] = -s * (int64_t)(h - 1);   CASE();  // row h - 1 alone
      B[0] = s;  f[0] = -s * (int64_t)(h - 1) + s - 1; CASE();  // still row h - 1 alone (or more when s == 1 .. the walk decides)
      B[0] = s;  f[0] = 0;                       CASE();  // full
      B[0] = -s; f[0] = s * (int64_t)(h - 1);    CASE();  // full, tie on the last row
      B[0] = -s; f[0] = s * (int64_t)(h - 1) - 1; CASE(); // all but the last row
    }
    // each edge in turn sets each end: a rising edge `lo` opens the span at row a, a falling edge `hi` closes it after
    // row b, the third passes; and two rising (two falling) edges where the later (earlier) one decides
    for (int lo = 0; lo < 3; lo++)
      for (int hi = 0; hi < 3; hi++) {
        if (lo == hi) continue;
        for (int64_t s : {(int64_t)1, (int64_t)256, (int64_t)65537, B_MAX})
          for (int a = 0; a < h; a += (h > 8 ? 3 : 1))
            for (int b = a - 1; b < h; b += (h > 8 ? 4 : 1))
              for (int64_t d = 0; d <= 1; d++) {
                for (int i = 0; i < 3; i++) pass_all(f[i], B[i]);
                B[lo] = s;  f[lo] = -s * (int64_t)a + d * (s - 1);   // crosses at a (d: as late as possible within the row)
                B[hi] = -s; f[hi] = s * (int64_t)b + d * (s - 1);    // last passing row b (b = a - 1: empty)
                CASE();
                const int third = 3 - lo - hi;
                B[third] = s; f[third] = -s * (int64_t)((a + b + 1) / 2);  // a second rising edge, later or earlier than `lo`
                CASE();
                B[third] = -s; f[third] = s * (int64_t)((a + b) / 2);      // a second falling edge
                CASE();
              }
      }
  }
#undef CASE
  return 0;
}

int main(int argc, char** argv) {
  unsigned long long n_random = 12000000ull, random_done = 0, constructed_done = 0;
  if (argc > 1) n_random = std::strtoull(argv[1], nullptr, 10);
  if (constructed_cases(&constructed_done)) return 1;
  if (random_cases(n_random, &random_done)) return 1;
  std::printf("random %llu constructed %llu runs %llu ok\n", random_done, constructed_done, n_runs);
  return 0;
}
