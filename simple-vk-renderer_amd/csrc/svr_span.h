// The covered rows of one pixel column, found once and exactly (phase A).
//
// A work item of the column scan (k_tile.hip scan_columns) is one pixel column of a triangle's tile-clamped box: h rows,
// 1 <= h <= 32.  Its three edge values at the first row are f0, f1, f2 and grow by B0, B1, B2 per row; all six are
// integers below 2^53 in magnitude (edge functions over snapped vertices), so f + k * B is exact in fp64 for every
// row of the box.  Row k is covered when all three values are >= 0.  Each edge is linear in k, so it admits a prefix
// of the rows (B < 0), a suffix (B > 0), or all or none (B == 0), and the covered rows are one interval:
//
//     column_span(f0, f1, f2, B0, B1, B2, h, k_first, k_count):
//         { k in [0, h) : f_i + k * B_i >= 0 for i = 0, 1, 2 }  ==  [k_first, k_first + k_count),   k_count == 0: empty
//
// Per edge the figure wanted is the crossing c, clamped to [0, h]: the number of leading rows on which the edge has
// NOT yet taken the sign it ends with.  With q = -f / B (real arithmetic):
//     B > 0: rows k >= ceil(q) pass       c = ceil(q)        the edge admits [c, h)
//     B < 0: rows k <= floor(q) pass      c = floor(q) + 1   the edge admits [0, c)
// Both are found the same way.
//  1. An estimate in fp32: x = fma((float)-f, rcp((float)B), -2^-14), c_low = clamp(floor(x) + 1, 0, h).
//     The two conversions are off by at most 2^-24 each (relative), the reciprocal by at most 1 ulp (2^-23) as the
//     ISA documents for v_rcp_f32 -- the proof has room for 5 ulp, and tests/native/column_span_check.cpp runs it
//     with the reciprocal pushed by -2 .. +2 ulp through SVR_SPAN_RCP: the product is within (3 + 10) * 2^-24 <
//     2^-20 of q relatively.  For |q| <= 34 that is under 0.54 * 2^-14 absolutely, and the fma's one rounding of
//     the sum (|x| < 35) is under 2^-18: q - 2^-13 < x < q, strictly on both sides.  Hence floor(x) + 1 is c or
//     c - 1: for B < 0 because floor(q) - 1 <= floor(x) <= floor(q); for B > 0 because x < q gives floor(x) + 1 <=
//     ceil(q) and x > q - 1 gives floor(x) >= ceil(q) - 2 + 1.  Outside |q| <= 34 the estimate keeps q's sign and
//     stays above 33 or below -1 (the relative bound), and the clamp gives what clamping c gives.  The operands are
//     integers, |f| >= 1 or f == 0 and 1 <= |B| < 2^53: no denormal, overflow or NaN arises while B != 0.
//  2. One exact test decides between the two candidates: e = fma(B, c_low, f) is f + c_low * B rounded ONCE, and
//     rounding keeps the sign of a non-zero value and leaves zero zero, so (e >= 0) is the row's own predicate even
//     where c_low == h lies one row outside the box.  If row c_low has not crossed yet, c = c_low + 1.  (c_low == h
//     may thus end as h + 1: "crossing beyond the box", which the clamps of the intersection take as h.)
// B == 0: the edge admits all rows (f >= 0) or none; said as an edge of the second kind with c = h or 0.
// The estimate (float) is clamped BEFORE it is converted: no float-to-integer conversion out of range anywhere.
//
// Self-contained, __host__ __device__: tests/native/column_span_check.cpp compiles it with plain g++ (the two
// qualifiers defined away) against the row-by-row predicate.
#pragma once

#ifndef SVR_SPAN_RCP  // the test's hook: the fp32 reciprocal, which the proof allows to be off by 4 ulp
#if defined(__HIP_DEVICE_COMPILE__)
#define SVR_SPAN_RCP(x) __builtin_amdgcn_rcpf(x)
#else
#define SVR_SPAN_RCP(x) (1.0f / (x))
#endif
#endif

namespace svr_span {

// One edge's admitted rows [lo, hi) as floats (small integers, exact), before the clamp to [0, h] of the caller.
__host__ __device__ inline void edge_rows(double f, double B, float hf, float& lo, float& hi) {
  const float x = __builtin_fmaf((float)-f, SVR_SPAN_RCP((float)B), -0x1p-14f);
  float c = __builtin_fminf(__builtin_fmaxf(__builtin_floorf(x) + 1.0f, 0.0f), hf);  // (B == 0: x is +-inf or NaN, c any of 0..h; replaced below)
  const bool rising = B > 0.0;
  const bool passes = __builtin_fma(B, (double)c, f) >= 0.0;  // row c's own predicate, exact in sign
  c += (passes != rising) ? 1.0f : 0.0f;                       // not crossed yet at c: the crossing is the next row
  if (B == 0.0) c = f >= 0.0 ? hf : 0.0f;
  lo = rising ? c : 0.0f;
  hi = rising ? hf : c;
}

__host__ __device__ inline void column_span(double f0, double f1, double f2, double B0, double B1, double B2, int h, int& k_first, int& k_count) {
  const float hf = (float)h;
  float lo, hi, l, r;
  edge_rows(f0, B0, hf, lo, hi);  // one edge after the other: an edge's temporaries are dead before the next one's live
  edge_rows(f1, B1, hf, l, r);
  lo = __builtin_fmaxf(lo, l);
  hi = __builtin_fminf(hi, r);
  edge_rows(f2, B2, hf, l, r);
  lo = __builtin_fmaxf(lo, l);
  hi = __builtin_fminf(__builtin_fminf(hi, r), hf);
  k_first = (int)lo;                                  // 0 .. h + 1
  k_count = (int)__builtin_fmaxf(hi - lo, 0.0f);      // 0 .. h
}

}  // namespace svr_span
