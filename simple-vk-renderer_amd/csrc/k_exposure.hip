// k_exposure.hip — auto-exposure (include/svr_exposure.h): the histogram of the colour target's log2 luminance and the
// exposure adapted from it, both in device memory.  Arithmetic: DESIGN.md C38-C42; ordering and the exactly-once
// argument: DESIGN.md §5 "Auto-exposure".
//
// Two kernels (launch_exposure):
//   exposure_histogram_kernel   a bounded grid (exposure_grid); a workgroup of 256 lanes walks chunks of 512 pixels of
//                               one scissor row, eight chunks' loads in flight at a time.  A lane takes two pixels: one
//                               16-byte load where the address allows, else one pixel at a time.  Counts go into a
//                               private histogram per wave in LDS (257 counters: the bins, then black); at the end the
//                               workgroup sums its four copies and issues one global integer atomic add per non-zero
//                               bin, lanes on consecutive bins.
//   exposure_resolve_kernel     one workgroup of 256 lanes, a bin per lane: prefix sum, the kept window, the integer
//                               totals, then lane 0 does C40-C42 and writes the state.  Every lane copies its bin into
//                               the last-histogram words and zeroes it for the next meter.
// Plain vector loads, LDS atomics and global integer atomics only; nothing is handed between workgroups of one launch.
// Both kernels read the context's poison flag first: after an overflow they change nothing, so the working bins stay
// zero across a void meter.
#include "svr_exp2.h"
#include "svr_launch.h"
#include "svr_pixel.h"

namespace svr {

namespace {

constexpr uint32_t BINS = SVR_EXPOSURE_BINS;
constexpr uint32_t BLACK = BINS;         // the counter behind the bins
constexpr uint32_t NO_BIN = 0xffffffffu;  // a lane without a pixel
constexpr uint32_t CHUNK = 512u;          // pixels of one row a workgroup takes at a time: 256 lanes x 2
#if defined(SVR_AB_EXPOSURE_GRID) && defined(SVR_AB_EXPOSURE_BATCH)  // A/B builds only
constexpr uint32_t GRID_MAX = SVR_AB_EXPOSURE_GRID, BATCH = SVR_AB_EXPOSURE_BATCH;
#else
// Measured (DESIGN.md §5 "Auto-exposure"): every workgroup ends with up to 257 global atomics on the same 257 words, so
// the grid is kept small and the loads in flight come from the batch instead: 512 x 8 beat 1024 x 4, 256 x 8 and 2048 x 4.
constexpr uint32_t GRID_MAX = 512u;       // two workgroups for each of the 256 compute units
constexpr uint32_t BATCH = 8u;            // chunks whose loads are issued before the first is counted
#endif

// C38, C39: the counter of one texel.
// The top bound: san() leaves each channel in [0, 65504].  The three weights as fp32 are 0x1.b367ap-3, 0x1.6e2eb2p-1 and
// 0x1.27bb3p-4; their sum is 1 exactly.  Each of the three roundings grows the value by at most a factor
// 1 + 2^-24, so L <= 65504 (1 + 2^-24)^3 < 65504.02 < 2^16, whose exponent field is 142 at most:
// (bits(L) >> 20) - 888 <= 142 * 8 + 7 - 888 = 255.  The min() of the contract never binds; it is kept, as one v_min.
// The bottom: L >= 2^-16 has an exponent field of 111 at least, and 111 * 8 = 888.  L is never NaN or negative.
__device__ __forceinline__ uint32_t bin_of(uint2 t) {
  const Rgb c = decode_rgb(t);
  const float r = san(c.r), g = san(c.g), b = san(c.b);
  const float L = fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r));
  if (L < 0x1p-16f) return BLACK;
  return min((__float_as_uint(L) >> 20) - 888u, BINS - 1u);
}

// One count per lane with a pixel, into the wave's own histogram.  A flat image puts all 64 lanes on one counter, and
// same-address LDS atomics of a wave run one after the other: the bin of the first lane with a pixel is peeled, counted
// by a ballot and added once; the other lanes add their own.  Every lane of the wave must arrive here.
__device__ __forceinline__ void count(uint32_t* hist, uint32_t bin) {
#ifdef SVR_AB_EXPOSURE_NO_PEEL  // A/B builds only: every lane adds its own
  if (bin != NO_BIN) atomicAdd(&hist[bin], 1u);
#else
  const unsigned long long with_pixel = __ballot(bin != NO_BIN);
  if (with_pixel == 0ull) return;
  const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)with_pixel) - 1);
  const unsigned long long same = __ballot(bin == lead);
  if (bin == lead) {
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&hist[lead], (uint32_t)__popcll(same));
  } else if (bin != NO_BIN) {
    atomicAdd(&hist[bin], 1u);
  }
#endif
}

}  // namespace

struct HistogramArgs {
  const uint2* color;  // texel (0, 0) of the scissor
  uint32_t pitch;      // texels per row of the target
  uint32_t sw, sh;
  uint32_t segs;       // chunks per row: (sw + CHUNK - 1) / CHUNK
  uint32_t n_chunks;   // sh * segs
  uint32_t* bins;      // the working bins: BINS counters, then black
  const uint32_t* poison;
};

__global__ __launch_bounds__(256) void exposure_histogram_kernel(HistogramArgs A) {
  if (*A.poison) return;
  __shared__ uint32_t s_hist[4][BINS + 1u];
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < 4u * (BINS + 1u); i += 256u) (&s_hist[0][0])[i] = 0u;
  __syncthreads();
  uint32_t* hist = s_hist[t >> 6];

  // the trip count is the workgroup's: every lane of a wave reaches every count()
  for (uint32_t c0 = blockIdx.x; c0 < A.n_chunks; c0 += BATCH * gridDim.x) {
    uint2 pa[BATCH], pb[BATCH];
    uint32_t n[BATCH];  // pixels this lane holds of chunk k: 0, 1 or 2
#pragma unroll
    for (uint32_t k = 0; k < BATCH; k++) {
      const uint32_t c = c0 + k * gridDim.x;
      n[k] = 0u;
      pa[k] = pb[k] = make_uint2(0u, 0u);
      if (c < A.n_chunks) {
        const uint32_t y = c / A.segs, x = (c - y * A.segs) * CHUNK + 2u * t;
        if (x < A.sw) {
          const uint2* at = A.color + (size_t)y * A.pitch + x;
          if (x + 1u < A.sw && aligned_to(at, 16u)) {
            const uint4 q = *reinterpret_cast<const uint4*>(at);
            pa[k] = make_uint2(q.x, q.y);
            pb[k] = make_uint2(q.z, q.w);
            n[k] = 2u;
          } else {
            pa[k] = at[0];
            n[k] = 1u;
            if (x + 1u < A.sw) {
              pb[k] = at[1];
              n[k] = 2u;
            }
          }
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < BATCH; k++) {
      if (c0 + k * gridDim.x >= A.n_chunks) break;  // the workgroup's, not the lane's
      count(hist, n[k] >= 1u ? bin_of(pa[k]) : NO_BIN);
      count(hist, n[k] >= 2u ? bin_of(pb[k]) : NO_BIN);
    }
  }
  __syncthreads();

  const uint32_t sum = s_hist[0][t] + s_hist[1][t] + s_hist[2][t] + s_hist[3][t];
  if (sum) atomicAdd(&A.bins[t], sum);
  if (t == 0u) {
    const uint32_t black = s_hist[0][BLACK] + s_hist[1][BLACK] + s_hist[2][BLACK] + s_hist[3][BLACK];
    if (black) atomicAdd(&A.bins[BLACK], black);
  }
}

struct ResolveArgs {
  uint32_t* mem;  // EXPOSURE_WORDS words: state, working bins, last histogram
  SvrExposureMeter meter;
  uint32_t snap;
  const uint32_t* poison;
};

// C40: log2(1 + (j + 1/2) / 8), j = 0 .. 7, as fp64
__device__ const double kSubLog2[8] = {0x1.663f6fac91316p-4, 0x1.fbc16b902680ap-3, 0x1.91bba891f1709p-2, 0x1.0c10500d63aa6p-1,
                                       0x1.49a784bcd1b8bp-1, 0x1.82809d5be7073p-1, 0x1.b74948f5532dap-1, 0x1.e88c6b3626a73p-1};

// C41's 2^x for |x| <= 16: exp2_poly of svr_exp2.h

__global__ __launch_bounds__(256) void exposure_resolve_kernel(ResolveArgs A) {
  if (*A.poison) return;
  __shared__ uint32_t s_scan[BINS];
  __shared__ uint32_t s_kept[BINS];
  __shared__ uint32_t s_sub[8];
  __shared__ uint32_t s_oct[32];
  const uint32_t t = threadIdx.x;
  uint32_t* bins = A.mem + EXPOSURE_STATE_WORDS;
  const uint32_t mine = bins[t];
  const uint32_t black = bins[BLACK];

  s_scan[t] = mine;
  __syncthreads();
  for (uint32_t d = 1u; d < BINS; d <<= 1) {  // inclusive prefix sum
    const uint32_t v = t >= d ? s_scan[t - d] : 0u;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const uint32_t T = s_scan[BINS - 1u], end = s_scan[t], begin = end - mine;

  // C40: the kept ranks [lo, hi); low T < 2^56 is exact in fp64 below T = 2^29 and correctly rounded above; hi <= T
  // because high <= 1
  const uint32_t lo = (uint32_t)floor((double)A.meter.low_fraction * (double)T);
  const uint32_t hi = (uint32_t)ceil((double)A.meter.high_fraction * (double)T);
  const uint32_t from = max(begin, lo), to = min(end, hi);
  s_kept[t] = to > from ? to - from : 0u;
  __syncthreads();
  if (t < 8u) {  // per place in the octave
    uint32_t s = 0u;
    for (uint32_t o = 0; o < 32u; o++) s += s_kept[8u * o + t];
    s_sub[t] = s;
  } else if (t >= 64u && t < 96u) {  // per octave
    uint32_t s = 0u;
    for (uint32_t j = 0; j < 8u; j++) s += s_kept[8u * (t - 64u) + j];
    s_oct[t - 64u] = s;
  }
  __syncthreads();

  A.mem[EXPOSURE_STATE_WORDS + EXPOSURE_BINS_WORDS + t] = mine;
  bins[t] = 0u;
  if (t != 0u) return;
  bins[BLACK] = 0u;
  SvrExposureState* st = reinterpret_cast<SvrExposureState*>(A.mem);
  st->counted = T;
  st->black = black;
  st->meters += 1u;
  uint32_t kept = 0u;
  unsigned long long octaves = 0ull;
  for (uint32_t o = 0; o < 32u; o++) {
    kept += s_oct[o];
    octaves += (unsigned long long)o * s_oct[o];
  }
  if (kept == 0u) return;  // an empty window, T == 0 among them
  double acc = (double)((long long)octaves - 16ll * (long long)kept);  // an integer below 2^37: exact
  for (uint32_t j = 0; j < 8u; j++) acc = acc + (double)s_sub[j] * kSubLog2[j];
  const float mean_log2 = (float)(acc / (double)kept);
  // C42
  const float raw = A.meter.key * exp2_poly(-mean_log2);
  const float target = raw < A.meter.min_exposure ? A.meter.min_exposure : (raw > A.meter.max_exposure ? A.meter.max_exposure : raw);
  st->mean_log2 = mean_log2;
  st->target = target;
  st->exposure = A.snap ? target : fmaf(A.meter.adapt, target - st->exposure, st->exposure);
}

uint32_t exposure_grid(uint32_t sw, uint32_t sh) {
  const unsigned long long chunks = (unsigned long long)((sw + CHUNK - 1u) / CHUNK) * sh;
  return (uint32_t)(chunks < GRID_MAX ? chunks : GRID_MAX);
}

void launch_exposure(const ExposureLaunch& E, hipStream_t s) {
  if (E.sw != 0u && E.sh != 0u) {
    HistogramArgs H{};
    H.color = E.color + (size_t)E.sy * E.W + E.sx;
    H.pitch = E.W;
    H.sw = E.sw;
    H.sh = E.sh;
    H.segs = (E.sw + CHUNK - 1u) / CHUNK;
    H.n_chunks = H.segs * E.sh;
    H.bins = E.mem + EXPOSURE_STATE_WORDS;
    H.poison = E.poison;
    hipLaunchKernelGGL(exposure_histogram_kernel, dim3(exposure_grid(E.sw, E.sh)), dim3(256), 0, s, H);
  }
  ResolveArgs R{};
  R.mem = E.mem;
  R.meter = E.meter;
  R.snap = E.snap;
  R.poison = E.poison;
  hipLaunchKernelGGL(exposure_resolve_kernel, dim3(1), dim3(256), 0, s, R);
}

}  // namespace svr
