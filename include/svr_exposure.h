/* svr_exposure.h — auto-exposure: the colour target's luminance metered on the device, an exposure adapted in device
 * memory, and a post pass that reads it there.
 *
 * svr_post_pass (include/svr_post.h) scales the RGBA16F target by a host constant.  With thousands of lights adding into
 * the target the right constant moves by orders of magnitude from one view to the next, and finding it on the host costs
 * a fence and a read-back of the whole target per frame.  svr_meter_exposure finds it where the frame is: a 256-bin
 * histogram of log2 luminance over the scissor's pixels, a percentile window over its non-black pixels, the window's
 * geometric mean mapped to a key value, and an exposure that moves towards that target by a fraction per meter.  With
 * svr_set_post_auto_exposure on, later post passes multiply their own exposure (then a compensation) by the state's.
 *
 * The meter reads the scissor's pixels of the context's RGBA16F colour target and writes only the context-owned state
 *   - Colour, depth, IDs, the attribute planes, the ambient plane and the temporal histories are untouched.
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.  Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call reads colour.
 *
 * Arithmetic; san(v) = v > 0 ? min(v, 65504) : 0
 *   - L = fmaf(0.0722f, san(b), fmaf(0.7152f, san(g), 0.2126f * san(r))), fp32;
 *   - L < 2^-16 counts as black; else bin = (bits(L) >> 20) - 888: eight bins per octave over [2^-16, 2^16);
 *   - counts are uint32 sums, so the histogram does not depend on the order the pixels were counted in;
 *   - T = the sum of the bins; the kept pixels are the cumulative ranks [floor(low_fraction T), ceil(high_fraction T)),
 *     both products taken in fp64; an empty window (T = 0 among them) leaves exposure, target and mean_log2 as they
 *     were, and still sets counted and black, and counts in meters;
 *   - mean_log2 = the kept pixels' mean of (octave - 16) + log2(1 + (j + 1/2) / 8), j the bin's place in its octave, from
 *     integer totals, in fp64, rounded to fp32 once;
 *   - target = clamp(key * 2^(-mean_log2), min_exposure, max_exposure), 2^x a stated polynomial;
 *   - exposure = target where the meter snaps, else fmaf(adapt, target - exposure, exposure).
 *   The first accepted meter of a context snaps, and so does the first after svr_reset_exposure, whatever their adapt.
 *   Whether a meter snaps is decided at the call and travels with the logged operation.
 *
 * The post pass with auto-exposure on: e = pass.exposure * state.exposure, one fp32 multiply on the device, stands
 * wherever C23 and C26 say `exposure`.  Before any meter the state's exposure is 1.0, so the pass is what it was.
 *
 * Refusals, with nothing changed (SVR_ERR_INVALID_ARGUMENT): null arguments; a key, min_exposure or max_exposure that is
 * not finite and greater than 0; max_exposure below min_exposure; low_fraction outside [0, 1); high_fraction outside
 * (low_fraction, 1]; adapt outside [0, 1]; a histogram buffer of another size than 256 * 4 bytes.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_post_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the meter changes nothing and runs again, once, in call order behind the
 *     replayed passes and in front of any post pass that reads its result; a meter that ran before the overflowing pass
 *     is not run again (DESIGN.md §5 "Auto-exposure").  The result is that of applying every meter exactly once.
 *   - The state (24 bytes), the working bins and the copy of the last histogram are owned by the context, allocated and
 *     initialised (exposure 1.0, target 1.0, everything else 0) by whichever call below comes first.
 *     svr_get_exposure_state gives the state's device address, stable for the context's life: a caller's own kernels
 *     may read it in stream order.
 *
 * Out of scope
 *   - Multiview layers, RGBA8 targets, interleaved row ownership.
 *   - The sharded frame (svr_dist.h): each rank meters its own band, so the ranks' exposures disagree.  The histogram is
 *     resident on the device: it is what a later all-reduce would sum.
 *
 * HIP library only: the CPU oracle has no auto-exposure.
 */
#ifndef SVR_EXPOSURE_H
#define SVR_EXPOSURE_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_EXPOSURE_BINS 256

typedef struct SvrExposureMeter {
  float key;           /* luminance the kept pixels' geometric mean is mapped to; finite, > 0 (0.18 is usual) */
  float low_fraction;  /* share of the non-black pixels dropped from the dark end, in [0, 1) */
  float high_fraction; /* share kept up to, in (low_fraction, 1] */
  float min_exposure;  /* finite, > 0 */
  float max_exposure;  /* finite, >= min_exposure */
  float adapt;         /* in [0, 1]: exposure += adapt * (target - exposure); 1 goes all the way */
} SvrExposureMeter; /* 24 bytes */

typedef struct SvrExposureState {
  float exposure;   /* what svr_post_pass multiplies by when auto-exposure is on; 1.0 until the first meter */
  float target;     /* of the last meter with a window, after the clamp */
  float mean_log2;  /* of the kept pixels' luminance */
  uint32_t counted; /* non-black pixels of the last meter */
  uint32_t black;   /* pixels below the lowest bin (zero, NaN and negative count here) */
  uint32_t meters;  /* meters applied so far */
} SvrExposureState; /* 24 bytes */

/* Meter the scissor's pixels of the colour target and adapt the state (see above). */
int svr_meter_exposure(SvrContext* ctx, const SvrExposureMeter* meter);
/* The next accepted meter snaps, whatever its adapt.  The state itself is left as it is. */
int svr_reset_exposure(SvrContext* ctx);
/* on != 0: later svr_post_pass calls use pass.exposure * state.exposure.  Legal before any meter. */
int svr_set_post_auto_exposure(SvrContext* ctx, int on);
/* The state behind everything enqueued so far (a fence). */
int svr_read_exposure(SvrContext* ctx, SvrExposureState* out);
/* The last applied meter's SVR_EXPOSURE_BINS bins (a fence); bytes must be SVR_EXPOSURE_BINS * 4.  All 0 before any. */
int svr_debug_read_exposure_histogram(SvrContext* ctx, uint32_t* out, size_t bytes);
/* The device address of the SvrExposureState. */
int svr_get_exposure_state(SvrContext* ctx, const void** device);

#ifdef __cplusplus
}
#endif
#endif /* SVR_EXPOSURE_H */
