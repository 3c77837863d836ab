/*
 * baler_amd_frames.h -- the frame-statistics entry points of libbaler_amd.so: the report mode for 2-D data.  Included by
 * baler_amd.h, whose conventions (status codes, bamd_dtype, caller-owned device buffers, everything enqueued on `stream`,
 * nothing read or written outside the arrays a call is given) hold here; the 38 entry points declared there are unchanged.
 *
 * Both functions take two row-major tables before / after (n_frames, frame_elems) of `dtype`, BAMD_F32 or BAMD_F64 (anything else:
 * BAMD_ERR_INVALID); frame_elems >= 1 of any size, n_frames >= 0.  Handle-free.  Null pointers and negative sizes are refused by
 * name before anything is launched.  Arithmetic: d = before - after in the input dtype with one rounding (numpy's subtract), then
 * widened; every square and every sum is float64; extrema skip NaN (a frame or pixel without a value that is not NaN has
 * +inf / -inf); sums propagate inf / NaN as IEEE does.  No float atomics: two calls give the same bits.
 */
#ifndef BALER_AMD_FRAMES_H
#define BALER_AMD_FRAMES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces: the per-frame data path of plotting.plot_2D (plotting.py:404-423): diff = data[ind] - decompressed[ind] (the sign is the
 * opposite of plot_1D's residual), max_value = np.amax([np.amax(tile), np.amax(tile_dec)]) and min_value likewise -- the colour
 * scale of the three imshow panels -- for EVERY frame in one pass, plus the sums behind the per-frame error figures.
 * out: (10, n_frames) float64, device memory, one row per statistic of every frame:
 *    0 min(before)   1 max(before)   2 min(after)   3 max(after)   4 min(d)   5 max(d)
 *    6 sum(d)        7 sum(d^2)      8 sum(before^2)
 *    9 number of elements where before or after is NaN   (np.amin / np.amax propagate NaN: the caller turns a non-zero count
 *      into the NaN colour scale of the reference, baler_amd.native.frame_summary)
 * diff: NULL, or (n_frames, frame_elems) of `dtype`, device memory: receives d bit for bit.
 * Order rule: a frame's ten values are a pure function of the frame's values and of frame_elems -- they do not depend on n_frames,
 * on the frame's index, on how the table was cut into calls, on the 16-byte alignment of any base address or on the grid.
 * n_frames = 0: BAMD_OK, nothing is written. */
int bamd_frame_stats(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems,
                     double *out, void *diff, void *stream);
/* Has no counterpart in the reference (plot_2D draws frame by frame): the per-pixel error map over all frames, the column
 * reduction of the same d -- where in the field the autoencoder fails.
 * out: (5, frame_elems) float64, device memory, per pixel over the frames:
 *    0 sum(d)   1 sum(d^2)   2 min(d)   3 max(d)   4 number of frames where that pixel is NaN in before or after
 * accumulate != 0: `out` holds the result of earlier calls and this call's frames are added to it (sums and counts add, extrema
 * combine), so a table can be fed in frame chunks.  The order of a call's sums depends on (n_frames, frame_elems) alone.
 * n_frames = 0: BAMD_OK; `out` is set to the neutral elements (0, 0, +inf, -inf, 0), or left alone under accumulate. */
int bamd_pixel_moments(const void *before, const void *after, int dtype, int64_t n_frames, int64_t frame_elems,
                       double *out, int accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BALER_AMD_FRAMES_H */
