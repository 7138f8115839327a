/*
 * fosphor_amd_view.h -- zoomed, display-width views of the plain device buffers
 *
 * The reference zooms with texture coordinates: struct fosphor_render carries freq_center, freq_span and wf_span, and its GL side
 * stretches the matching part of the waterfall / histogram textures over the quad (lib/fosphor/gl.c:396-400, 430-431, 477-478,
 * 508-509); its demo keeps a second, zoomed render next to the main one (lib/fosphor/main.c:188-237).  Without GL the same job is a
 * device pass: it reduces a frequency window and a time window of the instance's buffers to a picture of the caller's pixel size,
 * and can colour it in the same launch (the lookup of fosphor_amd_cmap.h).  At fft_len_log = 16 a full-resolution picture is
 * 65536 pixels wide; a view of it is as wide as the window it is drawn in.
 *
 * The pass only reads the instance: no state of it is written.
 */
#ifndef FOSPHOR_AMD_VIEW_H
#define FOSPHOR_AMD_VIEW_H

#include <stdint.h>

#include "fosphor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Detectors: how the cells that one pixel covers become that pixel's value.
 *   PEAK     fmaxf over the cells, in any order: a NaN cell is ignored unless every cell is NaN; +0 and -0 are not told apart.
 *            Exact: the value is one of the cells (numpy: np.fmax.reduce).
 *   AVERAGE  the float32 sum of the cells (in an order of the kernel's choosing) times the float32 reciprocal of their count;
 *            non-finite cells propagate as IEEE arithmetic has it.  For k cells:
 *            |result - mean| <= k * 2^-24 * mean(|cell|) + 2^-23 * |mean|. */
#define FOSPHOR_AMD_DET_PEAK    0
#define FOSPHOR_AMD_DET_AVERAGE 1

/* The window and the picture size.  Columns are counted fft-shifted, as on screen: column 0 is -fs/2, column N/2 is DC.
 *
 * Pixel-to-cell mapping, the same along frequency and along time: output index p of n_out covers the source indices [lo, hi) of
 * n_src with   lo = floor(p * n_src / n_out),   hi = max(lo + 1, floor((p + 1) * n_src / n_out))   (fosphor_amd_view_span).
 * With n_src >= n_out the spans tile [0, n_src) without gap or overlap; with n_src < n_out every pixel shows exactly one cell
 * (nearest, repeated) -- there is no interpolation between cells (the reference's GL_LINEAR magnification is not reproduced).
 *
 *   frequency:  n_src = n_cols, n_out = width; source index i is shifted column first_bin + i, which is memory column
 *               (first_bin + i) ^ (N/2) of the waterfall and the histogram and vertex first_bin + i of the spectrum lines
 *   time:       n_src = wf_src_rows, n_out = wf_out_rows; source index j (0 = newest) is ring row (waterfall_pos - 1 - j) mod wf_rows
 *   histogram rows are never resampled: output row r is dB bin n_bins - 1 - r
 *
 * The waterfall is reduced over the 2-D block (row span x column span); histogram, live and max-hold over the column span. */
struct fosphor_amd_view
{
	int first_bin;		/* first fft-shifted column of the window, 0 .. N - 1 */
	int n_cols;		/* shifted columns in the window, 1 .. N - first_bin */
	int width;		/* output pixels across, 1 .. 65536 */
	int wf_src_rows;	/* newest waterfall rows in the window, 1 .. wf_rows */
	int wf_out_rows;	/* output waterfall rows, 1 .. wf_rows */
	int detector;		/* FOSPHOR_AMD_DET_* */
};

/* Colouring of one picture: the palette, n, use_defaults, scale and offset arguments of fosphor_amd_colorize with their meaning
 * (palette in HOST memory or NULL for the reference's 256 entries; use_defaults != 0 for the reference's scale / offset). */
struct fosphor_amd_view_color
{
	const uint32_t *palette;
	int   n;
	int   use_defaults;
	float scale, offset;
};

/* What to produce: device pointers, any of which may be NULL (= not produced; at least one must be set).
 * An RGBA picture is   lookup(value)   of the float picture of the same call, bit for bit, whether or not the latter is stored. */
struct fosphor_amd_view_out
{
	float    *d_waterfall;		/* [wf_out_rows][width], row 0 = newest */
	float    *d_histogram;		/* [n_bins][width], row 0 = highest dB bin */
	float    *d_live, *d_max;	/* [width]: y of the live / max-hold vertices */
	uint32_t *d_waterfall_rgba;	/* [wf_out_rows][width] */
	uint32_t *d_histogram_rgba;	/* [n_bins][width] */
	struct fosphor_amd_view_color wf_color, histo_color;	/* read only for the RGBA picture they belong to */
};

/* Render a view.  Waits for pending fosphor_process work first (fosphor_amd_finish), runs on the instance's stream and returns when
 * the outputs are complete.  0; -EINVAL: a field of *v out of range, an unknown detector, nothing to produce, a palette of fewer than
 * 2 or more than 4096 entries (nothing is written); -EIO: device error. */
int fosphor_amd_view(struct fosphor *self, const struct fosphor_amd_view *v, const struct fosphor_amd_view_out *out);

/* View launches since the instance was made, by the form the launch took.  The form follows from the shape of the view, never from
 * the data:
 *   stats[FOSPHOR_AMD_VIEW_TILED]        picture launches in which a work-group reads the columns of several pixels at once and
 *                                        one lane reduces each pixel
 *   stats[FOSPHOR_AMD_VIEW_TILED_LANES]  ... and 2 .. 64 lanes share a pixel (spans of 8 cells and more)
 *   stats[FOSPHOR_AMD_VIEW_WIDE]         picture launches in which a pixel's span is longer than one work-group's read (about 1000
 *                                        cells): the lanes accumulate over several reads before they are combined
 *   stats[FOSPHOR_AMD_VIEW_LINES]        launches over the live / max-hold vertices (in any of the forms above)
 * Host counters that only grow; nothing reads them but this call.  stats may be NULL. */
enum {
	FOSPHOR_AMD_VIEW_TILED, FOSPHOR_AMD_VIEW_TILED_LANES, FOSPHOR_AMD_VIEW_WIDE, FOSPHOR_AMD_VIEW_LINES,
	FOSPHOR_AMD_VIEW_STATS
};
int fosphor_amd_view_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_VIEW_STATS]);

/* ---- host only (no GPU needed) ---- */

/* The mapping rule above, in 64-bit integers: [*lo, *hi) of n_src for output index p of n_out.
 * 0, or -EINVAL (p outside [0, n_out), a size below 1, a NULL pointer). */
int fosphor_amd_view_span(int n_src, int n_out, int p, int *lo, int *hi);

/* Fill *v from the reference's zoom fields as gl.c:396-400 places the textured quad; all arithmetic in double from the float fields:
 *   first_bin   = clamp(floor(0.5 + N * (freq_center - freq_span / 2)), 0, N - 1)
 *   n_cols      = clamp(lrint(N * freq_span), 1, N - first_bin)
 *   wf_src_rows = clamp(lrint(wf_rows * wf_span), 1, wf_rows)
 * with the detector PEAK; width and wf_out_rows are copied.  The defaults (0.5, 1.0, 1.0) give the whole buffer.
 * -EINVAL: freq_span or wf_span outside ]0, 1], freq_center outside ]0, 1[, fft_len or wf_rows not positive, width outside
 * 1 .. 65536, wf_out_rows outside 1 .. wf_rows, a NULL pointer. */
int fosphor_amd_view_from_render(int fft_len, int wf_rows, const struct fosphor_render *r,
                                 int width, int wf_out_rows, struct fosphor_amd_view *v);

#ifdef __cplusplus
}
#endif

#endif
