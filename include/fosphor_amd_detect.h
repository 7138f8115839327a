/*
 * fosphor_amd_detect.h -- emissions found on the device: percentile traces of the persistence histogram, a noise floor,
 *                         occupied bands and a marker on each band's peak
 *
 * A frame at fft_len_log = 16 is 65536 columns wide and the box that computes it is headless: nobody scans such a picture by eye,
 * and copying 128 MiB of histogram to the host every frame to search it there defeats the device-resident design.  These passes
 * read the instance's plain buffers (the persistence histogram, the live / max-hold vertices) and leave a few numbers per band
 * in device memory.
 *
 * Conventions, those of fosphor_amd_view.h: every device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided before anything is written; -EIO is a device error.  Columns are counted fft-shifted: shifted
 * column i is memory column i ^ (N/2) of the histogram and vertex i of the spectrum lines.  "y" is the unit of the traces and the
 * waterfall, log10(|X|).
 *
 * Valid where the histogram is complete on the device (single GPU, or after fosphor_amd_gather_state).
 */
#ifndef FOSPHOR_AMD_DETECT_H
#define FOSPHOR_AMD_DETECT_H

#include <stdint.h>

#include "fosphor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_DETECT_MAX_Q     4		/* percentiles per fosphor_amd_percentiles call */
#define FOSPHOR_AMD_DETECT_MAX_BANDS 65536

/* ---- percentile traces ---- */

/* Per-column percentiles of the persistence histogram.  q: HOST memory, n_q = 1 .. 4 values in ]0, 1] (a NaN is out of range).
 * d_y (float) and d_bin (int32): DEVICE memory, [n_q][N] in shifted column order; either may be NULL, not both.
 *
 * Per memory column x, all in float32, no contraction:
 *   c_b = c_(b-1) + histogram[b][x]   for b = 0 .. n_bins - 1 in that order, from c_(-1) = +0      (sequential prefix sum)
 *   T   = c_(n_bins-1)
 *   !(T > 0):   bin -1, y NaN                                                                     (an empty column)
 *   otherwise:  bin = the smallest b with c_b >= q[k] * T  (the product rounded once to float32),
 *               y   = the bin's entry of the table of fosphor_amd_detect_bin_y, bit for bit
 * The summation order is part of the contract: np.cumsum(h, axis=0, dtype=np.float32) reproduces every bin exactly.
 * Histogram cells are finite and non-negative by construction; other contents give unspecified bins but no fault.
 * 0; -EINVAL (nothing is written); -EIO. */
int fosphor_amd_percentiles(struct fosphor *self, const float *q, int n_q, float *d_y, int32_t *d_bin);

/* ---- noise floor, bands, markers ---- */

#define FOSPHOR_AMD_TRACE_LIVE    0
#define FOSPHOR_AMD_TRACE_MAXHOLD 1

#define FOSPHOR_AMD_FLOOR_ABSOLUTE   0		/* threshold_y is given */
#define FOSPHOR_AMD_FLOOR_PERCENTILE 1		/* threshold_y = floor_y + margin_y, the floor taken from the histogram */

struct fosphor_amd_detect_cfg
{
	int   trace;		/* FOSPHOR_AMD_TRACE_* */
	int   first_bin;	/* first fft-shifted column of the window, 0 .. N - 1 */
	int   n_cols;		/* shifted columns in the window, 1 .. N - first_bin */
	int   floor_mode;	/* FOSPHOR_AMD_FLOOR_* */
	float floor_q;		/* PERCENTILE: the percentile, ]0, 1] */
	float margin_y;		/* PERCENTILE: added to the floor */
	float threshold_y;	/* ABSOLUTE: the threshold */
	int   max_gap;		/* >= 0: longest run of columns below the threshold that is closed */
	int   min_cols;		/* >= 1: shortest band that is kept */
};

struct fosphor_amd_detect_result
{
	int32_t n_found;	/* bands found */
	int32_t n_written;	/* min(n_found, max_bands): entries of d_bands written */
	int32_t floor_bin;	/* PERCENTILE: the floor's histogram bin, -1 when every column of the window is empty; ABSOLUTE: -1 */
	float   floor_y;	/* that bin's y, NaN for bin -1 */
	float   threshold_y;	/* the threshold the mask used */
};

struct fosphor_amd_band
{
	int32_t first, last;	/* shifted columns, inclusive */
	int32_t peak_col;	/* the lowest column of [first, last] that attains the maximum trace y; NaN columns are skipped */
	float   peak_y;		/* the trace's y there, exactly */
	float   power_y;	/* 0.5 * log10(sum over [first, last] of 10^(2 y)): the integrated power in the traces' unit */
};

/* Find the bands of a trace.  cfg: HOST memory.  d_result (one struct) and d_bands ([max_bands], max_bands = 1 .. 65536): DEVICE
 * memory.
 *
 *   floor      PERCENTILE: take the floor_q bins of fosphor_amd_percentiles over the window's columns; of the m columns whose bin
 *              is >= 0, floor_bin is the lower median, element (m - 1) / 2 of the sorted bins (an integer selection, exact whatever
 *              the order); floor_y is its table entry and threshold_y = floor_y + margin_y in float32.  m = 0: floor_bin -1,
 *              floor_y and threshold_y NaN, no band.  One floor for the whole window, on purpose: a floor per column would
 *              swallow every persistent signal.
 *   mask       column i is above when trace_y[i] > threshold_y; a NaN column is not above
 *   gaps       a maximal run of not-above columns no longer than max_gap with an above column immediately on both sides, inside
 *              the window, counts as above; a run that touches an edge of the window is never closed
 *   bands      the maximal runs of above columns after closing that are at least min_cols long, in ascending column order.
 *              n_found counts them all; the first max_bands are written, so overflow shows and is no error
 *   per band   first, last, peak_col, peak_y as the struct says; power_y sums the finite terms 10^(2 y_i) of every column of the
 *              band, closed gaps included, in fp64 (no finite positive term: -inf)
 * fosphor_amd_detect_bands_host states the mask, gap and band rules in plain C.
 * 0; -EINVAL (an unknown trace or floor mode, a window outside the buffer, floor_q outside ]0, 1], max_gap < 0, min_cols < 1,
 * max_bands outside 1 .. 65536, a NULL pointer; nothing is written); -EIO. */
int fosphor_amd_detect(struct fosphor *self, const struct fosphor_amd_detect_cfg *cfg,
                       struct fosphor_amd_detect_result *d_result, struct fosphor_amd_band *d_bands, int max_bands);

/* Launches since the instance was made.  The kernels have one form each at every geometry (the percentile pass gives a lane one
 * column and sums its bins in order), so these count calls:
 *   stats[FOSPHOR_AMD_DETECT_PERCENTILES]  percentile launches: one per fosphor_amd_percentiles, one per PERCENTILE detect
 *   stats[FOSPHOR_AMD_DETECT_FLOOR]        floor selections (PERCENTILE detects)
 *   stats[FOSPHOR_AMD_DETECT_BANDS]        band passes (every detect)
 * Host counters that only grow; nothing reads them but this call.  stats may be NULL. */
enum {
	FOSPHOR_AMD_DETECT_PERCENTILES, FOSPHOR_AMD_DETECT_FLOOR, FOSPHOR_AMD_DETECT_BANDS,
	FOSPHOR_AMD_DETECT_STATS
};
int fosphor_amd_detect_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DETECT_STATS]);

/* Columns one lane of the band pass owns: ceil(n_cols / FOSPHOR_AMD_DETECT_LANES).  Its lanes meet at the multiples of that
 * chunk, counted from the window's first column; tests place bands across those seams. */
#define FOSPHOR_AMD_DETECT_LANES 1024

/* ---- host only (no GPU needed) ---- */

/* The y of each histogram bin: out[b] = (float)b / histo_scale - histo_offset in float32, b = 0 .. n_bins - 1.
 * 0, or -EINVAL (out NULL, n_bins < 1). */
int fosphor_amd_detect_bin_y(int n_bins, float histo_scale, float histo_offset, float *out);

/* The mask, gap and band rules above on a host trace of n columns (column 0 is the window's first: first, last and peak_col are
 * indices into trace_y).  Writes the first max_bands bands to out and the count of all of them to *n_found; power_y is computed in
 * double.  Returns the number written, or -EINVAL (a NULL pointer, n < 1, max_gap < 0, min_cols < 1, max_bands < 1). */
int fosphor_amd_detect_bands_host(const float *trace_y, int n, float threshold_y, int max_gap, int min_cols,
                                  struct fosphor_amd_band *out, int max_bands, int *n_found);

#ifdef __cplusplus
}
#endif

#endif
