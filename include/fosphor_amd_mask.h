/*
 * fosphor_amd_mask.h -- frequency-mask trigger and channel power over the waterfall ring
 *
 * The question a real-time spectrum analyser exists for is which spectra broke the limit line, and when.  The live trace is an
 * average and max-hold forgets time, so a burst of one spectrum shows in neither; the only per-spectrum record is the waterfall
 * ring, which is far too large to cross PCIe to be searched (fosphor_amd_detect.h).  This pass tests every stored spectrum of a time
 * window against an upper and a lower limit line on the device, leaves a small record per row and a compact list of the offending
 * rows, and integrates the power of up to FOSPHOR_MAX_CHANNELS column ranges per row from the same bytes (channel power versus
 * time, "zero span").
 *
 * Conventions, those of fosphor_amd_view.h / fosphor_amd_detect.h: every device entry point waits for pending fosphor_process work
 * first (fosphor_amd_finish), takes the ring and its position after that wait (the waterfall is one of two rings), runs on the
 * instance's stream and returns when its outputs are complete; it writes no state of the instance; -EINVAL is decided before anything
 * is written; -EIO is a device error.  Columns are counted fft-shifted: shifted column i is memory column i ^ (N/2) of the waterfall
 * and vertex i of the spectrum lines.  Rows follow the view's time convention: source index j = 0 is the newest row, ring row
 * (waterfall_pos - 1 - j) mod wf_rows.  "y" is the waterfall's unit, log10(|X|).
 *
 * Rows never written since the instance was made hold the boot fill, the noise floor -power.offset: they are scanned like any other
 * row, and whether they mean anything is the caller's business (scan no more rows than have been processed).
 */
#ifndef FOSPHOR_AMD_MASK_H
#define FOSPHOR_AMD_MASK_H

#include <stdint.h>

#include "fosphor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_MASK_MAX_EVENTS 65536
#define FOSPHOR_AMD_MASK_MAX_SPREAD 1024

struct fosphor_amd_mask_channel
{
	int32_t first, last;	/* shifted columns, inclusive, anywhere in 0 .. N - 1 */
};

struct fosphor_amd_mask_cfg
{
	int first_bin, n_cols;	/* the mask's window: shifted columns, as in fosphor_amd_view */
	int rows;		/* newest rows scanned, 1 .. wf_rows */
	int min_cols;		/* >= 1: a row triggers when n_over + n_under >= min_cols */
	int n_channels;		/* 0 .. FOSPHOR_MAX_CHANNELS */
	struct fosphor_amd_mask_channel channels[FOSPHOR_MAX_CHANNELS];
};

struct fosphor_amd_mask_row	/* one per scanned row, index j */
{
	int32_t n_over, n_under;	/* columns of the window with y > upper[i] / y < lower[i] */
	int32_t first_col, last_col;	/* lowest / highest violating shifted column; -1, -1 when none */
	int32_t peak_col;		/* lowest column attaining the greatest excess; -1 when n_over == 0 */
	float   peak_over;		/* that excess, y - upper[i], one float32 subtraction; NaN when n_over == 0 */
};

struct fosphor_amd_mask_result
{
	int32_t n_triggered;	/* rows that triggered */
	int32_t n_written;	/* min(n_triggered, max_events) entries of d_events written */
	int32_t newest, oldest;	/* smallest / largest triggered j; -1, -1 when none */
};

/* Scan the newest cfg->rows rows of the waterfall.  cfg: HOST memory.  Everything else is DEVICE memory:
 *   d_upper, d_lower  float[N] limit lines indexed by shifted column (the whole array, so the same array serves any window); either
 *                     or both may be NULL
 *   d_result          one struct, required
 *   d_rows            [cfg->rows] or NULL
 *   d_events          int32[max_events], max_events = 1 .. 65536; or NULL with max_events = 0
 *   d_power           float[n_channels][cfg->rows]; required when n_channels > 0, NULL otherwise
 *
 * Comparisons   all plain IEEE float32: column i of the window is over when y > upper[i] and under when y < lower[i].  A NaN y
 *               violates nothing; a NaN limit is violated by nothing; -inf (silence) is below any finite lower limit; y equal to a
 *               limit violates neither side; a NULL limit is never violated.  Only the window's columns are tested.
 * peak_over     the float32 y - upper[i] over the over columns: it can be +inf but never NaN (y > upper[i] excludes the cases that
 *               would make it so); ties go to the lowest column.
 * d_events      the triggered j in ascending order (newest first).  Overflow shows as n_triggered > n_written and is no error;
 *               entries beyond n_written are not written.
 * d_power       d_power[c][j] = (float)(0.5 * log10(sum)), sum adding in fp64 the finite terms 10^(2 y) of row j's columns
 *               channels[c].first .. last: the power_y of fosphor_amd_detect.  The order of the sum is the kernel's; a term is
 *               computed to float32 accuracy or better (relative error below 1e-6, which is 3e-7 in the result).  No finite positive
 *               term gives -inf.  Channels are independent of the mask window and of each other, and may overlap.
 * Both limits NULL: a pure channel-power pass; every row record is all-zero / -1 / NaN and nothing triggers.  With no channels
 * either the call is -EINVAL.
 * Everything but the power is exact and independent of how the work is split: integer sums, minima and maxima.
 *
 * 0; -EINVAL (nothing is written): a window outside the buffer, rows outside 1 .. wf_rows, min_cols < 1, n_channels outside
 * 0 .. FOSPHOR_MAX_CHANNELS, a channel with first > last or outside 0 .. N - 1, max_events outside its range or not matching
 * d_events, a NULL self / cfg / d_result, d_power not matching n_channels, nothing to do; -EIO. */
int fosphor_amd_mask_scan(struct fosphor *self, const struct fosphor_amd_mask_cfg *cfg,
                          const float *d_upper, const float *d_lower,
                          struct fosphor_amd_mask_result *d_result,
                          struct fosphor_amd_mask_row *d_rows,
                          int32_t *d_events, int max_events,
                          float *d_power);

/* ---- limit lines ---- */

/* DEVICE: out[i] = fmaxf over k in [max(0, i - spread), min(N - 1, i + spread)] of trace_y[k], plus margin_y, in float32 (NaN vertices
 * are skipped; all NaN -> NaN; +0 and -0 are not told apart).  trace: FOSPHOR_AMD_TRACE_* (fosphor_amd_detect.h); spread_cols
 * 0 .. 1024; d_out float[N] shifted.  "Learn the mask, then arm it": the result is a d_upper for fosphor_amd_mask_scan.
 * 0; -EINVAL (an unknown trace, spread_cols out of range, a NULL pointer; nothing is written); -EIO. */
int fosphor_amd_mask_from_trace(struct fosphor *self, int trace, float margin_y, int spread_cols, float *d_out);

/* HOST only: piecewise-linear limit line out[0 .. n - 1] through n_pts points (col[k] strictly ascending doubles in shifted-column
 * units, y[k]): left of the first point its y, right of the last its y, between two points
 * y0 + (y1 - y0) * ((i - c0) / (c1 - c0)) evaluated in double exactly as written and rounded once to float32 (a column on a point
 * belongs to the segment that starts there; the last point gives its own y).
 * 0; -EINVAL: n < 1, n_pts < 1, not ascending (a NaN column is not), a NULL pointer. */
int fosphor_amd_mask_from_points(int n, const double *col, const float *y, int n_pts, float *out);

/* HOST only: the row rule above on one host row of n columns (column 0 = the window's first): fills *out, indices relative to the
 * row.  upper / lower may be NULL.  0; -EINVAL: n < 1, a NULL row_y or out. */
int fosphor_amd_mask_row_host(const float *row_y, const float *upper, const float *lower, int n, struct fosphor_amd_mask_row *out);

/* Launches since the instance was made.  The scan kernel has two forms, chosen from the shape of the call alone, never from the data
 * (a call reads the aligned 4-column groups from (first column & ~3) on, in strips of FOSPHOR_AMD_MASK_STRIP columns):
 *   stats[FOSPHOR_AMD_MASK_SCANS]        fosphor_amd_mask_scan calls that reached the device
 *   stats[FOSPHOR_AMD_MASK_FROM_TRACE]   fosphor_amd_mask_from_trace launches
 *   stats[FOSPHOR_AMD_MASK_FORM_ROWS]    scan launches whose columns fit one strip: a work-group owns whole rows, several of them,
 *                                        and writes their records itself
 *   stats[FOSPHOR_AMD_MASK_FORM_SHARED]  scan launches over several strips: the work-groups that share a row leave partial records
 *                                        and a combine launch merges them
 * A call makes one scan launch, and a second one over the channels that do not lie inside the mask's window, if there are any.
 * Host counters that only grow; nothing reads them but this call.  stats may be NULL. */
enum {
	FOSPHOR_AMD_MASK_SCANS, FOSPHOR_AMD_MASK_FROM_TRACE, FOSPHOR_AMD_MASK_FORM_ROWS, FOSPHOR_AMD_MASK_FORM_SHARED,
	FOSPHOR_AMD_MASK_STATS
};
int fosphor_amd_mask_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_MASK_STATS]);

/* Columns of a strip.  Inside a strip a lane owns an aligned group of 4 columns, a wave 256 columns and a work-group the strip;
 * all counted from (first column of the call & ~3).  Tests plant violations on both sides of those seams. */
#define FOSPHOR_AMD_MASK_STRIP 1024

#ifdef __cplusplus
}
#endif

#endif
