/*
 * fosphor_amd_burst.h -- bursts in time and frequency: connected regions of the waterfall ring
 *
 * fosphor_amd_detect finds occupied bands in the averaged traces (frequency extent, no time); fosphor_amd_mask_scan finds the rows of
 * the ring that broke a limit line (time, no extent).  This pass gives each emission as one object: when it started, how long it
 * lasted, from which column to which, how strong it was and whether it is still on -- a pulse list, or SigMF-style annotations --
 * without the ring crossing to the host (fosphor_amd_detect.h says why it cannot).  Every cell of a time-frequency window is compared
 * with a threshold, short gaps along a row are closed as detect closes them, the runs of consecutive rows that overlap in column are
 * joined (union-find), and every connected component that is large enough leaves one record.
 *
 * Conventions, those of fosphor_amd_mask.h: the device entry point waits for pending fosphor_process work first (fosphor_amd_finish),
 * takes the ring and its position after that wait (the waterfall is one of two rings), runs on the instance's stream and returns when
 * its outputs are complete; it writes no state of the instance; -EINVAL is decided before anything is written; -EIO is a device error.
 * Columns are counted fft-shifted: shifted column i is memory column i ^ (N/2) of the waterfall.  Rows follow the view's time
 * convention: source index j = 0 is the newest row, ring row (waterfall_pos - 1 - j) mod wf_rows.  "y" is the waterfall's unit,
 * log10(|X|).  Rows never written since the instance was made hold the boot fill: they are scanned like any other row.
 * Because of the dead-store rule (a waterfall row that a later spectrum of the same call overwrites is never stored), the rows of one
 * multi-batch call are not consecutive spectra: a duration in rows means what the caller's call pattern makes it mean.
 */
#ifndef FOSPHOR_AMD_BURST_H
#define FOSPHOR_AMD_BURST_H

#include <stdint.h>

#include "fosphor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_BURST_MAX_RUNS   (1 << 20)
#define FOSPHOR_AMD_BURST_MAX_BURSTS 65536
#define FOSPHOR_AMD_BURST_MAX_ROWS   65536
#define FOSPHOR_AMD_BURST_MAX_GAP_ROWS 7

struct fosphor_amd_burst_cfg
{
	int   first_bin, n_cols;	/* window, shifted columns, as in the mask */
	int   rows;			/* newest rows scanned, 1 .. min(wf_rows, 65536) */
	float threshold_y;		/* used when d_threshold is NULL */
	int   max_gap_cols;		/* >= 0 */
	int   max_gap_rows;		/* 0 .. 7 */
	int   min_rows, min_cols;	/* >= 1: smallest row extent / column extent of a burst that is kept */
	int   max_runs;			/* 1 .. FOSPHOR_AMD_BURST_MAX_RUNS */
};

struct fosphor_amd_burst
{
	int32_t newest, oldest;		/* smallest / largest j of its cells */
	int32_t first_col, last_col;	/* bounding columns, shifted, absolute */
	int32_t n_cells;		/* cells of its runs, closed gaps included */
	int32_t peak_row, peak_col;	/* the (j, column) of the greatest y among those cells; NaN skipped; ties: smallest j, then smallest column */
	float   peak_y;
	float   energy_y;		/* 0.5 * log10(sum of the finite 10^(2 y) over those cells), fp64 sum: the power_y of detect / mask */
	uint32_t flags;			/* FOSPHOR_AMD_BURST_* below */
};

#define FOSPHOR_AMD_BURST_ON        1u	/* has a cell in row 0: still on */
#define FOSPHOR_AMD_BURST_CUT       2u	/* has a cell in row rows - 1: began before the window */
#define FOSPHOR_AMD_BURST_FIRST_COL 4u	/* touches the window's first column */
#define FOSPHOR_AMD_BURST_LAST_COL  8u	/* touches the window's last column */

struct fosphor_amd_burst_result
{
	int32_t n_runs, n_components, n_found, n_written, overflow;
};

/* Find the bursts of the newest cfg->rows rows.  cfg: HOST memory.  Everything else is DEVICE memory:
 *   d_threshold  float[N] indexed by shifted column (the whole array, so the same array serves any window), or NULL: then every
 *                column's threshold is cfg->threshold_y
 *   d_result     one struct, required
 *   d_bursts     [max_bursts], max_bursts = 1 .. 65536, required
 *
 * 1. On cells   cell (j, i) of the window is on when y > thr[i], plain IEEE float32: a NaN on either side is not on, equality is not
 *               on, +inf is on (against anything but +inf and NaN), -inf is not.
 * 2. Runs       gap closing is detect's rule, per row and within the window: a maximal run of not-on cells no longer than
 *               max_gap_cols with an on cell immediately on both sides is closed; one that touches a window edge never is.  A run is
 *               a maximal run of on-or-closed cells of one row.  Runs are numbered row-major: ascending j, then ascending column.
 *               n_runs is their exact number.
 * 3. Links      a run of row j and a run of row j + k, 1 <= k <= max_gap_rows + 1, are linked when their column intervals
 *               intersect (a1 <= b2 && a2 <= b1): 4-connectivity, no diagonal touch.  A component is a connected set of runs, its
 *               root its lowest run number; n_components counts them.
 * 4. Bursts     a burst is a component with oldest - newest + 1 >= min_rows and last_col - first_col + 1 >= min_cols.  Bursts come
 *               in ascending root order.  n_found counts them all, the first max_bursts are written; n_found > n_written is no
 *               error, and entries behind n_written are not written.
 * 5. Overflow   when n_runs > cfg->max_runs the call returns 0 with overflow = 1 and n_runs exact; the other three counts are 0 and
 *               d_bursts is untouched.  It means the threshold sits in the noise.
 * 6. Exactness  everything but energy_y is integer sums, minima, maxima and one total order on (y, j, column), so it is
 *               bit-identical however the work is split or ordered.  (-0 counts as +0 in that order, and peak_y reports +0.)
 *               A run always holds an on cell, so a burst always has a peak.  energy_y follows the mask's rule: a term is computed
 *               to float32 accuracy or better and the terms are summed in fp64 in the kernel's order; no finite positive term
 *               gives -inf.
 *
 * 0; -EINVAL (nothing is written): a window outside the buffer, rows outside 1 .. min(wf_rows, 65536), a negative gap,
 * max_gap_rows > 7, min_rows or min_cols below 1, max_runs or max_bursts out of range, a NULL self / cfg / d_result / d_bursts;
 * -EIO. */
int fosphor_amd_bursts(struct fosphor *self, const struct fosphor_amd_burst_cfg *cfg, const float *d_threshold,
                       struct fosphor_amd_burst_result *d_result, struct fosphor_amd_burst *d_bursts, int max_bursts);

/* HOST only, no GPU: rules 1 - 5 in plain C on host rows.  ys [rows][n], row 0 the newest, column 0 the window's first; thr_or_null
 * float[n] indexed like a row, or NULL for cfg->threshold_y.  cfg->rows and cfg->n_cols must equal rows and n; cfg->first_bin is added
 * to every column reported.  The energy is summed in double, row-major.  *res and out[0 .. n_written - 1] are written as the device
 * entry point writes them.
 * 0; -EINVAL: what the device entry point refuses (the buffer being 65536 columns), rows or n not matching cfg, a NULL ys. */
int fosphor_amd_bursts_host(const float *ys, int rows, int n, const float *thr_or_null, const struct fosphor_amd_burst_cfg *cfg,
                            struct fosphor_amd_burst_result *res, struct fosphor_amd_burst *out, int max_bursts);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.  The run kernel has one form (a work-group per
 * row and strip of FOSPHOR_AMD_BURST_STRIP columns); it is launched once to count and, unless the call ends there, once to write.
 *   stats[FOSPHOR_AMD_BURST_CALLS]      fosphor_amd_bursts calls that reached the device
 *   stats[FOSPHOR_AMD_BURST_OVERFLOWS]  of those, calls that ended with overflow = 1
 *   stats[FOSPHOR_AMD_BURST_K_COUNT]    launches of the run kernel that counts
 *   stats[FOSPHOR_AMD_BURST_K_ROWS]     launches of the kernel that joins the strips of a row
 *   stats[FOSPHOR_AMD_BURST_K_SCAN]     launches of the scan over the rows' run counts
 *   stats[FOSPHOR_AMD_BURST_K_INIT]     launches of the kernel that clears the run and component records
 *   stats[FOSPHOR_AMD_BURST_K_WRITE]    launches of the run kernel that writes the run records
 *   stats[FOSPHOR_AMD_BURST_K_LINK]     launches of the link kernel
 *   stats[FOSPHOR_AMD_BURST_K_REDUCE]   launches of the reduce kernel
 *   stats[FOSPHOR_AMD_BURST_K_EMIT]     launches of the emit kernel
 * A call without a run (n_runs = 0) and one that overflows stop after the scan. */
enum {
	FOSPHOR_AMD_BURST_CALLS, FOSPHOR_AMD_BURST_OVERFLOWS, FOSPHOR_AMD_BURST_K_COUNT, FOSPHOR_AMD_BURST_K_ROWS,
	FOSPHOR_AMD_BURST_K_SCAN, FOSPHOR_AMD_BURST_K_INIT, FOSPHOR_AMD_BURST_K_WRITE, FOSPHOR_AMD_BURST_K_LINK,
	FOSPHOR_AMD_BURST_K_REDUCE, FOSPHOR_AMD_BURST_K_EMIT,
	FOSPHOR_AMD_BURST_STATS
};
int fosphor_amd_burst_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_BURST_STATS]);

/* Columns of a strip, counted from (first column of the call & ~3): inside a strip a lane owns an aligned group of 4 columns, a wave
 * 256 columns and a work-group the strip.  Tests plant runs and gaps across those seams. */
#define FOSPHOR_AMD_BURST_STRIP 1024

#ifdef __cplusplus
}
#endif

#endif
