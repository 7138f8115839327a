/*
 * fosphor_pass.h -- what every pass in a file of its own shares with the instance and with the others: the slots of the instance's
 * scratch buffers and counters, the private accessors (fosphor_api.cpp), and the checked launch and the drain that end a call.
 * fosphor_ring.h (passes over the plain buffers) and fosphor_jobs.h (passes over burst IQ) build on it.
 */
#ifndef FOSPHOR_PASS_H
#define FOSPHOR_PASS_H

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/fosphor_amd.h"

/* the instance's scratch buffers that only grow, one per user (fosphor_burst.hip has two: by rows and strips, by runs); detect's and
 * mask's are of a size that is fixed for the life of an instance, so theirs are allocated once, on first use */
enum {
	FOSPHOR_SCRATCH_DETECT,
	FOSPHOR_SCRATCH_MASK,
	FOSPHOR_SCRATCH_BURST_ROWS,
	FOSPHOR_SCRATCH_BURST_RUNS,
	FOSPHOR_SCRATCH_EXTRACT,
	FOSPHOR_SCRATCH_MEASURE,
	FOSPHOR_SCRATCH_DEMOD,
	FOSPHOR_SCRATCH_CORRELATE,
	FOSPHOR_SCRATCH_RESAMPLE,
	FOSPHOR_SCRATCH_PSD,
	FOSPHOR_SCRATCH_SYMBOLS,
	FOSPHOR_SCRATCH_CARRIER,
	FOSPHOR_SCRATCH_DECIDE,
	FOSPHOR_SCRATCH_DECODE,
	FOSPHOR_SCRATCH_SOFT,
	FOSPHOR_SCRATCH_RS,
	FOSPHOR_SCRATCH_COUNT
};

/* the instance's host counters that only grow, one row per pass: what its public fosphor_amd_*_stats copies out */
enum {
	FOSPHOR_COUNTERS_VIEW,
	FOSPHOR_COUNTERS_DETECT,
	FOSPHOR_COUNTERS_MASK,
	FOSPHOR_COUNTERS_BURST,
	FOSPHOR_COUNTERS_EXTRACT,
	FOSPHOR_COUNTERS_MEASURE,
	FOSPHOR_COUNTERS_DEMOD,
	FOSPHOR_COUNTERS_CORRELATE,
	FOSPHOR_COUNTERS_RESAMPLE,
	FOSPHOR_COUNTERS_PSD,
	FOSPHOR_COUNTERS_SYMBOLS,
	FOSPHOR_COUNTERS_CARRIER,
	FOSPHOR_COUNTERS_DECIDE,
	FOSPHOR_COUNTERS_DECODE,
	FOSPHOR_COUNTERS_SOFT,
	FOSPHOR_COUNTERS_RS,
	FOSPHOR_COUNTERS_COUNT
};
#define FOSPHOR_COUNTERS_MAX 10		/* counters of one pass at most (FOSPHOR_AMD_BURST_STATS) */

/* implemented in fosphor_api.cpp, on struct fosphor (fosphor_instance.h, which no pass includes): scratch buffer `which`, at least `bytes` long -- its user has drained the
 * stream of every launch that used the old one before it asks for more; the counters of pass `which`; the copy behind every public
 * fosphor_amd_*_stats (n <= FOSPHOR_COUNTERS_MAX); and what fosphor_cmap.hip needs of the instance */
extern "C" int fosphor_amd_priv_scratch(struct fosphor *self, int which, size_t bytes, void **d_scratch);
extern "C" long long *fosphor_amd_priv_counters(struct fosphor *self, int which);
extern "C" int fosphor_amd_priv_copy_stats(struct fosphor *self, int which, int n, long long *stats);
extern "C" int fosphor_amd_priv_palette(struct fosphor *self, int n, uint32_t **d_palette);
extern "C" void fosphor_amd_priv_power(struct fosphor *self, float *scale, float *offset);

namespace pass {

inline int launch_ok(void) { return hipGetLastError() == hipSuccess ? 0 : -EIO; }

/* launch_ok(), counted in stats[counter] if the launch went */
inline int launch_counted(long long *stats, int counter)
{
	const int rv = launch_ok();
	if (!rv)
		stats[counter]++;
	return rv;
}

/* one launch of `groups` work-groups of kThreads lanes, checked, and counted in stats[counter] if it went */
template <int kThreads, class P>
int launch(void (*kernel)(const P), unsigned groups, hipStream_t st, const P &p, long long *stats, int counter)
{
	hipLaunchKernelGGL(kernel, dim3(groups), dim3(kThreads), 0, st, p);
	return launch_counted(stats, counter);
}

/* the end of a call: rv of its launches once the stream is empty */
inline int drain(hipStream_t st, int rv) { return hipStreamSynchronize(st) != hipSuccess ? -EIO : rv; }

} // namespace pass

#endif
