/*
 * fosphor_ring.h -- the ring-pass substrate of the read-only passes over the instance's plain buffers (fosphor_cmap.hip,
 * fosphor_view.hip, fosphor_detect.hip, fosphor_mask.hip, fosphor_burst.hip); DESIGN.md, "the ring-pass substrate"
 *
 * A pass waits for the compute side, takes the buffers, refuses a geometry or a window it cannot read, and reads a window
 * [c0, c1) of fft-shifted columns of the newest rows of the waterfall ring (or of the histogram, or of a trace).  A pass supplies its
 * parameter struct, its kernels, its forms and counters and the checks of its own arguments, in its own order.  It gets from here:
 *   device  the strip read of the ring: the columns of a call are cut, from (c0 & ~3) on, into strips of kStrip = 1024; lane t of a
 *           strip's 256 owns the aligned group of 4 shifted columns at strip + 4t, which is an aligned, contiguous group of memory
 *           columns on either side of the N/2 wrap (N/2 is a multiple of 4): one 16-byte load; a group that the window cuts (its
 *           head and tail) loads its columns one by one, so no byte outside the window is read.  group_of(), mem_col() and
 *           ring_row() are here and k_burst_runs uses them.  The bitmask `in` of a lane's columns inside the window and the load it
 *           steers stay written out in k_mask_scan and k_burst_runs: as helpers (by value, by reference, four scalars) they changed
 *           the register allocation of k_mask_scan (82 VGPRs for 80, occupancy 5 for 6) and of k_burst_runs<true>, which then
 *           waited for the load at once.  k_mask_scan keeps the three address expressions too: through the helpers its listing
 *           moved (the same resources, 13 vector instructions more);
 *           power_term(); the lane of a ballot's lowest / highest bit and the 64-bit shuffles; the inclusive scan of one work-group
 *           through LDS and the split of n items into one chunk per lane;
 *   host    open() (the wait and the buffers), geometry_ok(), window_ok(), strips_of(), the (base, mask) of the rows of the
 *           waterfall and of the histogram, and from fosphor_pass.h the checked launch and the drain.
 */
#ifndef FOSPHOR_RING_H
#define FOSPHOR_RING_H

#include <math.h>

#include "fosphor_pass.h"
#include "../../include/fosphor_amd_burst.h"
#include "../../include/fosphor_amd_mask.h"

namespace ring_pass {

constexpr int kMaxCols = 65536;
constexpr int kStrip = FOSPHOR_AMD_MASK_STRIP;		/* columns of a strip: one 16-byte load for each of 256 lanes */
constexpr int kMaxStrips = kMaxCols / kStrip;		/* 64: a pass that merges the strips of a row gives a strip a lane of one wave */

static_assert(FOSPHOR_AMD_MASK_STRIP == FOSPHOR_AMD_BURST_STRIP, "mask and burst cut a window into the same strips");
static_assert(kMaxStrips == 64, "one lane per strip");

/* ---- device: the strip read ---- */

/* the first of the 4 shifted columns of lane t of a strip of the window that begins at c0 */
__device__ __forceinline__ int group_of(int c0, int strip, int t) { return (c0 & ~3) + strip * kStrip + 4 * t; }

/* the memory column of shifted column s of n, and the ring row of source row j (0 = the newest) */
__device__ __forceinline__ int mem_col(int s, int n) { return (s ^ (n >> 1)) & (n - 1); }
__device__ __forceinline__ int ring_row(int row_base, int row_mask, int j) { return (row_base - j) & row_mask; }

/* 10^(2 y) as a sum of powers takes it: 0 for a term that is not finite.  The float32 path covers every y a spectrum produces;
 * what it cannot represent (or a NaN) takes the fp64 path, which decides what is finite as fosphor_amd_detect does. */
__device__ __forceinline__ double power_term(float y)
{
	const float t = exp10f(2.0f * y);
	if (t > 1e-30f && t < 1e30f)
		return (double)t;
	const double d = exp10(2.0 * (double)y);
	return isfinite(d) ? d : 0.0;
}

/* ---- device: lanes ---- */

__device__ __forceinline__ int low_lane(unsigned long long m) { return __ffsll(m) - 1; }		/* m != 0 */
__device__ __forceinline__ int top_lane(unsigned long long m) { return 63 - __clzll((long long)m); }	/* m != 0 */

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int d)
{
	const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d);
	const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
	return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d)
{
	const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d);
	const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
	return ((unsigned long long)hi << 32) | lo;
}

/* ---- device: one work-group of kLanes lanes over n items ---- */

struct OpMax { template <class T> __device__ T operator()(T a, T b) const { return max(a, b); } };
struct OpMin { template <class T> __device__ T operator()(T a, T b) const { return min(a, b); } };
struct OpAdd { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };

/* Inclusive scan of one value per lane over the work-group's kLanes lanes, left in s[]; pos is the position of this lane's value
 * (its lane, or kLanes - 1 - lane for a scan from above).  Begins and ends with a barrier. */
template <int kLanes, class T, class Op>
__device__ __forceinline__ void block_scan(T *s, int pos, T v, Op op)
{
	s[pos] = v;
	__syncthreads();
	for (int d = 1; d < kLanes; d <<= 1) {
		T w = s[pos];
		if (pos >= d)
			w = op(s[pos - d], w);
		__syncthreads();
		s[pos] = w;
		__syncthreads();
	}
}

/* lane t owns the items [g0, g1) of n: chunks of ceil(n / kLanes), the last ones short or empty */
template <int kLanes>
__device__ __forceinline__ void chunk_of(int n, int t, int &g0, int &g1)
{
	const int chunk = (n + kLanes - 1) / kLanes;
	g0 = min(t * chunk, n);
	g1 = min(g0 + chunk, n);
}

/* ---- host ---- */

/* what every pass does first: the wait for the compute side, then the buffers (after the wait: the waterfall is one of two rings) */
inline int open(struct fosphor *self, struct fosphor_amd_buffers *b)
{
	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	return fosphor_amd_get_buffers_nohc(self, b) ? -EIO : 0;
}

inline bool pow2(int v) { return v >= 1 && !(v & (v - 1)); }

/* what the aligned groups and the ring mask rely on; min_n: 8 for a pass that reads by strips, 4 for the others */
inline bool geometry_ok(const struct fosphor_amd_buffers &b, int min_n)
{
	return b.fft_len >= min_n && b.fft_len <= kMaxCols && pow2(b.fft_len) && pow2(b.wf_rows);
}

/* the shifted columns [first_bin, first_bin + n_cols) inside [0, n) */
inline bool window_ok(int first_bin, int n_cols, int n)
{
	return first_bin >= 0 && first_bin < n && n_cols >= 1 && n_cols <= n - first_bin;
}

/* the strips of the window [c0, c1) */
inline int strips_of(int c0, int c1) { return (c1 - (c0 & ~3) + kStrip - 1) / kStrip; }

/* memory row of source row j: (base - j) & mask.  The waterfall's newest row is j = 0; the base is kept non-negative before the mask.
 * The histogram is no ring: row j is bin n_bins - 1 - j. */
struct Rows {
	int base, mask;
};

inline Rows waterfall_rows(const struct fosphor_amd_buffers &b) { return Rows{ b.waterfall_pos - 1 + b.wf_rows, b.wf_rows - 1 }; }
inline Rows histogram_rows(const struct fosphor_amd_buffers &b) { return Rows{ b.n_bins - 1, 0x7fffffff }; }

using pass::launch_ok;
using pass::launch_counted;
using pass::launch;
using pass::drain;

} // namespace ring_pass

#endif
