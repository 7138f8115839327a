/*
 * fosphor_detect.hip -- percentile traces of the persistence histogram, noise floor, bands and markers (include/fosphor_amd_detect.h)
 *
 * Read-only passes over the instance's plain buffers, in a file of their own: nothing here is on the process / merge path.
 *
 *   k_percentiles  the hot pass.  The contract fixes the order of a column's sum (c_b = c_(b-1) + h_b), so a column's bins cannot be
 *                  split over lanes.  A lane owns one column and the 64 lanes of a wave own 64 adjacent ones: every load is a
 *                  coalesced 256-byte row segment, the loads do not depend on the sum and are issued kPctRows rows ahead of it, and
 *                  65536 columns make 1024 waves, one for every SIMD of the chip (a wider load per lane would leave SIMDs idle and
 *                  win nothing: with one wave per SIMD the bytes in flight are what fills the memory system, and
 *                  1024 waves x 32 rows x 256 B = 8 MiB is about bandwidth x latency).  Two reads: the first gives T, the second
 *                  repeats the same sum (bit for bit the same c_b) and notes where it crosses q * T; a wave leaves the second read
 *                  once all its columns have crossed.  One form at every geometry.
 *   k_floor        one work-group: counts the window's columns per floor bin in LDS (integer atomics: exact in any order) and walks
 *                  the counts to the lower median
 *   k_bands        one work-group of 1024 lanes over at most 65536 columns, which is not the hot path.  Lane t owns the chunk
 *                  [t * chunk, (t + 1) * chunk) of the window, chunk = ceil(n_cols / 1024) <= 64, so a chunk's mask is the bits of
 *                  one 64-bit word.  What a chunk needs from the others is the nearest above column and the nearest column outside
 *                  a band on either side of it: four scans over the lanes.  A band belongs to the lane that owns its last column;
 *                  a sum scan numbers the bands.  Then each wave takes whole bands and reduces their columns (peak, fp64 power)
 *                  with coalesced loads and shuffles.
 * No global atomics.
 */
#include <errno.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "fosphor_ring.h"
#include "../../include/fosphor_amd_detect.h"

namespace {

using namespace ring_pass;		/* kMaxCols, the lanes' helpers, block_scan and chunk_of, the host side of a call */

constexpr int kMaxBins = 512;		/* fosphor_amd_init admits no more */
constexpr int kPctLanes = 64;		/* one wave per work-group: 1024 work-groups at 65536 columns spread over every SIMD */
constexpr int kPctRows = 32;		/* rows loaded ahead of the sum */
constexpr int kLanes = FOSPHOR_AMD_DETECT_LANES;
static_assert(FOSPHOR_AMD_DETECT_STATS <= FOSPHOR_COUNTERS_MAX, "the instance holds the counters");
constexpr size_t kScratchBytes = sizeof(int32_t) * kMaxCols + sizeof(float) * kMaxBins;	/* floor bins [N], y table [n_bins] */

struct PctParams {
	const float *hist;		/* [n_bins][n], unshifted columns */
	const float *ytab;		/* [n_bins], read when d_y is set */
	float       *d_y;		/* [NQ][n] shifted, or NULL */
	int32_t     *d_bin;		/* [NQ][n] shifted, or NULL */
	int   n, n_bins;
	int   c0, c1;			/* shifted columns [c0, c1) */
	float q[FOSPHOR_AMD_DETECT_MAX_Q];
};

template <int NQ>
__global__ __launch_bounds__(kPctLanes)
void k_percentiles(const PctParams p)
{
	const int i = p.c0 + blockIdx.x * kPctLanes + threadIdx.x;
	if (i >= p.c1)
		return;
	const size_t n = p.n;
	const float *col = p.hist + (i ^ (p.n >> 1));
	const int full = p.n_bins - p.n_bins % kPctRows;

	/* first read: T */
	float c = 0.0f;
	for (int b0 = 0; b0 < full; b0 += kPctRows) {
		float v[kPctRows];
#pragma unroll
		for (int u = 0; u < kPctRows; u++)
			v[u] = col[(size_t)(b0 + u) * n];
#pragma unroll
		for (int u = 0; u < kPctRows; u++)
			c = c + v[u];
	}
	for (int b = full; b < p.n_bins; b++)
		c = c + col[(size_t)b * n];
	const float T = c;
	const bool some = T > 0.0f;

	/* second read: the same sum, and where it crosses.  An empty column compares against NaN and crosses nowhere. */
	float thr[NQ];
	int bin[NQ];
#pragma unroll
	for (int k = 0; k < NQ; k++) {
		thr[k] = some ? p.q[k] * T : __builtin_nanf("");
		bin[k] = -1;
	}
	bool open = some;
	c = 0.0f;
	int b0 = 0;
	for (; b0 < full && __any(open); b0 += kPctRows) {
		float v[kPctRows];
#pragma unroll
		for (int u = 0; u < kPctRows; u++)
			v[u] = col[(size_t)(b0 + u) * n];
#pragma unroll
		for (int u = 0; u < kPctRows; u++) {
			c = c + v[u];
#pragma unroll
			for (int k = 0; k < NQ; k++)
				bin[k] = (bin[k] < 0 && c >= thr[k]) ? b0 + u : bin[k];
		}
		open = false;
#pragma unroll
		for (int k = 0; k < NQ; k++)
			open = open || bin[k] < 0;
		open = open && some;
	}
	if (b0 == full)
		for (int b = full; b < p.n_bins; b++) {
			c = c + col[(size_t)b * n];
#pragma unroll
			for (int k = 0; k < NQ; k++)
				bin[k] = (bin[k] < 0 && c >= thr[k]) ? b : bin[k];
		}

#pragma unroll
	for (int k = 0; k < NQ; k++) {
		if (p.d_bin)
			p.d_bin[(size_t)k * n + i] = bin[k];
		if (p.d_y)
			p.d_y[(size_t)k * n + i] = bin[k] >= 0 ? p.ytab[bin[k]] : __builtin_nanf("");
	}
}

int launch_percentiles(struct fosphor *self, hipStream_t st, const PctParams &p, int n_q)
{
	const dim3 grid((p.c1 - p.c0 + kPctLanes - 1) / kPctLanes), block(kPctLanes);
	switch (n_q) {
	case 1: hipLaunchKernelGGL(k_percentiles<1>, grid, block, 0, st, p); break;
	case 2: hipLaunchKernelGGL(k_percentiles<2>, grid, block, 0, st, p); break;
	case 3: hipLaunchKernelGGL(k_percentiles<3>, grid, block, 0, st, p); break;
	default: hipLaunchKernelGGL(k_percentiles<4>, grid, block, 0, st, p); break;
	}
	return launch_counted(fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_DETECT), FOSPHOR_AMD_DETECT_PERCENTILES);
}

/* The lower median of the window's floor bins: element (m - 1) / 2 of the m bins that are >= 0, sorted. */
__global__ __launch_bounds__(kLanes)
void k_floor(const int32_t *bins, int first_bin, int n_cols, int n_bins, const float *ytab, float margin_y,
             struct fosphor_amd_detect_result *res)
{
	__shared__ int cnt[kMaxBins];
	const int t = threadIdx.x;

	if (t < kMaxBins)
		cnt[t] = 0;
	__syncthreads();
	for (int i = t; i < n_cols; i += kLanes) {
		const int b = bins[first_bin + i];
		if (b >= 0 && b < n_bins)
			atomicAdd(&cnt[b], 1);
	}
	__syncthreads();
	if (t == 0) {
		int m = 0;
		for (int b = 0; b < n_bins; b++)
			m += cnt[b];
		int fb = -1;
		if (m > 0) {
			const int rank = (m - 1) / 2;
			int seen = 0;
			for (fb = 0; fb < n_bins - 1; fb++) {
				seen += cnt[fb];
				if (seen > rank)
					break;
			}
		}
		const float fy = fb >= 0 ? ytab[fb] : __builtin_nanf("");
		res->floor_bin = fb;
		res->floor_y = fy;
		res->threshold_y = fy + margin_y;
	}
}

struct BandParams {
	const float *trace;		/* float2[n] vertices of the trace, shifted order */
	struct fosphor_amd_detect_result *res;
	struct fosphor_amd_band *bands;
	int   first_bin, n_cols;
	int   max_gap, min_cols, max_bands;
	int   absolute;			/* threshold below; else res->threshold_y, which k_floor wrote */
	float threshold_y;
};

/* op over the values of the lanes below this one (ident for lane 0) */
template <typename Op>
__device__ int scan_below(int *s, int v, int ident, Op op)
{
	const int t = threadIdx.x;
	block_scan<kLanes>(s, t, v, op);
	const int r = t ? s[t - 1] : ident;
	__syncthreads();
	return r;
}

/* op over the values of the lanes above this one (ident for the last lane) */
template <typename Op>
__device__ int scan_above(int *s, int v, int ident, Op op)
{
	const int pos = kLanes - 1 - threadIdx.x;
	block_scan<kLanes>(s, pos, v, op);
	const int r = pos ? s[pos - 1] : ident;
	__syncthreads();
	return r;
}

__global__ __launch_bounds__(kLanes)
void k_bands(const BandParams p)
{
	__shared__ int s[kLanes];
	const int t = threadIdx.x, n = p.n_cols;
	const int chunk = (n + kLanes - 1) / kLanes;			/* 1 .. 64; chunk_of() with g1 - g0 for len moved this kernel's listing */
	const int g0 = min(t * chunk, n), len = min(chunk, n - g0);	/* this lane's window columns [g0, g0 + len); len may be 0 */
	const float *y = p.trace + 2 * (size_t)p.first_bin + 1;	/* y of window column i: y[2 * i] */
	const float thr = p.absolute ? p.threshold_y : p.res->threshold_y;
	const uint64_t valid = len == 64 ? ~0ull : (1ull << len) - 1;

	/* the mask: bit j = column g0 + j is above (false for NaN on either side) */
	uint64_t ab = 0;
	for (int j = 0; j < len; j++)
		if (y[2 * (size_t)(g0 + j)] > thr)
			ab |= 1ull << j;

	/* gap closing: the nearest above column on each side of a not-above one, inside the window or none (-1 / n) */
	const int left_above  = scan_below(s, ab ? g0 + top_lane(ab) : -1, -1, OpMax());
	const int right_above = scan_above(s, ab ? g0 + low_lane(ab) : n, n, OpMin());
	uint64_t m = ab;
	int prev = left_above;
	for (int j = 0; j < len; j++) {
		if ((ab >> j) & 1) {
			prev = g0 + j;
			continue;
		}
		const uint64_t rest = j < 63 ? ab >> (j + 1) : 0;
		const int next = rest ? g0 + j + 1 + low_lane(rest) : right_above;
		if (prev >= 0 && next < n && next - prev - 1 <= p.max_gap)
			m |= 1ull << j;
	}

	/* runs of m: the nearest column outside a run on each side of this chunk (-1 / n: the window's edge) */
	const uint64_t z = ~m & valid;
	const int left_out  = scan_below(s, z ? g0 + top_lane(z) : -1, -1, OpMax());
	const int right_out = scan_above(s, z ? g0 + low_lane(z) : n, n, OpMin());
	/* a run ends at bit j when bit j + 1 is clear; the column after the chunk is in a run unless it is right_out (or the edge) */
	uint64_t ends = 0;
	if (len) {
		const uint64_t after = right_out != g0 + len ? 1ull << (len - 1) : 0;
		ends = m & ~((m >> 1) | after);
	}

	/* the bands that end in this chunk, and their numbers */
	int mine = 0;
	for (uint64_t e = ends; e; e &= e - 1) {
		const int j = low_lane(e);
		const uint64_t zb = z & ((1ull << j) - 1);
		const int start = zb ? g0 + top_lane(zb) + 1 : left_out + 1;
		mine += g0 + j - start + 1 >= p.min_cols;
	}
	block_scan<kLanes>(s, t, mine, OpAdd());
	int k = t ? s[t - 1] : 0;
	const int n_found = s[kLanes - 1];
	const int n_written = min(n_found, p.max_bands);
	for (uint64_t e = ends; e; e &= e - 1) {
		const int j = low_lane(e);
		const uint64_t zb = z & ((1ull << j) - 1);
		const int start = zb ? g0 + top_lane(zb) + 1 : left_out + 1;
		if (g0 + j - start + 1 < p.min_cols)
			continue;
		if (k < p.max_bands) {
			p.bands[k].first = p.first_bin + start;
			p.bands[k].last = p.first_bin + g0 + j;
		}
		k++;
	}
	if (t == 0) {
		p.res->n_found = n_found;
		p.res->n_written = n_written;
		if (p.absolute) {
			p.res->floor_bin = -1;
			p.res->floor_y = __builtin_nanf("");
			p.res->threshold_y = p.threshold_y;
		}
	}
	__syncthreads();					/* the bands' first / last are visible to the work-group */

	/* per band: a wave reduces its columns */
	const int lane = t & 63;
	for (int b = t >> 6; b < n_written; b += kLanes / 64) {
		const int first = p.bands[b].first - p.first_bin, last = p.bands[b].last - p.first_bin;
		float best = 0.0f;
		int best_col = -1;
		double sum = 0.0;
		for (int i = first + lane; i <= last; i += 64) {
			const float v = y[2 * (size_t)i];
			if (v != v)
				continue;
			if (best_col < 0 || v > best) {		/* ascending i: the lowest column of equal maxima stays */
				best = v;
				best_col = i;
			}
			const double term = exp10(2.0 * (double)v);
			if (isfinite(term))
				sum += term;
		}
		for (int d = 32; d; d >>= 1) {
			const float ov = __shfl_xor(best, d);
			const int oc = __shfl_xor(best_col, d);
			sum += __shfl_xor(sum, d);
			if (oc >= 0 && (best_col < 0 || ov > best || (ov == best && oc < best_col))) {
				best = ov;
				best_col = oc;
			}
		}
		if (lane == 0) {
			p.bands[b].peak_col = p.first_bin + best_col;
			p.bands[b].peak_y = best;
			p.bands[b].power_y = (float)(0.5 * log10(sum));
		}
	}
}

bool q_ok(float q)
{
	return q > 0.0f && q <= 1.0f;		/* false for NaN */
}

void bin_y(int n_bins, float histo_scale, float histo_offset, float *out)
{
	for (int b = 0; b < n_bins; b++) {
		const float c = (float)b / histo_scale;	/* rounded before the subtraction, whatever the contraction setting */
		out[b] = c - histo_offset;
	}
}

/* what both device entry points do first: the wait, the buffers, the scratch.  0 / -EINVAL / -EIO */
int prepare(struct fosphor *self, struct fosphor_amd_buffers *b, int32_t **d_bins, float **d_ytab)
{
	void *d;
	if (open(self, b))
		return -EIO;
	if (!geometry_ok(*b, 4) || b->n_bins < 1 || b->n_bins > kMaxBins)
		return -EINVAL;
	if (fosphor_amd_priv_scratch(self, FOSPHOR_SCRATCH_DETECT, kScratchBytes, &d))
		return -EIO;
	*d_bins = (int32_t *)d;
	*d_ytab = (float *)((int32_t *)d + kMaxCols);
	return 0;
}

} // namespace

extern "C" int fosphor_amd_detect_bin_y(int n_bins, float histo_scale, float histo_offset, float *out)
{
	if (!out || n_bins < 1)
		return -EINVAL;
	bin_y(n_bins, histo_scale, histo_offset, out);
	return 0;
}

extern "C" int fosphor_amd_detect_bands_host(const float *trace_y, int n, float threshold_y, int max_gap, int min_cols,
                                             struct fosphor_amd_band *out, int max_bands, int *n_found)
{
	if (!trace_y || !out || !n_found || n < 1 || max_gap < 0 || min_cols < 1 || max_bands < 1)
		return -EINVAL;
	std::vector<char> m(n);
	for (int i = 0; i < n; i++)
		m[i] = trace_y[i] > threshold_y;
	/* close the runs of not-above columns that have an above column on both sides and are no longer than max_gap */
	for (int i = 0; i < n;) {
		if (m[i]) {
			i++;
			continue;
		}
		int e = i;
		while (e < n && !(trace_y[e] > threshold_y))
			e++;
		if (i > 0 && e < n && e - i <= max_gap)
			for (int j = i; j < e; j++)
				m[j] = 1;
		i = e;
	}
	int found = 0, written = 0;
	for (int i = 0; i < n;) {
		if (!m[i]) {
			i++;
			continue;
		}
		int e = i;
		while (e < n && m[e])
			e++;
		if (e - i >= min_cols) {
			if (found < max_bands) {
				struct fosphor_amd_band *b = &out[written++];
				double sum = 0.0;
				b->first = i;
				b->last = e - 1;
				b->peak_col = -1;
				b->peak_y = 0.0f;
				for (int j = i; j < e; j++) {
					const float v = trace_y[j];
					if (v != v)
						continue;
					if (b->peak_col < 0 || v > b->peak_y) {
						b->peak_col = j;
						b->peak_y = v;
					}
					const double term = pow(10.0, 2.0 * (double)v);
					if (isfinite(term))
						sum += term;
				}
				b->power_y = (float)(0.5 * log10(sum));
			}
			found++;
		}
		i = e;
	}
	*n_found = found;
	return written;
}

extern "C" int fosphor_amd_detect_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DETECT_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_DETECT, FOSPHOR_AMD_DETECT_STATS, stats);
}

extern "C" int fosphor_amd_percentiles(struct fosphor *self, const float *q, int n_q, float *d_y, int32_t *d_bin)
{
	struct fosphor_amd_buffers b;
	PctParams p;
	int32_t *d_bins;
	float *d_ytab;
	int rv;

	if (!self || !q || n_q < 1 || n_q > FOSPHOR_AMD_DETECT_MAX_Q || (!d_y && !d_bin))
		return -EINVAL;
	for (int k = 0; k < n_q; k++)
		if (!q_ok(q[k]))
			return -EINVAL;
	if ((rv = prepare(self, &b, &d_bins, &d_ytab)))
		return rv;
	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);

	std::vector<float> ytab(b.n_bins);		/* lives until the stream has been waited for */
	if (d_y) {
		bin_y(b.n_bins, b.histo_scale, b.histo_offset, ytab.data());
		if (hipMemcpyAsync(d_ytab, ytab.data(), sizeof(float) * b.n_bins, hipMemcpyHostToDevice, st) != hipSuccess) {
			(void)hipStreamSynchronize(st);
			return -EIO;
		}
	}
	p.hist = b.d_histogram; p.ytab = d_ytab; p.d_y = d_y; p.d_bin = d_bin;
	p.n = b.fft_len; p.n_bins = b.n_bins; p.c0 = 0; p.c1 = b.fft_len;
	for (int k = 0; k < FOSPHOR_AMD_DETECT_MAX_Q; k++)
		p.q[k] = k < n_q ? q[k] : 1.0f;
	return drain(st, launch_percentiles(self, st, p, n_q));
}

extern "C" int fosphor_amd_detect(struct fosphor *self, const struct fosphor_amd_detect_cfg *cfg,
                                  struct fosphor_amd_detect_result *d_result, struct fosphor_amd_band *d_bands, int max_bands)
{
	struct fosphor_amd_buffers b;
	int32_t *d_bins;
	float *d_ytab;
	int rv;

	if (!self || !cfg || !d_result || !d_bands || max_bands < 1 || max_bands > FOSPHOR_AMD_DETECT_MAX_BANDS)
		return -EINVAL;
	if (cfg->trace != FOSPHOR_AMD_TRACE_LIVE && cfg->trace != FOSPHOR_AMD_TRACE_MAXHOLD)
		return -EINVAL;
	if (cfg->floor_mode != FOSPHOR_AMD_FLOOR_ABSOLUTE && cfg->floor_mode != FOSPHOR_AMD_FLOOR_PERCENTILE)
		return -EINVAL;
	const bool pct = cfg->floor_mode == FOSPHOR_AMD_FLOOR_PERCENTILE;
	if ((pct && !q_ok(cfg->floor_q)) || cfg->max_gap < 0 || cfg->min_cols < 1)
		return -EINVAL;
	if ((rv = prepare(self, &b, &d_bins, &d_ytab)))
		return rv;
	if (!window_ok(cfg->first_bin, cfg->n_cols, b.fft_len))
		return -EINVAL;
	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_DETECT);

	std::vector<float> ytab(b.n_bins);		/* lives until the stream has been waited for */
	rv = 0;
	if (pct) {
		PctParams p;
		bin_y(b.n_bins, b.histo_scale, b.histo_offset, ytab.data());
		if (hipMemcpyAsync(d_ytab, ytab.data(), sizeof(float) * b.n_bins, hipMemcpyHostToDevice, st) != hipSuccess)
			rv = -EIO;
		p.hist = b.d_histogram; p.ytab = d_ytab; p.d_y = NULL; p.d_bin = d_bins;
		p.n = b.fft_len; p.n_bins = b.n_bins; p.c0 = cfg->first_bin; p.c1 = cfg->first_bin + cfg->n_cols;
		for (int k = 0; k < FOSPHOR_AMD_DETECT_MAX_Q; k++)
			p.q[k] = cfg->floor_q;
		if (!rv)
			rv = launch_percentiles(self, st, p, 1);
		if (!rv) {
			hipLaunchKernelGGL(k_floor, dim3(1), dim3(kLanes), 0, st, d_bins, cfg->first_bin, cfg->n_cols, b.n_bins, d_ytab,
			                   cfg->margin_y, d_result);
			rv = launch_counted(stats, FOSPHOR_AMD_DETECT_FLOOR);
		}
	}
	if (!rv) {
		BandParams bp;
		bp.trace = b.d_spectrum + (cfg->trace == FOSPHOR_AMD_TRACE_MAXHOLD ? 2 * (size_t)b.fft_len : 0);
		bp.res = d_result; bp.bands = d_bands;
		bp.first_bin = cfg->first_bin; bp.n_cols = cfg->n_cols;
		bp.max_gap = cfg->max_gap; bp.min_cols = cfg->min_cols; bp.max_bands = max_bands;
		bp.absolute = !pct; bp.threshold_y = cfg->threshold_y;
		hipLaunchKernelGGL(k_bands, dim3(1), dim3(kLanes), 0, st, bp);
		rv = launch_counted(stats, FOSPHOR_AMD_DETECT_BANDS);
	}
	return drain(st, rv);
}
