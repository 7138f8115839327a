/*
 * fosphor_mask.hip -- frequency-mask trigger and channel power over the waterfall ring (include/fosphor_amd_mask.h)
 *
 * Read-only passes over the instance's plain buffers, in a file of their own: nothing here is on the process / merge path.
 *
 *   k_mask_scan     the hot pass, a pure streaming read of rows x columns x 4 B by the strip read of the ring-pass substrate
 *                   (fosphor_ring.h): a work-group of 256 lanes owns one strip of 1024 columns and a run of `rpg` consecutive rows,
 *                   one 16-byte load per lane and row, a coalesced 1 KiB per wave.  What depends on the column only is fetched once
 *                   per work-group and kept in registers for all its rows: the two limits of each column (NaN where there is none,
 *                   which no y violates, so the row loop carries no window test) and one bit per column and channel.  Rows are
 *                   loaded kUnroll at a time, independent of each other.
 *                   Per row a wave needs no shuffle for the counts and the first / last column: a comparison is a 64-bit lane
 *                   mask, the counts are its population counts, and lanes ascend with columns, so the first / last violating lane
 *                   is the mask's lowest / highest bit.  The peak is one 64-bit maximum of (excess bits, ~column): an excess is
 *                   positive, so its bits order as it does, and the lowest column wins a tie.  A channel's fp64 sum is reduced only
 *                   in the waves that hold columns of it (known from the shape, not from the data).  The four waves of the
 *                   work-group meet in LDS once, after the last row.
 *                   Two forms, chosen on the host from the shape alone.  ROWS: the columns fit one strip (every call at N = 1024),
 *                   the work-group owns its rows and writes their records, powers and trigger flags itself.  SHARED: several
 *                   strips (N = 65536: up to 64), the work-groups of a row leave partial records in scratch and
 *   k_mask_combine  merges them, one wave per row and one lane per strip.  Every reduction but the power is an integer sum, minimum
 *                   or maximum: the records are bit-identical whatever the split.
 *                   rpg = rows x strips / 1024, at least 1 and at most 32: a call is cut into 1024 work-groups before they take
 *                   more rows, so both extremes of shape fill the chip.  65536 rows of 1024 columns and 1024 rows of 65536 columns
 *                   both give 2048 work-groups of 32 rows; 3 rows of 65536 columns give 192 of one row.
 *   k_mask_events   compaction of the trigger flags into the ascending event list: one work-group, not the hot path.  A lane owns a
 *                   run of consecutive rows (so any number of rows fits), a sum scan over the lanes numbers the events.
 *   k_mask_trace    limit line from a trace: sliding fmaxf over 2 * spread + 1 vertices, tile plus halo in LDS.
 * Channels that do not lie inside the mask's window cannot share its read: they get a second scan launch, without limits, over the
 * columns from the first of them to the last.
 * No global atomics.
 */
#include <errno.h>
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "fosphor_ring.h"
#include "../../include/fosphor_amd_detect.h"
#include "../../include/fosphor_amd_mask.h"

namespace {

using namespace ring_pass;				/* kMaxCols, kStrip, kMaxStrips (k_mask_combine gives a strip a lane of one wave) */

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRpg = 32;				/* rows of a work-group at most (the size of its LDS) */
constexpr int kUnroll = 4;				/* rows loaded ahead of their reduction */
constexpr int kTargetGroups = 1024;			/* work-groups a call is cut into before they take more rows: 4 for each of the 256 CUs */
constexpr int kMaxCh = FOSPHOR_MAX_CHANNELS;
constexpr int kEvLanes = 1024;
constexpr int kTraceTile = 256;

static_assert(kStrip == kThreads * 4, "a lane owns 4 columns of the strip");
static_assert(FOSPHOR_AMD_MASK_STATS <= FOSPHOR_COUNTERS_MAX, "the instance holds the counters");

/* What a set of columns leaves of a row.  first / last: INT32_MAX / -1 when nothing violates; key: 0 when nothing is over, else
 * (bits of the excess) << 32 | (0xffffffff - column). */
struct Part {
	int32_t n_over, n_under, first, last;
	unsigned long long key;
};

struct ScanParams {
	const float *wf;		/* the ring, [wf_rows][n], unshifted columns */
	const float *upper, *lower;	/* [n] shifted, or NULL */
	struct fosphor_amd_mask_row *rows;	/* [n_rows] or NULL */
	float   *power;			/* [n_channels of the call][n_rows] */
	uint8_t *flags;			/* [n_rows]: the row triggered */
	Part    *parts;			/* SHARED: [n_rows][strips] */
	double  *pows;			/* SHARED: [n_rows][strips][kMaxCh] */
	int n;
	int c0, c1;			/* the shifted columns [c0, c1) this launch reads */
	int n_rows, rpg, strips;
	int row_base, row_mask;		/* ring row of source row j: (row_base - j) & row_mask */
	int min_cols;
	int emit_rows;			/* this launch writes the records and the flags (the launch over the mask's window) */
	int n_ch;			/* channels this launch sums */
	int ch_first[kMaxCh], ch_last[kMaxCh], ch_out[kMaxCh];	/* their columns, and their index in the call */
};

__device__ __forceinline__ Part part_none()
{
	Part m;
	m.n_over = 0; m.n_under = 0; m.first = INT32_MAX; m.last = -1; m.key = 0;
	return m;
}

__device__ __forceinline__ void part_merge(Part &a, const Part &b)
{
	a.n_over += b.n_over;
	a.n_under += b.n_under;
	a.first = min(a.first, b.first);
	a.last = max(a.last, b.last);
	a.key = a.key > b.key ? a.key : b.key;
}

/* the record and the trigger flag of row j from the merged parts of all its columns */
__device__ __forceinline__ void emit_row(const ScanParams &p, int j, const Part &m)
{
	if (p.rows) {
		struct fosphor_amd_mask_row r;
		r.n_over = m.n_over;
		r.n_under = m.n_under;
		r.first_col = m.last >= 0 ? m.first : -1;
		r.last_col = m.last;
		r.peak_col = m.key ? (int32_t)(0xffffffffu - (uint32_t)m.key) : -1;
		r.peak_over = m.key ? __uint_as_float((uint32_t)(m.key >> 32)) : __builtin_nanf("");
		p.rows[j] = r;
	}
	p.flags[j] = (m.n_over + m.n_under >= p.min_cols) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads)
void k_mask_scan(const ScanParams p)
{
	__shared__ Part   s_part[kMaxRpg][kWaves];
	__shared__ double s_pow[kMaxRpg][kWaves][kMaxCh];

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int strip = blockIdx.x;
	const int j0 = blockIdx.y * p.rpg;
	const int nj = min(p.rpg, p.n_rows - j0);			/* >= 1 by the grid */
	const int s = (p.c0 & ~3) + strip * kStrip + 4 * tid;		/* this lane's shifted columns s .. s + 3 */

	/* what depends on the column only: which of the 4 are read, their limits, their channels */
	uint32_t in = 0;						/* the strip read, written out: fosphor_ring.h says why */
#pragma unroll
	for (int e = 0; e < 4; e++)
		if (s + e >= p.c0 && s + e < p.c1)
			in |= 1u << e;
	float up[4], lo[4];
#pragma unroll
	for (int e = 0; e < 4; e++) {
		const bool on = (in >> e) & 1;
		up[e] = (on && p.upper) ? p.upper[s + e] : __builtin_nanf("");
		lo[e] = (on && p.lower) ? p.lower[s + e] : __builtin_nanf("");
	}
	uint32_t chbits = 0;						/* bit 4c + e: column s + e is in channel c */
	uint32_t wch = 0;						/* bit c: this wave holds columns of channel c */
	for (int c = 0; c < p.n_ch; c++) {
		uint32_t b = 0;
#pragma unroll
		for (int e = 0; e < 4; e++)
			if (((in >> e) & 1) && s + e >= p.ch_first[c] && s + e <= p.ch_last[c])
				b |= 1u << e;
		chbits |= b << (4 * c);
		if (__ballot(b != 0))
			wch |= 1u << c;
	}
	uint32_t chany = 0;
	for (int c = 0; c < kMaxCh; c++)
		chany |= (chbits >> (4 * c)) & 15u;

	for (int i = tid; i < kMaxRpg * kWaves * kMaxCh; i += kThreads)
		(&s_pow[0][0][0])[i] = 0.0;
	__syncthreads();

	const float *base = p.wf + ((s ^ (p.n >> 1)) & (p.n - 1));	/* read where `in` says only */
	const float nan = __builtin_nanf("");

	for (int r0 = 0; r0 < nj; r0 += kUnroll) {
		float4 v[kUnroll];
#pragma unroll
		for (int u = 0; u < kUnroll; u++) {
			v[u] = make_float4(nan, nan, nan, nan);
			if (r0 + u < nj && in) {
				const float *q = base + (size_t)((p.row_base - (j0 + r0 + u)) & p.row_mask) * p.n;
				if (in == 15u) {
					v[u] = *reinterpret_cast<const float4 *>(q);
				} else {				/* a group the window cuts: its columns one by one */
					if (in & 1u) v[u].x = q[0];
					if (in & 2u) v[u].y = q[1];
					if (in & 4u) v[u].z = q[2];
					if (in & 8u) v[u].w = q[3];
				}
			}
		}
#pragma unroll
		for (int u = 0; u < kUnroll; u++) {
			const int r = r0 + u;
			if (r >= nj)
				break;
			const float y[4] = { v[u].x, v[u].y, v[u].z, v[u].w };
			bool ov[4], un[4];
			unsigned long long m_over = 0, m_any = 0;
			int n_over = 0, n_under = 0;
#pragma unroll
			for (int e = 0; e < 4; e++) {
				ov[e] = y[e] > up[e];
				un[e] = y[e] < lo[e];
				const unsigned long long bo = __ballot(ov[e]), bu = __ballot(un[e]);
				n_over += __popcll(bo);
				n_under += __popcll(bu);
				m_over |= bo;
				m_any |= bo | bu;
			}
			Part w = part_none();
			w.n_over = n_over;
			w.n_under = n_under;
			if (m_any) {					/* the same in every lane */
				int my_first = 0, my_last = 0;
#pragma unroll
				for (int e = 3; e >= 0; e--)
					if (ov[e] || un[e])
						my_first = s + e;
#pragma unroll
				for (int e = 0; e < 4; e++)
					if (ov[e] || un[e])
						my_last = s + e;
				w.first = __shfl(my_first, low_lane(m_any));
				w.last = __shfl(my_last, top_lane(m_any));
			}
			if (m_over) {
				unsigned long long key = 0;
#pragma unroll
				for (int e = 0; e < 4; e++) {
					if (ov[e]) {
						const unsigned long long k = ((unsigned long long)__float_as_uint(y[e] - up[e]) << 32) |
						                             (0xffffffffu - (uint32_t)(s + e));
						key = k > key ? k : key;
					}
				}
				for (int d = 32; d; d >>= 1) {
					const unsigned long long o = shfl_xor_u64(key, d);
					key = o > key ? o : key;
				}
				w.key = key;
			}
			if (lane == 0)
				s_part[r][wave] = w;

			if (wch) {					/* the same in every lane, and known from the shape */
				double t[4];
#pragma unroll
				for (int e = 0; e < 4; e++)
					t[e] = ((chany >> e) & 1) ? power_term(y[e]) : 0.0;
				for (uint32_t m = wch; m; m &= m - 1) {
					const int c = __ffs(m) - 1;
					const uint32_t b = chbits >> (4 * c);
					double sum = 0.0;
#pragma unroll
					for (int e = 0; e < 4; e++)
						sum += ((b >> e) & 1) ? t[e] : 0.0;
					for (int d = 32; d; d >>= 1)
						sum += __shfl_xor(sum, d);
					if (lane == 0)
						s_pow[r][wave][c] = sum;
				}
			}
		}
	}
	__syncthreads();

	/* the waves meet: a lane per row, then a lane per row and channel */
	if (tid < nj) {
		Part m = s_part[tid][0];
#pragma unroll
		for (int w = 1; w < kWaves; w++)
			part_merge(m, s_part[tid][w]);
		const int j = j0 + tid;
		if (p.strips > 1)
			p.parts[(size_t)j * p.strips + strip] = m;
		else if (p.emit_rows)
			emit_row(p, j, m);
	}
	for (int i = tid; i < nj * p.n_ch; i += kThreads) {
		const int r = i / p.n_ch, c = i - r * p.n_ch;
		double sum = s_pow[r][0][c];
#pragma unroll
		for (int w = 1; w < kWaves; w++)
			sum += s_pow[r][w][c];
		const int j = j0 + r;
		if (p.strips > 1)
			p.pows[((size_t)j * p.strips + strip) * kMaxCh + c] = sum;
		else
			p.power[(size_t)p.ch_out[c] * p.n_rows + j] = (float)(0.5 * log10(sum));
	}
}

/* SHARED: one wave per row, lane = strip */
__global__ __launch_bounds__(kThreads)
void k_mask_combine(const ScanParams p)
{
	const int lane = threadIdx.x & 63;
	const int j = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (j >= p.n_rows)
		return;
	const bool have = lane < p.strips;
	const size_t at = (size_t)j * p.strips + lane;

	if (p.emit_rows) {
		Part m = have ? p.parts[at] : part_none();
		for (int d = 32; d; d >>= 1) {
			Part o;
			o.n_over = __shfl_xor(m.n_over, d);
			o.n_under = __shfl_xor(m.n_under, d);
			o.first = __shfl_xor(m.first, d);
			o.last = __shfl_xor(m.last, d);
			o.key = shfl_xor_u64(m.key, d);
			part_merge(m, o);
		}
		if (lane == 0)
			emit_row(p, j, m);
	}
	for (int c = 0; c < p.n_ch; c++) {
		double sum = have ? p.pows[at * kMaxCh + c] : 0.0;
		for (int d = 32; d; d >>= 1)
			sum += __shfl_xor(sum, d);
		if (lane == 0)
			p.power[(size_t)p.ch_out[c] * p.n_rows + j] = (float)(0.5 * log10(sum));
	}
}

/* The event list and the result.  Lane t owns the rows [t * chunk, (t + 1) * chunk), chunk = ceil(n_rows / 1024). */
__global__ __launch_bounds__(kEvLanes)
void k_mask_events(const uint8_t *flags, int n_rows, int32_t *events, int max_events, struct fosphor_amd_mask_result *res)
{
	__shared__ int s[kEvLanes];
	__shared__ int s_newest, s_oldest;
	const int t = threadIdx.x;
	int g0, g1;
	chunk_of<kEvLanes>(n_rows, t, g0, g1);

	if (t == 0) {
		s_newest = INT32_MAX;
		s_oldest = -1;
	}
	int mine = 0, first = INT32_MAX, last = -1;
	for (int j = g0; j < g1; j++)
		if (flags[j]) {
			mine++;
			first = min(first, j);
			last = j;
		}
	block_scan<kEvLanes>(s, t, mine, OpAdd());		/* its barriers order the initialisation above */
	if (mine) {
		atomicMin(&s_newest, first);			/* LDS integer atomics: exact in any order */
		atomicMax(&s_oldest, last);
	}
	int k = t ? s[t - 1] : 0;
	const int total = s[kEvLanes - 1];
	if (events)
		for (int j = g0; j < g1 && k < max_events; j++)
			if (flags[j])
				events[k++] = j;
	__syncthreads();
	if (t == 0) {
		res->n_triggered = total;
		res->n_written = min(total, max_events);
		res->newest = total ? s_newest : -1;
		res->oldest = s_oldest;
	}
}

/* out[i] = fmaxf of the trace's y over [i - spread, i + spread] (clipped to the buffer) + margin */
__global__ __launch_bounds__(kTraceTile)
void k_mask_trace(const float *trace, int n, int spread, float margin_y, float *out)
{
	__shared__ float s[kTraceTile + 2 * FOSPHOR_AMD_MASK_MAX_SPREAD];
	const int t = threadIdx.x;
	const int i0 = blockIdx.x * kTraceTile;
	const int lo = i0 - spread;					/* column of s[0] */

	for (int k = t; k < kTraceTile + 2 * spread; k += kTraceTile) {
		const int col = lo + k;
		s[k] = (col >= 0 && col < n) ? trace[2 * (size_t)col + 1] : __builtin_nanf("");	/* fmaxf skips a NaN */
	}
	__syncthreads();
	const int i = i0 + t;
	if (i >= n)
		return;
	float m = __builtin_nanf("");
	for (int k = t; k <= t + 2 * spread; k++)
		m = fmaxf(m, s[k]);
	out[i] = m + margin_y;
}

int launch_scan(struct fosphor *self, hipStream_t st, ScanParams &p)
{
	p.strips = strips_of(p.c0, p.c1);
	if (p.strips < 1 || p.strips > kMaxStrips)
		return -EINVAL;
	long long rpg = (long long)p.n_rows * p.strips / kTargetGroups;
	p.rpg = (int)(rpg < 1 ? 1 : rpg > kMaxRpg ? kMaxRpg : rpg);
	const dim3 grid(p.strips, (p.n_rows + p.rpg - 1) / p.rpg), block(kThreads);
	hipLaunchKernelGGL(k_mask_scan, grid, block, 0, st, p);
	int rv = launch_counted(fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_MASK),
	                        p.strips > 1 ? FOSPHOR_AMD_MASK_FORM_SHARED : FOSPHOR_AMD_MASK_FORM_ROWS);
	if (!rv && p.strips > 1) {
		hipLaunchKernelGGL(k_mask_combine, dim3((p.n_rows + kWaves - 1) / kWaves), block, 0, st, p);
		rv = launch_ok();
	}
	return rv;
}

void row_rule(const float *y, const float *upper, const float *lower, int n, struct fosphor_amd_mask_row *out)
{
	out->n_over = out->n_under = 0;
	out->first_col = out->last_col = out->peak_col = -1;
	out->peak_over = __builtin_nanf("");
	for (int i = 0; i < n; i++) {
		const bool over = upper && y[i] > upper[i], under = lower && y[i] < lower[i];
		if (over) {
			const float e = y[i] - upper[i];
			out->n_over++;
			if (out->peak_col < 0 || e > out->peak_over) {	/* ascending i: the lowest column of equal excesses stays */
				out->peak_col = i;
				out->peak_over = e;
			}
		}
		if (under)
			out->n_under++;
		if (over || under) {
			if (out->first_col < 0)
				out->first_col = i;
			out->last_col = i;
		}
	}
}

} // namespace

extern "C" int fosphor_amd_mask_row_host(const float *row_y, const float *upper, const float *lower, int n,
                                         struct fosphor_amd_mask_row *out)
{
	if (!row_y || !out || n < 1)
		return -EINVAL;
	row_rule(row_y, upper, lower, n, out);
	return 0;
}

extern "C" int fosphor_amd_mask_from_points(int n, const double *col, const float *y, int n_pts, float *out)
{
	if (!col || !y || !out || n < 1 || n_pts < 1)
		return -EINVAL;
	for (int k = 0; k < n_pts; k++)
		if (col[k] != col[k] || (k && !(col[k] > col[k - 1])))
			return -EINVAL;
	int k = 0;						/* the segment [col[k], col[k + 1]) that holds i */
	for (int i = 0; i < n; i++) {
		const double x = i;
		if (x <= col[0]) {
			out[i] = y[0];
		} else if (x >= col[n_pts - 1]) {
			out[i] = y[n_pts - 1];
		} else {
			while (x >= col[k + 1])
				k++;
			const double c0 = col[k], c1 = col[k + 1], y0 = y[k], y1 = y[k + 1];
			out[i] = (float)(y0 + (y1 - y0) * ((x - c0) / (c1 - c0)));
		}
	}
	return 0;
}

extern "C" int fosphor_amd_mask_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_MASK_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_MASK, FOSPHOR_AMD_MASK_STATS, stats);
}

extern "C" int fosphor_amd_mask_from_trace(struct fosphor *self, int trace, float margin_y, int spread_cols, float *d_out)
{
	struct fosphor_amd_buffers b;

	if (!self || !d_out || spread_cols < 0 || spread_cols > FOSPHOR_AMD_MASK_MAX_SPREAD)
		return -EINVAL;
	if (trace != FOSPHOR_AMD_TRACE_LIVE && trace != FOSPHOR_AMD_TRACE_MAXHOLD)
		return -EINVAL;
	if (open(self, &b))
		return -EIO;
	if (b.fft_len < 1 || b.fft_len > kMaxCols)
		return -EINVAL;
	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);
	const float *tr = b.d_spectrum + (trace == FOSPHOR_AMD_TRACE_MAXHOLD ? 2 * (size_t)b.fft_len : 0);
	hipLaunchKernelGGL(k_mask_trace, dim3((b.fft_len + kTraceTile - 1) / kTraceTile), dim3(kTraceTile), 0, st,
	                   tr, b.fft_len, spread_cols, margin_y, d_out);
	return drain(st, launch_counted(fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_MASK), FOSPHOR_AMD_MASK_FROM_TRACE));
}

extern "C" int fosphor_amd_mask_scan(struct fosphor *self, const struct fosphor_amd_mask_cfg *cfg,
                                     const float *d_upper, const float *d_lower,
                                     struct fosphor_amd_mask_result *d_result,
                                     struct fosphor_amd_mask_row *d_rows,
                                     int32_t *d_events, int max_events,
                                     float *d_power)
{
	struct fosphor_amd_buffers b;
	void *d;

	if (!self || !cfg || !d_result)
		return -EINVAL;
	if (cfg->min_cols < 1 || cfg->n_channels < 0 || cfg->n_channels > kMaxCh)
		return -EINVAL;
	if (d_events ? (max_events < 1 || max_events > FOSPHOR_AMD_MASK_MAX_EVENTS) : max_events != 0)
		return -EINVAL;
	if ((cfg->n_channels > 0) != (d_power != NULL))
		return -EINVAL;
	const bool masked = d_upper || d_lower;
	if (!masked && cfg->n_channels == 0)
		return -EINVAL;
	if (open(self, &b))
		return -EIO;
	const int n = b.fft_len;
	if (!geometry_ok(b, 8))
		return -EINVAL;
	if (!window_ok(cfg->first_bin, cfg->n_cols, n) || cfg->rows < 1 || cfg->rows > b.wf_rows)
		return -EINVAL;
	for (int c = 0; c < cfg->n_channels; c++)
		if (cfg->channels[c].first < 0 || cfg->channels[c].last >= n || cfg->channels[c].first > cfg->channels[c].last)
			return -EINVAL;

	/* scratch of a size the instance's geometry fixes: flags [wf_rows], parts and pows [wf_rows][strips of the whole width] */
	const size_t max_strips = n > kStrip ? n / kStrip : 1;
	const size_t flag_bytes = ((size_t)b.wf_rows + 255) & ~(size_t)255;
	const size_t part_bytes = sizeof(Part) * b.wf_rows * max_strips;
	const size_t pow_bytes = sizeof(double) * kMaxCh * b.wf_rows * max_strips;
	if (fosphor_amd_priv_scratch(self, FOSPHOR_SCRATCH_MASK, flag_bytes + part_bytes + pow_bytes, &d))
		return -EIO;
	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);

	ScanParams p;
	p.wf = b.d_waterfall;
	p.rows = d_rows; p.power = d_power;
	p.flags = (uint8_t *)d;
	p.parts = (Part *)((uint8_t *)d + flag_bytes);
	p.pows = (double *)((uint8_t *)d + flag_bytes + part_bytes);
	p.n = n;
	p.n_rows = cfg->rows;
	const Rows ring = waterfall_rows(b);
	p.row_base = ring.base; p.row_mask = ring.mask;
	p.min_cols = cfg->min_cols;

	/* the launch over the mask's window takes the channels that lie inside it; without a mask one launch takes them all */
	const int w0 = cfg->first_bin, w1 = cfg->first_bin + cfg->n_cols;
	int rest[kMaxCh], n_rest = 0, h0 = n, h1 = 0;
	p.n_ch = 0;
	for (int c = 0; c < cfg->n_channels; c++) {
		const struct fosphor_amd_mask_channel &ch = cfg->channels[c];
		if (!masked || (ch.first >= w0 && ch.last < w1)) {
			p.ch_first[p.n_ch] = ch.first; p.ch_last[p.n_ch] = ch.last; p.ch_out[p.n_ch] = c;
			p.n_ch++;
		} else {
			rest[n_rest++] = c;
		}
		if (!masked || !(ch.first >= w0 && ch.last < w1)) {
			h0 = ch.first < h0 ? ch.first : h0;
			h1 = ch.last + 1 > h1 ? ch.last + 1 : h1;
		}
	}
	for (int c = p.n_ch; c < kMaxCh; c++)
		p.ch_first[c] = p.ch_last[c] = p.ch_out[c] = 0;
	p.upper = d_upper; p.lower = d_lower;
	p.c0 = masked ? w0 : h0;
	p.c1 = masked ? w1 : h1;
	p.emit_rows = 1;
	fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_MASK)[FOSPHOR_AMD_MASK_SCANS]++;
	int rv = launch_scan(self, st, p);
	if (!rv && n_rest) {
		p.upper = p.lower = NULL;
		p.c0 = h0; p.c1 = h1;
		p.emit_rows = 0;
		p.n_ch = n_rest;
		for (int k = 0; k < n_rest; k++) {
			p.ch_first[k] = cfg->channels[rest[k]].first;
			p.ch_last[k] = cfg->channels[rest[k]].last;
			p.ch_out[k] = rest[k];
		}
		rv = launch_scan(self, st, p);
	}
	if (!rv) {
		hipLaunchKernelGGL(k_mask_events, dim3(1), dim3(kEvLanes), 0, st, p.flags, cfg->rows, d_events, max_events, d_result);
		rv = launch_ok();
	}
	return drain(st, rv);
}
