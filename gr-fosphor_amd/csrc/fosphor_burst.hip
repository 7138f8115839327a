/*
 * fosphor_burst.hip -- bursts in time and frequency: connected regions of the waterfall ring (include/fosphor_amd_burst.h)
 *
 * Read-only passes over the instance's waterfall, in a file of their own: nothing here is on the process / merge path.  All ordering
 * between the stages is by kernel boundaries on the instance's stream: no work-group ever waits for another, nothing is polled, and
 * every loop has a bound that can be read off the code.
 *
 *   k_burst_runs    the streaming pass, by the strip read of the ring-pass substrate (fosphor_ring.h): a work-group of 256 lanes
 *                   owns one strip of 1024 columns of one row, lane t the aligned group of 4 shifted columns at strip + 4t, one
 *                   16-byte load.  Gap closing needs, per cell, the nearest on cell before and after it
 *                   (detect's k_bands takes them from a max and a min scan): here a lane finds them among its own 4 cells, then in
 *                   its wave with one ballot and one shuffle each way (lanes ascend with columns, so the nearest lane with an on cell
 *                   is the highest / lowest bit of the ballot on that side), then among the 4 waves through LDS, then from the other
 *                   strips of the row.  An on cell starts a run when no on cell precedes it or the gap between them is longer than
 *                   max_gap_cols; a cell is in a run when it is on, or lies between two on cells no further apart than that.
 *                   The kernel runs twice.  <false> counts: per row and strip the first and last on column and the starts whose
 *                   predecessor lies in the same strip.  <true> writes: it knows the row's other strips and its place in the run
 *                   list, numbers its starts with two ballots (a lane holds at most 2), and leaves first / last (one writer each),
 *                   peak key and energy of every run.  A lane's 4 cells lie in at most 2 runs; the cells of a run are contiguous, so
 *                   a segmented shuffle scan over "the last run of each lane" sums a run within a wave and one lane per run and wave
 *                   sends the atomics (64-bit max, fp64 add).
 *   k_burst_rows    between the two: one wave per row, one lane per strip (at most 64): what precedes and follows each strip,
 *                   whether its first on cell is a start, the strip's place in the row, the row's count, and whether the strip holds
 *                   any cell of a run at all (if not, <true> returns before it loads anything: a sparse field is read once).
 *   k_burst_scan    exclusive scan of the rows' counts, one work-group (the substrate's block_scan); the host reads the total, decides
 *                   overflow and sizes the scratch that grows with the runs.
 *   k_burst_init    parent[r] = r, empty run and component records.
 *   k_burst_link    one lane per run: for each of the next max_gap_rows + 1 rows a binary search for the first run that can
 *                   intersect, a walk while they do, a lock-free union (root = lowest index).
 *   k_burst_reduce  one lane per run: find the root, fold the record into the root's with integer atomics, the 64-bit max and the
 *                   fp64 add.
 *   k_burst_emit    one work-group: roots that pass the filters are numbered by a sum scan over lane-owned chunks, ascending.
 */
#include <errno.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "fosphor_ring.h"
#include "../../include/fosphor_amd_burst.h"

namespace {

using namespace ring_pass;				/* kMaxCols, kStrip, kMaxStrips (k_burst_rows gives a strip a lane of one wave) */

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kScanLanes = 1024;
constexpr int kSearchSteps = 17;			/* a binary search over at most 65536 + 1 entries */
constexpr int kNone = INT32_MAX;

static_assert(kStrip == kThreads * 4, "a lane owns 4 columns of the strip");
static_assert(FOSPHOR_AMD_BURST_STATS <= FOSPHOR_COUNTERS_MAX, "the instance holds the counters");
static_assert(FOSPHOR_AMD_BURST_MAX_ROWS <= 65536 && kMaxCols <= 65536, "16 bits each in the peak key");

typedef unsigned long long u64;

/* One run of one row.  key: (orderable bits of y) << 32 | (0xffff - j) << 16 | (0xffff - column) of its greatest y, 0 while empty. */
struct Run {
	int32_t first, last;
	u64     key;
	double  energy;
};

struct Comp {
	int32_t newest, oldest, first, last, n_cells, pad;
	u64     key;
	double  energy;
};

struct RunParams {
	const float *wf;		/* the ring, [wf_rows][n], unshifted columns */
	const float *thr;		/* [n] shifted, or NULL */
	float thr_y;
	int n;
	int c0, c1;			/* the window [c0, c1), shifted columns */
	int gap;			/* max_gap_cols */
	int n_rows, strips;
	int row_base, row_mask;		/* ring row of source row j: (row_base - j) & row_mask */
	/* [n_rows][strips].  <false> leaves (first on column or kNone, last on column or -1, starts inside the strip); k_burst_rows
	 * replaces them by (next on column after the strip or kNone, last on column before it or -1, runs of the row that start before
	 * the strip, or -1 when the strip holds no cell of a run) */
	int *sum_first, *sum_last, *sum_cnt;
	int *row_cnt;			/* [n_rows] */
	const int *row_off;		/* [n_rows + 1] */
	Run *runs;
	int n_runs;
};

/* y (not NaN) -> 32 bits that order as y does; -0 counts as +0; never 0 */
__device__ __host__ __forceinline__ uint32_t order_bits(float y)
{
	union { float f; uint32_t u; } c;
	c.f = y + 0.0f;
	return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

__device__ __host__ __forceinline__ float order_value(uint32_t b)
{
	union { float f; uint32_t u; } c;
	c.u = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
	return c.f;
}

__device__ __forceinline__ void run_send(const RunParams &p, int id, u64 key, double energy)
{
	if ((unsigned)id < (unsigned)p.n_runs) {
		atomicMax(&p.runs[id].key, key);
		unsafeAtomicAdd(&p.runs[id].energy, energy);
	}
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads)
void k_burst_runs(const RunParams p)
{
	__shared__ int s_first[kWaves], s_last[kWaves], s_n[kWaves];

	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int j = blockIdx.x / p.strips, strip = blockIdx.x - j * p.strips;
	const size_t at = blockIdx.x;
	int base = 0, carry_prev = -1, carry_next = kNone;
	if (kWrite) {
		base = p.sum_cnt[at];
		if (base < 0)						/* the same in the whole work-group */
			return;
		carry_next = p.sum_first[at];
		carry_prev = p.sum_last[at];
	}
	const int s = group_of(p.c0, strip, tid);			/* this lane's shifted columns s .. s + 3 */

	uint32_t in = 0;						/* the strip read, written out: fosphor_ring.h says why */
#pragma unroll
	for (int e = 0; e < 4; e++)
		if (s + e >= p.c0 && s + e < p.c1)
			in |= 1u << e;
	const float nan = __builtin_nanf("");
	float4 v = make_float4(nan, nan, nan, nan);
	float thr[4] = { nan, nan, nan, nan };
	if (in) {							/* read where `in` says only */
		const float *q = p.wf + (size_t)ring_row(p.row_base, p.row_mask, j) * p.n + mem_col(s, p.n);
		if (in == 15u) {
			v = *reinterpret_cast<const float4 *>(q);
		} else {						/* a group the window cuts: its columns one by one */
			if (in & 1u) v.x = q[0];
			if (in & 2u) v.y = q[1];
			if (in & 4u) v.z = q[2];
			if (in & 8u) v.w = q[3];
		}
#pragma unroll
		for (int e = 0; e < 4; e++)
			if ((in >> e) & 1)
				thr[e] = p.thr ? p.thr[s + e] : p.thr_y;
	}
	const float y[4] = { v.x, v.y, v.z, v.w };
	bool on[4];
	int my_first = kNone, my_last = -1;
#pragma unroll
	for (int e = 0; e < 4; e++) {
		on[e] = y[e] > thr[e];					/* false for a NaN on either side, and outside the window */
		if (on[e]) {
			my_first = min(my_first, s + e);
			my_last = s + e;
		}
	}

	/* the nearest on cell before and after this lane's group: in the wave, then among the waves, then from the other strips */
	const u64 b = __ballot(my_last >= 0);
	const u64 lt = (1ull << lane) - 1, gt = ~((lt << 1) | 1ull);
	const u64 below = b & lt, above = b & gt;
	int prev_w = __shfl(my_last, below ? top_lane(below) : lane);
	int next_w = __shfl(my_first, above ? low_lane(above) : lane);
	int w_first = __shfl(my_first, b ? low_lane(b) : 0);
	int w_last = __shfl(my_last, b ? top_lane(b) : 0);
	if (!below) prev_w = -1;
	if (!above) next_w = kNone;
	if (lane == 0) {
		s_first[wave] = b ? w_first : kNone;
		s_last[wave] = b ? w_last : -1;
	}
	__syncthreads();
	int prev_in = carry_prev, next_in = carry_next;
#pragma unroll
	for (int w = 0; w < kWaves; w++) {
		if (w < wave) prev_in = max(prev_in, s_last[w]);
		if (w > wave) next_in = min(next_in, s_first[w]);
	}
	int prev[4], next[4];						/* per cell, strictly before / after it */
	int run = max(prev_w, prev_in);
#pragma unroll
	for (int e = 0; e < 4; e++) {
		prev[e] = run;
		if (on[e]) run = s + e;
	}
	run = min(next_w, next_in);
#pragma unroll
	for (int e = 3; e >= 0; e--) {
		next[e] = run;
		if (on[e]) run = s + e;
	}
	/* a start: an on cell without a predecessor, or further than the gap from it.  <false> knows no other strip: the strip's first on
	 * cell is left to k_burst_rows. */
	bool start[4];
	int n_start = 0;
#pragma unroll
	for (int e = 0; e < 4; e++) {
		start[e] = on[e] && (prev[e] < 0 ? kWrite : (s + e - prev[e] - 1 > p.gap));
		n_start += start[e] ? 1 : 0;
	}
	const u64 b1 = __ballot(n_start >= 1), b2 = __ballot(n_start >= 2);	/* a lane holds at most 2 starts */
	if (lane == 0)
		s_n[wave] = __popcll(b1) + __popcll(b2);
	__syncthreads();

	if (!kWrite) {
		if (tid == 0) {
			int f = kNone, l = -1, c = 0;
#pragma unroll
			for (int w = 0; w < kWaves; w++) {
				f = min(f, s_first[w]);
				l = max(l, s_last[w]);
				c += s_n[w];
			}
			p.sum_first[at] = f;
			p.sum_last[at] = l;
			p.sum_cnt[at] = c;
		}
		return;
	}

	int open = p.row_off[j] + base + __popcll(b1 & lt) + __popcll(b2 & lt) - 1;	/* the run open where this lane's group begins */
#pragma unroll
	for (int w = 0; w < kWaves; w++)
		if (w < wave) open += s_n[w];
	int id[4];
	bool any = false;
#pragma unroll
	for (int e = 0; e < 4; e++) {
		open += start[e] ? 1 : 0;
		const bool inr = ((in >> e) & 1) &&
		                 (on[e] || (prev[e] >= 0 && next[e] != kNone && next[e] - prev[e] - 1 <= p.gap));
		id[e] = (inr && (unsigned)open < (unsigned)p.n_runs) ? open : -1;	/* the bound holds by construction; checked all the same */
		any = any || id[e] >= 0;
	}
	if (!__ballot(any))						/* no barrier follows */
		return;

	/* first and last have one writer each; the lane's cells fold into its first and its last run (at most 2: two runs are a gap apart) */
	int id_a = -1, id_l = -1;					/* the lane's earlier run when it holds two; its last (or only) run */
	u64 k_a = 0, k_l = 0;
	double e_a = 0.0, e_l = 0.0;
#pragma unroll
	for (int e = 0; e < 4; e++) {
		if (id[e] < 0)
			continue;
		if (start[e])
			p.runs[id[e]].first = s + e;
		if (on[e] && (next[e] == kNone || next[e] - (s + e) - 1 > p.gap))
			p.runs[id[e]].last = s + e;
		const u64 k = (y[e] == y[e]) ? ((u64)order_bits(y[e]) << 32) | ((u64)(0xffffu - (uint32_t)j) << 16) | (0xffffu - (uint32_t)(s + e))
		                             : 0ull;
		const double t = power_term(y[e]);
		if (id[e] != id_l && id_l >= 0) {			/* a second run begins: the first is complete in this lane */
			id_a = id_l; k_a = k_l; e_a = e_l;
			id_l = -1;
		}
		if (id_l < 0) {
			id_l = id[e]; k_l = k; e_l = t;
		} else {
			k_l = k > k_l ? k : k_l;
			e_l += t;
		}
	}
	const int id_head = id_a >= 0 ? id_a : id_l;			/* the run of the lane's first cell that is in one */
	/* Inclusive segmented scan over the lanes' last runs.  Equal ids are contiguous in lane order (a run's cells are contiguous
	 * columns, ids ascend with columns), so "the lane d below has my id" means every lane between has it.  log2(64) steps. */
	for (int d = 1; d < 64; d <<= 1) {
		const int oid = __shfl_up(id_l, d);
		const u64 ok = shfl_up_u64(k_l, d);
		const double oe = __shfl_up(e_l, d);
		if (lane >= d && oid == id_l && id_l >= 0) {
			k_l = ok > k_l ? ok : k_l;
			e_l += oe;
		}
	}
	const int pid = __shfl_up(id_l, 1);
	const u64 pk = shfl_up_u64(k_l, 1);
	const double pe = __shfl_up(e_l, 1);
	const int nhead = __shfl_down(id_head, 1);
	if (id_a >= 0) {						/* the earlier of two runs ends in this lane: add what the lanes below hold of it */
		if (lane > 0 && pid == id_a) {
			k_a = pk > k_a ? pk : k_a;
			e_a += pe;
		}
		run_send(p, id_a, k_a, e_a);
	}
	if (id_l >= 0 && (lane == 63 || nhead != id_l))		/* the last lane of the wave that holds cells of this run */
		run_send(p, id_l, k_l, e_l);
}

/* one wave per row, lane = strip */
__global__ __launch_bounds__(kThreads)
void k_burst_rows(const RunParams p)
{
	const int lane = threadIdx.x & 63;
	const int j = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (j >= p.n_rows)						/* the same in the whole wave */
		return;
	const bool have = lane < p.strips;
	const size_t at = (size_t)j * p.strips + lane;
	const int first = have ? p.sum_first[at] : kNone, last = have ? p.sum_last[at] : -1;
	int cnt = have ? p.sum_cnt[at] : 0;

	const u64 b = __ballot(last >= 0);
	const u64 lt = (1ull << lane) - 1, gt = ~((lt << 1) | 1ull);
	const u64 below = b & lt, above = b & gt;
	int prev = __shfl(last, below ? top_lane(below) : lane);
	int next = __shfl(first, above ? low_lane(above) : lane);
	if (!below) prev = -1;
	if (!above) next = kNone;
	if (last >= 0 && (prev < 0 || first - prev - 1 > p.gap))	/* the strip's first on cell starts a run */
		cnt++;
	int incl = cnt;
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(incl, d);
		if (lane >= d)
			incl += o;
	}
	const int total = __shfl(incl, 63);
	const bool need = last >= 0 || (prev >= 0 && next != kNone && next - prev - 1 <= p.gap);
	if (have) {
		p.sum_first[at] = next;
		p.sum_last[at] = prev;
		p.sum_cnt[at] = need ? incl - cnt : -1;
	}
	if (lane == 0)
		p.row_cnt[j] = total;
}

/* row_off[j] = runs of the rows before j, row_off[n_rows] = *total = all of them.  Lane t owns the rows [t * chunk, (t + 1) * chunk).
 * The sums are 64-bit (65536 rows of 32768 runs are 2^31) and leave saturated; offsets mean something only below the run limit. */
__global__ __launch_bounds__(kScanLanes)
void k_burst_scan(const int *row_cnt, int n_rows, int *row_off, int *total)
{
	__shared__ long long s[kScanLanes];
	const int t = threadIdx.x;
	int g0, g1;
	chunk_of<kScanLanes>(n_rows, t, g0, g1);

	long long mine = 0;
	for (int j = g0; j < g1; j++)
		mine += row_cnt[j];
	block_scan<kScanLanes>(s, t, mine, OpAdd());
	long long k = t ? s[t - 1] : 0;
	for (int j = g0; j < g1; j++) {
		row_off[j] = (int)(k < INT32_MAX ? k : INT32_MAX);
		k += row_cnt[j];
	}
	if (t == kScanLanes - 1) {
		const long long all = s[kScanLanes - 1];
		row_off[n_rows] = *total = (int)(all < INT32_MAX ? all : INT32_MAX);
	}
}

__global__ __launch_bounds__(kThreads)
void k_burst_init(int *parent, Run *runs, Comp *comps, int n_runs)
{
	const int r = blockIdx.x * kThreads + threadIdx.x;
	if (r >= n_runs)
		return;
	parent[r] = r;
	Run u;
	u.first = 0; u.last = -1; u.key = 0; u.energy = 0.0;
	runs[r] = u;
	Comp c;
	c.newest = kNone; c.oldest = -1; c.first = kNone; c.last = -1; c.n_cells = 0; c.pad = 0; c.key = 0; c.energy = 0.0;
	comps[r] = c;
}

/* The root of x.  parent[v] <= v always (k_burst_init sets v, uf_union only ever lowers it, to a smaller index), so the walk strictly
 * decreases until it stands: at most x steps.  A stale read is a former parent, which is still in x's set and still below. */
__device__ __forceinline__ int uf_find(const int *parent, int x)
{
	for (int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED); p < x; p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED))
		x = p;
	return x;
}

/* Join the sets of a and b: hang the larger root under the smaller.  atomicMin on parent[a] with b < a returns a when a was still a
 * root (done: a now points to b), else a value old < a that another lane put there first; min(old, b) is now a's parent, both are
 * in a's set, and the pair left to join is (old, b), whose larger root is strictly below a.  So the larger root strictly decreases
 * with every retry, which the loop's own counter restates: at most max(a, b) + 1 rounds, each a bounded uf_find.  No lane waits for
 * another; every round completes alone. */
__device__ __forceinline__ void uf_union(int *parent, int a, int b)
{
	for (int left = max(a, b); left >= 0; left--) {
		a = uf_find(parent, a);
		b = uf_find(parent, b);
		if (a == b)
			return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(&parent[a], b);
		if (old == a)
			return;
		a = old;						/* old < a */
	}
}

/* the row of run r: the greatest j with row_off[j] <= r (rows without runs share an offset with the next row that has some) */
__device__ __forceinline__ int row_of(const int *row_off, int n_rows, int r)
{
	int lo = 0, hi = n_rows - 1;
	for (int it = 0; it < kSearchSteps && lo < hi; it++) {
		const int mid = (lo + hi + 1) >> 1;
		if (row_off[mid] <= r) lo = mid; else hi = mid - 1;
	}
	return lo;
}

__global__ __launch_bounds__(kThreads)
void k_burst_link(const Run *runs, const int *row_off, int n_rows, int n_runs, int gap_rows, int *parent)
{
	const int r = blockIdx.x * kThreads + threadIdx.x;
	if (r >= n_runs)
		return;
	const int j = row_of(row_off, n_rows, r);
	const int a1 = runs[r].first, a2 = runs[r].last;
	for (int k = 1; k <= gap_rows + 1 && j + k < n_rows; k++) {
		const int b0 = row_off[j + k], b1 = min(row_off[j + k + 1], n_runs);
		int lo = b0, hi = b1;					/* the first run of that row that ends at or after a1 */
		for (int it = 0; it < kSearchSteps && lo < hi; it++) {
			const int mid = (lo + hi) >> 1;
			if (runs[mid].last < a1) lo = mid + 1; else hi = mid;
		}
		for (int q = lo; q < b1 && runs[q].first <= a2; q++)	/* the runs of a row are disjoint and ascending */
			uf_union(parent, r, q);
	}
}

__global__ __launch_bounds__(kThreads)
void k_burst_reduce(const Run *runs, const int *row_off, int n_rows, int n_runs, const int *parent, Comp *comps)
{
	const int r = blockIdx.x * kThreads + threadIdx.x;
	if (r >= n_runs)
		return;
	const int j = row_of(row_off, n_rows, r);
	const int root = uf_find(parent, r);
	const Run u = runs[r];
	Comp *c = &comps[root];
	atomicMin(&c->newest, j);
	atomicMax(&c->oldest, j);
	atomicMin(&c->first, u.first);
	atomicMax(&c->last, u.last);
	atomicAdd(&c->n_cells, u.last - u.first + 1);
	atomicMax(&c->key, u.key);
	unsafeAtomicAdd(&c->energy, u.energy);
}

struct EmitParams {
	const int *parent;
	const Comp *comps;
	int n_runs, n_rows, c0, c1, min_rows, min_cols, max_bursts;
	struct fosphor_amd_burst *bursts;
	struct fosphor_amd_burst_result *res;
};

__device__ __forceinline__ bool kept(const EmitParams &p, int r)
{
	if (p.parent[r] != r)
		return false;
	const Comp &c = p.comps[r];
	return c.oldest - c.newest + 1 >= p.min_rows && c.last - c.first + 1 >= p.min_cols;
}

/* Lane t owns the runs [t * chunk, (t + 1) * chunk), chunk = ceil(n_runs / 1024) <= 1024. */
__global__ __launch_bounds__(kScanLanes)
void k_burst_emit(const EmitParams p)
{
	__shared__ int s[kScanLanes];
	__shared__ int s_roots;
	const int t = threadIdx.x;
	int g0, g1;
	chunk_of<kScanLanes>(p.n_runs, t, g0, g1);

	if (t == 0)
		s_roots = 0;
	int mine = 0, roots = 0;
	for (int r = g0; r < g1; r++) {
		roots += p.parent[r] == r ? 1 : 0;
		mine += kept(p, r) ? 1 : 0;
	}
	block_scan<kScanLanes>(s, t, mine, OpAdd());	/* its barriers order the initialisation above */
	if (roots)
		atomicAdd(&s_roots, roots);				/* LDS integer atomic: exact in any order */
	int k = t ? s[t - 1] : 0;
	const int total = s[kScanLanes - 1];
	for (int r = g0; r < g1 && k < p.max_bursts; r++) {
		if (!kept(p, r))
			continue;
		const Comp &c = p.comps[r];
		struct fosphor_amd_burst o;
		o.newest = c.newest; o.oldest = c.oldest;
		o.first_col = c.first; o.last_col = c.last;
		o.n_cells = c.n_cells;
		o.peak_row = 0xffff - (int)((c.key >> 16) & 0xffffu);
		o.peak_col = 0xffff - (int)(c.key & 0xffffu);
		o.peak_y = order_value((uint32_t)(c.key >> 32));
		o.energy_y = (float)(0.5 * log10(c.energy));
		o.flags = (c.newest == 0 ? FOSPHOR_AMD_BURST_ON : 0u) | (c.oldest == p.n_rows - 1 ? FOSPHOR_AMD_BURST_CUT : 0u) |
		          (c.first == p.c0 ? FOSPHOR_AMD_BURST_FIRST_COL : 0u) | (c.last == p.c1 - 1 ? FOSPHOR_AMD_BURST_LAST_COL : 0u);
		p.bursts[k++] = o;
	}
	__syncthreads();
	if (t == 0) {
		struct fosphor_amd_burst_result r;
		r.n_runs = p.n_runs;
		r.n_components = s_roots;
		r.n_found = total;
		r.n_written = min(total, p.max_bursts);
		r.overflow = 0;
		*p.res = r;
	}
}

/* what both entry points refuse before they look at the data; n = columns of the buffer the window lies in */
bool cfg_ok(const struct fosphor_amd_burst_cfg *cfg, int n, int max_rows, int max_bursts)
{
	if (!window_ok(cfg->first_bin, cfg->n_cols, n))
		return false;
	if (cfg->rows < 1 || cfg->rows > max_rows || cfg->rows > FOSPHOR_AMD_BURST_MAX_ROWS)
		return false;
	if (cfg->max_gap_cols < 0 || cfg->max_gap_rows < 0 || cfg->max_gap_rows > FOSPHOR_AMD_BURST_MAX_GAP_ROWS)
		return false;
	if (cfg->min_rows < 1 || cfg->min_cols < 1)
		return false;
	if (cfg->max_runs < 1 || cfg->max_runs > FOSPHOR_AMD_BURST_MAX_RUNS)
		return false;
	return max_bursts >= 1 && max_bursts <= FOSPHOR_AMD_BURST_MAX_BURSTS;
}

} // namespace

extern "C" int fosphor_amd_burst_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_BURST_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_BURST, FOSPHOR_AMD_BURST_STATS, stats);
}

extern "C" int fosphor_amd_bursts_host(const float *ys, int rows, int n, const float *thr_or_null,
                                       const struct fosphor_amd_burst_cfg *cfg, struct fosphor_amd_burst_result *res,
                                       struct fosphor_amd_burst *out, int max_bursts)
{
	struct HostRun { int j, first, last; };

	if (!ys || !cfg || !res || !out || rows < 1 || n < 1)
		return -EINVAL;
	if (cfg->rows != rows || cfg->n_cols != n || !cfg_ok(cfg, kMaxCols, FOSPHOR_AMD_BURST_MAX_ROWS, max_bursts))
		return -EINVAL;

	/* rules 1 and 2: an on cell extends the open run when the gap behind it is short enough, else it starts one */
	std::vector<HostRun> runs;
	std::vector<int> row_off(rows + 1, 0);
	long long n_runs = 0;
	for (int j = 0; j < rows; j++) {
		const float *y = ys + (size_t)j * n;
		int last_on = -1;
		for (int i = 0; i < n; i++) {
			if (!(y[i] > (thr_or_null ? thr_or_null[i] : cfg->threshold_y)))
				continue;
			if (last_on >= 0 && i - last_on - 1 <= cfg->max_gap_cols) {
				if (n_runs <= cfg->max_runs)
					runs.back().last = i;
			} else {
				n_runs++;
				if (n_runs <= cfg->max_runs)
					runs.push_back(HostRun{ j, i, i });
			}
			last_on = i;
		}
		row_off[j + 1] = (int)(n_runs < INT32_MAX ? n_runs : INT32_MAX);
	}
	res->n_runs = (int32_t)(n_runs < INT32_MAX ? n_runs : INT32_MAX);
	res->n_components = res->n_found = res->n_written = 0;
	res->overflow = n_runs > cfg->max_runs;
	if (res->overflow)
		return 0;

	/* rule 3: the root of a set is its lowest index */
	const int nr = (int)runs.size();
	std::vector<int> parent(nr);
	for (int r = 0; r < nr; r++)
		parent[r] = r;
	auto find = [&](int x) { while (parent[x] != x) x = parent[x]; return x; };
	for (int r = 0; r < nr; r++) {
		const int j = runs[r].j;
		for (int k = 1; k <= cfg->max_gap_rows + 1 && j + k < rows; k++)
			for (int q = row_off[j + k]; q < row_off[j + k + 1]; q++)
				if (runs[r].first <= runs[q].last && runs[q].first <= runs[r].last) {
					const int a = find(r), b = find(q);
					if (a != b)
						parent[a > b ? a : b] = a > b ? b : a;
				}
	}

	/* rule 4: the records, folded in run order (row-major: a strict > keeps the smallest j, then the smallest column) */
	struct HostComp { int newest, oldest, first, last, n_cells, peak_row, peak_col; bool has; float peak; double sum; };
	std::vector<HostComp> comps(nr, HostComp{ INT32_MAX, -1, INT32_MAX, -1, 0, -1, -1, false, 0.0f, 0.0 });
	for (int r = 0; r < nr; r++) {
		HostComp &c = comps[find(r)];
		const HostRun &u = runs[r];
		c.newest = u.j < c.newest ? u.j : c.newest;
		c.oldest = u.j > c.oldest ? u.j : c.oldest;
		c.first = u.first < c.first ? u.first : c.first;
		c.last = u.last > c.last ? u.last : c.last;
		c.n_cells += u.last - u.first + 1;
		for (int i = u.first; i <= u.last; i++) {
			const float y = ys[(size_t)u.j * n + i];
			if (y == y && (!c.has || y > c.peak)) {
				c.has = true;
				c.peak = y + 0.0f;
				c.peak_row = u.j;
				c.peak_col = i;
			}
			const double t = pow(10.0, 2.0 * (double)y);
			if (isfinite(t))
				c.sum += t;
		}
	}
	for (int r = 0; r < nr; r++) {
		if (parent[r] != r)
			continue;
		res->n_components++;
		const HostComp &c = comps[r];
		if (c.oldest - c.newest + 1 < cfg->min_rows || c.last - c.first + 1 < cfg->min_cols)
			continue;
		if (res->n_found++ >= max_bursts)
			continue;
		struct fosphor_amd_burst &o = out[res->n_written++];
		o.newest = c.newest; o.oldest = c.oldest;
		o.first_col = cfg->first_bin + c.first; o.last_col = cfg->first_bin + c.last;
		o.n_cells = c.n_cells;
		o.peak_row = c.peak_row; o.peak_col = cfg->first_bin + c.peak_col;
		o.peak_y = c.peak;
		o.energy_y = (float)(0.5 * log10(c.sum));
		o.flags = (c.newest == 0 ? FOSPHOR_AMD_BURST_ON : 0u) | (c.oldest == rows - 1 ? FOSPHOR_AMD_BURST_CUT : 0u) |
		          (c.first == 0 ? FOSPHOR_AMD_BURST_FIRST_COL : 0u) | (c.last == n - 1 ? FOSPHOR_AMD_BURST_LAST_COL : 0u);
	}
	return 0;
}

extern "C" int fosphor_amd_bursts(struct fosphor *self, const struct fosphor_amd_burst_cfg *cfg, const float *d_threshold,
                                  struct fosphor_amd_burst_result *d_result, struct fosphor_amd_burst *d_bursts, int max_bursts)
{
	struct fosphor_amd_buffers b;
	void *d;

	if (!self || !cfg || !d_result || !d_bursts)
		return -EINVAL;
	if (!cfg_ok(cfg, kMaxCols, FOSPHOR_AMD_BURST_MAX_ROWS, max_bursts))	/* what needs no geometry, before the wait */
		return -EINVAL;
	if (open(self, &b))
		return -EIO;
	const int n = b.fft_len;
	if (!geometry_ok(b, 8))
		return -EINVAL;
	if (!cfg_ok(cfg, n, b.wf_rows, max_bursts))
		return -EINVAL;

	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_BURST);
	const int rows = cfg->rows;
	const int c0 = cfg->first_bin, c1 = cfg->first_bin + cfg->n_cols;
	const int strips = strips_of(c0, c1);
	if (strips < 1 || strips > kMaxStrips)
		return -EINVAL;

	/* scratch by rows and strips: three summaries per row and strip, the rows' counts and offsets, the total */
	const size_t cells = (size_t)rows * strips;
	const size_t fixed_ints = 3 * cells + (size_t)rows + (size_t)rows + 1 + 1;
	if (fosphor_amd_priv_scratch(self, FOSPHOR_SCRATCH_BURST_ROWS, fixed_ints * sizeof(int), &d))
		return -EIO;
	int *ints = (int *)d;

	RunParams p;
	p.wf = b.d_waterfall;
	p.thr = d_threshold;
	p.thr_y = cfg->threshold_y;
	p.n = n;
	p.c0 = c0; p.c1 = c1;
	p.gap = cfg->max_gap_cols;
	p.n_rows = rows; p.strips = strips;
	const Rows ring = waterfall_rows(b);
	p.row_base = ring.base; p.row_mask = ring.mask;
	p.sum_first = ints; p.sum_last = ints + cells; p.sum_cnt = ints + 2 * cells;
	p.row_cnt = ints + 3 * cells;
	int *row_off = p.row_cnt + rows;
	int *d_total = row_off + rows + 1;
	p.row_off = row_off;
	p.runs = NULL;
	p.n_runs = 0;

	stats[FOSPHOR_AMD_BURST_CALLS]++;
	const dim3 block(kThreads);
	hipLaunchKernelGGL(k_burst_runs<false>, dim3((unsigned)cells), block, 0, st, p);
	if (launch_counted(stats, FOSPHOR_AMD_BURST_K_COUNT))
		return -EIO;
	hipLaunchKernelGGL(k_burst_rows, dim3((rows + kWaves - 1) / kWaves), block, 0, st, p);
	if (launch_counted(stats, FOSPHOR_AMD_BURST_K_ROWS))
		return -EIO;
	hipLaunchKernelGGL(k_burst_scan, dim3(1), dim3(kScanLanes), 0, st, p.row_cnt, rows, row_off, d_total);
	if (launch_counted(stats, FOSPHOR_AMD_BURST_K_SCAN))
		return -EIO;

	/* the one integer the host waits for between the two run passes: the call is synchronous anyway */
	int total = 0;
	if (hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return -EIO;
	if (total < 0)
		return -EIO;
	if (total == 0 || total > cfg->max_runs) {
		struct fosphor_amd_burst_result r;
		r.n_runs = total;
		r.n_components = r.n_found = r.n_written = 0;
		r.overflow = total > cfg->max_runs;
		if (r.overflow)
			stats[FOSPHOR_AMD_BURST_OVERFLOWS]++;
		if (hipMemcpyAsync(d_result, &r, sizeof(r), hipMemcpyHostToDevice, st) != hipSuccess ||
		    hipStreamSynchronize(st) != hipSuccess)
			return -EIO;
		return 0;
	}

	/* scratch by runs, grown in powers of two: parent, run records, component records.  The stream is idle here. */
	size_t cap = 1024;
	while (cap < (size_t)total)
		cap <<= 1;
	if (fosphor_amd_priv_scratch(self, FOSPHOR_SCRATCH_BURST_RUNS, cap * (sizeof(Run) + sizeof(Comp) + sizeof(int)), &d))
		return -EIO;
	Run *runs = (Run *)d;
	Comp *comps = (Comp *)(runs + cap);
	int *parent = (int *)(comps + cap);
	p.runs = runs;
	p.n_runs = total;

	const dim3 per_run((total + kThreads - 1) / kThreads);
	hipLaunchKernelGGL(k_burst_init, per_run, block, 0, st, parent, runs, comps, total);
	int rv = launch_counted(stats, FOSPHOR_AMD_BURST_K_INIT);
	if (!rv) {
		hipLaunchKernelGGL(k_burst_runs<true>, dim3((unsigned)cells), block, 0, st, p);
		rv = launch_counted(stats, FOSPHOR_AMD_BURST_K_WRITE);
	}
	if (!rv) {
		hipLaunchKernelGGL(k_burst_link, per_run, block, 0, st, (const Run *)runs, (const int *)row_off, rows, total,
		                   cfg->max_gap_rows, parent);
		rv = launch_counted(stats, FOSPHOR_AMD_BURST_K_LINK);
	}
	if (!rv) {
		hipLaunchKernelGGL(k_burst_reduce, per_run, block, 0, st, (const Run *)runs, (const int *)row_off, rows, total,
		                   (const int *)parent, comps);
		rv = launch_counted(stats, FOSPHOR_AMD_BURST_K_REDUCE);
	}
	if (!rv) {
		EmitParams e;
		e.parent = parent; e.comps = comps;
		e.n_runs = total; e.n_rows = rows; e.c0 = c0; e.c1 = c1;
		e.min_rows = cfg->min_rows; e.min_cols = cfg->min_cols; e.max_bursts = max_bursts;
		e.bursts = d_bursts; e.res = d_result;
		hipLaunchKernelGGL(k_burst_emit, dim3(1), dim3(kScanLanes), 0, st, e);
		rv = launch_counted(stats, FOSPHOR_AMD_BURST_K_EMIT);
	}
	return drain(st, rv);
}
