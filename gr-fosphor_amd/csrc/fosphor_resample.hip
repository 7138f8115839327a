/*
 * fosphor_resample.hip -- burst IQ at U / D of its rate: a polyphase real FIR per job (include/fosphor_amd_resample.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote) and taps, in a file of its own: nothing here is on
 * the process / merge path and no buffer of the instance is read or written but the job table this file owns.
 *
 * The table of jobs, the search that gives a work-group its job, load_span(), the refusals every pass over burst IQ shares and the
 * tail of the call are those of fosphor_jobs.h; only jobs that write something are uploaded.  One launch per form present.
 *
 *   k_resample_tile    a work-group of 256 lanes owns kTile consecutive outputs of a job.  The tile begins at position p0 of the
 *                      up-sampled rate; b0 = ceil(p0 / U) is its first input sample and s0 = b0 U - p0 the branch of its first
 *                      output: two int64 operations per work-group, everything after them is 32-bit and relative to the tile.
 *                      Output k of the tile reads samples b0 + db .. b0 + db + Q - 1 and taps s, s + U, .., with
 *                      db = (k D - s0 + U - 1) / U and s = db U - (k D - s0).  LDS holds the taps as they lie in memory and,
 *                      behind them on a 16-byte boundary, the span as float2; each is widened where it is read.  Lane i owns
 *                      outputs i and i + 256: two independent chains of fused multiply-adds per component.  A lane without an
 *                      output computes the tile's last output once more and stores nothing: it reads loaded words only.
 *   k_resample_direct  jobs whose span and taps do not fit the budget: a lane owns one output and reads x and h from global memory.
 * The form is a function of (U, D, T) alone: tile_form().  Every output is computed by the operations of mac() in q ascending,
 * on the device and in fosphor_amd_resample_host alike.  No atomics of any kind, no work-group waits for another, every loop carries
 * its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_resample.h"

namespace {

typedef struct fosphor_amd_resample_job Job;

constexpr int kThreads = 256;
constexpr int kTile = FOSPHOR_AMD_RESAMPLE_TILE;
constexpr int kSlots = kTile / kThreads;			/* outputs of a lane */
constexpr int kTileLds = FOSPHOR_AMD_RESAMPLE_TILE_LDS;		/* bytes */
constexpr int kDirectOut = FOSPHOR_AMD_RESAMPLE_DIRECT_OUT;
constexpr int kMaxUp = FOSPHOR_AMD_RESAMPLE_MAX_UP;
constexpr int kMaxDown = FOSPHOR_AMD_RESAMPLE_MAX_DOWN;
constexpr int kMaxBranch = FOSPHOR_AMD_RESAMPLE_MAX_BRANCH;

static_assert(FOSPHOR_AMD_RESAMPLE_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 48, "the job table is uploaded as it is");
static_assert(kTile % kThreads == 0 && kSlots == 2, "two outputs a lane");
static_assert(kDirectOut == kThreads, "a lane owns one output");
static_assert(kTileLds % 16 == 0 && kTileLds <= 160 * 1024, "the LDS of a CU");
static_assert((long long)(kTile - 1) * kMaxDown < 0x7fffffffLL, "a tile's positions are 32-bit");

/* taps of a job in LDS, rounded up so that the span behind them begins on a 16-byte boundary */
inline __host__ __device__ int taps_room(int t) { return (t + 3) & ~3; }

/* the most samples a tile reads, and the form: (U, D, T) alone */
inline int tile_span(int u, int d, int t) { return (int)(((long long)(kTile - 1) * d + u - 1) / u) + t / u; }
inline bool tile_form(int u, int d, int t) { return 8LL * (tile_span(u, d, t) + 1) + 4LL * taps_room(t) <= kTileLds; }

inline bool ratio_ok(int up, int down) { return up >= 1 && up <= kMaxUp && down >= 1 && down <= kMaxDown; }

inline bool taps_ok(int up, int n_taps) { return n_taps >= 1 && n_taps % up == 0 && n_taps / up <= kMaxBranch; }

/* rule 1: the largest valid n_out; n >= 0, phase0 >= 0, the ratio and the taps in range.  (n - Q) * U < 2^39 */
inline int64_t max_n_out(int32_t n, int up, int down, int n_taps, int64_t phase0)
{
	const int q = n_taps / up;
	if (n < q)
		return 0;
	const int64_t room = (int64_t)(n - q) * up;
	return phase0 > room ? 0 : (room - phase0) / down + 1;
}

struct Params {
	const float2   *iq;
	const float    *taps;
	float2         *out;
	const Job      *jobs;		/* the jobs of this form that write something */
	const uint32_t *prefix;		/* [n_jobs + 1]: work-groups before job j */
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }		/* rule 2: one NaN */

/* rule 2: s + a * b with a * b exact, one rounding either way */
inline __host__ __device__ double mac(double s, double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_fma(a, b, s);
#else
	return s + a * b;
#endif
}

__global__ __launch_bounds__(kThreads)
void k_resample_tile(const Params p)
{
	__shared__ __align__(16) float s_lds[kTileLds / 4];
	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const Job job = p.jobs[j];
	const int U = job.up, D = job.down, T = job.n_taps, Q = T / U;
	const int m0 = (int)(blockIdx.x - p.prefix[j]) * kTile;		/* the tile's first output: m0 < n_out by the prefix */
	const int n_tile = min(kTile, job.n_out - m0);			/* 1 .. kTile */
	const int64_t p0 = job.phase0 + (int64_t)m0 * D;		/* >= 0 */
	const int64_t b0 = (p0 + U - 1) / U;
	const int s0 = (int)(b0 * U - p0);				/* 0 .. U - 1 */
	/* the last output's first sample, relative to b0; span <= tile_span(U, D, T), and b0 + span <= n: the job is valid */
	const int span = ((n_tile - 1) * D - s0 + U - 1) / U + Q;

	float *s_h = s_lds;
	float2 *s_x = reinterpret_cast<float2 *>(s_lds + taps_room(T));
	const int at = job_table::load_span<kThreads>(s_x, p.iq + job.offset + b0, span, tid);
	const float *h = p.taps + job.taps_offset;
	for (int i = tid; i < T; i += kThreads)
		s_h[i] = h[i];
	__syncthreads();

	const float2 *x[kSlots];
	const float *hs[kSlots];
	double re[kSlots], im[kSlots];
#pragma unroll
	for (int e = 0; e < kSlots; e++) {
		const int k = min(tid + kThreads * e, n_tile - 1);
		const int pos = k * D - s0;				/* > -U */
		const int db = (pos + U - 1) / U;
		x[e] = s_x + at + db;
		hs[e] = s_h + (db * U - pos);
		re[e] = im[e] = 0.0;
	}
	for (int q = 0; q < Q; q++) {
#pragma unroll
		for (int e = 0; e < kSlots; e++) {
			const double hv = (double)hs[e][q * U];
			const float2 xv = x[e][q];
			re[e] = mac(re[e], hv, (double)xv.x);
			im[e] = mac(im[e], hv, (double)xv.y);
		}
	}
	float2 *out = p.out + job.out_offset + m0;
#pragma unroll
	for (int e = 0; e < kSlots; e++) {
		const int k = tid + kThreads * e;
		if (k < n_tile)
			out[k] = make_float2(quiet((float)re[e]), quiet((float)im[e]));
	}
}

__global__ __launch_bounds__(kThreads)
void k_resample_direct(const Params p)
{
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const Job job = p.jobs[j];
	const int64_t m = (int64_t)(blockIdx.x - p.prefix[j]) * kDirectOut + threadIdx.x;
	if (m >= job.n_out)						/* there is no barrier below */
		return;
	const int U = job.up, Q = job.n_taps / U;
	const int64_t pos = job.phase0 + m * job.down;
	const int64_t b = (pos + U - 1) / U;				/* b + Q <= n: the job is valid */
	const float2 *x = p.iq + job.offset + b;
	const float *h = p.taps + job.taps_offset + (int)(b * U - pos);
	double re = 0.0, im = 0.0;
	for (int q = 0; q < Q; q++) {
		const double hv = (double)h[q * U];
		const float2 xv = x[q];
		re = mac(re, hv, (double)xv.x);
		im = mac(im, hv, (double)xv.y);
	}
	p.out[job.out_offset + m] = make_float2(quiet((float)re), quiet((float)im));
}

struct Plan {
	long long groups[2], jobs[2], outputs, macs;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, int64_t n_taps_total, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_RESAMPLE_MAX_JOBS) || n_samples < 0 || n_taps_total < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { { 0, 0 }, { 0, 0 }, 0, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || b.phase0 < 0)
			return -EINVAL;
		if (!ratio_ok(b.up, b.down) || !taps_ok(b.up, b.n_taps) || !job_table::inside(b.taps_offset, b.n_taps, n_taps_total))
			return -EINVAL;
		if (b.n_out < 0 || b.n_out > max_n_out(b.n, b.up, b.down, b.n_taps, b.phase0))
			return -EINVAL;
		const int f = tile_form(b.up, b.down, b.n_taps) ? 0 : 1;
		if (!job_table::inside(b.out_offset, b.n_out, out_capacity) || !job_table::add_groups(pl.groups[f], b.n_out, f ? kDirectOut : kTile))
			return -EINVAL;
		pl.jobs[f]++;
		pl.outputs += b.n_out;
		pl.macs += (long long)b.n_out * (b.n_taps / b.up);
		if (b.n_out > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + b.n_out));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

/* one more term of the continued fraction search: is up / down inside the terms and better than what is held? */
struct Best {
	int up, down, max_term;
	double err, r;
	void consider(long long u, long long d)
	{
		if (u < 1 || d < 1 || u > max_term || d > max_term)
			return;
		const double e = fabs((double)u / (double)d - r);
		if (up == 0 || e < err || (e == err && d < down)) {
			up = (int)u;
			down = (int)d;
			err = e;
		}
	}
};

} // namespace

extern "C" int fosphor_amd_resample_host(const float *iq, int64_t n_samples,
                                         const struct fosphor_amd_resample_job *jobs, int n_jobs,
                                         const float *taps, int64_t n_taps_total,
                                         float *out, int64_t out_capacity)
{
	if (!iq || !taps || !out || ((uintptr_t)iq & 7) || ((uintptr_t)taps & 3) || ((uintptr_t)out & 7))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs, n_taps_total, out_capacity, nullptr))
		return -EINVAL;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const int U = b.up, Q = b.n_taps / U;
		for (int64_t m = 0; m < b.n_out; m++) {
			const int64_t pos = b.phase0 + m * b.down;
			const int64_t first = (pos + U - 1) / U;
			const float *x = iq + 2 * (b.offset + first);
			const float *h = taps + b.taps_offset + (first * U - pos);
			double re = 0.0, im = 0.0;
			for (int q = 0; q < Q; q++) {
				const double hv = (double)h[(int64_t)q * U];
				re = mac(re, hv, (double)x[2 * q]);
				im = mac(im, hv, (double)x[2 * q + 1]);
			}
			out[2 * (b.out_offset + m)] = quiet((float)re);
			out[2 * (b.out_offset + m) + 1] = quiet((float)im);
		}
	}
	return 0;
}

extern "C" int fosphor_amd_resample_n_out(int32_t n, int up, int down, int n_taps, int64_t phase0)
{
	if (n < 0 || !ratio_ok(up, down) || !taps_ok(up, n_taps) || phase0 < 0)
		return -EINVAL;
	const int64_t n_out = max_n_out(n, up, down, n_taps, phase0);
	return n_out > 0x7fffffffLL ? -EINVAL : (int)n_out;
}

extern "C" int fosphor_amd_resample_design(int up, int down, int branch_taps, double guard, float *out)
{
	if (!out || !ratio_ok(up, down) || branch_taps < 1 || branch_taps > kMaxBranch || !(guard > 0.0) || !(guard <= 1.0))
		return -EINVAL;
	const int n_taps = branch_taps * up;
	const double pi = 3.14159265358979323846;
	const double fc = guard / (2.0 * (up > down ? up : down)), c = 0.5 * (n_taps - 1);
	std::vector<double> g(n_taps);
	for (int k = 0; 2 * k <= n_taps - 1; k++) {
		const double t = k - c;
		const double s = t == 0.0 ? 2.0 * fc : sin(2.0 * pi * fc * t) / (pi * t);
		const double w = n_taps == 1 ? 1.0 : 0.54 - 0.46 * cos(2.0 * pi * k / (n_taps - 1));
		g[k] = g[n_taps - 1 - k] = s * w;
	}
	double sum = 0.0;
	for (int k = 0; k < n_taps; k++)
		sum += g[k];
	for (int k = 0; k < n_taps; k++)
		out[k] = (float)((g[k] / sum) * up);
	return 0;
}

extern "C" int fosphor_amd_resample_ratio(double rate_in, double rate_out, int max_term, int *up, int *down, double *error)
{
	if (!up || !down || !(rate_in > 0.0) || !(rate_in < INFINITY) || !(rate_out > 0.0) || !(rate_out < INFINITY) || max_term < 1)
		return -EINVAL;
	const int cap = max_term < kMaxUp ? max_term : kMaxUp;
	const double r = rate_out / rate_in;
	Best best = { 0, 0, cap, 0.0, r };
	best.consider(1, 1);					/* the ends, for a ratio outside [1 / cap, cap] */
	best.consider(cap, 1);
	best.consider(1, cap);
	/* convergents h1 / k1 of r and, where the next one leaves the terms, the last semiconvergents that stay inside: every best
	 * approximation of r by a fraction of bounded terms is one of them.  At most 64 terms; cap <= 256 ends it far earlier. */
	long long h0 = 0, k0 = 1, h1 = 1, k1 = 0;
	double x = r;
	for (int step = 0; step < 64; step++) {
		const double fl = floor(x);
		if (!(fl < 1e9))				/* r beyond every term: the ends hold the answer */
			break;
		const long long a = (long long)fl;
		long long t = a;
		if (h1 > 0 && (cap - h0) / h1 < t)
			t = (cap - h0) / h1;
		if (k1 > 0 && (cap - k0) / k1 < t)
			t = (cap - k0) / k1;
		for (long long s = t > 1 ? t - 1 : 1; s <= t; s++)
			best.consider(h0 + s * h1, k0 + s * k1);
		if (t < a)
			break;
		const long long h2 = h0 + a * h1, k2 = k0 + a * k1;
		h0 = h1; k0 = k1; h1 = h2; k1 = k2;
		const double f = x - fl;
		if (!(f > 0.0))
			break;
		x = 1.0 / f;
	}
	*up = best.up;
	*down = best.down;
	if (error)
		*error = (rate_in * best.up / best.down - rate_out) / rate_out;
	return 0;
}

extern "C" int fosphor_amd_resample_from_extract(const struct fosphor_amd_extract_job *e, int up, int down, int n_taps,
                                                 struct fosphor_amd_resample_job *job)
{
	if (!e || !job || e->out_offset < 0 || e->n_out < 0)
		return -EINVAL;
	const int n_out = fosphor_amd_resample_n_out(e->n_out, up, down, n_taps, 0);
	if (n_out < 0)
		return -EINVAL;
	job->offset = e->out_offset;
	job->out_offset = 0;
	job->phase0 = 0;
	job->n = e->n_out;
	job->n_out = n_out;
	job->up = up;
	job->down = down;
	job->taps_offset = 0;
	job->n_taps = n_taps;
	return 0;
}

extern "C" int fosphor_amd_resample_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_RESAMPLE_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_RESAMPLE, FOSPHOR_AMD_RESAMPLE_STATS, stats);
}

extern "C" int fosphor_amd_resample(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                    const struct fosphor_amd_resample_job *jobs, int n_jobs,
                                    const float *d_taps, int64_t n_taps_total,
                                    void *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_taps || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_taps & 3) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, n_taps_total, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs that write something, TILE jobs first, and behind them the two prefixes */
	std::vector<Job> live[2];
	std::vector<uint32_t> prefix[2] = { std::vector<uint32_t>(1, 0u), std::vector<uint32_t>(1, 0u) };
	for (int i = 0; i < n_jobs; i++) {
		if (jobs[i].n_out == 0)
			continue;
		const int f = tile_form(jobs[i].up, jobs[i].down, jobs[i].n_taps) ? 0 : 1;
		prefix[f].push_back(prefix[f].back() + (uint32_t)job_table::groups_of(jobs[i].n_out, f ? kDirectOut : kTile));
		live[f].push_back(jobs[i]);
	}
	const job_table::Table table = job_table::pack_table(live, prefix, 0, 0);

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_RESAMPLE);
	stats[FOSPHOR_AMD_RESAMPLE_CALLS]++;
	stats[FOSPHOR_AMD_RESAMPLE_JOBS_TILE] += plan.jobs[0];
	stats[FOSPHOR_AMD_RESAMPLE_JOBS_DIRECT] += plan.jobs[1];
	stats[FOSPHOR_AMD_RESAMPLE_OUTPUTS] += plan.outputs;
	stats[FOSPHOR_AMD_RESAMPLE_MACS] += plan.macs;
	if (live[0].empty() && live[1].empty())
		return 0;						/* every job has n_out = 0 */

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_RESAMPLE, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.taps = d_taps;
	p.out = static_cast<float2 *>(d_out);
	int rv = 0;
	for (int f = 0; f < 2 && !rv; f++) {
		if (live[f].empty())
			continue;
		p.jobs = reinterpret_cast<const Job *>(d + table.jobs_at[f]);
		p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[f]);
		p.n_jobs = (int)live[f].size();
		rv = job_table::launch<kThreads>(f ? k_resample_direct : k_resample_tile, prefix[f].back(), st, p, stats,
		                                 f ? FOSPHOR_AMD_RESAMPLE_K_DIRECT : FOSPHOR_AMD_RESAMPLE_K_TILE);
	}
	return job_table::drain(st, rv);
}
