/*
 * fosphor_demod.hip -- burst IQ demodulated where it lies: power, phase and FM traces per job (include/fosphor_amd_demod.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table and the
 * prefixes of work-group counts).
 *
 *   k_demod_direct  L = 1: a work-group of 256 lanes owns kTile consecutive trace values of one job, which it finds in the prefix
 *                   (fosphor_jobs.h).  It brings their samples into LDS, computes value i, i + 256, .. per lane and stores 4 bytes
 *                   per lane, consecutive lanes to consecutive floats.
 *   k_demod_avg     L > 1: a work-group owns kTile / L outputs.  The same load; the (kTile / L) * L trace values are computed one
 *                   per lane into LDS rows of L floats, row stride L | 1 (odd: the 32 lanes of a half wave that walk 32 rows read
 *                   32 banks); then one lane per output adds its row in ascending order in double.
 * Both load their span with load_span() of fosphor_jobs.h, which also has the table, the shared refusals and the tail of the call.
 * An FM span is one sample longer than its trace values: v[m] needs y[m + 1], and n_trace = n - 1 says the job has it.
 * Every trace value is computed by trace_value() and every output by dump(), on the device and in fosphor_amd_demod_host alike.
 * No atomics of any kind, no work-group waits for another, every loop carries its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_demod.h"

namespace {

typedef struct fosphor_amd_demod_job Job;

constexpr int kThreads = 256;
constexpr int kTile = FOSPHOR_AMD_DEMOD_TILE;
constexpr int kMaxAvg = FOSPHOR_AMD_DEMOD_MAX_AVG;
constexpr int kImage = kTile + 2;				/* a tile's samples, FM's one more, and the slot before an odd start */
constexpr int kRows = kTile / 2 * 3;				/* (kTile / L) * (L | 1) is largest at L = 2 */

static_assert(FOSPHOR_AMD_DEMOD_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 32, "the job is 32 bytes");
static_assert(kTile % 2 == 0 && kMaxAvg <= kTile, "a tile holds an output of every L");

inline __host__ __device__ int per_group(int avg) { return avg == 1 ? kTile : kTile / avg; }	/* outputs of a work-group */

inline int n_trace_of(int mode, int n) { return mode == FOSPHOR_AMD_DEMOD_FM ? (n > 0 ? n - 1 : 0) : n; }

inline bool mode_ok(int mode) { return mode >= FOSPHOR_AMD_DEMOD_POWER && mode <= FOSPHOR_AMD_DEMOD_FM; }

/* a job that writes something, on the device */
struct DevJob {
	int64_t offset;
	int64_t out_offset;
	int32_t n_out;
	int32_t mode;
	int32_t avg;
	int32_t pad;
};

struct Params {
	const float2   *iq;
	const DevJob   *jobs;		/* the jobs of this form with n_out > 0 */
	const uint32_t *prefix;		/* [n_jobs + 1] work-groups before job j */
	float          *out;
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }		/* rule 3: one NaN */

/* rule 1: three rounded float32 operations (-ffp-contract=off: no fused multiply-add is formed) */
inline __host__ __device__ float power(float2 y) { return quiet((y.x * y.x) + (y.y * y.y)); }

/* trace value m of a job in `mode` from y[m] and, for FM, y[m + 1] */
inline __host__ __device__ float trace_value(int mode, float2 y0, float2 y1)
{
	if (mode == FOSPHOR_AMD_DEMOD_POWER)
		return power(y0);
	if (mode == FOSPHOR_AMD_DEMOD_PHASE)
		return fosphor_amd_atan2_turns((double)y0.y, (double)y0.x);
	const double re0 = y0.x, im0 = y0.y, re1 = y1.x, im1 = y1.y;	/* the products are exact in double: each component rounds once */
	const double zr = re1 * re0 + im1 * im0;
	const double zi = im1 * re0 - re1 * im0;
	return fosphor_amd_atan2_turns(zi, zr);
}

/* rule 3: L consecutive trace values to one output (L > 1) */
inline __host__ __device__ float dump(const float *v, int L)
{
	double S = 0.0;
	for (int k = 0; k < L; k++)
		S += (double)v[k];
	return quiet((float)(S / (double)L));
}

__global__ __launch_bounds__(kThreads)
void k_demod_direct(const Params p)
{
	__shared__ __align__(16) float2 s_y[kImage];
	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* the tile: c * kTile < n_out by the prefix */
	const int t0 = c * kTile;
	const int count = min(job.n_out - t0, kTile);			/* 1 .. kTile trace values */
	const int fm = job.mode == FOSPHOR_AMD_DEMOD_FM;
	const int at = job_table::load_span<kThreads>(s_y, p.iq + job.offset + t0, count + fm, tid);
	__syncthreads();
	float *out = p.out + job.out_offset + t0;
	const float2 *y = s_y + at;
	if (job.mode == FOSPHOR_AMD_DEMOD_POWER) {
		for (int i = tid; i < count; i += kThreads)
			out[i] = power(y[i]);
	} else if (job.mode == FOSPHOR_AMD_DEMOD_PHASE) {
		for (int i = tid; i < count; i += kThreads)
			out[i] = trace_value(FOSPHOR_AMD_DEMOD_PHASE, y[i], y[i]);
	} else {
		for (int i = tid; i < count; i += kThreads)
			out[i] = trace_value(FOSPHOR_AMD_DEMOD_FM, y[i], y[i + 1]);	/* i + 1 <= count: loaded */
	}
}

__global__ __launch_bounds__(kThreads)
void k_demod_avg(const Params p)
{
	__shared__ __align__(16) float2 s_y[kImage];
	__shared__ float s_v[kRows];
	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int L = job.avg;						/* 2 .. kMaxAvg */
	const int per = kTile / L;
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* c * per < n_out by the prefix */
	const int o0 = c * per;
	const int outs = min(job.n_out - o0, per);			/* 1 .. per outputs */
	const int count = outs * L;					/* <= kTile trace values, from t0 = o0 * L <= n_trace - count */
	const int fm = job.mode == FOSPHOR_AMD_DEMOD_FM;
	const int at = job_table::load_span<kThreads>(s_y, p.iq + job.offset + (int64_t)o0 * L, count + fm, tid);
	__syncthreads();
	const float2 *y = s_y + at;
	const int stride = L | 1;
	for (int i = tid; i < count; i += kThreads) {
		const int row = i / L;
		s_v[row * stride + (i - row * L)] = trace_value(job.mode, y[i], y[i + fm]);	/* row < outs: below kRows */
	}
	__syncthreads();
	float *out = p.out + job.out_offset + o0;
	for (int o = tid; o < outs; o += kThreads)
		out[o] = dump(s_v + o * stride, L);
}

struct Plan {
	long long groups[2], jobs[2], samples, outputs;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_DEMOD_MAX_JOBS) || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { { 0, 0 }, { 0, 0 }, 0, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples))
			return -EINVAL;
		if (!mode_ok(b.mode) || b.avg < 1 || b.avg > kMaxAvg || b.reserved != 0)
			return -EINVAL;
		const int n_out = n_trace_of(b.mode, b.n) / b.avg;
		const int f = b.avg > 1;
		if (!job_table::inside(b.out_offset, n_out, out_capacity) || !job_table::add_groups(pl.groups[f], n_out, per_group(b.avg)))
			return -EINVAL;
		pl.jobs[f]++;
		pl.samples += b.n;
		pl.outputs += n_out;
		if (n_out > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + n_out));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

} // namespace

extern "C" int fosphor_amd_demod_host(const float *iq, int64_t n_samples, const struct fosphor_amd_demod_job *jobs, int n_jobs,
                                      float *out, int64_t out_capacity)
{
	if (!iq || !out || ((uintptr_t)iq & 7) || ((uintptr_t)out & 3))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, nullptr))
		return -EINVAL;
	std::vector<float> v(kMaxAvg);
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const float *y = iq + 2 * b.offset;
		const int L = b.avg, fm = b.mode == FOSPHOR_AMD_DEMOD_FM;
		const int n_out = n_trace_of(b.mode, b.n) / L;
		float *o = out + b.out_offset;
		for (int j = 0; j < n_out; j++) {
			for (int k = 0; k < L; k++) {
				const int64_t m = (int64_t)j * L + k;
				v[k] = trace_value(b.mode, make_float2(y[2 * m], y[2 * m + 1]),
				                   make_float2(y[2 * (m + fm)], y[2 * (m + fm) + 1]));
			}
			o[j] = L == 1 ? v[0] : dump(v.data(), L);
		}
	}
	return 0;
}

extern "C" int fosphor_amd_demod_n_out(int mode, int32_t n, int avg)
{
	if (!mode_ok(mode) || n < 0 || avg < 1 || avg > kMaxAvg)
		return -EINVAL;
	return n_trace_of(mode, n) / avg;
}

extern "C" int fosphor_amd_demod_from_extract(const struct fosphor_amd_extract_job *e, int mode, int avg,
                                              struct fosphor_amd_demod_job *job)
{
	if (!e || !job || e->out_offset < 0 || e->n_out < 0 || !mode_ok(mode) || avg < 1 || avg > kMaxAvg)
		return -EINVAL;
	job->offset = e->out_offset;
	job->out_offset = 0;
	job->n = e->n_out;
	job->mode = mode;
	job->avg = avg;
	job->reserved = 0;
	return 0;
}

extern "C" float fosphor_amd_demod_atan2_turns(double y, double x)
{
	return fosphor_amd_atan2_turns(y, x);
}

extern "C" int fosphor_amd_demod_atan2_turns_n(const double *y, const double *x, int64_t n, float *out)
{
	if (!y || !x || !out || n < 0)
		return -EINVAL;
	for (int64_t i = 0; i < n; i++)
		out[i] = fosphor_amd_atan2_turns(y[i], x[i]);
	return 0;
}

extern "C" int fosphor_amd_demod_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DEMOD_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_DEMOD, FOSPHOR_AMD_DEMOD_STATS, stats);
}

extern "C" int fosphor_amd_demod(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                 const struct fosphor_amd_demod_job *jobs, int n_jobs,
                                 float *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: DIRECT and AVG jobs, their prefixes; only jobs that write something */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2] = { std::vector<uint32_t>(1, 0u), std::vector<uint32_t>(1, 0u) };
	for (int i = 0; i < n_jobs; i++) {
		const int n_out = n_trace_of(jobs[i].mode, jobs[i].n) / jobs[i].avg;
		if (n_out == 0)
			continue;
		const int f = jobs[i].avg > 1;
		DevJob d;
		d.offset = jobs[i].offset;
		d.out_offset = jobs[i].out_offset;
		d.n_out = n_out;
		d.mode = jobs[i].mode;
		d.avg = jobs[i].avg;
		d.pad = 0;
		form[f].push_back(d);
		prefix[f].push_back(prefix[f].back() + (uint32_t)job_table::groups_of(n_out, per_group(jobs[i].avg)));
	}
	const job_table::Table table = job_table::pack_table(form, prefix, 0, 0);

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_DEMOD);
	stats[FOSPHOR_AMD_DEMOD_CALLS]++;
	stats[FOSPHOR_AMD_DEMOD_JOBS_DIRECT] += plan.jobs[0];
	stats[FOSPHOR_AMD_DEMOD_JOBS_AVG] += plan.jobs[1];
	stats[FOSPHOR_AMD_DEMOD_SAMPLES] += plan.samples;
	stats[FOSPHOR_AMD_DEMOD_OUTPUTS] += plan.outputs;
	if (form[0].empty() && form[1].empty())
		return 0;						/* no job writes anything */

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_DEMOD, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = d_out;
	int rv = 0;
	for (int f = 0; f < 2 && !rv; f++) {
		if (form[f].empty())
			continue;
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[f]);
		p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[f]);
		p.n_jobs = (int)form[f].size();
		rv = job_table::launch<kThreads>(f ? k_demod_avg : k_demod_direct, prefix[f].back(), st, p, stats,
		                                 f ? FOSPHOR_AMD_DEMOD_K_AVG : FOSPHOR_AMD_DEMOD_K_DIRECT);
	}
	return job_table::drain(st, rv);
}
