/*
 * fosphor_demod.hip -- burst IQ demodulated where it lies: power, phase and FM traces per job (include/fosphor_amd_demod.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table and the
 * prefixes of work-group counts).
 *
 *   k_demod_direct  L = 1: a work-group of 256 lanes owns kTile consecutive trace values of one job, which it finds by a bounded
 *                   binary search of the prefix (13 steps cover 4096 jobs).  It brings their samples into LDS, computes value
 *                   i, i + 256, .. per lane and stores 4 bytes per lane, consecutive lanes to consecutive floats.
 *   k_demod_avg     L > 1: a work-group owns kTile / L outputs.  The same load; the (kTile / L) * L trace values are computed one
 *                   per lane into LDS rows of L floats, row stride L | 1 (odd: the 32 lanes of a half wave that walk 32 rows read
 *                   32 banks); then one lane per output adds its row in ascending order in double.
 * Both load with one routine: 16-byte loads, a pair of samples per lane, from the first 16-byte boundary of the span on; the single
 * samples before it and behind the last whole pair go one by one, so no byte outside the job's range is read.  A pair lands on a
 * 16-byte boundary of the LDS image too (the image begins one slot in when the span begins off the boundary).  An FM span is one
 * sample longer than its trace values: v[m] needs y[m + 1], and n_trace = n - 1 says the job has it.
 * Every trace value is computed by trace_value() and every output by dump(), on the device and in fosphor_amd_demod_host alike.
 * No atomics of any kind, no work-group waits for another, every loop carries its bound in its header.
 */
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/fosphor_amd.h"
#include "../../include/fosphor_amd_demod.h"

/* accessors implemented next to struct fosphor (fosphor_api.cpp) */
extern "C" long long *fosphor_amd_priv_demod_stats(struct fosphor *self);
extern "C" int fosphor_amd_priv_demod_scratch(struct fosphor *self, size_t bytes, void **d_scratch);

namespace {

typedef struct fosphor_amd_demod_job Job;

constexpr int kThreads = 256;
constexpr int kTile = FOSPHOR_AMD_DEMOD_TILE;
constexpr int kMaxAvg = FOSPHOR_AMD_DEMOD_MAX_AVG;
constexpr int kImage = kTile + 2;				/* a tile's samples, FM's one more, and the slot before an odd start */
constexpr int kRows = kTile / 2 * 3;				/* (kTile / L) * (L | 1) is largest at L = 2 */
constexpr int kSearchSteps = 13;				/* 2^12 = MAX_JOBS */
constexpr long long kMaxGroups = 0x7fffffffLL;

static_assert(FOSPHOR_AMD_DEMOD_MAX_JOBS <= (1 << (kSearchSteps - 1)), "the job search is bounded");
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

/* Samples y[0 .. count) into the image, by the 256 lanes of a work-group of which this is lane t; 1 <= count <= kTile + 1.
 * -> the image index of y[0] (0 or 1).  Reads y[0 .. count) and nothing else. */
__device__ __forceinline__ int load_span(float2 *image, const float2 *y, int count, int t)
{
	const int head = min(count, (int)(((uintptr_t)y >> 3) & 1));	/* 0 or 1 sample before the 16-byte boundary */
	const int pairs = (count - head) >> 1;
	const int tail = head + 2 * pairs;					/* the single sample behind the last pair, if tail < count */
	if (t == 0 && head)
		image[1] = y[0];
	for (int g = t; g < pairs; g += kThreads)
		*reinterpret_cast<float4 *>(image + 2 * head + 2 * g) = *reinterpret_cast<const float4 *>(y + head + 2 * g);
	if (t == kThreads - 1 && tail < count)
		image[head + tail] = y[tail];
	return head;
}

/* the job of work-group g: the largest j with prefix[j] <= g (every job of the table has a work-group) */
__device__ __forceinline__ int find_job(const uint32_t *prefix, int n_jobs, uint32_t g)
{
	int lo = 0, hi = n_jobs;
	for (int step = 0; step < kSearchSteps && hi - lo > 1; step++) {
		const int mid = (lo + hi) >> 1;
		if (prefix[mid] <= g)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__global__ __launch_bounds__(kThreads)
void k_demod_direct(const Params p)
{
	__shared__ __align__(16) float2 s_y[kImage];
	const int tid = threadIdx.x;
	const int j = find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* the tile: c * kTile < n_out by the prefix */
	const int t0 = c * kTile;
	const int count = min(job.n_out - t0, kTile);			/* 1 .. kTile trace values */
	const int fm = job.mode == FOSPHOR_AMD_DEMOD_FM;
	const int at = load_span(s_y, p.iq + job.offset + t0, count + fm, tid);
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
	const int j = find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int L = job.avg;						/* 2 .. kMaxAvg */
	const int per = kTile / L;
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* c * per < n_out by the prefix */
	const int o0 = c * per;
	const int outs = min(job.n_out - o0, per);			/* 1 .. per outputs */
	const int count = outs * L;					/* <= kTile trace values, from t0 = o0 * L <= n_trace - count */
	const int fm = job.mode == FOSPHOR_AMD_DEMOD_FM;
	const int at = load_span(s_y, p.iq + job.offset + (int64_t)o0 * L, count + fm, tid);
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
	if (!jobs || n_jobs < 1 || n_jobs > FOSPHOR_AMD_DEMOD_MAX_JOBS || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { { 0, 0 }, { 0, 0 }, 0, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (b.offset < 0 || b.n < 0 || b.offset > n_samples || b.n > n_samples - b.offset)
			return -EINVAL;
		if (!mode_ok(b.mode) || b.avg < 1 || b.avg > kMaxAvg || b.reserved != 0)
			return -EINVAL;
		const int n_out = n_trace_of(b.mode, b.n) / b.avg;
		if (b.out_offset < 0 || b.out_offset > out_capacity || n_out > out_capacity - b.out_offset)
			return -EINVAL;
		const int f = b.avg > 1;
		const int per = per_group(b.avg);
		pl.groups[f] += ((long long)n_out + per - 1) / per;
		pl.jobs[f]++;
		pl.samples += b.n;
		pl.outputs += n_out;
		if (n_out > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + n_out));
	}
	if (pl.groups[0] > kMaxGroups || pl.groups[1] > kMaxGroups)
		return -EINVAL;
	std::sort(ranges.begin(), ranges.end());
	for (size_t i = 1; i < ranges.size(); i++)
		if (ranges[i].first < ranges[i - 1].second)
			return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

int launch_ok(void) { return hipGetLastError() == hipSuccess ? 0 : -EIO; }

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
	if (!self)
		return -EINVAL;
	if (stats)
		for (int i = 0; i < FOSPHOR_AMD_DEMOD_STATS; i++)
			stats[i] = fosphor_amd_priv_demod_stats(self)[i];
	return 0;
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

	/* the table: DIRECT jobs, AVG jobs, the DIRECT prefix, the AVG prefix; only jobs that write something */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2] = { std::vector<uint32_t>(1, 0u), std::vector<uint32_t>(1, 0u) };
	for (int i = 0; i < n_jobs; i++) {
		const int n_out = n_trace_of(jobs[i].mode, jobs[i].n) / jobs[i].avg;
		if (n_out == 0)
			continue;
		const int f = jobs[i].avg > 1;
		const int per = per_group(jobs[i].avg);
		DevJob d;
		d.offset = jobs[i].offset;
		d.out_offset = jobs[i].out_offset;
		d.n_out = n_out;
		d.mode = jobs[i].mode;
		d.avg = jobs[i].avg;
		d.pad = 0;
		form[f].push_back(d);
		prefix[f].push_back(prefix[f].back() + (uint32_t)(((long long)n_out + per - 1) / per));
	}
	const size_t n_form[2] = { form[0].size(), form[1].size() };
	const size_t job_bytes = sizeof(DevJob) * (n_form[0] + n_form[1]);
	const size_t bytes = job_bytes + sizeof(uint32_t) * (prefix[0].size() + prefix[1].size());
	std::vector<uint8_t> table(bytes);
	for (int f = 0; f < 2; f++) {
		if (n_form[f])
			memcpy(table.data() + (f ? sizeof(DevJob) * n_form[0] : 0), form[f].data(), sizeof(DevJob) * n_form[f]);
		memcpy(table.data() + job_bytes + (f ? sizeof(uint32_t) * prefix[0].size() : 0), prefix[f].data(),
		       sizeof(uint32_t) * prefix[f].size());
	}

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_demod_stats(self);
	stats[FOSPHOR_AMD_DEMOD_CALLS]++;
	stats[FOSPHOR_AMD_DEMOD_JOBS_DIRECT] += plan.jobs[0];
	stats[FOSPHOR_AMD_DEMOD_JOBS_AVG] += plan.jobs[1];
	stats[FOSPHOR_AMD_DEMOD_SAMPLES] += plan.samples;
	stats[FOSPHOR_AMD_DEMOD_OUTPUTS] += plan.outputs;
	if (!n_form[0] && !n_form[1])
		return 0;						/* no job writes anything */

	void *d;
	if (fosphor_amd_priv_demod_scratch(self, bytes, &d))
		return -EIO;
	const hipStream_t st = (hipStream_t)fosphor_amd_stream(self);
	if (hipMemcpyAsync(d, table.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess)
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = d_out;
	int rv = 0;
	if (n_form[0]) {
		p.jobs = static_cast<const DevJob *>(d);
		p.prefix = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(d) + job_bytes);
		p.n_jobs = (int)n_form[0];
		hipLaunchKernelGGL(k_demod_direct, dim3(prefix[0].back()), dim3(kThreads), 0, st, p);
		if (!(rv = launch_ok()))
			stats[FOSPHOR_AMD_DEMOD_K_DIRECT]++;
	}
	if (n_form[1] && !rv) {
		p.jobs = static_cast<const DevJob *>(d) + n_form[0];
		p.prefix = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(d) + job_bytes) + prefix[0].size();
		p.n_jobs = (int)n_form[1];
		hipLaunchKernelGGL(k_demod_avg, dim3(prefix[1].back()), dim3(kThreads), 0, st, p);
		if (!(rv = launch_ok()))
			stats[FOSPHOR_AMD_DEMOD_K_AVG]++;
	}
	if (hipStreamSynchronize(st) != hipSuccess)			/* the table on the host lives until here */
		return -EIO;
	return rv;
}
