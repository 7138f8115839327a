/*
 * fosphor_measure.hip -- burst IQ reduced where it lies: power, edges, lag-1 product and moments per job (include/fosphor_amd_measure.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table, the
 * prefix of work-group counts and the SPLIT partials).
 *
 *   k_measure_wave     n <= kWaveMax: a wave owns a job, four jobs per work-group, no LDS.
 *   k_measure_split    longer jobs: a work-group of 256 lanes owns a chunk of kChunk samples of one job, which it finds in the
 *                      prefix (fosphor_jobs.h), and writes the chunk's partial record.
 *   k_measure_combine  a wave per SPLIT job folds the job's partials in ascending chunk order.
 * All three scan with one routine: a team of lanes (a wave, or the four waves of a work-group) strides a span of a job with
 * 16-byte loads, two samples per lane per load, split as split_span() of fosphor_jobs.h splits it, so no byte outside the job's
 * range is read; that header also has the table, the shared refusals and the tail of the call.  A sample needs two things of its neighbours:
 * above(m - 1) for the edge count and y[m + 1] for the lag-1 product.  Inside a pair both are at hand; between pairs they come from
 * the neighbouring lanes by a shuffle, and at the ends of a wave -- lane 0, and lane 63 or the team's last pair -- from one
 * 8-byte load of a sample the neighbouring wave reads anyway.  A lane sums its samples in ascending order; 64 partials meet by
 * xor-shuffles 32, 16, .. 1, which leave the same bits in every lane (a + b is b + a).  No atomics of any kind, no work-group
 * waits for another, every loop carries its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_measure.h"

namespace {

typedef struct fosphor_amd_measure_job Job;
typedef struct fosphor_amd_measure_record Record;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;				/* jobs of a WAVE work-group */
constexpr int kWaveMax = FOSPHOR_AMD_MEASURE_WAVE_MAX;
constexpr int kChunk = FOSPHOR_AMD_MEASURE_CHUNK;
constexpr int kNone = 0x7fffffff;				/* first_above of a partial without one, until the record is written */

static_assert(FOSPHOR_AMD_MEASURE_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 16, "the job table is built from it");
static_assert(sizeof(Record) == 96, "the record is 96 bytes");
static_assert(kChunk % 2 == 0 && kChunk > kWaveMax, "a chunk is whole pairs, and a SPLIT job has two samples at least");

inline __host__ __device__ int form_of(int n) { return n <= kWaveMax ? FOSPHOR_AMD_MEASURE_FORM_WAVE : FOSPHOR_AMD_MEASURE_FORM_SPLIT; }

/* a job on the device: where its record goes and, in the SPLIT form, where its partials begin */
struct DevJob {
	int64_t offset;
	int32_t n;
	float   threshold;
	int32_t record;			/* index into d_records */
	int32_t part0;			/* SPLIT: index of its first partial */
};

struct Params {
	const float2   *iq;
	const DevJob   *jobs;		/* the jobs of this form */
	const uint32_t *prefix;		/* SPLIT: [n_jobs + 1] work-groups before job j */
	Record         *parts;		/* SPLIT: one per work-group */
	Record         *records;
	int n_jobs;
};

/* What a lane, a wave, a chunk or a job has seen: Record's fields with first = kNone while nothing is above. */
struct Acc {
	int n_above, first, last, n_edges, peak_index;
	float peak;
	double s[8];			/* s_re, s_im, s_p, s_p2, s_zz_re, s_zz_im, r1_re, r1_im */
};

inline __host__ __device__ void acc_clear(Acc &a)
{
	a.n_above = 0; a.first = kNone; a.last = -1; a.n_edges = 0; a.peak_index = -1; a.peak = 0.0f;
	for (int i = 0; i < 8; i++)
		a.s[i] = 0.0;
}

/* Which NaN an operation on two NaNs hands on is the first operand's on the host's processor, and which operand is the first the
 * compiler decides anew in every build: IEEE 754 leaves it open.  The host statement pins it (kPin): a NaN operand comes through as
 * it is, the left one before the right one, so that a build of this source for one target gives the same bytes at every
 * optimisation level and under instrumentation.  The kernels (kPin false) are the plain operations: `r` alone. */
template <bool kPin, class T>
inline __host__ __device__ T pinned(T a, T b, T r)
{
	if constexpr (kPin) {
		if (a != a)
			return a;
		if (b != b)
			return b;
	}
	return r;
}

template <bool kPin, class T> inline __host__ __device__ T op_add(T a, T b) { return pinned<kPin>(a, b, a + b); }
template <bool kPin, class T> inline __host__ __device__ T op_sub(T a, T b) { return pinned<kPin>(a, b, a - b); }
template <bool kPin, class T> inline __host__ __device__ T op_mul(T a, T b) { return pinned<kPin>(a, b, a * b); }

/* rule 1: three rounded float32 operations (-ffp-contract=off: no fused multiply-add is formed) */
template <bool kPin = false>
inline __host__ __device__ float power(float2 y) { return op_add<kPin>(op_mul<kPin>(y.x, y.x), op_mul<kPin>(y.y, y.y)); }

/* sample m of the job.  prev_above: above(m - 1), false for m == 0; next: y[m + 1] where has_next.  Every product below is of two
 * float32 values in double, hence exact; the terms of s_zz_re and r1_* round once, in their one addition or subtraction. */
template <bool kPin = false>
inline __host__ __device__ void acc_take(Acc &a, int m, float2 y, float thr, bool prev_above, float2 next, bool has_next)
{
	const float p = power<kPin>(y);
	if (p >= thr) {
		a.n_above++;
		a.first = m < a.first ? m : a.first;
		a.last = m > a.last ? m : a.last;
		a.n_edges += prev_above ? 0 : 1;
	}
	if (p > a.peak || (a.peak_index < 0 && p == p)) {	/* m ascends: the smallest index of the largest p */
		a.peak = p;
		a.peak_index = m;
	}
	const double re = y.x, im = y.y, pd = p;
	a.s[0] = op_add<kPin>(a.s[0], re);
	a.s[1] = op_add<kPin>(a.s[1], im);
	a.s[2] = op_add<kPin>(a.s[2], pd);
	a.s[3] = op_add<kPin>(a.s[3], op_mul<kPin>(pd, pd));
	a.s[4] = op_add<kPin>(a.s[4], op_sub<kPin>(op_mul<kPin>(re, re), op_mul<kPin>(im, im)));
	a.s[5] = op_add<kPin>(a.s[5], op_mul<kPin>(op_mul<kPin>(2.0, re), im));
	if (has_next) {
		const double nr = next.x, ni = next.y;
		a.s[6] = op_add<kPin>(a.s[6], op_add<kPin>(op_mul<kPin>(nr, re), op_mul<kPin>(ni, im)));
		a.s[7] = op_add<kPin>(a.s[7], op_sub<kPin>(op_mul<kPin>(ni, re), op_mul<kPin>(nr, im)));
	}
}

/* a <- a then b: b's sums are added to a's.  The integers and the peak do not care about the order. */
inline __host__ __device__ void acc_fold(Acc &a, const Acc &b)
{
	a.n_above += b.n_above;
	a.first = b.first < a.first ? b.first : a.first;
	a.last = b.last > a.last ? b.last : a.last;
	a.n_edges += b.n_edges;
	if (b.peak_index >= 0 && (a.peak_index < 0 || b.peak > a.peak || (b.peak == a.peak && b.peak_index < a.peak_index))) {
		a.peak = b.peak;
		a.peak_index = b.peak_index;
	}
	for (int i = 0; i < 8; i++)
		a.s[i] += b.s[i];
}

inline __host__ __device__ void acc_store(const Acc &a, int n, Record *r)
{
	r->n_above = a.n_above;
	r->first_above = a.first == kNone ? -1 : a.first;
	r->last_above = a.last;
	r->n_edges = a.n_edges;
	r->peak_index = a.peak_index;
	r->peak_power = a.peak;
	r->s_re = a.s[0]; r->s_im = a.s[1]; r->s_p = a.s[2]; r->s_p2 = a.s[3];
	r->s_zz_re = a.s[4]; r->s_zz_im = a.s[5]; r->r1_re = a.s[6]; r->r1_im = a.s[7];
	r->n = n;
	r->form = form_of(n);
}

__device__ __forceinline__ void acc_load(Acc &a, const Record *r)
{
	a.n_above = r->n_above;
	a.first = r->first_above < 0 ? kNone : r->first_above;
	a.last = r->last_above;
	a.n_edges = r->n_edges;
	a.peak_index = r->peak_index;
	a.peak = r->peak_power;
	a.s[0] = r->s_re; a.s[1] = r->s_im; a.s[2] = r->s_p; a.s[3] = r->s_p2;
	a.s[4] = r->s_zz_re; a.s[5] = r->s_zz_im; a.s[6] = r->r1_re; a.s[7] = r->r1_im;
}

/* lane `from`'s Acc in every lane (from is the same in every lane) */
__device__ __forceinline__ Acc acc_of_lane(const Acc &a, int from)
{
	Acc b;
	b.n_above = __shfl(a.n_above, from);
	b.first = __shfl(a.first, from);
	b.last = __shfl(a.last, from);
	b.n_edges = __shfl(a.n_edges, from);
	b.peak_index = __shfl(a.peak_index, from);
	b.peak = __shfl(a.peak, from);
#pragma unroll
	for (int i = 0; i < 8; i++)
		b.s[i] = __shfl(a.s[i], from);			/* a double is two 32-bit shuffles */
	return b;
}

/* the 64 lanes' Accs into one, the same bits in every lane */
__device__ __forceinline__ void acc_wave_reduce(Acc &a)
{
#pragma unroll
	for (int d = 32; d; d >>= 1) {
		Acc b;
		b.n_above = __shfl_xor(a.n_above, d);
		b.first = __shfl_xor(a.first, d);
		b.last = __shfl_xor(a.last, d);
		b.n_edges = __shfl_xor(a.n_edges, d);
		b.peak_index = __shfl_xor(a.peak_index, d);
		b.peak = __shfl_xor(a.peak, d);
#pragma unroll
		for (int i = 0; i < 8; i++)
			b.s[i] = __shfl_xor(a.s[i], d);
		acc_fold(a, b);
	}
}

/* Samples [m0, m1) of the job at y (its sample 0; n samples), by a team of `team` lanes of which this is lane t; team is a multiple
 * of 64 and every lane of the team calls this with the same arguments.  Reads y[max(m0 - 1, 0) .. min(m1 + 1, n)) and nothing else. */
__device__ __forceinline__ void scan(Acc &a, const float2 *y, int n, int m0, int m1, float thr, int t, int team)
{
	const int lane = t & 63;
	const job_table::Span s = job_table::split_span(y + m0, m1 - m0);
	const int head = s.head, pairs = s.pairs;
	const int mb = m0 + head;						/* the first pair */
	const int mt = m0 + s.tail;						/* the single sample behind the last pair, if mt < m1 */

	if (t == 0 && head) {
		const bool prev = m0 > 0 && power(y[m0 - 1]) >= thr;
		const bool has_next = m0 + 1 < n;
		acc_take(a, m0, y[m0], thr, prev, has_next ? y[m0 + 1] : make_float2(0.0f, 0.0f), has_next);
	}
	for (int g0 = 0; g0 < pairs; g0 += team) {
		const int g = g0 + t;
		const bool act = g < pairs;
		const int m = mb + 2 * g;
		float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (act)
			q = *reinterpret_cast<const float4 *>(y + m);
		const float2 ya = make_float2(q.x, q.y), yb = make_float2(q.z, q.w);
		const bool above_a = power(ya) >= thr, above_b = power(yb) >= thr;
		/* the neighbours, from the lanes beside this one (every lane of the wave is here: the loop's bound is the team's) */
		bool prev = __shfl_up((int)above_b, 1) != 0;
		float2 next = make_float2(__shfl_down(ya.x, 1), __shfl_down(ya.y, 1));
		bool has_next = true;
		if (act) {
			if (lane == 0)
				prev = m > 0 && power(y[m - 1]) >= thr;
			if (lane == 63 || g == pairs - 1) {
				has_next = m + 2 < n;
				if (has_next)
					next = y[m + 2];
			}
			acc_take(a, m, ya, thr, prev, yb, true);
			acc_take(a, m + 1, yb, thr, above_a, next, has_next);
		}
	}
	if (t == 0 && mt < m1) {
		const bool prev = mt > 0 && power(y[mt - 1]) >= thr;
		const bool has_next = mt + 1 < n;
		acc_take(a, mt, y[mt], thr, prev, has_next ? y[mt + 1] : make_float2(0.0f, 0.0f), has_next);
	}
}

__global__ __launch_bounds__(kThreads)
void k_measure_wave(const Params p)
{
	const int lane = threadIdx.x & 63;
	const int j = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
	if (j >= p.n_jobs)						/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	Acc a;
	acc_clear(a);
	scan(a, p.iq + job.offset, job.n, 0, job.n, job.threshold, lane, 64);
	acc_wave_reduce(a);
	if (lane == 0)
		acc_store(a, job.n, p.records + job.record);
}

__global__ __launch_bounds__(kThreads)
void k_measure_split(const Params p)
{
	__shared__ Record s_part[kWaves];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* the chunk: c * kChunk < n by the prefix */
	const int m0 = c * kChunk;
	const int m1 = min(job.n - m0, kChunk) + m0;			/* no overflow: n - m0 >= 1 */
	Acc a;
	acc_clear(a);
	scan(a, p.iq + job.offset, job.n, m0, m1, job.threshold, tid, kThreads);
	acc_wave_reduce(a);
	if (lane == 0)
		acc_store(a, job.n, &s_part[wave]);
	__syncthreads();
	if (tid == 0) {
		for (int w = 1; w < kWaves; w++) {
			Acc b;
			acc_load(b, &s_part[w]);
			acc_fold(a, b);
		}
		acc_store(a, job.n, p.parts + job.part0 + c);
	}
}

__global__ __launch_bounds__(kThreads)
void k_measure_combine(const Params p)
{
	const int lane = threadIdx.x & 63;
	const int j = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
	if (j >= p.n_jobs)						/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const int chunks = (int)(p.prefix[j + 1] - p.prefix[j]);
	const Record *parts = p.parts + job.part0;
	Acc total;
	acc_clear(total);
	/* 64 partials at a time, one per lane, then folded in lane order: every lane holds the same running total */
	for (int c0 = 0; c0 < chunks; c0 += 64) {
		Acc mine;
		acc_clear(mine);
		if (c0 + lane < chunks)
			acc_load(mine, parts + c0 + lane);
		const int k1 = min(64, chunks - c0);
		for (int k = 0; k < k1; k++) {
			const Acc b = acc_of_lane(mine, k);
			acc_fold(total, b);
		}
	}
	if (lane == 0)
		acc_store(total, job.n, p.records + job.record);
}

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_MEASURE_MAX_JOBS) || n_samples < 0)
		return -EINVAL;
	long long chunks = 0;				/* of the SPLIT jobs; the WAVE jobs are kWaves to a work-group: MAX_JOBS / kWaves at most */
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || b.threshold != b.threshold)
			return -EINVAL;
		if (form_of(b.n) == FOSPHOR_AMD_MEASURE_FORM_SPLIT && !job_table::add_groups(chunks, b.n, kChunk))
			return -EINVAL;
	}
	return 0;
}

} // namespace

extern "C" int fosphor_amd_measure_host(const float *iq, int64_t n_samples, const struct fosphor_amd_measure_job *jobs,
                                        int n_jobs, struct fosphor_amd_measure_record *records)
{
	if (!iq || !records || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs))
		return -EINVAL;
	for (int i = 0; i < n_jobs; i++) {
		const float *y = iq + 2 * jobs[i].offset;
		const int n = jobs[i].n;
		const float thr = jobs[i].threshold;
		Acc a;
		acc_clear(a);
		bool prev = false;
		for (int m = 0; m < n; m++) {
			const float2 v = make_float2(y[2 * m], y[2 * m + 1]);
			const bool has_next = m + 1 < n;
			acc_take<true>(a, m, v, thr, prev, has_next ? make_float2(y[2 * m + 2], y[2 * m + 3]) : make_float2(0.0f, 0.0f), has_next);
			prev = power<true>(v) >= thr;
		}
		acc_store(a, n, &records[i]);
	}
	return 0;
}

extern "C" int fosphor_amd_measure_from_extract(const struct fosphor_amd_extract_job *e, float threshold,
                                                struct fosphor_amd_measure_job *job)
{
	if (!e || !job || threshold != threshold || e->out_offset < 0 || e->n_out < 0)
		return -EINVAL;
	job->offset = e->out_offset;
	job->n = e->n_out;
	job->threshold = threshold;
	return 0;
}

extern "C" int fosphor_amd_measure_derive(const struct fosphor_amd_measure_record *r, double sample_rate,
                                          struct fosphor_amd_measure_values *v)
{
	if (!r || !v || !(sample_rate > 0.0) || !(sample_rate < INFINITY))
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	if (r->n <= 0)
		return 0;
	const double n = r->n, sp = r->s_p, pi = 3.14159265358979323846;
	v->mean_power = sp / n;
	v->peak_db = r->peak_power != 0.0f ? 10.0 * log10((double)r->peak_power) : 0.0;
	v->freq_offset = atan2(r->r1_im, r->r1_re) / (2.0 * pi) * sample_rate;
	if (sp != 0.0) {
		v->mean_db = 10.0 * log10(v->mean_power);
		v->papr_db = v->peak_db - v->mean_db;
		v->coherence = hypot(r->r1_re, r->r1_im) / sp;
		v->kurtosis = (r->s_p2 / n) / (v->mean_power * v->mean_power);
		v->circularity = hypot(r->s_zz_re, r->s_zz_im) / sp;
		v->dc_fraction = (r->s_re * r->s_re + r->s_im * r->s_im) / (n * sp);
	}
	if (r->n_above > 0) {
		v->duty = r->n_above / n;
		v->rise = r->first_above / sample_rate;
		v->fall = (r->last_above + 1.0) / sample_rate;
		v->pulses = r->n_edges;
	}
	return 0;
}

extern "C" int fosphor_amd_measure_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_MEASURE_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_MEASURE, FOSPHOR_AMD_MEASURE_STATS, stats);
}

extern "C" int fosphor_amd_measure(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                   const struct fosphor_amd_measure_job *jobs, int n_jobs,
                                   struct fosphor_amd_measure_record *d_records)
{
	if (!self || !d_iq || !jobs || !d_records)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs))
		return -EINVAL;

	/* the table: WAVE jobs, SPLIT jobs, the SPLIT prefix; behind it the SPLIT partials */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2];
	std::vector<uint32_t> &chunks = prefix[FOSPHOR_AMD_MEASURE_FORM_SPLIT];
	chunks.assign(1, 0u);
	long long samples = 0;
	for (int i = 0; i < n_jobs; i++) {
		const int f = form_of(jobs[i].n);
		DevJob d;
		d.offset = jobs[i].offset;
		d.n = jobs[i].n;
		d.threshold = jobs[i].threshold;
		d.record = i;
		d.part0 = 0;
		if (f == FOSPHOR_AMD_MEASURE_FORM_SPLIT) {
			d.part0 = (int32_t)chunks.back();
			chunks.push_back(chunks.back() + (uint32_t)job_table::groups_of(jobs[i].n, kChunk));
		}
		form[f].push_back(d);
		samples += jobs[i].n;
	}
	const job_table::Table table = job_table::pack_table(form, prefix, chunks.back(), sizeof(Record));

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_MEASURE);
	stats[FOSPHOR_AMD_MEASURE_CALLS]++;
	stats[FOSPHOR_AMD_MEASURE_JOBS_WAVE] += (long long)form[0].size();
	stats[FOSPHOR_AMD_MEASURE_JOBS_SPLIT] += (long long)form[1].size();
	stats[FOSPHOR_AMD_MEASURE_SAMPLES] += samples;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_MEASURE, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[FOSPHOR_AMD_MEASURE_FORM_SPLIT]);
	p.parts = reinterpret_cast<Record *>(d + table.parts_at);
	p.records = d_records;
	int rv = 0;
	if (!form[0].empty()) {
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
		p.n_jobs = (int)form[0].size();
		rv = job_table::launch<kThreads>(k_measure_wave, (unsigned)job_table::groups_of(p.n_jobs, kWaves), st, p, stats,
		                                 FOSPHOR_AMD_MEASURE_K_WAVE);
	}
	if (!form[1].empty() && !rv) {
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[1]);
		p.n_jobs = (int)form[1].size();
		rv = job_table::launch<kThreads>(k_measure_split, chunks.back(), st, p, stats, FOSPHOR_AMD_MEASURE_K_SPLIT);
		if (!rv)
			rv = job_table::launch<kThreads>(k_measure_combine, (unsigned)job_table::groups_of(p.n_jobs, kWaves), st, p, stats,
			                                 FOSPHOR_AMD_MEASURE_K_COMBINE);
	}
	return job_table::drain(st, rv);
}
