/*
 * fosphor_correlate.hip -- burst IQ correlated against templates where it lies: matched filter, peak, lags above a threshold
 * (include/fosphor_amd_correlate.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote) and templates, in a file of its own: nothing here
 * is on the process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table,
 * the prefix of work-group counts and the tile partials).
 *
 *   k_correlate_tile     a work-group of 256 lanes owns kTile consecutive lags of one job, which it finds in the prefix
 *                        (fosphor_jobs.h).  It brings y[k0 .. k0 + lags + T - 1) and the template into LDS;
 *                        lane i owns lags i, i + 256, i + 512, i + 768: at step i of the template the 64 lanes of a wave read 64
 *                        consecutive samples (no bank conflict) and one template value (a broadcast), and each lane issues
 *                        26 fused multiply-adds in double for its 5 LDS reads.  Then rho, the trace, and the tile's partial.
 *   k_correlate_combine  a wave per job folds the job's partials and writes the record; lane l takes tiles l, l + 64, ...  Every
 *                        folded quantity is an integer, a minimum or a maximum, so the order of the fold does not matter; the
 *                        seam between tile c - 1 and tile c is settled by the lane that owns tile c.
 * Both spans are loaded by load_span() of fosphor_jobs.h, which also has the table, the shared refusals and the tail of the call.
 * Every lag is computed by the operations of window() and rho_of(), on the device and in fosphor_amd_correlate_host alike.
 * No atomics of any kind, no work-group waits for another, every loop carries its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_correlate.h"

namespace {

typedef struct fosphor_amd_correlate_job Job;
typedef struct fosphor_amd_correlate_record Record;

/* What LDS holds: doubles, converted once at the load, 16 bytes a sample.  float2, converted at each read (10 conversions beside
 * the 26 multiply-adds of a template step, twice the work-groups on a CU), was built and timed too: 6 % faster at T = 32, 12 %
 * slower at T = 128 and 19 % slower at T = 1024 (profiles/r15_correlate.md).  The two differ in this typedef alone. */
typedef double2 LdsSample;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = FOSPHOR_AMD_CORRELATE_TILE;
constexpr int kSlots = kTile / kThreads;			/* lags of a lane */
constexpr int kMaxTpl = FOSPHOR_AMD_CORRELATE_MAX_TPL;
constexpr int kImageY = kTile + kMaxTpl;			/* a tile's span, kTile + T - 1 samples, and the slot before an odd start */
constexpr int kImageT = kMaxTpl + 2;
constexpr int kNone = 0x7fffffff;				/* first_above of a partial without one, until the record is written */

static_assert(FOSPHOR_AMD_CORRELATE_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 40, "the job is 40 bytes");
static_assert(sizeof(Record) == 64, "the record is 64 bytes");
static_assert(kTile % kThreads == 0 && kSlots == 4, "four lags a lane");
static_assert(sizeof(LdsSample) * kImageY >= sizeof(float) * 2 * kTile, "the TRACE_C floats of a tile fit where its samples were");

inline bool trace_ok(int trace) { return trace >= FOSPHOR_AMD_CORRELATE_TRACE_NONE && trace <= FOSPHOR_AMD_CORRELATE_TRACE_C; }

inline int n_lags_of(int n, int T) { return n >= T ? n - T + 1 : 0; }

inline int64_t n_out_of(int trace, int n_lags) { return (int64_t)n_lags * trace; }	/* NONE 0, RHO 1, C 2 */

/* a job on the device; its record is d_records[j] and its partials begin at prefix[j] */
struct DevJob {
	int64_t offset;
	int64_t out_offset;
	int64_t tpl_offset;
	int32_t n_lags;
	int32_t tpl_len;
	int32_t trace;
	float   threshold;
};

/* what a tile says about its lags (64 bytes); lags are relative to the job */
struct Part {
	int32_t n_above, first, last, n_edges;	/* first = kNone when none; n_edges counts the tile's first lag as an edge if it is above */
	int32_t flags;				/* 1: the tile's first lag is above, 2: its last lag is */
	int32_t peak_lag;
	float   peak_rho;
	int32_t pad;
	double  c_re, c_im, energy;		/* at peak_lag */
	double  tpl_energy;
};

static_assert(sizeof(Part) == 64, "a partial is 64 bytes");

struct Params {
	const float2   *iq;
	const float2   *tpl;
	const DevJob   *jobs;
	const uint32_t *prefix;		/* [n_jobs + 1] work-groups before job j */
	Part           *parts;		/* one per work-group of the tile kernel */
	Record         *records;
	float          *out;
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }		/* rule 2: one NaN */
inline __host__ __device__ double quiet(double v) { return v != v ? (double)NAN : v; }

/* rule 1: s + a * b with a * b exact, one rounding either way */
inline __host__ __device__ double mac(double s, double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_fma(a, b, s);
#else
	return s + a * b;
#endif
}

/* rule 1: step i of a lag, in the pinned order */
inline __host__ __device__ void step(double &cre, double &cim, double &E, double yr, double yi, double tr, double ti)
{
	cre = mac(cre, yr, tr);
	cre = mac(cre, yi, ti);
	cim = mac(cim, yi, tr);
	cim = mac(cim, -yr, ti);		/* cim - yr * ti: the product is exact, its sign costs nothing */
	E = mac(E, yr, yr);
	E = mac(E, yi, yi);
}

/* rule 1 on the host: a whole window */
inline void window(const float *y, const float *t, int T, double &cre, double &cim, double &E)
{
	cre = cim = E = 0.0;
	for (int i = 0; i < T; i++)
		step(cre, cim, E, (double)y[2 * i], (double)y[2 * i + 1], (double)t[2 * i], (double)t[2 * i + 1]);
}

/* rule 2: three rounded operations and one division (-ffp-contract=off: no fused multiply-add is formed) */
inline __host__ __device__ float rho_of(double cre, double cim, double E, double Et)
{
	const double num = (cre * cre) + (cim * cim);
	const double den = E * Et;
	return quiet((float)(den == 0.0 ? 0.0 : num / den));
}

/* the running peak: does (rho, lag) beat (best, best_lag)?  Larger rho first, then the smaller lag; a NaN never */
inline __host__ __device__ bool beats(float rho, int lag, float best, int best_lag)
{
	return lag >= 0 && rho == rho && (best_lag < 0 || rho > best || (rho == best && lag < best_lag));
}

/* what a lane, a wave, a tile or a job has seen of its lags */
struct Acc {
	int n_above, first, last, n_edges, peak_lag;
	float peak_rho;
};

__device__ __forceinline__ void acc_clear(Acc &a)
{
	a.n_above = 0; a.first = kNone; a.last = -1; a.n_edges = 0; a.peak_lag = -1; a.peak_rho = 0.0f;
}

/* integers, minima and maxima: the order does not matter */
__device__ __forceinline__ void acc_fold(Acc &a, const Acc &b)
{
	a.n_above += b.n_above;
	a.first = b.first < a.first ? b.first : a.first;
	a.last = b.last > a.last ? b.last : a.last;
	a.n_edges += b.n_edges;
	if (beats(b.peak_rho, b.peak_lag, a.peak_rho, a.peak_lag)) {
		a.peak_rho = b.peak_rho;
		a.peak_lag = b.peak_lag;
	}
}

/* the 64 lanes' Accs into one, the same in every lane */
__device__ __forceinline__ void acc_wave_reduce(Acc &a)
{
#pragma unroll
	for (int d = 32; d; d >>= 1) {
		Acc b;
		b.n_above = __shfl_xor(a.n_above, d);
		b.first = __shfl_xor(a.first, d);
		b.last = __shfl_xor(a.last, d);
		b.n_edges = __shfl_xor(a.n_edges, d);
		b.peak_lag = __shfl_xor(a.peak_lag, d);
		b.peak_rho = __shfl_xor(a.peak_rho, d);
		acc_fold(a, b);
	}
}

__global__ __launch_bounds__(kThreads)
void k_correlate_tile(const Params p)
{
	__shared__ __align__(16) LdsSample s_y[kImageY];
	__shared__ __align__(16) LdsSample s_t[kImageT];
	__shared__ unsigned char s_above[kTile];
	__shared__ Acc s_acc[kWaves];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.prefix[j]);			/* the tile: c * kTile < n_lags by the prefix */
	const int k0 = c * kTile;
	const int lags = min(job.n_lags - k0, kTile);			/* 1 .. kTile */
	const int T = job.tpl_len;					/* 1 .. kMaxTpl */
	const int at_y = job_table::load_span<kThreads>(s_y, p.iq + job.offset + k0, lags + T - 1, tid);	/* the job has them: k0 + lags + T - 1 <= n */
	const int at_t = job_table::load_span<kThreads>(s_t, p.tpl + job.tpl_offset, T, tid);
	__syncthreads();

	/* Lags tid + 256 s of the tile.  A lane beyond `lags` reads samples of the image that nobody loaded -- inside the array:
	 * at_y + tid + 768 + T - 1 <= 1 + 255 + 768 + 1023 < kImageY -- and its sums are never looked at. */
	double cre[kSlots], cim[kSlots], E[kSlots], Et = 0.0;
#pragma unroll
	for (int s = 0; s < kSlots; s++)
		cre[s] = cim[s] = E[s] = 0.0;
	const LdsSample *y = s_y + at_y + tid;
	const LdsSample *t = s_t + at_t;
	for (int i = 0; i < T; i++) {
		const LdsSample tv = t[i];
		const double tr = tv.x, ti = tv.y;
		Et = mac(Et, tr, tr);
		Et = mac(Et, ti, ti);
#pragma unroll
		for (int s = 0; s < kSlots; s++) {
			const LdsSample yv = y[i + kThreads * s];
			step(cre[s], cim[s], E[s], yv.x, yv.y, tr, ti);
		}
	}
	__syncthreads();						/* every lane has read its samples: s_y becomes the TRACE_C floats */

	float *s_c = reinterpret_cast<float *>(s_y);
	float rho[kSlots];
	float best = 0.0f;
	int best_lag = -1;
	double best_cre = 0.0, best_cim = 0.0, best_E = 0.0;
	Acc a;
	acc_clear(a);
#pragma unroll
	for (int s = 0; s < kSlots; s++) {
		const int q = tid + kThreads * s;
		rho[s] = rho_of(cre[s], cim[s], E[s], Et);
		if (q < lags) {
			const bool above = rho[s] >= job.threshold;
			s_above[q] = above;
			if (above) {
				a.n_above++;
				a.first = min(a.first, k0 + q);
				a.last = max(a.last, k0 + q);
			}
			if (beats(rho[s], k0 + q, best, best_lag)) {	/* q ascends: the smallest lag of the largest rho */
				best = rho[s];
				best_lag = k0 + q;
				best_cre = cre[s]; best_cim = cim[s]; best_E = E[s];
			}
			if (job.trace == FOSPHOR_AMD_CORRELATE_TRACE_RHO)
				p.out[job.out_offset + k0 + q] = rho[s];
			else if (job.trace == FOSPHOR_AMD_CORRELATE_TRACE_C) {
				s_c[2 * q] = quiet((float)cre[s]);
				s_c[2 * q + 1] = quiet((float)cim[s]);
			}
		}
	}
	a.peak_rho = best;
	a.peak_lag = best_lag;
	__syncthreads();
#pragma unroll
	for (int s = 0; s < kSlots; s++) {
		const int q = tid + kThreads * s;
		if (q < lags && s_above[q] && (q == 0 || !s_above[q - 1]))
			a.n_edges++;
	}
	if (job.trace == FOSPHOR_AMD_CORRELATE_TRACE_C) {
		float *out = p.out + job.out_offset + 2 * (int64_t)k0;
		for (int e = tid; e < 2 * lags; e += kThreads)
			out[e] = s_c[e];
	}

	acc_wave_reduce(a);
	if (lane == 0)
		s_acc[wave] = a;
	__syncthreads();
	Acc total = s_acc[0];
	for (int w = 1; w < kWaves; w++)
		acc_fold(total, s_acc[w]);
	Part *part = p.parts + blockIdx.x;
	if (tid == 0) {
		part->n_above = total.n_above;
		part->first = total.first;
		part->last = total.last;
		part->n_edges = total.n_edges;
		part->flags = (s_above[0] ? 1 : 0) | (s_above[lags - 1] ? 2 : 0);
		part->peak_lag = total.peak_lag;
		part->peak_rho = total.peak_rho;
		part->pad = 0;
		part->tpl_energy = quiet(Et);
		if (total.peak_lag < 0)
			part->c_re = part->c_im = part->energy = 0.0;
	}
	if (total.peak_lag >= 0 && best_lag == total.peak_lag) {	/* one lane: a lag has one owner */
		part->c_re = quiet(best_cre);
		part->c_im = quiet(best_cim);
		part->energy = quiet(best_E);
	}
}

__global__ __launch_bounds__(kThreads)
void k_correlate_combine(const Params p)
{
	const int lane = threadIdx.x & 63;
	const int j = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
	if (j >= p.n_jobs)						/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const int tiles = (int)(p.prefix[j + 1] - p.prefix[j]);
	const Part *parts = p.parts + p.prefix[j];
	Acc a;
	acc_clear(a);
	int best_tile = -1;
	for (int c0 = 0; c0 < tiles; c0 += 64) {
		const int c = c0 + lane;
		if (c < tiles) {
			Acc b;
			b.n_above = parts[c].n_above;
			b.first = parts[c].first;
			b.last = parts[c].last;
			b.n_edges = parts[c].n_edges;
			b.peak_lag = parts[c].peak_lag;
			b.peak_rho = parts[c].peak_rho;
			if (c > 0 && (parts[c - 1].flags & 2) && (parts[c].flags & 1))
				b.n_edges--;				/* the run came over the seam: not an edge */
			if (beats(b.peak_rho, b.peak_lag, a.peak_rho, a.peak_lag))
				best_tile = c;
			acc_fold(a, b);
		}
	}
	const int mine = a.peak_lag;
	acc_wave_reduce(a);
	Record *r = p.records + j;
	if (lane == 0) {
		r->n_lags = job.n_lags;
		r->n_above = a.n_above;
		r->first_above = a.first == kNone ? -1 : a.first;
		r->last_above = a.last;
		r->n_edges = a.n_edges;
		r->peak_lag = a.peak_lag;
		r->peak_rho = a.peak_rho;
		r->tpl_len = job.tpl_len;
		if (a.peak_lag < 0)
			r->peak_c_re = r->peak_c_im = r->peak_energy = 0.0;
		if (tiles > 0) {
			r->tpl_energy = parts[0].tpl_energy;
		} else {						/* no lag, no tile: the template's energy all the same */
			const float2 *t = p.tpl + job.tpl_offset;
			double Et = 0.0;
			for (int i = 0; i < job.tpl_len; i++) {
				const float2 tv = t[i];
				Et = mac(Et, (double)tv.x, (double)tv.x);
				Et = mac(Et, (double)tv.y, (double)tv.y);
			}
			r->tpl_energy = quiet(Et);
		}
	}
	if (a.peak_lag >= 0 && mine == a.peak_lag) {			/* one lane: a lag is in one tile */
		r->peak_c_re = parts[best_tile].c_re;
		r->peak_c_im = parts[best_tile].c_im;
		r->peak_energy = parts[best_tile].energy;
	}
}

struct Plan {
	long long groups, lags, macs;
	bool traces;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, int64_t n_tpl, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_CORRELATE_MAX_JOBS) || n_samples < 0 || n_tpl < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { 0, 0, 0, false };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples))
			return -EINVAL;
		if (b.tpl_len < 1 || b.tpl_len > kMaxTpl || !job_table::inside(b.tpl_offset, b.tpl_len, n_tpl))
			return -EINVAL;
		if (!trace_ok(b.trace) || b.threshold != b.threshold)
			return -EINVAL;
		if (b.trace == FOSPHOR_AMD_CORRELATE_TRACE_NONE && b.out_offset != 0)
			return -EINVAL;
		const int n_lags = n_lags_of(b.n, b.tpl_len);
		const int64_t n_out = n_out_of(b.trace, n_lags);
		if (!job_table::inside(b.out_offset, n_out, out_capacity) || !job_table::add_groups(pl.groups, n_lags, kTile))
			return -EINVAL;
		pl.lags += n_lags;
		pl.macs += (long long)n_lags * b.tpl_len;
		pl.traces |= b.trace != FOSPHOR_AMD_CORRELATE_TRACE_NONE;
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

extern "C" int fosphor_amd_correlate_host(const float *iq, int64_t n_samples, const float *tpl, int64_t n_tpl,
                                          const struct fosphor_amd_correlate_job *jobs, int n_jobs,
                                          struct fosphor_amd_correlate_record *records, float *out, int64_t out_capacity)
{
	if (!iq || !tpl || !records || ((uintptr_t)iq & 7) || ((uintptr_t)tpl & 7) || ((uintptr_t)records & 7) || ((uintptr_t)out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, n_tpl, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	if (plan.traces && !out)
		return -EINVAL;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const float *y = iq + 2 * b.offset, *t = tpl + 2 * b.tpl_offset;
		const int T = b.tpl_len, n_lags = n_lags_of(b.n, T);
		float *o = b.trace == FOSPHOR_AMD_CORRELATE_TRACE_NONE ? nullptr : out + b.out_offset;
		double Et = 0.0;
		for (int k = 0; k < T; k++) {
			Et = mac(Et, (double)t[2 * k], (double)t[2 * k]);
			Et = mac(Et, (double)t[2 * k + 1], (double)t[2 * k + 1]);
		}
		Record r;
		memset(&r, 0, sizeof(r));
		r.n_lags = n_lags;
		r.first_above = r.last_above = r.peak_lag = -1;
		r.tpl_len = T;
		r.tpl_energy = quiet(Et);
		bool prev = false;
		for (int k = 0; k < n_lags; k++) {
			double cre, cim, E;
			window(y + 2 * (int64_t)k, t, T, cre, cim, E);
			const float rho = rho_of(cre, cim, E, Et);
			const bool above = rho >= b.threshold;
			if (above) {
				r.n_above++;
				if (r.first_above < 0)
					r.first_above = k;
				r.last_above = k;
				r.n_edges += prev ? 0 : 1;
			}
			prev = above;
			if (beats(rho, k, r.peak_rho, r.peak_lag)) {
				r.peak_rho = rho;
				r.peak_lag = k;
				r.peak_c_re = quiet(cre); r.peak_c_im = quiet(cim); r.peak_energy = quiet(E);
			}
			if (b.trace == FOSPHOR_AMD_CORRELATE_TRACE_RHO)
				o[k] = rho;
			else if (b.trace == FOSPHOR_AMD_CORRELATE_TRACE_C) {
				o[2 * (int64_t)k] = quiet((float)cre);
				o[2 * (int64_t)k + 1] = quiet((float)cim);
			}
		}
		records[i] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_correlate_n_out(int trace, int32_t n, int tpl_len)
{
	if (!trace_ok(trace) || n < 0 || tpl_len < 1 || tpl_len > kMaxTpl)
		return -EINVAL;
	const int64_t n_out = n_out_of(trace, n_lags_of(n, tpl_len));
	return n_out > 0x7fffffffLL ? -EINVAL : (int)n_out;
}

extern "C" int fosphor_amd_correlate_from_extract(const struct fosphor_amd_extract_job *e, int64_t tpl_offset, int tpl_len,
                                                  int trace, float threshold, struct fosphor_amd_correlate_job *job)
{
	if (!e || !job || e->out_offset < 0 || e->n_out < 0 || tpl_offset < 0 || tpl_len < 1 || tpl_len > kMaxTpl || !trace_ok(trace) ||
	    threshold != threshold)
		return -EINVAL;
	job->offset = e->out_offset;
	job->out_offset = 0;
	job->tpl_offset = tpl_offset;
	job->n = e->n_out;
	job->tpl_len = tpl_len;
	job->trace = trace;
	job->threshold = threshold;
	return 0;
}

extern "C" int fosphor_amd_correlate_derive(const struct fosphor_amd_correlate_record *r, double sample_rate,
                                            struct fosphor_amd_correlate_values *v)
{
	if (!r || !v || !(sample_rate > 0.0) || !(sample_rate < INFINITY))
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	if (r->peak_lag < 0 || r->tpl_energy == 0.0)
		return 0;
	const double rho = r->peak_rho;
	v->time = r->peak_lag / sample_rate;
	v->rho = rho;
	v->gain_re = r->peak_c_re / r->tpl_energy;
	v->gain_im = r->peak_c_im / r->tpl_energy;
	v->gain_db = 10.0 * log10(v->gain_re * v->gain_re + v->gain_im * v->gain_im);
	v->phase_turns = fosphor_amd_atan2_turns(r->peak_c_im, r->peak_c_re);
	v->snr_db = rho >= 1.0 ? INFINITY : 10.0 * log10(rho / (1.0 - rho));
	v->detections = r->n_edges;
	return 0;
}

extern "C" int fosphor_amd_correlate_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_CORRELATE_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_CORRELATE, FOSPHOR_AMD_CORRELATE_STATS, stats);
}

extern "C" int fosphor_amd_correlate(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                     const void *d_tpl, int64_t n_tpl,
                                     const struct fosphor_amd_correlate_job *jobs, int n_jobs,
                                     struct fosphor_amd_correlate_record *d_records,
                                     float *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !d_tpl || !jobs || !d_records)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_tpl & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, n_tpl, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	if (plan.traces && !d_out)
		return -EINVAL;

	/* the table: every job in job order (one form), written where it goes, the prefix; behind it the partials */
	const size_t n_form[2] = { (size_t)n_jobs, 0 }, n_prefix[2] = { (size_t)n_jobs + 1, 0 };
	job_table::Table table = job_table::lay_table(sizeof(DevJob), n_form, n_prefix, (size_t)plan.groups, sizeof(Part));
	DevJob *dj = reinterpret_cast<DevJob *>(table.image.data() + table.jobs_at[0]);
	uint32_t *prefix = reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[0]);
	for (int i = 0; i < n_jobs; i++) {
		DevJob &d = dj[i];
		d.offset = jobs[i].offset;
		d.out_offset = jobs[i].out_offset;
		d.tpl_offset = jobs[i].tpl_offset;
		d.n_lags = n_lags_of(jobs[i].n, jobs[i].tpl_len);
		d.tpl_len = jobs[i].tpl_len;
		d.trace = jobs[i].trace;
		d.threshold = jobs[i].threshold;
		prefix[i + 1] = prefix[i] + (uint32_t)job_table::groups_of(d.n_lags, kTile);
	}

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_CORRELATE);
	stats[FOSPHOR_AMD_CORRELATE_CALLS]++;
	stats[FOSPHOR_AMD_CORRELATE_JOBS] += n_jobs;
	stats[FOSPHOR_AMD_CORRELATE_LAGS] += plan.lags;
	stats[FOSPHOR_AMD_CORRELATE_MACS] += plan.macs;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_CORRELATE, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.tpl = static_cast<const float2 *>(d_tpl);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.parts = reinterpret_cast<Part *>(d + table.parts_at);
	p.records = d_records;
	p.out = d_out;
	p.n_jobs = n_jobs;
	int rv = 0;
	if (plan.groups)
		rv = job_table::launch<kThreads>(k_correlate_tile, (unsigned)plan.groups, st, p, stats, FOSPHOR_AMD_CORRELATE_K_TILE);
	if (!rv)
		rv = job_table::launch<kThreads>(k_correlate_combine, (unsigned)job_table::groups_of(n_jobs, kWaves), st, p, stats,
		                                 FOSPHOR_AMD_CORRELATE_K_COMBINE);
	return job_table::drain(st, rv);
}
