/*
 * fosphor_carrier.hip -- carrier frequency and phase of burst symbols where they lie: the M-th power of every symbol, its lag-1 and
 * lag-L sums, two pinned angles for the frequency, the sum of the powers with that frequency removed, one angle for the phase, and
 * the symbols turned back by both (include/fosphor_amd_carrier.h)
 *
 * A read-only pass over the CALLER's float32 symbols (what fosphor_amd_symbols wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table, the two
 * prefixes of tile counts, the tiles' partial sums and the jobs' two states).
 *
 *   k_car_lag    256 lanes own one tile (4096 terms) of one job that estimates its frequency, which they find in the prefix
 *                (fosphor_jobs.h).  256 terms a pass: the pass's symbols go into the LDS image of double pairs, every lane raises its
 *                own entries to M in place, lane t forms the terms of j and j + 1 and of j and j + Le.
 *   k_car_freq   a wave per job: lanes 0 .. 3 add the job's tiles in ascending order, every lane runs rule 3, lane 0 writes Freq.
 *   k_car_sum    256 lanes own one tile of 4096 symbols of a job; every lane loads its own symbol, 8 bytes, consecutive lanes from
 *                consecutive addresses.
 *   k_car_phase  a wave per job adds the tiles, takes the angle of rule 5, writes the record and Turn.
 *   k_car_turn   the tiles of k_car_sum again, for rule 6.
 * In k_car_lag and k_car_sum a wave's 64 terms of a pass are one block: the lanes write their four terms into rows of 65 doubles,
 * and lanes 0 .. 3 add a row each, in order -- row m begins 130 m dwords into the image, so the four read four different banks.
 * Every sum is formed by the operations of the helpers below, on the device and in fosphor_amd_carrier_host alike; the build's
 * -ffp-contract=off keeps each of them one rounding.  No atomics of any kind, no work-group waits for another, every loop carries
 * its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_carrier.h"

namespace {

typedef struct fosphor_amd_carrier_job Job;
typedef struct fosphor_amd_carrier_record Record;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlock = FOSPHOR_AMD_CARRIER_BLOCK;
constexpr int kTile = FOSPHOR_AMD_CARRIER_TILE;
constexpr int kMaxLag = FOSPHOR_AMD_CARRIER_MAX_LAG;
constexpr int kPass = kThreads;					/* terms of a pass */
constexpr int kSums = 4;					/* lag: R1 re, R1 im, RL re, RL im; phase: Z re, Z im, m2, mm */
constexpr int kFreqFixed = FOSPHOR_AMD_CARRIER_FREQ_FIXED;
constexpr int kPhaseFixed = FOSPHOR_AMD_CARRIER_PHASE_FIXED;

static_assert(FOSPHOR_AMD_CARRIER_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 48, "the job is 48 bytes");
static_assert(sizeof(Record) == 96, "the record is 96 bytes");
static_assert(kBlock == 64 && kTile == kBlock * kBlock, "a wave's lanes are a block, 64 blocks a tile");
static_assert(kMaxLag <= kBlock, "lanes 0 .. Le - 1 raise the image's entries behind the pass's 256");

inline bool order_ok(int order) { return order == 2 || order == 4 || order == 8; }
/* rule 8, of one value that a mode bit allows; a NaN fails the comparisons */
inline bool fixed_ok(bool fixed, double v) { return fixed ? (v >= -0.5 && v <= 0.5) : v == 0.0; }
inline bool carrier_ok(int order, int mode, int lag, double freq, double phase)
{
	return order_ok(order) && !(mode & ~(kFreqFixed | kPhaseFixed)) && lag >= 1 && lag <= kMaxLag &&
	       fixed_ok(mode & kFreqFixed, freq) && fixed_ok(mode & kPhaseFixed, phase);
}

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t offset;
	int64_t out_offset;
	int64_t lag0;			/* the job's first tile of kSums doubles in the lag partials */
	int64_t sum0;			/* ... in the phase-sum partials */
	double  freq, phase;
	int32_t n;
	int32_t order;
	int32_t mode;
	int32_t lag;
};

static_assert(sizeof(DevJob) == 64, "a device job is 64 bytes");

/* what k_car_freq leaves of a job that estimates its frequency */
struct Freq {
	double  g, f;
	double  r[kSums];
	int32_t status, lag_used;
};

/* what k_car_phase leaves of every job for k_car_turn */
struct Turn {
	double  theta, f;
	int32_t status, pad;
};

static_assert(sizeof(Freq) == 56 && sizeof(Turn) == 24, "the states are whole doubles");

struct Params {
	const float2   *iq;
	float2         *out;
	const DevJob   *jobs;
	const uint32_t *lag_prefix;	/* [n_jobs + 1] lag tiles before job j */
	const uint32_t *sum_prefix;	/* [n_jobs + 1] symbol tiles before job j */
	double         *lag_parts;
	double         *sum_parts;
	Freq           *freq;
	Turn           *turn;
	Record         *records;
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }
inline __host__ __device__ double quiet(double v) { return v != v ? (double)NAN : v; }

inline __host__ __device__ int lag_used_of(int n, int lag) { return n >= 2 * lag ? lag : 1; }
/* the tiles of n terms, n <= 2^31 - 1 */
inline __host__ __device__ int tiles_of(int n) { return (int)(((int64_t)n + kTile - 1) / kTile); }

/* rule 1: s^M in place */
inline __host__ __device__ void power_of(int order, double &re, double &im)
{
	for (int m = 2; m <= 8 && m <= order; m *= 2) {
		const double r = (re * re) - (im * im), i = (re * im) + (re * im);
		re = r;
		im = i;
	}
}

/* rule 1: w and |s|^M */
inline __host__ __device__ void moduli_of(int order, double re, double im, double &w, double &wm)
{
	w = (re * re) + (im * im);
	wm = w;
	for (int m = 4; m <= 8 && m <= order; m *= 2)
		wm = wm * wm;
}

/* rule 2: a conj(b) */
inline __host__ __device__ void lag_term(double ar, double ai, double br, double bi, double &tr, double &ti)
{
	tr = (ar * br) + (ai * bi);
	ti = (ai * br) - (ar * bi);
}

/* rule 3 from the lag sums R[4] of a job that estimates its frequency */
inline __host__ __device__ void freq_of(int n, int order, int lag, const double *R, Freq &st)
{
	const int Le = lag_used_of(n, lag);
	for (int k = 0; k < kSums; k++)
		st.r[k] = quiet(R[k]);
	st.lag_used = Le;
	st.status = FOSPHOR_AMD_CARRIER_OK;
	const float a1 = fosphor_amd_atan2_turns(R[1], R[0]);
	double g = (double)a1;
	bool lost = a1 != a1;
	if (Le > 1) {
		const float aL = fosphor_amd_atan2_turns(R[3], R[2]);
		const double k = floor((((double)Le * (double)a1) - (double)aL) + 0.5);
		g = ((double)aL + k) / (double)Le;
		lost = lost || aL != aL;
	}
	if (lost) {
		st.status = FOSPHOR_AMD_CARRIER_NO_CARRIER;
		st.g = st.f = (double)NAN;
		return;
	}
	st.g = g;
	st.f = g / (double)order;
}

/* ... and of a job under FREQ_FIXED */
inline __host__ __device__ void freq_fixed(int order, double freq, Freq &st)
{
	for (int k = 0; k < kSums; k++)
		st.r[k] = 0.0;
	st.lag_used = 0;
	st.status = FOSPHOR_AMD_CARRIER_OK;
	st.g = freq * (double)order;
	st.f = st.g / (double)order;
}

/* rule 5: the four terms of symbol j */
inline __host__ __device__ void sum_terms(int order, double g, int64_t j, float fr, float fi, double *t)
{
	double pr = fr, pi = fi, c, sn;
	moduli_of(order, pr, pi, t[2], t[3]);
	power_of(order, pr, pi);
	const double psi = g * (double)j;
	fosphor_amd_cossin_turns(psi, &c, &sn);
	t[0] = (pr * c) + (pi * sn);
	t[1] = (pi * c) - (pr * sn);
}

/* rule 5 from the sums S[4]: the record and the state of rule 6 */
inline __host__ __device__ void phase_of(int n, int order, int mode, double phase, const Freq &fq, const double *S, Record &r, Turn &tn)
{
	r.n = n;
	r.order = order;
	r.lag_used = fq.lag_used;
	r.status = fq.status;
	r.r1_re = fq.r[0];
	r.r1_im = fq.r[1];
	r.rl_re = fq.r[2];
	r.rl_im = fq.r[3];
	r.freq = fq.f;
	r.z_re = r.z_im = r.m2 = r.mm = 0.0;
	double theta = phase;
	if (fq.status == FOSPHOR_AMD_CARRIER_OK) {
		r.z_re = quiet(S[0]);
		r.z_im = quiet(S[1]);
		r.m2 = quiet(S[2]);
		r.mm = quiet(S[3]);
		if (!(mode & kPhaseFixed)) {
			const float thM = fosphor_amd_atan2_turns(S[1], S[0]);
			if (thM != thM)
				r.status = FOSPHOR_AMD_CARRIER_NO_CARRIER;
			theta = (double)thM / (double)order;
		}
	}
	if (r.status != FOSPHOR_AMD_CARRIER_OK) {
		r.freq = (double)NAN;
		theta = (double)NAN;
	}
	r.phase = theta;
	tn.theta = theta;
	tn.f = r.freq;
	tn.status = r.status;
	tn.pad = 0;
}

/* rule 6: symbol j */
inline __host__ __device__ float2 turned(double theta, double f, int64_t j, float fr, float fi)
{
	const double sr = fr, si = fi;
	double c, sn;
	const double phi = theta + (f * (double)j);
	fosphor_amd_cossin_turns(phi, &c, &sn);
	float2 o;
	o.x = quiet((float)((sr * c) + (si * sn)));
	o.y = quiet((float)((si * c) - (sr * sn)));
	return o;
}

/* the wave's own stores to LDS before its loads from it (the form of fosphor_kernels.hip) */
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* One block of the ordered sums: the wave has written its lanes' terms into s_t[m][lane]; lane m < kSums adds the first
 * count[m] of row m in order and leaves the sum as block `block` of the tile.  A row without terms leaves 0.0. */
__device__ __forceinline__ void block_sums(const double (*s_t)[kBlock + 1], double (*s_bs)[kBlock + 1], int lane, int block,
                                           int count_lo, int count_hi)
{
	wave_lds_sync();
	if (lane < kSums) {
		const int count = lane < 2 ? count_lo : count_hi;
		double run = 0.0;
		for (int l = 0; l < kBlock && l < count; l++)
			run = run + s_t[lane][l];
		s_bs[lane][block] = run;
	}
}

/* the tile's `blocks` block sums, by lane t < kSums, in order */
__device__ __forceinline__ void tile_sums(const double (*s_bs)[kBlock + 1], int t, int blocks, double *part)
{
	if (t < kSums) {
		double T = 0.0;
		for (int b = 0; b < kBlock && b < blocks; b++)
			T = T + s_bs[t][b];
		part[t] = T;
	}
}

__global__ __launch_bounds__(kThreads)
void k_car_lag(const Params p)
{
	__shared__ __align__(16) double2 s_p[kPass + kMaxLag + 1];
	__shared__ double s_t[kWaves][kSums][kBlock + 1];
	__shared__ double s_bs[kSums][kBlock + 1];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int j = job_table::find_job(p.lag_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.lag_prefix[j]);
	const int Le = lag_used_of(job.n, job.lag);
	const int j0 = c * kTile;						/* the tile's first term: below n - 1 by the prefix */
	const int terms = min(job.n - 1 - j0, kTile);				/* of lag 1: 1 .. kTile */
	const float2 *y = p.iq + job.offset + j0;
	for (int s0 = 0; s0 < terms; s0 += kPass) {
		const int count = min(terms - s0, kPass);			/* lag-1 terms of the pass; lane t has term j0 + s0 + t */
		const int span = min(job.n - (j0 + s0), count + Le);		/* symbols j0 + s0 .. that the pass's terms read: inside the job */
		const int at = job_table::load_span<kThreads>(s_p, y + s0, span, t);
		__syncthreads();
		/* rule 1 in place: every entry by one lane */
		if (t < span)
			power_of(job.order, s_p[at + t].x, s_p[at + t].y);
		if (t < kMaxLag && kPass + t < span)
			power_of(job.order, s_p[at + kPass + t].x, s_p[at + kPass + t].y);
		__syncthreads();
		const int count_l = Le > 1 ? min(job.n - Le - (j0 + s0), count) : 0;	/* lag-Le terms of the pass; below 1: none */
		double term[kSums];
#pragma unroll
		for (int m = 0; m < kSums; m++)
			term[m] = 0.0;
		if (t < count) {
			const double2 b = s_p[at + t], a = s_p[at + t + 1];
			lag_term(a.x, a.y, b.x, b.y, term[0], term[1]);
			if (t < count_l) {
				const double2 al = s_p[at + t + Le];
				lag_term(al.x, al.y, b.x, b.y, term[2], term[3]);
			}
		}
#pragma unroll
		for (int m = 0; m < kSums; m++)
			s_t[wave][m][lane] = term[m];
		if (wave * kBlock < count)					/* the whole wave: block (s0 / 64) + wave of the tile */
			block_sums(s_t[wave], s_bs, lane, (s0 >> 6) + wave, count - wave * kBlock, count_l - wave * kBlock);
		__syncthreads();						/* s_p and s_t are free; the block sums are written */
	}
	tile_sums(s_bs, t, (terms + kBlock - 1) / kBlock, p.lag_parts + (job.lag0 + c) * kSums);
}

/* the sums of `tiles` tiles of kSums doubles by lanes 0 .. kSums - 1, in order, handed to every lane */
__device__ __forceinline__ void job_sums(const double *parts, int tiles, int lane, double *S)
{
	double acc = 0.0;
	if (lane < kSums) {
		const double *T = parts + lane;
#pragma unroll 8								/* eight loads in flight; the additions keep their order */
		for (int c = 0; c < tiles; c++)
			acc = acc + T[(int64_t)c * kSums];
	}
#pragma unroll
	for (int k = 0; k < kSums; k++)
		S[k] = __shfl(acc, k);
}

__global__ __launch_bounds__(kThreads)
void k_car_freq(const Params p)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	if (job.mode & kFreqFixed)						/* the whole wave: its state is made where it is used */
		return;
	double R[kSums];
	job_sums(p.lag_parts + job.lag0 * kSums, tiles_of(max(job.n - 1, 0)), lane, R);
	Freq st;
	freq_of(job.n, job.order, job.lag, R, st);
	if (lane == 0)
		p.freq[j] = st;
}

/* the frequency state of job j: what k_car_freq left, or what FREQ_FIXED says */
__device__ __forceinline__ Freq freq_state(const Params &p, const DevJob &job, int j)
{
	if (!(job.mode & kFreqFixed))
		return p.freq[j];
	Freq st;
	freq_fixed(job.order, job.freq, st);
	return st;
}

__global__ __launch_bounds__(kThreads)
void k_car_sum(const Params p)
{
	__shared__ double s_t[kWaves][kSums][kBlock + 1];
	__shared__ double s_bs[kSums][kBlock + 1];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int j = job_table::find_job(p.sum_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const Freq fq = freq_state(p, job, j);
	if (fq.status != FOSPHOR_AMD_CARRIER_OK)				/* the whole work-group: rule 3 found no carrier */
		return;
	const int c = (int)(blockIdx.x - p.sum_prefix[j]);
	const int j0 = c * kTile;						/* the tile's first symbol: below n by the prefix */
	const int syms = min(job.n - j0, kTile);
	const float2 *y = p.iq + job.offset + j0;
	for (int s0 = 0; s0 < syms; s0 += kPass) {
		const int count = min(syms - s0, kPass);			/* symbols of the pass; lane t has symbol j0 + s0 + t */
		double term[kSums];
#pragma unroll
		for (int m = 0; m < kSums; m++)
			term[m] = 0.0;
		if (t < count) {
			const float2 v = y[s0 + t];
			sum_terms(job.order, fq.g, (int64_t)j0 + s0 + t, v.x, v.y, term);
		}
#pragma unroll
		for (int m = 0; m < kSums; m++)
			s_t[wave][m][lane] = term[m];
		if (wave * kBlock < count)					/* the whole wave */
			block_sums(s_t[wave], s_bs, lane, (s0 >> 6) + wave, count - wave * kBlock, count - wave * kBlock);
		__syncthreads();						/* s_t is free; the block sums are written */
	}
	tile_sums(s_bs, t, (syms + kBlock - 1) / kBlock, p.sum_parts + (job.sum0 + c) * kSums);
}

__global__ __launch_bounds__(kThreads)
void k_car_phase(const Params p)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const Freq fq = freq_state(p, job, j);
	/* the tiles that k_car_sum wrote: none of a job without a carrier */
	const int tiles = fq.status == FOSPHOR_AMD_CARRIER_OK ? tiles_of(job.n) : 0;
	double S[kSums];
	job_sums(p.sum_parts + job.sum0 * kSums, tiles, lane, S);
	Record r;
	Turn tn;
	phase_of(job.n, job.order, job.mode, job.phase, fq, S, r, tn);
	if (lane == 0) {
		p.records[j] = r;
		p.turn[j] = tn;
	}
}

__global__ __launch_bounds__(kThreads)
void k_car_turn(const Params p)
{
	const int t = threadIdx.x;
	const int j = job_table::find_job(p.sum_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const Turn tn = p.turn[j];
	if (tn.status != FOSPHOR_AMD_CARRIER_OK)				/* the whole work-group: nothing is written */
		return;
	const int j0 = (int)(blockIdx.x - p.sum_prefix[j]) * kTile;		/* the tile's first symbol: below n by the prefix */
	const int syms = min(job.n - j0, kTile);
	const float2 *y = p.iq + job.offset + j0;
	float2 *out = p.out + job.out_offset + j0;
	for (int s = t; s < syms; s += kThreads) {				/* at most kTile / kThreads turns */
		const float2 v = y[s];
		out[s] = turned(tn.theta, tn.f, (int64_t)j0 + s, v.x, v.y);
	}
}

struct Plan {
	long long tiles_lag, tiles_sum, jobs_freq, jobs_phase, symbols;
};

/* the lag-1 terms of a job that estimates its frequency */
inline long long lag_terms_of(const Job &b) { return (b.mode & kFreqFixed) || b.n < 2 ? 0 : b.n - 1; }

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_CARRIER_MAX_JOBS) || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { 0, 0, 0, 0, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || !carrier_ok(b.order, b.mode, b.lag, b.freq, b.phase))
			return -EINVAL;
		if (!job_table::inside(b.out_offset, b.n, out_capacity) || !job_table::add_groups(pl.tiles_lag, lag_terms_of(b), kTile) ||
		    !job_table::add_groups(pl.tiles_sum, b.n, kTile))
			return -EINVAL;
		pl.jobs_freq += !(b.mode & kFreqFixed);
		pl.jobs_phase += !(b.mode & kPhaseFixed);
		pl.symbols += b.n;
		if (b.n > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + b.n));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

/* the three-level order of rules 2 and 5 on the host: terms come in ascending order, one add() each */
struct Ordered {
	double block, tile, job;
	int64_t n;
	Ordered() : block(0.0), tile(0.0), job(0.0), n(0) {}
	void add(double v)
	{
		block = block + v;
		n++;
		if (n % kBlock == 0) {
			tile = tile + block;
			block = 0.0;
		}
		if (n % kTile == 0) {
			job = job + tile;
			tile = 0.0;
		}
	}
	double sum()
	{
		if (n % kBlock) {
			tile = tile + block;
			block = 0.0;
		}
		if (n % kTile) {
			job = job + tile;
			tile = 0.0;
		}
		n = 0;
		return job;
	}
};

} // namespace

extern "C" int fosphor_amd_carrier_host(const float *iq, int64_t n_samples, const struct fosphor_amd_carrier_job *jobs, int n_jobs,
                                        struct fosphor_amd_carrier_record *records, float *out, int64_t out_capacity)
{
	if (!iq || !records || !out || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7) || ((uintptr_t)out & 7))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, nullptr))
		return -EINVAL;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const float *y = iq + 2 * b.offset;
		Freq fq;
		if (b.mode & kFreqFixed) {
			freq_fixed(b.order, b.freq, fq);
		} else {
			const int Le = lag_used_of(b.n, b.lag);
			Ordered sums[kSums];
			for (int64_t j = 0; j + 1 < b.n; j++) {
				double br = y[2 * j], bi = y[2 * j + 1], ar = y[2 * j + 2], ai = y[2 * j + 3], term[kSums] = { 0.0, 0.0, 0.0, 0.0 };
				power_of(b.order, br, bi);
				power_of(b.order, ar, ai);
				lag_term(ar, ai, br, bi, term[0], term[1]);
				if (Le > 1 && j + Le < b.n) {
					double lr = y[2 * (j + Le)], li = y[2 * (j + Le) + 1];
					power_of(b.order, lr, li);
					lag_term(lr, li, br, bi, term[2], term[3]);
				}
				for (int m = 0; m < kSums; m++)
					sums[m].add(term[m]);
			}
			double R[kSums];
			for (int m = 0; m < kSums; m++)
				R[m] = sums[m].sum();
			freq_of(b.n, b.order, b.lag, R, fq);
		}
		double S[kSums] = { 0.0, 0.0, 0.0, 0.0 };
		if (fq.status == FOSPHOR_AMD_CARRIER_OK) {
			Ordered sums[kSums];
			for (int64_t j = 0; j < b.n; j++) {
				double term[kSums];
				sum_terms(b.order, fq.g, j, y[2 * j], y[2 * j + 1], term);
				for (int m = 0; m < kSums; m++)
					sums[m].add(term[m]);
			}
			for (int m = 0; m < kSums; m++)
				S[m] = sums[m].sum();
		}
		Record r;
		Turn tn;
		memset(&r, 0, sizeof(r));
		phase_of(b.n, b.order, b.mode, b.phase, fq, S, r, tn);
		records[i] = r;
		if (tn.status != FOSPHOR_AMD_CARRIER_OK)
			continue;
		float *o = out + 2 * b.out_offset;
		for (int64_t j = 0; j < b.n; j++) {
			const float2 v = turned(tn.theta, tn.f, j, y[2 * j], y[2 * j + 1]);
			o[2 * j] = v.x;
			o[2 * j + 1] = v.y;
		}
	}
	return 0;
}

extern "C" int fosphor_amd_carrier_from_symbols(const struct fosphor_amd_symbols_job *s, const struct fosphor_amd_symbols_record *r,
                                                int order, int mode, int lag, double freq, double phase,
                                                struct fosphor_amd_carrier_job *job)
{
	if (!s || !r || !job || s->out_offset < 0 || r->n_sym < 0 || !carrier_ok(order, mode, lag, freq, phase))
		return -EINVAL;
	job->offset = s->out_offset;
	job->out_offset = 0;
	job->n = r->n_sym;
	job->order = order;
	job->mode = mode;
	job->lag = lag;
	job->freq = freq;
	job->phase = phase;
	return 0;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_carrier_derive(const struct fosphor_amd_carrier_record *r, double symbol_rate,
                                          struct fosphor_amd_carrier_values *v)
{
	if (!r || !v || !(symbol_rate > 0.0) || !(symbol_rate < INFINITY))
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	if (r->n <= 0 || r->status != FOSPHOR_AMD_CARRIER_OK)
		return 0;
	const double n = r->n;
	v->freq_hz = finite_or_zero(r->freq * symbol_rate);
	v->phase_rad = finite_or_zero(6.283185307179586 * r->phase);
	v->sym_power = finite_or_zero(r->m2 / n);
	if (r->mm > 0.0) {
		v->lock = finite_or_zero(hypot(r->z_re, r->z_im) / r->mm);
		v->lag_lock = finite_or_zero(hypot(r->r1_re, r->r1_im) * n / (r->mm * r->mm));
		if (r->lag_used > 1)
			v->lagl_lock = finite_or_zero(hypot(r->rl_re, r->rl_im) * n / (r->mm * r->mm));
	}
	return 0;
}

extern "C" int fosphor_amd_carrier_cossin_turns(double t, double *c, double *s)
{
	if (!c || !s)
		return -EINVAL;
	fosphor_amd_cossin_turns(t, c, s);
	return 0;
}

extern "C" int fosphor_amd_carrier_cossin_turns_n(const double *t, int64_t n, double *c, double *s)
{
	if (!t || !c || !s || n < 0)
		return -EINVAL;
	for (int64_t i = 0; i < n; i++)
		fosphor_amd_cossin_turns(t[i], c + i, s + i);
	return 0;
}

extern "C" int fosphor_amd_carrier_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_CARRIER_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_CARRIER, FOSPHOR_AMD_CARRIER_STATS, stats);
}

extern "C" int fosphor_amd_carrier(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                   const struct fosphor_amd_carrier_job *jobs, int n_jobs,
                                   struct fosphor_amd_carrier_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order, the prefix of their lag tiles, the prefix of their symbol tiles; behind it, in
	 * doubles: the lag partials, the phase-sum partials, the frequency states, the states of rule 6 */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2];
	prefix[0].assign(1, 0u);
	prefix[1].assign(1, 0u);
	int64_t lag0 = 0, sum0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		DevJob d;
		memset(&d, 0, sizeof(d));
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.lag0 = lag0;
		d.sum0 = sum0;
		d.freq = b.freq;
		d.phase = b.phase;
		d.n = b.n;
		d.order = b.order;
		d.mode = b.mode;
		d.lag = b.lag;
		const long long lag = job_table::groups_of(lag_terms_of(b), kTile), sum = job_table::groups_of(b.n, kTile);
		lag0 += lag;
		sum0 += sum;
		prefix[0].push_back(prefix[0].back() + (uint32_t)lag);
		prefix[1].push_back(prefix[1].back() + (uint32_t)sum);
		form[0].push_back(d);
	}
	const size_t n_freq = (size_t)n_jobs * (sizeof(Freq) / sizeof(double)), n_turn = (size_t)n_jobs * (sizeof(Turn) / sizeof(double));
	const job_table::Table table = job_table::pack_table(form, prefix, (size_t)(lag0 + sum0) * kSums + n_freq + n_turn, sizeof(double));

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_CARRIER);
	stats[FOSPHOR_AMD_CARRIER_CALLS]++;
	stats[FOSPHOR_AMD_CARRIER_JOBS_FREQ] += plan.jobs_freq;
	stats[FOSPHOR_AMD_CARRIER_JOBS_PHASE] += plan.jobs_phase;
	stats[FOSPHOR_AMD_CARRIER_SYMBOLS] += plan.symbols;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_CARRIER, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = static_cast<float2 *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.lag_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.sum_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[1]);
	p.lag_parts = reinterpret_cast<double *>(d + table.parts_at);
	p.sum_parts = p.lag_parts + lag0 * kSums;
	p.freq = reinterpret_cast<Freq *>(p.sum_parts + sum0 * kSums);
	p.turn = reinterpret_cast<Turn *>(reinterpret_cast<double *>(p.freq) + n_freq);
	p.records = d_records;
	p.n_jobs = n_jobs;
	const unsigned per_wave = (unsigned)job_table::groups_of(n_jobs, kWaves);
	int rv = 0;
	if (plan.tiles_lag)
		rv = job_table::launch<kThreads>(k_car_lag, (unsigned)plan.tiles_lag, st, p, stats, FOSPHOR_AMD_CARRIER_K_LAG);
	if (plan.jobs_freq && !rv)
		rv = job_table::launch<kThreads>(k_car_freq, per_wave, st, p, stats, FOSPHOR_AMD_CARRIER_K_FREQ);
	if (plan.tiles_sum && !rv)
		rv = job_table::launch<kThreads>(k_car_sum, (unsigned)plan.tiles_sum, st, p, stats, FOSPHOR_AMD_CARRIER_K_SUM);
	if (!rv)
		rv = job_table::launch<kThreads>(k_car_phase, per_wave, st, p, stats, FOSPHOR_AMD_CARRIER_K_PHASE);
	if (plan.tiles_sum && !rv)
		rv = job_table::launch<kThreads>(k_car_turn, (unsigned)plan.tiles_sum, st, p, stats, FOSPHOR_AMD_CARRIER_K_TURN);
	return job_table::drain(st, rv);
}
