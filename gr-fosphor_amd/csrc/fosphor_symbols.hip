/*
 * fosphor_symbols.hip -- symbol timing and symbol-rate samples of burst IQ where it lies: |y|^2 folded modulo the samples per
 * symbol, the symbol-rate line, one pinned angle, a cubic Lagrange fractional delay and a decimation (include/fosphor_amd_symbols.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract and fosphor_amd_resample wrote), in a file of its own:
 * nothing here is on the process / merge path and no buffer of the instance is read or written but the scratch this file owns (the
 * job table, the two prefixes of tile counts, the twiddles, the tiles' partial sums, the jobs' states and their symbol counts).
 *
 *   k_sym_fold    256 lanes own one tile (4096 symbols) of one ESTIMATE job, which they find in the prefix (fosphor_jobs.h).  A piece
 *                 is 64 / sps whole blocks, at most 4096 samples: every lane squares its share into the LDS image of doubles, then
 *                 lane (b, k) of wave 0 adds block b's 64 values of phase k serially and lane k the piece's blocks.
 *   k_sym_time    a wave per job: lane k adds the job's tiles in ascending order, every lane runs rules 2 to 5 over the 64 sums in
 *                 LDS, lane 0 writes the job's State.  FIXED jobs enter here.
 *   k_sym_pick    256 lanes own one tile of 4096 symbols of a job's RESERVED outputs; the State says how many exist.  256 symbols
 *                 a pass, a wave's 64 are one block of rule 6.
 *   k_sym_record  a wave per job adds the tiles that exist and writes the record.
 * The fold image has one row of 64 sps doubles per block and sps doubles of padding behind it: the double of lane p = b sps + k in
 * step r lies at sps (65 b + r) + k, which is p + sps r modulo 32 -- the 32 lanes of a half wave read 32 different 8-byte slots.
 * Every sum is formed by the operations of the helpers below, on the device and in fosphor_amd_symbols_host alike; the build's
 * -ffp-contract=off keeps each of them one rounding.  No atomics of any kind, no work-group waits for another, every loop carries
 * its bound in its header.
 */
#include <math.h>

#include <map>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_demod.h"			/* fosphor_amd_atan2_turns */
#include "../../include/fosphor_amd_symbols.h"

namespace {

typedef struct fosphor_amd_symbols_job Job;
typedef struct fosphor_amd_symbols_record Record;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlock = FOSPHOR_AMD_SYMBOLS_BLOCK;
constexpr int kTile = FOSPHOR_AMD_SYMBOLS_TILE;
constexpr int kMinSps = FOSPHOR_AMD_SYMBOLS_MIN_SPS;
constexpr int kMaxSps = FOSPHOR_AMD_SYMBOLS_MAX_SPS;
constexpr int kStageSps = FOSPHOR_AMD_SYMBOLS_STAGE_SPS;
constexpr int kFoldImage = (kBlock + 1) * kMaxSps;		/* doubles: 64 / sps rows of 65 sps */
constexpr int kPass = kThreads;					/* symbols of a pass of k_sym_pick */
constexpr int kStage = (kPass - 1) * kStageSps + 4;		/* samples of the longest staged span */
constexpr int kMoments = 6;					/* m2, m4, z2 re, z2 im, z4 re, z4 im */

static_assert(FOSPHOR_AMD_SYMBOLS_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 40, "the job is 40 bytes");
static_assert(sizeof(Record) == 96, "the record is 96 bytes");
static_assert(kBlock == 64 && kTile == kBlock * kBlock, "a wave's lanes are a block, 64 blocks a tile");
static_assert(kMaxSps <= kBlock, "the chains of a piece, 64 / sps x sps of them, are lanes of one wave");

inline bool sps_ok(int sps) { return sps >= kMinSps && sps <= kMaxSps; }
inline bool mode_ok(int mode) { return mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE || mode == FOSPHOR_AMD_SYMBOLS_FIXED; }
/* rule 8, of one job's sps, mode and tau; a NaN tau fails both comparisons */
inline bool timing_ok(int sps, int mode, float tau)
{
	if (!sps_ok(sps) || !mode_ok(mode) || !(tau >= 0.0f && tau < 1.0f))
		return false;
	return mode == FOSPHOR_AMD_SYMBOLS_FIXED || (sps >= 3 && tau == 0.0f);
}
inline int max_out_of(int n, int sps) { return n < 4 ? 0 : (n - 4) / sps + 1; }

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t offset;
	int64_t out_offset;
	int64_t part0;			/* doubles into the fold partials: tile c of the job is parts[part0 + c sps .. + sps) */
	int64_t mom0;			/* the job's first tile of kMoments doubles in the pick partials */
	int32_t n;
	int32_t sps;
	int32_t mode;
	int32_t tw0;			/* doubles into the twiddles: the table of this sps */
	int32_t tiles_max;		/* tiles of the reserved outputs */
	float   tau;
	int32_t pad[2];
};

static_assert(sizeof(DevJob) == 64, "a device job is 64 bytes");

/* what k_sym_time leaves of a job for k_sym_pick and k_sym_record */
struct State {
	double  c[4];			/* rule 5 */
	double  mu, xr, xi, a0;
	int32_t first, n_sym, status;
	float   tau;
};

static_assert(sizeof(State) == 80, "a state is 80 bytes");

struct Params {
	const float2   *iq;
	float2         *out;
	const DevJob   *jobs;
	const uint32_t *fold_prefix;	/* [n_jobs + 1] fold tiles before job j */
	const uint32_t *pick_prefix;	/* [n_jobs + 1] reserved output tiles before job j */
	const double   *tw;
	double         *parts;
	double         *mom;
	State          *state;
	int32_t        *counts;		/* n_sym per job, for the host's counter */
	Record         *records;
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }
inline __host__ __device__ double quiet(double v) { return v != v ? (double)NAN : v; }

/* rule 1: one sample's |y|^2 */
inline __host__ __device__ double q_of(float fre, float fim)
{
	const double re = fre, im = fim;
	return (re * re) + (im * im);
}

/* rule 2: the line of the folded sums; X and a0 come in as 0.0 */
inline __host__ __device__ void line_of(const double *A, const double *tw, int sps, double &xr, double &xi, double &a0)
{
	for (int k = 0; k < kMaxSps && k < sps; k++) {
		const double a = A[k];
		xr = xr + (a * tw[2 * k]);
		xi = xi + (a * tw[2 * k + 1]);
		a0 = a0 + a;
	}
}

/* rules 3 to 5: the State of a job from its mode, its tau and its line */
inline __host__ __device__ void state_of(int n, int sps, int mode, float tau, double xr, double xi, double a0, State &st)
{
	st.xr = quiet(xr);
	st.xi = quiet(xi);
	st.a0 = quiet(a0);
	double e = (double)tau;
	if (mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE) {
		const float a = fosphor_amd_atan2_turns(-xi, xr);
		if (a != a) {
			st.c[0] = st.c[1] = st.c[2] = st.c[3] = st.mu = 0.0;
			st.first = st.n_sym = 0;
			st.status = FOSPHOR_AMD_SYMBOLS_NO_TIMING;
			st.tau = NAN;
			return;
		}
		e = (double)a;
		if (e < 0.0)
			e = e + 1.0;
		if (!(e < 1.0))
			e = 0.0;
		e = e + 0.0;
	}
	const double base = e * (double)sps;
	const int i0 = (int)floor(base);
	const double mu = base - (double)i0;
	const double u = mu + 1.0, b = mu - 1.0, c = mu - 2.0;
	st.c[0] = -(((mu * b) * c) / 6.0);
	st.c[1] = ((u * b) * c) / 2.0;
	st.c[2] = -(((u * mu) * c) / 2.0);
	st.c[3] = ((u * mu) * b) / 6.0;
	st.mu = mu;
	st.first = i0 >= 1 ? i0 : sps;
	st.n_sym = n - 3 - st.first < 0 ? 0 : (n - 3 - st.first) / sps + 1;
	st.status = FOSPHOR_AMD_SYMBOLS_OK;
	st.tau = (float)e;
}

/* rule 5: one component of one symbol */
inline __host__ __device__ float interp(const double *c, float y_1, float y0, float y1, float y2)
{
	const double s = (((c[0] * (double)y_1) + (c[1] * (double)y0)) + (c[2] * (double)y1)) + (c[3] * (double)y2);
	return quiet((float)s);
}

/* rule 6: the six terms of one symbol */
inline __host__ __device__ void moment_terms(float fr, float fi, double *t)
{
	const double sr = fr, si = fi;
	const double w = (sr * sr) + (si * si);
	const double ar = (sr * sr) - (si * si), ai = (sr * si) + (sr * si);
	t[0] = w;
	t[1] = w * w;
	t[2] = ar;
	t[3] = ai;
	t[4] = (ar * ar) - (ai * ai);
	t[5] = (ar * ai) + (ar * ai);
}

inline __host__ __device__ void record_of(const State &st, const double *m, Record &r)
{
	r.n_sym = st.n_sym;
	r.first = st.first;
	r.tau = st.tau;
	r.status = st.status;
	r.mu = st.mu;
	r.x_re = st.xr;
	r.x_im = st.xi;
	r.a0 = st.a0;
	r.m2 = quiet(m[0]);
	r.m4 = quiet(m[1]);
	r.z2_re = quiet(m[2]);
	r.z2_im = quiet(m[3]);
	r.z4_re = quiet(m[4]);
	r.z4_im = quiet(m[5]);
}

/* the wave's own stores to LDS before its loads from it (the form of fosphor_kernels.hip) */
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads)
void k_sym_fold(const Params p)
{
	__shared__ double s_q[kFoldImage];
	__shared__ double s_b[kBlock];
	const int t = threadIdx.x;
	const int j = job_table::find_job(p.fold_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.fold_prefix[j]);
	const int sps = job.sps;
	const int syms = min(job.n / sps - c * kTile, kTile);			/* 1 .. kTile by the prefix */
	const int pb = kBlock / sps;						/* blocks of a piece: pb sps <= 64 chains, pb 64 sps <= 4096 samples */
	const int row = kBlock * sps;						/* samples of a block; its row is row + sps doubles */
	const int b = t / sps, k = t - b * sps;					/* the chain of lane t < pb sps */
	const float2 *tile = p.iq + job.offset + (int64_t)c * kTile * sps;
	double acc = 0.0;
	for (int s0 = 0; s0 < syms; s0 += pb * kBlock) {
		const int piece = min(syms - s0, pb * kBlock);			/* symbols of the piece */
		const int count = piece * sps;					/* samples: at most 4096, inside the job's R sps */
		const float2 *y = tile + s0 * sps;
		/* y[0 .. count) by 16-byte loads from the first 16-byte boundary on (fosphor_jobs.h); sample i lands at i + (i / row) sps */
		const job_table::Span s = job_table::split_span(y, count);
		if (t == 0 && s.head)
			s_q[0] = q_of(y[0].x, y[0].y);
		for (int g = t; g < s.pairs; g += kThreads) {
			const float4 v = *reinterpret_cast<const float4 *>(y + s.head + 2 * g);
			const int i = s.head + 2 * g;
			s_q[i + (i / row) * sps] = q_of(v.x, v.y);
			s_q[i + 1 + ((i + 1) / row) * sps] = q_of(v.z, v.w);
		}
		if (t == kThreads - 1 && s.tail < count)
			s_q[s.tail + (s.tail / row) * sps] = q_of(y[s.tail].x, y[s.tail].y);
		__syncthreads();
		if (t < pb * sps) {
			const int rows = min(piece - b * kBlock, kBlock);	/* below 1 for a block the piece does not have */
			const double *v = s_q + b * (row + sps) + k;
			double run = 0.0;
			for (int r = 0; r < kBlock && r < rows; r++)
				run = run + v[r * sps];
			s_b[t] = run;
		}
		wave_lds_sync();						/* the chains and the lanes below are wave 0's */
		if (t < sps) {
			const int blocks = (piece + kBlock - 1) / kBlock;
			for (int bb = 0; bb < pb && bb < blocks; bb++)
				acc = acc + s_b[bb * sps + t];
		}
		__syncthreads();						/* the image is free */
	}
	if (t < sps)
		p.parts[job.part0 + (int64_t)c * sps + t] = acc;
}

__global__ __launch_bounds__(kThreads)
void k_sym_time(const Params p)
{
	__shared__ double s_a[kWaves][kBlock];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	double xr = 0.0, xi = 0.0, a0 = 0.0;
	if (job.mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE) {
		const int R = job.n / job.sps;
		const int tiles = (R + kTile - 1) / kTile;
		double A = 0.0;
		if (lane < job.sps) {
			const double *T = p.parts + job.part0 + lane;
#pragma unroll 8							/* eight loads in flight; the additions keep their order */
			for (int c = 0; c < tiles; c++)
				A = A + T[(int64_t)c * job.sps];
		}
		s_a[wave][lane] = A;
		wave_lds_sync();
		line_of(s_a[wave], p.tw + job.tw0, job.sps, xr, xi, a0);	/* every lane, the same values in the same order */
	}
	State st;
	state_of(job.n, job.sps, job.mode, job.tau, xr, xi, a0, st);
	if (lane == 0)
		p.state[j] = st;
}

__global__ __launch_bounds__(kThreads)
void k_sym_pick(const Params p)
{
	__shared__ __align__(16) float2 s_y[kStage + 2];
	__shared__ double s_t[kWaves][kMoments][kBlock + 1];
	__shared__ double s_bs[kMoments][kBlock + 1];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int j = job_table::find_job(p.pick_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const State st = p.state[j];
	const int j0 = (int)(blockIdx.x - p.pick_prefix[j]) * kTile;		/* the tile's first symbol: below max_out by the prefix */
	if (j0 >= st.n_sym)							/* the whole work-group: a reserved tile without a symbol */
		return;
	const int syms = min(st.n_sym - j0, kTile);
	const int sps = job.sps;
	const float2 *y = p.iq + job.offset;
	float2 *out = p.out + job.out_offset + j0;
	for (int s0 = 0; s0 < syms; s0 += kPass) {
		const int count = min(syms - s0, kPass);			/* symbols of the pass, lane t has symbol j0 + s0 + t */
		const float2 *span = y + (st.first - 1) + (int64_t)(j0 + s0) * sps;	/* y[g - 1] of the pass's first symbol: first >= 1 */
		float2 v0, v1, v2, v3;
		v0 = v1 = v2 = v3 = make_float2(0.0f, 0.0f);
		if (sps <= kStageSps) {
			/* the last symbol of the pass ends at g + 2 <= n - 1 by n_sym: the span is inside the job */
			const int at = job_table::load_span<kThreads>(s_y, span, (count - 1) * sps + 4, t);
			__syncthreads();
			if (t < count) {
				const float2 *v = s_y + at + t * sps;
				v0 = v[0]; v1 = v[1]; v2 = v[2]; v3 = v[3];
			}
		} else if (t < count) {
			const float2 *v = span + t * sps;
			v0 = v[0]; v1 = v[1]; v2 = v[2]; v3 = v[3];
		}
		double term[kMoments];
#pragma unroll
		for (int m = 0; m < kMoments; m++)
			term[m] = 0.0;
		if (t < count) {
			const float sr = interp(st.c, v0.x, v1.x, v2.x, v3.x), si = interp(st.c, v0.y, v1.y, v2.y, v3.y);
			out[s0 + t] = make_float2(sr, si);
			moment_terms(sr, si, term);
		}
		/* the wave's 64 symbols are block (s0 / 64) + wave of the tile: lane m adds its term m over them, lanes ascending */
#pragma unroll
		for (int m = 0; m < kMoments; m++)
			s_t[wave][m][lane] = term[m];
		wave_lds_sync();
		const int in_block = min(count - wave * kBlock, kBlock);
		if (lane < kMoments && in_block > 0) {
			double run = 0.0;
			for (int l = 0; l < kBlock && l < in_block; l++)
				run = run + s_t[wave][lane][l];
			s_bs[lane][(s0 >> 6) + wave] = run;
		}
		__syncthreads();						/* s_y and s_t are free; the block sums are written */
	}
	if (t < kMoments) {
		const int blocks = (syms + kBlock - 1) / kBlock;
		double T = 0.0;
		for (int b = 0; b < kBlock && b < blocks; b++)
			T = T + s_bs[t][b];
		p.mom[(job.mom0 + (j0 / kTile)) * kMoments + t] = T;
	}
}

__global__ __launch_bounds__(kThreads)
void k_sym_record(const Params p)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const State st = p.state[j];
	const int tiles = min((st.n_sym + kTile - 1) / kTile, job.tiles_max);	/* the tiles that k_sym_pick wrote */
	double S = 0.0;
	if (lane < kMoments) {
		const double *T = p.mom + job.mom0 * kMoments + lane;
#pragma unroll 8							/* eight loads in flight; the additions keep their order */
		for (int c = 0; c < tiles; c++)
			S = S + T[(int64_t)c * kMoments];
	}
	double m[kMoments];
#pragma unroll
	for (int k = 0; k < kMoments; k++)
		m[k] = __shfl(S, k);
	if (lane == 0) {
		Record r;
		record_of(st, m, r);
		p.records[j] = r;
		p.counts[j] = st.n_sym;
	}
}

/* rule 2's table of one sps */
void twiddles_of(int sps, double *out)
{
	const long double quarter = 1.57079632679489661923132169163975144L;	/* pi / 2 */
	for (int k = 0; k < sps; k++) {
		const int quad = 4 * k / sps, rem = 4 * k - quad * sps;		/* the angle is (quad + rem / sps) quarter turns */
		const bool swap = 2 * rem > sps;
		const int r = swap ? sps - rem : rem;				/* r / sps <= 1 / 2: the first octant */
		double c = (double)cosl(quarter * r / sps), s = (double)sinl(quarter * r / sps);
		if (r == 0) {
			c = 1.0;
			s = 0.0;
		}
		if (2 * r == sps)
			c = s = sqrt(0.5);
		if (swap)
			std::swap(c, s);
		double cr = c, sr = s;						/* cos and sin of the whole angle */
		if (quad == 1) {
			cr = 0.0 - s; sr = c;
		} else if (quad == 2) {
			cr = 0.0 - c; sr = 0.0 - s;
		} else if (quad == 3) {
			cr = s; sr = 0.0 - c;
		}
		out[2 * k] = cr + 0.0;
		out[2 * k + 1] = (0.0 - sr) + 0.0;
	}
}

struct Plan {
	long long tiles_fold, tiles_pick, jobs[2], samples;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_SYMBOLS_MAX_JOBS) || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { 0, 0, { 0, 0 }, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || !timing_ok(b.sps, b.mode, b.tau) || b.reserved[0] || b.reserved[1])
			return -EINVAL;
		const int64_t max_out = max_out_of(b.n, b.sps);
		const long long fold = b.mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE ? b.n / b.sps : 0;
		if (!job_table::inside(b.out_offset, max_out, out_capacity) || !job_table::add_groups(pl.tiles_fold, fold, kTile) ||
		    !job_table::add_groups(pl.tiles_pick, max_out, kTile))
			return -EINVAL;
		pl.jobs[b.mode]++;
		pl.samples += b.n;
		if (max_out > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + max_out));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

/* the three-level order of rules 1 and 6 on the host: terms come in ascending order, one add() each */
struct Ordered {
	double block, tile, job;
	int n;
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

extern "C" int fosphor_amd_symbols_host(const float *iq, int64_t n_samples, const struct fosphor_amd_symbols_job *jobs, int n_jobs,
                                        struct fosphor_amd_symbols_record *records, float *out, int64_t out_capacity)
{
	if (!iq || !records || !out || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7) || ((uintptr_t)out & 7))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, nullptr))
		return -EINVAL;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const float *y = iq + 2 * b.offset;
		double A[kMaxSps], tw[2 * kMaxSps], xr = 0.0, xi = 0.0, a0 = 0.0;
		if (b.mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE) {
			const int R = b.n / b.sps;
			for (int k = 0; k < b.sps; k++) {
				Ordered sum;
				for (int r = 0; r < R; r++) {
					const int64_t m = (int64_t)r * b.sps + k;
					sum.add(q_of(y[2 * m], y[2 * m + 1]));
				}
				A[k] = sum.sum();
			}
			twiddles_of(b.sps, tw);
			line_of(A, tw, b.sps, xr, xi, a0);
		}
		State st;
		state_of(b.n, b.sps, b.mode, b.tau, xr, xi, a0, st);
		Ordered sums[kMoments];
		float *o = out + 2 * b.out_offset;
		for (int s = 0; s < st.n_sym; s++) {
			const float *v = y + 2 * ((int64_t)st.first - 1 + (int64_t)s * b.sps);
			double term[kMoments];
			o[2 * s] = interp(st.c, v[0], v[2], v[4], v[6]);
			o[2 * s + 1] = interp(st.c, v[1], v[3], v[5], v[7]);
			moment_terms(o[2 * s], o[2 * s + 1], term);
			for (int m = 0; m < kMoments; m++)
				sums[m].add(term[m]);
		}
		double m[kMoments];
		for (int k = 0; k < kMoments; k++)
			m[k] = sums[k].sum();
		Record r;
		memset(&r, 0, sizeof(r));
		record_of(st, m, r);
		records[i] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_symbols_max_out(int32_t n, int sps)
{
	if (n < 0 || !sps_ok(sps))
		return -EINVAL;
	return max_out_of(n, sps);
}

extern "C" int fosphor_amd_symbols_twiddles(int sps, double *out)
{
	if (!sps_ok(sps) || !out)
		return -EINVAL;
	twiddles_of(sps, out);
	return 0;
}

static int job_over(int64_t offset, int32_t n, int sps, int mode, float tau, struct fosphor_amd_symbols_job *job)
{
	if (!job || offset < 0 || n < 0 || !timing_ok(sps, mode, tau))
		return -EINVAL;
	job->offset = offset;
	job->out_offset = 0;
	job->n = n;
	job->sps = sps;
	job->mode = mode;
	job->tau = tau;
	job->reserved[0] = job->reserved[1] = 0;
	return 0;
}

extern "C" int fosphor_amd_symbols_from_extract(const struct fosphor_amd_extract_job *e, int sps, int mode, float tau,
                                                struct fosphor_amd_symbols_job *job)
{
	return e ? job_over(e->out_offset, e->n_out, sps, mode, tau, job) : -EINVAL;
}

extern "C" int fosphor_amd_symbols_from_resample(const struct fosphor_amd_resample_job *r, int sps, int mode, float tau,
                                                 struct fosphor_amd_symbols_job *job)
{
	return r ? job_over(r->out_offset, r->n_out, sps, mode, tau, job) : -EINVAL;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_symbols_derive(const struct fosphor_amd_symbols_record *r, int sps, double sample_rate,
                                          struct fosphor_amd_symbols_values *v)
{
	if (!r || !v || !sps_ok(sps) || !(sample_rate > 0.0) || !(sample_rate < INFINITY))
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	v->tau = finite_or_zero((double)r->tau);
	v->symbol_rate = sample_rate / sps;
	if (r->n_sym <= 0)
		return 0;
	const double n = r->n_sym, M2 = r->m2 / n, M4 = r->m4 / n;
	v->t_first = finite_or_zero(((double)r->first + r->mu) / sample_rate);
	if (r->a0 > 0.0)
		v->timing_depth = finite_or_zero(2.0 * hypot(r->x_re, r->x_im) / r->a0);
	v->sym_power = finite_or_zero(M2);
	const double S2 = 2.0 * M2 * M2 - M4;
	if (S2 > 0.0) {
		const double S = sqrt(S2), N = M2 - S;
		if (S > 0.0 && N > 0.0)
			v->snr_db = finite_or_zero(10.0 * log10(S / N));
	}
	v->phase2 = finite_or_zero(atan2(r->z2_im, r->z2_re) / 2.0);
	v->phase4 = finite_or_zero(atan2(r->z4_im, r->z4_re) / 4.0);
	if (r->m2 > 0.0)
		v->lock2 = finite_or_zero(hypot(r->z2_re, r->z2_im) / r->m2);
	if (r->m4 > 0.0)
		v->lock4 = finite_or_zero(hypot(r->z4_re, r->z4_im) / r->m4);
	return 0;
}

extern "C" int fosphor_amd_symbols_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_SYMBOLS_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_SYMBOLS, FOSPHOR_AMD_SYMBOLS_STATS, stats);
}

extern "C" int fosphor_amd_symbols(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                   const struct fosphor_amd_symbols_job *jobs, int n_jobs,
                                   struct fosphor_amd_symbols_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order, the prefix of their fold tiles, the prefix of their reserved output tiles;
	 * behind it, in doubles: a twiddle table per distinct sps, the fold partials, the pick partials, the states, the counts */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2];
	prefix[0].assign(1, 0u);
	prefix[1].assign(1, 0u);
	std::map<int, int> tw_at_of;
	std::vector<double> tw;
	int64_t part0 = 0, mom0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!tw_at_of.count(b.sps)) {
			tw_at_of[b.sps] = (int)tw.size();
			tw.resize(tw.size() + 2 * b.sps);
			twiddles_of(b.sps, tw.data() + tw_at_of[b.sps]);
		}
		DevJob d;
		memset(&d, 0, sizeof(d));
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.part0 = part0;
		d.mom0 = mom0;
		d.n = b.n;
		d.sps = b.sps;
		d.mode = b.mode;
		d.tw0 = tw_at_of[b.sps];
		d.tiles_max = (int32_t)job_table::groups_of(max_out_of(b.n, b.sps), kTile);
		d.tau = b.tau;
		const long long fold = b.mode == FOSPHOR_AMD_SYMBOLS_ESTIMATE ? job_table::groups_of(b.n / b.sps, kTile) : 0;
		part0 += fold * b.sps;
		mom0 += d.tiles_max;
		prefix[0].push_back(prefix[0].back() + (uint32_t)fold);
		prefix[1].push_back(prefix[1].back() + (uint32_t)d.tiles_max);
		form[0].push_back(d);
	}
	const size_t n_tw = tw.size(), n_state = (size_t)n_jobs * (sizeof(State) / sizeof(double)), n_counts = ((size_t)n_jobs + 1) / 2;
	job_table::Table table = job_table::pack_table(form, prefix, n_tw + (size_t)part0 + (size_t)mom0 * kMoments + n_state + n_counts,
	                                               sizeof(double));
	const size_t tw_at = table.parts_at;
	table.image.resize(tw_at + sizeof(double) * n_tw);
	memcpy(table.image.data() + tw_at, tw.data(), sizeof(double) * n_tw);

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_SYMBOLS);
	stats[FOSPHOR_AMD_SYMBOLS_CALLS]++;
	stats[FOSPHOR_AMD_SYMBOLS_JOBS_ESTIMATE] += plan.jobs[FOSPHOR_AMD_SYMBOLS_ESTIMATE];
	stats[FOSPHOR_AMD_SYMBOLS_JOBS_FIXED] += plan.jobs[FOSPHOR_AMD_SYMBOLS_FIXED];
	stats[FOSPHOR_AMD_SYMBOLS_SAMPLES] += plan.samples;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_SYMBOLS, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = static_cast<float2 *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.fold_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.pick_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[1]);
	p.tw = reinterpret_cast<const double *>(d + tw_at);
	p.parts = reinterpret_cast<double *>(d + tw_at) + n_tw;
	p.mom = p.parts + part0;
	p.state = reinterpret_cast<State *>(p.mom + mom0 * kMoments);
	p.counts = reinterpret_cast<int32_t *>(reinterpret_cast<double *>(p.state) + n_state);
	p.records = d_records;
	p.n_jobs = n_jobs;
	const unsigned per_wave = (unsigned)job_table::groups_of(n_jobs, kWaves);
	int rv = 0;
	if (plan.tiles_fold)
		rv = job_table::launch<kThreads>(k_sym_fold, (unsigned)plan.tiles_fold, st, p, stats, FOSPHOR_AMD_SYMBOLS_K_FOLD);
	if (!rv)
		rv = job_table::launch<kThreads>(k_sym_time, per_wave, st, p, stats, FOSPHOR_AMD_SYMBOLS_K_TIME);
	if (plan.tiles_pick && !rv)
		rv = job_table::launch<kThreads>(k_sym_pick, (unsigned)plan.tiles_pick, st, p, stats, FOSPHOR_AMD_SYMBOLS_K_PICK);
	if (!rv)
		rv = job_table::launch<kThreads>(k_sym_record, per_wave, st, p, stats, FOSPHOR_AMD_SYMBOLS_K_RECORD);
	std::vector<int32_t> counts(n_jobs, 0);
	if (!rv && hipMemcpyAsync(counts.data(), p.counts, sizeof(int32_t) * n_jobs, hipMemcpyDeviceToHost, st) != hipSuccess)
		rv = -EIO;
	rv = job_table::drain(st, rv);
	if (!rv)
		for (int i = 0; i < n_jobs; i++)
			stats[FOSPHOR_AMD_SYMBOLS_SYMBOLS] += counts[i];
	return rv;
}
