/*
 * fosphor_psd.hip -- the power spectrum of burst IQ where it lies: Welch's method per job, a batched radix-2 FFT in double in LDS,
 * peak, occupied bandwidth, x-dB bandwidth and spectral moments (include/fosphor_amd_psd.h)
 *
 * A read-only pass over the CALLER's float32 IQ (what fosphor_amd_extract wrote) and windows, in a file of its own: nothing here is
 * on the process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table, the
 * prefixes of tile counts, the twiddles and the tiles' partial spectra).
 *
 *   k_psd_group    L >= 256: a work-group of 256 lanes owns one tile (32 segments) of one job, which it finds in the prefix
 *                  (fosphor_jobs.h).  Per segment: load_span() stages the samples, pre and window write the bit-reversed image of L
 *                  complex doubles, the stages run in place with one barrier each -- a butterfly's two elements belong to one lane
 *                  for the length of a stage -- and each lane adds its L / 256 bins of |X|^2 in registers.
 *   k_psd_wave     L <= 128: the same body (psd_tile) with a wave where the work-group was; four tiles to a work-group, each wave
 *                  on its own LDS slice, no work-group barrier anywhere.
 *   k_psd_combine  a wave per job adds the job's tiles bin by bin in ascending tile order, divides, writes the trace, keeps P32 in
 *                  LDS and computes the record in the two-level order of rule 5: lane k owns block k of L / 64 indices.
 * The image is two arrays of doubles, re and im, padded by one double after every 16 (pad()): the bit-reversed writes of 64
 * consecutive lanes are L / 64 doubles apart, which without the padding is one bank for all of them at L = 1024.
 * Every segment is computed by the operations of pre_of() and butterfly(), on the device and in fosphor_amd_psd_host alike; the
 * build's -ffp-contract=off keeps each of them one rounding.  No atomics of any kind, no work-group waits for another, every loop
 * carries its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_psd.h"

namespace {

typedef struct fosphor_amd_psd_job Job;
typedef struct fosphor_amd_psd_record Record;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = FOSPHOR_AMD_PSD_TILE;
constexpr int kMinLog = FOSPHOR_AMD_PSD_MIN_LOG;
constexpr int kMaxLog = FOSPHOR_AMD_PSD_MAX_LOG;
constexpr int kWaveLog = 7;					/* the longest transform of the WAVE form */
constexpr int kMaxL = 1 << kMaxLog;
constexpr int kTwiddles = kMaxL / 2;
constexpr int kBlocks = 64;					/* of rule 5 */
constexpr int kNone = 0x7fffffff;				/* a minimum over nothing, until the record is written */
enum { kGroup, kWave };						/* the forms */

static_assert(FOSPHOR_AMD_PSD_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 56, "the job is 56 bytes");
static_assert(sizeof(Record) == 64, "the record is 64 bytes");
static_assert(kMinLog == 6 && kBlocks == 1 << kMinLog, "a block of rule 5 has at least one index");

inline bool log_ok(int log) { return log >= kMinLog && log <= kMaxLog; }
inline bool pre_ok(int pre) { return pre >= FOSPHOR_AMD_PSD_PRE_NONE && pre <= FOSPHOR_AMD_PSD_PRE_MAGSQ; }
inline bool trace_ok(int trace) { return trace == FOSPHOR_AMD_PSD_TRACE_NONE || trace == FOSPHOR_AMD_PSD_TRACE_POWER; }
inline bool ratio_ok(float v) { return v > 0.0f && v <= 1.0f; }			/* a NaN is not */
inline int form_of(int log) { return log > kWaveLog ? kGroup : kWave; }

inline int n_seg_of(int n, int L, int hop) { return n < L ? 0 : (n - L) / hop + 1; }	/* rule 1 */
inline int n_out_of(int trace, int n_seg, int L) { return trace == FOSPHOR_AMD_PSD_TRACE_POWER && n_seg > 0 ? L : 0; }

/* a job on the device; the two forms' jobs lie one behind the other, so k_psd_combine sees all of them */
struct DevJob {
	int64_t offset;
	int64_t out_offset;
	int64_t win_offset;
	int64_t part0;			/* doubles into the partials: tile c of the job is parts[part0 + c L .. + L) */
	int32_t n_seg;
	int32_t fft_len_log;
	int32_t hop;
	int32_t pre;
	int32_t trace;
	int32_t record;			/* the job's place in the caller's order */
	float   obw_fraction;
	float   xdb_ratio;
};

static_assert(sizeof(DevJob) == 64, "a device job is 64 bytes");

struct Params {
	const float2   *iq;
	const float    *win;
	const DevJob   *jobs;		/* of the form; all of them for k_psd_combine */
	const uint32_t *prefix;		/* [n_jobs + 1] tiles before job j of the form */
	const double   *tw;		/* 512 (re, im) pairs */
	double         *parts;
	Record         *records;
	float          *out;
	int n_jobs;
};

inline __host__ __device__ float quiet(float v) { return v != v ? NAN : v; }		/* rule 4: one NaN */
inline __host__ __device__ double quiet(double v) { return v != v ? (double)NAN : v; }

inline __host__ __device__ int pad(int r) { return r + (r >> 4); }

inline __host__ __device__ int bitrev(int i, int log)
{
	unsigned v = (unsigned)i, r = 0;
	for (int b = 0; b < kMaxLog && b < log; b++) {
		r = (r << 1) | (v & 1);
		v >>= 1;
	}
	return (int)r;
}

/* rule 2: the windowed, pre-transformed sample */
inline __host__ __device__ void pre_of(int pre, float fre, float fim, float fw, double &xr, double &xi)
{
	const double re = fre, im = fim, w = fw;
	double zr = re, zi = im;
	if (pre == FOSPHOR_AMD_PSD_PRE_MAGSQ) {
		zr = (re * re) + (im * im);
		zi = 0.0;
	} else if (pre != FOSPHOR_AMD_PSD_PRE_NONE) {
		zr = (re * re) - (im * im);
		zi = (re * im) + (re * im);
		if (pre == FOSPHOR_AMD_PSD_PRE_FOURTH) {
			const double sr = zr, si = zi;
			zr = (sr * sr) - (si * si);
			zi = (sr * si) + (sr * si);
		}
	}
	xr = w * zr;
	xi = w * zi;
}

/* rule 3: one butterfly, in place */
inline __host__ __device__ void butterfly(double wr, double wi, double &ur, double &ui, double &vr, double &vi)
{
	const double tr = (wr * vr) - (wi * vi);
	const double ti = (wr * vi) + (wi * vr);
	const double ar = ur, ai = ui;
	ur = ar + tr;
	ui = ai + ti;
	vr = ar - tr;
	vi = ai - ti;
}

/* the wave's own stores to LDS before its loads from it (the form of fosphor_kernels.hip) */
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int kLanes>
__device__ __forceinline__ void team_sync()
{
	if constexpr (kLanes == kThreads)
		__syncthreads();
	else
		wave_lds_sync();
}

/* Tile c of `job` by a team of kLanes lanes of which this is lane t; kLog is the longest transform of the form.  s_tw is the form's
 * share of the table: s_tw[e] = tw[e << (kMaxLog - kLog)], so stage tt takes W = s_tw[j << (kLog - tt)] = tw[j * (512 / h)]. */
template <int kLanes, int kLog>
__device__ __forceinline__ void psd_tile(const Params &p, const DevJob &job, int c, int t,
                                         double *a_re, double *a_im, float2 *staged, float *s_win, double2 *s_tw)
{
	constexpr int kFormL = 1 << kLog, kBins = kFormL / kLanes, kFly = kFormL / 2 / kLanes;
	static_assert(kBins >= 1 && kFly >= 1, "a lane has a bin and a butterfly at the form's longest transform");
	const int log = job.fft_len_log, L = 1 << log;				/* L <= kFormL by the form */
	const float *w = p.win + job.win_offset;
	for (int i = t; i < L; i += kLanes)
		s_win[i] = w[i];
	for (int e = t; e < kFormL / 2; e += kLanes) {
		const int m = e << (kMaxLog - kLog);
		s_tw[e] = make_double2(p.tw[2 * m], p.tw[2 * m + 1]);
	}
	double acc[kBins];
#pragma unroll
	for (int k = 0; k < kBins; k++)
		acc[k] = 0.0;
	const int s0 = c * kTile, s1 = min(s0 + kTile, job.n_seg);		/* s0 < n_seg by the prefix */
	const float2 *y = p.iq + job.offset;
	for (int s = s0; s < s1; s++) {
		/* the job has them: s hop + L <= n.  The image is free: every lane read its bins before it came here, and the barrier
		 * below is between that and the first write */
		const int at = job_table::load_span<kLanes>(staged, y + (int64_t)s * job.hop, L, t);
		team_sync<kLanes>();
#pragma unroll
		for (int k = 0; k < kBins; k++) {
			const int i = t + kLanes * k;
			if (i < L) {
				const float2 v = staged[at + i];
				const int r = pad(bitrev(i, log));
				pre_of(job.pre, v.x, v.y, s_win[i], a_re[r], a_im[r]);
			}
		}
		for (int tt = 1; tt <= kLog && tt <= log; tt++) {
			team_sync<kLanes>();
			const int h = 1 << (tt - 1);
#pragma unroll
			for (int k = 0; k < kFly; k++) {
				const int q = t + kLanes * k;
				if (q < L / 2) {
					const int j = q & (h - 1);
					const int i0 = pad(((q - j) << 1) + j), i1 = pad(((q - j) << 1) + j + h);
					const double2 W = s_tw[j << (kLog - tt)];
					double ur = a_re[i0], ui = a_im[i0], vr = a_re[i1], vi = a_im[i1];
					butterfly(W.x, W.y, ur, ui, vr, vi);
					a_re[i0] = ur; a_im[i0] = ui;
					a_re[i1] = vr; a_im[i1] = vi;
				}
			}
		}
		team_sync<kLanes>();
#pragma unroll
		for (int k = 0; k < kBins; k++) {
			const int b = t + kLanes * k;
			if (b < L) {
				const double xr = a_re[pad(b)], xi = a_im[pad(b)];
				acc[k] = acc[k] + ((xr * xr) + (xi * xi));
			}
		}
	}
	double *T = p.parts + job.part0 + (int64_t)c * L;
#pragma unroll
	for (int k = 0; k < kBins; k++) {
		const int b = t + kLanes * k;
		if (b < L)
			T[b] = acc[k];
	}
}

constexpr int kGroupL = 1 << kMaxLog, kWaveL = 1 << kWaveLog;
constexpr int kGroupImage = kGroupL + kGroupL / 16, kWaveImage = kWaveL + kWaveL / 16;

__global__ __launch_bounds__(kThreads)
void k_psd_group(const Params p)
{
	__shared__ double s_re[kGroupImage], s_im[kGroupImage];
	__shared__ __align__(16) float2 s_staged[kGroupL + 2];
	__shared__ float s_win[kGroupL];
	__shared__ __align__(16) double2 s_tw[kGroupL / 2];
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	psd_tile<kThreads, kMaxLog>(p, job, (int)(blockIdx.x - p.prefix[j]), threadIdx.x, s_re, s_im, s_staged, s_win, s_tw);
}

__global__ __launch_bounds__(kThreads)
void k_psd_wave(const Params p)
{
	__shared__ double s_re[kWaves][kWaveImage], s_im[kWaves][kWaveImage];
	__shared__ __align__(16) float2 s_staged[kWaves][kWaveL + 2];
	__shared__ float s_win[kWaves][kWaveL];
	__shared__ __align__(16) double2 s_tw[kWaves][kWaveL / 2];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t g = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;	/* the tile: below 2^31 by the refusals */
	if (g >= p.prefix[p.n_jobs])						/* the whole wave; there is no barrier below */
		return;
	const int j = job_table::find_job(p.prefix, p.n_jobs, g);
	const DevJob job = p.jobs[j];
	psd_tile<64, kWaveLog>(p, job, (int)(g - p.prefix[j]), lane, s_re[wave], s_im[wave], s_staged[wave], s_win[wave], s_tw[wave]);
}

/* the running peak: does (v, i) beat (best, best_i)?  Larger first, then the smaller index; a NaN never */
inline __host__ __device__ bool beats(float v, int i, float best, int best_i)
{
	return i >= 0 && v == v && (best_i < 0 || v > best || (v == best && i < best_i));
}

inline __host__ __device__ bool finite_positive(double v) { return v > 0.0 && v < (double)INFINITY; }

inline __host__ __device__ void record_clear(Record &r, int n_seg, int L, double U)
{
	r.n_seg = n_seg;
	r.fft_len = L;
	r.peak_bin = r.obw_lo = r.obw_hi = r.xdb_lo = r.xdb_hi = -1;
	r.peak_power = 0.0f;
	r.total = r.m1 = r.m2 = 0.0;
	r.win_energy = quiet(U);
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
	for (int d = 32; d; d >>= 1)
		v = min(v, __shfl_xor(v, d));
	return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
	for (int d = 32; d; d >>= 1)
		v = max(v, __shfl_xor(v, d));
	return v;
}

__global__ __launch_bounds__(kThreads)
void k_psd_combine(const Params p)
{
	__shared__ float s_p[kWaves][kMaxL];
	__shared__ double s_b[kWaves][3][kBlocks];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const int L = 1 << job.fft_len_log, half = L >> 1;
	float *P = s_p[wave];

	/* rule 4: U, i ascending; every lane adds the same values in the same order */
	const float *w = p.win + job.win_offset;
	for (int i = lane; i < L; i += 64)
		P[i] = w[i];
	wave_lds_sync();
	double U = 0.0;
	for (int i = 0; i < L; i++) {
		const double wi = P[i];
		U = U + (wi * wi);
	}
	wave_lds_sync();
	Record r;
	record_clear(r, job.n_seg, L, U);
	if (job.n_seg == 0) {							/* no segment, no tile, no trace */
		if (lane == 0)
			p.records[job.record] = r;
		return;
	}

	/* rule 4: the tiles in ascending order, the division, the trace */
	const int tiles = (job.n_seg + kTile - 1) / kTile;
	const double den = (double)job.n_seg * U;
	for (int i = lane; i < L; i += 64) {
		const double *T = p.parts + job.part0 + ((i + half) & (L - 1));
		double S = 0.0;
		for (int c = 0; c < tiles; c++)
			S = S + T[(int64_t)c * L];
		const float v = den == 0.0 ? 0.0f : quiet((float)(S / den));
		P[i] = v;
		if (job.trace == FOSPHOR_AMD_PSD_TRACE_POWER)
			p.out[job.out_offset + i] = v;
	}
	wave_lds_sync();

	/* rule 5: lane k owns block k */
	const int per = L >> 6, i0 = lane * per;
	double run_t = 0.0, run_1 = 0.0, run_2 = 0.0;
	float best = 0.0f;
	int best_i = -1;
	for (int k = 0; k < per; k++) {
		const int i = i0 + k;
		const float v = P[i];
		const double Pd = v, d = (double)(i - half);
		run_t = run_t + Pd;
		run_1 = run_1 + (d * Pd);
		run_2 = run_2 + ((d * d) * Pd);
		if (beats(v, i, best, best_i)) {
			best = v;
			best_i = i;
		}
	}
	s_b[wave][0][lane] = run_t;
	s_b[wave][1][lane] = run_1;
	s_b[wave][2][lane] = run_2;
	wave_lds_sync();
	double base_t = 0.0, base_1 = 0.0, base_2 = 0.0, mine = 0.0;		/* the serial prefix, the same in every lane */
#pragma unroll 4
	for (int k = 0; k < kBlocks; k++) {
		if (k == lane)
			mine = base_t;
		base_t = base_t + s_b[wave][0][k];
		base_1 = base_1 + s_b[wave][1][k];
		base_2 = base_2 + s_b[wave][2][k];
	}
	r.total = quiet(base_t);
	r.m1 = quiet(base_1);
	r.m2 = quiet(base_2);
#pragma unroll
	for (int d = 32; d; d >>= 1) {						/* the peak pair: the order does not matter */
		const float ov = __shfl_xor(best, d);
		const int oi = __shfl_xor(best_i, d);
		if (beats(ov, oi, best, best_i)) {
			best = ov;
			best_i = oi;
		}
	}
	int xlo = kNone, xhi = -1, olo = kNone, ohi = kNone;
	if (best_i >= 0) {
		r.peak_bin = best_i;
		r.peak_power = best;
		const float level = best * job.xdb_ratio;
		for (int k = 0; k < per; k++)
			if (P[i0 + k] >= level) {
				xlo = min(xlo, i0 + k);
				xhi = max(xhi, i0 + k);
			}
	}
	if (finite_positive(base_t)) {
		const double th = (1.0 - (double)job.obw_fraction) * 0.5;
		const double lo_thr = base_t * th, hi_thr = base_t - lo_thr;
		double run = 0.0;
		for (int k = 0; k < per; k++) {
			run = run + (double)P[i0 + k];
			const double cum = mine + run;
			if (cum > lo_thr)
				olo = min(olo, i0 + k);
			if (cum >= hi_thr)
				ohi = min(ohi, i0 + k);
		}
	}
	xlo = wave_min(xlo); xhi = wave_max(xhi); olo = wave_min(olo); ohi = wave_min(ohi);
	r.xdb_lo = xlo == kNone ? -1 : xlo;
	r.xdb_hi = xhi;
	r.obw_lo = olo == kNone ? -1 : olo;
	r.obw_hi = ohi == kNone ? -1 : ohi;
	if (lane == 0)
		p.records[job.record] = r;
}

/* the table of rule 3, built once */
const double *twiddles(void)
{
	static const std::vector<double> table = [] {
		const double pi = 3.14159265358979323846;
		double c[kMaxL / 4 + 1], s[kMaxL / 4 + 1];			/* the first quadrant, mirrored about its middle */
		for (int k = 0; k <= kMaxL / 8; k++) {
			c[k] = cos(2.0 * pi * k / kMaxL);
			s[k] = sin(2.0 * pi * k / kMaxL);
		}
		c[0] = 1.0; s[0] = 0.0;
		c[kMaxL / 8] = s[kMaxL / 8] = sqrt(0.5);
		for (int k = kMaxL / 8 + 1; k <= kMaxL / 4; k++) {
			c[k] = s[kMaxL / 4 - k];
			s[k] = c[kMaxL / 4 - k];
		}
		std::vector<double> t(2 * kTwiddles);
		for (int m = 0; m <= kMaxL / 4; m++) {
			t[2 * m] = c[m];
			t[2 * m + 1] = 0.0 - s[m];
		}
		for (int k = 1; k < kMaxL / 4; k++) {
			t[2 * (kMaxL / 4 + k)] = 0.0 - s[k];
			t[2 * (kMaxL / 4 + k) + 1] = 0.0 - c[k];
		}
		return t;
	}();
	return table.data();
}

struct Plan {
	long long tiles[2], segments;
	bool traces;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, int64_t n_win, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_PSD_MAX_JOBS) || n_samples < 0 || n_win < 0 || out_capacity < 0)
		return -EINVAL;
	Plan pl = { { 0, 0 }, 0, false };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || !log_ok(b.fft_len_log))
			return -EINVAL;
		const int L = 1 << b.fft_len_log;
		if (!job_table::inside(b.win_offset, L, n_win) || b.hop < 1 || b.hop > L)
			return -EINVAL;
		if (!pre_ok(b.pre) || !trace_ok(b.trace) || !ratio_ok(b.obw_fraction) || !ratio_ok(b.xdb_ratio))
			return -EINVAL;
		if (b.trace == FOSPHOR_AMD_PSD_TRACE_NONE && b.out_offset != 0)
			return -EINVAL;
		const int n_seg = n_seg_of(b.n, L, b.hop);
		const int64_t n_out = n_out_of(b.trace, n_seg, L);
		if (!job_table::inside(b.out_offset, n_out, out_capacity) || !job_table::add_groups(pl.tiles[form_of(b.fft_len_log)], n_seg, kTile))
			return -EINVAL;
		pl.segments += n_seg;
		pl.traces |= b.trace != FOSPHOR_AMD_PSD_TRACE_NONE;
		if (n_out > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + n_out));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

/* rules 2 to 4 on the host: S[b] of one job */
void spectrum(const float *y, const float *w, const Job &b, int n_seg, const double *tw, std::vector<double> &S)
{
	const int log = b.fft_len_log, L = 1 << log;
	std::vector<double> re(L), im(L), T(L);
	S.assign(L, 0.0);
	for (int s0 = 0; s0 < n_seg; s0 += kTile) {
		T.assign(L, 0.0);
		for (int s = s0; s < n_seg && s < s0 + kTile; s++) {
			const float *ys = y + 2 * ((int64_t)s * b.hop);
			for (int i = 0; i < L; i++) {
				const int r = bitrev(i, log);
				pre_of(b.pre, ys[2 * i], ys[2 * i + 1], w[i], re[r], im[r]);
			}
			for (int tt = 1; tt <= log; tt++) {
				const int h = 1 << (tt - 1);
				for (int k = 0; k < L; k += 2 * h)
					for (int j = 0; j < h; j++) {
						const int m = j * (kTwiddles / h);
						butterfly(tw[2 * m], tw[2 * m + 1], re[k + j], im[k + j], re[k + j + h], im[k + j + h]);
					}
			}
			for (int i = 0; i < L; i++)
				T[i] = T[i] + ((re[i] * re[i]) + (im[i] * im[i]));
		}
		for (int i = 0; i < L; i++)
			S[i] = S[i] + T[i];
	}
}

/* rule 5 on the host */
void record_of(const float *P, int L, float obw_fraction, float xdb_ratio, Record &r)
{
	const int per = L / kBlocks, half = L / 2;
	double base_t[kBlocks + 1], base_1 = 0.0, base_2 = 0.0;
	base_t[0] = 0.0;
	for (int k = 0; k < kBlocks; k++) {
		double run_t = 0.0, run_1 = 0.0, run_2 = 0.0;
		for (int i = k * per; i < (k + 1) * per; i++) {
			const double Pd = P[i], d = (double)(i - half);
			run_t = run_t + Pd;
			run_1 = run_1 + (d * Pd);
			run_2 = run_2 + ((d * d) * Pd);
			if (beats(P[i], i, r.peak_power, r.peak_bin)) {
				r.peak_power = P[i];
				r.peak_bin = i;
			}
		}
		base_t[k + 1] = base_t[k] + run_t;
		base_1 = base_1 + run_1;
		base_2 = base_2 + run_2;
	}
	const double total = base_t[kBlocks];
	r.total = quiet(total);
	r.m1 = quiet(base_1);
	r.m2 = quiet(base_2);
	if (r.peak_bin >= 0) {
		const float level = r.peak_power * xdb_ratio;
		for (int i = 0; i < L; i++)
			if (P[i] >= level) {
				if (r.xdb_lo < 0)
					r.xdb_lo = i;
				r.xdb_hi = i;
			}
	}
	if (finite_positive(total)) {
		const double th = (1.0 - (double)obw_fraction) * 0.5;
		const double lo_thr = total * th, hi_thr = total - lo_thr;
		for (int k = 0; k < kBlocks; k++) {
			double run = 0.0;
			for (int i = k * per; i < (k + 1) * per; i++) {
				run = run + (double)P[i];
				const double cum = base_t[k] + run;
				if (r.obw_lo < 0 && cum > lo_thr)
					r.obw_lo = i;
				if (r.obw_hi < 0 && cum >= hi_thr)
					r.obw_hi = i;
			}
		}
	}
}

} // namespace

extern "C" int fosphor_amd_psd_host(const float *iq, int64_t n_samples, const float *win, int64_t n_win,
                                    const struct fosphor_amd_psd_job *jobs, int n_jobs,
                                    struct fosphor_amd_psd_record *records, float *out, int64_t out_capacity)
{
	if (!iq || !win || !records || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7) || ((uintptr_t)win & 3) || ((uintptr_t)out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, n_win, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	if (plan.traces && !out)
		return -EINVAL;
	const double *tw = twiddles();
	std::vector<double> S;
	std::vector<float> P;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const int L = 1 << b.fft_len_log, n_seg = n_seg_of(b.n, L, b.hop);
		const float *w = win + b.win_offset;
		double U = 0.0;
		for (int k = 0; k < L; k++)
			U = U + ((double)w[k] * (double)w[k]);
		Record r;
		memset(&r, 0, sizeof(r));
		record_clear(r, n_seg, L, U);
		if (n_seg > 0) {
			spectrum(iq + 2 * b.offset, w, b, n_seg, tw, S);
			const double den = (double)n_seg * U;
			P.resize(L);
			for (int k = 0; k < L; k++)
				P[k] = den == 0.0 ? 0.0f : quiet((float)(S[(k + L / 2) & (L - 1)] / den));
			record_of(P.data(), L, b.obw_fraction, b.xdb_ratio, r);
			if (b.trace == FOSPHOR_AMD_PSD_TRACE_POWER)
				memcpy(out + b.out_offset, P.data(), sizeof(float) * L);
		}
		records[i] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_psd_n_seg(int32_t n, int fft_len_log, int hop)
{
	if (n < 0 || !log_ok(fft_len_log) || hop < 1 || hop > (1 << fft_len_log))
		return -EINVAL;
	return n_seg_of(n, 1 << fft_len_log, hop);
}

extern "C" int fosphor_amd_psd_window(int kind, int fft_len_log, float *out)
{
	if (kind < FOSPHOR_AMD_PSD_WINDOW_RECT || kind > FOSPHOR_AMD_PSD_WINDOW_BLACKMAN_HARRIS || !log_ok(fft_len_log) || !out)
		return -EINVAL;
	const int L = 1 << fft_len_log;
	const double pi = 3.14159265358979323846;
	for (int i = 0; i < L; i++) {
		const double x = 2.0 * pi * i / L;
		double w = 1.0;
		if (kind == FOSPHOR_AMD_PSD_WINDOW_HANN)
			w = 0.5 - 0.5 * cos(x);
		else if (kind == FOSPHOR_AMD_PSD_WINDOW_BLACKMAN_HARRIS)
			w = 0.35875 - 0.48829 * cos(x) + 0.14128 * cos(2.0 * x) - 0.01168 * cos(3.0 * x);
		out[i] = (float)w;
	}
	return 0;
}

extern "C" int fosphor_amd_psd_twiddles(double *out)
{
	if (!out)
		return -EINVAL;
	memcpy(out, twiddles(), sizeof(double) * 2 * kTwiddles);
	return 0;
}

extern "C" int fosphor_amd_psd_from_extract(const struct fosphor_amd_extract_job *e, int64_t win_offset, int fft_len_log, int hop,
                                            int pre, int trace, float obw_fraction, float xdb_ratio,
                                            struct fosphor_amd_psd_job *job)
{
	if (!e || !job || e->out_offset < 0 || e->n_out < 0 || win_offset < 0 || !log_ok(fft_len_log) || hop < 1 ||
	    hop > (1 << fft_len_log) || !pre_ok(pre) || !trace_ok(trace) || !ratio_ok(obw_fraction) || !ratio_ok(xdb_ratio))
		return -EINVAL;
	job->offset = e->out_offset;
	job->out_offset = 0;
	job->win_offset = win_offset;
	job->n = e->n_out;
	job->fft_len_log = fft_len_log;
	job->hop = hop;
	job->pre = pre;
	job->trace = trace;
	job->obw_fraction = obw_fraction;
	job->xdb_ratio = xdb_ratio;
	job->reserved = 0;
	return 0;
}

extern "C" double fosphor_amd_psd_ratio_from_db(double db)
{
	return db <= 0.0 ? pow(10.0, db / 10.0) : (double)NAN;
}

extern "C" int fosphor_amd_psd_derive(const struct fosphor_amd_psd_record *r, double sample_rate, struct fosphor_amd_psd_values *v)
{
	if (!r || !v || !(sample_rate > 0.0) || !(sample_rate < INFINITY))
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	if (r->n_seg <= 0 || r->fft_len <= 0 || !finite_positive(r->total))
		return 0;
	const double L = r->fft_len, bin = sample_rate / L, mean = r->m1 / r->total;
	const double var = r->m2 / r->total - mean * mean;
	v->mean_power = r->total / L;
	v->peak_freq = (r->peak_bin - L / 2.0) * bin;
	v->peak_db = 10.0 * log10((double)r->peak_power);
	v->centroid = mean * bin;
	v->rms_width = sqrt(var > 0.0 ? var : 0.0) * bin;
	/* the bins in double: a record is the caller's memory, and the sum or difference of two int32 of any value is exact there */
	v->obw = ((double)r->obw_hi - (double)r->obw_lo + 1.0) * bin;
	v->obw_centre = (((double)r->obw_lo + (double)r->obw_hi) * 0.5 - L / 2.0) * bin;
	v->xdb_bandwidth = ((double)r->xdb_hi - (double)r->xdb_lo + 1.0) * bin;
	return 0;
}

extern "C" int fosphor_amd_psd_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_PSD_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_PSD, FOSPHOR_AMD_PSD_STATS, stats);
}

extern "C" int fosphor_amd_psd(struct fosphor *self, const void *d_iq, int64_t n_samples,
                               const float *d_win, int64_t n_win,
                               const struct fosphor_amd_psd_job *jobs, int n_jobs,
                               struct fosphor_amd_psd_record *d_records,
                               float *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !d_win || !jobs || !d_records)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_win & 3) || ((uintptr_t)d_out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, n_win, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	if (plan.traces && !d_out)
		return -EINVAL;

	/* the table: GROUP jobs, WAVE jobs, their prefixes of tile counts; behind it the twiddles, then the tiles' partial spectra */
	std::vector<DevJob> form[2];
	std::vector<uint32_t> prefix[2];
	prefix[kGroup].assign(1, 0u);
	prefix[kWave].assign(1, 0u);
	int64_t part0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const int f = form_of(jobs[i].fft_len_log), L = 1 << jobs[i].fft_len_log;
		DevJob d;
		d.offset = jobs[i].offset;
		d.out_offset = jobs[i].out_offset;
		d.win_offset = jobs[i].win_offset;
		d.part0 = part0;
		d.n_seg = n_seg_of(jobs[i].n, L, jobs[i].hop);
		d.fft_len_log = jobs[i].fft_len_log;
		d.hop = jobs[i].hop;
		d.pre = jobs[i].pre;
		d.trace = jobs[i].trace;
		d.record = i;
		d.obw_fraction = jobs[i].obw_fraction;
		d.xdb_ratio = jobs[i].xdb_ratio;
		const long long tiles = job_table::groups_of(d.n_seg, kTile);
		part0 += tiles * L;
		prefix[f].push_back(prefix[f].back() + (uint32_t)tiles);
		form[f].push_back(d);
	}
	job_table::Table table = job_table::pack_table(form, prefix, (size_t)(2 * kTwiddles) + (size_t)part0, sizeof(double));
	const size_t tw_at = table.parts_at;
	table.image.resize(tw_at + sizeof(double) * 2 * kTwiddles);
	memcpy(table.image.data() + tw_at, twiddles(), sizeof(double) * 2 * kTwiddles);

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_PSD);
	stats[FOSPHOR_AMD_PSD_CALLS]++;
	stats[FOSPHOR_AMD_PSD_JOBS] += n_jobs;
	stats[FOSPHOR_AMD_PSD_SEGMENTS] += plan.segments;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_PSD, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.win = d_win;
	p.tw = reinterpret_cast<const double *>(d + tw_at);
	p.parts = reinterpret_cast<double *>(d + tw_at) + 2 * kTwiddles;
	p.records = d_records;
	p.out = d_out;
	int rv = 0;
	if (plan.tiles[kGroup]) {
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[kGroup]);
		p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[kGroup]);
		p.n_jobs = (int)form[kGroup].size();
		rv = job_table::launch<kThreads>(k_psd_group, (unsigned)plan.tiles[kGroup], st, p, stats, FOSPHOR_AMD_PSD_K_GROUP);
	}
	if (plan.tiles[kWave] && !rv) {
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[kWave]);
		p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[kWave]);
		p.n_jobs = (int)form[kWave].size();
		rv = job_table::launch<kThreads>(k_psd_wave, (unsigned)job_table::groups_of(plan.tiles[kWave], kWaves), st, p, stats,
		                                 FOSPHOR_AMD_PSD_K_WAVE);
	}
	if (!rv) {
		p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[kGroup]);		/* both forms, one behind the other */
		p.prefix = nullptr;
		p.n_jobs = n_jobs;
		rv = job_table::launch<kThreads>(k_psd_combine, (unsigned)job_table::groups_of(n_jobs, kWaves), st, p, stats,
		                                 FOSPHOR_AMD_PSD_K_COMBINE);
	}
	return job_table::drain(st, rv);
}
