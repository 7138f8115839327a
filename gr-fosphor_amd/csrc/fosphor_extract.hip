/*
 * fosphor_extract.hip -- burst IQ at baseband: batched mix, FIR, decimate over device-resident IQ (include/fosphor_amd_extract.h)
 *
 * A read-only pass over the CALLER's samples, in a file of its own: nothing here is on the process / merge path and no buffer of
 * the instance is read or written but the job table this file owns.
 *
 * The table of jobs, the search that gives a work-group its job, the refusals every pass over burst IQ shares and the tail of the
 * call are those of fosphor_jobs.h; only jobs that write something are uploaded.  One launch per form present; no work-group waits
 * for another; every loop carries its bound in its header.
 *
 *   k_extract_tile  small D: a work-group of 256 lanes owns kTileOut = 256 consecutive outputs of a job.  It loads their input span
 *                   (n - 1) * D + T samples coalesced, 16 bytes per lane where the address allows (the samples before the first
 *                   16-byte boundary and behind the last go one by one, so no byte outside the span is read), widens and mixes
 *                   every sample ONCE -- the phase comes from the sample's index in the job, not in the tile -- and leaves the mixed
 *                   float2 in LDS.  Then lane l owns output l and walks the taps in order; a tap is the same for the whole
 *                   work-group (a scalar load).
 *                   The LDS image is polyphase: local sample i sits at row i mod D, column i / D of D rows of R float2,
 *                   R = (256 + (T - 1) / D + 1) | 1.  Output l, tap k reads row k mod D, column l + k / D: the lanes of a wave read
 *                   consecutive float2, which no ds_read_b64 half-wave can conflict on, for every D, even or odd (an image in
 *                   sample order would be read at stride D: 2-, 4-, .. 32-way for even D).  The price is paid once per sample, at
 *                   the write, not T / D ~ 8 times at the reads: the lanes of a ds_write_b64 group hold samples 2 (fp32) or 4
 *                   (fp16 / sc16) apart and write them rows apart, 1- to 5-way by D (DESIGN.md has the counts; R is odd, which
 *                   is what keeps D = 2, 4, 8, 16 at 1- or 2-way).  i / D is a multiply-high by ceil(2^32 / D), exact for
 *                   i * D < 2^32.
 *   k_extract_wave  large D, where a tile's span no longer fits in LDS and a sample feeds T / D ~ 8 outputs only: a wave owns one
 *                   output, lane l takes the taps l, l + 64, ... with coalesced loads of x and h, mixes its own samples, and the
 *                   64 partial sums meet by xor-shuffles 32, 16, .. 1.
 * The form is a function of (D, T) alone: TILE when D * R <= kTileLds.  Both kernels are templates over the IQ format; the tags
 * below restate, for single samples and 16-byte groups, the exact widening of the FFT kernels' tags (fosphor_kernels.hip: sc16
 * (float)(short) * 2^-15, fp16 v_cvt_f32_f16), which live inside that translation unit with its FFT-shaped loads.
 * The mixer: phi is a 32-bit integer, its quarter turn is split off exactly and the rest, at most an eighth of a turn, goes through
 * sincospif -- no fast intrinsic, whose absolute error near pi the tolerance does not allow.  float32 sums, explicit fmaf, no
 * atomics of any kind.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_extract.h"

/* accessor implemented next to struct fosphor (fosphor_api.cpp) */
extern "C" int fosphor_amd_priv_iq_format(struct fosphor *self);

namespace {

typedef struct fosphor_amd_extract_job Job;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileOut = FOSPHOR_AMD_EXTRACT_TILE_OUT;	/* outputs of a TILE work-group: one per lane */
constexpr int kTileLds = FOSPHOR_AMD_EXTRACT_TILE_LDS;	/* float2 of its LDS image: 52 KiB, three work-groups per CU */
constexpr int kWaveOut = FOSPHOR_AMD_EXTRACT_WAVE_OUT;	/* outputs of a WAVE work-group: one per wave */

static_assert(kTileOut == kThreads, "a lane owns one output of the tile");
static_assert(kWaveOut == kWaves, "a wave owns one output");
static_assert(FOSPHOR_AMD_EXTRACT_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 40, "the job table is uploaded as it is");
static_assert(kTileLds * sizeof(float2) <= 64 * 1024, "static LDS");

/* rows' length of the TILE image, and the form: (D, T) alone */
inline __host__ __device__ int tile_row(int d, int t) { return (kTileOut + (t - 1) / d + 1) | 1; }
inline bool tile_form(int d, int t) { return (long long)d * tile_row(d, t) <= kTileLds; }

struct Params {
	const void   *x;
	const float  *taps;
	float2       *out;
	const Job    *jobs;		/* the jobs of this form that write something */
	const uint32_t *prefix;		/* [n_jobs + 1]: work-groups before job j */
	int n_jobs;
};

/* IQ formats: a sample in memory, samples of a 16-byte group, and the two loads, widened */
struct iq_fp32 {
	typedef float2 elem;
	static constexpr int per = 2;
	static __device__ __forceinline__ float2 ld(const elem *p) { return *p; }
	static __device__ __forceinline__ void ld16(const elem *p, float2 (&v)[per])
	{
		const float4 q = *reinterpret_cast<const float4 *>(p);
		v[0] = make_float2(q.x, q.y);
		v[1] = make_float2(q.z, q.w);
	}
};
struct iq_sc16 {
	typedef uint32_t elem;
	static constexpr int per = 4;
	static __device__ __forceinline__ float2 widen(uint32_t v)
	{
		return make_float2((float)(short)(v & 0xffffu) * 0x1p-15f, (float)(short)(v >> 16) * 0x1p-15f);
	}
	static __device__ __forceinline__ float2 ld(const elem *p) { return widen(*p); }
	static __device__ __forceinline__ void ld16(const elem *p, float2 (&v)[per])
	{
		const uint4 q = *reinterpret_cast<const uint4 *>(p);
		v[0] = widen(q.x); v[1] = widen(q.y); v[2] = widen(q.z); v[3] = widen(q.w);
	}
};
struct iq_fp16 {
	typedef uint32_t elem;
	static constexpr int per = 4;
	static __device__ __forceinline__ float2 widen(uint32_t q)
	{
		typedef _Float16 h2 __attribute__((ext_vector_type(2)));
		const h2 h = __builtin_bit_cast(h2, q);
		return make_float2((float)h.x, (float)h.y);		/* v_cvt_f32_f16: exact, subnormals included */
	}
	static __device__ __forceinline__ float2 ld(const elem *p) { return widen(*p); }
	static __device__ __forceinline__ void ld16(const elem *p, float2 (&v)[per])
	{
		const uint4 q = *reinterpret_cast<const uint4 *>(p);
		v[0] = widen(q.x); v[1] = widen(q.y); v[2] = widen(q.z); v[3] = widen(q.w);
	}
};

/* x * exp(-2 pi i phi / 2^32).  The nearest quarter turn q leaves r in [-2^29, 2^29), an angle of at most 1/4 half-turn; its
 * conversion to float is off by at most 2^-25 of that, the rotation by q is exact. */
__device__ __forceinline__ float2 mix(float2 x, uint32_t phi)
{
	const uint32_t q = (phi + 0x20000000u) >> 30;
	const int32_t r = (int32_t)(phi - (q << 30));
	float s, c;
	sincospif((float)r * 0x1p-31f, &s, &c);
	const float cc = (q & 1u) ? -s : c, ss = (q & 1u) ? c : s;
	const float co = (q & 2u) ? -cc : cc, si = (q & 2u) ? -ss : ss;
	return make_float2(fmaf(x.x, co, x.y * si), fmaf(x.y, co, -(x.x * si)));
}

template <class IQ>
__global__ __launch_bounds__(kThreads)
void k_extract_tile(const Params p)
{
	__shared__ float2 s_x[kTileLds];
	typedef typename IQ::elem elem;
	constexpr int per = IQ::per;

	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const Job job = p.jobs[j];
	const int D = job.decim, T = job.n_taps;
	const int m0 = (int)(blockIdx.x - p.prefix[j]) * kTileOut;	/* first output of the tile */
	const int n_tile = min(kTileOut, job.n_out - m0);		/* >= 1 by the prefix */
	const int span = (n_tile - 1) * D + T;				/* <= D * R - 1 */
	const int R = tile_row(D, T);
	const int64_t base = (int64_t)m0 * D;				/* index in the job of local sample 0 */
	const elem *src = static_cast<const elem *>(p.x) + job.first + base;
	const uint32_t phi0 = job.phase0 + (uint32_t)(uint64_t)base * job.phase_inc;
	const uint32_t inc = job.phase_inc;
	const uint64_t magic = ((1ull << 32) + (uint32_t)D - 1) / (uint32_t)D;

	auto put = [&](int i, float2 x) {
		const uint32_t q = (uint32_t)(((uint64_t)(uint32_t)i * magic) >> 32);	/* i / D */
		const uint32_t r = (uint32_t)i - q * (uint32_t)D;
		s_x[r * (uint32_t)R + q] = mix(x, phi0 + (uint32_t)i * inc);
	};

	/* head: up to the first 16-byte boundary; body: 16 bytes per lane; tail: what is left of the span */
	const int lead = (int)((per - (int)(((uintptr_t)src / sizeof(elem)) % per)) % per);
	const int head = min(span, lead);
	const int groups = (span - head) / per;
	const int tail0 = head + groups * per;
	if (tid < head)
		put(tid, IQ::ld(src + tid));
	for (int g = tid; g < groups; g += kThreads) {
		float2 v[per];
		IQ::ld16(src + head + g * per, v);
#pragma unroll
		for (int e = 0; e < per; e++)
			put(head + g * per + e, v[e]);
	}
	if (tail0 + tid < span)
		put(tail0 + tid, IQ::ld(src + tail0 + tid));
	__syncthreads();

	/* lane l: output m0 + l.  Tap k0 + r reads row r, column l + k0 / D; a lane without an output reads inside the image too
	 * (columns up to 255 + (T - 1) / D < R) and stores nothing. */
	const float *h = p.taps + job.taps_offset;
	const float2 *sx = s_x + tid;
	float re = 0.0f, im = 0.0f;
	for (int k0 = 0; k0 < T; k0 += D) {
		const int nr = min(D, T - k0);
		const float2 *row = sx + k0 / D;
#pragma unroll 4
		for (int r = 0; r < nr; r++) {
			const float hk = h[k0 + r];
			const float2 v = row[r * R];
			re = fmaf(hk, v.x, re);
			im = fmaf(hk, v.y, im);
		}
	}
	if (tid < n_tile)
		p.out[job.out_offset + m0 + tid] = make_float2(re, im);
}

template <class IQ>
__global__ __launch_bounds__(kThreads)
void k_extract_wave(const Params p)
{
	typedef typename IQ::elem elem;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const Job job = p.jobs[j];
	const int T = job.n_taps;
	const int64_t m = (int64_t)(blockIdx.x - p.prefix[j]) * kWaveOut + wave;
	if (m >= job.n_out)						/* the whole wave; there is no barrier below */
		return;
	const int64_t n0 = m * job.decim;
	const elem *src = static_cast<const elem *>(p.x) + job.first + n0;
	const float *h = p.taps + job.taps_offset;
	const uint32_t phi0 = job.phase0 + (uint32_t)(uint64_t)n0 * job.phase_inc;

	float re = 0.0f, im = 0.0f;
	for (int k = lane; k < T; k += 64) {
		const float hk = h[k];
		const float2 v = mix(IQ::ld(src + k), phi0 + (uint32_t)k * job.phase_inc);
		re = fmaf(hk, v.x, re);
		im = fmaf(hk, v.y, im);
	}
	for (int d = 32; d; d >>= 1) {
		re += __shfl_xor(re, d);
		im += __shfl_xor(im, d);
	}
	if (lane == 0)
		p.out[job.out_offset + m] = make_float2(re, im);
}

template <class IQ>
int launch_form(int f, const Params &p, unsigned groups, hipStream_t st, long long *stats)
{
	return job_table::launch<kThreads>(f ? k_extract_wave<IQ> : k_extract_tile<IQ>, groups, st, p, stats,
	                                   f ? FOSPHOR_AMD_EXTRACT_K_WAVE : FOSPHOR_AMD_EXTRACT_K_TILE);
}

int sample_bytes(int fmt) { return fmt == FOSPHOR_AMD_IQ_FP32 ? 8 : 4; }

/* What both entry points refuse, but for the pointers.  fmt: 0, 1 or 2. */
int check_call(int64_t n_samples, int fmt, const Job *jobs, int n_jobs, int n_taps_total, int64_t out_capacity)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_EXTRACT_MAX_JOBS) || n_samples < 0 || n_taps_total < 0 || out_capacity < 0)
		return -EINVAL;
	if (fmt != FOSPHOR_AMD_IQ_FP32 && fmt != FOSPHOR_AMD_IQ_FP16 && fmt != FOSPHOR_AMD_IQ_SC16)
		return -EINVAL;
	std::vector<std::pair<int64_t, int64_t>> ranges;
	long long groups[2] = { 0, 0 };
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (b.first < 0 || b.decim < 1 || b.decim > FOSPHOR_AMD_EXTRACT_MAX_DECIM ||
		    b.n_taps < 1 || b.n_taps > FOSPHOR_AMD_EXTRACT_MAX_TAPS || !job_table::inside(b.taps_offset, b.n_taps, n_taps_total))
			return -EINVAL;
		if (!job_table::inside(b.out_offset, b.n_out, out_capacity))
			return -EINVAL;
		if (b.n_out == 0)
			continue;
		const int64_t need = (int64_t)(b.n_out - 1) * b.decim + b.n_taps;	/* < 2^41 */
		if (!job_table::inside(b.first, need, n_samples))
			return -EINVAL;
		ranges.emplace_back(b.out_offset, b.out_offset + b.n_out);
		const int f = tile_form(b.decim, b.n_taps) ? 0 : 1;
		if (!job_table::add_groups(groups[f], b.n_out, f ? kWaveOut : kTileOut))
			return -EINVAL;
	}
	return job_table::ranges_disjoint(ranges) ? 0 : -EINVAL;
}

float half_to_float(uint16_t h)
{
	const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
	const int e = (h >> 10) & 31, f = h & 0x3ff;
	float v;
	if (e == 0)
		v = ldexpf((float)f, -24);				/* zero and subnormals: exact */
	else if (e == 31)
		v = f ? NAN : INFINITY;
	else
		v = ldexpf((float)(f | 0x400), e - 25);
	uint32_t u;
	memcpy(&u, &v, 4);
	u |= sign;
	memcpy(&v, &u, 4);
	return v;
}

void host_sample(const void *x, int fmt, int64_t i, double *re, double *im)
{
	if (fmt == FOSPHOR_AMD_IQ_FP32) {
		const float *p = static_cast<const float *>(x) + 2 * i;
		*re = p[0]; *im = p[1];
	} else if (fmt == FOSPHOR_AMD_IQ_SC16) {
		const int16_t *p = static_cast<const int16_t *>(x) + 2 * i;
		*re = (double)p[0] * 0x1p-15; *im = (double)p[1] * 0x1p-15;
	} else {
		const uint16_t *p = static_cast<const uint16_t *>(x) + 2 * i;
		*re = half_to_float(p[0]); *im = half_to_float(p[1]);
	}
}

} // namespace

extern "C" int fosphor_amd_extract_host(const void *samples, int64_t n_samples, int iq_format,
                                        const struct fosphor_amd_extract_job *jobs, int n_jobs,
                                        const float *taps, int n_taps_total,
                                        float *out, int64_t out_capacity)
{
	if (!samples || !taps || !out)
		return -EINVAL;
	if (check_call(n_samples, iq_format, jobs, n_jobs, n_taps_total, out_capacity))
		return -EINVAL;
	const double turn = 6.283185307179586476925286766559 / 4294967296.0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		for (int64_t m = 0; m < b.n_out; m++) {
			double sr = 0.0, si = 0.0;
			for (int k = 0; k < b.n_taps; k++) {
				const uint64_t n = (uint64_t)m * (uint64_t)b.decim + (uint64_t)k;
				const uint32_t phi = b.phase0 + (uint32_t)n * b.phase_inc;
				const double c = cos(turn * (double)phi), s = sin(turn * (double)phi);
				const double h = taps[b.taps_offset + k];
				double xr, xi;
				host_sample(samples, iq_format, b.first + (int64_t)n, &xr, &xi);
				sr += h * (xr * c + xi * s);
				si += h * (xi * c - xr * s);
			}
			out[2 * (b.out_offset + m)] = (float)sr;
			out[2 * (b.out_offset + m) + 1] = (float)si;
		}
	}
	return 0;
}

extern "C" int fosphor_amd_extract_design(int decim, int n_taps, double guard, float *out)
{
	if (!out || decim < 1 || decim > FOSPHOR_AMD_EXTRACT_MAX_DECIM || n_taps < 1 || n_taps > FOSPHOR_AMD_EXTRACT_MAX_TAPS ||
	    !(guard > 0.0) || !(guard <= 1.0))
		return -EINVAL;
	const double pi = 3.14159265358979323846;
	const double fc = guard / (2.0 * decim), c = 0.5 * (n_taps - 1);
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
		out[k] = (float)(g[k] / sum);
	return 0;
}

extern "C" int fosphor_amd_extract_from_burst(const struct fosphor_amd_burst *b, int fft_len, int64_t newest_first_sample,
                                              int row_hop, int max_decim, double guard, struct fosphor_amd_extract_job *job,
                                              int *n_taps_wanted)
{
	if (!b || !job || !n_taps_wanted || fft_len < 2 || (fft_len & (fft_len - 1)) || row_hop < 1 || max_decim < 1 ||
	    !(guard > 0.0) || !(guard <= 1.0))
		return -EINVAL;
	if (b->newest < 0 || b->oldest < b->newest || b->first_col < 0 || b->last_col >= fft_len || b->first_col > b->last_col)
		return -EINVAL;
	const int64_t first = newest_first_sample - (int64_t)b->oldest * row_hop;
	if (first < 0)
		return -EINVAL;
	const int64_t length = (int64_t)(b->oldest - b->newest) * row_hop + fft_len;
	const double centre = (0.5 * ((double)b->first_col + (double)b->last_col + 1.0) - 0.5 * fft_len) / fft_len;
	const int width = b->last_col - b->first_col + 1;
	const int cap = max_decim < FOSPHOR_AMD_EXTRACT_MAX_DECIM ? max_decim : FOSPHOR_AMD_EXTRACT_MAX_DECIM;
	int d = 1;
	for (int t = cap; t > 1; t--)				/* at most 1023 steps; the comparison is the contract's, no division */
		if ((double)width * t <= guard * fft_len) {
			d = t;
			break;
		}
	const int taps = 8 * d + 1;
	const int64_t n_out = length >= taps ? (length - taps) / d + 1 : 0;
	if (n_out > INT32_MAX)
		return -EINVAL;
	job->first = first;
	job->out_offset = 0;
	job->n_out = (int32_t)n_out;
	job->decim = d;
	job->phase_inc = (uint32_t)(int64_t)llround(centre * 4294967296.0);
	job->phase0 = 0;
	job->taps_offset = 0;
	job->n_taps = taps;
	*n_taps_wanted = taps;
	return 0;
}

extern "C" int fosphor_amd_extract_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_EXTRACT_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_EXTRACT, FOSPHOR_AMD_EXTRACT_STATS, stats);
}

extern "C" int fosphor_amd_extract(struct fosphor *self, const void *d_samples, int64_t n_samples, int iq_format,
                                   const struct fosphor_amd_extract_job *jobs, int n_jobs,
                                   const float *d_taps, int n_taps_total,
                                   void *d_out, int64_t out_capacity)
{
	if (!self || !d_samples || !jobs || !d_taps || !d_out)
		return -EINVAL;
	if (iq_format < -1 || iq_format > FOSPHOR_AMD_IQ_SC16)
		return -EINVAL;
	const int fmt = iq_format == -1 ? fosphor_amd_priv_iq_format(self) : iq_format;
	if (((uintptr_t)d_samples % sample_bytes(fmt)) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_taps & 3))
		return -EINVAL;
	if (check_call(n_samples, fmt, jobs, n_jobs, n_taps_total, out_capacity))
		return -EINVAL;

	/* the table: the jobs that write something, TILE jobs first, and behind them the two prefixes */
	std::vector<Job> live[2];
	std::vector<uint32_t> prefix[2] = { std::vector<uint32_t>(1, 0u), std::vector<uint32_t>(1, 0u) };
	long long n_form[2] = { 0, 0 }, samples = 0;
	for (int i = 0; i < n_jobs; i++) {
		const int f = tile_form(jobs[i].decim, jobs[i].n_taps) ? 0 : 1;
		n_form[f]++;
		if (jobs[i].n_out == 0)
			continue;
		prefix[f].push_back(prefix[f].back() + (uint32_t)job_table::groups_of(jobs[i].n_out, f ? kWaveOut : kTileOut));
		live[f].push_back(jobs[i]);
		samples += (long long)(jobs[i].n_out - 1) * jobs[i].decim + jobs[i].n_taps;
	}
	const job_table::Table table = job_table::pack_table(live, prefix, 0, 0);

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_EXTRACT);
	stats[FOSPHOR_AMD_EXTRACT_CALLS]++;
	stats[FOSPHOR_AMD_EXTRACT_JOBS_TILE] += n_form[0];
	stats[FOSPHOR_AMD_EXTRACT_JOBS_WAVE] += n_form[1];
	stats[FOSPHOR_AMD_EXTRACT_SAMPLES] += samples;
	if (live[0].empty() && live[1].empty())
		return 0;						/* every job has n_out = 0 */

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_EXTRACT, table, &d, &st))
		return -EIO;
	Params p;
	p.x = d_samples;
	p.taps = d_taps;
	p.out = static_cast<float2 *>(d_out);
	int rv = 0;
	for (int f = 0; f < 2 && !rv; f++) {
		if (live[f].empty())
			continue;
		p.jobs = reinterpret_cast<const Job *>(d + table.jobs_at[f]);
		p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[f]);
		p.n_jobs = (int)live[f].size();
		const unsigned groups = prefix[f].back();
		rv = fmt == FOSPHOR_AMD_IQ_FP32 ? launch_form<iq_fp32>(f, p, groups, st, stats)
		   : fmt == FOSPHOR_AMD_IQ_SC16 ? launch_form<iq_sc16>(f, p, groups, st, stats)
		   :                              launch_form<iq_fp16>(f, p, groups, st, stats);
	}
	return job_table::drain(st, rv);
}
