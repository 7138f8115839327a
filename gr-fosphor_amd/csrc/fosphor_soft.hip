/*
 * fosphor_soft.hip -- the decoded bits of burst symbols with their reliabilities kept: one quantised max-log soft value per coded
 * bit, depunctured into one word per trellis step, a soft-input Viterbi decoder with one lane per state, the traceback over the
 * whole frame, the decoded bits packed MSB first and a CRC over them (include/fosphor_amd_soft.h)
 *
 * A read-only pass over the CALLER's symbols (what fosphor_amd_carrier wrote and fosphor_amd_decide read), in a file of its own:
 * nothing here is on the process / merge path and no buffer of the instance is read or written but the scratch this file owns (the
 * job table, the prefix, the survivor decisions, the partial sums, the jobs' ends and the soft words).
 *
 *   k_sft_bits   256 lanes own 256 steps of one job, which they find in the prefix (fosphor_jobs.h); a lane forms its step's up to
 *                three soft values and stores them as one word; the group's three integer sums leave as one partial.
 *   k_sft_acs    a wave per job, a lane per state: add-compare-select over all steps; __ballot is a step's decision word.
 *   k_sft_trace  a wave per job walks the decisions back, 64 steps a block, and stores 64 decoded bits a block.
 *   k_sft_rec    a wave per job adds the job's partials, runs the CRC over the decoded bits and writes the record.
 * The soft values are double arithmetic of one rounding an operation (rules S1 and S2), everything behind them integer work, both
 * formed by the helpers below and in fosphor_trellis.h on the device and in fosphor_amd_soft_host alike.  No atomics of any kind,
 * no work-group waits for another, every loop carries its bound in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "fosphor_trellis.h"					/* kept_of, expected_of, bit_place, crc_of, steps_that_fit and the checks of the code */
#include "../../include/fosphor_amd_soft.h"

namespace {

using namespace trellis;

typedef struct fosphor_amd_soft_job Job;
typedef struct fosphor_amd_soft_record Record;

constexpr int kWave = 64;
constexpr int kBitsThreads = FOSPHOR_AMD_SOFT_GROUP;		/* steps of a work-group of k_sft_bits */
constexpr int kBlock = FOSPHOR_AMD_SOFT_BLOCK;
constexpr int kInf = FOSPHOR_AMD_SOFT_INF;
constexpr int kMaxValue = FOSPHOR_AMD_SOFT_MAX_VALUE;
constexpr int kMaxSteps = FOSPHOR_AMD_SOFT_MAX_STEPS;
constexpr int kMaxParts = kMaxSteps / kBitsThreads;		/* partials of one job */
constexpr int kTerminated = FOSPHOR_AMD_SOFT_TERMINATED;
constexpr int kGray = FOSPHOR_AMD_SOFT_GRAY;

static_assert(FOSPHOR_AMD_SOFT_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 64, "the job is 64 bytes");
static_assert(sizeof(Record) == 64, "the record is 64 bytes");
static_assert(kBlock == kWave, "a wave's lanes are a block of steps, and the states of K = 7");
static_assert(kBitsThreads == 4 * kWave && kMaxSteps % kBitsThreads == 0, "four waves a work-group of k_sft_bits");
static_assert(kInf == 1 << 25 && kInf + 3 * kMaxValue * kMaxSteps < (1 << 26), "a metric fits 26 bits");
static_assert((((uint64_t)(kInf + 3 * kMaxValue * kMaxSteps) << 6) | 63u) < 0xffffffffull, "the worst key lies below an idle lane's");
static_assert(3 * kMaxValue * kBitsThreads < (1 << 30) && 3 * kBitsThreads < (1 << 15), "a work-group's sums fit their fields");

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t  offset;		/* complex samples */
	int64_t  out_offset;		/* bytes */
	int64_t  step0;			/* the job's first step in the soft words and the decisions */
	int32_t  n_steps, n_bits, n_coded;
	int32_t  bits, order;		/* b and M of rule S1 */
	int32_t  flags, k, n_poly, period;
	int32_t  weight;		/* W of rule 2 */
	int32_t  crc_width;
	uint16_t polys[3], punct[3];
	uint32_t crc_poly, crc_init, crc_xorout;
	float    scale;
	double   pts[8][2];		/* rule S1: (C_q, S_q), formed on the host; the entries from M on are 0 */
};

static_assert(sizeof(DevJob) == 224, "a device job is 224 bytes");

/* the sums of rule S2 over the steps of one work-group of k_sft_bits */
struct Part {
	int32_t erasures, saturated;
	int64_t abs_sum;
};

static_assert(sizeof(Part) == 16, "a partial is 16 bytes");

struct Params {
	const float2   *iq;
	uint64_t       *out;		/* d_out in 64-bit words */
	const DevJob   *jobs;
	const uint32_t *prefix;		/* [n_jobs + 1] work-groups of k_sft_bits before job j */
	uint64_t       *dec;		/* a decision word a step */
	Part           *parts;		/* a partial a work-group of k_sft_bits */
	int32_t        *ends;		/* [n_jobs][4] end_state, metric, best_state, best_metric */
	uint32_t       *words;		/* a soft word a step */
	Record         *records;
	int n_jobs;
};

/* rule S2: x to the nearest integer, halves upwards (the 0.5 is in x already), clamped */
inline __host__ __device__ int quantised(double x)
{
	if (x != x)
		return 0;
	if (x >= (double)kMaxValue)
		return kMaxValue;
	if (x < -(double)kMaxValue)
		return -kMaxValue;
	return (int)__builtin_floor(x);
}

/* rules S1 and S2: the soft values of the b bits of the symbol (fr, fi) -> a part is a NaN.  Every array index is a constant once
 * the loops are unrolled. */
inline __host__ __device__ bool soft_of(float fr, float fi, const double (*pts)[2], int M, int b, bool gray, double scale, int (&v)[3])
{
	v[0] = v[1] = v[2] = 0;
	if (fr != fr || fi != fi)
		return true;
	const double sr = (double)fr, si = (double)fi;
	double zero[3], one[3];						/* the largest corr_q over the points whose bit i is 0, is 1 */
#pragma unroll
	for (int i = 0; i < 3; i++)
		zero[i] = one[i] = -INFINITY;
#pragma unroll
	for (int q = 0; q < 8; q++) {
		if (q < M) {
			const double corr = (sr * pts[q][0]) + (si * pts[q][1]);
			const int label = gray ? q ^ (q >> 1) : q;
#pragma unroll
			for (int i = 0; i < 3; i++) {
				if (i < b) {
					if ((label >> (b - 1 - i)) & 1)
						one[i] = corr > one[i] ? corr : one[i];
					else
						zero[i] = corr > zero[i] ? corr : zero[i];
				}
			}
		}
	}
#pragma unroll
	for (int i = 0; i < 3; i++)
		if (i < b)
			v[i] = quantised(((zero[i] - one[i]) * scale) + 0.5);
	return false;
}

/* rules 2, S1 and S2: the soft word of step t of a job whose symbol 0 is y[0] (float32 pairs): stream i's value in byte i, 0 where
 * it was not sent; the step's share of the three sums is added */
inline __host__ __device__ uint32_t word_of(const float *y, const double (*pts)[2], int M, int b, bool gray, double scale, int n_poly,
                                            int period, const uint16_t *punct, int weight, int t, int &erasures, int &saturated, int &abs_sum)
{
	int q = (int)kept_of(t, period, punct, weight);			/* below 3 * 65536 */
	const int phase = t % period;
	int have = -1, v[3] = { 0, 0, 0 };
	bool nan = false;
	uint32_t w = 0;
#pragma unroll
	for (int i = 0; i < 3; i++) {
		if (i < n_poly && ((punct[i] >> phase) & 1)) {
			const int s = q / b, place = q - s * b;
			if (s != have) {
				nan = soft_of(y[2 * (int64_t)s], y[2 * (int64_t)s + 1], pts, M, b, gray, scale, v);
				have = s;
			}
			if (place == 0 && nan)				/* a symbol counts where its first bit is consumed */
				erasures++;
			const int value = place == 0 ? v[0] : (place == 1 ? v[1] : v[2]);
			const int mag = value < 0 ? -value : value;
			abs_sum += mag;
			saturated += mag == kMaxValue;
			w |= ((uint32_t)value & 0xffu) << (8 * i);
			q++;
		}
	}
	return w;
}

/* rule S3: the cost of a branch that expects e (stream i in bit i) under the soft word c */
inline __host__ __device__ int cost_of(uint32_t e, uint32_t c)
{
	int cost = 0;
#pragma unroll
	for (int i = 0; i < 3; i++) {
		const int v = (int)(int8_t)(uint8_t)(c >> (8 * i));
		cost += ((e >> i) & 1) ? (v > 0 ? v : 0) : (v < 0 ? -v : 0);
	}
	return cost;
}

/* rule 4 as one integer: the least metric, then the smallest state */
inline __host__ __device__ uint32_t end_key(int metric, int state) { return ((uint32_t)metric << 6) | (uint32_t)state; }

/* the whole record, from rule 4's values, the sums and the job's owned bytes */
inline __host__ __device__ void record_of(int n_steps, int n_bits, int n_coded, int k, int flags, const int *ends, const Part &sums,
                                          const uint8_t *out, int w, uint32_t poly, uint32_t init, uint32_t xorout, Record &r)
{
	r.n_steps = n_steps;
	r.n_bits = n_bits;
	r.n_coded = n_coded;
	r.end_state = ends[0];
	r.metric = ends[1];
	r.best_state = ends[2];
	r.best_metric = ends[3];
	crc_of(out, n_bits, w, poly, init, xorout, r.crc_calc, r.crc_recv, r.status);
	r.k = k;
	r.flags = flags;
	r.erasures = sums.erasures;
	r.saturated = sums.saturated;
	r.abs_sum = sums.abs_sum;
}

__global__ __launch_bounds__(kBitsThreads)
void k_sft_bits(const Params p)
{
	__shared__ int s_sums[kBitsThreads / kWave][2];
	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob &job = p.jobs[j];
	const int t = (int)(blockIdx.x - p.prefix[j]) * kBitsThreads + tid;	/* the group's first step is below n_steps by the prefix */
	int erasures = 0, saturated = 0, abs_sum = 0;
	if (t < job.n_steps)
		p.words[job.step0 + t] = word_of(reinterpret_cast<const float *>(p.iq + job.offset), job.pts, job.order, job.bits,
		                                 job.flags & kGray, (double)job.scale, job.n_poly, job.period, job.punct, job.weight, t,
		                                 erasures, saturated, abs_sum);
	/* integers: any order.  At most 3 * 256 erasures and saturated bits a work-group, in 16 bits each; every lane takes part */
	int counts = (erasures << 16) | saturated;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		counts += __shfl_xor(counts, d);
		abs_sum += __shfl_xor(abs_sum, d);
	}
	if (!(tid & (kWave - 1))) {
		s_sums[tid / kWave][0] = counts;
		s_sums[tid / kWave][1] = abs_sum;
	}
	__syncthreads();
	if (tid == 0) {
		int c = 0, a = 0;
#pragma unroll
		for (int w = 0; w < kBitsThreads / kWave; w++) {
			c += s_sums[w][0];
			a += s_sums[w][1];
		}
		Part part;
		part.erasures = c >> 16;
		part.saturated = c & 0xffff;
		part.abs_sum = a;
		p.parts[blockIdx.x] = part;
	}
}

__global__ __launch_bounds__(kWave)
void k_sft_acs(const Params p)
{
	const int lane = threadIdx.x;
	const int j = (int)blockIdx.x;
	const DevJob &job = p.jobs[j];
	const int T = job.n_steps;
	if (T <= 0)								/* the whole wave */
		return;
	const int k = job.k, S = 1 << (k - 1);
	const bool live = lane < S;
	const uint64_t live_mask = S == kWave ? ~0ull : (1ull << S) - 1ull;
	const int p0 = (lane << 1) & (S - 1), p1 = p0 | 1;			/* lanes below S, for every lane */
	const int u = (lane >> (k - 2)) & 1;
	const uint32_t e0 = expected_of(job.polys, job.n_poly, k, u, p0), e1 = expected_of(job.polys, job.n_poly, k, u, p1);
	const uint32_t *words = p.words + job.step0;
	uint64_t *dec = p.dec + job.step0;
	int metric = lane == 0 ? 0 : kInf;
	for (int t0 = 0; t0 < T; t0 += kBlock) {
		const int count = min(T - t0, kBlock);
		const uint32_t mine = lane < count ? words[t0 + lane] : 0u;
		uint64_t keep = 0;
		for (int i = 0; i < kBlock && i < count; i++) {
			const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
			const int c0 = __shfl(metric, p0) + cost_of(e0, c);
			const int c1 = __shfl(metric, p1) + cost_of(e1, c);
			const bool one = c1 < c0;				/* ties go to x = 0 */
			const uint64_t word = __ballot(one) & live_mask;
			metric = live ? (one ? c1 : c0) : kInf;
			if (lane == i)
				keep = word;
		}
		if (lane < count)
			dec[t0 + lane] = keep;
	}
	uint32_t key = live ? end_key(metric, lane) : 0xffffffffu;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		key = min(key, (uint32_t)__shfl_xor((int)key, d));
	const int zero_metric = __shfl(metric, 0);
	if (lane == 0) {
		const int best_state = (int)(key & 63u), best_metric = (int)(key >> 6);
		const bool term = job.flags & kTerminated;
		int32_t *e = p.ends + 4 * j;
		e[0] = term ? 0 : best_state;
		e[1] = term ? zero_metric : best_metric;
		e[2] = best_state;
		e[3] = best_metric;
	}
}

__global__ __launch_bounds__(kWave)
void k_sft_trace(const Params p)
{
	const int lane = threadIdx.x;
	const int j = (int)blockIdx.x;
	const DevJob &job = p.jobs[j];
	const int T = job.n_steps;
	if (T <= 0)								/* the whole wave */
		return;
	const int k = job.k, S = 1 << (k - 1);
	const uint64_t *dec = p.dec + job.step0;
	uint64_t *out = p.out + (job.out_offset >> 3);
	int state = __builtin_amdgcn_readfirstlane(p.ends[4 * j]) & (S - 1);
	for (int t0 = (T - 1) & ~(kBlock - 1); t0 >= 0; t0 -= kBlock) {
		const int count = min(T - t0, kBlock);
		const uint64_t mine = lane < count ? dec[t0 + lane] : 0ull;
		const int lo = (int)(uint32_t)mine, hi = (int)(uint32_t)(mine >> 32);
		uint64_t bits = 0;
		for (int i = min(count, kBlock) - 1; i >= 0; i--) {
			const uint64_t word = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(lo, i) |
			                      ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, i) << 32);
			const uint64_t u = (uint64_t)(state >> (k - 2));	/* the input that led into this state */
			if (t0 + i < job.n_bits)				/* the tail and what lies behind n_bits stay 0 */
				bits |= u << bit_place(i);
			state = ((state << 1) | (int)((word >> state) & 1ull)) & (S - 1);
		}
		if (lane == 0 && t0 < job.n_bits)				/* word t0 / 64 is one of the ceil(n_bits / 64) the job owns */
			out[t0 >> 6] = bits;
	}
}

__global__ __launch_bounds__(kWave)
void k_sft_rec(const Params p)
{
	const int lane = threadIdx.x;
	const int j = (int)blockIdx.x;
	const DevJob &job = p.jobs[j];
	int ends[4] = { 0, 0, 0, 0 };
	Part sums = { 0, 0, 0 };
	if (job.n_steps > 0) {
#pragma unroll
		for (int i = 0; i < 4; i++)
			ends[i] = p.ends[4 * j + i];
		const uint32_t g0 = p.prefix[j], g1 = p.prefix[j + 1];		/* the job's work-groups of k_sft_bits, in ascending order */
		for (uint32_t g = g0; g < g1 && g < g0 + (uint32_t)kMaxParts; g++) {
			const Part part = p.parts[g];
			sums.erasures += part.erasures;
			sums.saturated += part.saturated;
			sums.abs_sum += part.abs_sum;
		}
	}
	Record r;
	record_of(job.n_steps, job.n_bits, job.n_coded, job.k, job.flags, ends, sums, reinterpret_cast<const uint8_t *>(p.out) + job.out_offset,
	          job.crc_width, job.crc_poly, job.crc_init, job.crc_xorout, r);
	if (lane == 0)
		p.records[j] = r;
}

/* rule S1: the job's points */
inline void points_of(int M, int rot, double (*pts)[2])
{
	for (int q = 0; q < 8; q++) {
		pts[q][0] = pts[q][1] = 0.0;
		if (q < M)
			fosphor_amd_cossin_turns((double)((q + rot) & (M - 1)) / (double)M, &pts[q][0], &pts[q][1]);
	}
}

inline bool scale_ok(float scale) { return scale > 0.0f && scale <= 3.4028234663852886e38f; }	/* finite and above 0; a NaN is neither */

struct Shape {
	int32_t n_steps, n_bits, n_coded, weight;
};

struct Plan {
	long long groups, steps, jobs_crc;
	std::vector<Shape> shape;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_SOFT_MAX_JOBS) || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	plan->groups = plan->steps = plan->jobs_crc = 0;
	plan->shape.resize((size_t)n_jobs);
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		Shape &s = plan->shape[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || !order_ok(b.order) || (b.flags & ~(kTerminated | kGray)) ||
		    b.k < 3 || b.k > 7 || b.steps < 0 || !punct_ok(b.n_poly, b.period, b.punct, &s.weight))
			return -EINVAL;
		if (b.rot < 0 || b.rot >= b.order || !scale_ok(b.scale))
			return -EINVAL;
		for (int m = 0; m < 3; m++)
			if (m < b.n_poly ? (!b.polys[m] || b.polys[m] >> b.k) : b.polys[m] != 0)
				return -EINVAL;
		const int w = b.crc_width;
		if (w != 0 && w != 8 && w != 16 && w != 24 && w != 32)
			return -EINVAL;
		const uint64_t limit = w ? 1ull << w : 1ull;			/* w = 0: the fields are 0 */
		if (b.crc_poly >= limit || b.crc_init >= limit || b.crc_xorout >= limit)
			return -EINVAL;
		const int64_t coded = (int64_t)b.n * bits_of(b.order);
		const int64_t T = b.steps ? b.steps : steps_that_fit(coded, b.period, b.punct, s.weight);
		if (T > kMaxSteps || kept_of(T, b.period, b.punct, s.weight) > coded)
			return -EINVAL;
		s.n_steps = (int32_t)T;
		s.n_coded = (int32_t)kept_of(T, b.period, b.punct, s.weight);
		s.n_bits = (b.flags & kTerminated) ? std::max(s.n_steps - (b.k - 1), 0) : s.n_steps;
		if ((b.out_offset & 7) || !job_table::inside(b.out_offset, owned_of(s.n_bits), out_capacity))
			return -EINVAL;
		plan->steps += T;
		plan->groups += job_table::groups_of(T, kBitsThreads);
		plan->jobs_crc += w != 0;
		if (plan->steps > FOSPHOR_AMD_SOFT_MAX_CALL_STEPS)
			return -EINVAL;
		if (s.n_bits > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + owned_of(s.n_bits)));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	return 0;
}

} // namespace

extern "C" int fosphor_amd_soft_host(const float *iq, int64_t n_samples, const struct fosphor_amd_soft_job *jobs, int n_jobs,
                                     struct fosphor_amd_soft_record *records, uint8_t *out, int64_t out_capacity)
{
	if (!iq || !records || !out || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7) || ((uintptr_t)out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	std::vector<uint64_t> dec;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const Shape &s = plan.shape[i];
		const int T = s.n_steps, k = b.k, S = 1 << (k - 1);
		uint32_t e[2][kWave];
		int metric[kWave], next[kWave];
		double pts[8][2];
		points_of(b.order, b.rot, pts);
		for (int st = 0; st < S; st++) {
			for (int x = 0; x < 2; x++)
				e[x][st] = expected_of(b.polys, b.n_poly, k, st >> (k - 2), ((st << 1) | x) & (S - 1));
			metric[st] = st ? kInf : 0;
		}
		dec.resize((size_t)T);
		Part sums = { 0, 0, 0 };
		for (int t = 0; t < T; t++) {
			int erasures = 0, saturated = 0, abs_sum = 0;
			const uint32_t c = word_of(iq + 2 * b.offset, pts, b.order, bits_of(b.order), b.flags & kGray, (double)b.scale, b.n_poly,
			                           b.period, b.punct, s.weight, t, erasures, saturated, abs_sum);
			sums.erasures += erasures;
			sums.saturated += saturated;
			sums.abs_sum += abs_sum;
			uint64_t word = 0;
			for (int st = 0; st < S; st++) {
				const int p0 = (st << 1) & (S - 1);
				const int c0 = metric[p0] + cost_of(e[0][st], c), c1 = metric[p0 | 1] + cost_of(e[1][st], c);
				const bool one = c1 < c0;
				word |= (uint64_t)one << st;
				next[st] = one ? c1 : c0;
			}
			memcpy(metric, next, sizeof(int) * (size_t)S);
			dec[t] = word;
		}
		int ends[4] = { 0, 0, 0, 0 };
		if (T > 0) {
			uint32_t key = 0xffffffffu;
			for (int st = 0; st < S; st++)
				key = std::min(key, end_key(metric[st], st));
			const bool term = b.flags & kTerminated;
			ends[2] = (int)(key & 63u);
			ends[3] = (int)(key >> 6);
			ends[0] = term ? 0 : ends[2];
			ends[1] = term ? metric[0] : ends[3];
		}
		uint8_t *o = out + b.out_offset;
		memset(o, 0, (size_t)owned_of(s.n_bits));
		int state = ends[0];
		for (int t = T - 1; t >= 0; t--) {
			if (t < s.n_bits && (state >> (k - 2)))
				o[t >> 3] |= (uint8_t)(0x80 >> (t & 7));
			state = ((state << 1) | (int)((dec[t] >> state) & 1)) & (S - 1);
		}
		Record r;
		memset(&r, 0, sizeof(r));
		record_of(T, s.n_bits, s.n_coded, k, b.flags, ends, sums, o, b.crc_width, b.crc_poly, b.crc_init, b.crc_xorout, r);
		records[i] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_soft_from_decide(const struct fosphor_amd_decide_job *d, const struct fosphor_amd_decide_record *r,
                                            int uw_len, int n_payload, struct fosphor_amd_soft_job *job)
{
	if (!d || !r || !job || (d->flags & FOSPHOR_AMD_DECIDE_DIFF) || d->offset < 0 || d->n < 0 || !order_ok(r->order) || uw_len < 0 ||
	    n_payload < 0)
		return -EINVAL;
	int64_t skip = 0, rest = d->n;
	int rot = 0;
	const bool lost = (d->flags & FOSPHOR_AMD_DECIDE_UW) && r->status != FOSPHOR_AMD_DECIDE_OK;
	if ((d->flags & FOSPHOR_AMD_DECIDE_UW) && !lost) {
		skip = (int64_t)r->uw_pos + uw_len;
		rot = r->uw_rot;
		if (r->uw_pos < 0 || skip > d->n || rot < 0 || rot >= r->order)
			return -EINVAL;
		rest = d->n - skip;
	}
	if (!lost && n_payload > rest)
		return -EINVAL;
	const int32_t n = (int32_t)(lost ? 0 : (n_payload ? n_payload : rest));
	float scale = 1.0f;
	if (n > 0) {
		if (!(r->a > 0.0 && r->a <= 1.7976931348623157e308))
			return -EINVAL;
		scale = (float)(16.0 * (double)r->n / r->a);
		if (!scale_ok(scale))
			return -EINVAL;
	}
	memset(job, 0, sizeof(*job));
	job->offset = d->offset + skip;
	job->n = n;
	job->order = (int16_t)r->order;
	job->flags = (d->flags & FOSPHOR_AMD_DECIDE_GRAY) ? kGray : 0;
	job->rot = rot;
	job->scale = scale;
	return 0;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_soft_derive(const struct fosphor_amd_soft_record *r, struct fosphor_amd_soft_values *v)
{
	if (!r || !v)
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	v->mean_abs = finite_or_zero((double)r->abs_sum / (double)r->n_coded);
	v->corrected_share = finite_or_zero((double)r->metric / (double)r->abs_sum);
	v->rate = finite_or_zero((double)r->n_steps / (double)r->n_coded);
	v->crc_ok = r->status == FOSPHOR_AMD_SOFT_OK ? 1.0 : 0.0;
	return 0;
}

extern "C" int fosphor_amd_soft_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_SOFT_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_SOFT, FOSPHOR_AMD_SOFT_STATS, stats);
}

extern "C" int fosphor_amd_soft(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                const struct fosphor_amd_soft_job *jobs, int n_jobs,
                                struct fosphor_amd_soft_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order and the prefix of their work-groups of k_sft_bits; behind it, in bytes from an
	 * 8-byte boundary on: a decision word a step, a partial a work-group, the jobs' ends, a soft word a step */
	const size_t n_form[2] = { (size_t)n_jobs, 0 }, n_prefix[2] = { (size_t)n_jobs + 1, 0 };
	const size_t dec_bytes = sizeof(uint64_t) * (size_t)plan.steps, parts_bytes = sizeof(Part) * (size_t)plan.groups;
	const size_t ends_bytes = 4 * sizeof(int32_t) * (size_t)n_jobs, words_bytes = sizeof(uint32_t) * (size_t)plan.steps;
	job_table::Table table = job_table::lay_table(sizeof(DevJob), n_form, n_prefix, dec_bytes + parts_bytes + ends_bytes + words_bytes, 1);
	DevJob *form = reinterpret_cast<DevJob *>(table.image.data() + table.jobs_at[0]);
	uint32_t *prefix = reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[0]);
	int64_t group0 = 0, step0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const Shape &s = plan.shape[i];
		DevJob &d = form[i];
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.step0 = step0;
		d.n_steps = s.n_steps;
		d.n_bits = s.n_bits;
		d.n_coded = s.n_coded;
		d.bits = bits_of(b.order);
		d.order = b.order;
		d.flags = b.flags;
		d.k = b.k;
		d.n_poly = b.n_poly;
		d.period = b.period;
		d.weight = s.weight;
		d.crc_width = b.crc_width;
		for (int m = 0; m < 3; m++) {
			d.polys[m] = b.polys[m];
			d.punct[m] = b.punct[m];
		}
		d.crc_poly = b.crc_poly;
		d.crc_init = b.crc_init;
		d.crc_xorout = b.crc_xorout;
		d.scale = b.scale;
		points_of(b.order, b.rot, d.pts);
		prefix[i] = (uint32_t)group0;
		group0 += job_table::groups_of(s.n_steps, kBitsThreads);
		step0 += s.n_steps;
	}
	prefix[n_jobs] = (uint32_t)group0;

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_SOFT);
	stats[FOSPHOR_AMD_SOFT_CALLS]++;
	stats[FOSPHOR_AMD_SOFT_JOBS_CRC] += plan.jobs_crc;
	stats[FOSPHOR_AMD_SOFT_STEPS] += plan.steps;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_SOFT, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = static_cast<uint64_t *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.dec = reinterpret_cast<uint64_t *>(d + table.parts_at);
	p.parts = reinterpret_cast<Part *>(d + table.parts_at + dec_bytes);
	p.ends = reinterpret_cast<int32_t *>(d + table.parts_at + dec_bytes + parts_bytes);
	p.words = reinterpret_cast<uint32_t *>(d + table.parts_at + dec_bytes + parts_bytes + ends_bytes);
	p.records = d_records;
	p.n_jobs = n_jobs;
	int rv = 0;
	if (plan.groups) {
		rv = job_table::launch<kBitsThreads>(k_sft_bits, (unsigned)plan.groups, st, p, stats, FOSPHOR_AMD_SOFT_K_BITS);
		if (!rv)
			rv = job_table::launch<kWave>(k_sft_acs, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_SOFT_K_ACS);
		if (!rv)
			rv = job_table::launch<kWave>(k_sft_trace, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_SOFT_K_TRACE);
	}
	if (!rv)
		rv = job_table::launch<kWave>(k_sft_rec, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_SOFT_K_REC);
	return job_table::drain(st, rv);
}
