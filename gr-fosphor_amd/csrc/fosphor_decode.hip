/*
 * fosphor_decode.hip -- the decoded bits of burst symbols where they lie: the symbols' bits depunctured into one code byte per
 * trellis step, a Viterbi decoder with one lane per state, the traceback over the whole frame, the decoded bits packed MSB first
 * and a CRC over them (include/fosphor_amd_decode.h)
 *
 * A read-only pass over the CALLER's bytes (what fosphor_amd_decide wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table, the prefix,
 * the survivor decisions, the jobs' ends and the code bytes).
 *
 *   k_dcd_bits   256 lanes own 256 steps of one job, which they find in the prefix (fosphor_jobs.h); a lane forms its step's
 *                code byte, four lanes' bytes leave as one word.
 *   k_dcd_acs    a wave per job, a lane per state: add-compare-select over all steps; __ballot is a step's decision word.
 *   k_dcd_trace  a wave per job walks the decisions back, 64 steps a block, and stores 64 decoded bits a block.
 *   k_dcd_rec    a wave per job runs the CRC over the decoded bits and writes the record.
 * All of it is integer work, formed by the helpers below on the device and in fosphor_amd_decode_host alike.  No atomics of any
 * kind, no work-group waits for another, no LDS, every loop carries its bound in its header.
 */
#include "fosphor_jobs.h"
#include "fosphor_trellis.h"					/* kept_of, expected_of, bit_place, crc_of, steps_that_fit and the checks of the code */
#include "../../include/fosphor_amd_decode.h"

namespace {

using namespace trellis;

typedef struct fosphor_amd_decode_job Job;
typedef struct fosphor_amd_decode_record Record;

constexpr int kWave = 64;
constexpr int kBitsThreads = 256;				/* steps of a work-group of k_dcd_bits */
constexpr int kBlock = FOSPHOR_AMD_DECODE_BLOCK;
constexpr int kInf = FOSPHOR_AMD_DECODE_INF;
constexpr int kMaxSteps = FOSPHOR_AMD_DECODE_MAX_STEPS;
constexpr int kTerminated = FOSPHOR_AMD_DECODE_TERMINATED;

static_assert(FOSPHOR_AMD_DECODE_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 64, "the job is 64 bytes");
static_assert(sizeof(Record) == 64, "the record is 64 bytes");
static_assert(kBlock == kWave, "a wave's lanes are a block of steps, and the states of K = 7");
static_assert(kInf + 3 * kMaxSteps < (1 << 25), "a metric and a state fit one 31-bit key");

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t  offset;
	int64_t  out_offset;		/* bytes */
	int64_t  step0;			/* the job's first step in the codes and the decisions, a multiple of 4 */
	int32_t  n_steps, n_bits, n_coded;
	int32_t  bits;			/* b of rule 1 */
	int32_t  flags, k, n_poly, period;
	int32_t  weight;		/* W of rule 2 */
	int32_t  crc_width;
	uint16_t polys[3], punct[3];
	uint32_t crc_poly, crc_init, crc_xorout;
	int32_t  pad[2];
};

static_assert(sizeof(DevJob) == 96, "a device job is 96 bytes");

struct Params {
	const uint8_t  *sym;
	uint64_t       *out;		/* d_out in 64-bit words */
	const DevJob   *jobs;
	const uint32_t *prefix;		/* [n_jobs + 1] work-groups of k_dcd_bits before job j */
	uint64_t       *dec;		/* a decision word a step */
	int32_t        *ends;		/* [n_jobs][4] end_state, metric, best_state, best_metric */
	uint32_t       *codes;		/* a code byte a step, four a word */
	Record         *records;
	int n_jobs;
};

/* rules 1 and 2: the code byte of step t of a job whose symbol 0 is sym[0]: received bits in bits 0 .. 2, erased flags in 4 .. 6 */
inline __host__ __device__ uint32_t code_of(const uint8_t *sym, int b, int n_poly, int period, const uint16_t *punct, int weight, int t)
{
	int q = (int)kept_of(t, period, punct, weight);			/* below 3 * 65536 */
	const int phase = t % period;
	uint32_t c = 0;
	for (int i = 0; i < 3 && i < n_poly; i++) {
		if ((punct[i] >> phase) & 1) {
			const int s = q / b;
			c |= (uint32_t)((sym[s] >> (b - 1 - (q - s * b))) & 1) << i;
			q++;
		} else {
			c |= 16u << i;
		}
	}
	return c;
}

/* rule 3: the sent bits of a branch that differ from the received ones of code c */
inline __host__ __device__ int branch_of(uint32_t e, uint32_t c) { return popc((e ^ c) & 7u & ~(c >> 4)); }

/* rule 4 as one integer: the least metric, then the smallest state */
inline __host__ __device__ uint32_t end_key(int metric, int state) { return ((uint32_t)metric << 6) | (uint32_t)state; }

/* the whole record, from rule 4's values and the job's owned bytes */
inline __host__ __device__ void record_of(int n_steps, int n_bits, int n_coded, int k, int flags, const int *ends, const uint8_t *out,
                                          int w, uint32_t poly, uint32_t init, uint32_t xorout, Record &r)
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
	r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
}

__global__ __launch_bounds__(kBitsThreads)
void k_dcd_bits(const Params p)
{
	const int tid = threadIdx.x;
	const int j = job_table::find_job(p.prefix, p.n_jobs, blockIdx.x);
	const DevJob &job = p.jobs[j];
	const int t = (int)(blockIdx.x - p.prefix[j]) * kBitsThreads + tid;	/* the group's first step is below n_steps by the prefix */
	uint32_t c = 0;
	if (t < job.n_steps)
		c = code_of(p.sym + job.offset, job.bits, job.n_poly, job.period, job.punct, job.weight, t);
	/* four lanes' codes as one word, the job's last word filled up with 0; every lane takes part in the shuffles */
	const uint32_t word = c | ((uint32_t)__shfl_down((int)c, 1) << 8) | ((uint32_t)__shfl_down((int)c, 2) << 16) |
	                      ((uint32_t)__shfl_down((int)c, 3) << 24);
	if (!(tid & 3) && t < job.n_steps)
		p.codes[(job.step0 + t) >> 2] = word;
}

__global__ __launch_bounds__(kWave)
void k_dcd_acs(const Params p)
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
	const uint8_t *codes = reinterpret_cast<const uint8_t *>(p.codes) + job.step0;
	uint64_t *dec = p.dec + job.step0;
	int metric = lane == 0 ? 0 : kInf;
	for (int t0 = 0; t0 < T; t0 += kBlock) {
		const int count = min(T - t0, kBlock);
		const uint32_t mine = lane < count ? codes[t0 + lane] : 0u;
		uint64_t keep = 0;
		for (int i = 0; i < kBlock && i < count; i++) {
			const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
			const int c0 = __shfl(metric, p0) + branch_of(e0, c);
			const int c1 = __shfl(metric, p1) + branch_of(e1, c);
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
void k_dcd_trace(const Params p)
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
void k_dcd_rec(const Params p)
{
	const int lane = threadIdx.x;
	const int j = (int)blockIdx.x;
	const DevJob &job = p.jobs[j];
	int ends[4] = { 0, 0, 0, 0 };
	if (job.n_steps > 0) {
#pragma unroll
		for (int i = 0; i < 4; i++)
			ends[i] = p.ends[4 * j + i];
	}
	Record r;
	record_of(job.n_steps, job.n_bits, job.n_coded, job.k, job.flags, ends, reinterpret_cast<const uint8_t *>(p.out) + job.out_offset,
	          job.crc_width, job.crc_poly, job.crc_init, job.crc_xorout, r);
	if (lane == 0)
		p.records[j] = r;
}

struct Shape {
	int32_t n_steps, n_bits, n_coded, weight;
};

struct Plan {
	long long groups, steps, jobs_crc;
	std::vector<Shape> shape;
};

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_bytes, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_DECODE_MAX_JOBS) || n_bytes < 0 || out_capacity < 0)
		return -EINVAL;
	plan->groups = plan->steps = plan->jobs_crc = 0;
	plan->shape.resize((size_t)n_jobs);
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		Shape &s = plan->shape[i];
		if (!job_table::inside(b.offset, b.n, n_bytes) || b.reserved || !order_ok(b.order) || (b.flags & ~kTerminated) ||
		    b.k < 3 || b.k > 7 || b.steps < 0 || !punct_ok(b.n_poly, b.period, b.punct, &s.weight))
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
		if (plan->steps > FOSPHOR_AMD_DECODE_MAX_CALL_STEPS)
			return -EINVAL;
		if (s.n_bits > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + owned_of(s.n_bits)));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	return 0;
}

} // namespace

extern "C" int fosphor_amd_decode_host(const uint8_t *sym, int64_t n_bytes, const struct fosphor_amd_decode_job *jobs, int n_jobs,
                                       struct fosphor_amd_decode_record *records, uint8_t *out, int64_t out_capacity)
{
	if (!sym || !records || !out || ((uintptr_t)records & 7) || ((uintptr_t)out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_bytes, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;
	std::vector<uint64_t> dec;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const Shape &s = plan.shape[i];
		const int T = s.n_steps, k = b.k, S = 1 << (k - 1);
		uint32_t e[2][kWave];
		int metric[kWave], next[kWave];
		for (int st = 0; st < S; st++) {
			for (int x = 0; x < 2; x++)
				e[x][st] = expected_of(b.polys, b.n_poly, k, st >> (k - 2), ((st << 1) | x) & (S - 1));
			metric[st] = st ? kInf : 0;
		}
		dec.resize((size_t)T);
		for (int t = 0; t < T; t++) {
			const uint32_t c = code_of(sym + b.offset, bits_of(b.order), b.n_poly, b.period, b.punct, s.weight, t);
			uint64_t word = 0;
			for (int st = 0; st < S; st++) {
				const int p0 = (st << 1) & (S - 1);
				const int c0 = metric[p0] + branch_of(e[0][st], c), c1 = metric[p0 | 1] + branch_of(e[1][st], c);
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
		record_of(T, s.n_bits, s.n_coded, k, b.flags, ends, o, b.crc_width, b.crc_poly, b.crc_init, b.crc_xorout, r);
		records[i] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_decode_steps(int n, int order, int n_poly, int period, const uint16_t punct[3])
{
	int weight;
	if (n < 0 || !order_ok(order) || !punct_ok(n_poly, period, punct, &weight))
		return -EINVAL;
	const int64_t T = steps_that_fit((int64_t)n * bits_of(order), period, punct, weight);
	return T > 0x7fffffff ? -EINVAL : (int)T;
}

extern "C" int fosphor_amd_decode_from_decide(const struct fosphor_amd_decide_job *d, const struct fosphor_amd_decide_record *r,
                                              int uw_len, int n_payload, struct fosphor_amd_decode_job *job)
{
	if (!d || !r || !job || d->out_offset < 0 || d->n < 0 || !order_ok(r->order) || uw_len < 0 || n_payload < 0)
		return -EINVAL;
	int64_t skip = 0, rest = d->n;
	if (d->flags & FOSPHOR_AMD_DECIDE_UW) {
		if (r->status != FOSPHOR_AMD_DECIDE_OK) {
			rest = 0;
		} else {
			skip = (int64_t)r->uw_pos + uw_len;
			if (r->uw_pos < 0 || skip > d->n)
				return -EINVAL;
			rest = d->n - skip;
		}
	}
	const bool lost = (d->flags & FOSPHOR_AMD_DECIDE_UW) && r->status != FOSPHOR_AMD_DECIDE_OK;
	if (!lost && n_payload > rest)
		return -EINVAL;
	memset(job, 0, sizeof(*job));
	job->offset = d->out_offset + skip;
	job->n = (int32_t)(lost ? 0 : (n_payload ? n_payload : rest));
	job->order = r->order;
	return 0;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_decode_derive(const struct fosphor_amd_decode_record *r, struct fosphor_amd_decode_values *v)
{
	if (!r || !v)
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	v->channel_ber = finite_or_zero((double)r->metric / (double)r->n_coded);
	v->rate = finite_or_zero((double)r->n_steps / (double)r->n_coded);
	v->crc_ok = r->status == FOSPHOR_AMD_DECODE_OK ? 1.0 : 0.0;
	return 0;
}

extern "C" int fosphor_amd_decode_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DECODE_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_DECODE, FOSPHOR_AMD_DECODE_STATS, stats);
}

extern "C" int fosphor_amd_decode(struct fosphor *self, const void *d_sym, int64_t n_bytes,
                                  const struct fosphor_amd_decode_job *jobs, int n_jobs,
                                  struct fosphor_amd_decode_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_sym || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_bytes, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order and the prefix of their work-groups of k_dcd_bits; behind it, in bytes from an
	 * 8-byte boundary on: a decision word a step, the jobs' ends, a code byte a step.  A job's steps begin at a multiple of 4. */
	std::vector<int64_t> step0((size_t)n_jobs);
	int64_t steps_at = 0;
	for (int i = 0; i < n_jobs; i++) {
		step0[i] = steps_at;
		steps_at += ((int64_t)plan.shape[i].n_steps + 3) & ~(int64_t)3;
	}
	const size_t n_form[2] = { (size_t)n_jobs, 0 }, n_prefix[2] = { (size_t)n_jobs + 1, 0 };
	const size_t dec_bytes = sizeof(uint64_t) * (size_t)steps_at, ends_bytes = 4 * sizeof(int32_t) * (size_t)n_jobs;
	job_table::Table table = job_table::lay_table(sizeof(DevJob), n_form, n_prefix, dec_bytes + ends_bytes + (size_t)steps_at, 1);
	DevJob *form = reinterpret_cast<DevJob *>(table.image.data() + table.jobs_at[0]);
	uint32_t *prefix = reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[0]);
	int64_t group0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const Shape &s = plan.shape[i];
		DevJob &d = form[i];
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.step0 = step0[i];
		d.n_steps = s.n_steps;
		d.n_bits = s.n_bits;
		d.n_coded = s.n_coded;
		d.bits = bits_of(b.order);
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
		prefix[i] = (uint32_t)group0;
		group0 += job_table::groups_of(s.n_steps, kBitsThreads);
	}
	prefix[n_jobs] = (uint32_t)group0;

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_DECODE);
	stats[FOSPHOR_AMD_DECODE_CALLS]++;
	stats[FOSPHOR_AMD_DECODE_JOBS_CRC] += plan.jobs_crc;
	stats[FOSPHOR_AMD_DECODE_STEPS] += plan.steps;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_DECODE, table, &d, &st))
		return -EIO;
	Params p;
	p.sym = static_cast<const uint8_t *>(d_sym);
	p.out = static_cast<uint64_t *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.dec = reinterpret_cast<uint64_t *>(d + table.parts_at);
	p.ends = reinterpret_cast<int32_t *>(d + table.parts_at + dec_bytes);
	p.codes = reinterpret_cast<uint32_t *>(d + table.parts_at + dec_bytes + ends_bytes);
	p.records = d_records;
	p.n_jobs = n_jobs;
	int rv = 0;
	if (plan.groups) {
		rv = job_table::launch<kBitsThreads>(k_dcd_bits, (unsigned)plan.groups, st, p, stats, FOSPHOR_AMD_DECODE_K_BITS);
		if (!rv)
			rv = job_table::launch<kWave>(k_dcd_acs, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_DECODE_K_ACS);
		if (!rv)
			rv = job_table::launch<kWave>(k_dcd_trace, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_DECODE_K_TRACE);
	}
	if (!rv)
		rv = job_table::launch<kWave>(k_dcd_rec, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_DECODE_K_REC);
	return job_table::drain(st, rv);
}
