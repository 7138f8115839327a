/*
 * fosphor_rs.hip -- the outer code of decoded bursts where they lie: interleaved Reed-Solomon frames over GF(2^8) descrambled,
 * de-interleaved by index arithmetic, every codeword's syndromes, Berlekamp-Massey, root search and Forney's formula, and the
 * corrected data bytes in their transmitted order (include/fosphor_amd_rs.h)
 *
 * A read-only pass over the CALLER's bytes (what fosphor_amd_decode or fosphor_amd_soft wrote), in a file of its own: nothing here
 * is on the process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table,
 * two prefixes, the scrambler sequences, and per codeword its syndromes, a state word and up to 16 corrections).
 *
 *   k_rs_syn   a wave per codeword: the bytes at stride I, descrambled; Horner's rule, lane = syndrome, the two halves of the wave
 *              over the two halves of the codeword.
 *   k_rs_fix   a wave per codeword that is not clean: Berlekamp-Massey with lane = coefficient, the root search four positions a
 *              lane, Forney's formula in the lanes that found a root.
 *   k_rs_out   256 lanes own 256 output words of one job, which they find in the prefix (fosphor_jobs.h); a lane assembles eight
 *              corrected bytes and stores one word.
 *   k_rs_rec   a wave per job sums its codewords and writes the record.
 * All of it is integer work over the helpers of fosphor_rs.h, which fosphor_amd_rs_host (fosphor_rs_host.cpp) uses as well.  No
 * atomics of any kind, no work-group waits for another, no LDS, every loop carries its bound in its header.
 */
#include "fosphor_jobs.h"
#include "fosphor_rs.h"

namespace {

using namespace rs;

typedef struct fosphor_amd_rs_job Job;
typedef struct fosphor_amd_rs_record Record;

constexpr int kWave = 64;
constexpr int kOutThreads = 256;				/* words of a work-group of k_rs_out */
constexpr int kMaxRoots = FOSPHOR_AMD_RS_MAX_ROOTS;
constexpr int kMaxT = kMaxRoots / 2;				/* corrections of a codeword at the most */
constexpr int kFailed = FOSPHOR_AMD_RS_FAILED;
constexpr uint32_t kDirty = 0x100;				/* a state word between k_rs_syn and k_rs_fix: syndromes that are not 0 */
constexpr int kSynWords = kMaxRoots / 4;			/* a codeword's syndromes, four a word */

static_assert(FOSPHOR_AMD_RS_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(FOSPHOR_AMD_RS_MAX_CALL_CODEWORDS == FOSPHOR_AMD_RS_MAX_JOBS * FOSPHOR_AMD_RS_MAX_DEPTH, "the header says so");
static_assert(kMaxRoots == 32 && kMaxT == 16, "half a wave holds the syndromes, 16 lanes the corrections");

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t offset;
	int64_t out_offset;		/* bytes */
	int32_t cw0;			/* the job's first codeword in the scratch */
	int32_t seq_at;			/* where its scrambler sequence begins, -1 without one */
	int32_t n_data, flags;
	int32_t gf_poly, fcr, prim, n_roots, n_code, depth;
	int32_t pad[2];
};

static_assert(sizeof(DevJob) == 64, "a device job is 64 bytes");

struct Params {
	const uint8_t  *in;
	uint64_t       *out;		/* d_out in 64-bit words */
	const DevJob   *jobs;
	const uint32_t *out_prefix;	/* [n_jobs + 1] work-groups of k_rs_out before job j */
	const uint32_t *cw_prefix;	/* [n_jobs + 1] codewords before job j */
	const uint8_t  *seq;		/* rule 1's bytes */
	uint32_t       *syn;		/* [codewords][kSynWords] */
	uint32_t       *state;		/* [codewords] 0 clean, kDirty, then the corrections 1 .. 16 or kFailed */
	uint32_t       *pairs;		/* [codewords][kMaxT] position | value << 8 */
	Record         *records;
	int n_jobs;
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v ^= (uint32_t)__shfl_xor((int)v, d);
	return v;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += __shfl_xor(v, d);
	return v;
}

__device__ __forceinline__ uint32_t lane_of(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

__global__ __launch_bounds__(kWave)
void k_rs_syn(const Params p)
{
	const int lane = threadIdx.x;
	const int cw = (int)blockIdx.x;
	const int j = job_table::find_job(p.cw_prefix, p.n_jobs, blockIdx.x);
	const DevJob &job = p.jobs[j];
	const int c = cw - (int)p.cw_prefix[j];					/* below depth by the prefix */
	const uint32_t poly = (uint32_t)job.gf_poly;
	const int n = job.n_code, I = job.depth, n_roots = job.n_roots;
	/* the codeword behind `lead` (0 or 1) zero bytes, which change no syndrome, is two halves of n1 <= 128 bytes: the lanes of
	 * half h hold the bytes of half h, 32 a register */
	const int n1 = (n + 1) >> 1, lead = 2 * n1 - n;
	const int h = lane >> 5, m = lane & 31;
	const bool descramble = job.flags & FOSPHOR_AMD_RS_DESCRAMBLE_IN;
	const uint8_t *in = p.in + job.offset;
	const uint8_t *seq = p.seq + (job.seq_at >= 0 ? job.seq_at : 0);
	uint32_t a[4];
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int i = h * n1 + k * 32 + m - lead;
		a[k] = 0;
		if (k * 32 + m < n1 && i >= 0) {
			const int at = i * I + c;
			a[k] = in[at];
			if (descramble)
				a[k] ^= seq[at];
		}
	}
	const uint32_t root = gf_exp(root_exp(job.prim, job.fcr, m), poly);
	uint32_t s = 0;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		for (int i = 0; i < 32 && k * 32 + i < n1; i++) {
			const uint32_t v = (uint32_t)__shfl((int)a[k], (lane & 32) | i);
			s = gf_mul(s, root, poly) ^ v;
		}
	}
	/* r(x) = first(x) x^n1 + second(x) */
	const uint32_t second = (uint32_t)__shfl((int)s, m + 32);
	s = gf_mul(s, gf_pow(root, (uint32_t)n1, poly), poly) ^ second;
	if (lane >= n_roots)
		s = 0;
	const bool dirty = __ballot(s != 0) != 0ull;
	const uint32_t word = s | ((uint32_t)__shfl_down((int)s, 1) << 8) | ((uint32_t)__shfl_down((int)s, 2) << 16) |
	                      ((uint32_t)__shfl_down((int)s, 3) << 24);
	if (lane < kMaxRoots && !(lane & 3))
		p.syn[(size_t)cw * kSynWords + (lane >> 2)] = word;
	if (lane == 0)
		p.state[cw] = dirty ? kDirty : 0u;
}

__global__ __launch_bounds__(kWave)
void k_rs_fix(const Params p)
{
	const int lane = threadIdx.x;
	const int cw = (int)blockIdx.x;
	if (__builtin_amdgcn_readfirstlane((int)p.state[cw]) == 0)		/* clean: the whole wave */
		return;
	const int j = job_table::find_job(p.cw_prefix, p.n_jobs, blockIdx.x);
	const DevJob &job = p.jobs[j];
	const uint32_t poly = (uint32_t)job.gf_poly;
	const int n = job.n_code, n_roots = job.n_roots, t = n_roots >> 1;
	const uint32_t S = lane < n_roots ? (p.syn[(size_t)cw * kSynWords + ((lane >> 2) & (kSynWords - 1))] >> (8 * (lane & 3))) & 255u : 0u;

	/* Berlekamp-Massey, lane = coefficient: n_roots rounds whatever the syndromes say */
	uint32_t lam = lane == 0, prev = lane == 0, last = 1;
	int L = 0, m = 1;
	for (int k = 0; k < kMaxRoots && k < n_roots; k++) {
		const uint32_t sv = (uint32_t)__shfl((int)S, (k - lane) & 63);
		const uint32_t term = (lane <= k && lane <= L) ? gf_mul(lam, sv, poly) : 0u;
		const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_xor(term));
		if (!d) {
			m++;
			continue;
		}
		const uint32_t coef = gf_mul(d, gf_inv(last, poly), poly);
		uint32_t moved = (uint32_t)__shfl((int)prev, (lane - m) & 63);
		if (lane < m || lane > kMaxRoots)
			moved = 0;
		const uint32_t keep = lam;
		lam ^= gf_mul(coef, moved, poly);
		if (2 * L <= k) {
			L = k + 1 - L;
			prev = keep;
			last = d;
			m = 1;
		} else {
			m++;
		}
	}
	if (L > t) {								/* uniform */
		if (lane == 0)
			p.state[cw] = kFailed;
		return;
	}
	const int deg = min(L, kMaxT);

	/* the root search: position lane + 64 q */
	uint32_t z[4];
	uint64_t roots[4];
	int count = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const int i = lane + 64 * q;
		z[q] = gf_exp(inv_locator_exp(job.prim, n, min(i, n - 1)), poly);
		uint32_t v = 0;
		for (int k = deg; k >= 0; k--)
			v = gf_mul(v, z[q], poly) ^ lane_of(lam, k);
		roots[q] = __ballot(i < n && v == 0);
		count += __popcll(roots[q]);
	}
	if (count != L) {							/* uniform */
		if (lane == 0)
			p.state[cw] = kFailed;
		return;
	}

	/* Forney: Omega = S Lambda mod x^L, lane = coefficient; then a value per root, in the lane that found it */
	uint32_t omega = 0;
	for (int k = 0; k < kMaxT && k < L; k++) {
		const uint32_t sv = (uint32_t)__shfl((int)S, (lane - k) & 63);
		if (k <= lane && lane < L)
			omega ^= gf_mul(lane_of(lam, k), sv, poly);
	}
	int before = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		if (!roots[q])							/* uniform */
			continue;
		uint32_t num = 0, den = 0;
		for (int k = deg - 1; k >= 0; k--)
			num = gf_mul(num, z[q], poly) ^ lane_of(omega, k);
		for (int k = deg; k >= 0; k--)					/* z Lambda'(z): the odd terms of Lambda(z) */
			den = gf_mul(den, z[q], poly) ^ ((k & 1) ? lane_of(lam, k) : 0u);
		num = gf_mul(num, gf_pow(z[q], (uint32_t)job.fcr, poly), poly);
		const uint32_t value = gf_mul(num, gf_inv(den, poly), poly);
		const int rank = before + __popcll(roots[q] & ((1ull << lane) - 1ull));
		if (((roots[q] >> lane) & 1ull) && rank < kMaxT)
			p.pairs[(size_t)cw * kMaxT + rank] = (uint32_t)(lane + 64 * q) | (value << 8);
		before += __popcll(roots[q]);
	}
	if (lane == 0)
		p.state[cw] = (uint32_t)L;
}

__global__ __launch_bounds__(kOutThreads)
void k_rs_out(const Params p)
{
	const int j = job_table::find_job(p.out_prefix, p.n_jobs, blockIdx.x);
	const DevJob &job = p.jobs[j];
	const int w = (int)(blockIdx.x - p.out_prefix[j]) * kOutThreads + (int)threadIdx.x;
	const int n_data = job.n_data, I = job.depth;
	if (8 * w >= n_data)							/* the job owns ceil(n_data / 8) words */
		return;
	const uint8_t *in = p.in + job.offset;
	const uint8_t *seq = p.seq + (job.seq_at >= 0 ? job.seq_at : 0);
	const bool on_in = job.flags & FOSPHOR_AMD_RS_DESCRAMBLE_IN, on_out = job.flags & FOSPHOR_AMD_RS_DESCRAMBLE_OUT;
	uint64_t word = 0;
#pragma unroll
	for (int b = 0; b < 8; b++) {
		const int at = 8 * w + b;
		if (at >= n_data)
			continue;
		uint32_t byte = in[at];
		if (on_in || on_out)						/* never both: either way the byte of place `at` */
			byte ^= seq[at];
		const int i = at / I, cw = job.cw0 + (at - i * I);
		const int st = (int)p.state[cw];
		const int fixes = st <= kMaxT ? st : 0;				/* kFailed and clean: none */
		for (int e = 0; e < kMaxT && e < fixes; e++) {
			const uint32_t pair = p.pairs[(size_t)cw * kMaxT + e];
			if ((int)(pair & 255u) == i)
				byte ^= pair >> 8;
		}
		word |= (uint64_t)byte << (8 * b);
	}
	p.out[(job.out_offset >> 3) + w] = word;
}

__global__ __launch_bounds__(kWave)
void k_rs_rec(const Params p)
{
	const int lane = threadIdx.x;
	const int j = (int)blockIdx.x;
	const DevJob &job = p.jobs[j];
	const int I = job.depth;
	const bool mine = lane < I;
	const int st = mine ? (int)p.state[job.cw0 + lane] : 0;
	const bool failed = mine && st > kMaxT;
	const int fixes = failed ? 0 : st;
	int bits = 0;
	for (int e = 0; e < kMaxT && e < fixes; e++)
		bits += __popc(p.pairs[(size_t)(job.cw0 + lane) * kMaxT + e] >> 8);
	const uint64_t failed_mask = __ballot(failed);
	const int n_clean = __popcll(__ballot(mine && st == 0));
	const int symbols = wave_sum(fixes);
	bits = wave_sum(bits);
	int most = fixes;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		most = max(most, __shfl_xor(most, d));
	Record r;
	r.n_codewords = I;
	r.n_data = job.n_data;
	r.n_failed = __popcll(failed_mask);
	r.status = r.n_failed ? FOSPHOR_AMD_RS_FAIL : FOSPHOR_AMD_RS_OK;
	r.n_clean = n_clean;
	r.corrected_symbols = symbols;
	r.corrected_bits = bits;
	r.max_errors = most;
	r.failed_mask = (uint32_t)failed_mask;
	const int mark = failed ? kFailed : fixes;
#pragma unroll
	for (int c = 0; c < 16; c++)
		r.errors[c] = (uint8_t)__shfl(mark, c);
	r.n_code = (uint16_t)job.n_code;
	r.n_roots = (uint16_t)job.n_roots;
	r.reserved[0] = r.reserved[1] = 0;
	if (lane == 0)
		p.records[j] = r;
}

} // namespace

extern "C" int fosphor_amd_rs_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_RS_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_RS, FOSPHOR_AMD_RS_STATS, stats);
}

extern "C" int fosphor_amd_rs(struct fosphor *self, const void *d_in, int64_t n_bytes, const struct fosphor_amd_rs_job *jobs, int n_jobs,
                              struct fosphor_amd_rs_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_in || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7))
		return -EINVAL;
	Plan plan;
	if (check_call(n_bytes, jobs, n_jobs, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order, the prefix of their work-groups of k_rs_out and the prefix of their codewords; the
	 * scrambler sequences from the next 8-byte boundary on; behind what is uploaded, per codeword: eight words of syndromes, a
	 * state word, sixteen corrections */
	const size_t n_cw = (size_t)plan.codewords;
	const size_t n_form[2] = { (size_t)n_jobs, 0 }, n_prefix[2] = { (size_t)n_jobs + 1, (size_t)n_jobs + 1 };
	job_table::Table table = job_table::lay_table(sizeof(DevJob), n_form, n_prefix, 0, 8);
	const size_t seq_at = table.parts_at, syn_at = seq_at + ((plan.seq.size() + 7) & ~(size_t)7);
	const size_t state_at = syn_at + sizeof(uint32_t) * kSynWords * n_cw, pairs_at = state_at + sizeof(uint32_t) * n_cw;
	table.bytes = pairs_at + sizeof(uint32_t) * kMaxT * n_cw;
	table.image.resize(syn_at);
	if (!plan.seq.empty())
		memcpy(table.image.data() + seq_at, plan.seq.data(), plan.seq.size());
	DevJob *form = reinterpret_cast<DevJob *>(table.image.data() + table.jobs_at[0]);
	uint32_t *out_prefix = reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[0]);
	uint32_t *cw_prefix = reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[1]);
	long long group0 = 0, cw0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		DevJob &d = form[i];
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.cw0 = (int32_t)cw0;
		d.seq_at = plan.seq_at[i];
		d.n_data = n_data_of(b);
		d.flags = b.flags;
		d.gf_poly = b.gf_poly;
		d.fcr = b.fcr;
		d.prim = b.prim;
		d.n_roots = b.n_roots;
		d.n_code = b.n_code;
		d.depth = b.depth;
		out_prefix[i] = (uint32_t)group0;
		cw_prefix[i] = (uint32_t)cw0;
		group0 += job_table::groups_of(owned_of(d.n_data) / 8, kOutThreads);
		cw0 += b.depth;
	}
	out_prefix[n_jobs] = (uint32_t)group0;
	cw_prefix[n_jobs] = (uint32_t)cw0;

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_RS);
	stats[FOSPHOR_AMD_RS_CALLS]++;
	stats[FOSPHOR_AMD_RS_CODEWORDS] += plan.codewords;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_RS, table, &d, &st))
		return -EIO;
	Params p;
	p.in = static_cast<const uint8_t *>(d_in);
	p.out = static_cast<uint64_t *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.out_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.cw_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[1]);
	p.seq = d + seq_at;
	p.syn = reinterpret_cast<uint32_t *>(d + syn_at);
	p.state = reinterpret_cast<uint32_t *>(d + state_at);
	p.pairs = reinterpret_cast<uint32_t *>(d + pairs_at);
	p.records = d_records;
	p.n_jobs = n_jobs;

	/* the state words come back twice: behind k_rs_syn to see whether k_rs_fix has work, and at the end for the counters */
	std::vector<uint32_t> state(n_cw);
	int rv = job_table::launch<kWave>(k_rs_syn, (unsigned)n_cw, st, p, stats, FOSPHOR_AMD_RS_K_SYN);
	if (rv || hipMemcpyAsync(state.data(), p.state, sizeof(uint32_t) * n_cw, hipMemcpyDeviceToHost, st) != hipSuccess)
		return job_table::drain(st, -EIO);
	if (hipStreamSynchronize(st) != hipSuccess)
		return -EIO;
	const long long clean = std::count(state.begin(), state.end(), 0u);
	stats[FOSPHOR_AMD_RS_CLEAN] += clean;
	const bool fix = clean != plan.codewords;
	if (fix)
		rv = job_table::launch<kWave>(k_rs_fix, (unsigned)n_cw, st, p, stats, FOSPHOR_AMD_RS_K_FIX);
	if (!rv)
		rv = job_table::launch<kOutThreads>(k_rs_out, (unsigned)group0, st, p, stats, FOSPHOR_AMD_RS_K_OUT);
	if (!rv)
		rv = job_table::launch<kWave>(k_rs_rec, (unsigned)n_jobs, st, p, stats, FOSPHOR_AMD_RS_K_REC);
	if (!rv && fix && hipMemcpyAsync(state.data(), p.state, sizeof(uint32_t) * n_cw, hipMemcpyDeviceToHost, st) != hipSuccess)
		rv = -EIO;
	rv = job_table::drain(st, rv);
	if (!rv && fix)
		stats[FOSPHOR_AMD_RS_FAILED_CW] += std::count(state.begin(), state.end(), (uint32_t)kFailed);
	return rv;
}
