/*
 * fosphor_rs_host.cpp -- the host side of the Reed-Solomon pass (include/fosphor_amd_rs.h): what rule 7 refuses, the host
 * statement fosphor_amd_rs_host, the encoder, from_decode and derive.  Plain C++: no HIP header, no device, no instance, so that
 * tests/test_rs_sanitized_cpu.py builds this one file under the sanitizers.  The kernels and the device entry point are
 * fosphor_rs.hip; the arithmetic both use is fosphor_rs.h.
 */
#include <errno.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <utility>

#include "fosphor_rs.h"

namespace rs {

typedef struct fosphor_amd_rs_job Job;
typedef struct fosphor_amd_rs_record Record;

constexpr int kFlags = FOSPHOR_AMD_RS_DESCRAMBLE_IN | FOSPHOR_AMD_RS_DESCRAMBLE_OUT;

static_assert(sizeof(Job) == 64, "the job is 64 bytes");
static_assert(sizeof(Record) == 64, "the record is 64 bytes");

/* [offset, offset + n) inside [0, total), safe against offsets of 2^62 */
static bool inside(int64_t offset, int64_t n, int64_t total)
{
	return offset >= 0 && n >= 0 && offset <= total && n <= total - offset;
}

static bool ranges_disjoint(std::vector<std::pair<int64_t, int64_t> > &ranges)
{
	std::sort(ranges.begin(), ranges.end());
	for (size_t i = 1; i < ranges.size(); i++)
		if (ranges[i].first < ranges[i - 1].second)
			return false;
	return true;
}

/* alpha walked through 255 steps comes back to 1 at the last and not before */
static bool primitive(uint32_t poly)
{
	uint32_t x = 1;
	for (int i = 1; i <= 255; i++) {
		x <<= 1;
		if (x & 0x100u)
			x ^= poly;
		if (x == 1)
			return i == 255;
	}
	return false;
}

static int gcd(int a, int b)
{
	for (int i = 0; i < 16 && b; i++) {
		const int r = a % b;
		a = b;
		b = r;
	}
	return a;
}

bool job_ok(const Job &b)
{
	if (b.gf_poly < 0x100 || b.gf_poly > 0x1ff || !primitive(b.gf_poly) || b.fcr > 254 || b.prim < 1 || b.prim > 254 ||
	    gcd(255, b.prim) != 1 || b.n_roots < 2 || b.n_roots > FOSPHOR_AMD_RS_MAX_ROOTS || b.n_code <= b.n_roots ||
	    b.depth < 1 || b.depth > FOSPHOR_AMD_RS_MAX_DEPTH || b.scr_width == 1 || b.scr_width > 32)
		return false;
	const uint64_t limit = 1ull << b.scr_width;				/* w = 0: the fields are 0 */
	if (b.scr_taps >= limit || b.scr_init >= limit)
		return false;
	if ((b.flags & ~kFlags) || b.flags == kFlags || (b.flags && !b.scr_width))
		return false;
	for (int i = 0; i < 7; i++)
		if (b.reserved[i])
			return false;
	return true;
}

void scramble_bytes(int w, uint32_t taps, uint32_t init, uint8_t *seq, int n)
{
	const uint32_t mask = w == 32 ? 0xffffffffu : (1u << w) - 1u;
	uint32_t reg = init;
	for (int p = 0; p < n; p++) {
		uint32_t byte = 0;
		for (int i = 0; i < 8; i++) {
			byte = (byte << 1) | ((reg >> (w - 1)) & 1u);
			const uint32_t fb = (uint32_t)__builtin_popcount(reg & taps) & 1u;
			reg = ((reg << 1) | fb) & mask;
		}
		seq[p] = (uint8_t)byte;
	}
}

/* mode 0: fosphor_amd_rs and fosphor_amd_rs_host; mode 1: the encoder, whose outputs are the frames */
static int check(int64_t n_bytes, const Job *jobs, int n_jobs, int64_t out_capacity, int mode, Plan *plan)
{
	if (!jobs || n_jobs < 1 || n_jobs > FOSPHOR_AMD_RS_MAX_JOBS || n_bytes < 0 || out_capacity < 0)
		return -EINVAL;
	plan->codewords = plan->words = 0;
	plan->seq_at.assign((size_t)n_jobs, -1);
	plan->seq.clear();
	std::vector<std::pair<int64_t, int64_t> > ranges;
	typedef std::tuple<int, uint32_t, uint32_t> Key;
	std::map<Key, int> longest;						/* scrambler -> the bytes the call needs of it */
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_ok(b))
			return -EINVAL;
		const int64_t frame = (int64_t)b.depth * b.n_code;
		const int32_t n_data = n_data_of(b);
		if (!inside(b.offset, frame, n_bytes))
			return -EINVAL;
		if (mode == 0) {
			if ((b.out_offset & 7) || !inside(b.out_offset, owned_of(n_data), out_capacity))
				return -EINVAL;
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + owned_of(n_data)));
		} else {
			if (!inside(b.out_offset, n_data, out_capacity))
				return -EINVAL;
			ranges.push_back(std::make_pair(b.offset, b.offset + frame));
		}
		plan->codewords += b.depth;
		plan->words += owned_of(n_data) / 8;
		if (plan->codewords > FOSPHOR_AMD_RS_MAX_CALL_CODEWORDS)
			return -EINVAL;
		if (b.flags) {
			int &len = longest[Key(b.scr_width, b.scr_taps, b.scr_init)];
			len = std::max(len, (int)((frame + 7) & ~(int64_t)7));
		}
	}
	if (!ranges_disjoint(ranges))
		return -EINVAL;
	std::map<Key, int> at;
	for (std::map<Key, int>::const_iterator it = longest.begin(); it != longest.end(); ++it) {
		at[it->first] = (int)plan->seq.size();
		plan->seq.resize(plan->seq.size() + (size_t)it->second);
		scramble_bytes(std::get<0>(it->first), std::get<1>(it->first), std::get<2>(it->first),
		               plan->seq.data() + at[it->first], it->second);
	}
	for (int i = 0; i < n_jobs; i++)
		if (jobs[i].flags)
			plan->seq_at[i] = at[Key(jobs[i].scr_width, jobs[i].scr_taps, jobs[i].scr_init)];
	return 0;
}

int check_call(int64_t n_bytes, const Job *jobs, int n_jobs, int64_t out_capacity, Plan *plan)
{
	return check(n_bytes, jobs, n_jobs, out_capacity, 0, plan);
}

/* Rules 3 and 4 over one codeword r[0 .. n): -> the number of error positions (0: clean) with pos[] ascending and val[], or
 * FOSPHOR_AMD_RS_FAILED.  Berlekamp-Massey over the n_roots syndromes, the root search over the n positions, Forney's formula. */
static int decode_codeword(const uint8_t *r, const Job &b, int *pos, uint8_t *val)
{
	const uint32_t poly = b.gf_poly;
	const int n = b.n_code, n_roots = b.n_roots, t = n_roots / 2;
	uint32_t S[FOSPHOR_AMD_RS_MAX_ROOTS];
	uint32_t any = 0;
	for (int j = 0; j < n_roots; j++) {
		const uint32_t root = gf_exp(root_exp(b.prim, b.fcr, j), poly);
		uint32_t s = 0;
		for (int i = 0; i < n; i++)
			s = gf_mul(s, root, poly) ^ r[i];
		S[j] = s;
		any |= s;
	}
	if (!any)
		return 0;
	constexpr int kCoef = FOSPHOR_AMD_RS_MAX_ROOTS + 1;
	uint32_t lam[kCoef] = { 1 }, prev[kCoef] = { 1 }, keep[kCoef];
	uint32_t last = 1;
	int L = 0, m = 1;
	for (int k = 0; k < n_roots; k++) {
		uint32_t d = S[k];
		for (int i = 1; i <= L && i <= k; i++)
			d ^= gf_mul(lam[i], S[k - i], poly);
		if (!d) {
			m++;
			continue;
		}
		const uint32_t coef = gf_mul(d, gf_inv(last, poly), poly);
		memcpy(keep, lam, sizeof(lam));
		for (int i = 0; i + m < kCoef; i++)
			lam[i + m] ^= gf_mul(coef, prev[i], poly);
		if (2 * L <= k) {
			L = k + 1 - L;
			memcpy(prev, keep, sizeof(lam));
			last = d;
			m = 1;
		} else {
			m++;
		}
	}
	if (L > t)
		return FOSPHOR_AMD_RS_FAILED;
	int count = 0;
	uint32_t zs[FOSPHOR_AMD_RS_MAX_ROOTS / 2];
	for (int i = 0; i < n; i++) {
		const uint32_t z = gf_exp(inv_locator_exp(b.prim, n, i), poly);
		uint32_t v = 0;
		for (int k = L; k >= 0; k--)
			v = gf_mul(v, z, poly) ^ lam[k];
		if (v)
			continue;
		if (count < L) {
			pos[count] = i;
			zs[count] = z;
		}
		count++;
	}
	if (count != L)
		return FOSPHOR_AMD_RS_FAILED;
	uint32_t omega[FOSPHOR_AMD_RS_MAX_ROOTS / 2];
	for (int j = 0; j < L; j++) {
		uint32_t o = 0;
		for (int k = 0; k <= j; k++)
			o ^= gf_mul(lam[k], S[j - k], poly);
		omega[j] = o;
	}
	for (int e = 0; e < L; e++) {
		const uint32_t z = zs[e];
		uint32_t num = 0, den = 0;
		for (int j = L - 1; j >= 0; j--)
			num = gf_mul(num, z, poly) ^ omega[j];
		for (int k = L; k >= 0; k--)					/* z Lambda'(z): the odd terms of Lambda(z) */
			den = gf_mul(den, z, poly) ^ ((k & 1) ? lam[k] : 0u);
		num = gf_mul(num, gf_pow(z, b.fcr, poly), poly);
		val[e] = (uint8_t)gf_mul(num, gf_inv(den, poly), poly);		/* the roots are simple: den != 0 */
	}
	return L;
}

static void record_begin(const Job &b, Record &r)
{
	memset(&r, 0, sizeof(r));
	r.n_codewords = b.depth;
	r.n_data = n_data_of(b);
	r.n_code = b.n_code;
	r.n_roots = b.n_roots;
}

} // namespace rs

using namespace rs;

extern "C" int fosphor_amd_rs_host(const uint8_t *in, int64_t n_bytes, const struct fosphor_amd_rs_job *jobs, int n_jobs,
                                   struct fosphor_amd_rs_record *records, uint8_t *out, int64_t out_capacity)
{
	if (!in || !records || !out || ((uintptr_t)records & 7) || ((uintptr_t)out & 7))
		return -EINVAL;
	Plan plan;
	if (check(n_bytes, jobs, n_jobs, out_capacity, 0, &plan))
		return -EINVAL;
	std::vector<uint8_t> frame;
	for (int j = 0; j < n_jobs; j++) {
		const Job &b = jobs[j];
		const int I = b.depth, n = b.n_code, n_data = n_data_of(b);
		const uint8_t *seq = plan.seq_at[j] >= 0 ? plan.seq.data() + plan.seq_at[j] : NULL;
		frame.assign(in + b.offset, in + b.offset + (size_t)I * n);
		if (b.flags & FOSPHOR_AMD_RS_DESCRAMBLE_IN)
			for (int p = 0; p < I * n; p++)
				frame[p] ^= seq[p];
		Record r;
		record_begin(b, r);
		for (int c = 0; c < I; c++) {
			uint8_t word[255], val[16];
			int pos[16];
			for (int i = 0; i < n; i++)
				word[i] = frame[(size_t)i * I + c];
			const int count = decode_codeword(word, b, pos, val);
			r.errors[c] = (uint8_t)count;
			if (count == FOSPHOR_AMD_RS_FAILED) {
				r.n_failed++;
				r.failed_mask |= 1u << c;
				continue;
			}
			r.n_clean += count == 0;
			r.corrected_symbols += count;
			r.max_errors = std::max(r.max_errors, count);
			for (int e = 0; e < count; e++) {
				r.corrected_bits += __builtin_popcount(val[e]);
				frame[(size_t)pos[e] * I + c] ^= val[e];
			}
		}
		r.status = r.n_failed ? FOSPHOR_AMD_RS_FAIL : FOSPHOR_AMD_RS_OK;
		uint8_t *o = out + b.out_offset;
		memset(o, 0, (size_t)owned_of(n_data));
		for (int p = 0; p < n_data; p++)
			o[p] = (uint8_t)(frame[p] ^ ((b.flags & FOSPHOR_AMD_RS_DESCRAMBLE_OUT) ? seq[p] : 0));
		records[j] = r;
	}
	return 0;
}

extern "C" int fosphor_amd_rs_encode_host(const uint8_t *data, int64_t data_capacity, const struct fosphor_amd_rs_job *jobs, int n_jobs,
                                          uint8_t *frames, int64_t n_bytes)
{
	if (!data || !frames)
		return -EINVAL;
	Plan plan;
	if (check(n_bytes, jobs, n_jobs, data_capacity, 1, &plan))
		return -EINVAL;
	for (int j = 0; j < n_jobs; j++) {
		const Job &b = jobs[j];
		const uint32_t poly = b.gf_poly;
		const int I = b.depth, n = b.n_code, n_roots = b.n_roots, k = n - n_roots, n_data = I * k;
		const uint8_t *seq = plan.seq_at[j] >= 0 ? plan.seq.data() + plan.seq_at[j] : NULL;
		uint32_t g[FOSPHOR_AMD_RS_MAX_ROOTS + 1] = { 1 };		/* g[i]: the coefficient of x^i */
		for (int q = 0; q < n_roots; q++) {
			const uint32_t root = gf_exp(root_exp(b.prim, b.fcr, q), poly);
			for (int i = q + 1; i >= 1; i--)
				g[i] = g[i - 1] ^ gf_mul(g[i], root, poly);
			g[0] = gf_mul(g[0], root, poly);
		}
		uint8_t *f = frames + b.offset;
		for (int p = 0; p < n_data; p++)
			f[p] = (uint8_t)(data[b.out_offset + p] ^ ((b.flags & FOSPHOR_AMD_RS_DESCRAMBLE_OUT) ? seq[p] : 0));
		for (int c = 0; c < I; c++) {
			uint32_t par[FOSPHOR_AMD_RS_MAX_ROOTS] = { 0 };	/* par[i]: the coefficient of x^i of the remainder */
			for (int i = 0; i < k; i++) {
				const uint32_t fb = f[(size_t)i * I + c] ^ par[n_roots - 1];
				for (int q = n_roots - 1; q >= 1; q--)
					par[q] = par[q - 1] ^ gf_mul(fb, g[q], poly);
				par[0] = gf_mul(fb, g[0], poly);
			}
			for (int i = 0; i < n_roots; i++)
				f[(size_t)(k + i) * I + c] = (uint8_t)par[n_roots - 1 - i];
		}
		if (b.flags & FOSPHOR_AMD_RS_DESCRAMBLE_IN)
			for (int p = 0; p < I * n; p++)
				f[p] ^= seq[p];
	}
	return 0;
}

extern "C" int fosphor_amd_rs_from_decode(int64_t out_offset, int32_t n_bits, int64_t skip_bytes, int n_code, int depth,
                                          struct fosphor_amd_rs_job *job)
{
	if (!job || out_offset < 0 || n_bits < 0 || skip_bytes < 0 || n_code < 3 || n_code > 255 || depth < 1 || depth > FOSPHOR_AMD_RS_MAX_DEPTH)
		return -EINVAL;
	const int64_t bytes = n_bits / 8, frame = (int64_t)depth * n_code;
	if (skip_bytes > bytes || frame > bytes - skip_bytes || out_offset > INT64_MAX - skip_bytes)
		return -EINVAL;
	memset(job, 0, sizeof(*job));
	job->offset = out_offset + skip_bytes;
	job->n_code = (uint8_t)n_code;
	job->depth = (uint8_t)depth;
	return 0;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_rs_derive(const struct fosphor_amd_rs_record *r, struct fosphor_amd_rs_values *v)
{
	if (!r || !v)
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	v->byte_error_rate = finite_or_zero((double)r->corrected_symbols / ((double)r->n_code * ((double)r->n_codewords - (double)r->n_failed)));
	v->failed_share = finite_or_zero((double)r->n_failed / (double)r->n_codewords);
	v->ok = r->status == FOSPHOR_AMD_RS_OK ? 1.0 : 0.0;
	return 0;
}
