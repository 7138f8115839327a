/*
 * fosphor_decide.hip -- PSK decisions over derotated burst symbols where they lie: the nearest of M points per symbol, the sums
 * of the error-vector magnitude, the differences of consecutive decisions, the search for a unique word over positions and
 * rotations, and one byte per symbol with the rotation taken out (include/fosphor_amd_decide.h)
 *
 * A read-only pass over the CALLER's float32 symbols (what fosphor_amd_carrier wrote), in a file of its own: nothing here is on the
 * process / merge path and no buffer of the instance is read or written but the scratch this file owns (the job table, the call's
 * unique-word table, the two prefixes, the tiles' partial records, the work-groups' keys, the jobs' rotations and the decisions).
 *
 *   k_dec_hard  256 lanes own one tile (4096 symbols) of one job, which they find in the prefix (fosphor_jobs.h).  256 symbols a
 *               pass: every lane loads and decides its own symbol; four lanes' decisions leave as one word; a wave's 64 terms are
 *               one block of the ordered sums.
 *   k_dec_uw    256 lanes own 256 candidate positions of one job with a unique word; the decisions they read come from scratch
 *               into LDS, the differences are formed there, every lane counts the values of d[p + i] - u[i] of its position.
 *   k_dec_job   a wave per job adds the tiles in ascending order, reduces the keys and writes the record and the rotation.
 *   k_dec_out   the tiles again, for rules 3 and 5: four symbols a lane, one 32-bit store.
 * In k_dec_hard the lanes write their three terms into rows of 65 doubles, and lanes 0 .. 2 add a row each, in order -- row m begins
 * 130 m dwords into the image, so the three read different banks.  Every sum of doubles is formed by the operations of the helpers
 * below, on the device and in fosphor_amd_decide_host alike; the build's -ffp-contract=off keeps each of them one rounding.  What
 * crosses lanes in another order is integer.  No atomics of any kind, no work-group waits for another, every loop carries its bound
 * in its header.
 */
#include <math.h>

#include "fosphor_jobs.h"
#include "../../include/fosphor_amd_decide.h"

namespace {

typedef struct fosphor_amd_decide_job Job;
typedef struct fosphor_amd_decide_record Record;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlock = FOSPHOR_AMD_DECIDE_BLOCK;
constexpr int kTile = FOSPHOR_AMD_DECIDE_TILE;
constexpr int kPass = kThreads;					/* symbols of a pass of k_dec_hard */
constexpr int kSums = 3;					/* a, b, m2 */
constexpr int kMaxUw = FOSPHOR_AMD_DECIDE_MAX_UW;
constexpr int kUwGroup = FOSPHOR_AMD_DECIDE_UW_GROUP;		/* candidate positions of a work-group of k_dec_uw */
constexpr int kUwWords = (kUwGroup + kMaxUw + 3) / 4 + 1;	/* words that hold 1 + 256 + 63 decisions from any byte of a word on */
constexpr int kOutPass = 4 * kThreads;				/* symbols of a pass of k_dec_out */
constexpr int kDiff = FOSPHOR_AMD_DECIDE_DIFF;
constexpr int kGray = FOSPHOR_AMD_DECIDE_GRAY;
constexpr int kUw = FOSPHOR_AMD_DECIDE_UW;

static_assert(FOSPHOR_AMD_DECIDE_MAX_JOBS <= job_table::kMaxJobs, "the job search is bounded");
static_assert(sizeof(Job) == 64, "the job is 64 bytes");
static_assert(sizeof(Record) == 96, "the record is 96 bytes");
static_assert(kBlock == 64 && kTile == kBlock * kBlock, "a wave's lanes are a block, 64 blocks a tile");
static_assert(kUwGroup == kThreads && kMaxUw <= kBlock, "a lane a position; lanes 0 .. 63 bring the decisions behind the 256");
static_assert(kTile % kOutPass == 0 && kTile / kPass <= 16, "a lane counts at most 16 decisions of a tile in a 16-bit field");

inline bool order_ok(int order) { return order == 2 || order == 4 || order == 8; }

/* rule 7, of what a job says about its word, without the table */
inline bool word_ok(int order, int flags, int uw_offset, int uw_len, int uw_first, int uw_count, int uw_max_errors)
{
	if (!order_ok(order) || (flags & ~(kDiff | kGray | kUw)))
		return false;
	if (!(flags & kUw))
		return !uw_offset && !uw_len && !uw_first && !uw_count && !uw_max_errors;
	return uw_len >= 1 && uw_len <= kMaxUw && uw_offset >= 0 && uw_first >= 0 && uw_count >= 0 && uw_max_errors >= 0;
}

/* rule 4: the candidate positions of a job, first .. first + count - 1; count = 0: none */
inline void candidates_of(const Job &b, int64_t &first, int64_t &count)
{
	first = count = 0;
	if (!(b.flags & kUw))
		return;
	int64_t last = (int64_t)b.n - b.uw_len;
	if (b.uw_count > 0)
		last = std::min(last, (int64_t)b.uw_first + b.uw_count - 1);
	first = std::max((int64_t)b.uw_first, (int64_t)((b.flags & kDiff) ? 1 : 0));
	count = std::max(last - first + 1, (int64_t)0);
}

/* a job on the device, in the caller's order: job j writes record j */
struct DevJob {
	int64_t offset;
	int64_t out_offset;		/* bytes */
	int64_t tile0;			/* the job's first tile: of the partial records and of the decisions */
	int64_t key0;			/* the job's first key */
	int32_t n;
	int32_t order;
	int32_t flags;
	int32_t uw_at;			/* the word in the call's table */
	int32_t uw_len;
	int32_t p_first, p_count;	/* the candidate positions */
	int32_t uw_max_errors;
};

static_assert(sizeof(DevJob) == 64, "a device job is 64 bytes");

/* what k_dec_hard leaves of a tile */
struct TilePart {
	double  s[kSums];
	int32_t cnt[10];		/* the decisions per index, the erasures, 0 */
};

static_assert(sizeof(TilePart) == 64, "a partial record is eight doubles");

struct Params {
	const float2   *iq;
	uint32_t       *out;		/* d_out in words */
	const DevJob   *jobs;
	const uint8_t  *uw;
	const uint32_t *tile_prefix;	/* [n_jobs + 1] symbol tiles before job j */
	const uint32_t *uw_prefix;	/* [n_jobs + 1] work-groups of k_dec_uw before job j */
	TilePart       *parts;
	uint64_t       *keys;
	int32_t        *rot;		/* [n_jobs] uw_rot of rule 4 for k_dec_out */
	uint32_t       *dec;		/* the decisions, four a word, kTile / 4 words a tile */
	Record         *records;
	int n_jobs;
};

inline __host__ __device__ double quiet(double v) { return v != v ? (double)NAN : v; }

/* the tiles of n symbols, n <= 2^31 - 1 */
inline __host__ __device__ int tiles_of(int n) { return (int)(((int64_t)n + kTile - 1) / kTile); }

/* rule 1: the index of one symbol; erased: a NaN angle */
inline __host__ __device__ int decide(int order, float fr, float fi, bool &erased)
{
	const float t = fosphor_amd_atan2_turns((double)fi, (double)fr);
	erased = t != t;
	if (erased)
		return 0;
	return (int)floor(((double)t * (double)order) + 0.5) & (order - 1);
}

/* rule 2: the three terms of a symbol decided as k */
inline __host__ __device__ void sum_terms(int order, int k, float fr, float fi, double *t)
{
	const double sr = fr, si = fi;
	double c, sn;
	fosphor_amd_cossin_turns((double)k / (double)order, &c, &sn);
	t[0] = (sr * c) + (si * sn);
	t[1] = (si * c) - (sr * sn);
	t[2] = (sr * sr) + (si * si);
}

inline __host__ __device__ uint64_t larger(uint64_t a, uint64_t b) { return a > b ? a : b; }

/* rule 4 as one integer: more matches beat fewer, then the smaller p, then the smaller r; every key of a candidate is above 0 */
inline __host__ __device__ uint64_t key_of(int matches, int p, int r)
{
	return ((uint64_t)matches << 35) | ((uint64_t)(0x7fffffff - p) << 3) | (uint64_t)(7 - r);
}

/* rule 4: the best rotation of one position from cnt, eight 8-bit counts of (d[p + i] - u[i]) & (M - 1) */
inline __host__ __device__ uint64_t best_key(uint64_t cnt, int order, int flags, int p)
{
	const int rots = (flags & kDiff) ? 1 : order;
	uint64_t best = 0;
	for (int r = 0; r < 8 && r < rots; r++)
		best = larger(best, key_of((int)((cnt >> (8 * r)) & 0xff), p, r));
	return best;
}

/* rules 1 and 4 into the record, from the job's sums S, its counts and its largest key (0: no candidate) */
inline __host__ __device__ void record_of(int n, int order, int flags, int uw_len, int uw_max_errors, const double *S, const int *hist,
                                          int erasures, uint64_t key, Record &r)
{
	r.n = n;
	r.order = order;
	r.flags = flags;
	r.status = FOSPHOR_AMD_DECIDE_OK;
	r.uw_pos = -1;
	r.uw_rot = 0;
	r.uw_errors = 0;
	r.erasures = erasures;
	r.a = quiet(S[0]);
	r.b = quiet(S[1]);
	r.m2 = quiet(S[2]);
	for (int i = 0; i < 8; i++)
		r.hist[i] = hist[i];
	r.reserved[0] = r.reserved[1] = 0;
	if (!(flags & kUw))
		return;
	r.uw_errors = uw_len;
	if (key) {
		r.uw_pos = 0x7fffffff - (int)((key >> 3) & 0x7fffffff);
		r.uw_rot = 7 - (int)(key & 7);
		r.uw_errors = uw_len - (int)(key >> 35);
	}
	if (!key || r.uw_errors > uw_max_errors)
		r.status = FOSPHOR_AMD_DECIDE_NO_UW;
}

/* rules 3 and 5: the byte of a symbol decided as k behind one decided as k_before (0 for the first) */
inline __host__ __device__ uint32_t output_of(int order, int flags, int rot, int k, int k_before)
{
	const int d = (flags & kDiff) ? (k - k_before) & (order - 1) : k;
	const int q = (d - rot) & (order - 1);
	return (uint32_t)((flags & kGray) ? q ^ (q >> 1) : q);
}

/* the wave's own stores to LDS before its loads from it (the form of fosphor_kernels.hip) */
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* One block of the ordered sums: the wave has written its lanes' terms into s_t[m][lane]; lane m < kSums adds the first `count`
 * of row m in order and leaves the sum as block `block` of the tile. */
__device__ __forceinline__ void block_sums(const double (*s_t)[kBlock + 1], double (*s_bs)[kBlock + 1], int lane, int block, int count)
{
	wave_lds_sync();
	if (lane < kSums) {
		double run = 0.0;
		for (int l = 0; l < kBlock && l < count; l++)
			run = run + s_t[lane][l];
		s_bs[lane][block] = run;
	}
}

/* the largest of a wave's keys, in every lane: integers, so the order is free */
__device__ __forceinline__ uint64_t wave_max(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v = larger(v, (uint64_t)__shfl_xor((unsigned long long)v, d));
	return v;
}

/* the sum of a wave's packed integer fields, in every lane: no field overflows by the caller's bound */
__device__ __forceinline__ uint64_t wave_add(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += (uint64_t)__shfl_xor((unsigned long long)v, d);
	return v;
}

__global__ __launch_bounds__(kThreads)
void k_dec_hard(const Params p)
{
	__shared__ double s_t[kWaves][kSums][kBlock + 1];
	__shared__ double s_bs[kSums][kBlock + 1];
	__shared__ uint64_t s_cnt[kWaves][3];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int j = job_table::find_job(p.tile_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int c = (int)(blockIdx.x - p.tile_prefix[j]);
	const int j0 = c * kTile;						/* the tile's first symbol: below n by the prefix */
	const int syms = min(job.n - j0, kTile);
	const float2 *y = p.iq + job.offset + j0;
	uint32_t *dec = p.dec + (job.tile0 + c) * (kTile / 4);
	/* the lane's counts, at most 16 a field: indices 0 .. 3 and 4 .. 7 in 16-bit fields, the erasures */
	uint64_t cnt_lo = 0, cnt_hi = 0, cnt_er = 0;
	for (int s0 = 0; s0 < syms; s0 += kPass) {
		const int count = min(syms - s0, kPass);			/* symbols of the pass; lane t has symbol j0 + s0 + t */
		double term[kSums];
#pragma unroll
		for (int m = 0; m < kSums; m++)
			term[m] = 0.0;
		int k = 0;
		if (t < count) {
			const float2 v = y[s0 + t];
			bool erased;
			k = decide(job.order, v.x, v.y, erased);
			sum_terms(job.order, k, v.x, v.y, term);
			cnt_lo += k < 4 ? 1ull << (16 * k) : 0ull;
			cnt_hi += k < 4 ? 0ull : 1ull << (16 * (k - 4));
			cnt_er += erased ? 1ull : 0ull;
		}
		/* four lanes' decisions as one word, the pass's last word filled up with 0; every lane takes part in the shuffles */
		const uint32_t word = (uint32_t)k | ((uint32_t)__shfl_down(k, 1) << 8) | ((uint32_t)__shfl_down(k, 2) << 16) |
		                      ((uint32_t)__shfl_down(k, 3) << 24);
		if (!(t & 3) && t < count)
			dec[(s0 + t) >> 2] = word;
#pragma unroll
		for (int m = 0; m < kSums; m++)
			s_t[wave][m][lane] = term[m];
		if (wave * kBlock < count)					/* the whole wave: block (s0 / 64) + wave of the tile */
			block_sums(s_t[wave], s_bs, lane, (s0 >> 6) + wave, count - wave * kBlock);
		__syncthreads();						/* s_t is free; the block sums are written */
	}
	cnt_lo = wave_add(cnt_lo);
	cnt_hi = wave_add(cnt_hi);
	cnt_er = wave_add(cnt_er);
	if (lane == 0) {
		s_cnt[wave][0] = cnt_lo;
		s_cnt[wave][1] = cnt_hi;
		s_cnt[wave][2] = cnt_er;
	}
	__syncthreads();
	TilePart *part = p.parts + (job.tile0 + c);
	if (t < kSums) {							/* the tile's block sums, in order */
		const int blocks = (syms + kBlock - 1) / kBlock;
		double T = 0.0;
		for (int b = 0; b < kBlock && b < blocks; b++)
			T = T + s_bs[t][b];
		part->s[t] = T;
	} else if (t >= 64 && t < 64 + 10) {					/* the counts, by lanes of another wave */
		const int f = t - 64;						/* 0 .. 7: an index; 8: the erasures; 9: the padding */
		uint64_t sum = 0;
		for (int w = 0; w < kWaves; w++)
			sum += f < 8 ? (s_cnt[w][f >> 2] >> (16 * (f & 3))) & 0xffff : (f == 8 ? s_cnt[w][2] : 0);
		part->cnt[f] = (int32_t)sum;
	}
}

__global__ __launch_bounds__(kThreads)
void k_dec_uw(const Params p)
{
	__shared__ uint32_t s_w[kUwWords];					/* the decisions, from an aligned word on */
	__shared__ uint8_t s_d[kUwGroup + kMaxUw];				/* d[p0 ..] */
	__shared__ uint8_t s_u[kMaxUw];
	__shared__ uint64_t s_key[kWaves];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int j = job_table::find_job(p.uw_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int g = (int)(blockIdx.x - p.uw_prefix[j]);
	const int p0 = job.p_first + g * kUwGroup;				/* the first position: a candidate by the prefix */
	const int count = min(job.p_first + job.p_count - p0, kUwGroup);	/* positions of the work-group, 1 .. 256 */
	const int diff = (job.flags & kDiff) ? 1 : 0;				/* p0 >= 1 under DIFF */
	const int lo = p0 - diff;						/* the first decision that is read */
	const int span = count + job.uw_len - 1 + diff;				/* decisions lo .. lo + span - 1 <= n - 1 */
	/* span >= 1 and lo + span <= n, so nothing here passes n: lo + span + 3 would pass 2^31 - 1 in a job of 2^31 - 3 symbols or more */
	const int w0 = lo >> 2, words = ((lo + span - 1) >> 2) + 1 - w0;	/* <= kUwWords; the last ends within the job's tiles */
	const uint32_t *dec = p.dec + job.tile0 * (kTile / 4);
	if (t < words && t < kUwWords)
		s_w[t] = dec[w0 + t];
	if (t < job.uw_len && t < kMaxUw)
		s_u[t] = p.uw[job.uw_at + t];
	__syncthreads();
	const uint8_t *s_k = reinterpret_cast<const uint8_t *>(s_w) + (lo & 3);	/* s_k[m] = k[lo + m] */
	const int mask = job.order - 1;
	for (int m = t; m < count + job.uw_len - 1 && m < kUwGroup + kMaxUw; m += kThreads)	/* at most two turns */
		s_d[m] = (uint8_t)(diff ? (s_k[m + 1] - s_k[m]) & mask : s_k[m]);
	__syncthreads();
	uint64_t key = 0;
	if (t < count) {
		uint64_t cnt = 0;						/* eight 8-bit counts, at most 64 each */
		for (int i = 0; i < kMaxUw && i < job.uw_len; i++)
			cnt += 1ull << (8 * ((s_d[t + i] - s_u[i]) & mask));
		key = best_key(cnt, job.order, job.flags, p0 + t);
	}
	key = wave_max(key);
	if (lane == 0)
		s_key[wave] = key;
	__syncthreads();
	if (t == 0) {
		for (int w = 1; w < kWaves; w++)
			key = larger(key, s_key[w]);
		p.keys[job.key0 + g] = key;
	}
}

__global__ __launch_bounds__(kThreads)
void k_dec_job(const Params p)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int j = (int)blockIdx.x * kWaves + wave;
	if (j >= p.n_jobs)							/* the whole wave; there is no barrier below */
		return;
	const DevJob job = p.jobs[j];
	const int tiles = tiles_of(job.n);
	const TilePart *parts = p.parts + job.tile0;
	/* lanes 0 .. 2 add a sum each over the tiles in ascending order; lanes 8 .. 16 a count each */
	double acc = 0.0;
	int count = 0;
	if (lane < kSums) {
#pragma unroll 8								/* eight loads in flight; the additions keep their order */
		for (int c = 0; c < tiles; c++)
			acc = acc + parts[c].s[lane];
	} else if (lane >= 8 && lane < 17) {
		for (int c = 0; c < tiles; c++)
			count += parts[c].cnt[lane - 8];
	}
	double S[kSums];
	int hist[8];
#pragma unroll
	for (int k = 0; k < kSums; k++)
		S[k] = __shfl(acc, k);
#pragma unroll
	for (int k = 0; k < 8; k++)
		hist[k] = __shfl(count, 8 + k);
	const int erasures = __shfl(count, 16);
	uint64_t key = 0;
	const int groups = (int)(((int64_t)job.p_count + kUwGroup - 1) / kUwGroup);
	for (int g = lane; g < groups; g += 64)
		key = larger(key, p.keys[job.key0 + g]);
	key = wave_max(key);
	Record r;
	record_of(job.n, job.order, job.flags, job.uw_len, job.uw_max_errors, S, hist, erasures, key, r);
	if (lane == 0) {
		p.records[j] = r;
		p.rot[j] = r.uw_rot;
	}
}

__global__ __launch_bounds__(kThreads)
void k_dec_out(const Params p)
{
	const int t = threadIdx.x;
	const int j = job_table::find_job(p.tile_prefix, p.n_jobs, blockIdx.x);
	const DevJob job = p.jobs[j];
	const int rot = p.rot[j];
	const int c = (int)(blockIdx.x - p.tile_prefix[j]);
	const int j0 = c * kTile;						/* the tile's first symbol: below n by the prefix */
	const int syms = min(job.n - j0, kTile);
	const uint32_t *dec = p.dec + (job.tile0 + c) * (kTile / 4);		/* the tile before lies before it */
	uint32_t *out = p.out + (job.out_offset >> 2) + (j0 >> 2);
	for (int s = 4 * t; s < syms; s += kOutPass) {				/* at most kTile / kOutPass turns; a word a lane */
		const int w = s >> 2;
		const uint32_t word = dec[w];
		int before = 0;							/* d[0] = k[0] */
		if (j0 + s > 0)
			before = (int)(dec[w - 1] >> 24);
		uint32_t o = 0;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int k = (int)((word >> (8 * i)) & 0xff);
			if (s + i < syms)					/* the bytes behind the job's last symbol are 0 */
				o |= output_of(job.order, job.flags, rot, k, before) << (8 * i);
			before = k;
		}
		out[w] = o;
	}
}

struct Plan {
	long long tiles, groups, jobs_uw, symbols;
};

/* the bytes a job owns in d_out */
inline int64_t owned_of(int32_t n) { return 4 * (((int64_t)n + 3) / 4); }

/* What both entry points refuse, but for the pointers. */
int check_call(int64_t n_samples, const Job *jobs, int n_jobs, const uint8_t *uw, int n_uw, int64_t out_capacity, Plan *plan)
{
	if (!jobs || !job_table::count_ok(n_jobs, FOSPHOR_AMD_DECIDE_MAX_JOBS) || n_samples < 0 || out_capacity < 0)
		return -EINVAL;
	if (n_uw < 0 || n_uw > FOSPHOR_AMD_DECIDE_MAX_UW_TABLE || (!uw && n_uw))
		return -EINVAL;
	Plan pl = { 0, 0, 0, 0 };
	std::vector<std::pair<int64_t, int64_t> > ranges;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		if (!job_table::inside(b.offset, b.n, n_samples) || b.reserved[0] || b.reserved[1] || b.reserved[2] || b.reserved[3] ||
		    !word_ok(b.order, b.flags, b.uw_offset, b.uw_len, b.uw_first, b.uw_count, b.uw_max_errors))
			return -EINVAL;
		if ((b.out_offset & 3) || !job_table::inside(b.out_offset, owned_of(b.n), out_capacity))
			return -EINVAL;
		int64_t first, count;
		candidates_of(b, first, count);
		if (b.flags & kUw) {
			if (b.uw_len > n_uw - b.uw_offset)
				return -EINVAL;
			for (int k = 0; k < b.uw_len; k++)
				if (uw[b.uw_offset + k] >= b.order)
					return -EINVAL;
			pl.jobs_uw++;
		}
		if (!job_table::add_groups(pl.tiles, b.n, kTile) || !job_table::add_groups(pl.groups, count, kUwGroup))
			return -EINVAL;
		pl.symbols += b.n;
		if (b.n > 0)
			ranges.push_back(std::make_pair(b.out_offset, b.out_offset + owned_of(b.n)));
	}
	if (!job_table::ranges_disjoint(ranges))
		return -EINVAL;
	if (plan)
		*plan = pl;
	return 0;
}

/* the three-level order of rule 2 on the host: terms come in ascending order, one add() each */
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

extern "C" int fosphor_amd_decide_host(const float *iq, int64_t n_samples, const struct fosphor_amd_decide_job *jobs, int n_jobs,
                                       const uint8_t *uw, int n_uw, struct fosphor_amd_decide_record *records,
                                       uint8_t *out, int64_t out_capacity)
{
	if (!iq || !records || !out || ((uintptr_t)iq & 7) || ((uintptr_t)records & 7) || ((uintptr_t)out & 3))
		return -EINVAL;
	if (check_call(n_samples, jobs, n_jobs, uw, n_uw, out_capacity, nullptr))
		return -EINVAL;
	std::vector<uint8_t> k, d;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		const float *y = iq + 2 * b.offset;
		const int mask = b.order - 1;
		Ordered sums[kSums];
		int hist[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, erasures = 0;
		k.resize((size_t)b.n);
		d.resize((size_t)b.n);
		for (int64_t j = 0; j < b.n; j++) {
			bool erased;
			double term[kSums];
			k[j] = (uint8_t)decide(b.order, y[2 * j], y[2 * j + 1], erased);
			sum_terms(b.order, k[j], y[2 * j], y[2 * j + 1], term);
			for (int m = 0; m < kSums; m++)
				sums[m].add(term[m]);
			hist[k[j]]++;
			erasures += erased;
			d[j] = (uint8_t)((b.flags & kDiff) && j ? (k[j] - k[j - 1]) & mask : k[j]);
		}
		double S[kSums];
		for (int m = 0; m < kSums; m++)
			S[m] = sums[m].sum();
		int64_t first, count;
		candidates_of(b, first, count);
		uint64_t key = 0;
		for (int64_t p = first; p < first + count; p++) {
			uint64_t cnt = 0;
			for (int u = 0; u < b.uw_len; u++)
				cnt += 1ull << (8 * ((d[p + u] - uw[b.uw_offset + u]) & mask));
			key = larger(key, best_key(cnt, b.order, b.flags, (int)p));
		}
		Record r;
		memset(&r, 0, sizeof(r));
		record_of(b.n, b.order, b.flags, b.uw_len, b.uw_max_errors, S, hist, erasures, key, r);
		records[i] = r;
		uint8_t *o = out + b.out_offset;
		for (int64_t j = 0; j < owned_of(b.n); j++)
			o[j] = j < b.n ? (uint8_t)output_of(b.order, b.flags, r.uw_rot, k[j], j ? k[j - 1] : 0) : 0;
	}
	return 0;
}

extern "C" int fosphor_amd_decide_from_carrier(const struct fosphor_amd_carrier_job *c, const struct fosphor_amd_carrier_record *r,
                                               int flags, int uw_offset, int uw_len, int uw_first, int uw_count, int uw_max_errors,
                                               struct fosphor_amd_decide_job *job)
{
	if (!c || !r || !job || c->out_offset < 0 || r->n < 0 ||
	    !word_ok(r->order, flags, uw_offset, uw_len, uw_first, uw_count, uw_max_errors))
		return -EINVAL;
	memset(job, 0, sizeof(*job));
	job->offset = c->out_offset;
	job->n = r->status == FOSPHOR_AMD_CARRIER_OK ? r->n : 0;
	job->order = r->order;
	job->flags = flags;
	job->uw_offset = uw_offset;
	job->uw_len = uw_len;
	job->uw_first = uw_first;
	job->uw_count = uw_count;
	job->uw_max_errors = uw_max_errors;
	return 0;
}

static double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }

extern "C" int fosphor_amd_decide_derive(const struct fosphor_amd_decide_record *r, int uw_len, struct fosphor_amd_decide_values *v)
{
	if (!r || !v || uw_len < 0 || uw_len > kMaxUw)
		return -EINVAL;
	memset(v, 0, sizeof(*v));
	if (uw_len > 0)
		v->uw_error_rate = finite_or_zero((double)r->uw_errors / (double)uw_len);
	if (r->n <= 0)
		return 0;
	const double n = r->n, ref = r->a * r->a / n;
	v->gain = finite_or_zero(r->a / n);
	v->evm_rms = finite_or_zero(sqrt(fmax(r->m2 - ref, 0.0) / ref));
	v->mer_db = finite_or_zero(-20.0 * log10(v->evm_rms));
	v->phase_err_rad = finite_or_zero(atan2(r->b, r->a));
	return 0;
}

extern "C" int fosphor_amd_decide_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DECIDE_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_DECIDE, FOSPHOR_AMD_DECIDE_STATS, stats);
}

extern "C" int fosphor_amd_decide(struct fosphor *self, const void *d_iq, int64_t n_samples,
                                  const struct fosphor_amd_decide_job *jobs, int n_jobs, const uint8_t *uw, int n_uw,
                                  struct fosphor_amd_decide_record *d_records, void *d_out, int64_t out_capacity)
{
	if (!self || !d_iq || !jobs || !d_records || !d_out)
		return -EINVAL;
	if (((uintptr_t)d_iq & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 3))
		return -EINVAL;
	Plan plan;
	if (check_call(n_samples, jobs, n_jobs, uw, n_uw, out_capacity, &plan))
		return -EINVAL;

	/* the table: the jobs in the caller's order; in the room of a second form the call's unique-word table, if a job has a word;
	 * the prefix of the jobs' tiles, the prefix of their work-groups of k_dec_uw; behind it, in doubles: the tiles' partial
	 * records, the keys, the jobs' rotations, the decisions */
	const size_t uw_slots = plan.jobs_uw ? ((size_t)n_uw + sizeof(DevJob) - 1) / sizeof(DevJob) : 0;
	const size_t n_form[2] = { (size_t)n_jobs, uw_slots }, n_prefix[2] = { (size_t)n_jobs + 1, (size_t)n_jobs + 1 };
	const size_t part_d = sizeof(TilePart) / sizeof(double), rot_d = ((size_t)n_jobs + 1) / 2, dec_d = kTile / sizeof(double);
	job_table::Table table = job_table::lay_table(sizeof(DevJob), n_form, n_prefix,
	                                              (size_t)plan.tiles * (part_d + dec_d) + (size_t)plan.groups + rot_d, sizeof(double));
	DevJob *form = reinterpret_cast<DevJob *>(table.image.data() + table.jobs_at[0]);
	uint32_t *prefix[2] = { reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[0]),
	                        reinterpret_cast<uint32_t *>(table.image.data() + table.prefix_at[1]) };
	if (uw_slots)
		memcpy(table.image.data() + table.jobs_at[1], uw, (size_t)n_uw);
	int64_t tile0 = 0, key0 = 0;
	for (int i = 0; i < n_jobs; i++) {
		const Job &b = jobs[i];
		int64_t first, count;
		candidates_of(b, first, count);
		DevJob &d = form[i];
		d.offset = b.offset;
		d.out_offset = b.out_offset;
		d.tile0 = tile0;
		d.key0 = key0;
		d.n = b.n;
		d.order = b.order;
		d.flags = b.flags;
		d.uw_at = b.uw_offset;
		d.uw_len = b.uw_len;
		d.p_first = (int32_t)(count ? first : 0);
		d.p_count = (int32_t)count;
		d.uw_max_errors = b.uw_max_errors;
		prefix[0][i] = (uint32_t)tile0;
		prefix[1][i] = (uint32_t)key0;
		tile0 += job_table::groups_of(b.n, kTile);
		key0 += job_table::groups_of(count, kUwGroup);
	}
	prefix[0][n_jobs] = (uint32_t)tile0;
	prefix[1][n_jobs] = (uint32_t)key0;

	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	long long *stats = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_DECIDE);
	stats[FOSPHOR_AMD_DECIDE_CALLS]++;
	stats[FOSPHOR_AMD_DECIDE_JOBS_UW] += plan.jobs_uw;
	stats[FOSPHOR_AMD_DECIDE_SYMBOLS] += plan.symbols;

	uint8_t *d;
	hipStream_t st;
	if (job_table::upload_table(self, FOSPHOR_SCRATCH_DECIDE, table, &d, &st))
		return -EIO;
	Params p;
	p.iq = static_cast<const float2 *>(d_iq);
	p.out = static_cast<uint32_t *>(d_out);
	p.jobs = reinterpret_cast<const DevJob *>(d + table.jobs_at[0]);
	p.uw = d + table.jobs_at[1];
	p.tile_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[0]);
	p.uw_prefix = reinterpret_cast<const uint32_t *>(d + table.prefix_at[1]);
	p.parts = reinterpret_cast<TilePart *>(d + table.parts_at);
	p.keys = reinterpret_cast<uint64_t *>(p.parts + plan.tiles);
	p.rot = reinterpret_cast<int32_t *>(p.keys + plan.groups);
	p.dec = reinterpret_cast<uint32_t *>(reinterpret_cast<double *>(p.rot) + rot_d);
	p.records = d_records;
	p.n_jobs = n_jobs;
	int rv = 0;
	if (plan.tiles)
		rv = job_table::launch<kThreads>(k_dec_hard, (unsigned)plan.tiles, st, p, stats, FOSPHOR_AMD_DECIDE_K_HARD);
	if (plan.groups && !rv)
		rv = job_table::launch<kThreads>(k_dec_uw, (unsigned)plan.groups, st, p, stats, FOSPHOR_AMD_DECIDE_K_UW);
	if (!rv)
		rv = job_table::launch<kThreads>(k_dec_job, (unsigned)job_table::groups_of(n_jobs, kWaves), st, p, stats, FOSPHOR_AMD_DECIDE_K_JOB);
	if (plan.tiles && !rv)
		rv = job_table::launch<kThreads>(k_dec_out, (unsigned)plan.tiles, st, p, stats, FOSPHOR_AMD_DECIDE_K_OUT);
	return job_table::drain(st, rv);
}
