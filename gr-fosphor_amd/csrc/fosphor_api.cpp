/*
 * fosphor_api.cpp -- C ABI of libfosphor_amd.so (include/fosphor.h, include/fosphor_amd.h)
 *
 * Host runtime that replaces lib/fosphor/cl.c + the compute half of
 * lib/fosphor/fosphor.c: device buffers, lazy window upload (cl.c:889-900),
 * first-run fills (cl.c:406-465), per-call launch sequence (cl.c:903-954),
 * waterfall ring position (cl.c:954,1073-1079), histogram range (cl.c:1081-1089),
 * tri-state BOOTING/PENDING/READY (cl.c:92-96), errno-style returns.
 *
 * There is no CPU fallback: without a HIP device fosphor_init() fails loudly.
 */
#include <assert.h>
#include <errno.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fosphor_internal.h"
#include "fosphor_jobs.h"
#include "../../include/fosphor_amd.h"
#include "../../include/fosphor_amd_sink.h"
#include "../../include/fosphor_amd_wire.h"
#include "../../include/fosphor_portable_math.h"

using namespace fosphor_amd;

#define FOSPHOR_AMD_VERSION "fosphor_amd 0.1 gfx950"

#define HIP_TRY(expr, what) do { \
		hipError_t _e = (expr); \
		if (_e != hipSuccess) { \
			fprintf(stderr, "[!] fosphor_amd: %s: %s\n", what, hipGetErrorString(_e)); \
			goto error; \
		} \
	} while (0)

enum { ST_BOOTING = 0, ST_PENDING = 1, ST_READY = 2 };	/* cl.c:92-96 */

static const int kMaxN = 65536;
static const int kSets = 5;		/* intermediate (bin index / partial) sets in rotation */
static const int kMaxK1Streams = 4;	/* `stream` + up to three more FFT streams */
/* N = 8192, space sharing: the FFT kernel (one work-group per CU, every register of it) takes 224 CUs when a launch's tiles divide
 * evenly among them, and the count / merge kernels of the launch before run on the 32 it leaves free -- the dispatcher fills CUs it
 * finds empty, no CU mask involved (hardware masks that remove CUs unevenly from the shader engines unbalance a grid of CU-sized
 * work-groups: tools/ubench/cu_mask_big.hip).  Measured at BASELINE C3: 333 -> 367-371 GSamples/s with 28 batches per call, 358
 * with 14, 345 with 7; 232 / 240 CUs leave the tail too little (it becomes the longer side), 216: 356 (DESIGN.md sections 4-5; DESIGN_HISTORY.md section 8). */
static const int kK1wShareCus = 224;	/* (208 / 240 with 26 / 30 batches per call measured no better, profiles/r06_c3.md) */
static const int kSubSamplesLog2 = 26;	/* default sub-launch: 64 Mi samples (64 reference batches of 1024 x 1024) */

static const int kRiseMax = 8192;	/* largest batch served by the rise/decay table */

/* An event that may not have been recorded yet: the work queued on one stream that work on another must follow.  Nothing waits
 * for a fence that was never recorded (or that was forgotten: `recorded = 0`). */
struct Fence
{
	hipEvent_t  ev;
	int         recorded;
	hipStream_t stream;			/* the stream it was last recorded on */

	hipError_t create(unsigned flags) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }	/* (no-op when it exists) */
	/* behind everything queued on st so far */
	hipError_t record(hipStream_t st)
	{
		const hipError_t e = hipEventRecord(ev, st);
		if (e == hipSuccess) { recorded = 1; stream = st; }
		return e;
	}
	/* what is queued on st next follows the record; unless_same: not when st is the stream of the record (stream order does it) */
	hipError_t wait(hipStream_t st, bool unless_same = false) const
	{
		if (!recorded || (unless_same && stream == st))
			return hipSuccess;
		return hipStreamWaitEvent(st, ev, 0);
	}
};

/* Every fence of an instance (nothing but Fence members: fosphor_amd_init and fosphor_release walk them as an array) */
struct Fences
{
	/* made by fosphor_amd_init, with dep_event_flags() */
	Fence wf[2];				/* last K1 that stored rows into ring b */
	Fence in;				/* what the caller queued on `stream` before a call, for the other FFT streams */
	Fence k1_done[kSets];			/* K1 wrote set pp */
	Fence set_free[kSets];			/* K2 finished reading set pp */
	Fence k2_done[2];			/* K2 wrote hit-count set h */
	Fence h_free[2];			/* K3 finished reading hit-count set h */
	Fence k3_done;				/* orders K3s that are issued on different streams */
	Fence tail;				/* N = 8192: behind the merge kernel of the last launch (is there a tail to share the chip with?) */
	/* made with the stream or the staging slot they belong to */
	Fence k1s_done[kMaxK1Streams];
	Fence stage_free[2];
	Fence upload_slot[2];			/* upload into d_stage[k] done: the instance's stream waits for it before the FFT kernel */
	Fence upload_done;			/* H2D of the last fosphor_amd_process_pinned */
};
static const int kInitFences = offsetof(Fences, k1s_done) / sizeof(Fence);
static const int kFences = sizeof(Fences) / sizeof(Fence);
static_assert(sizeof(Fences) == kFences * sizeof(Fence) && offsetof(Fences, upload_done) == (kFences - 1) * sizeof(Fence), "Fences is an array of Fence");

struct fosphor
{
	/* geometry / constants */
	int log2n, n, n_bins, wf_rows;
	int bins16;				/* bin indices are 16-bit (2 spectra per dword) */
	int tw_len, tw_off[8];
	float t0r, t0d, alpha;
	int max_spectra, max_batches;
	int iq_format;				/* FOSPHOR_AMD_IQ_*: fp32, fp16 (N = 65536 only) or sc16 pairs */
	size_t sample_bytes;			/* bytes per sample of that format: 8, 4, 4 */
	size_t stage_samples;			/* capacity of one host staging slot, samples */

	/* reference-visible settings (private.h:44-54) */
	float fft_win[kMaxN];
	int   win_dirty;
	struct { int db_ref, db_per_div; float scale, offset; } power;
	struct { double center, span; } frequency;
	float histo_scale, histo_offset;	/* cl.c:1087-1088 */
	int   thr_dirty;

	/* device */
	int device;
	hipStream_t stream;
	int own_stream;
	float    *d_win;
	float2   *d_tw;
	double   *d_thr;
	float    *d_wf_pp[2], *d_hist;		/* two waterfall rings: a call that rewrites every row targets the other one,
						 * so its K1s need not wait for the previous call's (see run()) */
	int       wf_cur;			/* ring the results are in */
	Fences    f;
	float2   *d_spectrum;
	uint32_t *d_bins_pp[kSets];		/* rotating sets: K1 of launch i+1 overlaps K2/K3 of launch i */
	float2   *d_partial_pp[kSets];
	uint32_t *d_bins;			/* current set */
	float2   *d_partial;
	int       pp;
	hipStream_t k1_streams[kMaxK1Streams];	/* [0] = `stream`; the K1s of consecutive sub-launches of a device-resident call rotate over
						 * n_k1_streams of them: the next K1s are already queued when work-groups of the current one exit */
	int       n_sets;			/* intermediate sets in use (3, <= kSets) */
	int       n_k1_streams;			/* FOSPHOR_AMD_K1_STREAMS (default 2) */
	int       alt;				/* FOSPHOR_AMD_ALT=0 keeps every K1 on `stream` */
	int       k1_seq;
	int       relaxed;			/* fosphor_amd_set_input_ordering(self, 0) */
	long long sub_samples;			/* samples per sub-launch of a device-resident call */
	hipStream_t stream2;			/* K2 (and K3 unless pipe3) of the multi-batch path */
	hipStream_t stream3;			/* K3 of the multi-batch path: K3 of launch i beside K2 of launch i+1 */
	int       pipe3;			/* FOSPHOR_AMD_PIPE3=0 keeps K3 on stream2 */
	int       hset;				/* hit-count / live-sum set of the next launch (two, like the bin sets) */
	hipStream_t last_k3_stream;
	hipStream_t k2_stream_last;		/* stream of the most recent count kernel */
	int       overlap;			/* 1: two-stream pipeline for process paths */
	int       k1_variant;			/* FOSPHOR_AMD_K1: 1 (default) = wave per spectrum, 2 = two waves per spectrum (what odd hops use) */
	/* tuning / test knobs, read from the environment ONCE, at init (nothing on the submit path calls getenv) */
	int       kn_tile;			/* FOSPHOR_AMD_TILE: spectra per tile, 0 = pick_tile's choice */
	int       kn_rowmask_off;		/* FOSPHOR_AMD_ROWMASK=0: dense count hand-off at N = 65536 */
	int       kn_no_sum16;			/* FOSPHOR_AMD_NO_SUM16 */
	int       kn_frame_group;		/* FOSPHOR_AMD_FRAME_GROUP: chunks per count work-group of a sharded frame (default 4) */
	int       kn_k1w_share_off;		/* FOSPHOR_AMD_K1W_SHARE=0: no space sharing at N = 8192 */
	int       n_cus;			/* hipDeviceProp_t::multiProcessorCount */
	int       share_cus;			/* N = 8192: work-groups of an FFT launch that leaves CUs to the count / merge kernels (0: never) */
	long long k1w_shared, k1w_full;		/* N = 8192: FFT launches made in the shared / the full-chip form (fosphor_amd_share_stats) */
	long long k3_forms[K3_FORMS], k3_rise_mem;	/* merge launches by form; long-batch launches that read the (d, e) table from memory (fosphor_amd_merge_stats) */
	const uint32_t *k3_listed;		/* device word holding the row count of the last sparse launch's list, and the stream it ran on */
	hipStream_t k3_listed_stream;
	int       k3_sparse_max[2];		/* most batches in one sparse launch: batches up to 1024 spectra / longer ones */
	long long acc_pieces, n_k2c, n_k2b;	/* FFT pieces launched by accumulate(); chunk sums (k2c) / chunk reduces (k2b) launched (fosphor_amd_launch_stats) */
	uint32_t *d_hc;
	uint32_t *d_hc_export;			/* [n_bins][N] last batch, written by K3 on the 16-bit path */
	const uint16_t *export_src;		/* ... made from the last batch's slabs when fosphor_amd_get_buffers asks */
	const uint32_t *export_mask;
	hipStream_t export_stream;		/* the stream the K2 that wrote export_src ran on */
	uint32_t *d_rowmask;			/* K2 -> K3: one bit per (batch, slab, bin row) "this row has counts and is stored"; 2 sets */
	int       mask_words;			/* ceil(n_bins / 32) */
	uint8_t  *d_hot;			/* [N/64][n_bins]: some cell of the row is above the fast-exit level (K3 maintains it) */
	uint32_t *d_rowlist;			/* [2 + rows]: the live rows of a merge (sparse form) between two counts used alternately */
	int       rowlist_flip;
	int       hot_valid;			/* 0 after anything but the 16-bit K3 wrote the histogram */
	uint16_t *d_slab16;			/* per-chunk packed 16-bit count slabs of batches longer than 1024 spectra / of a shard */
	int       slab_chunks;			/* capacity of d_slab16 in 1024-spectrum chunks */
	const uint32_t *hc_view;		/* the hit counts of the last batch merged, as fosphor_amd_get_buffers shows them */
	float    *d_live_sum, *d_vmax;
	float    *d_chunk_sum, *d_chunk_max;	/* [max_spectra/16][N] */
	long long *d_dbg;			/* K1_TIMING builds only (FOSPHOR_AMD_K1_TIMING=1) */
	uint32_t *d_palette;			/* colour-map scratch (fosphor_cmap.hip), allocated on first use */
	long long counters[FOSPHOR_COUNTERS_COUNT][FOSPHOR_COUNTERS_MAX];	/* launches, calls, jobs of the passes in files of their own, by FOSPHOR_COUNTERS_*
						 * (fosphor_pass.h): host counters that only grow, behind every fosphor_amd_*_stats of theirs */
	struct {				/* scratch of detect, mask, burst (two) and of the passes over burst IQ (job tables, partials), by */
		void  *d;			/* FOSPHOR_SCRATCH_* (fosphor_pass.h); grown on demand, the instance never reads them */
		size_t cap;
	} scratch[FOSPHOR_SCRATCH_COUNT];
	/* compact wire of the sharded frame (fosphor_wire.hip, include/fosphor_amd_wire.h); every buffer is allocated on first use */
	struct {
		uint32_t *d_masks;		/* [mask_cap][rows / 32] presence bits, one part per rank */
		int       mask_cap;		/* parts d_masks holds */
		int       world;		/* parts it is laid out for (the last mask stage's world) */
		int       masked;		/* world of a mask stage no sparse pack has consumed yet, else 0 */
		int       masked_slot, packed_slot;	/* the slot that mask stage read; the slot the last pack read */
		uint32_t *d_union, *d_prefix;	/* [rows / 32] union mask, live rows in the words before each */
		uint32_t *d_live;		/* the union's live-row count, for the row copies ... */
		uint32_t *h_live;		/* ... and in pinned host memory, for the host (the one wait of the sparse form) */
		uint32_t *d_words;		/* [cells / 2] wire words */
		int       form;			/* form the last pack took, 0 once it is unpacked */
		int       n_words, live_rows;	/* of the last pack */
		long long stats[FOSPHOR_AMD_WIRE_STATS];
		hipEvent_t ev[6];		/* (start, stop) of the last mask / pack / unpack launch made while profiling was on */
		int       ev_rec[3];
	} wire;
	float2   *d_rise;			/* [kRiseMax+1] (d, e) per hit count */
	float2   *h_rise;			/* pinned */
	int       rise_batch;			/* batch the table was built for (0 = none) */
	float     rise_t0r, rise_t0d;
	int       slot;				/* partial-array slot used by accumulate/merge */
	float2   *d_scratch;			/* N = 65536: [max_spectra][N] spectrum between the two FFT stages */
	uint32_t *d_k1h_sync;			/* N = 65536 (both levels of the plan in one kernel, the intermediate in the XCDs' L2): its cluster counters */
	uint32_t *h_k1h_err;			/* ... and its error word (host memory the kernel writes: work-groups of a cluster on different XCDs) */

	/* host->device staging for fosphor_process (pinned ring of 2) */
	float2   *h_stage[2];
	float2   *d_stage[2];
	hipStream_t copy_stream;		/* the H2D of fosphor_amd_process_pinned is queued here, so that the upload of one batch runs beside
						 * the kernels of the batch before (created by the first fosphor_amd_process_pinned) */
	size_t    d_stage_cap[2];		/* samples d_stage[k] holds */
	int       pend_slot[2], pend_len[2], pend_head, pend_n;	/* uploads queued by fosphor_amd_upload_pinned, kernels not yet */
	int       stage_idx;
	double   *h_thr;			/* pinned, n_bins+1 */
	float    *h_win;			/* pinned, N */

	/* state */
	int state;
	int wf_pos;

	/* where a launch's count hand-off lives */
	size_t cells() const { return (size_t)n_bins * n; }
	uint32_t *hc_slot(int slot) const { return d_hc + (size_t)slot * cells(); }				/* 32-bit counts of one batch */
	uint16_t *hc16_set(int hset) const { return (uint16_t *)d_hc + (size_t)hset * max_batches * cells(); }	/* 16-bit counts of a launch */
	int       live_slot(int slot, int hset) const { return slot + hset * max_batches; }			/* live-sum / max slot ... */
	float    *live_sum_at(int lslot) const { return d_live_sum + (size_t)lslot * n; }			/* ... and its arrays */
	float    *vmax_at(int lslot) const { return d_vmax + (size_t)lslot * n; }
	uint32_t *rowmask_set(int hset) const { return d_rowmask + (size_t)hset * max_batches * (n / 64) * mask_words; }

	/* profiling */
	int prof;				/* 0 off, 1 every kernel, 2 K1 only (fewer events beside K2/K3) */
	int prof_open;
	std::vector<hipEvent_t> ev_pool;
	std::vector<int> ev_kind;		/* kernel index per (start, stop) pair */
	size_t ev_used;
	std::vector<hipEvent_t> xev_pool;	/* (start, stop) pairs around the exchanges of the multi-GPU path, while profiling is on */
	size_t xev_used;
};

/* ------------------------------------------------------------------------ */
/* Host-side tables                                                         */
/* ------------------------------------------------------------------------ */

/* Twiddles.  N = 1024: exactly as the reference forms them (fft.cl:62-68,162-166,286-297), native_sin / native_cos pinned to
 * fosphor_portable_math.h; one block per radix-8 pass with p = 8, 64 ([k < p][n = 1..7]), then the final radix-2 pass
 * ([k < N/2]): the kTw2Off / kTw3Off / kTw4Off layout of fosphor_internal.h.
 *
 * N = 8192 and N = 65536 run this build's own plans (no reference behaviour exists at these lengths; oracle/fosphor_oracle.c,
 * o_pass_radix8_fma / o_pass_radix16_fma / o_pass_radix2_fma, restates them): the reference's Stockham passes with the twiddles
 * ON the radix-2 butterflies of a pass instead of on its inputs, so an item needs the twiddles of its stages -- every one of them
 * exp(-j pi q / den) for integers q, den, formed like the reference's (one float expression, pinned sin / cos): tw_long().
 *   both:       block  0    the constants W16, W8, W16^3 (first pass)
 *   N = 8192:   blocks 1-2  passes p = 16, 256: [k < p][8] = w^8, w^4, w^2, w^2 W8, w, w W16, w W8, w W16^3   (w = exp(-j pi k / (8 p)))
 *               block  3    the radix-2 pass: [k < 4096] = exp(-j pi k / 4096)
 *   N = 65536:  blocks 1-3  passes p = 16, 256, 4096: [k < p][8], as above */
static float2 tw_long(int q, int den)
{
	const float PI_F = 3.141592653589f;		/* fft.cl:26 */
	const float arg = -PI_F * (float)q / (float)den;
	return make_float2(fpm_cosf(arg), fpm_sinf(arg));
}

static int build_twiddles16(float2 *tw, int *offsets /* [8] or NULL */)
{
	int pos = 0, q = 0;
	if (offsets) offsets[q] = pos;
	q++;
	for (int m = 1; m <= 3; m++) {
		if (tw) tw[pos] = tw_long(m, 8);
		pos++;
	}
	for (int p = 16; p <= 4096; p *= 16, q++) {
		if (offsets) offsets[q] = pos;
		const int d = 8 * p;
		for (int k = 0; k < p; k++) {
			const int qs[8] = { 8 * k, 4 * k, 2 * k, 2 * k + 2 * p, k, k + p, k + 2 * p, k + 3 * p };
			for (int f = 0; f < 8; f++) {
				if (tw) tw[pos] = tw_long(qs[f], d);
				pos++;
			}
		}
	}
	return pos;
}

static int build_twiddles13(float2 *tw, int *offsets /* [8] or NULL */)
{
	const int n = 8192;
	int pos = 0, q = 0;
	if (offsets) offsets[q] = pos;
	q++;
	for (int m = 1; m <= 3; m++) {
		if (tw) tw[pos] = tw_long(m, 8);
		pos++;
	}
	for (int p = 16; p <= 256; p *= 16, q++) {
		if (offsets) offsets[q] = pos;
		const int d = 8 * p;
		for (int k = 0; k < p; k++) {
			const int qs[8] = { 8 * k, 4 * k, 2 * k, 2 * k + 2 * p, k, k + p, k + 2 * p, k + 3 * p };
			for (int f = 0; f < 8; f++) {
				if (tw) tw[pos] = tw_long(qs[f], d);
				pos++;
			}
		}
	}
	if (offsets) offsets[q] = pos;
	for (int k = 0; k < n / 2; k++) {
		if (tw) tw[pos] = tw_long(k, n / 2);
		pos++;
	}
	return pos;
}

static int build_twiddles(float2 *tw, int log2n, int *offsets /* [8] or NULL */)
{
	const float PI_F = 3.141592653589f;		/* fft.cl:26 */
	const int n = 1 << log2n;
	int pos = 0, q = 0;
	if (log2n == 16)
		return build_twiddles16(tw, offsets);
	if (log2n == 13)
		return build_twiddles13(tw, offsets);
	for (int p = 8; p < n / 2; p *= 8, q++) {
		if (offsets) offsets[q] = pos;
		for (int k = 0; k < p; k++) {
			const float alpha = -PI_F * (float)k / (float)(4 * p);
			for (int f = 1; f < 8; f++) {
				const float arg = (float)f * alpha;
				if (tw) tw[pos] = make_float2(fpm_cosf(arg), fpm_sinf(arg));
				pos++;
			}
		}
	}
	if (offsets) offsets[q] = pos;
	for (int k = 0; k < n / 2; k++) {
		const float alpha = -PI_F * (float)k / (float)(n / 2);
		const float arg = (float)1 * alpha;
		if (tw) tw[pos] = make_float2(fpm_cosf(arg), fpm_sinf(arg));
		pos++;
	}
	return pos;
}

/* Exact bin thresholds on the double squared magnitude: thr[b] = smallest s >= 0 with
 * oracle bin(s) >= b.  bin(s) is monotone while hypot(s) is finite (checked exhaustively by
 * oracle/tools/pm_check.c); thr[nb] = smallest s whose hypot overflows float. */
static void build_thresholds(double *thr, int nb, float hs, float ho)
{
	/* largest s with finite (float)sqrt(s) */
	uint64_t lo = 0, hi = fpm_d2u(1.0e80);
	while (hi - lo > 1) {
		uint64_t mid = lo + (hi - lo) / 2;
		if (isinf(fpm_hypot_from_sqmag(fpm_u2d(mid)))) hi = mid; else lo = mid;
	}
	const uint64_t s_inf = hi;
	thr[0] = -1.0;
	thr[nb] = fpm_u2d(s_inf);
	for (int b = 1; b < nb; b++) {
		/* invariant: bin(lo) < b <= bin(hi) on [0, s_inf) */
		if (fpm_bin_from_sqmag(fpm_u2d(s_inf - 1), hs, ho, nb) < b) {
			thr[b] = fpm_u2d(s_inf);	/* unreachable bin */
			continue;
		}
		lo = 0; hi = s_inf - 1;
		while (hi - lo > 1) {
			uint64_t mid = lo + (hi - lo) / 2;
			if (fpm_bin_from_sqmag(fpm_u2d(mid), hs, ho, nb) >= b) hi = mid; else lo = mid;
		}
		thr[b] = fpm_u2d(hi);
	}
}

/* ------------------------------------------------------------------------ */
/* Init / release                                                           */
/* ------------------------------------------------------------------------ */

/* Events that order kernels of this device among the instance's own streams (and the timing
 * events) need no system-scope fence: a default event makes the queue write back and invalidate
 * the L2s when it is recorded, which costs microseconds between dependent kernels and sends the
 * consumer's reads to HBM.  Kernel boundaries keep their device-scope release/acquire.
 * (Events the HOST waits on for host-visible data -- staging, upload -- keep the default.) */
/* Output streams of the 65536-point kernel (waterfall rows, bin indices) live in UNCACHED device memory: its clusters keep their
 * intermediate in the XCD's L2 and every byte streamed through that L2 pushes intermediate lines out, to be written back to HBM although
 * they are dead.  Uncached stores go past the L2: WRITE_SIZE per 1024-spectrum frame 649 -> 541 MiB at the same kernel time (DESIGN.md
 * section 8; A/B'd in round 4 through an environment switch that has since gone).  The other configurations have no such hot set and keep plain memory (the 8192-point
 * kernel's index stores run 6 % slower uncached). */
static hipError_t alloc_output(void **p, size_t bytes, bool uncached)
{
	if (uncached && hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached) == hipSuccess)
		return hipSuccess;
	return hipMalloc(p, bytes);
}

static unsigned dep_event_flags(void)
{
	/* (no system fence: the events order kernels of this device among its own streams, nothing the host or another device reads) */
	return hipEventDisableTiming | hipEventDisableSystemFence;
}

extern "C" const char *fosphor_amd_version(void) { return FOSPHOR_AMD_VERSION; }

extern "C" void fosphor_release(struct fosphor *self)
{
	if (!self)
		return;
	if (self->stream)
		(void)hipStreamSynchronize(self->stream);
	(void)hipFree(self->d_win); (void)hipFree(self->d_tw); (void)hipFree(self->d_thr);
	(void)hipFree(self->d_wf_pp[0]); (void)hipFree(self->d_wf_pp[1]);
	(void)hipFree(self->d_hist); (void)hipFree(self->d_spectrum);
	for (int i = 1; i < kMaxK1Streams; i++)
		if (self->k1_streams[i]) { (void)hipStreamSynchronize(self->k1_streams[i]); (void)hipStreamDestroy(self->k1_streams[i]); }
	for (int i = 0; i < kSets; i++) {
		(void)hipFree(self->d_bins_pp[i]); (void)hipFree(self->d_partial_pp[i]);
	}
	if (self->copy_stream) { (void)hipStreamSynchronize(self->copy_stream); (void)hipStreamDestroy(self->copy_stream); }
	if (self->stream2) { (void)hipStreamSynchronize(self->stream2); (void)hipStreamDestroy(self->stream2); }
	if (self->stream3) { (void)hipStreamSynchronize(self->stream3); (void)hipStreamDestroy(self->stream3); }
	for (Fence *f = (Fence *)&self->f; f < (Fence *)&self->f + kFences; f++)
		if (f->ev) (void)hipEventDestroy(f->ev);
	(void)hipFree(self->d_hc); (void)hipFree(self->d_hc_export); (void)hipFree(self->d_slab16);
	(void)hipFree(self->d_rowmask); (void)hipFree(self->d_hot); (void)hipFree(self->d_rowlist);
	(void)hipFree(self->d_live_sum); (void)hipFree(self->d_vmax);
	(void)hipFree(self->d_chunk_sum); (void)hipFree(self->d_chunk_max);
	(void)hipFree(self->d_rise);
	(void)hipFree(self->d_palette);
	for (int i = 0; i < FOSPHOR_SCRATCH_COUNT; i++)
		(void)hipFree(self->scratch[i].d);
	(void)hipFree(self->wire.d_masks); (void)hipFree(self->wire.d_union); (void)hipFree(self->wire.d_prefix);
	(void)hipFree(self->wire.d_live); (void)hipFree(self->wire.d_words);
	if (self->wire.h_live) (void)hipHostFree(self->wire.h_live);
	for (hipEvent_t e : self->wire.ev)
		if (e) (void)hipEventDestroy(e);
	(void)hipFree(self->d_scratch);
	(void)hipFree(self->d_k1h_sync);
	if (self->h_k1h_err) (void)hipHostFree(self->h_k1h_err);
	(void)hipFree(self->d_dbg);
	if (self->h_rise) (void)hipHostFree(self->h_rise);
	for (int i = 0; i < 2; i++) {
		if (self->h_stage[i]) (void)hipHostFree(self->h_stage[i]);
		if (self->d_stage[i]) (void)hipFree(self->d_stage[i]);
	}
	if (self->h_thr) (void)hipHostFree(self->h_thr);
	if (self->h_win) (void)hipHostFree(self->h_win);
	for (hipEvent_t e : self->ev_pool) (void)hipEventDestroy(e);
	for (hipEvent_t e : self->xev_pool) (void)hipEventDestroy(e);
	if (self->own_stream && self->stream)
		(void)hipStreamDestroy(self->stream);
	delete self;
}

extern "C" struct fosphor *fosphor_amd_init(const struct fosphor_amd_config *cfg)
{
	struct fosphor *self = new (std::nothrow) fosphor();
	int ndev = 0;
	size_t tiles_max;
	std::vector<float2> tw;

	if (!self)
		return NULL;

	self->log2n   = (cfg && cfg->fft_len_log > 0) ? cfg->fft_len_log : kLog2N;
	self->n       = 1 << self->log2n;
	self->n_bins  = (cfg && cfg->n_bins > 0) ? cfg->n_bins : 128;
	self->wf_rows = (cfg && cfg->wf_rows > 0) ? cfg->wf_rows : 1024;
	self->t0r     = (cfg && cfg->t0r > 0.0f) ? cfg->t0r : 16.0f;		/* cl.c:714 */
	self->t0d     = (cfg && cfg->t0d > 0.0f) ? cfg->t0d : 1024.0f;		/* cl.c:715 */
	self->alpha   = (cfg && cfg->alpha > 0.0f) ? cfg->alpha : 0.002f;	/* cl.c:716 */
	self->max_spectra = (cfg && cfg->max_spectra > 0) ? cfg->max_spectra : 1024;
	self->max_batches = (cfg && cfg->max_batches > 0) ? cfg->max_batches
	                    : (self->max_spectra / 1024 > 8 ? self->max_spectra / 1024 : 8);

	self->wire.live_rows = -1;
	self->wire.stats[FOSPHOR_AMD_WIRE_LAST_LIVE_ROWS] = -1;

	if (self->log2n != 10 && self->log2n != 13 && self->log2n != 16) {
		fprintf(stderr, "[!] fosphor_amd: fft_len_log=%d not supported (10, 13 or 16)\n", self->log2n);
		goto error;
	}
	self->iq_format = cfg ? cfg->iq_format : FOSPHOR_AMD_IQ_FP32;
	if (self->iq_format != FOSPHOR_AMD_IQ_FP32 && self->iq_format != FOSPHOR_AMD_IQ_FP16 && self->iq_format != FOSPHOR_AMD_IQ_SC16) {
		fprintf(stderr, "[!] fosphor_amd: iq_format=%d unknown\n", self->iq_format);
		goto error;
	}
	self->sample_bytes = self->iq_format == FOSPHOR_AMD_IQ_FP32 ? sizeof(float2) : 4;
	if (self->iq_format == FOSPHOR_AMD_IQ_FP16 && self->log2n != 16) {
		fprintf(stderr, "[!] fosphor_amd: fp16 IQ is only implemented for fft_len_log=16\n");
		goto error;
	}
	if (self->n_bins < 16 || self->n_bins > 512 || (self->n_bins & 15)) {
		fprintf(stderr, "[!] fosphor_amd: n_bins=%d not supported (16..512, multiple of 16)\n", self->n_bins);
		goto error;
	}
	/* 8-bit bin indices (4 spectra per dword) need n_bins <= 256 and the 1024-point kernels */
	self->bins16 = (self->n_bins > 256) || (self->log2n != 10);
	if (self->wf_rows & (self->wf_rows - 1)) {
		fprintf(stderr, "[!] fosphor_amd: wf_rows=%d is not a power of two\n", self->wf_rows);
		goto error;
	}
	if (self->max_spectra & 15) {
		fprintf(stderr, "[!] fosphor_amd: max_spectra=%d is not a multiple of 16\n", self->max_spectra);
		goto error;
	}

	{
		hipError_t e = hipGetDeviceCount(&ndev);
		if (e != hipSuccess || ndev < 1) {
			fprintf(stderr, "[!] fosphor_amd: no HIP device available (%s, %d devices); this library has no CPU path\n",
			        hipGetErrorString(e), ndev);
			goto error;
		}
	}
	if (cfg && cfg->device >= 0) {
		HIP_TRY(hipSetDevice(cfg->device), "hipSetDevice");
		self->device = cfg->device;
	} else {
		HIP_TRY(hipGetDevice(&self->device), "hipGetDevice");
	}
	{
		hipDeviceProp_t prop;
		HIP_TRY(hipGetDeviceProperties(&prop, self->device), "hipGetDeviceProperties");
		self->n_cus = prop.multiProcessorCount;
		/* space sharing is laid out for the whole MI355X (256 CUs: 224 + 32); any other CU count -- a partitioned part -- runs
		 * every launch in the full-chip form */
		self->share_cus = (self->n_cus == 256) ? kK1wShareCus : 0;
	}
	{
		const char *e;
		e = getenv("FOSPHOR_AMD_TILE");        self->kn_tile = e ? atoi(e) : 0;
		e = getenv("FOSPHOR_AMD_ROWMASK");     self->kn_rowmask_off = (e && *e == '0');
		self->kn_no_sum16 = getenv("FOSPHOR_AMD_NO_SUM16") != NULL;
		e = getenv("FOSPHOR_AMD_FRAME_GROUP"); self->kn_frame_group = e ? atoi(e) : 4;
		e = getenv("FOSPHOR_AMD_K1W_SHARE");   self->kn_k1w_share_off = (e && *e == '0');
	}

	if (cfg && cfg->stream) {
		self->stream = (hipStream_t)cfg->stream;
	} else {
		HIP_TRY(hipStreamCreateWithFlags(&self->stream, hipStreamNonBlocking), "hipStreamCreate");
		self->own_stream = 1;
	}

	tiles_max = (size_t)self->max_spectra / 4;
	HIP_TRY(hipMalloc((void **)&self->d_win, sizeof(float) * self->n), "alloc window");
	self->tw_len = build_twiddles(NULL, self->log2n, NULL);
	HIP_TRY(hipMalloc((void **)&self->d_tw, sizeof(float2) * self->tw_len), "alloc twiddles");
	HIP_TRY(hipMalloc((void **)&self->d_thr, sizeof(double) * (self->n_bins + 1)), "alloc thresholds");
	for (int i = 0; i < 2; i++) {
		HIP_TRY(alloc_output((void **)&self->d_wf_pp[i], sizeof(float) * (size_t)self->wf_rows * self->n, self->log2n == 16), "alloc waterfall");
	}
	for (Fence *f = (Fence *)&self->f; f < (Fence *)&self->f + kInitFences; f++)
		HIP_TRY(f->create(dep_event_flags()), "create event");
	/* Only the streams in use are created: the runtime spreads streams over a few hardware queues (4 unless
	 * GPU_MAX_HW_QUEUES says otherwise) and two streams that share one do not overlap. */
	{
		const char *e = getenv("FOSPHOR_AMD_K1_STREAMS");
		self->n_k1_streams = (e && atoi(e) >= 1 && atoi(e) <= kMaxK1Streams) ? atoi(e) : 2;
	}
	self->k1_streams[0] = self->stream;
	for (int i = 1; i < self->n_k1_streams; i++) {
		HIP_TRY(hipStreamCreateWithFlags(&self->k1_streams[i], hipStreamNonBlocking), "hipStreamCreate (FFT stream)");
		HIP_TRY(self->f.k1s_done[i].create(dep_event_flags()), "create event");
	}
	HIP_TRY(hipMalloc((void **)&self->d_hist, sizeof(float) * (size_t)self->n_bins * self->n), "alloc histogram");
	HIP_TRY(hipMalloc((void **)&self->d_spectrum, sizeof(float2) * 2 * self->n), "alloc spectrum");
	for (int i = 0; i < kSets; i++) {
		HIP_TRY(alloc_output((void **)&self->d_bins_pp[i], (size_t)self->max_spectra * self->n * (self->bins16 ? 2 : 1), self->log2n == 16), "alloc bin indices");
		HIP_TRY(hipMalloc((void **)&self->d_partial_pp[i], sizeof(float2) * tiles_max * self->n), "alloc partials");
	}
	self->d_bins = self->d_bins_pp[0];
	self->d_partial = self->d_partial_pp[0];
	if (self->log2n == 16) {
		/* One FFT kernel takes a spectrum through both 256-point levels of the radix-16 plan, the intermediate staying in the
		 * XCD's L2 (DESIGN.md sections 4-5; DESIGN_HISTORY.md section 8; the two-kernel form of rounds 1-3 went with the radix-8 plan in round 4). */
		/* 512 KiB of intermediate per cluster, at most 8 clusters on each of the 8 XCDs */
		HIP_TRY(hipMalloc((void **)&self->d_scratch, sizeof(float2) * (size_t)64 * self->n), "alloc cluster intermediates");
		HIP_TRY(hipMalloc((void **)&self->d_k1h_sync, sizeof(uint32_t) * 64 * 64), "alloc cluster counters");
		HIP_TRY(hipMemset(self->d_k1h_sync, 0, sizeof(uint32_t) * 64 * 64), "clear cluster counters");
		HIP_TRY(hipHostMalloc((void **)&self->h_k1h_err, 64, hipHostMallocMapped), "alloc error word");
		self->h_k1h_err[0] = 0;
	}
	/* host staging slot: the reference's cap of 1024 spectra per call (cl.c:885), or this instance's */
	self->stage_samples = (size_t)self->n * (self->max_spectra < 1024 ? self->max_spectra : 1024);
	HIP_TRY(hipStreamCreateWithFlags(&self->stream2, hipStreamNonBlocking), "hipStreamCreate (count stream)");
	HIP_TRY(hipStreamCreateWithFlags(&self->stream3, hipStreamNonBlocking), "hipStreamCreate (merge stream)");
	if (getenv("FOSPHOR_AMD_K1_TIMING")) {
		HIP_TRY(hipMalloc((void **)&self->d_dbg, sizeof(long long) * 16 * 4 * kK1MaxBlocks), "alloc timing buffer");
		HIP_TRY(hipMemset(self->d_dbg, 0, sizeof(long long) * 16 * 4 * kK1MaxBlocks), "clear timing buffer");
	}
	{
		const char *e = getenv("FOSPHOR_AMD_OVERLAP");
		self->overlap = !(e && *e == '0');
		/* The fused 65536-point kernel fills every CU.  Rounds 2-3 therefore ran FFT -> count -> scan -> merge one after the other on
		 * ONE stream (then 134-136 -> 142-144 GSamples/s: the radix-8 kernel of 16 waves and 134 KiB of LDS crawled when count / merge
		 * work-groups reached the CUs first).  The radix-16 kernel of round 4 (8 waves) does not: with the streams, count on the
		 * second and merge on the third, the tail of frame f runs in the gaps of frame f + 1's FFT kernel -- its ramp-up, and the
		 * CUs its clusters leave as the tiles run out: 215.3 -> 229.5 GSamples/s (four interleaved runs each; two streams 224.5;
		 * with the FFT kernel made to wait for the previous merge 199.7).  FOSPHOR_AMD_OVERLAP=0: one stream. */
		/* N = 8192: the FFT kernel owns every CU's LDS and registers, so count and merge cannot run beside it either way; on one
		 * stream the kernel boundaries are cheaper than cross-stream events (measured 286.6 / 287.8 / 287.1 against 286.1 / 284.7 /
		 * 283.5 GSamples/s), and K1's busy time is no longer stretched by launches waiting for each other (0.363 vs 0.29-0.345). */
		/* (round 4: the streams are back for N = 8192 -- with space sharing, kK1wShareCus, count and merge DO run beside the next FFT
		 * launch; for launch shapes that cannot share, the streams cost 0.3 %: 326 against 327 GSamples/s.  FOSPHOR_AMD_OVERLAP=0:
		 * one stream.) */
		e = getenv("FOSPHOR_AMD_K1");
		self->k1_variant = (e && *e == '2') ? 2 : 1;
		e = getenv("FOSPHOR_AMD_PIPE3");
		self->pipe3 = e ? (*e == '1') : (self->log2n == 16);	/* (N = 65536: merge on its own stream, above) */
		e = getenv("FOSPHOR_AMD_ALT");
		self->alt = !(e && *e == '0');
		self->n_sets = 3;		/* (of kSets allocated: more in rotation measured nothing) */
		if (self->log2n == 13 && !getenv("FOSPHOR_AMD_K1_STREAMS"))
			self->n_k1_streams = 1;		/* a second FFT launch in flight would take the CUs left to count / merge */
		if (self->n_k1_streams == 1)
			self->alt = 0;
		e = getenv("FOSPHOR_AMD_SUB_LOG2");		/* tuning: log2 of the samples per sub-launch */
		/* (N = 8192: the one-work-group-per-CU FFT kernel owns the whole LDS, so K2 cannot run beside it and a
		 * smaller piece only adds serialised kernel boundaries: twice the default) */
		/* (round 4, N = 8192: 1 Gi samples -- up to 32 batches of 4096 spectra in one FFT launch: with space sharing a launch boundary
		 * costs ~40 us, during which the count kernels of the finished launch and the work-groups of the next FFT launch compete for
		 * the CUs) */
		self->sub_samples = 1LL << ((e && atoi(e) >= 14 && atoi(e) <= 34) ? atoi(e) : (self->log2n == 13 ? 30 : kSubSamplesLog2));
	}
	HIP_TRY(hipMalloc((void **)&self->d_hc, sizeof(uint32_t) * (size_t)self->max_batches * self->n_bins * self->n), "alloc hit counts");
	HIP_TRY(hipMalloc((void **)&self->d_hc_export, sizeof(uint32_t) * (size_t)self->n_bins * self->n), "alloc hit count view");
	self->mask_words = (self->n_bins + 31) / 32;
	HIP_TRY(hipMalloc((void **)&self->d_rowmask, sizeof(uint32_t) * 2 * (size_t)self->max_batches * (self->n / 64) * self->mask_words), "alloc row masks");
	HIP_TRY(hipMalloc((void **)&self->d_hot, (size_t)(self->n / 64) * self->n_bins), "alloc row flags");
	HIP_TRY(hipMemset(self->d_hot, 1, (size_t)(self->n / 64) * self->n_bins), "set row flags");
	HIP_TRY(hipMalloc((void **)&self->d_rowlist, sizeof(uint32_t) * (2 + (size_t)(self->n / 64) * self->n_bins)), "alloc row list");
	HIP_TRY(hipMemset(self->d_rowlist, 0, sizeof(uint32_t) * (2 + (size_t)(self->n / 64) * self->n_bins)), "clear row list");
	self->rowlist_flip = 0;
	self->hot_valid = 0;
	self->hc_view = self->d_hc;
	if (self->max_spectra > 1024) {
		/* one slab per 1024-spectrum chunk of the largest launch: a whole shard (accumulate) or a sub-launch */
		self->slab_chunks = self->max_spectra / 1024;
		HIP_TRY(hipMalloc((void **)&self->d_slab16, sizeof(uint16_t) * (size_t)self->slab_chunks * self->n_bins * self->n), "alloc count slabs");
	}
	/* two sets of max_batches slots (the 16-bit hit counts of the second set use the upper half of d_hc) */
	HIP_TRY(hipMalloc((void **)&self->d_live_sum, sizeof(float) * 2 * (size_t)self->max_batches * self->n), "alloc live sums");
	HIP_TRY(hipMalloc((void **)&self->d_vmax, sizeof(float) * 2 * (size_t)self->max_batches * self->n), "alloc max");
	HIP_TRY(hipMalloc((void **)&self->d_chunk_sum, sizeof(float) * (size_t)(self->max_spectra / 16) * self->n), "alloc chunk sums");
	HIP_TRY(hipMalloc((void **)&self->d_chunk_max, sizeof(float) * (size_t)(self->max_spectra / 16) * self->n), "alloc chunk max");
	HIP_TRY(hipMalloc((void **)&self->d_rise, sizeof(float2) * (kRiseMax + 1)), "alloc rise table");
	HIP_TRY(hipHostMalloc((void **)&self->h_rise, sizeof(float2) * (kRiseMax + 1), hipHostMallocDefault), "alloc pinned rise table");
	HIP_TRY(hipHostMalloc((void **)&self->h_thr, sizeof(double) * (self->n_bins + 1), hipHostMallocDefault), "alloc pinned thr");
	HIP_TRY(hipHostMalloc((void **)&self->h_win, sizeof(float) * self->n, hipHostMallocDefault), "alloc pinned win");

	tw.resize(self->tw_len);
	build_twiddles(tw.data(), self->log2n, self->tw_off);
	HIP_TRY(hipMemcpy(self->d_tw, tw.data(), sizeof(float2) * self->tw_len, hipMemcpyHostToDevice), "upload twiddles");

	/* Initial state (fosphor.c:64-66) */
	fosphor_set_fft_window_default(self);
	fosphor_set_power_range(self, 0, 10);
	self->state = ST_BOOTING;
	return self;

error:
	fosphor_release(self);
	return NULL;
}

extern "C" struct fosphor *fosphor_init(void)
{
	return fosphor_amd_init(NULL);
}

/* ------------------------------------------------------------------------ */
/* Settings                                                                 */
/* ------------------------------------------------------------------------ */

extern "C" void fosphor_set_fft_window_default(struct fosphor *self)
{
	/* periodic Hamming x 1.855, fosphor.c:113-118 */
	for (int i = 0; i < self->n; i++) {
		float ft = (float)self->n;
		float fp = (float)i;
		self->fft_win[i] = (0.54f - 0.46f * cosf((2.0f * 3.141592f * fp) / ft)) * 1.855f;
	}
	self->win_dirty = 1;
}

extern "C" void fosphor_set_fft_window(struct fosphor *self, float *win)
{
	memcpy(self->fft_win, win, sizeof(float) * self->n);		/* fosphor.c:123-128 */
	self->win_dirty = 1;
}

extern "C" void fosphor_set_power_range(struct fosphor *self, int db_ref, int db_per_div)
{
	/* fosphor.c:131-152 */
	int db0 = db_ref - 10 * db_per_div;
	int db1 = db_ref;
	float k = fpm_log10f((float)self->n);
	float offset = -(k + ((float)db0 / 20.0f));
	float scale  = 20.0f / (float)(db1 - db0);

	self->power.db_ref = db_ref;
	self->power.db_per_div = db_per_div;
	self->power.scale = scale;
	self->power.offset = offset;

	/* cl.c:1081-1089, with the bin count a parameter instead of 128 */
	self->histo_scale  = scale * (float)self->n_bins;
	self->histo_offset = offset;
	self->thr_dirty = 1;
}

extern "C" void fosphor_set_frequency_range(struct fosphor *self, double center, double span)
{
	self->frequency.center = center;	/* fosphor.c:154-160 */
	self->frequency.span   = span;
}

/* ------------------------------------------------------------------------ */
/* Launch sequence                                                          */
/* ------------------------------------------------------------------------ */

static void prof_begin(struct fosphor *self, int kind, hipStream_t st)
{
	self->prof_open = 0;
	if (!self->prof || (self->prof == 2 && kind != 0)) return;
	if (self->ev_used + 2 > self->ev_pool.size()) {
		for (int i = 0; i < 2; i++) {
			hipEvent_t e;
			if (hipEventCreateWithFlags(&e, dep_event_flags() & ~hipEventDisableTiming) != hipSuccess) return;
			self->ev_pool.push_back(e);
		}
	}
	if (hipEventRecord(self->ev_pool[self->ev_used], st) != hipSuccess)
		return;				/* this launch goes untimed */
	self->prof_open = 1;
	self->ev_kind.push_back(kind);
}

static void prof_end(struct fosphor *self, hipStream_t st)
{
	if (!self->prof_open) return;
	self->prof_open = 0;
	if (self->ev_used + 2 > self->ev_pool.size() || hipEventRecord(self->ev_pool[self->ev_used + 1], st) != hipSuccess) {
		self->ev_kind.pop_back();	/* drop the half-recorded pair */
		return;
	}
	self->ev_used += 2;
}

/* The stream K2 / K3 and the exchanges run on: a second stream when the two-stream pipeline is on, else the main one */
static hipStream_t count_stream(const struct fosphor *self)
{
	return self->overlap ? self->stream2 : self->stream;
}

static int sync_all(struct fosphor *self)
{
	int rv = 0;
	if (self->stream  && hipStreamSynchronize(self->stream)  != hipSuccess) rv = -EIO;
	for (int i = 1; i < kMaxK1Streams; i++)
		if (self->k1_streams[i] && hipStreamSynchronize(self->k1_streams[i]) != hipSuccess) rv = -EIO;
	if (self->stream2 && hipStreamSynchronize(self->stream2) != hipSuccess) rv = -EIO;
	if (self->stream3 && hipStreamSynchronize(self->stream3) != hipSuccess) rv = -EIO;
	return rv;
}

/* K3s update the persistent state in launch order.  They normally follow each other on one
 * stream; when the stream changes (pipelined process path <-> accumulate/merge path) the new
 * stream waits for the last K3 of the old one. */
static int k3_stream_enter(struct fosphor *self, hipStream_t st)
{
	if (self->last_k3_stream && self->last_k3_stream != st) {
		if (self->f.k3_done.record(self->last_k3_stream) != hipSuccess || self->f.k3_done.wait(st) != hipSuccess)
			return -EIO;
	}
	self->last_k3_stream = st;
	return 0;
}

/* Before anything else than the pipelined 16-bit path writes d_hc / live sums: K3s still
 * reading the two hit-count sets must be done. */
static int drain_h_sets(struct fosphor *self, hipStream_t st)
{
	for (int h = 0; h < 2; h++) {
		if (self->f.h_free[h].wait(st) != hipSuccess)
			return -EIO;
		self->f.h_free[h].recorded = 0;
	}
	return 0;
}

/* Upload lazily-changed tables (cl.c:889-900) and boot fills (cl.c:406-465, 930-934) */
static int prepare(struct fosphor *self)
{
	if (self->win_dirty || self->thr_dirty) {
		/* The tables are read by every K1 still queued -- with relaxed input ordering those of the previous call may be
		 * running on the other FFT streams, which `stream` does not wait for -- and the pinned staging copies (h_win,
		 * h_thr) may still be in flight: drain all FFT streams before either is rewritten. */
		for (int i = 0; i < self->n_k1_streams; i++)
			HIP_TRY(hipStreamSynchronize(self->k1_streams[i]), "drain FFT streams before a table upload");
	}
	if (self->win_dirty) {
		memcpy(self->h_win, self->fft_win, sizeof(float) * self->n);
		HIP_TRY(hipMemcpyAsync(self->d_win, self->h_win, sizeof(float) * self->n, hipMemcpyHostToDevice, self->stream), "upload window");
		self->win_dirty = 0;
	}
	if (self->thr_dirty) {
		build_thresholds(self->h_thr, self->n_bins, self->histo_scale, self->histo_offset);
		HIP_TRY(hipMemcpyAsync(self->d_thr, self->h_thr, sizeof(double) * (self->n_bins + 1), hipMemcpyHostToDevice, self->stream), "upload thresholds");
		self->thr_dirty = 0;
	}
	if (self->state == ST_BOOTING) {
		const float noise_floor = -self->power.offset;
		HIP_TRY(launch_fill((float *)self->d_spectrum, noise_floor, (size_t)4 * self->n, self->stream), "fill spectrum");
		for (int i = 0; i < 2; i++)
			HIP_TRY(launch_fill(self->d_wf_pp[i], noise_floor, (size_t)self->wf_rows * self->n, self->stream), "fill waterfall");
		HIP_TRY(launch_fill(self->d_hist, 0.0f, (size_t)self->n_bins * self->n, self->stream), "fill histogram");
	}
	return 0;
error:
	return -EIO;
}

/* The FFT launch of `total` spectra in batches of `batch` on this instance, as k1_plan (fosphor_kernels.hip) lays it out: hop 0 = the
 * FFT length; tile 0 = the plan's own choice */
static K1Shape k1_shape(const struct fosphor *self, const void *d_iq, int hop, int total, int batch, int tile)
{
	K1Shape s = {};
	s.log2n = self->log2n; s.n_bins = self->n_bins; s.iq_format = self->iq_format;
	s.hop = hop ? hop : self->n;
	s.align = (int)((uintptr_t)d_iq & 15);
	s.tile_knob = self->kn_tile; s.k1_knob = self->k1_variant;
	s.n_cus = self->n_cus;
	s.total = total; s.batch = batch; s.tile = tile;
	return s;
}

/* Spectra per tile of an FFT launch (the rule is k1_plan's; the tile depends on neither the hop nor the sample pointer) */
static int pick_tile(const struct fosphor *self, int total, int batch)
{
	assert(self->log2n != 13 || batch % 16 == 0);	/* (every entry point asks for it: the fallback tile of 8 divides the batch) */
	return k1_plan(k1_shape(self, NULL, 0, total, batch, 0)).tile;
}

static void fill_k1(struct fosphor *self, K1Params *k1, const void *d_iq, int total, int tile,
                    int wf_pos0, int wf_first, int hop = 0)
{
	const double A = (double)self->histo_scale * 0.150514997831990597606869447362;
	const double C = (double)self->histo_scale * (double)self->histo_offset;
	/* |v_fast - v_pinned| bound, DESIGN.md section 2.3.  Part that does not scale with
	 * |l2|: the float roundings of v itself and of the pinned chain (v < 256: <= 3e-5) plus
	 * histo_scale x (pwr, pwr+offset roundings + the mult by log10(2)/2: <= 8e-7), doubled.
	 * Part proportional to |l2| = |log2 s|: v_log_f32 (<= 1 ulp of l2) and the rounding of
	 * s32 (<= 1.5 ulp of s -> 2.2e-7 in l2, absorbed for |l2| >= 1 ... and by delta0 below
	 * that), through the slope A: kappa = 2 x A x 2^-23. */
	const float delta0 = 6.0e-5f + 2.0e-6f * self->histo_scale;
	const float kappa = (float)(2.0 * A * 1.1920928955078125e-07);

	memset(k1, 0, sizeof(*k1));
	k1->iq = (const float2 *)d_iq;
	k1->hop = hop ? hop : self->n;
	k1->n = self->n; k1->log2n = self->log2n; k1->bins16 = self->bins16;
	for (int q = 0; q < 8; q++) k1->tw_off[q] = self->tw_off[q];
	k1->win = self->d_win;
	k1->tw = self->d_tw;
	k1->thr = self->d_thr;
	k1->bins = self->d_bins;
	k1->partial = self->d_partial;
	k1->wf = self->d_wf_pp[self->wf_cur];
	k1->fft_out = NULL;
	k1->dbg = self->d_dbg;
	k1->total = total;
	k1->tile = tile;
	k1->wf_pos0 = wf_pos0;
	k1->wf_mask = self->wf_rows - 1;
	k1->wf_first = wf_first;
	k1->n_bins = self->n_bins;
	k1->binA = (float)A;
	k1->binC = (float)C;
	k1->amb = 0.5f - delta0;
	k1->kappa = kappa;
	k1->w = 1.0f - self->alpha;		/* display.cl:99 */
	/* (the two-wave kernel where FOSPHOR_AMD_K1 asks for it, and where the wave-per-spectrum kernel cannot load: odd hops, sc16 on a
	 * start that is not 8-byte aligned) */
	k1->variant = k1_variant_of(k1_plan(k1_shape(self, d_iq, hop, total, total, tile)).kernel);
	k1->scratch = self->d_scratch;
	k1->sync = (self->log2n == 16) ? self->d_k1h_sync : NULL;
	k1->sync_err = self->h_k1h_err;
	k1->iq_format = self->iq_format;
	k1->n_cus = self->n_cus;
	{
		const int sc = self->share_cus;
		k1->cus = (self->log2n == 13 && self->overlap && !self->kn_k1w_share_off && sc > 0 && tile > 0 && (total / tile) % sc == 0) ? sc : 0;
		/* ... when there is a tail to share with: the count / merge kernels of the launch before this one are still queued or running
		 * (calls issued back to back).  A launch that finds the chip idle takes all of it.  (The choice depends on timing; the results
		 * do not: the tile loop is grid-stride.  fosphor_amd_share_stats reports how many launches took which form.) */
		if (k1->cus && !(self->f.tail.recorded && hipEventQuery(self->f.tail.ev) == hipErrorNotReady))
			k1->cus = 0;
	}
}

static int gcd_int(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

/* Batches per sub-launch ("piece") of a device-resident call of n_batches batches: about sub_samples samples each, pieces of equal
 * size.  N = 8192 with the streams on: pieces of whole `unit`s of batches where the call allows it, so that every piece's tiles are a
 * multiple of kK1wShareCus and the FFT launch can leave CUs to the count / merge kernels (tiles are 64 spectra or the batch:
 * pick_tile).  Pure host arithmetic, exported for the CPU test suite (include/fosphor_amd.h). */
extern "C" int fosphor_amd_plan_piece_batches(int log2n, int overlap, int n_batches, int batch, long long sub_samples)
{
	if (n_batches < 1 || batch < 1 || log2n < 1 || log2n > 30 || sub_samples < 1)
		return -EINVAL;
	const long long per_batch = (long long)batch << log2n;
	const int cap = (int)(sub_samples / per_batch < 1 ? 1 : (sub_samples / per_batch > n_batches ? n_batches : sub_samples / per_batch));
	const int n_sub = (n_batches + cap - 1) / cap;
	int sub_b = (n_batches + n_sub - 1) / n_sub;
	if (log2n == 13 && overlap && n_sub > 1) {
		const int tpb = batch >= 64 ? batch / 64 : 1;
		const int unit = kK1wShareCus / gcd_int(kK1wShareCus, tpb);
		if (n_batches % unit == 0 && cap >= unit)
			sub_b = cap / unit * unit;
	}
	return sub_b;
}

/* The count hand-off of one launch: which buffer the count kernel fills and the merge kernel reads, for n_batches batches of
 * `batch` spectra on an instance of 2^log2n columns, n_bins bins and room for slab_chunks 1024-spectrum count slabs.  pipelined: the
 * process paths (run()), whose launches hand 16-bit counts from kernel to kernel where they can; else the partial arrays of
 * accumulate / merge, 32-bit because they are exchanged.  Every launch site takes its decisions from here and nowhere else.  Pure
 * host arithmetic, exported for the CPU test suite as fosphor_amd_plan_count (include/fosphor_amd.h). */
static struct fosphor_amd_count_plan plan_count(int log2n, int n_bins, int slab_chunks, int rowmask_off, int no_sum16,
                                                int n_batches, int batch, int pipelined)
{
	struct fosphor_amd_count_plan p;
	const int n = 1 << log2n;
	/* the rise/decay table serves batches up to kRiseMax (K3's 16-bit path needs it) */
	p.table = batch <= kRiseMax;
	/* A batch longer than 1024 spectra is counted as ONE chunk where that still gives the chip enough work-groups
	 * (N/64 slabs per batch) and the (d, e) table covers it: the 16-bit packed counters hold up to 65535 spectra, and K3
	 * then reads slab-major 16-bit counts (0.5 B per cell) instead of 32-bit sums of per-chunk slabs. */
	const int count_one_chunk = pipelined && batch > 1024 && p.table && (n / 64) * n_batches >= 128;
	const int direct16 = pipelined && (batch <= 1024 || count_one_chunk);
	p.chunk = (batch <= 1024 || count_one_chunk) ? batch : gcd_int(batch, 1024);
	p.cpb = batch / p.chunk;
	/* Batches of several 1024-spectrum chunks (a batch longer than the reference's cap, or the time shard of
	 * a display frame): K2 leaves per-chunk packed 16-bit slabs in d_slab16 (no zeroing, no global atomics)
	 * and k2c_sum adds each batch's slabs into its 32-bit array.  Needs whole chunks and room for the slabs. */
	const int sum16 = p.chunk == 1024 && p.cpb > 1 && n_batches * p.cpb <= slab_chunks && !no_sum16;
	p.handoff = direct16 ? FOSPHOR_AMD_COUNT_DIRECT16 : sum16 ? FOSPHOR_AMD_COUNT_SUM16 : FOSPHOR_AMD_COUNT_32;
	/* only batches up to the reference's cap alternate between two sets of 16-bit counts (the merge of one launch beside the count of the next) */
	p.two_sets = direct16 && !count_one_chunk;
	/* Sparse K2 -> K3 hand-off (row masks + hot flags) for the large state of N = 65536 (128 MiB, one batch = one frame: +10 % for
	 * the path).  At N = 1024 / 8192 it measured slower (K3 there is bound by its dependent chain over the batches of a launch,
	 * not by the rows it touches: -1 % / -2.5 %) and is not offered.  FOSPHOR_AMD_ROWMASK=0 selects the dense form at N = 65536
	 * (the tests run both). */
	p.rowmask = direct16 && log2n == 16 && !rowmask_off;
	const K3Shape shape = { direct16 != 0, p.rowmask != 0, p.table != 0, n_batches, batch, n_bins, n };
	p.merge_form = k3_form(shape);
	p.table_in_memory = p.merge_form == K3_SPARSE16_LONG ||
	                    ((p.merge_form == K3_DENSE16_LONG4 || p.merge_form == K3_DENSE16_LONG) && batch >= kK3RiseLdsLong);
	return p;
}

extern "C" int fosphor_amd_plan_count(int log2n, int n_bins, int slab_chunks, int rowmask_off, int no_sum16,
                                      int n_batches, int batch, int pipelined, struct fosphor_amd_count_plan *out)
{
	if (!out || n_batches < 1 || batch < 1 || log2n < 1 || log2n > 30 || n_bins < 1 || slab_chunks < 0)
		return -EINVAL;
	*out = plan_count(log2n, n_bins, slab_chunks, rowmask_off != 0, no_sum16 != 0, n_batches, batch, pipelined != 0);
	return 0;
}

/* The FFT launch of one piece, exported for the CPU test suite (include/fosphor_amd.h): k1_plan, which pick_tile, fill_k1 and the
 * launch itself take their values from, for a launch that finds the chip idle (the full-chip form at N = 8192). */
extern "C" int fosphor_amd_plan_k1(int log2n, int n_bins, int iq_format, int hop, int iq_align, int tile_knob, int k1_knob,
                                   int n_cus, int total, int batch, struct fosphor_amd_k1_plan *out)
{
	if (!out || (log2n != 10 && log2n != 13 && log2n != 16) || n_bins < 1 || n_bins > 512 || hop < 1 || iq_align < 0 || n_cus < 0 ||
	    iq_format < FOSPHOR_AMD_IQ_FP32 || iq_format > FOSPHOR_AMD_IQ_SC16 || (iq_format == FOSPHOR_AMD_IQ_FP16 && log2n != 16) ||
	    batch < 4 || total < batch || total % batch || (batch & (log2n == 13 ? 15 : 3)))
		return -EINVAL;
	static_assert(K1_WAVE == FOSPHOR_AMD_K1_WAVE && K1_V2 == FOSPHOR_AMD_K1_V2 && K1_BIG == FOSPHOR_AMD_K1_BIG &&
	              K1_WIDE == FOSPHOR_AMD_K1_WIDE && K1_FUSED == FOSPHOR_AMD_K1_FUSED, "the public names of K1Kernel");
	K1Shape s = {};
	s.log2n = log2n; s.n_bins = n_bins; s.iq_format = iq_format; s.hop = hop; s.align = iq_align & 15;
	s.tile_knob = tile_knob; s.k1_knob = k1_knob == 2 ? 2 : 1;
	s.n_cus = n_cus; s.total = total; s.batch = batch;
	const K1Plan pl = k1_plan(s);
	out->kernel = pl.kernel; out->tile = pl.tile; out->tiles = pl.tiles; out->units = pl.units;
	out->max_tiles = pl.max_tiles; out->min_tiles = pl.min_tiles;
	return 0;
}

/* ... of a launch of this instance */
static struct fosphor_amd_count_plan plan_count(const struct fosphor *self, int n_batches, int batch, int pipelined)
{
	return plan_count(self->log2n, self->n_bins, self->slab_chunks, self->kn_rowmask_off, self->kn_no_sum16, n_batches, batch, pipelined);
}

/* The count-kernel fields every K2 launch sets alike: `total` spectra of the current set's bin indices / tile partials in batches of
 * `batch`, counted `chunk` spectra per work-group; the first of them is spectrum t_offset of a batch of weight_batch (live-sum weights) */
static void fill_k2(const struct fosphor *self, K2Params *k2, int total, int batch, int chunk, int tile, int t_offset, int weight_batch)
{
	memset(k2, 0, sizeof(*k2));
	k2->bins = self->d_bins; k2->partial = self->d_partial;
	k2->n = self->n; k2->bins16 = self->bins16 && self->log2n != 13; k2->bins8p1 = (self->log2n == 13);
	k2->bins9 = (self->log2n == 16); k2->total = total;
	k2->batch = batch; k2->chunk = chunk; k2->tile = tile; k2->n_bins = self->n_bins;
	k2->w = 1.0f - self->alpha;
	k2->log2_w = (float)log2((double)(1.0f - self->alpha));
	k2->t_offset = t_offset; k2->weight_batch = weight_batch;
}

/* The per-chunk float partials of n_batches batches of cpb chunks each, reduced into live-sum / max slot lslot; sum16: the chunks'
 * 16-bit count slabs in d_slab16 added into the 32-bit hit counts of slot slot0 as well (k2c_sum) */
static hipError_t launch_chunk_sum(struct fosphor *self, int n_batches, int cpb, int slot0, int lslot, int sum16, hipStream_t st)
{
	K2bParams k2b;
	memset(&k2b, 0, sizeof(k2b));
	k2b.chunk_sum = self->d_chunk_sum; k2b.chunk_max = self->d_chunk_max;
	k2b.live_sum = self->live_sum_at(lslot);
	k2b.vmax = self->vmax_at(lslot);
	k2b.n_batches = n_batches; k2b.cpb = cpb; k2b.n = self->n;
	if (!sum16) {
		self->n_k2b++;
		return launch_k2b(k2b, st);
	}
	k2b.hc16 = self->d_slab16; k2b.hc = self->hc_slot(slot0); k2b.n_bins = self->n_bins;
	self->n_k2c++;
	return launch_k2c(k2b, st);
}

/* K2 (+K2b) for n_batches batches of `batch` spectra whose bin indices / tile partials are in
 * d_bins / d_partial, handed off as `plan` says; results land in slot `slot0`.. of hc / live_sum / vmax (pipelined launches: of
 * hit-count set hset). */
static int run_count(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int tile, int slot0,
                     int hset, int t_offset, int weight_batch, hipStream_t st)
{
	K2Params k2;
	const int cpb = plan.cpb;
	const int sum16 = plan.handoff == FOSPHOR_AMD_COUNT_SUM16;
	const int lslot = self->live_slot(slot0, hset);

	fill_k2(self, &k2, n_batches * batch, batch, plan.chunk, tile, t_offset, weight_batch);
	k2.hc = self->hc_slot(slot0);
	if (plan.handoff == FOSPHOR_AMD_COUNT_DIRECT16)
		k2.hc16 = self->hc16_set(hset);
	if (plan.rowmask) {
		k2.rowmask = self->rowmask_set(hset);
		k2.mask_words = self->mask_words;
		k2.mask_stride = self->max_batches;
	}
	if (sum16)
		k2.hc16 = self->d_slab16;
	if (cpb == 1) {
		k2.chunk_sum = self->live_sum_at(lslot);
		k2.chunk_max = self->vmax_at(lslot);
	} else {
		k2.chunk_sum = self->d_chunk_sum;
		k2.chunk_max = self->d_chunk_max;
		if (!sum16)
			HIP_TRY(hipMemsetAsync(k2.hc, 0, sizeof(uint32_t) * self->cells() * n_batches, st), "zero hit counts");
	}
	prof_begin(self, 1, st);
	HIP_TRY(launch_k2(k2, n_batches * cpb, st), "launch count");
	self->k2_stream_last = st;
	if (cpb > 1)
		HIP_TRY(launch_chunk_sum(self, n_batches, cpb, slot0, lslot, sum16, st), sum16 ? "launch chunk sum" : "launch chunk reduce");
	prof_end(self, st);
	return 0;
error:
	return -EIO;
}

/* (d, e) of display.cl:241-245 for every possible hit count of a batch.  Same float
 * expressions as the kernel source, powf from the host libm (the oracle's binding). */
static int ensure_rise_table(struct fosphor *self, int batch, hipStream_t st)
{
	if (self->rise_batch == batch && self->rise_t0r == self->t0r && self->rise_t0d == self->t0d)
		return 1;
	if (sync_all(self))				/* h_rise may be in flight */
		return -1;
	for (int hc = 0; hc <= batch; hc++) {
		const float a = (float)hc / (float)batch;
		const float b = a * (1.0f / self->t0r);
		const float c = b + (1.0f / self->t0d);
		const float d = b * (1.0f / c);
		const float e = powf(1.0f - c, (float)batch);
		self->h_rise[hc] = make_float2(d, e);
	}
	if (hipMemcpyAsync(self->d_rise, self->h_rise, sizeof(float2) * (batch + 1), hipMemcpyHostToDevice, st) != hipSuccess)
		return -1;
	self->rise_batch = batch; self->rise_t0r = self->t0r; self->rise_t0d = self->t0d;
	return 1;
}

static int run_merge(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int slot0, int hset,
                     hipStream_t st, int cell_begin = 0, int cell_end = 0)
{
	K3Params k3;
	const int lslot = self->live_slot(slot0, hset);
	if ((plan.table && ensure_rise_table(self, batch, st) < 0) || k3_stream_enter(self, st))
		return -EIO;
	memset(&k3, 0, sizeof(k3));
	k3.rise = plan.table ? self->d_rise : NULL;
	k3.live_decay = powf(1.0f - self->alpha, (float)batch);	/* display.cl:210 */
	k3.hc = self->hc_slot(slot0);
	k3.hc_export = self->d_hc_export;
	if (plan.handoff == FOSPHOR_AMD_COUNT_DIRECT16) {
		/* the uint32 view of the last batch is made when somebody asks for it (fosphor_amd_get_buffers) */
		k3.hc16 = self->hc16_set(hset);
		k3.hc_export = NULL;
		self->export_src = k3.hc16 + (size_t)(n_batches - 1) * self->cells();
		self->export_mask = NULL;
		self->export_stream = self->k2_stream_last ? self->k2_stream_last : st;
		self->hc_view = self->d_hc_export;
		if (plan.rowmask) {
			k3.rowmask = self->rowmask_set(hset);
			k3.mask_words = self->mask_words;
			k3.mask_stride = self->max_batches;
			self->export_mask = k3.rowmask + (n_batches - 1);
			k3.hot = self->d_hot;
			k3.rowlist = self->d_rowlist;
			k3.rowlist_cnt = self->rowlist_flip ? 1 + self->n_bins * (self->n / 64) : 0;
			self->k3_listed = k3.rowlist + k3.rowlist_cnt;
			self->k3_listed_stream = st;
			self->rowlist_flip ^= 1;
			k3.hot_all = !self->hot_valid;
			self->hot_valid = 1;
		} else {
			self->hot_valid = 0;
		}
	} else {
		self->export_src = NULL;
		self->hot_valid = 0;
		self->hc_view = self->hc_slot(slot0 + n_batches - 1);
	}
	k3.live_sum = self->live_sum_at(lslot);
	k3.vmax = self->vmax_at(lslot);
	k3.hist = self->d_hist; k3.spectrum = self->d_spectrum;
	k3.n_batches = n_batches; k3.batch = batch; k3.n_bins = self->n_bins; k3.n = self->n;
	k3.t0r = self->t0r; k3.t0d = self->t0d; k3.alpha = self->alpha;
	k3.cell_begin = cell_begin; k3.cell_end = cell_end;
	prof_begin(self, 2, st);
	HIP_TRY(launch_k3(k3, st), "launch merge");
	{
		const int form = plan.merge_form;	/* (what launch_k3 launched: k3_form of the buffers filled in above) */
		assert(form == k3_form(k3_shape(k3)));
		self->k3_forms[form]++;
		if (plan.table_in_memory)
			self->k3_rise_mem++;
		if ((form == K3_SPARSE16 || form == K3_SPARSE16_LONG) && n_batches > self->k3_sparse_max[form == K3_SPARSE16_LONG])
			self->k3_sparse_max[form == K3_SPARSE16_LONG] = n_batches;
	}
	prof_end(self, st);
	return 0;
error:
	return -EIO;
}

/* the other FFT streams see what the caller (and prepare()) queued on `stream` ... */
static int k1_streams_fork(struct fosphor *self)
{
	if (self->f.in.record(self->stream) != hipSuccess)
		return -EIO;
	for (int i = 1; i < self->n_k1_streams; i++)
		if (self->f.in.wait(self->k1_streams[i]) != hipSuccess)
			return -EIO;
	return 0;
}

/* ... and what the caller queues on `stream` next follows every K1 queued on them */
static int k1_streams_join(struct fosphor *self)
{
	for (int i = 1; i < self->n_k1_streams; i++)
		if (self->f.k1s_done[i].record(self->k1_streams[i]) != hipSuccess || self->f.k1s_done[i].wait(self->stream) != hipSuccess)
			return -EIO;
	return 0;
}

/* One FFT launch ("piece") of sub_total spectra from d_iq on FFT stream ks; its first spectrum is spectrum t of the waterfall ring's
 * time frame (its row goes to ring position wf_pos + t), and rows are stored for the spectra from first_row on (same frame).  The
 * piece writes the next intermediate set of the rotation once the count kernel that read that set last is done, and the count
 * stream waits for the piece.  Returns the set (k1_set_release() behind the count kernel that reads it), -1 on error. */
static int k1_piece(struct fosphor *self, hipStream_t ks, const void *d_iq, int t, int sub_total, int tile, int first_row, int hop)
{
	K1Params k1;
	const int set = self->pp;
	int wf_first = first_row - t > 0 ? first_row - t : 0;
	const int stores_rows = wf_first < sub_total;

	self->pp = (self->pp + 1) % self->n_sets;
	self->d_bins = self->d_bins_pp[set];
	self->d_partial = self->d_partial_pp[set];
	if (self->overlap)
		HIP_TRY(self->f.set_free[set].wait(ks), "wait for intermediate set");
	if (!stores_rows)
		wf_first = sub_total;
	fill_k1(self, &k1, d_iq, sub_total, tile, (self->wf_pos + t) & (self->wf_rows - 1), wf_first, hop);
	/* waterfall ring ownership between K1s that may run on different streams: a K1 that stores rows into ring b follows the
	 * previous K1 that did (on its own stream it does anyway) */
	if (stores_rows)
		HIP_TRY(self->f.wf[self->wf_cur].wait(ks, true), "wait for the waterfall ring");
	prof_begin(self, 0, ks);
	HIP_TRY(launch_k1(k1, ks), "launch fft_bin");
	prof_end(self, ks);
	if (self->log2n == 13) {
		if (k1.cus) self->k1w_shared++; else self->k1w_full++;
	}
	if (stores_rows)
		HIP_TRY(self->f.wf[self->wf_cur].record(ks), "record waterfall rows");
	if (self->overlap) {
		HIP_TRY(self->f.k1_done[set].record(ks), "record K1 done");
		HIP_TRY(self->f.k1_done[set].wait(count_stream(self)), "K2 waits for K1");
	}
	return set;
error:
	return -1;
}

/* ... behind the count kernel (queued on the count stream) that read intermediate set `set`: the set is free again */
static int k1_set_release(struct fosphor *self, int set)
{
	if (self->overlap)
		HIP_TRY(self->f.set_free[set].record(count_stream(self)), "record set free");
	return 0;
error:
	return -EIO;
}

/* n_batches consecutive batches of `batch` spectra.  device_call: the samples are the caller's device buffer
 * (fosphor_amd_process_device*), which may be cut into sub-launches whose K1s alternate between two streams. */
static int run(struct fosphor *self, const void *d_iq, int n_batches, int batch, int hop = 0, int device_call = 0)
{
	const int total = n_batches * batch;
	const size_t sample_bytes = self->sample_bytes;
	const int hop_samples = hop ? hop : self->n;
	hipStream_t st2 = count_stream(self);
	const int did_prep = self->win_dirty || self->thr_dirty || self->state == ST_BOOTING;
	int sub_b, n_sub, use_alt;

	if (prepare(self))
		return -EIO;

	/* Sub-launches.  A call is cut into pieces of about sub_samples samples (64 reference batches): the
	 * bin-index / partial intermediates of a piece stay small enough to be consumed by K2 out of the Infinity
	 * Cache, and the pipeline below overlaps K2/K3 of piece j with K1 of piece j+1 INSIDE one call.
	 *   K1 (j)   on `stream` and the other FFT streams in rotation: K1 of piece j+1 is dispatched while K1 of piece j
	 *            drains, so no CU idles between them (kernel tail, dispatch gap and prologue overlap);
	 *   K2 (j)   on stream2 once K1 (j) has finished; K3 (j) follows it there, so the persistent state sees the
	 *            batches in order.
	 * The intermediates rotate among kSets sets: K1 may reuse a set once the K2 that read it has finished. */
	sub_b = fosphor_amd_plan_piece_batches(self->log2n, self->overlap, n_batches, batch, self->sub_samples);
	n_sub = (n_batches + sub_b - 1) / sub_b;
	use_alt = self->overlap && self->alt && device_call && (n_sub > 1 || self->relaxed);
	if (self->log2n == 16)
		use_alt = 0;		/* one fused FFT kernel at a time: its clusters own the counters and the intermediate */

	/* A call that stores every row of the ring does so in the other ring: its K1s then owe nothing to the
	 * row stores of the calls before it.  Otherwise the untouched rows must survive: same ring. */
	if (use_alt && total >= self->wf_rows)
		self->wf_cur ^= 1;
	if (use_alt && (did_prep || !self->relaxed)) {
		if (k1_streams_fork(self))
			return -EIO;
	}

	for (int b0 = 0; b0 < n_batches; b0 += sub_b) {
		const int nb = (n_batches - b0 < sub_b) ? n_batches - b0 : sub_b;
		const int t0 = b0 * batch, sub_total = nb * batch;
		const int tile = pick_tile(self, sub_total, batch);
		const struct fosphor_amd_count_plan plan = plan_count(self, nb, batch, 1);
		/* third stream: only a hand-off with a second hit-count set lets the merge run beside the next count */
		const int three = self->overlap && self->pipe3 && plan.two_sets;
		hipStream_t st3 = three ? self->stream3 : st2;
		hipStream_t ks = use_alt ? self->k1_streams[self->k1_seq++ % self->n_k1_streams] : self->stream;
		const int set = k1_piece(self, ks, (const char *)d_iq + (size_t)t0 * hop_samples * sample_bytes, t0, sub_total, tile,
		                         total - self->wf_rows, hop);
		int hset = 0;

		if (set < 0)
			return -EIO;
		if (three) {
			hset = self->hset;
			self->hset ^= 1;
			HIP_TRY(self->f.h_free[hset].wait(st2), "wait for hit-count set");
		} else if (drain_h_sets(self, st2)) {
			return -EIO;
		}
		if (run_count(self, plan, nb, batch, tile, 0, hset, 0, batch, st2))
			return -EIO;
		if (k1_set_release(self, set))
			return -EIO;
		if (three) {
			HIP_TRY(self->f.k2_done[hset].record(st2), "record K2 done");
			HIP_TRY(self->f.k2_done[hset].wait(st3), "K3 waits for K2");
		}
		if (run_merge(self, plan, nb, batch, 0, hset, st3))
			return -EIO;
		if (self->overlap && self->log2n == 13)
			HIP_TRY(self->f.tail.record(st3), "record tail");
		if (three)
			HIP_TRY(self->f.h_free[hset].record(st3), "record hit-count set free");
	}
	if (use_alt && !self->relaxed) {
		/* what the caller queues on `stream` next (e.g. refilling the sample buffer) follows every K1 */
		if (k1_streams_join(self))
			return -EIO;
	}

	self->wf_pos = (self->wf_pos + total) & (self->wf_rows - 1);	/* cl.c:954 */
	self->state = ST_PENDING;
	return 0;
error:
	return -EIO;
}

/* The checks of every call that reads the caller's device samples: `spectra` spectra from d_samples, their windows advancing
 * N / overlap samples (1: back to back).  sc16 samples are dwords: a device pointer to them must be 4-byte aligned (fp32 / fp16
 * callers are not checked here). */
static int device_call_ok(const struct fosphor *self, const void *d_samples, long long spectra, int overlap)
{
	return self && d_samples && spectra <= self->max_spectra && overlap >= 1 && overlap <= self->n && self->n % overlap == 0 &&
	       !(self->iq_format == FOSPHOR_AMD_IQ_SC16 && ((uintptr_t)d_samples & 3));
}

extern "C" int fosphor_amd_process_device(struct fosphor *self, const void *d_samples, int n_batches, int batch)
{
	return fosphor_amd_process_device_overlap(self, d_samples, n_batches, batch, 1);
}

/* overlap_cc (lib/overlap_cc_impl.cc:48-79) emits wlen-sample windows whose starts advance
 * wlen/overlap input samples, i.e. it materialises an overlap-times larger stream for the sink.
 * Here the same windows are read straight from the unexpanded stream: spectrum t starts at
 * sample t * N / overlap, so the unique HBM read per FFT'd sample drops to 8/overlap bytes. */
extern "C" int fosphor_amd_process_device_overlap(struct fosphor *self, const void *d_samples,
                                                  int n_batches, int batch, int overlap)
{
	if (!device_call_ok(self, d_samples, (long long)n_batches * batch, overlap) || n_batches < 1 || n_batches > self->max_batches ||
	    batch < 16 || (batch & 15))
		return -EINVAL;
	return run(self, d_samples, n_batches, batch, self->n / overlap, 1);
}

/* The kernels for the samples in staging slot k.  The slot is free again once everything queued so far (copy + kernels reading
 * d_stage[k]) has finished: a later fosphor_amd_upload_pinned into this slot (its own stream) waits for stage_free[k]. */
static int run_staged(struct fosphor *self, int k, int n_batches, int batch)
{
	int rv = run(self, self->d_stage[k], n_batches, batch);
	if (self->f.stage_free[k].record(self->stream) != hipSuccess && !rv)
		rv = -EIO;
	return rv;
}

extern "C" int fosphor_process(struct fosphor *self, void *samples, int len)
{
	int k;
	const size_t sample_bytes = self->sample_bytes;

	/* cl.c:882-886 */
	if (len <= 0 || (len & ((16 * self->n) - 1)))
		return -EINVAL;
	if ((long long)len > (long long)self->n * 1024)
		return -EINVAL;
	if (len / self->n > self->max_spectra)
		return -EINVAL;

	/* cl.c:903-910 enqueues a non-blocking write straight from the caller's memory, which the
	 * sink reuses immediately (base_sink_c_impl.cc:168-174: a latent race).  Here the samples
	 * are copied into a pinned ring slot before returning, and the slot is recycled only when
	 * its H2D copy has completed. */
	/* (uploads queued by fosphor_amd_upload_pinned and not yet processed come first: the sample stream is applied in order, and a
	 * pending upload may own the staging slot this call is about to fill) */
	while (self->pend_n) {
		const int rv = fosphor_amd_process_uploaded(self, NULL);
		if (rv)
			return rv;
	}
	k = self->stage_idx;
	/* (each piece behind its own check: fosphor_amd_process_pinned shares d_stage / stage_free) */
	if (!self->h_stage[k])
		HIP_TRY(hipHostMalloc((void **)&self->h_stage[k], sample_bytes * self->stage_samples, hipHostMallocDefault), "alloc pinned staging");
	if (!self->d_stage[k]) {
		HIP_TRY(hipMalloc((void **)&self->d_stage[k], sample_bytes * self->stage_samples), "alloc device staging");
		self->d_stage_cap[k] = self->stage_samples;
	}
	if (!self->f.stage_free[k].ev)
		HIP_TRY(self->f.stage_free[k].create(hipEventDisableTiming), "create staging event");
	else
		HIP_TRY(hipEventSynchronize(self->f.stage_free[k].ev), "wait staging slot");	/* (the HOST waits: it refills h_stage[k] next) */
	memcpy(self->h_stage[k], samples, sample_bytes * (size_t)len);
	HIP_TRY(hipMemcpyAsync(self->d_stage[k], self->h_stage[k], sample_bytes * (size_t)len, hipMemcpyHostToDevice, self->stream), "H2D samples");
	{
		const int rv = run_staged(self, k, 1, len / self->n);
		self->stage_idx ^= 1;
		return rv;
	}
error:
	return -EIO;
}

/* The upload of fosphor_amd_process_pinned and its kernels as two calls: a host that queues the NEXT upload before it waits for the
 * kernels of this one (the streaming sink: its per-frame synchronisation point drains the kernel streams, not the upload stream)
 * keeps the link busy across frames.  At most two uploads can be pending (two staging buffers): -EBUSY beyond. */
extern "C" int fosphor_amd_upload_pinned(struct fosphor *self, const void *samples, int len)
{
	int k;
	const size_t sample_bytes = self->sample_bytes;

	/* cl.c:882-886 for one batch; beyond it a whole number of 1024-spectrum batches in one call (applied one after the other like so
	 * many calls, one upload and one set of launches: what the host spends per call -- ~250 us -- is then spent per 64 MiB, not per 8) */
	const long long one = (long long)self->n * 1024;
	if (len <= 0 || (len & ((16 * self->n) - 1)) || len / self->n > self->max_spectra || ((long long)len > one && (long long)len % one))
		return -EINVAL;
	if (((long long)len > one ? (int)((long long)len / one) : 1) > self->max_batches)
		return -EINVAL;
	if (self->pend_n == 2)
		return -EBUSY;

	k = self->stage_idx;
	if (self->d_stage[k] && self->d_stage_cap[k] < (size_t)len) {		/* grown on demand (behind everything that reads the old one) */
		/* (this instance's streams only: the caller's unrelated streams are not stalled) */
		if (sync_all(self) || (self->copy_stream && hipStreamSynchronize(self->copy_stream) != hipSuccess))
			return -EIO;
		(void)hipFree(self->d_stage[k]);
		self->d_stage[k] = NULL;
	}
	if (!self->d_stage[k]) {
		const size_t cap = (size_t)len > self->stage_samples ? (size_t)len : self->stage_samples;
		HIP_TRY(hipMalloc((void **)&self->d_stage[k], sample_bytes * cap), "alloc device staging");
		self->d_stage_cap[k] = cap;
	}
	/* (events the host waits on, or behind a copy from host memory: no hipEventDisableSystemFence) */
	HIP_TRY(self->f.stage_free[k].create(hipEventDisableTiming), "create staging event");
	HIP_TRY(self->f.upload_done.create(hipEventDisableTiming), "create upload event");
	if (!self->copy_stream)
		HIP_TRY(hipStreamCreateWithFlags(&self->copy_stream, hipStreamNonBlocking), "create upload stream");
	HIP_TRY(self->f.upload_slot[k].create(hipEventDisableTiming), "create upload event");
	/* The upload runs on its own stream, beside the kernels of the batch before it (on one stream a batch cost its 150 us of DMA PLUS
	 * its kernels: 3.9 GSamples/s where the link does 7).  d_stage[k] was last read by the FFT kernel of the call before the last:
	 * the copy waits for the event recorded behind that call; the instance's stream waits for the copy. */
	HIP_TRY(self->f.stage_free[k].wait(self->copy_stream), "upload waits for the staging slot");
	HIP_TRY(hipMemcpyAsync(self->d_stage[k], samples, sample_bytes * (size_t)len, hipMemcpyHostToDevice, self->copy_stream), "H2D samples (pinned)");
	HIP_TRY(self->f.upload_slot[k].record(self->copy_stream), "record upload");
	HIP_TRY(self->f.upload_done.record(self->copy_stream), "record upload");
	self->pend_slot[(self->pend_head + self->pend_n) & 1] = k;
	self->pend_len[(self->pend_head + self->pend_n) & 1] = len;
	self->pend_n++;
	self->stage_idx ^= 1;
	return 0;
error:
	return -EIO;
}

extern "C" int fosphor_amd_pending_uploads(struct fosphor *self)
{
	return self ? self->pend_n : 0;
}

/* The kernels for the oldest pending upload; *len_out = its samples.  -EINVAL when nothing is pending. */
extern "C" int fosphor_amd_process_uploaded(struct fosphor *self, int *len_out)
{
	if (!self || !self->pend_n)
		return -EINVAL;
	const int k = self->pend_slot[self->pend_head], len = self->pend_len[self->pend_head];
	const long long one = (long long)self->n * 1024;
	const int n_batches = (long long)len > one ? (int)((long long)len / one) : 1;
	self->pend_head ^= 1;
	self->pend_n--;
	if (len_out)
		*len_out = len;
	HIP_TRY(self->f.upload_slot[k].wait(self->stream), "kernels wait for the upload");
	return run_staged(self, k, n_batches, len / self->n / n_batches);
error:
	return -EIO;
}

extern "C" int fosphor_amd_process_pinned(struct fosphor *self, const void *samples, int len)
{
	int rv;
	/* (uploads queued by fosphor_amd_upload_pinned and not yet processed come first: the stream is applied in order) */
	while (self->pend_n)
		if ((rv = fosphor_amd_process_uploaded(self, NULL)) != 0)
			return rv;
	if ((rv = fosphor_amd_upload_pinned(self, samples, len)) != 0)
		return rv;
	return fosphor_amd_process_uploaded(self, NULL);
}

extern "C" int fosphor_amd_wait_upload(struct fosphor *self)
{
	if (!self || !self->f.upload_done.ev)
		return 0;
	return hipEventSynchronize(self->f.upload_done.ev) == hipSuccess ? 0 : -EIO;
}

extern "C" int fosphor_amd_finish(struct fosphor *self)
{
	if (self->state == ST_READY)
		return 0;				/* cl.c:977-979 */
	if (self->state == ST_BOOTING) {		/* cl.c:981-995: finish the boot */
		if (prepare(self))
			return -EIO;
	}
	if (sync_all(self))
		return -EIO;
	if (self->h_k1h_err && self->h_k1h_err[0]) {
		fprintf(stderr, "[fosphor_amd] fused 65536-point FFT: a cluster wait timed out (code 0x%x); "
		        "results are invalid\n", self->h_k1h_err[0]);
		self->h_k1h_err[0] = 0;
		return -EIO;
	}
	self->state = ST_READY;
	return 1;
}

extern "C" void fosphor_draw(struct fosphor *self, struct fosphor_render *render)
{
	(void)fosphor_amd_finish(self);			/* fosphor.c:100-101 */
	if (render)
		render->_wf_pos = self->wf_pos;		/* fosphor.c:103 */
}

/* ------------------------------------------------------------------------ */
/* Buffers                                                                  */
/* ------------------------------------------------------------------------ */

static int get_buffers(struct fosphor *self, struct fosphor_amd_buffers *out, int want_hitcount)
{
	if (!self || !out)
		return -EINVAL;
	if (want_hitcount && self->export_src) {
		/* queued on the stream of the K2 that wrote the slabs (stream order = behind it); the view is complete when
		 * this call returns */
		hipStream_t st = self->export_stream ? self->export_stream : self->stream;
		if (launch_export_hc16(self->export_src, self->export_mask, self->mask_words, self->max_batches, self->d_hc_export, self->n_bins, self->n, st) != hipSuccess ||
		    hipStreamSynchronize(st) != hipSuccess)
			return -EIO;
		self->export_src = NULL;
	}
	out->d_waterfall = self->d_wf_pp[self->wf_cur];
	out->d_histogram = self->d_hist;
	out->d_spectrum  = (float *)self->d_spectrum;
	out->d_hitcount  = want_hitcount ? (uint32_t *)self->hc_view : NULL;	/* (run_merge: the export view, or the last batch's 32-bit slot) */
	out->waterfall_pos = self->wf_pos;
	out->fft_len = self->n; out->n_bins = self->n_bins; out->wf_rows = self->wf_rows;
	out->histo_scale = self->histo_scale; out->histo_offset = self->histo_offset;
	return 0;
}

extern "C" int fosphor_amd_get_buffers(struct fosphor *self, struct fosphor_amd_buffers *out)
{
	return get_buffers(self, out, 1);
}

/* The same without the hit-count view (d_hitcount = NULL): nothing is launched, nothing is waited for. */
extern "C" int fosphor_amd_get_buffers_nohc(struct fosphor *self, struct fosphor_amd_buffers *out)
{
	return get_buffers(self, out, 0);
}

extern "C" int fosphor_amd_read(struct fosphor *self, int which, void *host, uint64_t bytes)
{
	struct fosphor_amd_buffers b;
	const void *src; uint64_t want;
	int rv;

	if (!self || !host)
		return -EINVAL;
	rv = fosphor_amd_finish(self);
	if (rv < 0)
		return rv;
	rv = get_buffers(self, &b, which == 3);
	if (rv < 0)
		return rv;
	switch (which) {
	case 0: src = b.d_waterfall; want = sizeof(float) * (uint64_t)self->wf_rows * self->n; break;
	case 1: src = b.d_histogram; want = sizeof(float) * (uint64_t)self->n_bins * self->n; break;
	case 2: src = b.d_spectrum;  want = sizeof(float) * 4 * self->n; break;
	case 3: src = b.d_hitcount;  want = sizeof(uint32_t) * (uint64_t)self->n_bins * self->n; break;
	default: return -EINVAL;
	}
	if (bytes != want)
		return -EINVAL;
	if (hipMemcpy(host, src, want, hipMemcpyDeviceToHost) != hipSuccess)
		return -EIO;
	return 0;
}

/* ------------------------------------------------------------------------ */
/* Test hooks                                                               */
/* ------------------------------------------------------------------------ */

/* The tables uploaded for a hook's kernel, without the boot fills, behind everything queued (the intermediate sets the hook
 * writes may still be read by a queued K2) */
static int prepare_hook(struct fosphor *self)
{
	if (sync_all(self))
		return -EIO;
	const int saved_state = self->state;
	self->state = ST_READY;
	const int rv = prepare(self);
	self->state = saved_state;
	return rv;
}

extern "C" int fosphor_amd_fft(struct fosphor *self, const void *d_in, void *d_out, int n_spectra)
{
	K1Params k1;
	/* (N = 8192: tiles of at least 8 spectra -- the 9th bits of the bin indices go out per eight spectra) */
	if (!device_call_ok(self, d_in, n_spectra, 1) || !d_out || n_spectra < 4 || (n_spectra & (self->log2n == 13 ? 7 : 3)))
		return -EINVAL;
	if (prepare_hook(self))
		return -EIO;
	/* rows are not stored (wf_first = total); bins/partials land in scratch */
	fill_k1(self, &k1, d_in, n_spectra, self->log2n == 13 ? 8 : 4, 0, n_spectra);
	k1.fft_out = (float2 *)d_out;
	if (launch_k1(k1, self->stream) != hipSuccess)
		return -EIO;
	return hipStreamSynchronize(self->stream) == hipSuccess ? 0 : -EIO;
}

extern "C" int fosphor_amd_bin(struct fosphor *self, const void *d_fft, void *d_bin, void *d_pwr, int n)
{
	K1Params k1;
	int force = 0;
	const char *e = getenv("FOSPHOR_AMD_FORCE_EXACT_BIN");
	if (!self || !d_fft || !d_bin || !d_pwr || n < 1)
		return -EINVAL;
	if (e && *e == '1') force = 1;
	if (prepare_hook(self))
		return -EIO;
	fill_k1(self, &k1, NULL, 0, 4, 0, 0);
	if (launch_bin_hook((const float2 *)d_fft, (uint8_t *)d_bin, (float *)d_pwr, n, k1, force, self->stream) != hipSuccess)
		return -EIO;
	return hipStreamSynchronize(self->stream) == hipSuccess ? 0 : -EIO;
}

/* ------------------------------------------------------------------------ */
/* Multi-GPU split                                                          */
/* ------------------------------------------------------------------------ */

/* Spectra [t_offset, t_offset + n_local) of a batch of total_batch spectra (a time shard of a display frame), windows advancing
 * N / overlap samples, counted into partial slot `slot`; rows are stored for the spectra that survive in the ring */
static int accumulate(struct fosphor *self, const void *d_samples, int n_local, int t_offset, int total_batch, int overlap)
{
	if (!device_call_ok(self, d_samples, n_local, overlap) || n_local < 16 || (n_local & 15) || (t_offset & 15) ||
	    t_offset < 0 || t_offset + n_local > total_batch)
		return -EINVAL;
	const int did_prep = self->win_dirty || self->thr_dirty || self->state == ST_BOOTING;
	const int hop = self->n / overlap;
	const int first_row = total_batch - self->wf_rows;	/* spectrum t_offset + t stores its row iff t_offset + t >= first_row */
	hipStream_t st2 = count_stream(self);
	const struct fosphor_amd_count_plan plan = plan_count(self, 1, n_local, 0);
	const int cpb = plan.cpb;
	const int chunked = plan.handoff == FOSPHOR_AMD_COUNT_SUM16;	/* whole 1024-spectrum chunks, and room for their slabs */
	const int sub_c = self->sub_samples / (1024LL * self->n) > 1 ? (int)(self->sub_samples / (1024LL * self->n)) : 1;

	if (prepare(self))
		return -EIO;
	if (chunked && cpb > sub_c) {
		/* A shard of several whole 1024-spectrum chunks runs like a device-resident call: sub-launches of
		 * sub_samples samples, K1s alternating between two streams, K2 of piece j beside K1 of piece j + 1.
		 * Each K2 leaves its chunks' packed 16-bit count slabs and float partials at the chunks' places;
		 * one k2c_sum at the end adds all of them into the 32-bit slot that is exchanged. */
		const size_t cells = self->cells();
		const int use_alt = self->overlap && self->alt && self->log2n != 16;
		/* K2 counts G consecutive 1024-spectrum chunks per work-group (16-bit counters hold 65535 spectra): 1 / G of the
		 * slab traffic, as long as enough work-groups are left to keep the bin-index reads in flight */
		int G = 1;
		/* measured, N = 1024, 256 batches per frame: G = 1 / 2 / 4 / 8 -> 486 / 510 / 528 / 450 GSamples/s (at 8 the
		 * count kernel's 128 work-groups no longer keep up with the FFT kernel) */
		for (int want = self->kn_frame_group; want >= 1; want >>= 1)
			if (want <= 32 && !(want & (want - 1)) && sub_c % want == 0 && cpb % want == 0) {
				G = want;
				break;
			}
		if (drain_h_sets(self, st2) || (use_alt && (did_prep || !self->relaxed) && k1_streams_fork(self)))
			return -EIO;
		for (int c0 = 0; c0 < cpb; c0 += sub_c) {
			const int nc = (cpb - c0 < sub_c) ? cpb - c0 : sub_c;
			const int t0 = c0 * 1024, sub_total = nc * 1024;
			const int tile = pick_tile(self, sub_total, 1024);
			hipStream_t ks = use_alt ? self->k1_streams[self->k1_seq++ % self->n_k1_streams] : self->stream;
			const int set = k1_piece(self, ks, (const char *)d_samples + (size_t)t0 * hop * self->sample_bytes, t_offset + t0,
			                         sub_total, tile, first_row, hop);
			K2Params k2;

			if (set < 0)
				return -EIO;
			self->acc_pieces++;
			fill_k2(self, &k2, sub_total, sub_total, 1024 * G, tile, t_offset + t0, total_batch);
			k2.hc = self->hc_slot(self->slot);
			k2.hc16 = self->d_slab16 + (size_t)(c0 / G) * cells;
			k2.chunk_sum = self->d_chunk_sum + (size_t)(c0 / G) * self->n;
			k2.chunk_max = self->d_chunk_max + (size_t)(c0 / G) * self->n;
			prof_begin(self, 1, st2);
			HIP_TRY(launch_k2(k2, nc / G, st2), "launch count");
			prof_end(self, st2);
			if (k1_set_release(self, set))
				return -EIO;
		}
		HIP_TRY(launch_chunk_sum(self, 1, cpb / G, self->slot, self->slot, 1, st2), "launch chunk sum");
		if (use_alt && !self->relaxed && k1_streams_join(self))
			return -EIO;
	} else {
		/* one K1 launch: same two-stream pipeline as run(): K1 on `stream`, K2 (and later the exchange and
		 * fosphor_amd_merge's K3) on the count stream, intermediates rotating between the sets */
		const int tile = pick_tile(self, n_local, n_local);
		const int set = k1_piece(self, self->stream, d_samples, t_offset, n_local, tile, first_row, hop);
		if (set < 0)
			return -EIO;
		self->acc_pieces++;
		if (drain_h_sets(self, st2) || run_count(self, plan, 1, n_local, tile, self->slot, 0, t_offset, total_batch, st2) ||
		    k1_set_release(self, set))
			return -EIO;
	}
	/* the ring advances with the data (host state), so the next frame can be accumulated
	 * before this one is merged */
	self->wf_pos = (self->wf_pos + total_batch) & (self->wf_rows - 1);
	self->state = ST_PENDING;
	return 0;
error:
	return -EIO;
}

extern "C" int fosphor_amd_accumulate_device(struct fosphor *self, const void *d_samples,
                                             int n_local, int t_offset, int total_batch)
{
	return accumulate(self, d_samples, n_local, t_offset, total_batch, 1);
}

/* the same with overlap_cc fused into the read (see fosphor_amd_process_device_overlap): d_samples is this rank's part
 * of the UNEXPANDED stream, (n_local - 1) * N / overlap + N samples starting at the first sample of its first spectrum */
extern "C" int fosphor_amd_accumulate_device_overlap(struct fosphor *self, const void *d_samples,
                                                     int n_local, int t_offset, int total_batch, int overlap)
{
	return accumulate(self, d_samples, n_local, t_offset, total_batch, overlap);
}

extern "C" int fosphor_amd_set_partial_slot(struct fosphor *self, int slot)
{
	if (!self || slot < 0 || slot >= self->max_batches)
		return -EINVAL;
	self->slot = slot;
	return 0;
}

extern "C" int fosphor_amd_get_partials(struct fosphor *self, struct fosphor_amd_partials *out)
{
	if (!self || !out)
		return -EINVAL;
	out->d_hc = self->hc_slot(self->slot);
	out->d_live_sum = self->live_sum_at(self->slot);
	out->d_max = self->vmax_at(self->slot);
	out->n_hc = self->n_bins * self->n;
	out->n_cols = self->n;
	return 0;
}

/* K3 on the partial arrays of the current slot (a batch of total_batch spectra), for the cells [cell_begin, cell_end) of the
 * histogram (0, 0: all of them) */
static int merge_slot(struct fosphor *self, int total_batch, int cell_begin, int cell_end)
{
	if (prepare(self) || run_merge(self, plan_count(self, 1, total_batch, 0), 1, total_batch, self->slot, 0, count_stream(self), cell_begin, cell_end))
		return -EIO;
	self->state = ST_PENDING;
	return 0;
}

extern "C" int fosphor_amd_merge(struct fosphor *self, int total_batch)
{
	if (!self || total_batch < 16)
		return -EINVAL;
	return merge_slot(self, total_batch, 0, 0);
}

/* ---- native exchange (RCCL over xGMI), fosphor_exchange.cpp --------------- */

/* 1 when the RCCL library can be bound in this process (no communicator, no collective: purely local) */
extern "C" int fosphor_amd_comm_available(void)
{
	return xchg_available();
}

/* ncclCommCount of a communicator made by fosphor_amd_comm_init */
extern "C" int fosphor_amd_comm_count(void *comm)
{
	return comm ? xchg_comm_count(comm) : -EINVAL;
}

/* events around an exchange on its stream, while profiling is on (fosphor_amd_exchange_time) */
static void xprof_begin(struct fosphor *self, hipStream_t st)
{
	if (!self->prof)
		return;
	while (self->xev_used + 2 > self->xev_pool.size()) {
		hipEvent_t e;
		if (hipEventCreateWithFlags(&e, dep_event_flags() & ~hipEventDisableTiming) != hipSuccess)
			return;
		self->xev_pool.push_back(e);
	}
	(void)hipEventRecord(self->xev_pool[self->xev_used], st);
}

static void xprof_end(struct fosphor *self, hipStream_t st)
{
	if (!self->prof || self->xev_used + 2 > self->xev_pool.size())
		return;
	if (hipEventRecord(self->xev_pool[self->xev_used + 1], st) == hipSuccess)
		self->xev_used += 2;
}

/* Sum of the durations of the exchanges recorded since the last call (hipEvents on the count/merge stream around the
 * ncclGroup), and how many there were; resets.  0 exchanges when profiling was off. */
extern "C" int fosphor_amd_exchange_time(struct fosphor *self, float *ms_total, int *count)
{
	if (!self || !ms_total || !count)
		return -EINVAL;
	if (sync_all(self))
		return -EIO;
	*ms_total = 0.0f; *count = 0;
	for (size_t i = 0; i + 1 < self->xev_used; i += 2) {
		float t = 0.0f;
		if (hipEventElapsedTime(&t, self->xev_pool[i], self->xev_pool[i + 1]) == hipSuccess) {
			*ms_total += t;
			(*count)++;
		}
	}
	self->xev_used = 0;
	return 0;
}

extern "C" int fosphor_amd_comm_unique_id(void *id128)
{
	return id128 ? xchg_unique_id(id128) : -EINVAL;
}

extern "C" int fosphor_amd_comm_init(void **comm, int world, int rank, const void *id128)
{
	if (!comm || !id128 || world < 1 || rank < 0 || rank >= world)
		return -EINVAL;
	return xchg_comm_init(comm, world, rank, id128);
}

extern "C" int fosphor_amd_comm_destroy(void *comm)
{
	return comm ? xchg_comm_destroy(comm) : -EINVAL;
}

/* Between fosphor_amd_accumulate_device and fosphor_amd_merge: one ncclGroup of three all-reduces over the
 * partial arrays of the current slot, queued on the count/merge stream (behind K2, in front of K3). */
extern "C" int fosphor_amd_exchange(struct fosphor *self, void *comm)
{
	if (!self || !comm)
		return -EINVAL;
	hipStream_t st = count_stream(self);
	xprof_begin(self, st);
	const int rv = xchg_allreduce3(comm, st, self->hc_slot(self->slot), self->cells(),
	                               self->live_sum_at(self->slot), self->vmax_at(self->slot), (size_t)self->n);
	xprof_end(self, st);
	return rv;
}

/* Frequency-sliced form for large states (128 MiB of counts at 65536 x 512): the counts are
 * reduce-scattered -- rank r owns cells [r C / world, (r + 1) C / world) of the [bin][x] array -- and
 * fosphor_amd_merge_sliced updates only that slice of the histogram; fosphor_amd_gather_state all-gathers the
 * slices when a complete histogram is wanted on every rank (once per draw, not once per exchange). */
static int slice_ok(const struct fosphor *self, int world, int rank)
{
	return self && world >= 1 && rank >= 0 && rank < world && (size_t)self->n_bins * self->n % (size_t)world == 0;
}

extern "C" int fosphor_amd_exchange_sliced(struct fosphor *self, void *comm, int world, int rank)
{
	if (!comm || !slice_ok(self, world, rank))
		return -EINVAL;
	hipStream_t st = count_stream(self);
	xprof_begin(self, st);
	const int rv = xchg_reduce_scatter(comm, st, self->hc_slot(self->slot), self->cells(), world, rank,
	                                   self->live_sum_at(self->slot), self->vmax_at(self->slot), (size_t)self->n);
	xprof_end(self, st);
	return rv;
}

extern "C" int fosphor_amd_merge_sliced(struct fosphor *self, int total_batch, int world, int rank)
{
	if (!slice_ok(self, world, rank) || total_batch < 16)
		return -EINVAL;
	const int per = self->n_bins * self->n / world;
	return merge_slot(self, total_batch, per * rank, per * (rank + 1));
}

extern "C" int fosphor_amd_gather_state(struct fosphor *self, void *comm, int world, int rank)
{
	if (!comm || !slice_ok(self, world, rank))
		return -EINVAL;
	const size_t cells = (size_t)self->n_bins * self->n;
	hipStream_t st = count_stream(self);
	if (k3_stream_enter(self, st))
		return -EIO;
	self->hot_valid = 0;		/* other ranks' cells arrive: the hot-row flags of the sparse merge no longer describe d_hist */
	return xchg_allgather_f32(comm, st, self->d_hist, cells, world, rank);
}

/* ---- compact wire formats (include/fosphor_amd_wire.h, kernels in fosphor_wire.hip) ---- */

static unsigned wire_rows(const struct fosphor *self)
{
	return (unsigned)(self->cells() / FOSPHOR_AMD_WIRE_ROW_CELLS);
}

/* what every entry point refuses before it does anything */
static int wire_args_ok(const struct fosphor *self, int total_batch, int form, int world, int rank)
{
	return self && total_batch >= 16 && total_batch <= FOSPHOR_AMD_WIRE_MAX_BATCH &&
	       (form == FOSPHOR_AMD_WIRE_PACKED16 || form == FOSPHOR_AMD_WIRE_SPARSE16) &&
	       world >= 1 && rank >= 0 && rank < world && self->cells() % (FOSPHOR_AMD_WIRE_ROW_CELLS * 32) == 0;
}

/* hipEvents around the last launch of wire kernel `kind` (0 mask, 1 pack, 2 unpack), while profiling is on */
static void wire_prof(struct fosphor *self, int kind, int end, hipStream_t st)
{
	hipEvent_t *e = &self->wire.ev[2 * kind + end];
	if (!self->prof)
		return;
	if (!end)
		self->wire.ev_rec[kind] = 0;
	if (!*e && hipEventCreateWithFlags(e, dep_event_flags() & ~hipEventDisableTiming) != hipSuccess)
		return;
	if (hipEventRecord(*e, st) == hipSuccess && end && self->wire.ev[2 * kind])
		self->wire.ev_rec[kind] = 1;
}

/* work is queued on the count stream: fosphor_amd_finish has something to wait for again (an instance that is still booting
 * stays so: its boot fills are yet to be queued) */
static void wire_queued(struct fosphor *self)
{
	if (self->state == ST_READY)
		self->state = ST_PENDING;
}

static void wire_fill(const struct fosphor *self, struct fosphor_amd_wire *out)
{
	out->d_masks = self->wire.d_masks;
	out->mask_words = (int)(wire_rows(self) / 32);
	out->world = self->wire.world;
	out->d_words = self->wire.d_words;
	out->n_words = self->wire.form ? self->wire.n_words : 0;
	out->form = self->wire.form;
	out->live_rows = self->wire.live_rows;
	out->rows = (int)wire_rows(self);
}

static int wire_mask_stage(struct fosphor *self, int world, int rank, hipStream_t st)
{
	const unsigned rows = wire_rows(self);
	const size_t part = rows / 32;
	if (world > self->wire.mask_cap) {
		/* (kernels of an earlier frame may still read the old buffer) */
		HIP_TRY(hipStreamSynchronize(st), "drain the count stream before the mask buffer grows");
		(void)hipFree(self->wire.d_masks);
		self->wire.d_masks = nullptr;
		self->wire.mask_cap = 0;
		HIP_TRY(hipMalloc((void **)&self->wire.d_masks, sizeof(uint32_t) * part * world), "alloc wire masks");
		self->wire.mask_cap = world;
	}
	self->wire.world = world;
	wire_prof(self, 0, 0, st);
	HIP_TRY(launch_wire_mask(self->hc_slot(self->slot), self->wire.d_masks + part * rank, rows, st), "launch wire mask");
	wire_prof(self, 0, 1, st);
	wire_queued(self);
	self->wire.masked = world;
	self->wire.masked_slot = self->slot;
	return 0;
error:
	return -EIO;
}

static int wire_pack_stage(struct fosphor *self, int form, int world, hipStream_t st)
{
	const unsigned rows = wire_rows(self);
	const size_t cells = self->cells();
	int taken = form;
	if (!self->wire.d_words)
		HIP_TRY(hipMalloc((void **)&self->wire.d_words, sizeof(uint32_t) * (cells / 2)), "alloc wire words");
	self->wire.form = 0;
	if (form == FOSPHOR_AMD_WIRE_SPARSE16) {
		if (!self->wire.d_union)
			HIP_TRY(hipMalloc((void **)&self->wire.d_union, sizeof(uint32_t) * (rows / 32)), "alloc wire union mask");
		if (!self->wire.d_prefix)
			HIP_TRY(hipMalloc((void **)&self->wire.d_prefix, sizeof(uint32_t) * (rows / 32)), "alloc wire prefix counts");
		if (!self->wire.d_live)
			HIP_TRY(hipMalloc((void **)&self->wire.d_live, sizeof(uint32_t)), "alloc wire live-row count");
		if (!self->wire.h_live)
			HIP_TRY(hipHostMalloc((void **)&self->wire.h_live, 64, hipHostMallocMapped), "alloc wire live-row word");
		self->wire.masked = 0;
		wire_prof(self, 1, 0, st);
		HIP_TRY(launch_wire_pack_sparse(self->hc_slot(self->slot), self->wire.d_masks, world, self->wire.d_union, self->wire.d_prefix,
		                                self->wire.d_live, self->wire.h_live, self->wire.d_words, rows, st), "launch wire pack (sparse)");
		wire_prof(self, 1, 1, st);
		/* THE host wait of the sparse form: the all-reduce is sized by the union's live rows */
		HIP_TRY(hipStreamSynchronize(st), "wait for the live-row count");
		self->wire.live_rows = (int)self->wire.h_live[0];
		if ((unsigned)self->wire.live_rows > rows / 2)
			taken = FOSPHOR_AMD_WIRE_PACKED16;
	} else {
		self->wire.live_rows = -1;
	}
	if (taken == FOSPHOR_AMD_WIRE_PACKED16) {
		wire_prof(self, 1, 0, st);		/* (of a frame that fell back, the dense pack is the one timed) */
		HIP_TRY(launch_wire_pack_dense(self->hc_slot(self->slot), self->wire.d_words, cells, st), "launch wire pack (dense)");
		wire_prof(self, 1, 1, st);
	}
	wire_queued(self);
	self->wire.form = taken;
	self->wire.packed_slot = self->slot;
	self->wire.n_words = taken == FOSPHOR_AMD_WIRE_PACKED16 ? (int)(cells / 2) : self->wire.live_rows * FOSPHOR_AMD_WIRE_ROW_WORDS;
	self->wire.stats[form == FOSPHOR_AMD_WIRE_PACKED16 ? FOSPHOR_AMD_WIRE_FRAMES_PACKED16 :
	                 taken == form ? FOSPHOR_AMD_WIRE_FRAMES_SPARSE16 : FOSPHOR_AMD_WIRE_FRAMES_FELL_BACK]++;
	self->wire.stats[FOSPHOR_AMD_WIRE_LAST_LIVE_ROWS] = self->wire.live_rows;
	self->wire.stats[FOSPHOR_AMD_WIRE_LAST_WIRE_BYTES] = 4LL * self->wire.n_words +
		(form == FOSPHOR_AMD_WIRE_SPARSE16 ? 4LL * world * (rows / 32) : 0);
	return 0;
error:
	return -EIO;
}

static int wire_unpack_stage(struct fosphor *self, hipStream_t st)
{
	wire_prof(self, 2, 0, st);
	if (self->wire.form == FOSPHOR_AMD_WIRE_PACKED16)
		HIP_TRY(launch_wire_unpack_dense(self->wire.d_words, self->hc_slot(self->slot), self->cells(), st), "launch wire unpack (dense)");
	else
		HIP_TRY(launch_wire_unpack_sparse(self->wire.d_words, self->wire.d_union, self->wire.d_prefix, self->wire.d_live,
		                                  self->hc_slot(self->slot), wire_rows(self), st), "launch wire unpack (sparse)");
	wire_prof(self, 2, 1, st);
	wire_queued(self);
	self->wire.form = 0;
	return 0;
error:
	return -EIO;
}

extern "C" int fosphor_amd_wire_mask(struct fosphor *self, int total_batch, int world, int rank)
{
	if (!wire_args_ok(self, total_batch, FOSPHOR_AMD_WIRE_SPARSE16, world, rank))
		return -EINVAL;
	return wire_mask_stage(self, world, rank, count_stream(self));
}

extern "C" int fosphor_amd_wire_pack(struct fosphor *self, int total_batch, int form, int world, struct fosphor_amd_wire *out)
{
	if (!out || !wire_args_ok(self, total_batch, form, world, 0) ||
	    (form == FOSPHOR_AMD_WIRE_SPARSE16 && (self->wire.masked != world || self->wire.masked_slot != self->slot)))
		return -EINVAL;
	const int rv = wire_pack_stage(self, form, world, count_stream(self));
	wire_fill(self, out);
	return rv;
}

extern "C" int fosphor_amd_wire_unpack(struct fosphor *self)
{
	if (!self || !self->wire.form || self->wire.packed_slot != self->slot)
		return -EINVAL;
	return wire_unpack_stage(self, count_stream(self));
}

extern "C" int fosphor_amd_wire_get(struct fosphor *self, struct fosphor_amd_wire *out)
{
	if (!self || !out)
		return -EINVAL;
	wire_fill(self, out);
	return 0;
}

extern "C" int fosphor_amd_exchange_compact(struct fosphor *self, void *comm, int total_batch, int form, int world, int rank)
{
	if (!comm || !wire_args_ok(self, total_batch, form, world, rank))
		return -EINVAL;
	hipStream_t st = count_stream(self);
	int rv = 0;
	xprof_begin(self, st);
	if (form == FOSPHOR_AMD_WIRE_SPARSE16) {
		rv = wire_mask_stage(self, world, rank, st);
		rv = rv ? rv : xchg_allgather_u32(comm, st, self->wire.d_masks, wire_rows(self) / 32, rank);
	}
	rv = rv ? rv : wire_pack_stage(self, form, world, st);
	rv = rv ? rv : xchg_allreduce3(comm, st, self->wire.d_words, (size_t)self->wire.n_words,
	                               self->live_sum_at(self->slot), self->vmax_at(self->slot), (size_t)self->n);
	rv = rv ? rv : wire_unpack_stage(self, st);
	xprof_end(self, st);
	return rv;
}

extern "C" int fosphor_amd_wire_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_WIRE_STATS])
{
	if (!self || !stats)
		return -EINVAL;
	for (int i = 0; i < FOSPHOR_AMD_WIRE_STATS; i++)
		stats[i] = self->wire.stats[i];
	return 0;
}

extern "C" int fosphor_amd_wire_kernel_times(struct fosphor *self, float ms[3])
{
	if (!self || !ms)
		return -EINVAL;
	if (hipStreamSynchronize(count_stream(self)) != hipSuccess)
		return -EIO;
	for (int k = 0; k < 3; k++) {
		ms[k] = -1.0f;
		if (self->wire.ev_rec[k] && hipEventElapsedTime(&ms[k], self->wire.ev[2 * k], self->wire.ev[2 * k + 1]) != hipSuccess)
			ms[k] = -1.0f;
	}
	return 0;
}

/* ------------------------------------------------------------------------ */
/* Measurement                                                              */
/* ------------------------------------------------------------------------ */

extern "C" void fosphor_amd_profile(struct fosphor *self, int enable)
{
	self->prof = enable == 2 ? 2 : (enable ? 1 : 0);
}

extern "C" int fosphor_amd_kernel_times(struct fosphor *self, float ms[3], int launches[3])
{
	if (!self)
		return -EINVAL;
	if (sync_all(self))
		return -EIO;
	for (int i = 0; i < 3; i++) { ms[i] = 0.0f; launches[i] = 0; }
	for (size_t i = 0; i + 1 < self->ev_used; i += 2) {
		float t = 0.0f;
		int kind = self->ev_kind[i / 2];
		if (hipEventElapsedTime(&t, self->ev_pool[i], self->ev_pool[i + 1]) == hipSuccess) {
			ms[kind] += t;
			launches[kind]++;
		}
	}
	self->ev_used = 0;
	self->ev_kind.clear();
	return 0;
}

/* Time during which at least one kernel of each kind was running (union of the recorded intervals), from the
 * same events fosphor_amd_kernel_times sums.  K1s of consecutive sub-launches overlap on two streams, so the sum
 * of their individual durations counts the shared time twice; the union is what a launch costs.  Call before
 * fosphor_amd_kernel_times (which resets). */
extern "C" int fosphor_amd_kernel_busy(struct fosphor *self, float busy_ms[3])
{
	if (!self)
		return -EINVAL;
	if (sync_all(self))
		return -EIO;
	for (int kind = 0; kind < 3; kind++) {
		std::vector<std::pair<float, float> > iv;
		for (size_t i = 0; i + 1 < self->ev_used; i += 2) {
			float a = 0.0f, b = 0.0f;
			if (self->ev_kind[i / 2] != kind)
				continue;
			if (hipEventElapsedTime(&a, self->ev_pool[0], self->ev_pool[i]) != hipSuccess ||
			    hipEventElapsedTime(&b, self->ev_pool[0], self->ev_pool[i + 1]) != hipSuccess)
				continue;
			iv.push_back(std::make_pair(a, b));
		}
		std::sort(iv.begin(), iv.end());
		float busy = 0.0f, cur_a = 0.0f, cur_b = -1.0f;
		for (size_t i = 0; i < iv.size(); i++) {
			if (cur_b < cur_a || iv[i].first > cur_b) {
				if (cur_b >= cur_a) busy += cur_b - cur_a;
				cur_a = iv[i].first; cur_b = iv[i].second;
			} else if (iv[i].second > cur_b) {
				cur_b = iv[i].second;
			}
		}
		if (cur_b >= cur_a) busy += cur_b - cur_a;
		busy_ms[kind] = busy;
	}
	return 0;
}

/* Measurement hook: the memory traffic of one K1 launch (same loads, same stores, same order)
 * without its arithmetic, on this instance's buffers; average of `reps` launches in ms.  The
 * intermediates of the current set are overwritten (call between launches, results unaffected:
 * every launch rewrites them before reading). */
extern "C" int fosphor_amd_traffic_twin(struct fosphor *self, const void *d_samples, int n_batches, int batch,
                                        int reps, float *ms_out)
{
	K1Params k1;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	const int total = n_batches * batch;
	float ms = 0.0f;
	if (!self || !d_samples || !ms_out || reps < 1 || total < 16 || total > self->max_spectra || self->log2n != 10 || self->bins16 ||
	    self->iq_format != FOSPHOR_AMD_IQ_FP32)
		return -EINVAL;
	if (fosphor_amd_finish(self) < 0 || prepare(self))
		return -EIO;
	fill_k1(self, &k1, d_samples, total, pick_tile(self, total, batch), 0, total);
	hipError_t le = hipEventCreate(&e0);
	if (le == hipSuccess) le = hipEventCreate(&e1);
	for (int i = 0; i < 3 && le == hipSuccess; i++)
		le = launch_k1_traffic_twin(k1, self->stream);
	if (le == hipSuccess) le = hipEventRecord(e0, self->stream);
	for (int i = 0; i < reps && le == hipSuccess; i++)
		le = launch_k1_traffic_twin(k1, self->stream);
	if (le == hipSuccess) le = hipEventRecord(e1, self->stream);
	if (le == hipSuccess) le = hipEventSynchronize(e1);
	if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	if (le != hipSuccess)
		return -EIO;
	*ms_out = ms / (float)reps;
	return 0;
}

/* Placement tuning.  On MI355X the same FFT launch runs in one of two states -- its bare memory traffic takes 98 or 109 us per 512 MiB of
 * IQ -- and which one is a property of the ALLOCATIONS involved: the caller's IQ buffer against this instance's intermediate sets (bin
 * indices + tile partials).  Re-allocating either re-rolls it (about even odds; offsets inside an allocation do not matter: measured up to
 * 1 GiB; tools/twin_state.py).  This call measures the memory twin of the FFT kernel against `d_samples` for every intermediate set and
 * re-allocates a set (keeping the rejected allocations until the end, so that the allocator hands out different memory) until its traffic
 * runs at >= 6.0 TB/s or `max_tries` allocations have been tried, keeping the fastest.  us_before / us_after: the slowest set before and
 * after (NULL allowed).  Returns the number of re-allocations made, or -EINVAL / -EIO.  Results never depend on it. */
extern "C" int fosphor_amd_tune_placement(struct fosphor *self, const void *d_samples, int n_batches, int batch, int max_tries,
                                          float *us_before, float *us_after)
{
	const int total = n_batches * batch;
	if (!self || !d_samples || total < 16 || total > self->max_spectra || self->log2n != 10 || self->bins16 || max_tries < 1 ||
	    self->iq_format != FOSPHOR_AMD_IQ_FP32)
		return -EINVAL;
	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	const size_t bins_bytes = (size_t)self->max_spectra * self->n * (self->bins16 ? 2 : 1);
	size_t tiles_max = (size_t)self->max_spectra / 4;
	const size_t part_bytes = sizeof(float2) * tiles_max * self->n;
	/* what the twin moves per launch: the IQ, one byte of bin index per sample, the tile partials */
	const double bytes = (double)total * self->n * 9.0 + (double)(total / pick_tile(self, total, batch)) * self->n * 8.0;
	/* (a launch of less than 128 MiB is timed by its launch overhead, not by the memory behind it: measured, nothing replaced) */
	if (bytes < 128.0 * 1048576.0)
		max_tries = 1;
	const float good_ms = (float)(bytes / 6.0e12 * 1e3);
	std::vector<void *> rejected;
	int reallocs = 0;
	float worst_before = 0.0f, worst_after = 0.0f;
	uint32_t *const cur_bins = self->d_bins;
	int cur_set = 0;
	for (int i = 0; i < kSets; i++)
		if (self->d_bins_pp[i] == cur_bins) cur_set = i;
	for (int i = 0; i < self->n_sets; i++) {
		float best = 0.0f;
		for (int t = 0; t < max_tries; t++) {
			uint32_t *nb = self->d_bins_pp[i];
			float2 *np = self->d_partial_pp[i];
			if (t > 0) {
				if (hipMalloc((void **)&nb, bins_bytes) != hipSuccess)
					break;
				if (hipMalloc((void **)&np, part_bytes) != hipSuccess) {
					(void)hipFree(nb);
					break;
				}
			}
			uint32_t *const ob = self->d_bins_pp[i];
			float2 *const op = self->d_partial_pp[i];
			self->d_bins_pp[i] = nb; self->d_partial_pp[i] = np;
			self->d_bins = nb; self->d_partial = np;
			float ms = 0.0f;
			if (fosphor_amd_traffic_twin(self, d_samples, n_batches, batch, 8, &ms) != 0) {
				self->d_bins_pp[i] = ob; self->d_partial_pp[i] = op;
				if (t > 0) { (void)hipFree(nb); (void)hipFree(np); }
				break;
			}
			if (t == 0) {
				best = ms;
				if (ms > worst_before) worst_before = ms;
			} else if (ms < best) {
				rejected.push_back(ob); rejected.push_back(op);		/* the new pair is the better one */
				best = ms;
				reallocs++;
			} else {
				self->d_bins_pp[i] = ob; self->d_partial_pp[i] = op;	/* keep what we had */
				rejected.push_back(nb); rejected.push_back(np);
			}
			if (best <= good_ms)
				break;
		}
		if (best > worst_after) worst_after = best;
	}
	for (void *q : rejected)
		(void)hipFree(q);
	self->d_bins = self->d_bins_pp[cur_set];
	self->d_partial = self->d_partial_pp[cur_set];
	if (us_before) *us_before = worst_before * 1e3f;
	if (us_after) *us_after = worst_after * 1e3f;
	return reallocs;
}

/* N = 8192: how many FFT launches ran in the space-sharing form (share_cus work-groups, beside the previous launch's count / merge
 * kernels) and how many took every CU, since the instance was made; cus = the shared form's work-group count (0: this device never
 * shares).  The form is chosen from the state of the queue at submit time, so two runs of the same calls may differ here -- never in
 * their results. */
extern "C" int fosphor_amd_share_stats(struct fosphor *self, long long *shared, long long *full, int *cus)
{
	if (!self)
		return -EINVAL;
	if (shared) *shared = self->k1w_shared;
	if (full) *full = self->k1w_full;
	if (cus) *cus = self->share_cus;
	return 0;
}

/* What the calls so far launched, since the instance was made: FFT pieces of fosphor_amd_accumulate_device[_overlap] (1 per call on
 * the single-launch path, one per sub-launch otherwise), chunk sums over 16-bit slabs (k2c_sum) and chunk reduces beside 32-bit
 * counts (k2b_reduce), the latter two by any entry point.  Host counters that only grow; nothing on the submit path reads them. */
extern "C" int fosphor_amd_launch_stats(struct fosphor *self, long long *pieces, long long *k2c, long long *k2b)
{
	if (!self)
		return -EINVAL;
	if (pieces) *pieces = self->acc_pieces;
	if (k2c) *k2c = self->n_k2c;
	if (k2b) *k2b = self->n_k2b;
	return 0;
}

/* Merge launches since the instance was made, by the form launch_k3 chose (k3_form): stats[0..6] in the order of K3Form, stats[7] =
 * how many of the long-batch launches (forms 1, 2, 6) read the (d, e) table from memory, stats[8] / stats[9] = the most batches one
 * launch of form 5 / form 6 merged, stats[10] = the rows the last sparse launch listed (read back from the device behind that launch;
 * -1: none yet).  The others are host counters that only grow; nothing on the submit path reads them. */
extern "C" int fosphor_amd_merge_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_MERGE_STATS])
{
	if (!self)
		return -EINVAL;
	if (!stats)
		return 0;
	for (int i = 0; i < K3_FORMS; i++)
		stats[i] = self->k3_forms[i];
	stats[FOSPHOR_AMD_MERGE_TABLE_IN_MEMORY] = self->k3_rise_mem;
	stats[FOSPHOR_AMD_MERGE_SPARSE_MAX_BATCHES] = self->k3_sparse_max[0];
	stats[FOSPHOR_AMD_MERGE_SPARSE_LONG_MAX_BATCHES] = self->k3_sparse_max[1];
	stats[FOSPHOR_AMD_MERGE_SPARSE_LISTED_ROWS] = -1;
	if (self->k3_listed) {
		/* (the word stays as the launch left it until the scan after the next one zeroes it: k3_scan) */
		uint32_t listed = 0;
		if (hipMemcpyAsync(&listed, self->k3_listed, sizeof(listed), hipMemcpyDeviceToHost, self->k3_listed_stream) != hipSuccess ||
		    hipStreamSynchronize(self->k3_listed_stream) != hipSuccess)
			return -EIO;
		stats[FOSPHOR_AMD_MERGE_SPARSE_LISTED_ROWS] = listed;
	}
	return 0;
}

extern "C" void *fosphor_amd_stream(struct fosphor *self)
{
	return self ? (void *)self->stream : NULL;
}

extern "C" void *fosphor_amd_upload_stream(struct fosphor *self)
{
	return self ? (void *)(self->copy_stream ? self->copy_stream : self->stream) : NULL;
}

/* private accessor for fosphor_render.cpp (keeps struct fosphor opaque there) */
extern "C" void fosphor_amd_priv_ranges(struct fosphor *self, int *db_ref, int *db_per_div,
                                        double *center, double *span)
{
	*db_ref = self->power.db_ref;
	*db_per_div = self->power.db_per_div;
	*center = self->frequency.center;
	*span = self->frequency.span;
}

/* private accessors for fosphor_cmap.hip */
extern "C" int fosphor_amd_priv_palette(struct fosphor *self, int n, uint32_t **d_palette)
{
	if (!self->d_palette && hipMalloc((void **)&self->d_palette, sizeof(uint32_t) * n) != hipSuccess)
		return -EIO;
	*d_palette = self->d_palette;
	return 0;
}

extern "C" void fosphor_amd_priv_power(struct fosphor *self, float *scale, float *offset)
{
	*scale = self->power.scale;
	*offset = self->power.offset;
}

/* The scratch buffers that only grow, by FOSPHOR_SCRATCH_* (fosphor_pass.h): one each for fosphor_detect.hip and fosphor_mask.hip (of a
 * size fixed for the life of the instance: allocated on first use, never again), the two of fosphor_burst.hip, and one each for the
 * job tables and partials of fosphor_extract / _measure / _demod / _correlate / _resample.hip.  Every user has drained the stream of the
 * launches that used the old buffer before it asks for a larger one. */
extern "C" int fosphor_amd_priv_scratch(struct fosphor *self, int which, size_t bytes, void **d_scratch)
{
	if (which < 0 || which >= FOSPHOR_SCRATCH_COUNT)
		return -EINVAL;
	if (bytes > self->scratch[which].cap) {
		(void)hipFree(self->scratch[which].d);
		self->scratch[which].d = nullptr;
		self->scratch[which].cap = 0;
		if (hipMalloc(&self->scratch[which].d, bytes) != hipSuccess)
			return -EIO;
		self->scratch[which].cap = bytes;
	}
	*d_scratch = self->scratch[which].d;
	return 0;
}

/* the counters of pass `which` (FOSPHOR_COUNTERS_*, fosphor_pass.h); nothing on the submit path reads them */
extern "C" long long *fosphor_amd_priv_counters(struct fosphor *self, int which)
{
	return self->counters[which];
}

/* what every public fosphor_amd_*_stats does with its pass's counters */
extern "C" int fosphor_amd_priv_copy_stats(struct fosphor *self, int which, int n, long long *stats)
{
	if (!self || which < 0 || which >= FOSPHOR_COUNTERS_COUNT || n < 0 || n > FOSPHOR_COUNTERS_MAX)
		return -EINVAL;
	if (stats)
		memcpy(stats, self->counters[which], sizeof(long long) * n);
	return 0;
}

/* the format that -1 stands for in fosphor_amd_extract */
extern "C" int fosphor_amd_priv_iq_format(struct fosphor *self)
{
	return self->iq_format;
}

/* ------------------------------------------------------------------------ */
/* Host-side tables (no GPU)                                                */
/* ------------------------------------------------------------------------ */

extern "C" int fosphor_amd_host_thresholds(int n_bins, float histo_scale, float histo_offset, double *out)
{
	if (!out || n_bins < 2 || n_bins > 65536)
		return -EINVAL;
	build_thresholds(out, n_bins, histo_scale, histo_offset);
	return 0;
}


extern "C" int fosphor_amd_host_twiddle_count(void) { return build_twiddles(NULL, 10, NULL); }

extern "C" int fosphor_amd_host_twiddles(float *out)
{
	if (!out)
		return -EINVAL;
	build_twiddles((float2 *)out, 10, NULL);
	return 0;
}

/* debug: copy the K1 phase-timing accumulators (K1_TIMING builds) to the host */
extern "C" int fosphor_amd_debug_k1_timing(struct fosphor *self, long long *out, int n)
{
	if (!self || !self->d_dbg || !out || n > 16 * 4 * kK1MaxBlocks)
		return -EINVAL;
	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	return hipMemcpy(out, self->d_dbg, sizeof(long long) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -EIO;
}

/* Two-stream pipelining of the process paths on (1, default) or off (0: K1, K2, K3 in order on
 * one stream).  Drains queued work first.  Results are identical either way. */
extern "C" int fosphor_amd_set_overlap(struct fosphor *self, int enable)
{
	if (!self)
		return -EINVAL;
	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	self->overlap = enable ? 1 : 0;
	/* (everything queued has finished: nothing is left to wait for) */
	for (int i = 0; i < kSets; i++)
		self->f.set_free[i].recorded = 0;
	self->f.h_free[0].recorded = self->f.h_free[1].recorded = 0;
	return 0;
}

/* strict = 1 (default): a device-resident call behaves like work queued on `stream`: its K1s start after what
 * the caller queued there before the call, and what the caller queues there afterwards starts after them.
 * strict = 0: no ordering against `stream` in either direction (the caller guarantees the samples are complete
 * before the call and keeps them until fosphor_amd_finish() or fosphor_amd_wait_input()); consecutive calls then
 * overlap at their edges like the sub-launches inside one call. */
extern "C" int fosphor_amd_set_input_ordering(struct fosphor *self, int strict)
{
	if (!self)
		return -EINVAL;
	self->relaxed = strict ? 0 : 1;
	return 0;
}

/* Makes `stream` wait for every K1 queued so far (the readers of the callers' sample buffers). */
extern "C" int fosphor_amd_wait_input(struct fosphor *self)
{
	if (!self)
		return -EINVAL;
	return k1_streams_join(self);
}

/* The stream K2 / K3 run on: a second stream when the two-stream pipeline is on, else the main
 * one.  A multi-GPU caller enqueues its all-reduce of the partial arrays relative to THIS stream
 * (after fosphor_amd_accumulate_device, before fosphor_amd_merge). */
extern "C" void *fosphor_amd_stream2(struct fosphor *self)
{
	return self ? (void *)count_stream(self) : NULL;
}
