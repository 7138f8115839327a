/*
 * fosphor_instance.h -- struct fosphor and what the host files around it share: fosphor_api.cpp (the instance and the K1 -> K2 -> K3
 * pipeline), fosphor_shard.cpp (sharded frames), fosphor_prof.cpp (measurement), fosphor_tables.cpp (host tables).  Nothing else
 * includes it: the passes in files of their own go through fosphor_pass.h.
 */
#ifndef FOSPHOR_INSTANCE_H
#define FOSPHOR_INSTANCE_H

#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "fosphor_internal.h"
#include "fosphor_pass.h"
#include "../../include/fosphor_amd.h"
#include "../../include/fosphor_amd_wire.h"

using namespace fosphor_amd;		/* (the launch wrappers and parameter blocks of fosphor_internal.h) */

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

/* (start, stop) pairs of timing events around launches, each pair with a tag; the events are created on first use and used again
 * after reset().  One rule for every failure, hipEventCreate or hipEventRecord, start or stop: that launch goes untimed -- only a
 * pair whose two records both succeeded is counted, so no half-recorded pair is ever read.  (Bodies: fosphor_prof.cpp.) */
struct EventTimer
{
	std::vector<hipEvent_t> ev;		/* pair i < n is ev[2 i] (start), ev[2 i + 1] (stop) ... */
	std::vector<int> tag;			/* ... and has tag[i] */
	size_t n;				/* completed pairs: what a reader walks */
	int    open;				/* begin() recorded the start of pair n; end() has not yet recorded its stop */

	void begin(int tag, hipStream_t st);
	void end(hipStream_t st);		/* (no-op unless open) */
	bool ms(size_t i, float *out) const { return hipEventElapsedTime(out, ev[2 * i], ev[2 * i + 1]) == hipSuccess; }
	void reset() { n = 0; open = 0; }	/* forget the pairs, keep the events */
	void destroy();
};
/* an instance's timers: the K1 / K2 / K3 launches (tag = kernel), the exchanges, the last launch of wire kernel 0 mask, 1 pack, 2 unpack */
enum { TIMER_KERNELS, TIMER_EXCHANGE, TIMER_WIRE /* + kind */, TIMER_COUNT = TIMER_WIRE + 3 };

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
	EventTimer timers[TIMER_COUNT];		/* by TIMER_*; nothing is recorded while prof is 0 */
};

namespace fosphor_amd {

/* fosphor_tables.cpp */
int build_twiddles(float2 *tw, int log2n, int *offsets /* [8] or NULL */);
void build_thresholds(double *thr, int nb, float hs, float ho);

/* fosphor_api.cpp: streams and fences */
unsigned dep_event_flags(void);
hipStream_t count_stream(const struct fosphor *self);
int sync_all(struct fosphor *self);
int k3_stream_enter(struct fosphor *self, hipStream_t st);
int drain_h_sets(struct fosphor *self, hipStream_t st);
int k1_streams_fork(struct fosphor *self);
int k1_streams_join(struct fosphor *self);
/* ... the launch sequence */
int prepare(struct fosphor *self);
int device_call_ok(const struct fosphor *self, const void *d_samples, long long spectra, int overlap);
int pick_tile(const struct fosphor *self, int total, int batch);
void fill_k1(struct fosphor *self, K1Params *k1, const void *d_iq, int total, int tile, int wf_pos0, int wf_first, int hop = 0);
void fill_k2(const struct fosphor *self, K2Params *k2, int total, int batch, int chunk, int tile, int t_offset, int weight_batch);
struct fosphor_amd_count_plan plan_count(const struct fosphor *self, int n_batches, int batch, int pipelined);
int k1_piece(struct fosphor *self, hipStream_t ks, const void *d_iq, int t, int sub_total, int tile, int first_row, int hop);
int k1_set_release(struct fosphor *self, int set);
hipError_t launch_chunk_sum(struct fosphor *self, int n_batches, int cpb, int slot0, int lslot, int sum16, hipStream_t st);
int run_count(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int tile, int slot0,
              int hset, int t_offset, int weight_batch, hipStream_t st);
int run_merge(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int slot0, int hset,
              hipStream_t st, int cell_begin = 0, int cell_end = 0);

} // namespace fosphor_amd

/* The kernels' timer around a launch of kernel `kind` (0 K1, 1 K2, 2 K3); prof == 2: K1 only.  Profiling off: one branch each. */
static inline void prof_begin(struct fosphor *self, int kind, hipStream_t st)
{
	if (self->prof && (self->prof != 2 || kind == 0)) self->timers[TIMER_KERNELS].begin(kind, st);
}
static inline void prof_end(struct fosphor *self, hipStream_t st)
{
	if (self->timers[TIMER_KERNELS].open) self->timers[TIMER_KERNELS].end(st);
}

#endif
