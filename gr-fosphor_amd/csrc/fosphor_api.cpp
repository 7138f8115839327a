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
 *
 * This file: the instance and the K1 -> K2 -> K3 pipeline.  struct fosphor is in fosphor_instance.h; the host tables, the
 * sharded-frame path and the measurement hooks are in fosphor_tables.cpp, fosphor_shard.cpp and fosphor_prof.cpp.
 */
#include <assert.h>
#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "fosphor_instance.h"
#include "../../include/fosphor_amd_sink.h"
#include "../../include/fosphor_portable_math.h"

#define FOSPHOR_AMD_VERSION "fosphor_amd 0.1 gfx950"

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

unsigned fosphor_amd::dep_event_flags(void)
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
	for (EventTimer &t : self->timers) t.destroy();
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

/* The stream K2 / K3 and the exchanges run on: a second stream when the two-stream pipeline is on, else the main one */
hipStream_t fosphor_amd::count_stream(const struct fosphor *self)
{
	return self->overlap ? self->stream2 : self->stream;
}

int fosphor_amd::sync_all(struct fosphor *self)
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
int fosphor_amd::k3_stream_enter(struct fosphor *self, hipStream_t st)
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
int fosphor_amd::drain_h_sets(struct fosphor *self, hipStream_t st)
{
	for (int h = 0; h < 2; h++) {
		if (self->f.h_free[h].wait(st) != hipSuccess)
			return -EIO;
		self->f.h_free[h].recorded = 0;
	}
	return 0;
}

/* Upload lazily-changed tables (cl.c:889-900) and boot fills (cl.c:406-465, 930-934) */
int fosphor_amd::prepare(struct fosphor *self)
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
int fosphor_amd::pick_tile(const struct fosphor *self, int total, int batch)
{
	assert(self->log2n != 13 || batch % 16 == 0);	/* (every entry point asks for it: the fallback tile of 8 divides the batch) */
	return k1_plan(k1_shape(self, NULL, 0, total, batch, 0)).tile;
}

void fosphor_amd::fill_k1(struct fosphor *self, K1Params *k1, const void *d_iq, int total, int tile,
                          int wf_pos0, int wf_first, int hop)
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
struct fosphor_amd_count_plan fosphor_amd::plan_count(const struct fosphor *self, int n_batches, int batch, int pipelined)
{
	return ::plan_count(self->log2n, self->n_bins, self->slab_chunks, self->kn_rowmask_off, self->kn_no_sum16, n_batches, batch, pipelined);
}

/* The count-kernel fields every K2 launch sets alike: `total` spectra of the current set's bin indices / tile partials in batches of
 * `batch`, counted `chunk` spectra per work-group; the first of them is spectrum t_offset of a batch of weight_batch (live-sum weights) */
void fosphor_amd::fill_k2(const struct fosphor *self, K2Params *k2, int total, int batch, int chunk, int tile, int t_offset, int weight_batch)
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
hipError_t fosphor_amd::launch_chunk_sum(struct fosphor *self, int n_batches, int cpb, int slot0, int lslot, int sum16, hipStream_t st)
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
int fosphor_amd::run_count(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int tile, int slot0,
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

int fosphor_amd::run_merge(struct fosphor *self, const struct fosphor_amd_count_plan &plan, int n_batches, int batch, int slot0, int hset,
                           hipStream_t st, int cell_begin, int cell_end)
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
int fosphor_amd::k1_streams_fork(struct fosphor *self)
{
	if (self->f.in.record(self->stream) != hipSuccess)
		return -EIO;
	for (int i = 1; i < self->n_k1_streams; i++)
		if (self->f.in.wait(self->k1_streams[i]) != hipSuccess)
			return -EIO;
	return 0;
}

/* ... and what the caller queues on `stream` next follows every K1 queued on them */
int fosphor_amd::k1_streams_join(struct fosphor *self)
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
int fosphor_amd::k1_piece(struct fosphor *self, hipStream_t ks, const void *d_iq, int t, int sub_total, int tile, int first_row, int hop)
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
int fosphor_amd::k1_set_release(struct fosphor *self, int set)
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
int fosphor_amd::device_call_ok(const struct fosphor *self, const void *d_samples, long long spectra, int overlap)
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
 * job tables and partials of fosphor_extract / _measure / _demod / _correlate / _resample / _psd / _symbols / _carrier / _decide / _decode.hip.  Every user has drained the stream of the
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
