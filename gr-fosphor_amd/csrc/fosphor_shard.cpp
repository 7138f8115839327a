/*
 * fosphor_shard.cpp -- the multi-GPU split of libfosphor_amd.so: a time shard of a display frame accumulated into partial arrays,
 * their exchange (RCCL, fosphor_exchange.cpp; the compact wire formats, fosphor_wire.hip) and the merge of the sum.  The launches
 * themselves are the pipeline's (fosphor_api.cpp, through fosphor_instance.h).
 */
#include <errno.h>

#include "fosphor_instance.h"

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
static void xprof_begin(struct fosphor *self, hipStream_t st) { if (self->prof) self->timers[TIMER_EXCHANGE].begin(0, st); }
static void xprof_end(struct fosphor *self, hipStream_t st) { self->timers[TIMER_EXCHANGE].end(st); }

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
	EventTimer &t = self->timers[TIMER_WIRE + kind];
	if (end) t.end(st);
	else if (self->prof) { t.reset(); t.begin(kind, st); }
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
