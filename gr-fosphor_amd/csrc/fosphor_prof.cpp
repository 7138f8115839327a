/*
 * fosphor_prof.cpp -- the measurement hooks of libfosphor_amd.so: the event-pair timer behind every profiling read-out, the kernel,
 * exchange and wire-kernel times, the traffic twin and placement tuning, the launch statistics, the debug timers.  Nothing here is
 * on the submit path.
 */
#include <errno.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fosphor_instance.h"

/* The event-pair timer (fosphor_instance.h) */
void EventTimer::begin(int t, hipStream_t st)
{
	open = 0;
	while (ev.size() < 2 * n + 2) {
		hipEvent_t e;
		if (hipEventCreateWithFlags(&e, dep_event_flags() & ~hipEventDisableTiming) != hipSuccess) return;
		ev.push_back(e);
	}
	tag.resize(ev.size() / 2);
	tag[n] = t;
	open = hipEventRecord(ev[2 * n], st) == hipSuccess;
}

void EventTimer::end(hipStream_t st)
{
	if (open && hipEventRecord(ev[2 * n + 1], st) == hipSuccess) n++;
	open = 0;
}

void EventTimer::destroy()
{
	for (hipEvent_t e : ev) (void)hipEventDestroy(e);
	ev.clear();
	reset();
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
	EventTimer &timer = self->timers[TIMER_KERNELS];
	for (size_t i = 0; i < timer.n; i++) {
		float t = 0.0f;
		int kind = timer.tag[i];
		if (timer.ms(i, &t)) {
			ms[kind] += t;
			launches[kind]++;
		}
	}
	timer.reset();
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
	const EventTimer &timer = self->timers[TIMER_KERNELS];
	for (int kind = 0; kind < 3; kind++) {
		std::vector<std::pair<float, float> > iv;
		for (size_t i = 0; i < timer.n; i++) {
			float a = 0.0f, b = 0.0f;
			if (timer.tag[i] != kind)
				continue;
			if (hipEventElapsedTime(&a, timer.ev[0], timer.ev[2 * i]) != hipSuccess ||		/* (from the first recorded start) */
			    hipEventElapsedTime(&b, timer.ev[0], timer.ev[2 * i + 1]) != hipSuccess)
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

/* Sum of the durations of the exchanges recorded since the last call (hipEvents on the count/merge stream around the
 * ncclGroup), and how many there were; resets.  0 exchanges when profiling was off. */
extern "C" int fosphor_amd_exchange_time(struct fosphor *self, float *ms_total, int *count)
{
	if (!self || !ms_total || !count)
		return -EINVAL;
	if (sync_all(self))
		return -EIO;
	*ms_total = 0.0f; *count = 0;
	EventTimer &timer = self->timers[TIMER_EXCHANGE];
	for (size_t i = 0; i < timer.n; i++) {
		float t = 0.0f;
		if (timer.ms(i, &t)) {
			*ms_total += t;
			(*count)++;
		}
	}
	timer.reset();
	return 0;
}

extern "C" int fosphor_amd_wire_kernel_times(struct fosphor *self, float ms[3])
{
	if (!self || !ms)
		return -EINVAL;
	if (hipStreamSynchronize(count_stream(self)) != hipSuccess)
		return -EIO;
	for (int k = 0; k < 3; k++) {
		const EventTimer &timer = self->timers[TIMER_WIRE + k];	/* (reset before each launch: at most the last one's pair) */
		ms[k] = -1.0f;
		if (timer.n && !timer.ms(0, &ms[k]))
			ms[k] = -1.0f;
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

/* debug: copy the K1 phase-timing accumulators (K1_TIMING builds) to the host */
extern "C" int fosphor_amd_debug_k1_timing(struct fosphor *self, long long *out, int n)
{
	if (!self || !self->d_dbg || !out || n > 16 * 4 * kK1MaxBlocks)
		return -EINVAL;
	if (fosphor_amd_finish(self) < 0)
		return -EIO;
	return hipMemcpy(out, self->d_dbg, sizeof(long long) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -EIO;
}
