/*
 * fosphor_amd_extract.h -- burst IQ at baseband: a batched mix, FIR and decimate over IQ that is already in device memory
 *
 * fosphor_amd_detect, fosphor_amd_mask_scan and fosphor_amd_bursts say where and when an emission is.  This pass hands out its
 * samples: every job of a call is one digital down-converter run -- its own time range, centre frequency, decimation and real
 * low-pass -- over the caller's device-resident IQ stream, and leaves float32 (re, im) pairs in a device buffer.  A burst is a few
 * columns of N and a few rows of the ring, so its baseband IQ is orders of magnitude fewer bytes than the stream it came from; the
 * stream itself never crosses to the host.  The library owns no IQ ring: the caller keeps the samples, as with
 * fosphor_amd_process_device, and says which sample a ring row began at (fosphor_amd_extract_from_burst).
 *
 * Conventions, those of fosphor_amd_mask.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided before anything is written or launched; -EIO is a device error.  It is the first pass of the family
 * that reads samples, not power: the three IQ formats are widened exactly where they are loaded, as the FFT kernels widen them.
 */
#ifndef FOSPHOR_AMD_EXTRACT_H
#define FOSPHOR_AMD_EXTRACT_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_burst.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_EXTRACT_MAX_JOBS   4096
#define FOSPHOR_AMD_EXTRACT_MAX_DECIM  1024
#define FOSPHOR_AMD_EXTRACT_MAX_TAPS   8192

struct fosphor_amd_extract_job
{
	int64_t  first;		/* s0: index into d_samples of the first input sample the job reads */
	int64_t  out_offset;	/* index into d_out (complex samples) of its first output */
	int32_t  n_out;		/* outputs to write, >= 0 (0: the job writes nothing) */
	int32_t  decim;		/* D, 1 .. MAX_DECIM */
	uint32_t phase_inc;	/* NCO step per INPUT sample, cycles * 2^32 (two's complement: 0x80000000.. = negative frequencies) */
	uint32_t phase0;	/* NCO phase at input sample `first`, cycles * 2^32 */
	int32_t  taps_offset;	/* index into d_taps of h[0] */
	int32_t  n_taps;	/* T, 1 .. MAX_TAPS */
};

/* Run n_jobs jobs over d_samples.  jobs: HOST memory.  DEVICE memory:
 *   d_samples  n_samples samples in iq_format (a FOSPHOR_AMD_IQ_* value, or -1 for the instance's format; fp16 is allowed here
 *              at every FFT length, this pass does not depend on N), aligned to one sample: 8 B fp32, 4 B fp16 / sc16
 *   d_taps     n_taps_total float32 real taps, shared by the jobs through taps_offset / n_taps
 *   d_out      out_capacity float32 (re, im) pairs, 8-byte aligned
 *
 * 1. Contract   for output m of a job, with x widened exactly (sc16: i * 2^-15; fp16: exact), D = decim, T = n_taps:
 *                   n    = m * D + k
 *                   phi(n) = (phase0 + n * phase_inc) mod 2^32         exact unsigned 32-bit arithmetic, n truncated to 32 bits
 *                   y[m] = sum over k = 0 .. T - 1 of  h[k] * x[first + n] * exp(-2 pi i * phi(n) / 2^32)
 *               (a correlation with h as written: a symmetric low-pass does not care.)  The mode is "valid" only: first >= 0
 *               and, for n_out > 0, first + (n_out - 1) * D + T <= n_samples.
 * 2. Phase      phi is an integer on purpose: it depends on the sample's index alone, never on how a job is cut into tiles or
 *               into jobs.  A job of 64 outputs and the same job as two jobs of 32, the second with first advanced by 32 * D and
 *               phase0 by 32 * D * phase_inc, give bit-identical outputs.  The angle (int32_t) phi * 2^-31 half-turns is reduced
 *               exactly and evaluated with a full-precision sincospi; the mixer's sine and cosine are within 4 * 2^-24.
 * 3. Sum        float32, explicit fmaf, no float atomics: the same call repeated gives bit-identical output.  The form that
 *               computes a job is chosen from (D, T) alone (below); within a form the order of the sum is fixed, so a job's
 *               outputs do not depend on the other jobs of the call.  The TILE form sums k = 0 .. T - 1 in order; the WAVE form
 *               sums the taps k = l, l + 64, ... in lane l and reduces the 64 lanes by xor-shuffles 32, 16, .. 1.  The two forms'
 *               sums need NOT equal each other bit for bit; both are within (T + 16) * 2^-24 * sum|h[k]| * max|x| per component
 *               of the exact value.
 * 4. Writes     only d_out[out_offset .. out_offset + n_out) of each job.  The output ranges of two jobs must not overlap
 *               (checked on the host, by sorting, before anything is launched); the input ranges may.
 * 5. Launches   one per form present in the call, whatever the number of jobs.
 *
 * 0; -EINVAL (nothing is written or launched): a NULL self / d_samples / jobs / d_taps / d_out; n_jobs outside 1 .. MAX_JOBS;
 * n_samples, n_taps_total or out_capacity below 0; a job with first < 0, out_offset < 0, n_out < 0, decim outside 1 .. MAX_DECIM,
 * n_taps outside 1 .. MAX_TAPS, taps outside [0, n_taps_total), reading outside [0, n_samples) (n_out > 0), writing outside
 * [0, out_capacity) or over another job's outputs; an iq_format that is none of -1, 0, 1, 2; d_samples not aligned to one sample,
 * d_out not to 8 bytes, d_taps not to 4; a call of more than 2^31 - 1 work-groups in one form.  -EIO. */
int fosphor_amd_extract(struct fosphor *self, const void *d_samples, int64_t n_samples, int iq_format,
                        const struct fosphor_amd_extract_job *jobs, int n_jobs,
                        const float *d_taps, int n_taps_total,
                        void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers; iq_format must be 0, 1 or 2.  The sum is taken
 * in double, with sin / cos of 2 pi phi / 2^32 in double, k ascending, and rounded once to float32.
 * 0; -EINVAL: what the device entry point refuses (but for self), iq_format -1. */
int fosphor_amd_extract_host(const void *samples, int64_t n_samples, int iq_format,
                             const struct fosphor_amd_extract_job *jobs, int n_jobs,
                             const float *taps, int n_taps_total,
                             float *out, int64_t out_capacity);

/* HOST only: a Hamming-windowed sinc low-pass of n_taps taps for decimation decim.  With fc = guard / (2 * decim) cycles per sample
 * (0 < guard <= 1), c = (n_taps - 1) / 2 and, for k = 0 .. n_taps - 1,
 *     t    = k - c
 *     s[k] = 2 * fc                          where t == 0
 *            sin(2 * pi * fc * t) / (pi * t)   elsewhere
 *     w[k] = 0.54 - 0.46 * cos(2 * pi * k / (n_taps - 1))          (1 when n_taps == 1)
 *     g[k] = s[k] * w[k]
 * all in double; g[k] is computed for k <= c and mirrored (g[n_taps - 1 - k] = g[k]), so h is symmetric to the bit;
 * out[k] = (float)(g[k] / sum of g in ascending k): the taps sum to 1 before rounding.
 * 0; -EINVAL: decim outside 1 .. MAX_DECIM, n_taps outside 1 .. MAX_TAPS, guard not in (0, 1], a NULL out. */
int fosphor_amd_extract_design(int decim, int n_taps, double guard, float *out);

/* HOST only: the job that extracts a burst.  newest_first_sample is the index in the caller's stream of the first sample of the
 * spectrum that ring row j = 0 holds, row_hop the samples between the spectra of consecutive rows: only the caller knows them
 * (fosphor_amd_burst.h, the dead-store rule).
 *     first     = newest_first_sample - oldest * row_hop
 *     length    = (oldest - newest) * row_hop + fft_len                  the input samples of the burst's rows
 *     centre    = ((first_col + last_col + 1) / 2 - fft_len / 2) / fft_len   cycles per sample, in double; phase_inc is centre * 2^32
 *                 rounded to the nearest integer (ties away from zero), mod 2^32
 *     decim     = the largest D <= min(max_decim, MAX_DECIM) with (last_col - first_col + 1) * D <= guard * fft_len, and 1 when
 *                 there is none
 *     n_taps    = *n_taps_wanted = 8 * D + 1
 *     n_out     = the largest value that keeps the job "valid" inside `length`: (length - n_taps) / D + 1, or 0 when
 *                 length < n_taps
 *     phase0 = 0, out_offset = 0, taps_offset = 0: the caller places the job.
 * 0; -EINVAL: a NULL pointer; fft_len below 2 or no power of two; row_hop or max_decim below 1; guard not in (0, 1]; a record
 * with newest < 0, oldest < newest, first_col < 0, last_col >= fft_len or first_col > last_col; first < 0. */
int fosphor_amd_extract_from_burst(const struct fosphor_amd_burst *b, int fft_len, int64_t newest_first_sample, int row_hop,
                                   int max_decim, double guard, struct fosphor_amd_extract_job *job, int *n_taps_wanted);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_EXTRACT_CALLS]      fosphor_amd_extract calls that reached the device
 *   stats[FOSPHOR_AMD_EXTRACT_K_TILE]     launches of the TILE kernel
 *   stats[FOSPHOR_AMD_EXTRACT_K_WAVE]     launches of the WAVE kernel
 *   stats[FOSPHOR_AMD_EXTRACT_JOBS_TILE]  jobs of those calls in the TILE form (n_out = 0 included)
 *   stats[FOSPHOR_AMD_EXTRACT_JOBS_WAVE]  ... in the WAVE form
 *   stats[FOSPHOR_AMD_EXTRACT_SAMPLES]    input samples those jobs span: the sum of (n_out - 1) * D + T over the jobs with n_out > 0 */
enum {
	FOSPHOR_AMD_EXTRACT_CALLS, FOSPHOR_AMD_EXTRACT_K_TILE, FOSPHOR_AMD_EXTRACT_K_WAVE, FOSPHOR_AMD_EXTRACT_JOBS_TILE,
	FOSPHOR_AMD_EXTRACT_JOBS_WAVE, FOSPHOR_AMD_EXTRACT_SAMPLES,
	FOSPHOR_AMD_EXTRACT_STATS
};
int fosphor_amd_extract_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_EXTRACT_STATS]);

/* The forms.  TILE: a work-group owns FOSPHOR_AMD_EXTRACT_TILE_OUT consecutive outputs of a job and keeps their mixed input span
 * in LDS, as D rows of R = (TILE_OUT + (T - 1) / D + 1) | 1 samples; a job is in the TILE form when D * R <=
 * FOSPHOR_AMD_EXTRACT_TILE_LDS.  WAVE: every other job; a wave owns one output and a work-group FOSPHOR_AMD_EXTRACT_WAVE_OUT.
 * Tests plant job lengths and decimations across those seams. */
#define FOSPHOR_AMD_EXTRACT_TILE_OUT 256
#define FOSPHOR_AMD_EXTRACT_TILE_LDS 6656
#define FOSPHOR_AMD_EXTRACT_WAVE_OUT 4

#ifdef __cplusplus
}
#endif

#endif
