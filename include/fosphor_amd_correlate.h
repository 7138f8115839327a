/*
 * fosphor_amd_correlate.h -- is this burst the thing I am looking for, and at which sample does it start: a sliding correlation
 * of burst IQ against a known sequence, one record and optionally one trace per job
 *
 * fosphor_amd_extract leaves each emission's baseband IQ in a device buffer, fosphor_amd_measure reduces it to a few numbers and
 * fosphor_amd_demod gives its traces.  This pass is the matched filter: every job of a call is one range of float32 (re, im) pairs
 * y and one template t of T such pairs, both in device memory, and gets, for every lag k at which the template fits inside the
 * range ("valid" mode, k = 0 .. n - T), the correlation c[k], the window's energy E[k] and the normalised rho[k] = |c|^2 / (E Et),
 * which is 1 where the window is a complex multiple of the template and near T^-1 in noise.  The record holds the peak and the lags
 * above a threshold; the trace, if asked for, holds rho or c per lag.  Preamble and sync-word search, pulse compression of a chirp
 * and the time of arrival of one capture against another are this one operation.  It is the step of the chain with arithmetic in
 * it, n_lags * T complex multiply-adds per job, all of it in double: the device runs it on its fp64 fused multiply-add.
 *
 * Not this pass: a per-job derotator (a carrier offset inside the burst costs correlation gain; remove it by extracting at the
 * corrected centre, fosphor_amd_measure_derive's freq_offset), sub-sample interpolation of the peak, and FFT-based correlation
 * for templates beyond FOSPHOR_AMD_CORRELATE_MAX_TPL samples.  A signal at another sample rate than the template's is brought to
 * it first, on the device, by fosphor_amd_resample (fosphor_amd_resample.h); it is no longer a step for the host.
 *
 * Conventions, those of fosphor_amd_measure.h and fosphor_amd_demod.h: the device entry point waits for pending fosphor_process
 * work first (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of
 * the instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_CORRELATE_H
#define FOSPHOR_AMD_CORRELATE_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_demod.h"
#include "fosphor_amd_extract.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_CORRELATE_MAX_JOBS 4096
#define FOSPHOR_AMD_CORRELATE_MAX_TPL  1024	/* template samples of a job */
#define FOSPHOR_AMD_CORRELATE_TILE     1024	/* lags of a work-group (rule 4); tests plant lag counts across this seam */

#define FOSPHOR_AMD_CORRELATE_TRACE_NONE 0	/* the record only */
#define FOSPHOR_AMD_CORRELATE_TRACE_RHO  1	/* one float32 per lag:  rho[k]                         n_out = n_lags */
#define FOSPHOR_AMD_CORRELATE_TRACE_C    2	/* two float32 per lag: (float)Re c[k], (float)Im c[k]  n_out = 2 * n_lags */

struct fosphor_amd_correlate_job		/* 40 bytes */
{
	int64_t offset;		/* index into d_iq  (complex samples) of y[0] */
	int64_t out_offset;	/* index into d_out (floats) of the trace; must be 0 with TRACE_NONE */
	int64_t tpl_offset;	/* index into d_tpl (complex samples) of t[0] */
	int32_t n;		/* input samples, >= 0 */
	int32_t tpl_len;	/* T, 1 .. MAX_TPL */
	int32_t trace;		/* FOSPHOR_AMD_CORRELATE_TRACE_* */
	float   threshold;	/* on rho (rule 3); +inf and negative values allowed, NaN refused */
};

struct fosphor_amd_correlate_record		/* 64 bytes, 8-byte aligned */
{
	int32_t n_lags;				/* max(n - T + 1, 0) */
	int32_t n_above;			/* lags k with above(k) */
	int32_t first_above, last_above;	/* the smallest and the largest such k; -1 when none */
	int32_t n_edges;			/* k with above(k) && (k == 0 || !above(k - 1)) */
	int32_t peak_lag;			/* rule 3; -1 when no lag has a non-NaN rho */
	float   peak_rho;			/* 0.0f then */
	int32_t tpl_len;			/* the job's T */
	double  peak_c_re, peak_c_im;		/* c at peak_lag (0 when none) */
	double  peak_energy;			/* E at peak_lag (0 when none) */
	double  tpl_energy;			/* Et */
};

/* Correlate n_jobs ranges of d_iq against n_jobs ranges of d_tpl.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract writes
 *   d_tpl      n_tpl such pairs, 8-byte aligned.  It may lie inside d_iq's buffer: one burst is correlated against another
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity floats, 4-byte aligned; job j owns d_out[out_offset .. out_offset + n_out).  NULL, with capacity 0,
 *              when every job has TRACE_NONE
 * y[m] = d_iq[offset + m], m = 0 .. n - 1; t[i] = d_tpl[tpl_offset + i], i = 0 .. T - 1; re_ and im_ their parts as double.
 * The mode is "valid": lags k = 0 .. n_lags - 1, n_lags = max(n - T + 1, 0).
 *
 * Every output -- each trace float and the whole record -- is BIT-IDENTICAL between the device, fosphor_amd_correlate_host and the
 * numpy model (tests/correlate_model.py), and depends on its job alone: not on the other jobs, not on the tiles, not on how a job
 * is cut (rule 4).
 *
 * 1. Sums       c[k] = sum over i < T of y[k + i] conj(t[i]), E[k] = sum over i < T of |y[k + i]|^2, Et = sum over i < T of
 *               |t[i]|^2.  Each is accumulated in double, i ascending, from 0.0, the additions in this fixed order:
 *                   cre += re_y * re_t;  cre += im_y * im_t;  cim += im_y * re_t;  cim -= re_y * im_t;
 *                   E   += re_y * re_y;  E   += im_y * im_y;       (Et the same over the template)
 *               Every product of two finite float32 values is exact in double (48 bits of product in 53, exponents far inside
 *               the range), so each addition is ONE rounding whether or not it is fused with its product: fma(a, b, s) of an exact
 *               a * b gives the bits of s + a * b.  The device's hot loop is fused multiply-adds; the host adds products; numpy
 *               multiplies, then adds.  A lag depends on its window and the template alone.  Non-finite inputs propagate as IEEE
 *               arithmetic does (inf * 0 is a NaN either way).
 * 2. rho        num = (cre * cre) + (cim * cim), den = E * Et, in double, three rounded operations, no contraction (the build's
 *               -ffp-contract=off).  rho = den == 0 ? 0 : num / den, rounded once to float32: rho32.  No clamp: the roundings may
 *               leave rho32 an ulp above 1.  Silence and an all-zero template give den == 0, hence rho = 0.  The TRACE_C floats
 *               are (float)cre and (float)cim.  A NaN float is the quiet NaN 0x7fc00000 whatever the payloads were (rule 3 of
 *               fosphor_amd_demod.h), and a NaN double of the record (tpl_energy of a template that holds a NaN or an infinity
 *               beside a zero) is 0x7ff8000000000000.
 * 3. Record     above(k) is rho32[k] >= threshold; a NaN is not above.  n_above, first_above, last_above and n_edges follow
 *               from `above` as in rule 2 of fosphor_amd_measure.h.  The peak is the largest non-NaN rho32, at the smallest lag
 *               that attains it; peak_c_* and peak_energy are c and E of that lag.  Everything in the record is exact or pinned
 *               by rules 1 and 2, so the whole record is bit-identical to the host's and the model's, whatever the tiling.
 *               A job with n_lags == 0 writes no trace; its record is zeros with the -1 indices, plus its tpl_len and tpl_energy.
 * 4. Cut rule   a job, and its two halves cut at lag c -- (offset, n = c + T - 1) and (offset + c, n - c) -- give the same trace
 *               values and the same per-lag facts, bit for bit: lag k of the second half is lag c + k of the whole.
 *               On the device a work-group of 256 lanes owns FOSPHOR_AMD_CORRELATE_TILE consecutive lags of one job, which it
 *               finds in a prefix of work-group counts by a bounded binary search; it brings y[k0 .. k0 + lags + T - 1) and the
 *               template into LDS with 16-byte loads from the first 16-byte boundary on (the single samples before that boundary
 *               and behind the last whole pair go one by one); lane i owns lags i, i + 256, i + 512, i + 768 of the tile and
 *               reuses each template value, one LDS broadcast, across them.  It stores its trace floats, consecutive lanes to
 *               consecutive addresses, and reduces its lags to one partial (counts, first, last, edges inside the tile, whether
 *               its first and last lag are above, the peak with c and E) by wave shuffles, then LDS in wave order.  A second
 *               kernel, one wave per job, folds the partials -- lane l takes tiles l, l + 64, .. in ascending order, then the
 *               64 lanes meet by xor-shuffles; the lane of tile c does not count the edge again where tile c - 1 ended above
 *               and tile c begins above -- and writes the record.  Every quantity folded is an integer, a minimum, a maximum
 *               or the (rho, lag) pair, so the order of the fold does not matter: no sum of doubles crosses a lane.  At most two launches per call, whatever the number of jobs; no
 *               atomics, no work-group waits for another, every loop carries its bound.
 * 5. Access     reads touch only d_iq[offset .. offset + n) and d_tpl[tpl_offset .. tpl_offset + T) of each job; writes only
 *               d_records[0 .. n_jobs) and each job's d_out[out_offset .. out_offset + n_out).  Input ranges may overlap, each
 *               other and the templates; output ranges must not.
 * 6. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, d_tpl, jobs or
 *               d_records; a NULL d_out while some job has a trace; n_jobs outside 1 .. MAX_JOBS; n_samples, n_tpl or
 *               out_capacity below 0; a job with offset, out_offset or tpl_offset < 0, n < 0, offset + n > n_samples, tpl_len
 *               outside 1 .. MAX_TPL, tpl_offset + tpl_len > n_tpl, an unknown trace, out_offset != 0 with TRACE_NONE, a NaN
 *               threshold, out_offset + n_out > out_capacity, or outputs over another job's; d_iq, d_tpl or d_records not 8-byte
 *               aligned; d_out not 4-byte aligned; more than 2^31 - 1 work-groups.  Every check is safe against offsets of 2^62.
 *
 * 0; -EINVAL (rule 6); -EIO. */
int fosphor_amd_correlate(struct fosphor *self, const void *d_iq, int64_t n_samples,
                          const void *d_tpl, int64_t n_tpl,
                          const struct fosphor_amd_correlate_job *jobs, int n_jobs,
                          struct fosphor_amd_correlate_record *d_records,
                          float *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_correlate_host(const float *iq, int64_t n_samples, const float *tpl, int64_t n_tpl,
                               const struct fosphor_amd_correlate_job *jobs, int n_jobs,
                               struct fosphor_amd_correlate_record *records, float *out, int64_t out_capacity);

/* HOST only: n_out of a job (0, n_lags or 2 * n_lags), or -EINVAL: an unknown trace, n < 0, tpl_len outside 1 .. MAX_TPL, or
 * a count beyond 2^31 - 1 (TRACE_C of more than 2^30 lags: the entry points accept such a job, this int cannot say it). */
int fosphor_amd_correlate_n_out(int trace, int32_t n, int tpl_len);

/* HOST only: the job that correlates what an extract job wrote into fosphor_amd_extract's d_out: offset = out_offset of e,
 * n = n_out of e; out_offset = 0: the caller places it.  0; -EINVAL: a NULL pointer, out_offset < 0 or n_out < 0 in e,
 * tpl_offset < 0, tpl_len outside 1 .. MAX_TPL, an unknown trace, a NaN threshold. */
int fosphor_amd_correlate_from_extract(const struct fosphor_amd_extract_job *e, int64_t tpl_offset, int tpl_len,
                                       int trace, float threshold, struct fosphor_amd_correlate_job *job);

/* HOST only: a record as seconds, ratios and dB, all in double:
 *   time         peak_lag / sample_rate: seconds from the job's sample 0 to the template's sample 0
 *   rho          peak_rho
 *   gain_re/_im  c / Et at the peak: the least-squares complex amplitude of the template in the signal
 *   gain_db      10 log10(gain_re^2 + gain_im^2)
 *   phase_turns  fosphor_amd_atan2_turns(peak_c_im, peak_c_re)
 *   snr_db       10 log10(rho / (1 - rho)): what of the window is the template over what is not; +INFINITY when rho >= 1
 *   detections   n_edges
 * With no peak (peak_lag < 0) or Et == 0 every field is 0.  Never NaN for finite sums; a peak of rho == 0 (a silent window)
 * gives gain_db and snr_db of -INFINITY, the logarithm's own answer, as rho >= 1 gives +INFINITY.
 * 0; -EINVAL: a NULL pointer, a sample_rate that is not finite and positive. */
struct fosphor_amd_correlate_values
{
	double time, rho, gain_re, gain_im, gain_db, phase_turns, snr_db, detections;
};
int fosphor_amd_correlate_derive(const struct fosphor_amd_correlate_record *r, double sample_rate,
                                 struct fosphor_amd_correlate_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_CORRELATE_CALLS]      fosphor_amd_correlate calls that reached the device
 *   stats[FOSPHOR_AMD_CORRELATE_K_TILE]     launches of the tile kernel
 *   stats[FOSPHOR_AMD_CORRELATE_K_COMBINE]  launches of the kernel that folds the partials and writes the records
 *   stats[FOSPHOR_AMD_CORRELATE_JOBS]       jobs of those calls (n_lags = 0 included)
 *   stats[FOSPHOR_AMD_CORRELATE_LAGS]       the sum of n_lags over those jobs
 *   stats[FOSPHOR_AMD_CORRELATE_MACS]       the sum of n_lags * T: complex multiply-adds */
enum {
	FOSPHOR_AMD_CORRELATE_CALLS, FOSPHOR_AMD_CORRELATE_K_TILE, FOSPHOR_AMD_CORRELATE_K_COMBINE, FOSPHOR_AMD_CORRELATE_JOBS,
	FOSPHOR_AMD_CORRELATE_LAGS, FOSPHOR_AMD_CORRELATE_MACS,
	FOSPHOR_AMD_CORRELATE_STATS
};
int fosphor_amd_correlate_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_CORRELATE_STATS]);

#ifdef __cplusplus
}
#endif

#endif
