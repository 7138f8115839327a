/*
 * fosphor_amd_measure.h -- what a burst's samples say: power, edges, lag-1 product and moments, a few numbers per job
 *
 * fosphor_amd_extract leaves each emission's baseband IQ in a device buffer.  The burst record that led there knows time in ring
 * rows and frequency in FFT columns; the samples know both to the sample.  This pass reduces them where they lie: every job of a
 * call is one range of float32 (re, im) pairs in device memory and gets one record of exact integers (how many samples are above a
 * threshold, the first and the last, how many times the envelope rises, where the peak is) and of double-precision sums (the mean,
 * the power and its square, y * y, and the lag-1 product).  Nothing transcendental runs on the device: fosphor_amd_measure_derive
 * turns a record into dB, Hz and ratios on the host.  Per-sample outputs (an envelope trace, a discriminator) are fosphor_amd_demod.h's.
 *
 * Conventions, those of fosphor_amd_extract.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when the records are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written or launched; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_MEASURE_H
#define FOSPHOR_AMD_MEASURE_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_extract.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_MEASURE_MAX_JOBS 4096

struct fosphor_amd_measure_job
{
	int64_t offset;		/* index into d_iq (complex samples) of the job's sample 0 */
	int32_t n;		/* samples, >= 0 */
	float   threshold;	/* on p (rule 1), linear power; +inf and negative values allowed, NaN refused */
};

struct fosphor_amd_measure_record	/* 96 bytes, 8-byte aligned */
{
	int32_t n_above;		/* samples m with above(m) */
	int32_t first_above, last_above;/* the smallest and the largest such m, relative to offset; -1 when none */
	int32_t n_edges;		/* m with above(m) && (m == 0 || !above(m - 1)) */
	int32_t peak_index;		/* rule 2 */
	float   peak_power;
	double  s_re, s_im;		/* sum y */
	double  s_p, s_p2;		/* sum p, sum p * p */
	double  s_zz_re, s_zz_im;	/* sum y * y: re * re - im * im, 2 * re * im */
	double  r1_re, r1_im;		/* sum over m = 0 .. n - 2 of y[m + 1] * conj(y[m]) */
	int32_t n;			/* the job's n */
	int32_t form;			/* FOSPHOR_AMD_MEASURE_FORM_WAVE / _SPLIT: the form that computed the record */
};

/* The forms (rule 4).  Tests plant job lengths across these seams. */
#define FOSPHOR_AMD_MEASURE_FORM_WAVE 0
#define FOSPHOR_AMD_MEASURE_FORM_SPLIT 1
#define FOSPHOR_AMD_MEASURE_WAVE_MAX 4096	/* the longest job of the WAVE form */
#define FOSPHOR_AMD_MEASURE_CHUNK    8192	/* samples of a SPLIT work-group */

/* Measure n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract writes
 *   d_records  n_jobs records in job order, 8-byte aligned
 * The input ranges of jobs may overlap; they are only read.  y[m] = d_iq[offset + m], m = 0 .. n - 1, re and im its parts.
 *
 * 1. Power      p = (re * re) + (im * im) in float32: three rounded operations, no contraction (the build's -ffp-contract=off;
 *               no fmaf), so that numpy float32 arithmetic reproduces p to the bit.  above(m) is p[m] >= threshold; a NaN p is
 *               not above.
 * 2. Integers   are exact.  n_above, first_above, last_above and n_edges follow from `above`.  peak_power is the largest non-NaN
 *               p and peak_index the smallest index that attains it; with no such sample (n == 0, or every p NaN) they are -1 and
 *               0.0f.  For finite inputs the six fields are bit-identical to fosphor_amd_measure_host and to the numpy model
 *               (tests/measure_model.py); they do not depend on the form, on the other jobs of the call, or on how a job is cut.
 * 3. Sums       in double.  Every term is formed in double from the float32 values: the products re * re, im * im, p * p and
 *               re1 * re0 are exact there, so each term of s_zz_* and r1_* rounds once and every other term not at all.  The
 *               terms are accumulated in double, with no float atomics and no atomics of any kind: the same call repeated gives
 *               bit-identical records, and a job's record does not depend on the other jobs of the call.  The order of the
 *               summation is fixed per form (rule 4); the forms need NOT agree bit for bit.  Each sum is within
 *                   n * 2^-52 * sum|term|
 *               of the exact sum of its terms: (n - 1) * 2^-53 for any order of n double additions, 2^-53 for each term's own
 *               rounding, doubled for slack.  A float32 accumulator does not meet that, on purpose.  Non-finite inputs
 *               propagate through the sums as IEEE arithmetic does.
 * 4. Forms      chosen from n alone and reported in record.form.
 *               WAVE (n <= FOSPHOR_AMD_MEASURE_WAVE_MAX): one wave owns a job, four jobs per 256-lane work-group.  The lanes
 *               stride the samples with 16-byte loads, two samples per lane per load, from the first 16-byte boundary on; the
 *               single samples before that boundary and behind the last whole pair are loaded one by one (lane 0), so no byte
 *               outside the job's range is read.  A lane sums its samples in ascending order; the 64 partials meet by
 *               xor-shuffles 32, 16, .. 1 (a double is two 32-bit shuffles); the peak is reduced as the pair (p, index): larger
 *               p first, then smaller index.  No LDS.
 *               SPLIT (every longer job): work-groups of 256 lanes own chunks of FOSPHOR_AMD_MEASURE_CHUNK samples, stride them
 *               as a wave of the WAVE form does, reduce each wave by the same shuffles, pass the four waves' partials through LDS
 *               where wave 0 folds them in wave order, and write one partial record per chunk into the instance's scratch.  A
 *               chunk reads sample m - 1 at its head for n_edges, and one sample past its end, if the job has one, for r1: the
 *               term y[m + 1] * conj(y[m]) belongs to the chunk of m.  A second kernel, one wave per job, folds a job's
 *               partials in ascending chunk order.  Two launches; no work-group waits for another, and every loop carries its
 *               bound.  A work-group finds its job in a prefix of work-group counts, as fosphor_amd_extract's does.
 *               Launches per call: at most one WAVE, one SPLIT and one combine, whatever the number of jobs.
 * 5. Writes     only d_records[0 .. n_jobs).  A job with n == 0 gets a record of zeros with the -1 indices (and its n and form).
 *
 * 0; -EINVAL (nothing is written or launched): a NULL self, d_iq, jobs or d_records; n_jobs outside 1 .. MAX_JOBS;
 * n_samples < 0; a job with offset < 0, n < 0 or offset + n > n_samples; a NaN threshold; d_iq or d_records not 8-byte aligned;
 * more than 2^31 - 1 work-groups in one form (MAX_JOBS jobs of 2^31 - 1 samples stay below that: the check is there for other
 * values of the constants).  -EIO. */
int fosphor_amd_measure(struct fosphor *self, const void *d_iq, int64_t n_samples,
                        const struct fosphor_amd_measure_job *jobs, int n_jobs,
                        struct fosphor_amd_measure_record *d_records);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers; one pass in ascending index, double sums;
 * record.form is the form the device would choose.  Where an operation meets two NaNs the left operand's comes through, the
 * accumulator's before the term's (this statement only, not the kernels, whose sums rule 3 holds to a bound): a build of one source
 * for one target gives the same bytes at every optimisation level.  0; -EINVAL: what the device entry point refuses, but for self. */
int fosphor_amd_measure_host(const float *iq, int64_t n_samples, const struct fosphor_amd_measure_job *jobs, int n_jobs,
                             struct fosphor_amd_measure_record *records);

/* HOST only: the job that measures what an extract job wrote into fosphor_amd_extract's d_out: offset = out_offset, n = n_out.
 * 0; -EINVAL: a NULL pointer, a NaN threshold, out_offset < 0 or n_out < 0. */
int fosphor_amd_measure_from_extract(const struct fosphor_amd_extract_job *e, float threshold,
                                     struct fosphor_amd_measure_job *job);

/* HOST only: a record as dB, Hz and ratios, all in double.  With n the record's n and "above" its n_above > 0:
 *   mean_power   s_p / n
 *   mean_db      10 log10(mean_power)
 *   peak_db      10 log10(peak_power)
 *   papr_db      peak_db - mean_db, the peak-to-average ratio
 *   freq_offset  atan2(r1_im, r1_re) / (2 pi) * sample_rate: the lag-1 estimate of the carrier offset, within +- sample_rate / 2
 *   coherence    |r1| / s_p: near 1 for a carrier, near 0 for noise
 *   kurtosis     (s_p2 / n) / (s_p / n)^2: 1 for a constant envelope, 2 for complex Gaussian noise
 *   circularity  |s_zz| / s_p: 1 for a real-valued or BPSK signal, 0 for QPSK or noise
 *   dc_fraction  |s|^2 / (n * s_p): the share of the power that sits at 0 Hz
 *   duty         n_above / n
 *   rise, fall   first_above / sample_rate, (last_above + 1) / sample_rate: seconds from the job's sample 0
 *   pulses       n_edges
 * Never NaN for finite sums: with n == 0 every field is 0; with s_p == 0 (n samples of silence) mean_db, papr_db, coherence,
 * kurtosis, circularity and dc_fraction are 0, as is peak_db when peak_power is 0 (no -inf); with nothing above, duty, rise, fall
 * and pulses are 0.  Sums that are not finite (rule 3) come through as IEEE arithmetic leaves them.
 * 0; -EINVAL: a NULL pointer, a sample_rate that is not finite and positive. */
struct fosphor_amd_measure_values
{
	double mean_power, mean_db, peak_db, papr_db, freq_offset, coherence, kurtosis, circularity, dc_fraction, duty, rise, fall,
	       pulses;
};
int fosphor_amd_measure_derive(const struct fosphor_amd_measure_record *r, double sample_rate,
                               struct fosphor_amd_measure_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_MEASURE_CALLS]       fosphor_amd_measure calls that reached the device
 *   stats[FOSPHOR_AMD_MEASURE_K_WAVE]      launches of the WAVE kernel
 *   stats[FOSPHOR_AMD_MEASURE_K_SPLIT]     launches of the SPLIT kernel
 *   stats[FOSPHOR_AMD_MEASURE_K_COMBINE]   launches of the kernel that folds the SPLIT partials
 *   stats[FOSPHOR_AMD_MEASURE_JOBS_WAVE]   jobs of those calls in the WAVE form (n = 0 included)
 *   stats[FOSPHOR_AMD_MEASURE_JOBS_SPLIT]  ... in the SPLIT form
 *   stats[FOSPHOR_AMD_MEASURE_SAMPLES]     the sum of n over those jobs */
enum {
	FOSPHOR_AMD_MEASURE_CALLS, FOSPHOR_AMD_MEASURE_K_WAVE, FOSPHOR_AMD_MEASURE_K_SPLIT, FOSPHOR_AMD_MEASURE_K_COMBINE,
	FOSPHOR_AMD_MEASURE_JOBS_WAVE, FOSPHOR_AMD_MEASURE_JOBS_SPLIT, FOSPHOR_AMD_MEASURE_SAMPLES,
	FOSPHOR_AMD_MEASURE_STATS
};
int fosphor_amd_measure_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_MEASURE_STATS]);

#ifdef __cplusplus
}
#endif

#endif
