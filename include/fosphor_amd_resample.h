/*
 * fosphor_amd_resample.h -- burst IQ at the rate the next pass needs: a rate change by U / D, a polyphase real FIR, batched per job
 *
 * fosphor_amd_extract divides the stream's rate by an integer.  fosphor_amd_demod's integrate-and-dump wants a whole number of
 * samples per symbol and fosphor_amd_correlate wants the signal at the template's rate: a burst found at 61.44 MS/s with a symbol
 * rate of 1.0 MS/s is at neither, whatever the integer.  This pass is the missing link of extract -> resample -> measure / demod /
 * correlate: every job of a call is one range of float32 (re, im) pairs x in device memory, exactly what fosphor_amd_extract writes,
 * one real prototype low-pass h of T = Q * U taps and a ratio U / D, and leaves float32 pairs at U / D of the rate in a device
 * buffer that the later passes read as they read extract's.  Q multiply-adds per component and output, all in double: the device
 * runs them on its fp64 fused multiply-add, and every output is pinned bit for bit (rule 2).
 *
 * Not this pass: a time-varying ratio (timing recovery; the ratio of a job is fixed, its phase0 is free), a complex prototype, and
 * ratios whose terms exceed MAX_UP / MAX_DOWN (fosphor_amd_resample_ratio gives the best one inside them).
 *
 * Conventions, those of fosphor_amd_correlate.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_RESAMPLE_H
#define FOSPHOR_AMD_RESAMPLE_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_extract.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_RESAMPLE_MAX_JOBS   4096
#define FOSPHOR_AMD_RESAMPLE_MAX_UP     256
#define FOSPHOR_AMD_RESAMPLE_MAX_DOWN   256
#define FOSPHOR_AMD_RESAMPLE_MAX_BRANCH 64	/* Q: taps of a polyphase branch, multiply-adds per component and output */

/* The forms (rule 4).  TILE: a work-group owns FOSPHOR_AMD_RESAMPLE_TILE consecutive outputs of a job and keeps their input span
 * and the job's taps in LDS.  A job is in the TILE form when
 *     8 * (span + 1) + 4 * ((T + 3) & ~3) <= FOSPHOR_AMD_RESAMPLE_TILE_LDS,   span = ((TILE - 1) * D + U - 1) / U + Q
 * (integer divisions; span is the most samples a tile reads, the + 1 the slot before an odd start).  DIRECT: every other job; a
 * lane owns one output and a work-group FOSPHOR_AMD_RESAMPLE_DIRECT_OUT.  Tests plant output counts, D and T across those seams. */
#define FOSPHOR_AMD_RESAMPLE_TILE       512
#define FOSPHOR_AMD_RESAMPLE_TILE_LDS   40960	/* bytes: four work-groups on a CU's 160 KiB (profiles/r17_resample.md) */
#define FOSPHOR_AMD_RESAMPLE_DIRECT_OUT 256

struct fosphor_amd_resample_job		/* 48 bytes */
{
	int64_t offset;		/* index into d_iq  (complex samples) of x[0] */
	int64_t out_offset;	/* index into d_out (complex samples) of y[0] */
	int64_t phase0;		/* position of output 0, in units of 1 / U input sample from x[0], >= 0 */
	int32_t n;		/* input samples, >= 0 */
	int32_t n_out;		/* outputs to write, 0 .. the largest valid (rule 1) */
	int32_t up;		/* U, 1 .. MAX_UP */
	int32_t down;		/* D, 1 .. MAX_DOWN */
	int32_t taps_offset;	/* index into d_taps of h[0] */
	int32_t n_taps;		/* T = Q * U, Q in 1 .. MAX_BRANCH */
};

/* Resample n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq    n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract writes
 *   d_taps  n_taps_total float32 real prototype taps, 4-byte aligned, shared by the jobs through taps_offset / n_taps
 *   d_out   out_capacity float32 (re, im) pairs, 8-byte aligned; job j owns d_out[out_offset .. out_offset + n_out)
 * x[i] = d_iq[offset + i], i = 0 .. n - 1; h[k] = d_taps[taps_offset + k], k = 0 .. T - 1; U = up, D = down, Q = T / U.
 *
 * Every output is BIT-IDENTICAL between the device, fosphor_amd_resample_host and the numpy model (tests/resample_model.py), and
 * depends on its job alone: not on the other jobs, not on the form that computed it, not on how a job is cut (rule 3).
 *
 * 1. Contract   Put U - 1 zeros between the samples of x, filter with h (a correlation with h as written, as in
 *               fosphor_amd_extract.h: a symmetric low-pass does not care) and pick the outputs phase0 + m * D of the up-sampled
 *               rate.  Only every U-th product is not zero, so it is computed as the polyphase sum it equals.  For output m:
 *                   p = phase0 + m * D                  int64; the position in units of 1 / U input sample
 *                   b = ceil(p / U)                     the first input sample at or behind p
 *                   s = b * U - p                       0 .. U - 1: the polyphase branch
 *                   y[m] = sum over q = 0 .. Q - 1 of  h[s + q * U] * x[b + q]
 *               The mode is "valid" only: every output needs b + Q <= n, so the largest valid n_out is
 *               ((n - Q) * U - phase0) / D + 1 when n >= Q and phase0 <= (n - Q) * U, and 0 otherwise
 *               (fosphor_amd_resample_n_out).  With U = 1 this is a decimating FIR; with U = D = 1, T = 1, h = { 1.0f } a copy,
 *               bit for bit but for what rule 2 does to a -0.0 (the sum from +0.0 gives +0.0) and to a NaN's payload.
 *               Output m is centred (T - 1) / (2 U) input samples behind p / U: the group delay of a symmetric h.
 * 2. Arithmetic per output two double accumulators, from 0.0, q ascending:
 *                   re += (double)h * (double)re_x;   im += (double)h * (double)im_x;
 *               each rounded ONCE to float32 at the end.  The product of two finite float32 values is exact in double (rule 1 of
 *               fosphor_amd_correlate.h), so a fused multiply-add and a multiply followed by an add give the same bits: the device
 *               uses the fp64 fused multiply-add, the host adds products, numpy multiplies, then adds.  No sum crosses a lane.  A
 *               NaN output is the quiet NaN 0x7fc00000 whatever the payloads were (rule 3 of fosphor_amd_demod.h); other
 *               non-finite values propagate as IEEE arithmetic does (a zero tap times an infinite sample is a NaN).
 * 3. Cut rule   a job of n_out outputs and its two halves cut at output c -- the same job with n_out = c, and the same job with
 *               phase0 + c * D and n_out - c (the same offset and n) -- give the same bits: p is an integer function of m, as the
 *               phase of fosphor_amd_extract is of the sample's index.
 * 4. Forms      chosen from (U, D, T) alone, by the #defines above.
 *               TILE: a work-group of 256 lanes owns FOSPHOR_AMD_RESAMPLE_TILE consecutive outputs of one job, which it finds in
 *               a prefix of work-group counts by a bounded binary search.  It brings the tile's input span x[b_first .. b_last + Q)
 *               into LDS with 16-byte loads from the first 16-byte boundary on (the single samples before that boundary and behind
 *               the last whole pair go one by one: no byte outside the span is read) and the job's T taps beside it, in the order
 *               they have: for a fixed q branch s lies at word s + q * U, so the lanes of a wave, which read the same q and
 *               different s, read different words of one stretch of U, and lanes with the same s read the same word (a
 *               broadcast).  Lane i computes outputs i and i + 256 of the tile and stores 8 bytes per output, consecutive lanes
 *               to consecutive addresses.
 *               DIRECT: every job whose span plus taps exceed the LDS budget (a large D / U or a large T); one output per lane,
 *               x and h straight from global memory.
 *               At most one launch per form per call, whatever the number of jobs; no atomics, no work-group waits for another,
 *               every loop carries its bound.  A job with n_out = 0 is counted in its form and takes no work-group.
 * 5. Access     reads touch only d_iq[offset .. offset + n) and d_taps[taps_offset .. taps_offset + T) of each job; writes only
 *               each job's d_out[out_offset .. out_offset + n_out).  Input ranges may overlap; output ranges must not.
 * 6. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, jobs, d_taps or d_out;
 *               n_jobs outside 1 .. MAX_JOBS; n_samples, n_taps_total or out_capacity below 0; a job with offset, out_offset,
 *               phase0, n or n_out below 0, offset + n > n_samples, up outside 1 .. MAX_UP, down outside 1 .. MAX_DOWN, n_taps
 *               that is not Q * up with Q in 1 .. MAX_BRANCH, taps_offset < 0 or taps_offset + n_taps > n_taps_total, n_out
 *               above the largest valid n_out, out_offset + n_out > out_capacity, or outputs over another job's; d_iq or d_out
 *               not 8-byte aligned; d_taps not 4-byte aligned; more than 2^31 - 1 work-groups in one form.  Every check is safe
 *               against values of 2^62.
 *
 * 0; -EINVAL (rule 6); -EIO. */
int fosphor_amd_resample(struct fosphor *self, const void *d_iq, int64_t n_samples,
                         const struct fosphor_amd_resample_job *jobs, int n_jobs,
                         const float *d_taps, int64_t n_taps_total,
                         void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_resample_host(const float *iq, int64_t n_samples,
                              const struct fosphor_amd_resample_job *jobs, int n_jobs,
                              const float *taps, int64_t n_taps_total,
                              float *out, int64_t out_capacity);

/* HOST only: the largest valid n_out of a job (rule 1), or -EINVAL: n < 0, up outside 1 .. MAX_UP, down outside 1 .. MAX_DOWN,
 * n_taps that is not Q * up with Q in 1 .. MAX_BRANCH, phase0 < 0, or a count beyond 2^31 - 1 (a job cannot say it either). */
int fosphor_amd_resample_n_out(int32_t n, int up, int down, int n_taps, int64_t phase0);

/* HOST only: a Hamming-windowed sinc prototype of T = branch_taps * up taps for the ratio up / down: the formula of
 * fosphor_amd_extract_design with fc = guard / (2 * max(up, down)) cycles per sample OF THE UP-SAMPLED RATE (0 < guard <= 1), which
 * is below both Nyquist rates -- c = (T - 1) / 2 and, for k = 0 .. T - 1,
 *     t    = k - c
 *     s[k] = 2 * fc                          where t == 0
 *            sin(2 * pi * fc * t) / (pi * t)   elsewhere
 *     w[k] = 0.54 - 0.46 * cos(2 * pi * k / (T - 1))          (1 when T == 1)
 *     g[k] = s[k] * w[k]
 * all in double; g[k] is computed for k <= c and mirrored, so h is symmetric to the bit; out[k] = (float)((g[k] / sum of g in
 * ascending k) * up): the taps sum to up before rounding, so every branch has a gain near 1.  With up = down = 1 these are the
 * taps of fosphor_amd_extract_design(1, T, guard), bit for bit.  The group delay is (T - 1) / (2 * up) input samples.
 * 0; -EINVAL: up outside 1 .. MAX_UP, down outside 1 .. MAX_DOWN, branch_taps outside 1 .. MAX_BRANCH, guard not in (0, 1], a NULL
 * out. */
int fosphor_amd_resample_design(int up, int down, int branch_taps, double guard, float *out);

/* HOST only: the best up / down for rate_out / rate_in with both terms in 1 .. min(max_term, 256): the fraction in lowest terms
 * that minimises |up / down - rate_out / rate_in|, the smaller down on a tie, found among the convergents and semiconvergents of
 * the continued fraction of rate_out / rate_in.  *error (may be NULL) is the achieved rate's relative error,
 * (rate_in * up / down - rate_out) / rate_out.
 * 0; -EINVAL: a rate that is not finite and positive, max_term below 1, a NULL up or down. */
int fosphor_amd_resample_ratio(double rate_in, double rate_out, int max_term, int *up, int *down, double *error);

/* HOST only: the job that resamples what an extract job wrote into fosphor_amd_extract's d_out: offset = out_offset of e,
 * n = n_out of e, phase0 = 0, n_out the largest valid value; out_offset = taps_offset = 0: the caller places it.
 * 0; -EINVAL: a NULL pointer, out_offset < 0 or n_out < 0 in e, what fosphor_amd_resample_n_out refuses. */
int fosphor_amd_resample_from_extract(const struct fosphor_amd_extract_job *e, int up, int down, int n_taps,
                                      struct fosphor_amd_resample_job *job);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_RESAMPLE_CALLS]        fosphor_amd_resample calls that reached the device
 *   stats[FOSPHOR_AMD_RESAMPLE_K_TILE]       launches of the TILE kernel
 *   stats[FOSPHOR_AMD_RESAMPLE_K_DIRECT]     launches of the DIRECT kernel
 *   stats[FOSPHOR_AMD_RESAMPLE_JOBS_TILE]    jobs of those calls in the TILE form (n_out = 0 included)
 *   stats[FOSPHOR_AMD_RESAMPLE_JOBS_DIRECT]  ... in the DIRECT form
 *   stats[FOSPHOR_AMD_RESAMPLE_OUTPUTS]      the sum of n_out over those jobs
 *   stats[FOSPHOR_AMD_RESAMPLE_MACS]         the sum of n_out * Q: real-by-complex multiply-adds, two fp64 operations each */
enum {
	FOSPHOR_AMD_RESAMPLE_CALLS, FOSPHOR_AMD_RESAMPLE_K_TILE, FOSPHOR_AMD_RESAMPLE_K_DIRECT, FOSPHOR_AMD_RESAMPLE_JOBS_TILE,
	FOSPHOR_AMD_RESAMPLE_JOBS_DIRECT, FOSPHOR_AMD_RESAMPLE_OUTPUTS, FOSPHOR_AMD_RESAMPLE_MACS,
	FOSPHOR_AMD_RESAMPLE_STATS
};
int fosphor_amd_resample_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_RESAMPLE_STATS]);

#ifdef __cplusplus
}
#endif

#endif
