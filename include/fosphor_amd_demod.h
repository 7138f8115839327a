/*
 * fosphor_amd_demod.h -- what a burst carried: power, phase and instantaneous-frequency traces, one float32 trace per job
 *
 * fosphor_amd_extract leaves each emission's baseband IQ in a device buffer and fosphor_amd_measure reduces it to a few numbers.
 * This pass is the per-sample half: every job of a call is one range of float32 (re, im) pairs in device memory and gets one
 * float32 trace in a device buffer of the caller's -- the envelope power (AM, pulse shape), the phase, or the phase step between
 * consecutive samples (FSK, chirps, drift) -- optionally integrated and dumped over L trace values.  The only transcendental is
 * the angle, and it is pinned the way fosphor_portable_math.h pins log10: fosphor_amd_atan2_turns below is a fixed sequence of
 * IEEE double operations rounded once to float32, so the device, fosphor_amd_demod_host and the numpy model
 * (tests/demod_model.py) agree to the bit.  No sqrt, no libm call and no float32 division anywhere in the pass: magnitude and dB
 * traces, which would need a pinned sqrt / log10 on the device, are not this pass; neither is phase unwrapping, and symbol timing
 * is fosphor_amd_symbols' work (fosphor_amd_symbols.h), which takes its angle from fosphor_amd_atan2_turns below.
 * The whole number of samples per symbol that integrate-and-dump wants is fosphor_amd_resample's work (fosphor_amd_resample.h).
 *
 * Conventions, those of fosphor_amd_measure.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written or launched; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_DEMOD_H
#define FOSPHOR_AMD_DEMOD_H

#include <math.h>
#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_extract.h"

#define FOSPHOR_AMD_DEMOD_MAX_JOBS 4096
#define FOSPHOR_AMD_DEMOD_MAX_AVG  256
#define FOSPHOR_AMD_DEMOD_TILE     2048	/* trace values of a work-group (rule 4); tests plant job lengths across this seam */

/* The modes.  y[m] = d_iq[offset + m], m = 0 .. n - 1, re and im its parts; v[m] is the trace, n_trace its length. */
#define FOSPHOR_AMD_DEMOD_POWER 0	/* v[m] = p[m]                                      n_trace = n */
#define FOSPHOR_AMD_DEMOD_PHASE 1	/* v[m] = turns(im[m], re[m])                       n_trace = n */
#define FOSPHOR_AMD_DEMOD_FM    2	/* v[m] = turns(Im z, Re z), z = y[m + 1] conj(y[m]) n_trace = max(n - 1, 0) */

#if defined(__HIPCC__)
#define FOSPHOR_AMD_DEMOD_INLINE static inline __host__ __device__
#else
#define FOSPHOR_AMD_DEMOD_INLINE static inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define FOSPHOR_AMD_DEMOD_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define FOSPHOR_AMD_DEMOD_NO_CONTRACT
#endif
#if defined(__GNUC__)
#define FOSPHOR_AMD_DEMOD_SIGNBIT(v) (__builtin_signbit(v) != 0)
#define FOSPHOR_AMD_DEMOD_FABS(v) __builtin_fabs(v)
#else
#define FOSPHOR_AMD_DEMOD_SIGNBIT(v) (signbit(v) != 0)
#define FOSPHOR_AMD_DEMOD_FABS(v) fabs(v)
#endif

/* The angle of (x, y) in turns, in [-0.5, 0.5], as float32: rule 2 below, operation for operation.  Double + - * /, comparisons
 * and sign bits only; no multiply-add is formed (the pragma / attribute here, -ffp-contract=off in the library's build).
 * C99 and C++, host and device. */
FOSPHOR_AMD_DEMOD_INLINE FOSPHOR_AMD_DEMOD_NO_CONTRACT float fosphor_amd_atan2_turns(double y, double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (y != y || x != x)
		return NAN;
	const double ax = FOSPHOR_AMD_DEMOD_FABS(x), ay = FOSPHOR_AMD_DEMOD_FABS(y);
	const double mn = ay > ax ? ax : ay, mx = ay > ax ? ay : ax;
	double t;
	if (mx == 0.0)
		t = 0.0;
	else if (mn > 1.7976931348623157e308)		/* both infinite */
		t = 1.0;
	else
		t = mn / mx;
	const int big = t > 0.41421356237309503;	/* tan(pi / 8) */
	const double u = big ? (t - 1.0) / (t + 1.0) : t;
	const double z = u * u;
	double q = 1.0 / 25.0;				/* atan(u) / u = sum over k of (-1)^k z^k / (2k + 1), k = 12 .. 0 by Horner */
	q = q * z + -1.0 / 23.0;
	q = q * z + 1.0 / 21.0;
	q = q * z + -1.0 / 19.0;
	q = q * z + 1.0 / 17.0;
	q = q * z + -1.0 / 15.0;
	q = q * z + 1.0 / 13.0;
	q = q * z + -1.0 / 11.0;
	q = q * z + 1.0 / 9.0;
	q = q * z + -1.0 / 7.0;
	q = q * z + 1.0 / 5.0;
	q = q * z + -1.0 / 3.0;
	q = q * z + 1.0 / 1.0;
	double a = (u * q) * 0.15915494309189535;	/* 1 / (2 pi) */
	if (big)
		a = 0.125 + a;
	if (ay > ax)
		a = 0.25 - a;
	if (FOSPHOR_AMD_DEMOD_SIGNBIT(x))
		a = 0.5 - a;
	if (FOSPHOR_AMD_DEMOD_SIGNBIT(y))
		a = -a;
	return (float)a;
}

#ifdef __cplusplus
extern "C" {
#endif

struct fosphor_amd_demod_job		/* 32 bytes */
{
	int64_t offset;		/* index into d_iq (complex samples) of the job's sample 0 */
	int64_t out_offset;	/* index into d_out (floats) of its first output */
	int32_t n;		/* input samples, >= 0 */
	int32_t mode;		/* FOSPHOR_AMD_DEMOD_* */
	int32_t avg;		/* L, 1 .. MAX_AVG: integrate and dump, L trace values per output */
	int32_t reserved;	/* must be 0 */
};

/* Demodulate n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq   n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract writes
 *   d_out  out_capacity floats, 4-byte aligned; job j owns d_out[out_offset .. out_offset + n_out), n_out = n_trace / L
 *
 * Every output is BIT-IDENTICAL between the device, fosphor_amd_demod_host and the numpy model, and depends on its job alone:
 * not on the other jobs of the call, not on the form's tiles, not on how a job is cut (rule 3).
 *
 * 1. Trace      p = (re * re) + (im * im) in float32: three rounded operations, no contraction (rule 1 of fosphor_amd_measure.h).
 *               PHASE passes ((double)im, (double)re) to fosphor_amd_atan2_turns.  FM forms z in double from the float32 values,
 *               as fosphor_amd_measure forms its r1 terms: Re z = re1 * re0 + im1 * im0, Im z = im1 * re0 - re1 * im0, every
 *               product exact, each component rounded once; then it passes (Im z, Re z).  The mean of an FM trace therefore
 *               estimates what fosphor_amd_measure_derive's freq_offset / sample_rate estimates.
 * 2. Angle      fosphor_amd_atan2_turns(y, x), in this order: a NaN argument gives NaN.  ax = |x|, ay = |y|, mn their minimum,
 *               mx their maximum.  t = 0 when mx == 0, 1 when mn is infinite, else mn / mx.  big = t > 0.41421356237309503;
 *               u = (t - 1) / (t + 1) when big, else t.  z = u * u.  q = 1.0 / 25.0; for k = 11 down to 0,
 *               q = q * z + s_k / (2k + 1) with s_k = +1 for even k and -1 for odd k (a multiplication, then an addition).
 *               a = (u * q) * 0.15915494309189535.  If big, a = 0.125 + a.  If ay > ax, a = 0.25 - a.  If signbit(x),
 *               a = 0.5 - a.  If signbit(y), a = -a.  The result is (float)a.  The double chain is within 4e-12 relative of
 *               atan2 / (2 pi) (the series is cut at z^13 / 27 with z <= tan(pi / 8)^2), the one rounding costs at most half a
 *               float32 ulp more.  Seams: (0, 1) -> 0, (-0, 1) -> -0, (0, -1) -> 0.5, (-0, -1) -> -0.5, (+-1, 0) -> +-0.25,
 *               (1, 1) -> 0.125, (1, -1) -> 0.375, (0, 0) -> 0, (inf, inf) -> 0.125, (inf, 1) -> 0.25, (1, -inf) -> 0.5.
 *               On the device the same sequence runs in fp64; fp64 division is the IEEE-correct expansion.
 * 3. Average    integrate and dump: output j of a job is (float)(S / (double)L), S the sum in double of (double)v[jL] ..
 *               (double)v[jL + L - 1] added in ascending order starting from 0.0.  n_out = n_trace / L (integer division); a
 *               trailing remainder is dropped.  With L = 1 the output is v itself (a -0 stays -0).  The order is pinned per
 *               output: the kernels parallelise over outputs, never inside one.  Hence a job of n_out outputs gives, bit for
 *               bit, the outputs of two jobs cut at a multiple c * L of trace values: (offset, n = c * L [+ 1 for FM]) and
 *               (offset + c * L, n - c * L).  For FM the two ranges share the sample y[c * L].
 *               Non-finite inputs propagate as IEEE arithmetic does; a NaN output is the quiet NaN 0x7fc00000 whatever the
 *               payloads were (the p of rule 1 and S / L pass through x != x ? NAN : x; the angle returns NAN itself).
 * 4. Forms      chosen from avg alone and counted in the stats.  Work-groups of 256 lanes; a work-group finds its job in a
 *               prefix of work-group counts by a bounded binary search, as fosphor_amd_extract's and fosphor_amd_measure's do.
 *               Both forms bring their tile's samples into LDS with 16-byte loads from the first 16-byte boundary on, one
 *               pair of samples per lane per load; the single samples before that boundary and behind the last whole pair
 *               are loaded one by one.  An FM tile reads one sample past its last trace value's y[m]: the job always has it.
 *               DIRECT (L = 1): a work-group owns FOSPHOR_AMD_DEMOD_TILE consecutive trace values of a job; lane i computes
 *               values i, i + 256, .. from LDS and stores them, 4 bytes per lane, consecutive lanes to consecutive floats.
 *               AVG (L > 1): a work-group owns TILE / L outputs, (TILE / L) * L trace values.  The trace values are computed
 *               one per lane in parallel (the angle is the expensive part) into LDS rows of L values with a row stride of
 *               L | 1 floats, so that the lanes that then add one row each, in order, read 32 different banks.
 *               Launches per call: at most one DIRECT and one AVG, whatever the number of jobs.  No atomics, no work-group
 *               waits for another, every loop carries its bound.
 * 5. Access     reads touch only d_iq[offset .. offset + n) of each job, writes only d_out[out_offset .. out_offset + n_out).
 *               Input ranges may overlap; output ranges must not.  A job with n_out == 0 writes nothing.
 *
 * 0; -EINVAL (nothing is written, launched or counted): a NULL self, d_iq, jobs or d_out; n_jobs outside 1 .. MAX_JOBS;
 * n_samples or out_capacity below 0; a job with offset < 0, n < 0, offset + n > n_samples, out_offset < 0, an unknown mode, avg
 * outside 1 .. MAX_AVG, reserved != 0, out_offset + n_out > out_capacity, or outputs over another job's; d_iq not 8-byte
 * aligned; d_out not 4-byte aligned; more than 2^31 - 1 work-groups in one form.  -EIO. */
int fosphor_amd_demod(struct fosphor *self, const void *d_iq, int64_t n_samples,
                      const struct fosphor_amd_demod_job *jobs, int n_jobs,
                      float *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_demod_host(const float *iq, int64_t n_samples, const struct fosphor_amd_demod_job *jobs, int n_jobs,
                           float *out, int64_t out_capacity);

/* HOST only: n_out = n_trace / avg of a job (rule 3), or -EINVAL: an unknown mode, n < 0, avg outside 1 .. MAX_AVG. */
int fosphor_amd_demod_n_out(int mode, int32_t n, int avg);

/* HOST only: the job that demodulates what an extract job wrote into fosphor_amd_extract's d_out: offset = out_offset of e,
 * n = n_out of e; out_offset = 0 and reserved = 0: the caller places it.  0; -EINVAL: a NULL pointer, out_offset < 0 or
 * n_out < 0 in e, an unknown mode, avg outside 1 .. MAX_AVG. */
int fosphor_amd_demod_from_extract(const struct fosphor_amd_extract_job *e, int mode, int avg,
                                   struct fosphor_amd_demod_job *job);

/* HOST only: fosphor_amd_atan2_turns as the library compiled it, for callers that cannot include this header (one pair, and n
 * pairs: out[i] = turns(y[i], x[i]); -EINVAL: a NULL pointer or n < 0). */
float fosphor_amd_demod_atan2_turns(double y, double x);
int fosphor_amd_demod_atan2_turns_n(const double *y, const double *x, int64_t n, float *out);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_DEMOD_CALLS]        fosphor_amd_demod calls that reached the device
 *   stats[FOSPHOR_AMD_DEMOD_K_DIRECT]     launches of the DIRECT kernel
 *   stats[FOSPHOR_AMD_DEMOD_K_AVG]        launches of the AVG kernel
 *   stats[FOSPHOR_AMD_DEMOD_JOBS_DIRECT]  jobs of those calls in the DIRECT form (n_out = 0 included)
 *   stats[FOSPHOR_AMD_DEMOD_JOBS_AVG]     ... in the AVG form
 *   stats[FOSPHOR_AMD_DEMOD_SAMPLES]      the sum of n over those jobs
 *   stats[FOSPHOR_AMD_DEMOD_OUTPUTS]      the sum of n_out */
enum {
	FOSPHOR_AMD_DEMOD_CALLS, FOSPHOR_AMD_DEMOD_K_DIRECT, FOSPHOR_AMD_DEMOD_K_AVG, FOSPHOR_AMD_DEMOD_JOBS_DIRECT,
	FOSPHOR_AMD_DEMOD_JOBS_AVG, FOSPHOR_AMD_DEMOD_SAMPLES, FOSPHOR_AMD_DEMOD_OUTPUTS,
	FOSPHOR_AMD_DEMOD_STATS
};
int fosphor_amd_demod_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DEMOD_STATS]);

#ifdef __cplusplus
}
#endif

#endif
