/*
 * fosphor_amd_carrier.h -- what is left of this burst's carrier, and its symbols without it: feed-forward frequency and phase per
 * job over the symbols of a burst, one derotated complex sample per symbol and one record (frequency, phase, lag sums, lock) per job
 *
 * fosphor_amd_symbols leaves one complex sample per symbol of a burst.  The offset that fosphor_amd_measure or fosphor_amd_psd found
 * and fosphor_amd_extract mixed out is good to a fraction of a PSD bin; what remains turns the constellation by many degrees over a
 * few hundred symbols.  This pass takes that last step.  The M-th power of an M-ary PSK symbol carries no data: p = s^M turns by M f
 * per symbol.  The angle of the sum of p[j + 1] conj(p[j]) gives M f coarsely and without ambiguity; the angle of the same sum at a
 * lag of L symbols gives it L times finer and is unwrapped by the first (two-lag estimate, rule 3).  The angle of the sum of p with
 * that frequency removed is M times the phase (rule 5), and the symbols are turned back by both (rule 6).  It is feed-forward: two
 * reductions, three angles, one rotation per symbol, nothing that a symbol's result feeds back into, so up to 4096 bursts go in
 * one call.  A job may also name its frequency or its phase (FREQ_FIXED, PHASE_FIXED) and have the rest estimated.
 *
 * Not this pass: decisions and differential decoding (the phase is known modulo 1 / M turns only; a later pass over what this one
 * writes), loops with feedback (PLL, Costas), an FFT search for the line (fosphor_amd_psd with its fourth-power pre-step shows it),
 * and lags above FOSPHOR_AMD_CARRIER_MAX_LAG.
 *
 * Conventions, those of fosphor_amd_symbols.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_CARRIER_H
#define FOSPHOR_AMD_CARRIER_H

#include <math.h>
#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_demod.h"			/* fosphor_amd_atan2_turns and the macros of an inline of the contract */
#include "fosphor_amd_symbols.h"

#define FOSPHOR_AMD_CARRIER_MAX_JOBS 4096
#define FOSPHOR_AMD_CARRIER_MAX_LAG  64
#define FOSPHOR_AMD_CARRIER_BLOCK    64		/* symbols of a block of the ordered sums (rules 2 and 5) */
#define FOSPHOR_AMD_CARRIER_TILE     4096	/* symbols of a tile: 64 blocks; tests plant symbol counts across both seams */

#define FOSPHOR_AMD_CARRIER_FREQ_FIXED  1	/* mode bits; 0 = estimate both */
#define FOSPHOR_AMD_CARRIER_PHASE_FIXED 2

#define FOSPHOR_AMD_CARRIER_OK         0
#define FOSPHOR_AMD_CARRIER_NO_CARRIER 1	/* an angle of rule 3 or rule 5 is a NaN: no symbol is written */

/* static LDS of a work-group of each kernel, bytes (tests/test_carrier_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_CARRIER_LDS_LAG   15536	/* 321 double pairs of p; four waves x 4 x 65 terms; 4 x 65 block sums */
#define FOSPHOR_AMD_CARRIER_LDS_FREQ  0
#define FOSPHOR_AMD_CARRIER_LDS_SUM   10400	/* four waves x 4 x 65 terms; 4 x 65 block sums */
#define FOSPHOR_AMD_CARRIER_LDS_PHASE 0
#define FOSPHOR_AMD_CARRIER_LDS_TURN  0

#if defined(__GNUC__)
#define FOSPHOR_AMD_CARRIER_FLOOR(v) __builtin_floor(v)
#else
#define FOSPHOR_AMD_CARRIER_FLOOR(v) floor(v)
#endif

/* The cosine and the sine of t turns: rule 4 below, operation for operation.  Double + - *, floor, comparisons and a conversion to
 * int only; no multiply-add is formed (the pragma / attribute here, -ffp-contract=off in the library's build).  The coefficients
 * are quotients of two exact literals, which the compiler rounds once, as IEEE division does.  C99 and C++, host and device. */
FOSPHOR_AMD_DEMOD_INLINE FOSPHOR_AMD_DEMOD_NO_CONTRACT void fosphor_amd_cossin_turns(double t, double *c, double *s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (!(FOSPHOR_AMD_DEMOD_FABS(t) <= 1.7976931348623157e308)) {	/* a NaN or an infinity */
		*c = NAN;
		*s = NAN;
		return;
	}
	double r = t - FOSPHOR_AMD_CARRIER_FLOOR(t);
	if (!(r < 1.0))							/* a tiny negative t: t + 1 rounds to 1 */
		r = 0.0;
	const double q = FOSPHOR_AMD_CARRIER_FLOOR((r * 4.0) + 0.5);	/* the nearest quarter turn, 0 .. 4 */
	const double d = r - (q * 0.25);				/* exact; within an eighth of a turn */
	const double x = d * 6.283185307179586;
	const double z = x * x;
	double S = 1.0 / 355687428096000.0;				/* sin x / x = sum over k of (-1)^k z^k / (2k + 1)!, k = 8 .. 0 by Horner */
	S = S * z + -1.0 / 1307674368000.0;
	S = S * z + 1.0 / 6227020800.0;
	S = S * z + -1.0 / 39916800.0;
	S = S * z + 1.0 / 362880.0;
	S = S * z + -1.0 / 5040.0;
	S = S * z + 1.0 / 120.0;
	S = S * z + -1.0 / 6.0;
	S = S * z + 1.0 / 1.0;
	S = x * S;
	double C = 1.0 / 20922789888000.0;				/* cos x = sum over k of (-1)^k z^k / (2k)!, k = 8 .. 0 by Horner */
	C = C * z + -1.0 / 87178291200.0;
	C = C * z + 1.0 / 479001600.0;
	C = C * z + -1.0 / 3628800.0;
	C = C * z + 1.0 / 40320.0;
	C = C * z + -1.0 / 720.0;
	C = C * z + 1.0 / 24.0;
	C = C * z + -1.0 / 2.0;
	C = C * z + 1.0 / 1.0;
	const int quad = (int)q & 3;
	if (quad == 0) {
		*c = C;
		*s = S;
	} else if (quad == 1) {
		*c = -S;
		*s = C;
	} else if (quad == 2) {
		*c = -C;
		*s = -S;
	} else {
		*c = S;
		*s = -C;
	}
}

#ifdef __cplusplus
extern "C" {
#endif

struct fosphor_amd_carrier_job			/* 48 bytes */
{
	int64_t offset;		/* index into d_iq  (complex samples) of the job's symbol 0 */
	int64_t out_offset;	/* index into d_out (complex samples) of its first output */
	int32_t n;		/* symbols, >= 0 */
	int32_t order;		/* M: 2 (BPSK), 4 (QPSK) or 8 (8PSK) */
	int32_t mode;		/* 0 or a sum of FOSPHOR_AMD_CARRIER_FREQ_FIXED and _PHASE_FIXED */
	int32_t lag;		/* L, 1 .. MAX_LAG: the long lag of rule 2 (checked under FREQ_FIXED too, where it is not used) */
	double  freq;		/* FREQ_FIXED: f in turns per symbol, finite, |freq| <= 0.5.  Must be 0 otherwise */
	double  phase;		/* PHASE_FIXED: theta in turns, finite, |phase| <= 0.5.  Must be 0 otherwise */
};

struct fosphor_amd_carrier_record		/* 96 bytes, 8-byte aligned */
{
	int32_t n;				/* the job's */
	int32_t order;				/* the job's */
	int32_t lag_used;			/* Le of rule 2; 0 under FREQ_FIXED */
	int32_t status;				/* FOSPHOR_AMD_CARRIER_OK or _NO_CARRIER */
	double  freq;				/* f of rule 3, turns per symbol; the quiet NaN with NO_CARRIER */
	double  phase;				/* theta of rule 5, turns; the quiet NaN with NO_CARRIER */
	double  r1_re, r1_im, rl_re, rl_im;	/* the lag sums of rule 2; 0 under FREQ_FIXED; rl = 0 when lag_used == 1 */
	double  z_re, z_im;			/* Z of rule 5 */
	double  m2, mm;				/* sums of |s|^2 and |s|^order (rule 5) */
};

/* Carrier frequency, phase and derotated symbols of n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, one per symbol, 8-byte aligned: exactly what fosphor_amd_symbols writes
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity float32 (re, im) pairs, 8-byte aligned.  Job j owns d_out[out_offset .. out_offset + n): the host knows
 *              n, so nothing is reserved beyond it.  All n are written, or none (NO_CARRIER)
 * s[j] = d_iq[offset + j], its float32 parts widened to double; M = order, L = lag.
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_carrier_host and the numpy
 * model (tests/carrier_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels'
 * grid, not on repetition.  The build's -ffp-contract=off holds: every operation below is one IEEE double operation, rounded once,
 * in the order the parentheses give, and no fused multiply-add appears in this pass.  A NaN float is the quiet NaN 0x7fc00000 and a
 * NaN double of the record 0x7ff8000000000000, whatever the payloads were.
 *
 * 1. Power      p[j] = s[j] raised to M by log2 M applications of the SQUARE rule of fosphor_amd_psd.h, ((re * re) - (im * im),
 *               (re * im) + (re * im)).  w[j] = (re * re) + (im * im) of s[j]; |s[j]|^M is w for M = 2, w * w for M = 4 and
 *               (w * w) * (w * w) for M = 8: w squared log2 M - 1 times.
 * 2. Lag sums   frequency ESTIMATE (FREQ_FIXED not set) only.  Le = L if n >= 2 L, else 1: lag_used.  For d in {1, Le} and
 *               j < n - d, with a = p[j + d] and b = p[j], t = ((ar * br) + (ai * bi), (ai * br) - (ar * bi)): a conj(b).  R_d is
 *               the sum of t over j in the three-level order of fosphor_amd_symbols.h rule 1: blocks of 64 consecutive j, j
 *               ascending, from 0.0; tiles of 64 blocks (FOSPHOR_AMD_CARRIER_TILE terms), blocks ascending, from 0.0; the job,
 *               tiles ascending, from 0.0.  The term j belongs to the block of j, though it reads symbol j + d.  A block or a tile
 *               that the terms end in holds what there is.  With Le == 1 the record's rl is 0; under FREQ_FIXED r1 and rl are 0
 *               and lag_used is 0.
 * 3. Frequency  a1 = fosphor_amd_atan2_turns(R1i, R1r) (fosphor_amd_demod.h), a float32.  If Le > 1: aL the same angle of R_Le,
 *               k = floor((((double)Le * (double)a1) - (double)aL) + 0.5), g = ((double)aL + k) / (double)Le.  Otherwise
 *               g = (double)a1.  A NaN a1 or aL gives status NO_CARRIER: freq and phase are the quiet NaN, z_re, z_im, m2 and mm
 *               are 0, nothing is written to d_out; the lag sums stay what rule 2 gave.  Under FREQ_FIXED g = freq * (double)M.
 *               f = g / (double)M, which is exact; freq of the record is f.  g is M f, the turn of p per symbol: the estimator's
 *               range is |f| < 1 / (2 M) turns per symbol, and the long lag resolves it while the error of a1 stays below
 *               1 / (2 Le) turns.  n <= 1 has no term: R = 0, a1 = 0, f = 0.
 * 4. Rotation   fosphor_amd_cossin_turns(t, &c, &s) above: the cosine and sine of t turns.  A t that is not finite gives NaN for
 *               both.  r = t - floor(t); if !(r < 1.0), r = 0.0.  q = floor((r * 4.0) + 0.5); d = r - (q * 0.25);
 *               x = d * 6.283185307179586; z = x * x.  S = 1.0 / 17!; for k = 7 down to 0, S = (S * z) + s_k / (2k + 1)! with
 *               s_k = +1 for even k and -1 for odd k (a multiplication, then an addition); S = x * S: the Taylor series of sin x
 *               to x^17.  C = 1.0 / 16!; for k = 7 down to 0, C = (C * z) + s_k / (2k)!: cos x to x^16.  The quadrant
 *               (int)q & 3 selects (c, s) from (C, S), (-S, C), (-C, -S), (S, -C); - flips the sign bit.  |x| <= pi / 4, so the
 *               truncation is below 1e-17; the chain is within 2e-15 of cos and sin of 2 pi r (x carries at most 1.8e-16 from
 *               its one product, nine steps on values <= 1 add at most 1.1e-16 each; 1.9e-16 was seen over 2.2 M points).
 *               Seams: whole quarter turns have d = 0, x = +0, S = +0 and C = 1, so t = 0 (and every whole number, and -0)
 *               gives (1, +0), 1/4 gives (-0, 1), 1/2 gives (-1, -0), 3/4 gives (+0, -1); t = -1/4 is 3/4.  r >= 7/8 has q = 4
 *               and lands in quadrant 0 with d < 0.
 * 5. Phase sum  psi = g * (double)j; (c, sn) = cossin_turns(psi); v[j] = ((pr * c) + (pi * sn), (pi * c) - (pr * sn)): p[j] turned
 *               back by psi.  Z = the sum of v[j], m2 = the sum of w[j], mm = the sum of |s[j]|^M, each over j < n in the
 *               three-level order.  thM = fosphor_amd_atan2_turns(Zi, Zr); a NaN gives NO_CARRIER as in rule 3, except that z_re,
 *               z_im, m2 and mm stay.  theta = (double)thM / (double)M: phase of the record, known modulo 1 / M.  Under
 *               PHASE_FIXED theta is the job's phase and no angle is taken: Z is still computed, and a NaN in it changes no
 *               status.
 * 6. Derotate   phi = theta + (f * (double)j); (c, sn) = cossin_turns(phi); out[j] = ((float)((sr * c) + (si * sn)),
 *               (float)((si * c) - (sr * sn))): s[j] turned back by phi.
 *    Device     k_car_lag: 256 lanes own a tile of 4096 terms of a frequency-ESTIMATE job, found in a prefix of tile counts by a
 *               bounded binary search; 256 terms a pass, the pass's symbols (up to 256 + Le) brought into an LDS image of double
 *               pairs by 16-byte loads that read nothing outside the job and raised to M in place, once per symbol and pass; a
 *               wave's 64 terms of a pass are one block, four lanes add its terms serially, four lanes the tile's blocks; four
 *               doubles per tile go to the pass's scratch.  k_car_freq: a wave per job adds the tiles in ascending order, applies
 *               rule 3 and writes the job's state.  k_car_sum: tiles as in k_car_lag, over the symbols, for rule 5; every lane
 *               loads its own symbol; a tile of a NO_CARRIER job returns at once.  k_car_phase: a wave per job adds the tiles,
 *               finds theta and writes the record.  k_car_turn: rule 6 over the same tiles; a tile of a NO_CARRIER job returns at
 *               once; each lane stores 8 bytes, consecutive lanes to consecutive addresses.  The rows of terms are 65 doubles
 *               long, so that the four serial adders of a wave read different banks.  No sum of doubles crosses lanes in another
 *               order than the rules'.  At most five launches per call, whatever the number of jobs; a launch with no work is
 *               not made; no atomics, no work-group waits for another, every loop carries its bound.
 * 7. Access     reads touch only d_iq[offset .. offset + n) of each job; writes only d_records[0 .. n_jobs) and each job's
 *               d_out[out_offset .. out_offset + n).  Input ranges may overlap; output ranges must not.
 * 8. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, jobs, d_records or
 *               d_out; n_jobs outside 1 .. MAX_JOBS; n_samples or out_capacity below 0; a job with offset, out_offset or n below
 *               0, offset + n > n_samples, out_offset + n > out_capacity, an order that is not 2, 4 or 8, a lag outside
 *               1 .. MAX_LAG, a mode with other bits than the two, a freq or a phase that is not 0 without its bit, or with it
 *               is NaN, infinite or outside [-0.5, 0.5], or outputs over another job's; d_iq, d_out or d_records not 8-byte
 *               aligned; more than 2^31 - 1 work-groups in a launch.  Every check is safe against offsets of 2^62.
 * n = 0 gives status OK, zero sums, f = 0 and theta = 0 (or the job's), and writes nothing but the record.
 *
 * 0; -EINVAL (rule 8); -EIO. */
int fosphor_amd_carrier(struct fosphor *self, const void *d_iq, int64_t n_samples,
                        const struct fosphor_amd_carrier_job *jobs, int n_jobs,
                        struct fosphor_amd_carrier_record *d_records,
                        void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_carrier_host(const float *iq, int64_t n_samples,
                             const struct fosphor_amd_carrier_job *jobs, int n_jobs,
                             struct fosphor_amd_carrier_record *records,
                             float *out, int64_t out_capacity);

/* HOST only: the job over what a symbols job wrote into fosphor_amd_symbols' d_out: offset = out_offset of the symbols job,
 * n = n_sym of its record; out_offset = 0: the caller places it.  0; -EINVAL: a NULL pointer, out_offset < 0 in the job, n_sym < 0
 * in the record, and what rule 8 refuses of order, mode, lag, freq and phase. */
int fosphor_amd_carrier_from_symbols(const struct fosphor_amd_symbols_job *s, const struct fosphor_amd_symbols_record *r,
                                     int order, int mode, int lag, double freq, double phase,
                                     struct fosphor_amd_carrier_job *job);

/* HOST only: a record as Hz, radians and ratios, all in double; symbol_rate in symbols per second:
 *   freq_hz     freq symbol_rate
 *   phase_rad   2 pi phase
 *   sym_power   m2 / n
 *   lock        |Z| / mm: 1 for noiseless M-ary PSK whose frequency was found, near 0 without a carrier or with a wrong order
 *   lag_lock    |R1| n / mm^2: (n - 1) / n for noiseless constant-modulus symbols at any frequency; 0 under FREQ_FIXED
 *   lagl_lock   |RL| n / mm^2: (n - Le) / n likewise; 0 when lag_used <= 1
 * A field whose value is not finite is 0; every field is 0 when n == 0 or status is NO_CARRIER.
 * 0; -EINVAL: a NULL pointer, a symbol_rate that is not finite and positive. */
struct fosphor_amd_carrier_values
{
	double freq_hz, phase_rad, sym_power, lock, lag_lock, lagl_lock;
};
int fosphor_amd_carrier_derive(const struct fosphor_amd_carrier_record *r, double symbol_rate,
                               struct fosphor_amd_carrier_values *v);

/* HOST only: fosphor_amd_cossin_turns as the library compiled it, for callers that cannot include this header (one angle, and n
 * angles: c[i], s[i] = the cosine and sine of t[i] turns).  0; -EINVAL: a NULL pointer or n < 0. */
int fosphor_amd_carrier_cossin_turns(double t, double *c, double *s);
int fosphor_amd_carrier_cossin_turns_n(const double *t, int64_t n, double *c, double *s);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_CARRIER_CALLS]       fosphor_amd_carrier calls that reached the device
 *   stats[FOSPHOR_AMD_CARRIER_K_LAG]       launches of k_car_lag (none when no job that estimates its frequency has two symbols)
 *   stats[FOSPHOR_AMD_CARRIER_K_FREQ]      launches of k_car_freq (none when every job has FREQ_FIXED)
 *   stats[FOSPHOR_AMD_CARRIER_K_SUM]       launches of k_car_sum (none when every job has n = 0)
 *   stats[FOSPHOR_AMD_CARRIER_K_PHASE]     launches of k_car_phase
 *   stats[FOSPHOR_AMD_CARRIER_K_TURN]      launches of k_car_turn (none when every job has n = 0)
 *   stats[FOSPHOR_AMD_CARRIER_JOBS_FREQ]   jobs of those calls that estimate their frequency
 *   stats[FOSPHOR_AMD_CARRIER_JOBS_PHASE]  ... their phase
 *   stats[FOSPHOR_AMD_CARRIER_SYMBOLS]     the sum of n over those jobs */
enum {
	FOSPHOR_AMD_CARRIER_CALLS, FOSPHOR_AMD_CARRIER_K_LAG, FOSPHOR_AMD_CARRIER_K_FREQ, FOSPHOR_AMD_CARRIER_K_SUM,
	FOSPHOR_AMD_CARRIER_K_PHASE, FOSPHOR_AMD_CARRIER_K_TURN, FOSPHOR_AMD_CARRIER_JOBS_FREQ, FOSPHOR_AMD_CARRIER_JOBS_PHASE,
	FOSPHOR_AMD_CARRIER_SYMBOLS,
	FOSPHOR_AMD_CARRIER_STATS
};
int fosphor_amd_carrier_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_CARRIER_STATS]);

#ifdef __cplusplus
}
#endif

#endif
