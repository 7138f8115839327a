/*
 * fosphor_amd_symbols.h -- where are this burst's symbols, and what are they: feed-forward symbol timing per job over burst IQ,
 * one complex sample per symbol and one record (timing, line, moments) per job
 *
 * fosphor_amd_extract leaves each emission's baseband IQ in a device buffer and fosphor_amd_resample brings it to a whole number of
 * samples per symbol, sps.  This pass takes the last step of that chain.  |y|^2 of a linearly modulated burst carries a line at the
 * symbol rate (the one FOSPHOR_AMD_PSD_PRE_MAGSQ shows); its phase is the symbol phase.  The pass folds |y|^2 modulo sps, takes
 * that one line with a host-built table, turns its angle into the symbol phase tau with the pinned fosphor_amd_atan2_turns
 * (fosphor_amd_demod.h), and then reads the burst at first + j sps + mu samples with a four-tap cubic Lagrange interpolator.  It is
 * feed-forward: one reduction, one angle, one fixed fractional delay per job, no loop that a sample's result feeds back into, so
 * up to 4096 bursts go in one call.  A job may also name its tau (FIXED) and take the interpolation alone.  The record holds what a
 * caller asks of the symbols next: their second and fourth moments (an SNR estimate for constant-modulus symbols) and the sums of
 * s^2 and s^4 (the residual carrier phase of BPSK and QPSK, and whether it is locked).
 *
 * Not this pass: carrier derotation (the offset that measure or psd found is mixed out in extract; what is left is a phase, in
 * derive), decisions, equalisers and every loop with feedback, a fractional sps (fosphor_amd_resample's work), and interpolators
 * longer than four taps.
 *
 * Conventions, those of fosphor_amd_psd.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_SYMBOLS_H
#define FOSPHOR_AMD_SYMBOLS_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_extract.h"
#include "fosphor_amd_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_SYMBOLS_MAX_JOBS 4096
#define FOSPHOR_AMD_SYMBOLS_MIN_SPS  2		/* FIXED only; ESTIMATE needs 3: at 2 the line sits at fs / 2 and its phase is a sign */
#define FOSPHOR_AMD_SYMBOLS_MAX_SPS  64
#define FOSPHOR_AMD_SYMBOLS_BLOCK    64		/* symbols of a block of the ordered sums (rules 1 and 6) */
#define FOSPHOR_AMD_SYMBOLS_TILE     4096	/* symbols of a tile: 64 blocks; tests plant symbol counts across both seams */
#define FOSPHOR_AMD_SYMBOLS_STAGE_SPS 8		/* up to here k_sym_pick stages its span in LDS, above it reads y[g - 1 .. g + 2] directly */

#define FOSPHOR_AMD_SYMBOLS_ESTIMATE 0		/* tau from the symbol-rate line of |y|^2 (rules 1 to 3) */
#define FOSPHOR_AMD_SYMBOLS_FIXED    1		/* tau from the job */

#define FOSPHOR_AMD_SYMBOLS_OK        0
#define FOSPHOR_AMD_SYMBOLS_NO_TIMING 1		/* the angle of the line is a NaN (rule 3): no symbol is written */

/* static LDS of a work-group of each kernel, bytes (tests/test_symbols_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_SYMBOLS_LDS_FOLD   33792	/* 65 x 64 doubles of |y|^2, a padded row per block, and 64 block sums */
#define FOSPHOR_AMD_SYMBOLS_LDS_TIME   2048	/* four waves, each 64 doubles of A */
#define FOSPHOR_AMD_SYMBOLS_LDS_PICK   31968	/* 2046 staged samples, four waves x 6 x 65 terms, 6 x 65 block sums */
#define FOSPHOR_AMD_SYMBOLS_LDS_RECORD 0

struct fosphor_amd_symbols_job			/* 40 bytes */
{
	int64_t offset;		/* index into d_iq  (complex samples) of y[0] */
	int64_t out_offset;	/* index into d_out (complex samples) of the job's first symbol */
	int32_t n;		/* input samples, >= 0 */
	int32_t sps;		/* samples per symbol, MIN_SPS .. MAX_SPS; ESTIMATE needs >= 3 */
	int32_t mode;		/* FOSPHOR_AMD_SYMBOLS_ESTIMATE or _FIXED */
	float   tau;		/* FIXED: the symbol phase in symbols, in [0, 1).  Must be 0 under ESTIMATE */
	int32_t reserved[2];	/* must be 0 */
};

struct fosphor_amd_symbols_record		/* 96 bytes, 8-byte aligned */
{
	int32_t n_sym;				/* symbols written (rule 4); 0 with NO_TIMING */
	int32_t first;				/* g of symbol 0 (rule 4); 0 with NO_TIMING */
	float   tau;				/* (float)e of rule 3; the quiet NaN with NO_TIMING */
	int32_t status;				/* FOSPHOR_AMD_SYMBOLS_OK or _NO_TIMING */
	double  mu;				/* the fractional delay in samples, in [0, 1) (rule 4); 0 with NO_TIMING */
	double  x_re, x_im;			/* the line X of rule 2; 0 under FIXED */
	double  a0;				/* the sum of the folded |y|^2 (rule 2); 0 under FIXED */
	double  m2, m4;				/* sums of |s|^2 and |s|^4 over the symbols (rule 6) */
	double  z2_re, z2_im, z4_re, z4_im;	/* sums of s^2 and s^4 */
};

/* The symbols of n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract and fosphor_amd_resample write
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity float32 (re, im) pairs, 8-byte aligned.  Job j RESERVES d_out[out_offset .. out_offset + max_out),
 *              max_out = n < 4 ? 0 : (n - 4) / sps + 1 (fosphor_amd_symbols_max_out): the most symbols any tau gives.  Only the
 *              first n_sym of them are written; n_sym is in the record
 * y[m] = d_iq[offset + m].
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_symbols_host and the numpy
 * model (tests/symbols_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels'
 * grid, not on repetition.  The build's -ffp-contract=off holds: every operation below is one IEEE double operation, rounded once,
 * in the order the parentheses give, and no fused multiply-add appears in this pass.  A NaN float is the quiet NaN 0x7fc00000 and a
 * NaN double of the record 0x7ff8000000000000, whatever the payloads were.
 *
 * 1. Fold       ESTIMATE only.  R = n / sps whole symbols; samples behind them are not read by this rule.  q[m] = (re * re) +
 *               (im * im) in double from the float32 parts widened: the products are exact, the sum rounds once.  A[k], k < sps,
 *               is the sum of q[r sps + k] over r < R in a three-level order: blocks of 64 consecutive r, r ascending, from 0.0;
 *               tiles of 64 blocks (FOSPHOR_AMD_SYMBOLS_TILE symbols), blocks ascending, from 0.0; the job, tiles ascending,
 *               from 0.0.  A block or a tile that the job ends in holds what the job has.
 * 2. Line       tw[k] = e^(-2 pi i k / sps), k < sps, is a table of doubles built on the host (fosphor_amd_symbols_twiddles) and
 *               used by the device, the host statement and the model alike; the entry point builds one per distinct sps of the
 *               call and uploads them behind the job table.  Xr = sum A[k] * twr[k], Xi = sum A[k] * twi[k], a0 = sum A[k], each
 *               with k ascending, from 0.0, each product rounded.
 * 3. Phase      a = fosphor_amd_atan2_turns(-Xi, Xr) (fosphor_amd_demod.h).  A NaN a gives status NO_TIMING: n_sym = 0, first
 *               = 0, mu = 0, tau the quiet NaN, zero moments, no output; x_re, x_im and a0 stay what rule 2 gave.  Otherwise, in
 *               double: e = a; if e < 0, e = e + 1.0; if !(e < 1.0), e = 0.0; e = e + 0.0 (a -0 becomes +0).  Under FIXED
 *               e = (double)tau and Xr, Xi and a0 are 0.  tau of the record is (float)e.
 * 4. Place      base = e * (double)sps; i0 = (int)floor(base); mu = base - (double)i0; first = i0 >= 1 ? i0 : sps;
 *               n_sym = n - 3 - first < 0 ? 0 : (n - 3 - first) / sps + 1.  Symbol j has g = first + j sps and is made of
 *               y[g - 1 .. g + 2] and of nothing else of the input; it sits first + j sps + mu samples from y[0].  (With i0 = 0
 *               the symbol at mu would need y[-1]: it is dropped and the next one is symbol 0.)
 * 5. Interpolate  cubic Lagrange, in double, the coefficients once per job: u = mu + 1.0, b = mu - 1.0, c = mu - 2.0,
 *                   c_1 = -(((mu * b) * c) / 6.0)     for y[g - 1]
 *                   c0  =   ((u * b) * c) / 2.0       for y[g]
 *                   c1  = -(((u * mu) * c) / 2.0)     for y[g + 1]
 *                   c2  =   ((u * mu) * b) / 6.0      for y[g + 2]
 *               and per component s = (((c_1 * y_1) + (c0 * y0)) + (c1 * y1)) + (c2 * y2), the samples widened to double.  The
 *               output is (float)s, re then im.
 * 6. Moments    from the float32 outputs widened to double, sr and si: w = (sr * sr) + (si * si); s^2 = ((sr * sr) - (si * si),
 *               (sr * si) + (sr * si)); s^4 the same rule applied to s^2 (SQUARE and FOURTH of fosphor_amd_psd.h).  m2 = sum w,
 *               m4 = sum w * w, z2 = sum s^2, z4 = sum s^4, each in the three-level order of rule 1 over the symbol index j.  A
 *               job with n_sym = 0 has zeros.
 *    Device     k_sym_fold: 256 lanes own a tile of 4096 sps samples of an ESTIMATE job, found in a prefix of tile counts by a
 *               bounded binary search; they walk it in pieces of 64 / sps whole blocks, write q in double into an LDS image with
 *               one row per block, padded by sps doubles so that the 64 / sps x sps serial block sums of a wave read different
 *               banks, and lane k adds the blocks; sps doubles per tile go to the pass's scratch.  k_sym_time: a wave per job;
 *               lane k adds its tiles in ascending order, then every lane computes rules 2 to 5 and lane 0 writes the job's
 *               state to the scratch.  k_sym_pick: 256 lanes own a tile of 4096 symbols of the RESERVED range -- n_sym is known
 *               on the device only -- and a tile at or behind n_sym returns at once; 256 symbols a pass, the span staged in LDS
 *               up to FOSPHOR_AMD_SYMBOLS_STAGE_SPS (by 16-byte loads that read nothing outside it), 8 bytes stored per lane,
 *               consecutive lanes to consecutive addresses; a wave's 64 symbols of a pass are one block, six lanes add its terms
 *               serially, six lanes the tile's blocks.  k_sym_record: a wave per job adds the tiles that exist in ascending order
 *               and writes the record.  No sum of doubles crosses lanes in another order than the rules'.  At most four launches
 *               per call, whatever the number of jobs; no atomics, no work-group waits for another, every loop carries its bound.
 * 7. Access     reads touch only d_iq[offset .. offset + (n / sps) sps) (ESTIMATE) and y[first - 1 .. first + (n_sym - 1) sps
 *               + 3) of each job; writes only d_records[0 .. n_jobs) and each job's d_out[out_offset .. out_offset + n_sym).
 *               Input ranges may overlap; reserved output ranges must not.
 * 8. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, jobs, d_records or
 *               d_out; n_jobs outside 1 .. MAX_JOBS; n_samples or out_capacity below 0; a job with offset, out_offset or n below
 *               0, offset + n > n_samples, sps outside MIN_SPS .. MAX_SPS, sps = 2 under ESTIMATE, an unknown mode, a tau that is
 *               NaN or outside [0, 1) or not 0 under ESTIMATE, reserved != 0, out_offset + max_out > out_capacity, or a reserved
 *               range over another job's; d_iq, d_out or d_records not 8-byte aligned; more than 2^31 - 1 work-groups in a
 *               launch (MAX_JOBS jobs of 2^31 - 1 samples stay below it; the check stands for other limits).  Every check is
 *               safe against offsets of 2^62.
 *
 * 0; -EINVAL (rule 8); -EIO. */
int fosphor_amd_symbols(struct fosphor *self, const void *d_iq, int64_t n_samples,
                        const struct fosphor_amd_symbols_job *jobs, int n_jobs,
                        struct fosphor_amd_symbols_record *d_records,
                        void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_symbols_host(const float *iq, int64_t n_samples,
                             const struct fosphor_amd_symbols_job *jobs, int n_jobs,
                             struct fosphor_amd_symbols_record *records,
                             float *out, int64_t out_capacity);

/* HOST only: max_out of a job, n < 4 ? 0 : (n - 4) / sps + 1, or -EINVAL: n < 0, sps outside MIN_SPS .. MAX_SPS. */
int fosphor_amd_symbols_max_out(int32_t n, int sps);

/* HOST only: the table of rule 2 as sps (re, im) pairs of doubles, out[2 k] + i out[2 k + 1] = e^(-2 pi i k / sps).  The angle is
 * reduced in integers to the first octant, evaluated there in long double and rounded once; the rest follows by swapping and
 * negating, so the table is exact at whole quarter turns -- (1, 0), (0, -1), (-1, 0), (0, 1) -- every zero is +0, and an eighth
 * turn has two equal parts.  0; -EINVAL: sps outside MIN_SPS .. MAX_SPS, a NULL out. */
int fosphor_amd_symbols_twiddles(int sps, double *out);

/* HOST only: the job over what an extract job wrote into fosphor_amd_extract's d_out, or a resample job into
 * fosphor_amd_resample's: offset = out_offset of the source, n = its n_out; out_offset = 0: the caller places it.
 * 0; -EINVAL: a NULL pointer, out_offset < 0 or n_out < 0 in the source, and what rule 8 refuses of sps, mode and tau. */
int fosphor_amd_symbols_from_extract(const struct fosphor_amd_extract_job *e, int sps, int mode, float tau,
                                     struct fosphor_amd_symbols_job *job);
int fosphor_amd_symbols_from_resample(const struct fosphor_amd_resample_job *r, int sps, int mode, float tau,
                                      struct fosphor_amd_symbols_job *job);

/* HOST only: a record as seconds, Hz, dB and radians, all in double; fs = sample_rate of the samples the job read, sps the job's
 * (the record has no room for it):
 *   tau           tau of the record, in symbols
 *   t_first       (first + mu) / fs: symbol 0 behind y[0]
 *   symbol_rate   fs / sps
 *   timing_depth  2 |X| / a0: the depth of the symbol-rate line in |y|^2; 0 under FIXED
 *   sym_power     m2 / n_sym
 *   snr_db        the M2M4 estimate for constant-modulus symbols: with M2 = m2 / n_sym and M4 = m4 / n_sym, S = sqrt(2 M2^2 - M4),
 *                 N = M2 - S, 10 log10(S / N); 0 when 2 M2^2 - M4, S or N is not positive
 *   phase2        arg(z2) / 2, radians: the symbols' phase modulo pi (BPSK)
 *   lock2         |z2| / m2: 1 for BPSK at any phase, near 0 for QPSK
 *   phase4        arg(z4) / 4, radians: the symbols' phase modulo pi / 2, with QPSK at +-1 +-i read as pi / 4
 *   lock4         |z4| / m4: 1 for QPSK and BPSK
 * A field whose value is not finite is 0; every field but tau and symbol_rate is 0 when n_sym == 0.
 * 0; -EINVAL: a NULL pointer, sps outside MIN_SPS .. MAX_SPS, a sample_rate that is not finite and positive. */
struct fosphor_amd_symbols_values
{
	double tau, t_first, symbol_rate, timing_depth, sym_power, snr_db, phase2, lock2, phase4, lock4;
};
int fosphor_amd_symbols_derive(const struct fosphor_amd_symbols_record *r, int sps, double sample_rate,
                               struct fosphor_amd_symbols_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_SYMBOLS_CALLS]          fosphor_amd_symbols calls that reached the device
 *   stats[FOSPHOR_AMD_SYMBOLS_K_FOLD]         launches of k_sym_fold (none when no job has a whole symbol to fold)
 *   stats[FOSPHOR_AMD_SYMBOLS_K_TIME]         launches of k_sym_time
 *   stats[FOSPHOR_AMD_SYMBOLS_K_PICK]         launches of k_sym_pick (none when max_out is 0 for every job)
 *   stats[FOSPHOR_AMD_SYMBOLS_K_RECORD]       launches of k_sym_record
 *   stats[FOSPHOR_AMD_SYMBOLS_JOBS_ESTIMATE]  jobs of those calls under ESTIMATE
 *   stats[FOSPHOR_AMD_SYMBOLS_JOBS_FIXED]     ... under FIXED
 *   stats[FOSPHOR_AMD_SYMBOLS_SAMPLES]        the sum of n over those jobs
 *   stats[FOSPHOR_AMD_SYMBOLS_SYMBOLS]        the sum of n_sym over those jobs, read back from the device at the end of a call */
enum {
	FOSPHOR_AMD_SYMBOLS_CALLS, FOSPHOR_AMD_SYMBOLS_K_FOLD, FOSPHOR_AMD_SYMBOLS_K_TIME, FOSPHOR_AMD_SYMBOLS_K_PICK,
	FOSPHOR_AMD_SYMBOLS_K_RECORD, FOSPHOR_AMD_SYMBOLS_JOBS_ESTIMATE, FOSPHOR_AMD_SYMBOLS_JOBS_FIXED, FOSPHOR_AMD_SYMBOLS_SAMPLES,
	FOSPHOR_AMD_SYMBOLS_SYMBOLS,
	FOSPHOR_AMD_SYMBOLS_STATS
};
int fosphor_amd_symbols_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_SYMBOLS_STATS]);

#ifdef __cplusplus
}
#endif

#endif
