/*
 * fosphor_amd_psd.h -- what does this burst's spectrum look like at its own rate: a Welch power spectrum per job over burst IQ,
 * one record (peak, occupied bandwidth, x-dB bandwidth, spectral moments) and optionally one trace per job
 *
 * fosphor_amd_extract leaves each emission's baseband IQ in a device buffer at the burst's own, decimated rate.  The waterfall's
 * columns have the stream's resolution, not the burst's, and fosphor_amd_measure says where the carrier is and nothing about the
 * width.  This pass cuts each job's range y into segments of L = 64 .. 1024 samples, hop samples apart, multiplies each by the
 * job's window, transforms it in double and averages |X|^2 over the segments: Welch's method.  The record holds the figures of a
 * spectrum analyser -- peak, 99 % occupied bandwidth, x-dB bandwidth, centroid and RMS width -- and the trace, if asked for, the
 * averaged spectrum in float32, DC in the middle.  A pre-transform applied to each sample first -- y^2, y^4 or |y|^2 -- gives the
 * classic lines of carrier recovery (twice and four times the offset), of the modulation order and of the symbol rate.  It is the
 * one step of the chain with an FFT in it: a batched radix-2 FFT in double, in LDS.
 *
 * Not this pass: transforms beyond FOSPHOR_AMD_PSD_MAX_LOG (average shorter segments, or decimate further), detrending, a
 * logarithmic trace (10 log10 of a float is the caller's), and the symbol timing itself, which starts from the line that
 * FOSPHOR_AMD_PSD_PRE_MAGSQ shows: fosphor_amd_symbols (fosphor_amd_symbols.h) takes that one line and gives the symbols.
 *
 * Conventions, those of fosphor_amd_correlate.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_PSD_H
#define FOSPHOR_AMD_PSD_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_extract.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_PSD_MAX_JOBS 4096
#define FOSPHOR_AMD_PSD_MIN_LOG  6		/* L = 64 .. */
#define FOSPHOR_AMD_PSD_MAX_LOG  10		/* .. 1024 */
#define FOSPHOR_AMD_PSD_TILE     32		/* segments of a tile (rule 4); tests plant segment counts across this seam */

#define FOSPHOR_AMD_PSD_PRE_NONE   0		/* z = y */
#define FOSPHOR_AMD_PSD_PRE_SQUARE 1		/* z = y^2 */
#define FOSPHOR_AMD_PSD_PRE_FOURTH 2		/* z = y^4 */
#define FOSPHOR_AMD_PSD_PRE_MAGSQ  3		/* z = |y|^2 */

#define FOSPHOR_AMD_PSD_TRACE_NONE  0		/* the record only */
#define FOSPHOR_AMD_PSD_TRACE_POWER 1		/* L float32: P32 of rule 4; none when the job has no segment */

#define FOSPHOR_AMD_PSD_WINDOW_RECT            0
#define FOSPHOR_AMD_PSD_WINDOW_HANN            1
#define FOSPHOR_AMD_PSD_WINDOW_BLACKMAN_HARRIS 2	/* the four-term, -92 dB one */

/* static LDS of a work-group of each kernel, bytes (tests/test_psd_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_PSD_LDS_GROUP   37904	/* L <= 1024: the image of 1088 + 1088 doubles, 1026 staged samples, 1024 window floats, 512 twiddles */
#define FOSPHOR_AMD_PSD_LDS_WAVE    19008	/* four waves, each L <= 128: 136 + 136 doubles, 130 samples, 128 floats, 64 twiddles */
#define FOSPHOR_AMD_PSD_LDS_COMBINE 22528	/* four waves, each 1024 floats of P32 and 3 x 64 block sums */

struct fosphor_amd_psd_job			/* 56 bytes */
{
	int64_t offset;		/* index into d_iq  (complex samples) of y[0] */
	int64_t out_offset;	/* index into d_out (floats) of the trace; must be 0 with TRACE_NONE */
	int64_t win_offset;	/* index into d_win (floats) of w[0]; the job's window is d_win[win_offset .. win_offset + L) */
	int32_t n;		/* input samples, >= 0 */
	int32_t fft_len_log;	/* log2 L, MIN_LOG .. MAX_LOG */
	int32_t hop;		/* samples from one segment to the next, 1 .. L */
	int32_t pre;		/* FOSPHOR_AMD_PSD_PRE_* */
	int32_t trace;		/* FOSPHOR_AMD_PSD_TRACE_* */
	float   obw_fraction;	/* of the total power inside the occupied bandwidth, in (0, 1]; 0.99 is the usual one */
	float   xdb_ratio;	/* a LINEAR power ratio in (0, 1]: fosphor_amd_psd_ratio_from_db(-26.0); no pow runs on the device */
	int32_t reserved;	/* not read */
};

struct fosphor_amd_psd_record			/* 64 bytes, 8-byte aligned */
{
	int32_t n_seg;				/* rule 1 */
	int32_t fft_len;			/* L */
	int32_t peak_bin;			/* trace index of the peak (DC is L / 2); -1 when no P32 is a number */
	float   peak_power;			/* P32 there; 0.0f when none */
	int32_t obw_lo, obw_hi;			/* rule 5; -1 unless total is finite and > 0 */
	int32_t xdb_lo, xdb_hi;			/* rule 5; -1 without a peak */
	double  total, m1, m2;			/* sum of P, of (i - L/2) P, of (i - L/2)^2 P over the trace */
	double  win_energy;			/* U of rule 4 */
};

/* The power spectra of n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, 8-byte aligned: exactly what fosphor_amd_extract writes
 *   d_win      n_win floats, 4-byte aligned: the windows (fosphor_amd_psd_window makes one); jobs may share one
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity floats, 4-byte aligned; job j owns d_out[out_offset .. out_offset + n_out), n_out = L with
 *              TRACE_POWER and n_seg > 0, else 0.  NULL, with capacity 0, when every job has TRACE_NONE
 * y[m] = d_iq[offset + m]; w[i] = d_win[win_offset + i]; L = 2^fft_len_log.
 *
 * Every output -- each trace float and the whole record -- is BIT-IDENTICAL between the device, fosphor_amd_psd_host and the numpy
 * model (tests/psd_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels' grid,
 * not on repetition.  The build's -ffp-contract=off holds: every operation below is one IEEE double operation, rounded once, in
 * the order the parentheses give, and no fused multiply-add appears in this pass.
 *
 * 1. Segments   n_seg = n < L ? 0 : (n - L) / hop + 1.  Segment s is y[s hop .. s hop + L).  Samples behind the last whole
 *               segment are not read.
 * 2. Pre        per sample, in double, from the float32 parts re and im widened:
 *                   NONE    zr = re, zi = im
 *                   SQUARE  zr = (re * re) - (im * im), zi = (re * im) + (re * im)
 *                   FOURTH  the SQUARE rule applied again to the zr and zi of SQUARE
 *                   MAGSQ   zr = (re * re) + (im * im), zi = +0.0
 *               then x[i] = ((double)w[i] * zr, (double)w[i] * zi).
 * 3. FFT        radix 2, decimation in time, pinned as an operation tree (the data flow is the implementation's).  tw[m] =
 *               e^(-2 pi i m / 1024), m < 512, is ONE table of doubles, built on the host (fosphor_amd_psd_twiddles) and used by
 *               the device, the host statement and the model alike.  a0[i] = x[bitrev(i)] over log2 L bits.  Stage t = 1 ..
 *               log2 L, h = 2^(t - 1); for every block base k (a multiple of 2 h) and j < h:
 *                   W = tw[j * (512 / h)],  u = a[k + j],  v = a[k + j + h]
 *                   tr = (Wr * vr) - (Wi * vi),  ti = (Wr * vi) + (Wi * vr)
 *                   a'[k + j] = (ur + tr, ui + ti),  a'[k + j + h] = (ur - tr, ui - ti)
 *               Every butterfly multiplies -- no shortcut for W = 1 or -i -- so non-finite samples propagate exactly as IEEE
 *               arithmetic does.  X = a after the last stage; p_s[b] = (Xr * Xr) + (Xi * Xi).
 * 4. Average    tile c holds segments 32 c .. min(32 c + 32, n_seg).  T_c[b] = the sum of p_s[b] over the tile's segments, s
 *               ascending, from 0.0; S[b] = the sum of T_c[b] over the tiles, c ascending, from 0.0.  U = the sum of
 *               (double)w[i] * (double)w[i], i ascending, from 0.0: win_energy.  den = (double)n_seg * U.
 *               P32[i] = (float)(S[b] / den), b = (i + L / 2) mod L: the trace runs in ascending frequency, DC at index L / 2;
 *               with den == 0 it is +0.0f.  A NaN float is the quiet NaN 0x7fc00000 whatever the payloads were, and a NaN double
 *               of the record is 0x7ff8000000000000.  By Parseval, total / L is the mean power of the windowed signal over the
 *               mean power of the window.
 * 5. Record     a function of the P32 values alone, P[i] = (double)P32[i], d = (double)(i - L / 2).  The sums total = sum P[i],
 *               m1 = sum d * P[i], m2 = sum (d * d) * P[i] each run in a two-level order: 64 blocks of L / 64 consecutive
 *               indices; inside block k a running sum `run`, i ascending, from 0.0, whose last value is B[k]; base[0] = 0.0,
 *               base[k] = base[k - 1] + B[k - 1]; cum[i] = base[k] + run (run with P[i] in it); the sum is base[63] + B[63].
 *               Peak: the largest non-NaN P32 at the smallest index, or peak_bin = -1, peak_power = 0.0f if there is none.
 *               Occupied bandwidth, in double: t = (1.0 - (double)obw_fraction) * 0.5, lo_thr = total * t, hi_thr = total -
 *               lo_thr; obw_lo is the smallest i with cum[i] > lo_thr and obw_hi the smallest i with cum[i] >= hi_thr (cum of
 *               total's sum); both are -1 unless total is finite and > 0.  level = peak_power * xdb_ratio, one float32
 *               multiply; xdb_lo and xdb_hi are the smallest and the largest i with P32[i] >= level, both -1 without a peak.
 *               A job with n_seg == 0 writes no trace; its record is zeros with the -1 indices, plus fft_len and win_energy.
 *               The record carries float32's rounding: total / L is the mean power to 2^-24 relative, not to a double's.
 *    Device     a tile is owned by 256 lanes (L >= 256, the GROUP form: k_psd_group) or by one wave, four tiles to
 *               a work-group (L <= 128, the WAVE form: k_psd_wave), found in a prefix of tile counts by a bounded binary search.
 *               Per segment the samples come by 16-byte loads that read nothing outside the span, pre and window put the
 *               bit-reversed image of L complex doubles into LDS, the stages run with one barrier each (none across waves in the
 *               WAVE form), and each lane adds its L / 256 (L / 64) bins of p in registers.  T_c goes to the pass's scratch,
 *               consecutive lanes to consecutive addresses.  k_psd_combine, one wave per job, adds the tiles in ascending order,
 *               divides, writes the trace, keeps P32 in LDS and computes the record: lane k owns block k, the 64 block sums
 *               are prefixed serially, minima, maxima and the peak pair meet by shuffles.  No sum of doubles crosses lanes in
 *               another order than this rule's.  At most three launches per call, whatever the number of jobs; no atomics, no
 *               work-group waits for another, every loop carries its bound.  The scratch holds 8 L bytes per tile; a call
 *               whose tiles need more than the device can give (hop 1 over 2^31 samples is 32 GiB) ends in -EIO.
 * 6. Access     reads touch only d_iq[offset .. offset + (n_seg - 1) hop + L) of each job with n_seg > 0 and its window
 *               d_win[win_offset .. win_offset + L); writes only d_records[0 .. n_jobs) and each job's d_out[out_offset ..
 *               out_offset + n_out).  Input ranges may overlap; output ranges must not.
 * 7. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, d_win, jobs or
 *               d_records; a NULL d_out while some job has TRACE_POWER; n_jobs outside 1 .. MAX_JOBS; n_samples, n_win or
 *               out_capacity below 0; a job with offset, out_offset or win_offset < 0, n < 0, offset + n > n_samples,
 *               fft_len_log outside MIN_LOG .. MAX_LOG, win_offset + L > n_win, hop outside 1 .. L, an unknown pre or trace,
 *               obw_fraction or xdb_ratio NaN or outside (0, 1], out_offset != 0 with TRACE_NONE, out_offset + n_out >
 *               out_capacity, or outputs over another job's; d_iq or d_records not 8-byte aligned; d_win or d_out not 4-byte
 *               aligned; more than 2^31 - 1 tiles (hence work-groups) in a form.  Every check is safe against offsets of 2^62.
 *
 * 0; -EINVAL (rule 7); -EIO. */
int fosphor_amd_psd(struct fosphor *self, const void *d_iq, int64_t n_samples,
                    const float *d_win, int64_t n_win,
                    const struct fosphor_amd_psd_job *jobs, int n_jobs,
                    struct fosphor_amd_psd_record *d_records,
                    float *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_psd_host(const float *iq, int64_t n_samples, const float *win, int64_t n_win,
                         const struct fosphor_amd_psd_job *jobs, int n_jobs,
                         struct fosphor_amd_psd_record *records, float *out, int64_t out_capacity);

/* HOST only: n_seg of rule 1, or -EINVAL: n < 0, fft_len_log outside MIN_LOG .. MAX_LOG, hop outside 1 .. L. */
int fosphor_amd_psd_n_seg(int32_t n, int fft_len_log, int hop);

/* HOST only: a window of L floats in periodic form (the phase is 2 pi i / L, so that overlapped segments add up flat), designed in
 * double and rounded once to float32:
 *   RECT             1
 *   HANN             0.5 - 0.5 cos(x)
 *   BLACKMAN_HARRIS  0.35875 - 0.48829 cos(x) + 0.14128 cos(2 x) - 0.01168 cos(3 x)
 * 0; -EINVAL: an unknown kind, fft_len_log out of range, a NULL out. */
int fosphor_amd_psd_window(int kind, int fft_len_log, float *out);

/* HOST only: the table of rule 3 as 512 (re, im) pairs of doubles, out[2 m] + i out[2 m + 1] = e^(-2 pi i m / 1024).  Built in
 * double with exact symmetries: the first octant comes from cos and sin, the rest by swapping and negating, so tw[0] = (1, +0),
 * tw[256] = (+0, -1), tw[128] = (r, -r) with r = sqrt(0.5), Re tw[m] = -Im tw[256 - m] and tw[256 + m] = (Im tw[m], -Re tw[m]).
 * 0; -EINVAL: a NULL out. */
int fosphor_amd_psd_twiddles(double *out);

/* HOST only: the job over what an extract job wrote into fosphor_amd_extract's d_out: offset = out_offset of e, n = n_out of e;
 * out_offset = 0: the caller places it.  0; -EINVAL: a NULL pointer, out_offset < 0 or n_out < 0 in e, win_offset < 0, and what
 * rule 7 refuses of fft_len_log, hop, pre, trace, obw_fraction and xdb_ratio. */
int fosphor_amd_psd_from_extract(const struct fosphor_amd_extract_job *e, int64_t win_offset, int fft_len_log, int hop, int pre,
                                 int trace, float obw_fraction, float xdb_ratio, struct fosphor_amd_psd_job *job);

/* HOST only: 10^(db / 10) for db <= 0, as xdb_ratio wants it: -3.0 gives 0.501..., -26.0 gives 0.00251...  A db above 0 or a NaN
 * gives NaN, and a db so low that the ratio rounds to 0 as a float gives 0: the entry points refuse both. */
double fosphor_amd_psd_ratio_from_db(double db);

/* HOST only: a record as Hz and dB, all in double; fs = sample_rate, frequencies are relative to the burst's centre:
 *   mean_power     total / L
 *   peak_freq      (peak_bin - L / 2) fs / L
 *   peak_db        10 log10(peak_power)
 *   centroid       m1 / total * fs / L
 *   rms_width      sqrt(max(m2 / total - (m1 / total)^2, 0)) fs / L
 *   obw            (obw_hi - obw_lo + 1) fs / L
 *   obw_centre     ((obw_lo + obw_hi) / 2 - L / 2) fs / L
 *   xdb_bandwidth  (xdb_hi - xdb_lo + 1) fs / L
 * Every field is 0 when n_seg == 0 or total is not finite and positive.
 * 0; -EINVAL: a NULL pointer, a sample_rate that is not finite and positive. */
struct fosphor_amd_psd_values
{
	double mean_power, peak_freq, peak_db, centroid, rms_width, obw, obw_centre, xdb_bandwidth;
};
int fosphor_amd_psd_derive(const struct fosphor_amd_psd_record *r, double sample_rate, struct fosphor_amd_psd_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_PSD_CALLS]      fosphor_amd_psd calls that reached the device
 *   stats[FOSPHOR_AMD_PSD_K_GROUP]    launches of the GROUP-form tile kernel
 *   stats[FOSPHOR_AMD_PSD_K_WAVE]     launches of the WAVE-form tile kernel
 *   stats[FOSPHOR_AMD_PSD_K_COMBINE]  launches of the kernel that adds the tiles and writes traces and records
 *   stats[FOSPHOR_AMD_PSD_JOBS]       jobs of those calls (n_seg = 0 included)
 *   stats[FOSPHOR_AMD_PSD_SEGMENTS]   the sum of n_seg over those jobs */
enum {
	FOSPHOR_AMD_PSD_CALLS, FOSPHOR_AMD_PSD_K_GROUP, FOSPHOR_AMD_PSD_K_WAVE, FOSPHOR_AMD_PSD_K_COMBINE, FOSPHOR_AMD_PSD_JOBS,
	FOSPHOR_AMD_PSD_SEGMENTS,
	FOSPHOR_AMD_PSD_STATS
};
int fosphor_amd_psd_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_PSD_STATS]);

#ifdef __cplusplus
}
#endif

#endif
