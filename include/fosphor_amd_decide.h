/*
 * fosphor_amd_decide.h -- the data of a burst: hard PSK decisions over the derotated symbols of a burst, the 1 / M ambiguity taken
 * out by differential decoding or by a unique word, optional Gray demapping, one byte per symbol and one record (unique word's
 * place, rotation and errors, decision histogram, the sums of the error-vector magnitude) per job
 *
 * fosphor_amd_carrier leaves symbols whose constellation points lie at k / M turns, k unknown by a constant.  This pass takes the
 * last step of the chain extract -> resample -> symbols -> carrier -> decide: the nearest point per symbol (rule 1), the sums from
 * which gain, EVM and residual phase follow (rule 2), and what removes the constant: the difference of consecutive indices (rule 3)
 * or the rotation under which a known word is found (rule 4).  Nothing a symbol's result feeds back into, so up to 4096 bursts go
 * in one call.
 *
 * Not this pass: other constellations than M-ary PSK, error correction, and words longer than FOSPHOR_AMD_DECIDE_MAX_UW.  Soft
 * decisions over the same symbols are fosphor_amd_soft.h.
 *
 * Conventions, those of fosphor_amd_carrier.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_DECIDE_H
#define FOSPHOR_AMD_DECIDE_H

#include <math.h>
#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_carrier.h"		/* fosphor_amd_cossin_turns, fosphor_amd_atan2_turns, the carrier job and record */

#define FOSPHOR_AMD_DECIDE_MAX_JOBS     4096
#define FOSPHOR_AMD_DECIDE_MAX_UW       64	/* symbols of one unique word */
#define FOSPHOR_AMD_DECIDE_MAX_UW_TABLE 65536	/* entries of the call's unique-word table */
#define FOSPHOR_AMD_DECIDE_BLOCK        64	/* symbols of a block of the ordered sums (rule 2) */
#define FOSPHOR_AMD_DECIDE_TILE         4096	/* symbols of a tile: 64 blocks; tests plant symbol counts across both seams */
#define FOSPHOR_AMD_DECIDE_UW_GROUP     256	/* candidate positions of a work-group of k_dec_uw; tests plant windows across this seam */

#define FOSPHOR_AMD_DECIDE_DIFF 1		/* flag bits; 0 = the indices as decided */
#define FOSPHOR_AMD_DECIDE_GRAY 2
#define FOSPHOR_AMD_DECIDE_UW   4

#define FOSPHOR_AMD_DECIDE_OK    0
#define FOSPHOR_AMD_DECIDE_NO_UW 1		/* no candidate position, or more than uw_max_errors errors at the best one */

/* static LDS of a work-group of each kernel, bytes (tests/test_decide_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_DECIDE_LDS_HARD 7904	/* four waves x 3 x 65 terms; 3 x 65 block sums; four waves x 3 packed counts */
#define FOSPHOR_AMD_DECIDE_LDS_UW   752		/* 81 words of decisions, 320 differences, 64 symbols of the word, four keys */
#define FOSPHOR_AMD_DECIDE_LDS_JOB  0
#define FOSPHOR_AMD_DECIDE_LDS_OUT  0

#ifdef __cplusplus
extern "C" {
#endif

struct fosphor_amd_decide_job			/* 64 bytes */
{
	int64_t offset;		/* index into d_iq (complex samples) of the job's symbol 0 */
	int64_t out_offset;	/* index into d_out in BYTES of its first output, a multiple of 4 */
	int32_t n;		/* symbols, >= 0 */
	int32_t order;		/* M: 2 (BPSK), 4 (QPSK) or 8 (8PSK) */
	int32_t flags;		/* 0 or a sum of FOSPHOR_AMD_DECIDE_DIFF, _GRAY and _UW */
	int32_t uw_offset;	/* UW: index into the call's table of the word's first symbol */
	int32_t uw_len;		/* UW: symbols of the word, 1 .. MAX_UW */
	int32_t uw_first;	/* UW: the first candidate position */
	int32_t uw_count;	/* UW: candidate positions from uw_first on; 0 = to the end of the job */
	int32_t uw_max_errors;	/* UW: more errors than this at the best position give NO_UW */
	int32_t reserved[4];	/* must be 0 */
};

struct fosphor_amd_decide_record		/* 96 bytes, 8-byte aligned */
{
	int32_t n;		/* the job's */
	int32_t order;		/* the job's */
	int32_t flags;		/* the job's */
	int32_t status;		/* FOSPHOR_AMD_DECIDE_OK or _NO_UW */
	int32_t uw_pos;		/* rule 4: the position of the word, -1 when none */
	int32_t uw_rot;		/* rule 4: the rotation taken out of every output */
	int32_t uw_errors;	/* rule 4: symbols of the word that do not match there */
	int32_t erasures;	/* rule 1: symbols with a NaN part */
	double  a, b, m2;	/* rule 2 */
	int32_t hist[8];	/* rule 1: decisions per index, before any rotation; hist[M ..] is 0 */
	int32_t reserved[2];	/* 0 */
};

/* Decisions of n_jobs ranges of d_iq.  jobs and uw: HOST memory; uw holds n_uw constellation indices, one byte each, and may be
 * NULL only when n_uw == 0.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, one per symbol, 8-byte aligned: exactly what fosphor_amd_carrier writes
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity bytes, 4-byte aligned.  Job j owns d_out[out_offset .. out_offset + 4 ceil(n / 4))
 * s[j] = d_iq[offset + j], its float32 parts sr and si widened to double; M = order.
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_decide_host and the numpy
 * model (tests/decide_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels'
 * grid, not on repetition.  The build's -ffp-contract=off holds: every floating-point operation below is one IEEE double operation,
 * rounded once, in the order the parentheses give.  The only transcendentals are the two pinned inlines.  A NaN double of the record
 * is 0x7ff8000000000000, whatever the payloads were.
 *
 * 1. Decision   t = fosphor_amd_atan2_turns(si, sr), a float32.  k[j] = (int)floor(((double)t * (double)M) + 0.5) & (M - 1).  A NaN
 *               t (a NaN part of s) gives k[j] = 0 and counts one in erasures.  (0, 0) has the angle 0: k = 0, no erasure; a real
 *               part of -0 has the angle of half a turn, as for atan2: (-0, +-0) goes to M / 2.  An angle exactly between two
 *               points, (k + 0.5) / M, goes to k + 1; t = -0.5 and t = +0.5 both go to M / 2.  Infinite parts have angles.
 *               hist[i] counts the j with k[j] == i, erasures included, before any rotation; hist[M ..] is 0.
 * 2. Sums       (c, sn) = fosphor_amd_cossin_turns((double)k[j] / (double)M): the decided point.  a = the sum of
 *               (sr * c) + (si * sn), b = the sum of (si * c) - (sr * sn), m2 = the sum of (sr * sr) + (si * si), each over j < n
 *               in the three-level order of fosphor_amd_carrier.h rule 2: blocks of 64 consecutive j, j ascending, from 0.0;
 *               tiles of 64 blocks, blocks ascending, from 0.0; the job, tiles ascending, from 0.0.  A NaN in the sums changes no
 *               status.
 * 3. Difference with DIFF d[0] = k[0] and d[j] = (k[j] - k[j - 1]) & (M - 1); without it d = k.
 * 4. Word       with UW, u[i] = uw[uw_offset + i] for i < uw_len: constellation indices, before any Gray mapping.  The candidate
 *               positions p are uw_first <= p < uw_first + uw_count (uw_count == 0: to the end) with p + uw_len <= n, and p >= 1
 *               under DIFF (d[0] is no difference).  The candidate rotations r are 0 .. M - 1 without DIFF and 0 alone with it (a
 *               difference has no ambiguity left).  matches(p, r) = the number of i with ((d[p + i] - u[i] - r) & (M - 1)) == 0.
 *               The winner has the most matches; ties go to the smallest p, then to the smallest r.  uw_pos and uw_rot are the
 *               winner's, uw_errors = uw_len - matches.  No candidate position: uw_pos = -1, uw_rot = 0, uw_errors = uw_len,
 *               status NO_UW.  uw_errors > uw_max_errors: status NO_UW; the winner stays and the output is still written.
 *               Without UW: uw_pos = -1, uw_rot = 0, uw_errors = 0.  All of it is integer work: any order of evaluation gives
 *               the same bits.
 * 5. Output     q[j] = (d[j] - uw_rot) & (M - 1); v[j] = q ^ (q >> 1) with GRAY, else q.  Byte out_offset + j of d_out is v[j],
 *               j < n; the bytes behind it up to the next multiple of 4 are written 0: job j owns
 *               d_out[out_offset .. out_offset + 4 ceil(n / 4)).  On the device every store to d_out is one aligned 32-bit store
 *               of four symbols; there are no byte stores.
 *    Device     k_dec_hard: 256 lanes own a tile of 4096 symbols of a job, found in a prefix of tile counts by a bounded binary
 *               search; 256 symbols a pass, every lane loads its own symbol (8 bytes, consecutive lanes from consecutive addresses),
 *               decides it and forms its three terms; a wave's 64 terms of a pass are one block, three lanes add its terms
 *               serially out of rows of 65 doubles, three lanes the tile's blocks; four lanes' decisions go as one 32-bit word to
 *               the pass's scratch; the tile's three doubles, its histogram and its erasures (counted in packed 16-bit integer
 *               fields, reduced across lanes in any order) go there too.  k_dec_uw (only when a job with UW has a candidate): a
 *               work-group per 256 candidate positions brings the 256 + uw_len - 1 decisions they read (one more before them under
 *               DIFF) from scratch into LDS by aligned 32-bit loads, forms d there once, and every lane scores its position over
 *               all rotations at once: a count per value of (d[p + i] - u[i]) & (M - 1).  The work-group's best goes to scratch as
 *               one 64-bit integer key (matches, then the complement of p, then the complement of r): the largest key is rule 4's
 *               winner in any order of comparison.  k_dec_job: a wave per job adds the tiles' sums in ascending order and the
 *               integer counts, reduces the keys, and writes the whole record and the job's rotation.  k_dec_out: rules 3 and 5
 *               over the tiles; a lane reads the word of its four decisions and the word before it (the previous tile's last
 *               word lies before the tile's first in scratch) and makes one 32-bit store, consecutive lanes to consecutive
 *               addresses.  At most four launches per call, whatever the number of jobs; a launch with no work is not made; no
 *               atomics, no work-group waits for another, every loop carries its bound.
 * 6. Access     reads touch only d_iq[offset .. offset + n) of each job; writes only d_records[0 .. n_jobs) and each job's owned
 *               bytes.  Input ranges may overlap; owned output ranges must not.
 * 7. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_iq, jobs, d_records or
 *               d_out, a NULL uw with n_uw != 0; n_jobs outside 1 .. MAX_JOBS; n_samples, out_capacity or n_uw below 0; n_uw above
 *               MAX_UW_TABLE; a job with offset, out_offset or n below 0, offset + n > n_samples, its owned bytes outside
 *               out_capacity, an out_offset that is no multiple of 4, an order that is not 2, 4 or 8, flags with other bits than
 *               the three, reserved bytes that are not 0; with UW a uw_len outside 1 .. MAX_UW, a uw_offset below 0 or
 *               uw_offset + uw_len > n_uw, a symbol of the word >= M, a uw_first, uw_count or uw_max_errors below 0; without UW
 *               any of uw_offset, uw_len, uw_first, uw_count and uw_max_errors that is not 0; owned outputs over another job's;
 *               d_iq or d_records not 8-byte aligned, d_out not 4-byte aligned; more than 2^31 - 1 work-groups in a launch.
 *               Every check is safe against offsets of 2^62.
 * n = 0 gives status OK (NO_UW with UW, which has no candidate then), zero sums and counts and rule 4's values, and writes nothing
 * but the record.
 *
 * 0; -EINVAL (rule 7); -EIO. */
int fosphor_amd_decide(struct fosphor *self, const void *d_iq, int64_t n_samples,
                       const struct fosphor_amd_decide_job *jobs, int n_jobs,
                       const uint8_t *uw, int n_uw,
                       struct fosphor_amd_decide_record *d_records,
                       void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_decide_host(const float *iq, int64_t n_samples,
                            const struct fosphor_amd_decide_job *jobs, int n_jobs,
                            const uint8_t *uw, int n_uw,
                            struct fosphor_amd_decide_record *records,
                            uint8_t *out, int64_t out_capacity);

/* HOST only: the job over what a carrier job wrote into fosphor_amd_carrier's d_out: offset = out_offset of the carrier job,
 * n = n of its record if its status is FOSPHOR_AMD_CARRIER_OK, else 0 (nothing was written), order = the record's; out_offset = 0:
 * the caller places it.  0; -EINVAL: a NULL pointer, out_offset < 0 in the job, n < 0 in the record, and what rule 7 refuses of
 * order, flags and the uw_ fields without the table. */
int fosphor_amd_decide_from_carrier(const struct fosphor_amd_carrier_job *c, const struct fosphor_amd_carrier_record *r,
                                    int flags, int uw_offset, int uw_len, int uw_first, int uw_count, int uw_max_errors,
                                    struct fosphor_amd_decide_job *job);

/* HOST only: a record as ratios, dB and radians, all in double with libm; uw_len is the job's (0 without UW):
 *   gain           a / n: the mean length of the symbols along their decided points
 *   evm_rms        sqrt(max(m2 - a^2 / n, 0) / (a^2 / n)): the rms error vector over the rms reference at that gain
 *   mer_db         -20 log10(evm_rms)
 *   phase_err_rad  atan2(b, a): the mean residual phase against the decided points
 *   uw_error_rate  uw_errors / uw_len
 * A field whose value is not finite is 0; every field but uw_error_rate is 0 when n == 0.
 * 0; -EINVAL: a NULL pointer, uw_len outside 0 .. MAX_UW. */
struct fosphor_amd_decide_values
{
	double gain, evm_rms, mer_db, phase_err_rad, uw_error_rate;
};
int fosphor_amd_decide_derive(const struct fosphor_amd_decide_record *r, int uw_len, struct fosphor_amd_decide_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_DECIDE_CALLS]     fosphor_amd_decide calls that reached the device
 *   stats[FOSPHOR_AMD_DECIDE_K_HARD]    launches of k_dec_hard (none when every job has n = 0)
 *   stats[FOSPHOR_AMD_DECIDE_K_UW]      launches of k_dec_uw (none when no job with UW has a candidate position)
 *   stats[FOSPHOR_AMD_DECIDE_K_JOB]     launches of k_dec_job
 *   stats[FOSPHOR_AMD_DECIDE_K_OUT]     launches of k_dec_out (none when every job has n = 0)
 *   stats[FOSPHOR_AMD_DECIDE_JOBS_UW]   jobs of those calls with UW
 *   stats[FOSPHOR_AMD_DECIDE_SYMBOLS]   the sum of n over those jobs */
enum {
	FOSPHOR_AMD_DECIDE_CALLS, FOSPHOR_AMD_DECIDE_K_HARD, FOSPHOR_AMD_DECIDE_K_UW, FOSPHOR_AMD_DECIDE_K_JOB,
	FOSPHOR_AMD_DECIDE_K_OUT, FOSPHOR_AMD_DECIDE_JOBS_UW, FOSPHOR_AMD_DECIDE_SYMBOLS,
	FOSPHOR_AMD_DECIDE_STATS
};
int fosphor_amd_decide_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DECIDE_STATS]);

#ifdef __cplusplus
}
#endif

#endif
