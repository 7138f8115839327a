/*
 * fosphor_amd_soft.h -- the bits of a weak burst: the derotated symbols of fosphor_amd_carrier taken as the coded bits of a
 * punctured convolutional code with their reliabilities, one quantised soft value per coded bit (max-log over the PSK points),
 * depunctured, decoded by a soft-input Viterbi decoder over the whole frame and checked by a CRC; the decoded bits and one record
 * (steps, the cost of the decoded path, end state, both CRCs, the sums of the soft values) per job
 *
 * fosphor_amd_decide reduces every symbol to its nearest point and fosphor_amd_decode counts the bits that differ.  This pass
 * stands beside the two: it reads the same symbols that decide reads, keeps how far each lies from the decision boundaries, and
 * pays for a disagreement what the symbol says it is worth: the roughly 2 dB of a soft-input decoder.  The rotation and the gain
 * come from the decide record (fosphor_amd_soft_from_decide).  The chain is extract -> resample -> symbols -> carrier -> decide
 * -> soft.  A job's result depends on its job alone, so up to 4096 bursts go in one call.
 *
 * Word for word from fosphor_amd_decode.h, and not restated here: 4096 jobs a call, the limits MAX_STEPS and MAX_CALL_STEPS, the
 * conventions, alignment, ownership and the style of the refusals, and its rules 2 (depuncture), 3 (trellis; ties go to x = 0),
 * 4 (end), 5 (traceback), 6 (output) and 7 (CRC).  "Rule n" below is that header's rule n; the new rules are S1 to S3.
 *
 * Not this pass: differential decisions (a difference of two symbols has no soft value here: FOSPHOR_AMD_DECIDE_DIFF jobs stay
 * with fosphor_amd_decode), tail-biting, writing the soft values out, constellations other than 2-, 4- and 8-PSK, interleavers
 * (fosphor_amd_rs.h reads this pass's output and has the block interleaver, the scrambler and the Reed-Solomon code behind it),
 * reflected CRCs.
 */
#ifndef FOSPHOR_AMD_SOFT_H
#define FOSPHOR_AMD_SOFT_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_decode.h"			/* the limits, rules 2 to 7, the decide job and record */

#define FOSPHOR_AMD_SOFT_MAX_JOBS       FOSPHOR_AMD_DECODE_MAX_JOBS
#define FOSPHOR_AMD_SOFT_MAX_STEPS      FOSPHOR_AMD_DECODE_MAX_STEPS
#define FOSPHOR_AMD_SOFT_MAX_CALL_STEPS FOSPHOR_AMD_DECODE_MAX_CALL_STEPS	/* the survivor decisions are 8 bytes a step, the soft
									 * values 4: a call needs at most 32 MiB + 16 MiB of scratch */
#define FOSPHOR_AMD_SOFT_BLOCK          64		/* steps of a block of k_sft_acs and k_sft_trace; tests plant seams here */
#define FOSPHOR_AMD_SOFT_GROUP          256		/* steps of a work-group of k_sft_bits: one partial of the sums; seams here too */
#define FOSPHOR_AMD_SOFT_MAX_VALUE      127		/* |v| of rule S2 at the most */
#define FOSPHOR_AMD_SOFT_INF            33554432	/* 2^25: the metric of a state that cannot be reached yet */

#define FOSPHOR_AMD_SOFT_TERMINATED 1			/* flag bit: the encoder was driven back to state 0 by k - 1 tail bits */
#define FOSPHOR_AMD_SOFT_GRAY       2			/* flag bit: the symbols' labels are Gray coded (FOSPHOR_AMD_DECIDE_GRAY) */

#define FOSPHOR_AMD_SOFT_OK       FOSPHOR_AMD_DECODE_OK
#define FOSPHOR_AMD_SOFT_CRC_FAIL FOSPHOR_AMD_DECODE_CRC_FAIL
#define FOSPHOR_AMD_SOFT_SHORT    FOSPHOR_AMD_DECODE_SHORT

/* static LDS of a work-group of each kernel, bytes (tests/test_soft_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_SOFT_LDS_BITS  32			/* four waves x two words: the packed counts, the sum of |v| */
#define FOSPHOR_AMD_SOFT_LDS_ACS   0
#define FOSPHOR_AMD_SOFT_LDS_TRACE 0
#define FOSPHOR_AMD_SOFT_LDS_REC   0

#ifdef __cplusplus
extern "C" {
#endif

/* The decode job's fields under their names, and rot and scale.  Those fields and the two new ones are 68 bytes at the decode
 * job's types; the job stays 64 bytes, as every job of the chain, by order and flags being 16 bits wide here (their values are
 * at most 8 and 3) and by leaving out the reserved word. */
struct fosphor_amd_soft_job			/* 64 bytes */
{
	int64_t  offset;	/* index into d_iq (complex samples) of the job's symbol 0 */
	int64_t  out_offset;	/* index into d_out in BYTES of its first output, a multiple of 8 */
	int32_t  n;		/* symbols, >= 0 */
	int16_t  order;		/* M: 2, 4 or 8; b = log2 M coded bits a symbol */
	int16_t  flags;		/* 0 or a sum of FOSPHOR_AMD_SOFT_TERMINATED and _GRAY */
	int32_t  steps;		/* trellis steps T; 0 = as many as the symbols hold (rule 2) */
	uint8_t  k;		/* constraint length, 3 .. 7 */
	uint8_t  n_poly;	/* streams of the code: 2 or 3 */
	uint8_t  period;	/* steps of the puncture pattern, 1 .. 16 */
	uint8_t  crc_width;	/* w: 0 (none), 8, 16, 24 or 32 */
	uint16_t polys[3];	/* the generators, below 2^k (rule 3); polys[2] = 0 with two streams */
	uint16_t punct[3];	/* the puncture masks, below 2^period (rule 2); all bits set = nothing punctured */
	uint32_t crc_poly;	/* rule 7, below 2^w */
	uint32_t crc_init;
	uint32_t crc_xorout;
	int32_t  rot;		/* 0 .. M - 1: the rotation that decide found (uw_rot), taken out of the labels (rule S1) */
	float    scale;		/* soft units per unit of L (rule S2): finite and above 0 */
};

struct fosphor_amd_soft_record			/* 64 bytes, 8-byte aligned: the decode record with its reserved words in use */
{
	int32_t  n_steps;	/* T of rule 2 */
	int32_t  n_bits;	/* decoded bits written (rule 5) */
	int32_t  n_coded;	/* coded bits consumed: kept(T) */
	int32_t  status;	/* FOSPHOR_AMD_SOFT_OK, _CRC_FAIL or _SHORT */
	int32_t  end_state;	/* rule 4: where the traceback began */
	int32_t  metric;	/* rule 4 with the costs of rule S3: the sum of |v| over the sent bits that the decoded path overrules */
	int32_t  best_state;	/* rule 4 */
	int32_t  best_metric;
	uint32_t crc_calc;	/* rule 7 */
	uint32_t crc_recv;
	int32_t  k;		/* the job's */
	int32_t  flags;		/* the job's */
	int32_t  erasures;	/* rule S2: symbols with a NaN part, of the ceil(n_coded / b) symbols that hold a consumed bit */
	int32_t  saturated;	/* rule S2: sent bits with |v| = 127 */
	int64_t  abs_sum;	/* rule S2: the sum of |v| over the sent bits */
};

/* Decoded bits of n_jobs ranges of d_iq.  jobs: HOST memory.  DEVICE memory:
 *   d_iq       n_samples float32 (re, im) pairs, one per symbol, 8-byte aligned: exactly what fosphor_amd_carrier writes and
 *              fosphor_amd_decide reads
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity bytes, 8-byte aligned.  Job j owns d_out[out_offset .. out_offset + 8 ceil(n_bits / 64))
 * s[j] = d_iq[offset + j], its float32 parts sr and si widened to double; M = order, b = log2 M.
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_soft_host and the numpy
 * model (tests/soft_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels' grid,
 * not on repetition.  The build's -ffp-contract=off holds: every floating-point operation below is one IEEE double operation,
 * rounded once, in the order the parentheses give.  The only transcendental is the pinned fosphor_amd_cossin_turns
 * (fosphor_amd_carrier.h); everything behind rule S2 is integer work, which any order of evaluation gives the same bits.
 *
 * S1. Points    the point that carries the value q, 0 <= q < M, lies at
 *               (C_q, S_q) = fosphor_amd_cossin_turns((double)((q + rot) & (M - 1)) / (double)M).  Its label is q ^ (q >> 1) with
 *               GRAY, else q.  Coded bit i of a symbol, 0 <= i < b, MSB first, is bit b - 1 - i of the label.  This is rule 5 of
 *               fosphor_amd_decide.h followed by rule 1 of fosphor_amd_decode.h: the sign of a soft value agrees with the bit
 *               that the hard chain decide -> decode reads, wherever the symbol lies off a decision boundary.
 * S2. Value     corr_q = (sr * C_q) + (si * S_q).  For a set of points, "the largest" is m after m = -infinity and, for q
 *               ascending, m = corr_q where corr_q > m: a NaN corr_q (an infinite part times a zero of a point) is never the
 *               largest.  L_i = (the largest corr_q over the points whose bit i is 0) - (the largest over those whose bit i
 *               is 1).  x = (L_i * (double)scale) + 0.5.  v = 0 if x is a NaN (infinity - infinity among them), 127 if x >= 127,
 *               -127 if x < -127, else (int)floor(x): the nearest integer, halves upwards, clamped to -127 .. 127.  A symbol with
 *               a NaN part gives v = 0 for all its bits and counts once in erasures; (0, 0) gives v = 0 and counts nowhere.  A
 *               positive v favours bit 0.  The soft value of coded bit q' of the job, 0 <= q' < n_coded, is v of bit q' % b of
 *               symbol q' / b; depuncturing (rule 2) hands it to its step and stream, and a coded bit that the pattern did not
 *               send has v = 0.  erasures counts the symbols below ceil(n_coded / b) with a NaN part, saturated the sent bits
 *               with |v| = 127, abs_sum adds |v| over the sent bits.  All three are integers: the order of summation is free.
 * S3. Cost      stream i of a branch with the expected bit e_i (rule 3) costs |v_i| when (v_i < 0) differs from e_i, else 0: a
 *               value of 0, sent or not, costs nothing.  Metrics are int32 and start at 0 for state 0 and at
 *               FOSPHOR_AMD_SOFT_INF = 2^25 for the others.  INF + 3 * 127 * MAX_STEPS < 2^26, so rule 4's key (metric, then
 *               state) is one unsigned 32-bit integer whose worst value lies below the all-ones key of the idle lanes.
 *               metric, best_metric: rule 4 over these costs.  With every |v| = 127 this is 127 times the hard decoder.
 *    Device     k_sft_bits: the grid runs over steps, 256 lanes own 256 steps of a job that they find in a prefix by a bounded
 *               binary search (fosphor_jobs.h).  The job's M points are formed once, on the host, by the pinned inline and
 *               travel in the device job.  A lane forms its step's up to three soft values from kept(t) on (one 8-byte load a
 *               symbol) and stores them as one aligned 32-bit word: three int8 values, stream i in byte i, byte 3 is 0.  The
 *               group's erasures, saturated count and sum of |v| are reduced across lanes in any order (integers) and go to
 *               scratch as one partial a work-group.
 *               k_sft_acs: one wave per job, lane = state; lanes >= S stay active with the metric INF, masked out of the ballot.
 *               Per block of 64 steps lane i loads the word of step t0 + i in one coalesced load; per step the word comes by a
 *               wave-uniform lane read, the two predecessors' metrics by two cross-lane reads, the cost is three selects and
 *               two adds a branch, and __ballot of the comparison is the step's 64-bit decision word, which lane t & 63 keeps;
 *               after the block the wave stores 64 words at once.  Neither LDS nor a barrier.  A wave reduction gives rule 4's
 *               values into scratch.
 *               k_sft_trace: as k_dcd_trace.  k_sft_rec: one wave per job adds the job's partials in ascending order (at most
 *               256), runs the CRC over the job's output and writes the whole record, once.  One launch per kernel per call,
 *               whatever the number of jobs; a launch with no work is not made (every T = 0: k_sft_rec alone); no atomics, no
 *               work-group waits for another, every loop carries its bound.
 * S4. Access    reads touch only d_iq[offset .. offset + n) of each job; writes only d_records[0 .. n_jobs) and each job's owned
 *               bytes.  Input ranges may overlap; owned output ranges must not.
 * S5. Refusals  -EINVAL, on the host, before anything is written, launched or counted: everything in rule 9 of
 *               fosphor_amd_decode.h with d_iq for d_sym and n_samples for n_bytes (there is no reserved field), and: d_iq not
 *               8-byte aligned; rot outside 0 .. M - 1; a scale that is zero, negative, infinite or a NaN; flags with other bits
 *               than TERMINATED and GRAY.  Every check is safe against offsets of 2^62.
 * A job with T = 0 writes nothing but its record (n_bits 0; the three sums 0; status OK, or SHORT with a CRC).
 *
 * 0; -EINVAL (rule S5); -EIO. */
int fosphor_amd_soft(struct fosphor *self, const void *d_iq, int64_t n_samples,
                     const struct fosphor_amd_soft_job *jobs, int n_jobs,
                     struct fosphor_amd_soft_record *d_records,
                     void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_soft_host(const float *iq, int64_t n_samples,
                          const struct fosphor_amd_soft_job *jobs, int n_jobs,
                          struct fosphor_amd_soft_record *records,
                          uint8_t *out, int64_t out_capacity);

/* HOST only: the job over the symbols that a decide job read.  With a unique word found (the decide job has
 * FOSPHOR_AMD_DECIDE_UW, the record's status is OK) the payload begins behind the word: offset = d->offset + uw_pos + uw_len and
 * rot = uw_rot; a record with NO_UW gives n = 0 and offset = d->offset, as in fosphor_amd_decode_from_decide; a decide job without
 * UW gives offset = d->offset, rot = 0 and uw_len is not used.  n = n_payload, or everything behind the word when n_payload == 0.
 * order = the record's; GRAY is copied from the decide job.  scale = (float)(16.0 * (double)r->n / r->a), r->n and r->a the
 * record's symbol count and sum a (its rule 2): the mean length of the symbols along their decided points is a / n, and a BPSK
 * symbol of that length gets |v| = 32 (L = 2 a / n); a job that comes out with n == 0 gets scale = 1.  steps, TERMINATED, the code, the puncture masks, the
 * CRC and out_offset are left 0 for the caller.  0; -EINVAL: a NULL pointer, a decide job with DIFF, offset < 0 or n < 0 in it,
 * an order that is not 2, 4 or 8, uw_len < 0, n_payload < 0, a word or a payload that runs past the decide job's n, a uw_rot
 * outside 0 .. M - 1, and, when the job comes out with n > 0, an a that is not finite and above 0 or a scale that float32 cannot
 * hold as a finite number above 0. */
int fosphor_amd_soft_from_decide(const struct fosphor_amd_decide_job *d, const struct fosphor_amd_decide_record *r,
                                 int uw_len, int n_payload, struct fosphor_amd_soft_job *job);

/* HOST only: a record as ratios, in double:
 *   mean_abs         abs_sum / n_coded: the mean reliability of the received coded bits, in soft units
 *   corrected_share  metric / abs_sum: the share of the received reliability that the decoded path overrules
 *   rate             n_steps / n_coded: the rate of the punctured code
 *   crc_ok           1 when status is FOSPHOR_AMD_SOFT_OK, else 0
 * A field whose value is not finite is 0.  0; -EINVAL: a NULL pointer. */
struct fosphor_amd_soft_values
{
	double mean_abs, corrected_share, rate, crc_ok;
};
int fosphor_amd_soft_derive(const struct fosphor_amd_soft_record *r, struct fosphor_amd_soft_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_SOFT_CALLS]     fosphor_amd_soft calls that reached the device
 *   stats[FOSPHOR_AMD_SOFT_K_BITS]    launches of k_sft_bits (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_SOFT_K_ACS]     launches of k_sft_acs (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_SOFT_K_TRACE]   launches of k_sft_trace (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_SOFT_K_REC]     launches of k_sft_rec
 *   stats[FOSPHOR_AMD_SOFT_JOBS_CRC]  jobs of those calls with crc_width > 0
 *   stats[FOSPHOR_AMD_SOFT_STEPS]     the sum of T over those jobs */
enum {
	FOSPHOR_AMD_SOFT_CALLS, FOSPHOR_AMD_SOFT_K_BITS, FOSPHOR_AMD_SOFT_K_ACS, FOSPHOR_AMD_SOFT_K_TRACE,
	FOSPHOR_AMD_SOFT_K_REC, FOSPHOR_AMD_SOFT_JOBS_CRC, FOSPHOR_AMD_SOFT_STEPS,
	FOSPHOR_AMD_SOFT_STATS
};
int fosphor_amd_soft_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_SOFT_STATS]);

#ifdef __cplusplus
}
#endif

#endif
