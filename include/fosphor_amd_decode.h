/*
 * fosphor_amd_decode.h -- the bits of a burst: the hard decisions of fosphor_amd_decide taken as the coded bits of a punctured
 * convolutional code, depunctured, decoded by a Viterbi decoder over the whole frame and checked by a CRC; the decoded bits and
 * one record (steps, corrected channel errors, end state, both CRCs) per job
 *
 * fosphor_amd_decide leaves one byte per symbol.  This pass takes the step behind the chain extract -> resample -> symbols ->
 * carrier -> decide: the symbols' bits in transmission order (rule 1), the puncture pattern put back as erasures (rule 2), the
 * maximum-likelihood path through the trellis of a rate 1/2 or 1/3 code of constraint length 3 .. 7 (rules 3 to 5), its input bits
 * packed MSB first (rule 6) and a CRC over them (rule 7).  A job's result depends on its job alone, so up to 4096 bursts go in one
 * call.  K = 7 has 64 states and a wave has 64 lanes: add-compare-select is one lane per state.
 *
 * Not this pass: soft decisions (fosphor_amd_soft.h has them), tail-biting, truncated or block-parallel traceback, several
 * short-K jobs in one wave, interleavers and scramblers (the block interleaver, the additive scrambler and the Reed-Solomon code
 * that usually stand behind this decoder are fosphor_amd_rs.h), reflected CRCs.
 *
 * Conventions, those of fosphor_amd_decide.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_DECODE_H
#define FOSPHOR_AMD_DECODE_H

#include <stdint.h>

#include "fosphor.h"
#include "fosphor_amd_decide.h"			/* the decide job and record */

#define FOSPHOR_AMD_DECODE_MAX_JOBS       4096
#define FOSPHOR_AMD_DECODE_MAX_STEPS      65536		/* trellis steps of one job */
#define FOSPHOR_AMD_DECODE_MAX_CALL_STEPS 4194304	/* 2^22: the sum of the jobs' steps; the survivor decisions are 8 bytes a step,
							 * the codes one: a call needs at most 32 MiB + 4 MiB of scratch */
#define FOSPHOR_AMD_DECODE_BLOCK          64		/* steps of a block of k_dcd_acs and k_dcd_trace; tests plant seams here */
#define FOSPHOR_AMD_DECODE_INF            16777216	/* 2^24: the metric of a state that cannot be reached yet */

#define FOSPHOR_AMD_DECODE_TERMINATED 1			/* flag bit: the encoder was driven back to state 0 by k - 1 tail bits */

#define FOSPHOR_AMD_DECODE_OK       0
#define FOSPHOR_AMD_DECODE_CRC_FAIL 1
#define FOSPHOR_AMD_DECODE_SHORT    2			/* fewer decoded bits than the CRC is wide */

/* static LDS of a work-group of each kernel, bytes (tests/test_decode_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_DECODE_LDS_BITS  0
#define FOSPHOR_AMD_DECODE_LDS_ACS   0
#define FOSPHOR_AMD_DECODE_LDS_TRACE 0
#define FOSPHOR_AMD_DECODE_LDS_REC   0

#ifdef __cplusplus
extern "C" {
#endif

struct fosphor_amd_decode_job			/* 64 bytes */
{
	int64_t  offset;	/* index into d_sym in BYTES of the job's symbol 0 */
	int64_t  out_offset;	/* index into d_out in BYTES of its first output, a multiple of 8 */
	int32_t  n;		/* symbols, >= 0 */
	int32_t  order;		/* M: 2, 4 or 8; b = log2 M coded bits a symbol */
	int32_t  steps;		/* trellis steps T; 0 = as many as the symbols hold (rule 2) */
	int32_t  flags;		/* 0 or FOSPHOR_AMD_DECODE_TERMINATED */
	uint8_t  k;		/* constraint length, 3 .. 7 */
	uint8_t  n_poly;	/* streams of the code: 2 or 3 */
	uint8_t  period;	/* steps of the puncture pattern, 1 .. 16 */
	uint8_t  crc_width;	/* w: 0 (none), 8, 16, 24 or 32 */
	uint16_t polys[3];	/* the generators, below 2^k (rule 3); polys[2] = 0 with two streams */
	uint16_t punct[3];	/* the puncture masks, below 2^period (rule 2); all bits set = nothing punctured */
	uint32_t crc_poly;	/* rule 7, below 2^w */
	uint32_t crc_init;
	uint32_t crc_xorout;
	uint32_t reserved;	/* must be 0 */
};

struct fosphor_amd_decode_record		/* 64 bytes, 8-byte aligned */
{
	int32_t  n_steps;	/* T of rule 2 */
	int32_t  n_bits;	/* decoded bits written (rule 5) */
	int32_t  n_coded;	/* coded bits consumed: kept(T) */
	int32_t  status;	/* FOSPHOR_AMD_DECODE_OK, _CRC_FAIL or _SHORT */
	int32_t  end_state;	/* rule 4: where the traceback began */
	int32_t  metric;	/* rule 4: the coded bits that differ from the decoded path's: the channel errors corrected */
	int32_t  best_state;	/* rule 4 */
	int32_t  best_metric;
	uint32_t crc_calc;	/* rule 7 */
	uint32_t crc_recv;
	int32_t  k;		/* the job's */
	int32_t  flags;		/* the job's */
	int32_t  reserved[4];	/* 0 */
};

/* Decoded bits of n_jobs ranges of d_sym.  jobs: HOST memory.  DEVICE memory:
 *   d_sym      n_bytes bytes, one symbol each, no alignment: exactly what fosphor_amd_decide writes
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity bytes, 8-byte aligned.  Job j owns d_out[out_offset .. out_offset + 8 ceil(n_bits / 64))
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_decode_host and the numpy
 * model (tests/decode_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels'
 * grid, not on repetition.  All of it is integer work: any order of evaluation gives the same bits.
 *
 * 1. Coded bits b = log2 M.  Coded bit q, 0 <= q < n b, is (d_sym[offset + q / b] >> (b - 1 - q % b)) & 1: a symbol's bits MSB
 *               first.  Bits of a byte above b are ignored.
 * 2. Depuncture bit p (LSB = 0) of punct[i] says that stream i's bit of a step t with t mod period == p was sent.  Kept bits are
 *               consumed in order of ascending step, and within a step in order of ascending stream.  With W the popcount of all
 *               masks, kept(T) = (T / period) W + the sum over i of popcount(punct[i] & ((1 << (T % period)) - 1)).  T is the
 *               job's steps; with steps == 0 it is the largest T with kept(T) <= n b.  n_coded = kept(T).  A bit that was not
 *               sent is an erasure and costs nothing.
 * 3. Trellis    S = 2^(k - 1) states.  The register at step t is R = (u_t << (k - 1)) | s_t, stream i's bit is the parity of
 *               polys[i] & R, and the next state is s_{t + 1} = R >> 1.  State s' has the input u = s' >> (k - 2) and the
 *               predecessors p_x = ((s' << 1) | x) & (S - 1), x = 0, 1.  Metrics are int32.  At t = 0 state 0 has the metric 0 and
 *               every other state INF.  A branch costs the number of its sent bits that differ from the received ones.
 *               c_x = metric[p_x] + branch_x; the survivor is x = 1 if c_1 < c_0, else x = 0: ties go to x = 0.
 * 4. End        best_state is the smallest state of least metric after T steps and best_metric its metric.  end_state is 0
 *               with TERMINATED, else best_state; metric is its metric.  T = 0 gives end_state = best_state = 0 and both
 *               metrics 0.
 * 5. Traceback  from end_state over all T steps: only the whole path is the maximum-likelihood one, so there is no truncated
 *               window.  n_bits = T without TERMINATED; with it n_bits = max(T - (k - 1), 0): the tail is dropped.
 * 6. Output     decoded bit t (u_t) goes to byte out_offset + t / 8, bit 7 - t % 8.  The job owns 8 ceil(n_bits / 64) bytes; the
 *               bits behind n_bits are written 0.  On the device every store to d_out is one aligned 64-bit store.
 * 7. CRC        w = crc_width, mask = 2^w - 1.  reg = crc_init; for each of the first n_bits - w decoded bits:
 *               top = ((reg >> (w - 1)) & 1) ^ bit; reg = (reg << 1) & mask; if (top) reg ^= crc_poly.  crc_calc = reg ^ crc_xorout.
 *               crc_recv is the last w decoded bits, MSB first.  status is OK if they are equal, else CRC_FAIL.  n_bits < w:
 *               status SHORT and both fields 0.  w = 0: both fields 0 and status OK.  Reflected CRCs are not this pass.
 *    Device     k_dcd_bits: the grid runs over steps, 256 lanes own 256 steps of a job that they find in a prefix by a bounded
 *               binary search (fosphor_jobs.h).  A lane forms its step's code byte -- the received bits in bits 0 .. 2, the
 *               erased flags in bits 4 .. 6 -- from kept(t) on, and four steps leave as one 32-bit word into scratch.
 *               k_dcd_acs: one wave per job, lane = state; lanes >= S stay active with the metric INF, masked out of the
 *               ballot (the cross-lane reads need all 64 lanes).  Each lane forms its two expected-output codes once.  Per block
 *               of 64 steps lane i loads the code of step t0 + i in one coalesced load; per step the code comes by a
 *               wave-uniform lane read, the two predecessors' metrics by two cross-lane reads, the branch cost is a popcount,
 *               and __ballot of the comparison is the step's 64-bit decision word, which lane t & 63 keeps; after the block the
 *               wave stores 64 words at once.  Neither LDS nor a barrier.  A wave reduction gives rule 4's values into scratch.
 *               k_dcd_trace: one wave per job, blocks in descending order: lane i loads the decision word of step t0 + i, the
 *               state walks the 64 steps by wave-uniform lane reads, and the block's 64 decoded bits become output word t0 / 64,
 *               byte-ordered for rule 6, the tail masked.  k_dcd_rec: one wave per job runs the CRC over the job's output, bit
 *               by bit, and writes the whole record, once.  At most four launches per call, whatever the number of jobs; a launch
 *               with no work is not made (every T = 0: k_dcd_rec alone); no atomics, no work-group waits for another, every
 *               loop carries its bound.
 * 8. Access     reads touch only d_sym[offset .. offset + n) of each job; writes only d_records[0 .. n_jobs) and each job's owned
 *               bytes.  Input ranges may overlap; owned output ranges must not.
 * 9. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_sym, jobs, d_records or
 *               d_out; n_jobs outside 1 .. MAX_JOBS; n_bytes or out_capacity below 0; a job with offset, out_offset or n below
 *               0, offset + n > n_bytes, its owned bytes outside out_capacity, an out_offset that is no multiple of 8; an order
 *               that is not 2, 4 or 8, k outside 3 .. 7, n_poly that is not 2 or 3, period outside 1 .. 16, crc_width that is
 *               not 0, 8, 16, 24 or 32; polys[i] of a stream that is 0 or >= 2^k; punct[i] >= 2^period; W = 0; with n_poly == 2 a
 *               polys[2] or punct[2] that is not 0; steps < 0 or kept(steps) > n b; T > MAX_STEPS; the sum of T over the call
 *               > MAX_CALL_STEPS; with w = 0 a crc_poly, crc_init or crc_xorout that is not 0, with w > 0 one that is >= 2^w;
 *               flags with other bits than TERMINATED; reserved that is not 0; owned outputs over another job's; d_records or
 *               d_out not 8-byte aligned (d_sym needs no alignment).  Every check is safe against offsets of 2^62.
 * A job with T = 0 writes nothing but its record (n_bits 0; status OK, or SHORT with a CRC).
 *
 * 0; -EINVAL (rule 9); -EIO. */
int fosphor_amd_decode(struct fosphor *self, const void *d_sym, int64_t n_bytes,
                       const struct fosphor_amd_decode_job *jobs, int n_jobs,
                       struct fosphor_amd_decode_record *d_records,
                       void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_decode_host(const uint8_t *sym, int64_t n_bytes,
                            const struct fosphor_amd_decode_job *jobs, int n_jobs,
                            struct fosphor_amd_decode_record *records,
                            uint8_t *out, int64_t out_capacity);

/* HOST only: rule 2's T for steps = 0: the largest T with kept(T) <= n b.  -EINVAL: n < 0, an order, n_poly or period outside
 * its set, a NULL punct, a mask >= 2^period (or punct[2] != 0 with two streams), W = 0, a T that an int cannot hold. */
int fosphor_amd_decode_steps(int n, int order, int n_poly, int period, const uint16_t punct[3]);

/* HOST only: the job over what a decide job wrote into fosphor_amd_decide's d_out.  With a unique word found (the decide job has
 * FOSPHOR_AMD_DECIDE_UW, the record's status is OK) the payload begins behind the word: offset = d->out_offset + uw_pos + uw_len;
 * a record with NO_UW gives n = 0; a decide job without UW gives offset = d->out_offset and uw_len is not used.  n = n_payload, or
 * everything behind the word when n_payload == 0.  order = the record's.  steps, flags, the code, the puncture masks, the CRC and
 * out_offset are left 0 for the caller.  0; -EINVAL: a NULL pointer, out_offset < 0 or n < 0 in the decide job, an order that is
 * not 2, 4 or 8, uw_len < 0, n_payload < 0, a word or a payload that runs past the decide job's n. */
int fosphor_amd_decode_from_decide(const struct fosphor_amd_decide_job *d, const struct fosphor_amd_decide_record *r,
                                   int uw_len, int n_payload, struct fosphor_amd_decode_job *job);

/* HOST only: a record as ratios, in double:
 *   channel_ber  metric / n_coded: the share of the received coded bits that the decoded path corrects
 *   rate         n_steps / n_coded: the rate of the punctured code
 *   crc_ok       1 when status is FOSPHOR_AMD_DECODE_OK, else 0
 * A field whose value is not finite is 0.  0; -EINVAL: a NULL pointer. */
struct fosphor_amd_decode_values
{
	double channel_ber, rate, crc_ok;
};
int fosphor_amd_decode_derive(const struct fosphor_amd_decode_record *r, struct fosphor_amd_decode_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_DECODE_CALLS]     fosphor_amd_decode calls that reached the device
 *   stats[FOSPHOR_AMD_DECODE_K_BITS]    launches of k_dcd_bits (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_DECODE_K_ACS]     launches of k_dcd_acs (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_DECODE_K_TRACE]   launches of k_dcd_trace (none when every job has T = 0)
 *   stats[FOSPHOR_AMD_DECODE_K_REC]     launches of k_dcd_rec
 *   stats[FOSPHOR_AMD_DECODE_JOBS_CRC]  jobs of those calls with crc_width > 0
 *   stats[FOSPHOR_AMD_DECODE_STEPS]     the sum of T over those jobs */
enum {
	FOSPHOR_AMD_DECODE_CALLS, FOSPHOR_AMD_DECODE_K_BITS, FOSPHOR_AMD_DECODE_K_ACS, FOSPHOR_AMD_DECODE_K_TRACE,
	FOSPHOR_AMD_DECODE_K_REC, FOSPHOR_AMD_DECODE_JOBS_CRC, FOSPHOR_AMD_DECODE_STEPS,
	FOSPHOR_AMD_DECODE_STATS
};
int fosphor_amd_decode_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_DECODE_STATS]);

#ifdef __cplusplus
}
#endif

#endif
