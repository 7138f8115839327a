/*
 * fosphor_amd_rs.h -- the outer code of a burst: the bits that fosphor_amd_decode or fosphor_amd_soft wrote taken as the bytes of
 * an interleaved, optionally scrambled Reed-Solomon frame over GF(2^8): descrambled, de-interleaved, every codeword corrected up
 * to t = n_roots / 2 byte errors, the data bytes in their transmitted order and one record (codewords, clean, failed, corrected
 * symbols and bits) per job
 *
 * The inner code of a burst almost never travels alone: CCSDS telemetry puts a pseudo-randomiser and an interleaved RS(255,223)
 * behind it, DVB-S an energy-dispersal sequence and RS(204,188).  This pass takes the step behind the chain extract -> resample ->
 * symbols -> carrier -> decide -> decode (or soft): it reads what those passes wrote, as it lies, and changes neither.  The code
 * is named by the parameters that users of Karn's libfec and of GNU Radio know: gf_poly, fcr, prim, n_roots.  A job's result
 * depends on its job alone, so up to 4096 frames go in one call, and jobs of different fields and codes may share it.
 *
 * Not this pass: erasure decoding; the CCSDS dual basis (rule 3 is the conventional basis); convolutional (Forney) interleavers
 * and bit interleavers in front of the Viterbi decoder; multiplicative (self-synchronising) scramblers; DVB's sync-byte inversion;
 * a CRC over the RS output; fields other than GF(2^8).
 *
 * Conventions, those of fosphor_amd_decode.h: the device entry point waits for pending fosphor_process work first
 * (fosphor_amd_finish), runs on the instance's stream and returns when its outputs are complete; it writes no state of the
 * instance; -EINVAL is decided on the host before anything is written, launched or counted; -EIO is a device error.
 */
#ifndef FOSPHOR_AMD_RS_H
#define FOSPHOR_AMD_RS_H

#include <stdint.h>

#include "fosphor.h"

#define FOSPHOR_AMD_RS_MAX_JOBS           4096
#define FOSPHOR_AMD_RS_MAX_ROOTS          32		/* parity bytes of a codeword: t <= 16 */
#define FOSPHOR_AMD_RS_MAX_DEPTH          16		/* codewords of a frame */
#define FOSPHOR_AMD_RS_MAX_CALL_CODEWORDS 65536		/* the sum of the jobs' depths: MAX_JOBS frames of MAX_DEPTH; the scratch of a
							 * call is 100 bytes a codeword */

#define FOSPHOR_AMD_RS_DESCRAMBLE_IN  1			/* flag bit: the sequence of rule 1 is taken off the input (CCSDS) */
#define FOSPHOR_AMD_RS_DESCRAMBLE_OUT 2			/* flag bit: ... off the output (DVB) */

#define FOSPHOR_AMD_RS_OK   0
#define FOSPHOR_AMD_RS_FAIL 1				/* at least one codeword of the frame could not be corrected */

#define FOSPHOR_AMD_RS_FAILED 255			/* errors[c] of a codeword that failed */

/* static LDS of a work-group of each kernel, bytes (tests/test_rs_cpu.py holds the compiled kernels to them) */
#define FOSPHOR_AMD_RS_LDS_SYN 0
#define FOSPHOR_AMD_RS_LDS_FIX 0
#define FOSPHOR_AMD_RS_LDS_OUT 0
#define FOSPHOR_AMD_RS_LDS_REC 0

#ifdef __cplusplus
extern "C" {
#endif

struct fosphor_amd_rs_job			/* 64 bytes */
{
	int64_t  offset;	/* index into d_in in BYTES of the frame's byte 0 */
	int64_t  out_offset;	/* index into d_out in BYTES of its first output, a multiple of 8 */
	int32_t  flags;		/* 0, FOSPHOR_AMD_RS_DESCRAMBLE_IN or FOSPHOR_AMD_RS_DESCRAMBLE_OUT */
	uint16_t gf_poly;	/* the field polynomial of GF(2^8), 0x100 .. 0x1ff, primitive (rule 3) */
	uint8_t  fcr;		/* first consecutive root, 0 .. 254 */
	uint8_t  prim;		/* root spacing, 1 .. 254, coprime with 255 */
	uint8_t  n_roots;	/* parity bytes of a codeword, 2 .. 32; t = n_roots / 2 rounded down */
	uint8_t  n_code;	/* bytes of a codeword, n_roots + 1 .. 255; a shortened code's missing leading bytes are zero */
	uint8_t  depth;		/* I: codewords of the frame, 1 .. 16 (rule 2) */
	uint8_t  scr_width;	/* w: 0 (no scrambler) or 2 .. 32 (rule 1) */
	uint32_t scr_taps;	/* below 2^w */
	uint32_t scr_init;	/* below 2^w */
	uint32_t reserved[7];	/* must be 0 */
};

struct fosphor_amd_rs_record			/* 64 bytes, 8-byte aligned */
{
	int32_t  n_codewords;		/* I */
	int32_t  n_data;		/* data bytes written: I (n_code - n_roots) */
	int32_t  status;		/* FOSPHOR_AMD_RS_OK, or _FAIL when any codeword failed */
	int32_t  n_failed;		/* codewords that failed (rule 4) */
	int32_t  n_clean;		/* codewords whose syndromes are all 0 */
	int32_t  corrected_symbols;	/* bytes changed, over the codewords that did not fail */
	int32_t  corrected_bits;	/* the popcount of their error values: the bit errors the inner decoder left */
	int32_t  max_errors;		/* the most bytes changed in one codeword that did not fail */
	uint32_t failed_mask;		/* bit c set when codeword c failed */
	uint8_t  errors[16];		/* per codeword the bytes changed, FOSPHOR_AMD_RS_FAILED where it failed, 0 for c >= I */
	uint16_t n_code;		/* the job's */
	uint16_t n_roots;		/* the job's */
	uint32_t reserved[2];		/* 0 */
};

/* Corrected data bytes of n_jobs frames of d_in.  jobs: HOST memory.  DEVICE memory:
 *   d_in       n_bytes bytes, no alignment: exactly what fosphor_amd_decode or fosphor_amd_soft wrote to their d_out, decoded bits
 *              packed MSB first.  A job reads d_in[offset .. offset + depth n_code)
 *   d_records  n_jobs records in job order, 8-byte aligned
 *   d_out      out_capacity bytes, 8-byte aligned.  Job j owns d_out[out_offset .. out_offset + 8 ceil(n_data / 8))
 *
 * Every byte of every record and every written output is BIT-IDENTICAL between the device, fosphor_amd_rs_host and the numpy model
 * (tests/rs_model.py), and depends on its job alone: not on the other jobs, not on their order, not on the kernels' grid, not on
 * repetition.  All of it is integer work; rule 4 states the decision as mathematics, so any algorithm gives the same bits (the
 * device and the host statement run Berlekamp-Massey and Forney's formula, the model solves the Newton identities by elimination).
 *
 * 1. Scrambler  w = scr_width.  reg = scr_init; per bit: out = (reg >> (w - 1)) & 1; fb = parity(reg & scr_taps);
 *               reg = ((reg << 1) | fb) & (2^w - 1).  Eight bits make a byte, MSB first.  The sequence restarts at byte 0 of each
 *               job.  With DESCRAMBLE_IN byte p of the sequence is XORed onto input byte p before decoding, over all depth n_code
 *               bytes (CCSDS: randomised after RS encoding).  With DESCRAMBLE_OUT it is XORed onto output byte p after decoding
 *               (DVB: randomised before RS encoding).  w = 8, taps 0x95, init 0xff gives ff 48 0e c0 9a 0d 70 bc, the CCSDS
 *               pseudo-random sequence.  w > 0 without a flag changes nothing.
 * 2. Interleave codeword c, 0 <= c < I, is the bytes p = i I + c of the frame, i = 0 .. n_code - 1, i = 0 first.  Its first
 *               n_code - n_roots bytes are data, its last n_roots parity.  De-interleaving is index arithmetic only.
 * 3. Field      alpha = 0x02 in GF(2^8) modulo gf_poly.  The generator is g(x) = the product over j = 0 .. n_roots - 1 of
 *               (x - alpha^(prim (fcr + j))).  Byte i of a codeword is the coefficient of x^(n_code - 1 - i).  The syndromes are
 *               S_j = r(alpha^(prim (fcr + j))), j = 0 .. n_roots - 1.  Conventional basis only.
 * 4. Decision   t = n_roots / 2, rounded down.  Let L be the linear complexity of S_0 .. S_(n_roots - 1): the length of the
 *               shortest linear recurrence S_j = Lambda_1 S_(j - 1) + ... + Lambda_L S_(j - L), L <= j < n_roots.  All S_j = 0:
 *               the codeword is clean.  L > t: FAIL.  Otherwise Lambda(x) = 1 + Lambda_1 x + ... + Lambda_L x^L is unique.
 *               Position i, 0 <= i < n_code, has the locator X_i = alpha^(prim (n_code - 1 - i)); it is an error position when
 *               Lambda(1 / X_i) = 0.  A root at a shortened position (an exponent of n_code and more) does not count.  If the
 *               number of error positions is not L: FAIL.  Otherwise the error values Y are the solution of
 *               S_j = the sum over the positions of Y X^(fcr + j) (Forney's formula gives it), and byte i becomes r_i ^ Y_i.  A
 *               codeword that FAILs is passed on as received, after DESCRAMBLE_IN.  More than t errors may also lead to
 *               another codeword: that is what the rule says and no defect.
 * 5. Output     output byte p, 0 <= p < n_data = I (n_code - n_roots), is corrected frame byte p: the parity is dropped, the
 *               data keeps its transmitted order.  It goes to d_out[out_offset + p].  The job owns 8 ceil(n_data / 8) bytes; the
 *               bytes behind the data are written 0.  On the device every store to d_out is one aligned 64-bit store.
 * 6. Record     written once.  errors[c] is the number of error positions of codeword c (0 for a clean one), FAILED where it
 *               failed, 0 for c >= I.  corrected_symbols, corrected_bits and max_errors run over the codewords that did not fail.
 *    Device     GF(2^8) products are an eight-step shift-and-XOR with no table, on the device and in the host statement alike
 *               (profiles/r25_rs.md says why).  k_rs_syn: one wave per codeword, found through a prefix of the jobs' codewords
 *               (fosphor_jobs.h).  A lane loads four bytes of the codeword at stride I and takes the scrambler off them; the two
 *               halves of the wave run Horner's rule over the two halves of the codeword, lane = syndrome, and one product with
 *               a power of the root joins them.  Syndromes and a state word (clean or not) go to scratch.  The host reads the
 *               state words: k_rs_fix is launched only if a codeword is not clean.  k_rs_fix: one wave per codeword, clean ones
 *               leave at once.  Berlekamp-Massey with lane = coefficient, the discrepancy by a cross-lane XOR reduction, n_roots
 *               rounds; the root search over the n_code positions, four a lane, counted by __ballot; Forney's formula in the
 *               lanes that found a root.  Up to 16 (position, value) pairs and the count, or FAILED, go to scratch.  k_rs_out:
 *               the grid runs over output words, 256 lanes own 256 words of a job that they find in a prefix; a lane assembles
 *               eight bytes -- received, descrambled as flagged, a correction looked up in its codeword's short list -- and
 *               stores one 64-bit word.  k_rs_rec: one wave per job sums its codewords and writes the record.  At most four
 *               launches per call, whatever the number of jobs; a launch with no work is not made; no atomics, no work-group
 *               waits for another, no LDS, every loop carries its bound: Berlekamp-Massey n_roots <= 32 rounds and the root search
 *               n_code <= 255 positions, whatever the bytes say.
 * 7. Refusals   -EINVAL, on the host, before anything is written, launched or counted: a NULL self, d_in, jobs, d_records or
 *               d_out; n_jobs outside 1 .. MAX_JOBS; n_bytes or out_capacity below 0; a job with offset or out_offset below 0,
 *               offset + depth n_code > n_bytes, its owned bytes outside out_capacity, an out_offset that is no multiple of 8;
 *               gf_poly outside 0x100 .. 0x1ff or not primitive (alpha walked through 255 steps must come back to 1 at the last
 *               and not before); fcr > 254; prim outside 1 .. 254 or not coprime with 255; n_roots outside 2 .. 32; n_code
 *               outside n_roots + 1 .. 255; depth outside 1 .. 16; scr_width 1 or above 32; scr_taps or scr_init >= 2^w (with
 *               w = 0: not 0); flags with other bits than the two, both at once, or one with w = 0; reserved that is not 0;
 *               more than MAX_CALL_CODEWORDS codewords in the call (MAX_JOBS frames of MAX_DEPTH are exactly that many); owned
 *               outputs over another job's; d_records or d_out not 8-byte aligned (d_in needs no alignment).  Every check is safe
 *               against offsets of 2^62.
 * Input ranges may overlap; owned output ranges must not.  Reads touch only each job's frame; writes only d_records[0 .. n_jobs)
 * and each job's owned bytes.
 *
 * 0; -EINVAL (rule 7); -EIO. */
int fosphor_amd_rs(struct fosphor *self, const void *d_in, int64_t n_bytes,
                   const struct fosphor_amd_rs_job *jobs, int n_jobs,
                   struct fosphor_amd_rs_record *d_records,
                   void *d_out, int64_t out_capacity);

/* HOST only, no GPU: the contract in plain C.  Same arguments with host pointers.  0; -EINVAL: what the device entry point
 * refuses, but for self. */
int fosphor_amd_rs_host(const uint8_t *in, int64_t n_bytes,
                        const struct fosphor_amd_rs_job *jobs, int n_jobs,
                        struct fosphor_amd_rs_record *records,
                        uint8_t *out, int64_t out_capacity);

/* HOST only: the way back, for tests, benchmarks and loopback checks.  The same jobs read the other way round: job j takes its
 * n_data data bytes, in the order of rule 5, from data[out_offset .. out_offset + n_data), scrambles them with DESCRAMBLE_OUT,
 * appends every codeword's parity (rules 2 and 3), scrambles the frame with DESCRAMBLE_IN, and writes the depth n_code bytes to
 * frames[offset ..).  fosphor_amd_rs over `frames` with the same jobs gives `data` back.  0; -EINVAL: a NULL pointer, what rule 7
 * refuses of a job's fields and of n_jobs, a frame outside n_bytes or data outside data_capacity, frames that overlap. */
int fosphor_amd_rs_encode_host(const uint8_t *data, int64_t data_capacity,
                               const struct fosphor_amd_rs_job *jobs, int n_jobs,
                               uint8_t *frames, int64_t n_bytes);

/* HOST only: the job over what a decode or a soft job wrote.  out_offset: that job's; n_bits: its record's; the frame begins
 * skip_bytes behind the job's first output byte (a sync marker that was decoded with it).  *job is zeroed, then offset =
 * out_offset + skip_bytes, n_code and depth are set; the code, the scrambler, flags and out_offset are left 0 for the caller.
 * 0; -EINVAL: a NULL job, out_offset, skip_bytes or n_bits below 0, n_code outside 3 .. 255, depth outside 1 .. 16, a frame that
 * n_bits does not cover: 8 (skip_bytes + depth n_code) > n_bits. */
int fosphor_amd_rs_from_decode(int64_t out_offset, int32_t n_bits, int64_t skip_bytes, int n_code, int depth,
                               struct fosphor_amd_rs_job *job);

/* HOST only: a record as ratios, in double:
 *   byte_error_rate  corrected_symbols / (n_code (n_codewords - n_failed)): the byte errors before correction, over the codewords
 *                    that did not fail
 *   failed_share     n_failed / n_codewords
 *   ok               1 when status is FOSPHOR_AMD_RS_OK, else 0
 * A field whose value is not finite is 0.  0; -EINVAL: a NULL pointer. */
struct fosphor_amd_rs_values
{
	double byte_error_rate, failed_share, ok;
};
int fosphor_amd_rs_derive(const struct fosphor_amd_rs_record *r, struct fosphor_amd_rs_values *v);

/* Host counters that only grow; nothing reads them but this call.  stats may be NULL.
 *   stats[FOSPHOR_AMD_RS_CALLS]      fosphor_amd_rs calls that reached the device
 *   stats[FOSPHOR_AMD_RS_K_SYN]      launches of k_rs_syn
 *   stats[FOSPHOR_AMD_RS_K_FIX]      launches of k_rs_fix (none in a call whose codewords are all clean)
 *   stats[FOSPHOR_AMD_RS_K_OUT]      launches of k_rs_out
 *   stats[FOSPHOR_AMD_RS_K_REC]      launches of k_rs_rec
 *   stats[FOSPHOR_AMD_RS_CODEWORDS]  codewords of those calls
 *   stats[FOSPHOR_AMD_RS_CLEAN]      ... that were clean
 *   stats[FOSPHOR_AMD_RS_FAILED_CW]  ... that failed */
enum {
	FOSPHOR_AMD_RS_CALLS, FOSPHOR_AMD_RS_K_SYN, FOSPHOR_AMD_RS_K_FIX, FOSPHOR_AMD_RS_K_OUT, FOSPHOR_AMD_RS_K_REC,
	FOSPHOR_AMD_RS_CODEWORDS, FOSPHOR_AMD_RS_CLEAN, FOSPHOR_AMD_RS_FAILED_CW,
	FOSPHOR_AMD_RS_STATS
};
int fosphor_amd_rs_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_RS_STATS]);

#ifdef __cplusplus
}
#endif

#endif
