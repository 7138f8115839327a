/*
 * fosphor_amd_wire.h -- compact wire formats for the hit counts of a sharded display frame
 *
 * The exchange of include/fosphor_amd.h (fosphor_amd_exchange, fosphor_amd_exchange_sliced) sends the partial hit counts of a
 * slot as they lie in memory: uint32[n_bins][N], 4 B per cell (128 MiB per rank and frame at N = 65536 with 512 bins).  The data
 * needs neither the width nor the density: one sample increments one cell, so a cell of a frame of total_batch spectra is at most
 * total_batch, on every rank and in the sum over the ranks; and at long FFT lengths most 64-cell rows of a frame hold no hit at all.
 * The two formats below carry the same counts in fewer bytes.  Both are exact: after fosphor_amd_wire_unpack the slot holds the
 * uint32 sums, bit for bit what the uint32 exchange leaves, and fosphor_amd_merge / fosphor_amd_merge_sliced /
 * fosphor_amd_gather_state work on it unchanged.  Both are opt-in: the uint32 exchange stays the default.
 *
 * Notation: hc = the slot's counts flattened, cell c = hc[c], n_hc = n_bins * N cells (fosphor_amd_get_partials).
 *
 * FOSPHOR_AMD_WIRE_PACKED16  (2 B per cell)
 *   word w of n_hc / 2 words =  hc[2 w] | hc[2 w + 1] << 16.
 *   The words are summed over the ranks as uint32 (RCCL has no 16-bit integer type).  Both halves are at most
 *   total_batch <= 65535 on every rank and in the sum, so no carry crosses from the low half into the high half and the sum of the
 *   words is the packing of the sums.  total_batch > 65535 is refused.
 *
 * FOSPHOR_AMD_WIRE_SPARSE16  (one bit per row + 128 B per live row)
 *   A row is 64 consecutive cells -- one bin, one 64-column slab; packed: 32 words, 128 B.  rows = n_hc / 64.
 *   (a) mask:   every rank writes one presence bit per row of ITS counts (bit r & 31 of word r >> 5: some cell of row r is not
 *               zero) into part `rank` of uint32[world][rows / 32]; the parts are all-gathered.
 *   (b) pack:   every rank ORs the `world` parts into the union mask, numbers the union's live rows in ascending row order and
 *               packs exactly those rows, in that order, into live_rows * 32 words (a row that is empty on this rank but live on
 *               another is packed as zeros).  The union is the same on every rank, so the layout is too.
 *   (c) the live_rows * 32 words are all-reduced as uint32 sums.
 *   When more than half of the rows are live in the union, the frame goes out as PACKED16 instead (a full mask plus 128 B per row
 *   would be more than that).  Every rank sees the same union, so every rank takes the same decision without further agreement.
 *   THE HOST WAIT: the host needs live_rows to size the all-reduce.  The pack step leaves it in pinned host memory and
 *   fosphor_amd_wire_pack / fosphor_amd_exchange_compact wait on the count stream for it: one host wait per frame for one integer.
 *   (The PACKED16 form queues everything and waits for nothing.)  An instance has one set of wire buffers for all its slots.
 *
 * The two float column arrays (live sum, max) travel as in the uint32 exchange, in the same ncclGroup as the count words.
 */
#ifndef FOSPHOR_AMD_WIRE_H
#define FOSPHOR_AMD_WIRE_H

#include <stdint.h>

#include "fosphor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOSPHOR_AMD_WIRE_PACKED16 1
#define FOSPHOR_AMD_WIRE_SPARSE16 2

#define FOSPHOR_AMD_WIRE_ROW_CELLS 64		/* cells of a row */
#define FOSPHOR_AMD_WIRE_ROW_WORDS 32		/* packed words of a row */
#define FOSPHOR_AMD_WIRE_MAX_BATCH 65535	/* largest total_batch either format carries */

/* The buffers between the stages, and what the last pack decided.  The pointers stay valid until fosphor_release (the mask buffer
 * until a mask stage with a larger world). */
struct fosphor_amd_wire
{
	uint32_t *d_masks;	/* [world][mask_words]: part r is rank r's presence bits (NULL before the first mask stage) */
	int mask_words;		/* rows / 32: words of one rank's part */
	int world;		/* parts the mask buffer was last laid out for (0: none yet) */
	uint32_t *d_words;	/* the wire words (NULL before the first pack) */
	int n_words;		/* words to all-reduce: n_hc / 2 (PACKED16), live_rows * 32 (SPARSE16); 0 when nothing is packed */
	int form;		/* the form the last pack took (FOSPHOR_AMD_WIRE_*; PACKED16 after a sparse pack = it fell back); 0: nothing is packed */
	int live_rows;		/* rows live in the union mask of the last sparse pack, fallen back or not (-1: the pack was PACKED16 by request) */
	int rows;		/* rows in total */
};

/* Every call below works on the partial arrays of the current slot (fosphor_amd_set_partial_slot) and queues its kernels on the
 * count / merge stream (fosphor_amd_stream2), behind the count kernel of fosphor_amd_accumulate_device and in front of the merge.
 * Whoever plays the collective between the stages operates on the buffers of struct fosphor_amd_wire, ordered against that stream.
 *
 * Argument errors return -EINVAL before anything is queued or changed: total_batch > 65535 or < 16, an unknown form, world < 1,
 * rank outside [0, world), a state whose rows do not fill whole mask words (n_bins * N no multiple of 2048); and the stage errors
 * named with each call.  -EIO: device error. */

/* Stage (a) of SPARSE16: the presence bits of the slot's rows, into part `rank` of the mask buffer. */
int fosphor_amd_wire_mask(struct fosphor *self, int total_batch, int world, int rank);

/* Pack the slot into the wire words in the form asked for, and fill *out.  SPARSE16 reads the `world` parts of the mask buffer
 * (all-gathered since the mask stage), waits for live_rows (the host wait above) and falls back to PACKED16 when
 * live_rows > rows / 2.  -EINVAL also for a SPARSE16 pack that no mask stage with the same world and on the same slot precedes
 * (every sparse pack needs a mask stage of its own; the instance has one set of wire buffers for all its slots, so the slot must
 * not change between the stages of a frame). */
int fosphor_amd_wire_pack(struct fosphor *self, int total_batch, int form, int world, struct fosphor_amd_wire *out);

/* The inverse of the last pack, from the (all-reduced) wire words into the slot as uint32 counts.  SPARSE16 writes the union's
 * live rows only: every other row is zero on every rank already.  -EINVAL when nothing is packed or the current slot is not the one that was packed; a pack is
 * unpacked once. */
int fosphor_amd_wire_unpack(struct fosphor *self);

/* The buffers and the state of the last pack without doing anything (n_words, form = 0 when nothing is packed). */
int fosphor_amd_wire_get(struct fosphor *self, struct fosphor_amd_wire *out);

/* The native path: the same stages with the library's RCCL communicator (fosphor_amd_comm_init) playing the collective, between
 * fosphor_amd_accumulate_device and fosphor_amd_merge / fosphor_amd_merge_sliced:
 *   SPARSE16: mask, ncclAllGather of the parts, pack (host wait), ncclGroup of three all-reduces, unpack
 *   PACKED16: pack, ncclGroup of three all-reduces, unpack (nothing waits on the host)
 * The ncclGroup holds the count words (uint32 sum) and the two float column arrays (sum, max), as fosphor_amd_exchange's does.
 * While profiling is on, the events of fosphor_amd_exchange_time wrap the whole of it, kernels and host wait included. */
int fosphor_amd_exchange_compact(struct fosphor *self, void *comm, int total_batch, int form, int world, int rank);

/* Host counters, since the instance was made; nothing on the submit path reads them.
 *   FRAMES_PACKED16   packs that were asked for PACKED16
 *   FRAMES_SPARSE16   packs that were asked for SPARSE16 and went out sparse
 *   FRAMES_FELL_BACK  packs that were asked for SPARSE16 and went out as PACKED16
 *   LAST_LIVE_ROWS    live rows of the last sparse pack's union, fallen back or not (-1: none yet, or the last pack was PACKED16 by request)
 *   LAST_WIRE_BYTES   bytes of count data the last pack puts on the wire per rank: 4 B per wire word, plus -- for a pack
 *                     asked for SPARSE16, fallen back or not -- the all-gathered masks, 4 * world * mask_words.  (The float column arrays, 8 B per column, are not counted:
 *                     they are the same in every form.) */
enum {
	FOSPHOR_AMD_WIRE_FRAMES_PACKED16, FOSPHOR_AMD_WIRE_FRAMES_SPARSE16, FOSPHOR_AMD_WIRE_FRAMES_FELL_BACK,
	FOSPHOR_AMD_WIRE_LAST_LIVE_ROWS, FOSPHOR_AMD_WIRE_LAST_WIRE_BYTES,
	FOSPHOR_AMD_WIRE_STATS
};
int fosphor_amd_wire_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_WIRE_STATS]);

/* Durations of the most recent launch of each of the three kernels (k_wire_mask, k_wire_pack, k_wire_unpack), in ms, from
 * hipEvents recorded around them while profiling is on (fosphor_amd_profile); -1 for a kernel that has not run with profiling on.
 * The sparse pack's time covers its union / prefix-count pass and its row copy.  Waits for the count stream. */
int fosphor_amd_wire_kernel_times(struct fosphor *self, float ms[3]);

#ifdef __cplusplus
}
#endif

#endif
