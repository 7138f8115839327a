/*
 * fosphor_trellis.h -- the integer rules that the two decoders of burst symbols share: fosphor_decode.hip (hard decisions,
 * include/fosphor_amd_decode.h) and fosphor_soft.hip (soft decisions, include/fosphor_amd_soft.h).  Rules 2, 3, 6 and 7 of
 * fosphor_amd_decode.h and the checks of its rule 9 that concern the code alone, each formed by one helper on the device and in
 * the host statements alike.  Private to gr-fosphor_amd/csrc: no caller includes it.
 */
#ifndef FOSPHOR_TRELLIS_H
#define FOSPHOR_TRELLIS_H

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/fosphor_amd_decode.h"			/* the status values of rule 7 */

namespace trellis {

inline __host__ __device__ int popc(uint32_t v) { return __builtin_popcount(v); }

/* rule 2: the kept bits of the first T steps */
inline __host__ __device__ int64_t kept_of(int64_t T, int period, const uint16_t *punct, int weight)
{
	const uint32_t below = (1u << (int)(T % period)) - 1u;
	return (T / period) * weight + popc(punct[0] & below) + popc(punct[1] & below) + popc(punct[2] & below);
}

/* rule 3: what the encoder sends on the branch from state p with input u, stream i in bit i */
inline __host__ __device__ uint32_t expected_of(const uint16_t *polys, int n_poly, int k, int u, int p)
{
	const uint32_t R = ((uint32_t)u << (k - 1)) | (uint32_t)p;
	uint32_t e = 0;
	for (int i = 0; i < 3 && i < n_poly; i++)
		e |= (uint32_t)(popc(polys[i] & R) & 1) << i;
	return e;
}

/* rule 6: where decoded bit i of a block of 64 lies in the block's output word, stored little-endian */
inline __host__ __device__ int bit_place(int i) { return 8 * (i >> 3) + 7 - (i & 7); }

/* rule 7 over the job's owned bytes */
inline __host__ __device__ void crc_of(const uint8_t *out, int n_bits, int w, uint32_t poly, uint32_t init, uint32_t xorout,
                                       uint32_t &calc, uint32_t &recv, int &status)
{
	calc = recv = 0;
	status = FOSPHOR_AMD_DECODE_OK;
	if (w == 0)
		return;
	if (n_bits < w) {
		status = FOSPHOR_AMD_DECODE_SHORT;
		return;
	}
	const int n_data = n_bits - w;
	const uint32_t mask = w == 32 ? 0xffffffffu : (1u << w) - 1u;
	uint32_t reg = init;
	for (int t0 = 0; t0 < n_data; t0 += 8) {
		const uint32_t byte = out[t0 >> 3];
		for (int i = 0; i < 8 && t0 + i < n_data; i++) {
			const uint32_t top = ((reg >> (w - 1)) ^ (byte >> (7 - i))) & 1u;
			reg = (reg << 1) & mask;
			if (top)
				reg ^= poly;
		}
	}
	calc = reg ^ xorout;
	for (int t = n_data; t < n_bits && t < n_data + 32; t++)
		recv = (recv << 1) | ((out[t >> 3] >> (7 - (t & 7))) & 1u);
	if (calc != recv)
		status = FOSPHOR_AMD_DECODE_CRC_FAIL;
}

inline bool order_ok(int order) { return order == 2 || order == 4 || order == 8; }
inline int bits_of(int order) { return order == 2 ? 1 : (order == 4 ? 2 : 3); }

/* rule 9, of the puncture pattern alone */
inline bool punct_ok(int n_poly, int period, const uint16_t *punct, int *weight)
{
	if ((n_poly != 2 && n_poly != 3) || period < 1 || period > 16 || !punct)
		return false;
	int w = 0;
	for (int i = 0; i < 3; i++) {
		if ((uint32_t)punct[i] >> period || (i >= n_poly && punct[i]))
			return false;
		w += popc(punct[i]);
	}
	*weight = w;
	return w > 0;
}

/* rule 2: the largest T with kept(T) <= coded */
inline int64_t steps_that_fit(int64_t coded, int period, const uint16_t *punct, int weight)
{
	int64_t T = (coded / weight) * period;
	for (int i = 0; i < 16 && kept_of(T + 1, period, punct, weight) <= coded; i++)
		T++;
	return T;
}

/* the bytes a job owns in d_out */
inline int64_t owned_of(int32_t n_bits) { return 8 * (((int64_t)n_bits + 63) / 64); }

} // namespace trellis

#endif
