/*
 * fosphor_rs.h -- what the two files of the Reed-Solomon pass share (include/fosphor_amd_rs.h): fosphor_rs.hip (the kernels and
 * the device entry point) and fosphor_rs_host.cpp (the host statement, the encoder and the helpers, plain C++ without a HIP
 * header, so that a sanitized build of the host side is one file).  The arithmetic of GF(2^8), formed by one helper on the device
 * and on the host alike, and the plan of a call as rule 7 checks it.  Private to gr-fosphor_amd/csrc: no caller includes it.
 */
#ifndef FOSPHOR_RS_H
#define FOSPHOR_RS_H

#include <stdint.h>

#include <vector>

#include "../../include/fosphor_amd_rs.h"

#ifdef __HIPCC__
#define RS_HD inline __host__ __device__
#else
#define RS_HD inline
#endif

namespace rs {

/* ---- GF(2^8) modulo poly (bit 8 set), alpha = 2: eight steps of shift and XOR, no table ---- */

RS_HD uint32_t gf_mul(uint32_t a, uint32_t b, uint32_t poly)
{
	uint32_t acc = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		acc ^= a & (0u - ((b >> i) & 1u));
		a <<= 1;
		a ^= poly & (0u - (a >> 8));
	}
	return acc;
}

/* a^e, 0 <= e < 256 */
RS_HD uint32_t gf_pow(uint32_t a, uint32_t e, uint32_t poly)
{
	uint32_t r = 1;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		if ((e >> i) & 1u)
			r = gf_mul(r, a, poly);
		a = gf_mul(a, a, poly);
	}
	return r;
}

/* alpha^e, 0 <= e < 256 */
RS_HD uint32_t gf_exp(uint32_t e, uint32_t poly) { return gf_pow(2u, e, poly); }

/* 1 / a = a^254; a != 0 */
RS_HD uint32_t gf_inv(uint32_t a, uint32_t poly) { return gf_pow(a, 254u, poly); }

/* the exponent of root j of the generator, prim (fcr + j) mod 255 */
RS_HD uint32_t root_exp(int prim, int fcr, int j) { return (uint32_t)((prim * (fcr + j)) % 255); }

/* rule 4: the exponent of 1 / X_i, X_i = alpha^(prim (n_code - 1 - i)) */
RS_HD uint32_t inv_locator_exp(int prim, int n_code, int i) { return (uint32_t)((255 - (prim * (n_code - 1 - i)) % 255) % 255); }

/* ---- the plan of a call ---- */

struct Plan {
	long long codewords, words;		/* of the call: the sum of the depths, and of the owned 64-bit words */
	std::vector<int32_t> seq_at;		/* per job where its scrambler sequence begins in `seq`, -1 without one */
	std::vector<uint8_t> seq;		/* rule 1's bytes, one sequence for all the jobs of one scrambler, each padded to 8 bytes */
};

inline int32_t n_data_of(const struct fosphor_amd_rs_job &b) { return (int32_t)b.depth * ((int32_t)b.n_code - (int32_t)b.n_roots); }
inline int64_t owned_of(int32_t n_data) { return 8 * (((int64_t)n_data + 7) / 8); }

/* rule 7 of one job's fields, without its ranges */
bool job_ok(const struct fosphor_amd_rs_job &b);

/* rule 1: n bytes of the sequence */
void scramble_bytes(int w, uint32_t taps, uint32_t init, uint8_t *seq, int n);

/* What both entry points refuse, but for the pointers; fills the plan. */
int check_call(int64_t n_bytes, const struct fosphor_amd_rs_job *jobs, int n_jobs, int64_t out_capacity, Plan *plan);

} // namespace rs

#endif
