/*
 * fosphor_wire.hip -- the compact wire formats of the sharded frame's hit counts (include/fosphor_amd_wire.h)
 *
 * Three kernels between the count kernel and the merge kernel of a sharded frame, all on the count / merge stream:
 *   k_wire_mask    one presence bit per 64-cell row of the slot's uint32 counts
 *   k_wire_pack    counts -> 16-bit halves of uint32 wire words; dense (every cell) or sparse (the live rows of the union of every
 *                  rank's mask, numbered in ascending row order by a prefix count over the mask words: k_wire_scan)
 *   k_wire_unpack  the inverse, from the all-reduced words
 * Everything is a stream of 16 B loads per lane; no kernel orders anything through atomics, so the layout of the sparse form is
 * a function of the union mask alone and therefore the same on every rank.
 *
 * Geometry: a row is 64 cells = 16 uint4 of counts = 16 uint2 of wire words.  A wave works on a group of 64 rows (16 KiB of
 * counts, two mask words); 16 lanes share a row.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fosphor_internal.h"

namespace fosphor_amd {

constexpr int kWireBlock = 256;			/* 4 waves = 4 groups of 64 rows */
constexpr int kWireScanBlock = 1024;		/* the one work-group of the prefix count */
constexpr unsigned kWireDenseBlocksMax = 4096;	/* grid-stride above 1 Mi uint4 */

__device__ __forceinline__ uint2 wire_pack4(uint4 v)
{
	return make_uint2(v.x | (v.y << 16), v.z | (v.w << 16));
}

__device__ __forceinline__ uint4 wire_unpack4(uint2 w)
{
	return make_uint4(w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16);
}

/* One wave per group of 64 rows: in pass i lane l reads uint4 number 64 i + l of the group, i.e. a 16th of row 4 i + (l >> 4);
 * the ballot over "my uint4 holds a count" has the four rows of the pass in its four 16-bit quarters. */
__global__ __launch_bounds__(kWireBlock) void k_wire_mask(const uint4 *__restrict__ hc, uint32_t *__restrict__ mask, unsigned rows)
{
	const unsigned lane = threadIdx.x & 63;
	const unsigned g = blockIdx.x * (kWireBlock / 64) + (threadIdx.x >> 6);
	if ((size_t)g * 64 >= rows)
		return;							/* (the whole wave) */
	const unsigned left = rows - g * 64;
	const unsigned n16 = (left < 64 ? left : 64) * 16;		/* uint4s of the group */
	const uint4 *src = hc + (size_t)g * 64 * 16;
	uint4 v[16];
#pragma unroll
	for (int i = 0; i < 16; i++) {
		const unsigned k = i * 64 + lane;
		v[i] = k < n16 ? src[k] : make_uint4(0, 0, 0, 0);
	}
	unsigned long long bits = 0;
#pragma unroll
	for (int i = 0; i < 16; i++) {
		const unsigned long long b = __ballot((v[i].x | v[i].y | v[i].z | v[i].w) != 0);
#pragma unroll
		for (int r = 0; r < 4; r++)
			if ((b >> (16 * r)) & 0xffffull)
				bits |= 1ull << (4 * i + r);
	}
	if (lane < 2 && lane * 32 < left)
		mask[2 * g + lane] = (uint32_t)(bits >> (32 * lane));
}

/* dense form: uint4 of counts in, uint2 of words out */
__global__ __launch_bounds__(kWireBlock) void k_wire_pack_dense(const uint4 *__restrict__ hc, uint2 *__restrict__ words, size_t n4)
{
	for (size_t i = (size_t)blockIdx.x * kWireBlock + threadIdx.x; i < n4; i += (size_t)gridDim.x * kWireBlock)
		words[i] = wire_pack4(hc[i]);
}

__global__ __launch_bounds__(kWireBlock) void k_wire_unpack_dense(const uint2 *__restrict__ words, uint4 *__restrict__ hc, size_t n4)
{
	for (size_t i = (size_t)blockIdx.x * kWireBlock + threadIdx.x; i < n4; i += (size_t)gridDim.x * kWireBlock)
		hc[i] = wire_unpack4(words[i]);
}

/* sparse form, first pass -- ONE work-group: uni[w] = OR over the ranks of masks[r][w]; prefix[w] = live rows of the union in the
 * words before w; the total to the device word the row copies read and to the pinned word the host waits for.  Tiles of 1024
 * words: a wave scan (shuffles), the 16 wave totals through LDS, a running carry. */
__global__ __launch_bounds__(kWireScanBlock) void k_wire_scan(const uint32_t *__restrict__ masks, int world, unsigned n_words,
                                                              uint32_t *__restrict__ uni, uint32_t *__restrict__ prefix,
                                                              uint32_t *__restrict__ live, uint32_t *__restrict__ h_live)
{
	__shared__ uint32_t wave_total[kWireScanBlock / 64];
	const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for (unsigned base = 0; base < n_words; base += kWireScanBlock) {
		const unsigned w = base + threadIdx.x;
		uint32_t u = 0;
		if (w < n_words)
			for (int r = 0; r < world; r++)
				u |= masks[(size_t)r * n_words + w];
		const uint32_t c = __popc(u);
		uint32_t incl = c;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t t = __shfl_up(incl, d);
			if (lane >= (unsigned)d)
				incl += t;
		}
		if (lane == 63)
			wave_total[wave] = incl;
		__syncthreads();
		uint32_t before = 0, total = 0;
#pragma unroll
		for (unsigned k = 0; k < kWireScanBlock / 64; k++) {
			const uint32_t t = wave_total[k];
			before += k < wave ? t : 0;
			total += t;
		}
		__syncthreads();					/* (the next tile rewrites the totals) */
		if (w < n_words) {
			uni[w] = u;
			prefix[w] = carry + before + incl - c;
		}
		carry += total;
	}
	if (threadIdx.x == 0) {
		*live = carry;
		*h_live = carry;
	}
}

/* sparse form, the row copy in either direction.  One wave per group of 64 rows; per pass its four 16-lane quarters take the four
 * lowest live rows left in the group's 64 union bits.  Live row r of the group is row  prefix[2 g] + popcount(bits below r)  of the
 * wire.  More than half of the rows live: the frame goes out dense instead, nothing to do here. */
template <bool PACK>
__global__ __launch_bounds__(kWireBlock) void k_wire_rows(uint4 *__restrict__ hc, uint2 *__restrict__ words,
                                                          const uint32_t *__restrict__ uni, const uint32_t *__restrict__ prefix,
                                                          const uint32_t *__restrict__ live, unsigned rows)
{
	const unsigned lane = threadIdx.x & 63, quarter = lane >> 4, q = lane & 15;
	const unsigned g = blockIdx.x * (kWireBlock / 64) + (threadIdx.x >> 6);
	if ((size_t)g * 64 >= rows || *live > rows / 2)
		return;							/* (the whole wave) */
	/* (a last group of 32 rows has one mask word) */
	const unsigned long long all = uni[2 * g] | (g * 64 + 32 < rows ? (unsigned long long)uni[2 * g + 1] << 32 : 0ull);
	const uint32_t first = prefix[2 * g];
	for (unsigned long long left = all; left; ) {
		unsigned long long mine = left;
#pragma unroll
		for (unsigned k = 0; k < 3; k++)
			if (k < quarter)
				mine &= mine - 1;			/* drop the rows of the quarters before mine */
		if (mine) {
			const unsigned r = __ffsll((long long)mine) - 1;
			const size_t src = ((size_t)g * 64 + r) * 16 + q;
			const size_t dst = ((size_t)first + __popcll(all & ((1ull << r) - 1))) * 16 + q;
			if (PACK)
				words[dst] = wire_pack4(hc[src]);
			else
				hc[src] = wire_unpack4(words[dst]);
		}
#pragma unroll
		for (int k = 0; k < 4; k++)
			left &= left - 1;
	}
}

static unsigned wire_group_blocks(unsigned rows)
{
	const unsigned groups = (rows + 63) / 64;
	return (groups + kWireBlock / 64 - 1) / (kWireBlock / 64);
}

static unsigned wire_dense_blocks(size_t n4)
{
	const size_t b = (n4 + kWireBlock - 1) / kWireBlock;
	return b < kWireDenseBlocksMax ? (unsigned)b : kWireDenseBlocksMax;
}

hipError_t launch_wire_mask(const uint32_t *hc, uint32_t *mask, unsigned rows, hipStream_t s)
{
	hipLaunchKernelGGL(k_wire_mask, dim3(wire_group_blocks(rows)), dim3(kWireBlock), 0, s, (const uint4 *)hc, mask, rows);
	return hipGetLastError();
}

hipError_t launch_wire_pack_dense(const uint32_t *hc, uint32_t *words, size_t cells, hipStream_t s)
{
	const size_t n4 = cells / 4;
	hipLaunchKernelGGL(k_wire_pack_dense, dim3(wire_dense_blocks(n4)), dim3(kWireBlock), 0, s, (const uint4 *)hc, (uint2 *)words, n4);
	return hipGetLastError();
}

hipError_t launch_wire_unpack_dense(const uint32_t *words, uint32_t *hc, size_t cells, hipStream_t s)
{
	const size_t n4 = cells / 4;
	hipLaunchKernelGGL(k_wire_unpack_dense, dim3(wire_dense_blocks(n4)), dim3(kWireBlock), 0, s, (const uint2 *)words, (uint4 *)hc, n4);
	return hipGetLastError();
}

hipError_t launch_wire_pack_sparse(const uint32_t *hc, const uint32_t *masks, int world, uint32_t *uni, uint32_t *prefix,
                                   uint32_t *live, uint32_t *h_live, uint32_t *words, unsigned rows, hipStream_t s)
{
	hipLaunchKernelGGL(k_wire_scan, dim3(1), dim3(kWireScanBlock), 0, s, masks, world, rows / 32, uni, prefix, live, h_live);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_wire_rows<true>, dim3(wire_group_blocks(rows)), dim3(kWireBlock), 0, s, (uint4 *)const_cast<uint32_t *>(hc),
	                   (uint2 *)words, (const uint32_t *)uni, (const uint32_t *)prefix, (const uint32_t *)live, rows);
	return hipGetLastError();
}

hipError_t launch_wire_unpack_sparse(const uint32_t *words, const uint32_t *uni, const uint32_t *prefix, const uint32_t *live,
                                     uint32_t *hc, unsigned rows, hipStream_t s)
{
	hipLaunchKernelGGL(k_wire_rows<false>, dim3(wire_group_blocks(rows)), dim3(kWireBlock), 0, s, (uint4 *)hc,
	                   (uint2 *)const_cast<uint32_t *>(words), uni, prefix, live, rows);
	return hipGetLastError();
}

} // namespace fosphor_amd
