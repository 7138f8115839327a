/*
 * fosphor_kernels.hip -- CDNA4 (gfx950) kernels of the fosphor compute core
 *
 * Replaces lib/fosphor/fft.cl + lib/fosphor/display.cl of the reference.
 * Compile with:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
 * -ffp-contract=off is REQUIRED: the FFT must round exactly where the reference's
 * expressions round (mul, then add), or histogram counts stop being bit-exact.
 *
 * K1  k1_fft_bin   one WAVE per spectrum (64 lanes x 16 points), no block barriers.
 *                  Radix 8.8.8.2 Stockham with the reference's exact butterfly and
 *                  twiddle order (fft.cl:86-145,278-350,397-466); three exchanges
 *                  through an XOR-swizzled 8 KiB LDS slab per wave; twiddles and
 *                  window live in registers for the whole tile of spectra.
 *                  Epilogue per sample: |X|^2 -> v_log_f32 -> bin guess, accepted
 *                  when provably on the right side of a bin edge, otherwise decided
 *                  by comparing the double-precision |X|^2 with host-computed exact
 *                  thresholds (fosphor_portable_math.h) -- so integer bins equal the
 *                  oracle's log10(hypot()) pipeline bit for bit without evaluating it.
 * K2  k2_count     LDS-privatised histogram per (16-column slab, batch): ds_add on
 *                  [bin][col] (display.cl:161-177), plus the per-batch live sum / max.
 * K3  k3_merge     per (bin, x) cell rise/decay over all batches of the launch in
 *                  order (display.cl:217-254); live EMA + max-hold (display.cl:186-214,
 *                  257-310).
 */
#include <atomic>

#include "fosphor_internal.h"

#pragma clang fp contract(off)

namespace fosphor_amd {

/* Build switches.  The only ones these sources have are the phase-timing builds, each a -D on the hipcc line; results stay correct:
 *   K1_TIMING=1   the 1024-point kernel    (tools/k1_phase_timing.py)     K1W_TIMING=1  the 8192-point kernel   (tools/k1w_phase_timing.py)
 *   K1H_TIMING=1  the 65536-point kernel   (tools/k1h_phase_timing.py)    K2_TIMING     the count kernel        (tools/k2_phase_timing.py)
 * The alternatives measured against the shipped code are recorded in profiles/ and DESIGN_HISTORY.md. */

/* ------------------------------------------------------------------------ */
/* Complex helpers: same operations, same order as fft.cl                   */
/* ------------------------------------------------------------------------ */
/* A complex value is one 64-bit VGPR pair (re, im).  Every helper performs exactly the IEEE
 * operations of the reference expression it cites -- only the instruction selection differs:
 * the half-swaps and sign flips of the reference's "multiply by -j" and of the
 * complex product ride on VOP3P op_sel / neg modifiers instead of costing v_mov / extra adds.
 * x - (-y) and x + y are the same IEEE operation, as are a*b and b*a, a+b and b+a.          */


typedef float v2f __attribute__((ext_vector_type(2)));

#define F_SQRT_1_2 (0.707106781188f)	/* fft.cl:72 */

/* fft.cl:37-46 : (a.x*w.x - a.y*w.y, a.x*w.y + a.y*w.x) */
static __device__ __forceinline__ v2f c_mul(v2f a, v2f w)
{
	v2f t1, t2, r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t1) : "v"(a), "v"(w));			/* (a.x*w.x, a.y*w.x) */
	asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t2) : "v"(a), "v"(w));	/* (a.y*w.y, a.x*w.y) */
	asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(t1), "v"(t2));			/* (t1.x - t2.x, t1.y + t2.y) */
	return r;
}
/* N complex products step by step (all first products, all second, all sums; pinned order): written one after the other, the dependent
 * statements of a product end up adjacent and the compiler puts an s_nop between them (it assumes a value written by inline assembly
 * cannot be forwarded) -- 28 issue slots per spectrum in the 1024-point kernel.  out[j] = in[j] * w[j], the same three operations. */
template <int N>
static __device__ __forceinline__ void c_mul_n(v2f (&out)[N], const v2f (&in)[N], const v2f (&w)[N])
{
	v2f t1[N], t2[N];
#pragma unroll
	for (int j = 0; j < N; j++)
		asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t1[j]) : "v"(in[j]), "v"(w[j]));
#pragma unroll
	for (int j = 0; j < N; j++)
		asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t2[j]) : "v"(in[j]), "v"(w[j]));
#pragma unroll
	for (int j = 0; j < N; j++)
		asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(out[j]) : "v"(t1[j]), "v"(t2[j]));
}

/* a + mul_p1q2(b) and a - mul_p1q2(b), mul_p1q2(b) = (b.y, -b.x)  (fft.cl:77, used by dft8) */
static __device__ __forceinline__ v2f add_mj(v2f a, v2f b)
{
	v2f r;
	asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
	return r;
}
static __device__ __forceinline__ v2f sub_mj(v2f a, v2f b)
{
	v2f r;
	asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
	return r;
}

/* fft.cl:80 : SQRT_1_2 * (a.x + a.y, -a.x + a.y) */
static __device__ __forceinline__ v2f mul_p1q4(v2f a, v2f s12)
{
	v2f t, r;
	asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(t) : "v"(a));	/* (a.x + a.y, a.y + -a.x) */
	asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(t), "v"(s12));
	return r;
}
/* fft.cl:82 : SQRT_1_2 * (-a.x + a.y, -a.x - a.y) */
static __device__ __forceinline__ v2f mul_p3q4(v2f a, v2f s12)
{
	v2f t, r;
	asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_lo:[1,0] neg_hi:[1,1]" : "=v"(t) : "v"(a));	/* (-a.x + a.y, -a.x + -a.y) */
	asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(t), "v"(s12));
	return r;
}

/* fft.cl:86-94 */
#define DFT2(a, b) do { v2f _t = (a) - (b); (a) = (a) + (b); (b) = _t; } while (0)
/* dft2(a, mul_p1q2(b)) */
#define DFT2_MJ(a, b) do { v2f _t = sub_mj((a), (b)); (a) = add_mj((a), (b)); (b) = _t; } while (0)

/* fft.cl:112-145.  The three mul_p1q2 twiddles (r6 after stage 1; r3, r7 after stage 2) are
 * folded into the butterflies that consume them. */
static __device__ __forceinline__ void dft8(v2f (&r)[8], v2f s12)
{
	DFT2(r[0], r[4]); DFT2(r[1], r[5]); DFT2(r[2], r[6]); DFT2(r[3], r[7]);
	r[5] = mul_p1q4(r[5], s12); r[7] = mul_p3q4(r[7], s12);
	DFT2(r[0], r[2]); DFT2(r[1], r[3]); DFT2_MJ(r[4], r[6]); DFT2(r[5], r[7]);
	DFT2(r[0], r[1]); DFT2_MJ(r[2], r[3]); DFT2(r[4], r[5]); DFT2_MJ(r[6], r[7]);
}

/* ------------------------------------------------------------------------ */
/* The long plans (N = 8192, 65536): twiddles on the butterflies, fused multiply-adds */
/* ------------------------------------------------------------------------ */
/* No reference behaviour exists at these lengths; the plan is this build's and the oracle restates it operation for operation
 * (oracle/fosphor_oracle.c: o_bf, o_bf_mj, o_bf_win, o_pass_radix16_fma, o_pass_radix2_fma -- the derivation is
 * written there).  A radix-R pass is log2 R radix-2 stages in decimation-in-time form, every butterfly
 *      a' = a + T b  (two v_pk_fma_f32)      b' = 2 a - a'  (one)
 * with T the twiddle of its stage and position: 36 packed operations per 8 points and pass instead of 49 (21 for seven complex
 * products + 28 for dft8), 96 per 16 points instead of 133, and 4 / 8 twiddles per item instead of 7 / 15.  Every operation is one
 * IEEE operation here and one fmaf / add / multiply there. */

/* o_bf: u = (a.x - b.y T.y, a.y + b.x T.y);  a' = (u.x + b.x T.x, u.y + b.y T.x);  b' = 2 a - a'
 * SC (the 8192-point kernel, which has no vector register to spare): `two` = (2, 2) travels in a scalar register pair -- a packed operation
 * takes one scalar source --, and so do the twiddles that are the same for every thread (bf_s, bf_mj_s: W8, W16, W16^3 of a first pass). */
template <bool SC = false>
static __device__ __forceinline__ void bf(v2f &a, v2f &b, v2f t, v2f two)
{
	v2f u, pa, nb;
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(u) : "v"(b), "v"(t), "v"(a));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(pa) : "v"(b), "v"(t), "v"(u));
	if (SC) asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "s"(two), "v"(pa));
	else    asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "v"(two), "v"(pa));
	a = pa; b = nb;
}
/* o_bf_mj (T := -j T): u = (a.x + b.x T.y, a.y + b.y T.y);  a' = (u.x + b.y T.x, u.y - b.x T.x);  b' = 2 a - a' */
template <bool SC = false>
static __device__ __forceinline__ void bf_mj(v2f &a, v2f &b, v2f t, v2f two)
{
	v2f u, pa, nb;
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(u) : "v"(b), "v"(t), "v"(a));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(pa) : "v"(b), "v"(t), "v"(u));
	if (SC) asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "s"(two), "v"(pa));
	else    asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "v"(two), "v"(pa));
	a = pa; b = nb;
}
/* ... with a twiddle that is the same for every thread */
template <bool SC = false>
static __device__ __forceinline__ void bf_s(v2f &a, v2f &b, v2f t, v2f two)
{
	if (!SC) { bf<false>(a, b, t, two); return; }
	v2f u, pa, nb;
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(u) : "v"(b), "s"(t), "v"(a));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(pa) : "v"(b), "s"(t), "v"(u));
	asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "s"(two), "v"(pa));
	a = pa; b = nb;
}
template <bool SC = false>
static __device__ __forceinline__ void bf_mj_s(v2f &a, v2f &b, v2f t, v2f two)
{
	if (!SC) { bf_mj<false>(a, b, t, two); return; }
	v2f u, pa, nb;
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(u) : "v"(b), "s"(t), "v"(a));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(pa) : "v"(b), "s"(t), "v"(u));
	asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb) : "v"(a), "s"(two), "v"(pa));
	a = pa; b = nb;
}
/* Eight (CNT) butterflies of one stage, STEP BY STEP (all first operations, all second, all third): written butterfly by butterfly, dependent
 * inline-assembly statements end up adjacent and the compiler separates each such pair by an s_nop (it assumes a value written by inline
 * assembly cannot be forwarded): ~50 issue slots per thread and spectrum in the 8192-point kernel.  IA / IB: registers of the a / b inputs,
 * MJ: bit j set = butterfly j takes -j T (bf_mj). */
template <bool SC, bool TS, int MJ, int I0, int I1, int I2, int I3, int I4, int I5, int I6, int I7, int D, int CNT = 8, bool SW = SC>
static __device__ __forceinline__ void bf8(v2f (&r)[16], v2f t0, v2f t1, v2f t2, v2f t3, v2f t4, v2f t5, v2f t6, v2f t7, v2f two)
{
	constexpr int ia[8] = { I0, I1, I2, I3, I4, I5, I6, I7 };
	const v2f t[8] = { t0, t1, t2, t3, t4, t5, t6, t7 };
	if (SW) {		/* (SW: the 65536-point kernel measured 5 % slower in this form: 207 -> 217 registers under its skewed loop) */
	v2f u[8], pa[8], nb[8];
#pragma unroll
	for (int j = 0; j < CNT; j++) {
		if (MJ & (1 << j)) {
			if (TS) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(u[j]) : "v"(r[ia[j] + D]), "s"(t[j]), "v"(r[ia[j]]));
			else    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(u[j]) : "v"(r[ia[j] + D]), "v"(t[j]), "v"(r[ia[j]]));
		} else {
			if (TS) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(u[j]) : "v"(r[ia[j] + D]), "s"(t[j]), "v"(r[ia[j]]));
			else    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(u[j]) : "v"(r[ia[j] + D]), "v"(t[j]), "v"(r[ia[j]]));
		}
	}
#pragma unroll
	for (int j = 0; j < CNT; j++) {
		if (MJ & (1 << j)) {
			if (TS) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(pa[j]) : "v"(r[ia[j] + D]), "s"(t[j]), "v"(u[j]));
			else    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(pa[j]) : "v"(r[ia[j] + D]), "v"(t[j]), "v"(u[j]));
		} else {
			if (TS) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(pa[j]) : "v"(r[ia[j] + D]), "s"(t[j]), "v"(u[j]));
			else    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(pa[j]) : "v"(r[ia[j] + D]), "v"(t[j]), "v"(u[j]));
		}
	}
#pragma unroll
	for (int j = 0; j < CNT; j++) {
		if (SC) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb[j]) : "v"(r[ia[j]]), "s"(two), "v"(pa[j]));
		else    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(nb[j]) : "v"(r[ia[j]]), "v"(two), "v"(pa[j]));
	}
#pragma unroll
	for (int j = 0; j < CNT; j++) { r[ia[j]] = pa[j]; r[ia[j] + D] = nb[j]; }
	} else {
#pragma unroll
	for (int j = 0; j < CNT; j++) {
		if (MJ & (1 << j)) { if (TS) bf_mj_s<SC>(r[ia[j]], r[ia[j] + D], t[j], two); else bf_mj<SC>(r[ia[j]], r[ia[j] + D], t[j], two); }
		else               { if (TS) bf_s<SC>(r[ia[j]], r[ia[j] + D], t[j], two);    else bf<SC>(r[ia[j]], r[ia[j] + D], t[j], two); }
	}
	}
}

/* o_bf_win, stage A of the first pass: m = a wab.x;  a' = fma(b, wab.y, m);  b' = fma(-b, wab.y, m)   (wab = the two window taps) */
static __device__ __forceinline__ void bf_win(v2f &a, v2f &b, v2f wab)
{
	v2f m, pa, nb;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(m) : "v"(a), "v"(wab));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(pa) : "v"(b), "v"(wab), "v"(m));
	asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(nb) : "v"(b), "v"(wab), "v"(m));
	a = pa; b = nb;
}

/* o_pass_radix16_fma, p > 1, in two halves (the 65536-point kernel runs other work between them):
 * stages A, B: t8 = w^8, t4 = w^4;  stages C, D: t2 = w^2, t2w = w^2 W8, t1 = w, t1a = w W16, t1b = w W8, t1c = w W16^3.
 * X[m] is left in r[bitrev4(m)] (R16_PERM). */
template <bool SC = false, bool SW = SC>
static __device__ __forceinline__ void pass16_ab(v2f (&r)[16], v2f t8, v2f t4, v2f two)
{
	bf8<SC, false, 0x00, 0, 1, 2, 3, 4, 5, 6, 7, 8, 8, SW>(r, t8, t8, t8, t8, t8, t8, t8, t8, two);		/* stage A: (j, j + 8) */
	bf8<SC, false, 0xf0, 0, 1, 2, 3, 8, 9, 10, 11, 4, 8, SW>(r, t4, t4, t4, t4, t4, t4, t4, t4, two);		/* stage B: (j, j + 4); -j on the upper half */
}
template <bool SC = false, bool SW = SC>
static __device__ __forceinline__ void pass16_cd(v2f (&r)[16], v2f t2, v2f t2w, v2f t1, v2f t1a, v2f t1b, v2f t1c, v2f two)
{
	bf8<SC, false, 0xf0, 0, 1, 8, 9, 4, 5, 12, 13, 2, 8, SW>(r, t2, t2, t2w, t2w, t2, t2, t2w, t2w, two);	/* stage C: (j, j + 2) */
	bf8<SC, false, 0xaa, 0, 2, 4, 6, 8, 10, 12, 14, 1, 8, SW>(r, t1, t1, t1b, t1b, t1a, t1a, t1c, t1c, two);	/* stage D: (j, j + 1) */
}
/* ... p = 1: the window on stage A (wab[j] = taps of r[j], r[j + 8]); w16 = W16, w8 = W8, w163 = W16^3 */
template <bool SC = false, bool SW = SC>
static __device__ __forceinline__ void pass16_first(v2f (&r)[16], const v2f (&wab)[8], v2f w16, v2f w8, v2f w163, v2f two)
{
	if (SW) {
		/* stage A step by step as well: the products, then the sums, then the differences */
		v2f m[8], pa[8], nb[8];
#pragma unroll
		for (int j = 0; j < 8; j++)
			asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(m[j]) : "v"(r[j]), "v"(wab[j]));
#pragma unroll
		for (int j = 0; j < 8; j++)
			asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(pa[j]) : "v"(r[j + 8]), "v"(wab[j]), "v"(m[j]));
#pragma unroll
		for (int j = 0; j < 8; j++)
			asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(nb[j]) : "v"(r[j + 8]), "v"(wab[j]), "v"(m[j]));
#pragma unroll
		for (int j = 0; j < 8; j++) { r[j] = pa[j]; r[j + 8] = nb[j]; }
	} else {
#pragma unroll
		for (int j = 0; j < 8; j++)
			bf_win(r[j], r[j + 8], wab[j]);
	}
#pragma unroll
	for (int j = 0; j < 4; j++) {
		DFT2(r[j], r[j + 4]);
		DFT2_MJ(r[8 + j], r[12 + j]);
	}
#pragma unroll
	for (int j = 0; j < 2; j++) {
		DFT2(r[j], r[j + 2]);
		DFT2_MJ(r[4 + j], r[6 + j]);
	}
	bf8<SC, true, 0x0c, 8, 9, 12, 13, 0, 0, 0, 0, 2, 4, SW>(r, w8, w8, w8, w8, w8, w8, w8, w8, two);	/* stage C, the twiddled half: (8, 10), (9, 11), -j: (12, 14), (13, 15) */
	DFT2(r[0], r[1]);          DFT2_MJ(r[2], r[3]);
	bf8<SC, true, 0x2a, 4, 6, 8, 10, 12, 14, 0, 0, 1, 6, SW>(r, w8, w8, w16, w16, w163, w163, w8, w8, two);	/* stage D: (4, 5) W8, -j (6, 7) W8, (8, 9) W16, -j (10, 11), (12, 13) W16^3, -j (14, 15) */
}

/* x * w with w broadcast from the low / high half of a pair (fft.cl:415-417) */
static __device__ __forceinline__ v2f mul_bcast_lo(v2f x, v2f w)
{
	v2f r; asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(w)); return r;
}
static __device__ __forceinline__ v2f mul_bcast_hi(v2f x, v2f w)
{
	v2f r; asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(x), "v"(w)); return r;
}

/* Order in which a radix-8 pass stores its outputs: offsets {0,p,..,7p} receive
 * r[0,4,2,6,1,5,3,7] (fft.cl:321-328). */
#define R8_PERM(jj) (((jj) == 0) ? 0 : ((jj) == 1) ? 4 : ((jj) == 2) ? 2 : ((jj) == 3) ? 6 : \
                     ((jj) == 4) ? 1 : ((jj) == 5) ? 5 : ((jj) == 6) ? 3 : 7)

/* Intra-wave LDS exchange: the store phase and the load phase of an exchange are separated by wavefront-scope release /
 * acquire fences around a wave barrier (the compiler must not move a load above a store it cannot prove aliases; the fences
 * cost an s_waitcnt lgkmcnt(0) each).  In principle program order alone would do -- all DS instructions of one wave execute in
 * order -- and a build with compiler-only barriers was measured in round 3: 519-525 against 523-526 GSamples/s, nothing; the
 * conservative form stays. */
static __device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* ------------------------------------------------------------------------ */
/* Exact binning                                                            */
/* ------------------------------------------------------------------------ */

#define F_HALF_LOG10_2 (0.150514997831990597606869447362f)	/* pwr = log10|X| = this * log2(|X|^2) */
/* Inside K1 the log-power is carried as l2 = log2(|X|^2) and scaled once where it leaves. */

/* Decide a sample the fast path could not: compare |X|^2, formed in double with one
 * rounding (both squares are exact), against the exact thresholds.
 * thr[b] for b in [1, nb) = smallest double s with oracle_bin(s) >= b; thr[0] = -1;
 * thr[nb] = smallest s whose hypot overflows float (-> non-finite -> bin 0,
 * fosphor_portable_math.h fpm_bin_from_pwr). */
/* Where the exact path finds its thresholds.  It runs for ~1.5e-4 of the samples, i.e. in every sixth wave-spectrum, and a table load
 * through the vector memory path returns IN ORDER behind whatever the wave has in flight -- the next spectrum's IQ, requested from HBM
 * before the epilogue: measured on the 8192-point kernel, whose eight waves then all wait at the next barrier, 369 -> 318 us per launch
 * with the path removed.  Two ways around it:
 *   an LDS copy of the table (address_space(3) pointer: ds_read, its own counter) where the kernel has 2-4 KiB of LDS to spare;
 *   ThrScalar: the table entries fetched by the SCALAR unit (s_load_dwordx4 through the scalar cache, counted by lgkmcnt, out of order
 *   with the vector loads), one active lane after the other (usually there is exactly one). */
struct ThrScalar { const double *p; };
typedef uint32_t thr_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t thr_u2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ double thr_mk(uint32_t lo, uint32_t hi)
{
	return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
/* t0 = thr[i], t1 = thr[i + 1] for every active lane */
template <typename ThrPtr>
static __device__ __forceinline__ void thr_pair(ThrPtr thr, int i, double *t0, double *t1)
{
	*t0 = thr[i];
	*t1 = thr[i + 1];
}
template <>
__device__ __forceinline__ void thr_pair<ThrScalar>(ThrScalar thr, int i, double *t0, double *t1)
{
	double a = 0.0, b = 0.0;
	unsigned long long todo = __builtin_amdgcn_ballot_w64(true);		/* the active lanes */
	while (todo) {
		const int l = __builtin_ctzll(todo);
		const int g = __builtin_amdgcn_readlane(i, l);
		thr_u4 v;
		asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(thr.p + g) : "memory");
		const bool mine = (i == g);
		if (mine) { a = thr_mk(v.x, v.y); b = thr_mk(v.z, v.w); }
		todo &= ~__builtin_amdgcn_ballot_w64(mine);
	}
	*t0 = a; *t1 = b;
}
template <typename ThrPtr>
static __device__ __forceinline__ double thr_one(ThrPtr thr, int i)
{
	return thr[i];
}
template <>
__device__ __forceinline__ double thr_one<ThrScalar>(ThrScalar thr, int i)
{
	double a = 0.0;
	unsigned long long todo = __builtin_amdgcn_ballot_w64(true);
	while (todo) {
		const int l = __builtin_ctzll(todo);
		const int g = __builtin_amdgcn_readlane(i, l);
		thr_u2 v;
		asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(thr.p + g) : "memory");
		const bool mine = (i == g);
		if (mine) a = thr_mk(v.x, v.y);
		todo &= ~__builtin_amdgcn_ballot_w64(mine);
	}
	return a;
}

template <typename ThrPtr>		/* const double * (vector loads), an LDS pointer (a kernel's own copy of the table), or ThrScalar */
static __device__ __forceinline__ uint32_t bin_exact(float re, float im, float l2_fast, int guess,
                                                      ThrPtr thr, int nb, float *l2_out)
{
	const double xr = (double)re, xi = (double)im;
	const double sd = __builtin_fma(xr, xr, xi * xi);
	const float  sf = (float)sd;
	int bin;

	if (sf >= 1e-30f && sf <= 1e30f) {
		/* the guess is within one bin of the truth */
		double t0, t1;
		thr_pair(thr, guess, &t0, &t1);
		bin = guess - (sd < t0 ? 1 : 0) + (sd >= t1 ? 1 : 0);
		*l2_out = l2_fast;
	} else {
		/* zero, denormal, huge, inf or NaN: full search, and a log-power that does not
		 * depend on |X|^2 fitting a float: split sd = m * 2^e, m in [1,2) */
		int lo = 0, hi = nb;		/* invariant: sd >= thr[lo] (thr[0] = -1); sd < thr[hi] or hi == nb */
		const double t_top = thr_one(thr, nb);
		if (sd >= t_top) {
			bin = nb;
		} else if (!(sd >= 0.0)) {
			bin = 0;		/* NaN */
		} else {
			while (hi - lo > 1) {
				int mid = (lo + hi) >> 1;
				if (sd >= thr_one(thr, mid)) lo = mid; else hi = mid;
			}
			bin = lo;
		}
		if (__builtin_isinf(re) || __builtin_isinf(im) || sd >= t_top) {
			*l2_out = __builtin_inff();		/* hypot(inf, anything) = inf; float hypot overflow */
		} else if (sd == 0.0) {
			*l2_out = -__builtin_inff();		/* log10(0) */
		} else if (sd != sd) {
			*l2_out = __builtin_nanf("");
		} else {
			/* A float hypot below 2^-126 is a subnormal float, k * 2^-149 with few bits, and the reference takes the logarithm of
			 * THAT (display.cl:136): with k = 8 the rounding moves log10 by up to 0.03.  re and im are then subnormal themselves,
			 * so m = sd * 2^298 is an integer below 2^47 and exact; (k + 1/2)^2 is no integer, so no tie exists and k is the
			 * integer with k^2 - k < m <= k^2 + k: a float estimate of sqrt(m), within 2 of it, corrected twice. */
			double sl = sd;
			if (sd < 0x1p-252) {
				const double m = sd * 0x1p298;
				double k = __builtin_rint((double)__builtin_sqrtf((float)m));
				for (int it = 0; it < 2; it++)
					k += (m > __builtin_fma(k, k, k)) ? 1.0 : (m <= __builtin_fma(k, k, -k)) ? -1.0 : 0.0;
				sl = (k * k) * 0x1p-298;
			}
			const unsigned long long u = (unsigned long long)__double_as_longlong(sl);
			const int e = (int)((u >> 52) & 0x7ff) - 1023;
			const double m = __longlong_as_double((long long)((u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL));
			*l2_out = (float)e + __builtin_amdgcn_logf((float)m);
		}
	}
	if (bin >= nb)
		bin = 0;
	return (uint32_t)bin;
}

struct BinConst { float A, C, amb, kappa; int nb; const double *thr; };

/* Fast path.  Returns r = rint(v) (the bin guess before clamping, as a float), l2 = log2(|X|^2)
 * and the sample's ambiguity measure
 *     amb = |v - r| + kappa * |l2|
 * -- distance of the scaled log-power from the bin centre, plus the v_log_f32 error bound
 * (<= 1 ulp of l2, through the slope A: kappa = 2 * A * 2^-23, the factor 2 is margin; it also
 * covers the rounding of s32).  The guess is provably exact iff amb <= 0.5 - delta0, delta0
 * bounding the roundings that do not scale with l2.  amb is >= 0,
 * +inf for |X|^2 in {0, denormal-flushed, inf}, NaN for NaN: compared as an unsigned bit
 * pattern all of those order above every finite value, so one running v_max_u32 per spectrum
 * collects "some sample needs the exact path" without per-sample compares or branches. */
static __device__ __forceinline__ float bin_fast(float re, float im, const BinConst &k, float *l2_out, uint32_t *amb_bits)
{
	const float s  = __builtin_fmaf(re, re, im * im);
	const float l2 = __builtin_amdgcn_logf(s);		/* v_log_f32 */
	const float v  = __builtin_fmaf(k.A, l2, k.C);
	const float r  = __builtin_rintf(v);
	const float a  = __builtin_fmaf(__builtin_fabsf(l2), k.kappa, __builtin_fabsf(v - r));
	*l2_out = l2;
	*amb_bits = __float_as_uint(a);
	return r;
}

/* bin byte of a float guess r: saturating float -> u8 (NaN -> 0), capped at nb-1 */
static __device__ __forceinline__ uint32_t pack_bin(float r, float top, uint32_t byte, uint32_t old)
{
	return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fminf(r, top), byte, old);
}

static __device__ __forceinline__ float max_f32(float a, float b)
{
	/* one v_max_f32 (IEEE mode: a NaN operand is dropped = OpenCL max(acc, NaN) keeps acc,
	 * display.cl:139); fmaxf() would add two canonicalising self-max instructions */
	float r;
	asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
	return r;
}

/* ------------------------------------------------------------------------ */
/* K1                                                                       */
/* ------------------------------------------------------------------------ */

constexpr int kK1WavesPerSimd = 2;		/* __launch_bounds__ second argument (measured) */

/* K1_TIMING=1 (debug builds only, tools/k1_phase_timing.py): s_memtime stamps per phase,
 * accumulated per wave into K1Params::dbg[wave][phase]. */
#ifndef K1_TIMING
#define K1_TIMING 0
#endif
#if K1_TIMING
#define K1_STAMP(i) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
		const long long _now = __builtin_readcyclecounter(); tacc[i] += _now - tprev; tprev = _now; } while (0)
#else
#define K1_STAMP(i) do { } while (0)
#endif

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

/* Buffer addressing for the 8192- and 65536-point kernels: every global access of their loops is `scalar base (descriptor) + ONE 32-bit per-lane
 * offset + a scalar offset` -- buffer_load / buffer_store ... offen -- where the per-lane offset is fixed for the kernel's lifetime and
 * everything that changes (spectrum, row, column block c) is scalar arithmetic.  With plain pointers the compiler folded the
 * column-block constants into 64-bit per-lane adds (240 of them per spectrum) and spilled.  Arrays addressed this way are < 4 GiB. */
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base)
{
	return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0xffffffff, 0x00020000);	/* raw buffer, 32-bit data format */
}
constexpr int kAuxNT = 2, kAuxSC1 = 16;		/* gfx94x / gfx950 cache-policy bits of the buffer intrinsics: nt, sc1 */
template <int AUX>
static __device__ __forceinline__ void bst_v2f(v2f v, __amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff)
{
	__builtin_amdgcn_raw_buffer_store_b64(u2v{ __float_as_uint(v.x), __float_as_uint(v.y) }, rs, voff, soff, AUX);
}
template <int AUX>
static __device__ __forceinline__ v2f bld_v2f(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff)
{
	const u2v u = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, AUX);
	return v2f{ __uint_as_float(u.x), __uint_as_float(u.y) };
}

/* IQ formats (K1Params::iq_format, FOSPHOR_AMD_IQ_*).  The format is a compile-time property of an FFT kernel: each kernel of k1*.inc is a
 * template whose first parameter IQ is one of the tags below, and reads K1Params::iq as `const IQ::elem *`.  A tag holds what differs
 * between the formats and nothing else -- the type of a sample in memory and the loads that turn samples into v2f; behind the loads the
 * kernels are one text.  The tag is part of an entry point's name: k1_fft_bin<iq_fp32, ...>, k1_fft_bin<iq_sc16, ...>.
 * An sc16 sample (re in the low, im in the high half of a dword) is widened where it is loaded: (float)(short) v * 2^-15 is exact
 * (int16 -> float is exact, and a power-of-two scale of a value >= 2^-15 in magnitude stays normal), so everything behind the load
 * computes on the very floats an fp32 instance fed those values would -- no conversion pass, no fp32 copy in memory. */
constexpr int kIqFp32 = 0, kIqFp16 = 1, kIqSc16 = 2;
static __device__ __forceinline__ v2f widen_sc16(uint32_t v)
{
	return v2f{ (float)(short)(v & 0xffffu) * 0x1p-15f, (float)(short)(v >> 16) * 0x1p-15f };
}
/* Members of a tag:
 *   elem         a sample in memory
 *   ld_sample    one sample, non-temporal (read-once)
 *   load_iq16    the 1024-point kernel's 16 samples of a lane: `src` points at this lane's pair, elements (2L, 2L+1) + 128k land in
 *                x[2k], x[2k+1]
 *   load_iq8     the two-wave kernel's 8 samples of a thread: elements i + 128 j
 *   raw, ld_iq, request, mov, widen
 *                the 8192-point kernel: what it holds of a sample between the request and the first pass (one register per dword of
 *                elem), the request of row j of a window (element th + 512 j: `voff` = sizeof(elem) * th), the same request written by
 *                hand and the hand-written move of the overlap reuse (why by hand: k1w_fft_bin.inc), and raw -> v2f
 * The 65536-point kernel stages one-dword formats in LDS and takes them out with widen(); iq_fp16 exists for it alone. */
struct iq_fp32 {
	typedef float2 elem;
	static __device__ __forceinline__ v2f ld_sample(const elem *src) { return __builtin_nontemporal_load(reinterpret_cast<const v2f *>(src)); }
	/* 8 x (64 lanes x 16 B) = 1 KiB per instruction.  (Ablation on MI355X: with 8-byte-per-lane loads the load path alone caps K1
	 * near 4.7 TB/s; 16-byte ones do not.) */
	static __device__ __forceinline__ void load_iq16(v2f (&x)[16], const elem *__restrict__ src)
	{
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const v4f q = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(src + 128 * k));
			x[2 * k]     = v2f{ q.x, q.y };
			x[2 * k + 1] = v2f{ q.z, q.w };
		}
	}
	static __device__ __forceinline__ void load_iq8(v2f (&x)[8], const elem *__restrict__ src)
	{
#pragma unroll
		for (int j = 0; j < 8; j++)
			x[j] = __builtin_nontemporal_load(reinterpret_cast<const v2f *>(src + 128 * j));
	}
	typedef v2f raw;
	static __device__ __forceinline__ raw ld_iq(__amdgpu_buffer_rsrc_t rs, uint32_t voff, int j) { return bld_v2f<kAuxNT>(rs, voff, 4096u * (uint32_t)j); }
	static __device__ __forceinline__ void request(raw &d, uint32_t voff, __amdgpu_buffer_rsrc_t rs, int j)
	{
		asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen nt" : "=v"(d) : "v"(voff), "s"(rs), "s"(4096u * (uint32_t)j));
	}
	static __device__ __forceinline__ void mov(raw &d, const raw &s) { asm volatile("v_mov_b64 %0, %1" : "=v"(d) : "v"(s)); }
	static __device__ __forceinline__ v2f widen(raw q) { return q; }
};
struct iq_sc16 {
	typedef uint32_t elem;
	static __device__ __forceinline__ v2f ld_sample(const elem *src) { return widen_sc16(__builtin_nontemporal_load(src)); }
	/* the same lane-to-sample map at half the bytes, 8 x (64 lanes x 8 B): `src` 8-byte aligned (even hop, 8-byte aligned base) */
	static __device__ __forceinline__ void load_iq16(v2f (&x)[16], const elem *__restrict__ src)
	{
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const u2v q = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(src + 128 * k));
			x[2 * k]     = widen_sc16(q.x);
			x[2 * k + 1] = widen_sc16(q.y);
		}
	}
	static __device__ __forceinline__ void load_iq8(v2f (&x)[8], const elem *__restrict__ src)
	{
#pragma unroll
		for (int j = 0; j < 8; j++)
			x[j] = ld_sample(src + 128 * j);
	}
	/* one dword per sample and request -- the same number of requests as fp32's dwordx2 (the 8192-point kernel's counted wait is the
	 * same); the raw dwords are what is held and moved down for the overlap reuse (16 registers fewer), widened where x is formed */
	typedef uint32_t raw;
	static __device__ __forceinline__ raw ld_iq(__amdgpu_buffer_rsrc_t rs, uint32_t voff, int j) { return __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 2048u * (uint32_t)j, kAuxNT); }
	static __device__ __forceinline__ void request(raw &d, uint32_t voff, __amdgpu_buffer_rsrc_t rs, int j)
	{
		asm volatile("buffer_load_dword %0, %1, %2, %3 offen nt" : "=v"(d) : "v"(voff), "s"(rs), "s"(2048u * (uint32_t)j));
	}
	static __device__ __forceinline__ void mov(raw &d, const raw &s) { asm volatile("v_mov_b32 %0, %1" : "=v"(d) : "v"(s)); }
	static __device__ __forceinline__ v2f widen(raw q) { return widen_sc16(q); }
};
struct iq_fp16 {
	typedef uint32_t elem;
	static __device__ __forceinline__ v2f widen(uint32_t q)
	{
		typedef _Float16 h2 __attribute__((ext_vector_type(2)));
		const h2 h = __builtin_bit_cast(h2, q);
		return v2f{ (float)h.x, (float)h.y };		/* v_cvt_f32_f16: exact */
	}
};
#define K1_LANE_SRC(lane) (2 * (lane))

#include "k1_fft_bin.inc"

/* ------------------------------------------------------------------------ */
/* K1's memory traffic without K1's arithmetic (measurement hook)             */
/* ------------------------------------------------------------------------ */
/* The same persistent grid, tile order, 16-byte non-temporal loads one spectrum ahead, and the same
 * stores (bin dwords every 4 spectra, tile partials every tile) as k1_fft_bin -- and nothing else.
 * Its duration is the practical floor the memory system sets for K1 on this chip: bench.py reports
 * K1's duration next to it (roofline.traffic_twin). */
__global__ __launch_bounds__(256, kK1WavesPerSimd)
void k1_traffic_twin(const K1Params p)
{
	const int lane   = threadIdx.x & 63;
	const int wv     = threadIdx.x >> 6;
	const int ntiles = p.total / p.tile;
	const int stride = gridDim.x * 4;
	int tile = blockIdx.x * 4 + wv;
	if (tile >= ntiles)
		return;
	v2f xn[16];
	iq_fp32::load_iq16(xn, p.iq + (size_t)tile * p.tile * p.hop + K1_LANE_SRC(lane));
	for (; tile < ntiles; tile += stride) {
		const int t0 = tile * p.tile;
		v2f acc = { 0.0f, 0.0f };
		for (int g0 = 0; g0 < p.tile; g0 += 4) {
#pragma unroll 1
			for (int u = 0; u < 4; u++) {
				const int t = t0 + g0 + u;
				v2f x[16];
#pragma unroll
				for (int m = 0; m < 16; m++)
					x[m] = xn[m];
				const bool last = (g0 + u + 1 == p.tile);
				const int t_next = last ? (tile + stride) * p.tile : t + 1;
				if (!last || tile + stride < ntiles)
					iq_fp32::load_iq16(xn, p.iq + (size_t)t_next * p.hop + K1_LANE_SRC(lane));
#pragma unroll
				for (int m = 0; m < 16; m++)
					acc += x[m];			/* consume the data: 16 adds per spectrum */
			}
			uint32_t *dst = p.bins + (size_t)((t0 + g0) >> 2) * kN + lane;
#pragma unroll
			for (int m = 0; m < 16; m++)
				dst[64 * m] = __float_as_uint(acc.x) + (uint32_t)m;
		}
		float2 *pp = p.partial + (size_t)tile * kN + lane;
#pragma unroll
		for (int m = 0; m < 16; m++)
			pp[64 * m] = make_float2(acc.x, acc.y + (float)m);
	}
}

hipError_t launch_k1_traffic_twin(const K1Params &p, hipStream_t s)
{
	const int tiles = p.total / p.tile;
	int blocks = (tiles + 3) / 4;
	if (blocks > kK1MaxBlocks)
		blocks = kK1MaxBlocks;
	hipLaunchKernelGGL(k1_traffic_twin, dim3(blocks), dim3(256), 0, s, p);
	return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* K1 v2: two waves per spectrum                                             */
/* ------------------------------------------------------------------------ */
/* Same arithmetic, same LDS layout, same outputs as k1_fft_bin, but a spectrum is shared by
 * the two waves of a 128-thread work-group exactly like the reference's 128 work-items
 * (fft.cl:403: WG_SIZE = N/8): lane l of wave w IS virtual work-item i = l + 64w and owns 8
 * points.  Every per-lane array halves (x, prefetch, l2, live/max, pack), which fits
 * 4 waves per SIMD without spills; the price is one 2-wave s_barrier per exchange.
 * After pass 3 wave w takes the pass-4 butterflies c in [4w, 4w+4), i.e. columns
 * lane + 64m for m in {4w..4w+3} U {8+4w..8+4w+3}. */
constexpr int kK1v2WavesPerSimd = 3;		/* __launch_bounds__ second argument (measured) */

#include "k1v2_fft_bin.inc"

/* ------------------------------------------------------------------------ */
/* K1 general N: N/8 threads per spectrum                                    */
/* ------------------------------------------------------------------------ */
/* The reference's plan for any N = 8^k * 2 (fft.cl:397-466 is the N = 1024 instance): k radix-8
 * Stockham passes with p = 1, 8, 64, ... and a final radix-2 pass with p = N/2, N/8 work-items
 * of 8 points each.  One work-group of N/8 threads per spectrum, the N-point exchange slab, the twiddles and
 * the window in dynamic LDS.  Instantiated for N = 1024 with 16-bit bin indices (more than 256 bins): a parity
 * case, not a tuned one (N = 8192 has its own kernel and plan, k1w_fft_bin).
 * Same swizzle phys(e) = e ^ ((e >> 3) & 15): the store patterns of every pass and the
 * lane-contiguous reads stay bank-conflict free for any N (the argument of DESIGN_HISTORY.md only
 * involves address bits 0..6).  Bin indices are 16-bit, 2 spectra per dword. */
static __device__ __forceinline__ int swz(int e) { return e ^ ((e >> 3) & 15); }

#include "k1big_fft_bin.inc"

/* X[jj] of a radix-16 pass sits in r[bitrev4(jj)] */
#define R16_PERM(jj) ((((jj) & 1) << 3) | (((jj) & 2) << 1) | (((jj) & 4) >> 1) | (((jj) & 8) >> 3))

/* ------------------------------------------------------------------------ */
/* K1 for N = 8192: 512 threads per spectrum, 16 points per thread            */
/* ------------------------------------------------------------------------ */
/* The oracle's plan at this length (oracle/fosphor_oracle.c: o_pass_radix16_fma x 3 + o_pass_radix2_fma; no reference behaviour
 * exists beyond N = 1024): Stockham radix-16 passes p = 1, 16, 256 over 512 work-items of 16 points -- ONE item per thread in every
 * pass -- and the radix-2 pass p = 4096 of fft.cl:428-458.  Round 5 measured that this kernel's LDS is as busy as its VALUs (three
 * exchanges of 64 KiB each way per spectrum = 2.2 us per CU next to 2.0 us of VALU issue, and the two add up: profiles/r05_lds.md);
 * against the radix 8.8.8.8.2 form it replaced this plan moves TWO AND A HALF exchanges through the LDS:
 *   - exchanges 1 and 2 (behind the passes p = 1 and p = 16) are full: 16 stores, one barrier, 16 loads per thread (two 64 KiB slabs
 *     used alternately: the barrier behind the stores of an exchange also proves that every thread has finished the loads of the
 *     exchange before the previous one, i.e. of the slab written next);
 *   - behind the pass p = 256 item i = k + 256 h holds X3[4096 h + k + 256 m], m < 16, and the radix-2 butterflies pair (jb, jb + 4096):
 *     thread (h, k) keeps its eight outputs m in [8 h, 8 h + 8), hands the other eight to thread (1 - h, k) through the LDS and does the
 *     butterflies jb = k + 256 m of its half: 8 stores + 8 loads per thread.  Its columns are k + 2048 h + 256 c + 4096 v, c < 8, v < 2;
 *   - LDS swizzle phys(e) = e ^ ((e >> 4) & 31) (8-byte elements): the three store patterns (16 i + m; 256 (i >> 4) + (i & 15) + 16 m;
 *     4096 h + k + 256 m) put the 16 lanes of a ds_write_b64 group into 16 different bank pairs, the lane-contiguous loads e = i + 512 j
 *     the 32 lanes of a ds_read_b64 group into 32; each store is `per-thread constant ^ compile-time constant`, each load an immediate;
 *   - everything a thread needs from the tables is fixed per thread and sits in registers: 16 window taps (as the 8 pairs of the first
 *     pass's stage-A butterflies), 2 x 8 twiddles of the passes p = 16, 256, the 8 of its radix-2 butterflies;
 *   - the overlap of overlap_cc (overlap_cc_impl.cc:64-79) lives in REGISTERS: a thread holds the raw IQ of elements th + 512 j, j < 16;
 *     the next window of a tile starts hop = N / R samples later, i.e. 16 / R rows of 512 -- its row j is this window's row j + 16 / R
 *     of the same thread.  With R = 2 (BASELINE C3) a spectrum costs eight 8-byte loads per thread: every sample of the stream is fetched
 *     once.  Any hop works (8-byte loads need no 16-byte alignment): odd hops reload all sixteen rows.
 * One work-group (8 waves, <= 256 registers) per CU.  16-bit bin indices, 2 spectra per dword. */
/* Work-group barrier for exchanges through LDS only: waits for this wave's LDS operations, not for its outstanding
 * global loads and stores (__syncthreads() also drains vmcnt, which would park every wave of the work-group behind the
 * IQ requested for the NEXT spectrum).  Nothing is handed from thread to thread through global memory in these kernels. */
static __device__ __forceinline__ void wg_barrier_lds()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

/* K1W_TIMING=1 (timing builds only, tools/k1w_phase_timing.py): s_memtime stamps per phase of the 8192-point kernel's loop, accumulated per
 * wave (waves 0 and 4 of a work-group: the early and the late one of a SIMD) into K1Params::dbg[(work-group * 2 + slot) * 16 + phase].
 * Reading the clock waits for the wave's LDS operations (s_memtime answers on lgkmcnt). */
#ifndef K1W_TIMING
#define K1W_TIMING 0
#endif
#if K1W_TIMING
#define K1W_STAMP(i) do { const uint32_t _now = (uint32_t)__builtin_readcyclecounter(); wacc[i] += _now - wprev; wprev = _now; } while (0)
#else
#define K1W_STAMP(i) do { } while (0)
#endif

constexpr int kK1wIdxStores = 16;	/* index stores a thread issues per ODD spectrum (one dword per column and pair of spectra): the immediate of the
					 * hand-written wait for the IQ requested before them */
#include "k1w_fft_bin.inc"

/* ------------------------------------------------------------------------ */
/* K1 for N = 65536: radix-16 plan, two stages, the intermediate in the XCD's L2 */
/* ------------------------------------------------------------------------ */
/* No reference behaviour exists at N = 65536 (fft.cl has one length, 1024): the plan is this build's own and the oracle
 * restates it (oracle/fosphor_oracle.c, o_pass_radix16_fma): four Stockham radix-16 passes, p = 1, 16, 256, 4096,
 * 4096 virtual work-items of 16 points, a pass = four radix-2 stages with the twiddles on the butterflies (bf(), above).  512 KiB per
 * spectrum does not fit one CU's LDS, but the data flow factors into two 256-point levels:
 *
 *   stage A  passes 1-2 only mix inputs whose index is congruent mod 256: for each residue q they ARE the two passes of a
 *            256-point transform on x[q + 256 m], m < 256, and leave its 256 results at w[256 q + kk], kk < 256.
 *            SIXTEEN LANES do one such transform (16 points each, one 16 x 16 transpose through LDS in between), so a
 *            wavefront does four residues ON ITS OWN: no work-group barrier anywhere in stage A.
 *   stage B  passes 3-4 only mix elements with the same offset kk: for each kk a 256-point transform over w[256 q + kk],
 *            q < 256, whose outputs are columns kk + 256 jj3 + 4096 jj4.  A work-group takes 32 adjacent offsets with
 *            thread = (offset, item): every global access of the stage -- the intermediate coming in, rows, bin indices
 *            and partials going out -- is a run of 32 consecutive columns (128 / 256 B), and the one exchange between its
 *            two passes goes through a work-group-wide LDS array behind ONE barrier.
 *
 * A CLUSTER of 8 work-groups on ONE XCD takes a spectrum through both stages (member m: residues [32 m, 32 m + 32) in stage A,
 * offsets [32 m, 32 m + 32) in stage B); between the stages the spectrum makes one round trip through the XCD's L2 (plain
 * stores + s_waitcnt vmcnt(0) + relaxed agent-scope atomics: the L2 is the coherence point of its CUs), laid out
 * [offset / 32][residue][offset % 32] so that both sides move whole 128-byte runs.  Clusters form from XCC_ID tickets and
 * claim tiles dynamically (progress never depends on a work-group that is not resident); every wait on another work-group
 * is bounded and ends in an error word the host turns into -EIO.
 *
 * Against the radix-8 form this replaces (8.8.8 | 8.8.2, 1024 threads of 8 points, eight work-group barriers per spectrum):
 * 512 threads of 16 points, ONE work-group barrier per spectrum besides the cluster hand-off, twiddles of a thread fixed
 * for its lifetime (registers / two small LDS tables), ~40 % fewer instructions per sample.
 *
 * Bin indices: 512 bins need 9 bits.  The low 8 bits go out like the 1024-point path's (one dword = 4 consecutive spectra of
 * a column), the 9th as one bit per spectrum in a dword per (tile, column): 1.125 B per sample instead of 2.
 *
 * THE LOOP IS SKEWED (DESIGN.md sections 4-5; DESIGN_HISTORY.md section 8, "C5, round 4", has the measurement behind every choice).  A spectrum's blocks make a round
 * trip store -> L2 -> cluster barrier -> load; with the loop in program order all eight waves of a CU sat through it (132 of 326 us).
 * Instead the same threads run stage A of spectrum u + 1 meanwhile: its first pass between the stores of spectrum u and their
 * s_waitcnt vmcnt(0), its wave-internal transpose and pass-2 twiddle products between the arrival at the cluster barrier and
 * everybody else's, its pass-2 butterflies beside the loads of the intermediate.  What the in-order return of a wave's loads
 * dictates around it:
 *   - the fp16 IQ of spectrum u + 3 is requested (LDS-DMA, two 32 KiB buffers) only once the loads of the intermediate have been
 *     used: a request to HBM ahead of them would delay them;
 *   - that LDS-DMA is issued by hand (inline asm): the compiler parks every barrier and LDS read that follows an LDS-DMA it knows
 *     about behind s_waitcnt vmcnt(0); the reads of the buffer sit behind an explicit vmcnt(0) of the requesting wave + a barrier;
 *   - work-group barriers are s_waitcnt lgkmcnt(0) + s_barrier (wg_barrier_lds): __syncthreads() would drain vmcnt;
 *   - a poll of a cluster counter through the vector path is a load too (it returns behind whatever its wave has in flight): the "has
 *     everybody read the intermediate" question therefore goes through the SCALAR path, every wave for itself (round 6; until
 *     round 5 the last wave, which requested no IQ, asked ahead of its epilogue's stores and a barrier passed the answer on);
 *   - the exact path's threshold table sits in LDS (ds_read has its own counter). */

/* Loads return IN ORDER and the first stage of a radix-16 pass pairs inputs j and j + 8: requested in this order, a butterfly's two inputs
 * arrive together (requested 0..15, the first butterfly waited for nine loads). */
#define K1H_PAIR(i) ((((i) & 1) << 3) | ((i) >> 1))
/* K1H_TIMING=1 (timing builds only, tools/k1h_phase_timing.py): s_memtime stamps per phase of the 65536-point kernel's loop, accumulated per
 * wave (waves 0, 3 and 7 of a work-group) into K1Params::dbg[(work-group * 3 + slot) * 16 + phase]. */
#ifndef K1H_TIMING
#define K1H_TIMING 0
#endif
/* Round 6: the "has every member read the intermediate" question is asked by EVERY wave for itself, through the SCALAR data
 * path (s_dcache_inv + s_load_dword: its answer does not queue behind the wave's vector stores -- another counter, another path), right before the
 * wave's stores of the next spectrum: by then the answer has long been yes.  Before, the last wave asked ahead of its epilogue (a vector
 * load behind the epilogue's stores would have waited for them), saw the spread between the cluster's members (~1 900 cycles per spectrum,
 * K1H_TIMING builds) and everybody else sat at a work-group barrier for the answer.  That barrier goes with it: nothing else needs it
 * (the exchange array's readers are separated from its next writers by the barrier behind the stores). */
/* Round 6: the YOUNGER wave of each SIMD (waves 4-7 of the work-group) issues at a higher priority than the older one.  Left to the
 * arbiter's age order the older wave of a SIMD won every tie and the younger ones reached each of the four barriers ~2 000 cycles late
 * (K1H_TIMING builds); with the priority the other way round the halves of the work-group take turns at being early -- the early wave's stores
 * and first pass run beside the late wave's epilogue -- and the kernel alone went from 231 to 216 us (profiles/r06_c5.md: the mirror image,
 * priority to the OLDER half, changes nothing; levels 1 / 2 / 3 measure the same). */
static __device__ __forceinline__ uint32_t sload_fresh(const uint32_t *p)
{
	uint32_t v;
	/* (NOT `s_load_dword ... glc`: tools/ubench/poll_latency.hip measured 16 200 ticks per look for it on gfx950, against 217 for an
	 * invalidate of the scalar cache followed by a plain scalar load and 253 for a vector load with sc1) */
	asm volatile("s_dcache_inv\n\ts_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
	return v;
}
#if K1H_TIMING
#define K1H_STAMP(i) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
		const long long _now = __builtin_readcyclecounter(); hacc[i] += _now - hprev; hprev = _now; } while (0)
#else
#define K1H_STAMP(i) do { } while (0)
#endif

constexpr int kXaWave = 4 * 272;		/* stage-A exchange, elements per wave: [residue 4][jj 16][a 16], rows padded to 17 */
constexpr int kThrMax  = 520;			/* exact-bin thresholds kept in LDS (n_bins + 1 <= 513 doubles) */
constexpr int kTwRow = 9;			/* LDS twiddle tables: 8 twiddles per row, rows padded to 9 entries (72 B: 16 / 32 rows fall into different banks) */
/* The work-group's size decides the cluster's: a work-group of NWV waves takes 4 NWV residues (stage A) / offsets (stage B) of a spectrum,
 * so 64 / NWV work-groups make a cluster.  NWV = 8 is what runs: one work-group per CU, clusters of 8.  NWV = 4 -- TWO work-groups per CU,
 * members of different clusters of 16, so that one's arithmetic could run beside the other's LDS / memory phases -- was built in round 6,
 * parity-green, and 45-85 % SLOWER (450 against 245 us per frame: twice the members to wait for at each of a spectrum's two hand-overs,
 * and the hand-overs are what the loop's time is made of; profiles/r06_c5.md).  The geometry stays parametrised; only NWV = 8 is instantiated. */
template <int NWV> struct K1hGeom {
	static constexpr int kMem   = 64 / NWV;		/* members of a cluster */
	static constexpr int kRpm   = 4 * NWV;		/* residues = offsets per member */
	static constexpr int kXbLen = kRpm * 257;	/* stage-B exchange: [offset][jj3 16][a3 16], offsets padded to 257 */
	static constexpr int kXLen  = NWV * kXaWave > kXbLen ? NWV * kXaWave : kXbLen;	/* the two exchanges share one region (a barrier separates their uses) */
	static constexpr int kInLen = 256 * kRpm;	/* staged fp16 input of one spectrum: [row m 256][residue] dwords, 16-byte pieces permuted inside a row */
	static constexpr size_t kLds = ((size_t)kXLen + 16 * kTwRow + kRpm * kTwRow) * sizeof(float2) + (size_t)2 * kInLen * sizeof(uint32_t) + (size_t)kThrMax * sizeof(double);
						/* (exchange, two twiddle tables, staged input, thresholds) */
};

#include "k1h_fused.inc"

typedef void (*k1_fn)(const K1Params);

/* The dynamic-LDS limit of the n kernels of `fns`, raised to `lds` bytes once per device: the attribute belongs to the function object of
 * the CURRENT device.  `done` holds a bit per device that has it (atomic: host threads may drive different devices at once; two threads
 * on one device may both set it, which is harmless). */
static hipError_t set_lds_once(const k1_fn *fns, int n, int lds, std::atomic<unsigned long long> &done)
{
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
		return hipErrorInvalidDevice;
	if (done.load() >> dev & 1)
		return hipSuccess;
	for (int i = 0; i < n; i++) {
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fns[i]), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
		if (e != hipSuccess)
			return e;
	}
	done.fetch_or(1ull << dev);
	return hipSuccess;
}

template <typename IQ, int NWV>
static hipError_t launch_k1h_form(const K1Params &p0, hipStream_t s)
{
	static const k1_fn fn[2] = { k1h_fused<IQ, false, NWV>, k1h_fused<IQ, true, NWV> };
	constexpr size_t lds = K1hGeom<NWV>::kLds;
	static std::atomic<unsigned long long> attr_dev{0};
	const hipError_t ae = set_lds_once(fn, 2, (int)lds, attr_dev);
	if (ae != hipSuccess)
		return ae;
	/* (the counters in p0.sync are zero: cleared at allocation, and by the last work-group of every launch) */
	/* 32 clusters: 8 work-groups of 8 waves, one per CU -- or 16 work-groups of 4 waves, two per CU */
	hipLaunchKernelGGL(fn[p0.fft_out ? 1 : 0], dim3(256 * 8 / NWV), dim3(64 * NWV), lds, s, p0);
	return hipGetLastError();
}

static hipError_t launch_k1h(const K1Params &p0, hipStream_t s)
{
	/* tiles of 4 .. 32 spectra (whole quads of low bytes, the 9th bits of a tile in one dword); tile index: 20 bits of the claim word */
	if (!p0.sync || !p0.scratch || p0.tile < 4 || p0.tile > 32 || (p0.tile & 3) || p0.total % p0.tile || p0.total / p0.tile >= (1 << 20))
		return hipErrorInvalidValue;
	return p0.iq_format == kIqSc16 ? launch_k1h_form<iq_sc16, 8>(p0, s)
	     : p0.iq_format == kIqFp16 ? launch_k1h_form<iq_fp16, 8>(p0, s) : launch_k1h_form<iq_fp32, 8>(p0, s);
}

/* Spectra per K1 wave (N = 1024) / per work-group pass (other lengths).  One tile = one row of live / max
 * partials (8 B per column), so longer tiles mean fewer intermediate bytes: 64 spectra per wave is 0.125 B per
 * sample written and read back, 16 was 0.5.  A tile never straddles a batch (K2 weights whole tiles). */
static int k1_tile(const K1Shape &s)
{
	const int v = s.tile_knob, total = s.total, batch = s.batch;
	const bool bins16 = s.n_bins > 256 || s.log2n != 10;
	if (v >= (s.log2n == 13 ? 8 : 4) && v <= (s.log2n == 16 ? 32 : 128) && !(v & (v - 1)) && batch % v == 0 && total % v == 0)
		return v;
	if (s.log2n == 16) {
		/* a cluster owns whole tiles: the largest tile that still gives each of the 32 clusters one (at most 32 spectra: the
		 * 9th bits of a tile's bin indices share one dword per column) */
		for (int t = 32; t >= 8; t >>= 1)
			if (batch % t == 0 && total / t >= 32)
				return t;
		return 4;
	}
	if (s.log2n == 13) {
		/* one work-group per CU walks whole tiles; inside a tile the overlapped half of a window is reused from registers,
		 * so long tiles fetch less (tile 64 at 50 % overlap: 65 half-windows for 64 spectra) and leave fewer partial rows;
		 * every CU gets a tile (measured, 16384 spectra per launch: tile 16 / 32 / 64 -> 279 / 288 / 289 GSamples/s) */
		for (int t = 64; t >= 8; t >>= 1)
			if (batch % t == 0 && total / t >= 256)
				return t;
		return 8;		/* (at least 8: the 9th bits of a tile's bin indices go out as one byte per column and eight spectra) */
	}
	if (s.log2n != 10 || bins16) {
		/* largest tile that still gives every resident wave (256 CUs x 8) a tile */
		if (total / 16 >= 2048) return 16;
		if (total / 8 >= 2048) return 8;
		return 4;
	}
	/* 1024 waves (one 4-wave work-group per CU) per launch: consecutive launches overlap on alternating
	 * streams, so two of them fill the chip's 512 work-group slots */
	for (int t = 64; t >= 8; t >>= 1)
		if (batch % t == 0 && total / t >= 1024)
			return t;
	return 4;
}

/* `units` persistent units walk `tiles` tiles, unit u taking u, u + units, ... */
static void k1_walk(K1Plan *pl, int cap)
{
	pl->units = pl->tiles < cap ? pl->tiles : cap;
	pl->max_tiles = pl->units > 0 ? (pl->tiles + pl->units - 1) / pl->units : 0;
	pl->min_tiles = pl->units > 0 ? pl->tiles / pl->units : 0;
}

K1Plan k1_plan(const K1Shape &s)
{
	K1Plan pl;
	const bool bins16 = s.n_bins > 256 || s.log2n != 10;
	pl.tile = s.tile > 0 ? s.tile : k1_tile(s);
	pl.tiles = s.total / pl.tile;
	if (s.log2n == 16) {
		/* 32 clusters: 8 work-groups of 8 waves, one per CU; a cluster claims its next tile when it is done with the last */
		pl.kernel = K1_FUSED;
		pl.grid = 256;
		pl.units = 32;
		pl.max_tiles = pl.min_tiles = 0;
		return pl;
	}
	if (bins16 && s.log2n == 10) {
		/* N = 1024 with 16-bit bin indices (more than 256 bins): the general kernel at 128 threads per spectrum */
		pl.kernel = K1_BIG;
		k1_walk(&pl, 4096);
		pl.grid = pl.units;
		return pl;
	}
	if (bins16) {
		/* one 8-wave work-group per CU -- or per CU of the share the host leaves to this kernel (K1Params.cus: the count and
		 * merge kernels of the previous launch run on the rest) */
		const int all_cus = s.n_cus > 0 ? s.n_cus : 256;
		pl.kernel = K1_WIDE;
		k1_walk(&pl, (s.share > 0 && s.share < all_cus && pl.tiles % s.share == 0) ? s.share : all_cus);
		pl.grid = pl.units;
		return pl;
	}
	/* 16-byte IQ loads of the wave-per-spectrum kernel need an even hop, its 8-byte sc16 loads an 8-byte aligned start (the
	 * two-wave kernel loads one 4-byte sample per lane) */
	if (s.k1_knob == 2 || (s.hop & 1) || (s.iq_format == kIqSc16 && (s.align & 7))) {
		pl.kernel = K1_V2;
		k1_walk(&pl, 256 * 2 * kK1v2WavesPerSimd);	/* resident 2-wave work-groups on 256 CUs */
		pl.grid = pl.units;
		return pl;
	}
	/* FOSPHOR_AMD_K1_BLOCKS: debugging aid (e.g. 256 = one wave per SIMD, for phase timing) */
	static const int max_blocks = [] { const char *e = getenv("FOSPHOR_AMD_K1_BLOCKS"); const int v = e ? atoi(e) : 0;
	                                   return (v > 0 && v < kK1MaxBlocks) ? v : kK1MaxBlocks; }();
	pl.kernel = K1_WAVE;
	pl.grid = (pl.tiles + 3) / 4;
	if (pl.grid > max_blocks)
		pl.grid = max_blocks;		/* persistent: 2 work-groups per CU */
	k1_walk(&pl, 4 * pl.grid);		/* (the waves of the grid; a wave without a tile leaves at once) */
	return pl;
}

/* ... of the launch that p describes */
static K1Plan k1_plan(const K1Params &p)
{
	K1Shape s = {};
	s.log2n = p.log2n; s.n_bins = p.n_bins; s.iq_format = p.iq_format; s.hop = p.hop;
	s.align = (int)((uintptr_t)p.iq & 15);
	s.k1_knob = p.variant == 2 ? 2 : 1;
	s.n_cus = p.n_cus; s.share = p.cus;
	s.total = p.total; s.batch = p.total; s.tile = p.tile;
	return k1_plan(s);
}

/* The 1024- and 8192-point kernels of one format; each kernel's options are chosen here, once */
template <typename IQ>
static hipError_t launch_k1_as(const K1Params &p, hipStream_t s)
{
	const K1Plan pl = k1_plan(p);
	if (k1_variant_of(pl.kernel) != p.variant)
		return hipErrorInvalidValue;		/* (fill_k1 takes the variant from the same plan) */
	if (p.variant == 3) {
		if (p.log2n == 10) {
			/* N = 1024 with 16-bit bin indices (more than 256 bins): the general kernel at 128 threads per spectrum */
			constexpr int N = 1024;
			constexpr int lds = (N + ((N / 2 - 8) / 7) * 7 + N / 2) * 8 + N * 4;		/* exchange slab + the reference's twiddles + window */
			hipLaunchKernelGGL((p.fft_out ? k1big_fft_bin<IQ, 10, true> : k1big_fft_bin<IQ, 10, false>), dim3(pl.grid), dim3(N / 8), lds, s, p);
			return hipGetLastError();
		}
		if (p.log2n != 13 || (p.tile & 7) || (p.total & 7))	/* (the kernel packs the 9th bits of spectra 8 u .. 8 u + 7 of a tile into one byte per column) */
			return hipErrorInvalidValue;
		/* N = 8192: 16 points per thread, tables in registers, overlap reuse in registers (k1w_fft_bin); any hop */
		constexpr int ldsw = 2 * 8192 * 8 + 520 * 8;	/* two slabs + the exact-bin thresholds */
		static const k1_fn fns[5] = { k1w_fft_bin<IQ, 8>, k1w_fft_bin<IQ, 4>, k1w_fft_bin<IQ, 2>, k1w_fft_bin<IQ, 1>, k1w_fft_bin<IQ, 16> };
		static std::atomic<unsigned long long> attr_dev{0};
		const hipError_t ae = set_lds_once(fns, 5, ldsw, attr_dev);
		if (ae != hipSuccess)
			return ae;
		/* rows of 512 samples the next window of a tile shares with this one: hop = 8192 / R, R = 2, 4, 8, 16; any other hop: none */
		const int which = (p.hop == 4096) ? 0 : (p.hop == 2048) ? 1 : (p.hop == 1024) ? 2 : (p.hop == 512) ? 3 : 4;
		hipLaunchKernelGGL(fns[which], dim3(pl.grid), dim3(512), ldsw, s, p);
		return hipGetLastError();
	}
	if (p.variant == 2) {
		hipLaunchKernelGGL((p.fft_out ? k1v2_fft_bin<IQ, true> : k1v2_fft_bin<IQ, false>), dim3(pl.grid), dim3(128), 0, s, p);
		return hipGetLastError();
	}
	hipLaunchKernelGGL((p.fft_out ? k1_fft_bin<IQ, true, false> : p.n_bins == 256 ? k1_fft_bin<IQ, false, true> : k1_fft_bin<IQ, false, false>),
	                   dim3(pl.grid), dim3(256), 0, s, p);
	return hipGetLastError();
}

hipError_t launch_k1(const K1Params &p, hipStream_t s)
{
	if (p.variant == 4)
		return launch_k1h(p, s);
	if (p.iq_format == kIqFp32)
		return launch_k1_as<iq_fp32>(p, s);
	if (p.iq_format == kIqSc16)
		return launch_k1_as<iq_sc16>(p, s);
	return hipErrorInvalidValue;		/* (fp16: the 65536-point kernel only) */
}

/* Test hook: the K1 epilogue alone on FFT values read from memory */
__global__ __launch_bounds__(256)
void k_bin_hook(const float2 *__restrict__ fft, uint8_t *__restrict__ bin, float *__restrict__ pwr, int n,
                const K1Params p, int force_exact)
{
	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float top = (float)(bk.nb - 1);
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		float2 v = fft[i];
		float l2; uint32_t ab;
		const float r = bin_fast(v.x, v.y, bk, &l2, &ab);
		/* the two ways the K1 variants turn the guess into an index: saturating byte convert
		 * (<= 256 bins) or clamp + integer convert (16-bit indices) */
		uint32_t b = p.bins16 ? (uint32_t)(int)__builtin_amdgcn_fmed3f(r, 0.0f, top) : (pack_bin(r, top, 0, 0) & 0xff);
		if (ab > __float_as_uint(bk.amb) || force_exact)
			b = bin_exact(v.x, v.y, l2, (int)__builtin_amdgcn_fmed3f(r, 0.0f, top), ThrScalar{ bk.thr }, bk.nb, &l2);
		if (p.bins16)
			reinterpret_cast<uint16_t *>(bin)[i] = (uint16_t)b;
		else
			bin[i] = (uint8_t)b;
		pwr[i] = l2 * F_HALF_LOG10_2;
	}
}

hipError_t launch_bin_hook(const float2 *fft, uint8_t *bin, float *pwr, int n,
                           const K1Params &p, int force_exact, hipStream_t s)
{
	int blocks = (n + 255) / 256;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(k_bin_hook, dim3(blocks), dim3(256), 0, s, fft, bin, pwr, n, p, force_exact);
	return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* K2: hit counts per (slab of 64 columns, chunk)                            */
/* ------------------------------------------------------------------------ */

/* One lane per column: the 64 lanes of a wave count 64 different columns, so an LDS atomic
 * never meets a bank conflict between different (bin, column) cells.  Columns c and c + 32 of
 * the slab share one dword (low / high 16 bits; a chunk has <= 1024 spectra, so the low half
 * cannot carry into the high one): the two lanes that meet in a bank are serialised by the
 * hardware either way, and the histogram is half the size (32 KiB at 256 bins), which lets a
 * work-group of this kernel sit beside the two K1 work-groups of a CU.
 * (The previous layout, display.cl:96,176's [bin][16] with 4 spectra x 16 columns per wave,
 * had 4 lanes per column in every atomic instruction and kept the LDS pipe busy ~3x longer.) */
/* Independent index loads in flight per thread (IF): 8 for the per-batch chunks of the 1024-point path (45 VGPRs: still beside two K1
 * waves of 228 on a SIMD; 4 -> 8: K2 59 -> 51 us beside K1, path +1.6 %; 12 / 16 = 61 / 63 VGPRs no longer fit there), 4 where a work-group
 * counts several chunks (sharded frames: 532 against 527 GSamples/s) and for the 16-bit-index geometries (N = 8192: 4 / 8 / 16 -> 62 / 67 /
 * 72 us). */
/* NW waves per work-group: 4 where the kernel has to fit beside K1 (8-bit indices, N = 1024); 16 for the
 * 16-bit-index geometries, whose grids are small (N/64 x chunks) and whose rows are latency-bound */
/* K2_TIMING (timing builds with -DK2_TIMING, tools/k2_phase_timing.py): s_memtime stamps per phase of the count kernel, summed
 * over the work-groups' first waves into g_k2_time[] (read through fosphor_amd_debug_k2_timing) */
#ifdef K2_TIMING
__device__ unsigned long long g_k2_time[16];
#define K2_STAMP(i) do { if (tid == 0) { const long long _n = __builtin_readcyclecounter(); atomicAdd(&g_k2_time[i], (unsigned long long)(_n - k2prev)); k2prev = _n; } } while (0)
#else
#define K2_STAMP(i) do { } while (0)
#endif
/* one hit: row `bin` of the [bin][32] histogram (128 bytes per row), the lane's column at byte hc4 */
static __device__ __forceinline__ void lds_count(uint32_t *h, uint32_t bin, uint32_t hc4, uint32_t inc)
{
	atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(h) + ((bin << 7) + hc4)), inc);	/* v_lshl_add_u32 + ds_add_u32 */
}
/* v & 0xffff / v & 0xff as ONE instruction the compiler cannot merge into the shift that follows */
static __device__ __forceinline__ uint32_t lo16(uint32_t v) { uint32_t r; asm("v_and_b32 %0, 0xffff, %1" : "=v"(r) : "v"(v)); return r; }
static __device__ __forceinline__ uint32_t lo8(uint32_t v)  { uint32_t r; asm("v_and_b32 %0, 0xff, %1" : "=v"(r) : "v"(v)); return r; }

template <int NW, int IF>
__global__ __launch_bounds__(64 * NW)
void k2_count(const K2Params p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t h[];	/* [n_bins][32] packed pairs */
	__shared__ float red_s[NW][64], red_m[NW][64];

	const int tid  = threadIdx.x;
	const int lane = tid & 63;
	const int wv   = __builtin_amdgcn_readfirstlane(tid >> 6);	/* (the compiler does not know it is wave-uniform: with it in an SGPR the row
								 * addresses below are scalar arithmetic + one VGPR of lane offset; as a VGPR every
								 * load cost a v_mul_lo_u32 and a 64-bit add: 23 instead of 31 VGPRs, 2 instead of 22
								 * v_mul_lo_u32; the kernel's time did not change, it does not wait for its VALUs) */
	const int x0   = blockIdx.x * 64;
	const int c    = blockIdx.y;			/* chunk index within the launch */
	const int cpb  = p.batch / p.chunk;		/* chunks per batch */
	const int f    = c / cpb;			/* batch index */
	const int t_in = (c - f * cpb) * p.chunk;	/* first spectrum of the chunk within its batch */
	const int nb   = p.n_bins;
	const int hcol = lane & 31;
	const uint32_t inc = (lane & 32) ? 0x10000u : 1u;
#ifdef K2_TIMING
	long long k2prev = __builtin_readcyclecounter();
	if (tid == 0) atomicAdd(&g_k2_time[15], 1ull);		/* work-groups */
#endif

	__shared__ uint32_t rowbits[16];		/* n_bins <= 512 */
	{
		/* 16 bytes per instruction (n_bins is a multiple of 16: nb * 32 dwords = whole uint4s) */
		uint4 *h4 = reinterpret_cast<uint4 *>(h);
		for (int i = tid; i < nb * 8; i += 64 * NW)
			h4[i] = make_uint4(0u, 0u, 0u, 0u);
	}
	if (tid < 16)
		rowbits[tid] = 0;
	K2_STAMP(0);		/* zeroing issued */
	__syncthreads();
	K2_STAMP(1);		/* barrier */

	/* bins: one dword = 4 consecutive spectra of one column (8-bit indices), or 2 (16-bit
	 * indices, n_bins > 256 or N > 1024); a wave reads 256 contiguous bytes per row */
	/* (uniform base pointer + 32-bit lane offsets: one address register per load in flight) */
	if (p.bins9) {
		/* 9-bit indices of the 65536-point kernel: a wave takes whole tiles -- one dword of 9th bits per lane and tile, then the
		 * tile's (at most 8) dwords of low bytes, all requested before the first is used */
		const uint32_t n = p.n, qpt = (uint32_t)p.tile >> 2, ntl = (uint32_t)(p.chunk / p.tile);
		const uint32_t *lo = p.bins + (size_t)c * (p.chunk >> 2) * n + x0 + lane;
		const uint32_t *hi = p.bins + (size_t)(p.total >> 2) * n + (size_t)c * ntl * n + x0 + lane;
#pragma unroll 1
		for (uint32_t tl = wv; tl < ntl; tl += NW) {
			/* the index planes read non-temporally: they are read once, and the FFT kernel of the next frame keeps its intermediates in the same L2 */
			const uint32_t hv = __builtin_nontemporal_load(&hi[(size_t)tl * n]);
			uint32_t v[8];
#pragma unroll
			for (uint32_t u = 0; u < 8; u++)
				v[u] = (u < qpt) ? __builtin_nontemporal_load(&lo[(size_t)(tl * qpt + u) * n]) : 0u;
#pragma unroll
			for (uint32_t u = 0; u < 8; u++) {
				if (u < qpt) {			/* uniform */
					const uint32_t h4 = hv >> (4 * u);
					atomicAdd(&h[(((v[u]      ) & 0xff) | ((h4 & 1u) << 8)) * 32 + hcol], inc);
					atomicAdd(&h[(((v[u] >>  8) & 0xff) | ((h4 & 2u) << 7)) * 32 + hcol], inc);
					atomicAdd(&h[(((v[u] >> 16) & 0xff) | ((h4 & 4u) << 6)) * 32 + hcol], inc);
					atomicAdd(&h[(((v[u] >> 24)       ) | ((h4 & 8u) << 5)) * 32 + hcol], inc);
				}
			}
		}
	} else if (p.bins8p1) {
		/* the 8192-point kernel's indices: shorts [t / 2][column] (low bytes of two spectra) and, behind them, bytes [t / 8][column]
		 * (the 9th bits of eight).  A wave takes whole groups of eight spectra of its 64 columns: one byte and four shorts per lane,
		 * two groups' worth requested before the first is used.  Scalar descriptor + one lane offset + scalar row offsets. */
		const __amdgpu_buffer_rsrc_t rlo = make_rsrc(reinterpret_cast<const char *>(p.bins) + ((size_t)c * (p.chunk >> 1) * p.n + x0) * 2);
		const __amdgpu_buffer_rsrc_t rhi = make_rsrc(reinterpret_cast<const char *>(p.bins) + (size_t)p.total * p.n + (size_t)c * (p.chunk >> 3) * p.n + x0);
		const uint32_t noct = (uint32_t)p.chunk >> 3, rowlo = 2u * (uint32_t)p.n, rowhi = (uint32_t)p.n;
		const uint32_t lane2 = 2u * (uint32_t)lane, hc4 = 4u * (uint32_t)hcol;
		auto count8 = [&](uint32_t hv, const uint32_t (&v)[4]) {
#pragma unroll
			for (int u = 0; u < 4; u++) {
				/* bin = low byte | 9th bit << 8; the row of the histogram is bin << 7 (lds_count) */
				lds_count(h, lo8(v[u]) | ((hv << (8 - 2 * u)) & 0x100u), hc4, inc);
				lds_count(h, ((v[u] >> 8) & 0xffu) | ((hv << (7 - 2 * u)) & 0x100u), hc4, inc);
			}
		};
		uint32_t o = wv;
#pragma unroll 1
		for (; o + NW < noct; o += 2 * NW) {
			const uint32_t so_l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(o * 4u * rowlo));
			const uint32_t so_h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(o * rowhi));
			uint32_t va[4], vb[4];
			const uint32_t ha = __builtin_amdgcn_raw_buffer_load_b8(rhi, (uint32_t)lane, so_h, 0);
			const uint32_t hb = __builtin_amdgcn_raw_buffer_load_b8(rhi, (uint32_t)lane, so_h + (uint32_t)NW * rowhi, 0);
#pragma unroll
			for (int u = 0; u < 4; u++) {
				va[u] = __builtin_amdgcn_raw_buffer_load_b16(rlo, lane2, so_l + (uint32_t)u * rowlo, 0);
				vb[u] = __builtin_amdgcn_raw_buffer_load_b16(rlo, lane2, so_l + (uint32_t)(4 * NW + u) * rowlo, 0);
			}
			count8(ha, va);
			count8(hb, vb);
		}
#pragma unroll 1
		for (; o < noct; o += NW) {
			const uint32_t so_l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(o * 4u * rowlo));
			uint32_t va[4];
			const uint32_t ha = __builtin_amdgcn_raw_buffer_load_b8(rhi, (uint32_t)lane, (uint32_t)__builtin_amdgcn_readfirstlane((int)(o * rowhi)), 0);
#pragma unroll
			for (int u = 0; u < 4; u++)
				va[u] = __builtin_amdgcn_raw_buffer_load_b16(rlo, lane2, so_l + (uint32_t)u * rowlo, 0);
			count8(ha, va);
		}
	} else if (p.bins16) {
		/* scalar descriptor + ONE lane offset + a scalar row offset per load (plain pointers cost a 64-bit per-lane address, two VALU
		 * operations, per row), and two operations per atomic's address (mask / shift, then shift-and-add onto the lane's column offset;
		 * left to it, the compiler shifts first and masks afterwards: three): 3.6 -> 2.1 VALU instructions per atomic */
		const __amdgpu_buffer_rsrc_t rs16 = make_rsrc(p.bins + (size_t)c * (p.chunk >> 1) * p.n + x0);	/* (a chunk's rows: < 4 GiB) */
		const uint32_t nq16 = p.chunk >> 1, rowb = 4u * (uint32_t)p.n, lane4 = 4u * (uint32_t)lane, hc4 = 4u * (uint32_t)hcol;
		uint32_t q = wv;
#pragma unroll 1
		for (; q + NW * (IF - 1) < nq16; q += NW * IF) {
			uint32_t v[IF];
			const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q * rowb));
#pragma unroll
			for (int u = 0; u < IF; u++)
				v[u] = __builtin_amdgcn_raw_buffer_load_b32(rs16, lane4, so + (uint32_t)(NW * u) * rowb, 0);
#pragma unroll
			for (int u = 0; u < IF; u++) {
				lds_count(h, lo16(v[u]), hc4, inc);
				lds_count(h, v[u] >> 16, hc4, inc);
			}
		}
#pragma unroll 1
		for (; q < nq16; q += NW) {
			const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(rs16, lane4, (uint32_t)__builtin_amdgcn_readfirstlane((int)(q * rowb)), 0);
			lds_count(h, lo16(v), hc4, inc);
			lds_count(h, v >> 16, hc4, inc);
		}
	} else {
		const __amdgpu_buffer_rsrc_t rs8 = make_rsrc(p.bins + (size_t)c * (p.chunk >> 2) * p.n + x0);
		const uint32_t nq = p.chunk >> 2, rowb = 4u * (uint32_t)p.n, lane4 = 4u * (uint32_t)lane, hc4 = 4u * (uint32_t)hcol;
		uint32_t q = wv;
#pragma unroll 1
		for (; q + NW * (IF - 1) < nq; q += NW * IF) {	/* independent loads in flight per thread */
			uint32_t v[IF];
			const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q * rowb));
#pragma unroll
			for (int u = 0; u < IF; u++)
				v[u] = __builtin_amdgcn_raw_buffer_load_b32(rs8, lane4, so + (uint32_t)(NW * u) * rowb, 0);
#pragma unroll
			for (int u = 0; u < IF; u++) {
				lds_count(h, lo8(v[u]), hc4, inc);
				lds_count(h, (v[u] >>  8) & 0xff, hc4, inc);
				lds_count(h, (v[u] >> 16) & 0xff, hc4, inc);
				lds_count(h, v[u] >> 24, hc4, inc);
			}
		}
#pragma unroll 1
		for (; q < nq; q += NW) {
			const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(rs8, lane4, (uint32_t)__builtin_amdgcn_readfirstlane((int)(q * rowb)), 0);
			lds_count(h, lo8(v), hc4, inc);
			lds_count(h, (v >>  8) & 0xff, hc4, inc);
			lds_count(h, (v >> 16) & 0xff, hc4, inc);
			lds_count(h, v >> 24, hc4, inc);
		}
	}

	K2_STAMP(2);		/* counting loop (wave 0) */
	/* live sum: sum_t pwr_t (1-a)^(B-1-t) from the tile partials, which hold
	 * sum_{t in tile} pwr_t (1-a)^(t_last - t) (display.cl:149-150) */
	{
		const int tiles = p.chunk / p.tile;
		const float2 *pp = p.partial + (size_t)c * tiles * p.n + x0 + lane;
		float s = 0.0f, m = -1000.0f;
#pragma unroll 2
		for (int j = wv; j < tiles; j += NW) {
			const float2 v = pp[(size_t)j * p.n];
			const int t_last = p.t_offset + t_in + (j + 1) * p.tile - 1;
			/* (1-a)^k as exp2(k log2(1-a)): relative error ~1e-6 where the weight is not negligible */
			s += v.x * __builtin_amdgcn_exp2f(p.log2_w * (float)(p.weight_batch - 1 - t_last));
			m = (m < v.y) ? v.y : m;
		}
		red_s[wv][lane] = s;
		red_m[wv][lane] = m;
	}
	K2_STAMP(3);		/* live-sum partials */
	__syncthreads();
	K2_STAMP(4);		/* barrier: the slowest wave's counting */

	if (tid < 64) {
		float s = 0.0f, m = -1000.0f;
#pragma unroll
		for (int j = 0; j < NW; j++) {				/* fixed order: deterministic floats */
			s += red_s[j][tid];
			m = (m < red_m[j][tid]) ? red_m[j][tid] : m;
		}
		p.chunk_sum[(size_t)c * p.n + x0 + tid] = s;
		p.chunk_max[(size_t)c * p.n + x0 + tid] = m;
	}

	if (p.hc16) {
		/* the LDS image as it is: [bin][32] packed pairs, one contiguous block per work-group
		 * (32 KiB at 256 bins); K3 unpacks */
		uint32_t *d = reinterpret_cast<uint32_t *>(p.hc16) + ((size_t)c * (p.n / 64) + blockIdx.x) * nb * 32;
		if (p.rowmask) {
			/* sparse hand-off: only the bin rows with a count are stored (a wave covers two rows of 32 dwords per
			 * step), one bit per row tells K3 which; with noise-like input 4 rows in 5 are empty */
			for (int i = tid; i < nb * 32; i += 64 * NW) {
				const uint32_t v = h[i];
				const unsigned long long bal = __ballot(v != 0);
				const uint32_t nz = (lane & 32) ? (uint32_t)(bal >> 32) : (uint32_t)bal;
				if (nz) {
					d[i] = v;
					if ((lane & 31) == 0)
						atomicOr(&rowbits[i >> 10], 1u << ((i >> 5) & 31));
				}
			}
			K2_STAMP(5);		/* sparse hand-off */
			__syncthreads();
			if (tid < p.mask_words)
				p.rowmask[((size_t)blockIdx.x * p.mask_words + tid) * p.mask_stride + c] = rowbits[tid];
			K2_STAMP(6);
			return;
		}
		{
			const uint4 *h4 = reinterpret_cast<const uint4 *>(h);
			uint4 *d4 = reinterpret_cast<uint4 *>(d);
#pragma unroll 2
			for (int i = tid; i < nb * 8; i += 64 * NW)
				d4[i] = h4[i];
		}
		return;
	}
	/* (rolled loops: the register budget of this kernel is what lets it share a SIMD with K1) */
	uint32_t *dst = p.hc + (size_t)f * nb * p.n + x0 + lane;
	const int sh = (lane & 32) ? 16 : 0;
	if (cpb == 1) {
#pragma unroll 1
		for (int b = wv; b < nb; b += NW)
			dst[(size_t)b * p.n] = (h[b * 32 + hcol] >> sh) & 0xffffu;
	} else {
#pragma unroll 1
		for (int b = wv; b < nb; b += NW) {
			const uint32_t v = (h[b * 32 + hcol] >> sh) & 0xffffu;
			if (v)
				atomicAdd(&dst[(size_t)b * p.n], v);
		}
	}
}

#ifdef K2_TIMING
extern "C" int fosphor_amd_debug_k2_timing(unsigned long long *out, int reset)
{
	unsigned long long z[16] = {};
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_k2_time), sizeof(z)) != hipSuccess) return -2;
	if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_k2_time), z, sizeof(z)) != hipSuccess) return -3;
	return 0;
}
#endif

hipError_t launch_k2(const K2Params &p, int n_chunks, hipStream_t s)
{
	const size_t lds = (size_t)p.n_bins * 32 * sizeof(uint32_t);
	constexpr int kIf16 = 4;	/* index loads in flight per thread, 16-bit / 9-bit index geometries (measured, see k2_count) */
	constexpr int kIf8  = 8;	/* ... 8-bit indices, chunks of at most 1024 spectra (measured) */
	if (p.bins16 || p.bins9 || p.bins8p1)
		hipLaunchKernelGGL((k2_count<16, kIf16>), dim3((p.n / 64), n_chunks), dim3(1024), lds, s, p);
	else if (p.chunk > 1024)
		hipLaunchKernelGGL((k2_count<4, 4>), dim3((p.n / 64), n_chunks), dim3(256), lds, s, p);
	else
		hipLaunchKernelGGL((k2_count<4, kIf8>), dim3((p.n / 64), n_chunks), dim3(256), lds, s, p);
	return hipGetLastError();
}

/* fixed-order reduction of the chunk partials of each batch */
__global__ __launch_bounds__(256)
void k2b_reduce(const K2bParams p)
{
	const int gid = blockIdx.x * 256 + threadIdx.x;
	if (gid >= p.n_batches * p.n)
		return;
	const int f = gid / p.n, x = gid - f * p.n;
	float s = 0.0f, m = -1000.0f;
	for (int c = 0; c < p.cpb; c++) {
		const size_t i = (size_t)(f * p.cpb + c) * p.n + x;
		s += p.chunk_sum[i];
		m = (m < p.chunk_max[i]) ? p.chunk_max[i] : m;
	}
	p.live_sum[gid] = s;
	p.vmax[gid] = m;
}

hipError_t launch_k2b(const K2bParams &p, hipStream_t s)
{
	const int threads = p.n_batches * p.n;
	hipLaunchKernelGGL(k2b_reduce, dim3((threads + 255) / 256), dim3(256), 0, s, p);
	return hipGetLastError();
}

/* One batch of cpb chunks (the time shard of a display frame): sum the chunks' packed 16-bit
 * count slabs into the 32-bit [bin][x] array the all-reduce and K3 work on, and reduce the float
 * partials in the same fixed order as k2b_reduce.  Integer sums: exact, order-independent. */
__global__ __launch_bounds__(256)
void k2c_sum(const K2bParams p)
{
	const int pairs = p.n_bins * p.n / 2;		/* dwords per chunk slab set: columns c, c + 32 packed */
	const int cells = pairs;			/* thread index space: one thread per packed pair */
	const int gid = blockIdx.x * 256 + threadIdx.x;
	const int f = blockIdx.y;			/* batch of the launch */
	if (gid < pairs) {
		const int nb = p.n_bins;
		const int slab = gid / (nb * 32);
		const int rem = gid - slab * nb * 32;
		const int bin = rem >> 5, hcol = rem & 31;
		const uint32_t *src = reinterpret_cast<const uint32_t *>(p.hc16) + (size_t)f * p.cpb * pairs + gid;
		uint32_t lo = 0, hi = 0;
		int c = 0;
		for (; c + 8 <= p.cpb; c += 8) {
			uint32_t v[8];
#pragma unroll
			for (int u = 0; u < 8; u++)
				v[u] = __builtin_nontemporal_load(&src[(size_t)(c + u) * pairs]);
#pragma unroll
			for (int u = 0; u < 8; u++) {
				lo += v[u] & 0xffffu;
				hi += v[u] >> 16;
			}
		}
		for (; c < p.cpb; c++) {
			const uint32_t v = src[(size_t)c * pairs];
			lo += v & 0xffffu;
			hi += v >> 16;
		}
		uint32_t *dst = p.hc + (size_t)f * p.n_bins * p.n + bin * p.n + slab * 64 + hcol;
		dst[0]  = lo;
		dst[32] = hi;
	} else if (gid < cells + p.n) {
		const int x = gid - cells;
		const float *cs = p.chunk_sum + (size_t)f * p.cpb * p.n, *cm = p.chunk_max + (size_t)f * p.cpb * p.n;
		float s = 0.0f, m = -1000.0f;
		int c = 0;
		for (; c + 8 <= p.cpb; c += 8) {
			float a[8], b[8];
#pragma unroll
			for (int u = 0; u < 8; u++) {
				a[u] = cs[(size_t)(c + u) * p.n + x];
				b[u] = cm[(size_t)(c + u) * p.n + x];
			}
#pragma unroll
			for (int u = 0; u < 8; u++) {		/* same order as k2b_reduce */
				s += a[u];
				m = (m < b[u]) ? b[u] : m;
			}
		}
		for (; c < p.cpb; c++) {
			s += cs[(size_t)c * p.n + x];
			m = (m < cm[(size_t)c * p.n + x]) ? cm[(size_t)c * p.n + x] : m;
		}
		p.live_sum[(size_t)f * p.n + x] = s;
		p.vmax[(size_t)f * p.n + x] = m;
	}
}

hipError_t launch_k2c(const K2bParams &p, hipStream_t s)
{
	const int threads = p.n_bins * p.n / 2 + p.n;
	hipLaunchKernelGGL(k2c_sum, dim3((threads + 255) / 256, p.n_batches), dim3(256), 0, s, p);
	return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* K3: state update                                                          */
/* ------------------------------------------------------------------------ */

/* MODE 0: 16-bit slab-major counts + LDS (d, e) table (batch <= 1024); 3: the same counts, table in memory
 * (batches of up to 8192 spectra counted as one chunk); 1: 32-bit counts + (d, e) table in memory;
 * 2: 32-bit counts, (d, e) evaluated per cell (batches beyond the table).  Separate instantiations keep
 * the common one (0) at a register budget that lets it share a SIMD with K1. */
constexpr int kK3Rows = 2;		/* rows in flight per wave of the sparse form: measured at N = 65536, 1 / 2 / 3 / 4 / 8 / 16 -> scan + merge 56 / 49 / 49 /
					 * 53 / 61 / 114 us per frame (42 / 58 / 74 / ... / 256 VGPRs: more resident waves beat more requests per wave) */
constexpr int kK3Batches = 2;		/* batches of counts in flight per row of the sparse form (measured) */
template <int MODE, bool SPARSE = false>
__global__ __launch_bounds__(256)
void k3_merge(const K3Params p)
{
	const int cells = p.n_bins * p.n;
	const float fbatch = (float)p.batch;

	/* the (d, e) table of the 16-bit path sits in LDS: loaded once per work-group, which then strides
	 * over the cells (the grid is capped, so a 128 MiB state does not reload it 131 072 times) */
	/* (long batches, MODE 3: in LDS as well up to 4096 spectra -- a look-up in memory is one more dependent round trip per batch
	 * and cell; longer batches read it from memory) */
	constexpr int kRiseLds = (MODE == 0) ? 1025 : (MODE == 3 && !SPARSE) ? kK3RiseLdsLong : 1;
	__shared__ float2 rise_lds[kRiseLds];
	const bool rise_in_lds = (MODE == 0) || (MODE == 3 && !SPARSE && p.batch < kRiseLds);
	if (rise_in_lds) {
		for (int i = threadIdx.x; i <= p.batch && i < kRiseLds; i += 256)
			rise_lds[i] = p.rise[i];
		__syncthreads();
	}

	/* one column: live EMA (display.cl:186-214) and max-hold (display.cl:257-310) */
	auto update_column = [&](const int x) {
		const int half = p.n >> 1;
		const int i = x ^ half;
		const float decay = p.live_decay;
		float live = p.spectrum[i].y;
		float mh   = p.spectrum[p.n + i].y;
		for (int f = 0; f < p.n_batches; f++) {
			const float sum = p.live_sum[(size_t)f * p.n + x];
			const float mx  = p.vmax[(size_t)f * p.n + x];
			if (!__builtin_isfinite(live))
				live = sum / 16.0f;			/* display.cl:206-207 */
			live = live * decay + sum * p.alpha;		/* display.cl:210-211 */
			if (!__builtin_isfinite(mh))
				mh = -3.402823466e+38f;			/* display.cl:290-291 */
			mh = mh * 0.999f + 0.001f * live;		/* display.cl:303 */
			mh = (mh < mx) ? mx : mh;			/* display.cl:304-305 */
		}
		const float vx = ((float)i / (float)half) - 1.0f;	/* display.cl:209,293 */
		p.spectrum[i]      = make_float2(vx, live);
		p.spectrum[p.n + i] = make_float2(vx, mh);
	};

	if (SPARSE) {
		/* Sparse form: k3_scan has listed the rows that are alive (hot, or with a count in some batch of the launch);
		 * a wave takes every n_waves-th entry of the list, its 64 lanes are the row's 64 cells.  A cold, empty row
		 * costs one byte of flag and a few mask bits in the scan and nothing here. */
		const int lane = threadIdx.x & 63;
		const int nb = p.n_bins;
		const int n_waves = gridDim.x * 4;
		const int count = (int)p.rowlist[p.rowlist_cnt];
		const int col = (lane >> 1) + ((lane & 1) << 5);
		constexpr int R = kK3Rows;		/* rows in flight per wave: every step below is R independent requests */
		constexpr int U = kK3Batches;		/* batches of counts in flight per row */
		if (p.n_batches <= U) {
			/* One or two batches per launch (a display frame of the 65536-point configuration is ONE): a row is a list entry, then
			 * the histogram value and the counts it points to -- two dependent round trips for a few instructions of arithmetic, and a
			 * wave walks ~20 rows.  Software pipeline, three deep: while row set i is computed and stored, the values of set i + 1 are
			 * on their way and so are the list entries of set i + 2 (loads return in order: each wait leaves the younger requests
			 * outstanding). */
			const int step = R * n_waves;
			const int fe = p.n_batches;
			int idx = (blockIdx.x * 256 + threadIdx.x) >> 6;
			uint32_t e_c[R], e_n[R], hc_c[R][U], hc_n[R][U];
			int hidx_c[R], hidx_n[R];
			float hv0_c[R], hv0_n[R];
			auto entries = [&](int at, uint32_t (&e)[R]) {
#pragma unroll
				for (int r = 0; r < R; r++)
					e[r] = (at + r * n_waves < count) ? p.rowlist[1 + at + r * n_waves] : 0xffffffffu;	/* (no such entry: row index 0xfffff with every flag) */
			};
			auto values = [&](const uint32_t (&e)[R], int (&hidx)[R], float (&hv0)[R], uint32_t (&hc)[R][U]) {
#pragma unroll
				for (int r = 0; r < R; r++) {
					const bool ok = e[r] != 0xffffffffu;
					const int row = (int)(e[r] & 0xfffffu);
					const int slab = row / nb, bin = row - slab * nb;
					hidx[r] = bin * p.n + slab * 64 + col;
					hv0[r] = ok ? p.hist[hidx[r]] : 0.0f;
#pragma unroll
					for (int u = 0; u < U; u++)
						hc[r][u] = (ok && u < fe && ((e[r] >> (20 + u)) & 1u))
						        ? (uint32_t)__builtin_nontemporal_load(&p.hc16[(size_t)u * cells + row * 64 + lane]) : 0u;
				}
			};
			entries(idx, e_c);
			values(e_c, hidx_c, hv0_c, hc_c);
			entries(idx + step, e_n);
			for (; idx < count; idx += step) {
				uint32_t e_nn[R];
				values(e_n, hidx_n, hv0_n, hc_n);
				entries(idx + 2 * step, e_nn);
#pragma unroll
				for (int r = 0; r < R; r++) {
					if (e_c[r] == 0xffffffffu)		/* uniform */
						continue;
					float hv = hv0_c[r];
#pragma unroll
					for (int u = 0; u < U; u++) {
						if (u < fe && !((hv <= 0.01f) && (hc_c[r][u] == 0))) {	/* display.cl:237-238 */
							const float2 de = (MODE == 0) ? rise_lds[hc_c[r][u]] : p.rise[hc_c[r][u]];
							hv = (hv - de.x) * de.y + de.x;			/* display.cl:247 */
							hv = (hv < 0.0f) ? 0.0f : hv;			/* clamp, display.cl:250 */
							hv = (1.0f < hv) ? 1.0f : hv;
						}
					}
					if (__float_as_uint(hv) != __float_as_uint(hv0_c[r]))
						p.hist[hidx_c[r]] = hv;		/* cold cells (display.cl:237-238) keep their line clean */
					const bool was_hot = (e_c[r] >> 31) != 0;
					const bool now_hot = __ballot(!(hv <= 0.01f)) != 0;
					if (lane == 0 && (p.hot_all || now_hot != was_hot))
						p.hot[e_c[r] & 0xfffffu] = now_hot ? 1 : 0;
				}
#pragma unroll
				for (int r = 0; r < R; r++) {
					e_c[r] = e_n[r]; hidx_c[r] = hidx_n[r]; hv0_c[r] = hv0_n[r];
#pragma unroll
					for (int u = 0; u < U; u++)
						hc_c[r][u] = hc_n[r][u];
					e_n[r] = e_nn[r];
				}
			}
		} else
		for (int idx0 = (blockIdx.x * 256 + threadIdx.x) >> 6; idx0 < count; idx0 += R * n_waves) {
			uint32_t e[R];
			int slab[R], bin[R], hidx[R], gid[R];
			float hv0[R], hv[R];
			bool valid[R];
#pragma unroll
			for (int r = 0; r < R; r++) {
				valid[r] = idx0 + r * n_waves < count;		/* uniform */
				e[r] = valid[r] ? p.rowlist[1 + idx0 + r * n_waves] : 0u;
			}
#pragma unroll
			for (int r = 0; r < R; r++) {
				const int row = (int)(e[r] & 0xfffffu);
				slab[r] = row / nb; bin[r] = row - slab[r] * nb;
				gid[r] = row * 64 + lane;
				hidx[r] = bin[r] * p.n + slab[r] * 64 + col;
				hv0[r] = valid[r] ? p.hist[hidx[r]] : 0.0f;
				hv[r] = hv0[r];
			}
			for (int f0 = 0; f0 < p.n_batches; f0 += 64) {
				unsigned long long m[R];
				const int fl = f0 + lane;
				if (p.n_batches <= 11) {
#pragma unroll
					for (int r = 0; r < R; r++)
						m[r] = (e[r] >> 20) & 0x7ffu;		/* carried by the list entry */
				} else {
#pragma unroll
					for (int r = 0; r < R; r++) {
						const uint32_t wd = (valid[r] && fl < p.n_batches)
						        ? p.rowmask[((size_t)slab[r] * p.mask_words + (bin[r] >> 5)) * p.mask_stride + fl] : 0u;
						m[r] = __ballot((wd >> (bin[r] & 31)) & 1u);
					}
				}
				const int fe = (p.n_batches - f0 < 64) ? p.n_batches : f0 + 64;
				for (int f = f0; f < fe; f += U) {
					uint32_t hc[R][U];
#pragma unroll
					for (int r = 0; r < R; r++)
#pragma unroll
						for (int u = 0; u < U; u++)
							hc[r][u] = (f + u < fe && ((m[r] >> (f + u - f0)) & 1ull))
							        ? (uint32_t)__builtin_nontemporal_load(&p.hc16[(size_t)(f + u) * cells + gid[r]]) : 0u;
#pragma unroll
					for (int r = 0; r < R; r++)
#pragma unroll
						for (int u = 0; u < U; u++) {
							if (f + u < fe && !((hv[r] <= 0.01f) && (hc[r][u] == 0))) {	/* display.cl:237-238 */
								const float2 de = (MODE == 0) ? rise_lds[hc[r][u]] : p.rise[hc[r][u]];
								hv[r] = (hv[r] - de.x) * de.y + de.x;		/* display.cl:247 */
								hv[r] = (hv[r] < 0.0f) ? 0.0f : hv[r];		/* clamp, display.cl:250 */
								hv[r] = (1.0f < hv[r]) ? 1.0f : hv[r];
							}
						}
				}
			}
#pragma unroll
			for (int r = 0; r < R; r++) {
				if (!valid[r])
					continue;
				if (__float_as_uint(hv[r]) != __float_as_uint(hv0[r]))
					p.hist[hidx[r]] = hv[r];	/* cold cells (display.cl:237-238) keep their line clean */
				const bool was_hot = (e[r] >> 31) != 0;
				const bool now_hot = __ballot(!(hv[r] <= 0.01f)) != 0;
				if (lane == 0 && (p.hot_all || now_hot != was_hot))
					p.hot[e[r] & 0xfffffu] = now_hot ? 1 : 0;
			}
		}
		for (int x = blockIdx.x * 256 + threadIdx.x; x < p.n; x += gridDim.x * 256)
			update_column(x);
		return;
	}

	if (MODE == 3 && !SPARSE && p.n_batches <= kK3LongFew) {
		/* Long batches come a few per launch (4 at N = 8192): too few for the batches-in-flight scheme below to hide anything, and a
		 * thread that walks its cells one after the other pays a memory round trip per cell.  FOUR CELLS IN FLIGHT per thread instead:
		 * their histogram values and all their counts are requested together. */
		constexpr int R = 4;
		const int stride = gridDim.x * 256;
		const int nb = p.n_bins, fe = p.n_batches;
		const int pairs = cells >> 1;		/* a dword of the slabs = columns c and c + 32 of one (slab, bin) */
		const uint32_t *hc32 = reinterpret_cast<const uint32_t *>(p.hc16);
		for (int base = blockIdx.x * 256 + threadIdx.x; base < pairs; base += R * stride) {
			int hidx[R]; float hv0[R][2]; uint32_t hc[R][kK3LongFew];
#pragma unroll
			for (int r = 0; r < R; r++) {
				const int g = base + r * stride;
				const bool ok = g < pairs;
				const int gg = ok ? g : base;
				const int slab = gg / (nb * 32);
				const int rem = gg - slab * nb * 32;
				hidx[r] = ok ? (rem >> 5) * p.n + slab * 64 + (rem & 31) : -1;
				hv0[r][0] = p.hist[ok ? hidx[r] : 0];
				hv0[r][1] = p.hist[ok ? hidx[r] + 32 : 0];
#pragma unroll
				for (int f = 0; f < kK3LongFew; f++)
					hc[r][f] = (f < fe) ? __builtin_nontemporal_load(&hc32[(size_t)f * pairs + gg]) : 0u;
			}
#pragma unroll
			for (int r = 0; r < R; r++) {
#pragma unroll
				for (int h = 0; h < 2; h++) {
					float hv = hv0[r][h];
#pragma unroll
					for (int f = 0; f < kK3LongFew; f++) {
						const uint32_t c16 = h ? (hc[r][f] >> 16) : (hc[r][f] & 0xffffu);
						if (f < fe && !((hv <= 0.01f) && (c16 == 0))) {	/* display.cl:237-238 */
							const float2 de = rise_in_lds ? rise_lds[c16] : p.rise[c16];
							hv = (hv - de.x) * de.y + de.x;			/* display.cl:247 */
							hv = (hv < 0.0f) ? 0.0f : hv;			/* clamp, display.cl:250 */
							hv = (1.0f < hv) ? 1.0f : hv;
						}
					}
					if (hidx[r] >= 0 && __float_as_uint(hv) != __float_as_uint(hv0[r][h]))
						p.hist[hidx[r] + 32 * h] = hv;	/* cold cells (display.cl:237-238) keep their line clean */
				}
			}
		}
		for (int x = blockIdx.x * 256 + threadIdx.x; x < p.n; x += stride)
			update_column(x);
		return;
	}

	for (int gid = blockIdx.x * 256 + threadIdx.x; gid < cells + p.n; gid += gridDim.x * 256) {
	if (MODE == 0 || MODE == 3) {
		/* 16-bit slab-major counts as K2 leaves them ([slab of 64 columns][bin][32] dwords, columns
		 * c and c + 32 in the low / high half): thread gid reads the gid-th 16-bit word of a batch
		 * (2 B per batch, 8 batches in flight); the (d, e) table sits in LDS (one dependent lookup
		 * per batch per cell). */
		if (gid < cells) {
			const int nb = p.n_bins;
			const int slab = gid / (nb * 64);
			const int rem = gid - slab * nb * 64;
			const int bin = rem >> 6;
			const int col = ((rem & 63) >> 1) + ((rem & 1) << 5);
			const int hidx = bin * p.n + slab * 64 + col;
			const float hv0 = p.hist[hidx];
			float hv = hv0;
			{
				const int fe = p.n_batches;
				int f = 0;
				for (; f + 8 <= fe; f += 8) {
					uint32_t hc[8];
#pragma unroll
					for (int u = 0; u < 8; u++)
						hc[u] = (uint32_t)__builtin_nontemporal_load(&p.hc16[(size_t)(f + u) * cells + gid]);
#pragma unroll
					for (int u = 0; u < 8; u++) {
						if (!((hv <= 0.01f) && (hc[u] == 0))) {	/* display.cl:237-238 */
							const float2 de = rise_in_lds ? rise_lds[hc[u]] : p.rise[hc[u]];
							hv = (hv - de.x) * de.y + de.x;		/* display.cl:247 */
							hv = (hv < 0.0f) ? 0.0f : hv;		/* clamp, display.cl:250 */
							hv = (1.0f < hv) ? 1.0f : hv;
						}
					}
				}
				/* (launches of fewer than 8 batches -- 4 at N = 8192 -- : the counts of what is left requested together as well) */
				if (f + 4 <= fe) {
					uint32_t hc[4];
#pragma unroll
					for (int u = 0; u < 4; u++)
						hc[u] = (uint32_t)__builtin_nontemporal_load(&p.hc16[(size_t)(f + u) * cells + gid]);
#pragma unroll
					for (int u = 0; u < 4; u++) {
						if (!((hv <= 0.01f) && (hc[u] == 0))) {
							const float2 de = rise_in_lds ? rise_lds[hc[u]] : p.rise[hc[u]];
							hv = (hv - de.x) * de.y + de.x;
							hv = (hv < 0.0f) ? 0.0f : hv;
							hv = (1.0f < hv) ? 1.0f : hv;
						}
					}
					f += 4;
				}
				for (; f < fe; f++) {
					const uint32_t hc = (uint32_t)p.hc16[(size_t)f * cells + gid];
					if (!((hv <= 0.01f) && (hc == 0))) {
						const float2 de = rise_in_lds ? rise_lds[hc] : p.rise[hc];
						hv = (hv - de.x) * de.y + de.x;
						hv = (hv < 0.0f) ? 0.0f : hv;
						hv = (1.0f < hv) ? 1.0f : hv;
					}
				}
			}
			if (__float_as_uint(hv) != __float_as_uint(hv0))
				p.hist[hidx] = hv;	/* cold cells (display.cl:237-238) keep their line clean */
		}
	}
	if (MODE == 0 || MODE == 3) {
		/* cells handled above */
	} else if (gid < cells && (p.cell_end == 0 || (gid >= p.cell_begin && gid < p.cell_end))) {
		/* one (bin, x) cell; batches applied in order (display.cl:217-254).
		 * d and e of display.cl:241-245 depend only on the hit count: with a table
		 * rise[hc] = (d, e) (host-computed with the same powf the oracle uses) the update
		 * is a lookup and display.cl:247,250. */
		float hv = p.hist[gid];
		if (MODE == 1) {
			/* 8 batches of counts in flight per thread: the loop is otherwise one dependent
			 * HBM/L2 round trip per batch */
			int f = 0;
			for (; f + 8 <= p.n_batches; f += 8) {
				uint32_t hc[8];
#pragma unroll
				for (int u = 0; u < 8; u++)
					hc[u] = __builtin_nontemporal_load(&p.hc[(size_t)(f + u) * cells + gid]);
#pragma unroll
				for (int u = 0; u < 8; u++) {
					if (!((hv <= 0.01f) && (hc[u] == 0))) {	/* display.cl:237-238 */
						const float2 de = p.rise[hc[u]];
						hv = (hv - de.x) * de.y + de.x;		/* display.cl:247 */
						hv = (hv < 0.0f) ? 0.0f : hv;		/* clamp, display.cl:250 */
						hv = (1.0f < hv) ? 1.0f : hv;
					}
				}
			}
			for (; f < p.n_batches; f++) {
				const uint32_t hc = p.hc[(size_t)f * cells + gid];
				if (!((hv <= 0.01f) && (hc == 0))) {
					const float2 de = p.rise[hc];
					hv = (hv - de.x) * de.y + de.x;
					hv = (hv < 0.0f) ? 0.0f : hv;
					hv = (1.0f < hv) ? 1.0f : hv;
				}
			}
		} else {
			const float rt0r = 1.0f / p.t0r, rt0d = 1.0f / p.t0d;
			for (int f = 0; f < p.n_batches; f++) {
				const uint32_t hc = p.hc[(size_t)f * cells + gid];
				if ((hv <= 0.01f) && (hc == 0))			/* display.cl:237-238 */
					continue;
				const float a = (float)hc / fbatch;		/* display.cl:241-245 */
				const float b = a * rt0r;
				const float c = b + rt0d;
				const float d = b * (1.0f / c);
				const float e = powf(1.0f - c, fbatch);
				hv = (hv - d) * e + d;				/* display.cl:247 */
				hv = (hv < 0.0f) ? 0.0f : hv;			/* clamp, display.cl:250 */
				hv = (1.0f < hv) ? 1.0f : hv;
			}
		}
		p.hist[gid] = hv;
	}
	if (gid >= cells && gid < cells + p.n)
		update_column(gid - cells);
	}	/* cell loop */
}

/* Sparse form, first step: the list of live rows.  rowlist[rowlist_cnt] = count -- two counters, word 0 and the word behind the list,
 * used by alternate launches: a scan zeroes the one the NEXT scan will add to (its last reader, the merge kernel before this scan, has
 * finished: same stream), so the host queues no memset per frame --, rowlist[1 + i] = row
 * index (20 bits), bits 20-30 = which batches have counts in the row (launches of <= 11 batches), bit 31 = the row's hot
 * flag as stored. */
__global__ __launch_bounds__(1024)
void k3_scan(const K3Params p)
{
	constexpr int RPT = 4;				/* rows per thread: 4096 rows and ONE atomic on the shared counter per block */
	__shared__ uint32_t wave_cnt[16], wave_base[16];
	const int rows = p.n_bins * (p.n >> 6);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int row0 = blockIdx.x * (1024 * RPT) + threadIdx.x;
	/* (list order = row order, slab-major like the count kernel's output.  Bin-major -- consecutive entries the same bin of adjacent
	 * slabs, i.e. adjacent 256-byte pieces of the histogram but counts 64 KiB apart -- measured 45 against 40 us at N = 65536.) */
	bool hot[RPT], act[RPT];
	uint32_t bits[RPT];			/* bit f: batch f of the launch has counts in this row (launches of <= 11 batches) */
	uint32_t mine = 0;
	const bool carry = p.n_batches <= 11;	/* ... then the list entry carries them and k3_merge needs no mask request */
#pragma unroll
	for (int k = 0; k < RPT; k++) {
		const int row = row0 + 1024 * k;
		hot[k] = (row < rows) && p.hot[row] != 0;
		act[k] = (row < rows) && (hot[k] || p.hot_all);
		bits[k] = 0;
	}
#pragma unroll
	for (int k = 0; k < RPT; k++) {
		const int row = row0 + 1024 * k;
		if (row < rows && (carry || !act[k])) {
			const int slab = row / p.n_bins, bin = row - slab * p.n_bins;
			const uint32_t *mw = p.rowmask + ((size_t)slab * p.mask_words + (bin >> 5)) * p.mask_stride;
			uint32_t any = 0;
			for (int f = 0; f < p.n_batches; f++) {
				const uint32_t b = (mw[f] >> (bin & 31)) & 1u;
				any |= b;
				if (carry)
					bits[k] |= b << f;
			}
			act[k] = act[k] || any;
		}
		mine += act[k] ? 1u : 0u;
	}
	/* wave prefix of `mine`, then the waves' totals through LDS */
	uint32_t incl = mine;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(incl, d, 64);
		if (lane >= d) incl += o;
	}
	if (lane == 63)
		wave_cnt[wv] = incl;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tot = 0;
		for (int w = 0; w < 16; w++) { wave_base[w] = tot; tot += wave_cnt[w]; }
		const uint32_t base = tot ? atomicAdd(&p.rowlist[p.rowlist_cnt], tot) : 0u;
		if (blockIdx.x == 0)
			p.rowlist[p.rowlist_cnt ? 0 : 1 + rows] = 0;
		for (int w = 0; w < 16; w++) wave_base[w] += base;
	}
	__syncthreads();
	uint32_t pos = wave_base[wv] + incl - mine;
#pragma unroll
	for (int k = 0; k < RPT; k++)
		if (act[k])
			p.rowlist[1 + pos++] = (uint32_t)(row0 + 1024 * k) | (bits[k] << 20) | (hot[k] ? 0x80000000u : 0u);
}

/* Which form a launch takes: the shape of the launch and the buffers the host filled in decide, never the data */
K3Form k3_form(const K3Shape &p)
{
	if (p.hc16 && p.rowmask && p.n_bins * (p.n / 64) <= (1 << 20))	/* (list entries hold 20 bits of row index: every geometry the library accepts) */
		return p.batch <= 1024 ? K3_SPARSE16 : K3_SPARSE16_LONG;
	if (p.hc16 && p.batch <= 1024)
		return K3_DENSE16;
	if (p.hc16)
		return p.n_batches <= kK3LongFew ? K3_DENSE16_LONG4 : K3_DENSE16_LONG;	/* (the branch k3_merge<3> takes inside) */
	return p.table ? K3_TABLE32 : K3_EVAL32;
}

hipError_t launch_k3(const K3Params &p, hipStream_t s)
{
	const int threads = p.n_bins * p.n + p.n;
	int blocks = (threads + 255) / 256;
	if (blocks > 8192) blocks = 8192;
	switch (k3_form(k3_shape(p))) {
	case K3_SPARSE16:
	case K3_SPARSE16_LONG: {
		/* sparse form: list the live rows, then one wave per listed row (strided) */
		const int rows = p.n_bins * (p.n / 64);
		hipLaunchKernelGGL(k3_scan, dim3((rows + 4095) / 4096), dim3(1024), 0, s, p);
		int sb = (rows + 4 * kK3Rows - 1) / (4 * kK3Rows);	/* 4 waves x kK3Rows rows in flight per block; the list is usually far shorter */
		if (sb > 2048) sb = 2048;
		if (p.batch <= 1024)
			hipLaunchKernelGGL((k3_merge<0, true>), dim3(sb), dim3(256), 0, s, p);
		else
			hipLaunchKernelGGL((k3_merge<3, true>), dim3(sb), dim3(256), 0, s, p);
		break;
	}
	case K3_DENSE16:
		hipLaunchKernelGGL(k3_merge<0>, dim3(blocks), dim3(256), 0, s, p);
		break;
	case K3_DENSE16_LONG4:
	case K3_DENSE16_LONG:	/* (each work-group loads the 32 KiB table: four per CU stride over the cells) */
		hipLaunchKernelGGL(k3_merge<3>, dim3(p.batch <= 4096 && blocks > 1024 ? 1024 : blocks), dim3(256), 0, s, p);
		break;
	case K3_TABLE32:
		hipLaunchKernelGGL(k3_merge<1>, dim3(blocks), dim3(256), 0, s, p);
		break;
	default:
		hipLaunchKernelGGL(k3_merge<2>, dim3(blocks), dim3(256), 0, s, p);
		break;
	}
	return hipGetLastError();
}

/* ------------------------------------------------------------------------ */

__global__ void k_fill(float *dst, float value, size_t n)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		dst[i] = value;
}

/* uint32 [bin][x] view of one batch of 16-bit slab-major counts (the layout K3 mode 0 / 3 reads; rows K2 did not
 * store -- clear bit in its row mask -- are zero) */
__global__ __launch_bounds__(256)
void k_export_hc16(const uint16_t *__restrict__ hc16, const uint32_t *__restrict__ rowmask, int mask_words, int mask_stride,
                   uint32_t *__restrict__ out, int n_bins, int n)
{
	const size_t cells = (size_t)n_bins * n;
	for (size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x; gid < cells; gid += (size_t)gridDim.x * 256) {
		const int slab = (int)(gid / ((size_t)n_bins * 64));
		const int rem = (int)(gid - (size_t)slab * n_bins * 64);
		const int bin = rem >> 6;
		const int col = ((rem & 63) >> 1) + ((rem & 1) << 5);
		const bool stored = !rowmask || ((rowmask[((size_t)slab * mask_words + (bin >> 5)) * mask_stride] >> (bin & 31)) & 1u);
		out[(size_t)bin * n + slab * 64 + col] = stored ? hc16[gid] : 0u;
	}
}

hipError_t launch_export_hc16(const uint16_t *hc16, const uint32_t *rowmask, int mask_words, int mask_stride, uint32_t *out, int n_bins, int n, hipStream_t s)
{
	size_t blocks = ((size_t)n_bins * n + 255) / 256;
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(k_export_hc16, dim3((unsigned)blocks), dim3(256), 0, s, hc16, rowmask, mask_words, mask_stride, out, n_bins, n);
	return hipGetLastError();
}

hipError_t launch_fill(float *dst, float value, size_t n, hipStream_t s)
{
	size_t blocks = (n + 255) / 256;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(k_fill, dim3((unsigned)blocks), dim3(256), 0, s, dst, value, n);
	return hipGetLastError();
}

} // namespace fosphor_amd
