/*
 * fosphor_tables.cpp -- the host-side tables of libfosphor_amd.so: FFT twiddles and exact bin thresholds, and the hooks that hand
 * them to the CPU tests (no GPU).
 */
#include <errno.h>
#include <math.h>

#include "fosphor_instance.h"
#include "../../include/fosphor_portable_math.h"

/* Twiddles.  N = 1024: exactly as the reference forms them (fft.cl:62-68,162-166,286-297), native_sin / native_cos pinned to
 * fosphor_portable_math.h; one block per radix-8 pass with p = 8, 64 ([k < p][n = 1..7]), then the final radix-2 pass
 * ([k < N/2]): the kTw2Off / kTw3Off / kTw4Off layout of fosphor_internal.h.
 *
 * N = 8192 and N = 65536 run this build's own plans (no reference behaviour exists at these lengths; oracle/fosphor_oracle.c,
 * o_pass_radix8_fma / o_pass_radix16_fma / o_pass_radix2_fma, restates them): the reference's Stockham passes with the twiddles
 * ON the radix-2 butterflies of a pass instead of on its inputs, so an item needs the twiddles of its stages -- every one of them
 * exp(-j pi q / den) for integers q, den, formed like the reference's (one float expression, pinned sin / cos): tw_long().
 *   both:       block  0    the constants W16, W8, W16^3 (first pass)
 *   N = 8192:   blocks 1-2  passes p = 16, 256: [k < p][8] = w^8, w^4, w^2, w^2 W8, w, w W16, w W8, w W16^3   (w = exp(-j pi k / (8 p)))
 *               block  3    the radix-2 pass: [k < 4096] = exp(-j pi k / 4096)
 *   N = 65536:  blocks 1-3  passes p = 16, 256, 4096: [k < p][8], as above */
static float2 tw_long(int q, int den)
{
	const float PI_F = 3.141592653589f;		/* fft.cl:26 */
	const float arg = -PI_F * (float)q / (float)den;
	return make_float2(fpm_cosf(arg), fpm_sinf(arg));
}

static int build_twiddles16(float2 *tw, int *offsets /* [8] or NULL */)
{
	int pos = 0, q = 0;
	if (offsets) offsets[q] = pos;
	q++;
	for (int m = 1; m <= 3; m++) {
		if (tw) tw[pos] = tw_long(m, 8);
		pos++;
	}
	for (int p = 16; p <= 4096; p *= 16, q++) {
		if (offsets) offsets[q] = pos;
		const int d = 8 * p;
		for (int k = 0; k < p; k++) {
			const int qs[8] = { 8 * k, 4 * k, 2 * k, 2 * k + 2 * p, k, k + p, k + 2 * p, k + 3 * p };
			for (int f = 0; f < 8; f++) {
				if (tw) tw[pos] = tw_long(qs[f], d);
				pos++;
			}
		}
	}
	return pos;
}

static int build_twiddles13(float2 *tw, int *offsets /* [8] or NULL */)
{
	const int n = 8192;
	int pos = 0, q = 0;
	if (offsets) offsets[q] = pos;
	q++;
	for (int m = 1; m <= 3; m++) {
		if (tw) tw[pos] = tw_long(m, 8);
		pos++;
	}
	for (int p = 16; p <= 256; p *= 16, q++) {
		if (offsets) offsets[q] = pos;
		const int d = 8 * p;
		for (int k = 0; k < p; k++) {
			const int qs[8] = { 8 * k, 4 * k, 2 * k, 2 * k + 2 * p, k, k + p, k + 2 * p, k + 3 * p };
			for (int f = 0; f < 8; f++) {
				if (tw) tw[pos] = tw_long(qs[f], d);
				pos++;
			}
		}
	}
	if (offsets) offsets[q] = pos;
	for (int k = 0; k < n / 2; k++) {
		if (tw) tw[pos] = tw_long(k, n / 2);
		pos++;
	}
	return pos;
}

int fosphor_amd::build_twiddles(float2 *tw, int log2n, int *offsets /* [8] or NULL */)
{
	const float PI_F = 3.141592653589f;		/* fft.cl:26 */
	const int n = 1 << log2n;
	int pos = 0, q = 0;
	if (log2n == 16)
		return build_twiddles16(tw, offsets);
	if (log2n == 13)
		return build_twiddles13(tw, offsets);
	for (int p = 8; p < n / 2; p *= 8, q++) {
		if (offsets) offsets[q] = pos;
		for (int k = 0; k < p; k++) {
			const float alpha = -PI_F * (float)k / (float)(4 * p);
			for (int f = 1; f < 8; f++) {
				const float arg = (float)f * alpha;
				if (tw) tw[pos] = make_float2(fpm_cosf(arg), fpm_sinf(arg));
				pos++;
			}
		}
	}
	if (offsets) offsets[q] = pos;
	for (int k = 0; k < n / 2; k++) {
		const float alpha = -PI_F * (float)k / (float)(n / 2);
		const float arg = (float)1 * alpha;
		if (tw) tw[pos] = make_float2(fpm_cosf(arg), fpm_sinf(arg));
		pos++;
	}
	return pos;
}

/* Exact bin thresholds on the double squared magnitude: thr[b] = smallest s >= 0 with
 * oracle bin(s) >= b.  bin(s) is monotone while hypot(s) is finite (checked exhaustively by
 * oracle/tools/pm_check.c); thr[nb] = smallest s whose hypot overflows float. */
void fosphor_amd::build_thresholds(double *thr, int nb, float hs, float ho)
{
	/* largest s with finite (float)sqrt(s) */
	uint64_t lo = 0, hi = fpm_d2u(1.0e80);
	while (hi - lo > 1) {
		uint64_t mid = lo + (hi - lo) / 2;
		if (isinf(fpm_hypot_from_sqmag(fpm_u2d(mid)))) hi = mid; else lo = mid;
	}
	const uint64_t s_inf = hi;
	thr[0] = -1.0;
	thr[nb] = fpm_u2d(s_inf);
	for (int b = 1; b < nb; b++) {
		/* invariant: bin(lo) < b <= bin(hi) on [0, s_inf) */
		if (fpm_bin_from_sqmag(fpm_u2d(s_inf - 1), hs, ho, nb) < b) {
			thr[b] = fpm_u2d(s_inf);	/* unreachable bin */
			continue;
		}
		lo = 0; hi = s_inf - 1;
		while (hi - lo > 1) {
			uint64_t mid = lo + (hi - lo) / 2;
			if (fpm_bin_from_sqmag(fpm_u2d(mid), hs, ho, nb) >= b) hi = mid; else lo = mid;
		}
		thr[b] = fpm_u2d(hi);
	}
}

extern "C" int fosphor_amd_host_thresholds(int n_bins, float histo_scale, float histo_offset, double *out)
{
	if (!out || n_bins < 2 || n_bins > 65536)
		return -EINVAL;
	build_thresholds(out, n_bins, histo_scale, histo_offset);
	return 0;
}

extern "C" int fosphor_amd_host_twiddle_count(void) { return build_twiddles(NULL, 10, NULL); }

extern "C" int fosphor_amd_host_twiddles(float *out)
{
	if (!out)
		return -EINVAL;
	build_twiddles((float2 *)out, 10, NULL);
	return 0;
}
