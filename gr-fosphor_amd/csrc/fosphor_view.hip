/*
 * fosphor_view.hip -- zoomed, display-width views of the plain buffers (include/fosphor_amd_view.h)
 *
 * One kernel, k_view, reduces a window of a [rows][N] plane (waterfall ring, histogram) or of the spectrum's vertex lines to
 * out_rows x width pixels and can colour them in the same launch.  HBM-read-bound: it reads the window once, 16 B per lane along the
 * contiguous column direction, and writes a picture of display size.
 *
 * A work-group owns `ppt` consecutive pixels of a picture row and the shifted columns [c0, c1) their spans cover.
 *   phase 1  lane t loads the aligned group of 4 columns a + 4t .. a + 4t + 3 (a = c0 rounded down to 4; an aligned group of shifted
 *            columns is an aligned, contiguous group of memory columns on either side of the N/2 wrap, because N/2 is a multiple of
 *            4) of every source row of kRows picture rows at once, reduces over the rows in registers and leaves one strip of kChunk
 *            column values per picture row in LDS; columns outside [c0, c1) hold the detector's identity (NaN for fmaxf, 0 for the sum)
 *   phase 2  2^tlog lanes share a pixel: each reduces its part of the pixel's span from the strip, xor-shuffles combine them, lane 0
 *            applies the reciprocal (AVERAGE), looks the colour up and stores
 * Forms, chosen on the host from the shape alone:
 *   tiled  ppt is sized so that [a, c1) fits one strip (kChunk columns): one read, phase 2 indexes the strip by the span
 *   wide   a pixel's span is longer than a strip (ppt = 1): the lanes accumulate over the strips of the span in registers, and phase 2
 *          reduces the whole strip with 64 lanes
 * No global atomics; the cross-lane part is registers + LDS.
 */
#include <errno.h>
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "fosphor_ring.h"
#include "../../include/fosphor_amd_cmap.h"
#include "../../include/fosphor_amd_view.h"
#include "fosphor_cmap_dev.h"

namespace {

using namespace ring_pass;		/* ring_row, the host side of a call */

static_assert(FOSPHOR_AMD_VIEW_STATS <= FOSPHOR_COUNTERS_MAX, "the instance holds the counters");
constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 4;	/* columns of one strip: one 16-byte load per lane */
constexpr int kRows = 4;		/* picture rows a work-group reduces at once (independent loads in flight per lane) */
constexpr int kTileCols = kChunk - 8;	/* columns the pixels of a tile may nominally cover: + 1 or 2 for the floors of the
					 * mapping + 3 for the alignment of `a` stays within kChunk */

struct ViewParams {
	const float *src;		/* plane: [..][n] unshifted columns; line: float2[n] vertices, already shifted */
	float       *dst_f;		/* [out_rows][width] or NULL */
	uint32_t    *dst_rgba;		/* [out_rows][width] or NULL */
	CmapLut      lut;		/* read when dst_rgba is set */
	int   n;			/* FFT length */
	int   first_bin, n_cols, width;
	int   src_rows, out_rows;	/* time mapping (both 1 for a line, both n_bins for the histogram) */
	int   row_base, row_mask;	/* memory row of source row j: (row_base - j) & row_mask */
	int   ppt;			/* pixels per tile */
	int   tlog;			/* log2 of the lanes that share a pixel in phase 2 */
	int   wide;
};

/* [lo, hi) of n_src for output index p of n_out (fosphor_amd_view_span).  The column form needs p * n_src < 2^32:
 * p < n_out <= 65536 and n_src <= N <= 65536, and (p + 1) * n_src is only formed for p + 1 < n_out. */
__device__ __forceinline__ void span_cols(uint32_t n_src, uint32_t n_out, uint32_t p, int &lo, int &hi)
{
	const uint32_t l = (p * n_src) / n_out;
	const uint32_t h = (p + 1 == n_out) ? n_src : ((p + 1) * n_src) / n_out;
	lo = (int)l;
	hi = (int)(h > l + 1 ? h : l + 1);
}

__device__ __forceinline__ void span_rows(int n_src, int n_out, int p, int &lo, int &hi)
{
	const long long l = ((long long)p * n_src) / n_out;
	const long long h = ((long long)(p + 1) * n_src) / n_out;
	lo = (int)l;
	hi = (int)(h > l + 1 ? h : l + 1);
}

template <int DET>
__device__ __forceinline__ float det_identity()
{
	return DET == FOSPHOR_AMD_DET_PEAK ? __builtin_nanf("") : 0.0f;
}

template <int DET>
__device__ __forceinline__ float det_op(float a, float b)
{
	return DET == FOSPHOR_AMD_DET_PEAK ? fmaxf(a, b) : a + b;
}

template <int DET, bool LINE>
__global__ __launch_bounds__(kThreads)
void k_view(const ViewParams p)
{
	extern __shared__ uint32_t smem[];
	float    *strip = reinterpret_cast<float *>(smem);		/* [kRows][kChunk] */
	int      *s_len = reinterpret_cast<int *>(smem + kRows * kChunk);	/* [kRows] source rows of each picture row (padded to 16 B) */
	uint32_t *pal   = smem + kRows * kChunk + 4;

	const int tid = threadIdx.x;
	const float ident = det_identity<DET>();

	if (p.dst_rgba)
		cmap_stage_lds(p.lut, pal);		/* made visible by the barriers of the first row block */

	const int p0 = blockIdx.x * p.ppt;
	const int p1 = min(p0 + p.ppt, p.width);
	const int npix = p1 - p0;
	int c0, c1, dummy;
	span_cols(p.n_cols, p.width, p0, c0, dummy);
	span_cols(p.n_cols, p.width, p1 - 1, dummy, c1);
	c0 += p.first_bin; c1 += p.first_bin;
	const int a0 = c0 & ~3;

	for (int r0 = blockIdx.y * kRows; r0 < p.out_rows; r0 += gridDim.y * kRows) {
		const int nr = min(kRows, p.out_rows - r0);
		int jlo[kRows], len[kRows], maxlen = 0;
#pragma unroll
		for (int q = 0; q < kRows; q++) {
			int hi = 0;
			jlo[q] = 0;
			if (q < nr)
				span_rows(p.src_rows, p.out_rows, r0 + q, jlo[q], hi);
			len[q] = hi - jlo[q];
			maxlen = max(maxlen, len[q]);
		}

		/* phase 1 */
		float4 acc[kRows];
#pragma unroll
		for (int q = 0; q < kRows; q++)
			acc[q] = make_float4(ident, ident, ident, ident);
		for (int a = a0; a < c1; a += kChunk) {
			const int s = a + 4 * tid;
			if (s >= c1)
				continue;
			const bool m0 = s >= c0, m1 = s + 1 >= c0 && s + 1 < c1, m2 = s + 2 >= c0 && s + 2 < c1, m3 = s + 3 >= c0 && s + 3 < c1;
			const int col = LINE ? s : (s ^ (p.n >> 1));
			for (int j = 0; j < maxlen; j++) {
#pragma unroll
				for (int q = 0; q < kRows; q++) {
					if (j < len[q]) {
						float4 v;
						if (LINE) {
							/* vertices (x, y): the y of 4 consecutive ones out of two 16-byte loads */
							const float4 *b = reinterpret_cast<const float4 *>(p.src + 2 * (size_t)col);
							const float4 u0 = b[0], u1 = b[1];
							v = make_float4(u0.y, u0.w, u1.y, u1.w);
						} else {
							const int row = ring_row(p.row_base, p.row_mask, jlo[q] + j);
							v = *reinterpret_cast<const float4 *>(p.src + (size_t)row * p.n + col);
						}
						acc[q].x = det_op<DET>(acc[q].x, m0 ? v.x : ident);
						acc[q].y = det_op<DET>(acc[q].y, m1 ? v.y : ident);
						acc[q].z = det_op<DET>(acc[q].z, m2 ? v.z : ident);
						acc[q].w = det_op<DET>(acc[q].w, m3 ? v.w : ident);
					}
				}
			}
		}
		__syncthreads();			/* the strips' readers of the previous row block are done */
#pragma unroll
		for (int q = 0; q < kRows; q++) {
			*reinterpret_cast<float4 *>(strip + q * kChunk + 4 * tid) = acc[q];
			if (tid == q)
				s_len[q] = len[q];
		}
		__syncthreads();

		/* phase 2 */
		const int T = 1 << p.tlog, lane = tid & (T - 1), grp = tid >> p.tlog, ngrp = kThreads >> p.tlog;
		const int items = nr * npix;
		for (int it = grp; it < items; it += ngrp) {	/* the lanes of a group run this loop together */
			const int q = it / npix, px = p0 + (it - q * npix);
			int lo, hi;
			span_cols(p.n_cols, p.width, px, lo, hi);
			const int b = p.wide ? 0 : p.first_bin + lo - a0;
			const int e = p.wide ? kChunk : b + (hi - lo);
			const float *row = strip + q * kChunk;
			float v = ident;
			for (int i = b + lane; i < e; i += T)
				v = det_op<DET>(v, row[i]);
			for (int m = T >> 1; m; m >>= 1)
				v = det_op<DET>(v, __shfl_xor(v, m));
			if (lane == 0) {
				if (DET == FOSPHOR_AMD_DET_AVERAGE)
					v = v * (1.0f / (float)((long long)(hi - lo) * s_len[q]));
				const size_t o = (size_t)(r0 + q) * p.width + px;
				if (p.dst_f)
					p.dst_f[o] = v;
				if (p.dst_rgba)
					p.dst_rgba[o] = lookup(v, p.lut, pal);
			}
		}
	}
}

/* Shape -> form and launch geometry.  The form is a function of (n_cols, width) alone. */
int launch_view(struct fosphor *self, hipStream_t st, ViewParams p, int detector, bool line)
{
	long long *forms = fosphor_amd_priv_counters(self, FOSPHOR_COUNTERS_VIEW);
	const long long span = ((long long)p.n_cols + p.width - 1) / p.width;	/* longest column span, cells (1 when magnifying) */

	p.ppt = p.n_cols <= p.width ? kTileCols : (int)(((long long)kTileCols * p.width) / p.n_cols);
	p.wide = p.ppt < 1;
	if (p.wide) {
		p.ppt = 1;
		p.tlog = 6;
	} else {
		p.tlog = 0;			/* about 4 cells per lane from spans of 8 cells on, 64 lanes at the most */
		if (span >= 8)
			while (p.tlog < 6 && (4LL << p.tlog) < span)
				p.tlog++;
	}
	const int tiles = (p.width + p.ppt - 1) / p.ppt;
	const int row_blocks = (p.out_rows + kRows - 1) / kRows;
	int gy = 8192 / tiles;			/* a few thousand work-groups; the rest of the rows by grid stride */
	if (gy < 1) gy = 1;
	if (gy > row_blocks) gy = row_blocks;
	const size_t lds = sizeof(uint32_t) * (kRows * kChunk + 4 + (p.dst_rgba ? p.lut.pal_n : 0));
	const dim3 grid(tiles, gy), block(kThreads);

	if (detector == FOSPHOR_AMD_DET_PEAK) {
		if (line) hipLaunchKernelGGL((k_view<FOSPHOR_AMD_DET_PEAK, true>), grid, block, lds, st, p);
		else      hipLaunchKernelGGL((k_view<FOSPHOR_AMD_DET_PEAK, false>), grid, block, lds, st, p);
	} else {
		if (line) hipLaunchKernelGGL((k_view<FOSPHOR_AMD_DET_AVERAGE, true>), grid, block, lds, st, p);
		else      hipLaunchKernelGGL((k_view<FOSPHOR_AMD_DET_AVERAGE, false>), grid, block, lds, st, p);
	}
	return launch_counted(forms, line ? FOSPHOR_AMD_VIEW_LINES
	                                  : p.wide ? FOSPHOR_AMD_VIEW_WIDE : (p.tlog ? FOSPHOR_AMD_VIEW_TILED_LANES : FOSPHOR_AMD_VIEW_TILED));
}

bool color_ok(const struct fosphor_amd_view_color &c)
{
	return !c.palette || (c.n >= 2 && c.n <= kPalMax);
}

} // namespace

extern "C" int fosphor_amd_view_span(int n_src, int n_out, int p, int *lo, int *hi)
{
	if (!lo || !hi || n_src < 1 || n_out < 1 || p < 0 || p >= n_out)
		return -EINVAL;
	const long long l = ((long long)p * n_src) / n_out;
	const long long h = ((long long)(p + 1) * n_src) / n_out;
	*lo = (int)l;
	*hi = (int)(h > l + 1 ? h : l + 1);
	return 0;
}

extern "C" int fosphor_amd_view_from_render(int fft_len, int wf_rows, const struct fosphor_render *r,
                                            int width, int wf_out_rows, struct fosphor_amd_view *v)
{
	if (!r || !v || fft_len < 1 || wf_rows < 1 || width < 1 || width > 65536 || wf_out_rows < 1 || wf_out_rows > wf_rows)
		return -EINVAL;
	const double fc = r->freq_center, fs = r->freq_span, ws = r->wf_span;
	if (!(fs > 0.0 && fs <= 1.0) || !(ws > 0.0 && ws <= 1.0) || !(fc > 0.0 && fc < 1.0))
		return -EINVAL;
	const double n = fft_len;
	double first = floor(0.5 + n * (fc - fs / 2.0));	/* left edge of the quad's texture window, gl.c:396-400 */
	if (first < 0.0) first = 0.0;
	if (first > n - 1.0) first = n - 1.0;
	long cols = lrint(n * fs);
	if (cols < 1) cols = 1;
	if (cols > fft_len - (long)first) cols = fft_len - (long)first;
	long rows = lrint((double)wf_rows * ws);
	if (rows < 1) rows = 1;
	if (rows > wf_rows) rows = wf_rows;
	v->first_bin = (int)first;
	v->n_cols = (int)cols;
	v->width = width;
	v->wf_src_rows = (int)rows;
	v->wf_out_rows = wf_out_rows;
	v->detector = FOSPHOR_AMD_DET_PEAK;
	return 0;
}

extern "C" int fosphor_amd_view_stats(struct fosphor *self, long long stats[FOSPHOR_AMD_VIEW_STATS])
{
	return fosphor_amd_priv_copy_stats(self, FOSPHOR_COUNTERS_VIEW, FOSPHOR_AMD_VIEW_STATS, stats);
}

extern "C" int fosphor_amd_view(struct fosphor *self, const struct fosphor_amd_view *v, const struct fosphor_amd_view_out *out)
{
	struct fosphor_amd_buffers b;
	ViewParams p;
	hipStream_t st;
	int rv;

	if (!self || !v || !out)
		return -EINVAL;
	const bool want_wf = out->d_waterfall || out->d_waterfall_rgba;
	const bool want_histo = out->d_histogram || out->d_histogram_rgba;
	if (!want_wf && !want_histo && !out->d_live && !out->d_max)
		return -EINVAL;
	if (v->detector != FOSPHOR_AMD_DET_PEAK && v->detector != FOSPHOR_AMD_DET_AVERAGE)
		return -EINVAL;
	if ((out->d_waterfall_rgba && !color_ok(out->wf_color)) || (out->d_histogram_rgba && !color_ok(out->histo_color)))
		return -EINVAL;
	if (open(self, &b))
		return -EIO;
	if (!geometry_ok(b, 4))					/* what span_cols and the ring mask rely on */
		return -EINVAL;
	if (!window_ok(v->first_bin, v->n_cols, b.fft_len) || v->width < 1 || v->width > 65536 ||
	    v->wf_src_rows < 1 || v->wf_src_rows > b.wf_rows || v->wf_out_rows < 1 || v->wf_out_rows > b.wf_rows)
		return -EINVAL;
	st = (hipStream_t)fosphor_amd_stream(self);

	p.n = b.fft_len;
	p.first_bin = v->first_bin; p.n_cols = v->n_cols; p.width = v->width;
	p.lut.pal = NULL; p.lut.pal_n = 0; p.lut.scale = p.lut.offset = 0.0f;
	if (want_wf) {
		const struct fosphor_amd_view_color &c = out->wf_color;
		p.src = b.d_waterfall;
		p.dst_f = out->d_waterfall; p.dst_rgba = out->d_waterfall_rgba;
		p.src_rows = v->wf_src_rows; p.out_rows = v->wf_out_rows;
		const Rows ring = waterfall_rows(b);
		p.row_base = ring.base; p.row_mask = ring.mask;
		if (p.dst_rgba && (rv = fosphor_cmap_stage(self, FOSPHOR_AMD_IMG_WATERFALL, c.palette, c.n, c.use_defaults,
		                                           c.scale, c.offset, 0, &p.lut)))
			return rv;
		if ((rv = launch_view(self, st, p, v->detector, false)))
			return rv;
	}
	if (want_histo) {
		const struct fosphor_amd_view_color &c = out->histo_color;
		p.src = b.d_histogram;
		p.dst_f = out->d_histogram; p.dst_rgba = out->d_histogram_rgba;
		p.src_rows = p.out_rows = b.n_bins;		/* never resampled */
		const Rows bins = histogram_rows(b);
		p.row_base = bins.base; p.row_mask = bins.mask;
		if (p.dst_rgba && (rv = fosphor_cmap_stage(self, FOSPHOR_AMD_IMG_HISTOGRAM, c.palette, c.n, c.use_defaults,
		                                           c.scale, c.offset, 1, &p.lut)))
			return rv;
		if ((rv = launch_view(self, st, p, v->detector, false)))
			return rv;
	}
	p.dst_rgba = NULL;
	p.src_rows = p.out_rows = 1;
	p.row_base = 0; p.row_mask = 0;
	if (out->d_live) {
		p.src = b.d_spectrum;
		p.dst_f = out->d_live;
		if ((rv = launch_view(self, st, p, v->detector, true)))
			return rv;
	}
	if (out->d_max) {
		p.src = b.d_spectrum + 2 * (size_t)b.fft_len;
		p.dst_f = out->d_max;
		if ((rv = launch_view(self, st, p, v->detector, true)))
			return rv;
	}
	return drain(st, 0);
}
