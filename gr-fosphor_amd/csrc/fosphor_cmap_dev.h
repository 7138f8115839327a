/*
 * fosphor_cmap_dev.h -- the palette lookup shared by the device passes that colour
 *
 * One statement of   pixel = lookup((intensity + offset) * scale)   (include/fosphor_amd_cmap.h) for the elementwise pass
 * (fosphor_cmap.hip, k_colorize) and the view pass (fosphor_view.hip, k_view): the struct that carries a staged palette into a
 * kernel, its copy into LDS, the lookup itself, and the host step that resolves the caller's arguments into that struct.
 */
#ifndef FOSPHOR_CMAP_DEV_H
#define FOSPHOR_CMAP_DEV_H

#include <stdint.h>

#include <hip/hip_runtime.h>

struct fosphor;

constexpr int kPalMax = 4096;		/* most palette entries a pass takes (16 KiB of LDS) */
constexpr int kPalSlots = 2;		/* palettes one call can stage side by side (a view colours two pictures) */

struct CmapLut {
	const uint32_t *pal;		/* [pal_n] device */
	int   pal_n;
	float scale, offset;
};

/* Resolve (palette, n, use_defaults, scale, offset) as fosphor_amd_colorize documents them for `image` (FOSPHOR_AMD_IMG_*) and queue
 * the palette's upload into the instance's staging slot `slot` (0 .. kPalSlots - 1) on the instance's stream.  Defined in
 * fosphor_cmap.hip.  0, -EINVAL (entry count outside 2 .. kPalMax), -EIO. */
int fosphor_cmap_stage(struct fosphor *self, int image, const uint32_t *palette, int n, int use_defaults,
                       float scale, float offset, int slot, CmapLut *lut);

#ifdef __HIPCC__

/* palette -> LDS; the caller synchronises the work-group before the first lookup */
__device__ __forceinline__ void cmap_stage_lds(const CmapLut &p, uint32_t *pal)
{
	for (int i = threadIdx.x; i < p.pal_n; i += blockDim.x)
		pal[i] = p.pal[i];
}

__device__ __forceinline__ uint32_t lookup(float t, const CmapLut &p, const uint32_t *pal)
{
	const float m = (t + p.offset) * p.scale;		/* cmap_simple.glsl:44 */
	float u = m * (float)p.pal_n - 0.5f;
	u = (u != u) ? -1.0f : u;				/* NaN -> entry 0 */
	u = fminf(fmaxf(u, -1.0f), (float)p.pal_n);
	const float fl = floorf(u);
	const float f  = u - fl;
	int i0 = (int)fl, i1 = i0 + 1;
	i0 = i0 < 0 ? 0 : (i0 > p.pal_n - 1 ? p.pal_n - 1 : i0);
	i1 = i1 < 0 ? 0 : (i1 > p.pal_n - 1 ? p.pal_n - 1 : i1);
	const uint32_t a = pal[i0], b = pal[i1];
	uint32_t out = 0;
#pragma unroll
	for (int ch = 0; ch < 4; ch++) {
		const float c0 = (float)((a >> (8 * ch)) & 0xffu);
		const float c1 = (float)((b >> (8 * ch)) & 0xffu);
		const float c  = c0 + f * (c1 - c0);		/* -ffp-contract=off: mul, add */
		out |= ((uint32_t)(c + 0.5f) & 0xffu) << (8 * ch);
	}
	return out;
}

#endif /* __HIPCC__ */

#endif
