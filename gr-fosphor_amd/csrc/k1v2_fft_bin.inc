/*
 * k1v2_fft_bin.inc -- the 1024-point kernel, two waves per spectrum.  A template over the IQ format: IQ is one of the tags of "IQ formats" in
 * fosphor_kernels.hip, which includes this file once; `iq` below is K1Params::iq as that format's samples and IQ::load_iq8 the only
 * place where the formats differ.
 */
template <typename IQ, bool WRITE_FFT>
__global__ __launch_bounds__(128, kK1v2WavesPerSimd)
void k1v2_fft_bin(const K1Params p)
{
	__shared__ v2f   buf[kN];			/* 8 KiB exchange slab of the work-group's spectrum */
	__shared__ v2f   tw4_tab[512];
	__shared__ float win_tab[kN];

	const int lane   = threadIdx.x & 63;
	const int w      = threadIdx.x >> 6;		/* wave = virtual-item half */
	const int i0     = threadIdx.x;			/* virtual work-item i = lane + 64w */
	const int ntiles = p.total / p.tile;
	const int stride = gridDim.x;
	int tile = blockIdx.x;
	const v2f *twg = reinterpret_cast<const v2f *>(p.tw);
	const typename IQ::elem *iq = reinterpret_cast<const typename IQ::elem *>(p.iq);

	for (int i = threadIdx.x; i < kN; i += 128)
		win_tab[i] = p.win[i];
	for (int i = threadIdx.x; i < 512; i += 128)
		tw4_tab[i] = twg[kTw4Off + i];
	__syncthreads();

	/* per-lane twiddles: k = i & 7 and k = i & 63 do not depend on w */
	v2f tw2[7];
	v2f tw3[7];
#pragma unroll
	for (int n = 0; n < 7; n++) {
		tw2[n] = twg[kTw2Off + (lane & 7) * 7 + n];
		tw3[n] = twg[kTw3Off + lane * 7 + n];
	}
	const v2f s12 = { F_SQRT_1_2, F_SQRT_1_2 };

	/* swizzled addressing, as in k1_fft_bin with v = w */
	const int rd_even = lane ^ ((lane >> 3) & 7);
	const int rd_w    = w ? (rd_even ^ 8) : rd_even;		/* e = lane + 64(w + 2j): parity of m is w */
	const int st1     = ((8 * lane) ^ (lane & 15)) + 512 * w;
	const int st2     = (((64 * (lane >> 3)) + (lane & 7)) ^ (lane & 8)) + 512 * w;
	const int st3     = 512 * w;					/* + (odd jj ? rd_odd : rd_even) + 64 jj */
	const int rd_odd  = rd_even ^ 8;

	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float vmax_init = -1000.0f / F_HALF_LOG10_2;
	const float top = (float)(bk.nb - 1);

	v2f xn[8];
	if (tile < ntiles)
		IQ::load_iq8(xn, iq + (size_t)tile * p.tile * p.hop + i0);

	for (; tile < ntiles; tile += stride) {		/* uniform over the work-group */
	const int t0 = tile * p.tile;

	float live[8], vmax[8];
#pragma unroll
	for (int q = 0; q < 8; q++) {
		live[q] = 0.0f;
		vmax[q] = vmax_init;
	}

	for (int g0 = 0; g0 < p.tile; g0 += 4) {
		uint32_t pack[8];
#pragma unroll
		for (int q = 0; q < 8; q++)
			pack[q] = 0;

#pragma unroll 1
		for (int u = 0; u < 4; u++) {
			const int t = t0 + g0 + u;
			v2f r[8];

			/* window (fft.cl:415-417) */
#pragma unroll
			for (int j = 0; j < 8; j += 2) {
				v2f ww;
				ww.x = win_tab[i0 + 128 * j];
				ww.y = win_tab[i0 + 128 * (j + 1)];
				r[j]     = mul_bcast_lo(xn[j], ww);
				r[j + 1] = mul_bcast_hi(xn[j + 1], ww);
			}
			{	/* prefetch the next spectrum of this work-group */
				const bool last = (g0 + u + 1 == p.tile);
				const int t_next = last ? (tile + stride) * p.tile : t + 1;
				if (!last || tile + stride < ntiles)
					IQ::load_iq8(xn, iq + (size_t)t_next * p.hop + i0);
			}

			/* pass 1 (fft.cl:419-420) */
			dft8(r, s12);
#pragma unroll
			for (int jj = 0; jj < 8; jj++)
				buf[st1 ^ jj] = r[R8_PERM(jj)];
			__syncthreads();
#pragma unroll
			for (int j = 0; j < 8; j++)
				r[j] = buf[rd_w + 64 * (w + 2 * j)];
			__syncthreads();

			/* pass 2 (fft.cl:422-423) */
#pragma unroll
			for (int j = 1; j < 8; j++)
				r[j] = c_mul(r[j], tw2[j - 1]);
			dft8(r, s12);
#pragma unroll
			for (int jj = 0; jj < 8; jj++)
				buf[st2 ^ (9 * jj)] = r[R8_PERM(jj)];
			__syncthreads();
#pragma unroll
			for (int j = 0; j < 8; j++)
				r[j] = buf[rd_w + 64 * (w + 2 * j)];
			__syncthreads();

			/* pass 3 (fft.cl:425-426) */
#pragma unroll
			for (int j = 1; j < 8; j++)
				r[j] = c_mul(r[j], tw3[j - 1]);
			dft8(r, s12);
#pragma unroll
			for (int jj = 0; jj < 8; jj++)
				buf[st3 + ((jj & 1) ? rd_odd : rd_even) + 64 * jj] = r[R8_PERM(jj)];
			__syncthreads();

			/* pass 4 (fft.cl:428-458): butterflies c = 4w + q on elements (j, j+512), j = lane + 64c.
			 * x[q] = X[lane + 64(4w+q)], x[q+4] = X[lane + 64(8+4w+q)] */
			v2f x[8];
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const int c = 4 * w + q;		/* parity of c is parity of q */
				v2f a = buf[((q & 1) ? rd_odd : rd_even) + 64 * c];
				v2f b = buf[((q & 1) ? rd_odd : rd_even) + 64 * (c + 8)];
				b = c_mul(b, tw4_tab[lane + 64 * c]);
				DFT2(a, b);
				x[q] = a;
				x[q + 4] = b;
			}
			__syncthreads();		/* the slab is rewritten by the next spectrum's pass 1 */

			if (WRITE_FFT) {
#pragma unroll
				for (int q = 0; q < 4; q++) {
					reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * kN + lane + 64 * (4 * w + q)] = x[q];
					reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * kN + lane + 64 * (8 + 4 * w + q)] = x[q + 4];
				}
			}

			/* epilogue (display.cl:136,161-168), as in k1_fft_bin */
			float    l2[8];
			uint32_t amb = 0;
#pragma unroll
			for (int q = 0; q < 8; q++) {
				uint32_t ab;
				const float rr = bin_fast(x[q].x, x[q].y, bk, &l2[q], &ab);
				amb = amb > ab ? amb : ab;
				pack[q] = pack_bin(rr, top, (uint32_t)u, pack[q]);
			}
			if (amb > __float_as_uint(bk.amb)) {
#pragma unroll
				for (int q = 0; q < 8; q++) {
					const float v = __builtin_fmaf(bk.A, l2[q], bk.C);
					const float rr = __builtin_rintf(v);
					const float a = __builtin_fmaf(__builtin_fabsf(l2[q]), bk.kappa, __builtin_fabsf(v - rr));
					if (!(a <= bk.amb)) {
						const int guess = (int)__builtin_amdgcn_fmed3f(rr, 0.0f, top);
						float nl2;
						const uint32_t nbn = bin_exact(x[q].x, x[q].y, l2[q], guess, ThrScalar{ bk.thr }, bk.nb, &nl2);
						pack[q] = (pack[q] & ~(0xffu << (8 * u))) | (nbn << (8 * u));
						l2[q] = nl2;
					}
				}
			}

			const bool store_row = (t >= p.wf_first);
			float *wf_row = p.wf + (size_t)((p.wf_pos0 + t) & p.wf_mask) * kN + lane + 256 * w;
#pragma unroll
			for (int q = 0; q < 8; q++) {
				live[q] = __builtin_fmaf(live[q], p.w, l2[q]);
				vmax[q] = max_f32(vmax[q], l2[q]);
				if (store_row)
					wf_row[64 * (q & 3) + 512 * (q >> 2)] = l2[q] * F_HALF_LOG10_2;
			}
		}

		uint32_t *dst = p.bins + (size_t)((t0 + g0) >> 2) * kN + lane + 256 * w;
#pragma unroll
		for (int q = 0; q < 8; q++)
			dst[64 * (q & 3) + 512 * (q >> 2)] = pack[q];
	}

	float2 *pp = p.partial + (size_t)tile * kN + lane + 256 * w;
#pragma unroll
	for (int q = 0; q < 8; q++)
		pp[64 * (q & 3) + 512 * (q >> 2)] = make_float2(live[q] * F_HALF_LOG10_2,
			(vmax[q] == vmax_init) ? -1000.0f : vmax[q] * F_HALF_LOG10_2);
	}	/* tile loop */
}
