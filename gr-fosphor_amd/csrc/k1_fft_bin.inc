/*
 * k1_fft_bin.inc -- the 1024-point kernel, one wave per spectrum (8-bit bin indices).  A template over the IQ format: IQ is one of the tags
 * of "IQ formats" in fosphor_kernels.hip, which includes this file once; `iq` below is K1Params::iq as that format's samples and
 * IQ::load_iq16 the only place where the formats differ.
 */
template <typename IQ, bool WRITE_FFT, bool NB256 = false>	/* NB256: 256 bins -- the saturating conversion of the bin byte IS the clamp at n_bins - 1 */
__global__ __launch_bounds__(256, kK1WavesPerSimd)
void k1_fft_bin(const K1Params p)
{
	__shared__ v2f   lds[4][kN];			/* 8 KiB exchange slab per wave */
	__shared__ v2f   tw4_tab[512];			/* pass-4 twiddles, shared by the block */
	__shared__ float win_tab[kN];			/* window, shared by the block */
	/* exact-bin thresholds (n_bins <= 256 in this kernel): the rare path that consults them would otherwise wait for its two table
	 * loads BEHIND the next spectrum's IQ, already requested from HBM -- loads return in order */
	__shared__ double thr_tab[264];

	const int lane   = threadIdx.x & 63;
	const int wv     = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);	/* tile, spectrum index, row predicate: SGPRs */
	const int ntiles = p.total / p.tile;
	const int stride = gridDim.x * 4;		/* waves in the grid */
#if K1_TIMING
	const long long t_wave_start = wall_clock64();	/* 100 MHz, common to all CUs */
#endif
	int tile = blockIdx.x * 4 + wv;
	const v2f *twg = reinterpret_cast<const v2f *>(p.tw);
	const typename IQ::elem *iq = reinterpret_cast<const typename IQ::elem *>(p.iq);

	for (int i = threadIdx.x; i < kN; i += 256)
		win_tab[i] = p.win[i];
	for (int i = threadIdx.x; i < 512; i += 256)
		tw4_tab[i] = twg[kTw4Off + i];
	for (int i = threadIdx.x; i <= p.n_bins && i < 264; i += 256)
		thr_tab[i] = p.thr[i];
	__syncthreads();				/* the only block-wide barrier */

	if (tile >= ntiles)
		return;					/* whole wave leaves */

	v2f *buf = lds[wv];

	/* ---- per-lane constants, loaded once per wave -------------------------- */
	v2f tw2[7];
	v2f tw3[7];
#pragma unroll
	for (int n = 0; n < 7; n++) {
		tw2[n] = twg[kTw2Off + (lane & 7) * 7 + n];	/* k = i & 7  (both virtual items) */
		tw3[n] = twg[kTw3Off + lane * 7 + n];		/* k = i & 63 = lane               */
	}
	const v2f s12 = { F_SQRT_1_2, F_SQRT_1_2 };

	/* ---- swizzled LDS addressing -------------------------------------------
	 * element e lives at phys(e) = e ^ ((e >> 3) & 15): every access below is
	 * bank-conflict free for ds_read_b64 (32-lane groups, 64 banks) and
	 * ds_write_b64 (16-lane groups, 32 banks).  The closed forms per access
	 * pattern are derived in DESIGN_HISTORY.md ("LDS exchange").                    */
	const int rd_even = lane ^ ((lane >> 3) & 7);		/* e = lane + 64m, m even */
	const int rd_odd  = rd_even ^ 8;			/*                 m odd  */
	const int st1     = (8 * lane) ^ (lane & 15);		/* pass 1: e = 8i + jj, i = lane (+64v)   */
	const int st1a    = (16 * lane) ^ ((2 * lane) & 15);		/* pass 1, i = 2 lane     */
	const int st1b    = (16 * lane + 8) ^ ((2 * lane + 1) & 15);	/* pass 1, i = 2 lane + 1 */
	(void)st1; (void)st1a; (void)st1b;
	const int st2     = ((64 * (lane >> 3)) + (lane & 7)) ^ (lane & 8);	/* pass 2: e = 64(i>>3)+(i&7)+8jj */

	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float vmax_init = -1000.0f / F_HALF_LOG10_2;	/* display.cl:91, in log2 units */

	v2f xn[16];
	IQ::load_iq16(xn, iq + (size_t)tile * p.tile * p.hop + K1_LANE_SRC(lane));
#if K1_TIMING
	long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	long long tprev = __builtin_readcyclecounter();
#endif

	/* persistent wave: tiles tile, tile + stride, ... (per-lane constants stay in registers) */
	for (; tile < ntiles; tile += stride) {
	const int t0 = tile * p.tile;

	/* live partial and running max of this tile, in log2(|X|^2) units */
	float live[16], vmax[16];
#pragma unroll
	for (int m = 0; m < 16; m++) {
		live[m] = 0.0f;
		vmax[m] = vmax_init;
	}

	/* The bin dwords of a quad of spectra are stored one window multiply LATER than they are complete: the wait for the prefetched IQ at
	 * the top of a spectrum is an s_waitcnt vmcnt(0) (the number of stores behind the loads varies, so the compiler cannot count them out),
	 * and stores issued behind those loads -- at the end of the previous spectrum -- made every fourth spectrum wait for its own stores'
	 * acknowledgements.  Stores issued AHEAD of the next prefetch are older than the loads the wave waits for next. */
	uint32_t pack[16];
#pragma unroll
	for (int m = 0; m < 16; m++)
		pack[m] = 0;
	int pend_row = -1;			/* row of p.bins the bytes in pack belong to, or -1 (uniform) */
	auto flush_pack = [&]() {
		uint32_t *dst = p.bins + (size_t)pend_row * kN + lane;
#pragma unroll
		for (int m = 0; m < 16; m++)
			dst[64 * m] = pack[m];
#pragma unroll
		for (int m = 0; m < 16; m++)
			pack[m] = 0;
		pend_row = -1;
	};

	for (int g0 = 0; g0 < p.tile; g0 += 4) {
#pragma unroll 1
		for (int u = 0; u < 4; u++) {
			const int t = t0 + g0 + u;
			v2f x[16];

			K1_STAMP(7);		/* loop overhead + stores of the previous iteration */
			/* window (fft.cl:415-417); taps fetched as pairs */
#pragma unroll
			for (int k = 0; k < 8; k++) {	/* x[2k], x[2k+1] = elements 2L + 128k, 2L + 1 + 128k */
				const v2f w = *reinterpret_cast<const v2f *>(&win_tab[2 * lane + 128 * k]);
				x[2 * k]     = mul_bcast_lo(xn[2 * k], w);
				x[2 * k + 1] = mul_bcast_hi(xn[2 * k + 1], w);
			}

			if (u == 0 && pend_row >= 0)
				flush_pack();		/* the previous quad's bin dwords: behind the wait above, ahead of the prefetch below */
			/* prefetch the next spectrum this wave will process */
			{
				const bool last = (g0 + u + 1 == p.tile);
				const int t_next = last ? (tile + stride) * p.tile : t + 1;
				if (!last || tile + stride < ntiles)
					IQ::load_iq16(xn, iq + (size_t)t_next * p.hop + K1_LANE_SRC(lane));
			}

			K1_STAMP(0);		/* window (includes waiting for the prefetched IQ) + prefetch issue */
			/* ---- pass 1: radix 8, p = 1, no twiddle (fft.cl:419-420) --------
			 * This lane is virtual work-items i = 2L + v (elements i + 128j = x[2j + v], as the 16-byte
			 * loads deliver them).  Item i stores its outputs at e = 8i + jj; which lane runs which
			 * item is free. */
#pragma unroll
			for (int v = 0; v < 2; v++) {
				v2f r[8];
#pragma unroll
				for (int j = 0; j < 8; j++)
					r[j] = x[v + 2 * j];
				dft8(r, s12);
#pragma unroll
				for (int jj = 0; jj < 8; jj++)
					buf[(v ? st1b : st1a) ^ jj] = r[R8_PERM(jj)];
			}
			wave_lds_sync();
#pragma unroll
			for (int m = 0; m < 16; m++)
				x[m] = buf[((m & 1) ? rd_odd : rd_even) + 64 * m];
			wave_lds_sync();

			K1_STAMP(1);		/* pass 1 + exchange */
			/* ---- pass 2: radix 8, p = 8 (fft.cl:422-423) ------------------- */
#pragma unroll
			for (int v = 0; v < 2; v++) {
				v2f r[8];
				{
					v2f in7[7], out7[7];
#pragma unroll
					for (int j = 1; j < 8; j++)
						in7[j - 1] = x[v + 2 * j];
					c_mul_n<7>(out7, in7, tw2);
					r[0] = x[v];
#pragma unroll
					for (int j = 1; j < 8; j++)
						r[j] = out7[j - 1];
				}
				dft8(r, s12);
#pragma unroll
				for (int jj = 0; jj < 8; jj++)
					buf[(st2 ^ (9 * jj)) + 512 * v] = r[R8_PERM(jj)];
			}
			wave_lds_sync();
#pragma unroll
			for (int m = 0; m < 16; m++)
				x[m] = buf[((m & 1) ? rd_odd : rd_even) + 64 * m];
			wave_lds_sync();

			K1_STAMP(2);		/* pass 2 + exchange */
			/* ---- pass 3: radix 8, p = 64 (fft.cl:425-426) ------------------
			 * Virtual item i = lane + 64v stores its outputs at e = 512v + lane + 64jj, and the
			 * pass-4 butterflies of this lane read exactly e = lane + 64m: with both items of a
			 * pair in the same lane the third exchange is the identity x[jj + 8v] = out_v[jj] --
			 * no LDS round trip (fft.cl:347-349 + 435-438 collapse to register renaming). */
			{
				v2f y[16];
#pragma unroll
				for (int v = 0; v < 2; v++) {
					v2f r[8];
					{
						v2f in7[7], out7[7];
#pragma unroll
						for (int j = 1; j < 8; j++)
							in7[j - 1] = x[v + 2 * j];
						c_mul_n<7>(out7, in7, tw3);
						r[0] = x[v];
#pragma unroll
						for (int j = 1; j < 8; j++)
							r[j] = out7[j - 1];
					}
					dft8(r, s12);
#pragma unroll
					for (int jj = 0; jj < 8; jj++)
						y[jj + 8 * v] = r[R8_PERM(jj)];
				}
#pragma unroll
				for (int m = 0; m < 16; m++)
					x[m] = y[m];
			}

			K1_STAMP(3);		/* pass 3 + exchange */
			/* ---- pass 4: radix 2, p = 512 (fft.cl:428-458) ------------------
			 * butterfly on elements (j, j + 512), j = lane + 64c, twiddle k = j.
			 * Results: X[j] -> x[c], X[j + 512] -> x[c + 8], i.e. column lane + 64m. */
			{
				v2f in8[8], w8[8], out8[8];
#pragma unroll
				for (int c = 0; c < 8; c++) { in8[c] = x[c + 8]; w8[c] = tw4_tab[lane + 64 * c]; }	/* k = lane + 64c */
				c_mul_n<8>(out8, in8, w8);
#pragma unroll
				for (int c = 0; c < 8; c++) {
					v2f a = x[c];
					v2f b = out8[c];
					DFT2(a, b);
					x[c] = a;
					x[c + 8] = b;
				}
			}

			K1_STAMP(4);		/* pass 4 */
			if (WRITE_FFT) {
#pragma unroll
				for (int m = 0; m < 16; m++)
					reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * kN + lane + 64 * m] = x[m];
			}

			/* ---- epilogue: log-power, exact bin (display.cl:136,161-168) ---- */
			float    l2[16];
			uint32_t amb = 0;
			const float top = (float)(bk.nb - 1);
#pragma unroll
			for (int m = 0; m < 16; m++) {
				uint32_t ab;
				const float r = bin_fast(x[m].x, x[m].y, bk, &l2[m], &ab);
				amb = amb > ab ? amb : ab;			/* v_max_u32: NaN / inf propagate */
				pack[m] = NB256 ? __builtin_amdgcn_cvt_pk_u8_f32(r, (uint32_t)u, pack[m]) : pack_bin(r, top, (uint32_t)u, pack[m]);
			}
			if (amb > __float_as_uint(bk.amb)) {
				/* rare (a few % of spectra have one such sample): find the samples, decide them
				 * against the exact thresholds, patch their bin byte and log-power */
#pragma unroll
				for (int m = 0; m < 16; m++) {
					const float v = __builtin_fmaf(bk.A, l2[m], bk.C);
					const float r = __builtin_rintf(v);
					const float a = __builtin_fmaf(__builtin_fabsf(l2[m]), bk.kappa, __builtin_fabsf(v - r));
					if (!(a <= bk.amb)) {
						const int guess = (int)__builtin_amdgcn_fmed3f(r, 0.0f, top);
						float nl2;
						const uint32_t nbn = bin_exact(x[m].x, x[m].y, l2[m], guess,
						                               (const __attribute__((address_space(3))) double *)thr_tab, bk.nb, &nl2);
						pack[m] = (pack[m] & ~(0xffu << (8 * u))) | (nbn << (8 * u));
						l2[m] = nl2;
					}
				}
			}

#pragma unroll
			for (int m = 0; m < 16; m++) {
				/* Horner form of display.cl:149-150, in place (v_fma with the accumulator as destination:
				 * the compiler's v_fmac into the dying l2 register costs a v_mov per column) */
				asm("v_fma_f32 %0, %0, %1, %2" : "+v"(live[m]) : "s"(p.w), "v"(l2[m]));
				vmax[m] = max_f32(vmax[m], l2[m]);		/* display.cl:139 */
			}
			if (t >= p.wf_first) {				/* uniform: one scalar branch */
				float *wf_row = p.wf + (size_t)((p.wf_pos0 + t) & p.wf_mask) * kN + lane;
#pragma unroll
				for (int m = 0; m < 16; m++)
					wf_row[64 * m] = l2[m] * F_HALF_LOG10_2;	/* display.cl:142-146 */
			}
			K1_STAMP(6);		/* epilogue */
		}

		K1_STAMP(5);			/* 4th epilogue (the first three land in 7) */
		/* 4 spectra x 1 column per dword, coalesced 256 B per instruction: stored at the top of the next quad (or below) */
		pend_row = (t0 + g0) >> 2;
	}
	if (pend_row >= 0)
		flush_pack();

	/* leave the log2 domain: pwr = log10|X| = l2 * log10(2)/2; an untouched max is exactly -1000 */
	float2 *pp = p.partial + (size_t)tile * kN + lane;
#pragma unroll
	for (int m = 0; m < 16; m++)
		pp[64 * m] = make_float2(live[m] * F_HALF_LOG10_2,
		                         (vmax[m] == vmax_init) ? -1000.0f : vmax[m] * F_HALF_LOG10_2);
	}	/* tile loop */
#if K1_TIMING
	if (p.dbg && lane == 0) {
		const int w = blockIdx.x * 4 + wv;
		for (int i = 0; i < 8; i++)
			p.dbg[w * 8 + i] = tacc[i];
		/* wave lifetime on the common clock replaces the two near-empty phase slots */
		p.dbg[w * 8 + 3] = t_wave_start;
		p.dbg[w * 8 + 5] = wall_clock64();
	}
#endif
}
