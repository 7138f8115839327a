/*
 * k1w_fft_bin.inc -- the 8192-point kernel.  A template over the IQ format: IQ is one of the tags of "IQ formats" in fosphor_kernels.hip, which
 * includes this file once.  The formats differ in what a thread holds of its sixteen rows between their request and the first pass
 * (IQ::raw q[16]) and in the four operations on it: IQ::ld_iq, IQ::request, IQ::mov, IQ::widen.
 */
template <typename IQ, int SHIFT>
__global__ __launch_bounds__(512, 2)
void k1w_fft_bin(const K1Params p)
{
	constexpr int N = 8192, TH = 512;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	/* two 64 KiB slabs; a spectrum's exchanges use A, B, A (the half one: its first 32 KiB) and the next spectrum's B, A, B */
	v2f *slab0 = reinterpret_cast<v2f *>(smem_raw);
	v2f *slab1 = slab0 + N;
	/* behind the slabs: the exact-bin thresholds (n_bins + 1 <= 513 doubles): the rare path that consults them must not wait behind the IQ
	 * in flight (a table load through the vector memory path returns in order), and while one wave is in it the other seven wait at the
	 * next barrier */
	typedef const __attribute__((address_space(3))) double *lds_cdp;
	double *thr_g = reinterpret_cast<double *>(slab0 + 2 * N);
	const lds_cdp thr_l = (lds_cdp)thr_g;

	const int th = threadIdx.x;
	const int ntiles = p.total / p.tile;
	const v2f *twg = reinterpret_cast<const v2f *>(p.tw);
	const v2f two = { 2.0f, 2.0f };
	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float vmax_init = -1000.0f / F_HALF_LOG10_2;
	const float top = (float)(bk.nb - 1);

	/* ---- per-thread constants ------------------------------------------------ */
	const int hh = th >> 8, kk = th & 255;		/* item th = kk + 256 hh of the pass p = 256 */
	const int hu = __builtin_amdgcn_readfirstlane(th >> 8);	/* = hh, as a scalar (wave-uniform: waves 0-3 / 4-7), for the whole kernel: taken inside the spectrum
								 * loop it kept th >> 8 alive in a vector register -- the one the general-hop form spilled */
	const v2f w16c = twg[p.tw_off[0]], w8c = twg[p.tw_off[0] + 1], w163c = twg[p.tw_off[0] + 2];	/* W16, W8, W16^3: the first pass */
	v2f wab[8];			/* taps of elements th + 512 j and th + 512 (j + 8): the pair of a first-pass stage-A butterfly */
	v2f tw16[8], tw256[8];		/* w^8, w^4, w^2, w^2 W8, w, w W16, w W8, w W16^3 for k = th & 15, th & 255 */
	v2f twr[8];			/* radix-2 twiddles k = kk + 256 (8 hh + c) */
#pragma unroll
	for (int j = 0; j < 8; j++) {
		wab[j] = v2f{ p.win[th + 512 * j], p.win[th + 512 * (j + 8)] };
		twr[j] = twg[p.tw_off[3] + kk + 256 * (8 * hh + j)];
	}
	for (int e = th; e <= p.n_bins && e < 520; e += TH)
		thr_g[e] = p.thr[e];
	__syncthreads();
#pragma unroll
	for (int n = 0; n < 8; n++) {
		tw16[n]  = twg[p.tw_off[1] + (th & 15) * 8 + n];
		tw256[n] = twg[p.tw_off[2] + kk * 8 + n];
	}

	/* ---- LDS addressing (8-byte elements, phys(e) = e ^ ((e >> 4) & 31)) ----
	 * loads of every pass: e = th + 512 j -> phys = rd + 512 j
	 * stores: pass p = 1    e = 16 th + m                          -> st1 ^ m
	 *         pass p = 16   e = 256 (th >> 4) + (th & 15) + 16 m   -> st2 ^ ((m ^ 16 (m & 1)) | 32 (m >> 1))
	 *         half exchange (plain layout [m''][th]: lane-contiguous both ways)  stores m'' 512 + th, loads m'' 512 + (th ^ 256) */
	const int rd  = th ^ ((th >> 4) & 31);
	const int st1 = (32 * (th >> 1)) | ((16 * (th & 1)) ^ (th & 31));
	const int st2 = (256 * (th >> 4)) | ((th & 15) ^ (16 * ((th >> 4) & 1)));

	/* SHIFT = 16 / R for hop = N / R, R = 2, 4, 8, 16: the next window's row j is this window's row j + SHIFT of the same thread;
	 * SHIFT = 16: any other hop, every row is requested again */
	const typename IQ::elem *iq = reinterpret_cast<const typename IQ::elem *>(p.iq);
	const uint32_t iq_vo = (uint32_t)sizeof(typename IQ::elem) * (uint32_t)th;	/* element th + 512 j of a window at this byte offset + that of row j (scalar descriptor + one lane offset) */
	typename IQ::raw q[16];		/* raw IQ of the spectrum to be processed next: rows th + 512 j */
	/* column of xo[m]: cb + 256 (m & 7) + 4096 (m >> 3), cb = kk + 2048 hh.  ONE register carries it through the spectrum loop, as the
	 * byte offset 2 cb of the column's short in an index row (the kernel has no register to spare: tools/check_k1w_loads.py); the rare
	 * users of cb itself (waterfall rows, the bytes of 9th bits, the tile's partials) take it back out of it where they run */
	const uint32_t cb2 = 2u * ((uint32_t)kk + 2048u * (uint32_t)hh);
#define K1W_CB() ({ uint32_t _c; asm volatile("v_lshrrev_b32 %0, 1, %1" : "=v"(_c) : "v"(cb2)); _c; })

	/* Epilogue of columns [M0, M1) of spectrum tp, whose FFT is in xo: log-power, exact 16-bit bin, live / max, waterfall row
	 * (display.cl:136-150,161-168).  Per column, nothing carried from column to column: it is cut into three pieces that
	 * run between the LDS stores of the NEXT spectrum's exchanges and the barrier behind them, i.e. while this wave
	 * would otherwise wait for the slowest one. */
	constexpr int kP1 = 6, kP2 = 11;	/* the three epilogue pieces: columns [0, kP1), [kP1, kP2), [kP2, 16) of a thread (measured) */
#define K1W_COL(m) (256 * ((m) & 7) + 4096 * ((m) >> 3))
#define K1W_EPI(M0, M1, tp) do { \
		__builtin_amdgcn_s_setprio(0);		/* the passes run at a higher issue priority than the epilogue pieces */ \
		const bool _row = ((tp) >= p.wf_first); \
		float *_wfr = p.wf + (size_t)((p.wf_pos0 + (tp)) & p.wf_mask) * N; \
		/* index stores (512 bins: 9 bits), 1.125 B per sample instead of the 2 B of a 16-bit index (round 6): \
		 *   low bytes   one SHORT per column and PAIR of spectra, [t / 2][column] (even spectrum in the low byte) \
		 *   9th bits    one BYTE per column and EIGHT spectra, [t / 8][column] behind the shorts (bit u = spectrum 8 (t / 8) + u) \
		 * A vector-memory instruction costs a CU 8-17 cycles whatever it carries (tools/ubench/vmem_rate.hip: 8.2 for 64 dense shorts, \
		 * 10.8 for 64 dwords), and with a store per sample the index stores were a quarter of this kernel's time: the low bytes of an \
		 * even spectrum wait in four registers (four columns each) for the odd one's, the 9th bits of eight spectra in four more \
		 * (tiles are multiples of 8: launch_k1).  Scalar base (SALU) + ONE lane offset + immediate; column cb + K1W_COL(m) of a row: \
		 * shorts at 2 cb + 512 (m & 7) + 8192 (m >> 3), bytes at cb + 256 (m & 7) + 4096 (m >> 3) */ \
		const char *_blo = reinterpret_cast<const char *>(p.bins) + (size_t)((tp) >> 1) * (N * 2); \
		const char *_bhi = reinterpret_cast<const char *>(p.bins) + (size_t)p.total * N + (size_t)((tp) >> 3) * N; \
		const uint32_t _bo2 = cb2; \
		const uint32_t _sh = (uint32_t)(tp) & 7u;		/* uniform */ \
		if ((M0) == 0 && _sh == 0) { hi9[0] = 0; hi9[1] = 0; hi9[2] = 0; hi9[3] = 0; } \
		float _l2[(M1) - (M0)]; uint32_t _bn[(M1) - (M0)]; uint32_t _amb = 0; \
		_Pragma("unroll") \
		for (int m = (M0); m < (M1); m++) { \
			uint32_t ab; \
			const float rr = bin_fast(xo[m].x, xo[m].y, bk, &_l2[m - (M0)], &ab); \
			_amb = _amb > ab ? _amb : ab;		/* v_max_u32: NaN / inf order above every finite measure */ \
			_bn[m - (M0)] = (uint32_t)(int)__builtin_amdgcn_fmed3f(rr, 0.0f, top); \
		} \
		/* ONE branch per piece (a compare + exec save + branch per sample cost 9 % of this kernel): rare -- find the samples again \
		 * and decide them against the exact thresholds */ \
		if (_amb > __float_as_uint(bk.amb)) { \
			_Pragma("unroll") \
			for (int m = (M0); m < (M1); m++) { \
				const float v = __builtin_fmaf(bk.A, _l2[m - (M0)], bk.C); \
				const float a = __builtin_fmaf(__builtin_fabsf(_l2[m - (M0)]), bk.kappa, __builtin_fabsf(v - __builtin_rintf(v))); \
				if (!(a <= bk.amb)) { \
					float nl2; \
					_bn[m - (M0)] = bin_exact(xo[m].x, xo[m].y, _l2[m - (M0)], (int)_bn[m - (M0)], thr_l, bk.nb, &nl2); \
					_l2[m - (M0)] = nl2; \
				} \
			} \
		} \
		_Pragma("unroll") \
		for (int m = (M0); m < (M1); m++)		/* the 9th bit joins its column's byte: bit (t & 7) */ \
			hi9[m >> 2] = (__builtin_amdgcn_ubfe(_bn[m - (M0)], 8, 1) << (8 * (m & 3) + _sh)) | hi9[m >> 2]; \
		if (!((tp) & 1)) {		/* (uniform: ONE branch per piece) even spectrum: keep the low bytes, four columns per register */ \
			_Pragma("unroll") \
			for (int m = (M0); m < (M1); m++) \
				held[m >> 2] = __builtin_amdgcn_perm(_bn[m - (M0)], held[m >> 2], \
				                                     (m & 3) == 0 ? 0x03020104u : (m & 3) == 1 ? 0x03020400u : (m & 3) == 2 ? 0x03040100u : 0x04020100u); \
		} else {		/* odd spectrum: the short of both */ \
			_Pragma("unroll") \
			for (int m = (M0); m < (M1); m++) { \
				const char *_sb = _blo + 8192 * (m >> 3); \
				const uint32_t _d = __builtin_amdgcn_perm(_bn[m - (M0)], held[m >> 2], 0x0c0c0400u | (uint32_t)(m & 3)); \
				switch (m & 7) { \
				case 0:  asm volatile("global_store_short %0, %1, %2" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 1:  asm volatile("global_store_short %0, %1, %2 offset:512" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 2:  asm volatile("global_store_short %0, %1, %2 offset:1024" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 3:  asm volatile("global_store_short %0, %1, %2 offset:1536" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 4:  asm volatile("global_store_short %0, %1, %2 offset:2048" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 5:  asm volatile("global_store_short %0, %1, %2 offset:2560" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				case 6:  asm volatile("global_store_short %0, %1, %2 offset:3072" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				default: asm volatile("global_store_short %0, %1, %2 offset:3584" :: "v"(_bo2), "v"(_d), "s"(_sb) : "memory"); break; \
				} \
			} \
			if (_sh == 7) {		/* (uniform) the eighth spectrum: the bytes of 9th bits, scalar base + one lane offset + immediate like the shorts; \
						 * byte 0 / 2 of a register as it is (global_store_byte / _d16_hi), byte 1 / 3 of its copy shifted by 8 */ \
				const uint32_t cb = K1W_CB(); \
				_Pragma("unroll") \
				for (int m = (M0); m < (M1); m++) { \
					const char *_hb = _bhi + 4096 * (m >> 3); \
					const uint32_t _hv = (m & 1) ? (hi9[m >> 2] >> 8) : hi9[m >> 2]; \
					if (m & 2) { \
						switch (m & 7) { \
						case 2:  asm volatile("global_store_byte_d16_hi %0, %1, %2 offset:512" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						case 3:  asm volatile("global_store_byte_d16_hi %0, %1, %2 offset:768" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						case 6:  asm volatile("global_store_byte_d16_hi %0, %1, %2 offset:1536" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						default: asm volatile("global_store_byte_d16_hi %0, %1, %2 offset:1792" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						} \
					} else { \
						switch (m & 7) { \
						case 0:  asm volatile("global_store_byte %0, %1, %2" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						case 1:  asm volatile("global_store_byte %0, %1, %2 offset:256" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						case 4:  asm volatile("global_store_byte %0, %1, %2 offset:1024" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						default: asm volatile("global_store_byte %0, %1, %2 offset:1280" :: "v"(cb), "v"(_hv), "s"(_hb) : "memory"); break; \
						} \
					} \
				} \
			} \
		} \
		_Pragma("unroll") \
		for (int m = (M0); m < (M1); m++) { \
			live[m] = __builtin_fmaf(live[m], p.w, _l2[m - (M0)]); \
			vmax[m] = max_f32(vmax[m], _l2[m - (M0)]); \
		} \
		if (_row) {		/* uniform, rare (the last wf_rows spectra of a call): one branch per piece instead of one per sample; the row \
					 * values are recomputed from the log-powers, which the live / max updates above kept alive anyway */ \
			float *_wf = _wfr + K1W_CB(); \
			_Pragma("unroll") \
			for (int m = (M0); m < (M1); m++) \
				_wf[K1W_COL(m)] = _l2[m - (M0)] * F_HALF_LOG10_2; \
		} \
		__builtin_amdgcn_s_setprio(2); \
	} while (0)

	__builtin_amdgcn_s_setprio(2);
#if K1W_TIMING
	uint32_t wacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t wprev = (uint32_t)__builtin_readcyclecounter();
#endif
	for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
	const int t0 = tile * p.tile;
	float live[16], vmax[16];
	uint32_t held[4] = { 0, 0, 0, 0 };		/* low bytes of the tile's last even spectrum's bin indices, four columns per register */
	uint32_t hi9[4] = { 0, 0, 0, 0 };		/* 9th bits of the indices of up to eight spectra, one byte per column, four columns per register */
#pragma unroll
	for (int m = 0; m < 16; m++) { live[m] = 0.0f; vmax[m] = vmax_init; }

	{
		const __amdgpu_buffer_rsrc_t src = make_rsrc(iq + (size_t)t0 * p.hop);
#pragma unroll
		for (int j = 0; j < 16; j++)
			q[j] = IQ::ld_iq(src, iq_vo, j);
	}

	v2f xo[16];			/* FFT of the previous spectrum of the tile, its epilogue still to do */
#pragma unroll
	for (int m = 0; m < 16; m++) xo[m] = v2f{ 0.0f, 0.0f };

#pragma unroll 1
	for (int g = 0; g < p.tile; g++) {
		const int t = t0 + g;
		const bool have_prev = g > 0;			/* uniform */
		/* The two waves of a SIMD (waves w and w + 4 of the work-group) run their epilogue pieces on opposite sides of the barrier:
		 * one computes while the other waits for its LDS loads, instead of all eight moving from LDS to VALU and back together */
		const bool late = hu != 0;
		v2f x[16];
		{ v2f *sw = slab0; slab0 = slab1; slab1 = sw; }		/* (the first spectrum starts on the second slab) */

		/* x[j] = element th + 512 j (the window multiply of fft.cl:415-417 rides on the first pass) */
		/* ---- pass 1: p = 1, item th, outputs e = 16 th + m -> slab0.  Before the next spectrum's IQ is requested: the requests then
		 * land in the registers this pass has just consumed (requested first, they needed sixteen more and a copy at the end of the loop) ---- */
		/* the IQ requested one iteration ago has arrived once at most the index stores issued BEHIND the requests are outstanding: the
		 * sixteen of an odd spectrum's epilogue, which ran in the previous iteration if that one's g was even and >= 2 (more, if waterfall
		 * rows or fft_out went out as well: the wait is then longer than needed, not shorter) */
#define K1W_Q16 "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]), \
		"+v"(q[8]), "+v"(q[9]), "+v"(q[10]), "+v"(q[11]), "+v"(q[12]), "+v"(q[13]), "+v"(q[14]), "+v"(q[15])
		/* (ONE statement, the choice inside it: two statements under an if made the compiler copy q -- before the wait) */
		/* (kK1wIdxStores: ONE constant for the wait's immediate and for what K1W_EPI issues per odd spectrum -- a change of the index
		 * format that packs the stores must change both; tools/check_k1w_loads.py counts the stores of the compiled loop against it) */
		static_assert(kK1wIdxStores == 16, "the counted wait below and K1W_EPI's index stores (one dword per column and pair of spectra) go together");
		asm volatile("s_cmp_eq_u32 %16, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt vmcnt(%17)\n\ts_branch 2f\n1:\ts_waitcnt vmcnt(0)\n2:"
		             : K1W_Q16 : "s"(__builtin_amdgcn_readfirstlane(((g & 1) && g >= 3) ? 1 : 0)), "n"(kK1wIdxStores) : "scc");
#undef K1W_Q16
#pragma unroll
		for (int j = 0; j < 16; j++)
			x[j] = IQ::widen(q[j]);
		K1W_STAMP(0);			/* radix 2 of the previous spectrum, loop overhead, wait for the IQ */
		pass16_first<true>(x, wab, w16c, w8c, w163c, two);
		K1W_STAMP(1);

		/* raw IQ of the next spectrum of this tile: shared rows move down, the new ones are requested now.  UNCONDITIONALLY (behind the
		 * tile's last spectrum: of that spectrum again, unused): a load inside a branch whose result merges with an older value at the
		 * join makes the compiler wait for it right there */
		{
			const int tn = (g + 1 < p.tile) ? t + 1 : t;
			const __amdgpu_buffer_rsrc_t src = make_rsrc(iq + (size_t)tn * p.hop);
			/* (moves the compiler cannot sink: left to it, they went behind the requests -- whose results then needed registers of their
			 * own, a copy at the end of the loop and, for that copy, a wait for every store issued in between) */
#pragma unroll
			for (int j = 0; j < 16 - SHIFT; j++)
				IQ::mov(q[j], q[j + SHIFT]);
			/* The requests are made by hand, and so is the wait for them at the top of the next iteration: loads and stores leave the
			 * vmcnt queue IN ORDER, and the wait the compiler places for loads it knows about -- vmcnt(0) -- also sat through the
			 * acknowledgement of every index store issued since (a third of this kernel's time: probe builds without the stores / without
			 * the requests, profiles/r05_c3.md) */
#pragma unroll
			for (int j = 16 - SHIFT; j < 16; j++)
				IQ::request(q[j], iq_vo, src, j);
		}

#pragma unroll
		for (int m = 0; m < 16; m++)
			slab0[st1 ^ m] = x[R16_PERM(m)];
		if (have_prev && !late) K1W_EPI(0, kP1, t - 1);
		K1W_STAMP(2);			/* IQ requests, stores (until done), early piece */
		wg_barrier_lds();
		K1W_STAMP(3);			/* barrier */
		/* a late wave runs its piece BEFORE it requests its operands (requesting them first measured 1.2 % slower) */
		if (have_prev && late) K1W_EPI(0, kP1, t - 1);
		K1W_STAMP(4);			/* late piece */
#pragma unroll
		for (int j = 0; j < 16; j++)
			x[j] = slab0[rd + 512 * j];
		K1W_STAMP(5);			/* reads (until all have arrived) */

		/* ---- pass 2: p = 16, k = th & 15, outputs e = 256 (th >> 4) + (th & 15) + 16 m -> slab1 ---- */
		pass16_ab<true>(x, tw16[0], tw16[1], two);
		pass16_cd<true>(x, tw16[2], tw16[3], tw16[4], tw16[5], tw16[6], tw16[7], two);
		K1W_STAMP(6);			/* pass 2 */
#pragma unroll
		for (int m = 0; m < 16; m++)
			slab1[st2 ^ ((m ^ (16 * (m & 1))) | (32 * (m >> 1)))] = x[R16_PERM(m)];
		if (have_prev && !late) K1W_EPI(kP1, kP2, t - 1);
		K1W_STAMP(7);
		wg_barrier_lds();
		K1W_STAMP(8);
		if (have_prev && late) K1W_EPI(kP1, kP2, t - 1);
		K1W_STAMP(9);
#pragma unroll
		for (int j = 0; j < 16; j++)
			x[j] = slab1[rd + 512 * j];
		K1W_STAMP(10);

		/* ---- pass 3: p = 256, k = kk: X3[4096 hh + kk + 256 m] = x[R16_PERM(m)]; the half this thread's butterflies do not need goes to
		 * thread th ^ 256 through slab0 ([m''][th]: m'' = m - 8 (1 - hh)) ---- */
		pass16_ab<true>(x, tw256[0], tw256[1], two);
		pass16_cd<true>(x, tw256[2], tw256[3], tw256[4], tw256[5], tw256[6], tw256[7], two);
		K1W_STAMP(11);			/* pass 3 */
		if (hu == 0) {			/* uniform per wave (waves 0-3 / 4-7): a scalar branch */
#pragma unroll
			for (int c = 0; c < 8; c++)
				slab0[512 * c + th] = x[R16_PERM(8 + c)];
		} else {
#pragma unroll
			for (int c = 0; c < 8; c++)
				slab0[512 * c + th] = x[R16_PERM(c)];
		}
		if (have_prev && !late) K1W_EPI(kP2, 16, t - 1);
		K1W_STAMP(12);
		wg_barrier_lds();
		K1W_STAMP(13);
		/* ---- radix 2, p = 4096 (fft.cl:428-458; o_pass_radix2_fma): (jb, jb + 4096), jb = kk + 256 (8 hh + c) ->
		 * xo[c] = X[jb], xo[c + 8] = X[jb + 4096] ---- */
		{
			v2f o[8];
			if (have_prev && late) K1W_EPI(kP2, 16, t - 1);
			K1W_STAMP(14);
#pragma unroll
			for (int c = 0; c < 8; c++)
				o[c] = slab0[512 * c + (th ^ 256)];
			K1W_STAMP(15);
			/* (step by step, like bf8; the two forms differ in where a and b come from) */
#define K1W_R2(A, B) do { \
				v2f u[8], pa[8]; \
				_Pragma("unroll") \
				for (int c = 0; c < 8; c++) \
					asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(u[c]) : "v"(B), "v"(twr[c]), "v"(A)); \
				_Pragma("unroll") \
				for (int c = 0; c < 8; c++) \
					asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(pa[c]) : "v"(B), "v"(twr[c]), "v"(u[c])); \
				_Pragma("unroll") \
				for (int c = 0; c < 8; c++) \
					asm volatile("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(xo[c + 8]) : "v"(A), "s"(two), "v"(pa[c])); \
				_Pragma("unroll") \
				for (int c = 0; c < 8; c++) \
					xo[c] = pa[c]; \
			} while (0)
			if (hu == 0)			/* X3[jb] is this item's output m = c, X3[jb + 4096] item th + 256's */
				K1W_R2(x[R16_PERM(c)], o[c]);
			else				/* X3[jb] is item th - 256's output m = 8 + c, X3[jb + 4096] this item's */
				K1W_R2(o[c], x[R16_PERM(8 + c)]);
#undef K1W_R2
		}

		if (p.fft_out) {		/* (tests) */
#pragma unroll
			for (int m = 0; m < 16; m++)
				reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * N + K1W_CB() + K1W_COL(m)] = xo[m];
		}
	}
	/* the last iteration's requests (made unconditionally, see above) still own their registers: nothing may reuse them before they have landed */
	asm volatile("s_waitcnt vmcnt(0)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]),
	             "+v"(q[8]), "+v"(q[9]), "+v"(q[10]), "+v"(q[11]), "+v"(q[12]), "+v"(q[13]), "+v"(q[14]), "+v"(q[15]));
	K1W_EPI(0, 16, t0 + p.tile - 1);		/* the tile's last spectrum */

	float2 *pp2 = p.partial + (size_t)tile * N + K1W_CB();
#pragma unroll
	for (int m = 0; m < 16; m++)
		pp2[K1W_COL(m)] = make_float2(live[m] * F_HALF_LOG10_2,
			(vmax[m] == vmax_init) ? -1000.0f : vmax[m] * F_HALF_LOG10_2);
	}
#if K1W_TIMING
	if (p.dbg && (th & 255) == 0) {
#pragma unroll
		for (int i = 0; i < 16; i++)
			p.dbg[((size_t)blockIdx.x * 2 + (th >> 8)) * 16 + i] = wacc[i];
	}
#endif
#undef K1W_EPI
#undef K1W_CB
#undef K1W_COL
}
