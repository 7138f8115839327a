/*
 * k1h_fused.inc -- the 65536-point kernel.  A template over the IQ format: IQ is one of the tags of "IQ formats" in fosphor_kernels.hip, which
 * includes this file once.  The formats of one dword per sample (HALF below: fp16, sc16) are staged in LDS by LDS-DMA and taken out
 * with IQ::widen; fp32 is gathered per lane where it is used.
 */
template <typename IQ, bool WRITE_FFT, int NWV>
__global__ __launch_bounds__(64 * NWV, 2)
void k1h_fused(const K1Params p)
{
	constexpr int N = 65536;
	constexpr bool HALF = sizeof(typename IQ::elem) == 4;
	typedef K1hGeom<NWV> G;
	constexpr int NT = 64 * NWV, kMem = G::kMem, kRpm = G::kRpm, kXLen = G::kXLen, kInLen = G::kInLen;
	/* Every wait on another work-group is bounded (a poll is ~1 us: seconds, far beyond any legitimate wait): a protocol failure
	 * ends the kernel with an error word the host turns into -EIO, it does not hang the GPU. */
	constexpr uint32_t kSpinLimit = 4u << 20;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	v2f *xa_all = reinterpret_cast<v2f *>(smem_raw);		/* stage A: one private exchange region per wave ... */
	v2f *xb = xa_all;						/* ... stage B: the work-group's exchange array, in the same memory */
	v2f *twa_t = xa_all + kXLen;					/* pass-2 twiddles [k2 16][8 of kTwRow] */
	v2f *tw3_t = twa_t + 16 * kTwRow;				/* pass-3 twiddles of this member's 32 offsets [32][8 of kTwRow] */
	uint32_t *inb = reinterpret_cast<uint32_t *>(tw3_t + kRpm * kTwRow);	/* fp16 IQ of the next two spectra (two buffers of kInLen dwords) */
	/* the exact-bin thresholds: the rare path that consults them must not wait for the loads and stores in flight (LDS reads have
	 * their own counter) */
	typedef const __attribute__((address_space(3))) double *lds_cdp;
	double *thr_g = reinterpret_cast<double *>(inb + 2 * kInLen);
	const lds_cdp thr_l = (lds_cdp)thr_g;

	const int tid = threadIdx.x;
	/* Cluster formation.  A work-group takes a ticket from the counter of the XCD it actually runs on (XCC_ID):
	 * tickets 8c .. 8c + 7 of an XCD are cluster c of that XCD, whatever the dispatcher did.  A cluster works once
	 * its 8 members are resident; complete clusters claim tiles until none is left, and a cluster still forming
	 * when the tiles run out (another kernel holds the CUs its members need) is abandoned as a whole: progress
	 * never depends on a work-group that is not resident. */
	__shared__ int sh_ticket, sh_tile;
	uint32_t xcc;
	asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
	xcc &= 7;
	uint32_t *next_tile = p.sync + 63 * 64 + 56;		/* (on the last cluster's line; tickets sit at word 48) */
	const int ntiles = p.total / p.tile;
	if (tid == 0) {
		uint32_t *tick = p.sync + xcc * 8 * 64 + 48;		/* on the line of the XCD's first cluster */
		const uint32_t tk = __hip_atomic_fetch_add(tick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		int ok = 0;
		if (tk < 64) {
			/* the cluster's state: 0 forming, 1 complete (set by the holder of its 8th ticket: all 8 are resident),
			 * 2 abandoned (set by a member that saw the tiles run out first) -- one compare-and-swap decides */
			uint32_t *state = p.sync + ((int)xcc * 8 + (int)(tk / kMem)) * 64 + 24;
			uint32_t st = 0;
			if ((tk % kMem) == kMem - 1) {
				__hip_atomic_compare_exchange_strong(state, &st, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				st = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			} else {
				uint32_t spins = 0;
				while ((st = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
					const bool tiles_left = (int)__hip_atomic_load(next_tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ntiles;
					if (!tiles_left || ++spins > kSpinLimit) {	/* (a cluster that never fills is abandoned, never waited for) */
						if (tiles_left)
							*p.sync_err = 0x80000004u;	/* ... but with work left that is a failed call, not a quiet exit */
						uint32_t expect = 0;
						__hip_atomic_compare_exchange_strong(state, &expect, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					}
					__builtin_amdgcn_s_sleep(8);
				}
			}
			ok = (st == 1);
		}
		sh_ticket = ok ? (int)tk : -1;
	}
	__syncthreads();
	/* The counters reset themselves: the last work-group to leave the kernel (an exit ticket, drawn behind everything else a work-group
	 * does with them) zeroes the whole array for the next launch -- no memset queued per frame (4.6 us each on this runtime). */
	auto leave = [&]() {
		__syncthreads();
		if (tid == 0)
			sh_ticket = (int)__hip_atomic_fetch_add(p.sync + 63 * 64 + 60, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__syncthreads();
		if (sh_ticket == (int)gridDim.x - 1)
			for (int e = tid; e < 64 * 64; e += NT)
				__hip_atomic_store(p.sync + e, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	};
	if (sh_ticket < 0) {
		leave();
		return;
	}
	/* (everything that is the same for the whole work-group is forced into SGPRs: addresses are then a scalar base plus ONE
	 * 32-bit per-lane offset -- global_load / global_store ... s[base:base+1] -- instead of a 64-bit vector add per access) */
	const int ticket = __builtin_amdgcn_readfirstlane(sh_ticket);
	const int member = ticket % kMem;
	const int gc = (int)xcc * 8 + ticket / kMem;			/* cluster: up to 8 per XCD */
	uint32_t *c_a = p.sync + gc * 64;				/* stage A done */
	uint32_t *c_t = p.sync + gc * 64 + 16;				/* (round << 20) | tile, published by member 0 */
	uint32_t *c_b = p.sync + gc * 64 + 32;				/* stage B has read the intermediate */
	v2f *wint = reinterpret_cast<v2f *>(p.scratch) + (size_t)gc * N;	/* the cluster's intermediate: [offset / 32][residue][offset % 32] */
	const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(wint);

	const int lane = tid & 63;
	const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
	const v2f *twg = reinterpret_cast<const v2f *>(p.tw);
	const v2f two = { 2.0f, 2.0f };
	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float vmax_init = -1000.0f / F_HALF_LOG10_2;
	const float top = (float)(bk.nb - 1);

	/* ---- per-thread constants -------------------------------------------------------------------------------------
	 * stage A: residue q = 32 member + 4 wave + (lane >> 4); pass-1 item a = lane & 15 reads m = a + 16 j; after the
	 *          exchange the same lane is pass-2 item k2 = lane & 15 (twiddle index k2)
	 * stage B: offset kk = 32 member + (tid & 31); pass-3 item a3 = tid >> 5 reads residues q = a3 + 16 j3 (twiddle
	 *          index kk); after the exchange the same thread is pass-4 item jj3 = tid >> 5 (twiddle index kk + 256 jj3)
	 *          and owns columns kk + 256 jj3 + 4096 jj4 */
	const int sa = lane >> 4, ia = lane & 15;
	const int qa = kRpm * member + 4 * wv + sa;
	const int kkl = tid % kRpm, ib = tid / kRpm;
	const int kk = kRpm * member + kkl;
	const int col0 = kk + 256 * ib;
	const unsigned ucol0 = (unsigned)col0;				/* the one per-lane offset of every output access */
	/* the intermediate is [offset / kRpm][residue][offset % kRpm].  32 offsets per block: see the stores below; 16: a row is one 128-byte run */
	const unsigned wst0 = kRpm == 32 ? 8u * (unsigned)(qa * 32 + (ia ^ ((qa & 1) << 4)))		/* stage-A stores of even / odd jj (byte offsets) */
	                                 : 8u * (unsigned)(qa * 16 + ia);
	const unsigned wst1 = wst0 ^ 128u;
	const unsigned wld = kRpm == 32 ? 8u * (unsigned)(ib * 32 + (kkl ^ ((ib & 1) << 4)))		/* stage-B loads */
	                                : 8u * (unsigned)(ib * 16 + kkl);
	const __amdgpu_buffer_rsrc_t rs_wf = make_rsrc(p.wf), rs_part = make_rsrc(p.partial);

	const v2f w16c = twg[p.tw_off[0]], w8c = twg[p.tw_off[0] + 1], w163c = twg[p.tw_off[0] + 2];	/* W16, W8, W16^3: the first pass */
	v2f wab[HALF ? 8 : 1];						/* wab[j]: the window taps of this thread's pass-1 inputs j and j + 8, the pair of
									 * a stage-A butterfly (fp32 IQ, not a BASELINE configuration at this length: read
									 * where they are used -- its 32 staging registers leave no room for them) */
#pragma unroll
	for (int j = 0; j < (HALF ? 8 : 1); j++)
		wab[j] = v2f{ p.win[qa + 256 * (ia + 16 * j)], p.win[qa + 256 * (ia + 16 * (j + 8))] };
	v2f tw4[8];							/* pass 4: w^8, w^4, w^2, w^2 W8, w, w W16, w W8, w W16^3 of k = kk + 256 ib */
#pragma unroll
	for (int j = 0; j < 8; j++)
		tw4[j] = twg[p.tw_off[3] + (kk + 256 * ib) * 8 + j];
	for (int e = tid; e <= p.n_bins && e < kThrMax; e += NT)
		thr_g[e] = p.thr[e];
	for (int e = tid; e < 16 * 8; e += NT)
		twa_t[(e >> 3) * kTwRow + (e & 7)] = twg[p.tw_off[1] + e];
	for (int e = tid; e < kRpm * 8; e += NT)
		tw3_t[(e >> 3) * kTwRow + (e & 7)] = twg[p.tw_off[2] + (kRpm * member) * 8 + e];
	__syncthreads();

	v2f *xa = xa_all + wv * kXaWave;
	const int ea_w = sa * 272 + ia;			/* + 17 jj : pass-1 outputs [residue][jj][a] */
	const int ea_r = sa * 272 + ia * 17;		/* + j2    : pass-2 inputs of item k2 = ia */
	const int eb_w = kkl * 257 + ib;		/* + 16 jj3: pass-3 outputs [offset][jj3][a3] */
	const int eb_r = kkl * 257 + ib * 16;		/* + j4    : pass-4 inputs of item jj3 = ib */

	if (wv >= NWV / 2)
		__builtin_amdgcn_s_setprio(2);
	uint32_t done = 0;						/* spectra this cluster has finished */
	uint32_t round = 0;						/* tiles this cluster has taken */

	/* fp16 IQ: the work-group fetches its 32 residues of a spectrum as whole 128-byte runs STRAIGHT INTO LDS (buffer_load_dwordx4 ... lds:
	 * no staging registers, no ds_write pass) -- one wave-instruction lands 64 x 16 B = 8 rows x 128 B back to back, so rows cannot be
	 * padded; the 16-byte piece pc of row m sits at slot 8 m + (pc ^ (m & 7)) instead (the permutation is applied to the per-lane SOURCE
	 * address and again to the read address; a wave's reads meet two-way conflicts at most).  A wave then finds the rows of its four
	 * residues in LDS (a wave gathering its own 16-byte pieces straight from memory touches every line eight times over: measured
	 * +205 us per frame against +37).  Two buffers: spectrum u of a tile in buffer u & 1.
	 * fp32 IQ (not a BASELINE configuration at this length) is gathered per lane where it is used. */
	/* (16 residues per member: rows of 64 B, one wave-instruction lands 16 of them; piece pc of row m at slot 4 m + (pc ^ ((m >> 2) & 3)):
	 * the 64 lanes of a read -- 16 rows x the 4 dwords of one piece -- then fall into 64 different banks) */
	constexpr int kRowsPerDma = 256 / kRpm;			/* rows one wave-instruction lands: 8 / 16 */
	const uint32_t iq_vo = kRpm == 32 ? 1024u * (unsigned)(lane >> 3) + 16u * (unsigned)((lane & 7) ^ ((lane >> 3) & 7))
	                                  : 1024u * (unsigned)(lane >> 2) + 16u * (unsigned)((lane & 3) ^ ((lane >> 4) & 3));
	const int in_rd  = kRpm == 32 ? ia * 32 + ((wv ^ (ia & 7)) << 2) + sa	/* + kRpm * 16 j: row m = ia + 16 j, residue 4 wave + sa (dwords) */
	                              : ia * 16 + ((wv ^ ((ia >> 2) & 3)) << 2) + sa;
	const uint32_t inb_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) void *)inb;
	auto fetch_iq = [&](int t, int buf) {		/* row groups g = wave, wave + NWV, ... (256 dwords each) into buffer `buf`: every wave fetches
							 * (the cluster counters are polled through the scalar path, not behind these requests) */
		if (!HALF || wv >= NWV)		/* (wv < NWV always; without the test the compiler allocates the kernel's scalar registers differently) */
			return;
		/* global_load_lds_dwordx4 by hand: the compiler parks every LDS read and every __syncthreads() that follows an LDS-DMA it
		 * knows about behind s_waitcnt vmcnt(0) -- the request would be waited for at the very next barrier instead of an iteration
		 * later.  Whoever reads the buffer is behind an explicit `s_waitcnt vmcnt(..)` of the requesting wave and a barrier. */
		const uint32_t *src = reinterpret_cast<const uint32_t *>(p.iq) + (size_t)t * p.hop + kRpm * member;
#pragma unroll 1
		for (int g = wv; g < kRpm; g += NWV) {
			const uint32_t *sk = src + 256 * kRowsPerDma * g;				/* 8 / 16 rows of 1 KiB */
			const uint32_t la = inb_lds + 4u * (unsigned)(buf * kInLen + 256 * g);
			uint32_t keep;
			asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
			             : "=&s"(keep) : "v"(iq_vo), "s"(sk), "s"(la) : "memory");
		}
	};

	v2f ra[16];				/* stage A of the spectrum AFTER the one stage B is working on */
	/* pass 1 (p = 1: no twiddles) of spectrum t and the 16 x 16 transpose inside the wave */
	auto stage_a1 = [&](int t, int buf) {
		const __amdgpu_buffer_rsrc_t rs_f = make_rsrc(p.iq + (size_t)t * p.hop);
#pragma unroll
		for (int jo = 0; jo < 16; jo++) {
			const int j = K1H_PAIR(jo);
			v2f xv;
			if constexpr (HALF) {
				xv = IQ::widen(inb[buf * kInLen + in_rd + 16 * kRpm * j]);
			} else {
				xv = bld_v2f<kAuxNT>(rs_f, 8u * (unsigned)(qa + 256 * ia), 32768u * j);
			}
			ra[j] = xv;
		}
		/* first pass (p = 1), the window of fft.cl:415-417 on its stage-A butterflies */
		if constexpr (HALF) {
			pass16_first(ra, wab, w16c, w8c, w163c, two);
		} else {
			v2f wl[8];
#pragma unroll
			for (int j = 0; j < 8; j++)
				wl[j] = v2f{ p.win[qa + 256 * (ia + 16 * j)], p.win[qa + 256 * (ia + 16 * (j + 8))] };
			pass16_first(ra, wl, w16c, w8c, w163c, two);
		}
	};
	/* ... and the 16 x 16 transpose inside the wave that follows it */
	auto stage_a1x = [&]() {
#pragma unroll
		for (int jj = 0; jj < 16; jj++)
			xa[ea_w + 17 * jj] = ra[R16_PERM(jj)];
		wave_lds_sync();
#pragma unroll
		for (int jo = 0; jo < 16; jo++)
			ra[K1H_PAIR(jo)] = xa[ea_r + K1H_PAIR(jo)];
		wave_lds_sync();
	};
	/* pass 2, p = 16, k = ia.  The pass-2 / pass-3 twiddles are read from LDS every spectrum: held in registers (round 5) the kernel alone
	 * ran 2.6 % faster and the path 10 % slower (233 instead of 209 VGPRs leave the previous frame's scan / merge kernels no room beside it) */
	const v2f *twa_r = twa_t + ia * kTwRow;
	const v2f *tw3_r = tw3_t + kkl * kTwRow;
	auto stage_a2 = [&]() {
		pass16_ab(ra, twa_r[0], twa_r[1], two);
		pass16_cd(ra, twa_r[2], twa_r[3], twa_r[4], twa_r[5], twa_r[6], twa_r[7], two);
	};

#if K1H_TIMING
	long long hacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	long long hprev = __builtin_readcyclecounter();
#endif
	uint32_t *bins_lo = p.bins;					/* [total / 4][N] dwords: 4 spectra x low 8 bits */
	uint32_t *bins_hi = p.bins + (size_t)(p.total >> 2) * N;	/* [total / tile][N] dwords: bit u = 9th bit of the tile's spectrum u */

	for (;;) {
	/* member 0 claims the cluster's next tile */
	if (tid == 0) {
		uint32_t v;
		if (member == 0) {
			v = __hip_atomic_fetch_add(next_tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (v > 0xfffffu) v = 0xfffffu;
			__hip_atomic_store(c_t, ((round + 1) << 20) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		} else {
			uint32_t spins = 0;
			while (((v = __hip_atomic_load(c_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 20) != round + 1) {
				if (++spins > kSpinLimit) { *p.sync_err = 0x80000001u; v = 0xfffffu; break; }	/* fail the call, not the GPU */
				__builtin_amdgcn_s_sleep(2);
			}
			v &= 0xfffffu;
		}
		sh_tile = (int)v;
	}
	__syncthreads();				/* (also: every read of the exchange array by the previous tile's last spectrum is done) */
	const int tile = __builtin_amdgcn_readfirstlane(sh_tile);
	round++;
	if (tile >= ntiles)
		break;
	const int t0 = tile * p.tile;
	float live[16], vmax[16];
	uint32_t plo[16], phi[16];
#pragma unroll
	for (int c = 0; c < 16; c++) { live[c] = 0.0f; vmax[c] = vmax_init; plo[c] = 0; phi[c] = 0; }
	auto epilogue = [&](v2f (&r)[16], const int t, const int u) {
		if (WRITE_FFT) {
#pragma unroll
			for (int c = 0; c < 16; c++)
				bst_v2f<0>(r[R16_PERM(c)], make_rsrc(reinterpret_cast<v2f *>(p.fft_out) + (size_t)t * N), 8u * ucol0, 32768u * c);
		}

		/* epilogue (display.cl:136-150,161-168), 9-bit bin indices: low byte into the quad's dword, 9th bit into the tile's */
		const bool store_row = (t >= p.wf_first);
		const uint32_t wf_so = (uint32_t)((p.wf_pos0 + t) & p.wf_mask) * (uint32_t)(N * 4);
		const int sh8 = 8 * (u & 3);
		/* four samples at a time: fast path, ONE branch for the four (rare: some sample is not provably exact -- find it again and
		 * decide it against the exact thresholds), then the updates and stores */
#pragma unroll
		for (int g = 0; g < 4; g++) {
			float l2g[4]; uint32_t bng[4]; uint32_t amb = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const v2f x = r[R16_PERM(4 * g + k)];
				uint32_t ab;
				const float rr = bin_fast(x.x, x.y, bk, &l2g[k], &ab);
				amb = amb > ab ? amb : ab;		/* v_max_u32: NaN / inf order above every finite measure */
				bng[k] = (uint32_t)(int)__builtin_amdgcn_fmed3f(rr, 0.0f, top);
			}
			if (amb > __float_as_uint(bk.amb)) {
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const v2f x = r[R16_PERM(4 * g + k)];
					const float v = __builtin_fmaf(bk.A, l2g[k], bk.C);
					const float a = __builtin_fmaf(__builtin_fabsf(l2g[k]), bk.kappa, __builtin_fabsf(v - __builtin_rintf(v)));
					if (!(a <= bk.amb)) {
						float nl2;
						bng[k] = bin_exact(x.x, x.y, l2g[k], (int)bng[k], thr_l, bk.nb, &nl2);
						l2g[k] = nl2;
					}
				}
			}
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const int c = 4 * g + k;
				const uint32_t bn = bng[k];
				const float l2v = l2g[k];
				plo[c] |= (bn & 0xffu) << sh8;
				phi[c] |= (bn >> 8) << u;
				live[c] = __builtin_fmaf(live[c], p.w, l2v);
				vmax[c] = max_f32(vmax[c], l2v);
				/* rows and bin indices are streamed out non-temporally: plain stores allocate in the XCD's L2 and push the cluster's
				 * intermediate out of it */
				if (store_row)
					__builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l2v * F_HALF_LOG10_2), rs_wf, 4u * ucol0, wf_so + 16384u * c, kAuxNT);
			}
		}
		if ((u & 3) == 3) {
			const __amdgpu_buffer_rsrc_t rs_lo = make_rsrc(bins_lo + (size_t)(t >> 2) * N);
#pragma unroll
			for (int c = 0; c < 16; c++) {
				__builtin_amdgcn_raw_buffer_store_b32(plo[c], rs_lo, 4u * ucol0, 16384u * c, kAuxNT);
				plo[c] = 0;
			}
		}
	};
	/* the tile's first spectrum: nothing to hide its stage A behind.  Input buffers: spectrum u of the tile in buffer u & 1 */
	fetch_iq(t0, 0);
	if (1 < p.tile)
		fetch_iq(t0 + 1, 1);
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	wg_barrier_lds();
	stage_a1(t0, 0);
	stage_a1x();
	wg_barrier_lds();				/* every wave has its rows out of buffer 0 */
	if (2 < p.tile)
		fetch_iq(t0 + 2, 0);
	stage_a2();

	/* The loop is skewed: while spectrum u's blocks travel to the L2 (stores), to the other members (cluster wait) and back (loads),
	 * the same threads run stage A of spectrum u + 1 -- its first pass between the stores and the arrival at the cluster barrier,
	 * its second between the loads of the intermediate and their use. */
#pragma unroll 1
	for (int u = 0; u < p.tile; u++) {
		const int t = t0 + u;
		const bool more = (u + 1 < p.tile);

		K1H_STAMP(0);		/* loop overhead, tile claim (first spectrum of a tile) */
		/* every member has read the previous spectrum out of the intermediate?  Every wave asks for itself, through the scalar path */
		{
			uint32_t spins = 0;
			while ((int)(sload_fresh(c_b) - (uint32_t)kMem * done) < 0) {
				if (++spins > kSpinLimit) { if (lane == 0) *p.sync_err = 0x80000002u; break; }
				__builtin_amdgcn_s_sleep(1);
			}
		}
		K1H_STAMP(1);		/* this wave's own look at the counter */
		/* w[256 q + kk], kk = ia + 16 jj2, at [kk >> 5][q][(kk & 31) ^ 16 (q & 1)]: 16 lanes x 8 B = 128-byte runs; odd residues
		 * keep their two halves swapped so that one store instruction (one jj for every lane) is spread over both halves of the
		 * 256-byte rows -- both values of the address bit that picks an L2 channel -- instead of one */
#pragma unroll
		for (int jj = 0; jj < 16; jj++) {
			if (kRpm == 32) bst_v2f<0>(ra[R16_PERM(jj)], rs_w, (jj & 1) ? wst1 : wst0, 65536u * (jj >> 1));
			else            bst_v2f<0>(ra[R16_PERM(jj)], rs_w, wst0, 32768u * jj);	/* (one instruction: four residues = 512 B in a row) */
		}
		if (more)
			stage_a1(t + 1, (u + 1) & 1);			/* (while the stores travel) */
		K1H_STAMP(2);		/* intermediate stores issued + first pass of the next spectrum */
		/* this wave's blocks are in the L2 (and the input rows it requested most of an iteration ago in LDS) */
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		K1H_STAMP(3);		/* waiting for the stores' acknowledgements (and the IQ requested an iteration ago) */
		wg_barrier_lds();
		if (tid == 0)
			__hip_atomic_fetch_add(c_a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		K1H_STAMP(4);		/* barrier + arrival */
		if (more)
			stage_a1x();				/* (while the arrivals travel) */

		K1H_STAMP(5);		/* transpose */
		if (tid == 0) {
			uint32_t spins = 0;
			while ((int)(__hip_atomic_load(c_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (uint32_t)kMem * (done + 1)) < 0) {
				if (++spins > kSpinLimit) { *p.sync_err = 0x80000003u; break; }
				__builtin_amdgcn_s_sleep(1);
			}
		}
		wg_barrier_lds();
		asm volatile("" ::: "memory");
		K1H_STAMP(6);		/* cluster barrier: poll + work-group barrier */

		/* ================= stage B: offsets kk = 32 member .. + 31 ================= */
		v2f r[16];
		/* residues q = ib + 16 j3 (q & 1 = ib & 1); sc1: the loads miss the CU's L1 by construction and are served by the L2 */
#pragma unroll
		for (int jo = 0; jo < 16; jo++)
			r[K1H_PAIR(jo)] = bld_v2f<kAuxSC1>(rs_w, wld, (uint32_t)(2048 * kRpm) * member + (uint32_t)(128 * kRpm) * K1H_PAIR(jo));
		if (more)						/* (while the loads travel) */
			stage_a2();
		K1H_STAMP(7);		/* loads of the intermediate issued + second pass of the next spectrum */
		pass16_ab(r, tw3_r[0], tw3_r[1], two);						/* pass 3, p = 256, k = kk */
#if K1H_TIMING
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
		K1H_STAMP(8);		/* third pass, stages A and B: includes the wait for the loads */
		/* spectrum u + 3 is requested into the buffer spectrum u + 1 has been read out of by every wave (two barriers ago); it is
		 * waited for by the `vmcnt(0)` of the NEXT iteration.  Requested only now that the loads of the intermediate have been used:
		 * loads return in order, and these come from HBM */
		if (u + 3 < p.tile)
			fetch_iq(t + 3, (u + 1) & 1);
		pass16_cd(r, tw3_r[2], tw3_r[3], tw3_r[4], tw3_r[5], tw3_r[6], tw3_r[7], two);
#pragma unroll
		for (int jj = 0; jj < 16; jj++)
			xb[eb_w + 16 * jj] = r[R16_PERM(jj)];
		K1H_STAMP(9);		/* IQ request + third pass, stages C and D + exchange stores */
		wg_barrier_lds();
		if (tid == 0)							/* everybody's loads of the intermediate have landed */
			__hip_atomic_fetch_add(c_b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		done++;
		K1H_STAMP(10);		/* exchange barrier */
#pragma unroll
		for (int jo = 0; jo < 16; jo++)
			r[K1H_PAIR(jo)] = xb[eb_r + K1H_PAIR(jo)];
		pass16_ab(r, tw4[0], tw4[1], two);							/* pass 4, p = 4096, k = kk + 256 ib */
		pass16_cd(r, tw4[2], tw4[3], tw4[4], tw4[5], tw4[6], tw4[7], two);

		K1H_STAMP(11);		/* exchange loads + fourth pass */
		K1H_STAMP(12);		/* (empty since round 6: the "everyone has read the intermediate" poll moved to the top of the loop) */
		epilogue(r, t, u);
		K1H_STAMP(13);		/* epilogue */
	}
	{
		const __amdgpu_buffer_rsrc_t rs_hi = make_rsrc(bins_hi + (size_t)tile * N);
#pragma unroll
		for (int c = 0; c < 16; c++)
			__builtin_amdgcn_raw_buffer_store_b32(phi[c], rs_hi, 4u * ucol0, 16384u * c, kAuxNT);
	}
#pragma unroll
	for (int c = 0; c < 16; c++)
		bst_v2f<0>(v2f{ live[c] * F_HALF_LOG10_2, (vmax[c] == vmax_init) ? -1000.0f : vmax[c] * F_HALF_LOG10_2 },
		           rs_part, 8u * ucol0, (uint32_t)tile * (uint32_t)(N * 8) + 32768u * c);
	}
#if K1H_TIMING
	if (p.dbg && lane == 0 && (wv == 0 || wv == NWV / 2 - 1 || wv == NWV - 1)) {
		const int slot = (wv == 0) ? 0 : (wv == NWV / 2 - 1) ? 1 : 2;
		for (int i = 0; i < 16; i++)
			p.dbg[((size_t)blockIdx.x * 3 + slot) * 16 + i] = hacc[i];
	}
#endif
	leave();
}
