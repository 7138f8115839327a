/*
 * k1big_fft_bin.inc -- the general-N kernel, N / 8 threads per spectrum (16-bit bin indices).  A template over the IQ format: IQ is one of the
 * tags of "IQ formats" in fosphor_kernels.hip, which includes this file once; IQ::ld_sample is the only place where the formats differ.
 */
template <typename IQ, int LOG2N, bool WRITE_FFT>
__global__ __launch_bounds__((1 << LOG2N) / 8)
void k1big_fft_bin(const K1Params p)
{
	constexpr int N = 1 << LOG2N, T = N / 8, NP8 = LOG2N / 3;
	static_assert(LOG2N % 3 == 1, "plan: radix-8 passes then one radix-2 pass");
	extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
	v2f *buf = reinterpret_cast<v2f *>(smem_raw);

	const int i = threadIdx.x;
	const int ntiles = p.total / p.tile;
	/* the whole twiddle table sits behind the exchange slab in LDS: read from global memory it was 21 B per sample of L2 traffic,
	 * against 8 B per sample of IQ.  The reference's layout, 7 per item and pass, then the radix-2 pass's */
	constexpr int TWLEN = ((N / 2 - 8) / 7) * 7 + N / 2;	/* (8 + 64 + ... + N/16) * 7 + N/2 */
	v2f *tws = buf + N;
	float *wins = reinterpret_cast<float *>(tws + TWLEN);	/* and the window behind it: 160 KiB in all at N = 8192 */
	for (int k = i; k < TWLEN; k += T)
		tws[k] = reinterpret_cast<const v2f *>(p.tw)[k];
	for (int k = i; k < N; k += T)
		wins[k] = p.win[k];
	__syncthreads();
	const v2f *twg = tws;
	const v2f s12 = { F_SQRT_1_2, F_SQRT_1_2 };
	const BinConst bk = { p.binA, p.binC, p.amb, p.kappa, p.n_bins, p.thr };
	const float vmax_init = -1000.0f / F_HALF_LOG10_2;
	const float top = (float)(bk.nb - 1);

	for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
	const int t0 = tile * p.tile;
	float live[8], vmax[8];
#pragma unroll
	for (int q = 0; q < 8; q++) { live[q] = 0.0f; vmax[q] = vmax_init; }

	for (int g0 = 0; g0 < p.tile; g0 += 2) {
		uint32_t pack[8];
#pragma unroll
		for (int q = 0; q < 8; q++) pack[q] = 0;

#pragma unroll 1
		for (int u = 0; u < 2; u++) {
			const int t = t0 + g0 + u;
			const typename IQ::elem *src = reinterpret_cast<const typename IQ::elem *>(p.iq) + (size_t)t * p.hop;
			v2f r[8];

			/* window (fft.cl:415-417) */
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const v2f xv = IQ::ld_sample(src + i + T * j);
				const float wv = wins[i + T * j];
				r[j] = v2f{ xv.x * wv, xv.y * wv };
			}

			/* radix-8 passes p = 1, 8, 64, ... (fft.cl:278-350) */
			int pp = 1;
#pragma unroll
			for (int q8 = 0; q8 < NP8; q8++) {
				const int k = i & (pp - 1);
				if (q8 > 0) {
					const v2f *tw = twg + p.tw_off[q8 - 1] + k * 7;
#pragma unroll
					for (int j = 1; j < 8; j++)
						r[j] = c_mul(r[j], tw[j - 1]);
				}
				dft8(r, s12);
				const int j0 = ((i - k) << 3) + k;
#pragma unroll
				for (int jj = 0; jj < 8; jj++)
					buf[swz(j0 + jj * pp)] = r[R8_PERM(jj)];
				__syncthreads();
				if (q8 + 1 < NP8) {
#pragma unroll
					for (int j = 0; j < 8; j++)
						r[j] = buf[swz(i + T * j)];
					__syncthreads();
				}
				pp <<= 3;
			}

			/* final radix-2 pass, p = N/2 (fft.cl:428-458): butterflies jb = i + T c on (jb, jb + N/2) */
			v2f x[8];
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const int jb = i + T * c;
				v2f a = buf[swz(jb)];
				v2f b = buf[swz(jb + N / 2)];
				b = c_mul(b, twg[p.tw_off[NP8 - 1] + jb]);
				DFT2(a, b);
				x[c] = a;		/* column jb */
				x[c + 4] = b;		/* column jb + N/2 */
			}
			__syncthreads();		/* slab free for the next spectrum */

			if (WRITE_FFT) {
#pragma unroll
				for (int c = 0; c < 4; c++) {
					reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * N + i + T * c] = x[c];
					reinterpret_cast<v2f *>(p.fft_out)[(size_t)t * N + i + T * c + N / 2] = x[c + 4];
				}
			}

			/* epilogue (display.cl:136,161-168), as in the 1024-point kernels, 16-bit bin indices */
			float l2[8];
			uint32_t bn[8];
			uint32_t amb = 0;
#pragma unroll
			for (int q = 0; q < 8; q++) {
				uint32_t ab;
				const float rr = bin_fast(x[q].x, x[q].y, bk, &l2[q], &ab);
				amb = amb > ab ? amb : ab;
				bn[q] = (uint32_t)(int)__builtin_amdgcn_fmed3f(rr, 0.0f, top);
			}
			if (amb > __float_as_uint(bk.amb)) {
#pragma unroll
				for (int q = 0; q < 8; q++) {
					const float v = __builtin_fmaf(bk.A, l2[q], bk.C);
					const float rr = __builtin_rintf(v);
					const float a = __builtin_fmaf(__builtin_fabsf(l2[q]), bk.kappa, __builtin_fabsf(v - rr));
					if (!(a <= bk.amb)) {
						float nl2;
						bn[q] = bin_exact(x[q].x, x[q].y, l2[q], (int)bn[q], ThrScalar{ bk.thr }, bk.nb, &nl2);
						l2[q] = nl2;
					}
				}
			}
			const bool store_row = (t >= p.wf_first);
			float *wf_row = p.wf + (size_t)((p.wf_pos0 + t) & p.wf_mask) * N + i;
#pragma unroll
			for (int q = 0; q < 8; q++) {
				const int col_off = T * (q & 3) + (N / 2) * (q >> 2);
				pack[q] |= bn[q] << (16 * u);
				live[q] = __builtin_fmaf(live[q], p.w, l2[q]);
				vmax[q] = max_f32(vmax[q], l2[q]);
				if (store_row)
					wf_row[col_off] = l2[q] * F_HALF_LOG10_2;
			}
		}
		uint32_t *dst = p.bins + (size_t)((t0 + g0) >> 1) * N + i;
#pragma unroll
		for (int q = 0; q < 8; q++)
			dst[T * (q & 3) + (N / 2) * (q >> 2)] = pack[q];
	}
	float2 *pp2 = p.partial + (size_t)tile * N + i;
#pragma unroll
	for (int q = 0; q < 8; q++)
		pp2[T * (q & 3) + (N / 2) * (q >> 2)] = make_float2(live[q] * F_HALF_LOG10_2,
			(vmax[q] == vmax_init) ? -1000.0f : vmax[q] * F_HALF_LOG10_2);
	}
}
