// modes_kernels.hpp -- the density and current modes of a state and their time correlations (include/nbco.h: nbco_modes_record,
// nbco_mode_corr); a section of k_reduce.hip, inside its anonymous namespace.  The rule of a term is modes.hpp.
//
// RECORDING is kgrid_accumulate_kernel (structure_factor_kernels.hpp) with MdTerm: the same kernel, items, lanes, copies, tiles and
// SkShape as nbco_structure_factor.  MdTerm stages the velocity of a particle beside its tables as two 16-byte slots {vx, vy},
// {vz, 0} -- zeros for a particle that does not count, so that its (0, 0) term meets no NaN.  A lane keeps the four complex sums of A
// consecutive ix in registers, A a template step of at most 4 (32 doubles of sums).  A (particle, k) is md_add -- two additions, six
// fused multiply-adds -- and one complex product for the next ix.  sk_reduce_kernel<8> adds the ranges.
//
// THE CORRELATION is the scheme of tc_accumulate_kernel (time_corr_kernels.hpp; TcShape, tc_lag and tc_lag_slots are the same).  A workgroup of 256
// lanes keeps the series of one k in LDS as four arrays of 16-byte slots -- rho, jx, jy, jz, each {re, im} per frame, 64 bytes a frame,
// 1024 frames 64 KiB -- and walks the origins t in increasing order: frame t is one address for the whole wave (a broadcast), frame
// t + tau consecutive addresses for consecutive lanes, read with ds_read_b128 from arrays whose stride is the access width.  P(a) is
// formed once per origin.  A lane keeps A lags in registers, A a template step in {1, 2, 4}; from A = 2 on they come in pairs, one from
// the bottom and one from the top, so that the waves finish together.  Where the W lanes of a k are at most 128, the workgroup serves
// S = 256 / W neighbouring k (S also bounded by the LDS), copy q the k number blockIdx.x * S + q.  A (k, tau) is formed by one lane from
// start to end and written by it: no sum across lanes or workgroups, the bytes of nbco_mode_corr_ref.

// the term of nbco_modes_record (the members: SkTerm)
struct MdTerm
{
	using Acc = MdRec;
	using Steps = std::integer_sequence<int, 1, 2, 3, 4>;   // (the last: 64 VGPRs of sums)
	static constexpr int kExtra = 2;                        // the velocity
	static constexpr int kParts = 4;                        // rho, jx, jy, jz
	static __device__ __forceinline__ void zero(Acc &a) { md_zero(a); }
	// the rows are the state: n positions, then n velocities
	static __device__ __forceinline__ bool stage(const float *p, long long n, size_t g, bool ok, SkC *slot)
	{
		const float *v = p + 3 * (size_t)n + 3 * g;
		const float vx = v[0], vy = v[1], vz = v[2];
		ok = ok && isfinite(vx) && isfinite(vy) && isfinite(vz);
		slot[0].re = ok ? (double)vx : 0.0; slot[0].im = ok ? (double)vy : 0.0;
		slot[1].re = ok ? (double)vz : 0.0; slot[1].im = 0.0;
		return ok;
	}
	static __device__ __forceinline__ void add(Acc &a, SkC w, const SkC *slot) { md_add(a, w, slot[0].re, slot[0].im, slot[1].re); }
	static __device__ __forceinline__ SkC &part(Acc &a, int c) { return c == 0 ? a.rho : c == 1 ? a.jx : c == 2 ? a.jy : a.jz; }
};

template <int A>
__global__ __launch_bounds__(kTcBlock) void mode_corr_kernel(const double *__restrict__ series, long long K, nbco_sk_grid g, TcShape s, nbco_mode_lag *__restrict__ out)
{
	extern __shared__ double2 mc_lds[];
	const int tid = (int)threadIdx.x;
	const int copy = tid / s.W, lane = tid % s.W;
	const int frames = s.frames;
	const long long k = (long long)blockIdx.x * s.S + copy;
	const bool live = copy < s.S && k < K;
	double2 *prho = mc_lds + (size_t)(copy < s.S ? copy : 0) * 4 * (size_t)frames;   // this copy's series: rho, jx, jy, jz
	double2 *pjx = prho + frames, *pjy = pjx + frames, *pjz = pjy + frames;

	int tau[A], end[A];
	MdSum acc[A];
	const int tend = tc_lag_slots<A>(s, live, lane, tau, end);
#pragma unroll
	for (int m = 0; m < A; ++m) md_sum_zero(acc[m]);

	if (live)
	{
		const double *src = series + (size_t)k * (size_t)s.cap * 8;   // (read as doubles: no alignment beyond theirs is asked of the caller)
		for (int f = lane; f < frames; f += s.W)
		{
			const double *r = src + 8 * (size_t)f;
			prho[f] = make_double2(r[0], r[1]);
			pjx[f] = make_double2(r[2], r[3]);
			pjy[f] = make_double2(r[4], r[5]);
			pjz[f] = make_double2(r[6], r[7]);
		}
	}
	__syncthreads();
	if (!live) return;
	double kv[3];
	md_wave_vector(k, g.h, g.kstep, kv);
	for (int t = 0; t < tend; ++t)
	{
		// every read of this origin is issued before the first is used (a lag past its end reads frame t again and is masked below)
		const double2 a0 = prho[t], a1 = pjx[t], a2 = pjy[t], a3 = pjz[t];
		double2 b0[A], b1[A], b2[A], b3[A];
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			const int f = t < end[m] ? t + tau[m] : t;
			b0[m] = prho[f];
			b1[m] = pjx[f];
			b2[m] = pjy[f];
			b3[m] = pjz[f];
		}
		SkC arho, ajx, ajy, ajz;
		arho.re = a0.x; arho.im = a0.y; ajx.re = a1.x; ajx.im = a1.y; ajy.re = a2.x; ajy.im = a2.y; ajz.re = a3.x; ajz.im = a3.y;
		const SkC pa = md_long(kv[0], kv[1], kv[2], ajx, ajy, ajz);
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			if (t < end[m])
			{
				SkC brho, bjx, bjy, bjz;
				brho.re = b0[m].x; brho.im = b0[m].y; bjx.re = b1[m].x; bjx.im = b1[m].y;
				bjy.re = b2[m].x; bjy.im = b2[m].y; bjz.re = b3[m].x; bjz.im = b3[m].y;
				md_term(acc[m], kv[0], kv[1], kv[2], arho, ajx, ajy, ajz, pa, brho, bjx, bjy, bjz);
			}
		}
	}
	nbco_mode_lag *o = out + (size_t)k * (size_t)s.lags;
#pragma unroll
	for (int m = 0; m < A; ++m)
	{
		if (end[m] > 0)
		{
			nbco_mode_lag r;
			r.rr = acc[m].rr; r.ll = acc[m].ll; r.jj = acc[m].jj;
			r.s0[0] = acc[m].s0.re; r.s0[1] = acc[m].s0.im;
			r.s1[0] = acc[m].s1.re; r.s1[1] = acc[m].s1.im;
			r.pairs = (unsigned long long)end[m];
			o[tau[m]] = r;
		}
	}
}
