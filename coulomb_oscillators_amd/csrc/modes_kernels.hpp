// modes_kernels.hpp -- the density and current modes of a state and their time correlations (include/nbco.h: nbco_modes_record,
// nbco_mode_corr); a section of k_reduce.hip, inside its anonymous namespace.  The rule of a term is modes.hpp.
//
// RECORDING is the tile / power-table scheme of sk_accumulate_kernel (structure_factor_kernels.hpp: items, lanes, copies, tiles and the
// SkShape that describes them are the same), with the velocity of a particle staged beside its tables as two 16-byte slots {vx, vy},
// {vz, 0} -- zeros for a particle that does not count, so that its (0, 0) term meets no NaN.  A lane keeps the four complex sums of A
// consecutive ix in registers, A a template step of at most kMdMaxAcc = 4 (32 doubles of sums; the loop over them is unrolled, the sums
// are never indexed at run time).  A (particle, k) is md_add -- two additions, six fused multiply-adds -- and one complex product for
// the next ix.  The record of a (range, k) goes to part[range][k] -- or straight to its place in the series where there is one range --
// and sk_reduce_kernel<8> adds the ranges in a fixed order.  No atomics; the ranges are a function of n and the grid alone.
//
// THE CORRELATION is the scheme of tc_accumulate_kernel (time_corr_kernels.hpp; TcShape and tc_lag are the same).  A workgroup of 256
// lanes keeps the series of one k in LDS as four arrays of 16-byte slots -- rho, jx, jy, jz, each {re, im} per frame, 64 bytes a frame,
// 1024 frames 64 KiB -- and walks the origins t in increasing order: frame t is one address for the whole wave (a broadcast), frame
// t + tau consecutive addresses for consecutive lanes, read with ds_read_b128 from arrays whose stride is the access width.  P(a) is
// formed once per origin.  A lane keeps A lags in registers, A a template step in {1, 2, 4}; from A = 2 on they come in pairs, one from
// the bottom and one from the top, so that the waves finish together.  Where the W lanes of a k are at most 128, the workgroup serves
// S = 256 / W neighbouring k (S also bounded by the LDS), copy q the k number blockIdx.x * S + q.  A (k, tau) is formed by one lane from
// start to end and written by it: no sum across lanes or workgroups, the bytes of nbco_mode_corr_ref.

constexpr int kMdMaxAcc = 4;            // the largest run of ix a lane keeps (64 VGPRs of sums)
constexpr int kMdExtra = 2;             // the 16-byte slots of a particle beside its tables: the velocity

template <int A>
__global__ __launch_bounds__(kSkBlock) void modes_accumulate_kernel(const float *__restrict__ buf, long long n, SkShape s, double *__restrict__ out, long long ostride)
{
	extern __shared__ double md_lds[];
	const float *__restrict__ p = buf, *__restrict__ vel = buf + 3 * (size_t)n;
	const int tid = (int)threadIdx.x;
	const int tile = s.tile, sy = s.hy + 1, sz = s.hz + 1, nch = s.nch;
	// LDS: ex[tile], vv[tile][2], ty[tile][hy + 1], tz[tile][hz + 1], tc[tile][nch] (nch > 1)
	SkC *ex = reinterpret_cast<SkC *>(md_lds);
	SkC *vv = ex + tile;
	SkC *ty = vv + (size_t)tile * 2;
	SkC *tz = ty + (size_t)tile * sy;
	SkC *tc = tz + (size_t)tile * sz;

	const int copy = tid / s.lanes, lane = tid % s.lanes, S = s.copies;
	const int item = (int)blockIdx.x * s.lanes + lane;
	const bool live = copy < S && item < s.items;
	// item -> (chunk, iy, iz), iz fastest
	const int col = live ? item % (s.ny * s.nz) : 0, chunk = live ? item / (s.ny * s.nz) : 0;
	const int iy = col / s.nz - s.hy, iz = col % s.nz - s.hz;
	const int ay = iy < 0 ? -iy : iy, az = iz < 0 ? -iz : iz;
	const double cy = iy < 0 ? -1.0 : 1.0, cz = iz < 0 ? -1.0 : 1.0;

	MdRec acc[A];
#pragma unroll
	for (int m = 0; m < A; ++m) md_zero(acc[m]);

	const long long lo = (long long)blockIdx.y * s.range;
	const long long hi = lo + s.range < n ? lo + s.range : n;
	for (long long base = lo; base < hi; base += tile)
	{
		const int cnt = hi - base < (long long)tile ? (int)(hi - base) : tile;   // particles of this tile
		__syncthreads();   // the previous tile has been read
		// the base phases and the velocity: one lane per particle
		for (int j = tid; j < cnt; j += kSkBlock)
		{
			const size_t g = (size_t)(base + j);
			SkC zero, first;   // z^0 of a particle: (1, 0) if it counts
			zero.re = zero.im = 0.0;
			const double tx = (double)p[g * 3] * s.wx, t1 = (double)p[g * 3 + 1] * s.wy, t2 = (double)p[g * 3 + 2] * s.wz;
			const float vx = vel[g * 3], vy = vel[g * 3 + 1], vz = vel[g * 3 + 2];
			const bool ok = isfinite(tx) && isfinite(t1) && isfinite(t2) && isfinite(vx) && isfinite(vy) && isfinite(vz);
			first.re = ok ? 1.0 : 0.0; first.im = 0.0;
			SkC e0 = zero, e1 = zero, e2 = zero, v0 = zero, v1 = zero;
			if (ok)
			{
				e0 = sk_phase(tx);
				e1 = sk_phase(t1);
				e2 = sk_phase(t2);
				v0.re = (double)vx; v0.im = (double)vy;
				v1.re = (double)vz;
			}
			ex[j] = e0;
			vv[(size_t)j * 2] = v0;
			vv[(size_t)j * 2 + 1] = v1;
			ty[(size_t)j * sy] = first;
			if (s.hy > 0) ty[(size_t)j * sy + 1] = e1;
			tz[(size_t)j * sz] = first;
			if (s.hz > 0) tz[(size_t)j * sz + 1] = e2;
			if (nch > 1) tc[(size_t)j * nch] = first;
		}
		__syncthreads();
		sk_power_tables<true>(s, cnt, ex, ty, tz, tc);
		__syncthreads();
		if (live)
		{
			for (int j = copy; j < cnt; j += S)
			{
				SkC w = ty[(size_t)j * sy + ay];
				w.im *= cy;
				SkC b = tz[(size_t)j * sz + az];
				b.im *= cz;
				w = sk_mul(w, b);
				if (nch > 1) w = sk_mul(w, tc[(size_t)j * nch + chunk]);
				const SkC e = ex[j], v0 = vv[(size_t)j * 2], v1 = vv[(size_t)j * 2 + 1];
#pragma unroll
				for (int m = 0; m < A; ++m)
				{
					md_add(acc[m], w, v0.re, v0.im, v1.re);
					if (m + 1 < A) w = sk_mul(w, e);
				}
			}
		}
	}
	if (S > 1)
	{
		// the copies of an item, added in the order of the copies: every lane lends one complex sum at a time, copy 0 collects
		SkC *red = reinterpret_cast<SkC *>(md_lds);
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			SkC v[4] = {acc[m].rho, acc[m].jx, acc[m].jy, acc[m].jz};
#pragma unroll
			for (int c = 0; c < 4; ++c)
			{
				__syncthreads();   // the last tile, or the sum before this one, has been read
				red[tid] = v[c];
				__syncthreads();
				if (live && copy == 0)
					for (int q = 1; q < S; ++q)
					{
						const SkC u = red[q * s.lanes + lane];
						v[c].re += u.re;
						v[c].im += u.im;
					}
			}
			acc[m].rho = v[0]; acc[m].jx = v[1]; acc[m].jy = v[2]; acc[m].jz = v[3];
		}
	}
	if (live && copy == 0)
	{
		double *o = out + (size_t)blockIdx.y * 8 * (size_t)s.K;   // (one range: blockIdx.y == 0)
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			const int ix = chunk * s.L + m;
			if (m < s.L && ix <= s.hx)
			{
				const size_t k = ((size_t)ix * s.ny + (size_t)(iy + s.hy)) * s.nz + (size_t)(iz + s.hz);
				double *r = o + k * (size_t)ostride;   // (doubles: the caller's buffer is aligned as doubles are, no more is asked)
				r[0] = acc[m].rho.re; r[1] = acc[m].rho.im;
				r[2] = acc[m].jx.re; r[3] = acc[m].jx.im;
				r[4] = acc[m].jy.re; r[5] = acc[m].jy.im;
				r[6] = acc[m].jz.re; r[7] = acc[m].jz.im;
			}
		}
	}
}

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

	int tau[A], end[A];   // end: the origins of this lag, frames - tau (0: none)
	MdSum acc[A];
	int tend = 0;         // the origins this lane has any lag for
#pragma unroll
	for (int m = 0; m < A; ++m)
	{
		const int l = live ? tc_lag<A>(s, lane, m) : -1;
		tau[m] = l < 0 ? 0 : l;
		end[m] = l < 0 ? 0 : frames - l;
		tend = end[m] > tend ? end[m] : tend;
		md_sum_zero(acc[m]);
	}
	// (the bound of the wave, so that the loop's branch is uniform)
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(tend, d);
		tend = o > tend ? o : tend;
	}
	tend = __builtin_amdgcn_readfirstlane(tend);

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
