// f2d_probe_kernels.hpp -- part of k_fmm2d.hip (included there, in this place: one translation unit, one anonymous namespace)
// 2-D probe evaluation: field and potential of the sources at points that are not particles
// (no include guard on purpose: this is a section of that file, not a header)
// ---- probes (no reference driver evaluates the field away from the particles) ----------------------------------------------------
// Every source counts at every probe t_i; there is no self exclusion, because a probe is not a particle:
//   a_i   =  param[0] sum_j d / (|d|^2 + EPS2),  d = t_i - x_j
//   psi_i = -param[0] sum_j 1/2 log(|d|^2 + EPS2)                 (a_i = -grad psi_i)
// The FMM call evaluates the multipoles at the probe itself instead of going through the locals: a leaf without sources has no
// local expansion (f2d_m2l_kernel / f2d_l2l_kernel skip it) and no centre, and a probe outside the sources' square is keyed into
// a border cell whose local expansion is not valid there.  With D = t_i - c_source and the M2L's softened w = conj(D) / (|D|^2 + EPS2)
//   f   += a_0 w + sum_{k=2..p} a_k w^(k+1)  = w (a_0 + sum_k a_k w^k),   field = conj(f)       (b_0 of f2d_m2l_kernel)
//   W   += a_0 1/2 log(|D|^2 + EPS2) - Re sum_{k=2..p} a_k w^k / k                                (the body of f2d_m2l0_kernel)
// over the M2L stencil of the probe's ancestor at every level 2..L.  All sources and centroids lie in the square, so the
// projection of a probe onto it (the clamp of f2d_keys_kernel) only shortens distances: the series converge at the probe at
// least as well as at its projection.  Every sum has a fixed order that depends on the tree and the probe's position alone.

// exact sums: one probe per thread, the sources staged through LDS as an x-row and a y-row (f2d_direct_kernel's shape)
template <bool WANT_A, bool WANT_PSI>
__global__ __launch_bounds__(kB) void f2d_probe_direct_kernel(const double2 *x, long long n, const double2 *t, long long m, double eps2,
                                                              const double *__restrict__ param, double2 *__restrict__ a, double *__restrict__ psi)
{
	__shared__ double sx[kB], sy[kB];
	const long long i = (long long)blockIdx.x * kB + threadIdx.x;
	const double2 zi = i < m ? t[i] : make_double2(0.0, 0.0);
	double ax = 0, ay = 0, lg = 0;
	for (long long j0 = 0; j0 < n; j0 += kB)
	{
		__syncthreads();
		const long long j = j0 + threadIdx.x;
		if (j < n)
		{
			const double2 s = x[j];
			sx[threadIdx.x] = s.x;
			sy[threadIdx.x] = s.y;
		}
		__syncthreads();
		const int cnt = (int)std::min<long long>(kB, n - j0);
		for (int u = 0; u < cnt; ++u)
		{
			const double dx = zi.x - sx[u], dy = zi.y - sy[u];
			const double r2 = dx * dx + dy * dy + eps2;
			if (WANT_A)
			{
				const double inv = 1.0 / r2;
				ax += dx * inv;
				ay += dy * inv;
			}
			if (WANT_PSI) lg += log(r2);
		}
	}
	if (i >= m) return;
	const double s0 = param[0];
	if (WANT_A) a[i] = make_double2(ax * s0, ay * s0);
	if (WANT_PSI) psi[i] = -s0 * 0.5 * lg;
}

// Near field and multipole-to-probe: f2d_near_kernel's shape (one wave per leaf that holds probes, one probe per lane in chunks of
// kNear, each neighbour row of SOURCES staged 64 at a time, grid-stride over the leaves).  pindex is the leaf index of the sorted
// probe keys, pidx the probes' sort permutation: positions are read and results written through it, in the caller's order.
// The stencil walk depends on the leaf alone, so the centre, multiplicity and multipole reads are the same address in every lane.
template <int P, bool WANT_A, bool WANT_PSI>
__global__ __launch_bounds__(kNear) void f2d_probe_kernel(const double2 *__restrict__ center, const double2 *__restrict__ mpole,
                                                          const int *__restrict__ mult, const int *__restrict__ sindex,
                                                          const int *__restrict__ pindex, const uint32_t *__restrict__ pidx,
                                                          const double2 *__restrict__ x, const double2 *t, int L, int radius, double eps2,
                                                          const double *__restrict__ param, double2 *__restrict__ a, double *__restrict__ psi)
{
	__shared__ double sx[kNear], sy[kNear];
	const int side = 1 << L;
	const int m = side * side;
	const double s0 = param[0];
	const int lane = threadIdx.x;
	for (int cell = blockIdx.x; cell < m; cell += gridDim.x)
	{
	const int b = pindex[cell], e = pindex[cell + 1];
	if (b == e) continue;   // uniform across the block
	const int i = cell / side, j = cell - i * side;
	const int kmin = std::max(i - radius, 0), kmax = std::min(i + radius, side - 1);
	const int lmin = std::max(j - radius, 0), lmax = std::min(j + radius, side - 1);
	for (int t0 = b; t0 < e; t0 += kNear)
	{
		const bool act = t0 + lane < e;
		const uint32_t dst = act ? pidx[t0 + lane] : 0u;
		const double2 zi = act ? t[dst] : make_double2(0.0, 0.0);
		double ax = 0, ay = 0, lg = 0;
		// near field: the sources of the leaf's 2r+1 neighbour rows; the leaf itself may hold none
		for (int k = kmin; k <= kmax; ++k)
		{
			const int rs = sindex[k * side + lmin], re = sindex[k * side + lmax + 1];
			for (int s0r = rs; s0r < re; s0r += kNear)
			{
				__syncthreads();
				if (s0r + lane < re)
				{
					const double2 sp = x[s0r + lane];
					sx[lane] = sp.x;
					sy[lane] = sp.y;
				}
				__syncthreads();
				const int cnt = std::min(kNear, re - s0r);
				for (int u = 0; u < cnt; ++u)
				{
					const double dx = zi.x - sx[u], dy = zi.y - sy[u];
					const double r2 = dx * dx + dy * dy + eps2;
					if (WANT_A)
					{
						const double inv = 1.0 / r2;
						ax += dx * inv;
						ay += dy * inv;
					}
					if (WANT_PSI) lg += log(r2);
				}
			}
		}
		// far field: the M2L stencil of the leaf's ancestor at every level, each source's multipole evaluated at the probe
		double2 f = make_double2(0.0, 0.0);
		double W = 0;
		for (int l = L; l >= 2; --l)
		{
			const int sh = L - l, sl = 1 << l;
			const int ci = i >> sh, cj = j >> sh;
			const long long beg = quad_beg(l);
			const int im = (ci / 2) * 2, jm = (cj / 2) * 2;
			const int k0 = std::max(im - 2 * radius, 0), k1 = std::min(im + 2 * radius + 1, sl - 1);
			const int g0 = std::max(jm - 2 * radius, 0), g1 = std::min(jm + 2 * radius + 1, sl - 1);
			for (int k = k0; k <= k1; ++k)
				for (int g = g0; g <= g1; ++g)
				{
					if (!(k > ci + radius || k < ci - radius || g > cj + radius || g < cj - radius)) continue;
					const long long src = beg + (long long)k * sl + g;
					if (mult[src] == 0) continue;
					const double2 cs = center[src];
					const double dx = zi.x - cs.x, dy = zi.y - cs.y;
					const double r2 = dx * dx + dy * dy + eps2;
					const double2 w = make_double2(dx / r2, -dy / r2);
					const double a0 = mpole[src * (P + 1)].x;
					double2 s = make_double2(a0, 0.0);   // a_0 + sum_k a_k w^k
					double tw = WANT_PSI ? a0 * (0.5 * log(r2)) : 0.0;
					double2 wk = w;
#pragma unroll
					for (int kk = 2; kk <= P; ++kk)
					{
						wk = cmul(wk, w);
						const double2 pk = cmul(mpole[src * (P + 1) + kk], wk);
						s = cadd(s, pk);
						if (WANT_PSI) tw -= pk.x * (1.0 / (double)kk);
					}
					if (WANT_A) f = cadd(f, cmul(s, w));
					if (WANT_PSI) W += tw;
				}
		}
		if (act)
		{
			if (WANT_A) a[dst] = make_double2((ax + f.x) * s0, (ay - f.y) * s0);
			if (WANT_PSI) psi[dst] = -s0 * (0.5 * lg + W);
		}
	}
	__syncthreads();   // the next leaf overwrites the LDS rows
	}
}
