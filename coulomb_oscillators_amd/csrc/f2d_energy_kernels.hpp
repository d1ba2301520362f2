// f2d_energy_kernels.hpp -- part of k_fmm2d.hip (included there, in this place: one translation unit, one anonymous namespace)
// 2-D energy diagnostics: kinetic / elastic sums, the exact pair potential and the FMM potential pass
// (no include guard on purpose: this is a section of that file, not a header)
// ---- 2-D potential energy (no reference driver computes an energy) ---------------------------------------------------------------
// The pair law a_i = param[0] sum_j d / (|d|^2 + EPS2) is minus the gradient of psi_i = -param[0] phi_i with
//   phi_i = sum_{j != i} 1/2 log(|x_i - x_j|^2 + EPS2)        (j != i by INDEX: coincident particles contribute 1/2 log EPS2)
// and coulomb = 1/2 sum_i psi_i.  In the complex form of this file W(z) = sum_j log(z - z_j) has W' = f and Re W = sum_j log|z - z_j|,
// so the field's local expansion f(u) = sum_{l<p} b_l u^l is the potential's too, up to one real constant c0 per cell:
//   Re W(u) = c0 + Re sum_{l<p} b_l u^(l+1) / (l+1)
//   M2L     c0 += a_0 1/2 log(|D|^2 + EPS2) - Re sum_{k=2..p} a_k w^k / k     (same stencil, same softened w = 1/D as the field's M2L)
//   L2L     c0_child += c0_parent + Re sum_{l<p} b^parent_l d^(l+1) / (l+1)   (the parent's FINAL locals and c0)
//   L2P     phi_i = near pairs + c0 + Re sum_l b_l u^(l+1) / (l+1),  u = z_i - c_leaf
// Every sum has a fixed order (per lane, per block into its own slot, one block over the slots): no atomics, same bits every call.

// kinetic = 1/2 sum |v|^2 and elastic = 1/2 sum (kx x^2 + ky y^2) in one pass (k_reduce.hip energy1_stage1, in doubles)
__global__ __launch_bounds__(kB) void f2d_kin_ela_kernel(const double2 *__restrict__ x, const double2 *__restrict__ v, long long n,
                                                         const double *__restrict__ k, double *__restrict__ part)
{
	__shared__ double sh[kB];
	const double kx = k[0], ky = k[1];
	double kin = 0, ela = 0;
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const double2 p = x[i], u = v[i];
		kin += 0.5 * (u.x * u.x + u.y * u.y);
		ela += 0.5 * (kx * p.x * p.x + ky * p.y * p.y);
	}
	const double s0 = block_sum(kin, sh), s1 = block_sum(ela, sh);
	if (threadIdx.x == 0)
	{
		part[2 * blockIdx.x] = s0;
		part[2 * blockIdx.x + 1] = s1;
	}
}

// exact pair potential: one target per thread, sources staged through LDS as an x-row and a y-row (f2d_direct_kernel's shape);
// the self pair is skipped by index.  part[block] = sum over the block's targets of sum_{j != i} log(r^2 + EPS2) (the 1/2 and
// param[0] are applied once, in f2d_energy_final_kernel); psi, if given, receives psi_i.
__global__ __launch_bounds__(kB) void f2d_pair_pot_kernel(const double2 *__restrict__ x, long long n, double eps2, const double *__restrict__ param,
                                                          double *__restrict__ psi, double *__restrict__ part)
{
	__shared__ double sx[kB], sy[kB];
	const long long i = (long long)blockIdx.x * kB + threadIdx.x;
	const double2 zi = i < n ? x[i] : make_double2(0.0, 0.0);
	double acc = 0;
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
		for (int t = 0; t < cnt; ++t)
		{
			const double dx = zi.x - sx[t], dy = zi.y - sy[t];
			const double lg = log(dx * dx + dy * dy + eps2);
			acc += (j0 + t == i) ? 0.0 : lg;
		}
	}
	if (i >= n) acc = 0;
	if (psi && i < n) psi[i] = -param[0] * 0.5 * acc;
	__syncthreads();   // sx is the reduction's scratch from here on
	const double s = block_sum(acc, sx);
	if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out = {kinetic, elastic, coulomb}: one block sums the slots of the two stages in a fixed order; coulomb = -param[0] / 4 * sum of logs
__global__ __launch_bounds__(kB) void f2d_energy_final_kernel(const double *__restrict__ ke, int nke, const double *__restrict__ pot, long long npot,
                                                              const double *__restrict__ param, double *__restrict__ out)
{
	__shared__ double sh[kB];
	double kin = 0, ela = 0, lg = 0;
	for (int i = threadIdx.x; i < nke; i += kB)
	{
		kin += ke[2 * i];
		ela += ke[2 * i + 1];
	}
	for (long long i = threadIdx.x; i < npot; i += kB) lg += pot[i];
	const double s0 = block_sum(kin, sh), s1 = block_sum(ela, sh), s2 = block_sum(lg, sh);
	if (threadIdx.x == 0)
	{
		out[0] = s0;
		out[1] = s1;
		out[2] = -param[0] * 0.25 * s2;
	}
}

// gather of the positions alone into scratch: the energy pass leaves the caller's buffer as it is
__global__ __launch_bounds__(kB) void f2d_gather_pos_kernel(const double2 *__restrict__ x, const uint32_t *__restrict__ idx, double2 *__restrict__ out, long long n)
{
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB) out[i] = x[idx[i]];
}

// the constant of the M2L: one thread per cell of levels 2..L, the stencil loop and the empty-cell skips of f2d_m2l_kernel.
// Writes (not accumulates) c0; an empty cell gets 0.
template <int P>
__global__ __launch_bounds__(kB) void f2d_m2l0_kernel(Quad q, double *__restrict__ c0, int L, int radius, double eps2)
{
	const long long cell = quad_beg(2) + (long long)blockIdx.x * kB + threadIdx.x;
	if (cell >= quad_beg(L + 1)) return;
	int l = 2;
	while (cell >= quad_beg(l + 1)) ++l;
	const long long beg = quad_beg(l);
	const int side = 1 << l;
	const int ij = (int)(cell - beg), i = ij / side, j = ij - i * side;
	double acc = 0;
	if (q.mult[cell] > 0)
	{
		const double2 ct = q.center[cell];
		const int im = (i / 2) * 2, jm = (j / 2) * 2;
		const int kmin = std::max(im - 2 * radius, 0), kmax = std::min(im + 2 * radius + 1, side - 1);
		const int gmin = std::max(jm - 2 * radius, 0), gmax = std::min(jm + 2 * radius + 1, side - 1);
		for (int k = kmin; k <= kmax; ++k)
			for (int g = gmin; g <= gmax; ++g)
			{
				if (!(k > i + radius || k < i - radius || g > j + radius || g < j - radius)) continue;
				const long long src = beg + (long long)k * side + g;
				if (q.mult[src] == 0) continue;
				const double2 cs = q.center[src];
				const double dx = ct.x - cs.x, dy = ct.y - cs.y;
				const double r2 = dx * dx + dy * dy + eps2;
				const double2 w = make_double2(dx / r2, -dy / r2);
				double t = q.mpole[src * (P + 1)].x * (0.5 * log(r2));
				double2 wk = w;
#pragma unroll
				for (int kk = 2; kk <= P; ++kk)
				{
					wk = cmul(wk, w);
					const double2 a = q.mpole[src * (P + 1) + kk];
					t -= (a.x * wk.x - a.y * wk.y) / (double)kk;
				}
				acc += t;
			}
	}
	c0[cell] = acc;
}

// the constant's L2L into the non-empty cells of level l: the parent's final locals and c0 (level l - 1 is complete)
template <int P>
__global__ __launch_bounds__(kB) void f2d_l2l0_kernel(Quad q, double *__restrict__ c0, int l)
{
	const int side = 1 << l;
	const int ij0 = blockIdx.x * kB + threadIdx.x;
	if (ij0 >= side * side) return;
	const long long cell = quad_beg(l) + ij0;
	if (q.mult[cell] == 0) return;
	const int i = ij0 / side, j = ij0 - i * side;
	const long long par = quad_beg(l - 1) + (long long)(i / 2) * (side / 2) + j / 2;
	const double2 cp = q.center[par], cc = q.center[cell];
	const double2 d = make_double2(cc.x - cp.x, cc.y - cp.y);
	// Re sum_l b_l d^(l+1) / (l+1) by Horner
	double2 g = cscale(q.local[par * P + P - 1], 1.0 / (double)P);
#pragma unroll
	for (int k = P - 2; k >= 0; --k) g = cadd(cmul(g, d), cscale(q.local[par * P + k], 1.0 / (double)(k + 1)));
	g = cmul(g, d);
	c0[cell] += c0[par] + g.x;
}

// Near-field potential fused with the L2P: f2d_near_kernel's shape (one wave per target leaf, one target per lane, each neighbour
// row staged 64 sources at a time, grid-stride over the leaves) with log(r^2 + EPS2) as the pair body.  The self pair is the source
// whose place in the sorted array is the target's; it may sit in any tile of the row.  psi goes back to the caller's order
// through the sort's index array.  part[block] = sum over the block's targets of (sum of pair logs + 2 far_i): the final kernel's
// factor -param[0] / 4 makes that 1/2 sum psi.
template <int P>
__global__ __launch_bounds__(kNear) void f2d_near_pot_kernel(Quad q, const double *__restrict__ c0, const double2 *__restrict__ x,
                                                             const uint32_t *__restrict__ idx, int L, int radius, double eps2,
                                                             const double *__restrict__ param, double *__restrict__ psi, double *__restrict__ part)
{
	__shared__ double sx[kNear], sy[kNear];
	const int side = 1 << L;
	const int m = side * side;
	const double s0 = param[0];
	const int lane = threadIdx.x;
	double total = 0;   // this lane's targets over all leaves of the block
	for (int cell = blockIdx.x; cell < m; cell += gridDim.x)
	{
	const int b = q.index[cell], e = q.index[cell + 1];
	if (b == e) continue;   // uniform across the block
	const long long qc = quad_beg(L) + cell;
	const int i = cell / side, j = cell - i * side;
	const int kmin = std::max(i - radius, 0), kmax = std::min(i + radius, side - 1);
	const int lmin = std::max(j - radius, 0), lmax = std::min(j + radius, side - 1);
	const double2 c = q.center[qc];
	const double cc0 = c0[qc];
	double2 bl[P];
#pragma unroll
	for (int k = 0; k < P; ++k) bl[k] = cscale(q.local[qc * P + k], 1.0 / (double)(k + 1));
	for (int t0 = b; t0 < e; t0 += kNear)
	{
		const int t = t0 + lane;
		const bool act = t < e;
		const double2 zi = act ? x[t] : make_double2(0.0, 0.0);
		double lg = 0;
		for (int k = kmin; k <= kmax; ++k)
		{
			const int rs = q.index[k * side + lmin], re = q.index[k * side + lmax + 1];
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
				const int self = t - s0r;   // the target's own slot in this tile, if 0 <= self < cnt
				for (int u = 0; u < cnt; ++u)
				{
					const double dx = zi.x - sx[u], dy = zi.y - sy[u];
					const double v = log(dx * dx + dy * dy + eps2);
					lg += (u == self) ? 0.0 : v;
				}
			}
		}
		// L2P: Re W(u) = c0 + Re (u sum_l b_l / (l+1) u^l) by Horner
		const double2 u = make_double2(zi.x - c.x, zi.y - c.y);
		double2 g = bl[P - 1];
#pragma unroll
		for (int k = P - 2; k >= 0; --k) g = cadd(cmul(g, u), bl[k]);
		g = cmul(g, u);
		const double both = lg + 2.0 * (cc0 + g.x);   // 2 phi_i
		if (act)
		{
			total += both;
			if (psi) psi[idx[t]] = -s0 * 0.5 * both;
		}
	}
	__syncthreads();   // the next leaf overwrites the LDS rows
	}
	__syncthreads();
	sx[lane] = total;
	__syncthreads();
	if (lane == 0)
	{
		double s = 0;
		for (int k = 0; k < kNear; ++k) s += sx[k];
		part[blockIdx.x] = s;
	}
}
