// k_fmm2d.hip -- the 2-D fp64 evaluators of the reference's `nbco` program (Simulation/main.cu, DIM 2, SCAL double):
// the -log r pair law a_i += d / (|d|^2 + EPS2), d = x_i - x_j (direct.cuh:23-26, appel.cuh:293-297), the direct sums
// `direct2` / `direct3` (direct.cuh:171,233) and the uniform-quadtree FMM `fmm_cart` (fmm_cart.cuh:395-544), plus the
// double-precision step / elastic / rescale kernels and the integrator sequence of integrator.cuh:32-167.
//
// FMM in complex form.  With z = x + iy and f(z) = sum_j 1 / (z - z_j), the field is a = conj(f).  A 2-D traceless tensor of
// order k has two components, so the reference's expansions map one-to-one onto complex coefficients:
//   multipole about c   a_k = sum_j (z_j - c)^k,  k = 0..p (a_1 = 0 about the centroid, not computed: fmm_cart.cuh:68-96)
//   local about c       f(z) = sum_l b_l (z - c)^l,  l = 0..p-1 (the reference's local orders 1..p, the field's Taylor terms)
//   M2L                 b_l += (-1)^l C(k+l, l) a_k w^(k+l+1),  w = conj(D) / (|D|^2 + EPS2) (= 1/D softened), D = c_t - c_s
//                       square truncation: k = 0..p, l = 0..p-1, total order k + l + 1 = 1..2p (fmm_cart_base.cuh:757-798)
//   M2M / L2L           exact binomial shifts of the truncated series (fmm_cart.cuh:116-188, 288-334)
// Cells are the reference's: keys ix * side + iy with x slowest (appel.cuh:44-55), a stable radix sort over 2L bits, and
// positions AND velocities left in cell order (fmm_cart.cuh:500-504).
//
// Kernel plan per evaluation (L levels): minmax partials, scalars, keys, radix sort, gather, cell ranges, P2M, L-2 M2M, one M2L
// launch for all levels, L-2 L2L, and the near field fused with L2P and the rescale.  No atomics anywhere: every sum has a fixed
// order, so results are bit-reproducible.
//
// Energy diagnostics (f2d_energy_kernels.hpp): nbco_2d_energy sums the pair potential exactly; nbco_2d_energy_fmm builds the same
// tree over a scratch copy of the positions and carries one real constant per cell next to the field's locals.
//
// Probes (f2d_probe_kernels.hpp): nbco_2d_probe sums field and potential of the sources at arbitrary points exactly;
// nbco_2d_probe_fmm builds that tree up to the multipoles and evaluates them at the probes, leaf by leaf in the probes' key order.
#include "nbco_internal.hpp"
#include "host_util.hpp"
#include "integ_compose.hpp"
#include "helix.hpp"
#include "bath.hpp"
#include <algorithm>
#include <string>
#include <cmath>
#include <random>

namespace {

constexpr int kB = 256;        // threads per block of the 1-D kernels
constexpr int kNear = 64;      // one wave per target cell in the near-field kernel
constexpr int kRedBlocks = 512;
constexpr int kMaxL2 = 15;     // 2L <= 30: keys stay below 2^30

constexpr int kGridCap = 1 << 20;   // blocks of a grid-stride launch
__host__ __device__ inline long long quad_beg(int l) { return ((1LL << (2 * l)) - 1) / 3; }

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 cscale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }

__host__ __device__ constexpr double binom(int n, int k)
{
	double r = 1;
	for (int i = 1; i <= k; ++i) r = r * (double)(n - k + i) / (double)i;
	return r;
}

// ---- basic fp64 kernels (kernel.cuh:100 step, :119 add_elastic, appel.cuh:514 rescale) -----------------------------------------
__global__ __launch_bounds__(kB) void f2d_axpy_kernel(double *__restrict__ b, const double *__restrict__ a, double ds, long long n2)
{
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n2; i += (long long)gridDim.x * kB) b[i] += a[i] * ds;
}

// the drift in a uniform magnetic field out of the plane (include/nbco.h, nbco_2d_drift_b): x += A v, v = R v, both from the old v
__global__ __launch_bounds__(kB) void f2d_drift_b_kernel(double2 *__restrict__ x, double2 *__restrict__ v, Helix2 h, long long n)
{
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		double2 p = x[i];
		const double2 u = v[i];
		p.x = fma(h.A[1], u.y, fma(h.A[0], u.x, p.x));
		p.y = fma(h.A[3], u.y, fma(h.A[2], u.x, p.y));
		x[i] = p;
		v[i] = make_double2(fma(h.R[1], u.y, h.R[0] * u.x), fma(h.R[3], u.y, h.R[2] * u.x));
	}
}

// the Langevin bath step O(s) on the velocities (include/nbco.h, nbco_2d_bath_apply; bath.hpp), one particle per lane
__global__ __launch_bounds__(kB) void f2d_bath_kernel(double2 *__restrict__ v, Bath2 b, long long n)
{
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const double2 u = v[i];
		double w[2] = {u.x, u.y};
		bath_kick(b, i, w);
		v[i] = make_double2(w[0], w[1]);
	}
}

__global__ __launch_bounds__(kB) void f2d_elastic_kernel(const double2 *__restrict__ x, double2 *__restrict__ a, long long n,
                                                         const double *__restrict__ k)
{
	const double kx = k[0], ky = k[1];
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		double2 t = a[i];
		const double2 p = x[i];
		t.x -= kx * p.x;
		t.y -= ky * p.y;
		a[i] = t;
	}
}

// ---- direct sums: all pairs, sources staged through LDS as an x-row and a y-row ------------------------------------------------
template <bool KAHAN>
__global__ __launch_bounds__(kB) void f2d_direct_kernel(const double2 *__restrict__ x, double2 *__restrict__ a, long long n, double eps2,
                                                        const double *__restrict__ param)
{
	__shared__ double sx[kB], sy[kB];
	const long long i = (long long)blockIdx.x * kB + threadIdx.x;
	const double2 zi = i < n ? x[i] : make_double2(0.0, 0.0);
	double ax = 0, ay = 0, cx = 0, cy = 0;
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
			const double inv = 1.0 / (dx * dx + dy * dy + eps2);
			if (KAHAN)
			{
				// compensated accumulation (direct.cuh:233 direct3)
				const double tx = dx * inv - cx, ty = dy * inv - cy;
				const double nx = ax + tx, ny = ay + ty;
				cx = (nx - ax) - tx;
				cy = (ny - ay) - ty;
				ax = nx;
				ay = ny;
			}
			else
			{
				ax += dx * inv;
				ay += dy * inv;
			}
		}
	}
	if (i < n)
	{
		const double s = param ? param[0] : 1.0;
		a[i] = make_double2(ax * s, ay * s);
	}
}

// ---- mean relative error (reductions.cuh:99 relerrReduce2): fixed-order block sums, then one block over the partials ------------
__device__ double block_sum(double v, double *sh)
{
	sh[threadIdx.x] = v;
	__syncthreads();
	for (int s = kB / 2; s > 0; s >>= 1)
	{
		if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
		__syncthreads();
	}
	const double r = sh[0];
	__syncthreads();
	return r;
}

__global__ __launch_bounds__(kB) void f2d_relerr_kernel(const double2 *__restrict__ x, const double2 *__restrict__ ref, long long n,
                                                        double *__restrict__ part)
{
	__shared__ double sh[kB];
	double acc = 0;
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const double2 p = x[i], q = ref[i];
		const double dx = p.x - q.x, dy = p.y - q.y;
		// rel_diff1 (reductions.cuh:37-42): the reference row's |ref|^2 is offset by 1e-18
		acc += std::sqrt(fmax((dx * dx + dy * dy) / (q.x * q.x + q.y * q.y + 1e-18), 0.0));
	}
	const double s = block_sum(acc, sh);
	if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kB) void f2d_relerr_final_kernel(const double *__restrict__ part, int nb, long long n, double *__restrict__ out)
{
	__shared__ double sh[kB];
	double acc = 0;
	for (int i = threadIdx.x; i < nb; i += kB) acc += part[i];
	const double s = block_sum(acc, sh);
	if (threadIdx.x == 0) out[0] = s / (double)n;
}

// ---- tree build -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void f2d_minmax_kernel(const double2 *__restrict__ x, long long n, double *__restrict__ part)
{
	__shared__ double sh[4][kB];
	double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const double2 p = x[i];
		mnx = fmin(mnx, p.x);
		mny = fmin(mny, p.y);
		mxx = fmax(mxx, p.x);
		mxy = fmax(mxy, p.y);
	}
	sh[0][threadIdx.x] = mnx;
	sh[1][threadIdx.x] = mny;
	sh[2][threadIdx.x] = mxx;
	sh[3][threadIdx.x] = mxy;
	__syncthreads();
	for (int s = kB / 2; s > 0; s >>= 1)
	{
		if ((int)threadIdx.x < s)
		{
			sh[0][threadIdx.x] = fmin(sh[0][threadIdx.x], sh[0][threadIdx.x + s]);
			sh[1][threadIdx.x] = fmin(sh[1][threadIdx.x], sh[1][threadIdx.x + s]);
			sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + s]);
			sh[3][threadIdx.x] = fmax(sh[3][threadIdx.x], sh[3][threadIdx.x + s]);
		}
		__syncthreads();
	}
	if (threadIdx.x < 4) part[4 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

#pragma clang fp contract(off)
// scal = {min x, min y, 1 / delta}: delta = max(max - min) / side, clamped below at sqrt(EPS2) (fmm_cart.cuh:476-481)
__global__ __launch_bounds__(64) void f2d_scalars_kernel(const double *__restrict__ part, int nb, int side, double eps2, double *__restrict__ scal)
{
	if (threadIdx.x != 0) return;
	double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
	for (int b = 0; b < nb; ++b)
	{
		mnx = fmin(mnx, part[4 * b + 0]);
		mny = fmin(mny, part[4 * b + 1]);
		mxx = fmax(mxx, part[4 * b + 2]);
		mxy = fmax(mxy, part[4 * b + 3]);
	}
	double delta = fmax(mxx - mnx, mxy - mny) / (double)side;
	const double eps = std::sqrt(eps2);
	if (delta < eps) delta = eps;
	scal[0] = mnx;
	scal[1] = mny;
	scal[2] = 1.0 / delta;
}

// integer cell keys, row-major ix * side + iy (appel.cuh:44-55; to_ivec truncates, clip to [0, side-1])
__global__ __launch_bounds__(kB) void f2d_keys_kernel(const double2 *__restrict__ x, long long n, const double *__restrict__ scal, int side,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ idx)
{
	const double mnx = scal[0], mny = scal[1], rd = scal[2];
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const double2 p = x[i];
		int ix = (int)((p.x - mnx) * rd), iy = (int)((p.y - mny) * rd);
		ix = std::min(std::max(ix, 0), side - 1);
		iy = std::min(std::max(iy, 0), side - 1);
		keys[i] = (uint32_t)(ix * side + iy);
		idx[i] = (uint32_t)i;
	}
}
#pragma clang fp contract(on)

__global__ __launch_bounds__(kB) void f2d_gather_kernel(const double2 *__restrict__ x, const double2 *__restrict__ v, const uint32_t *__restrict__ idx,
                                                        double2 *__restrict__ out, long long n)
{
	for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB)
	{
		const uint32_t j = idx[i];
		out[i] = x[j];
		out[n + i] = v[j];
	}
}

// index[c] = first particle of leaf c in the sorted order (c = 0..m; index[m] = n): appel.cuh:141-216
__global__ __launch_bounds__(kB) void f2d_index_kernel(const uint32_t *__restrict__ keys, long long n, int m, int *__restrict__ index)
{
	const int c = blockIdx.x * kB + threadIdx.x;
	if (c > m) return;
	long long lo = 0, hi = n;
	while (lo < hi)
	{
		const long long mid = (lo + hi) >> 1;
		if (keys[mid] < (uint32_t)c) lo = mid + 1;
		else hi = mid;
	}
	index[c] = (int)lo;
}

struct Quad
{
	double2 *center, *mpole, *local;   // [ntot], [ntot][P+1], [ntot][P]
	int *mult, *index;                 // [ntot], leaf level [m+1]
};

// P2M about the centroid, orders 0 and 2..P (appel.cuh:222-258, fmm_cart.cuh:68-96)
template <int P>
__global__ __launch_bounds__(kB) void f2d_leaf_kernel(Quad q, const double2 *__restrict__ x, int m, long long beg)
{
	const int c = blockIdx.x * kB + threadIdx.x;
	if (c >= m) return;
	const int b = q.index[c], e = q.index[c + 1], mlt = e - b;
	double2 t = make_double2(0.0, 0.0);
	double2 mp[P + 1];
#pragma unroll
	for (int k = 0; k <= P; ++k) mp[k] = make_double2(0.0, 0.0);
	if (mlt > 0)
	{
		for (int j = b; j < e; ++j) t = cadd(t, x[j]);
		t.x /= (double)mlt;
		t.y /= (double)mlt;
		for (int j = b; j < e; ++j)
		{
			const double2 w = make_double2(x[j].x - t.x, x[j].y - t.y);
			double2 pw = w;
#pragma unroll
			for (int k = 2; k <= P; ++k)
			{
				pw = cmul(pw, w);
				mp[k] = cadd(mp[k], pw);
			}
		}
		mp[0] = make_double2((double)mlt, 0.0);
	}
	q.center[beg + c] = t;
	q.mult[beg + c] = mlt;
#pragma unroll
	for (int k = 0; k <= P; ++k) q.mpole[(beg + c) * (P + 1) + k] = mp[k];
}

// M2M: the four children of a level-l cell, about their charge-weighted centroid (fmm_cart.cuh:116-188)
template <int P>
__global__ __launch_bounds__(kB) void f2d_m2m_kernel(Quad q, int l)
{
	const int side = 1 << l, sidep = side << 1;
	const int ij0 = blockIdx.x * kB + threadIdx.x;
	if (ij0 >= side * side) return;
	const int i = ij0 / side, j = ij0 - i * side;
	const long long ij = quad_beg(l) + ij0;
	const long long ijp = quad_beg(l + 1) + 2LL * (i * sidep + j);
	const long long ch[4] = {ijp, ijp + 1, ijp + sidep, ijp + sidep + 1};
	int mlt = 0;
#pragma unroll
	for (int s = 0; s < 4; ++s) mlt += q.mult[ch[s]];
	double2 coord = make_double2(0.0, 0.0);
	double2 mp[P + 1];
#pragma unroll
	for (int k = 0; k <= P; ++k) mp[k] = make_double2(0.0, 0.0);
	if (mlt > 0)
	{
#pragma unroll
		for (int s = 0; s < 4; ++s) coord = cadd(coord, cscale(q.center[ch[s]], (double)q.mult[ch[s]]));
		coord.x /= (double)mlt;
		coord.y /= (double)mlt;
#pragma unroll
		for (int s = 0; s < 4; ++s)
		{
			if (q.mult[ch[s]] == 0) continue;
			const double2 cc = q.center[ch[s]];
			const double2 d = make_double2(cc.x - coord.x, cc.y - coord.y);   // child centre seen from the parent's
			double2 dp[P + 1];
			dp[0] = make_double2(1.0, 0.0);
#pragma unroll
			for (int k = 1; k <= P; ++k) dp[k] = cmul(dp[k - 1], d);
			double2 a[P + 1];
#pragma unroll
			for (int k = 0; k <= P; ++k) a[k] = q.mpole[ch[s] * (P + 1) + k];
#pragma unroll
			for (int k = 2; k <= P; ++k)
			{
				double2 acc = cscale(dp[k], a[0].x);
#pragma unroll
				for (int r = 2; r <= k; ++r) acc = cadd(acc, cscale(cmul(a[r], dp[k - r]), binom(k, r)));
				mp[k] = cadd(mp[k], acc);
			}
		}
		mp[0] = make_double2((double)mlt, 0.0);
	}
	q.center[ij] = coord;
	q.mult[ij] = mlt;
#pragma unroll
	for (int k = 0; k <= P; ++k) q.mpole[ij * (P + 1) + k] = mp[k];
}

// M2L for every cell of levels 2..L in one launch: one thread per target, the stencil of its parent's (4r+2)^2 block minus its own
// (2r+1)^2 neighbourhood (fmm_cart.cuh:214-262); empty sources and empty targets are skipped.  Writes (not accumulates) the locals.
template <int P>
__global__ __launch_bounds__(kB) void f2d_m2l_kernel(Quad q, int L, int radius, double eps2)
{
	const long long cell = quad_beg(2) + (long long)blockIdx.x * kB + threadIdx.x;
	if (cell >= quad_beg(L + 1)) return;
	int l = 2;
	while (cell >= quad_beg(l + 1)) ++l;
	const long long beg = quad_beg(l);
	const int side = 1 << l;
	const int ij = (int)(cell - beg), i = ij / side, j = ij - i * side;
	double2 b[P];
#pragma unroll
	for (int k = 0; k < P; ++k) b[k] = make_double2(0.0, 0.0);
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
				double2 a[P + 1];
#pragma unroll
				for (int kk = 0; kk <= P; ++kk) a[kk] = q.mpole[src * (P + 1) + kk];
				double2 wm = make_double2(1.0, 0.0);
#pragma unroll
				for (int mm = 1; mm <= 2 * P; ++mm)   // total order k + l + 1
				{
					wm = cmul(wm, w);
#pragma unroll
					for (int ll = 0; ll < P; ++ll)
					{
						const int kk = mm - 1 - ll;
						if (kk < 0 || kk > P || kk == 1) continue;
						const double co = ((ll & 1) ? -1.0 : 1.0) * binom(mm - 1, ll);
						b[ll] = cadd(b[ll], cscale(cmul(a[kk], wm), co));
					}
				}
			}
	}
#pragma unroll
	for (int k = 0; k < P; ++k) q.local[cell * P + k] = b[k];
}

// L2L into the non-empty cells of level l from their parents (fmm_cart.cuh:288-334)
template <int P>
__global__ __launch_bounds__(kB) void f2d_l2l_kernel(Quad q, int l)
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
	double2 bp[P], dp[P];
#pragma unroll
	for (int k = 0; k < P; ++k) bp[k] = q.local[par * P + k];
	dp[0] = make_double2(1.0, 0.0);
#pragma unroll
	for (int k = 1; k < P; ++k) dp[k] = cmul(dp[k - 1], d);
#pragma unroll
	for (int mm = 0; mm < P; ++mm)
	{
		double2 acc = q.local[cell * P + mm];
#pragma unroll
		for (int ll = mm; ll < P; ++ll) acc = cadd(acc, cscale(cmul(bp[ll], dp[ll - mm]), binom(ll, mm)));
		q.local[cell * P + mm] = acc;
	}
}

// Near field fused with L2P and the rescale (appel.cuh:260-303, fmm_cart.cuh:353-376, :537-539): one wave per target leaf, one
// target per lane; each of the 2r+1 neighbour rows is one contiguous run of particles, staged through LDS 64 sources at a time.
// Without COLL the pair sum is skipped and a is multiplied by param[1] (fmm_cart.cuh:527-528).
template <int P, bool COLL>
__global__ __launch_bounds__(kNear) void f2d_near_kernel(Quad q, const double2 *__restrict__ x, double2 *__restrict__ a, int L, int radius,
                                                         double eps2, const double *__restrict__ param)
{
	__shared__ double sx[kNear], sy[kNear];
	const int side = 1 << L;
	const int m = side * side;
	const double s0 = param[0], s1 = param[1];
	const int lane = threadIdx.x;
	// grid-stride over the leaves: 4^L blocks exceed a dispatch's grid for L >= 13
	for (int cell = blockIdx.x; cell < m; cell += gridDim.x)
	{
	const int b = q.index[cell], e = q.index[cell + 1];
	if (b == e) continue;   // uniform across the block
	const long long qc = quad_beg(L) + cell;
	const int i = cell / side, j = cell - i * side;
	const int kmin = std::max(i - radius, 0), kmax = std::min(i + radius, side - 1);
	const int lmin = std::max(j - radius, 0), lmax = std::min(j + radius, side - 1);
	const double2 c = q.center[qc];
	double2 bl[P];
#pragma unroll
	for (int k = 0; k < P; ++k) bl[k] = q.local[qc * P + k];
	for (int t0 = b; t0 < e; t0 += kNear)
	{
		const int t = t0 + lane;
		const bool act = t < e;
		const double2 zi = act ? x[t] : make_double2(0.0, 0.0);
		double ax = 0, ay = 0;
		if (COLL)
		{
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
					for (int u = 0; u < cnt; ++u)
					{
						const double dx = zi.x - sx[u], dy = zi.y - sy[u];
						const double inv = 1.0 / (dx * dx + dy * dy + eps2);
						ax += dx * inv;
						ay += dy * inv;
					}
				}
			}
		}
		else if (act)
		{
			const double2 a0 = a[t];
			ax = a0.x * s1;
			ay = a0.y * s1;
		}
		// L2P: f(u) = sum_l b_l u^l by Horner, field = conj(f)
		const double2 u = make_double2(zi.x - c.x, zi.y - c.y);
		double2 f = bl[P - 1];
#pragma unroll
		for (int k = P - 2; k >= 0; --k) f = cadd(cmul(f, u), bl[k]);
		ax += f.x;
		ay -= f.y;
		if (act) a[t] = make_double2(ax * s0, ay * s0);
	}
	__syncthreads();   // the next leaf overwrites the LDS rows
	}
}

#include "f2d_energy_kernels.hpp"
#include "f2d_probe_kernels.hpp"

} // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int f2d_done(nbco_ctx *c)
{
	NBCO_HIP(hipGetLastError());
	if (c->o.sync) NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

static int f2d_direct(nbco_ctx *c, const double *p, double *a, long long n, const double *param, bool kahan)
{
	if (!c) return NBCO_ERR_ARG;
	if (!p || !a || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_direct: bad arguments");
	const long long nb = (n + kB - 1) / kB;
	if (nb > (1LL << 31) - 1) return c->fail(NBCO_ERR_ARG, "nbco_2d_direct: n too large");
	const double eps2 = (double)c->o.eps2;
	if (kahan)
		hipLaunchKernelGGL(f2d_direct_kernel<true>, dim3((unsigned)nb), dim3(kB), 0, c->stream, (const double2 *)p, (double2 *)a, n, eps2, param);
	else
		hipLaunchKernelGGL(f2d_direct_kernel<false>, dim3((unsigned)nb), dim3(kB), 0, c->stream, (const double2 *)p, (double2 *)a, n, eps2, param);
	return f2d_done(c);
}

// L = max(2, round(log2(dens_inhom n / (p sqrt p)) / 2)) (fmm_cart.cuh:415-417), or opts.tree_L; 2 <= L <= 15
static int f2d_levels(const nbco_opts &o, long long n)
{
	if (o.tree_L > 0) return o.tree_L;
	const double s = o.fmm_order * std::sqrt((double)o.fmm_order);
	int L = (int)std::round(std::log2((double)o.dens_inhom * (double)n / s) / 2);
	return std::min(std::max(L, 2), kMaxL2);
}

// ---- the five kernels that are compiled per order: each launch function is the one place where its kernel's order is chosen ----
static void f2d_launch_leaf(nbco_ctx *c, int P, const Quad &q, const double2 *x, int m, long long beg)
{
	with_order(P, [&](auto p) { hipLaunchKernelGGL((f2d_leaf_kernel<decltype(p)::value>), dim3((m + kB - 1) / kB), dim3(kB), 0, c->stream, q, x, m, beg); });
}
static void f2d_launch_m2m(nbco_ctx *c, int P, const Quad &q, int l)
{
	with_order(P, [&](auto p) { hipLaunchKernelGGL((f2d_m2m_kernel<decltype(p)::value>), dim3(((1 << (2 * l)) + kB - 1) / kB), dim3(kB), 0, c->stream, q, l); });
}
static void f2d_launch_m2l(nbco_ctx *c, int P, const Quad &q, int L, int radius, double eps2)
{
	const long long nm2l = quad_beg(L + 1) - quad_beg(2);
	with_order(P, [&](auto p) {
		hipLaunchKernelGGL((f2d_m2l_kernel<decltype(p)::value>), dim3((unsigned)((nm2l + kB - 1) / kB)), dim3(kB), 0, c->stream, q, L, radius, eps2);
	});
}
static void f2d_launch_l2l(nbco_ctx *c, int P, const Quad &q, int l)
{
	with_order(P, [&](auto p) { hipLaunchKernelGGL((f2d_l2l_kernel<decltype(p)::value>), dim3(((1 << (2 * l)) + kB - 1) / kB), dim3(kB), 0, c->stream, q, l); });
}
static void f2d_launch_near(nbco_ctx *c, int P, bool coll, const Quad &q, const double2 *x, double2 *a, int L, int radius, double eps2, const double *param)
{
	const int near_grid = std::min(1 << (2 * L), 1 << 22);
	with_order(P, [&](auto p) {
		if (coll) hipLaunchKernelGGL((f2d_near_kernel<decltype(p)::value, true>), dim3(near_grid), dim3(kNear), 0, c->stream, q, x, a, L, radius, eps2, param);
		else hipLaunchKernelGGL((f2d_near_kernel<decltype(p)::value, false>), dim3(near_grid), dim3(kNear), 0, c->stream, q, x, a, L, radius, eps2, param);
	});
}

// what nbco_2d_fmm asks of n and the options; the integrators ask it before their first launch, so that a refused step moves nothing
static int f2d_fmm_check(nbco_ctx *c, long long n)
{
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_ARG, "nbco_2d_fmm: n must be below 2^31");
	if (c->o.tree_radius < 1) return c->fail(NBCO_ERR_ARG, "nbco_2d_fmm: tree_radius must be >= 1");
	if (c->o.tree_L == 1 || c->o.tree_L > kMaxL2 || c->o.tree_L < 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_fmm: tree_L must be 0 or 2..15");
	return NBCO_OK;
}

// ---- the tree stage that the evaluator, the FMM energy and the FMM probes share ------------------------------------------------------
// what a tree call (`who`, for the refusals) takes from the options and n: side = 2^L, m = 4^L leaves, ntot nodes on levels 0..L
struct F2dPlan
{
	int P, L, radius, side, m;
	double eps2;
	long long ntot;
};
static int f2d_plan(nbco_ctx *c, const char *who, long long n, F2dPlan &pl)
{
	NBCO_TRY(f2d_fmm_check(c, n));
	if (c->o.fmm_order < 1 || c->o.fmm_order > kMaxOrder)
		return c->fail(NBCO_ERR_ARG, std::string(who) + ": fmm_order must be 1..10 (orders above 10 are not provided)");
	pl.P = c->o.fmm_order;
	pl.L = f2d_levels(c->o, n);
	if (pl.L < 2 || pl.L > kMaxL2) return c->fail(NBCO_ERR_ARG, std::string(who) + ": tree_L must be 0 or 2..15");
	pl.radius = (int)c->o.tree_radius;
	pl.eps2 = (double)c->o.eps2;
	pl.side = 1 << pl.L;
	pl.m = pl.side * pl.side;
	pl.ntot = quad_beg(pl.L + 1);
	return NBCO_OK;
}

// the tree, the constants of the potential's far field (with_c0), the sources in cell order, the sort permutation, the scalars of the keys
struct F2dTree
{
	Quad q;
	double *c0;
	const double2 *x;
	const uint32_t *idx;
	const double *scal;
};

// Keys, stable sort and gather of the n sources at x0, leaf index, centroids and multipoles up to level 2.  Scratch: f2d_keys = keys
// in / out, indices in / out; f2d_tree = centres | multipoles | locals (with_local) | c0 (with_c0) | multiplicities | leaf index;
// f2d_part = reduction partials + scalars + part_more doubles of the caller's behind them; f2d_tmp = the sort's scratch, then the
// gather's destination.  state: the caller's [x | v] with x0 = x, reordered in place; nullptr: x0 is only read, and the
// sorted positions stay in f2d_tmp.
static int f2d_tree_build(nbco_ctx *c, const F2dPlan &pl, const double2 *x0, long long n, bool with_local, bool with_c0, double *state, size_t part_more,
                          F2dTree &t)
{
	const int P = pl.P, m = pl.m;
	const long long ntot = pl.ntot;
	hipStream_t st = c->stream;
	NBCO_TRY(c->reserve(c->f2d_keys, sizeof(uint32_t) * 4 * (size_t)n));
	uint32_t *keys_in = c->f2d_keys.as<uint32_t>(), *keys = keys_in + n, *idx_in = keys + n, *idx = idx_in + n;
	const size_t tree_bytes = sizeof(double2) * (size_t)ntot * (1 + (P + 1) + (with_local ? P : 0)) + sizeof(double) * (with_c0 ? (size_t)ntot : 0) +
	                          sizeof(int) * ((size_t)ntot + (size_t)m + 1);
	NBCO_TRY(c->reserve(c->f2d_tree, tree_bytes));
	NBCO_TRY(c->reserve(c->f2d_part, sizeof(double) * (4 * kRedBlocks + 8 + part_more)));
	Quad &q = t.q;
	q.center = c->f2d_tree.as<double2>();
	q.mpole = q.center + ntot;
	double2 *after = q.mpole + ntot * (P + 1);
	q.local = with_local ? after : nullptr;
	if (with_local) after += ntot * P;
	t.c0 = with_c0 ? reinterpret_cast<double *>(after) : nullptr;
	q.mult = reinterpret_cast<int *>(reinterpret_cast<double *>(after) + (with_c0 ? ntot : 0));
	q.index = q.mult + ntot;
	double *part = c->f2d_part.as<double>(), *scal = part + 4 * kRedBlocks;

	const int nbr = std::min(kRedBlocks, grid_blocks(n, kB, kGridCap));
	hipLaunchKernelGGL(f2d_minmax_kernel, dim3(nbr), dim3(kB), 0, st, x0, n, part);
	hipLaunchKernelGGL(f2d_scalars_kernel, dim3(1), dim3(64), 0, st, (const double *)part, nbr, pl.side, pl.eps2, scal);
	hipLaunchKernelGGL(f2d_keys_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, st, x0, n, (const double *)scal, pl.side, keys_in, idx_in);
	NBCO_TRY(sort_pairs(c, c->f2d_tmp, keys_in, keys, idx_in, idx, n, 0u, (unsigned)(2 * pl.L), sizeof(double2) * (state ? 2 : 1) * (size_t)n));
	double2 *tmp = c->f2d_tmp.as<double2>();
	if (state)
	{
		hipLaunchKernelGGL(f2d_gather_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, st, x0, x0 + n, (const uint32_t *)idx, tmp, n);
		NBCO_HIP(hipMemcpyAsync(state, tmp, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToDevice, st));
	}
	else hipLaunchKernelGGL(f2d_gather_pos_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, st, x0, (const uint32_t *)idx, tmp, n);
	hipLaunchKernelGGL(f2d_index_kernel, dim3((m + kB) / kB), dim3(kB), 0, st, (const uint32_t *)keys, n, m, q.index);
	t.x = state ? x0 : tmp;
	t.idx = idx;
	t.scal = scal;
	f2d_launch_leaf(c, P, q, t.x, m, quad_beg(pl.L));
	for (int l = pl.L - 1; l >= 2; --l) f2d_launch_m2m(c, P, q, l);
	return NBCO_OK;
}

static int f2d_fmm(nbco_ctx *c, double *p, double *a, long long n, const double *param)
{
	if (!c) return NBCO_ERR_ARG;
	if (!p || !a || !param || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_fmm: bad arguments");
	F2dPlan pl;
	NBCO_TRY(f2d_plan(c, "nbco_2d_fmm", n, pl));
	F2dTree t;
	NBCO_TRY(f2d_tree_build(c, pl, (const double2 *)p, n, /*with_local*/ true, /*with_c0*/ false, /*state*/ p, /*part_more*/ 0, t));
	f2d_launch_m2l(c, pl.P, t.q, pl.L, pl.radius, pl.eps2);
	for (int l = 3; l <= pl.L; ++l) f2d_launch_l2l(c, pl.P, t.q, l);
	f2d_launch_near(c, pl.P, c->o.coll != 0, t.q, t.x, (double2 *)a, pl.L, pl.radius, pl.eps2, param);
	return f2d_done(c);
}

// ---- energy diagnostics ------------------------------------------------------------------------------------------------------
static void f2d_launch_m2l0(nbco_ctx *c, int P, const Quad &q, double *c0, int L, int radius, double eps2)
{
	const long long nm2l = quad_beg(L + 1) - quad_beg(2);
	with_order(P, [&](auto p) {
		hipLaunchKernelGGL((f2d_m2l0_kernel<decltype(p)::value>), dim3((unsigned)((nm2l + kB - 1) / kB)), dim3(kB), 0, c->stream, q, c0, L, radius, eps2);
	});
}
static void f2d_launch_l2l0(nbco_ctx *c, int P, const Quad &q, double *c0, int l)
{
	with_order(P, [&](auto p) { hipLaunchKernelGGL((f2d_l2l0_kernel<decltype(p)::value>), dim3(((1 << (2 * l)) + kB - 1) / kB), dim3(kB), 0, c->stream, q, c0, l); });
}
static void f2d_launch_near_pot(nbco_ctx *c, int P, int grid, const Quad &q, const double *c0, const double2 *x, const uint32_t *idx, int L, int radius,
                                double eps2, const double *param, double *psi, double *part)
{
	with_order(P, [&](auto p) {
		hipLaunchKernelGGL((f2d_near_pot_kernel<decltype(p)::value>), dim3(grid), dim3(kNear), 0, c->stream, q, c0, x, idx, L, radius, eps2, param, psi, part);
	});
}

// f2d_part for an energy call: | minmax partials 4 kRedBlocks | scalars 8 (out3 at + 4) | kinetic / elastic slots 2 kRedBlocks | npot potential slots |
// f2d_energy_more: what lies behind the scalars; f2d_energy_slots: the slots of a part that is reserved
static size_t f2d_energy_more(long long npot) { return 2 * (size_t)kRedBlocks + (size_t)npot; }
static void f2d_energy_slots(nbco_ctx *c, double **scal, double **ke, double **pot)
{
	*scal = c->f2d_part.as<double>() + 4 * kRedBlocks;
	*ke = *scal + 8;
	*pot = *ke + 2 * kRedBlocks;
}

// kinetic and elastic slots, then the final block and the copy to the host
static int f2d_energy_finish(nbco_ctx *c, const double *buf, long long n, const double *param, double *scal, double *ke, const double *pot, long long npot,
                             double *out3_host)
{
	const int nke = std::min(kRedBlocks, grid_blocks(n, kB, kGridCap));
	hipLaunchKernelGGL(f2d_kin_ela_kernel, dim3(nke), dim3(kB), 0, c->stream, (const double2 *)buf, (const double2 *)buf + n, n, param + 2, ke);
	hipLaunchKernelGGL(f2d_energy_final_kernel, dim3(1), dim3(kB), 0, c->stream, (const double *)ke, nke, pot, npot, param, scal + 4);
	NBCO_HIP(hipGetLastError());
	double h[3];
	NBCO_HIP(hipMemcpyAsync(h, scal + 4, sizeof h, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	out3_host[0] = h[0];
	out3_host[1] = h[1];
	out3_host[2] = h[2];
	return NBCO_OK;
}

static int f2d_energy(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev)
{
	if (!c) return NBCO_ERR_ARG;
	if (!buf || !param || !out3_host || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_energy: bad arguments");
	const long long nb = (n + kB - 1) / kB;
	if (nb > (1LL << 31) - 1) return c->fail(NBCO_ERR_ARG, "nbco_2d_energy: n too large");
	NBCO_TRY(c->reserve(c->f2d_part, sizeof(double) * (4 * kRedBlocks + 8 + f2d_energy_more(nb))));
	double *scal, *ke, *pot;
	f2d_energy_slots(c, &scal, &ke, &pot);
	hipLaunchKernelGGL(f2d_pair_pot_kernel, dim3((unsigned)nb), dim3(kB), 0, c->stream, (const double2 *)buf, n, (double)c->o.eps2, param, phi_dev, pot);
	return f2d_energy_finish(c, buf, n, param, scal, ke, pot, nb, out3_host);
}

// the evaluator's tree over a scratch copy of the positions, then the field's M2L / L2L with the constant's next to them, and the
// near-field potential.  buf is only read.
static int f2d_energy_fmm(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev)
{
	if (!c) return NBCO_ERR_ARG;
	if (!buf || !param || !out3_host || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_energy_fmm: bad arguments");
	F2dPlan pl;
	NBCO_TRY(f2d_plan(c, "nbco_2d_energy_fmm", n, pl));
	const int P = pl.P, L = pl.L, near_grid = std::min(1 << (2 * L), 1 << 22);
	F2dTree t;
	NBCO_TRY(f2d_tree_build(c, pl, (const double2 *)buf, n, /*with_local*/ true, /*with_c0*/ true, /*state*/ nullptr, f2d_energy_more(near_grid), t));
	double *scal, *ke, *pot;
	f2d_energy_slots(c, &scal, &ke, &pot);
	f2d_launch_m2l(c, P, t.q, L, pl.radius, pl.eps2);
	f2d_launch_m2l0(c, P, t.q, t.c0, L, pl.radius, pl.eps2);
	for (int l = 3; l <= L; ++l)
	{
		f2d_launch_l2l(c, P, t.q, l);
		f2d_launch_l2l0(c, P, t.q, t.c0, l);
	}
	f2d_launch_near_pot(c, P, near_grid, t.q, t.c0, t.x, t.idx, L, pl.radius, pl.eps2, param, phi_dev, pot);
	return f2d_energy_finish(c, buf, n, param, scal, ke, pot, near_grid, out3_host);
}

// ---- probes ------------------------------------------------------------------------------------------------------------------
static int f2d_probe_args(nbco_ctx *c, const char *who, const double *p, long long n, const double *t, long long m, const double *param,
                          const double *a, const double *psi)
{
	if (!p || !t || !param || n <= 0 || m <= 0 || (!a && !psi)) return c->fail(NBCO_ERR_ARG, std::string(who) + ": bad arguments");
	if (n >= (1LL << 31) || m >= (1LL << 31)) return c->fail(NBCO_ERR_ARG, std::string(who) + ": n and m must be below 2^31");
	return NBCO_OK;
}

static int f2d_probe(nbco_ctx *c, const double *p, long long n, const double *t, long long m, const double *param, double *a, double *psi)
{
	if (!c) return NBCO_ERR_ARG;
	NBCO_TRY(f2d_probe_args(c, "nbco_2d_probe", p, n, t, m, param, a, psi));
	const unsigned nb = (unsigned)((m + kB - 1) / kB);
	with_outputs(a, psi, [&](auto wa, auto wp) {
		hipLaunchKernelGGL((f2d_probe_direct_kernel<decltype(wa)::value, decltype(wp)::value>), dim3(nb), dim3(kB), 0, c->stream, (const double2 *)p, n,
		                   (const double2 *)t, m, (double)c->o.eps2, param, (double2 *)a, psi);
	});
	return f2d_done(c);
}

static void f2d_launch_probe(nbco_ctx *c, int P, const Quad &q, const int *pindex, const uint32_t *pidx, const double2 *x, const double2 *t, int L,
                             int radius, double eps2, const double *param, double *a, double *psi)
{
	const int grid = std::min(1 << (2 * L), 1 << 22);
	with_order(P, [&](auto p) {
		with_outputs(a, psi, [&](auto wa, auto wp) {
			hipLaunchKernelGGL((f2d_probe_kernel<decltype(p)::value, decltype(wa)::value, decltype(wp)::value>), dim3(grid), dim3(kNear), 0, c->stream,
			                   (const double2 *)q.center, (const double2 *)q.mpole, (const int *)q.mult, (const int *)q.index, pindex, pidx, x, t, L,
			                   radius, eps2, param, (double2 *)a, psi);
		});
	});
}

// the tree over a scratch copy of p, without locals; then the probes keyed with the sources' scalars, sorted, indexed by leaf (f2d_pkeys:
// keys in / out, indices in / out, leaf index), and summed leaf by leaf.  p and t are only read.
static int f2d_probe_fmm(nbco_ctx *c, const double *p, long long n, const double *t, long long mp, const double *param, double *a, double *psi)
{
	if (!c) return NBCO_ERR_ARG;
	NBCO_TRY(f2d_probe_args(c, "nbco_2d_probe_fmm", p, n, t, mp, param, a, psi));
	F2dPlan pl;
	NBCO_TRY(f2d_plan(c, "nbco_2d_probe_fmm", n, pl));
	const int m = pl.m;
	hipStream_t st = c->stream;
	NBCO_TRY(c->reserve(c->f2d_pkeys, sizeof(uint32_t) * 4 * (size_t)mp + sizeof(int) * ((size_t)m + 1)));
	uint32_t *pkeys_in = c->f2d_pkeys.as<uint32_t>(), *pkeys = pkeys_in + mp, *pidx_in = pkeys + mp, *pidx = pidx_in + mp;
	int *pindex = reinterpret_cast<int *>(pidx + mp);
	F2dTree tr;
	NBCO_TRY(f2d_tree_build(c, pl, (const double2 *)p, n, /*with_local*/ false, /*with_c0*/ false, /*state*/ nullptr, /*part_more*/ 0, tr));

	// the clamp of f2d_keys_kernel projects a probe outside the sources' square onto it
	const double2 *t0 = (const double2 *)t;
	hipLaunchKernelGGL(f2d_keys_kernel, dim3(grid_blocks(mp, kB, kGridCap)), dim3(kB), 0, st, t0, mp, tr.scal, pl.side, pkeys_in, pidx_in);
	NBCO_TRY(sort_pairs(c, c->f2d_ptmp, pkeys_in, pkeys, pidx_in, pidx, mp, 0u, (unsigned)(2 * pl.L)));
	hipLaunchKernelGGL(f2d_index_kernel, dim3((m + kB) / kB), dim3(kB), 0, st, (const uint32_t *)pkeys, mp, m, pindex);
	f2d_launch_probe(c, pl.P, tr.q, pindex, pidx, tr.x, t0, pl.L, pl.radius, pl.eps2, param, a, psi);
	return f2d_done(c);
}

static int f2d_step(nbco_ctx *c, double *b, const double *a, long double ds, long long n)
{
	hipLaunchKernelGGL(f2d_axpy_kernel, dim3(grid_blocks(2 * n, kB, kGridCap)), dim3(kB), 0, c->stream, b, a, (double)ds, 2 * n);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

static int f2d_drift_b(nbco_ctx *c, double *x, double *v, double omega, long double ds, long long n)
{
	Helix2 h;
	if (nbco_2d_helix_matrices(omega, (double)ds, h.R, h.A) != NBCO_OK) return c->fail(NBCO_ERR_ARG, "nbco_2d_drift_b: omega and s must be finite");
	if (n <= 0) return NBCO_OK;
	hipLaunchKernelGGL(f2d_drift_b_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, c->stream, (double2 *)x, (double2 *)v, h, n);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// O(s) of the bath on n velocities; false from the coefficients: gamma, kT or s is not finite or negative
static int f2d_bath(nbco_ctx *c, double *v, const nbco_bath *bath, double s, int half, unsigned long long tick, long long n)
{
	Bath2 b;
	if (bath_coeffs_dim(bath, s, b.c1, b.c2, 2) != NBCO_OK) return c->fail(NBCO_ERR_ARG, "nbco_2d_bath_apply: gamma, kT and s must be finite and not negative");
	b.key[0] = (uint32_t)bath->seed; b.key[1] = (uint32_t)(bath->seed >> 32);
	b.tick[0] = (uint32_t)tick; b.tick[1] = (uint32_t)(tick >> 32);
	b.half = half;
	if (n <= 0) return NBCO_OK;
	hipLaunchKernelGGL(f2d_bath_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, c->stream, (double2 *)v, b, n);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

static int f2d_eval(nbco_ctx *c, int kind, double *buf, long long n, const double *param, int elastic)
{
	double *a = buf + 4 * n;
	{
		SyncOff quiet(c);
		switch (kind)
		{
		case NBCO_2D_EVAL_DIRECT: NBCO_TRY(f2d_direct(c, buf, a, n, param, false)); break;
		case NBCO_2D_EVAL_DIRECT_KAHAN: NBCO_TRY(f2d_direct(c, buf, a, n, param, true)); break;
		case NBCO_2D_EVAL_FMM: NBCO_TRY(f2d_fmm(c, buf, a, n, param)); break;
		default: return c->fail(NBCO_ERR_ARG, "nbco_2d: unknown evaluator kind");
		}
	}
	if (elastic)   // main.cu:85-89: a -= k o x, k = param + 2
	{
		hipLaunchKernelGGL(f2d_elastic_kernel, dim3(grid_blocks(n, kB, kGridCap)), dim3(kB), 0, c->stream, (const double2 *)buf, (double2 *)a, n, param + 2);
		NBCO_HIP(hipGetLastError());
	}
	return NBCO_OK;
}

// host-side state initialisation (main.cu:96-170): centre, then scale each component to the wanted RMS
static void f2d_center_rms(double *d, long long nb, double ax, double ay)
{
	double sx = 0, sy = 0;
	for (long long i = 0; i < nb; ++i) { sx += d[2 * i]; sy += d[2 * i + 1]; }
	sx /= (double)nb;
	sy /= (double)nb;
	for (long long i = 0; i < nb; ++i) { d[2 * i] -= sx; d[2 * i + 1] -= sy; }
	double qx = 0, qy = 0;
	for (long long i = 0; i < nb; ++i) { qx += d[2 * i] * d[2 * i]; qy += d[2 * i + 1] * d[2 * i + 1]; }
	qx /= (double)nb;
	qy /= (double)nb;
	qx = std::sqrt(qx);
	qy = std::sqrt(qy);
	const double fx = ax / qx, fy = ay / qy;
	for (long long i = 0; i < nb; ++i) { d[2 * i] *= fx; d[2 * i + 1] *= fy; }
}

extern "C" {

int nbco_2d_direct(nbco_ctx *c, const double *p, double *a, long long n, const double *param) { return f2d_direct(c, p, a, n, param, false); }
int nbco_2d_direct3(nbco_ctx *c, const double *p, double *a, long long n, const double *param) { return f2d_direct(c, p, a, n, param, true); }
int nbco_2d_fmm(nbco_ctx *c, double *p, double *a, long long n, const double *param) { return f2d_fmm(c, p, a, n, param); }

int nbco_2d_energy(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev)
{
	return f2d_energy(c, buf, n, param, out3_host, phi_dev);
}
int nbco_2d_energy_fmm(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev)
{
	return f2d_energy_fmm(c, buf, n, param, out3_host, phi_dev);
}

int nbco_2d_probe(nbco_ctx *c, const double *p, long long n, const double *t, long long m, const double *param, double *a_dev, double *psi_dev)
{
	return f2d_probe(c, p, n, t, m, param, a_dev, psi_dev);
}
int nbco_2d_probe_fmm(nbco_ctx *c, const double *p, long long n, const double *t, long long m, const double *param, double *a_dev, double *psi_dev)
{
	return f2d_probe_fmm(c, p, n, t, m, param, a_dev, psi_dev);
}

int nbco_2d_force(nbco_ctx *c, int kind, double *buf, long long n, const double *param, int elastic)
{
	if (!c) return NBCO_ERR_ARG;
	if (!buf || !param || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_force: bad arguments");
	NBCO_TRY(f2d_eval(c, kind, buf, n, param, elastic));
	return f2d_done(c);
}

// omega = 0: the straight drift of the reference; otherwise the helix drift replaces it (nbco_2d_integrate_b).  bath: null, or the
// Langevin bath whose two half steps wrap the scheme (nbco_2d_integrate_t); with every gamma 0 it is no bath.
static int f2d_integrate(nbco_ctx *c, const char *who, int scheme, int kind, double *buf, long long n, const double *param, double dt_, double scale_,
                         int elastic, double omega, const nbco_bath *bath = nullptr, unsigned long long tick = 0)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!buf || !param || n <= 0) return c->fail(NBCO_ERR_ARG, w + ": bad arguments");
	if (kind < NBCO_2D_EVAL_DIRECT || kind > NBCO_2D_EVAL_FMM) return c->fail(NBCO_ERR_ARG, w + ": unknown evaluator kind");
	if (scheme < NBCO_INTEG_EULER || scheme > NBCO_INTEG_PEFRL) return c->fail(NBCO_ERR_ARG, w + ": unknown scheme");
	if (omega != 0.0 && (!std::isfinite(omega) || !std::isfinite(omega * dt_))) return c->fail(NBCO_ERR_ARG, w + ": omega must be finite");
	if (bath)
	{
		if (!bath_valid(bath, 2)) return c->fail(NBCO_ERR_ARG, w + ": gamma and kT must be finite and not negative");
		if (bath_off(bath, 2)) bath = nullptr;
		else if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n must be below 2^31 (the row is one counter word)");
		else if (!std::isfinite(dt_) || dt_ < 0.0) return c->fail(NBCO_ERR_ARG, w + ": dt must be finite and not negative with a bath");
	}
	if (kind == NBCO_2D_EVAL_FMM) NBCO_TRY(f2d_fmm_check(c, n));
	double *x = buf, *v = buf + 2 * n, *a = buf + 4 * n;
	const long double dt = dt_, scale = scale_;
	if (bath) NBCO_TRY(f2d_bath(c, v, bath, 0.5 * dt_, 0, tick, n));
	auto K = [&](long double s) { return f2d_step(c, v, a, s, n); };
	auto D = [&](long double s) { return omega == 0.0 ? f2d_step(c, x, v, s, n) : f2d_drift_b(c, x, v, omega, s, n); };
	auto F = [&]() { return f2d_eval(c, kind, buf, n, param, elastic); };
	NBCO_TRY(integ_compose(scheme, dt, scale, K, D, F));
	if (bath) NBCO_TRY(f2d_bath(c, v, bath, 0.5 * dt_, 1, tick, n));
	return f2d_done(c);
}

static int f2d_integrate_steps(nbco_ctx *c, const char *who, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                               int elastic, int steps, double omega, const nbco_bath *bath = nullptr, unsigned long long tick0 = 0)
{
	if (!c) return NBCO_ERR_ARG;
	if (steps < 0) return c->fail(NBCO_ERR_ARG, std::string(who) + ": steps < 0");
	{
		SyncOff quiet(c);
		for (int s = 0; s < steps; ++s)
			NBCO_TRY(f2d_integrate(c, who, scheme, kind, buf, n, param, dt, scale, elastic, omega, bath, tick0 + (unsigned long long)s));
	}
	return f2d_done(c);
}

int nbco_2d_integrate(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale, int elastic)
{
	return f2d_integrate(c, "nbco_2d_integrate", scheme, kind, buf, n, param, dt, scale, elastic, 0.0);
}

int nbco_2d_integrate_steps(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                            int elastic, int steps)
{
	return f2d_integrate_steps(c, "nbco_2d_integrate_steps", scheme, kind, buf, n, param, dt, scale, elastic, steps, 0.0);
}

int nbco_2d_drift_b(nbco_ctx *c, double *x, double *v, long long n, double omega, double s)
{
	if (!c) return NBCO_ERR_ARG;
	if (!x || !v || n < 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_drift_b: bad arguments");
	NBCO_TRY(f2d_drift_b(c, x, v, omega, s, n));
	return f2d_done(c);
}

int nbco_2d_integrate_b(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale, int elastic,
                        double omega)
{
	return f2d_integrate(c, "nbco_2d_integrate_b", scheme, kind, buf, n, param, dt, scale, elastic, omega);
}

int nbco_2d_integrate_steps_b(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                              int elastic, int steps, double omega)
{
	return f2d_integrate_steps(c, "nbco_2d_integrate_steps_b", scheme, kind, buf, n, param, dt, scale, elastic, steps, omega);
}

// ---- Langevin bath, 2-D (include/nbco.h): the bath reads gamma[0..1], kT[0..1] ----------------------------------------------------------
int nbco_2d_bath_apply(nbco_ctx *c, double *v, long long n, const nbco_bath *bath, double s, int half, unsigned long long tick)
{
	if (!c) return NBCO_ERR_ARG;
	if (!v || !bath || n < 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_bath_apply: bad arguments");
	if (half != 0 && half != 1) return c->fail(NBCO_ERR_ARG, "nbco_2d_bath_apply: half must be 0 or 1");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, "nbco_2d_bath_apply: n must be below 2^31 (the row is one counter word)");
	NBCO_TRY(f2d_bath(c, v, bath, s, half, tick, n));
	return f2d_done(c);
}

int nbco_2d_integrate_t(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale, int elastic,
                        double omega, const nbco_bath *bath_host, unsigned long long tick)
{
	if (!c) return NBCO_ERR_ARG;
	if (!bath_host) return c->fail(NBCO_ERR_ARG, "nbco_2d_integrate_t: bath_host is NULL");
	return f2d_integrate(c, "nbco_2d_integrate_t", scheme, kind, buf, n, param, dt, scale, elastic, omega, bath_host, tick);
}

int nbco_2d_integrate_steps_t(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                              int elastic, int steps, double omega, const nbco_bath *bath_host, unsigned long long tick0)
{
	if (!c) return NBCO_ERR_ARG;
	if (!bath_host) return c->fail(NBCO_ERR_ARG, "nbco_2d_integrate_steps_t: bath_host is NULL");
	return f2d_integrate_steps(c, "nbco_2d_integrate_steps_t", scheme, kind, buf, n, param, dt, scale, elastic, steps, omega, bath_host, tick0);
}

int nbco_2d_mean_relerr(nbco_ctx *c, const double *x, const double *ref, long long n, double *out_host)
{
	if (!c) return NBCO_ERR_ARG;
	if (!x || !ref || !out_host || n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_2d_mean_relerr: bad arguments");
	NBCO_TRY(c->reserve(c->f2d_part, sizeof(double) * (4 * kRedBlocks + 8)));
	double *part = c->f2d_part.as<double>();
	const int nb = std::min(kRedBlocks, grid_blocks(n, kB, kGridCap));
	hipLaunchKernelGGL(f2d_relerr_kernel, dim3(nb), dim3(kB), 0, c->stream, (const double2 *)x, (const double2 *)ref, n, part);
	hipLaunchKernelGGL(f2d_relerr_final_kernel, dim3(1), dim3(kB), 0, c->stream, (const double *)part, nb, n, part + 4 * kRedBlocks);
	NBCO_HIP(hipGetLastError());
	NBCO_HIP(hipMemcpyAsync(out_host, part + 4 * kRedBlocks, sizeof(double), hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

// main.cu:120-145 initKV over [positions nb | velocities nb], nb = n
int nbco_2d_init_kv(double *s, long long n, const double *A, const double *om, unsigned long long seed, unsigned long long discard)
{
	if (!s || n <= 0 || !A || !om) return NBCO_ERR_ARG;
	std::mt19937_64 gen(seed);
	gen.discard(discard);
	std::uniform_real_distribution<double> dist(0.0, 1.0);
	const double twopi = 6.283185307179586476925286766559;
	// one glibc sincos per angle: the reference's documented build (GCC at -O2 and above) fuses its sin / cos pair of main.cu:133-136
	// into sincos, whose last bit differs from separate sin and cos for some inputs
	for (long long i = 0; i < n; ++i)
	{
		const double eta = dist(gen), etax = twopi * dist(gen), etay = twopi * dist(gen);
		const double rt = std::sqrt(eta), rt1 = std::sqrt(1 - eta);
		double sx, cx, sy, cy;
		::sincos(etax, &sx, &cx);
		::sincos(etay, &sy, &cy);
		s[2 * i] = A[0] * rt * cx;
		s[2 * i + 1] = A[1] * rt1 * cy;
		s[2 * (n + i)] = A[0] * om[0] * rt * sx;
		s[2 * (n + i) + 1] = A[1] * om[1] * rt1 * sy;
	}
	f2d_center_rms(s, n, A[0] / 2, A[1] / 2);
	f2d_center_rms(s + 2 * n, n, om[0] * A[0] / 2, om[1] * A[1] / 2);
	return NBCO_OK;
}

// main.cu:147-170 initGA: 4n standard normals, positions scaled by x, velocities by u, then centred and RMS-adjusted
int nbco_2d_init_gaussian(double *s, long long n, const double *x2, const double *u2, unsigned long long seed, unsigned long long discard)
{
	if (!s || n <= 0 || !x2 || !u2) return NBCO_ERR_ARG;
	std::mt19937_64 gen(seed);
	gen.discard(discard);
	std::normal_distribution<double> dist(0.0, 1.0);
	for (long long i = 0; i < 4 * n; ++i) s[i] = dist(gen);
	for (long long i = 0; i < n; ++i) { s[2 * i] *= x2[0]; s[2 * i + 1] *= x2[1]; }
	for (long long i = n; i < 2 * n; ++i) { s[2 * i] *= u2[0]; s[2 * i + 1] *= u2[1]; }
	f2d_center_rms(s, n, x2[0], x2[1]);
	f2d_center_rms(s + 2 * n, n, u2[0], u2[1]);
	return NBCO_OK;
}

} // extern "C"
