// nbco_cpu.hpp -- host-only force / step functions for `nbco3 -cpu` (BASELINE config 1: direct O(N^2), leapfrog, C++20 threads).
//
// Plumbing, not the product: the MI355X engine has no CPU fallback and nothing here is used by libnbco_hip.so.  These are the
// reference's CPU function-pointer conventions (evaluator f(p, a, n, param), step(b, a, ds, n): direct.cuh:246-256,
// kernel.cuh:106-117, :151-173) over std::jthread: every worker owns a contiguous range of particles, as the reference's
// CPU_THREADS workers do.  The evaluator is the compensated direct sum (direct3_cpu, the project's accuracy reference); the
// reference's `-cpu` switch runs its kd-tree FMM on the host instead -- that twin is out of scope here, so `-cpu`
// is meant for small N.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>
#include <limits>
#include "../../include/nbco.h"
#include "../csrc/integ_compose.hpp"
#include "../csrc/bond_order.hpp"
#include "../csrc/structure_factor.hpp"
#include "../csrc/time_corr.hpp"
#include "../csrc/modes.hpp"

namespace nbco_cpu {

struct V3 { float x, y, z; };

inline int &threads() { static int t = 8; return t; }   // constants.cuh:51 CPU_THREADS

template <class F> void for_ranges(int n, F &&body)
{
	const int workers = std::max(1, std::min(threads(), n));
	const int per = (n - 1) / workers + 1;
	std::vector<std::jthread> pool;
	pool.reserve((size_t)workers);
	for (int w = 0; w < workers; ++w)
	{
		const int lo = per * w, hi = std::min(per * (w + 1), n);
		if (lo < hi) pool.emplace_back([=, &body] { body(lo, hi); });
	}
}   // (jthreads join here)

// a_i = k sum_j d_ij / (|d_ij|^2 + eps2)^(3/2), d_ij = p_i - p_j, j = i included (it contributes exactly zero), every term
// folded into a compensated (Kahan) running sum, all in fp32 (direct.cuh:192-226)
inline void direct3(const V3 *p, V3 *a, int n, const float *param, float eps2)
{
	const float k = param ? param[0] : 1.f;
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			float sx = 0.f, sy = 0.f, sz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
			const V3 pi = p[i];
			for (int j = 0; j < n; ++j)
			{
				const float dx = pi.x - p[j].x, dy = pi.y - p[j].y, dz = pi.z - p[j].z;
				const float inv2 = 1.f / (dx * dx + dy * dy + dz * dz + eps2);
				const float w = std::sqrt(inv2);
				const float yx = dx * inv2 * w - cx, yy = dy * inv2 * w - cy, yz = dz * inv2 * w - cz;
				const float tx = sx + yx, ty = sy + yy, tz = sz + yz;
				cx = (tx - sx) - yx; cy = (ty - sy) - yy; cz = (tz - sz) - yz;
				sx = tx; sy = ty; sz = tz;
			}
			a[i] = V3{k * sx, k * sy, k * sz};
		}
	});
}

inline void step(V3 *b, const V3 *a, float ds, int n)   // b += a * ds
{
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i) { b[i].x += a[i].x * ds; b[i].y += a[i].y * ds; b[i].z += a[i].z * ds; }
	});
}

inline void add_elastic(const V3 *p, V3 *a, int n, const float *k3)   // a -= k o p
{
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i) { a[i].x -= p[i].x * k3[0]; a[i].y -= p[i].y * k3[1]; a[i].z -= p[i].z * k3[2]; }
	});
}

// coulombOscillatorDirect_cpu (main3.cu:53-57): direct sum + trap
inline void force(V3 *buf, int n, const float *par, float eps2)
{
	direct3(buf, buf + 2 * (size_t)n, n, par, eps2);
	add_elastic(buf, buf + 2 * (size_t)n, n, par + 3);
}

// {kinetic, elastic, coulomb} of buf = [pos | vel | ..] in fp64 over the fp32 state (`nbco3 -cpu -energy`): the exact pair sum
// sum_{i < j} (|x_i - x_j|^2 + eps2)^(-1/2) par[0] -- the self pair is excluded by index, eps2 is widened from float -- with one
// partial sum per worker, added in worker order
inline void energy(const V3 *buf, int n, const float *par, float eps2, double (&out3)[3])
{
	const V3 *x = buf, *v = buf + n;
	double ke = 0, pe = 0;
	for (int i = 0; i < n; ++i)
	{
		ke += 0.5 * ((double)v[i].x * v[i].x + (double)v[i].y * v[i].y + (double)v[i].z * v[i].z);
		pe += 0.5 * ((double)par[3] * x[i].x * x[i].x + (double)par[4] * x[i].y * x[i].y + (double)par[5] * x[i].z * x[i].z);
	}
	const int workers = std::max(1, std::min(threads(), n)), per = (n - 1) / workers + 1;
	std::vector<double> part((size_t)workers, 0.0);
	double *pp = part.data();
	for_ranges(n, [=](int lo, int hi) {
		double s = 0;
		for (int i = lo; i < hi; ++i)
			for (int j = i + 1; j < n; ++j)
			{
				const double dx = (double)x[i].x - x[j].x, dy = (double)x[i].y - x[j].y, dz = (double)x[i].z - x[j].z;
				s += 1.0 / std::sqrt(dx * dx + dy * dy + dz * dz + (double)eps2);
			}
		pp[lo / per] = s;
	});
	double ce = 0;
	for (double s : part) ce += s;
	out3[0] = ke; out3[1] = pe; out3[2] = ce * (double)par[0];
}

// Phase-space sums of buf = [pos | vel | ..] for `nbco3 -cpu -moments`, the two passes of nbco_beam_moments in fp64 over the fp32
// state: first the means (sum / n; the value itself for a coordinate that is the same in every particle) and the exact extrema of
// q = (x, y, z, vx, vy, vz), then the central sums with d = q - mean: cov[a][b] = <d_a d_b> (both triangles) and per plane
// k = (q_k, q_(3 + k)) m4[k] = <x^4>, <x^3 e>, <x^2 e^2>, <x e^3>, <e^4>.  nbco_moments_derive (include/nbco.h) makes the
// emittances and halo parameters of them, as it does for the device's sums.
inline void moment_sums(const V3 *buf, int n, double (&mean)[6], double (&mn)[6], double (&mx)[6], double (&cov)[6][6], double (&m4)[3][5])
{
	auto coord = [=](int i, int a) { const V3 &r = buf[a < 3 ? i : n + i]; return (double)(a % 3 == 0 ? r.x : a % 3 == 1 ? r.y : r.z); };
	for (int a = 0; a < 6; ++a)
	{
		double s = 0;
		mn[a] = mx[a] = coord(0, a);
		for (int i = 0; i < n; ++i) { const double q = coord(i, a); s += q; mn[a] = std::min(mn[a], q); mx[a] = std::max(mx[a], q); }
		mean[a] = mn[a] == mx[a] ? mn[a] : s / (double)n;
	}
	for (auto &row : cov) for (double &v : row) v = 0;
	for (auto &row : m4) for (double &v : row) v = 0;
	for (int i = 0; i < n; ++i)
	{
		double d[6];
		for (int a = 0; a < 6; ++a) d[a] = coord(i, a) - mean[a];
		for (int a = 0; a < 6; ++a)
			for (int b = a; b < 6; ++b) cov[a][b] += d[a] * d[b];
		for (int k = 0; k < 3; ++k)
		{
			const double x2 = d[k] * d[k], e2 = d[3 + k] * d[3 + k], xe = d[k] * d[3 + k];
			m4[k][0] += x2 * x2; m4[k][1] += x2 * xe; m4[k][2] += x2 * e2; m4[k][3] += xe * e2; m4[k][4] += e2 * e2;
		}
	}
	for (int a = 0; a < 6; ++a)
		for (int b = a; b < 6; ++b) cov[b][a] = cov[a][b] = cov[a][b] / (double)n;
	for (auto &row : m4) for (double &v : row) v /= (double)n;
}

// The records of nbco_slice_moments for `nbco3 -cpu -slices`: a particle's slice by the bin rule of nbco_hist on the widened
// coordinate (scale = bins / (hi - lo) once; inside iff q >= lo && q < hi, so a NaN is outside; b = (int) ((q - lo) * scale), clamped to
// bins - 1), then moment_sums over each slice's particles in state order and nbco_moments_derive.  An empty slice is n = 0, dim and zeros.
// rec gets ax.bins records; returns the number of particles outside the window.
inline long long slice_moments(const V3 *buf, int n, const nbco_hist_axis &ax, std::vector<nbco_moments> &rec)
{
	const double scale = (double)ax.bins / (ax.hi - ax.lo);
	std::vector<std::vector<int>> rows((size_t)ax.bins);
	long long outside = 0;
	for (int i = 0; i < n; ++i)
	{
		const V3 &r = buf[ax.coord < 3 ? i : n + i];
		const double q = (double)(ax.coord % 3 == 0 ? r.x : ax.coord % 3 == 1 ? r.y : r.z);
		if (!(q >= ax.lo && q < ax.hi)) { ++outside; continue; }
		const double t = (q - ax.lo) * scale;
		rows[(size_t)(t < (double)ax.bins ? (int)t : ax.bins - 1)].push_back(i);
	}
	rec.assign((size_t)ax.bins, nbco_moments{});
	std::vector<V3> part;
	for (int s = 0; s < ax.bins; ++s)
	{
		nbco_moments &m = rec[(size_t)s];
		const int k = (int)rows[(size_t)s].size();
		m.n = k;
		m.dim = 3;
		if (!k) continue;
		part.resize(2 * (size_t)k);
		for (int j = 0; j < k; ++j) { part[(size_t)j] = buf[rows[(size_t)s][(size_t)j]]; part[(size_t)(k + j)] = buf[n + rows[(size_t)s][(size_t)j]]; }
		moment_sums(part.data(), k, m.mean, m.min, m.max, m.cov, m.m4);
		nbco_moments_derive(&m);
	}
	return outside;
}

// Pair statistics of the positions x[0..n) for `nbco3 -cpu -pairs`, by the pair rule of nbco_pair_hist (include/nbco.h) in fp64 over
// the fp32 positions: r2 = (dx dx + dy dy) + dz dz with every product and sum rounded once (the program is compiled with
// -ffp-contract=off), inside iff r2 < rmax * rmax, bin = the largest b with (b width)^2 <= r2, width = rmax / bins.  counts gets
// bins + 1 values: the unordered pairs i < j per bin, then the pairs outside; nn2 gets n values: the smallest r2 to another particle
// inside, +infinity where there is none.  Every worker owns a range of i, takes all j != i for the minimum and counts the pairs
// with i < j into counts of its own, which are added at the end: integers, so the split does not show.
inline void pair_stats(const V3 *x, int n, int bins, double rmax, std::vector<unsigned long long> &counts, std::vector<double> &nn2)
{
	const double R2 = rmax * rmax, width = rmax / (double)bins;
	std::vector<double> lower2((size_t)bins);
	for (int b = 0; b < bins; ++b) { const double e = (double)b * width; lower2[(size_t)b] = e * e; }
	const int workers = std::max(1, std::min(threads(), n)), per = (n - 1) / workers + 1;
	std::vector<unsigned long long> part((size_t)workers * (size_t)bins, 0ull);
	unsigned long long *pp = part.data();
	const double *l2 = lower2.data();
	double *nn = nn2.data();
	for_ranges(n, [=](int lo, int hi) {
		unsigned long long *mine = pp + (size_t)(lo / per) * (size_t)bins;
		for (int i = lo; i < hi; ++i)
		{
			double best = INFINITY;
			for (int j = 0; j < n; ++j)
			{
				if (j == i) continue;
				const double dx = (double)x[i].x - (double)x[j].x, dy = (double)x[i].y - (double)x[j].y, dz = (double)x[i].z - (double)x[j].z;
				const double xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = xx + yy, r2 = xy + zz;
				if (!(r2 < R2)) continue;
				best = std::min(best, r2);
				if (i < j) ++mine[(std::upper_bound(l2, l2 + bins, r2) - l2) - 1];   // (lower2[0] = 0 <= r2: never before the first)
			}
			nn[i] = best;
		}
	});
	counts.assign((size_t)bins + 1, 0ull);
	unsigned long long inside = 0;
	for (int w = 0; w < workers; ++w)
		for (int b = 0; b < bins; ++b) counts[(size_t)b] += part[(size_t)w * (size_t)bins + (size_t)b];
	for (int b = 0; b < bins; ++b) inside += counts[(size_t)b];
	counts[(size_t)bins] = (unsigned long long)n * (unsigned long long)(n - 1) / 2ull - inside;
}

// Bond-orientational order of the positions x[0..n) for `nbco3 -cpu -bonds`, by the neighbour rule of nbco_bond_order (include/nbco.h)
// in fp64 over the fp32 positions: d = x_j - x_i, r2 = (dx dx + dy dy) + dz dz with every product and sum rounded once (the program is
// compiled with -ffp-contract=off), j a neighbour of i iff 0 < r2 && r2 < rmax * rmax; the harmonics of a bond, q from the sums and the
// summary come from csrc/bond_order.hpp, the header the device kernels use.  nb gets n values, q gets n pairs {q4, q6}.  Every worker
// owns a range of i and takes all j in index order; the summary adds the particles in index order afterwards.
inline void bond_order(const V3 *x, int n, double rmax, std::vector<int> &nb, std::vector<double> &q, nbco_bond_summary &sum)
{
	const double R2 = rmax * rmax;
	nb.assign((size_t)n, 0);
	q.assign(2 * (size_t)n, 0.0);
	std::vector<double> sums((size_t)kBondSums3 * (size_t)n, 0.0);
	int *nbp = nb.data();
	double *qp = q.data(), *sp = sums.data();
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			double S[kBondSums3] = {};
			int cnt = 0;
			for (int j = 0; j < n; ++j)
			{
				const double dx = (double)x[j].x - (double)x[i].x, dy = (double)x[j].y - (double)x[i].y, dz = (double)x[j].z - (double)x[i].z;
				const double xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = xx + yy, r2 = xy + zz;
				if (!(0.0 < r2 && r2 < R2)) continue;
				++cnt;
				bond_add<3>(dx, dy, dz, r2, S);
			}
			double qi[2];
			bond_q<3>(S, cnt, qi);
			nbp[i] = cnt;
			qp[2 * (size_t)i] = qi[0]; qp[2 * (size_t)i + 1] = qi[1];
			std::copy(S, S + kBondSums3, sp + (size_t)kBondSums3 * (size_t)i);
		}
	});
	double S[kBondSums3] = {}, qsum[2] = {0.0, 0.0};
	long long bonds = 0, isolated = 0, top = 0;
	for (int i = 0; i < n; ++i)
	{
		for (int m = 0; m < kBondSums3; ++m) S[m] += sums[(size_t)kBondSums3 * (size_t)i + (size_t)m];
		if (nb[(size_t)i] > 0) { qsum[0] += q[2 * (size_t)i]; qsum[1] += q[2 * (size_t)i + 1]; }
		else ++isolated;
		bonds += nb[(size_t)i];
		top = std::max<long long>(top, nb[(size_t)i]);
	}
	sum = nbco_bond_summary{};
	bond_summary_fill(S, qsum, bonds, isolated, top, n, 3, sum);
}

// Crystalline particles of the positions x[0..n) for `nbco3 -cpu -solid`, by the rule of nbco_bond_solid (include/nbco.h) with the
// functions of csrc/bond_order.hpp that the device kernels use: pass 1 leaves every particle's bond vector record (bond_vector), pass 2
// takes the same neighbours again in index order, counts the bonds with bond_coherence > dmin into xi and adds the records into the
// averaged order (bond_avg_add, the particle itself first; bond_qbar).  nb and xi get n values, qbar n pairs {q-bar_4, q-bar_6}.
inline void bond_solid(const V3 *x, int n, double rmax, double dmin, int xi_min, std::vector<int> &nb, std::vector<int> &xi, std::vector<double> &qbar,
                       nbco_solid_summary &sum)
{
	const double R2 = rmax * rmax;
	nb.assign((size_t)n, 0);
	xi.assign((size_t)n, 0);
	qbar.assign(2 * (size_t)n, 0.0);
	std::vector<double> vec((size_t)kBondVec * (size_t)n, 0.0);
	int *nbp = nb.data(), *xip = xi.data();
	double *qp = qbar.data(), *vp = vec.data();
	// f(j) for the neighbours j of i, in index order
	auto neighbours = [=](int i, auto &&f) {
		for (int j = 0; j < n; ++j)
		{
			const double dx = (double)x[j].x - (double)x[i].x, dy = (double)x[j].y - (double)x[i].y, dz = (double)x[j].z - (double)x[i].z;
			const double xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = xx + yy, r2 = xy + zz;
			if (0.0 < r2 && r2 < R2) f(j, dx, dy, dz, r2);
		}
	};
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			double S[kBondSums3] = {}, v[kBondVec];
			int cnt = 0;
			neighbours(i, [&](int, double dx, double dy, double dz, double r2) { ++cnt; bond_add<3>(dx, dy, dz, r2, S); });
			bond_vector(S, cnt, v);
			nbp[i] = cnt;
			std::copy(v, v + kBondVec, vp + (size_t)kBondVec * (size_t)i);
		}
	});
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			const double *own = vp + (size_t)kBondVec * (size_t)i;
			double T[kBondSums3] = {}, q[2];
			bond_avg_add(own, T);
			int solid = 0;
			neighbours(i, [&](int j, double, double, double, double) {
				const double *f = vp + (size_t)kBondVec * (size_t)j;
				if (bond_coherence(own + kBondVec6, f + kBondVec6) > dmin) ++solid;
				bond_avg_add(f, T);
			});
			bond_qbar(T, nbp[i], q);
			xip[i] = solid;
			qp[2 * (size_t)i] = q[0]; qp[2 * (size_t)i + 1] = q[1];
		}
	});
	double qsum[2] = {0.0, 0.0};
	long long bonds = 0, isolated = 0, solid_bonds = 0, n_solid = 0, top = 0;
	for (int i = 0; i < n; ++i)
	{
		if (nb[(size_t)i] > 0) { qsum[0] += qbar[2 * (size_t)i]; qsum[1] += qbar[2 * (size_t)i + 1]; }
		else ++isolated;
		bonds += nb[(size_t)i];
		solid_bonds += xi[(size_t)i];
		if (xi[(size_t)i] >= xi_min) ++n_solid;
		top = std::max<long long>(top, xi[(size_t)i]);
	}
	sum = nbco_solid_summary{};
	bond_solid_summary_fill(qsum, bonds, isolated, solid_bonds, n_solid, top, n, dmin, xi_min, sum);
}

// The static structure factor of the positions x[0..n) for `nbco3 -cpu -sk`, by the rule of nbco_structure_factor (include/nbco.h) from
// csrc/structure_factor.hpp, the header the device kernels use: the phases sk_phase(t_a), the powers and the products by sk_mul, the
// term (e_y^iy e_z^iz) e_x^ix with one multiplication per ix.  rho gets K pairs {re, im}; returns the number of particles that counted.
// A fixed partition: every worker owns a range of columns (iy, iz) and adds all particles in index order, in blocks of 64 whose tables
// it forms itself, so the bytes do not depend on the number of threads.  The device adds in another order: equal to rounding only.
inline long long structure_factor(const V3 *x, int n, const nbco_sk_grid &g, std::vector<double> &rho)
{
	const int hx = g.h[0], hy = g.h[1], hz = g.h[2], ny = 2 * hy + 1, nz = 2 * hz + 1, cols = ny * nz;
	const double w[3] = {g.kstep[0] / kSkTwoPi, g.kstep[1] / kSkTwoPi, g.kstep[2] / kSkTwoPi};
	rho.assign(2 * (size_t)sk_count(g.h, 3), 0.0);
	double *out = rho.data();
	for_ranges(cols, [=](int lo, int hi) {
		constexpr int B = 64;
		std::vector<SkC> ex(B), ty((size_t)B * (hy + 1)), tz((size_t)B * (hz + 1));
		for (int base = 0; base < n; base += B)
		{
			const int cnt = std::min(B, n - base);
			for (int j = 0; j < cnt; ++j)
			{
				const V3 p = x[base + j];
				const double t0 = (double)p.x * w[0], t1 = (double)p.y * w[1], t2 = (double)p.z * w[2];
				const bool ok = std::isfinite(t0) && std::isfinite(t1) && std::isfinite(t2);
				const SkC zero{0.0, 0.0}, first{ok ? 1.0 : 0.0, 0.0};
				ex[j] = ok ? sk_phase(t0) : zero;
				SkC *py = &ty[(size_t)j * (hy + 1)], *pz = &tz[(size_t)j * (hz + 1)];
				const SkC ey = ok ? sk_phase(t1) : zero, ez = ok ? sk_phase(t2) : zero;
				py[0] = pz[0] = first;
				for (int m = 1; m <= hy; ++m) py[m] = m == 1 ? ey : sk_mul(py[m - 1], ey);
				for (int m = 1; m <= hz; ++m) pz[m] = m == 1 ? ez : sk_mul(pz[m - 1], ez);
			}
			for (int col = lo; col < hi; ++col)
			{
				const int iy = col / nz - hy, iz = col % nz - hz;
				for (int j = 0; j < cnt; ++j)
				{
					SkC v = sk_mul(sk_conj_if(ty[(size_t)j * (hy + 1) + std::abs(iy)], iy < 0), sk_conj_if(tz[(size_t)j * (hz + 1) + std::abs(iz)], iz < 0));
					for (int ix = 0; ix <= hx; ++ix)
					{
						double *o = out + 2 * ((size_t)ix * (size_t)cols + (size_t)col);
						o[0] += v.re;
						o[1] += v.im;
						v = sk_mul(v, ex[j]);
					}
				}
			}
		}
	});
	return (long long)rho[2 * ((size_t)hy * nz + hz)];
}

// One frame of mode records for `nbco3 -cpu -modes`, by the rule of nbco_modes_record (include/nbco.h) from csrc/modes.hpp, the header
// the device kernels use: the phases, powers and products of structure_factor above, a particle counting iff its phases and its three
// velocity floats are finite, md_add per counted particle and k.  st = [pos n | vel n | ..]; series holds K x frames_cap x 8 doubles and
// frame `frame` of every k is overwritten.  Returns the number of particles that counted.  A fixed partition: every worker owns a range
// of columns (iy, iz) and adds all particles in index order.  The device adds in another order: equal to rounding only.
inline long long modes_record(const V3 *st, int n, const nbco_sk_grid &g, std::vector<double> &series, int frames_cap, int frame)
{
	const int hx = g.h[0], hy = g.h[1], hz = g.h[2], ny = 2 * hy + 1, nz = 2 * hz + 1, cols = ny * nz;
	const double w[3] = {g.kstep[0] / kSkTwoPi, g.kstep[1] / kSkTwoPi, g.kstep[2] / kSkTwoPi};
	double *out = series.data();
	for_ranges(cols, [=](int lo, int hi) {
		std::vector<MdRec> acc((size_t)(hi - lo) * (hx + 1));
		for (MdRec &r : acc) md_zero(r);
		std::vector<SkC> ty((size_t)hy + 1), tz((size_t)hz + 1);
		for (int j = 0; j < n; ++j)
		{
			const V3 p = st[j], v = st[n + j];
			const double t0 = (double)p.x * w[0], t1 = (double)p.y * w[1], t2 = (double)p.z * w[2];
			if (!(std::isfinite(t0) && std::isfinite(t1) && std::isfinite(t2) && std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z))) continue;
			const SkC ex = sk_phase(t0), ey = sk_phase(t1), ez = sk_phase(t2);
			ty[0] = tz[0] = SkC{1.0, 0.0};
			for (int m = 1; m <= hy; ++m) ty[m] = m == 1 ? ey : sk_mul(ty[m - 1], ey);
			for (int m = 1; m <= hz; ++m) tz[m] = m == 1 ? ez : sk_mul(tz[m - 1], ez);
			for (int col = lo; col < hi; ++col)
			{
				const int iy = col / nz - hy, iz = col % nz - hz;
				SkC t = sk_mul(sk_conj_if(ty[std::abs(iy)], iy < 0), sk_conj_if(tz[std::abs(iz)], iz < 0));
				for (int ix = 0; ix <= hx; ++ix)
				{
					md_add(acc[(size_t)(col - lo) * (hx + 1) + ix], t, (double)v.x, (double)v.y, (double)v.z);
					t = sk_mul(t, ex);
				}
			}
		}
		for (int col = lo; col < hi; ++col)
			for (int ix = 0; ix <= hx; ++ix)
			{
				const MdRec &r = acc[(size_t)(col - lo) * (hx + 1) + ix];
				double *o = out + (((size_t)ix * (size_t)cols + (size_t)col) * (size_t)frames_cap + (size_t)frame) * 8;
				o[0] = r.rho.re; o[1] = r.rho.im; o[2] = r.jx.re; o[3] = r.jx.im; o[4] = r.jy.re; o[5] = r.jy.im; o[6] = r.jz.re; o[7] = r.jz.im;
			}
	});
	return (long long)series[(((size_t)hy * nz + hz) * (size_t)frames_cap + (size_t)frame) * 8];
}

// One frame of a trajectory buffer for `nbco3 -cpu -corr`, as nbco_traj_record (include/nbco.h) writes it: frame `frame` of every row
// NaN, then the six floats of every state row whose particle number ids[i] is a multiple of stride with ids[i] / stride < rows, bit for
// bit.  st = [pos n | vel n | ..]; traj holds rows x frames_cap x 6 floats.  The host never permutes: ids are the numbers the caller
// keeps through its apertures.
inline void traj_record(const V3 *st, int n, const std::vector<int> &ids, std::vector<float> &traj, long long rows, int frames_cap, int frame, int stride)
{
	const float q = std::numeric_limits<float>::quiet_NaN();
	for (long long r = 0; r < rows; ++r)
		for (int j = 0; j < 6; ++j) traj[((size_t)r * frames_cap + frame) * 6 + j] = q;
	for (int i = 0; i < n; ++i)
	{
		const int p = ids[(size_t)i];
		if (p < 0 || p % stride != 0 || p / stride >= rows) continue;
		float *o = &traj[((size_t)(p / stride) * frames_cap + frame) * 6];
		o[0] = st[i].x; o[1] = st[i].y; o[2] = st[i].z;
		o[3] = st[n + i].x; o[4] = st[n + i].y; o[5] = st[n + i].z;
	}
}

// The raw time-correlation sums of `nbco3 -cpu -corr`, by the rule of nbco_time_corr (include/nbco.h) from csrc/time_corr.hpp, the
// header the device kernel uses.  A fixed partition: every worker owns a range of lags and carries one sum per lag through all rows in
// index order, the origins of a row in increasing t, so the bytes do not depend on the number of threads.  The device adds the rows
// in another order: equal to rounding only; pairs equal.
inline void time_corr(const float *traj, long long rows, int frames_cap, int frames, int lags, std::vector<nbco_corr_lag> &out)
{
	out.assign((size_t)lags, nbco_corr_lag{});
	nbco_corr_lag *o = out.data();
	std::vector<unsigned char> fin((size_t)rows * frames);
	for (long long r = 0; r < rows; ++r)
		for (int f = 0; f < frames; ++f) fin[(size_t)r * frames + f] = tc_finite(traj + ((size_t)r * frames_cap + f) * 6) ? 1 : 0;
	const unsigned char *ok = fin.data();
	for_ranges(lags, [=](int lo, int hi) {
		for (int tau = lo; tau < hi; ++tau)
		{
			TcSum s;
			tc_zero(s);
			unsigned long long pairs = 0;
			for (long long r = 0; r < rows; ++r)
			{
				const float *row = traj + (size_t)r * frames_cap * 6;
				for (int t = 0; t + tau < frames; ++t)
				{
					if (!ok[(size_t)r * frames + t] || !ok[(size_t)r * frames + t + tau]) continue;
					const float *a = row + 6 * (size_t)t, *b = row + 6 * (size_t)(t + tau);
					tc_term(s, (double)a[0], (double)a[1], (double)a[2], (double)a[3], (double)a[4], (double)a[5], (double)b[0], (double)b[1], (double)b[2],
					        (double)b[3], (double)b[4], (double)b[5]);
					++pairs;
				}
			}
			for (int c = 0; c < 3; ++c) { o[tau].dx2[c] = s.dx2[c]; o[tau].vv[c] = s.vv[c]; }
			o[tau].r4 = s.r4;
			o[tau].pairs = pairs;
		}
	});
}

// The aperture of `nbco3 -cpu -aperture`, by the rule of nbco_aperture_apply (include/nbco.h) in fp64 over the fp32 positions:
// w_a = 1.0 / half_a (half_a = +infinity: w_a = 0, the axis is open), d_a = (double) x_a - centre_a, a non-finite coordinate is outside;
// shape 0 (ellipsoid): u_a = d_a w_a, s = (u_x u_x + u_y u_y) + u_z u_z with every product and sum rounded once (the program is
// compiled with -ffp-contract=off), inside iff s <= 1.0; shape 1 (box): inside iff fabs(d_a) <= half_a on every axis.
inline bool aperture_inside(const V3 &p, int shape, const double (&centre)[3], const double (&half)[3])
{
	const double q[3]{(double)p.x, (double)p.y, (double)p.z};
	double d[3], u[3];
	bool finite = true, box = true;
	for (int a = 0; a < 3; ++a)
	{
		const double w = 1.0 / half[a];
		finite = finite && std::isfinite(q[a]);
		d[a] = q[a] - centre[a];
		box = box && std::fabs(d[a]) <= half[a];
		u[a] = d[a] * w;
	}
	const double xx = u[0] * u[0], yy = u[1] * u[1], zz = u[2] * u[2], xy = xx + yy, s = xy + zz;
	return finite && (shape == 1 ? box : s <= 1.0);
}

// Stable compaction of buf = [pos n | vel n | acc n] to the particles inside: they keep their order and their bits, buf is resized to
// 3 n' and n becomes n'.  rows receives the rows of the lost particles before the call, in state order, recs one x y z vx vy vz each.
inline void aperture_apply(std::vector<V3> &buf, int &n, int shape, const double (&centre)[3], const double (&half)[3], std::vector<int> &rows,
                           std::vector<float> &recs)
{
	rows.clear();
	recs.clear();
	std::vector<char> keep((size_t)n);
	for (int i = 0; i < n; ++i) keep[(size_t)i] = aperture_inside(buf[(size_t)i], shape, centre, half);
	int kept = 0;
	for (int i = 0; i < n; ++i) kept += keep[(size_t)i];
	if (kept == n) return;
	std::vector<V3> out(3 * (size_t)kept);
	for (int i = 0, j = 0; i < n; ++i)
	{
		const V3 x = buf[(size_t)i], v = buf[(size_t)n + i], a = buf[2 * (size_t)n + i];
		if (keep[(size_t)i]) { out[(size_t)j] = x; out[(size_t)kept + j] = v; out[2 * (size_t)kept + j] = a; ++j; }
		else { rows.push_back(i); recs.insert(recs.end(), {x.x, x.y, x.z, v.x, v.y, v.z}); }
	}
	buf.swap(out);
	n = kept;
}

// The drift in a uniform magnetic field Omega over s (`nbco3 -cpu -B`; include/nbco.h, nbco_drift_b): the matrices from
// nbco_helix_matrices, narrowed to float, and per particle the fmaf order of the device kernels, both lines from the old v.
inline void drift_b(V3 *x, V3 *v, const double *omega, double s, int n)
{
	double Rd[9], Ad[9];
	nbco_helix_matrices(omega, s, Rd, Ad);
	float R[9], A[9];
	for (int i = 0; i < 9; ++i) { R[i] = (float)Rd[i]; A[i] = (float)Ad[i]; }
	const float *r = R, *m = A;
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			const V3 u = v[i], p = x[i];
			x[i] = V3{std::fmaf(m[2], u.z, std::fmaf(m[1], u.y, std::fmaf(m[0], u.x, p.x))), std::fmaf(m[5], u.z, std::fmaf(m[4], u.y, std::fmaf(m[3], u.x, p.y))),
			          std::fmaf(m[8], u.z, std::fmaf(m[7], u.y, std::fmaf(m[6], u.x, p.z)))};
			v[i] = V3{std::fmaf(r[2], u.z, std::fmaf(r[1], u.y, r[0] * u.x)), std::fmaf(r[5], u.z, std::fmaf(r[4], u.y, r[3] * u.x)),
			          std::fmaf(r[8], u.z, std::fmaf(r[7], u.y, r[6] * u.x))};
		}
	});
}

// The Langevin bath of `nbco3 -cpu -bath` (include/nbco.h, nbco_bath_apply), the device's rule restated: Philox4x32-10 over
// key = the seed's two words and counter = (row, axis + 4 half, the tick's two words), the four words summed as an integer, centred and
// scaled by sqrt(3) 2^-32 in double, narrowed to float; v' = (c1 v) + (c2 xi) with the coefficients of nbco_bath_coeffs narrowed to float
// and each product and the sum rounded once (the program is compiled with -ffp-contract=off).  An axis with c1 = 1 and c2 = 0 is left alone.
inline void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4])
{
	uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
	for (int r = 0; r < 10; ++r)
	{
		const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

inline double bath_xi(unsigned long long seed, unsigned long long tick, int half, uint32_t row, int axis)
{
	const uint32_t ctr[4]{row, (uint32_t)(axis + 4 * half), (uint32_t)tick, (uint32_t)(tick >> 32)}, key[2]{(uint32_t)seed, (uint32_t)(seed >> 32)};
	uint32_t w[4];
	philox4x32_10(ctr, key, w);
	const long long S = (long long)w[0] + (long long)w[1] + (long long)w[2] + (long long)w[3];
	return (double)(S - 0x1FFFFFFFELL) * 0x1.bb67ae8584caap-32;
}

inline void bath_apply(V3 *v, int n, const nbco_bath &bath, double s, int half, unsigned long long tick)
{
	double c1d[3], c2d[3];
	if (nbco_bath_coeffs(&bath, s, c1d, c2d) != NBCO_OK) return;
	const float c1[3]{(float)c1d[0], (float)c1d[1], (float)c1d[2]}, c2[3]{(float)c2d[0], (float)c2d[1], (float)c2d[2]};
	const unsigned long long seed = bath.seed;
	for_ranges(n, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			float *q = &v[i].x;
			for (int a = 0; a < 3; ++a)
			{
				if (c1[a] == 1.f && c2[a] == 0.f) continue;
				const float xi = (float)bath_xi(seed, tick, half, (uint32_t)i, a);
				const float p = c1[a] * q[a], r = c2[a] * xi;
				q[a] = p + r;
			}
		}
	});
}

// one step of a scheme (NBCO_INTEG_*), composed by integ_compose as in the library (coefficients in long double, narrowed at the step call);
// omega: null, or the uniform magnetic field whose helix drift replaces x += v c; bath: null, or the Langevin bath whose two half steps
// O(dt/2) wrap the scheme, at the step number `tick`
inline void integrate_scheme(int scheme, V3 *buf, int n, const float *par, float eps2, long double dt, const double *omega)
{
	V3 *x = buf, *v = buf + n, *a = buf + 2 * (size_t)n;
	auto K = [&](long double c) { step(v, a, (float)c, n); return NBCO_OK; };
	auto D = [&](long double c) { if (omega) drift_b(x, v, omega, (double)c, n); else step(x, v, (float)c, n); return NBCO_OK; };
	auto F = [&] { force(buf, n, par, eps2); return NBCO_OK; };
	integ_compose(scheme, dt, 1.0L, K, D, F);
}
inline void integrate(int scheme, V3 *buf, int n, const float *par, float eps2, long double dt, const double *omega = nullptr, const nbco_bath *bath = nullptr,
                      unsigned long long tick = 0)
{
	if (bath) bath_apply(buf + n, n, *bath, 0.5 * (double)dt, 0, tick);
	integrate_scheme(scheme, buf, n, par, eps2, dt, omega);
	if (bath) bath_apply(buf + n, n, *bath, 0.5 * (double)dt, 1, tick);
}

} // namespace nbco_cpu
