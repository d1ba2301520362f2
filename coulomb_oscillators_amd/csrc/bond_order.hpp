// bond_order.hpp -- bond-orientational order (include/nbco.h, nbco_bond_order): the one place where the harmonics of a bond are formed.
// The device kernels (bond_order_kernels.hpp), nbco_bond_harmonics, `nbco3 -cpu -bonds` (host/nbco_cpu.hpp) and, through the export,
// the tests all call bond_harmonics / bond_powers2, so that a bond contributes the same polynomials wherever it is met.  Further down,
// in the same spirit, the rule of the second pass (nbco_bond_solid): the bond vector record, the coherence of a bond, the averaged order.
// Real orthonormal harmonics of degree 4 and 6 as polynomials in the unit vector (x, y, z): the m-th derivative of the Legendre
// polynomial in z, with its integer coefficients, times the real and the imaginary part of (x + i y)^m from a recurrence, times a
// constant that holds the normalisation sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), the sqrt(2) of m > 0 and the common factor taken out of
// the integer coefficients.  No trigonometry, no table in memory.  Component 0 is m = 0, 2m - 1 the cosine and 2m the sine part of m.
#pragma once
#include <cmath>

#ifdef __HIP__   // (compiled as HIP; the host programs compile it as plain C++)
#define NBCO_BOND_HD __host__ __device__ __forceinline__
#else
#define NBCO_BOND_HD inline
#endif

constexpr double kBondK4[5] = {0.1057855469152043038028, 0.6690465435572891679521, 0.4730873478787800090463, 1.7701307697799305310368,
                               0.6258357354491761345866};
constexpr double kBondK6[7] = {0.0635692022676284259328, 0.5826213625187313888351, 0.4606026297574617495708, 0.9212052595149234991416,
                               0.5045649007287241592545, 2.3666191622317520319877, 0.6831841051919143219748};
constexpr double kBondQ4 = 1.3962634015954636615390;   // 4 pi / 9
constexpr double kBondQ6 = 0.9666438934122440733731;   // 4 pi / 13

// slots of the sums a particle keeps over its bonds: 3-D S_4m in [0, 9) and S_6m in [9, 22); 2-D Re, Im of sum z^4, then of sum z^6
constexpr int kBondSums3 = 22, kBondSums2 = 4;

// y4[9], y6[13] of the unit vector (x, y, z)
NBCO_BOND_HD void bond_harmonics(double x, double y, double z, double (&y4)[9], double (&y6)[13])
{
	const double z2 = z * z;
	// Legendre parts, common integer factors in the constants
	const double a40 = (35.0 * z2 - 30.0) * z2 + 3.0, a41 = z * (7.0 * z2 - 3.0), a42 = 7.0 * z2 - 1.0;
	const double a60 = ((231.0 * z2 - 315.0) * z2 + 105.0) * z2 - 5.0, a61 = z * ((33.0 * z2 - 30.0) * z2 + 5.0), a62 = (33.0 * z2 - 18.0) * z2 + 1.0;
	const double a63 = z * (11.0 * z2 - 3.0), a64 = 11.0 * z2 - 1.0;
	// (x + i y)^m = c_m + i s_m
	const double c2 = x * x - y * y, s2 = 2.0 * (x * y);
	const double c3 = c2 * x - s2 * y, s3 = c2 * y + s2 * x;
	const double c4 = c3 * x - s3 * y, s4 = c3 * y + s3 * x;
	const double c5 = c4 * x - s4 * y, s5 = c4 * y + s4 * x;
	const double c6 = c5 * x - s5 * y, s6 = c5 * y + s5 * x;
	double t;
	y4[0] = kBondK4[0] * a40;
	t = kBondK4[1] * a41; y4[1] = t * x; y4[2] = t * y;
	t = kBondK4[2] * a42; y4[3] = t * c2; y4[4] = t * s2;
	t = kBondK4[3] * z; y4[5] = t * c3; y4[6] = t * s3;
	y4[7] = kBondK4[4] * c4; y4[8] = kBondK4[4] * s4;
	y6[0] = kBondK6[0] * a60;
	t = kBondK6[1] * a61; y6[1] = t * x; y6[2] = t * y;
	t = kBondK6[2] * a62; y6[3] = t * c2; y6[4] = t * s2;
	t = kBondK6[3] * a63; y6[5] = t * c3; y6[6] = t * s3;
	t = kBondK6[4] * a64; y6[7] = t * c4; y6[8] = t * s4;
	t = kBondK6[5] * z; y6[9] = t * c5; y6[10] = t * s5;
	y6[11] = kBondK6[6] * c6; y6[12] = kBondK6[6] * s6;
}

// the 2-D counterpart: p = {Re z^4, Im z^4, Re z^6, Im z^6} of z = x + i y, by repeated complex multiplication
NBCO_BOND_HD void bond_powers2(double x, double y, double (&p)[4])
{
	const double c2 = x * x - y * y, s2 = 2.0 * (x * y);
	const double c4 = c2 * c2 - s2 * s2, s4 = 2.0 * (c2 * s2);
	p[0] = c4; p[1] = s4;
	p[2] = c4 * c2 - s4 * s2; p[3] = c4 * s2 + s4 * c2;
}

// one bond into the sums of its particle: d = x_j - x_i per axis and r2 > 0 by the neighbour rule; u = d * (1 / sqrt(r2))
template <int D> NBCO_BOND_HD void bond_add(double dx, double dy, double dz, double r2, double (&S)[D == 3 ? kBondSums3 : kBondSums2])
{
	const double inv = 1.0 / sqrt(r2);
	if constexpr (D == 3)
	{
		double y4[9], y6[13];
		bond_harmonics(dx * inv, dy * inv, dz * inv, y4, y6);
#pragma unroll
		for (int m = 0; m < 9; ++m) S[m] += y4[m];
#pragma unroll
		for (int m = 0; m < 13; ++m) S[9 + m] += y6[m];
	}
	else
	{
		double p[4];
		bond_powers2(dx * inv, dy * inv, p);
#pragma unroll
		for (int m = 0; m < 4; ++m) S[m] += p[m];
	}
}

// {q4, q6} (2-D: {psi4, psi6}) of a particle with nb neighbours and the sums S; 0 where nb = 0, never NaN
template <int D> NBCO_BOND_HD void bond_q(const double (&S)[D == 3 ? kBondSums3 : kBondSums2], int nb, double (&q)[2])
{
	q[0] = q[1] = 0.0;
	if (nb <= 0) return;
	double a = 0.0, b = 0.0;
	if constexpr (D == 3)
	{
#pragma unroll
		for (int m = 0; m < 9; ++m) a += S[m] * S[m];
#pragma unroll
		for (int m = 0; m < 13; ++m) b += S[9 + m] * S[9 + m];
		a *= kBondQ4; b *= kBondQ6;
	}
	else
	{
		a = S[0] * S[0] + S[1] * S[1];
		b = S[2] * S[2] + S[3] * S[3];
	}
	q[0] = sqrt(a) / (double)nb;
	q[1] = sqrt(b) / (double)nb;
}

// ---- crystalline particles (include/nbco.h, nbco_bond_solid): the second pass over stored S_lm -------------------------------------------
// The bond vector record of a particle, kBondVec doubles: the unit vectors q^_4m = S_4m / |S_4| in [0, 9) and q^_6m = S_6m / |S_6| in
// [9, 22), |S_l| = sqrt(sum_m S_lm^2), then a_4 = |S_4| / nb in [22] and a_6 in [23]: q_l = sqrt(4 pi / (2l+1)) a_l.  A particle without
// neighbours, or a norm of 0, leaves zeros behind, never a NaN.
constexpr int kBondVec = 24, kBondVec6 = 9, kBondVecA = 22;

NBCO_BOND_HD void bond_vector(const double (&S)[kBondSums3], int nb, double (&v)[kBondVec])
{
	double a = 0.0, b = 0.0;
#pragma unroll
	for (int m = 0; m < 9; ++m) a += S[m] * S[m];
#pragma unroll
	for (int m = 0; m < 13; ++m) b += S[9 + m] * S[9 + m];
	a = sqrt(a); b = sqrt(b);
	const bool ok4 = nb > 0 && a > 0.0, ok6 = nb > 0 && b > 0.0;
#pragma unroll
	for (int m = 0; m < 9; ++m) v[m] = ok4 ? S[m] / a : 0.0;
#pragma unroll
	for (int m = 0; m < 13; ++m) v[9 + m] = ok6 ? S[9 + m] / b : 0.0;
	v[kBondVecA] = ok4 ? a / (double)nb : 0.0;
	v[kBondVecA + 1] = ok6 ? b / (double)nb : 0.0;
}

// The coherence of a bond, the part that decides an integer: d6 = (((e0 f0 + e1 f1) + e2 f2) + ... + e12 f12) over the q^_6 of the two
// ends (e6, f6 point at entry kBondVec6 of their records), every product and every sum rounded once, from the left: the same bits from
// either end of the bond and from numpy's elementwise products and sequential adds.  The bond is solid iff d6 > dmin (a NaN is not).
NBCO_BOND_HD double bond_coherence(const double *e6, const double *f6)
{
#pragma clang fp contract(off)   // (a fused e f + d would round once where the rule rounds twice, and differently from the other end)
	double d = e6[0] * f6[0];
#pragma unroll
	for (int m = 1; m < 13; ++m)
	{
		const double t = e6[m] * f6[m];
		d = d + t;
	}
	return d;
}

// one term of the averaged order: T_lm += a_l q^_lm of the record f (the particle itself first, then its neighbours as they are met)
NBCO_BOND_HD void bond_avg_add(const double *f, double (&T)[kBondSums3])
{
	const double a4 = f[kBondVecA], a6 = f[kBondVecA + 1];
#pragma unroll
	for (int m = 0; m < 9; ++m) T[m] += a4 * f[m];
#pragma unroll
	for (int m = 0; m < 13; ++m) T[9 + m] += a6 * f[9 + m];
}

// {q-bar_4, q-bar_6} of Lechner and Dellago from those sums: sqrt(4 pi / (2l+1) sum_m T_lm^2) / (nb + 1); 0 for a particle without neighbours
NBCO_BOND_HD void bond_qbar(const double (&T)[kBondSums3], int nb, double (&q)[2])
{
	q[0] = q[1] = 0.0;
	if (nb <= 0) return;
	double a = 0.0, b = 0.0;
#pragma unroll
	for (int m = 0; m < 9; ++m) a += T[m] * T[m];
#pragma unroll
	for (int m = 0; m < 13; ++m) b += T[9 + m] * T[9 + m];
	q[0] = sqrt(kBondQ4 * a) / (double)(nb + 1);
	q[1] = sqrt(kBondQ6 * b) / (double)(nb + 1);
}

// What a solid summary is made of, in 8-byte slots: 0, 1: the sums of q-bar_4 and q-bar_6 over the particles with nb > 0, then as 64-bit
// integers 2: sum nb, 3: #{nb == 0}, 4: sum xi, 5: #{xi >= xi_min}, 6: max xi.
constexpr int kSolidRec = 7, kSolidRecBonds = 2, kSolidRecIsolated = 3, kSolidRecSolid = 4, kSolidRecCount = 5, kSolidRecMax = 6;

template <class Summary>
inline void bond_solid_summary_fill(const double (&qsum)[2], long long bonds, long long isolated, long long solid_bonds, long long n_solid, long long xi_max,
                                    long long n, double dmin, int xi_min, Summary &s)
{
	s.n = n; s.bonds = bonds; s.isolated = isolated; s.solid_bonds = solid_bonds; s.n_solid = n_solid;
	s.xi_max = (int)xi_max; s.xi_min = xi_min; s.dmin = dmin;
	const long long linked = n - isolated;
	for (int l = 0; l < 2; ++l) s.qbar_mean[l] = linked > 0 ? qsum[l] / (double)linked : 0.0;
}

// What a summary is made of: the sums over the particles, in 8-byte slots.  [0, 22): sum_i S(i) (2-D: the first 4, the others 0),
// 22, 23: the sums of q4 and q6 over the particles with nb > 0, then as 64-bit integers 24: sum nb, 25: #{nb == 0}, 26: max nb.
constexpr int kBondRec = 27, kBondRecQ = 22, kBondRecBonds = 24, kBondRecIsolated = 25, kBondRecMax = 26;

// the summary (nbco_bond_summary) from those sums: the means over the particles with nb > 0, and the global Q from sum_i S(i)
template <class Summary>
inline void bond_summary_fill(const double (&S)[kBondSums3], const double (&qsum)[2], long long bonds, long long isolated, long long nb_max, long long n, int dim,
                              Summary &s)
{
	s.n = n; s.bonds = bonds; s.isolated = isolated;
	s.nb_max = (int)nb_max; s.dim = dim;
	const long long linked = n - isolated;
	for (int l = 0; l < 2; ++l) s.q_mean[l] = linked > 0 ? qsum[l] / (double)linked : 0.0;
	double a = 0.0, b = 0.0;
	if (dim == 3)
	{
		for (int m = 0; m < 9; ++m) a += S[m] * S[m];
		for (int m = 0; m < 13; ++m) b += S[9 + m] * S[9 + m];
		a *= kBondQ4; b *= kBondQ6;
	}
	else
	{
		a = S[0] * S[0] + S[1] * S[1];
		b = S[2] * S[2] + S[3] * S[3];
	}
	s.Q[0] = bonds > 0 ? std::sqrt(a) / (double)bonds : 0.0;
	s.Q[1] = bonds > 0 ? std::sqrt(b) / (double)bonds : 0.0;
}
