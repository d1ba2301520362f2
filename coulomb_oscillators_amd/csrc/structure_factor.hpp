// structure_factor.hpp -- the static structure factor (include/nbco.h, nbco_structure_factor): the one place where the numerical rule
// of rho_k = sum_j exp(i k . x_j) is written down.  The device kernels (structure_factor_kernels.hpp), nbco_sk_phase, `nbco3 -cpu -sk`
// (host/nbco_cpu.hpp) and, through the export, the tests all call sk_phase / sk_mul, so that a phase and a complex product are the same
// operations wherever they are formed.
//
// The rule, for k = (ix kx, iy ky, iz kz):
//   w_a = kstep_a / 6.283185307179586 (one division, on the host); t_a = (double) x_a * w_a (one product): the phase in cycles.
//   A particle counts iff every t_a is finite -- for kstep_a below 1e269 that is: iff every coordinate is finite.  One that does not
//   count contributes nothing to any k.
//   e_a = sk_phase(t_a): r = t - rint(t) (exact), q = rint(4 r), s = r - q / 4 (both exact, |s| <= 1/8), theta = 6.283185307179586 * s
//   (one rounding), sin and cos of theta from the Taylor polynomials to theta^19 and theta^18 in z = theta^2 by Horner's scheme with
//   one fma per coefficient, then the quadrant swap by q.  No libm / ocml trigonometry: host and device run the same operations, and
//   each component is within 4 * 2^-53 of cos / sin(2 pi r) (measured against long double: 1.5 * 2^-53).  (1, 0) at integer t,
//   (0, 1) at 1/4, (-1, 0) at 1/2 are exact, and sk_phase(-t) is the conjugate of sk_phase(t).
//   Powers by repeated multiplication: z_0 = (1, 0) exactly, z_{m+1} = z_m * z_1 (sk_mul); a negative index takes the conjugate.
//   The term of (ix, iy, iz) is w_ix with w_0 = e_y^iy * e_z^iz (2-D: w_0 = e_y^iy) and w_{m+1} = w_m * e_x; where the ix run is cut
//   into chunks of L, a chunk that starts at c L > 0 begins with w_{cL} = w_0 * e_x^{cL}, the power again by repeated multiplication.
//   sk_mul(a, b) = (fma(a.re, b.re, -(a.im * b.im)), fma(a.re, b.im, a.im * b.re)): two products, two fused multiply-adds.
//   A product with (1, 0) or (0, 0) is exact, so rho at k = 0 is the exact count of the particles that counted.
//
// HOST VERSUS DEVICE: the device cuts the ix run into chunks where hx > 16 and adds the particles in a fixed order of its own (tiles,
// ranges); `nbco3 -cpu -sk` adds them in index order.  THE TWO AGREE ONLY TO ROUNDING, NOT BIT FOR BIT -- the situation of q (not nb)
// in bond_order.hpp.  Each of them returns the same bytes on every call.
#pragma once
#include <cmath>

#ifdef __HIP__   // (compiled as HIP; the host programs compile it as plain C++)
#define NBCO_SK_HD __host__ __device__ __forceinline__
#else
#define NBCO_SK_HD inline
#endif

constexpr double kSkTwoPi = 6.283185307179586;
constexpr int kSkMaxH = 64;   // the largest index per axis

struct SkC { double re, im; };

NBCO_SK_HD SkC sk_mul(SkC a, SkC b)
{
	SkC r;
	r.re = fma(a.re, b.re, -(a.im * b.im));
	r.im = fma(a.re, b.im, a.im * b.re);
	return r;
}

NBCO_SK_HD SkC sk_conj_if(SkC a, bool neg)
{
	if (neg) a.im = -a.im;
	return a;
}

// {cos 2 pi t, sin 2 pi t} of a finite t
NBCO_SK_HD SkC sk_phase(double t)
{
	const double r = t - rint(t);
	const double q = rint(4.0 * r);
	const double s = r - 0.25 * q;
	const double th = kSkTwoPi * s, z = th * th;
	// sin(theta) = theta + theta z (S1 + z (S2 + ..)), S_k = (-1)^k / (2k+1)!
	double p = -8.2206352466243297e-18;                 // -1/19!
	p = fma(p, z, 2.8114572543455206e-15);              //  1/17!
	p = fma(p, z, -7.6471637318198164e-13);             // -1/15!
	p = fma(p, z, 1.6059043836821613e-10);              //  1/13!
	p = fma(p, z, -2.5052108385441720e-08);             // -1/11!
	p = fma(p, z, 2.7557319223985893e-06);              //  1/9!
	p = fma(p, z, -1.9841269841269841e-04);             // -1/7!
	p = fma(p, z, 8.3333333333333332e-03);              //  1/5!
	p = fma(p, z, -1.6666666666666666e-01);             // -1/3!
	const double sn = fma(th * z, p, th);
	// cos(theta) = 1 + z (C1 + z (C2 + ..)), C_k = (-1)^k / (2k)!
	double c = -1.5619206968586225e-16;                 // -1/18!
	c = fma(c, z, 4.7794773323873853e-14);              //  1/16!
	c = fma(c, z, -1.1470745597729725e-11);             // -1/14!
	c = fma(c, z, 2.0876756987868100e-09);              //  1/12!
	c = fma(c, z, -2.7557319223985888e-07);             // -1/10!
	c = fma(c, z, 2.4801587301587302e-05);              //  1/8!
	c = fma(c, z, -1.3888888888888889e-03);             // -1/6!
	c = fma(c, z, 4.1666666666666664e-02);              //  1/4!
	c = fma(c, z, -0.5);                                // -1/2!
	const double cs = fma(z, c, 1.0);
	// the quarter turns: q in {-2, .., 2}; 0.0 - v keeps a zero positive
	SkC e;
	if (q == 0.0) { e.re = cs; e.im = sn; }
	else if (q == 1.0) { e.re = 0.0 - sn; e.im = cs; }
	else if (q == -1.0) { e.re = sn; e.im = 0.0 - cs; }
	else { e.re = 0.0 - cs; e.im = 0.0 - sn; }
	return e;
}

// K of a grid (dim 2 reads h[0..1])
inline long long sk_count(const int *h, int dim)
{
	return (long long)(h[0] + 1) * (2 * h[1] + 1) * (dim == 3 ? 2 * h[2] + 1 : 1);
}
