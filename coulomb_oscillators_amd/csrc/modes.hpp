// modes.hpp -- collective dynamics (include/nbco.h: nbco_modes_record, nbco_mode_corr): the one place where the numerical rule of the
// density and current modes rho_k = sum_j exp(i k . x_j), j_k = sum_j v_j exp(i k . x_j) and of their time correlations is written
// down.  The device kernels (modes_kernels.hpp), nbco_mode_corr_ref, nbco_mode_corr_derive and `nbco3 -cpu -modes`
// (host/nbco_cpu.hpp) all use it, so that a term is the same operations wherever it is formed.
//
// THE MODE RECORD of a wave vector k = (ix kx, iy ky, iz kz) is eight doubles {rho.re, rho.im, jx.re, jx.im, jy.re, jy.im, jz.re, jz.im}.
//   The phases t_a, their powers and the term w of (ix, iy, iz) are exactly those of structure_factor.hpp.
//   A particle counts iff every t_a is finite and all three velocity floats are finite; one that does not count adds nothing to any
//   of the four sums.  Per counted particle and k (md_add): rho.re += w.re; rho.im += w.im; j_c.re <- fma(v_c, w.re, j_c.re);
//   j_c.im <- fma(v_c, w.im, j_c.im), v_c the float widened to double (exact).
//   At k = 0 every w is (1, 0): rho is exactly (n_used, 0) and the imaginary part of j is exactly 0.
//   The rho of a record need not have the bytes of nbco_structure_factor: that call counts by the positions alone and cuts the ix runs
//   and the particle ranges differently.
//
// THE CORRELATION TERM of one k, an origin t and a lag tau, a = record(t), b = record(t + tau), k_c = (double) i_c * kstep_c (one product):
//   P(r).re = fma(k_z, r.jz.re, fma(k_y, r.jy.re, k_x * r.jx.re)), P(r).im likewise: k . j, the longitudinal current times |k|.
//   rr <- fma(a.rho.im, b.rho.im, fma(a.rho.re, b.rho.re, rr))                               Re[rho(t + tau) conj rho(t)]
//   jj <- six fma in the order x.re, x.im, y.re, y.im, z.re, z.im                            Re[j(t + tau) . conj j(t)]
//   ll <- fma(P(a).im, P(b).im, fma(P(a).re, P(b).re, ll))                                   Re[P(t + tau) conj P(t)]
//   s0 += a.rho, s1 += b.rho: complex, plain additions (the means that the connected part subtracts).
//   A (k, tau) adds its terms in increasing t; pairs = frames - tau.  There is no finiteness test: a record is finite by construction,
//   and a non-finite one supplied by the caller propagates.
// The fused multiply-adds are written out, never left to the compiler: the host programs are built with -ffp-contract=off, the library
// with contraction inside an expression only, and no expression here has a product and a sum of its own.
//
// HOST VERSUS DEVICE.  Recording: the device adds the particles in an order of its own (tiles, ranges), `nbco3 -cpu -modes` in index
// order: THE TWO AGREE ONLY TO ROUNDING -- the situation of rho_k in structure_factor.hpp.  Correlation: one lane, or one host loop,
// forms a (k, tau) from start to end in the order above: THE DEVICE AND nbco_mode_corr_ref RETURN THE SAME BYTES for the same series.
#pragma once
#include "structure_factor.hpp"

constexpr int kMdMaxFrames = 1024;   // the longest series a call correlates: 1024 records of 64 bytes are 64 KiB of LDS

// the four complex sums of one k
struct MdRec { SkC rho, jx, jy, jz; };

NBCO_SK_HD void md_zero(MdRec &r)
{
	r.rho.re = r.rho.im = r.jx.re = r.jx.im = r.jy.re = r.jy.im = r.jz.re = r.jz.im = 0.0;
}

// one counted particle: its term w and its widened velocity
NBCO_SK_HD void md_add(MdRec &r, SkC w, double vx, double vy, double vz)
{
	r.rho.re += w.re;
	r.rho.im += w.im;
	r.jx.re = fma(vx, w.re, r.jx.re);
	r.jx.im = fma(vx, w.im, r.jx.im);
	r.jy.re = fma(vy, w.re, r.jy.re);
	r.jy.im = fma(vy, w.im, r.jy.im);
	r.jz.re = fma(vz, w.re, r.jz.re);
	r.jz.im = fma(vz, w.im, r.jz.im);
}

// the wave vector of grid index k (nbco_structure_factor's index, 3-D): k_c = (double) i_c * kstep_c
NBCO_SK_HD void md_wave_vector(long long k, const int *h, const double *kstep, double *kv)
{
	const long long ny = 2 * h[1] + 1, nz = 2 * h[2] + 1;
	kv[0] = (double)(k / (ny * nz)) * kstep[0];
	kv[1] = (double)(k / nz % ny - h[1]) * kstep[1];
	kv[2] = (double)(k % nz - h[2]) * kstep[2];
}

// k . j of a record
NBCO_SK_HD SkC md_long(double kx, double ky, double kz, SkC jx, SkC jy, SkC jz)
{
	SkC p;
	p.re = fma(kz, jz.re, fma(ky, jy.re, kx * jx.re));
	p.im = fma(kz, jz.im, fma(ky, jy.im, kx * jx.im));
	return p;
}

// the seven sums of one (k, lag)
struct MdSum { double rr, ll, jj; SkC s0, s1; };

NBCO_SK_HD void md_sum_zero(MdSum &s)
{
	s.rr = s.ll = s.jj = s.s0.re = s.s0.im = s.s1.re = s.s1.im = 0.0;
}

// one term: a = record(t) with pa = P(a), b = record(t + tau); P(b) is formed here
NBCO_SK_HD void md_term(MdSum &s, double kx, double ky, double kz, SkC arho, SkC ajx, SkC ajy, SkC ajz, SkC pa, SkC brho, SkC bjx, SkC bjy, SkC bjz)
{
	const SkC pb = md_long(kx, ky, kz, bjx, bjy, bjz);
	s.rr = fma(arho.im, brho.im, fma(arho.re, brho.re, s.rr));
	double j = s.jj;
	j = fma(ajx.re, bjx.re, j);
	j = fma(ajx.im, bjx.im, j);
	j = fma(ajy.re, bjy.re, j);
	j = fma(ajy.im, bjy.im, j);
	j = fma(ajz.re, bjz.re, j);
	j = fma(ajz.im, bjz.im, j);
	s.jj = j;
	s.ll = fma(pa.im, pb.im, fma(pa.re, pb.re, s.ll));
	s.s0.re += arho.re;
	s.s0.im += arho.im;
	s.s1.re += brho.re;
	s.s1.im += brho.im;
}

// F, F_c, C_L, C_T of one (k, lag) from its raw sums: four doubles.  pairs == 0 or n_norm <= 0 gives four zeros, k2 == 0 gives
// C_L = C_T = 0: never NaN for finite input.  Every operation is a statement of its own: nothing to contract.
inline void md_derive(double rr, double ll, double jj, const double *s0, const double *s1, unsigned long long pairs, double k2, double n_norm, double *o)
{
	o[0] = o[1] = o[2] = o[3] = 0.0;
	if (pairs == 0 || !(n_norm > 0.0)) return;
	const double m = (double)pairs;
	const double den = m * n_norm;
	o[0] = rr / den;
	const double a = s1[0] * s0[0];
	const double b = s1[1] * s0[1];
	const double mean = (a + b) / m;
	const double conn = rr - mean;
	o[1] = conn / den;
	if (k2 == 0.0) return;
	const double kden = k2 * den;
	o[2] = ll / kden;
	const double lk = ll / k2;
	const double tr = jj - lk;
	o[3] = tr / (2.0 * den);
}

// k^2 = (k_x^2 + k_y^2) + k_z^2, every product and sum rounded on its own
inline double md_k2(const double *kv)
{
	const double x = kv[0] * kv[0];
	const double y = kv[1] * kv[1];
	const double z = kv[2] * kv[2];
	const double xy = x + y;
	return xy + z;
}
