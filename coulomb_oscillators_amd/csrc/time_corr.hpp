// time_corr.hpp -- time correlations of tracked particles (include/nbco.h, nbco_time_corr): the one place where the numerical rule of
// the mean-square displacement, its fourth moment and the velocity autocorrelation is written down.  The device kernel
// (time_corr_kernels.hpp), `nbco3 -cpu -corr` (host/nbco_cpu.hpp) and nbco_time_corr_derive all use it, and tests/corr_numpy.py
// follows it, so that a term is the same operations wherever it is formed.
//
// The rule, for one row, an origin t and a lag tau (frame f of a row is six floats x y z vx vy vz):
//   A frame is FINITE iff all six floats are; the triple (row, t, tau) counts iff frames t and t + tau are both finite.
//   Every float is widened to double first (exact).  D_c = x_c(t + tau) - x_c(t): one subtraction, one rounding (exact wherever the
//   exponents of the two floats differ by less than 29).
//   dx2[c] <- fma(D_c, D_c, dx2[c]): the square is not rounded on its own.
//   r2 = fma(D_z, D_z, fma(D_y, D_y, D_x * D_x)): the order (sx + sy) + sz, one product and two fused multiply-adds.
//   r4 <- fma(r2, r2, r4).
//   vv[c] <- fma(v_c(t), v_c(t + tau), vv[c]): the product of two widened floats is exact, so the only roundings are the additions.
//   pairs counts the triples, an exact integer.
// The fused multiply-adds are written out, never left to the compiler: the host programs are built with -ffp-contract=off, the
// library with contraction inside an expression only, and no expression here has a product and a sum of its own.
//
// ORDER OF THE SUMS: a (row, tau) adds its terms in increasing t on every route.  The device carries one sum per (row range, tau)
// through the rows of a range and then adds the ranges in index order; `nbco3 -cpu -corr` carries one sum per tau through all rows
// in index order.  THE TWO AGREE ONLY TO ROUNDING, NOT BIT FOR BIT -- the situation of rho_k in structure_factor.hpp.  Each of them
// returns the same bytes on every call; pairs is equal integer for integer everywhere.
#pragma once
#include <cmath>

#ifdef __HIP__   // (compiled as HIP; the host programs compile it as plain C++)
#define NBCO_TC_HD __host__ __device__ __forceinline__
#else
#define NBCO_TC_HD inline
#endif

constexpr int kTcMaxFrames = 2048;   // the longest series a call takes

// the seven sums of one lag
struct TcSum { double dx2[3], r4, vv[3]; };

NBCO_TC_HD void tc_zero(TcSum &s)
{
	s.dx2[0] = s.dx2[1] = s.dx2[2] = s.r4 = s.vv[0] = s.vv[1] = s.vv[2] = 0.0;
}

NBCO_TC_HD bool tc_finite(const float *f)
{
	return std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && std::isfinite(f[3]) && std::isfinite(f[4]) && std::isfinite(f[5]);
}

// one term: the widened frame t (x0, v0) and frame t + tau (x1, v1), both finite
NBCO_TC_HD void tc_term(TcSum &s, double x0x, double x0y, double x0z, double v0x, double v0y, double v0z,
                        double x1x, double x1y, double x1z, double v1x, double v1y, double v1z)
{
	const double dx = x1x - x0x;
	const double dy = x1y - x0y;
	const double dz = x1z - x0z;
	s.dx2[0] = fma(dx, dx, s.dx2[0]);
	s.dx2[1] = fma(dy, dy, s.dx2[1]);
	s.dx2[2] = fma(dz, dz, s.dx2[2]);
	const double sx = dx * dx;
	const double sxy = fma(dy, dy, sx);
	const double r2 = fma(dz, dz, sxy);
	s.r4 = fma(r2, r2, s.r4);
	s.vv[0] = fma(v0x, v1x, s.vv[0]);
	s.vv[1] = fma(v0y, v1y, s.vv[1]);
	s.vv[2] = fma(v0z, v1z, s.vv[2]);
}

// msd_x msd_y msd_z msd alpha2 vacf_x vacf_y vacf_z of one lag from its raw sums: eight doubles.  pairs == 0 gives eight zeros;
// msd == 0 (lag 0, particles at rest) gives alpha2 = 0: never NaN or infinity from an empty or a frozen lag.
inline void tc_derive(const double *dx2, double r4, const double *vv, unsigned long long pairs, double *o)
{
	for (int j = 0; j < 8; ++j) o[j] = 0.0;
	if (pairs == 0) return;
	const double m = (double)pairs;
	o[0] = dx2[0] / m; o[1] = dx2[1] / m; o[2] = dx2[2] / m;
	o[3] = (o[0] + o[1]) + o[2];
	if (o[3] != 0.0) o[4] = 3.0 * (r4 / m) / (5.0 * (o[3] * o[3])) - 1.0;
	o[5] = vv[0] / m; o[6] = vv[1] / m; o[7] = vv[2] / m;
}
