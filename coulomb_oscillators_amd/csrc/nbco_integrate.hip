// nbco_integrate.hip -- the 3-D symplectic integrators of include/nbco.h (integrator.cuh:32-167) with their uniform magnetic field and
// Langevin bath: the matrices and coefficients of the two, and ONE driver behind nbco_integrate, nbco_integrate_steps and their _b and
// _t forms -- one rule (StepRule), one check, one step, one run of steps.
#include "nbco_internal.hpp"
#include "integ_compose.hpp"
#include "helix.hpp"
#include "bath.hpp"
#include <chrono>
#include <cmath>

// ---- Langevin bath: coefficients of the exact Ornstein-Uhlenbeck step over s for the first `dim` axes (include/nbco.h; declared in
// nbco_internal.hpp: the 2-D calls of k_fmm2d.hip use them with dim = 2)
bool bath_valid(const nbco_bath *b, int dim)
{
	for (int a = 0; a < dim; ++a)
		if (!std::isfinite(b->gamma[a]) || b->gamma[a] < 0.0 || !std::isfinite(b->kT[a]) || b->kT[a] < 0.0) return false;
	return true;
}

bool bath_off(const nbco_bath *b, int dim)
{
	for (int a = 0; a < dim; ++a)
		if (b->gamma[a] != 0.0) return false;
	return true;
}

int bath_coeffs_dim(const nbco_bath *b, double s, double *c1, double *c2, int dim)
{
	if (!b || !c1 || !c2 || !bath_valid(b, dim) || !std::isfinite(s) || s < 0.0) return NBCO_ERR_ARG;
	for (int a = 0; a < dim; ++a)
	{
		const double gs = b->gamma[a] * s;
		c1[a] = std::exp(-gs);
		c2[a] = std::sqrt(b->kT[a] * (-std::expm1(-2.0 * gs)));
	}
	return NBCO_OK;
}

// ---- uniform magnetic field: the matrices of the helix drift (include/nbco.h) ---------------------------------------------------
namespace {

// sin(theta), 1 - cos(theta), (1 - cos(theta)) / w and (theta - sin(theta)) / w for theta = (w + dw) s.  theta = p + e with p the rounded
// product and e what the rounding and dw leave: at theta = 100 one ulp of theta alone is tens of ulps of the sine.
struct HelixCoef { double sn, vc, c1, c2; };
constexpr double kHelixSeries = 0.5;   // |theta| below which theta - sin(theta) is summed as a series (the difference cancels there)

HelixCoef helix_coef(double w, double dw, double s)
{
	const double p = w * s, e = std::fma(w, s, -p) + dw * s, h = 0.5 * p;
	const double sh = std::sin(h) + 0.5 * e * std::cos(h);   // sin(theta / 2)
	HelixCoef k;
	k.vc = 2.0 * sh * sh;
	k.sn = std::sin(p) + e * std::cos(p);
	double tms;
	if (std::fabs(p) < kHelixSeries)
	{
		// theta^3/3! - theta^5/5! + ..., nested; the first term left out is theta^17/17!: below 2^-60 of the sum
		const double t = p + e, t2 = t * t;
		tms = t * t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0 * (1.0 - t2 / 156.0 * (1.0 - t2 / 210.0))))));
	}
	else tms = (p - std::sin(p)) + e * k.vc;
	k.c1 = k.vc / w;
	k.c2 = tms / w;
	return k;
}

// float matrices of the 3-D device drift; false: Omega or s is not finite
bool helix3_make(const double *omega3, double s, Helix3 &h)
{
	double R[9], A[9];
	if (nbco_helix_matrices(omega3, s, R, A) != NBCO_OK) return false;
	for (int i = 0; i < 9; ++i) { h.R[i] = (float)R[i]; h.A[i] = (float)A[i]; }
	return true;
}

bool omega3_finite(const double *o) { return std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]); }

// which half step of which tick a built Bath3 stands for (the coefficients depend on the step length alone)
const Bath3 &bath3_at(Bath3 &b, int half, unsigned long long tick)
{
	b.tick[0] = (uint32_t)tick; b.tick[1] = (uint32_t)(tick >> 32);
	b.half = half;
	return b;
}

// the kernel argument of the 3-D bath step: coefficients narrowed to float once, the seed and the tick as two words each
bool bath3_make(const nbco_bath *b, double s, int half, unsigned long long tick, Bath3 &out)
{
	double c1[3], c2[3];
	if (bath_coeffs_dim(b, s, c1, c2, 3) != NBCO_OK) return false;
	for (int a = 0; a < 3; ++a) { out.c1[a] = (float)c1[a]; out.c2[a] = (float)c2[a]; }
	out.key[0] = (uint32_t)b->seed; out.key[1] = (uint32_t)(b->seed >> 32);
	bath3_at(out, half, tick);
	return true;
}

} // namespace

extern "C" {

int nbco_bath_coeffs(const nbco_bath *b, double s, double *c1, double *c2) { return bath_coeffs_dim(b, s, c1, c2, 3); }

int nbco_helix_matrices(const double *o, double s, double *R, double *A)
{
	if (!o || !R || !A || !omega3_finite(o) || !std::isfinite(s)) return NBCO_ERR_ARG;
	for (int i = 0; i < 9; ++i) { R[i] = i % 4 == 0 ? 1.0 : 0.0; A[i] = i % 4 == 0 ? s : 0.0; }
	const double m = std::fmax(std::fabs(o[0]), std::fmax(std::fabs(o[1]), std::fabs(o[2])));
	if (m == 0.0) return NBCO_OK;
	// u = Omega / 2^ex (exact), S = |u|^2 as hi + lo (two-products, two-sums), |u| = wu + dwu
	int ex;
	std::frexp(m, &ex);
	double u[3], hi = 0.0, lo = 0.0;
	for (int k = 0; k < 3; ++k)
	{
		u[k] = std::ldexp(o[k], -ex);
		const double q = u[k] * u[k], qe = std::fma(u[k], u[k], -q), t = hi + q, bb = t - hi;
		lo += ((hi - (t - bb)) + (q - bb)) + qe;
		hi = t;
	}
	const double S = hi + lo, wu = std::sqrt(S), dwu = (std::fma(-wu, wu, hi) + lo) / (2.0 * wu);
	const double w = std::ldexp(wu, ex), dw = std::ldexp(dwu, ex);
	if (!std::isfinite(w) || !std::isfinite(w * s)) return NBCO_ERR_ARG;
	const HelixCoef k = helix_coef(w, dw, s);
	const double n[3] = {u[0] / wu, u[1] / wu, u[2] / wu};
	const double N[9] = {0.0, -n[2], n[1], n[2], 0.0, -n[0], -n[1], n[0], 0.0};   // N v = n x v
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j)
		{
			const double d = i == j ? 1.0 : 0.0, n2 = u[i] * u[j] / S - d;         // N^2 = n n^T - I
			R[3 * i + j] = d - k.sn * N[3 * i + j] + k.vc * n2;
			A[3 * i + j] = s * d - k.c1 * N[3 * i + j] + k.c2 * n2;
		}
	return NBCO_OK;
}

// N = [[0, -1], [1, 0]], N^2 = -I: R = cos(theta) I - sin(theta) N, A = (sin(theta) / w) I - ((1 - cos(theta)) / w) N  (s - (theta - sin(theta)) / w
// is sin(theta) / w; taken directly, nothing cancels and no series is needed)
int nbco_2d_helix_matrices(double w, double s, double *R, double *A)
{
	if (!R || !A || !std::isfinite(w) || !std::isfinite(s) || !std::isfinite(w * s)) return NBCO_ERR_ARG;
	R[0] = R[3] = 1.0; R[1] = R[2] = 0.0;
	A[0] = A[3] = s; A[1] = A[2] = 0.0;
	if (w == 0.0) return NBCO_OK;
	const HelixCoef k = helix_coef(w, 0.0, s);
	R[0] = R[3] = 1.0 - k.vc; R[1] = k.sn; R[2] = -k.sn;
	A[0] = A[3] = k.sn / w; A[1] = k.c1; A[2] = -k.c1;
	return NBCO_OK;
}

} // extern "C"

// ---- the driver -----------------------------------------------------------------------------------------------------------------
namespace {

// What a checked call integrates with besides its scheme.  omega null: the straight drift; bath null: no bath; all null is the
// reference's scheme.  integrate_check fills h and b, once per call: nothing below builds them again for the step length dt.
struct StepRule
{
	const double *omega = nullptr;   // the uniform magnetic field whose helix drift replaces D
	const nbco_bath *bath = nullptr;   // the Langevin bath whose two half steps O(dt/2) wrap every step
	unsigned long long tick = 0;     // the bath's step number of the first step
	Helix3 h;                        // with omega: the drift over dt
	Bath3 b;                         // with bath: the half step over dt/2
	const Helix3 *helix() const { return omega ? &h : nullptr; }
	const Bath3 *half_step(int half, int step) { return bath ? &bath3_at(b, half, tick + (unsigned long long)step) : nullptr; }
};

enum { kNeedOmega = 1, kNeedBath = 2 };   // integrate_check: the _b forms must be given omega, the _t forms a bath

// What the six calls refuse before any launch, the state and the context untouched.  Omega = 0: r.omega comes back null; all gamma = 0:
// r.bath comes back null (the call is its counterpart).
int integrate_check(nbco_ctx *c, const char *who, int scheme, int kind, const float *buf, long long n, const float *param, double dt, int steps, int need,
                    StepRule &r)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!buf || !param || n <= 0 || steps < 0) return c->fail(NBCO_ERR_ARG, w + ": bad arguments");
	if ((need & kNeedBath) && !r.bath) return c->fail(NBCO_ERR_ARG, w + ": bath_host is NULL");
	if (r.bath && !bath_valid(r.bath, 3)) return c->fail(NBCO_ERR_ARG, w + ": gamma and kT must be finite and not negative");
	if ((need & kNeedOmega) && !r.omega) return c->fail(NBCO_ERR_ARG, w + ": omega3_host is NULL");
	if (r.omega && !omega3_finite(r.omega)) return c->fail(NBCO_ERR_ARG, w + ": Omega must be finite");
	if (scheme < NBCO_INTEG_EULER || scheme > NBCO_INTEG_PEFRL) return c->fail(NBCO_ERR_ARG, w + ": unknown integrator scheme");
	if (kind < NBCO_EVAL_DIRECT || kind > NBCO_EVAL_FMM_SYMMETRIC) return c->fail(NBCO_ERR_ARG, w + ": unknown evaluator kind");
	if (kind == NBCO_EVAL_FMM_KDTREE && n > 0x7fffffffLL / 4) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit tree indices");
	if (r.omega && r.omega[0] == 0.0 && r.omega[1] == 0.0 && r.omega[2] == 0.0) r.omega = nullptr;
	if (r.omega && !helix3_make(r.omega, dt, r.h)) return c->fail(NBCO_ERR_ARG, w + ": Omega dt is not finite");
	if (r.bath && bath_off(r.bath, 3)) r.bath = nullptr;
	if (!r.bath) return NBCO_OK;
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n must be below 2^31 (the row is one counter word)");
	if (!std::isfinite(dt) || dt < 0.0) return c->fail(NBCO_ERR_ARG, w + ": dt must be finite and not negative with a bath");
	bath3_make(r.bath, 0.5 * dt, 0, r.tick, r.b);
	return NBCO_OK;
}

// O(s) on the velocities where there is a bath
int bath_step(nbco_ctx *c, float *v, const Bath3 *bath, long long n)
{
	if (!bath) return NBCO_OK;
	PhaseScope ph(c, NBCO_PH_AXPY);
	return launch_bath(c, v, *bath, n);
}

// [O(half 0)] K(ds) D(dt) at the start of a leapfrog step: the kick and the drift are one pass over x, v, a
int opening_kick_drift(nbco_ctx *c, float *buf, long long n, float ds, float dt, const Helix3 *helix, const Bath3 *bath)
{
	float *x = buf, *v = buf + 3 * n, *a = buf + 6 * n;
	PhaseScope ph(c, NBCO_PH_AXPY);
	if (bath) NBCO_TRY(launch_bath(c, v, *bath, n));
	if (helix) return launch_kick_drift_b(c, x, v, a, ds, *helix, n);
	return launch_kick_drift(c, x, v, a, ds, dt, 3 * n);
}

// F K(ds) [O(half 1)] at the end of a leapfrog step.  `run` is what comes before the kick -- the force evaluation, or the re-ordering the
// last evaluation of a fused run has left.  The elastic term and the kick share one pass over x, v, a, and when `run` has just
// re-ordered the particles, the kick reads the tree-ordered velocities straight from the scratch copy.  bath: null, or the closing half
// of the step's Langevin bath.
template <class Run>
static int closing_kick(nbco_ctx *c, KdStepLink &link, Run run, float *buf, long long n, const float *param, float ds, bool elastic, const Bath3 *bath)
{
	float *x = buf, *v = buf + 3 * n, *a = buf + 6 * n;
	link.defer_v_copy = true;
	link.v_now = nullptr;
	const int rc = run();
	const float *v_in = link.v_now ? link.v_now : v;
	if (rc != NBCO_OK)
	{
		if (v_in != v) hipMemcpyAsync(v, v_in, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream);   // leave a whole state behind
		return rc;
	}
	{
		PhaseScope ph(c, NBCO_PH_AXPY);
		NBCO_TRY(launch_finish_kick(c, x, v_in, v, a, param, ds, n, elastic));
	}
	return bath_step(c, v, bath, n);
}

// One step [O(dt/2, half 0)] S(dt) [O(dt/2, half 1)], step number `step` of the call.  S is integrator.cuh:32-167: K(s): v += a*s,
// D(s): x += v*s (or the helix drift), F: a = f(x) (+ elastic term).  The step coefficients are formed in long double and narrowed to
// float at the step call, as the reference does at its step_func call sites.
int integrate_step(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt_, double scale_, int elastic, StepRule &r,
                   int step = 0)
{
	struct HostTimer
	{
		nbco_ctx *c;
		std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
		~HostTimer() { c->host_call_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); ++c->host_calls; }
	} host_timer{c};
	float *x = buf, *v = buf + 3 * n, *a = buf + 6 * n;
	const long long n3 = 3 * n;
	const long double dt = dt_, scale = scale_;
	if (scheme == NBCO_INTEG_LEAPFROG)
	{
		const float ds = (float)(dt * scale * 0.5L);
		NBCO_TRY(opening_kick_drift(c, buf, n, ds, (float)dt, r.helix(), r.half_step(0, step)));
		KdStepLink link;
		NBCO_TRY(closing_kick(c, link, [&] { return eval_kind(c, kind, x, a, n, param, &link); }, buf, n, param, ds, elastic != 0, r.half_step(1, step)));
		return maybe_sync(c);
	}
	auto K = [&](long double s) { PhaseScope ph(c, NBCO_PH_AXPY); return launch_step(c, v, a, (float)s, n3); };
	auto D = [&](long double s) {
		PhaseScope ph(c, NBCO_PH_AXPY);
		c->drifted = true;
		if (!r.omega) return launch_step(c, x, v, (float)s, n3);
		if ((double)s == dt_) return launch_drift_b(c, x, v, r.h, n);
		Helix3 h;   // a sub-step has its own length, never longer than dt
		if (!helix3_make(r.omega, (double)s, h)) return c->fail(NBCO_ERR_ARG, "nbco_integrate_b: Omega dt is not finite");
		return launch_drift_b(c, x, v, h, n);
	};
	auto F = [&]() {
		NBCO_TRY(eval_kind(c, kind, x, a, n, param));
		if (elastic)
		{
			PhaseScope ph(c, NBCO_PH_AXPY);
			NBCO_TRY(launch_add_elastic(c, x, a, n, param + 3, false));
		}
		return (int)NBCO_OK;
	};
	NBCO_TRY(bath_step(c, v, r.half_step(0, step), n));
	NBCO_TRY(integ_compose(scheme, dt, scale, K, D, F));
	NBCO_TRY(bath_step(c, v, r.half_step(1, step), n));
	return maybe_sync(c);
}

// `steps` steps of the scheme in one call.  Leapfrog over the kd-tree evaluator (tree order kept, opts.unsort = 0) fuses what lies
// between two force evaluations -- tree order for x and v, elastic term, the two half kicks, the drift and the next build's
// prologue: four passes over the state -- into one (kd_turnaround); every particle sees the same operations with the same
// roundings as in `steps` calls of integrate_step, and the final state is bit-identical to theirs.  Everything else loops.
// With a bath, step k is at tick + k; in the fused run the half bath steps between two force evaluations are part of the turnaround pass.
int integrate_steps(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt_, double scale_, int elastic, int steps,
                    StepRule &r)
{
	const bool fuse = scheme == NBCO_INTEG_LEAPFROG && kind == NBCO_EVAL_FMM_KDTREE && !c->o.unsort && !c->o.track_order && steps >= 2;
	if (!fuse)
	{
		{
			SyncOff quiet(c);
			for (int s = 0; s < steps; ++s) NBCO_TRY(integrate_step(c, scheme, kind, buf, n, param, dt_, scale_, elastic, r, s));
		}
		return maybe_sync(c);
	}
	float *x = buf, *v = buf + 3 * n;
	const long double dt = dt_, scale = scale_;
	const float ds = (float)(dt * scale * 0.5L), dtf = (float)dt;
	NBCO_TRY(opening_kick_drift(c, buf, n, ds, dtf, r.helix(), r.half_step(0, 0)));
	KdStepLink link;
	auto home = [&]() {   // the velocities back into the caller's array
		if (link.v_now) hipMemcpyAsync(v, link.v_now, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream);
		link.v_now = nullptr;
	};
	link.defer_order = true;
	for (int s = 0; s < steps; ++s)
	{
		int rc = eval_kind(c, kind, x, buf + 6 * n, n, param, &link);
		if (rc == NBCO_OK && s + 1 < steps) rc = kd_turnaround(c, buf, param, ds, dtf, elastic != 0, n, &link, nullptr, r.helix(), r.half_step(1, s));
		if (rc != NBCO_OK)
		{
			home();
			kd_finish_pending_order(c, x, n, &link);   // leave a whole state behind
			return rc;
		}
	}
	home();
	// tail of the last step, as in integrate_step: tree order, then a -= k o x, v += a ds, and the closing half of the bath
	NBCO_TRY(closing_kick(c, link, [&] { return kd_finish_pending_order(c, x, n, &link); }, buf, n, param, ds, elastic != 0, r.half_step(1, steps - 1)));
	return maybe_sync(c);
}

} // namespace

extern "C" {

int nbco_integrate(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic)
{
	StepRule r;
	NBCO_TRY(integrate_check(c, "nbco_integrate", scheme, kind, buf, n, param, dt, 0, 0, r));
	return integrate_step(c, scheme, kind, buf, n, param, dt, scale, elastic, r);
}

int nbco_integrate_steps(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic,
                         int steps)
{
	StepRule r;
	NBCO_TRY(integrate_check(c, "nbco_integrate_steps", scheme, kind, buf, n, param, dt, steps, 0, r));
	return integrate_steps(c, scheme, kind, buf, n, param, dt, scale, elastic, steps, r);
}

// ---- uniform magnetic field (include/nbco.h) ------------------------------------------------------------------------------------
// ---- uniform magnetic field (include/nbco.h) ------------------------------------------------------------------------------------
int nbco_drift_b(nbco_ctx *c, float *x, float *v, long long n, const double *omega3_host, double s)
{
	if (!c || !x || !v || !omega3_host || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_drift_b: bad arguments") : NBCO_ERR_ARG;
	Helix3 h;
	if (!helix3_make(omega3_host, s, h)) return c->fail(NBCO_ERR_ARG, "nbco_drift_b: Omega and s must be finite");
	PhaseScope ph(c, NBCO_PH_AXPY);
	c->drifted = true;
	return launch_drift_b(c, x, v, h, n);
}

int nbco_integrate_b(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic,
                     const double *omega3_host)
{
	StepRule r{omega3_host};
	NBCO_TRY(integrate_check(c, "nbco_integrate_b", scheme, kind, buf, n, param, dt, 0, kNeedOmega, r));
	return integrate_step(c, scheme, kind, buf, n, param, dt, scale, elastic, r);
}

int nbco_integrate_steps_b(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic,
                           int steps, const double *omega3_host)
{
	StepRule r{omega3_host};
	NBCO_TRY(integrate_check(c, "nbco_integrate_steps_b", scheme, kind, buf, n, param, dt, steps, kNeedOmega, r));
	return integrate_steps(c, scheme, kind, buf, n, param, dt, scale, elastic, steps, r);
}

// ---- Langevin bath (include/nbco.h) ---------------------------------------------------------------------------------------------
int nbco_bath_apply(nbco_ctx *c, float *v, long long n, const nbco_bath *bath, double s, int half, unsigned long long tick)
{
	if (!c) return NBCO_ERR_ARG;
	if (!v || !bath || n < 0) return c->fail(NBCO_ERR_ARG, "nbco_bath_apply: bad arguments");
	if (half != 0 && half != 1) return c->fail(NBCO_ERR_ARG, "nbco_bath_apply: half must be 0 or 1");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, "nbco_bath_apply: n must be below 2^31 (the row is one counter word)");
	Bath3 b;
	if (!bath3_make(bath, s, half, tick, b)) return c->fail(NBCO_ERR_ARG, "nbco_bath_apply: gamma, kT and s must be finite and not negative");
	{
		PhaseScope ph(c, NBCO_PH_AXPY);
		NBCO_TRY(launch_bath(c, v, b, n));
	}
	return maybe_sync(c);
}

int nbco_integrate_t(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic,
                     const double *omega3_host, const nbco_bath *bath_host, unsigned long long tick)
{
	StepRule r{omega3_host, bath_host, tick};
	NBCO_TRY(integrate_check(c, "nbco_integrate_t", scheme, kind, buf, n, param, dt, 0, kNeedBath, r));
	return integrate_step(c, scheme, kind, buf, n, param, dt, scale, elastic, r);
}

int nbco_integrate_steps_t(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param, double dt, double scale, int elastic,
                           int steps, const double *omega3_host, const nbco_bath *bath_host, unsigned long long tick0)
{
	StepRule r{omega3_host, bath_host, tick0};
	NBCO_TRY(integrate_check(c, "nbco_integrate_steps_t", scheme, kind, buf, n, param, dt, steps, kNeedBath, r));
	return integrate_steps(c, scheme, kind, buf, n, param, dt, scale, elastic, steps, r);
}

} // extern "C"
