// integ_compose.hpp -- the five symplectic compositions of the reference (integrator.cuh:32-167), once for the 3-D and the 2-D
// library and the host programs' CPU path: which kick, drift and force evaluation follow each other, and with which coefficients.
// Needs the ABI header alone, so that a host compiler without HIP can include it.
#pragma once
#include "../../include/nbco.h"

#define INTEG_TRY(call)                  \
	do {                                 \
		int rc_ = (call);                \
		if (rc_ != NBCO_OK) return rc_;  \
	} while (0)

// One step of `scheme` over K(s): v += a s, D(s): x += v s and F(): a = f(x), each returning a status; the first that fails ends the
// step.  The coefficients are formed in long double and handed to K and D as such: narrowing them to the state's type is theirs, as
// it is the reference's at its step_func call sites.  The caller has checked the scheme.
template <class Kick, class Drift, class Force>
static int integ_compose(int scheme, long double dt, long double scale, Kick &&K, Drift &&D, Force &&F)
{
	const long double th = 1.3512071919596576340476878089715L;   // integrator.cuh:98
	const long double xi = +0.1786178958448091E+00L, la = -0.2123418310626054E+00L, ch = -0.6626458266981849E-01L;  // :130-132
	switch (scheme)
	{
	case NBCO_INTEG_EULER:        // integrator.cuh:32
		INTEG_TRY(K(dt * scale)); INTEG_TRY(D(dt)); INTEG_TRY(F());
		return NBCO_OK;
	case NBCO_INTEG_PRE_EULER:    // :50
		INTEG_TRY(F()); INTEG_TRY(K(dt * scale)); INTEG_TRY(D(dt));
		return NBCO_OK;
	case NBCO_INTEG_LEAPFROG:     // :68
	{
		const long double ds = dt * scale * 0.5L;
		INTEG_TRY(K(ds)); INTEG_TRY(D(dt)); INTEG_TRY(F()); INTEG_TRY(K(ds));
		return NBCO_OK;
	}
	case NBCO_INTEG_FORESTRUTH:   // :100
	{
		const long double ds = dt * scale;
		INTEG_TRY(D(dt * th / 2)); INTEG_TRY(F());
		INTEG_TRY(K(ds * th)); INTEG_TRY(D(dt * (1 - th) / 2)); INTEG_TRY(F());
		INTEG_TRY(K(ds * (1 - 2 * th))); INTEG_TRY(D(dt * (1 - th) / 2)); INTEG_TRY(F());
		INTEG_TRY(K(ds * th)); INTEG_TRY(D(dt * th / 2));
		return NBCO_OK;
	}
	case NBCO_INTEG_PEFRL:        // :134
	{
		const long double ds = dt * scale;
		INTEG_TRY(D(dt * xi)); INTEG_TRY(F());
		INTEG_TRY(K(ds * (1 - 2 * la) / 2)); INTEG_TRY(D(dt * ch)); INTEG_TRY(F());
		INTEG_TRY(K(ds * la)); INTEG_TRY(D(dt * (1 - 2 * (ch + xi)))); INTEG_TRY(F());
		INTEG_TRY(K(ds * la)); INTEG_TRY(D(dt * ch)); INTEG_TRY(F());
		INTEG_TRY(K(ds * (1 - 2 * la) / 2)); INTEG_TRY(D(dt * xi));
		return NBCO_OK;
	}
	default: return NBCO_ERR_ARG;
	}
}

#undef INTEG_TRY
