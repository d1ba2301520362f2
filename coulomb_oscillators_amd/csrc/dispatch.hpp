// dispatch.hpp -- the switches that turn a run-time choice into a template argument: the expansion order, the element type of the
// far-field tuples, the output set of a probe call, the variant of the pass between two leapfrog steps, the template step of a run-time length.  A launch function calls them around its hipLaunchKernelGGL: the only place
// where that kernel's variant is chosen.  Nothing here needs rocPRIM, so the kernel translation units include it directly.
#pragma once
#include "nbco_internal.hpp"
#include <type_traits>
#include <utility>

// f(std::integral_constant<int, P>) for a run-time order 1 <= P <= PMAX; false (and no call) for any other order: the caller
// reports the refusal in its own words
template <int PMAX = kMaxOrder, class F>
static bool with_order(int P, F &&f)
{
	static_assert(PMAX <= 10 && kMaxOrder == 10, "the case list below ends at order 10");
#define NBCO_ORDER_CASE(PP) \
	case PP: \
		if constexpr (PP <= PMAX) { f(std::integral_constant<int, PP>{}); return true; } \
		return false;
	switch (P)
	{
	NBCO_ORDER_CASE(1) NBCO_ORDER_CASE(2) NBCO_ORDER_CASE(3) NBCO_ORDER_CASE(4) NBCO_ORDER_CASE(5)
	NBCO_ORDER_CASE(6) NBCO_ORDER_CASE(7) NBCO_ORDER_CASE(8) NBCO_ORDER_CASE(9) NBCO_ORDER_CASE(10)
	default: return false;
	}
#undef NBCO_ORDER_CASE
}

// f(T{}) with T = double for far-field tuples of doubles (f64: a flag, or real_bytes == 8 of a tree) and T = float otherwise
template <class F>
static void with_real(bool f64, F &&f)
{
	if (f64) f(double{});
	else f(float{});
}

// f(std::bool_constant<WANT_A>, std::bool_constant<WANT_PSI>) for the outputs of a probe call that are given (not both are NULL): an
// output that is NULL costs nothing, because the kernels are compiled per output set
template <class F>
static void with_outputs(const double *a, const double *psi, F &&f)
{
	if (a && psi) f(std::true_type{}, std::true_type{});
	else if (a) f(std::true_type{}, std::false_type{});
	else f(std::false_type{}, std::true_type{});
}

// f(std::bool_constant<ON>) for a run-time flag
template <class F>
static void with_flag(bool on, F &&f)
{
	if (on) f(std::true_type{});
	else f(std::false_type{});
}

// f(std::integral_constant<int, A>) for the first of the ascending template steps A, .. that is at least v (the last one for a v
// beyond them all); last_step is that last one
template <int A, int... REST, class F>
static void with_step(std::integer_sequence<int, A, REST...>, int v, F &&f)
{
	if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, A>{});
	else if (v <= A) f(std::integral_constant<int, A>{});
	else with_step(std::integer_sequence<int, REST...>{}, v, f);
}
template <int... A>
constexpr int last_step(std::integer_sequence<int, A...>) { return (A, ...); }

// f(drift) for the drift of a leapfrog step: the matrices of the helix drift (Helix3) where a magnetic field is given, the step length (float) otherwise
template <class H, class F>
static void with_drift(float ds, const H *helix, F &&f)
{
	if (helix) f(*helix);
	else f(ds);
}

// f(bath...) with the pack empty (no bath: the kernel has no such argument) or the one Bath3
template <class B, class F>
static void with_bath(const B *bath, F &&f)
{
	if (bath) f(*bath);
	else f();
}
