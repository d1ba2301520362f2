// host_util.hpp -- host idioms of the translation units that call rocPRIM (the tree evaluators and the re-partition): the size
// query / scratch growth / call triple, written once; the grid size of a 1-D launch; the switch that turns a run-time expansion
// order into a template argument.  The rocPRIM helpers enqueue on c->stream and grow the scratch buffer they are GIVEN: which
// buffer that is stays the caller's choice, because two streams must never share a scratch (sort_tmp on the main stream,
// scan_tmp_aux on the auxiliary one, f2d_tmp in the 2-D path).
#pragma once
#include "nbco_internal.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <type_traits>

// f(std::integral_constant<int, P>) for a run-time order 1 <= P <= PMAX; false (and no call) for any other order.  A launch
// function calls this once, around its hipLaunchKernelGGL: the only place where the order of that kernel is chosen.
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

// f(std::bool_constant<WANT_A>, std::bool_constant<WANT_PSI>) for the outputs of a probe call that are given (not both are NULL): an
// output that is NULL costs nothing, because the kernels are compiled per output set
template <class F>
static void with_outputs(const double *a, const double *psi, F &&f)
{
	if (a && psi) f(std::true_type{}, std::true_type{});
	else if (a) f(std::true_type{}, std::false_type{});
	else f(std::false_type{}, std::true_type{});
}

// blocks of `block` threads that cover n items, at most cap.  No lower bound: 0 for n <= 0.
static inline int grid_blocks(long long n, int block, long long cap) { return (int)std::min<long long>((n + block - 1) / block, cap); }

// call(temp, bytes) is one rocPRIM call: asked for its scratch size, then run in tmp, grown to that size (and to min_bytes, for a
// caller that keeps something else in the same buffer)
template <class Call>
static int prim_run(nbco_ctx *c, DevBuf &tmp, size_t min_bytes, Call call)
{
	size_t bytes = 0;
	NBCO_HIP(call(nullptr, bytes));
	NBCO_TRY(c->reserve(tmp, std::max(bytes, min_bytes)));
	bytes = tmp.bytes;
	NBCO_HIP(call(tmp.ptr, bytes));
	return NBCO_OK;
}

// stable radix sort of (key, value) pairs over the key bits [begin_bit, end_bit)
template <class KeyIn, class KeyOut, class ValIn, class ValOut>
static int sort_pairs(nbco_ctx *c, DevBuf &tmp, KeyIn kin, KeyOut kout, ValIn vin, ValOut vout, long long n, unsigned begin_bit, unsigned end_bit,
                      size_t min_bytes = 0)
{
	return prim_run(c, tmp, min_bytes, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, (size_t)n, begin_bit, end_bit, c->stream); });
}

template <class KeyIn, class KeyOut>
static int sort_keys(nbco_ctx *c, DevBuf &tmp, KeyIn kin, KeyOut kout, long long n, unsigned begin_bit, unsigned end_bit)
{
	return prim_run(c, tmp, 0, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, kin, kout, (size_t)n, begin_bit, end_bit, c->stream); });
}

// out[i] = init + in[0] + .. + in[i - 1], summed in Init.  The iterators may be fancy ones: the kd-tree lists scan a packed pair of
// counts through a transform iterator into an output iterator that splits the sums again (k_fmm_kd.hip).
template <class In, class Out, class Init>
static int exclusive_scan(nbco_ctx *c, DevBuf &tmp, In in, Out out, Init init, size_t count)
{
	return prim_run(c, tmp, 0, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, init, count, rocprim::plus<Init>(), c->stream); });
}
