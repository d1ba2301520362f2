// host_util.hpp -- host idioms of the translation units that call rocPRIM (the tree evaluators and the re-partition): the size
// query / scratch growth / call triple, written once; the grid size of a 1-D launch; and, through dispatch.hpp, the switches
// that turn a run-time choice into a template argument.  The rocPRIM helpers enqueue on c->stream and grow the scratch buffer
// they are GIVEN: which buffer that is stays the caller's choice, because two streams must never share a scratch (sort_tmp on
// the main stream, scan_tmp_aux on the auxiliary one, f2d_tmp in the 2-D path).
#pragma once
#include "nbco_internal.hpp"
#include "dispatch.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>

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
