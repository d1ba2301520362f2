// nbco_api.hip -- the C ABI of include/nbco.h: context, option handling, the evaluator dispatch
// of compute_force (integrator.cuh:22-28 over main3.cu:47-69) and thin wrappers over the launchers.
// The symplectic integrators (integrator.cuh:32-167) are nbco_integrate.hip.
#include "nbco_internal.hpp"
#include "bond_order.hpp"
#include "structure_factor.hpp"
#include "time_corr.hpp"
#include "modes.hpp"
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <new>
#include <random>

int nbco_ctx::reserve(DevBuf &b, size_t bytes)
{
	nbco_ctx *c = this;
	if (bytes <= b.bytes) return NBCO_OK;
	if (b.ptr)
	{
		// earlier launches on the stream may still use the old allocation
		NBCO_HIP(hipStreamSynchronize(stream));
		NBCO_HIP(hipFree(b.ptr));
		b.ptr = nullptr;
		b.bytes = 0;
	}
	size_t want = bytes + bytes / 8 + 256;
	NBCO_HIP(hipMalloc(&b.ptr, want));
	b.bytes = want;
	if (poison) NBCO_HIP(hipMemsetAsync(b.ptr, 0x7f, want, stream));
	return NBCO_OK;
}

void nbco_ctx::phase_begin(int ph)
{
	if (!(profiling & (1u << ph))) return;
	hipEvent_t a, b;
	if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
	hipEventRecord(a, stream);
	timers[ph].pending.push_back({a, b});
}

void nbco_ctx::phase_end(int ph)
{
	if (!(profiling & (1u << ph)) || timers[ph].pending.empty()) return;
	hipEventRecord(timers[ph].pending.back().second, stream);
}

int nbco_ctx::fork_mark()
{
	if (!aux && !aux_is_main)
	{
		// high priority: its kernels are small, latency-bound links of the far-field chain and must not queue up behind
		// the thousands of workgroups of the near-field kernel running on the main stream
		int prio_lo = 0, prio_hi = 0;
		NBCO_HIP_M(this, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
		if (getenv("NBCO_AUX_PRIO") && atoi(getenv("NBCO_AUX_PRIO")) == 0) prio_hi = prio_lo;   // A/B switch (diagnostics)
		if (getenv("NBCO_AUX_SERIAL") && atoi(getenv("NBCO_AUX_SERIAL")) != 0) { aux = stream; aux_is_main = true; }   // diagnostics: one stream
		else NBCO_HIP_M(this, hipStreamCreateWithPriority(&aux, hipStreamNonBlocking, prio_hi));
		NBCO_HIP_M(this, hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
		NBCO_HIP_M(this, hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
	}
	NBCO_HIP_M(this, hipEventRecord(ev_fork, stream));
	return NBCO_OK;
}

int nbco_ctx::fork_wait()
{
	NBCO_HIP_M(this, hipStreamWaitEvent(aux, ev_fork, 0));
	aux_pending = true;
	return NBCO_OK;
}

int nbco_ctx::fork_aux()
{
	NBCO_TRY(fork_mark());
	return fork_wait();
}

int nbco_ctx::flags_begin()
{
	if (!h_flags)
	{
		NBCO_HIP_M(this, hipHostMalloc((void **)&h_flags, 64 * sizeof(int), hipHostMallocDefault));
		memset(h_flags, 0, 64 * sizeof(int));
		NBCO_HIP_M(this, hipEventCreateWithFlags(&ev_flags, hipEventDisableTiming));
	}
	return NBCO_OK;
}

// The host looks at the traversal's counts and flags once per evaluation, after everything else has been enqueued.  A blocking
// hipEventSynchronize wakes up tens of microseconds after the kernel has finished -- time the next step's launches start
// late by -- so the host polls the sequence word that traverse_finish_kernel stores last in pinned memory, and asks the
// event only now and then (a failed launch or a lost device must not leave it spinning).
int nbco_ctx::wait_flags()
{
	nbco_ctx *c = this;
	volatile int *seq = h_flags + 4;
	for (unsigned spin = 1;; ++spin)
	{
		if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == flags_seq) return NBCO_OK;
		if ((spin & 0x3FFu) == 0)
		{
			const hipError_t e = hipEventQuery(ev_flags);
			if (e == hipSuccess) { if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == flags_seq) return NBCO_OK; NBCO_HIP(hipEventSynchronize(ev_flags)); return NBCO_OK; }
			if (e != hipErrorNotReady) return fail_hip(e, "hipEventQuery(ev_flags)", __FILE__, __LINE__);
		}
#if defined(__x86_64__)
		__builtin_ia32_pause();
#endif
	}
}

int nbco_ctx::join_aux()
{
	if (!aux_pending) return NBCO_OK;
	NBCO_HIP_M(this, hipEventRecord(ev_join, aux));
	NBCO_HIP_M(this, hipStreamWaitEvent(stream, ev_join, 0));
	aux_pending = false;
	return NBCO_OK;
}

static int check_opts(nbco_ctx *c, const nbco_opts *o)
{
	if (o->fmm_order < 1 || o->fmm_order > kMaxOrder) return c->fail(NBCO_ERR_ARG, "fmm_order must be in 1..10");
	if (!(o->tree_radius > 0)) return c->fail(NBCO_ERR_ARG, "tree_radius must be positive");
	if (!(o->eps2 > 0)) return c->fail(NBCO_ERR_ARG, "eps2 must be positive");
	if (!(o->dens_inhom > 0)) return c->fail(NBCO_ERR_ARG, "dens_inhom must be positive");
	if (o->tree_L < 0 || o->tree_L > 30) return c->fail(NBCO_ERR_ARG, "tree_L must be in 0..30");
	if (o->tree_steps < 1) return c->fail(NBCO_ERR_ARG, "tree_steps must be >= 1");
	if (o->list_factor < 1) return c->fail(NBCO_ERR_ARG, "list_factor must be >= 1");
	return NBCO_OK;
}

int maybe_sync(nbco_ctx *c)
{
	if (c->o.sync) NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

// the evaluator dispatch of compute_force (nbco_force and the integrators of nbco_integrate.hip)
int eval_kind(nbco_ctx *c, int kind, float *p, float *a, long long n, const float *param, KdStepLink *link)
{
	switch (kind)
	{
	case NBCO_EVAL_DIRECT: return launch_direct(c, p, a, n, param, false);
	case NBCO_EVAL_DIRECT_KAHAN: return launch_direct(c, p, a, n, param, true);
	case NBCO_EVAL_FMM_KDTREE: return fmm_kdtree_eval(c, p, a, n, param, link);
	case NBCO_EVAL_FMM_TRACELESS: return fmm_oct_traceless_eval(c, p, a, n, param, false);
	case NBCO_EVAL_FMM_SYMMETRIC: return fmm_oct_traceless_eval(c, p, a, n, param, true);
	default: return c->fail(NBCO_ERR_ARG, "unknown evaluator kind");
	}
}

extern "C" {

int nbco_opts_default(nbco_opts *o)
{
	if (!o) return NBCO_ERR_ARG;
	o->fmm_order = 3;        // constants.cuh:42
	o->tree_radius = 1.f;    // :43
	o->eps2 = 1.e-18f;       // :39
	o->coll = 1;             // :48
	o->unsort = 1;           // :48
	o->dens_inhom = 1.f;     // :50
	o->tree_L = 0;           // :44
	o->tree_steps = 1;
	o->m2l_first = 0;
	o->sync = 1;
	o->list_factor = 48;
	o->list_grow = 1;
	o->far_fp64 = 0;
	o->p2p_mutual = 0;
	o->track_order = 0;
	o->stream = nullptr;
	return NBCO_OK;
}

int nbco_create(nbco_ctx **out, const nbco_opts *o)
{
	if (!out) return NBCO_ERR_ARG;
	*out = nullptr;
	nbco_ctx *c = new (std::nothrow) nbco_ctx();
	if (!c) return NBCO_ERR_HIP;
	nbco_opts def;
	nbco_opts_default(&def);
	c->o = o ? *o : def;
	int rc = check_opts(c, &c->o);
	if (rc != NBCO_OK) { delete c; return rc; }
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0)
	{
		// no CPU fallback: the engine is HIP-only
		fprintf(stderr, "nbco_create: no usable HIP device (%s)\n", e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
		delete c;
		return NBCO_ERR_HIP;
	}
	if (hipGetDevice(&c->device) != hipSuccess) { delete c; return NBCO_ERR_HIP; }
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
	c->stream = (hipStream_t)c->o.stream;
	c->poison = getenv("NBCO_POISON") && atoi(getenv("NBCO_POISON")) != 0;
	if (getenv("NBCO_SEL_WARM")) c->sel_warm_enabled = atoi(getenv("NBCO_SEL_WARM")) != 0;
	if (hipMalloc(&c->small.ptr, 4096) != hipSuccess) { delete c; return NBCO_ERR_HIP; }
	c->small.bytes = 4096;
	// (the counters, totals and flags of many calls live here: none of them may rely on a zero that it has not written)
	if (c->poison && hipMemsetAsync(c->small.ptr, 0x7f, 4096, c->stream) != hipSuccess) { delete c; return NBCO_ERR_HIP; }
	*out = c;
	return NBCO_OK;
}

int nbco_destroy(nbco_ctx *c)
{
	if (c && getenv("NBCO_HOST_TIMING") && c->host_calls)
		fprintf(stderr, "[nbco] nbco_integrate: %lld calls, %.1f us host time per call, of which %.1f us waiting for the traversal flags\n", c->host_calls,
		        1e6 * c->host_call_s / c->host_calls, 1e6 * c->host_wait_s / c->host_calls);
	if (!c) return NBCO_OK;
	if (c->energy_child) { nbco_destroy(c->energy_child); c->energy_child = nullptr; }
	hipStreamSynchronize(c->stream);
	if (c->aux && !c->aux_is_main) { hipStreamSynchronize(c->aux); hipStreamDestroy(c->aux); }
	if (c->ev_fork) hipEventDestroy(c->ev_fork);
	if (c->ev_join) hipEventDestroy(c->ev_join);
	if (c->ev_flags) hipEventDestroy(c->ev_flags);
	if (c->h_flags) hipHostFree(c->h_flags);
	for (auto &t : c->timers)
		for (auto &ev : t.pending) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
	delete c;   // frees every buffer the context owns (DevBuf), behind the drained streams
	return NBCO_OK;
}

int nbco_set_opts(nbco_ctx *c, const nbco_opts *o)
{
	if (!c || !o) return NBCO_ERR_ARG;
	NBCO_TRY(check_opts(c, o));
	if ((hipStream_t)o->stream != c->stream) NBCO_HIP(hipStreamSynchronize(c->stream));
	if (o->list_factor != c->o.list_factor) c->list_growth = 1;
	bool topo = o->fmm_order != c->o.fmm_order || o->dens_inhom != c->o.dens_inhom || o->tree_L != c->o.tree_L
	            || o->unsort != c->o.unsort || o->p2p_mutual != c->o.p2p_mutual || o->track_order != c->o.track_order
	            || o->tree_steps != c->o.tree_steps;   // (a new rebuild schedule starts with a rebuild)
	c->o = *o;
	c->stream = (hipStream_t)o->stream;
	if (topo) { c->tree_valid = false; c->eval_counter = 0; }
	if (!o->track_order) c->order_n = -1;
	return NBCO_OK;
}

int nbco_get_opts(const nbco_ctx *c, nbco_opts *o)
{
	if (!c || !o) return NBCO_ERR_ARG;
	*o = c->o;
	return NBCO_OK;
}

const char *nbco_last_error(const nbco_ctx *c) { return c ? c->err.c_str() : "null context"; }

int nbco_sync(nbco_ctx *c)
{
	if (!c) return NBCO_ERR_ARG;
	NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

// ---- basic kernels -----------------------------------------------------------------------------
int nbco_step(nbco_ctx *c, float *b, const float *a, float ds, long long n)
{
	if (!c || !b || !a || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_step: bad arguments") : NBCO_ERR_ARG;
	PhaseScope ph(c, NBCO_PH_AXPY);
	return launch_step(c, b, a, ds, 3 * n);
}
int nbco_add_elastic(nbco_ctx *c, const float *p, float *a, long long n, const float *k)
{
	if (!c || !p || !a || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_add_elastic: bad arguments") : NBCO_ERR_ARG;
	PhaseScope ph(c, NBCO_PH_AXPY);
	return launch_add_elastic(c, p, a, n, k, false);
}
int nbco_elastic(nbco_ctx *c, const float *p, float *a, long long n, const float *k)
{
	if (!c || !p || !a || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_elastic: bad arguments") : NBCO_ERR_ARG;
	PhaseScope ph(c, NBCO_PH_AXPY);
	return launch_add_elastic(c, p, a, n, k, true);
}
int nbco_rescale(nbco_ctx *c, float *a, long long n, const float *param)
{
	if (!c || !a || !param || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_rescale: bad arguments") : NBCO_ERR_ARG;
	PhaseScope ph(c, NBCO_PH_AXPY);
	return launch_rescale(c, a, 3 * n, param);
}
int nbco_gather(nbco_ctx *c, float *dst, const float *src, const int *map, long long n)
{
	if (!c || !dst || !src || !map || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_gather: bad arguments") : NBCO_ERR_ARG;
	return launch_gather3(c, dst, src, map, n, false);
}
int nbco_gather_inverse(nbco_ctx *c, float *dst, const float *src, const int *map, long long n)
{
	if (!c || !dst || !src || !map || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_gather_inverse: bad arguments") : NBCO_ERR_ARG;
	return launch_gather3(c, dst, src, map, n, true);
}
int nbco_copy(nbco_ctx *c, float *dst, const float *src, long long n)
{
	if (!c || !dst || !src || n < 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_copy: bad arguments") : NBCO_ERR_ARG;
	return launch_copy(c, dst, src, 3 * n);
}

// ---- evaluators --------------------------------------------------------------------------------
int nbco_direct(nbco_ctx *c, const float *p, float *a, long long n, const float *param)
{
	if (!c || !p || !a) return c ? c->fail(NBCO_ERR_ARG, "nbco_direct: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(launch_direct(c, p, a, n, param, false));
	return maybe_sync(c);
}
int nbco_direct3(nbco_ctx *c, const float *p, float *a, long long n, const float *param)
{
	if (!c || !p || !a) return c ? c->fail(NBCO_ERR_ARG, "nbco_direct3: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(launch_direct(c, p, a, n, param, true));
	return maybe_sync(c);
}
int nbco_fmm_kdtree(nbco_ctx *c, float *p, float *a, long long n, const float *param)
{
	if (!c || !p || !a) return c ? c->fail(NBCO_ERR_ARG, "nbco_fmm_kdtree: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(fmm_kdtree_eval(c, p, a, n, param));
	return maybe_sync(c);
}
int nbco_fmm_traceless(nbco_ctx *c, float *p, float *a, long long n, const float *param)
{
	if (!c || !p || !a) return c ? c->fail(NBCO_ERR_ARG, "nbco_fmm_traceless: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(fmm_oct_traceless_eval(c, p, a, n, param));
	return maybe_sync(c);
}
int nbco_fmm_symmetric(nbco_ctx *c, float *p, float *a, long long n, const float *param)
{
	if (!c || !p || !a) return c ? c->fail(NBCO_ERR_ARG, "nbco_fmm_symmetric: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(fmm_oct_traceless_eval(c, p, a, n, param, true));
	return maybe_sync(c);
}
int nbco_oct_get_info(nbco_ctx *c, nbco_oct_info *out)
{
	if (!c || !out) return c ? c->fail(NBCO_ERR_ARG, "nbco_oct_get_info: null pointer") : NBCO_ERR_ARG;
	if (!c->oct.valid) return c->fail(NBCO_ERR_ARG, "nbco_oct_get_info: no octree evaluation has run");
	const OctTreeDev &o = c->oct;
	out->L = o.L; out->ntot = o.ntot; out->order = o.order; out->tpl = o.tpl; out->n = o.n;
	out->m2l_entries = o.m2l_entries; out->p2p_groups = o.p2p_groups; out->p2p_desc = o.p2p_desc; out->p2p_chunks = o.p2p_chunks;
	out->real_bytes = o.real_bytes;
	out->mpole_reals = o.mpole_reals;
	return NBCO_OK;
}
int nbco_oct_copy(nbco_ctx *c, int which, void *host_dst, long long host_bytes)
{
	if (!c || !host_dst) return c ? c->fail(NBCO_ERR_ARG, "nbco_oct_copy: null pointer") : NBCO_ERR_ARG;
	return oct_copy_out(c, which, host_dst, host_bytes);
}

int nbco_dist_layout_query(nbco_ctx *c, long long n_global, int world, int rank, nbco_dist_layout *out)
{
	if (!c || !out) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_layout_query: null pointer") : NBCO_ERR_ARG;
	return kd_dist_layout(c, n_global, world, rank, out);
}
int nbco_dist_partition(nbco_ctx *c, const float *state_all, long long n_global, int world, int rank, float *state_local)
{
	if (!c || !state_all || !state_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_partition: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_partition(c, state_all, n_global, world, rank, state_local));
	return maybe_sync(c);
}
int nbco_dist_local(nbco_ctx *c, float *buf_local, long long n_local, void *nodes_send, void *pos_send)
{
	if (!c || !buf_local || !nodes_send || !pos_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_local: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_build(c, buf_local, n_local, pos_send, nullptr, false));
	NBCO_TRY(kd_dist_local_upward(c, n_local, nodes_send, nullptr, false));
	return maybe_sync(c);
}
int nbco_dist_local_build(nbco_ctx *c, float *buf_local, long long n_local, void *pos_send)
{
	if (!c || !buf_local || !pos_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_local_build: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_build(c, buf_local, n_local, pos_send, nullptr, false));
	return maybe_sync(c);
}
int nbco_dist_local_upward(nbco_ctx *c, float *buf_local, long long n_local, void *nodes_send)
{
	if (!c || !buf_local || !nodes_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_local_upward: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_upward(c, n_local, nodes_send, nullptr, false));
	return maybe_sync(c);
}
int nbco_dist_local_geom(nbco_ctx *c, float *buf_local, long long n_local, void *pos_send, void *csz_send)
{
	if (!c || !buf_local || !pos_send || !csz_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_local_geom: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_build(c, buf_local, n_local, pos_send, csz_send, false));
	return maybe_sync(c);
}
int nbco_dist_local_mpole(nbco_ctx *c, float *buf_local, long long n_local, void *mpole_send)
{
	if (!c || !buf_local || !mpole_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_local_mpole: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_upward(c, n_local, nullptr, mpole_send, false));
	return maybe_sync(c);
}
int nbco_dist_let_local_geom(nbco_ctx *c, float *buf_local, long long n_local, void *csz_send)
{
	if (!c || !buf_local || !csz_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_local_geom: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_local_build(c, buf_local, n_local, nullptr, csz_send, true));
	return maybe_sync(c);
}
int nbco_dist_let_local_mpole(nbco_ctx *c, float *buf_local, long long n_local)
{
	if (!c || !buf_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_local_mpole: null pointer") : NBCO_ERR_ARG;
	return kd_dist_local_upward(c, n_local, nullptr, nullptr, true);
}
int nbco_dist_let_select(nbco_ctx *c, const void *csz_all, long long *counts_send)
{
	if (!c || !csz_all || !counts_send) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_select: null pointer") : NBCO_ERR_ARG;
	return kd_dist_let_select(c, csz_all, counts_send);
}
int nbco_dist_let_pack(nbco_ctx *c, const long long *counts_all, void *pos_send, void *mpole_send)
{
	if (!c || !counts_all) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_pack: null pointer") : NBCO_ERR_ARG;
	return kd_dist_let_pack(c, counts_all, pos_send, mpole_send);
}
int nbco_dist_let_finish(nbco_ctx *c, const long long *counts_all, const void *pos_recv, const void *mpole_recv, float *buf_local, float *a_local,
                         const float *param)
{
	if (!c || !counts_all || !buf_local || !a_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_finish: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_let_finish(c, counts_all, pos_recv, mpole_recv, buf_local, a_local, param));
	return maybe_sync(c);
}
int nbco_dist_turnaround(nbco_ctx *c, float *buf_local, long long n_local, const float *param, double dt_, double scale_, int elastic)
{
	if (!c || !buf_local || !param) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_turnaround: null pointer") : NBCO_ERR_ARG;
	const long double dt = dt_, scale = scale_;
	return kd_dist_turnaround(c, buf_local, n_local, param, (float)(dt * scale * 0.5L), (float)dt, elastic != 0);
}
int nbco_dist_let_check(nbco_ctx *c)
{
	if (!c) return NBCO_ERR_ARG;
	return kd_dist_let_check(c);
}
int nbco_dist_let_pack_capped(nbco_ctx *c, const long long *caps_out, void *pos_send, void *mpole_send)
{
	if (!c || !caps_out) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_pack_capped: null pointer") : NBCO_ERR_ARG;
	return kd_dist_let_pack_capped(c, caps_out, pos_send, mpole_send);
}
int nbco_dist_let_finish_capped(nbco_ctx *c, const long long *caps_in, const void *pos_recv, const void *mpole_recv, float *buf_local, float *a_local,
                                const float *param)
{
	if (!c || !caps_in || !buf_local || !a_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_let_finish_capped: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_let_finish_capped(c, caps_in, pos_recv, mpole_recv, buf_local, a_local, param));
	return maybe_sync(c);
}
int nbco_dist_let_settle(nbco_ctx *c, int ok)
{
	if (!c) return NBCO_ERR_ARG;
	return kd_dist_let_settle(c, ok);
}
int nbco_dist_repartition_workspace(nbco_ctx *c, long long n_global, int world, long long *bytes)
{
	if (!c || !bytes) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_repartition_workspace: null pointer") : NBCO_ERR_ARG;
	return dpart_workspace(c, n_global, world, bytes);
}
int nbco_dist_repartition_begin(nbco_ctx *c, float *state_local, long long n_global, int world, int rank, void *work, long long work_bytes, nbco_dist_step *next)
{
	if (!c || !state_local || !work || !next) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_repartition_begin: null pointer") : NBCO_ERR_ARG;
	return dpart_begin(c, state_local, n_global, world, rank, work, work_bytes, next);
}
int nbco_dist_repartition_next(nbco_ctx *c, nbco_dist_step *next)
{
	if (!c || !next) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_repartition_next: null pointer") : NBCO_ERR_ARG;
	return dpart_next(c, next);
}
int nbco_dist_finish_traverse(nbco_ctx *c, const void *csz_all, const void *pos_all)
{
	if (!c || !csz_all || !pos_all) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_finish_traverse: null pointer") : NBCO_ERR_ARG;
	return kd_dist_finish_traverse(c, csz_all, pos_all);   // (never syncs: its point is to leave the stream busy)
}
int nbco_dist_finish_rest(nbco_ctx *c, const void *mpole_all, float *buf_local, float *a_local, const float *param)
{
	if (!c || !mpole_all || !buf_local || !a_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_finish_rest: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_finish_rest(c, mpole_all, buf_local, a_local, param));
	return maybe_sync(c);
}
int nbco_aux_stream(nbco_ctx *c, void **stream_out)
{
	if (!c || !stream_out) return c ? c->fail(NBCO_ERR_ARG, "nbco_aux_stream: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(c->fork_mark());   // creates the stream on first use (the event it records is harmless)
	*stream_out = (void *)c->aux;
	return NBCO_OK;
}
int nbco_dist_finish(nbco_ctx *c, const void *nodes_all, const void *pos_all, float *buf_local, float *a_local, const float *param)
{
	if (!c || !nodes_all || !pos_all || !buf_local || !a_local) return c ? c->fail(NBCO_ERR_ARG, "nbco_dist_finish: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(kd_dist_finish(c, nodes_all, pos_all, buf_local, a_local, param));
	return maybe_sync(c);
}

// the uniform-octree evaluators on `world` GPUs: every rank holds the whole state and builds the whole tree, and evaluates the
// accelerations of its slab of the cell order only (k_fmm_oct.hip, oct_slab_kernel)
int nbco_fmm_oct_shard(nbco_ctx *c, float *p, float *a, long long n, const float *param, int symmetric, int world, int rank, long long *bounds_host)
{
	if (!c || !p || !a || !bounds_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_fmm_oct_shard: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(fmm_oct_traceless_eval(c, p, a, n, param, symmetric != 0, world, rank, bounds_host));
	return maybe_sync(c);
}

int nbco_force(nbco_ctx *c, int kind, float *buf, long long n, const float *param, int elastic)
{
	if (!c || !buf || !param || n <= 0) return c ? c->fail(NBCO_ERR_ARG, "nbco_force: bad arguments") : NBCO_ERR_ARG;
	float *x = buf, *a = buf + 6 * n;
	NBCO_TRY(eval_kind(c, kind, x, a, n, param));
	if (elastic)
	{
		PhaseScope ph(c, NBCO_PH_AXPY);
		NBCO_TRY(launch_add_elastic(c, x, a, n, param + 3, false));
	}
	return maybe_sync(c);
}

// ---- reductions --------------------------------------------------------------------------------
int nbco_minmax(nbco_ctx *c, const float *p, long long n, float *minmax6_dev)
{
	if (!c || !p || !minmax6_dev) return c ? c->fail(NBCO_ERR_ARG, "nbco_minmax: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(launch_minmax(c, p, n, minmax6_dev));
	return maybe_sync(c);
}
int nbco_mean_relerr(nbco_ctx *c, const float *x, const float *ref, long long n, float *out_host)
{
	if (!c || !x || !ref || !out_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_mean_relerr: null pointer") : NBCO_ERR_ARG;
	return launch_mean_relerr(c, x, ref, n, out_host);
}
int nbco_pow_sum(nbco_ctx *c, const float *x, int expo, long long n, double *out3_host)
{
	if (!c || !x || !out3_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_pow_sum: null pointer") : NBCO_ERR_ARG;
	return launch_pow_sum(c, x, expo, n, out3_host);
}
int nbco_energy(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host)
{
	if (!c || !buf || !param || !out3_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_energy: null pointer") : NBCO_ERR_ARG;
	return launch_energy(c, buf, n, param, out3_host);
}

// ---- beam diagnostics (k_reduce.hip) -------------------------------------------------------------
int nbco_beam_moments(nbco_ctx *c, const float *buf, long long n, nbco_moments *out_host)
{
	if (!c || !buf || !out_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_beam_moments: null pointer") : NBCO_ERR_ARG;
	return launch_beam_moments(c, buf, 3, n, out_host);
}
int nbco_2d_beam_moments(nbco_ctx *c, const double *buf, long long n, nbco_moments *out_host)
{
	if (!c || !buf || !out_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_2d_beam_moments: null pointer") : NBCO_ERR_ARG;
	return launch_beam_moments(c, buf, 2, n, out_host);
}
// emit, halo_q, halo from cov and m4 (host only).  Zero conventions: halo_q = 0 where <d^2> = 0; emit = halo = 0 where I2 <= 0
int nbco_moments_derive(nbco_moments *m)
{
	if (!m || (m->dim != 2 && m->dim != 3)) return NBCO_ERR_ARG;
	const int D = m->dim;
	for (int k = 0; k < 3; ++k) m->emit[k] = m->halo_q[k] = m->halo[k] = 0.0;
	for (int k = 0; k < D; ++k)
	{
		const double x2 = m->cov[k][k], e2 = m->cov[D + k][D + k], xe = m->cov[k][D + k], *f = m->m4[k];
		const double i2 = x2 * e2 - xe * xe;
		const double i4 = f[0] * f[4] + 3.0 * f[2] * f[2] - 4.0 * f[3] * f[1];
		if (x2 > 0.0) m->halo_q[k] = f[0] / (x2 * x2) - 2.0;
		if (i2 > 0.0)
		{
			m->emit[k] = std::sqrt(i2);
			m->halo[k] = std::sqrt(3.0 * std::fmax(i4, 0.0)) / (2.0 * i2) - 2.0;
		}
	}
	return NBCO_OK;
}
int nbco_hist(nbco_ctx *c, const float *buf, long long n, const nbco_hist_axis *axes_host, int naxes, unsigned long long *counts_dev)
{
	if (!c || !buf || !axes_host || !counts_dev) return c ? c->fail(NBCO_ERR_ARG, "nbco_hist: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(launch_hist(c, buf, 3, n, axes_host, naxes, counts_dev));
	return maybe_sync(c);
}
int nbco_2d_hist(nbco_ctx *c, const double *buf, long long n, const nbco_hist_axis *axes_host, int naxes, unsigned long long *counts_dev)
{
	if (!c || !buf || !axes_host || !counts_dev) return c ? c->fail(NBCO_ERR_ARG, "nbco_2d_hist: null pointer") : NBCO_ERR_ARG;
	NBCO_TRY(launch_hist(c, buf, 2, n, axes_host, naxes, counts_dev));
	return maybe_sync(c);
}
int nbco_slice_moments(nbco_ctx *c, const float *buf, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host, long long *n_outside_host)
{
	if (!c || !buf || !axis_host || !out_host || !n_outside_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_slice_moments: null pointer") : NBCO_ERR_ARG;
	return launch_slice_moments(c, buf, 3, n, axis_host, out_host, n_outside_host);
}
int nbco_2d_slice_moments(nbco_ctx *c, const double *buf, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host, long long *n_outside_host)
{
	if (!c || !buf || !axis_host || !out_host || !n_outside_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_2d_slice_moments: null pointer") : NBCO_ERR_ARG;
	return launch_slice_moments(c, buf, 2, n, axis_host, out_host, n_outside_host);
}

int nbco_energy_fmm(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host)
{
	if (!c || !buf || !param || !out3_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_energy_fmm: null pointer") : NBCO_ERR_ARG;
	double ke[2], half_phi = 0;
	NBCO_TRY(launch_energy_kin_ela(c, buf, n, param, ke));
	NBCO_TRY(kd_energy_fmm(c, n, &half_phi));
	float p0;
	NBCO_HIP(hipMemcpy(&p0, param, sizeof(float), hipMemcpyDeviceToHost));
	out3_host[0] = ke[0]; out3_host[1] = ke[1]; out3_host[2] = (double)p0 * half_phi;
	return NBCO_OK;
}

// {kinetic, elastic} from buf, the Coulomb part from the potential pass over the last kd evaluation of `c`
static int energy_from_potential(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host, double *phi_dev)
{
	double ke[2], half_psi = 0;
	NBCO_TRY(launch_energy_kin_ela(c, buf, n, param, ke));
	NBCO_TRY(kd_potential(c, n, param, phi_dev, &half_psi));
	out3_host[0] = ke[0]; out3_host[1] = ke[1]; out3_host[2] = half_psi;
	return NBCO_OK;
}

int nbco_kd_potential(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host, double *phi_dev)
{
	if (!c || !buf || !param || !out3_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_kd_potential: null pointer") : NBCO_ERR_ARG;
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_kd_potential: n must be positive");
	NBCO_TRY(kd_potential_check(c, n));   // (before any launch)
	return energy_from_potential(c, buf, n, param, out3_host, phi_dev);
}

// The private context of the four *_tree calls (`who`), created on first use: everything of theirs runs on it, and this
// context's tree, lists, schedule and bookkeeping are not touched.  The child follows this context's expansion and tree options
// (re-read at every call) and always rebuilds, in the caller's particle order.
static int private_child(nbco_ctx *c, const char *who, nbco_ctx *&k)
{
	nbco_opts o = c->o;
	o.unsort = 1; o.tree_steps = 1; o.track_order = 0; o.p2p_mutual = 0; o.coll = 1; o.sync = 0;
	if (!c->energy_child)
	{
		const int rc = nbco_create(&c->energy_child, &o);
		if (rc != NBCO_OK) return c->fail(rc, std::string(who) + ": could not create the private context");
	}
	k = c->energy_child;
	const int rc = nbco_set_opts(k, &o);
	if (rc != NBCO_OK) return c->fail(rc, std::string(who) + ": " + k->err);
	return NBCO_OK;
}

// body(k, x) on that context k, with x = a scratch copy of the positions src[0 .. 3n) at the head of `floats` * n floats of room, copied
// on k's stream; what k refuses comes back as this context's error under the caller's name
extern "C++" {   // (a template inside the extern "C" block of the exports)
template <class Body>
static int on_private_copy(nbco_ctx *c, const char *who, const float *src, long long n, int floats, Body body)
{
	nbco_ctx *k;
	NBCO_TRY(private_child(c, who, k));
	auto pass = [&]() -> int {
		NBCO_TRY(k->reserve(k->pot_xa, sizeof(float) * floats * (size_t)n));
		float *x = k->pot_xa.as<float>();
		NBCO_HIP_M(k, hipMemcpyAsync(x, src, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToDevice, k->stream));
		return body(k, x);
	};
	const int rc = pass();
	if (rc != NBCO_OK) return c->fail(rc, std::string(who) + ": " + k->err);
	return NBCO_OK;
}
}   // extern "C++"

int nbco_energy_tree(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host, double *phi_dev)
{
	if (!c || !buf || !param || !out3_host) return c ? c->fail(NBCO_ERR_ARG, "nbco_energy_tree: null pointer") : NBCO_ERR_ARG;
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "nbco_energy_tree: n must be positive");
	if (n > 0x7fffffffLL / 4) return c->fail(NBCO_ERR_UNSUPPORTED, "nbco_energy_tree: n too large for 32-bit tree indices");
	// (room behind the copy for the accelerations the evaluation writes)
	return on_private_copy(c, "nbco_energy_tree", buf, n, 6, [&](nbco_ctx *k, float *x) {
		NBCO_TRY(fmm_kdtree_eval(k, x, x + 3 * n, n, param));
		return energy_from_potential(k, buf, n, param, out3_host, phi_dev);
	});
}

// ---- 3-D probes --------------------------------------------------------------------------------
// what all three calls refuse before any launch (p == nullptr with need_p = false: the sources are the last evaluation's)
static int probe_args(nbco_ctx *c, const char *who, bool need_p, const float *p, long long n, const float *t, long long m, const float *param,
                      const double *a_dev, const double *psi_dev)
{
	if (!c) return NBCO_ERR_ARG;
	if ((need_p && !p) || !t || !param) return c->fail(NBCO_ERR_ARG, std::string(who) + ": null pointer");
	if ((need_p && n <= 0) || m <= 0) return c->fail(NBCO_ERR_ARG, std::string(who) + ": n and m must be positive");
	if (!a_dev && !psi_dev) return c->fail(NBCO_ERR_ARG, std::string(who) + ": both outputs are NULL");
	if (m >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, std::string(who) + ": m too large for 32-bit probe indices");
	if (need_p && n > 0x7fffffffLL / 4) return c->fail(NBCO_ERR_UNSUPPORTED, std::string(who) + ": n too large for 32-bit tree indices");
	return NBCO_OK;
}

int nbco_probe(nbco_ctx *c, const float *p, long long n, const float *t, long long m, const float *param, double *a_dev, double *psi_dev)
{
	NBCO_TRY(probe_args(c, "nbco_probe", true, p, n, t, m, param, a_dev, psi_dev));
	NBCO_TRY(launch_probe_direct(c, p, n, t, m, param, a_dev, psi_dev));
	return maybe_sync(c);
}

int nbco_kd_probe(nbco_ctx *c, const float *t, long long m, const float *param, double *a_dev, double *psi_dev)
{
	NBCO_TRY(probe_args(c, "nbco_kd_probe", false, nullptr, 0, t, m, param, a_dev, psi_dev));
	NBCO_TRY(kd_probe_check(c));   // (before any launch)
	NBCO_TRY(kd_probe_last(c, t, m, param, a_dev, psi_dev));
	return maybe_sync(c);
}

int nbco_probe_tree(nbco_ctx *c, const float *p, long long n, const float *t, long long m, const float *param, double *a_dev, double *psi_dev)
{
	NBCO_TRY(probe_args(c, "nbco_probe_tree", true, p, n, t, m, param, a_dev, psi_dev));
	NBCO_TRY(on_private_copy(c, "nbco_probe_tree", p, n, 3, [&](nbco_ctx *k, float *x) { return kd_probe_tree(k, x, n, t, m, param, a_dev, psi_dev); }));
	return maybe_sync(c);
}

// ---- pair statistics ---------------------------------------------------------------------------
// what all three calls refuse before any launch, and the window and bins of a good call (bins is ignored without counts)
static int pair_args(nbco_ctx *c, const char *who, bool tree, const void *p, long long n, int bins, double rmax, const void *counts_dev, const void *nn2_dev,
                     PairBins &pb)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!p) return c->fail(NBCO_ERR_ARG, w + ": null pointer");
	if (n <= 0) return c->fail(NBCO_ERR_ARG, w + ": n must be positive");
	if (!counts_dev && !nn2_dev) return c->fail(NBCO_ERR_ARG, w + ": both outputs are NULL");
	if (!std::isfinite(rmax) || !(rmax > 0.0)) return c->fail(NBCO_ERR_ARG, w + ": rmax must be finite and positive");
	if (!counts_dev) bins = 1;
	if (bins < 1 || bins > 65536) return c->fail(NBCO_ERR_ARG, w + ": bins must be 1..65536");
	pb.bins = bins;
	pb.R2 = rmax * rmax;
	pb.width = rmax / (double)bins;
	pb.inv_width = 1.0 / pb.width;
	if (counts_dev && pb.width * pb.width < DBL_MIN) return c->fail(NBCO_ERR_ARG, w + ": the square of the bin width underflows");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit particle indices");
	if (tree && n > 0x7fffffffLL / 4) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit tree indices");
	return NBCO_OK;
}

int nbco_pair_hist(nbco_ctx *c, const float *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev)
{
	PairBins pb;
	NBCO_TRY(pair_args(c, "nbco_pair_hist", false, p, n, bins, rmax, counts_dev, nn2_dev, pb));
	NBCO_TRY(launch_pair_hist(c, p, 3, n, pb, counts_dev, nn2_dev));
	return maybe_sync(c);
}

int nbco_2d_pair_hist(nbco_ctx *c, const double *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev)
{
	PairBins pb;
	NBCO_TRY(pair_args(c, "nbco_2d_pair_hist", false, p, n, bins, rmax, counts_dev, nn2_dev, pb));
	NBCO_TRY(launch_pair_hist(c, p, 2, n, pb, counts_dev, nn2_dev));
	return maybe_sync(c);
}

int nbco_pair_hist_tree(nbco_ctx *c, const float *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev)
{
	PairBins pb;
	NBCO_TRY(pair_args(c, "nbco_pair_hist_tree", true, p, n, bins, rmax, counts_dev, nn2_dev, pb));
	NBCO_TRY(on_private_copy(c, "nbco_pair_hist_tree", p, n, 3, [&](nbco_ctx *k, float *x) { return kd_pair_hist_tree(k, x, n, pb, counts_dev, nn2_dev); }));
	return maybe_sync(c);
}

// ---- bond-orientational order ------------------------------------------------------------------
int nbco_bond_harmonics(const double *u3, double *y4, double *y6)
{
	if (!u3 || !y4 || !y6) return NBCO_ERR_ARG;
	if (!std::isfinite(u3[0]) || !std::isfinite(u3[1]) || !std::isfinite(u3[2])) return NBCO_ERR_ARG;
	double a[9], b[13];
	bond_harmonics(u3[0], u3[1], u3[2], a, b);
	memcpy(y4, a, sizeof a);
	memcpy(y6, b, sizeof b);
	return NBCO_OK;
}

// what all three calls refuse before any launch
static int bond_args(nbco_ctx *c, const char *who, bool tree, const void *p, long long n, double rmax, const void *nb_dev, const void *q_dev, const void *sum_host)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!p) return c->fail(NBCO_ERR_ARG, w + ": null pointer");
	if (n <= 0) return c->fail(NBCO_ERR_ARG, w + ": n must be positive");
	if (!nb_dev && !q_dev && !sum_host) return c->fail(NBCO_ERR_ARG, w + ": all outputs are NULL");
	if (!std::isfinite(rmax) || !(rmax > 0.0)) return c->fail(NBCO_ERR_ARG, w + ": rmax must be finite and positive");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit particle indices");
	if (tree && n > 0x7fffffffLL / 4) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit tree indices");
	return NBCO_OK;
}

int nbco_bond_order(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host)
{
	NBCO_TRY(bond_args(c, "nbco_bond_order", false, p, n, rmax, nb_dev, q_dev, sum_host));
	NBCO_TRY(launch_bond_order(c, p, 3, n, rmax * rmax, nb_dev, q_dev, sum_host));
	return maybe_sync(c);
}

int nbco_2d_bond_order(nbco_ctx *c, const double *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host)
{
	NBCO_TRY(bond_args(c, "nbco_2d_bond_order", false, p, n, rmax, nb_dev, q_dev, sum_host));
	NBCO_TRY(launch_bond_order(c, p, 2, n, rmax * rmax, nb_dev, q_dev, sum_host));
	return maybe_sync(c);
}

int nbco_bond_order_tree(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host)
{
	NBCO_TRY(bond_args(c, "nbco_bond_order_tree", true, p, n, rmax, nb_dev, q_dev, sum_host));
	NBCO_TRY(on_private_copy(c, "nbco_bond_order_tree", p, n, 3, [&](nbco_ctx *k, float *x) { return kd_bond_order_tree(k, x, n, rmax * rmax, nb_dev, q_dev, sum_host); }));
	return maybe_sync(c);
}

// ---- crystalline particles: bond vector records, solid bonds and the averaged order -----------------
int nbco_bond_coherence(const double *vec_i, const double *vec_j, double *d6_host)
{
	if (!vec_i || !vec_j || !d6_host) return NBCO_ERR_ARG;
	*d6_host = bond_coherence(vec_i + kBondVec6, vec_j + kBondVec6);
	return NBCO_OK;
}

int nbco_bond_vectors(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *vec_dev)
{
	NBCO_TRY(bond_args(c, "nbco_bond_vectors", false, p, n, rmax, nb_dev, vec_dev, nullptr));
	NBCO_TRY(launch_bond_vectors(c, p, n, rmax * rmax, nb_dev, vec_dev));
	return maybe_sync(c);
}

int nbco_bond_vectors_tree(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *vec_dev)
{
	NBCO_TRY(bond_args(c, "nbco_bond_vectors_tree", true, p, n, rmax, nb_dev, vec_dev, nullptr));
	NBCO_TRY(on_private_copy(c, "nbco_bond_vectors_tree", p, n, 3, [&](nbco_ctx *k, float *x) { return kd_bond_vectors_tree(k, x, n, rmax * rmax, nb_dev, vec_dev); }));
	return maybe_sync(c);
}

// what both solid calls refuse before any launch: what the bond order refuses, and a bad threshold
static int solid_args(nbco_ctx *c, const char *who, bool tree, const void *p, long long n, double rmax, double dmin, int xi_min, const void *nb_dev, const void *xi_dev,
                      const void *qbar_dev, const void *sum_host)
{
	NBCO_TRY(bond_args(c, who, tree, p, n, rmax, nb_dev ? nb_dev : xi_dev, qbar_dev, sum_host));
	if (!std::isfinite(dmin)) return c->fail(NBCO_ERR_ARG, std::string(who) + ": dmin must be finite");
	if (xi_min < 0) return c->fail(NBCO_ERR_ARG, std::string(who) + ": xi_min must not be negative");
	return NBCO_OK;
}

int nbco_bond_solid(nbco_ctx *c, const float *p, long long n, double rmax, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev, double *qbar_dev,
                    nbco_solid_summary *sum_host)
{
	NBCO_TRY(solid_args(c, "nbco_bond_solid", false, p, n, rmax, dmin, xi_min, nb_dev, xi_dev, qbar_dev, sum_host));
	NBCO_TRY(launch_bond_solid(c, p, n, rmax * rmax, vec_dev, dmin, xi_min, nb_dev, xi_dev, qbar_dev, sum_host));
	return maybe_sync(c);
}

int nbco_bond_solid_tree(nbco_ctx *c, const float *p, long long n, double rmax, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev,
                         double *qbar_dev, nbco_solid_summary *sum_host)
{
	NBCO_TRY(solid_args(c, "nbco_bond_solid_tree", true, p, n, rmax, dmin, xi_min, nb_dev, xi_dev, qbar_dev, sum_host));
	NBCO_TRY(on_private_copy(c, "nbco_bond_solid_tree", p, n, 3, [&](nbco_ctx *k, float *x) {
		return kd_bond_solid_tree(k, x, n, rmax * rmax, vec_dev, dmin, xi_min, nb_dev, xi_dev, qbar_dev, sum_host);
	}));
	return maybe_sync(c);
}

// ---- static structure factor -------------------------------------------------------------------
int nbco_sk_phase(double t, double *cs_host)
{
	if (!cs_host || !std::isfinite(t)) return NBCO_ERR_ARG;
	const SkC e = sk_phase(t);
	cs_host[0] = e.re;
	cs_host[1] = e.im;
	return NBCO_OK;
}

// what both calls refuse before any launch
static int sk_args(nbco_ctx *c, const char *who, int dim, const void *p, long long n, const nbco_sk_grid *g, const void *rho_dev)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!p || !g || !rho_dev) return c->fail(NBCO_ERR_ARG, w + ": null pointer");
	if (n <= 0) return c->fail(NBCO_ERR_ARG, w + ": n must be positive");
	for (int a = 0; a < dim; ++a)
	{
		if (g->h[a] < 0 || g->h[a] > kSkMaxH) return c->fail(NBCO_ERR_ARG, w + ": h must be 0..64 on every axis");
		if (!std::isfinite(g->kstep[a]) || !(g->kstep[a] > 0.0)) return c->fail(NBCO_ERR_ARG, w + ": kstep must be finite and positive on every axis");
	}
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit particle indices");
	return NBCO_OK;
}

int nbco_structure_factor(nbco_ctx *c, const float *p, long long n, const nbco_sk_grid *g_host, double *rho_dev, long long *n_used_host)
{
	NBCO_TRY(sk_args(c, "nbco_structure_factor", 3, p, n, g_host, rho_dev));
	NBCO_TRY(launch_structure_factor(c, p, 3, n, *g_host, rho_dev, n_used_host));
	return maybe_sync(c);
}

int nbco_2d_structure_factor(nbco_ctx *c, const double *p, long long n, const nbco_sk_grid *g_host, double *rho_dev, long long *n_used_host)
{
	NBCO_TRY(sk_args(c, "nbco_2d_structure_factor", 2, p, n, g_host, rho_dev));
	NBCO_TRY(launch_structure_factor(c, p, 2, n, *g_host, rho_dev, n_used_host));
	return maybe_sync(c);
}

// ---- tracked trajectories and their time correlations ------------------------------------------
int nbco_traj_record(nbco_ctx *c, const float *buf, long long n, const int *ids_dev, float *traj, long long rows, int frames_cap, int frame, int stride)
{
	if (!c) return NBCO_ERR_ARG;
	if (!buf || !traj) return c->fail(NBCO_ERR_ARG, "nbco_traj_record: null pointer");
	if (n <= 0 || rows <= 0) return c->fail(NBCO_ERR_ARG, "nbco_traj_record: n and rows must be positive");
	if (stride < 1) return c->fail(NBCO_ERR_ARG, "nbco_traj_record: stride must be at least 1");
	if (frame < 0 || frame >= frames_cap) return c->fail(NBCO_ERR_ARG, "nbco_traj_record: frame must lie in [0, frames_cap)");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, "nbco_traj_record: n too large for 32-bit particle numbers");
	const int *ids = ids_dev;
	if (!ids && c->o.track_order)
	{
		// the map must describe this state: the condition of nbco_kd_copy(NBCO_KD_ORDER)
		if (c->order_n != n) return c->fail(NBCO_ERR_ARG, "nbco_traj_record: opts.track_order is set but no tracked evaluation of these n particles has run (pass ids_dev)");
		ids = c->order.as<int>();
	}
	NBCO_TRY(launch_traj_record(c, buf, n, ids, traj, rows, frames_cap, frame, stride));
	return maybe_sync(c);
}

int nbco_time_corr(nbco_ctx *c, const float *traj, long long rows, int frames_cap, int frames, int lags, nbco_corr_lag *out_dev)
{
	if (!c) return NBCO_ERR_ARG;
	if (!traj || !out_dev) return c->fail(NBCO_ERR_ARG, "nbco_time_corr: null pointer");
	if (rows <= 0) return c->fail(NBCO_ERR_ARG, "nbco_time_corr: rows must be positive");
	if (lags < 1 || lags > frames || frames > frames_cap) return c->fail(NBCO_ERR_ARG, "nbco_time_corr: need 1 <= lags <= frames <= frames_cap");
	if (frames > kTcMaxFrames) return c->fail(NBCO_ERR_ARG, "nbco_time_corr: at most 2048 frames");
	NBCO_TRY(launch_time_corr(c, traj, rows, frames_cap, frames, lags, out_dev));
	return maybe_sync(c);
}

int nbco_time_corr_derive(const nbco_corr_lag *in, int lags, double *out)
{
	if (!in || !out || lags < 0) return NBCO_ERR_ARG;
	for (int l = 0; l < lags; ++l) tc_derive(in[l].dx2, in[l].r4, in[l].vv, in[l].pairs, out + 8 * (size_t)l);
	return NBCO_OK;
}

// ---- collective modes ----------------------------------------------------------------------------
int nbco_modes_record(nbco_ctx *c, const float *buf, long long n, const nbco_sk_grid *g_host, double *series_dev, int frames_cap, int frame, long long *n_used_host)
{
	NBCO_TRY(sk_args(c, "nbco_modes_record", 3, buf, n, g_host, series_dev));
	if (frames_cap < 1) return c->fail(NBCO_ERR_ARG, "nbco_modes_record: frames_cap must be at least 1");
	if (frame < 0 || frame >= frames_cap) return c->fail(NBCO_ERR_ARG, "nbco_modes_record: frame must lie in [0, frames_cap)");
	NBCO_TRY(launch_modes_record(c, buf, n, *g_host, series_dev, frames_cap, frame, n_used_host));
	return maybe_sync(c);
}

// what the correlation calls refuse of a grid and a shape
static bool md_shape_ok(const nbco_sk_grid *g, int frames_cap, int frames, int lags)
{
	for (int a = 0; a < 3; ++a)
		if (g->h[a] < 0 || g->h[a] > kSkMaxH || !std::isfinite(g->kstep[a]) || !(g->kstep[a] > 0.0)) return false;
	return lags >= 1 && lags <= frames && frames <= frames_cap && frames <= kMdMaxFrames;
}

int nbco_mode_corr(nbco_ctx *c, const double *series_dev, const nbco_sk_grid *g_host, int frames_cap, int frames, int lags, nbco_mode_lag *out_dev)
{
	if (!c) return NBCO_ERR_ARG;
	if (!series_dev || !g_host || !out_dev) return c->fail(NBCO_ERR_ARG, "nbco_mode_corr: null pointer");
	if (!md_shape_ok(g_host, frames_cap, frames, lags))
		return c->fail(NBCO_ERR_ARG, "nbco_mode_corr: need h 0..64 and kstep finite and positive on every axis, 1 <= lags <= frames <= frames_cap and at most 1024 frames");
	NBCO_TRY(launch_mode_corr(c, series_dev, *g_host, frames_cap, frames, lags, out_dev));
	return maybe_sync(c);
}

int nbco_mode_corr_ref(const double *series_host, const nbco_sk_grid *g_host, int frames_cap, int frames, int lags, nbco_mode_lag *out_host)
{
	if (!series_host || !g_host || !out_host || !md_shape_ok(g_host, frames_cap, frames, lags)) return NBCO_ERR_ARG;
	const long long K = sk_count(g_host->h, 3);
	for (long long k = 0; k < K; ++k)
	{
		const double *row = series_host + (size_t)k * (size_t)frames_cap * 8;
		double kv[3];
		md_wave_vector(k, g_host->h, g_host->kstep, kv);
		for (int tau = 0; tau < lags; ++tau)
		{
			MdSum s;
			md_sum_zero(s);
			for (int t = 0; t + tau < frames; ++t)
			{
				const double *a = row + 8 * (size_t)t, *b = row + 8 * (size_t)(t + tau);
				const SkC arho = {a[0], a[1]}, ajx = {a[2], a[3]}, ajy = {a[4], a[5]}, ajz = {a[6], a[7]};
				const SkC brho = {b[0], b[1]}, bjx = {b[2], b[3]}, bjy = {b[4], b[5]}, bjz = {b[6], b[7]};
				md_term(s, kv[0], kv[1], kv[2], arho, ajx, ajy, ajz, md_long(kv[0], kv[1], kv[2], ajx, ajy, ajz), brho, bjx, bjy, bjz);
			}
			nbco_mode_lag &o = out_host[(size_t)k * (size_t)lags + (size_t)tau];
			o.rr = s.rr; o.ll = s.ll; o.jj = s.jj;
			o.s0[0] = s.s0.re; o.s0[1] = s.s0.im;
			o.s1[0] = s.s1.re; o.s1[1] = s.s1.im;
			o.pairs = (unsigned long long)(frames - tau);
		}
	}
	return NBCO_OK;
}

int nbco_mode_corr_derive(const nbco_mode_lag *in, const nbco_sk_grid *g_host, int lags, double n_norm, double *out)
{
	if (!in || !g_host || !out || lags < 0) return NBCO_ERR_ARG;
	for (int a = 0; a < 3; ++a)
		if (g_host->h[a] < 0 || g_host->h[a] > kSkMaxH) return NBCO_ERR_ARG;
	const long long K = sk_count(g_host->h, 3);
	for (long long k = 0; k < K; ++k)
	{
		double kv[3];
		md_wave_vector(k, g_host->h, g_host->kstep, kv);
		const double k2 = md_k2(kv);
		for (int l = 0; l < lags; ++l)
		{
			const nbco_mode_lag &r = in[(size_t)k * (size_t)lags + (size_t)l];
			md_derive(r.rr, r.ll, r.jj, r.s0, r.s1, r.pairs, k2, n_norm, out + 4 * ((size_t)k * (size_t)lags + (size_t)l));
		}
	}
	return NBCO_OK;
}

// ---- aperture ----------------------------------------------------------------------------------
// what the four calls refuse before any launch, and the rule of a good call (dim 2 reads the first two axes)
static int aperture_args(nbco_ctx *c, const char *who, int dim, const void *p, long long n, const nbco_aperture *ap, const void *count_host, long long lost_cap,
                         ApRule &r)
{
	if (!c) return NBCO_ERR_ARG;
	const std::string w(who);
	if (!p || !ap || !count_host) return c->fail(NBCO_ERR_ARG, w + ": null pointer");
	if (n <= 0) return c->fail(NBCO_ERR_ARG, w + ": n must be positive");
	if (ap->shape != NBCO_AP_ELLIPSOID && ap->shape != NBCO_AP_BOX) return c->fail(NBCO_ERR_ARG, w + ": unknown shape");
	r.shape = ap->shape;
	for (int a = 0; a < 3; ++a)
	{
		// (an axis the state does not have is open and centred: it decides nothing)
		const double centre = a < dim ? ap->centre[a] : 0.0, half = a < dim ? ap->half[a] : INFINITY;
		if (!std::isfinite(centre)) return c->fail(NBCO_ERR_ARG, w + ": centre must be finite");
		if (!(half > 0.0)) return c->fail(NBCO_ERR_ARG, w + ": half must be positive (+infinity opens an axis)");
		r.centre[a] = centre;
		r.half[a] = half;
		r.w[a] = 1.0 / half;
	}
	if (lost_cap < 0) return c->fail(NBCO_ERR_ARG, w + ": lost_cap must not be negative");
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, w + ": n too large for 32-bit row numbers");
	return NBCO_OK;
}

// the classification, the refusal of a record that is too small, the compaction; live: the order map travels (3-D only)
static int aperture_apply(nbco_ctx *c, const char *who, int dim, void *buf, long long n, const ApRule &r, long long *n_kept_host, void *lost_dev,
                          int *lost_row_dev, long long lost_cap)
{
	long long lost = 0;
	NBCO_TRY(launch_aperture_classify(c, buf, dim, n, r, true, &lost));
	*n_kept_host = n - lost;
	if (lost == 0) return NBCO_OK;
	if ((lost_dev || lost_row_dev) && lost > lost_cap) return c->fail(NBCO_ERR_CAPACITY, std::string(who) + ": more particles are lost than the record holds");
	const bool live = dim == 3 && c->o.track_order && c->order_n == n;
	NBCO_TRY(launch_aperture_compact(c, buf, dim, n, lost, r, lost_dev, lost_row_dev, live ? c->order.as<int>() : nullptr, live ? c->order_alt.as<int>() : nullptr));
	if (dim == 3)
	{
		// a new state: no tree, a new rebuild schedule (as nbco_set_opts), nothing of the last evaluation to read
		c->tree_valid = false;
		c->eval_counter = 0;
		c->last_eval.valid = false;
		if (live) { std::swap(c->order, c->order_alt); c->order_n = n - lost; }
		else c->order_n = -1;
	}
	NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

int nbco_aperture_count(nbco_ctx *c, const float *p, long long n, const nbco_aperture *ap_host, long long *n_lost_host)
{
	ApRule r;
	NBCO_TRY(aperture_args(c, "nbco_aperture_count", 3, p, n, ap_host, n_lost_host, 0, r));
	return launch_aperture_classify(c, p, 3, n, r, false, n_lost_host);
}

int nbco_2d_aperture_count(nbco_ctx *c, const double *p, long long n, const nbco_aperture *ap_host, long long *n_lost_host)
{
	ApRule r;
	NBCO_TRY(aperture_args(c, "nbco_2d_aperture_count", 2, p, n, ap_host, n_lost_host, 0, r));
	return launch_aperture_classify(c, p, 2, n, r, false, n_lost_host);
}

int nbco_aperture_apply(nbco_ctx *c, float *buf, long long n, const nbco_aperture *ap_host, long long *n_kept_host, float *lost_dev, int *lost_row_dev,
                        long long lost_cap)
{
	ApRule r;
	NBCO_TRY(aperture_args(c, "nbco_aperture_apply", 3, buf, n, ap_host, n_kept_host, lost_cap, r));
	return aperture_apply(c, "nbco_aperture_apply", 3, buf, n, r, n_kept_host, lost_dev, lost_row_dev, lost_cap);
}

int nbco_2d_aperture_apply(nbco_ctx *c, double *buf, long long n, const nbco_aperture *ap_host, long long *n_kept_host, double *lost_dev,
                           int *lost_row_dev, long long lost_cap)
{
	ApRule r;
	NBCO_TRY(aperture_args(c, "nbco_2d_aperture_apply", 2, buf, n, ap_host, n_kept_host, lost_cap, r));
	return aperture_apply(c, "nbco_2d_aperture_apply", 2, buf, n, r, n_kept_host, lost_dev, lost_row_dev, lost_cap);
}

// ---- introspection -----------------------------------------------------------------------------
int nbco_kd_get_info(nbco_ctx *c, nbco_kd_info *info)
{
	if (!c || !info) return NBCO_ERR_ARG;
	if (c->info.directed_p2p < 0 && c->counters.ptr && c->tree_valid)
	{
		long long v = 0;
		NBCO_TRY(kd_count_pairs(c, &v));   // one small kernel over the sorted P2P list of the last evaluation
		c->info.directed_p2p = v;
	}
	*info = c->info;
	info->build_mode = c->force_sort_build ? 2 : (c->sel_three_pass ? 1 : 0);
	info->warm_builds = c->sel_warm_builds; info->warm_misses = c->sel_warm_misses;
	info->real_bytes = c->kd.real_bytes;
	return NBCO_OK;
}
int nbco_kd_copy(nbco_ctx *c, int which, void *host_dst, long long host_bytes)
{
	if (!c || !host_dst) return NBCO_ERR_ARG;
	return kd_copy_out(c, which, host_dst, host_bytes);
}

// ---- checked build -----------------------------------------------------------------------------
int nbco_debug_violations(nbco_ctx *c, long long *out8)
{
	if (!c || !out8) return c ? c->fail(NBCO_ERR_ARG, "nbco_debug_violations: null pointer") : NBCO_ERR_ARG;
	for (int i = 0; i < NBCO_CHK_SITES; ++i) out8[i] = 0;
#ifdef NBCO_CHECKED
	NBCO_HIP(hipDeviceSynchronize());
	unsigned v[NBCO_CHK_SITES] = {};
	NBCO_TRY(nbco_checked_collect_kd(v));
	NBCO_TRY(nbco_checked_collect_oct(v));
	NBCO_TRY(nbco_checked_collect_far(v));
	NBCO_TRY(nbco_checked_collect_reduce(v));
	for (int i = 0; i < NBCO_CHK_SITES; ++i) out8[i] = v[i];
	return NBCO_OK;
#else
	return c->fail(NBCO_ERR_UNSUPPORTED, "nbco_debug_violations: this is not the checked build (libnbco_hip_checked.so)");
#endif
}

// ---- profiling ---------------------------------------------------------------------------------
int nbco_profile_enable(nbco_ctx *c, int on)
{
	if (!c) return NBCO_ERR_ARG;
	c->profiling = on < 0 ? 0xFFFFFFFFu : (unsigned)on;
	return NBCO_OK;
}
static int drain_timers(nbco_ctx *c)
{
	NBCO_HIP(hipStreamSynchronize(c->stream));
	for (auto &t : c->timers)
	{
		for (auto &ev : t.pending)
		{
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { t.total_ms += ms; t.launches += 1; }
			hipEventDestroy(ev.first);
			hipEventDestroy(ev.second);
		}
		t.pending.clear();
	}
	return NBCO_OK;
}
int nbco_profile_reset(nbco_ctx *c)
{
	if (!c) return NBCO_ERR_ARG;
	NBCO_TRY(drain_timers(c));
	for (auto &t : c->timers) { t.total_ms = 0; t.launches = 0; }
	return NBCO_OK;
}
int nbco_profile_get(nbco_ctx *c, int ph, double *total_ms, long long *launches)
{
	if (!c || ph < 0 || ph >= NBCO_PH_COUNT) return NBCO_ERR_ARG;
	NBCO_TRY(drain_timers(c));
	if (total_ms) *total_ms = c->timers[ph].total_ms;
	if (launches) *launches = c->timers[ph].launches;
	return NBCO_OK;
}

// ---- initial condition: initGA / initU of main3.cu:71-137 over the reference's generator (host only) --------------------------
namespace {
struct V3 { float x, y, z; };
void centre_dist(V3 *d, long long n)   // main3.cu:71-80 (fp32 running sums, as there)
{
	V3 c{0, 0, 0};
	for (long long i = 0; i < n; ++i) { c.x += d[i].x; c.y += d[i].y; c.z += d[i].z; }
	c.x /= (float)n; c.y /= (float)n; c.z /= (float)n;
	for (long long i = 0; i < n; ++i) { d[i].x -= c.x; d[i].y -= c.y; d[i].z -= c.z; }
}
void adjust_rms(V3 *d, long long n, V3 adj)   // main3.cu:82-92
{
	V3 s{0, 0, 0};
	for (long long i = 0; i < n; ++i) { s.x += d[i].x * d[i].x; s.y += d[i].y * d[i].y; s.z += d[i].z * d[i].z; }
	s.x = std::sqrt(s.x / (float)n); s.y = std::sqrt(s.y / (float)n); s.z = std::sqrt(s.z / (float)n);
	const V3 f{adj.x / s.x, adj.y / s.y, adj.z / s.z};   // `data[i] *= adj / d`: the quotient first, then one product
	for (long long i = 0; i < n; ++i) { d[i].x *= f.x; d[i].y *= f.y; d[i].z *= f.z; }
}
} // namespace

int nbco_init_gaussian(float *host_state, long long n, const float *sx, const float *su, unsigned long long seed, unsigned long long discard,
                       int uniform_positions)
{
	if (!host_state || !sx || !su || n <= 0) return NBCO_ERR_ARG;
	std::mt19937_64 gen(seed);
	gen.discard(discard);
	std::normal_distribution<float> dist(0.f, 1.f);
	for (long long i = 0; i < 6 * n; ++i) host_state[i] = dist(gen);   // all position deviates, then all velocity deviates (:121-123)
	V3 *pos = reinterpret_cast<V3 *>(host_state), *vel = pos + n;
	const V3 x{sx[0], sx[1], sx[2]}, u{su[0], su[1], su[2]};
	for (long long i = 0; i < n; ++i) { pos[i].x *= x.x; pos[i].y *= x.y; pos[i].z *= x.z; }
	for (long long i = 0; i < n; ++i) { vel[i].x *= u.x; vel[i].y *= u.y; vel[i].z *= u.z; }
	centre_dist(pos, n); adjust_rms(pos, n, x);
	centre_dist(vel, n); adjust_rms(vel, n, u);
	if (uniform_positions)   // initU with a = -1, b = 1 (main3.cu:94-111)
	{
		std::uniform_real_distribution<float> dx(-1, 1), dy(-1, 1), dz(-1, 1);
		for (long long i = 0; i < n; ++i) { pos[i].x = dx(gen); pos[i].y = dy(gen); pos[i].z = dz(gen); }
		centre_dist(pos, n);
	}
	return NBCO_OK;
}

// The rows [first, first + count) of the state nbco_init_gaussian(n, ..) would produce, without ever holding more than the slice:
// the generator is run through the whole stream twice (the centring and the RMS rescaling need sums over ALL n particles, taken
// in the same order and precision as there), so the result equals the corresponding rows of the full state bit for bit.
int nbco_init_gaussian_slice(float *host_slice, long long n, long long first, long long count, const float *sx, const float *su,
                             unsigned long long seed, unsigned long long discard, int uniform_positions)
{
	if (!host_slice || !sx || !su || n <= 0 || first < 0 || count <= 0 || first + count > n) return NBCO_ERR_ARG;
	V3 *pos = reinterpret_cast<V3 *>(host_slice), *vel = pos + count;
	const V3 sc[2] = {{sx[0], sx[1], sx[2]}, {su[0], su[1], su[2]}};
	V3 mean[2], fac[2];
	// pass 1: the scaled deviates of the slice, and the running sums of centre_dist
	{
		std::mt19937_64 gen(seed);
		gen.discard(discard);
		std::normal_distribution<float> dist(0.f, 1.f);
		for (int part = 0; part < 2; ++part)
		{
			V3 *out = part ? vel : pos;
			V3 c{0, 0, 0};
			for (long long i = 0; i < n; ++i)
			{
				V3 v;
				v.x = dist(gen); v.y = dist(gen); v.z = dist(gen);
				v.x *= sc[part].x; v.y *= sc[part].y; v.z *= sc[part].z;
				c.x += v.x; c.y += v.y; c.z += v.z;
				if (i >= first && i < first + count) out[i - first] = v;
			}
			mean[part] = V3{c.x / (float)n, c.y / (float)n, c.z / (float)n};
		}
	}
	// pass 2: the sums of squares of the centred values (adjust_rms)
	{
		std::mt19937_64 gen(seed);
		gen.discard(discard);
		std::normal_distribution<float> dist(0.f, 1.f);
		for (int part = 0; part < 2; ++part)
		{
			V3 s{0, 0, 0};
			for (long long i = 0; i < n; ++i)
			{
				V3 v;
				v.x = dist(gen); v.y = dist(gen); v.z = dist(gen);
				v.x *= sc[part].x; v.y *= sc[part].y; v.z *= sc[part].z;
				v.x -= mean[part].x; v.y -= mean[part].y; v.z -= mean[part].z;
				s.x += v.x * v.x; s.y += v.y * v.y; s.z += v.z * v.z;
			}
			s.x = std::sqrt(s.x / (float)n); s.y = std::sqrt(s.y / (float)n); s.z = std::sqrt(s.z / (float)n);
			fac[part] = V3{sc[part].x / s.x, sc[part].y / s.y, sc[part].z / s.z};
		}
		for (int part = 0; part < 2; ++part)
		{
			V3 *out = part ? vel : pos;
			for (long long i = 0; i < count; ++i)
			{
				out[i].x -= mean[part].x; out[i].y -= mean[part].y; out[i].z -= mean[part].z;
				out[i].x *= fac[part].x; out[i].y *= fac[part].y; out[i].z *= fac[part].z;
			}
		}
		if (uniform_positions)   // initU: the generator goes on behind the 6 n normal deviates
		{
			std::uniform_real_distribution<float> dx(-1, 1), dy(-1, 1), dz(-1, 1);
			V3 c{0, 0, 0};
			for (long long i = 0; i < n; ++i)
			{
				V3 v;
				v.x = dx(gen); v.y = dy(gen); v.z = dz(gen);
				c.x += v.x; c.y += v.y; c.z += v.z;
				if (i >= first && i < first + count) pos[i - first] = v;
			}
			c.x /= (float)n; c.y /= (float)n; c.z /= (float)n;
			for (long long i = 0; i < count; ++i) { pos[i].x -= c.x; pos[i].y -= c.y; pos[i].z -= c.z; }
		}
	}
	return NBCO_OK;
}

} // extern "C"
