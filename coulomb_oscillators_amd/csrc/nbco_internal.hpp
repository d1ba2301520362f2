// nbco_internal.hpp -- context, error plumbing and launch declarations shared by the HIP
// translation units of libnbco_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/nbco.h"

#define NBCO_HIP(call)                                                                           \
	do {                                                                                         \
		hipError_t e_ = (call);                                                                  \
		if (e_ != hipSuccess) return c->fail_hip(e_, #call, __FILE__, __LINE__);                 \
	} while (0)

#define NBCO_HIP_M(ctx_, call)                                                                   \
	do {                                                                                         \
		hipError_t e_ = (call);                                                                  \
		if (e_ != hipSuccess) return (ctx_)->fail_hip(e_, #call, __FILE__, __LINE__);            \
	} while (0)

#define NBCO_TRY(call)                   \
	do {                                 \
		int rc_ = (call);                \
		if (rc_ != NBCO_OK) return rc_;  \
	} while (0)

// ---- checked build (-DNBCO_CHECKED, libnbco_hip_checked.so) ------------------------------------------------------------
// Every index that a kernel READS FROM A LIST (frontier pairs, unordered pair lists and their slots, sorted entries, source
// descriptors, work units) is range-checked before it is used as an address: a violation is counted per site and the index
// replaced by a harmless one, so that a corrupted or stale list shows up as a number (nbco_debug_violations) instead of a GPU
// memory fault.  The production build compiles the checks away.
enum
{
	NBCO_CHK_FRONTIER = 0,   // traverse_kernel: node ids of a frontier pair
	NBCO_CHK_FILL = 1,       // list_fill_kernel: region slot, targets, slot inside the target's range
	NBCO_CHK_SORT = 2,       // list_segsort_kernel: source index of an entry, output slot
	NBCO_CHK_CHUNK = 3,      // pair kernels: work-unit record
	NBCO_CHK_DESC = 4,       // pair kernels: source descriptor
	NBCO_CHK_L2P = 5,        // l2p_gen_kernel: chunk range, reaction record
	NBCO_CHK_WALK = 6,       // probe walk, pair walk, potential pass: sorted probe, leaf and node ranges, decoded list entries, unsort map
	NBCO_CHK_GROUP = 7,      // slice and aperture kernels: chunk table, sorted row, slab range, compaction slot
	NBCO_CHK_SITES = 8
};
#ifdef NBCO_CHECKED
namespace { __device__ unsigned nbco_violation_count[NBCO_CHK_SITES]; }
#define NBCO_CHECKED_OK(cond, site) ((cond) ? true : (atomicAdd(&nbco_violation_count[site], 1u), false))
#define NBCO_CHECKED_COLLECT(fn)                                                                                      \
	int fn(unsigned *out)                                                                                             \
	{                                                                                                                 \
		unsigned v[NBCO_CHK_SITES];                                                                                   \
		if (hipMemcpyFromSymbol(v, HIP_SYMBOL(nbco_violation_count), sizeof v) != hipSuccess) return NBCO_ERR_HIP;    \
		for (int i = 0; i < NBCO_CHK_SITES; ++i) out[i] += v[i];                                                      \
		return NBCO_OK;                                                                                               \
	}
// a bound that only a check reads: a trailing kernel parameter and its argument exist in the checked build alone, so the production
// kernels keep their signatures (the name is used inside NBCO_CHECKED_OK conditions only, which the production build discards)
#define NBCO_CHECKED_ARG(...) , __VA_ARGS__
#else
#define NBCO_CHECKED_OK(cond, site) (true)
#define NBCO_CHECKED_COLLECT(fn) int fn(unsigned *) { return NBCO_OK; }
#define NBCO_CHECKED_ARG(...)
#endif
int nbco_checked_collect_kd(unsigned *out);
int nbco_checked_collect_reduce(unsigned *out);
int nbco_checked_collect_oct(unsigned *out);
int nbco_checked_collect_far(unsigned *out);

// device buffer that only grows (the reference's evaluators keep their scratch in function-local
// statics that grow monotonically, fmm_cart3_kdtree.cuh:1480-1498)
// Owns its allocation: move-only (std::swap exchanges two buffers), freed with the context once nbco_destroy has drained the streams.
struct DevBuf
{
	void *ptr = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }
	~DevBuf() { if (ptr) hipFree(ptr); }
	template <class T> T *as() const { return (T *)ptr; }
};

struct PhaseTimer
{
	std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
	double total_ms = 0;
	long long launches = 0;
};

constexpr int kMaxOrder = 10;

// kd-tree state in HBM (fmmTree_kd of fmm_cart3_kdtree.cuh:25-31, plus the packed arrays the
// gfx950 kernels read)
struct KdTreeDev
{
	int L = 0, ntot = 0, order = 0, mlt_max = 0;
	long long n = 0;
	float *center = nullptr, *lbound = nullptr, *rbound = nullptr;   // [ntot][3]
	float4 *csz = nullptr;                                           // [ntot] centre xyz + box diagonal^2
	float *mpole = nullptr, *local = nullptr;                        // [ntot][offM], [ntot][offL]; DOUBLE tuples behind these pointers when real_bytes == 8
	int *mult = nullptr, *index = nullptr, *splitdim = nullptr;      // [ntot]
	int real_bytes = 4;                                              // element size of mpole / local: 8 with opts.far_fp64
};

// uniform-octree state of the last nbco_fmm_traceless call (fmmTree of fmm_cart3_symmetric.cuh:24-30)
struct OctTreeDev
{
	bool valid = false;
	int L = 0, ntot = 0, order = 0, tpl = 0;
	long long n = 0, m2l_entries = 0, p2p_groups = 0, p2p_desc = 0, p2p_chunks = 0;
	float4 *csz = nullptr;
	void *mpole = nullptr, *local = nullptr;   // float or double (real_bytes)
	int real_bytes = 4;
	int mpole_reals = 0;   // reals per multipole tuple: (p+1)^2 traceless, (p+1)(p+2)(p+3)/6 symmetric
	int *mult = nullptr, *index = nullptr;
	uint32_t *keys = nullptr, *perm = nullptr;
};

// What a leapfrog driver (nbco_integrate, nbco_integrate_steps) and the kd-tree evaluations of one ABI call hand each other.  It
// lives on the driver's stack and goes down as a pointer; every other caller of the evaluator passes nullptr.
struct KdStepLink
{
	bool defer_order = false, defer_v_copy = false;   // in: leave the re-ordering after a rebuild to me / the tree-ordered velocities in scratch
	int prep_done = 0;              // in, consumed by the build: its prologue (1) / the packing for a reused tree (2) is already done
	bool order_pending = false;     // out: a re-ordering is due
	const float *v_now = nullptr;   // out: where the velocities are now; nullptr: in the caller's array
};

// The root of a local build; the default is the global root.  root6 (device, {lbound, rbound}): the box a kd-domain inherits from
// the global tree's top splits.  top_sd, top_root1: the split axes of the root's ancestors in the GLOBAL tree (the top tree of the
// partition step, device array) and the root's 1-based heap number there.
struct KdRoot { const float *root6 = nullptr; const int *top_sd = nullptr; int top_root1 = 1; };

struct nbco_ctx
{
	nbco_opts o;
	hipStream_t stream = nullptr;   // the stream work is enqueued on (the caller's, or `aux` inside a StreamScope)
	// second stream for the chains that do not depend on each other (multipoles || traversal, M2L lists || P2P lists);
	// created lazily, ordered against `stream` with events only
	hipStream_t aux = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	bool aux_pending = false;
	int list_growth = 1;   // the lists hold list_growth * opts.list_factor * nodes pairs (doubled after an overflow, opts.list_grow)
	bool grow_lists(int ntot)   // false: growth is off or exhausted
	{
		if (!o.list_grow || list_growth >= 64) return false;
		// 32-bit offsets: the DIRECTED P2P list holds up to 2 * cap + leaves entries, cap = 2 * (growth * factor * nodes + 4096),
		// and its prefix sums (start[], chunk_off[], the low word of the packed scan) are ints: the doubled capacity must keep
		// 2 * cap + nodes below 2^31
		if (8LL * list_growth * o.list_factor * (long long)ntot + 16384 + ntot >= (1LL << 31)) return false;
		list_growth *= 2;
		return true;
	}
	long long perm_primed_n = -1;   // particle count for which both permutation buffers were last filled with valid indices
	double host_wait_s = 0, host_call_s = 0;   // diagnostics (NBCO_HOST_TIMING): time blocked on the flags event / inside nbco_integrate
	long long host_calls = 0;
	bool aux_is_main = false;   // NBCO_AUX_SERIAL=1 (diagnostics): the second stream is the main stream
	bool poison = false;        // NBCO_POISON=1 (diagnostics): every new scratch allocation is filled with 0x7f bytes, the way a recycled
	                            // allocation holds stale data: nothing may depend on fresh memory being zero.  That includes `small`, the block
	                            // of device scalars (filled in nbco_create), and the private child context (energy_child), which is created
	                            // through nbco_create and reads the same variable
	// traversal counts / flags land in pinned host memory; looked at after the rest of the evaluation is enqueued
	int *h_flags = nullptr;
	hipEvent_t ev_flags = nullptr;
	long long hint_np2p = 0, hint_nm2l = 0;   // list sizes of the previous evaluation (launch-size hints only)
	int flags_begin();
	int flags_seq = 0;   // sequence number of the traversal whose results h_flags[0..3] hold (h_flags[4], written last)
	int wait_flags();    // until the traversal enqueued last has reported: spins on the pinned word, no interrupt-driven wake-up
	DevBuf scan_tmp_aux;
	int fork_aux();   // aux waits for everything enqueued on `stream` so far
	int fork_mark();  // remember this point of `stream` ...
	int fork_wait();  // ... and let aux wait for it (called after more work has been enqueued on `stream`)
	int join_aux();   // `stream` waits for everything enqueued on aux
	std::string err;
	int device = 0;
	int num_cu = 256;

	// generic scratch
	DevBuf pos4;          // float4[n] packed positions (xyz, 0)
	DevBuf pos4_alt;      // second buffer for gathers
	DevBuf part;          // partial results of reductions / direct j-splits
	DevBuf small;         // a few hundred bytes of device scalars
	DevBuf tmp3, tmp3b;   // float[3n] scratch for gathers of xyz triplets (tmp3b: second velocity copy of nbco_integrate_steps)
	// kd-tree build
	DevBuf keys, keys_alt, idx, idx_alt, unsort, unsort_alt, sort_tmp;
	DevBuf treebuf;
	KdTreeDev kd;
	// traversal and interaction lists
	DevBuf frontier_a, frontier_b, p2p_list, m2l_list, counters;
	DevBuf p2p_keys, p2p_keys_alt, m2l_keys, m2l_keys_alt, p2p_start, m2l_start;
	DevBuf p2p_chunk_off, p2p_chunks, p2p_desc;
	DevBuf order, order_alt;     // opts.track_order: position in the state -> particle number of the state the tracking started from
	long long order_n = -1;
	DevBuf p2p_sec, p2p_react;   // mutual near field: per-target range of entries delivered by other waves, reaction records
	const int *pc_mult = nullptr, *pc_total = nullptr;   // inputs of the on-demand directed pair count
	int pc_shift = 0;
	DevBuf list_cnt, trav_ctr;
	DevBuf prep_state;   // min / max accumulators + completion counter of the build prologue kernel
	DevBuf sel_hist, sel_nodes, sel_ties;   // selection build (k_kdselect.hip)
	// multi-GPU kd-domain sharding: boxes / split axes of the global levels 0 .. d, the assembled global tree
	DevBuf dist_top, dist_tree;
	// LET exchange: need masks + per-receiver selections, arrival flags, the (sparse) global position array
	DevBuf let_sel, let_have, dist_pos;
	// octree-traceless evaluator (k_fmm_oct.hip)
	DevBuf oct_tree, oct_groups;
	// 2-D fp64 evaluators (k_fmm2d.hip): quadtree arrays, keys / permutation, gather scratch, reduction partials
	DevBuf f2d_tree, f2d_keys, f2d_tmp, f2d_part;
	// probe calls: the probes' keys / permutation / leaf index, and their sort's scratch (f2d_tmp holds the sources meanwhile)
	DevBuf f2d_pkeys, f2d_ptmp;
	OctTreeDev oct;
	struct DistState
	{
		int world = 0, rank = 0, d = 0, L = 0;
		long long n_global = 0, n_local = 0;
		bool partitioned = false, build_done = false, local_done = false, rebuilt = false, traversed = false, let_selected = false, let_packed = false;
		const void *pos_all = nullptr;   // gathered positions, between the two halves of the finish stage
		// LET exchange with capped segments (nbco_dist_let_pack_capped): the attempt in flight is one, and its build turned out flagged
		bool let_capped = false, let_flagged = false;
		// attempts finished so far; the guard of attempt k reports into word pair k & 1, and a pair whose attempt the caller
		// declared void (nbco_dist_let_settle(ok = 0)) is dropped unread
		long long let_epoch = 0;
		bool let_ignore[2] = {false, false};
		// KdStepLink::prep_done of nbco_dist_turnaround, the one mark that outlives an ABI call: the next local build consumes it, a (re-)partition discards it
		int prep_done = 0;
	} dist;
	// warm select (k_kdselect.hip): one histogram pass per level around the previous build's pivots.  used: this build ran it;
	// a flagged build that used it is repeated cold before anything is escalated, three misses in a row switch it off
	bool sel_warm_enabled = true, sel_warm_used = false;
	// coarsen: bucket width x 4^coarsen after misses; recent / recent_miss: the current window of 32 warm builds; cooldown: cold builds left
	int sel_warm_coarsen = 0, sel_warm_good = 0, sel_warm_recent = 0, sel_warm_recent_miss = 0, sel_warm_cooldown = 0, sel_warm_cool_len = 128;
	long long sel_warm_builds = 0, sel_warm_misses = 0;
	// A miss costs a whole evaluation, a warm build saves ~5 % of one: it pays while fewer than one build in twenty misses.
	// Drift-type misses are answered with coarser buckets (a window 4x as wide per miss, three times); a node whose parent
	// changed its split axis cannot be predicted at all, and while the cloud changes shape that happens every few builds:
	// two misses within 32 warm builds send the warm select into a cool-down (128 builds, doubling up to 4096).
	void note_warm_miss()
	{
		++sel_warm_misses;
		sel_warm_good = 0;
		if (sel_warm_coarsen < 3) ++sel_warm_coarsen;
		if (++sel_warm_recent_miss >= 2)
		{
			sel_warm_cooldown = sel_warm_cool_len;
			sel_warm_cool_len = sel_warm_cool_len < 2048 ? 2 * sel_warm_cool_len : 4096;
			sel_warm_recent = sel_warm_recent_miss = 0;
		}
	}
	void note_warm_ok()
	{
		if (++sel_warm_recent >= 32) sel_warm_recent = sel_warm_recent_miss = 0;
		if (++sel_warm_good >= 64)   // a quiet stretch: back towards fine buckets and short cool-downs
		{
			if (sel_warm_coarsen > 0) --sel_warm_coarsen;
			sel_warm_cool_len = sel_warm_cool_len > 256 ? sel_warm_cool_len / 2 : 128;
			sel_warm_good = 0;
		}
	}
	bool sel_three_pass = false;            // set after the first tie / bucket overflow: three radix passes per select
	bool force_sort_build = false;          // set after the second: use the sorting build from then on
	bool escalate_build()                   // next more conservative build; false when there is none left
	{
		if (!sel_three_pass) { sel_three_pass = true; return true; }
		if (!force_sort_build) { force_sort_build = true; return true; }
		return false;
	}
	// a flagged build (tie overflow, or a window of the warm select that missed its median) is not the reference's tree: repeat it
	// cold if the warm select ran -- nothing escalated -- and one step more conservatively otherwise; false when nothing is left
	bool demote_build()
	{
		tree_valid = false;
		if (sel_warm_used) note_warm_miss();
		return sel_warm_used || escalate_build();
	}
	long long list_cap = 0;
	// distributed re-partition in progress (k_dpart.hip)
	struct DPart
	{
		int stage = 0, level = 0, pass = 0, world = 0, rank = 0, d = 0;
		long long n_global = 0, n_local = 0;
		float *state = nullptr;
		void *work = nullptr;
		size_t tie_bytes = 0;
		bool seg_flip = false, pos_flip = false;
		long long rows_send[64] = {}, rows_recv[64] = {};
	} dpart;
	DevBuf dpart_buf;
	// the last kd-tree evaluation, for nbco_energy_fmm (pointers into the context's buffers; valid while tree_valid)
	struct LastEval
	{
		bool valid = false, have_p2p = false;
		const float *center = nullptr, *mpole = nullptr;
		const float4 *csz = nullptr, *pos = nullptr;
		const int *mult = nullptr, *index = nullptr;
		int L = 0, ntot = 0, order = 0, shift = 0, real_bytes = 4;   // real_bytes: element size of mpole (8 after an evaluation with opts.far_fp64)
		long long n = 0, own0 = 0, own_n = 0;
		// for nbco_kd_potential: the final locals (element size real_bytes), the map back to the caller's order (used when scatter),
		// and whether the tree is the assembled global tree of a sharded evaluation
		const void *local = nullptr;
		const int *unsort = nullptr;
		bool scatter = false, sharded = false;
	} last_eval;
	DevBuf pot_c0, pot_slot;           // nbco_kd_potential: the far potential at the node centres, the per-leaf sums
	DevBuf pot_xa;                     // nbco_energy_tree (on the private context): scratch copy of the positions + the accelerations of its evaluation
	nbco_ctx *energy_child = nullptr;   // nbco_energy_tree, nbco_probe_tree: a private context for the tree they build (created on first use, freed by nbco_destroy)
	bool drifted = false;               // nbco_integrate has moved the particles since the last kd-tree evaluation (a scheme that ends on a drift): nbco_kd_probe refuses
	DevBuf probe_keys, probe_tmp;       // nbco_kd_probe / nbco_probe_tree: the probes' keys and sort permutation, their sort's scratch
	DevBuf bond_vec;                    // nbco_bond_solid: the bond vector records of its own pass 1; in the tree form (on the private context) the records in tree order
	DevBuf sk_part;                     // nbco_structure_factor: the partial sums of the particle ranges
	DevBuf tc_part;                     // nbco_time_corr: the records of the row ranges
	DevBuf md_part;                     // nbco_modes_record: the mode records of the particle ranges
	DevBuf ap_cnt, ap_state;            // nbco_aperture_*: the total and the levels of workgroup counts; the compacted state before it is copied back
	DevBuf sl_keys, sl_tmp, sl_tab, sl_part;   // nbco_slice_moments: keys and permutation, the sort's and the scan's scratch, the slice table and records, the chunk slabs
	// bookkeeping of the last evaluation
	nbco_kd_info info{};
	long long eval_counter = 0;
	bool tree_valid = false;
	long long tree_n = 0;
	int tree_order = 0;
	// profiling
	unsigned profiling = 0;   // bit i set: record events around phase i
	PhaseTimer timers[NBCO_PH_COUNT];

	int fail(int code, const std::string &msg) { err = msg; return code; }
	int fail_hip(hipError_t e, const char *what, const char *file, int line)
	{
		char buf[512];
		snprintf(buf, sizeof buf, "HIP error: %s (%s) at %s:%d", hipGetErrorString(e), what, file, line);
		err = buf;
		return NBCO_ERR_HIP;
	}
	int reserve(DevBuf &b, size_t bytes);
	void phase_begin(int ph);
	void phase_end(int ph);
};

// enqueue on the auxiliary stream for the lifetime of the scope (every launcher reads c->stream at call time)
struct StreamScope
{
	nbco_ctx *c;
	hipStream_t saved;
	StreamScope(nbco_ctx *c_, hipStream_t s) : c(c_), saved(c_->stream) { c->stream = s; }
	~StreamScope() { c->stream = saved; }
};

struct PhaseScope
{
	nbco_ctx *c;
	int ph;
	PhaseScope(nbco_ctx *c_, int ph_) : c(c_), ph(ph_) { c->phase_begin(ph); }
	~PhaseScope() { c->phase_end(ph); }
};

// opts.sync off for the lifetime of the scope: the calls a driver makes inside it do not drain the stream one by one, and what the
// driver does once the scope has ended (maybe_sync, f2d_done) sees the caller's setting again
struct SyncOff
{
	nbco_ctx *c;
	int saved;
	explicit SyncOff(nbco_ctx *c_) : c(c_), saved(c_->o.sync) { c->o.sync = 0; }
	~SyncOff() { c->o.sync = saved; }
};

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- launchers implemented in the kernel translation units -------------------------------------
// k_axpy.hip
int launch_step(nbco_ctx *c, float *b, const float *a, float ds, long long n3);
int launch_add_elastic(nbco_ctx *c, const float *p, float *a, long long n, const float *k, bool assign);
int launch_rescale(nbco_ctx *c, float *a, long long n3, const float *param);
int launch_gather3(nbco_ctx *c, float *dst, const float *src, const int *map, long long n, bool inverse);
int launch_copy(nbco_ctx *c, float *dst, const float *src, long long n3);
int launch_pack4(nbco_ctx *c, float4 *dst, const float *src3, long long n);
// fused integrator pieces
int launch_kick_drift(nbco_ctx *c, float *x, float *v, const float *a, float ks, float ds, long long n3);
int launch_finish_kick(nbco_ctx *c, const float *x, const float *v_in, float *v, float *a, const float *param, float ks, long long n, bool elastic);
// the drift in a uniform magnetic field (helix.hpp), alone and behind the kick K(ks)
struct Helix3;
int launch_drift_b(nbco_ctx *c, float *x, float *v, const Helix3 &h, long long n);
int launch_kick_drift_b(nbco_ctx *c, float *x, float *v, const float *a, float ks, const Helix3 &h, long long n);
// the Langevin bath step on the velocities (bath.hpp)
struct Bath3;
int launch_bath(nbco_ctx *c, float *v, const Bath3 &b, long long n);
// nbco_integrate.hip: the bath's checks and coefficients over the first `dim` axes
bool bath_valid(const nbco_bath *b, int dim);                                               // gamma, kT finite and not negative
bool bath_off(const nbco_bath *b, int dim);                                                 // every gamma exactly 0
int bath_coeffs_dim(const nbco_bath *b, double s, double *c1, double *c2, int dim);
// nbco_api.hip
// link: the leapfrog drivers' hand-off with the kd-tree evaluator (KdStepLink); the other evaluators take no part in it
int eval_kind(nbco_ctx *c, int kind, float *p, float *a, long long n, const float *param, KdStepLink *link = nullptr);
int maybe_sync(nbco_ctx *c);   // drains the stream with opts.sync
// k_direct.hip
int launch_direct(nbco_ctx *c, const float *p, float *a, long long n, const float *param, bool kahan);
// k_reduce.hip
int launch_minmax(nbco_ctx *c, const float *p3, long long n, float *out6_dev);
int launch_minmax4(nbco_ctx *c, const float4 *p4, long long n, float *out6_dev);
int launch_mean_relerr(nbco_ctx *c, const float *x, const float *ref, long long n, float *out_host);
int launch_pow_sum(nbco_ctx *c, const float *x, int expo, long long n, double *out3_host);
int launch_energy(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host);
// beam diagnostics; dim 3: buf holds fp32 xyz triplets, dim 2: fp64 xy pairs
int launch_beam_moments(nbco_ctx *c, const void *buf, int dim, long long n, nbco_moments *out_host);
int launch_hist(nbco_ctx *c, const void *buf, int dim, long long n, const nbco_hist_axis *axes_host, int naxes, unsigned long long *counts_dev);
// slice diagnostics (slice_diag_kernels.hpp): bins records to out_host; refuses a bad axis before any launch.  Synchronises.
int launch_slice_moments(nbco_ctx *c, const void *buf, int dim, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host, long long *n_outside_host);
// pair statistics (pair_stat_kernels.hpp): the window and the bins of a call, formed once on the host by the rule of include/nbco.h
struct PairBins
{
	int bins;
	double R2, width, inv_width;   // R2 = rmax * rmax, width = rmax / bins; inv_width only seeds the bin search
};
int launch_pair_hist(nbco_ctx *c, const void *p, int dim, long long n, const PairBins &pb, unsigned long long *counts_dev, double *nn2_dev);
// bond-orientational order (bond_order_kernels.hpp), exact forms; R2 = rmax * rmax.  With sum_host the call synchronises.
int launch_bond_order(nbco_ctx *c, const void *p, int dim, long long n, double R2, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host);
// the wave records of a bond-order call (`records` of them, on the device) -> *sum_host.  Synchronises.
int bond_summary_finish(nbco_ctx *c, const double *rec, long long records, long long n, int dim, nbco_bond_summary *sum_host);
// crystalline particles, exact forms: pass 1 alone (the bond vector records), and pass 2 over `vec_dev` or, if that is nullptr, over
// records of its own in c->bond_vec.  bond_solid_finish: the wave records of a solid pass -> *sum_host.  Synchronises.
int launch_bond_vectors(nbco_ctx *c, const float *p, long long n, double R2, int *nb_dev, double *vec_dev);
int launch_bond_solid(nbco_ctx *c, const float *p, long long n, double R2, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev, double *qbar_dev,
                      nbco_solid_summary *sum_host);
int bond_solid_finish(nbco_ctx *c, const double *rec, long long records, long long n, double dmin, int xi_min, nbco_solid_summary *sum_host);
// static structure factor (structure_factor_kernels.hpp): 2 K doubles to rho_dev; with n_used_host the call synchronises
int launch_structure_factor(nbco_ctx *c, const void *p, int dim, long long n, const nbco_sk_grid &g, double *rho_dev, long long *n_used_host);
// tracked trajectories (time_corr_kernels.hpp): frame `frame` of traj from the state buf, particle numbers from ids (device; NULL: the row);
// the raw sums of `lags` lags over the first `frames` frames of every row to out_dev.  Neither synchronises.
int launch_traj_record(nbco_ctx *c, const float *buf, long long n, const int *ids, float *traj, long long rows, int frames_cap, int frame, int stride);
int launch_time_corr(nbco_ctx *c, const float *traj, long long rows, int frames_cap, int frames, int lags, nbco_corr_lag *out_dev);
// collective modes (modes_kernels.hpp): the K records of the state buf to frame `frame` of series (with n_used_host the call synchronises);
// the raw sums of `lags` lags over the first `frames` frames of every k to out_dev, K * lags records (does not synchronise)
int launch_modes_record(nbco_ctx *c, const float *buf, long long n, const nbco_sk_grid &g, double *series, int frames_cap, int frame, long long *n_used_host);
int launch_mode_corr(nbco_ctx *c, const double *series, const nbco_sk_grid &g, int frames_cap, int frames, int lags, nbco_mode_lag *out_dev);
// aperture (aperture_kernels.hpp): the rule of a call, formed once on the host by include/nbco.h: w[a] = 1.0 / half[a]
struct ApRule
{
	int shape;
	double centre[3], half[3], w[3];
};
// the classification pass; tiles: keep the per-workgroup counts in c->ap_cnt for launch_aperture_compact.  Synchronises.
int launch_aperture_classify(nbco_ctx *c, const void *p, int dim, long long n, const ApRule &ap, bool tiles, long long *lost_host);
// behind a classification with tiles that found `lost` > 0 rows outside: buf = [pos n | vel n | acc n] -> [pos n' | vel n' | acc n'] through
// c->ap_state, the lost rows to the record, order_in -> order_out (n' entries) with the state; any of the last four may be NULL
int launch_aperture_compact(nbco_ctx *c, void *buf, int dim, long long n, long long lost, const ApRule &ap, void *lost_dev, int *lost_row_dev,
                            const int *order_in, int *order_out);
// k_fmm_kd.hip
int kd_pair_hist_tree(nbco_ctx *c, float *x, long long n, const PairBins &pb, unsigned long long *counts_dev, double *nn2_dev);
int kd_bond_order_tree(nbco_ctx *c, float *x, long long n, double R2, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host);
int kd_bond_vectors_tree(nbco_ctx *c, float *x, long long n, double R2, int *nb_dev, double *vec_dev);
int kd_bond_solid_tree(nbco_ctx *c, float *x, long long n, double R2, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev, double *qbar_dev,
                       nbco_solid_summary *sum_host);
int fmm_kdtree_eval(nbco_ctx *c, float *p, float *a, long long n, const float *param, KdStepLink *link = nullptr);
int kd_copy_out(nbco_ctx *c, int which, void *host_dst, long long host_bytes);
int kd_count_pairs(nbco_ctx *c, long long *out);
int kd_energy_fmm(nbco_ctx *c, long long n_own, double *half_phi_sum);
int kd_potential_check(nbco_ctx *c, long long n);
int kd_potential(nbco_ctx *c, long long n, const float *param, double *psi_dev, double *half_psi_sum);
int launch_energy_kin_ela(nbco_ctx *c, const float *buf, long long n, const float *param, double *out2_host);
int launch_probe_direct(nbco_ctx *c, const float *p, long long n, const float *t, long long m, const float *param, double *a, double *psi);
int kd_probe_check(nbco_ctx *c);
int kd_probe_last(nbco_ctx *c, const float *t, long long m, const float *param, double *a, double *psi);
int kd_probe_tree(nbco_ctx *c, float *x, long long n, const float *t, long long m, const float *param, double *a, double *psi);
// k_fmm_oct.hip
int fmm_oct_traceless_eval(nbco_ctx *c, float *p, float *a, long long n, const float *param, bool symmetric = false, int world = 1, int rank = 0,
                           long long *pbounds_host = nullptr);
int oct_copy_out(nbco_ctx *c, int which, void *host_dst, long long host_bytes);
// multi-GPU kd-domain sharding (k_fmm_kd.hip)
int kd_dist_layout(nbco_ctx *c, long long n_global, int world, int rank, nbco_dist_layout *out);
int kd_dist_partition(nbco_ctx *c, const float *state_all, long long n_global, int world, int rank, float *state_local);
int dpart_workspace(nbco_ctx *c, long long n_global, int world, long long *bytes);
int dpart_begin(nbco_ctx *c, float *state_local, long long n_global, int world, int rank, void *work, long long work_bytes, nbco_dist_step *out);
int dpart_next(nbco_ctx *c, nbco_dist_step *out);
int kd_finish_pending_order(nbco_ctx *c, float *p, long long n, KdStepLink *link);
int kd_turnaround(nbco_ctx *c, float *p, const float *param, float ks, float ds, bool elastic, long long n, KdStepLink *link, const float *root6 = nullptr,
                  const Helix3 *helix = nullptr, const Bath3 *bath_close = nullptr);
int kd_dist_turnaround(nbco_ctx *c, float *buf_local, long long n_local, const float *param, float ks, float ds, bool elastic);
int kd_dist_let_select(nbco_ctx *c, const void *csz_all, long long *counts);
int kd_dist_let_pack(nbco_ctx *c, const long long *counts_all, void *pos_send, void *mpole_send);
int kd_dist_let_finish(nbco_ctx *c, const long long *counts_all, const void *pos_recv, const void *mpole_recv, float *buf_local, float *a_local, const float *param);
int kd_dist_let_check(nbco_ctx *c);
int kd_dist_let_pack_capped(nbco_ctx *c, const long long *caps_out, void *pos_send, void *mpole_send);
int kd_dist_let_finish_capped(nbco_ctx *c, const long long *caps_in, const void *pos_recv, const void *mpole_recv, float *buf_local, float *a_local, const float *param);
int kd_dist_let_settle(nbco_ctx *c, int ok);
// the two stages of a domain's local evaluation; let: the LET exchange follows
int kd_dist_local_build(nbco_ctx *c, float *buf_local, long long n_local, void *pos_send, void *csz_send, bool let);
int kd_dist_local_upward(nbco_ctx *c, long long n_local, void *nodes_send, void *mpole_send, bool let);
int kd_dist_finish(nbco_ctx *c, const void *nodes_all, const void *pos_all, float *buf_local, float *a_local, const float *param);
int kd_dist_finish_traverse(nbco_ctx *c, const void *csz_all, const void *pos_all);
int kd_dist_finish_rest(nbco_ctx *c, const void *mpole_all, float *buf_local, float *a_local, const float *param);
// k_kdselect.hip
int kd_select_begin(nbco_ctx *c, int l0, bool zero = true, long long *words_a = nullptr, long long *words_b = nullptr);
int kd_select_level(nbco_ctx *c, int l, long long n, const float4 *pos_in, const int *unsort_in, float4 *pos_out, int *unsort_out,
                    float *lbound, float *rbound, int *splitdim, int *index, int *flag, bool warm = false, const KdRoot &root = KdRoot{});
// k_farfield.hip
int launch_upward_gen(nbco_ctx *c, int P, const float4 *pos, float *center, void *mpole, int *mult, const int *index, int L, int write_geom, int f64 = 0);
int launch_kd_centres(nbco_ctx *c, float *center, int *mult, int L, const float *lbound, const float *rbound, float4 *csz);
int launch_downward_gen(nbco_ctx *c, int P, const float *center, void *local, int L, int dom_d, int dom_g, int f64 = 0);
// (L: depth of the whole tree -- the high orders pick their loop form by a level's height above the leaves)
int launch_m2m_top_gen(nbco_ctx *c, int P, float *center, void *mpole, int *mult, int ltop, int L, int write_geom, int f64 = 0);
int launch_kd_centres_top(nbco_ctx *c, float *center, int *mult, int ltop, const float *lbound, const float *rbound, float4 *csz);
int launch_l2p_gen(nbco_ctx *c, int P, const float4 *pos, const float *center, const void *local, const float4 *near, const int *chunk_off,
                   const int *index, int mlt_max, const int *unsort, int scatter, const float *param, float *a, int have_near, long long n, int L,
                   long long own0, long long own_n, const int2 *sec_range = nullptr, const float4 *react = nullptr, long long react_cap = 0,
                   int react_stride = 32, int f64 = 0);
// k_m2l.hip
// mstride: reals per multipole tuple in `mpole` (0 = the offM(P) of the kd-tree layout; the symmetric octree evaluator keeps orders 0..P)
int launch_m2l_lanes(nbco_ctx *c, int P, const float4 *csz, const float *mpole, float *local, const uint64_t *keys, const int *start,
                     int shift, int ntot, int mstride = 0);
int launch_m2l_lanes_f64(nbco_ctx *c, int P, const float4 *csz, const double *mpole, double *local, const uint64_t *keys, const int *start,
                         int shift, int ntot, int mstride = 0);
