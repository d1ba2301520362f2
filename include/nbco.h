/* nbco.h -- C ABI of libnbco_hip.so, the MI355X (gfx950) force / integrate engine that drops in
 * behind the reference's evaluator / step / integrator function-pointer interface
 * (locuoco/coulomb_oscillators @ 2024_08_07, Simulation/).
 *
 * Conventions (they mirror the reference's GPU path):
 *   - every `p`, `a`, `b`, `buf`, `param` argument is a DEVICE pointer (main3.cu:699-704);
 *   - positions / velocities / accelerations are fp32 xyz triplets with a 12-byte stride, and a
 *     state buffer is [pos n | vel n | acc n] (kernel.cuh:67, integrator.cuh:24, main3.cu:655-657);
 *   - `param` is the 6-float array {xi/N, 0, 0, kx, ky, kz} of main3.cu:685-692; evaluators use
 *     param[0], the elastic term uses param+3;
 *   - evaluators overwrite `a`; tree evaluators may permute `p` (and then `p + 3n`, the
 *     velocities) unless opts.unsort is set (fmm_cart3_kdtree.cuh:1746-1760);
 *   - the reference's mutable globals (constants.cuh:36-52) become the explicit nbco_opts;
 *   - instead of gpuErrchk's exit() (kernel.cuh:52-65) every entry point returns an int status
 *     (0 = success) and nbco_last_error() gives the message;
 *   - work is enqueued on opts.stream; with opts.sync != 0 an evaluator returns after the stream
 *     has drained, as the reference's evaluators do (direct.cuh:243-244,
 *     fmm_cart3_kdtree.cuh:1762-1763).
 * There is no CPU fallback: every entry point fails with NBCO_ERR_HIP when no HIP device is usable.
 */
#ifndef NBCO_H
#define NBCO_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbco_ctx nbco_ctx;

enum {
	NBCO_OK = 0,
	NBCO_ERR_HIP = 1,        /* a HIP runtime call failed (message in nbco_last_error) */
	NBCO_ERR_ARG = 2,        /* invalid argument */
	NBCO_ERR_CAPACITY = 3,   /* interaction-list / traversal-frontier capacity exceeded
	                            (reference: printf + clamp, fmm_cart3_kdtree.cuh:552-566) */
	NBCO_ERR_UNSUPPORTED = 4
};

/* force evaluators: which f(p, a, n, param) an integrator or nbco_force drives */
enum {
	NBCO_EVAL_DIRECT = 0,         /* direct.cuh:104 `direct` / :171 `direct2` (LDS-tiled all pairs) */
	NBCO_EVAL_DIRECT_KAHAN = 1,   /* direct.cuh:233 `direct3` (compensated accumulation) */
	NBCO_EVAL_FMM_KDTREE = 2,     /* fmm_cart3_kdtree.cuh:1478 `fmm_cart3_kdtree` */
	NBCO_EVAL_FMM_TRACELESS = 3,  /* fmm_cart3_traceless.cuh:282 `fmm_cart3_traceless` */
	NBCO_EVAL_FMM_SYMMETRIC = 4   /* fmm_cart3_symmetric.cuh:413 `fmm_cart3` (uniform octree, symmetric multipoles) */
};

/* integrators of integrator.cuh:32-167 */
enum {
	NBCO_INTEG_EULER = 0,       /* symplectic_euler      :32 */
	NBCO_INTEG_PRE_EULER = 1,   /* pre_symplectic_euler  :50 */
	NBCO_INTEG_LEAPFROG = 2,    /* leapfrog              :68 */
	NBCO_INTEG_FORESTRUTH = 3,  /* forestruth            :100 */
	NBCO_INTEG_PEFRL = 4        /* pefrl                 :134 */
};

typedef struct nbco_opts {
	int   fmm_order;    /* constants.cuh:42 fmm_order, 1..10 */
	float tree_radius;  /* constants.cuh:43 tree_radius (used as given; the reference's CPU driver
	                       truncates it to int, fmm_cart3_kdtree.cuh:1775 -- callers that want that
	                       behaviour pass an integer value) */
	float eps2;         /* constants.cuh:39 EPS2 (softening squared) */
	int   coll;         /* constants.cuh:48 coll: 0 skips the P2P pass */
	int   unsort;       /* constants.cuh:48 b_unsort: restore the caller's particle order */
	float dens_inhom;   /* constants.cuh:50 dens_inhom */
	int   tree_L;       /* constants.cuh:44 tree_L (0 = derive from n and order) */
	int   tree_steps;   /* constants.cuh:45 tree_steps: rebuild the kd-tree every this many
	                       evaluations when unsort == 0.  1 = every evaluation, which is what the
	                       reference's CPU driver does (fmm_cart3_kdtree.cuh:1773-1929).  Setting a different
	                       value (nbco_set_opts) starts a new schedule: the next evaluation rebuilds -- which
	                       is also how a caller that puts a NEW state into an old context gets rid of the
	                       tree of the state before.  So does a change of fmm_order, dens_inhom, tree_L, unsort,
	                       p2p_mutual or track_order.  A change of far_fp64, of n or of the level count also makes
	                       the next evaluation rebuild, but does NOT restart the schedule: the context keeps
	                       counting its evaluations, and the next scheduled rebuild is the one whose number since
	                       the schedule began is a multiple of tree_steps (far_fp64 toggled before evaluation 3 of
	                       a tree_steps = 8 schedule: 3 rebuilds, 4..7 reuse its tree, 8 rebuilds).  tree_radius,
	                       m2l_first, coll and eps2 do not enter the tree build: changed between two evaluations
	                       they leave the tree and the schedule alone and take effect on the next evaluation's
	                       traversal and kernels. */
	int   m2l_first;    /* 0: leaf-leaf pairs go to P2P before the admissibility test (reference CPU
	                       traversal, fmm_cart3_kdtree.cuh:586-598); 1: admissibility first
	                       (reference GPU traversal <true>, :520-534) */
	int   sync;         /* != 0: evaluators return after the stream has drained */
	int   list_factor;  /* capacity of the P2P / M2L lists and of the traversal frontier, in units
	                       of the node count (reference: 1000, fmm_cart3_kdtree.cuh:1584-1586).  The
	                       lists are kept in 16 regions of list_factor * nodes / 8 pairs each; a region
	                       that runs full makes the evaluation grow the lists (list_grow) or return
	                       NBCO_ERR_CAPACITY with the caller's arrays untouched (default 48: ~10x the lists of
	                       the BASELINE runs at their start) */
	int   list_grow;    /* != 0 (default): a traversal that overflows its lists doubles the capacity (up to 64 x
	                       list_factor, and at most 2^31 pairs) and repeats the evaluation instead of failing:
	                       long runs change shape -- a ball that starts with 2.7e5 leaf pairs at N = 1M holds 6e6
	                       after 1200 steps, when a few ejected particles have stretched the outer leaves */
	int   far_fp64;     /* != 0: the FMM evaluators (nbco_fmm_kdtree, nbco_fmm_traceless, nbco_fmm_symmetric and the sharded
	                       nbco_dist_* forms) keep multipole / local expansions in double and do P2M, M2M, M2L, L2L and L2P
	                       in fp64 (BASELINE config 5: fp64 far field, fp32 P2P).  Positions, the tree geometry (centres,
	                       boxes, lists -- unchanged, bit for bit) and the near field stay fp32.  The fp32 far field overflows
	                       beyond N ~ 1e5 at orders 9-10 (r^-11 19!! ~ 1e40); this mode does not.
	                       No reference counterpart other than the -DSCAL=double build.  Sharded runs: the exchanged
	                       multipole blocks / LET node records are doubles (nbco_dist_layout sizes follow the option). */
	int   p2p_mutual;   /* != 0: nbco_fmm_kdtree evaluates every leaf pair of its near field once and applies the force to both
	                       leaves (Newton III), as the reference's GPU pair kernel does (fmm_cart3_kdtree.cuh:874-959) -- here
	                       without atomics: the second leaf's sums go to fixed-order "reaction" records, bit-reproducible.
	                       Leaves are taken as 1, 2 or 4 halves of up to 32 particles (nbco_kd_info.p2p_halves; sizes that fill
	                       the 16-lane rows too badly fall back to the one-directional kernel).  The pair kernel itself is 20 %
	                       faster (0.43 against 0.36 of the fp32 peak at N = 1M, p = 6), but writing, linking and summing the
	                       reaction records costs more than that: a step is 8 % slower.  Default 0: the one-directional kernel,
	                       whose sharded results also equal the single-GPU ones bit for bit. */
	int   track_order;  /* != 0: with unsort = 0 the context composes the permutations of all rebuilds since tracking started, so that
	                       NBCO_KD_ORDER maps a position of the (tree-ordered) state to the particle's number in the state the
	                       first tracked evaluation received: snapshots can be written in input order (the
	                       reference writes them in tree order, main3.cu:855-858) */
	void *stream;       /* hipStream_t; NULL = the null stream */
} nbco_opts;

/* reference defaults (constants.cuh:36-52), tree_steps = 1, m2l_first = 0, sync = 1 */
int nbco_opts_default(nbco_opts *o);

int nbco_create(nbco_ctx **out, const nbco_opts *o);   /* owns all scratch, like the reference's
                                                           function-local statics */
int nbco_destroy(nbco_ctx *c);
int nbco_set_opts(nbco_ctx *c, const nbco_opts *o);
int nbco_get_opts(const nbco_ctx *c, nbco_opts *o);
const char *nbco_last_error(const nbco_ctx *c);
int nbco_sync(nbco_ctx *c);

/* ---- basic kernels (kernel.cuh, appel.cuh) -------------------------------------------------- */
int nbco_step(nbco_ctx *c, float *b, const float *a, float ds, long long n);              /* kernel.cuh:100 step: b += a*ds */
int nbco_add_elastic(nbco_ctx *c, const float *p, float *a, long long n, const float *k);  /* kernel.cuh:145 add_elastic: a -= k o p (k == NULL: a -= p) */
int nbco_elastic(nbco_ctx *c, const float *p, float *a, long long n, const float *k);      /* kernel.cuh:198 elastic: a = -k o p */
int nbco_rescale(nbco_ctx *c, float *a, long long n, const float *param);                  /* appel.cuh:514 rescale: a *= param[0] */
int nbco_gather(nbco_ctx *c, float *dst, const float *src, const int *map, long long n);          /* kernel.cuh:229 dst[i] = src[map[i]] (xyz triplets) */
int nbco_gather_inverse(nbco_ctx *c, float *dst, const float *src, const int *map, long long n);  /* kernel.cuh:255 dst[map[i]] = src[i] */
int nbco_copy(nbco_ctx *c, float *dst, const float *src, long long n);                            /* kernel.cuh:281 */

/* ---- force evaluators: void f(VEC *p, VEC *a, int n, const SCAL *param) --------------------- */
int nbco_direct(nbco_ctx *c, const float *p, float *a, long long n, const float *param);   /* direct.cuh:104,171 */
int nbco_direct3(nbco_ctx *c, const float *p, float *a, long long n, const float *param);  /* direct.cuh:233 */
int nbco_fmm_kdtree(nbco_ctx *c, float *p, float *a, long long n, const float *param);     /* fmm_cart3_kdtree.cuh:1478 */
int nbco_fmm_traceless(nbco_ctx *c, float *p, float *a, long long n, const float *param);  /* fmm_cart3_traceless.cuh:282 */
int nbco_fmm_symmetric(nbco_ctx *c, float *p, float *a, long long n, const float *param);  /* fmm_cart3_symmetric.cuh:413 `fmm_cart3`, orders 1..9 */

/* evaluator `kind` on buf = [pos|vel|acc], followed by add_elastic(param+3) when elastic != 0:
 * compute_force (integrator.cuh:22) over the coulombOscillator* wrappers of main3.cu:47-69 */
int nbco_force(nbco_ctx *c, int kind, float *buf, long long n, const float *param, int elastic);

/* one step of integrator `scheme` with evaluator `kind` (+ elastic term), integrator.cuh:32-167.
 * dt and scale are the reference's long double arguments narrowed to double.  Refused before any launch, the state untouched:
 * NBCO_ERR_ARG for a null pointer, n <= 0, an unknown scheme or kind; NBCO_ERR_UNSUPPORTED for the kd-tree evaluator with
 * n > 0x7fffffff / 4. */
int nbco_integrate(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                   double dt, double scale, int elastic);
/* `steps` steps in one call: the loop body of main3.cu:840-870 between two snapshots.  The final state is bit-identical to
 * `steps` calls of nbco_integrate; leapfrog over the kd-tree evaluator (opts.unsort = 0, no order tracking) runs what lies
 * between two force evaluations -- tree order of x and v, elastic term, both half kicks, the drift, the next build's
 * prologue -- as ONE pass over the state instead of four.  Intermediate states are not observable.  Refused before any launch,
 * the state untouched, also with steps = 0: steps < 0 and everything nbco_integrate refuses. */
int nbco_integrate_steps(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                         double dt, double scale, int elastic, int steps);

/* ---- uniform magnetic field: the drift along a helix -------------------------------------------------------------------------
 * A uniform field Omega = (q/m) B adds the velocity-dependent force a_mag = v x Omega, which no kick v += a s expresses.  The flow
 * of "free motion in a uniform field" is known in closed form, and it replaces the drift D(s): x += v s of the five schemes, which
 * stay symplectic and keep their order; a free particle gyrates exactly at any step.  With w = |Omega|, n = Omega / w,
 * N v = n x v and theta = w s (s may be negative: PEFRL has negative drift coefficients)
 *
 *   R(s) = I - sin(theta) N + (1 - cos(theta)) N^2                          v <- R v
 *   A(s) = s I - ((1 - cos(theta)) / w) N + ((theta - sin(theta)) / w) N^2   x <- x + A v   (with the OLD v)
 *
 * (dA/ds = R, dR/ds = -w N R, which is dv/dt = v x Omega).  In 2-D Omega is a scalar, the field points out of the plane, and
 * N = [[0, -1], [1, 0]].  Omega is given in radians per unit of dt; `scale` multiplies kicks only and does not touch Omega.
 *
 * nbco_helix_matrices forms the two matrices, row-major, in double; host only, no GPU needed, and the one place they are formed:
 * the device calls below, `nbco3 -cpu` and the tests take them from it.  1 - cos(theta) is 2 sin^2(theta / 2) and theta - sin(theta)
 * a series below |theta| = 0.5, w and theta carry a correction term each, so every element is within a few ulp of the matrix's
 * largest at any theta; w = 0 gives R = I and A = s I exactly.  NBCO_ERR_ARG: a null pointer or a non-finite Omega or s. */
int nbco_helix_matrices(const double *omega3, double s, double *R9, double *A9);
int nbco_2d_helix_matrices(double omega, double s, double *R4, double *A4);
/* The helix drift of n particles on the context's stream.  The state is fp32: the matrices are narrowed to float once on the host,
 * and per component c, one rounding per fmaf, both lines from the old v:
 *   x'[c] = fmaf(A[c][2], vz, fmaf(A[c][1], vy, fmaf(A[c][0], vx, x[c])))
 *   v'[c] = fmaf(R[c][2], vz, fmaf(R[c][1], vy, R[c][0] * vx))
 * Every kernel that contains the drift uses this order.  Like a drift of nbco_integrate it marks the particles as moved since the
 * last kd-tree evaluation (nbco_kd_probe refuses).  NBCO_ERR_ARG: a null pointer, n < 0, a non-finite Omega or s. */
int nbco_drift_b(nbco_ctx *c, float *x, float *v, long long n, const double *omega3_host, double s);
/* nbco_integrate and nbco_integrate_steps with the drift replaced by the helix drift; K and F are as they are.  Omega = 0 exactly:
 * the call IS the counterpart, the bytes are identical.  Leapfrog fuses as there: the kick and the drift are one pass, and over the
 * kd-tree evaluator (opts.unsort = 0, no order tracking, steps >= 2) what lies between two force evaluations is one pass; the
 * final state of nbco_integrate_steps_b is bit-identical to `steps` calls of nbco_integrate_b.  Refused before any launch, the state
 * untouched: NBCO_ERR_ARG for a null omega3_host or a non-finite Omega, and everything the counterparts refuse.
 * Not offered: the nbco_dist_* path (nbco_dist_turnaround drifts straight) and non-uniform fields. */
int nbco_integrate_b(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                     double dt, double scale, int elastic, const double *omega3_host);
int nbco_integrate_steps_b(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                           double dt, double scale, int elastic, int steps, const double *omega3_host);

/* ---- Langevin bath: the exact friction-and-noise step ------------------------------------------------------------------------
 * Friction -gamma v plus noise at the temperature kT (laser or buffer-gas cooling) depends on v like the magnetic force, and no kick
 * expresses it.  The flow of dv = -gamma v dt + sqrt(2 gamma kT) dW alone, the Ornstein-Uhlenbeck process, is known in closed form,
 * and one step of any of the five schemes S(dt) becomes
 *
 *   O(dt/2, half = 0) . S(dt) . O(dt/2, half = 1)        (the form of Bussi and Parrinello, Phys. Rev. E 75, 056707)
 *
 * K, D (straight or helix) and F are as they are.  gamma[a] >= 0 is the friction rate of axis a per unit of dt, kT[a] >= 0 the bath
 * temperature of axis a in units of v^2 (mass 1).  The values are per axis on purpose: Doppler cooling acts along the beam; gamma[a] = 0
 * leaves axis a alone, kT[a] = 0 is pure cooling.  The 2-D calls read gamma[0..1] and kT[0..1] only.  HOST struct. */
typedef struct nbco_bath { double gamma[3]; double kT[3]; unsigned long long seed; } nbco_bath;
/* The coefficients of O(s), formed in double: c1 = exp(-gamma s), c2 = sqrt(kT * (-expm1(-2 gamma s))), so that a velocity of variance
 * sigma^2 leaves with c1^2 sigma^2 + c2^2 and kT is the fixed point at any s: the O step is exact, whatever gamma dt.  gamma = 0 gives
 * c1 = 1 and c2 = 0 exactly.  Host only, no GPU needed, and the one place they are formed: the device calls below, `nbco3 -cpu` and the
 * tests take them from it (the 3-D calls narrow them to float once).  NBCO_ERR_ARG: a null pointer, a non-finite or negative gamma, kT
 * or s. */
int nbco_bath_coeffs(const nbco_bath *bath, double s, double c1[3], double c2[3]);
/* O(s) alone on the velocities of n particles (xyz triplets, fp32), on the context's stream; returns as the evaluators do.  Per particle
 * row r and axis a, the whole numerical contract:
 *
 *   v' = (c1[a] * v) + (c2[a] * xi)      each product and the sum rounded once, in this order, no fused multiply-add
 *
 * so that numpy float32 arithmetic reproduces it bit for bit.  An axis whose narrowed coefficients are c1 = 1 and c2 = 0 (gamma = 0) is
 * not touched: its bytes stay whatever they are, and no noise is drawn for it.
 * The noise xi is counter-based and stateless, from Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85; ten rounds): key = (seed low word, seed high word), counter = (r, a + 4 half, tick low word, tick high word), with r the
 * particle's row in the state at the moment O is applied (after an evaluation's re-ordering) and tick the 64-bit step number.  The four
 * output words are summed as an integer, S = w0 + w1 + w2 + w3, and
 *   xi = (double) (int64) (S - 0x1FFFFFFFE) * 0x1.bb67ae8584caap-32      (sqrt(3) 2^-32; one rounding; in 3-D then narrowed to float)
 * That is a centred sum of four uniforms: mean 0, variance 1, kurtosis 2.7, and NOT a Gaussian: |xi| <= 3.47, there is no tail beyond.
 * Only the first two moments enter the stationary variance, so <v^2> -> kT holds exactly; a run that depends on rare large kicks
 * (escape over a barrier many kT high) needs another noise.
 * Consequences: a row's new v depends on (seed, tick, half, row, its old v) and on nothing else -- not on n, the launch shape or the
 * other rows; a second call with the same arguments draws the same noise; a run is reproducible and restartable from (state, tick).
 * An aperture that compacts the rows re-keys the noise, which is harmless: any independent stream serves.
 * The call does not move positions: it leaves the "moved since the last kd-tree evaluation" mark, the trees, the schedule and the
 * diagnostics' validity alone (nbco_kd_probe is still accepted after it).  Refused before any launch: NBCO_ERR_ARG for a null pointer,
 * n < 0, half not 0 or 1, a non-finite or negative gamma, kT or s; NBCO_ERR_UNSUPPORTED for n >= 2^31 (the row is one counter word). */
int nbco_bath_apply(nbco_ctx *c, float *v, long long n, const nbco_bath *bath_host, double s, int half, unsigned long long tick);
/* nbco_integrate(_b) and nbco_integrate_steps(_b) wrapped in the two half bath steps; omega3_host NULL: no magnetic field.  Step k of
 * nbco_integrate_steps_t uses tick0 + k.  Every gamma exactly 0 (any kT): the call IS nbco_integrate(_steps)(_b), byte for byte.
 * nbco_integrate_t is bit for bit the sequence nbco_bath_apply(dt/2, 0, tick), nbco_integrate(_b), nbco_bath_apply(dt/2, 1, tick), and
 * nbco_integrate_steps_t is bit for bit `steps` calls of nbco_integrate_t: leapfrog over the kd-tree evaluator fuses as in
 * nbco_integrate_steps, and the closing half of step k and the opening half of step k + 1 are part of the one pass between two force
 * evaluations (on the tree-order row); the opening half of the first step and the closing half of the last are passes of their own.
 * Refused before any launch, the state untouched: NBCO_ERR_ARG for a null bath_host, a non-finite or negative gamma or kT, a negative or
 * non-finite dt (with a bath), and everything the counterparts refuse; NBCO_ERR_UNSUPPORTED for n >= 2^31.
 * Not offered: the nbco_dist_* path, per-particle or position-dependent rates, a conserved "effective energy" bookkeeping. */
int nbco_integrate_t(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                     double dt, double scale, int elastic, const double *omega3_host, const nbco_bath *bath_host, unsigned long long tick);
int nbco_integrate_steps_t(nbco_ctx *c, int scheme, int kind, float *buf, long long n, const float *param,
                           double dt, double scale, int elastic, int steps, const double *omega3_host, const nbco_bath *bath_host,
                           unsigned long long tick0);

/* ---- reductions (reductions.cuh) -------------------------------------------------------------- */
int nbco_minmax(nbco_ctx *c, const float *p, long long n, float *minmax6_dev);           /* reductions.cuh:67 minmaxReduce2 */
int nbco_mean_relerr(nbco_ctx *c, const float *x, const float *ref, long long n, float *out_host);  /* reductions.cuh:99 relerrReduce2 (intent) */
int nbco_pow_sum(nbco_ctx *c, const float *x, int expo, long long n, double *out3_host);  /* reductions.cuh:590 powReduce */
/* total energy {kinetic, elastic, coulomb}; no reference counterpart */
int nbco_energy(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host);
/* the same with the Coulomb part from the interaction lists and multipoles of the LAST nbco_fmm_kdtree evaluation (which must
 * have been made at the positions in buf): near field pair by pair over the P2P list, far field by evaluating the multipole
 * expansions of the M2L sources at the particles (the reference's m2p_pot3, fmm_cart_base3.cuh:1474-1490), fp64, O(N log N)
 * instead of O(N^2).  Sharded runs: n = the domain's particles, every rank gets its share of the three sums.
 * The kd evaluation must be the context's LAST evaluator call: nbco_direct / nbco_direct3 / nbco_energy and the octree evaluators
 * (nbco_fmm_traceless, nbco_fmm_symmetric, nbco_fmm_oct_shard) reuse its position and list scratch, and after any of them this
 * call is refused with NBCO_ERR_ARG until nbco_fmm_kdtree has run again. */
int nbco_energy_fmm(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host);
/* The Coulomb part from the LOCAL expansions instead: psi_i = param[0] (near_i + c0[leaf] + sum_{1 <= |K| <= p} d^K / K! F[K]), with F
 * the leaf's final locals, d = x_i - c_leaf, c0 the far potential at the leaf centre (the node's M2L sources evaluated at its centre,
 * carried down the tree through the parents' locals) and near_i the fp64 pair sum over the leaf's P2P list (j != i by index;
 * skipped after an evaluation with coll = 0).  Inside a leaf -grad of it is the far-field force the evaluation applied, to
 * rounding.  One pass per node plus one per leaf, O(N); fp64, no atomics, fixed summation order (a second call returns the same
 * bits).  out3_host = {kinetic, elastic, coulomb}, coulomb = 1/2 sum psi_i.  phi_dev: NULL, or n doubles in DEVICE memory that
 * receive psi_i in the particle order of buf (through the kd unsort map after an unsort = 1 evaluation; after unsort = 0 buf is
 * in tree order).  Both calls synchronise and refuse bad arguments with NBCO_ERR_ARG before any launch.
 * nbco_kd_potential: on the lists, multipoles and locals of the LAST nbco_fmm_kdtree evaluation, under the preconditions of
 * nbco_energy_fmm (that evaluation was the context's last evaluator call, at the positions in buf, with this n; far_fp64,
 * m2l_first, p2p_mutual and a reused tree are all fine).  After a sharded (nbco_dist_*) evaluation: NBCO_ERR_UNSUPPORTED --
 * nbco_energy_fmm stays the tool there. */
int nbco_kd_potential(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host, double *phi_dev);
/* Self-contained: valid in any state of the context (after direct or octree evaluators, 2-D calls, or a drift -- Forest-Ruth and
 * PEFRL end a step on one), buf is neither modified nor reordered.  A private child context (created on first use, freed by
 * nbco_destroy) gets a scratch copy of the positions and one rebuild evaluation (unsort = 1, tree_steps = 1, track_order = 0,
 * p2p_mutual = 0, coll = 1, on this context's stream) at this context's fmm_order, tree_radius, eps2, dens_inhom, tree_L, far_fp64,
 * m2l_first, list_factor and list_grow (re-read on every call), then the potential pass.  This context's tree, rebuild schedule,
 * warm-select history, order tracking, nbco_kd_get_info and a valid nbco_energy_fmm are left exactly as they were. */
int nbco_energy_tree(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host, double *phi_dev);

/* ---- 3-D probes: field and potential of the charges at arbitrary points (no reference driver evaluates away from the particles).
 * All pointers except the context are DEVICE pointers.  p: n source positions as fp32 xyz triplets with a 12-byte stride (the head
 * of a state buffer works as it is); t: m probe positions in the same format; t == p is allowed, and neither array is modified or
 * reordered.  a_dev receives m xyz triplets of DOUBLE and psi_dev m doubles, both in the caller's probe order; either may be NULL
 * (not both), and an output that is NULL costs nothing.  Every source counts at every probe -- there is no self exclusion, because
 * a probe is not a particle:
 *   a_i   = param[0] sum_j d (|d|^2 + EPS2)^(-3/2),  d = t_i - x_j
 *   psi_i = param[0] sum_j   (|d|^2 + EPS2)^(-1/2)                 (a_i = -grad psi_i; no elastic term is added)
 * A probe on top of a source gets nothing from it in a and param[0] / sqrt(EPS2) in psi: with the default EPS2 = 1e-18 that self
 * term is 1e9 param[0], so callers who want the potential AT THE PARTICLES take nbco_energy_tree's phi_dev (j != i by index).
 * All arithmetic is fp64 over the widened floats; every sum has a fixed order and there are no atomics (a second call returns the
 * same bits).  The calls return as the evaluators do (opts.sync, opts.stream) and refuse before any launch, leaving the outputs as
 * they were: with NBCO_ERR_ARG a NULL p, t or param, n <= 0, m <= 0, both outputs NULL; with NBCO_ERR_UNSUPPORTED m >= 2^31 and an
 * n beyond what nbco_energy_tree takes.
 * nbco_probe: the exact sums, O(n m): the yardstick, and the tool for small sizes.  It reads p and t as they are and has no
 * scratch, so a valid nbco_energy_fmm / nbco_kd_potential stays valid. */
int nbco_probe(nbco_ctx *c, const float *p, long long n, const float *t, long long m, const float *param, double *a_dev, double *psi_dev);
/* Self-contained tree call, valid in any state of the context: nbco_energy_tree's private child context gets a scratch copy of p,
 * builds the kd-tree and runs the upward pass (kd_build + kd_upward only: no traversal, no lists, no fields; a flagged build is
 * settled behind the build with the evaluator's retry policy) at this context's fmm_order, tree_radius, eps2, dens_inhom, tree_L
 * and far_fp64 (re-read on every call), with unsort = 1, tree_steps = 1, on this context's stream; then the probes walk that tree
 * (below).  Reading the build's flag is one host round trip per call (a stream synchronisation behind the build), also with
 * opts.sync = 0; the walk itself is enqueued like any other call.  This context's tree, rebuild schedule, warm-select history, order tracking, nbco_kd_get_info and a valid
 * nbco_energy_fmm are left exactly as they were.  O(n log n + m log n). */
int nbco_probe_tree(nbco_ctx *c, const float *p, long long n, const float *t, long long m, const float *param, double *a_dev, double *psi_dev);
/* The walk alone, on the tree, the multipoles and the tree-ordered positions of the LAST nbco_fmm_kdtree evaluation, under the
 * preconditions of nbco_energy_fmm (that evaluation was the context's last evaluator call, and nbco_integrate has not ended a step on
 * a drift since: NBCO_ERR_ARG otherwise); far_fp64,
 * m2l_first, p2p_mutual, unsort 0 or 1 and a reused tree with stale boxes are all fine; after a sharded (nbco_dist_*) evaluation:
 * NBCO_ERR_UNSUPPORTED.  Every probe walks the tree depth first, left child first: a node that passes the evaluator's acceptance
 * test against the probe (as a node of size 0 and multiplicity 1; opts.tree_radius and opts.eps2 are read at call time, coll and
 * m2l_first are ignored) contributes its multipole expansion evaluated at the probe, a leaf is never expanded and always contributes
 * its particles pair by pair, any other node is opened.  A probe's result depends on the tree and its own position alone: the same bits in any probe set,
 * in any order.  last_eval, the lists and the rebuild schedule are untouched: a following nbco_energy_fmm or nbco_kd_potential
 * returns the bits it would have returned.  The truncation error is the evaluator's at the same order or below. */
int nbco_kd_probe(nbco_ctx *c, const float *t, long long m, const float *param, double *a_dev, double *psi_dev);

/* ---- introspection of the last kd-tree evaluation (parity tests, benchmarks) ----------------- */
typedef struct nbco_kd_info {
	int L, ntot, order, mlt_max;
	long long n;
	long long p2p_pairs;        /* unordered leaf pairs in the P2P list */
	long long m2l_pairs;        /* unordered node pairs in the M2L list */
	long long directed_p2p;     /* sum 2*m1*m2 over the list + sum m^2 over leaves */
	int rebuilt;                /* the last evaluation rebuilt the tree */
	int build_mode;             /* how this context builds trees: 0 = median selection with two radix passes + exact
	                               resolution of the pivot bucket (default), 1 = three radix passes (after a bucket held
	                               more candidates than the resolver takes), 2 = stable-sort chain (after a pivot had
	                               more exact ties than that).  The trees are identical; only the speed differs. */
	int p2p_halves;             /* near-field kernel of the last evaluation: 0 = one-directional; 1, 2, 4 = mutual (Newton III) with
	                               leaves taken as that many halves of up to 32 particles (opts.p2p_mutual) */
	long long warm_builds;      /* builds whose median selection ran ONE histogram pass per level around the previous build's pivots */
	long long warm_misses;      /* .. of which a window missed the median: the evaluation was repeated with the two-pass select */
	int real_bytes;             /* element size of NBCO_KD_MPOLE / NBCO_KD_LOCAL: 4, or 8 when the tree was built with opts.far_fp64 */
	int long_lists;             /* 1: the last evaluation sorted the long ranges of its near-field list (more than 512 entries of one
	                               target: leaves stretched by ejected particles, late in a run) with the kernel made for them */
} nbco_kd_info;
int nbco_kd_get_info(nbco_ctx *c, nbco_kd_info *info);

enum {
	NBCO_KD_MULT = 0, NBCO_KD_INDEX = 1, NBCO_KD_SPLITDIM = 2,   /* int[ntot] */
	NBCO_KD_CENTER = 3, NBCO_KD_LBOUND = 4, NBCO_KD_RBOUND = 5,  /* float[ntot][3] */
	NBCO_KD_MPOLE = 6,   /* float[ntot][offM], offM = p(p+1)(p+2)/6 */
	NBCO_KD_LOCAL = 7,   /* float[ntot][offL], offL = (p+1)^2 */
	NBCO_KD_P2P_LIST = 8, NBCO_KD_M2L_LIST = 9,                  /* int[pairs][2], unordered */
	NBCO_KD_UNSORT = 10, /* int[n]: tree position -> caller's index (of the last rebuild) */
	NBCO_KD_ORDER = 11   /* int[n]: position in the state -> particle number since opts.track_order was set (cumulative) */
};
int nbco_kd_copy(nbco_ctx *c, int which, void *host_dst, long long host_bytes);

/* ---- octree-traceless evaluator introspection (fmmTree, fmm_cart3_symmetric.cuh:24-30) ---------------------
 * Valid after nbco_fmm_traceless.  Cells are level-major (level l starts at (8^l - 1) / 7), row-major inside a
 * level; tuples are traceless, (order + 1)^2 reals per cell (orders 0..order); a real is a float, or a double
 * when the evaluation ran with opts.far_fp64 (nbco_oct_info.real_bytes). */
typedef struct nbco_oct_info {
	int L, ntot, order;
	int tpl;                /* target-group width of the near-field work units */
	long long n;
	long long m2l_entries;  /* directed (target, source) stencil entries with a non-empty source */
	long long p2p_groups, p2p_desc, p2p_chunks;
	int real_bytes;         /* 4 or 8: element size of NBCO_OCT_MPOLE / NBCO_OCT_LOCAL */
	int mpole_reals;        /* reals per tuple of NBCO_OCT_MPOLE: (order + 1)^2 after nbco_fmm_traceless (traceless, orders 0..order),
	                           (order + 1)(order + 2)(order + 3) / 6 after nbco_fmm_symmetric (symmetric layout, orders 0..order) */
} nbco_oct_info;
int nbco_oct_get_info(nbco_ctx *c, nbco_oct_info *out);
enum {
	NBCO_OCT_MULT = 0, NBCO_OCT_INDEX = 1,   /* int[ntot] (index: leaves only) */
	NBCO_OCT_CENTER4 = 2,                    /* float[ntot][4]: centre xyz, 0 */
	NBCO_OCT_MPOLE = 3, NBCO_OCT_LOCAL = 4,  /* real[ntot][(order+1)^2] */
	NBCO_OCT_KEYS = 5,                       /* uint32[n]: sorted cell keys (appel.cuh:44-55) */
	NBCO_OCT_PERM = 6                        /* uint32[n]: cell-order position -> caller's index */
};
int nbco_oct_copy(nbco_ctx *c, int which, void *host_dst, long long host_bytes);

/* ---- multi-GPU, uniform-octree evaluators: slabs of the sorted cell keys (fmm_cart3_traceless.cuh:196-254 and
 *      appel.cuh:320-381 are the single-GPU passes) ----
 * Every rank holds the whole state buf = [pos | vel | ..] and calls this with the same arguments but its own rank: the tree
 * and the upward pass are built redundantly (O(N)), M2L / L2L / P2P / L2P only for the rank's slab -- the leaf cells
 * [c_r, c_r+1) of the key order (x-layers), c_r = the first cell whose first particle is >= n r / world.  p and the
 * velocities behind it are re-ordered into cell order exactly as by nbco_fmm_traceless (identically on every rank);
 * a[3 i], i in [bounds_host[rank], bounds_host[rank + 1]) are written, the other accelerations are left alone --
 * bounds_host[0 .. world] (host) are the particle boundaries of all slabs, so the caller can all-gather the pieces.
 * Each written acceleration is bit-identical to the single-GPU nbco_fmm_traceless / nbco_fmm_symmetric. */
int nbco_fmm_oct_shard(nbco_ctx *c, float *p, float *a, long long n, const float *param, int symmetric, int world, int rank,
                       long long *bounds_host);

/* ---- multi-GPU: kd-domain sharding (the reference is single-GPU, the sharded tree is the
 *      balanced kd-tree of fmm_cart3_kdtree.cuh:109-137 whose level-log2(G) nodes hold N/G particles each) ----
 * One process per GPU, each with its own nbco_ctx.  This library never communicates: the caller moves
 * the two send buffers with an all-gather (RCCL) between nbco_dist_local and nbco_dist_finish.
 *
 *   nbco_dist_layout_query   sizes of the exchange buffers for (n_global, world, rank) under the current opts
 *   nbco_dist_partition      every `rebalance` steps: state_all = [pos N x 3 | vel N x 3] gathered from all
 *                            ranks (identical everywhere); runs the top log2(world) median splits and
 *                            writes the rank's domain [pos n_local x 3 | vel n_local x 3] to state_local
 *   nbco_dist_local          builds the domain's subtree over buf_local = [pos | vel | ..] (n_local
 *                            particles), upward pass; fills nodes_send (nodes_bytes) and pos_send (pos_bytes)
 *   nbco_dist_finish         nodes_all / pos_all = the world x gathered buffers in rank order; far + near
 *                            field for the own particles -> a_local (tree order); after a rebuild the
 *                            positions and velocities in buf_local are permuted into tree order, exactly
 *                            like nbco_fmm_kdtree with opts.unsort = 0
 * The accelerations equal those of a single-GPU nbco_fmm_kdtree over the n_global particles bit for bit
 * (rank r's particles are positions [r n_local, (r+1) n_local) of the single-GPU tree order).
 * Requirements: world a power of two, n_global % world == 0, n_local >= 4096, opts.unsort = 0. */
typedef struct nbco_dist_layout {
	int world, rank;
	int d;                 /* log2(world): global level of the domain roots */
	int L, L_local;        /* leaf level of the global tree, of the domain's subtree (L - d) */
	int ntot_local;        /* nodes of the domain's subtree */
	int order;
	long long n_global, n_local;
	long long nodes_bytes; /* per-rank node block: float4 csz[ntot_local], float mpole[ntot_local][offM] */
	long long pos_bytes;   /* per-rank position block: float4[n_local], tree order */
	long long csz_bytes;   /* the two parts of the node block on their own: traversal records (centre + squared box */
	long long mpole_bytes; /* diagonal) of the subtree's nodes, and their multipoles; csz_bytes + mpole_bytes = nodes_bytes */
	long long let_node_bytes; /* LET exchange: bytes of one node record {node id, multipole}, padded to 16 */
	int let_counts;           /* LET exchange: 64-bit values in one rank's count block (2 world + 2) */
} nbco_dist_layout;
int nbco_dist_layout_query(nbco_ctx *c, long long n_global, int world, int rank, nbco_dist_layout *out);
int nbco_dist_partition(nbco_ctx *c, const float *state_all, long long n_global, int world, int rank, float *state_local);
int nbco_dist_local(nbco_ctx *c, float *buf_local, long long n_local, void *nodes_send, void *pos_send);
/* The same re-partition WITHOUT gathering the state (no rank ever holds more than its own n_local particles): per level the
 * exact medians by a radix select whose histograms are summed across the ranks, pivot ties ordered by the stable-sort chain's
 * remaining keys, evalBox for the children, local partition; then one all-to-all of [pos | vel] by destination.  Top boxes,
 * split axes, the particles of every domain and their ORDER equal nbco_dist_partition's: both deliver a domain in the order of the
 * gathered state (source rank, then index in the source's state) -- the local build takes the local index as the last key of its
 * stable-sort chain, as the single-GPU build takes the index in its input.
 * The library never communicates: _begin / _next run the local stages and describe, in *next, the collective the caller runs
 * on its workspace (device memory, _workspace bytes) before calling _next again, until op == NBCO_COLL_DONE:
 *   ALLREDUCE_MIN_I32 / ALLREDUCE_SUM_I32   in place, `count` int32 at work + send_off
 *   ALLGATHER                               `count` bytes at work + send_off -> world x count bytes at work + recv_off (rank order)
 *   ALLTOALL                                records of row_bytes: rows_send[r] rows for rank r, consecutive from work + send_off;
 *                                           rows_recv[s] rows from rank s, consecutive at work + recv_off
 * state_local = [pos n_local x 3 | vel n_local x 3] is replaced by the rank's new domain.  world <= 32.  More than 64 particles
 * of one rank tying with a pivot: NBCO_ERR_UNSUPPORTED (nbco_dist_partition handles any input). */
enum {
	NBCO_COLL_DONE = 0,
	NBCO_COLL_ALLREDUCE_MIN_I32 = 1,
	NBCO_COLL_ALLREDUCE_SUM_I32 = 2,
	NBCO_COLL_ALLGATHER = 3,
	NBCO_COLL_ALLTOALL = 4
};
typedef struct nbco_dist_step {
	int op, row_bytes;
	long long send_off, recv_off, count;
	long long rows_send[64], rows_recv[64];
} nbco_dist_step;
int nbco_dist_repartition_workspace(nbco_ctx *c, long long n_global, int world, long long *bytes);
int nbco_dist_repartition_begin(nbco_ctx *c, float *state_local, long long n_global, int world, int rank, void *work,
                                long long work_bytes, nbco_dist_step *next);
int nbco_dist_repartition_next(nbco_ctx *c, nbco_dist_step *next);
/* nbco_dist_local in two halves, so that the all-gather of the positions can run beside the upward pass:
 * _build fills pos_send (subtree build), _upward fills nodes_send (multipoles). */
int nbco_dist_local_build(nbco_ctx *c, float *buf_local, long long n_local, void *pos_send);
int nbco_dist_local_upward(nbco_ctx *c, float *buf_local, long long n_local, void *nodes_send);
int nbco_dist_finish(nbco_ctx *c, const void *nodes_all, const void *pos_all, float *buf_local, float *a_local,
                     const float *param);
/* The same evaluation with the node block travelling in two all-gathers, so that the multipoles (224 of the 240 bytes per
 * node at order 6) are on the wire while the GPUs traverse:
 *   _local_geom        subtree build; fills pos_send (pos_bytes) and csz_send (csz_bytes)     -> all-gather both
 *   _local_mpole       upward pass; fills mpole_send (mpole_bytes)                            -> all-gather
 *   _finish_traverse   needs csz_all / pos_all (world x the blocks, rank order): global tree geometry + dual traversal;
 *                      returns with the work enqueued, pos_all must stay valid until _finish_rest has run
 *   _finish_rest       needs mpole_all: lists, near and far field, L2P -> a_local, buf_local as nbco_dist_finish
 * Results are identical to nbco_dist_local + nbco_dist_finish. */
int nbco_dist_local_geom(nbco_ctx *c, float *buf_local, long long n_local, void *pos_send, void *csz_send);
int nbco_dist_local_mpole(nbco_ctx *c, float *buf_local, long long n_local, void *mpole_send);
int nbco_dist_finish_traverse(nbco_ctx *c, const void *csz_all, const void *pos_all);
int nbco_dist_finish_rest(nbco_ctx *c, const void *mpole_all, float *buf_local, float *a_local, const float *param);
/* ---- the same evaluation with a locally-essential-tree (LET) exchange: a rank receives only the multipoles and positions
 *      its own interaction lists name, instead of every domain's whole block (north_star) ----
 * The dual traversal is symmetric and every rank runs it over the same global geometry, so the pairs a rank emits are also the
 * list of what the other ranks read of it: nothing is estimated.  Per evaluation:
 *   _let_local_geom   subtree build; fills csz_send (csz_bytes)                                  -> all-gather (16 B per node)
 *   _let_local_mpole  upward pass on the second stream (the multipoles stay on the device)
 *   _let_select       csz_all = world x csz_bytes: global geometry, traversal, selection; writes this rank's count block to
 *                     counts_send (DEVICE, let_counts 64-bit values: [2 r] node records / [2 r + 1] position records it
 *                     will send to rank r, [2 world] = 1 when its traversal ran out of list room, [2 world + 1] = 1 when its
 *                     tree build was flagged -- pivot ties beyond the resolver, a missed warm-select window)
 *                                                                                                  -> all-gather, copy to host
 *                     If any rank's block reports list overflow, every rank calls _let_select again (it repeats the traversal
 *                     with more room where needed, is a no-op elsewhere) and the blocks are gathered again.  If any reports a
 *                     flagged build, every rank starts the evaluation again from _let_local_geom (the flagged rank builds more
 *                     conservatively, the others reproduce their trees): the LET form needs no host round trip behind the build.
 *   _let_pack         counts_all = the gathered blocks on the HOST, [sender][let_counts]; fills pos_send (16 B records
 *                     {x, y, z, global particle index}) and mpole_send (let_node_bytes records {global node id, multipole}),
 *                     segments in receiver order                                                  -> two all-to-alls with
 *                     the splits counts_all[me][2 r + 1] / counts_all[me][2 r]
 *   _let_finish       pos_recv / mpole_recv = the received records in sender order; lists, near and far field, L2P ->
 *                     a_local, buf_local as nbco_dist_finish.  A guard checks every source of the sorted M2L and P2P lists
 *                     against what arrived; a miss is reported by the next _let_pack and by _let_check (which synchronises).
 * Accelerations are bit-identical to nbco_dist_finish and to the single-GPU nbco_fmm_kdtree. */
int nbco_dist_let_local_geom(nbco_ctx *c, float *buf_local, long long n_local, void *csz_send);
int nbco_dist_let_local_mpole(nbco_ctx *c, float *buf_local, long long n_local);
int nbco_dist_let_select(nbco_ctx *c, const void *csz_all, long long *counts_send);
int nbco_dist_let_pack(nbco_ctx *c, const long long *counts_all, void *pos_send, void *mpole_send);
int nbco_dist_let_finish(nbco_ctx *c, const long long *counts_all, const void *pos_recv, const void *mpole_recv, float *buf_local,
                         float *a_local, const float *param);
int nbco_dist_let_check(nbco_ctx *c);
/* The same exchange without the host round trip in the middle of the evaluation (nbco_dist_let_pack needs the gathered counts
 * on the host before anything behind it can be queued).  The caller sizes the segments from the counts of the evaluation BEFORE,
 * with head room -- caps_out[2 r] node records and caps_out[2 r + 1] position records for receiver r (0, 0 for itself), the
 * same numbers receiver r passes as caps_in[2 me], caps_in[2 me + 1] -- and exchanges whole segments:
 *   nbco_dist_let_select -> all-gather of the counts, copied to the host asynchronously
 *   nbco_dist_let_pack_capped(caps_out) -> the two all-to-alls with splits from the caps -> nbco_dist_let_finish_capped(caps_in)
 *   [everything queued; now wait for the counts]  ok = every counts_all[s][2 r], [2 r + 1] within the segment rank s sized for
 *   rank r, and no counts_all[s][2 world], [2 world + 1] flag  (the same matrix, hence the same verdict, on every rank)
 *   nbco_dist_let_settle(ok)
 * Records that do not fit a segment are dropped and free records are marked, so an attempt that is not ok has read nothing
 * out of bounds: it is void -- the accelerations are not to be used, buf_local holds the same particles (possibly reordered) --
 * and every rank repeats the evaluation from nbco_dist_let_local_geom, with nbco_dist_let_pack and exact sizes.  _settle also
 * reports the receiver guard of the attempt before (the guard of the last attempt: the next _settle / _pack, or _check). */
int nbco_dist_let_pack_capped(nbco_ctx *c, const long long *caps_out, void *pos_send, void *mpole_send);
int nbco_dist_let_finish_capped(nbco_ctx *c, const long long *caps_in, const void *pos_recv, const void *mpole_recv, float *buf_local,
                                float *a_local, const float *param);
int nbco_dist_let_settle(nbco_ctx *c, int ok);
/* Between the force evaluation of one leapfrog step of a sharded run and that of the next (any of the three forms above; the
 * accelerations a_local = buf_local + 6 n_local are those nbco_dist_*finish* wrote, WITHOUT the elastic term): one pass over the
 * domain's state that does  a -= k o x (elastic != 0), v += a dt scale / 2  [end of this step]  and  v += a dt scale / 2,
 * x += v dt  [start of the next]  -- the same operations with the same roundings as nbco_add_elastic + three nbco_step calls --
 * and the next local build's prologue.  The next call on this context must be the next evaluation's nbco_dist_local* /
 * nbco_dist_let_local_geom (a re-partition in between is fine: it discards the prologue). */
int nbco_dist_turnaround(nbco_ctx *c, float *buf_local, long long n_local, const float *param, double dt, double scale, int elastic);
/* The context's second stream (hipStream_t), on which the far-field chain runs and which alone reads mpole_all in
 * nbco_dist_finish_rest: a caller whose collective runs on its own stream can make THIS stream wait for the multipole
 * all-gather (hipStreamWaitEvent before calling _finish_rest) instead of the compute stream, so that the near-field
 * lists and the pair kernel do not wait for the multipoles either. */
int nbco_aux_stream(nbco_ctx *c, void **stream_out);

/* ---- per-phase device timing (HIP events on the context's stream) ---------------------------- */
enum {
	NBCO_PH_BUILD = 0, NBCO_PH_P2M_M2M = 1, NBCO_PH_TRAVERSE = 2, NBCO_PH_LISTS = 3, NBCO_PH_P2P = 4,
	NBCO_PH_M2L = 5, NBCO_PH_L2L = 6, NBCO_PH_L2P = 7, NBCO_PH_FINISH = 8, NBCO_PH_DIRECT = 9,
	NBCO_PH_AXPY = 10, NBCO_PH_COUNT = 11
};
int nbco_profile_enable(nbco_ctx *c, int mask);     /* bit i: record a pair of events around phase i; -1 = all, 0 = off */
int nbco_profile_reset(nbco_ctx *c);
int nbco_profile_get(nbco_ctx *c, int phase, double *total_ms, long long *launches);  /* syncs */

/* ---- checked build (libnbco_hip_checked.so, compiled with -DNBCO_CHECKED) -----------------------------------------
 * Same ABI; every index a kernel reads from a list (traversal frontier, pair lists, sorted entries, source descriptors,
 * work units) is range-checked on the device, counted per site and replaced by a harmless one instead of being used as
 * an address.  out8[site] = violations since the library was loaded (sites: 0 frontier, 1 list fill, 2 list sort,
 * 3 work unit, 4 source descriptor, 5 L2P); the production library returns NBCO_ERR_UNSUPPORTED.
 * NBCO_POISON=1 in the environment (either build) fills every new scratch allocation with 0x7f bytes. */
int nbco_debug_violations(nbco_ctx *c, long long *out8);

/* ---- initial condition (host only, no GPU needed) ----------------------------------------------
 * The reference's synthetic state: initGA (main3.cu:113-137) over std::mt19937_64(seed) after discard(discard)
 * (main3.cu:662-664: seed 5351550349027530206, discard 1248) -- 3n position deviates then 3n velocity deviates
 * from std::normal_distribution<float>, scaled by sigma_x / sigma_u per axis, centred and rescaled to exactly those
 * RMS values; with uniform_positions != 0 the positions are then redrawn uniformly in [-1, 1)^3 and centred, as
 * the -test mode does (initU, main3.cu:94-111,666).  host_state = [pos n x 3 | vel n x 3] floats in HOST memory. */
#define NBCO_REF_SEED 5351550349027530206ULL
#define NBCO_REF_DISCARD 1248ULL
int nbco_init_gaussian(float *host_state, long long n, const float *sigma_x3, const float *sigma_u3,
                       unsigned long long seed, unsigned long long discard, int uniform_positions);
/* Rows [first, first + count) of that state -- host_slice = [pos count x 3 | vel count x 3] -- bit for bit, without holding more
 * than the slice: the generator runs through the whole stream twice (the centring and the RMS rescaling of main3.cu:71-92 are
 * sums over all n particles).  What a rank of a multi-GPU run calls to draw its share of a system that fits no single host buffer
 * comfortably (N = 64M: 1.5 GB for the full state). */
int nbco_init_gaussian_slice(float *host_slice, long long n, long long first, long long count, const float *sigma_x3,
                             const float *sigma_u3, unsigned long long seed, unsigned long long discard, int uniform_positions);

/* ---- 2-D fp64 evaluators: the reference's `nbco` program (Simulation/main.cu, DIM 2, SCAL double) ----------------------------------
 * Conventions of this section:
 *   - positions / velocities / accelerations are fp64 xy pairs (16-byte stride); a state buffer is [pos n | vel n | acc n];
 *   - `param` is the 4-double DEVICE array {xi/N, 0, kx, ky} of main.cu:803-808: evaluators scale by param[0], the elastic term
 *     uses param + 2, and the FMM without near field (opts.coll == 0) multiplies a by param[1] (fmm_cart.cuh:527-528);
 *   - the pair law is a_i += d / (|d|^2 + EPS2), d = x_i - x_j (direct.cuh:23-26, appel.cuh:293-297);
 *   - options: the 2-D path reads fmm_order (1..10; higher orders return NBCO_ERR_ARG, the reference allows more), tree_radius
 *     (its integer part, >= 1), eps2 (the float widened to double), coll, dens_inhom, tree_L (0 = the formula of
 *     fmm_cart.cuh:415-417, else 2..15), sync and stream; it ignores every other field.  One context serves 2-D and 3-D calls.
 *   - nbco_2d_fmm leaves positions AND velocities (p + 2n) in cell order (fmm_cart.cuh:500-504); any n >= 1 is accepted (the
 *     reference asserts n > 128) and the tree has at most 15 levels below the root (2L <= 30). */
enum { NBCO_2D_EVAL_DIRECT = 0, NBCO_2D_EVAL_DIRECT_KAHAN = 1, NBCO_2D_EVAL_FMM = 2 };
int nbco_2d_direct(nbco_ctx *c, const double *p, double *a, long long n, const double *param);    /* direct.cuh:171 direct2, DIM 2 */
int nbco_2d_direct3(nbco_ctx *c, const double *p, double *a, long long n, const double *param);   /* direct.cuh:233 direct3 */
int nbco_2d_fmm(nbco_ctx *c, double *p, double *a, long long n, const double *param);             /* fmm_cart.cuh:395 fmm_cart; v at p + 2n */
/* integrator.cuh:22 compute_force: a = f(x), then a -= k o x when `elastic` (main.cu:85-89 coulombOscillatorFMM) */
int nbco_2d_force(nbco_ctx *c, int kind, double *buf, long long n, const double *param, int elastic);
/* integrator.cuh:32-167 (NBCO_INTEG_*): long double coefficient arithmetic, each step b += a * ds in double.  Arguments and, for
 * NBCO_2D_EVAL_FMM, the options nbco_2d_fmm would refuse are checked before the first launch: a refused step leaves buf as it was */
int nbco_2d_integrate(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                      int elastic);
/* `steps` calls of nbco_2d_integrate, bit for bit (main.cu:855-893 loop body) */
int nbco_2d_integrate_steps(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt,
                            double scale, int elastic, int steps);
/* The helix drift in 2-D (see nbco_drift_b; the field points out of the plane, omega is a scalar): fp64 state, double matrices from
 * nbco_2d_helix_matrices, x'[c] = fma(A[c][1], vy, fma(A[c][0], vx, x[c])), v'[c] = fma(R[c][1], vy, R[c][0] * vx), both from the
 * old v.  The integrators are nbco_2d_integrate / nbco_2d_integrate_steps with the drift replaced; omega = 0 exactly: the call is the
 * counterpart.  NBCO_ERR_ARG before any launch: a non-finite omega (or s) and everything the counterparts refuse.  Unlike nbco_drift_b
 * these drifts leave the context's "moved since the last kd-tree evaluation" mark alone, as the drift of nbco_2d_integrate does:
 * the mark belongs to the 3-D kd-tree (nbco_kd_probe reads it) and no 2-D call reads it. */
int nbco_2d_drift_b(nbco_ctx *c, double *x, double *v, long long n, double omega, double s);
int nbco_2d_integrate_b(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                        int elastic, double omega);
int nbco_2d_integrate_steps_b(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt,
                              double scale, int elastic, int steps, double omega);
/* The Langevin bath in 2-D (see nbco_bath_apply): fp64 state of xy pairs, gamma[0..1] and kT[0..1] of the bath, the coefficients of
 * nbco_bath_coeffs in double, v' = (c1[a] * v) + (c2[a] * xi) with each product and the sum rounded once and xi in double (not narrowed),
 * the same noise rule with a = 0, 1; numpy float64 arithmetic reproduces it bit for bit.  The integrators are nbco_2d_integrate(_steps)(_b)
 * wrapped in the two half steps (omega = 0: no field); gamma[0] = gamma[1] = 0 exactly: the call is its counterpart.  Refusals as in 3-D. */
int nbco_2d_bath_apply(nbco_ctx *c, double *v, long long n, const nbco_bath *bath_host, double s, int half, unsigned long long tick);
int nbco_2d_integrate_t(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt, double scale,
                        int elastic, double omega, const nbco_bath *bath_host, unsigned long long tick);
int nbco_2d_integrate_steps_t(nbco_ctx *c, int scheme, int kind, double *buf, long long n, const double *param, double dt,
                              double scale, int elastic, int steps, double omega, const nbco_bath *bath_host, unsigned long long tick0);
/* reductions.cuh:99 relerrReduce2: mean over particles of sqrt(|x_i - ref_i|^2 / (|ref_i|^2 + 1e-18)) (rel_diff1, :37-42;
 * main.cu:172 test_accuracy); syncs */
int nbco_2d_mean_relerr(nbco_ctx *c, const double *x, const double *ref, long long n, double *out_host);
/* ---- 2-D energy diagnostics (no reference driver computes an energy).  The pair law above is minus the gradient of a logarithmic
 * potential:
 *   phi_i   = sum_{j != i} 1/2 log(|x_i - x_j|^2 + EPS2)   (j != i by INDEX, not by distance: two coincident particles contribute
 *                                                           1/2 log EPS2 each)
 *   psi_i   = -param[0] phi_i                              (a_i = -grad psi_i, the evaluators' Coulomb term)
 *   kinetic = 1/2 sum |v_i|^2,  elastic = 1/2 sum (kx x_i^2 + ky y_i^2) with k = param + 2,  coulomb = 1/2 sum_i psi_i
 * With the elastic term on, kinetic + elastic + coulomb is the Hamiltonian of the flow nbco_2d_integrate integrates.
 * out3_host = {kinetic, elastic, coulomb} of buf = [pos n | vel n | ..]: only the first 4n doubles are read, buf is neither modified
 * nor reordered.  phi_dev: NULL, or n doubles in DEVICE memory that receive psi_i in the caller's particle order.  Both calls
 * synchronise, use only the 2-D scratch of the context (a valid nbco_energy_fmm stays valid), sum in a fixed order without atomics
 * (a second call returns the same bits) and refuse bad arguments with NBCO_ERR_ARG before any launch.
 * nbco_2d_energy: the Coulomb part from the exact all-pairs sum, O(N^2): the yardstick, and the tool for small N. */
int nbco_2d_energy(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev);
/* the Coulomb part from a quadtree FMM potential pass of its own, O(N): it builds the tree nbco_2d_fmm would build for these
 * positions (level formula, keys, stable sort, centroids, multipoles) over a scratch copy, so it needs no preceding evaluation and
 * is right after integrators that end a step on a drift.  Reads fmm_order (1..10), tree_radius, eps2, dens_inhom, tree_L and
 * stream, refuses exactly what nbco_2d_fmm refuses, and ignores coll: the near field is always summed.  The truncation error is
 * that of the field evaluation at the same order. */
int nbco_2d_energy_fmm(nbco_ctx *c, const double *buf, long long n, const double *param, double *out3_host, double *phi_dev);
/* ---- 2-D probes: field and potential of the sources at arbitrary points (no reference driver evaluates away from the particles).
 * All pointers except the context are DEVICE pointers.  p: n source positions as xy pairs (only the first 2n doubles are read);
 * t: m probe positions in the same format; t == p is allowed, and neither array is modified or reordered.  a_dev receives m xy
 * pairs and psi_dev m doubles, both in the caller's probe order; either may be NULL (not both), and an output that is NULL costs
 * nothing.  Every source counts at every probe -- there is no self exclusion, because a probe is not a particle:
 *   a_i   =  param[0] sum_j d / (|d|^2 + EPS2),  d = t_i - x_j
 *   psi_i = -param[0] sum_j 1/2 log(|d|^2 + EPS2)                  (a_i = -grad psi_i; no elastic term is added)
 * A probe on top of a source gets nothing from it in a and -param[0] 1/2 log EPS2 in psi.  So for t = p: a equals nbco_2d_direct's,
 * and psi equals the psi_i of nbco_2d_energy minus param[0] 1/2 log EPS2.
 * Both calls use only the 2-D scratch of the context (a valid nbco_energy_fmm stays valid), sum in a fixed order without atomics
 * (a second call returns the same bits), return as the evaluators do (opts.sync) and refuse with NBCO_ERR_ARG before any launch,
 * leaving the outputs as they were: a NULL p, t or param, n <= 0, m <= 0, n or m >= 2^31, both outputs NULL.
 * nbco_2d_probe: the exact sums, O(n m): the yardstick, and the tool for small sizes. */
int nbco_2d_probe(nbco_ctx *c, const double *p, long long n, const double *t, long long m, const double *param, double *a_dev,
                  double *psi_dev);
/* O(n + m log n): the quadtree nbco_2d_fmm would build for p (over a scratch copy, up to the multipoles; the level count comes
 * from n, not from m), then per probe the near field of its leaf and, at every level, the multipoles of its ancestor's M2L stencil
 * evaluated at the probe itself.  A probe outside the sources' bounding square is served through the border leaf nearest to it.
 * Reads fmm_order (1..10), tree_radius, eps2, dens_inhom, tree_L and stream, refuses exactly what nbco_2d_fmm refuses, and
 * ignores coll: the near field is always summed.  The truncation error is below the field evaluation's at the same order
 * (DESIGN 7a). */
int nbco_2d_probe_fmm(nbco_ctx *c, const double *p, long long n, const double *t, long long m, const double *param, double *a_dev,
                      double *psi_dev);
/* ---- beam diagnostics: phase-space moments and density maps of a state (the reference prints `emittances: x * u` once, at
 * initialisation, main.cu:774; nothing there bins particles).  buf = [pos n | vel n | ..] is a DEVICE pointer: fp32 xyz triplets
 * for the nbco_ calls, fp64 xy pairs for the nbco_2d_ calls.  Only positions and velocities are read; buf is neither modified nor
 * reordered.  Both passes are O(n), use only the transient reduction scratch of the context (a valid nbco_energy_fmm /
 * nbco_kd_potential / nbco_kd_probe stays valid and returns the bits it would have returned) and give the same bytes when called again.
 * Sharded runs: the calls describe the particles they are given.  Central moments of domains do not simply add (the centres
 * differ), so a sharded run gathers its state, or combines {n, mean, cov, m4} of the domains on the host with the usual shift formulas.
 *
 * nbco_beam_moments / nbco_2d_beam_moments: two passes.  The first takes the sums and the extrema of the 6 (4) coordinates and
 * leaves mean = sum / n on the device -- the coordinate's value itself where min == max, so that a constant axis has deviations of
 * exactly 0.  The second accumulates the products of d = (double) q - mean in fp64: the central form keeps the fourth moments of a
 * beam that sits off the origin, which raw power sums lose to cancellation.  Four launches and one synchronisation; every sum has a
 * fixed order and there are no float atomics.  The call synchronises and fills *out_host.  A NULL buf or out_host or n <= 0:
 * NBCO_ERR_ARG before any launch, *out_host left as it was.
 * Zero conventions: halo_q[k] = 0 where <d^2> = 0; emit[k] = halo[k] = 0 where I2 <= 0.  So n = 1, coincident particles and a
 * flat axis give zeros, never NaN. */
typedef struct nbco_moments {
	long long n; int dim;      /* 3 or 2 */
	double mean[6];            /* q = (x, y, z, vx, vy, vz); 2-D: (x, y, vx, vy), unused entries 0 */
	double min[6], max[6];     /* exact */
	double cov[6][6];          /* central: 1/n sum (q_a - mean_a)(q_b - mean_b), symmetric, both triangles filled */
	double m4[3][5];           /* per plane k = (x,vx), (y,vy), (z,vz), central, with d = q - mean_q, e = p - mean_p:
	                              <d^4>, <d^3 e>, <d^2 e^2>, <d e^3>, <e^4> */
	double emit[3];            /* sqrt(max(I2, 0)), I2 = <d^2><e^2> - <d e>^2 */
	double halo_q[3];          /* <d^4> / <d^2>^2 - 2          (0 for KV, 1 for a Gaussian) */
	double halo[3];            /* sqrt(3 I4) / (2 I2) - 2, I4 = <d^4><e^4> + 3 <d^2 e^2>^2 - 4 <d e^3><d^3 e>   (same values) */
} nbco_moments;
int nbco_beam_moments(nbco_ctx *c, const float *buf, long long n, nbco_moments *out_host);
int nbco_2d_beam_moments(nbco_ctx *c, const double *buf, long long n, nbco_moments *out_host);
/* Host only, no GPU needed: emit, halo_q and halo of *m from its cov and m4 (and dim), with the zero conventions above.  The two
 * calls above end with it; a caller that has formed the sums elsewhere (`nbco3 -cpu -moments`) gets the same derivation. */
int nbco_moments_derive(nbco_moments *m_host);
/* nbco_hist / nbco_2d_hist: counts of the particles over one (naxes = 1: a profile) or two (a map) phase-space coordinates.
 * axes_host[a] = {coord, bins, lo, hi} in HOST memory; counts_dev receives B + 1 values in DEVICE memory, B = bins0 * bins1
 * (bins1 = 1 for naxes = 1), axis 0 the slow index; counts[B] is the number of particles outside the window.  The buffer is
 * overwritten, not accumulated.  The bin rule, in fp64 over the widened coordinate: scale = bins / (hi - lo) (computed once on
 * the host); a particle is inside iff q >= lo && q < hi on every axis (a NaN is outside); b = (int) ((q - lo) * scale), clamped
 * to bins - 1.  Integer atomics only: the counts are exact and do not depend on the order of arrival.  The calls return as the
 * evaluators do (opts.sync, opts.stream) and refuse with NBCO_ERR_ARG before any launch, counts_dev untouched: NULL pointers,
 * n <= 0, naxes not 1 or 2, a coordinate the state does not have (Z and VZ in 2-D), bins < 1 or > 65536, B > 2^24, lo or hi not
 * finite, lo >= hi.  Radial coordinates and weights are not offered: a user folds the x-y map on the host. */
enum { NBCO_Q_X = 0, NBCO_Q_Y = 1, NBCO_Q_Z = 2, NBCO_Q_VX = 3, NBCO_Q_VY = 4, NBCO_Q_VZ = 5 };
typedef struct nbco_hist_axis { int coord; int bins; double lo, hi; } nbco_hist_axis;
int nbco_hist(nbco_ctx *c, const float *buf, long long n, const nbco_hist_axis *axes_host, int naxes, unsigned long long *counts_dev);
int nbco_2d_hist(nbco_ctx *c, const double *buf, long long n, const nbco_hist_axis *axes_host, int naxes, unsigned long long *counts_dev);
/* nbco_slice_moments / nbco_2d_slice_moments: how the beam differs along its length -- the moments above per slice along one
 * phase-space coordinate (slice emittance, slice centroid, rms size and halo per slice).  *axis_host = {coord, bins, lo, hi} in HOST
 * memory names the slicing coordinate (any NBCO_Q_* the state has) and the window; out_host receives bins records,
 * *n_outside_host the number of particles outside the window.  The call synchronises.
 * Membership: the slice of a particle is exactly nbco_hist's bin rule on that coordinate (a NaN there is outside); summed over the
 * slices, out_host[s].n plus *n_outside_host equals n.
 * A slice's record is what nbco_beam_moments means, applied to the slice's particles alone: n, dim, mean (over the slice, not over
 * the beam), the exact min / max, the central cov, the central m4 of every plane and, from nbco_moments_derive once per slice, emit /
 * halo_q / halo.  The min == max rule holds per slice -- a flat axis and a one-particle slice have deviations of exactly 0 -- and
 * so do the zero conventions.  An empty slice has n = 0 and the right dim; every other field is 0, never NaN.
 * Order and independence: the particles are grouped by slice with a stable sort of (slice, row) pairs, so a slice's particles
 * enter its sums in state order; a slice is cut into chunks of a fixed number of particles, one workgroup per chunk, and one wave
 * adds a slice's chunks in chunk order.  The shape of the summation depends on the slice's own population and on nothing else:
 * a second call returns the same bytes, and a slice's mean, cov and m4 are the same bytes whatever the other slices hold, however
 * many there are and wherever the window lies.  No float atomics.  A non-finite value in another coordinate of a particle reaches
 * that particle's slice only.  The sums behind the means are compensated -- carried as (sum, rounding error) pairs, the mean
 * (sum + error) / n, roughly twice the working precision -- so that a thin slice far from the origin (particles a bin's width
 * apart) keeps its fourth central moments, which answer an error eps of the mean with 4 eps <d^3>.  An infinite coordinate therefore
 * makes that coordinate's mean of its slice NaN (inf - inf in the compensation), where nbco_beam_moments would return inf.
 * State: the call uses scratch of its own.  The tree, the rebuild schedule, the warm-select history and the order tracking are
 * untouched, and a valid nbco_energy_fmm / nbco_kd_potential / nbco_kd_probe returns the bits it would have returned, also after
 * 2-D calls on the same context.
 * Refused before any launch, out_host and *n_outside_host left as they were: with NBCO_ERR_ARG a NULL pointer, n <= 0, a coordinate
 * the state does not have (Z and VZ in 2-D), bins < 1 or > 65536, lo or hi not finite, lo >= hi; with NBCO_ERR_UNSUPPORTED
 * n >= 2^31.  Sharded runs: the note above applies -- the call describes the particles it is given.
 * Not offered: radial slices, weights, two slicing axes. */
int nbco_slice_moments(nbco_ctx *c, const float *buf, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host,
                       long long *n_outside_host);
int nbco_2d_slice_moments(nbco_ctx *c, const double *buf, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host,
                          long long *n_outside_host);
/* nbco_pair_hist / nbco_pair_hist_tree / nbco_2d_pair_hist: how the particles sit relative to each other -- the histogram of the pair
 * distances below rmax (the raw counts behind g(r)) and, per particle, the squared distance to its nearest neighbour within rmax.
 * p holds n positions in DEVICE memory: fp32 xyz triplets (12-byte stride) in 3-D, fp64 xy pairs in 2-D; the head of a state buffer
 * works as it is.  p is neither modified nor reordered.  Either output may be NULL, not both; a NULL output costs nothing.
 * The pair rule, which is the whole numerical contract and uses no square root, so nothing depends on how a device rounds one:
 * d_a = (double) x_i[a] - (double) x_j[a]; r2 = (dx dx + dy dy) + dz dz (2-D: dx dx + dy dy), every product and sum rounded once in
 * this order, no fused multiply-add: the same bits for (i, j) and (j, i).  R2 = rmax * rmax (one product); a pair is inside iff
 * r2 < R2 (a NaN is outside).  width = rmax / bins (once, on the host); lower2(b) = e * e with e = (double) b * width; the bin of an
 * inside pair is the largest b in [0, bins - 1] with lower2(b) <= r2 (lower2 does not decrease with b, so it is unique).
 * counts_dev[0 .. bins) receives the number of UNORDERED pairs i < j per bin, counts_dev[bins] the pairs outside
 * (n (n - 1) / 2 less the others); the buffer is overwritten, not accumulated.  nn2_dev[i], in the caller's particle order, receives
 * min { r2_ij : j != i, the pair inside }, +infinity for a particle without a partner inside.  j != i is by INDEX: two coincident
 * particles are a pair with r2 = 0, in bin 0, and each has nn2 = 0.  Integer atomics only (a minimum over non-negative doubles is
 * an unsigned 64-bit minimum): counts and minima do not depend on the order of arrival, a second call returns the same bytes, and
 * THE TREE FORM RETURNS EXACTLY THE BYTES OF THE EXACT FORM -- the tree decides only what is skipped.
 * Refused before any launch, the outputs untouched: with NBCO_ERR_ARG a NULL c or p, n <= 0, both outputs NULL, rmax not finite or
 * <= 0, and with counts_dev given bins < 1, bins > 65536 or width * width below DBL_MIN (bins is ignored when counts_dev is NULL);
 * with NBCO_ERR_UNSUPPORTED n >= 2^31, and for the tree form an n beyond what nbco_energy_tree takes or a tree_L that leaves more
 * than 4096 particles per leaf (the kd-tree build finishes a leaf inside one workgroup's LDS).  The calls return as the
 * evaluators do (opts.sync, opts.stream) and read no other option, the tree form also dens_inhom and tree_L (and fmm_order, which
 * the level formula reads).  The exact forms count the pairs of a non-finite coordinate as outside; the tree form requires finite
 * coordinates, as the evaluator does.
 * State: the exact forms use no scratch of the context.  The tree form is self-contained like nbco_probe_tree: on the private
 * context it takes a scratch copy of p, builds the kd-tree over it (the build only: no multipoles, no traversal, no lists) and
 * walks it with the particles themselves, opening a node iff a particle of the wave is within rmax of its box.  This context's
 * tree, rebuild schedule, warm-select history, order tracking and nbco_kd_get_info stay as they were, and a following evaluation
 * or diagnostic returns the bits it would have returned.
 * Not offered: a form on the tree of the LAST EVALUATION (with tree_steps > 1 its boxes are stale, and pruning by them would drop
 * pairs), a 2-D tree form, weights, and the normalisation to g(r): a user divides by the shell volume and the density. */
int nbco_pair_hist(nbco_ctx *c, const float *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev);
int nbco_pair_hist_tree(nbco_ctx *c, const float *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev);
int nbco_2d_pair_hist(nbco_ctx *c, const double *p, long long n, int bins, double rmax, unsigned long long *counts_dev, double *nn2_dev);
/* nbco_bond_order / nbco_bond_order_tree / nbco_2d_bond_order: is the cloud ordered, and into which lattice -- the bond-orientational
 * order parameters of Steinhardt, Nelson and Ronchetti (Phys. Rev. B 28, 784): per particle the number of neighbours nb and q4, q6,
 * and a summary with their means and the global Q4, Q6; in 2-D |psi4| and |psi6| (the hexatic order).  g(r) is an angular average
 * and cannot tell bcc from fcc from hcp; these can, particle by particle.  p is as in nbco_pair_hist and is neither modified nor
 * reordered.
 * Neighbours, by the pair rule of nbco_pair_hist: d_a = (double) x_j[a] - (double) x_i[a]; r2 = (dx dx + dy dy) + dz dz (2-D:
 * dx dx + dy dy), every product and sum rounded once, no fused multiply-add; R2 = rmax * rmax; j is a neighbour of i iff
 * 0 < r2 && r2 < R2.  A NaN is outside, and two coincident particles are NOT neighbours of each other: a bond of length 0 has no
 * direction.  nb[i] is the number of neighbours, an exact integer, the same in every form.
 * 3-D, l = 4 and 6: u = d * (1 / sqrt(r2)) in fp64; S_lm(i) = sum over the neighbours of Y_lm(u_ij), Y_lm an orthonormal real basis of
 * the degree-l spherical harmonics (9 + 13 components); q_l(i) = sqrt(4 pi / (2l+1) * sum_m S_lm(i)^2) / nb[i], and 0 where nb[i] = 0,
 * never NaN.  q_l does not depend on the choice of basis: by the addition theorem q_l^2 = (1 / nb^2) sum_{j,k} P_l(u_ij . u_ik).
 * 2-D: psi_l(i) = |sum_j (u_x + i u_y)^l| / nb[i], the powers by repeated complex multiplication, no trigonometric call; 0 where nb = 0.
 * The harmonics are formed in one place (csrc/bond_order.hpp): polynomials in (x, y, z), the Legendre part in z times the real and
 * imaginary parts of (x + i y)^m by recurrence, no trigonometry and no table.  nbco_bond_harmonics exports them: host only, no GPU
 * needed; y4[0] and y6[0] are m = 0, entries 2m - 1 and 2m the cosine and sine parts of m.  u3 is taken as it is (not normalised).
 * NBCO_ERR_ARG: a null pointer or a non-finite component.  The device kernels, `nbco3 -cpu` and the tests take them from it. */
int nbco_bond_harmonics(const double u3[3], double y4[9], double y6[13]);
/* The summary: a HOST struct, filled when a non-NULL pointer is given; the call then synchronises. */
typedef struct nbco_bond_summary {
	long long n, bonds, isolated;   /* bonds = sum nb[i] (directed), isolated = #{nb[i] == 0} */
	int nb_max, dim;
	double q_mean[2];               /* mean of q4 / q6 (2-D: psi4 / psi6) over the particles with nb > 0; 0 if none */
	double Q[2];                    /* global: sqrt(4 pi/(2l+1) sum_m (sum_i S_lm(i))^2) / bonds; 2-D: |sum_i sum_j z^l| / bonds; 0 if bonds == 0 */
} nbco_bond_summary;
/* nb_dev receives n int32, q_dev n pairs {q4, q6} of doubles (2-D: {psi4, psi6}), both in the caller's particle order, both in DEVICE
 * memory.  Any of the three outputs may be NULL, not all three; a NULL output costs nothing.  Without sum_host the calls return as the
 * evaluators do (opts.sync, opts.stream).
 * Refused before any launch, the outputs untouched: with NBCO_ERR_ARG a NULL c or p, n <= 0, all outputs NULL, rmax not finite or <= 0;
 * with NBCO_ERR_UNSUPPORTED n >= 2^31, and for the tree form exactly the n and tree_L that nbco_pair_hist_tree refuses.  The exact
 * forms treat a non-finite coordinate as outside: that particle is isolated and nobody's neighbour; the tree form requires finite
 * coordinates, as the evaluator does.
 * Determinism: no float atomics; every sum has a fixed order, so a second call returns the same bytes.  The exact form meets a
 * particle's neighbours in index order, the tree form in the order of the tree's leaves, and the summary adds the particles in waves
 * of 64 of the caller's order and of the tree order respectively: nb IS EQUAL INTEGER FOR INTEGER IN BOTH FORMS, BUT q AND THE
 * SUMMARY AGREE ONLY TO ROUNDING (|delta q_l^2| below 1e-11 for nb <= 256), NOT BIT FOR BIT -- unlike nbco_pair_hist_tree.
 * State: the exact forms use only the transient reduction scratch of the context, as nbco_beam_moments does.  The tree form is
 * self-contained like nbco_pair_hist_tree: on the private context it takes a scratch copy of p, builds the kd-tree over it (the build
 * only) and walks it as that call does, with the harmonics of the bonds at the leaves.  In both forms this context's tree, rebuild
 * schedule, warm-select history, order tracking and nbco_kd_get_info stay as they were, and a following evaluation or diagnostic
 * returns the bits it would have returned.
 * Not offered: other l, the third-order invariants w_l, Voronoi or k-nearest neighbours instead of a cutoff, a 2-D tree form, sharded
 * runs, and a form on the tree of the LAST EVALUATION, for the reason given at nbco_pair_hist_tree.  (The neighbour-averaged q-bar_l
 * and solid-bond counting, a second pass over stored S_lm: nbco_bond_solid below.) */
int nbco_bond_order(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host);
int nbco_bond_order_tree(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host);
int nbco_2d_bond_order(nbco_ctx *c, const double *p, long long n, double rmax, int *nb_dev, double *q_dev, nbco_bond_summary *sum_host);
/* nbco_bond_vectors / nbco_bond_solid and their _tree forms: WHICH particles are crystalline, and how many.  q6 of a single particle is
 * noisy -- the distributions of a liquid and of a hot solid overlap -- so freezing, melting and grain growth are followed with two
 * quantities of a second pass over the stored S_lm: the number of SOLID BONDS xi_i of ten Wolde, Ruiz-Montero and Frenkel (J. Chem.
 * Phys. 104, 9932), the neighbours whose q6 vector is aligned with the particle's own, and the NEIGHBOUR-AVERAGED q-bar_l of Lechner and
 * Dellago (J. Chem. Phys. 129, 114707).  Neighbours, p, n and rmax are those of nbco_bond_order, in 3-D.
 * The bond vector record of a particle: 24 doubles (192 bytes).  [0, 9): q^_4m = S_4m / |S_4|, [9, 22): q^_6m = S_6m / |S_6|, with
 * |S_l| = sqrt(sum_m S_lm^2); [22], [23]: a_4, a_6 with a_l = |S_l| / nb, so q_l = sqrt(4 pi / (2l+1)) a_l.  nb = 0 or a norm of 0
 * leaves the 9 or 13 entries and a_l at 0, never NaN.
 * Coherence of the bond i-j: d6 = (((e0 f0 + e1 f1) + e2 f2) + ... + e12 f12) over e = record_i[9..22), f = record_j[9..22), every
 * product and every sum rounded once, left to right, no fused multiply-add: the same bits from either end, and what numpy gives with
 * elementwise products and sequential adds.  The bond is SOLID iff d6 > dmin (a NaN is not); xi[i] is the number of solid bonds of i.
 * Given the records, xi is an exact integer, the same in every form.  nbco_bond_coherence exports the rule (csrc/bond_order.hpp):
 * host only, no GPU needed; vec_i and vec_j are whole records.  NBCO_ERR_ARG: a null pointer.
 * Averaged order: T_lm(i) = a_l(i) q^_lm(i) + sum over the neighbours j of a_l(j) q^_lm(j) -- the particle first, then the neighbours in
 * the order the kernel meets them -- and q-bar_l(i) = sqrt(4 pi / (2l+1) sum_m T_lm^2) / (nb[i] + 1); 0 for a particle without
 * neighbours.  q-bar is specified to rounding only (|delta q-bar_l^2| below 1e-11 for nb <= 256 between the forms, given equal records).
 * nbco_bond_vectors / _tree: pass 1 of nbco_bond_order / _tree -- the same neighbours, the same order of summation -- with the records
 * as output: vec_dev receives n x 24 doubles, nb_dev n int32 (integer-equal to nbco_bond_order's), both in the caller's order in DEVICE
 * memory; either may be NULL, not both.
 * nbco_bond_solid / _tree: pass 2.  vec_dev: the records in the caller's order, read only; NULL: the call forms them itself by the same
 * form (the tree form then builds one tree and walks it twice, the records staying in tree order in scratch) and returns exactly the
 * bytes of the two-call sequence.  xi_dev receives n int32, qbar_dev n pairs {q-bar_4, q-bar_6} of doubles, nb_dev n int32, in the
 * caller's order; any of nb_dev, xi_dev, qbar_dev and sum_host may be NULL, not all four.  The summary is a HOST struct; with it the call
 * synchronises, without it the calls return as the evaluators do.  One record per wave of 64 particles and a sum of the records in a
 * fixed order; no floating-point atomics anywhere: a second call returns the same bytes.
 * Refused before any launch, the outputs untouched: what nbco_bond_order and its tree form refuse; dmin not finite; xi_min < 0.
 * State: as nbco_bond_order.  The exact forms use only transient scratch of the context, the tree forms run on the private context; this
 * context's tree, rebuild schedule, warm-select history, order tracking and nbco_kd_get_info stay as they were, and a following
 * evaluation or diagnostic returns the bits it would have returned.
 * Not offered: a coherence of l other than 6; the third-order invariants w_l; the largest connected crystalline cluster (connected
 * components over the solid bonds); 2-D forms; sharded runs; a form on the tree of the LAST EVALUATION. */
typedef struct nbco_solid_summary {
	long long n, bonds, isolated;   /* as in nbco_bond_summary */
	long long solid_bonds, n_solid; /* sum xi[i] (directed: even), #{xi[i] >= xi_min} */
	int xi_max, xi_min;             /* the largest xi[i]; xi_min as given */
	double dmin;                    /* as given */
	double qbar_mean[2];            /* mean of q-bar_4 / q-bar_6 over the particles with nb > 0; 0 if none */
} nbco_solid_summary;
int nbco_bond_coherence(const double vec_i[24], const double vec_j[24], double *d6_host);
int nbco_bond_vectors(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *vec_dev);
int nbco_bond_vectors_tree(nbco_ctx *c, const float *p, long long n, double rmax, int *nb_dev, double *vec_dev);
int nbco_bond_solid(nbco_ctx *c, const float *p, long long n, double rmax, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev,
                    double *qbar_dev, nbco_solid_summary *sum_host);
int nbco_bond_solid_tree(nbco_ctx *c, const float *p, long long n, double rmax, const double *vec_dev, double dmin, int xi_min, int *nb_dev, int *xi_dev,
                         double *qbar_dev, nbco_solid_summary *sum_host);
/* nbco_structure_factor / nbco_2d_structure_factor: the static structure factor -- what Bragg scattering off a Coulomb crystal and the
 * spatial spectrum of a beam's density (micro-bunching, density waves) measure.  For the wave vectors of a grid, k = (ix kstep[0],
 * iy kstep[1], iz kstep[2]) with ix = 0..h[0], iy = -h[1]..h[1], iz = -h[2]..h[2] (the half space ix >= 0: rho_{-k} is the conjugate;
 * the plane ix = 0 is stored whole), rho_dev receives rho_k = sum_j exp(i k . x_j) as K pairs of doubles {re, im} in DEVICE memory,
 * K = (h[0]+1)(2 h[1]+1)(2 h[2]+1), at index ((ix)(2 h[1]+1) + (iy + h[1]))(2 h[2]+1) + (iz + h[2]).  The 2-D form reads h[0..1]
 * and kstep[0..1]: K = (h[0]+1)(2 h[1]+1), index ix (2 h[1]+1) + (iy + h[1]), over the fp64 xy pairs.  S(k) = |rho_k|^2 / n_used is
 * the caller's.  p is as in nbco_pair_hist and is neither modified nor reordered; *g_host lies in HOST memory.  rho_dev is
 * overwritten, all K entries, not accumulated.  n_used_host may be NULL; with it the call synchronises and writes the number of
 * particles that counted, without it the call returns as the evaluators do (opts.sync, opts.stream).
 * The rule, which is the numerical contract, is written once, in csrc/structure_factor.hpp, for the kernels, nbco_sk_phase,
 * `nbco3 -cpu -sk` and `nbco -sk`: w_a = kstep[a] / 6.283185307179586 on the host; t_a = (double) x_a * w_a, the phase in cycles; a
 * particle counts iff every t_a is finite (for kstep below 1e269: iff every coordinate is finite) and otherwise contributes nothing
 * to any k; e_a = phase(t_a) from an exact reduction to |theta| <= pi/4 and fixed polynomials in fixed fma order -- no libm or ocml
 * trigonometry, the same operations on host and device, each component within 4 * 2^-53 of the true value, exact at the multiples
 * of a quarter turn; powers by repeated complex multiplication from (1, 0), the conjugate for negative indices; the term is
 * (e_y^iy e_z^iz) e_x^ix, the last factor applied one multiplication per ix; one fma order for the complex product.  rho at k = 0 is
 * exactly (n_used, 0).  nbco_sk_phase exports the phase: cs_host = {cos 2 pi t, sin 2 pi t}; host only, no GPU needed; NBCO_ERR_ARG
 * for a NULL cs_host or a non-finite t.
 * Determinism: every sum has a fixed order and there are no float atomics; the particles are cut into ranges by n and the grid alone,
 * never by the device, so a second call returns the same bytes, on any stream, in either opts.sync setting and on any card.
 * THE DEVICE AND `nbco3 -cpu -sk` AGREE ONLY TO ROUNDING, NOT BIT FOR BIT (they add the particles in different orders): within
 * n u (8 (h[0]+h[1]+h[2]+1) + n), u = 2^-53, of the exact sums of the rule's t, and far closer in practice.
 * Refused before any launch, the outputs untouched: with NBCO_ERR_ARG a NULL c, p, g_host or rho_dev, n <= 0, any h[a] < 0 or > 64,
 * any kstep[a] not finite or <= 0; with NBCO_ERR_UNSUPPORTED n >= 2^31.
 * State: the partial sums of the particle ranges live in scratch of the call's own (at most 256 MiB: the number of ranges is bounded
 * by it, no grid is refused for it).  The tree, the rebuild schedule, the warm-select history, the order tracking, nbco_kd_get_info
 * and a valid nbco_energy_fmm / nbco_kd_potential / nbco_kd_probe stay as they were; a following call returns the bits it would
 * have returned.
 * Not offered: arbitrary k lists, weights other than the velocities (the current modes and the time series behind the dynamic
 * S(k, omega): nbco_modes_record, nbco_mode_corr), the shell average S(|k|) and the division by n (fold on the host), and sharded
 * runs (add the rho of the shards). */
typedef struct nbco_sk_grid { int h[3]; double kstep[3]; } nbco_sk_grid;      /* HOST memory; 2-D reads [0..1] */
int nbco_structure_factor(nbco_ctx *c, const float *p, long long n, const nbco_sk_grid *g_host, double *rho_dev, long long *n_used_host);
int nbco_2d_structure_factor(nbco_ctx *c, const double *p, long long n, const nbco_sk_grid *g_host, double *rho_dev, long long *n_used_host);
int nbco_sk_phase(double t, double *cs_host);
/* ---- time correlations of individual particles: is the cloud solid?  The mean-square displacement (a plateau in a solid, linear
 * growth in a liquid; the Lindemann ratio, the diffusion constant), its non-Gaussian parameter alpha2 (caging and hopping) and the
 * velocity autocorrelation function (whose host-side transform is the spectrum of plasma and trap oscillations, the tune spread of
 * a space-charge-dominated beam).  3-D only.
 * nbco_traj_record keeps identity over time.  The caller owns a DEVICE buffer traj of rows x frames_cap x 6 floats; row r belongs to
 * particle number r * stride, and frame f of row r is the six floats x y z vx vy vz at traj[(r * frames_cap + f) * 6 ..].  buf is a
 * state (pos at buf, vel at buf + 3 n).  The call fills frame `frame` of every row with NaN (the quiet NaN 0x7fc00000) and then, for
 * every state row i with particle number p where p % stride == 0 and p / stride < rows, writes the six state floats with their bits
 * to row p / stride.  p is ids_dev[i] where ids_dev (int[n], DEVICE memory; for callers who compact or permute the state
 * themselves; a negative number is skipped, a number given twice is the caller's error) is not NULL; otherwise the context's order
 * map where tracking is live -- the condition of nbco_kd_copy(NBCO_KD_ORDER): opts.track_order and a tracked evaluation of these n
 * particles behind it; the map is read where it lies, on the device, and nbco_aperture_apply has already compacted it -- and
 * otherwise i.  A particle that an aperture has removed simply stops being written: its later frames stay NaN.
 * Refused with NBCO_ERR_ARG before any launch, traj untouched: a NULL c, buf or traj; n <= 0, rows <= 0, stride < 1; frame outside
 * [0, frames_cap); opts.track_order set without a tracked evaluation of these n particles and without ids_dev (the map does not
 * describe this state).  NBCO_ERR_UNSUPPORTED for n >= 2^31.
 * The call reads the state and the map and changes nothing in the context: tree, rebuild schedule, warm-select history, order map and
 * every valid diagnostic return the bits they would have returned.  Two passes on opts.stream; it returns as the evaluators do
 * (opts.sync) and never synchronises of its own.
 * nbco_time_corr sums over all rows and all origins t with t + tau < frames, for tau = 0 .. lags - 1; 1 <= lags <= frames <= frames_cap
 * and frames <= 2048.  A (row, t, tau) counts only if all twelve floats of frames t and t + tau are finite.  out_dev (DEVICE memory,
 * `lags` records, overwritten) receives per lag, as RAW SUMS -- the division is the caller's, or nbco_time_corr_derive's:
 *   pairs   the number of (row, t) that counted, an exact integer;
 *   dx2[c]  the sum of D_c^2, D_c = (double) x_c(t + tau) - (double) x_c(t);
 *   r4      the sum of (D_x^2 + D_y^2 + D_z^2)^2;
 *   vv[c]   the sum of v_c(t) v_c(t + tau).
 * The rule, which is the numerical contract, is written once, in csrc/time_corr.hpp, for the kernel, `nbco3 -cpu -corr` and
 * nbco_time_corr_derive: every float widened first; D_c one subtraction; dx2[c] <- fma(D_c, D_c, dx2[c]);
 * r2 = fma(D_z, D_z, fma(D_y, D_y, D_x * D_x)); r4 <- fma(r2, r2, r4); vv[c] <- fma(v_c(t), v_c(t + tau), vv[c]).
 * Determinism: a (row, tau) adds its terms in increasing t; the rows are cut into ranges by (rows, frames, lags) alone, a range's
 * rows are taken in a fixed order and the ranges are added in index order; no float atomics: a second call returns the same bytes,
 * on any stream and on any card.  THE DEVICE AND `nbco3 -cpu -corr` AGREE ONLY TO ROUNDING (they add the rows in different orders):
 * with u = 2^-53, dx2 and r4 within (pairs + 8) u of the exact sums of the rule's terms, relative; vv within (pairs + 8) u times the
 * sum of the |terms|; pairs equal.
 * Refused with NBCO_ERR_ARG before any launch, out_dev untouched: a NULL c, traj or out_dev; rows <= 0; lags < 1, lags > frames,
 * frames > frames_cap, frames > 2048.
 * State: the records of the row ranges live in scratch of the call's own (at most 64 MiB).  The tree, the rebuild schedule, the
 * warm-select history, the order tracking, nbco_kd_get_info and every valid diagnostic stay as they were.
 * nbco_time_corr_derive (host only, no GPU needed, like nbco_moments_derive): `in` and `out` in HOST memory; per lag the eight
 * doubles msd_x msd_y msd_z msd alpha2 vacf_x vacf_y vacf_z with msd_c = dx2[c] / pairs, msd = (msd_x + msd_y) + msd_z,
 * alpha2 = 3 <r^4> / (5 <r^2>^2) - 1 and vacf_c = vv[c] / pairs.  pairs == 0 gives eight zeros and msd == 0 (lag 0, particles at rest)
 * alpha2 = 0: never NaN.  NBCO_ERR_ARG for a NULL pointer or lags < 0.
 * Not offered: the 2-D state (nbco_2d_fmm leaves it in cell order and keeps no order map), sharded runs, correlations between
 * different particles (the collective ones, F(k, tau) and the current correlations behind S(k, omega): nbco_modes_record,
 * nbco_mode_corr), more than 2048 frames, and the Fourier transform of the VACF (a few thousand points: host). */
typedef struct nbco_corr_lag { double dx2[3]; double r4; double vv[3]; unsigned long long pairs; } nbco_corr_lag;   /* 64 bytes */
int nbco_traj_record(nbco_ctx *c, const float *buf, long long n, const int *ids_dev, float *traj, long long rows, int frames_cap, int frame, int stride);
int nbco_time_corr(nbco_ctx *c, const float *traj, long long rows, int frames_cap, int frames, int lags, nbco_corr_lag *out_dev);
int nbco_time_corr_derive(const nbco_corr_lag *in, int lags, double *out);
/* ---- collective dynamics: the time correlations of the density and current modes of the cloud -- what one-component-plasma and
 * Coulomb-crystal work reads off a run: the intermediate scattering function F(k, tau), whose host-side transform is S(k, omega)
 * (plasmon and trap-mode dispersion, the lifetime of a Bragg peak), the longitudinal current correlation C_L(k, tau) (the plasmon
 * peak and its damping) and the transverse one C_T(k, tau) (shear modes, which a fluid damps and a solid carries).  3-D only.  No
 * particle identity is needed: opts.track_order may stay off.
 * nbco_modes_record writes the MODE RECORD of every wave vector of the grid of nbco_structure_factor -- eight doubles {rho.re, rho.im,
 * jx.re, jx.im, jy.re, jy.im, jz.re, jz.im}, rho_k = sum_j exp(i k . x_j), j_k = sum_j v_j exp(i k . x_j) -- of the state buf (pos at
 * buf, vel at buf + 3 n, as for nbco_traj_record) to series_dev[(k * frames_cap + frame) * 8 ..], k nbco_structure_factor's index:
 * the caller owns a DEVICE buffer of K x frames_cap x 8 doubles in which the series of one k is contiguous; frames_cap = 1, frame = 0
 * is a plain snapshot of K records.  All K records of that frame are overwritten, not accumulated; nothing else in the buffer is
 * touched.  n_used_host may be NULL; with it the call synchronises and writes the number of particles that counted, without it the
 * call returns as the evaluators do (opts.sync, opts.stream).
 * The rule, which is the numerical contract, is written once, in csrc/modes.hpp, for the kernels, nbco_mode_corr_ref,
 * nbco_mode_corr_derive and `nbco3 -cpu -modes`.  Phases, powers and the term w of (ix, iy, iz) are those of nbco_structure_factor.  A
 * particle counts iff every t_a is finite and all three velocity floats are finite, and otherwise adds nothing to any of the four
 * sums.  Per counted particle and k: rho.re += w.re; rho.im += w.im; j_c.re <- fma(v_c, w.re, j_c.re); j_c.im <- fma(v_c, w.im, j_c.im),
 * v_c the float widened to double.  rho at k = 0 is exactly (n_used, 0) and j at k = 0 has the imaginary part exactly 0.  The rho
 * part NEED NOT have the bytes of nbco_structure_factor (that call counts by the positions alone and tiles differently); both lie
 * within its bound.  j_c lies within u V_c (8 (h[0]+h[1]+h[2]+1) + 2 n + 2) of the exact sum, V_c the sum of |v_c|, u = 2^-53.
 * Determinism is that of nbco_structure_factor: the particle ranges depend on n and the grid alone, every sum has a fixed order and
 * there are no float atomics: a second call returns the same bytes, on any stream, in either opts.sync setting and on any card.
 * `nbco3 -cpu -modes` records in index order and AGREES WITH THE DEVICE ONLY TO ROUNDING.
 * Refused before any launch, the outputs untouched: what nbco_structure_factor refuses (series_dev in the place of rho_dev), and with
 * NBCO_ERR_ARG frames_cap < 1 and a frame outside [0, frames_cap).
 * State: the records of the particle ranges live in scratch of the call's own (at most 256 MiB).  The tree, the rebuild schedule, the
 * warm-select history, the order map, nbco_kd_get_info and every valid diagnostic stay bit for bit as they were.
 * nbco_mode_corr sums, for every k and every lag tau = 0 .. lags - 1, over the origins t with t + tau < frames, in increasing t, and
 * writes record (k, tau) to out_dev[k * lags + tau] (DEVICE memory, K * lags records, overwritten); 1 <= lags <= frames <= frames_cap
 * and frames <= 1024.  With a = record(t), b = record(t + tau), k_c = (double) i_c * kstep[c] and P(r) = k . j of r,
 * P(r).re = fma(k_z, r.jz.re, fma(k_y, r.jy.re, k_x * r.jx.re)) and likewise .im, a record holds as RAW SUMS:
 *   rr      fma(a.rho.im, b.rho.im, fma(a.rho.re, b.rho.re, rr)): the sum of Re[rho(t + tau) conj rho(t)];
 *   jj      six fma in the order x.re, x.im, y.re, y.im, z.re, z.im: the sum of Re[j(t + tau) . conj j(t)];
 *   ll      fma(P(a).im, P(b).im, fma(P(a).re, P(b).re, ll)): the sum of Re[P(t + tau) conj P(t)];
 *   s0, s1  the complex sums of a.rho and of b.rho, plain additions (the means the connected part subtracts);
 *   pairs   frames - tau, an exact integer.
 * There is no finiteness test: a record written by nbco_modes_record is finite, and a non-finite one supplied by the caller
 * propagates.  A (k, tau) is formed by one lane from start to end; there is no sum across lanes or workgroups.
 * nbco_mode_corr_ref (host only, no GPU needed) is the same rule in plain loops over series_host and out_host in HOST memory:
 * THE DEVICE AND THIS CALL RETURN THE SAME BYTES for the same series.
 * Refused with NBCO_ERR_ARG before any launch, out untouched: a NULL pointer; any h[a] < 0 or > 64, any kstep[a] not finite or <= 0;
 * lags < 1, lags > frames, frames > frames_cap, frames > 1024.
 * nbco_mode_corr_derive (host only, compiled without contraction, like nbco_time_corr_derive): `in` K * lags records and `out`
 * K * lags * 4 doubles in HOST memory; per (k, lag), with m = (double) pairs, d = m * n_norm and k2 = (k_x^2 + k_y^2) + k_z^2,
 *   F   = rr / d;
 *   F_c = (rr - (s1.re * s0.re + s1.im * s0.im) / m) / d, the connected part: the rho_k of a trapped cloud has a large static
 *         mean, its form factor;
 *   C_L = ll / (k2 * d);
 *   C_T = (jj - ll / k2) / (2 d).
 * n_norm is the caller's particle number (the mean of rho.re at k = 0 over the frames).  k2 == 0 gives C_L = C_T = 0; pairs == 0 or
 * n_norm <= 0 gives four zeros: never NaN for finite input.  NBCO_ERR_ARG for a NULL pointer, lags < 0 or an h outside 0..64.
 * Not offered: the 2-D programs, sharded runs, lists of k, the imaginary parts of the correlations, the transform to omega (a few
 * thousand points per k: host) and more than 1024 frames per call. */
typedef struct nbco_mode_lag { double rr, ll, jj; double s0[2]; double s1[2]; unsigned long long pairs; } nbco_mode_lag;   /* 64 bytes */
int nbco_modes_record(nbco_ctx *c, const float *buf, long long n, const nbco_sk_grid *g_host, double *series_dev, int frames_cap, int frame, long long *n_used_host);
int nbco_mode_corr(nbco_ctx *c, const double *series_dev, const nbco_sk_grid *g_host, int frames_cap, int frames, int lags, nbco_mode_lag *out_dev);
int nbco_mode_corr_ref(const double *series_host, const nbco_sk_grid *g_host, int frames_cap, int frames, int lags, nbco_mode_lag *out_host);
int nbco_mode_corr_derive(const nbco_mode_lag *in, const nbco_sk_grid *g_host, int lags, double n_norm, double *out);
/* ---- aperture: particles that cross a boundary (a pipe wall, an electrode) are lost -- dropped from the state on the device,
 * recorded, and no longer simulated.  nbco_aperture_count / nbco_aperture_apply serve the 3-D fp32 state, the nbco_2d_ forms the
 * 2-D fp64 state (they read centre[0..1] and half[0..1] only).  *ap_host lies in HOST memory.
 * The rule, which is the whole numerical contract: in fp64 over the widened coordinates, no fused multiply-add, no division and no
 * square root on the device.  w_a = 1.0 / half_a is computed once on the host; half_a = +infinity gives w_a = 0: that axis is open
 * (pipes, slabs).  d_a = (double) x_a - centre_a.  A particle with a non-finite coordinate is outside in both shapes.
 *   NBCO_AP_ELLIPSOID: u_a = d_a * w_a; s = (u_x u_x + u_y u_y) + u_z u_z (2-D: u_x u_x + u_y u_y), every product and sum rounded
 *   once in this order; inside iff s <= 1.0.
 *   NBCO_AP_BOX: inside iff fabs(d_a) <= half_a on every axis.
 * Only positions decide.
 * nbco_aperture_count: the classification pass alone (one read of the positions p, wave ballots, integer sums).  p is not modified
 * and the context is not touched; *n_lost_host receives the number of particles outside.  The call synchronises.
 * nbco_aperture_apply: buf = [pos n | vel n | acc n] in DEVICE memory; all three blocks are read.  The particles inside keep their
 * relative order and buf becomes [pos n' | vel n' | acc n'] at the head of the same allocation, every kept row with the bits it had;
 * what lies behind 9 n' floats (2-D: 6 n' doubles) is unspecified.  The blocks move, so the state is compacted out of place into
 * scratch of the context and copied back.  The accelerations travel with the state: the next half kick of a leapfrog step uses
 * them, and the force a lost particle exerted at its last instant was real.  param is not touched: the coupling stays xi / N0,
 * because the charge per particle does not change when others are lost.
 * The loss record: lost_dev receives one row x y z vx vy vz (2-D: x y vx vy) per lost particle, in state order, and
 * lost_row_dev[k] that particle's row in buf before the call.  Either may be NULL; lost_cap is the room of the non-NULL outputs, in
 * records.  A row's slot is the number of lost (kept) rows before it -- ballot prefix + wave offset + workgroup offset from a scan
 * of the workgroup counts: no atomic decides a position, and a second call returns the same bytes.
 * The call always synchronises and always writes *n_kept_host = n - lost.  If an output is given and lost > lost_cap it returns
 * NBCO_ERR_CAPACITY and buf, the outputs and the context stay exactly as they were: the caller sizes the record from *n_kept_host
 * and calls again.  n' = 0 is a legal result.
 * The context.  lost == 0: nothing at all changes -- no copy, no invalidation; the tree, the rebuild schedule, the warm-select
 * history, order tracking, nbco_kd_get_info and a valid nbco_energy_fmm / nbco_kd_potential / nbco_kd_probe return the bits they
 * would have returned.  lost > 0: the state is a new state -- the tree is dropped and the rebuild schedule restarts, as nbco_set_opts
 * does for a new state, and nbco_energy_fmm / nbco_kd_potential / nbco_kd_probe refuse with NBCO_ERR_ARG until the next
 * nbco_fmm_kdtree.  With live order tracking (opts.track_order and a tracked evaluation of these n particles behind it) the order
 * map is compacted with the state: NBCO_KD_ORDER keeps meaning "particle number in the state the first tracked evaluation
 * received", and the numbers become sparse.  (The 2-D evaluators keep nothing between calls.)
 * Refused before any launch, everything untouched: with NBCO_ERR_ARG a NULL c, buf / p, ap_host or count pointer, n <= 0, an unknown
 * shape, a centre that is not finite, a half that is NaN or <= 0, lost_cap < 0; with NBCO_ERR_UNSUPPORTED n >= 2^31.
 * Not offered: sharded (nbco_dist_*) runs -- their domains must stay equal-sized; a sharded run gathers its state first. */
enum { NBCO_AP_ELLIPSOID = 0, NBCO_AP_BOX = 1 };
typedef struct nbco_aperture { int shape; double centre[3]; double half[3]; } nbco_aperture;   /* 2-D calls read [0], [1] */
int nbco_aperture_count(nbco_ctx *c, const float *p, long long n, const nbco_aperture *ap_host, long long *n_lost_host);
int nbco_aperture_apply(nbco_ctx *c, float *buf, long long n, const nbco_aperture *ap_host, long long *n_kept_host, float *lost_dev,
                        int *lost_row_dev, long long lost_cap);
int nbco_2d_aperture_count(nbco_ctx *c, const double *p, long long n, const nbco_aperture *ap_host, long long *n_lost_host);
int nbco_2d_aperture_apply(nbco_ctx *c, double *buf, long long n, const nbco_aperture *ap_host, long long *n_kept_host, double *lost_dev,
                           int *lost_row_dev, long long lost_cap);
/* main.cu:120-145 initKV and :147-170 initGA over std::mt19937_64(seed) after discard(discard) (main.cu:779-784 uses
 * NBCO_REF_SEED / NBCO_REF_DISCARD); host_state = [pos n x 2 | vel n x 2] doubles in HOST memory, centred with exactly the
 * RMS A/2, omega A/2 (KV) or x, u (Gaussian) per axis.  initKV takes each angle's sine and cosine from one glibc sincos call,
 * as the reference's documented build (GCC, -O2 and above) does. */
int nbco_2d_init_kv(double *host_state, long long n, const double *A2, const double *omega2, unsigned long long seed,
                    unsigned long long discard);
int nbco_2d_init_gaussian(double *host_state, long long n, const double *x2, const double *u2, unsigned long long seed,
                          unsigned long long discard);

#ifdef __cplusplus
}
#endif
#endif /* NBCO_H */
