// kd_probe_kernels.hpp -- part of k_fmm_kd.hip (included there, in this place: one translation unit, one anonymous namespace)
// 3-D probes: field and potential of the charges at points that are not particles
// (no include guard on purpose: this is a section of that file, not a header)
// ---- probes (no reference driver evaluates the field away from the particles) -----------------------------------------------------
// Every source counts at every probe t_i; there is no self exclusion, because a probe is not a particle:
//   a_i   = param[0] sum_j d (|d|^2 + EPS2)^(-3/2),  d = t_i - x_j
//   psi_i = param[0] sum_j   (|d|^2 + EPS2)^(-1/2)                 (a_i = -grad psi_i)
// The evaluator's lists are keyed by target leaves, and a probe far from the cloud belongs to none: the probes walk the tree
// themselves.  Depth first from the root, left child first: a node that passes the evaluator's own acceptance test -- with the
// probe as a node of size 0 and multiplicity 1 -- contributes its multipole expansion evaluated AT THE PROBE; a leaf is never
// expanded, whatever the test says: it contributes its particles pair by pair (at the leaf sizes the build makes the pair sum is
// cheaper than one expansion, and it is exact -- and a probe that is a particle never meets an expansion that contains it); any
// other node is opened.  A probe's sums therefore depend on the tree and its own position alone, in a fixed order.
// fp64 throughout over the widened floats, as the energy diagnostics.

// (c, sz) of node `node` with multiplicity mlt against the point t: kd_admissible with the point as the second node.  The node is
// always the bigger of the two (sz >= 0, mlt >= 1), so its level and multiplicity pick the table entry.
#pragma clang fp contract(off)   // every decision must be reproducible from a restatement in fp32: no fused multiply-adds
__device__ inline bool kd_probe_admissible(const float4 c, int mlt, int node, float tx, float ty, float tz, const AdmTab *tabp, float par)
{
	float dx = tx - c.x, dy = ty - c.y, dz = tz - c.z;
	float dist2 = dx * dx + dy * dy + dz * dz;
	int lev = 31 - __clz(node + 1);
	float M = (mlt == tabp->lo[lev]) ? tabp->Mlo[lev] : tabp->Mhi[lev];
	float parM = par * M;
	float sz = fmaxf(c.w, 0.f);
	return parM * parM * sz < dist2;
}
#pragma clang fp contract(fast)

// Multipole to point, potential and field in one pass over the Taylor coefficients b_K = d^K f / K! of f = (|d|^2 + EPS2)^(-1/2)
// (the recurrence of m2p_potential):
//   psi += sum_K M[K] |K|! b_K(d)                      orders 0 .. P-1 of b
//   a_c -= sum_K M[K] |K|! (K_c + 1) b_{K + e_c}(d)    orders 1 .. P of b (grad b_K = (K_c + 1) b_{K + e_c})
// Fully unrolled: every index is a compile-time constant, so B is taken apart into registers.  A coefficient is consumed by both
// sums the moment it exists and is not read after order k + 2 has been formed, so the recurrence NEEDS three orders at a time; what
// the compiler keeps is another matter -- it hoists the scalar multipole loads and their conversions, and from order 9 on the
// kernels with the field spill (DESIGN section 4 has the table).
template <int P, typename T, bool WANT_A, bool WANT_PSI>
__device__ inline void m2p_field_potential(const T *__restrict__ M, double dx, double dy, double dz, double eps2, double &ax, double &ay, double &az,
                                           double &psi)
{
	constexpr int KMAX = WANT_A ? P : P - 1;
	double B[sym_offset(KMAX + 1)];
	const double R2 = dx * dx + dy * dy + dz * dz + eps2, iR2 = 1.0 / R2;
	B[0] = sqrt(iR2);
	double phi = WANT_PSI ? (double)M[0] * B[0] : 0.0, fact = 1.0;   // fact = (k - 1)! at the head of order k's body, k! behind it
	double fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
	for (int k = 1; k <= KMAX; ++k)
	{
		const double c1 = -(double)(2 * k - 1) * iR2 / (double)k, c2 = -(double)(k - 1) * iR2 / (double)k;
		double s = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
		for (int z = 0; z <= k; ++z)
#pragma unroll
			for (int x = k - z; x >= 0; --x)
			{
				const int y = k - x - z;
				double t1 = 0.0, t2 = 0.0;
				if (x >= 1) t1 += dx * B[sym_offset(k - 1) + sym_index(x - 1, z, k - 1)];
				if (y >= 1) t1 += dy * B[sym_offset(k - 1) + sym_index(x, z, k - 1)];
				if (z >= 1) t1 += dz * B[sym_offset(k - 1) + sym_index(x, z - 1, k - 1)];
				if (k >= 2)
				{
					if (x >= 2) t2 += B[sym_offset(k - 2) + sym_index(x - 2, z, k - 2)];
					if (y >= 2) t2 += B[sym_offset(k - 2) + sym_index(x, z, k - 2)];
					if (z >= 2) t2 += B[sym_offset(k - 2) + sym_index(x, z - 2, k - 2)];
				}
				const double b = c1 * t1 + c2 * t2;
				B[sym_offset(k) + sym_index(x, z, k)] = b;
				if (WANT_PSI && k < P) s += (double)M[sym_offset(k) + sym_index(x, z, k)] * b;
				if (WANT_A)
				{
					// b_{K + e_c} with K + e_c = (x, y, z): K of order k - 1, K_c + 1 = the c-th exponent here
					if (x >= 1) gx += (double)M[sym_offset(k - 1) + sym_index(x - 1, z, k - 1)] * ((double)x * b);
					if (y >= 1) gy += (double)M[sym_offset(k - 1) + sym_index(x, z, k - 1)] * ((double)y * b);
					if (z >= 1) gz += (double)M[sym_offset(k - 1) + sym_index(x, z - 1, k - 1)] * ((double)z * b);
				}
			}
		if (WANT_A) { fx += fact * gx; fy += fact * gy; fz += fact * gz; }
		fact *= (double)k;
		if (WANT_PSI && k < P) phi += fact * s;
	}
	if (WANT_A) { ax -= fx; ay -= fy; az -= fz; }
	if (WANT_PSI) psi += phi;
}

// exact sums: one probe per thread, the sources staged through LDS in tiles of kBlock (direct_tiles' shape).  p and t may be the
// same array: neither is written.
template <bool WANT_A, bool WANT_PSI>
__global__ __launch_bounds__(kBlock) void kd_probe_direct_kernel(const float *p, long long n, const float *t, long long m, float eps2f,
                                                                 const float *__restrict__ param, double *__restrict__ a, double *__restrict__ psi)
{
	__shared__ float sx[kBlock], sy[kBlock], sz[kBlock];
	const long long i = (long long)blockIdx.x * kBlock + threadIdx.x, ic = i < m ? i : m - 1;
	const double tx = (double)t[3 * ic], ty = (double)t[3 * ic + 1], tz = (double)t[3 * ic + 2], eps2 = (double)eps2f;
	double ax = 0.0, ay = 0.0, az = 0.0, ps = 0.0;
	for (long long j0 = 0; j0 < n; j0 += kBlock)
	{
		__syncthreads();
		const long long j = j0 + threadIdx.x;
		if (j < n)
		{
			sx[threadIdx.x] = p[3 * j];
			sy[threadIdx.x] = p[3 * j + 1];
			sz[threadIdx.x] = p[3 * j + 2];
		}
		__syncthreads();
		const int cnt = (int)std::min<long long>(kBlock, n - j0);
		for (int u = 0; u < cnt; ++u)
		{
			const double dx = tx - (double)sx[u], dy = ty - (double)sy[u], dz = tz - (double)sz[u];
			const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz + eps2);
			if (WANT_PSI) ps += inv;
			if (WANT_A)
			{
				const double inv3 = inv * inv * inv;
				ax += dx * inv3;
				ay += dy * inv3;
				az += dz * inv3;
			}
		}
	}
	if (i >= m) return;
	const double s0 = (double)param[0];
	if (WANT_A) { a[3 * i] = s0 * ax; a[3 * i + 1] = s0 * ay; a[3 * i + 2] = s0 * az; }
	if (WANT_PSI) psi[i] = s0 * ps;
}

// Morton keys of the probes in the sources' root box (clamped: a probe outside is keyed into the border cell nearest to it) and the
// identity permutation.  The keys only decide which probes share a wave; no result depends on them.
__device__ inline uint32_t probe_spread10(uint32_t v)
{
	v = (v | (v << 16)) & 0x030000FFu;
	v = (v | (v << 8)) & 0x0300F00Fu;
	v = (v | (v << 4)) & 0x030C30C3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}
__global__ __launch_bounds__(kBlock) void kd_probe_keys_kernel(const float *t, long long m, const float *__restrict__ lbound, const float *__restrict__ rbound,
                                                               uint32_t *__restrict__ keys, uint32_t *__restrict__ idx)
{
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long long)gridDim.x * kBlock)
	{
		uint32_t q[3];
#pragma unroll
		for (int d = 0; d < 3; ++d)
		{
			const float lo = lbound[d], w = rbound[d] - lo;
			const float u = w > 0.f ? (t[3 * i + d] - lo) / w * 1024.f : 0.f;
			q[d] = u >= 0.f ? (u < 1023.f ? (uint32_t)u : 1023u) : 0u;   // (a NaN coordinate lands in cell 0)
		}
		keys[i] = probe_spread10(q[0]) | (probe_spread10(q[1]) << 1) | (probe_spread10(q[2]) << 2);
		idx[i] = (uint32_t)i;
	}
}

// One step of a walk through the implicit tree (children 2k + 1, 2k + 2) without a stack, k the same in every lane: down to the left
// child if the wave opens node k, else up while a right child and over to the sibling of a left child.  The node after k, or 0 (the
// root, which no step leads to): the walk is done.  (the probe walk here and the radius walk of pair_stat_kernels.hpp)
__device__ inline int kd_walk_next(int k, bool open)
{
	if (open) return 2 * k + 1;
	while (k != 0 && (k & 1) == 0) k = (k - 1) >> 1;
	return k == 0 ? 0 : k + 1;
}

// The walk.  One wave takes 64 consecutive probes of the sorted order and goes through the implicit tree (children 2k + 1, 2k + 2)
// without a stack; the current node k is the same in every lane, so its record, multiplicity and multipole are scalar loads.  Every
// lane takes its own decision.  A lane that has accepted a node is covered while the walk stays in that node's subtree (cov1: the
// accepted node's 1-based number, an ancestor of k + 1 iff a right shift of k + 1 gives it); the wave opens a node when at least one
// lane needs it open and skips the subtree otherwise.  A lane works on node k iff it accepted none of k's ancestors, and then the wave
// has opened them all: the nodes a probe sums over, and their order, are those of its own depth-first walk, whatever its neighbours.
// A leaf's particles are staged in LDS once, in tiles of 64, for the lanes that need them.
constexpr int kProbeWave = 64;
template <int P, typename T, bool WANT_A, bool WANT_PSI>
__global__ __launch_bounds__(kProbeWave) void kd_probe_walk_kernel(const float4 *__restrict__ csz, const T *__restrict__ mpole, const int *__restrict__ mult,
                                                                   const int *__restrict__ index, const float4 *__restrict__ pos, int ntot, AdmTab tab_arg,
                                                                   float par, float eps2f, const uint32_t *__restrict__ perm, const float *t, long long m,
                                                                   const float *__restrict__ param, double *__restrict__ a, double *__restrict__ psi
                                                                   NBCO_CHECKED_ARG(long long n))
{
	constexpr int offM = sym_offset(P);
	__shared__ AdmTab tab;   // LDS copy: the table is indexed by the node's level
	__shared__ float4 tile[kProbeWave];
	const int lane = threadIdx.x;
	for (int q = lane; q < (int)(sizeof(AdmTab) / sizeof(int)); q += kProbeWave) reinterpret_cast<int *>(&tab)[q] = reinterpret_cast<const int *>(&tab_arg)[q];
	__syncthreads();
	const long long s = (long long)blockIdx.x * kProbeWave + lane;
	const bool valid = s < m;
	uint32_t dst = valid ? perm[s] : 0u;
	if (!NBCO_CHECKED_OK((long long)dst < m, NBCO_CHK_WALK)) dst = 0u;   // (the sort's permutation of [0, m))
	const float tx = valid ? t[3 * (size_t)dst] : 0.f, ty = valid ? t[3 * (size_t)dst + 1] : 0.f, tz = valid ? t[3 * (size_t)dst + 2] : 0.f;
	const double X = (double)tx, Y = (double)ty, Z = (double)tz, eps2 = (double)eps2f;
	double ax = 0.0, ay = 0.0, az = 0.0, ps = 0.0;
	int cov1 = 0;
	int k = 0;
	for (;;)
	{
		k = __builtin_amdgcn_readfirstlane(k);   // (uniform by construction: it moves on ballots only)
		const int k1 = k + 1, lev = 31 - __clz(k1);
		bool covered = false;
		if (cov1 != 0)
		{
			const int lc = 31 - __clz(cov1);
			covered = lev >= lc && (k1 >> (lev - lc)) == cov1;
		}
		const bool act = valid && !covered;
		const float4 rec = csz[k];
		const int ml = mult[k];
		const bool leaf = 2 * k + 1 >= ntot;
		const bool adm = act && !leaf && kd_probe_admissible(rec, ml, k, tx, ty, tz, &tab, par);   // (a leaf is never expanded)
		if (adm)
		{
			cov1 = k1;
			m2p_field_potential<P, T, WANT_A, WANT_PSI>(mpole + (size_t)k * offM, X - (double)rec.x, Y - (double)rec.y, Z - (double)rec.z, eps2, ax, ay, az, ps);
		}
		const bool open = act && !adm;
		const bool any_open = __ballot(open) != 0;
		if (leaf && any_open)
		{
			const int i0 = index[k];
			// (a leaf's range lies inside [0, n) by the build; the checked build counts one that does not and takes the leaf as empty)
			const int nl = NBCO_CHECKED_OK(i0 >= 0 && ml >= 0 && (long long)i0 + ml <= n, NBCO_CHK_WALK) ? ml : 0;
			for (int j0 = 0; j0 < nl; j0 += kProbeWave)
			{
				__syncthreads();
				if (j0 + lane < nl) tile[lane] = pos[(size_t)i0 + j0 + lane];
				__syncthreads();
				const int cnt = min(kProbeWave, nl - j0);
				if (open)
					for (int u = 0; u < cnt; ++u)
					{
						const float4 q = tile[u];
						const double dx = X - (double)q.x, dy = Y - (double)q.y, dz = Z - (double)q.z;
						const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz + eps2);
						if (WANT_PSI) ps += inv;
						if (WANT_A)
						{
							const double inv3 = inv * inv * inv;
							ax += dx * inv3;
							ay += dy * inv3;
							az += dz * inv3;
						}
					}
			}
		}
		k = kd_walk_next(k, !leaf && any_open);
		if (k == 0) break;
	}
	if (!valid) return;
	const double s0 = (double)param[0];
	if (WANT_A) { a[3 * (size_t)dst] = s0 * ax; a[3 * (size_t)dst + 1] = s0 * ay; a[3 * (size_t)dst + 2] = s0 * az; }
	if (WANT_PSI) psi[dst] = s0 * ps;
}

// what a walk needs of a tree: the records, multipoles and tree-ordered positions of an evaluation, and the root box for the keys
struct ProbeSrc
{
	const float4 *csz = nullptr, *pos = nullptr;
	const void *mpole = nullptr;
	const int *mult = nullptr, *index = nullptr;
	const float *lbound = nullptr, *rbound = nullptr;
	int L = 0, ntot = 0, order = 0, real_bytes = 4;
	long long n = 0;
};

template <int P, typename T>
static void launch_probe_walk(nbco_ctx *c, const ProbeSrc &s, const AdmTab &tab, const uint32_t *perm, const float *t, long long m, const float *param,
                              double *a, double *psi)
{
	const dim3 grid((unsigned)((m + kProbeWave - 1) / kProbeWave)), block(kProbeWave);
	with_outputs(a, psi, [&](auto wa, auto wp) {
		hipLaunchKernelGGL((kd_probe_walk_kernel<P, T, decltype(wa)::value, decltype(wp)::value>), grid, block, 0, c->stream, s.csz, (const T *)s.mpole, s.mult,
		                   s.index, s.pos, s.ntot, tab, c->o.tree_radius, c->o.eps2, perm, t, m, param, a, psi NBCO_CHECKED_ARG(s.n));
	});
}
