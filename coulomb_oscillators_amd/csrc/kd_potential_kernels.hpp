// kd_potential_kernels.hpp -- part of k_fmm_kd.hip (included there, behind kd_energy_kernels.hpp: one translation unit, one anonymous namespace)
// O(N) potential pass over the locals of the last evaluation: per-node c0, downward, per-leaf psi, slot sum
// (no include guard on purpose: this is a section of that file, not a header)
// ---- FMM potential per particle from the LOCAL expansions ("3-D energy diagnostics") --------------------
// The locals of an evaluation are the derivatives of the far potential at the node centres, orders 1..p; l2p_body takes
//   a_c = -sum_K D~[K] F[e_c + K],   D~[K] = d^K / K!,  F = the full symmetric tensor behind the traceless storage (F_n = n! L_n),
// which is minus the gradient of
//   phi_far(c + d) = c0 + sum_{n = 1..p} sum_{|K| = n} D~[K] F_n[K].
// The evaluator never computes the order-0 term c0 (the far potential AT the centre); here it is
//   c0_own[node] = sum over the node's sorted M2L entries of m2p_potential(M[src], c_node - c_src)      (kd_c0_own_kernel)
//   c0[child]    = c0_own[child] + c0[parent] + lpot(F[parent], c_child - c_parent)                      (kd_c0_down_kernel, level by level)
//   psi_i        = param[0] (near_i + c0[leaf] + lpot(F[leaf], x_i - c_leaf))                            (kd_psi_leaf_kernel)
// with near_i the pair sum over the leaf's sorted P2P range (j != i by index).  fp64 throughout, no atomics, every sum in a
// fixed order: a second call returns the same bits.  One wave per node / leaf: F is expanded once into LDS with a lane per
// component, and every lane walks its own monomials against broadcast reads.
constexpr int kPotWave = 64;

// F[sym_offset(n) + sym_index(x, z, n)] = n! L_n[x, y, z] for orders 1..P from the traceless tuple Lp (components with z <= 1 are
// stored, tl_off(n) + (z + 1) n - x; the rest follow from the vanishing trace, two rows of z at a time).  Slot 0 is not written.
template <int P, typename T>
__device__ inline void expand_local_lds(const T *__restrict__ Lp, double *F, int t)
{
	for (int s = 1 + t; s < (P + 1) * (P + 1); s += kPotWave)
	{
		int n = 1;
		double fact = 1.0;
		while ((n + 1) * (n + 1) <= s) { ++n; fact *= (double)n; }
		const int r = s - n * n, z = r <= n ? 0 : 1, x = (z + 1) * n - r;
		F[sym_offset(n) + sym_index(x, z, n)] = (double)Lp[s] * fact;
	}
	__syncthreads();
	for (int z = 2; z <= P; ++z)
	{
		for (int n = z; n <= P; ++n)
			for (int x = t; x <= n - z; x += kPotWave)   // (x, y, z) <- -((x + 2, y, z - 2) + (x, y + 2, z - 2))
				F[sym_offset(n) + sym_index(x, z, n)] = -(F[sym_offset(n) + sym_index(x + 2, z - 2, n)] + F[sym_offset(n) + sym_index(x, z - 2, n)]);
		__syncthreads();
	}
}

// sum_{n = 1..P} sum_{|K| = n} D~[K] F_n[K] in storage order (what gen_ops.py's lpot_body computes from the traceless tuple)
template <int P>
__device__ inline double lpot_walk(const double *F, double dx, double dy, double dz)
{
	double px[P + 1], py[P + 1], pz[P + 1];
	px[0] = py[0] = pz[0] = 1.0;
#pragma unroll
	for (int k = 1; k <= P; ++k)
	{
		const double ik = 1.0 / (double)k;
		px[k] = px[k - 1] * (dx * ik); py[k] = py[k - 1] * (dy * ik); pz[k] = pz[k - 1] * (dz * ik);
	}
	double phi = 0.0;
#pragma unroll
	for (int n = 1; n <= P; ++n)
#pragma unroll
		for (int z = 0; z <= n; ++z)
#pragma unroll
			for (int x = n - z; x >= 0; --x) phi = fma(px[x] * py[n - x - z] * pz[z], F[sym_offset(n) + sym_index(x, z, n)], phi);
	return phi;
}

// one wave per node: the lanes share the node's sorted M2L entries (lane l takes entries l, l + 64, ..), butterfly combine
template <int P, typename T>
__global__ __launch_bounds__(kBlock) void kd_c0_own_kernel(const float4 *__restrict__ csz, const T *__restrict__ mpole, const uint64_t *__restrict__ m2l_keys,
                                                           const int *__restrict__ m2l_start, int shift, int ntot, float eps2f, double *__restrict__ c0)
{
	constexpr int offM = sym_offset(P);
	const int node = blockIdx.x * (kBlock / kPotWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint64_t mask = (1ull << shift) - 1;
	double s = 0.0;
	if (node < ntot)
	{
		const float4 ct = csz[node];
		const double eps2 = (double)eps2f;
		// (the node's run of the sorted list and the source node of an entry; the checked build counts a run outside the list, which it
		// takes as empty, and a source outside the tree, for which the node itself stands in)
		const int e0 = m2l_start[node];
		const int e1 = NBCO_CHECKED_OK(e0 >= 0 && e0 <= m2l_start[node + 1] && m2l_start[node + 1] <= m2l_start[ntot], NBCO_CHK_WALK) ? m2l_start[node + 1] : e0;
		for (int e = e0 + lane; e < e1; e += kPotWave)
		{
			int sn = (int)(m2l_keys[e] & mask);
			if (!NBCO_CHECKED_OK((unsigned)sn < (unsigned)ntot, NBCO_CHK_WALK)) sn = node;
			const float4 cs = csz[sn];
			s += m2p_potential<P, T>(mpole + (size_t)sn * offM, (double)ct.x - (double)cs.x, (double)ct.y - (double)cs.y, (double)ct.z - (double)cs.z, eps2);
		}
	}
	for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
	if (node < ntot && lane == 0) c0[node] = s;
}

// child level lc: one wave per PARENT (its expanded locals serve both children), c0[child] = (c0_own[child] + c0[parent]) + lpot
template <int P, typename T>
__global__ __launch_bounds__(kPotWave) void kd_c0_down_kernel(const float *__restrict__ center, const T *__restrict__ local, int lc, double *__restrict__ c0)
{
	constexpr int offL = (P + 1) * (P + 1);
	__shared__ double F[sym_offset(P + 1)];
	const int par = kd_beg(lc - 1) + blockIdx.x, t = threadIdx.x;
	expand_local_lds<P, T>(local + (size_t)par * offL, F, t);
	if (t < 2)
	{
		const int ch = 2 * par + 1 + t;
		const double dx = (double)center[3 * ch] - (double)center[3 * par], dy = (double)center[3 * ch + 1] - (double)center[3 * par + 1],
		             dz = (double)center[3 * ch + 2] - (double)center[3 * par + 2];
		c0[ch] = (c0[ch] + c0[par]) + lpot_walk<P>(F, dx, dy, dz);
	}
}

// one wave per leaf, one lane per target (tiles of 64 when the leaf holds more); psi in the caller's particle order, the leaf's sum in its slot
template <int P, typename T>
__global__ __launch_bounds__(kPotWave) void kd_psi_leaf_kernel(nbco_ctx::LastEval le, const T *__restrict__ local, const double *__restrict__ c0,
                                                              const uint64_t *__restrict__ p2p_keys, const int *__restrict__ p2p_start, float eps2f,
                                                              const float *__restrict__ param, const int *__restrict__ unsort, double *__restrict__ psi_out,
                                                              double *__restrict__ slot)
{
	constexpr int offL = (P + 1) * (P + 1);
	__shared__ double F[sym_offset(P + 1)];
	const int beg = kd_beg(le.L), lf = blockIdx.x, leaf = beg + lf, t = threadIdx.x;
	expand_local_lds<P, T>(local + (size_t)leaf * offL, F, t);
	const uint64_t mask = (1ull << le.shift) - 1;
	// (the checked build counts a particle range outside [0, n) and a run outside the sorted list, which it takes as empty, and a source
	// leaf outside the leaf level, for which the leaf itself stands in)
	const int i0 = le.index[leaf];
	const int m = NBCO_CHECKED_OK(i0 >= 0 && le.mult[leaf] >= 0 && (long long)i0 + le.mult[leaf] <= le.n, NBCO_CHK_WALK) ? le.mult[leaf] : 0;
	const double cx = (double)le.center[3 * leaf], cy = (double)le.center[3 * leaf + 1], cz = (double)le.center[3 * leaf + 2];
	const double eps2 = (double)eps2f, c0l = c0[leaf], p0 = (double)param[0];
	const int e0 = le.have_p2p ? p2p_start[lf] : 0, e1raw = le.have_p2p ? p2p_start[lf + 1] : 0;
	const int e1 = NBCO_CHECKED_OK(!le.have_p2p || (e0 >= 0 && e0 <= e1raw && e1raw <= p2p_start[gridDim.x]), NBCO_CHK_WALK) ? e1raw : e0;
	double acc = 0.0;
	for (int j = t; j < m; j += kPotWave)
	{
		const int i = i0 + j;
		const float4 p = le.pos[i];
		double phi = 0.0;
		for (int e = e0; e < e1; ++e)
		{
			const int sl = (int)(p2p_keys[e] & mask);
			const int src = beg + (NBCO_CHECKED_OK((unsigned)sl < gridDim.x, NBCO_CHK_WALK) ? sl : lf);
			const int is = le.index[src];
			const int ms = NBCO_CHECKED_OK(is >= 0 && le.mult[src] >= 0 && (long long)is + le.mult[src] <= le.n, NBCO_CHK_WALK) ? le.mult[src] : 0;
			for (int k = 0; k < ms; ++k)
			{
				if (is + k == i) continue;
				const float4 q = le.pos[is + k];
				const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
				phi += 1.0 / sqrt(dx * dx + dy * dy + dz * dz + eps2);
			}
		}
		// (the fence keeps the reads of F inside the tile loop: hoisted out of it they would occupy two registers per component for the
		// whole near-field loop)
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		phi += c0l + lpot_walk<P>(F, (double)p.x - cx, (double)p.y - cy, (double)p.z - cz);
		const double psi = p0 * phi;
		if (psi_out) psi_out[unsort ? unsort[i] : i] = psi;
		acc += psi;
	}
	for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if (t == 0) slot[lf] = acc;
}

// one block: out[0] = 1/2 sum of the slots (strided partial sums, then a tree in LDS: a fixed order)
__global__ __launch_bounds__(kBlock) void kd_slot_sum_kernel(const double *__restrict__ slot, int nslot, double *__restrict__ out)
{
	__shared__ double sh[kBlock];
	double s = 0.0;
	for (int k = threadIdx.x; k < nslot; k += kBlock) s += slot[k];
	sh[threadIdx.x] = s;
	__syncthreads();
	for (int w = kBlock / 2; w > 0; w >>= 1)
	{
		if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = 0.5 * sh[0];
}

// (T: multipoles and locals of the last evaluation are doubles when it ran with opts.far_fp64: LastEval::real_bytes)
template <int P, typename T>
static void launch_kd_psi(nbco_ctx *c, double *c0, double *slot, const float *param, double *psi_out)
{
	const nbco_ctx::LastEval &le = c->last_eval;
	const T *mpole = reinterpret_cast<const T *>(le.mpole), *local = reinterpret_cast<const T *>(le.local);
	hipStream_t st = c->stream;
	hipLaunchKernelGGL((kd_c0_own_kernel<P, T>), dim3((le.ntot + kBlock / kPotWave - 1) / (kBlock / kPotWave)), dim3(kBlock), 0, st, le.csz, mpole,
	                   (const uint64_t *)c->m2l_keys_alt.as<uint64_t>(), (const int *)c->m2l_start.as<int>(), le.shift, le.ntot, c->o.eps2, c0);
	for (int lc = 1; lc <= le.L; ++lc)
		hipLaunchKernelGGL((kd_c0_down_kernel<P, T>), dim3(kd_cnt(lc - 1)), dim3(kPotWave), 0, st, le.center, local, lc, c0);
	hipLaunchKernelGGL((kd_psi_leaf_kernel<P, T>), dim3(kd_cnt(le.L)), dim3(kPotWave), 0, st, le, local, (const double *)c0,
	                   (const uint64_t *)c->p2p_keys_alt.as<uint64_t>(), (const int *)c->p2p_start.as<int>(), c->o.eps2, param, le.scatter ? le.unsort : nullptr,
	                   psi_out, slot);
}
