// bond_order_kernels.hpp -- part of k_reduce.hip (the exact forms, with NBCO_BOND_EXACT defined) and of k_fmm_kd.hip (the tree walk,
// with NBCO_BOND_WALK defined): included there behind pair_stat_kernels.hpp, inside that file's anonymous namespace
// Bond-orientational order: per particle the number of neighbours and the Steinhardt q4, q6 (2-D: |psi4|, |psi6|), and a summary
// (no include guard on purpose: this is a section of those files, not a header)
// The neighbour rule of include/nbco.h is the pair rule of the pair statistics (pair_r2, contraction off) with 0 < r2 < R2; what a
// bond contributes comes from bond_order.hpp.  A particle's sums stay in the registers of the lane that owns it from the first
// neighbour to the last, in the order the kernel meets them: no atomics, and a second call adds in the same order.
// The summary: every wave of 64 consecutive particles (of the caller's order in the exact forms, of the tree order in the walk) adds
// its lanes' sums with a butterfly of fixed shape and writes one record of kBondRec slots; one workgroup then adds the records
// (bond_reduce_kernel, compiled with the exact forms and launched for both by bond_summary_finish).

__device__ inline double bond_wave_sum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline long long bond_wave_sum(long long v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline int bond_wave_max(int v) { for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; } return v; }

// The end of a lane's particle: q from the sums, nb and q to row `dst` of the outputs that are given (dst < 0: the lane has no
// particle, or no row to write to), and with SUM the wave's record (wave-uniform control flow; rec points at this wave's record).
// With VEC (3-D, no summary: nbco_bond_vectors) the particle's bond vector record instead of q: q_out then holds kBondVec doubles per row.
template <int D, bool SUM, bool VEC = false>
__device__ inline void bond_finish(bool valid, long long dst, int nb, const double (&S)[D == 3 ? kBondSums3 : kBondSums2], int *__restrict__ nb_out,
                                   double *__restrict__ q_out, double *__restrict__ rec)
{
	constexpr int NS = D == 3 ? kBondSums3 : kBondSums2;
	if constexpr (VEC)
	{
		static_assert(D == 3 && !SUM, "the records are those of the 3-D forms, and they have no summary");
		if (!valid || dst < 0) return;
		double v[kBondVec];
		bond_vector(S, nb, v);
		if (nb_out) nb_out[dst] = nb;
		if (q_out)
		{
#pragma unroll
			for (int m = 0; m < kBondVec; ++m) q_out[kBondVec * dst + m] = v[m];
		}
		return;
	}
	double q[2];
	bond_q<D>(S, nb, q);
	if (valid && dst >= 0)
	{
		if (nb_out) nb_out[dst] = nb;
		if (q_out) { q_out[2 * dst] = q[0]; q_out[2 * dst + 1] = q[1]; }
	}
	if (SUM)
	{
		const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
		for (int m = 0; m < NS; ++m)
		{
			const double v = bond_wave_sum(valid ? S[m] : 0.0);
			if (first) rec[m] = v;
		}
		if (first)
			for (int m = NS; m < kBondRecQ; ++m) rec[m] = 0.0;
#pragma unroll
		for (int l = 0; l < 2; ++l)
		{
			const double v = bond_wave_sum(valid ? q[l] : 0.0);
			if (first) rec[kBondRecQ + l] = v;
		}
		const long long bonds = bond_wave_sum(valid ? (long long)nb : 0ll), isolated = bond_wave_sum(valid && nb == 0 ? 1ll : 0ll);
		const int top = bond_wave_max(valid ? nb : 0);
		if (first)
		{
			rec[kBondRecBonds] = __longlong_as_double(bonds);
			rec[kBondRecIsolated] = __longlong_as_double(isolated);
			rec[kBondRecMax] = __longlong_as_double((long long)top);
		}
	}
}

// ---- crystalline particles: the second pass (nbco_bond_solid) ----------------------------------------------------------------------
// A lane keeps of its particle the q^_6 of its record (13 doubles: the left side of every coherence), the 22 sums T of the averaged
// order, xi and nb.  The staged source is the same in every lane of the wave, so its record sits at a wave-uniform address: it is read
// once per wave, only where a lane has the source for a neighbour, and its 24 doubles arrive as uniform values.  What a bond adds comes
// from bond_order.hpp: the coherence (contraction off there) decides xi, the 22 products go into T in the order the bonds are met.

// the lane's own record: its q^_6 into e, and T starts with the particle's own term
__device__ inline void solid_begin(const double *__restrict__ own, double (&e)[13], double (&T)[kBondSums3])
{
#pragma unroll
	for (int m = 0; m < 13; ++m) e[m] = own[kBondVec6 + m];
#pragma unroll
	for (int m = 0; m < kBondSums3; ++m) T[m] = 0.0;
	bond_avg_add(own, T);
}

// the record at the wave-uniform address f: 24 uniform values, loaded once for the wave
__device__ inline void solid_record(const double *__restrict__ f, double (&r)[kBondVec])
{
#pragma unroll
	for (int m = 0; m < kBondVec; ++m) r[m] = f[m];
}

// one bond of the lane's particle with the record r of the neighbour
__device__ inline void solid_bond(const double (&e)[13], const double (&r)[kBondVec], double dmin, int &nb, int &xi, double (&T)[kBondSums3])
{
	++nb;
	if (bond_coherence(e, r + kBondVec6) > dmin) ++xi;
	bond_avg_add(r, T);
}

// The end of a lane's particle, in the shape of bond_finish: nb, xi and {q-bar_4, q-bar_6} to row dst of the outputs that are given,
// and with SUM the wave's record of kSolidRec slots.
template <bool SUM>
__device__ inline void solid_finish(bool valid, long long dst, int nb, int xi, const double (&T)[kBondSums3], int xi_min, int *__restrict__ nb_out,
                                    int *__restrict__ xi_out, double *__restrict__ qbar_out, double *__restrict__ rec)
{
	double q[2];
	bond_qbar(T, nb, q);
	if (valid && dst >= 0)
	{
		if (nb_out) nb_out[dst] = nb;
		if (xi_out) xi_out[dst] = xi;
		if (qbar_out) { qbar_out[2 * dst] = q[0]; qbar_out[2 * dst + 1] = q[1]; }
	}
	if (SUM)
	{
		const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
		for (int l = 0; l < 2; ++l)
		{
			const double v = bond_wave_sum(valid ? q[l] : 0.0);
			if (first) rec[l] = v;
		}
		const long long bonds = bond_wave_sum(valid ? (long long)nb : 0ll), isolated = bond_wave_sum(valid && nb == 0 ? 1ll : 0ll);
		const long long solid = bond_wave_sum(valid ? (long long)xi : 0ll), count = bond_wave_sum(valid && xi >= xi_min ? 1ll : 0ll);
		const int top = bond_wave_max(valid ? xi : 0);
		if (first)
		{
			rec[kSolidRecBonds] = __longlong_as_double(bonds);
			rec[kSolidRecIsolated] = __longlong_as_double(isolated);
			rec[kSolidRecSolid] = __longlong_as_double(solid);
			rec[kSolidRecCount] = __longlong_as_double(count);
			rec[kSolidRecMax] = __longlong_as_double((long long)top);
		}
	}
}

#ifdef NBCO_BOND_EXACT
// The records of all waves -> out[REC], by one workgroup: thread (g, slot) adds the records of the g-th of kBondGroups contiguous
// ranges in record order, then the first REC threads add the groups in group order.  Slots below INTS are doubles, the others 64-bit
// integers: sums, and a maximum in slot MAX.  <kBondRec, kBondRecBonds, kBondRecMax> serves the bond order, <kSolidRec, kSolidRecBonds,
// kSolidRecMax> the solid pass.
constexpr int kBondGroups = 32, kBondSlots = 32;
static_assert(kBondRec <= kBondSlots && kSolidRec <= kBondSlots, "a slot per thread of a group");
template <int REC, int INTS, int MAX>
__global__ __launch_bounds__(kBondGroups * kBondSlots) void bond_reduce_kernel(const double *__restrict__ rec, long long records, double *__restrict__ out)
{
	__shared__ double sh[kBondGroups][kBondSlots];
	const int slot = threadIdx.x % kBondSlots, g = threadIdx.x / kBondSlots;
	const long long per = (records + kBondGroups - 1) / kBondGroups;
	const long long lo = g * per < records ? g * per : records, hi = lo + per < records ? lo + per : records;
	if (slot < INTS)
	{
		double s = 0.0;
		for (long long r = lo; r < hi; ++r) s += rec[r * REC + slot];
		sh[g][slot] = s;
	}
	else if (slot < REC)
	{
		long long s = 0;
		for (long long r = lo; r < hi; ++r)
		{
			const long long v = __double_as_longlong(rec[r * REC + slot]);
			s = slot == MAX ? (v > s ? v : s) : s + v;
		}
		sh[g][slot] = __longlong_as_double(s);
	}
	__syncthreads();
	if (threadIdx.x >= REC) return;
	if (slot < INTS)
	{
		double s = 0.0;
		for (int k = 0; k < kBondGroups; ++k) s += sh[k][slot];
		out[slot] = s;
	}
	else
	{
		long long s = 0;
		for (int k = 0; k < kBondGroups; ++k)
		{
			const long long v = __double_as_longlong(sh[k][slot]);
			s = slot == MAX ? (v > s ? v : s) : s + v;
		}
		out[slot] = __longlong_as_double(s);
	}
}

// ---- exact form: all pairs ---------------------------------------------------------------------------------------------------------
// The tiling of pair_hist_kernel with the full square instead of the triangle: a workgroup keeps the particles of tile I in
// registers, one per thread, and takes EVERY source tile through LDS, widened once when it is staged, so that a target meets all its
// neighbours itself, in index order, and nothing has to be handed to the other end of a pair.  The particle itself and a coincident
// one fall out through r2 > 0.  A pair outside costs the subtractions, r2, two compares and the wave's branch on the ballot; the
// harmonics are formed only where a lane of the wave has a neighbour.  One template covers T = float, D = 3 and T = double, D = 2.
// With VEC the bond vector records go where q would (bond_finish).
template <class T, int D, bool SUM, bool VEC = false>
__global__ __launch_bounds__(kBlock) void bond_exact_kernel(const T *__restrict__ p, long long n, double R2, int *__restrict__ nb_out, double *__restrict__ q_out,
                                                             double *__restrict__ rec)
{
	__shared__ double src[3][kBlock];
	const int tid = threadIdx.x;
	const long long nt = (n + kBlock - 1) / kBlock, i = (long long)blockIdx.x * kBlock + tid;
	double x0, x1, x2;
	pair_target<T, D>(p, i, n, x0, x1, x2);
	double S[D == 3 ? kBondSums3 : kBondSums2] = {};
	int nb = 0;
	for (long long J = 0; J < nt; ++J)
	{
		__syncthreads();
		const long long j = J * kBlock + tid;
		pair_stage<T, D>(p, j, n, src);
		__syncthreads();
		const int cnt = (int)(n - J * kBlock < kBlock ? n - J * kBlock : kBlock);
		for (int u = 0; u < cnt; ++u)
		{
			const double dx = src[0][u] - x0, dy = src[1][u] - x1, dz = D == 3 ? src[2][u] - x2 : 0.0;
			const double r2 = D == 3 ? pair_r2(dx, dy, dz) : pair_r2(dx, dy);
			const bool in = 0.0 < r2 && r2 < R2;
			if (__ballot(in) == 0) continue;
			if (in)
			{
				++nb;
				bond_add<D>(dx, dy, dz, r2, S);
			}
		}
	}
	// (a wave whose first thread has no particle has none at all: it writes no record)
	const long long first = i - (tid & 63);
	if (SUM && first >= n) return;
	bond_finish<D, SUM, VEC>(i < n, i < n ? i : -1, nb, S, nb_out, q_out, SUM ? rec + (first >> 6) * kBondRec : nullptr);
}

// The second pass in the same tiling: vec holds the records in the caller's order, so source u of tile J has its record at row
// J kBlock + u, the same for the whole workgroup.
template <bool SUM>
__global__ __launch_bounds__(kBlock) void bond_solid_exact_kernel(const float *__restrict__ p, long long n, double R2, const double *__restrict__ vec, double dmin,
                                                                   int xi_min, int *__restrict__ nb_out, int *__restrict__ xi_out, double *__restrict__ qbar_out,
                                                                   double *__restrict__ rec)
{
	__shared__ double src[3][kBlock];
	const int tid = threadIdx.x;
	const long long nt = (n + kBlock - 1) / kBlock, i = (long long)blockIdx.x * kBlock + tid;
	double x0, x1, x2;
	pair_target<float, 3>(p, i, n, x0, x1, x2);
	double e[13], T[kBondSums3];
	solid_begin(vec + kBondVec * (i < n ? i : n - 1), e, T);   // (a thread without a particle meets nobody and writes nothing)
	int nb = 0, xi = 0;
	for (long long J = 0; J < nt; ++J)
	{
		__syncthreads();
		const long long j = J * kBlock + tid;
		pair_stage<float, 3>(p, j, n, src);
		__syncthreads();
		const int cnt = (int)(n - J * kBlock < kBlock ? n - J * kBlock : kBlock);
		for (int u = 0; u < cnt; ++u)
		{
			const double dx = src[0][u] - x0, dy = src[1][u] - x1, dz = src[2][u] - x2;
			const double r2 = pair_r2(dx, dy, dz);
			const bool in = 0.0 < r2 && r2 < R2;
			if (__ballot(in) == 0) continue;
			double r[kBondVec];
			solid_record(vec + kBondVec * (J * kBlock + u), r);
			if (in) solid_bond(e, r, dmin, nb, xi, T);
		}
	}
	const long long first = i - (tid & 63);
	if (SUM && first >= n) return;
	solid_finish<SUM>(i < n, i < n ? i : -1, nb, xi, T, xi_min, nb_out, xi_out, qbar_out, SUM ? rec + (first >> 6) * kSolidRec : nullptr);
}
#endif   // NBCO_BOND_EXACT

#ifdef NBCO_BOND_WALK
// ---- tree form: a visitor of the radius walk (kd_radius_walk, pair_stat_kernels.hpp) ----------------------------------------------------
// A lane meets exactly its neighbours, in the order of the leaves: its sums are added in that order.  The particle itself and a
// coincident one fall out through r2 > 0, so the tree position is not asked.  nb and q go through the build's unsort map into the
// caller's order.  With VEC the bond vector records go where q would (bond_finish); with TREE_ROWS to the row of the tree position
// instead, where the second pass of the same call reads them.
template <bool SUM, bool VEC = false, bool TREE_ROWS = false>
__global__ __launch_bounds__(64 * kPairWalkWaves) void kd_bond_walk_kernel(const float *__restrict__ lbound, const float *__restrict__ rbound,
                                                                            const int *__restrict__ mult, const int *__restrict__ index,
                                                                            const float4 *__restrict__ pos, const int *__restrict__ unsort, int ntot, long long n,
                                                                            double R2m, double R2, int *__restrict__ nb_out, double *__restrict__ q_out,
                                                                            double *__restrict__ rec)
{
	__shared__ double tile[kPairWalkWaves][3][64];
	for (int q = 0; q < kPairWalkChunks; ++q)
	{
		const long long s0 = kd_walk_chunk(q), s = s0 + (threadIdx.x & 63);
		if (s0 >= n) break;   // (the whole wave)
		double S[kBondSums3] = {};
		int nb = 0;
		kd_radius_walk(lbound, rbound, mult, index, pos, ntot, n, R2m, s, tile[threadIdx.x >> 6], [&](bool need, long long, long long, double dx, double dy, double dz) {
			const double r2 = pair_r2(dx, dy, dz);
			const bool in = need && 0.0 < r2 && r2 < R2;
			if (__ballot(in) == 0) return;
			if (in)
			{
				++nb;
				bond_add<3>(dx, dy, dz, r2, S);
			}
		});
		const bool valid = s < n;
		bond_finish<3, SUM, VEC>(valid, !valid ? -1 : TREE_ROWS ? s : kd_walk_row(unsort, n, s), nb, S, nb_out, q_out, SUM ? rec + (s0 >> 6) * kBondRec : nullptr);
	}
}

// the caller's records into the tree order: row s of tvec is row unsort[s] of vec (zeros where the map is damaged)
__global__ __launch_bounds__(kBlock) void kd_solid_gather_kernel(const double *__restrict__ vec, const int *__restrict__ unsort, long long n, double *__restrict__ tvec)
{
	for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < kBondVec * n; t += (long long)gridDim.x * kBlock)
	{
		const long long s = t / kBondVec, src = kd_walk_row(unsort, n, s);
		tvec[t] = src >= 0 ? vec[kBondVec * src + (t - kBondVec * s)] : 0.0;
	}
}

// The second pass as a visitor of the same walk.  tvec holds the records in TREE order: the staged particle j has row j, the same in
// every lane, and a leaf's records lie together.  The outputs go through the unsort map into the caller's order.
template <bool SUM>
__global__ __launch_bounds__(64 * kPairWalkWaves) void kd_solid_walk_kernel(const float *__restrict__ lbound, const float *__restrict__ rbound,
                                                                             const int *__restrict__ mult, const int *__restrict__ index,
                                                                             const float4 *__restrict__ pos, const int *__restrict__ unsort, int ntot, long long n,
                                                                             double R2m, double R2, const double *__restrict__ tvec, double dmin, int xi_min,
                                                                             int *__restrict__ nb_out, int *__restrict__ xi_out, double *__restrict__ qbar_out,
                                                                             double *__restrict__ rec)
{
	__shared__ double tile[kPairWalkWaves][3][64];
	for (int q = 0; q < kPairWalkChunks; ++q)
	{
		const long long s0 = kd_walk_chunk(q), s = s0 + (threadIdx.x & 63);
		if (s0 >= n) break;   // (the whole wave)
		const bool valid = s < n;
		double e[13], T[kBondSums3];
		solid_begin(tvec + kBondVec * (valid ? s : n - 1), e, T);
		int nb = 0, xi = 0;
		kd_radius_walk(lbound, rbound, mult, index, pos, ntot, n, R2m, s, tile[threadIdx.x >> 6], [&](bool need, long long, long long j, double dx, double dy, double dz) {
			const double r2 = pair_r2(dx, dy, dz);
			const bool in = need && 0.0 < r2 && r2 < R2;
			if (__ballot(in) == 0) return;
			double r[kBondVec];
			solid_record(tvec + kBondVec * (long long)__builtin_amdgcn_readfirstlane((int)j), r);   // (j < n < 2^29, uniform by the walk)
			if (in) solid_bond(e, r, dmin, nb, xi, T);
		});
		solid_finish<SUM>(valid, valid ? kd_walk_row(unsort, n, s) : -1, nb, xi, T, xi_min, nb_out, xi_out, qbar_out, SUM ? rec + (s0 >> 6) * kSolidRec : nullptr);
	}
}
#endif   // NBCO_BOND_WALK
