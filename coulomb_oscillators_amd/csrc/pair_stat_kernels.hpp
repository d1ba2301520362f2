// pair_stat_kernels.hpp -- part of k_reduce.hip (the exact forms, with NBCO_PAIR_STAT_EXACT defined) and of k_fmm_kd.hip (the tree
// walk, with NBCO_PAIR_STAT_WALK defined): included there, in this place, inside that file's anonymous namespace
// Pair statistics: histogram of the pair distances below rmax and the squared distance to the nearest neighbour
// (no include guard on purpose: this is a section of those files, not a header)
// The pair rule of include/nbco.h, in fp64 over the widened coordinates and without a square root that decides anything:
//   r2 = (dx dx + dy dy) + dz dz, every product and sum rounded once; inside iff r2 < R2 (a NaN is outside);
//   bin = the largest b in [0, bins) with lower2(b) <= r2, lower2(b) = e e, e = (double) b * width.
// r2 is the same bits from either end of a pair, counts are integers and a minimum over non-negative doubles is the minimum of their
// bit patterns as unsigned integers: nothing depends on the order of arrival, and the tree walk returns the bytes of the exact form.

// ---- shared arithmetic -----------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)   // a contracted dx dx + dy dy moves a pair across a bin edge once in millions of pairs
__device__ inline double pair_r2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
__device__ inline double pair_r2(double dx, double dy) { return dx * dx + dy * dy; }
__device__ inline double pair_lower2(int b, double width)
{
	const double e = (double)b * width;
	return e * e;
}
// bin of an inside pair (0 <= r2 < R2).  The square root only makes the first guess; the two loops settle the bin by the rule, so how a
// device rounds the root does not matter.  lower2(0) = 0 <= r2 ends the first loop, bins - 1 the second.
__device__ inline int pair_bin(double r2, const PairBins &pb)
{
	const double g = sqrt(r2) * pb.inv_width;
	int b = g < (double)(pb.bins - 1) ? (int)g : pb.bins - 1;
	while (r2 < pair_lower2(b, pb.width)) --b;
	while (b + 1 < pb.bins && r2 >= pair_lower2(b + 1, pb.width)) ++b;
	return b;
}
#ifdef NBCO_PAIR_STAT_WALK
#pragma clang fp contract(fast)   // (the state of k_fmm_kd.hip at this place)
#else
#pragma clang fp contract(on)   // (the state of k_reduce.hip: the command line's)
#endif

constexpr int kPairLdsBins = 16384;   // = kHistLdsBins: 64 KB of 32-bit counters in LDS
constexpr unsigned long long kPairInfBits = 0x7FF0000000000000ull;   // +infinity: "no partner inside"

// One more pair in bin b for every lane that has `in` set.  Called in wave-uniform control flow with m = __ballot(in) != 0.  When all
// those lanes hit one bin (coincident particles, bins = 1, a wide bin) one lane adds the population count: 64 adds to one LDS word
// would serialise.
template <bool LDS>
__device__ inline void pair_count(bool in, unsigned long long m, int b, unsigned *hist, unsigned long long *__restrict__ counts)
{
	const int first = __builtin_ctzll(m);
	const int b0 = __builtin_amdgcn_readlane(b, first);
	if (__ballot(in && b == b0) == m)
	{
		if ((int)(threadIdx.x & 63) == first)
		{
			if (LDS) atomicAdd(&hist[b0], (unsigned)__popcll(m));
			else atomicAdd(&counts[b0], (unsigned long long)__popcll(m));
		}
	}
	else if (in)
	{
		if (LDS) atomicAdd(&hist[b], 1u);
		else atomicAdd(&counts[b], 1ull);
	}
}

// the workgroup's non-zero bins -> the 64-bit global counts (the caller has put a barrier behind the last LDS add)
__device__ inline void pair_flush(const unsigned *hist, int bins, unsigned long long *__restrict__ counts)
{
	for (int b = threadIdx.x; b < bins; b += blockDim.x)
	{
		const unsigned v = hist[b];
		if (v) atomicAdd(&counts[b], (unsigned long long)v);
	}
}

#ifdef NBCO_PAIR_STAT_EXACT
// ---- exact form: all pairs ---------------------------------------------------------------------------------------------------------
// One template covers both states (BeamVec): T = float, D = 3 and T = double, D = 2.  The particles are cut into tiles of kBlock; a
// workgroup keeps the particles of tile I in registers, one per thread, and takes source tiles J >= I through LDS, widened once when
// they are staged: the tile pairs are a triangle, and in the diagonal tile a thread takes the sources behind its own particle, so
// every unordered pair is evaluated once.  Workgroup (I, y) takes the source tiles I + c kPairSrcTiles .. of the chunks c = y,
// y + gridDim.y, ..  A pair outside costs the subtractions, the products and sums of r2, one compare and the wave's branch on the
// ballot.  A pair inside goes into the workgroup's LDS histogram (or, above kPairLdsBins bins, straight to the global counts), its r2
// into the target's minimum in a register and into the source's minimum in LDS, which is folded into nn2 with a 64-bit integer
// minimum when the tile is done.
// 32-bit LDS counters: a workgroup flushes once, at its end, and bins at most kBlock^2 pairs per source tile, kPairSrcTiles tiles per
// chunk and ceil(chunks / gridDim.y) chunks.  n < 2^31 gives fewer than 2^23 tiles and 2^19 chunks; the launch takes gridDim.y =
// min(chunks, kPairGridY), so a workgroup bins at most 2^16 * 2^4 * 2^9 = 2^29 pairs between its zeroing and its flush.
constexpr int kPairSrcTiles = 16;
constexpr int kPairGridY = 1024;
static_assert(kPairLdsBins == kHistLdsBins, "one LDS histogram size for the density maps and the pair statistics");
static_assert((long long)kBlock * kBlock * kPairSrcTiles * ((1LL << 31) / kBlock / kPairSrcTiles / kPairGridY) < (1LL << 32), "LDS counters could wrap");

// particle i of p, widened (2-D: x2 is left as it is)
template <class T, int D>
__device__ inline void pair_widen(const T *__restrict__ p, long long i, double &x0, double &x1, double &x2)
{
	const BeamVec<T, D> q = reinterpret_cast<const BeamVec<T, D> *>(p)[i];
	x0 = (double)q.v[0]; x1 = (double)q.v[1];
	if (D == 3) x2 = (double)q.v[D - 1];
}
// a thread's own particle i; a thread without one carries NaNs: none of its pairs is inside, nobody is its neighbour
template <class T, int D>
__device__ inline void pair_target(const T *__restrict__ p, long long i, long long n, double &x0, double &x1, double &x2)
{
	x0 = x1 = x2 = __longlong_as_double(0x7FF8000000000000ll);
	if (i < n) pair_widen<T, D>(p, i, x0, x1, x2);
}
// a thread's share of a source tile: particle j, widened once, into its slot of the LDS tile (the caller's barriers around it)
template <class T, int D>
__device__ inline void pair_stage(const T *__restrict__ p, long long j, long long n, double (*__restrict__ src)[kBlock])
{
	if (j < n) pair_widen<T, D>(p, j, src[0][threadIdx.x], src[1][threadIdx.x], src[2][threadIdx.x]);
}

template <int D, bool LDS, bool WANT_CNT, bool WANT_NN, bool DIAG>
__device__ inline void pair_tile(double x0, double x1, double x2, const double (*__restrict__ src)[kBlock], int cnt, const PairBins &pb, unsigned *hist,
                                 unsigned long long *__restrict__ counts, unsigned long long *smin, double &tmin)
{
	for (int u = 0; u < cnt; ++u)
	{
		const double r2 = D == 3 ? pair_r2(x0 - src[0][u], x1 - src[1][u], x2 - src[2][u]) : pair_r2(x0 - src[0][u], x1 - src[1][u]);
		bool in = r2 < pb.R2;
		if (DIAG) in = in && u > (int)threadIdx.x;
		const unsigned long long m = __ballot(in);
		if (m == 0) continue;
		if (WANT_NN && in)
		{
			tmin = fmin(tmin, r2);
			atomicMin(&smin[u], (unsigned long long)__double_as_longlong(r2));
		}
		if (WANT_CNT) pair_count<LDS>(in, m, in ? pair_bin(r2, pb) : 0, hist, counts);
	}
}

template <class T, int D, bool LDS, bool WANT_CNT, bool WANT_NN>
__global__ __launch_bounds__(kBlock) void pair_hist_kernel(const T *__restrict__ p, long long n, PairBins pb, unsigned long long *__restrict__ counts,
                                                            unsigned long long *__restrict__ nn2)
{
	extern __shared__ unsigned pair_hist_sh[];
	__shared__ double src[3][kBlock];
	__shared__ unsigned long long smin[kBlock];
	const int tid = threadIdx.x;
	const long long nt = (n + kBlock - 1) / kBlock, I = blockIdx.x;
	if (I + (long long)blockIdx.y * kPairSrcTiles >= nt) return;   // (the whole workgroup: its first chunk is beyond the last tile)
	if (WANT_CNT && LDS)
		for (int b = tid; b < pb.bins; b += kBlock) pair_hist_sh[b] = 0u;   // (the tile loop's first barrier comes before any add)
	const long long i = I * kBlock + tid;
	double x0, x1, x2;
	pair_target<T, D>(p, i, n, x0, x1, x2);
	double tmin = __longlong_as_double((long long)kPairInfBits);
	for (long long c0 = blockIdx.y;; c0 += gridDim.y)
	{
		const long long J0 = I + c0 * kPairSrcTiles;
		if (J0 >= nt) break;
		const long long J1 = J0 + kPairSrcTiles < nt ? J0 + kPairSrcTiles : nt;
		for (long long J = J0; J < J1; ++J)
		{
			__syncthreads();
			const long long j = J * kBlock + tid;
			pair_stage<T, D>(p, j, n, src);
			if (WANT_NN) smin[tid] = kPairInfBits;
			__syncthreads();
			const int cnt = (int)(n - J * kBlock < kBlock ? n - J * kBlock : kBlock);
			if (J == I) pair_tile<D, LDS, WANT_CNT, WANT_NN, true>(x0, x1, x2, src, cnt, pb, pair_hist_sh, counts, smin, tmin);
			else pair_tile<D, LDS, WANT_CNT, WANT_NN, false>(x0, x1, x2, src, cnt, pb, pair_hist_sh, counts, smin, tmin);
			if (WANT_NN)
			{
				__syncthreads();
				if (tid < cnt && smin[tid] != kPairInfBits) atomicMin(&nn2[j], smin[tid]);
			}
		}
	}
	if (WANT_NN && i < n && tmin < __longlong_as_double((long long)kPairInfBits)) atomicMin(&nn2[i], (unsigned long long)__double_as_longlong(tmin));
	if (WANT_CNT && LDS)
	{
		__syncthreads();
		pair_flush(pair_hist_sh, pb.bins, counts);
	}
}

__global__ __launch_bounds__(kBlock) void pair_fill_kernel(unsigned long long *__restrict__ v, long long n, unsigned long long bits)
{
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) v[i] = bits;
}
#endif   // NBCO_PAIR_STAT_EXACT

// counts[bins] = total - sum of counts[0 .. bins): the pairs outside, so that the hot loops do not count them (one workgroup)
__global__ __launch_bounds__(kBlock) void pair_outside_kernel(unsigned long long *__restrict__ counts, int bins, unsigned long long total)
{
	__shared__ unsigned long long sh[kBlock];
	unsigned long long s = 0;
	for (int b = threadIdx.x; b < bins; b += kBlock) s += counts[b];
	sh[threadIdx.x] = s;
	__syncthreads();
	for (int o = kBlock / 2; o > 0; o >>= 1)
	{
		if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
		__syncthreads();
	}
	if (threadIdx.x == 0) counts[bins] = total - sh[0];
}

#ifdef NBCO_PAIR_STAT_WALK
// ---- tree form: the radius walk, for every diagnostic over the neighbours within a radius --------------------------------------------
// One wave takes 64 consecutive particles of the tree order -- neighbours in space already -- and goes through the implicit tree
// without a stack (kd_walk_next); the current node is the same in every lane, so its box is scalar loads.  A lane needs a node iff the
// squared distance from its particle to the node's box, per axis max(lb - x, 0, x - rb) in fp64, is <= R2 (1 + 1e-9): the box holds the
// node's particles, so no pair inside is behind a node that is not needed, and the margin is far above any rounding of the comparison
// and free, because the result does not depend on what is opened -- the tree decides only what is skipped.  The wave opens a node iff a
// lane needs it.  A leaf's particles are staged in the wave's LDS tile, 64 at a time, and every lane hands each of them to its visitor,
// in wave-uniform control flow: visit(need, s, j, dx, dy, dz) with the lane's `need` of the leaf, the tree positions s of the lane's
// particle and j of the staged one, and (dx, dy, dz) = staged - own in fp64.  A lane meets its neighbours in the order of the leaves
// and, within a leaf, of the tree positions, whatever its neighbours in the wave need.
// A workgroup is kPairWalkWaves waves; every wave takes kPairWalkChunks chunks of 64 (kd_walk_chunk).
constexpr int kPairWalkWaves = 4, kPairWalkChunks = 4;
constexpr int kPairWgParticles = 64 * kPairWalkWaves * kPairWalkChunks;

// A walk kernel's parameter list begins with the tree, which launch_radius_walk (k_fmm_kd.hip) fills in: boxes, leaf ranges,
// tree-ordered positions, the map into the caller's order, ntot, n and R2m = R2 (1 + 1e-9).  They are kernel parameters of their own,
// const and __restrict__, and not members of a struct (measured: as members the boxes become vector loads): a visitor may issue global
// atomics, and the boxes stay scalar loads only while the compiler knows that nothing writes them.

// the first tree position of this wave's q-th chunk (at or beyond n: the wave is done)
__device__ inline long long kd_walk_chunk(int q) { return (((long long)blockIdx.x * kPairWalkWaves + (threadIdx.x >> 6)) * kPairWalkChunks + q) * 64; }

// the caller's row of tree position s < n, or -1 (a permutation of [0, n) by the build; the check keeps a damaged map from writing
// outside the outputs)
__device__ inline long long kd_walk_row(const int *__restrict__ unsort, long long n, long long s)
{
	const long long dst = unsort[s];
	(void)NBCO_CHECKED_OK(dst >= 0 && dst < n, NBCO_CHK_WALK);
	return dst >= 0 && dst < n ? dst : -1;
}

// the walk of the 64 particles at tree positions s0 .. s0 + 63 (s = s0 + lane; s0 < n and wave-uniform); tile is this wave's own
template <class Visit>
__device__ inline void kd_radius_walk(const float *__restrict__ lbound, const float *__restrict__ rbound, const int *__restrict__ mult,
                                      const int *__restrict__ index, const float4 *__restrict__ pos, int ntot, long long n, double R2m, long long s,
                                      double (&tile)[3][64], Visit visit)
{
	const int lane = threadIdx.x & 63;
	const bool valid = s < n;
	const float4 me = pos[valid ? s : n - 1];
	const double X = (double)me.x, Y = (double)me.y, Z = (double)me.z;
	int k = 0;
	for (;;)
	{
		k = __builtin_amdgcn_readfirstlane(k);   // (uniform by construction: it moves on ballots only)
		const double gx = fmax(fmax((double)lbound[3 * k] - X, 0.0), X - (double)rbound[3 * k]);
		const double gy = fmax(fmax((double)lbound[3 * k + 1] - Y, 0.0), Y - (double)rbound[3 * k + 1]);
		const double gz = fmax(fmax((double)lbound[3 * k + 2] - Z, 0.0), Z - (double)rbound[3 * k + 2]);
		const bool need = valid && gx * gx + gy * gy + gz * gz <= R2m;
		const bool any_need = __ballot(need) != 0;
		const bool leaf = 2 * k + 1 >= ntot;
		if (leaf && any_need)
		{
			// (a leaf's range lies inside [0, n) by the build; the clamp keeps a damaged tree from reading past the array, and the
			// checked build counts what the clamp would have hidden)
			const long long i0 = index[k];
			long long ml = mult[k];
			(void)NBCO_CHECKED_OK(i0 >= 0 && ml >= 0 && i0 + ml <= n, NBCO_CHK_WALK);
			if (i0 < 0 || i0 >= n) ml = 0;
			else if (ml > n - i0) ml = n - i0;
			for (long long j0 = 0; j0 < ml; j0 += 64)
			{
				wave_lds_sync();
				if (j0 + lane < ml)
				{
					const float4 v = pos[i0 + j0 + lane];
					tile[0][lane] = (double)v.x; tile[1][lane] = (double)v.y; tile[2][lane] = (double)v.z;
				}
				wave_lds_sync();
				const int cnt = (int)(ml - j0 < 64 ? ml - j0 : 64);
				for (int u = 0; u < cnt; ++u) visit(need, s, i0 + j0 + u, tile[0][u] - X, tile[1][u] - Y, tile[2][u] - Z);
			}
		}
		k = kd_walk_next(k, !leaf && any_need);
		if (k == 0) break;
	}
}

// Pair statistics as a visitor: the pair rule, self excluded by tree position.  A lane counts a pair only from the lower position and
// takes the minimum from both (each end meets the pair on its own walk), so nn2 needs no atomics.  One LDS histogram per workgroup,
// one flush for kPairWgParticles particles.  32-bit LDS counters: a particle counts fewer than n pairs, so a workgroup bins fewer
// than kPairWgParticles * n between its zeroing and its flush: the launch takes the LDS form only while that is below 2^32
// (kd_pair_hist_tree).
template <bool LDS, bool WANT_CNT, bool WANT_NN>
__global__ __launch_bounds__(64 * kPairWalkWaves) void kd_pair_walk_kernel(const float *__restrict__ lbound, const float *__restrict__ rbound,
                                                                            const int *__restrict__ mult, const int *__restrict__ index,
                                                                            const float4 *__restrict__ pos, const int *__restrict__ unsort, int ntot, long long n,
                                                                            double R2m, PairBins pb, unsigned long long *__restrict__ counts, double *__restrict__ nn2)
{
	extern __shared__ unsigned pair_hist_sh[];
	__shared__ double tile[kPairWalkWaves][3][64];
	if (WANT_CNT && LDS)
	{
		for (int b = threadIdx.x; b < pb.bins; b += 64 * kPairWalkWaves) pair_hist_sh[b] = 0u;
		__syncthreads();
	}
	for (int q = 0; q < kPairWalkChunks; ++q)
	{
		const long long s0 = kd_walk_chunk(q), s = s0 + (threadIdx.x & 63);
		if (s0 >= n) break;   // (the whole wave)
		double tmin = __longlong_as_double((long long)kPairInfBits);
		kd_radius_walk(lbound, rbound, mult, index, pos, ntot, n, R2m, s, tile[threadIdx.x >> 6], [&](bool need, long long, long long j, double dx, double dy, double dz) {
			// (& and not &&: with && the compiler guards r2 by a branch on `need` per staged source in the instance without a ballot)
			const double r2 = pair_r2(dx, dy, dz);
			const bool in = need & (r2 < pb.R2) & (j != s);
			if (WANT_NN && in) tmin = fmin(tmin, r2);
			if (WANT_CNT)
			{
				const bool mine = in && s < j;
				const unsigned long long m = __ballot(mine);
				if (m != 0) pair_count<LDS>(mine, m, mine ? pair_bin(r2, pb) : 0, pair_hist_sh, counts);
			}
		});
		if (WANT_NN && s < n)
		{
			const long long dst = kd_walk_row(unsort, n, s);
			if (dst >= 0) nn2[dst] = tmin;
		}
	}
	if (WANT_CNT && LDS)
	{
		__syncthreads();
		pair_flush(pair_hist_sh, pb.bins, counts);
	}
}
#endif   // NBCO_PAIR_STAT_WALK
