// aperture_kernels.hpp -- part of k_reduce.hip (included there, behind beam_diag_kernels.hpp: one translation unit, one anonymous namespace)
// Aperture: which particles are outside a boundary, and the stable compaction of a state without them
// (no include guard on purpose: this is a section of that file, not a header)
// One template covers both states (BeamVec): T = float, D = 3 (xyz triplets) and T = double, D = 2 (xy pairs); a particle's position,
// velocity and acceleration are each moved as one D-vector.
// The particles are cut into tiles of kBlock rows, one workgroup per tile.  A row's slot among the lost rows is the number of lost
// rows before it: the lost rows of the tiles before (a scan of the workgroup counts), of the waves before it in its tile (LDS) and of
// the lanes before it in its wave (the ballot's prefix).  A kept row's slot is its row less that number.  Nothing but the data
// decides a position, so a second call writes the same bytes.

// ---- the rule of include/nbco.h ----------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)   // a contracted u u + v v would move a particle on the surface across it
template <class T, int D> __device__ inline bool aperture_inside(const BeamVec<T, D> &x, const ApRule &ap)
{
	double d[D];
	bool finite = true, box = true;
#pragma unroll
	for (int a = 0; a < D; ++a)
	{
		const double q = (double)x.v[a];
		finite = finite && isfinite(q);
		d[a] = q - ap.centre[a];
		box = box && fabs(d[a]) <= ap.half[a];
	}
	const double ux = d[0] * ap.w[0], uy = d[1] * ap.w[1];
	const double xx = ux * ux, yy = uy * uy;
	double s = xx + yy;
	if (D == 3)
	{
		const double uz = d[D - 1] * ap.w[D - 1];
		const double zz = uz * uz;
		s = s + zz;
	}
	return finite && (ap.shape == NBCO_AP_BOX ? box : s <= 1.0);
}
#pragma clang fp contract(on)   // (the state of k_reduce.hip: the command line's)

// ---- classification: one read of the positions ---------------------------------------------------------------------------------------
// counts[tile] = lost rows of the tile (COUNTS), *total += the same: an integer sum, which does not depend on the order of arrival
// (the host has zeroed it).  A tile that loses nobody adds nothing.
template <class T, int D, bool COUNTS>
__global__ __launch_bounds__(kBlock) void aperture_classify_kernel(const T *__restrict__ p, long long n, ApRule ap, int *__restrict__ counts,
                                                                    unsigned long long *__restrict__ total)
{
	__shared__ int sh[kBlock / 64];
	const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
	bool lost = false;
	if (i < n) lost = !aperture_inside<T, D>(reinterpret_cast<const BeamVec<T, D> *>(p)[i], ap);
	const int in_wave = __popcll(__ballot(lost));
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = in_wave;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		int s = 0;
#pragma unroll
		for (int w = 0; w < kBlock / 64; ++w) s += sh[w];
		if (COUNTS) counts[blockIdx.x] = s;
		if (s) atomicAdd(total, (unsigned long long)s);
	}
}

// ---- scan of the workgroup counts ---------------------------------------------------------------------------------------------------
// One level: every wave takes a group of 64 values, replaces them by their exclusive prefix sums inside the group and writes the
// group's sum to sums[group].  The host applies it level by level until one group holds a whole level; a tile's offset is then the sum
// of its entries of all levels (ApOffsets), so no pass adds the upper levels back down.
constexpr int kApGroupBits = 6;   // 64 values per group: one wave
constexpr int kApLevels = 4;      // 2^31 rows / 256 = 2^23 tiles -> 2^17 -> 2^11 -> 2^5 values

__global__ __launch_bounds__(kBlock) void aperture_scan_kernel(int *__restrict__ v, long long m, int *__restrict__ sums)
{
	const int lane = threadIdx.x & 63;
	const long long group = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), i = (group << kApGroupBits) + lane;
	if ((group << kApGroupBits) >= m) return;   // (the whole wave)
	const int x = i < m ? v[i] : 0;
	int incl = x;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
	{
		const int y = __shfl_up(incl, o);
		if (lane >= o) incl += y;
	}
	if (i < m) v[i] = incl - x;
	if (lane == 63) sums[group] = incl;
}

struct ApOffsets { const int *level[kApLevels]; };   // level[k][tile >> (6 k)]; nullptr from the first level that is not needed

__device__ inline long long aperture_tile_offset(const ApOffsets &off, long long tile)
{
	long long s = off.level[0][tile];
	if (off.level[1]) s += off.level[1][tile >> kApGroupBits];
	if (off.level[2]) s += off.level[2][tile >> (2 * kApGroupBits)];
	if (off.level[3]) s += off.level[3][tile >> (3 * kApGroupBits)];
	return s;
}

// ---- scatter: kept rows of the three blocks -> out = [pos nk | vel nk | acc nk], lost rows -> the record, the order map with the state --
// lost / lost_row / order_in + order_out may be NULL.  The caller has made sure that the record has room for every lost row.
template <class T, int D>
__global__ __launch_bounds__(kBlock) void aperture_scatter_kernel(const T *__restrict__ buf, long long n, long long nk, ApRule ap, ApOffsets off,
                                                                   T *__restrict__ out, T *__restrict__ lost, int *__restrict__ lost_row,
                                                                   const int *__restrict__ order_in, int *__restrict__ order_out)
{
	using V = BeamVec<T, D>;
	__shared__ int sh[kBlock / 64];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
	const V *pos = reinterpret_cast<const V *>(buf), *vel = reinterpret_cast<const V *>(buf + D * n), *acc = reinterpret_cast<const V *>(buf + 2 * D * n);
	V x{};
	bool is_lost = false;
	if (i < n)
	{
		x = pos[i];
		is_lost = !aperture_inside<T, D>(x, ap);
	}
	const unsigned long long m = __ballot(is_lost);
	if (lane == 0) sh[w] = __popcll(m);
	__syncthreads();
	long long before = aperture_tile_offset(off, blockIdx.x);
#pragma unroll
	for (int j = 0; j < kBlock / 64 - 1; ++j) before += j < w ? sh[j] : 0;
	before += __popcll(m & ((1ull << lane) - 1ull));
	if (i >= n) return;
	const V u = vel[i];
	if (!is_lost)
	{
		const long long j = i - before;
		if (!NBCO_CHECKED_OK(j >= 0 && j < nk, NBCO_CHK_GROUP)) return;   // (a survivor's slot: the checked build counts one outside the compacted state)
		reinterpret_cast<V *>(out)[j] = x;
		reinterpret_cast<V *>(out + D * nk)[j] = u;
		reinterpret_cast<V *>(out + 2 * D * nk)[j] = acc[i];
		if (order_out) order_out[j] = order_in[i];
	}
	else
	{
		if (!NBCO_CHECKED_OK(before >= 0 && before < n - nk, NBCO_CHK_GROUP)) return;   // (a lost row's slot in the record of n - nk rows)
		if (lost)
		{
			V *row = reinterpret_cast<V *>(lost) + 2 * before;
			row[0] = x;
			row[1] = u;
		}
		if (lost_row) lost_row[before] = (int)i;
	}
}
