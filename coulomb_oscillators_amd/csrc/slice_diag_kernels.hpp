// slice_diag_kernels.hpp -- part of k_reduce.hip (included there, behind aperture_kernels.hpp: one translation unit, one anonymous namespace)
// Slice diagnostics: the moments of beam_diag_kernels.hpp per slice along one phase-space coordinate
// (no include guard on purpose: this is a section of that file, not a header)
// One template covers both states (BeamVec): T = float, D = 3 and T = double, D = 2.
// A slice is a bin of the histogram's rule (hist_bin) on the slicing coordinate.  The particles are grouped, not accumulated in
// place: the host sorts (key, row) pairs stably by key, so that a slice is one contiguous run of rows in state order.  Every slice is
// cut into chunks of kSliceChunk rows, one workgroup per chunk; a chunk's partial sums go to a slab of its own and one wave per slice
// adds the slabs in chunk order.  Which lane takes which row and which slab is decided by the row's place INSIDE ITS SLICE alone, so
// a slice's sums have the same bits whatever the other slices hold; nothing is accumulated with atomics.
constexpr int kSliceChunk = 1024;   // rows per workgroup (a multiple of kBlock); DESIGN 4 has the values tried
static_assert(kSliceChunk % kBlock == 0, "a chunk is a whole number of passes of a workgroup");

struct SliceAxis
{
	long long off;   // element offset of the slicing coordinate of particle 0
	int bins;
	double lo, hi, scale;
};

// key[i] = the slice of particle i, bins for a particle outside the window.  The coordinate is loaded as hist_kernel loads it: one
// element at a computed offset, no select among the elements of a loaded vector.
template <class T, int D>
__global__ __launch_bounds__(kBlock) void slice_key_kernel(const T *__restrict__ buf, long long n, SliceAxis ax, unsigned *__restrict__ key)
{
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		int b = 0;
		const bool in = hist_bin((double)buf[ax.off + D * i], ax.lo, ax.hi, ax.scale, ax.bins, b);
		key[i] = in ? (unsigned)b : (unsigned)ax.bins;
	}
}

// start[s] = the first place of the sorted keys that holds a key >= s, for s = 0 .. bins + 1: slice s is the run [start[s], start[s + 1]),
// the run of s = bins the particles outside (start[bins + 1] = n)
__global__ __launch_bounds__(kBlock) void slice_start_kernel(const unsigned *__restrict__ key, int n, int bins, int *__restrict__ start)
{
	const int s = blockIdx.x * kBlock + threadIdx.x;
	if (s > bins + 1) return;
	int a = 0, z = n;   // keys before a are below s, keys from z on are not
	while (a < z)
	{
		const int m = a + ((z - a) >> 1);
		if (key[m] < (unsigned)s) a = m + 1;
		else z = m;
	}
	start[s] = a;
}

// chunks of slice s; the scan of these over s = 0 .. bins (the last one 0) is the chunk table: slice s owns the workgroups
// [first[s], first[s + 1]) and first[bins] is their number
struct SliceChunksOf
{
	const int *start;
	int bins;
	__host__ __device__ int operator()(int s) const { return s < bins ? (start[s + 1] - start[s] + kSliceChunk - 1) / kSliceChunk : 0; }
};

// the chunk of this workgroup: its slice s and the places [lo, hi) of the sorted order.  false: a surplus workgroup of the upper bound
// (n: read by the checked build alone, which counts a table that does not bracket this workgroup or a chunk outside [0, n) and drops
// the workgroup)
__device__ inline bool slice_chunk(const int *__restrict__ first, const int *__restrict__ start, int bins, long long n, int &s, int &lo, int &hi)
{
	const int b = blockIdx.x;
	if (b >= first[bins]) return false;
	int a = 0, z = bins;   // first[a] <= b < first[z]
	while (z - a > 1)
	{
		const int m = (a + z) >> 1;
		if (first[m] <= b) a = m;
		else z = m;
	}
	s = a;
	if (!NBCO_CHECKED_OK(first[s] <= b && b < first[s + 1], NBCO_CHK_GROUP)) return false;
	lo = start[s] + (b - first[s]) * kSliceChunk;
	hi = lo + min(kSliceChunk, start[s + 1] - lo);   // (lo + kSliceChunk may pass 2^31 for the last chunk of a state near that size)
	if (!NBCO_CHECKED_OK(0 <= lo && lo <= hi && hi <= n, NBCO_CHK_GROUP)) return false;
	return true;
}

// ---- pass 1: the means, from compensated sums ---------------------------------------------------------------------------------------------
// A slice can be thin: along the slicing coordinate its particles differ by a bin's width, far less than they lie from the origin, and
// the fourth central moments answer an error eps of the mean with 4 eps <d^3>.  The sums of the coordinates are therefore carried as
// (sum, error) pairs -- two_sum keeps what each addition rounds off -- through the lanes, the waves, the chunks and the slabs, and the
// mean is (sum + error) / n.  The error terms themselves are added plainly, so this is a compensated sum of roughly twice the working
// precision, not a guarantee of the correctly rounded one; the order is still fixed.  An infinite coordinate gives inf - inf inside
// two_sum: that coordinate's mean of that slice is NaN, where a plain sum would have said inf.
__device__ inline void two_sum(double &s, double &c, double q, double qc)   // (s, c) += (q, qc); Knuth's form is exact for any magnitudes
{
	const double t = s + q, bp = t - s, e = (s - (t - bp)) + (q - bp);
	s = t;
	c += qc + e;
}

__device__ inline void wave_two_sum(double &s, double &c)
{
	for (int o = 32; o > 0; o >>= 1)
	{
		const double so = __shfl_xor(s, o), co = __shfl_xor(c, o);
		two_sum(s, c, so, co);
	}
}

// pass 1, first stage: per chunk the slab [sums Q | minima Q | maxima Q | errors of the sums Q]
template <class T, int D>
__global__ __launch_bounds__(kBlock) void slice_sums_stage1(const T *__restrict__ buf, long long n, const int *__restrict__ perm, const int *__restrict__ first,
                                                             const int *__restrict__ start, int bins, double *__restrict__ part)
{
	constexpr int Q = 2 * D;
	int slice, lo, hi;
	if (!slice_chunk(first, start, bins, n, slice, lo, hi)) return;   // (the whole workgroup)
	double s[Q], c[Q], mn[Q], mx[Q];
#pragma unroll
	for (int a = 0; a < Q; ++a) { s[a] = 0; c[a] = 0; mn[a] = DBL_MAX; mx[a] = -DBL_MAX; }
	for (int j = lo + threadIdx.x; j < hi; j += kBlock)
	{
		double q[Q];
		const int row = NBCO_CHECKED_OK((unsigned)perm[j] < (unsigned long long)n, NBCO_CHK_GROUP) ? perm[j] : 0;   // (the sort's permutation of [0, n))
		beam_load<T, D>(buf, n, row, q);
#pragma unroll
		for (int a = 0; a < Q; ++a) { two_sum(s[a], c[a], q[a], 0.0); mn[a] = fmin(mn[a], q[a]); mx[a] = fmax(mx[a], q[a]); }
	}
	__shared__ double sh[kBlock / 64][4 * Q];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int a = 0; a < Q; ++a) { wave_two_sum(s[a], c[a]); mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
	if (lane == 0)
#pragma unroll
		for (int a = 0; a < Q; ++a) { sh[w][a] = s[a]; sh[w][Q + a] = mn[a]; sh[w][2 * Q + a] = mx[a]; sh[w][3 * Q + a] = c[a]; }
	__syncthreads();
	double *slab = part + (size_t)blockIdx.x * 4 * Q;
	if (threadIdx.x < Q)
	{
		double t = sh[0][threadIdx.x], e = sh[0][3 * Q + threadIdx.x];
		for (int j = 1; j < kBlock / 64; ++j) two_sum(t, e, sh[j][threadIdx.x], sh[j][3 * Q + threadIdx.x]);
		slab[threadIdx.x] = t;
		slab[3 * Q + threadIdx.x] = e;
	}
	else if (threadIdx.x < 3 * Q)
	{
		const bool low = threadIdx.x < 2 * Q;
		double v = sh[0][threadIdx.x];
		for (int j = 1; j < kBlock / 64; ++j) v = low ? fmin(v, sh[j][threadIdx.x]) : fmax(v, sh[j][threadIdx.x]);
		slab[threadIdx.x] = v;
	}
}

// pass 1, last stage (one wave per slice, lane l takes the chunks l, l + 64, ..): rec[a] = mean, rec[Q + a] = min, rec[2 Q + a] = max
// of the slice, rec = out + s * stride.  As in beam_sums_stage2 a coordinate that is the same in every particle is its own mean.  An
// empty slice: zeros.
template <int Q>
__global__ __launch_bounds__(kBlock) void slice_sums_stage2(const double *__restrict__ part, const int *__restrict__ first, const int *__restrict__ start,
                                                             int bins, int stride, double *__restrict__ out)
{
	const int slice = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (slice >= bins) return;   // (the whole wave)
	// (the checked build counts a run of slabs outside the chunk table and takes the slice's chunks as none)
	const int c0 = first[slice], cnt = start[slice + 1] - start[slice];
	const int c1 = NBCO_CHECKED_OK(0 <= c0 && c0 <= first[slice + 1] && first[slice + 1] <= first[bins], NBCO_CHK_GROUP) ? first[slice + 1] : c0;
	double *rec = out + (size_t)slice * stride;
#pragma unroll
	for (int a = 0; a < Q; ++a)
	{
		double s = 0, c = 0, mn = DBL_MAX, mx = -DBL_MAX;
		for (int b = c0 + lane; b < c1; b += 64)
		{
			const double *slab = part + (size_t)b * 4 * Q;
			two_sum(s, c, slab[a], slab[3 * Q + a]);
			mn = fmin(mn, slab[Q + a]);
			mx = fmax(mx, slab[2 * Q + a]);
		}
		wave_two_sum(s, c);
		mn = wave_min(mn); mx = wave_max(mx);
		if (lane == 0)
		{
			rec[a] = !cnt ? 0.0 : mn == mx ? mn : (s + c) / (double)cnt;
			rec[Q + a] = cnt ? mn : 0.0;
			rec[2 * Q + a] = cnt ? mx : 0.0;
		}
	}
}

// pass 2, first stage: per chunk the sums of the central products (beam_central_add) about the mean of the chunk's slice
template <class T, int D>
__global__ __launch_bounds__(kBlock) void slice_central_stage1(const T *__restrict__ buf, long long n, const int *__restrict__ perm, const int *__restrict__ first,
                                                                const int *__restrict__ start, int bins, int stride, const double *__restrict__ out,
                                                                double *__restrict__ part)
{
	constexpr int Q = 2 * D, K = beam_central_count(D);
	int slice, lo, hi;
	if (!slice_chunk(first, start, bins, n, slice, lo, hi)) return;   // (the whole workgroup)
	const double *mean = out + (size_t)slice * stride;
	double m[Q], acc[K];
#pragma unroll
	for (int a = 0; a < Q; ++a) m[a] = mean[a];
#pragma unroll
	for (int k = 0; k < K; ++k) acc[k] = 0;
	for (int j = lo + threadIdx.x; j < hi; j += kBlock)
	{
		double d[Q];
		const int row = NBCO_CHECKED_OK((unsigned)perm[j] < (unsigned long long)n, NBCO_CHK_GROUP) ? perm[j] : 0;
		beam_load<T, D>(buf, n, row, d);
#pragma unroll
		for (int a = 0; a < Q; ++a) d[a] -= m[a];
		beam_central_add<D>(d, acc);
	}
	beam_block_sum<K>(acc, part + (size_t)blockIdx.x * K);
}

// pass 2, last stage (one wave per slice, as above): rec[3 Q + k] = the sum over the slice (the host divides by its population)
template <int Q, int K>
__global__ __launch_bounds__(kBlock) void slice_central_stage2(const double *__restrict__ part, const int *__restrict__ first, int bins, int stride,
                                                                double *__restrict__ out)
{
	const int slice = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (slice >= bins) return;   // (the whole wave)
	const int c0 = first[slice];
	const int c1 = NBCO_CHECKED_OK(0 <= c0 && c0 <= first[slice + 1] && first[slice + 1] <= first[bins], NBCO_CHK_GROUP) ? first[slice + 1] : c0;
	double *rec = out + (size_t)slice * stride + 3 * Q;
#pragma unroll
	for (int k = 0; k < K; ++k)
	{
		double s = 0;
		for (int b = c0 + lane; b < c1; b += 64) s += part[(size_t)b * K + k];
		s = wave_sum(s);
		if (lane == 0) rec[k] = s;
	}
}
