// beam_diag_kernels.hpp -- part of k_reduce.hip (included there, in this place: one translation unit, one anonymous namespace)
// Beam diagnostics: phase-space moments (two reduction passes) and density maps (integer histograms) of a state
// (no include guard on purpose: this is a section of that file, not a header)
// One template covers both states: T = float, D = 3 (xyz triplets, 12-byte stride) and T = double, D = 2 (xy pairs, 16-byte stride).
// A particle's position and velocity are each loaded as one D-vector (global_load_dwordx3 / dwordx4: the structs below promise no
// more alignment than the element's, which is all a caller's buffer guarantees).
// Moments follow the pattern of this file: grid-stride loads -> per-lane fp64 accumulators -> one wave64 reduction per accumulator
// -> LDS across the 4 waves -> one partial slab per block -> a last stage in a single block.  The order of every sum is fixed.

template <class T, int D> struct BeamVec;
template <> struct alignas(4) BeamVec<float, 3> { float v[3]; };
template <> struct alignas(8) BeamVec<double, 2> { double v[2]; };

__device__ inline double wave_min(double v) { for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o)); return v; }
__device__ inline double wave_max(double v) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o)); return v; }

// q = (x.., v..) of particle i, widened to double (exact)
template <class T, int D> __device__ inline void beam_load(const T *__restrict__ buf, long long n, long long i, double (&q)[2 * D])
{
	const BeamVec<T, D> x = reinterpret_cast<const BeamVec<T, D> *>(buf)[i];
	const BeamVec<T, D> u = reinterpret_cast<const BeamVec<T, D> *>(buf + D * n)[i];
#pragma unroll
	for (int a = 0; a < D; ++a) { q[a] = (double)x.v[a]; q[D + a] = (double)u.v[a]; }
}

// v[0 .. K) summed over the block in a fixed order -> slab[0 .. K)
template <int K> __device__ inline void beam_block_sum(double (&v)[K], double *__restrict__ slab)
{
	__shared__ double sh[kBlock / 64][K];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
	if (lane == 0)
#pragma unroll
		for (int k = 0; k < K; ++k) sh[w][k] = v[k];
	__syncthreads();
	if (threadIdx.x < K)
	{
		double s = sh[0][threadIdx.x];
		for (int j = 1; j < kBlock / 64; ++j) s += sh[j][threadIdx.x];
		slab[threadIdx.x] = s;
	}
}

// pass 1, first stage: per block the sums of the 2 D coordinates, then their minima, then their maxima (3 * 2 D doubles)
template <class T, int D>
__global__ __launch_bounds__(kBlock) void beam_sums_stage1(const T *__restrict__ buf, long long n, double *__restrict__ part)
{
	constexpr int Q = 2 * D;
	double s[Q], mn[Q], mx[Q];
#pragma unroll
	for (int a = 0; a < Q; ++a) { s[a] = 0; mn[a] = DBL_MAX; mx[a] = -DBL_MAX; }
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		double q[Q];
		beam_load<T, D>(buf, n, i, q);
#pragma unroll
		for (int a = 0; a < Q; ++a) { s[a] += q[a]; mn[a] = fmin(mn[a], q[a]); mx[a] = fmax(mx[a], q[a]); }
	}
	double *slab = part + (size_t)blockIdx.x * 3 * Q;
	__shared__ double sh[kBlock / 64][2 * Q];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int a = 0; a < Q; ++a) { mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
	if (lane == 0)
#pragma unroll
		for (int a = 0; a < Q; ++a) { sh[w][a] = mn[a]; sh[w][Q + a] = mx[a]; }
	beam_block_sum<Q>(s, slab);   // (its barrier also publishes sh)
	if (threadIdx.x < 2 * Q)
	{
		const bool lo = threadIdx.x < Q;
		double v = sh[0][threadIdx.x];
		for (int j = 1; j < kBlock / 64; ++j) v = lo ? fmin(v, sh[j][threadIdx.x]) : fmax(v, sh[j][threadIdx.x]);
		slab[Q + threadIdx.x] = v;
	}
}

// pass 1, last stage (one block; wave w takes the coordinates w, w + 4): out[a] = mean, out[6 + a] = min, out[12 + a] = max.
// A coordinate that is the same in every particle is its own mean: its deviations are exactly 0 whatever n copies sum to.
template <int Q>
__global__ __launch_bounds__(kBlock) void beam_sums_stage2(const double *__restrict__ part, int nblocks, long long n, double *__restrict__ out)
{
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (int a = w; a < Q; a += kBlock / 64)
	{
		double s = 0, mn = DBL_MAX, mx = -DBL_MAX;
		for (int b = lane; b < nblocks; b += 64)
		{
			const double *slab = part + (size_t)b * 3 * Q;
			s += slab[a];
			mn = fmin(mn, slab[Q + a]);
			mx = fmax(mx, slab[2 * Q + a]);
		}
		s = wave_sum(s); mn = wave_min(mn); mx = wave_max(mx);
		if (lane == 0)
		{
			out[a] = mn == mx ? mn : s / (double)n;
			out[6 + a] = mn;
			out[12 + a] = mx;
		}
	}
}

// number of central sums: the upper triangle of the covariance, then 5 fourth-order products per plane (q_k, p_k)
constexpr int beam_central_count(int D) { return D * (2 * D + 1) + 5 * D; }

// acc += the central products of one particle's deviations d: d_a d_b (a <= b, row by row), then per plane k with x = d_k,
// e = d_(D + k): x^4, x^3 e, x^2 e^2, x e^3, e^4
template <int D> __device__ inline void beam_central_add(const double (&d)[2 * D], double (&acc)[beam_central_count(D)])
{
	constexpr int Q = 2 * D;
	int k = 0;
#pragma unroll
	for (int a = 0; a < Q; ++a)
#pragma unroll
		for (int b = a; b < Q; ++b) acc[k++] += d[a] * d[b];
#pragma unroll
	for (int p = 0; p < D; ++p)
	{
		const double x2 = d[p] * d[p], e2 = d[D + p] * d[D + p], xe = d[p] * d[D + p];
		acc[k++] += x2 * x2;
		acc[k++] += x2 * xe;
		acc[k++] += x2 * e2;
		acc[k++] += xe * e2;
		acc[k++] += e2 * e2;
	}
}

// pass 2, first stage: d = (double) q - mean; per block the sums of the central products
template <class T, int D>
__global__ __launch_bounds__(kBlock) void beam_central_stage1(const T *__restrict__ buf, long long n, const double *__restrict__ mean,
                                                               double *__restrict__ part)
{
	constexpr int Q = 2 * D, K = beam_central_count(D);
	double m[Q], acc[K];
#pragma unroll
	for (int a = 0; a < Q; ++a) m[a] = mean[a];
#pragma unroll
	for (int k = 0; k < K; ++k) acc[k] = 0;
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		double d[Q];
		beam_load<T, D>(buf, n, i, d);
#pragma unroll
		for (int a = 0; a < Q; ++a) d[a] -= m[a];
		beam_central_add<D>(d, acc);
	}
	beam_block_sum<K>(acc, part + (size_t)blockIdx.x * K);
}

// pass 2, last stage (one block; wave w takes the sums w, w + 4, ..): out[k] = the sum over all particles (the host divides by n)
__global__ __launch_bounds__(kBlock) void beam_central_stage2(const double *__restrict__ part, int nblocks, int K, double *__restrict__ out)
{
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (int k = w; k < K; k += kBlock / 64)
	{
		double s = 0;
		for (int b = lane; b < nblocks; b += 64) s += part[(size_t)b * K + k];
		s = wave_sum(s);
		if (lane == 0) out[k] = s;
	}
}

// ---- density maps ------------------------------------------------------------------------------------------------------------------
// The bin rule of include/nbco.h, in fp64 over the widened coordinate: inside iff q >= lo && q < hi on every axis (a NaN fails
// both), b = (int) ((q - lo) * scale) clamped to bins - 1.  Subtract, then multiply: there is no multiply-add to fuse.
// While the B bins fit kHistLdsBins 32-bit counters (64 KB of the CU's 160 KB: two workgroups per CU), every workgroup bins its
// share into LDS with 32-bit LDS atomics and adds its non-zero bins to the 64-bit global counts; above that it adds straight to
// the global counts.  Integer sums do not depend on the order of arrival.  The particles outside the window cost one add per
// wave: the population counts of the ballots, kept in a wave-uniform register.
constexpr int kHistLdsBins = 16384;
constexpr int kHistPerBlock = 4096;   // particles per workgroup of the LDS form, so that a bin is flushed once per many hits

struct HistAxes
{
	long long off0, off1;   // element offset of the coordinate of particle 0
	int bins0, bins1, two;
	double lo0, hi0, scale0, lo1, hi1, scale1;
};

__device__ inline bool hist_bin(double q, double lo, double hi, double scale, int bins, int &b)
{
	const bool in = q >= lo && q < hi;
	const double t = (q - lo) * scale;
	b = !in ? 0 : t < (double)bins ? (int)t : bins - 1;
	return in;
}

template <class T, int D, bool LDS>
__global__ __launch_bounds__(kBlock) void hist_kernel(const T *__restrict__ buf, long long n, HistAxes ax, unsigned long long *__restrict__ counts)
{
	extern __shared__ unsigned hist_sh[];
	const int B = ax.bins0 * ax.bins1;
	if (LDS)
	{
		for (int b = threadIdx.x; b < B; b += kBlock) hist_sh[b] = 0u;
		__syncthreads();
	}
	unsigned long long outside = 0;   // wave-uniform
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		int b = 0, b1 = 0;
		bool in = hist_bin((double)buf[ax.off0 + D * i], ax.lo0, ax.hi0, ax.scale0, ax.bins0, b);
		if (ax.two)
		{
			in = hist_bin((double)buf[ax.off1 + D * i], ax.lo1, ax.hi1, ax.scale1, ax.bins1, b1) && in;
			b = b * ax.bins1 + b1;
		}
		if (in)
		{
			if (LDS) atomicAdd(&hist_sh[b], 1u);
			else atomicAdd(&counts[b], 1ull);
		}
		outside += (unsigned long long)__popcll(__ballot(!in));
	}
	if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&counts[B], outside);
	if (LDS)
	{
		__syncthreads();
		for (int b = threadIdx.x; b < B; b += kBlock)
		{
			const unsigned v = hist_sh[b];
			if (v) atomicAdd(&counts[b], (unsigned long long)v);
		}
	}
}
