// time_corr_kernels.hpp -- tracked trajectories and their time correlations (include/nbco.h: nbco_traj_record, nbco_time_corr); a
// section of k_reduce.hip, inside its anonymous namespace.  The rule of a term is time_corr.hpp.
//
// RECORDING is two passes on one stream: traj_fill_kernel writes NaN into frame `frame` of every row, traj_scatter_kernel copies the
// six floats of every state row whose particle number p is a multiple of `stride` with p / stride < rows to row p / stride.  p comes
// from the caller's ids, else from the context's order map (read where it lies, on the device), else it is the row itself.
//
// THE CORRELATION.  A workgroup of 256 lanes owns one range of rows and every lag.  It keeps the series of a row in LDS as two arrays
// of float4 -- {x, y, z, finite ? 1 : 0} and {vx, vy, vz, 0} per frame, 32 bytes, a row of 2048 frames 64 KiB -- and walks the origins
// t in increasing order: frame t is one address for the whole wave (a broadcast), frame t + tau consecutive addresses for consecutive
// lanes, both read with ds_read_b128 from arrays whose stride is the access width, so that no lane group meets a bank twice.  The
// fourth float of the positions carries the finiteness of the frame and the loop tests that one value.
// A lane keeps A lags, A a template step in {1, 2, 4, 8}: the loop over them is unrolled and the sums are never indexed at run time.
// Lag tau has frames - tau terms -- a triangle.  From A = 2 on, a lane's lags come in pairs, b from the bottom and lags - 1 - b from
// the top, b = m / 2 * W + lane: the two have 2 frames - lags + 1 terms together whatever b is, so the waves of a workgroup
// finish together.  A wave whose lanes are all past the end of a lag for an origin skips that lag's body (one compare, one branch).
// Where the W lanes of a row are at most 128, the workgroup runs S = 256 / W copies of them, copy q taking the rows q, q + S, .. of
// the range (S also bounded by the 64 KiB of LDS), and adds the copies in the order of q at the end, through LDS.
// The sums of a (range, lag) go to part[range][lag] -- or straight to the output where there is one range -- and tc_reduce_kernel
// adds the ranges in index order.  No atomics; ranges, W, S and A are functions of (rows, frames, lags) alone.

constexpr int kTcBlock = 256;
constexpr int kTcLdsBytes = 64 * 1024;
constexpr int kTcMaxRanges = 512;     // two workgroups per CU on 256 CUs

__global__ __launch_bounds__(256) void traj_fill_kernel(float *__restrict__ traj, long long rows, long long frames_cap, int frame)
{
	const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= rows) return;
	float2 *o = reinterpret_cast<float2 *>(traj + ((size_t)r * (size_t)frames_cap + (size_t)frame) * 6);   // (24-byte records: 8-byte aligned)
	const float q = __int_as_float(0x7fc00000);
	o[0] = make_float2(q, q);
	o[1] = make_float2(q, q);
	o[2] = make_float2(q, q);
}

__global__ __launch_bounds__(256) void traj_scatter_kernel(const float *__restrict__ buf, long long n, const int *__restrict__ ids, float *__restrict__ traj,
                                                           long long rows, long long frames_cap, int frame, int stride)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const long long p = ids ? (long long)ids[i] : i;
	if (p < 0 || p % stride != 0) return;
	const long long r = p / stride;
	if (r >= rows) return;
	const float *x = buf + 3 * (size_t)i, *v = buf + 3 * (size_t)n + 3 * (size_t)i;
	float2 *o = reinterpret_cast<float2 *>(traj + ((size_t)r * (size_t)frames_cap + (size_t)frame) * 6);
	o[0] = make_float2(x[0], x[1]);
	o[1] = make_float2(x[2], v[0]);
	o[2] = make_float2(v[1], v[2]);
}

// what the host works out for a call and the kernels read
struct TcShape
{
	int frames, lags, cap;
	int W, S;              // lanes of a row, rows in flight per workgroup: W * S <= 256
	int half;              // A >= 2: the lags taken from the bottom, ceil(lags / 2); A = 1: lags
	long long range;       // rows per range (a multiple of S)
	long long ranges;
};

// the lag of slot m of a lane (-1: none)
template <int A>
__device__ __forceinline__ int tc_lag(const TcShape &s, int lane, int m)
{
	if (A == 1) return lane < s.lags ? lane : -1;
	const int b = (m >> 1) * s.W + lane;
	if ((m & 1) == 0) return b < s.half ? b : -1;
	return b < s.lags - s.half ? s.lags - 1 - b : -1;
}

// The slots of a lane (mode_corr_kernel uses them too): tau[m] its lag and end[m] the origins of that lag, frames - tau (both 0: none,
// as for a lane that is not live).  Returns the origins any lane of the wave has a lag for, so that the loop over them is uniform.
template <int A>
__device__ __forceinline__ int tc_lag_slots(const TcShape &s, bool live, int lane, int (&tau)[A], int (&end)[A])
{
	int tend = 0;
#pragma unroll
	for (int m = 0; m < A; ++m)
	{
		const int l = live ? tc_lag<A>(s, lane, m) : -1;
		tau[m] = l < 0 ? 0 : l;
		end[m] = l < 0 ? 0 : s.frames - l;
		tend = end[m] > tend ? end[m] : tend;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(tend, d);
		tend = o > tend ? o : tend;
	}
	return __builtin_amdgcn_readfirstlane(tend);
}

template <int A>
__global__ __launch_bounds__(kTcBlock) void tc_accumulate_kernel(const float *__restrict__ traj, long long rows, TcShape s, nbco_corr_lag *__restrict__ out)
{
	extern __shared__ float4 tc_lds[];
	const int tid = (int)threadIdx.x;
	const int copy = tid / s.W, lane = tid % s.W;
	const int frames = s.frames;
	const bool live = copy < s.S;
	float4 *px = tc_lds + (size_t)(live ? copy : 0) * 2 * (size_t)frames;   // this copy's row: positions, then velocities
	float4 *pv = px + frames;

	int tau[A], end[A];
	TcSum acc[A];
	unsigned long long cnt[A];
	const int tend = tc_lag_slots<A>(s, live, lane, tau, end);
#pragma unroll
	for (int m = 0; m < A; ++m)
	{
		tc_zero(acc[m]);
		cnt[m] = 0;
	}

	const long long lo = (long long)blockIdx.x * s.range;
	const long long hi = lo + s.range < rows ? lo + s.range : rows;
	for (long long base = lo; base < hi; base += s.S)
	{
		const long long row = base + copy;
		const bool have = live && row < hi;
		__syncthreads();   // the previous rows have been read
		if (have)
		{
			const float2 *src = reinterpret_cast<const float2 *>(traj + (size_t)row * (size_t)s.cap * 6);
			for (int f = lane; f < frames; f += s.W)
			{
				const float2 a = src[3 * (size_t)f], b = src[3 * (size_t)f + 1], c = src[3 * (size_t)f + 2];
				const float six[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
				px[f] = make_float4(a.x, a.y, b.x, tc_finite(six) ? 1.0f : 0.0f);
				pv[f] = make_float4(b.y, c.x, c.y, 0.0f);
			}
		}
		__syncthreads();
		if (have)
		{
			unsigned int k[A];   // the terms of this row (at most 2048 each)
#pragma unroll
			for (int m = 0; m < A; ++m) k[m] = 0;
			for (int t = 0; t < tend; ++t)
			{
				// every read of this origin is issued before the first is used: one LDS round trip per origin, not one per lag
				// (a lag past its end reads frame t again and is masked below).  Measured: skipping the reads of the lags that no
				// lane of the wave has an origin t for, behind scalar tests, breaks that batch up and is 16 % slower.
				const float4 x0 = px[t], v0 = pv[t];
				float4 x1[A], v1[A];
#pragma unroll
				for (int m = 0; m < A; ++m)
				{
					const int f = t < end[m] ? t + tau[m] : t;
					x1[m] = px[f];
					v1[m] = pv[f];
				}
				// (the values exist here, in front of the branches: the compiler would otherwise move a lag's reads behind its test)
#pragma unroll
				for (int m = 0; m < A; ++m)
					asm volatile("" : "+v"(x1[m].x), "+v"(x1[m].y), "+v"(x1[m].z), "+v"(x1[m].w), "+v"(v1[m].x), "+v"(v1[m].y), "+v"(v1[m].z), "+v"(v1[m].w));
				const double x0x = (double)x0.x, x0y = (double)x0.y, x0z = (double)x0.z;
				const double v0x = (double)v0.x, v0y = (double)v0.y, v0z = (double)v0.z;
#pragma unroll
				for (int m = 0; m < A; ++m)
				{
					if (t < end[m] && x0.w * x1[m].w != 0.0f)
					{
						tc_term(acc[m], x0x, x0y, x0z, v0x, v0y, v0z, (double)x1[m].x, (double)x1[m].y, (double)x1[m].z, (double)v1[m].x, (double)v1[m].y,
						        (double)v1[m].z);
						k[m] += 1u;
					}
				}
			}
#pragma unroll
			for (int m = 0; m < A; ++m) cnt[m] += k[m];
		}
	}
	if (s.S > 1)
	{
		// the copies of a lag, added in the order of the copies: every lane lends one number at a time, copy 0 collects
		double *red = reinterpret_cast<double *>(tc_lds);
		unsigned long long *redc = reinterpret_cast<unsigned long long *>(tc_lds);
		const bool collect = live && copy == 0;
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			double v[7] = {acc[m].dx2[0], acc[m].dx2[1], acc[m].dx2[2], acc[m].r4, acc[m].vv[0], acc[m].vv[1], acc[m].vv[2]};
#pragma unroll
			for (int j = 0; j < 7; ++j)
			{
				__syncthreads();   // the last row, or the number before this one, has been read
				red[tid] = v[j];
				__syncthreads();
				if (collect)
					for (int q = 1; q < s.S; ++q) v[j] += red[q * s.W + lane];
			}
			__syncthreads();
			redc[tid] = cnt[m];
			__syncthreads();
			if (collect)
				for (int q = 1; q < s.S; ++q) cnt[m] += redc[q * s.W + lane];
			acc[m].dx2[0] = v[0]; acc[m].dx2[1] = v[1]; acc[m].dx2[2] = v[2];
			acc[m].r4 = v[3];
			acc[m].vv[0] = v[4]; acc[m].vv[1] = v[5]; acc[m].vv[2] = v[6];
		}
	}
	if (live && copy == 0)
	{
		nbco_corr_lag *o = out + (size_t)blockIdx.x * (size_t)s.lags;
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			if (end[m] > 0)
			{
				nbco_corr_lag r;
				r.dx2[0] = acc[m].dx2[0]; r.dx2[1] = acc[m].dx2[1]; r.dx2[2] = acc[m].dx2[2];
				r.r4 = acc[m].r4;
				r.vv[0] = acc[m].vv[0]; r.vv[1] = acc[m].vv[1]; r.vv[2] = acc[m].vv[2];
				r.pairs = cnt[m];
				o[tau[m]] = r;
			}
		}
	}
}

// out[lag] = the sum over the ranges of part[range][lag], in index order; one lane per number of a record (seven doubles and the count)
__global__ __launch_bounds__(kTcBlock) void tc_reduce_kernel(const nbco_corr_lag *__restrict__ part, long long ranges, int lags, nbco_corr_lag *__restrict__ out)
{
	const int j = (int)blockIdx.x * kTcBlock + (int)threadIdx.x;
	if (j >= 8 * lags) return;
	if ((j & 7) == 7)
	{
		const unsigned long long *p = reinterpret_cast<const unsigned long long *>(part);
		unsigned long long sum = 0;
		for (long long r = 0; r < ranges; ++r) sum += p[(size_t)r * 8 * (size_t)lags + (size_t)j];
		reinterpret_cast<unsigned long long *>(out)[j] = sum;
	}
	else
	{
		const double *p = reinterpret_cast<const double *>(part);
		double sum = 0.0;
#pragma unroll 4
		for (long long r = 0; r < ranges; ++r) sum += p[(size_t)r * 8 * (size_t)lags + (size_t)j];
		reinterpret_cast<double *>(out)[j] = sum;
	}
}
