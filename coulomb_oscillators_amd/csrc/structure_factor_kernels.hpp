// structure_factor_kernels.hpp -- sums over the particles on the wave-vector grid of nbco_structure_factor (include/nbco.h): rho_k =
// sum_j exp(i k . x_j) for that call (SkTerm, here) and the mode records of nbco_modes_record (MdTerm, modes_kernels.hpp); a section
// of k_reduce.hip, inside its anonymous namespace.  The rule (phases, powers, the complex product) is structure_factor.hpp.
//
// ONE KERNEL, kgrid_accumulate_kernel<Term, A, DIM3, T>, serves every such sum.  A TERM says what a particle adds to a k: the type
// of the sums of a k and their zero, the 16-byte LDS slots a particle needs beside its tables and how they are staged (which also
// decides whether the particle counts), the addition per (particle, ix), the complex parts of a record, the template steps of A.
//
// An ITEM is one (chunk, iy, iz): the column (iy, iz) of the grid and a run of up to A consecutive ix, ix = chunk * L + m, m < L <= A.
// A lane owns one item and keeps its A sums in registers (A is a template step: the loop over m is unrolled, the sums are
// never indexed at run time).  A workgroup of 256 lanes owns `lanes` <= 256 consecutive items and one range of particles; where
// lanes <= 128 it runs S = 256 / lanes copies of them, copy q taking the particles q, q + S, .. of a tile, and adds the copies in the
// order of q at the end, through LDS, one complex part of one sum at a time.  The range is taken in
// tiles: per tile the first lanes form the three phases of each particle once and the tables e_y^0..hy, e_z^0..hz and e_x^{cL} by
// repeated multiplication into LDS; then every lane runs over the tile's particles: two LDS reads (the same particle for the whole
// wave, neighbouring powers), one product for e_y^iy e_z^iz, one more with e_x^{cL} where the run is cut (a uniform branch), and A
// times: the term's addition, multiply by e_x.  Nothing in that loop is transcendental.  A particle that does not count gets tables
// and slots of zeros and adds (0, 0).  The record of a (range, k) goes to part[range][k] -- or straight to out + k * ostride where
// there is one range -- and sk_reduce_kernel adds the ranges in a fixed order.  No atomics; the ranges are a function of n and the
// grid alone.

constexpr int kSkBlock = 256;
constexpr int kSkLdsBytes = 48 * 1024;   // the tables of a tile: three workgroups per CU

// what the host works out for a call and the kernels read
struct SkShape
{
	int hx, hy, hz;        // (2-D: hz = 0)
	int L, nch;            // length of a run of ix, number of runs: nch * L >= hx + 1
	int ny, nz;            // 2 hy + 1, 2 hz + 1
	int items;             // nch * ny * nz
	int lanes, copies;     // items per workgroup, copies of them per workgroup: lanes * copies <= 256
	int tile;              // particles per tile
	int per;               // 16-byte LDS slots per particle: e_x, the term's, the tables
	long long range;       // particles per range (a multiple of 64)
	long long K;
	double wx, wy, wz;     // kstep / 2 pi
};

// The power tables of a tile of cnt particles from their base phases (ex[j], ty[j][1], tz[j][1]; the entries 0 are set): one lane per
// (particle, axis) chain fills ty[j][2..hy], tz[j][2..hz] and, where the ix run is cut, tc[j][1..nch-1] = e_x^{cL}.
template <bool DIM3>
__device__ __forceinline__ void sk_power_tables(const SkShape &s, int cnt, const SkC *ex, SkC *ty, SkC *tz, SkC *tc)
{
	const int tid = (int)threadIdx.x, sy = s.hy + 1, sz = s.hz + 1, nch = s.nch;
	const int chains = cnt * 3;
	for (int c = tid; c < chains; c += kSkBlock)
	{
		const int j = c / 3, a = c % 3;
		if (a == 0)
		{
			if (nch > 1)
			{
				const SkC z1 = ex[j];
				SkC z = z1;   // z = e_x^m
				for (int m = 1; m <= (nch - 1) * s.L; ++m)
				{
					if (m % s.L == 0) tc[(size_t)j * nch + m / s.L] = z;
					z = sk_mul(z, z1);
				}
			}
		}
		else if (a == 1)
		{
			if (s.hy > 1)
			{
				const SkC z1 = ty[(size_t)j * sy + 1];
				SkC z = z1;
				for (int m = 2; m <= s.hy; ++m) { z = sk_mul(z, z1); ty[(size_t)j * sy + m] = z; }
			}
		}
		else if (DIM3 && s.hz > 1)
		{
			const SkC z1 = tz[(size_t)j * sz + 1];
			SkC z = z1;
			for (int m = 2; m <= s.hz; ++m) { z = sk_mul(z, z1); tz[(size_t)j * sz + m] = z; }
		}
	}
}

// The term of nbco_structure_factor: a counted particle adds its w, a record is one complex number.  A term holds what a k-grid sum
// is apart from the tile scheme; kgrid_accumulate_kernel and the host (sk_shape, kgrid_run in k_reduce.hip) read everything from it.
struct SkTerm
{
	using Acc = SkC;                                                  // the sums of one k
	using Steps = std::integer_sequence<int, 1, 2, 3, 5, 9, 13, 17>;   // the template steps A of a run of ix (the last: 68 VGPRs of sums)
	static constexpr int kExtra = 0;                                  // 16-byte LDS slots of a particle beside its tables
	static constexpr int kParts = 1;                                  // complex numbers of a record
	static __device__ __forceinline__ void zero(Acc &a) { a.re = a.im = 0.0; }
	// Stage particle g of the n rows at p, whose phases are finite iff ok: fill its kExtra slots (zeros unless it counts) and say
	// whether it counts.
	template <typename T>
	static __device__ __forceinline__ bool stage(const T *, long long, size_t, bool ok, SkC *) { return ok; }
	// one (particle, ix): its term w and its slots
	static __device__ __forceinline__ void add(Acc &a, SkC w, const SkC *) { a.re += w.re; a.im += w.im; }
	// part c < kParts of the sums (c is a constant once the loop over it is unrolled)
	static __device__ __forceinline__ SkC &part(Acc &a, int) { return a; }
};

template <class Term, int A, bool DIM3, typename T>
__global__ __launch_bounds__(kSkBlock) void kgrid_accumulate_kernel(const T *__restrict__ p, long long n, SkShape s, double *__restrict__ out, long long ostride)
{
	extern __shared__ double sk_lds[];
	constexpr int D = DIM3 ? 3 : 2, X = Term::kExtra, P = Term::kParts;
	const int tid = (int)threadIdx.x;
	const int tile = s.tile, sy = s.hy + 1, sz = s.hz + 1, nch = s.nch;
	// LDS: ex[tile], xs[tile][X], ty[tile][hy + 1], tz[tile][hz + 1] (3-D), tc[tile][nch] (nch > 1)
	SkC *ex = reinterpret_cast<SkC *>(sk_lds);
	SkC *xs = ex + tile;
	SkC *ty = xs + (size_t)tile * X;
	SkC *tz = ty + (size_t)tile * sy;
	SkC *tc = DIM3 ? tz + (size_t)tile * sz : tz;

	const int copy = tid / s.lanes, lane = tid % s.lanes, S = s.copies;
	const int item = (int)blockIdx.x * s.lanes + lane;
	const bool live = copy < S && item < s.items;
	// item -> (chunk, iy, iz), iz fastest
	const int col = live ? item % (s.ny * s.nz) : 0, chunk = live ? item / (s.ny * s.nz) : 0;
	const int iy = col / s.nz - s.hy, iz = col % s.nz - s.hz;
	const int ay = iy < 0 ? -iy : iy, az = iz < 0 ? -iz : iz;
	const double cy = iy < 0 ? -1.0 : 1.0, cz = iz < 0 ? -1.0 : 1.0;

	typename Term::Acc acc[A];
#pragma unroll
	for (int m = 0; m < A; ++m) Term::zero(acc[m]);

	const long long lo = (long long)blockIdx.y * s.range;
	const long long hi = lo + s.range < n ? lo + s.range : n;
	for (long long base = lo; base < hi; base += tile)
	{
		const int cnt = hi - base < (long long)tile ? (int)(hi - base) : tile;   // particles of this tile
		__syncthreads();   // the previous tile has been read
		// the base phases and the term's slots: one lane per particle
		for (int j = tid; j < cnt; j += kSkBlock)
		{
			const size_t g = (size_t)(base + j);
			SkC zero, first;   // z^0 of a particle: (1, 0) if it counts
			zero.re = zero.im = 0.0;
			const double tx = (double)p[g * D] * s.wx, t1 = (double)p[g * D + 1] * s.wy;
			const double t2 = DIM3 ? (double)p[g * D + 2] * s.wz : 0.0;
			const bool ok = Term::stage(p, n, g, isfinite(tx) && isfinite(t1) && isfinite(t2), xs + (size_t)j * X);
			first.re = ok ? 1.0 : 0.0; first.im = 0.0;
			SkC e0 = zero, e1 = zero, e2 = zero;
			if (ok)
			{
				e0 = sk_phase(tx);
				e1 = sk_phase(t1);
				if (DIM3) e2 = sk_phase(t2);
			}
			ex[j] = e0;
			ty[(size_t)j * sy] = first;
			if (s.hy > 0) ty[(size_t)j * sy + 1] = e1;
			if (DIM3)
			{
				tz[(size_t)j * sz] = first;
				if (s.hz > 0) tz[(size_t)j * sz + 1] = e2;
			}
			if (nch > 1) tc[(size_t)j * nch] = first;
		}
		__syncthreads();
		sk_power_tables<DIM3>(s, cnt, ex, ty, tz, tc);
		__syncthreads();
		if (live)
		{
			for (int j = copy; j < cnt; j += S)
			{
				SkC w = ty[(size_t)j * sy + ay];
				w.im *= cy;
				if (DIM3)
				{
					SkC b = tz[(size_t)j * sz + az];
					b.im *= cz;
					w = sk_mul(w, b);
				}
				if (nch > 1) w = sk_mul(w, tc[(size_t)j * nch + chunk]);
				const SkC e = ex[j];
				SkC x[X > 0 ? X : 1];
#pragma unroll
				for (int c = 0; c < X; ++c) x[c] = xs[(size_t)j * X + c];
#pragma unroll
				for (int m = 0; m < A; ++m)
				{
					Term::add(acc[m], w, x);
					if (m + 1 < A) w = sk_mul(w, e);
				}
			}
		}
	}
	if (S > 1)
	{
		// the copies of an item, added in the order of the copies: every lane lends one complex sum at a time, copy 0 collects
		SkC *red = reinterpret_cast<SkC *>(sk_lds);
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
#pragma unroll
			for (int c = 0; c < P; ++c)
			{
				SkC &v = Term::part(acc[m], c);
				__syncthreads();   // the last tile, or the sum before this one, has been read
				red[tid] = v;
				__syncthreads();
				if (live && copy == 0)
					for (int q = 1; q < S; ++q)
					{
						const SkC u = red[q * s.lanes + lane];
						v.re += u.re;
						v.im += u.im;
					}
			}
		}
	}
	if (live && copy == 0)
	{
		double *o = out + (size_t)blockIdx.y * 2 * P * (size_t)s.K;   // (ostride != 2 P: one range, blockIdx.y == 0)
#pragma unroll
		for (int m = 0; m < A; ++m)
		{
			const int ix = chunk * s.L + m;
			if (m < s.L && ix <= s.hx)
			{
				const size_t k = ((size_t)ix * s.ny + (size_t)(iy + s.hy)) * s.nz + (size_t)(iz + s.hz);
				double *r = o + k * (size_t)ostride;   // (doubles: the caller's buffer is aligned as doubles are, no more is asked)
#pragma unroll
				for (int c = 0; c < P; ++c)
				{
					const SkC v = Term::part(acc[m], c);
					r[2 * c] = v.re;
					r[2 * c + 1] = v.im;
				}
			}
		}
	}
}

// rho[j] = the sum over the ranges of part[range][j], j over the 2 K doubles, in a fixed order: the ranges are cut into kSkSlices
// consecutive slices, a lane adds the ranges of one slice in index order, and the lane of slice 0 adds the slice sums in slice order.
// A workgroup serves 256 / kSkSlices neighbouring j (one 128-byte line per slice and range).  In general a k has a record of REC
// doubles and record k goes to rho + k * ostride: REC = ostride = 2 here, 8 doubles into a frame of a series for nbco_modes_record.
constexpr int kSkSlices = 16, kSkReduceJ = kSkBlock / kSkSlices;
template <int REC>
__global__ __launch_bounds__(kSkBlock) void sk_reduce_kernel(const double *__restrict__ part, long long ranges, long long K2, double *__restrict__ rho, long long ostride)
{
	__shared__ double slice_sum[kSkBlock];
	const int tid = (int)threadIdx.x, q = tid / kSkReduceJ;
	const long long j = (long long)blockIdx.x * kSkReduceJ + tid % kSkReduceJ;
	const long long per = (ranges + kSkSlices - 1) / kSkSlices;
	const long long r0 = q * per, r1 = r0 + per < ranges ? r0 + per : ranges;
	double sum = 0.0;
	if (j < K2)
	{
#pragma unroll 4
		for (long long r = r0; r < r1; ++r) sum += part[(size_t)r * (size_t)K2 + (size_t)j];
	}
	slice_sum[tid] = sum;
	__syncthreads();
	if (q == 0 && j < K2)
	{
		for (int t = 1; t < kSkSlices; ++t) sum += slice_sum[t * kSkReduceJ + tid];
		rho[(size_t)(j / REC) * (size_t)ostride + (size_t)(j % REC)] = sum;
	}
}
