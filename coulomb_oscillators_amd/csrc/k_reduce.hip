// k_reduce.hip -- reductions: component-wise min/max, mean relative error, power sums, energy.
// Reference behaviour: reductions.cuh:37-42 (rel_diff1), :67-80 (minmaxReduce2), :82-104
// (relerrReduce2; the evident intent is implemented, see SURVEY note N1), :497-653 (powReduce).
// Pattern: grid-stride loads -> wave64 shuffle reduction -> LDS across the 4 waves of a block ->
// one partial per block -> last stage in a single block (deterministic, no float atomics).
#include "nbco_internal.hpp"
#include "host_util.hpp"
#include "bond_order.hpp"
#include "structure_factor.hpp"
#include "time_corr.hpp"
#include "modes.hpp"
#include <algorithm>
#include <cfloat>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;

__device__ inline float wave_min(float v) { for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return v; }
__device__ inline float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }
__device__ inline float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline double wave_sum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

template <int STRIDE>   // 3: packed xyz triplets, 4: float4
__global__ __launch_bounds__(kBlock) void minmax_stage1(const float *__restrict__ p, long long n, float *__restrict__ part)
{
	float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
#pragma unroll
		for (int c = 0; c < 3; ++c)
		{
			float v = p[STRIDE * i + c];
			mn[c] = fminf(mn[c], v);
			mx[c] = fmaxf(mx[c], v);
		}
	__shared__ float sh[kBlock / 64][6];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int c = 0; c < 3; ++c) { mn[c] = wave_min(mn[c]); mx[c] = wave_max(mx[c]); }
	if (lane == 0)
#pragma unroll
		for (int c = 0; c < 3; ++c) { sh[w][c] = mn[c]; sh[w][3 + c] = mx[c]; }
	__syncthreads();
	if (threadIdx.x < 6)
	{
		float v = sh[0][threadIdx.x];
		for (int k = 1; k < kBlock / 64; ++k) v = threadIdx.x < 3 ? fminf(v, sh[k][threadIdx.x]) : fmaxf(v, sh[k][threadIdx.x]);
		part[blockIdx.x * 6 + threadIdx.x] = v;
	}
}

__global__ __launch_bounds__(64) void minmax_stage2(const float *__restrict__ part, int nblocks, float *__restrict__ out6)
{
	const int lane = threadIdx.x;
	for (int c = 0; c < 6; ++c)
	{
		float v = c < 3 ? FLT_MAX : -FLT_MAX;
		for (int b = lane; b < nblocks; b += 64) v = c < 3 ? fminf(v, part[b * 6 + c]) : fmaxf(v, part[b * 6 + c]);
		v = c < 3 ? wave_min(v) : wave_max(v);
		if (lane == 0) out6[c] = v;
	}
}

// per-block partial sums of up to 3 doubles
__device__ inline void block_sum3(double v[3], double *__restrict__ part)
{
	__shared__ double sh[kBlock / 64][3];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int c = 0; c < 3; ++c) v[c] = wave_sum(v[c]);
	if (lane == 0)
#pragma unroll
		for (int c = 0; c < 3; ++c) sh[w][c] = v[c];
	__syncthreads();
	if (threadIdx.x < 3)
	{
		double s = 0;
		for (int k = 0; k < kBlock / 64; ++k) s += sh[k][threadIdx.x];
		part[blockIdx.x * 3 + threadIdx.x] = s;
	}
}

__global__ __launch_bounds__(64) void sum3_stage2(const double *__restrict__ part, int nblocks, double *__restrict__ out3, double scale)
{
	const int lane = threadIdx.x;
	for (int c = 0; c < 3; ++c)
	{
		double v = 0;
		for (int b = lane; b < nblocks; b += 64) v += part[b * 3 + c];
		v = wave_sum(v);
		if (lane == 0) out3[c] = v * scale;
	}
}

// rel_diff1 (reductions.cuh:37-42): sqrt(max(|x-ref|^2 / (|ref|^2 + 1e-18), 0)), fp32 per particle,
// accumulated in fp64
__global__ __launch_bounds__(kBlock) void relerr_stage1(const float *__restrict__ x, const float *__restrict__ ref, long long n,
                                                        double *__restrict__ part)
{
	double v[3] = {0, 0, 0};
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		float rx = ref[3 * i], ry = ref[3 * i + 1], rz = ref[3 * i + 2];
		float dx = x[3 * i] - rx, dy = x[3 * i + 1] - ry, dz = x[3 * i + 2] - rz;
		float dist2 = dx * dx + dy * dy + dz * dz, ref2 = rx * rx + ry * ry + rz * rz + 1.e-18f;
		v[0] += (double)sqrtf(fmaxf(dist2 / ref2, 0.f));
	}
	block_sum3(v, part);
}

__global__ __launch_bounds__(kBlock) void powsum_stage1(const float *__restrict__ x, int expo, long long n, double *__restrict__ part)
{
	double v[3] = {0, 0, 0};
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
#pragma unroll
		for (int c = 0; c < 3; ++c)
		{
			double b = (double)x[3 * i + c], r = 1.0;
			for (int e = 0; e < expo; ++e) r *= b;
			v[c] += r;
		}
	block_sum3(v, part);
}

// kinetic and elastic energy: 1/2 sum v^2, 1/2 sum k.x^2
__global__ __launch_bounds__(kBlock) void energy1_stage1(const float *__restrict__ buf, long long n, const float *__restrict__ param,
                                                         double *__restrict__ part)
{
	double v[3] = {0, 0, 0};
	const double kx = param[3], ky = param[4], kz = param[5];
	const float *vel = buf + 3 * n;
	for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
	{
		double x = buf[3 * i], y = buf[3 * i + 1], z = buf[3 * i + 2];
		double ux = vel[3 * i], uy = vel[3 * i + 1], uz = vel[3 * i + 2];
		v[0] += 0.5 * (ux * ux + uy * uy + uz * uz);
		v[1] += 0.5 * (kx * x * x + ky * y * y + kz * z * z);
	}
	block_sum3(v, part);
}

// Coulomb energy sum_{i<j} (r^2+eps2)^(-1/2): fp32 pair terms from an LDS tile, fp64 accumulation
// per lane; every ordered pair is visited and the total halved (self terms removed analytically).
constexpr int kETile = 256;
__global__ __launch_bounds__(kBlock) void coulomb_energy_stage1(const float4 *__restrict__ pos, long long n, float eps2,
                                                                double *__restrict__ part)
{
	__shared__ float4 tile[kETile];
	double v[3] = {0, 0, 0};
	const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
	const float4 pi = pos[i < n ? i : n - 1];
	double acc = 0;
	for (long long t = 0; t < n; t += kETile)
	{
		long long j = t + threadIdx.x;
		__syncthreads();
		tile[threadIdx.x] = pos[j < n ? j : n - 1];
		__syncthreads();
		int cnt = (n - t) < kETile ? (int)(n - t) : kETile;
		float s = 0.f;
		for (int k = 0; k < cnt; ++k)
		{
			float dx = pi.x - tile[k].x, dy = pi.y - tile[k].y, dz = pi.z - tile[k].z;
			float r2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps2)));
			s += (t + k == i) ? 0.f : __builtin_amdgcn_rsqf(r2);
		}
		acc += (double)s;
	}
	if (i < n) v[2] = 0.5 * acc;
	block_sum3(v, part);
}

static int grid_for(long long n)
{
	long long b = (n + kBlock - 1) / kBlock;
	if (b > kMaxBlocks) b = kMaxBlocks;
	if (b < 1) b = 1;
	return (int)b;
}

#include "beam_diag_kernels.hpp"   // beam diagnostics: the two moment passes and the histogram kernel
#include "aperture_kernels.hpp"    // aperture: the rule, the classification pass, the scan of the workgroup counts, the scatter
#include "slice_diag_kernels.hpp" // slice diagnostics: the keys, the slice and chunk tables, the two moment passes per chunk and per slice
#define NBCO_PAIR_STAT_EXACT
#include "pair_stat_kernels.hpp"   // pair statistics: the pair rule, the all-pairs kernel, the count of the pairs outside
#undef NBCO_PAIR_STAT_EXACT
#define NBCO_BOND_EXACT
#include "bond_order_kernels.hpp"   // bond-orientational order: the all-pairs kernel, the wave records of the summary and their sum
#undef NBCO_BOND_EXACT
#include "structure_factor_kernels.hpp"   // the static structure factor: the tile kernel and the sum over the particle ranges
#include "time_corr_kernels.hpp"          // tracked trajectories: the recording passes, the correlation kernel and the sum over the row ranges
#include "modes_kernels.hpp"              // collective modes: the tile kernel with velocities, the sum over the particle ranges, the lag kernel

} // namespace

int launch_minmax(nbco_ctx *c, const float *p3, long long n, float *out6_dev)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "minmax: n must be positive");
	int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(float) * 6 * kMaxBlocks));
	hipLaunchKernelGGL(minmax_stage1<3>, dim3(g), dim3(kBlock), 0, c->stream, p3, n, c->part.as<float>());
	hipLaunchKernelGGL(minmax_stage2, dim3(1), dim3(64), 0, c->stream, c->part.as<float>(), g, out6_dev);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

int launch_minmax4(nbco_ctx *c, const float4 *p4, long long n, float *out6_dev)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "minmax: n must be positive");
	int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(float) * 6 * kMaxBlocks));
	hipLaunchKernelGGL(minmax_stage1<4>, dim3(g), dim3(kBlock), 0, c->stream, (const float *)p4, n, c->part.as<float>());
	hipLaunchKernelGGL(minmax_stage2, dim3(1), dim3(64), 0, c->stream, c->part.as<float>(), g, out6_dev);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

static int finish_sum3(nbco_ctx *c, int g, double scale, double *host3)
{
	double *out = c->small.as<double>();
	hipLaunchKernelGGL(sum3_stage2, dim3(1), dim3(64), 0, c->stream, c->part.as<double>(), g, out, scale);
	NBCO_HIP(hipGetLastError());
	NBCO_HIP(hipMemcpyAsync(host3, out, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	return NBCO_OK;
}

int launch_mean_relerr(nbco_ctx *c, const float *x, const float *ref, long long n, float *out_host)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "mean_relerr: n must be positive");
	int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(double) * 3 * kMaxBlocks));
	hipLaunchKernelGGL(relerr_stage1, dim3(g), dim3(kBlock), 0, c->stream, x, ref, n, c->part.as<double>());
	double h[3];
	NBCO_TRY(finish_sum3(c, g, 1.0 / (double)n, h));
	*out_host = (float)h[0];
	return NBCO_OK;
}

int launch_pow_sum(nbco_ctx *c, const float *x, int expo, long long n, double *out3_host)
{
	if (n <= 0 || expo < 0) return c->fail(NBCO_ERR_ARG, "pow_sum: bad arguments");
	int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(double) * 3 * kMaxBlocks));
	hipLaunchKernelGGL(powsum_stage1, dim3(g), dim3(kBlock), 0, c->stream, x, expo, n, c->part.as<double>());
	return finish_sum3(c, g, 1.0, out3_host);
}

// kinetic and elastic part only (nbco_energy_fmm adds the Coulomb part from the FMM lists)
int launch_energy_kin_ela(nbco_ctx *c, const float *buf, long long n, const float *param, double *out2_host)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "energy: n must be positive");
	double h1[3];
	int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(double) * 3 * kMaxBlocks));
	hipLaunchKernelGGL(energy1_stage1, dim3(g), dim3(kBlock), 0, c->stream, buf, n, param, c->part.as<double>());
	NBCO_TRY(finish_sum3(c, g, 1.0, h1));
	out2_host[0] = h1[0]; out2_host[1] = h1[1];
	return NBCO_OK;
}

int launch_energy(nbco_ctx *c, const float *buf, long long n, const float *param, double *out3_host)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "energy: n must be positive");
	double h1[3], h2[3];
	{
		int g = grid_for(n);
		NBCO_TRY(c->reserve(c->part, sizeof(double) * 3 * kMaxBlocks));
		hipLaunchKernelGGL(energy1_stage1, dim3(g), dim3(kBlock), 0, c->stream, buf, n, param, c->part.as<double>());
		NBCO_TRY(finish_sum3(c, g, 1.0, h1));
	}
	{
		NBCO_TRY(c->reserve(c->pos4, sizeof(float4) * (size_t)n));
		c->last_eval.valid = false;   // the tree-ordered positions of the last kd evaluation are overwritten
		NBCO_TRY(launch_pack4(c, c->pos4.as<float4>(), buf, n));
		int g = ceil_div(n, kBlock);
		NBCO_TRY(c->reserve(c->part, sizeof(double) * 3 * (size_t)g));
		hipLaunchKernelGGL(coulomb_energy_stage1, dim3(g), dim3(kBlock), 0, c->stream, c->pos4.as<float4>(), n, c->o.eps2, c->part.as<double>());
		NBCO_TRY(finish_sum3(c, g, 1.0, h2));
	}
	float p0;
	NBCO_HIP(hipMemcpy(&p0, param, sizeof(float), hipMemcpyDeviceToHost));
	out3_host[0] = h1[0];
	out3_host[1] = h1[1];
	out3_host[2] = h2[2] * (double)p0;
	return NBCO_OK;
}

// ---- beam diagnostics (beam_diag_kernels.hpp) --------------------------------------------------
// results in c->small, in doubles from kBeamOut on: mean[6], min[6], max[6], then the central sums
constexpr int kBeamOut = 128;

template <class T, int D> static int beam_moments(nbco_ctx *c, const T *buf, long long n, nbco_moments *out_host)
{
	constexpr int Q = 2 * D, K = beam_central_count(D);
	const int g = grid_for(n);
	NBCO_TRY(c->reserve(c->part, sizeof(double) * beam_central_count(3) * kMaxBlocks));   // (3 Q <= K)
	double *part = c->part.as<double>(), *out = c->small.as<double>() + kBeamOut;
	// two passes, no host round trip in between: the second reads the means the first left on the device
	hipLaunchKernelGGL((beam_sums_stage1<T, D>), dim3(g), dim3(kBlock), 0, c->stream, buf, n, part);
	hipLaunchKernelGGL(beam_sums_stage2<Q>, dim3(1), dim3(kBlock), 0, c->stream, part, g, n, out);
	hipLaunchKernelGGL((beam_central_stage1<T, D>), dim3(g), dim3(kBlock), 0, c->stream, buf, n, out, part);
	hipLaunchKernelGGL(beam_central_stage2, dim3(1), dim3(kBlock), 0, c->stream, part, g, K, out + 18);
	NBCO_HIP(hipGetLastError());
	double h[18 + K];
	NBCO_HIP(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	nbco_moments m;
	memset(&m, 0, sizeof m);
	m.n = n;
	m.dim = D;
	for (int a = 0; a < Q; ++a) { m.mean[a] = h[a]; m.min[a] = h[6 + a]; m.max[a] = h[12 + a]; }
	const double *s = h + 18;
	for (int a = 0; a < Q; ++a)
		for (int b = a; b < Q; ++b) m.cov[a][b] = m.cov[b][a] = *s++ / (double)n;
	for (int p = 0; p < D; ++p)
		for (int j = 0; j < 5; ++j) m.m4[p][j] = *s++ / (double)n;
	nbco_moments_derive(&m);
	*out_host = m;
	return NBCO_OK;
}

int launch_beam_moments(nbco_ctx *c, const void *buf, int dim, long long n, nbco_moments *out_host)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "beam_moments: n must be positive");
	return dim == 3 ? beam_moments<float, 3>(c, (const float *)buf, n, out_host) : beam_moments<double, 2>(c, (const double *)buf, n, out_host);
}

template <class T, int D> static void hist_run(nbco_ctx *c, const T *buf, long long n, const HistAxes &ax, int B, unsigned long long *counts)
{
	if (B <= kHistLdsBins)
	{
		long long g = (n + kHistPerBlock - 1) / kHistPerBlock;
		if (g > kMaxBlocks) g = kMaxBlocks;
		hipLaunchKernelGGL((hist_kernel<T, D, true>), dim3((int)g), dim3(kBlock), sizeof(unsigned) * (size_t)B, c->stream, buf, n, ax, counts);
	}
	else hipLaunchKernelGGL((hist_kernel<T, D, false>), dim3(grid_for(n)), dim3(kBlock), 0, c->stream, buf, n, ax, counts);
}

// element offset of a coordinate in buf = [pos n | vel n | ..]
static long long hist_coord_offset(int coord, int dim, long long n) { return coord < 3 ? (long long)coord : (long long)dim * n + (coord - 3); }

// what nbco_hist and nbco_slice_moments refuse in an axis
static int hist_axis_check(nbco_ctx *c, const char *who, int dim, const nbco_hist_axis &x)
{
	const std::string w = std::string(who) + ": ";
	const bool have = dim == 3 ? x.coord >= NBCO_Q_X && x.coord <= NBCO_Q_VZ
	                           : x.coord == NBCO_Q_X || x.coord == NBCO_Q_Y || x.coord == NBCO_Q_VX || x.coord == NBCO_Q_VY;
	if (!have) return c->fail(NBCO_ERR_ARG, w + "the state has no such coordinate");
	if (x.bins < 1 || x.bins > 65536) return c->fail(NBCO_ERR_ARG, w + "bins must be 1..65536");
	if (!std::isfinite(x.lo) || !std::isfinite(x.hi) || !std::isfinite(x.hi - x.lo)) return c->fail(NBCO_ERR_ARG, w + "lo and hi must be finite");
	if (!(x.lo < x.hi)) return c->fail(NBCO_ERR_ARG, w + "lo must be below hi");
	return NBCO_OK;
}

int launch_hist(nbco_ctx *c, const void *buf, int dim, long long n, const nbco_hist_axis *axes, int naxes, unsigned long long *counts)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "hist: n must be positive");
	if (naxes != 1 && naxes != 2) return c->fail(NBCO_ERR_ARG, "hist: one or two axes");
	long long B = 1;
	for (int a = 0; a < naxes; ++a)
	{
		NBCO_TRY(hist_axis_check(c, "hist", dim, axes[a]));
		B *= axes[a].bins;
	}
	if (B > (1LL << 24)) return c->fail(NBCO_ERR_ARG, "hist: more than 2^24 bins");
	auto off = [&](int coord) { return hist_coord_offset(coord, dim, n); };
	HistAxes ax{};
	ax.off0 = off(axes[0].coord);
	ax.bins0 = axes[0].bins; ax.lo0 = axes[0].lo; ax.hi0 = axes[0].hi; ax.scale0 = (double)axes[0].bins / (axes[0].hi - axes[0].lo);
	ax.bins1 = 1;
	if (naxes == 2)
	{
		ax.two = 1;
		ax.off1 = off(axes[1].coord);
		ax.bins1 = axes[1].bins; ax.lo1 = axes[1].lo; ax.hi1 = axes[1].hi; ax.scale1 = (double)axes[1].bins / (axes[1].hi - axes[1].lo);
	}
	NBCO_HIP(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)(B + 1), c->stream));
	if (dim == 3) hist_run<float, 3>(c, (const float *)buf, n, ax, (int)B, counts);
	else hist_run<double, 2>(c, (const double *)buf, n, ax, (int)B, counts);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// ---- slice diagnostics (slice_diag_kernels.hpp) --------------------------------------------------
// Scratch of the call's own (c->sl_*): a kd evaluation's buffers, the reduction partials and c->small are not touched.
template <class T, int D>
static int slice_moments(nbco_ctx *c, const T *buf, long long n, const nbco_hist_axis &x, nbco_moments *out_host, long long *n_outside_host)
{
	constexpr int Q = 2 * D, K = beam_central_count(D), R = 3 * Q + K;   // doubles of a slice's record on the device: mean, min, max, central sums
	static_assert(4 * Q <= K, "a slab of the first pass fits a slab of the second");
	const int bins = x.bins, ni = (int)n;
	const SliceAxis ax{hist_coord_offset(x.coord, D, n), bins, x.lo, x.hi, (double)bins / (x.hi - x.lo)};
	// at most n / kSliceChunk full chunks and one partial chunk per slice that holds anybody
	const long long grid = n / kSliceChunk + std::min<long long>(bins, n);
	// the table: start[bins + 2] and first[bins + 1] as ints, then the records
	const size_t ints = ((size_t)2 * bins + 3 + 1) & ~(size_t)1, tab_bytes = sizeof(int) * ints + sizeof(double) * R * (size_t)bins;
	NBCO_TRY(c->reserve(c->sl_keys, sizeof(unsigned) * 3 * (size_t)n));
	NBCO_TRY(c->reserve(c->sl_tab, tab_bytes));
	NBCO_TRY(c->reserve(c->sl_part, sizeof(double) * K * (size_t)grid));   // (4 Q <= K)
	unsigned *key = c->sl_keys.as<unsigned>(), *key_sorted = key + n;
	int *perm = reinterpret_cast<int *>(key + 2 * n), *start = c->sl_tab.as<int>(), *first = start + bins + 2;
	double *rec = reinterpret_cast<double *>(start + ints), *part = c->sl_part.as<double>();
	unsigned key_bits = 0;
	while ((bins >> key_bits) != 0) ++key_bits;   // the keys are 0 .. bins
	hipLaunchKernelGGL((slice_key_kernel<T, D>), dim3(grid_for(n)), dim3(kBlock), 0, c->stream, buf, n, ax, key);
	NBCO_TRY(sort_pairs(c, c->sl_tmp, key, key_sorted, rocprim::counting_iterator<int>(0), perm, n, 0, key_bits));
	hipLaunchKernelGGL(slice_start_kernel, dim3(ceil_div(bins + 2, kBlock)), dim3(kBlock), 0, c->stream, key_sorted, ni, bins, start);
	NBCO_TRY(exclusive_scan(c, c->sl_tmp, rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), SliceChunksOf{start, bins}), first, 0,
	                        (size_t)bins + 1));
	// two passes, no host round trip in between: the chunk table and the slices' means stay on the device
	const dim3 chunks((unsigned)grid), slices((unsigned)ceil_div(bins, kBlock / 64)), block(kBlock);
	hipLaunchKernelGGL((slice_sums_stage1<T, D>), chunks, block, 0, c->stream, buf, n, perm, first, start, bins, part);
	hipLaunchKernelGGL(slice_sums_stage2<Q>, slices, block, 0, c->stream, part, first, start, bins, R, rec);
	hipLaunchKernelGGL((slice_central_stage1<T, D>), chunks, block, 0, c->stream, buf, n, perm, first, start, bins, R, rec, part);
	hipLaunchKernelGGL((slice_central_stage2<Q, K>), slices, block, 0, c->stream, part, first, bins, R, rec);
	NBCO_HIP(hipGetLastError());
	std::vector<char> host(tab_bytes);
	NBCO_HIP(hipMemcpyAsync(host.data(), start, tab_bytes, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	const int *h_start = reinterpret_cast<const int *>(host.data());
	const double *h_rec = reinterpret_cast<const double *>(h_start + ints);
	for (int s = 0; s < bins; ++s)
	{
		nbco_moments m;
		memset(&m, 0, sizeof m);
		m.n = h_start[s + 1] - h_start[s];
		m.dim = D;
		if (m.n)
		{
			const double *h = h_rec + (size_t)R * s, *t = h + 3 * Q;
			for (int a = 0; a < Q; ++a) { m.mean[a] = h[a]; m.min[a] = h[Q + a]; m.max[a] = h[2 * Q + a]; }
			for (int a = 0; a < Q; ++a)
				for (int b = a; b < Q; ++b) m.cov[a][b] = m.cov[b][a] = *t++ / (double)m.n;
			for (int p = 0; p < D; ++p)
				for (int j = 0; j < 5; ++j) m.m4[p][j] = *t++ / (double)m.n;
		}
		nbco_moments_derive(&m);
		out_host[s] = m;
	}
	*n_outside_host = n - h_start[bins];
	return NBCO_OK;
}

int launch_slice_moments(nbco_ctx *c, const void *buf, int dim, long long n, const nbco_hist_axis *axis_host, nbco_moments *out_host, long long *n_outside_host)
{
	if (n <= 0) return c->fail(NBCO_ERR_ARG, "slice_moments: n must be positive");
	NBCO_TRY(hist_axis_check(c, "slice_moments", dim, *axis_host));
	if (n >= (1LL << 31)) return c->fail(NBCO_ERR_UNSUPPORTED, "slice_moments: n must be below 2^31");
	return dim == 3 ? slice_moments<float, 3>(c, (const float *)buf, n, *axis_host, out_host, n_outside_host)
	                : slice_moments<double, 2>(c, (const double *)buf, n, *axis_host, out_host, n_outside_host);
}

// ---- pair statistics, exact forms (pair_stat_kernels.hpp) ---------------------------------------
template <class T, int D, bool LDS> static void pair_hist_run(nbco_ctx *c, const T *p, long long n, const PairBins &pb, unsigned long long *counts, double *nn2)
{
	const long long nt = (n + kBlock - 1) / kBlock, chunks = (nt + kPairSrcTiles - 1) / kPairSrcTiles;
	const dim3 grid((unsigned)nt, (unsigned)std::min<long long>(chunks, kPairGridY));
	const size_t lds = LDS && counts ? sizeof(unsigned) * (size_t)pb.bins : 0;
	// (with_outputs looks only at which of the two pointers are given: a NULL output is compiled out)
	with_outputs((const double *)counts, nn2, [&](auto wc, auto wn) {
		hipLaunchKernelGGL((pair_hist_kernel<T, D, LDS, decltype(wc)::value, decltype(wn)::value>), grid, dim3(kBlock), lds, c->stream, p, n, pb, counts,
		                   reinterpret_cast<unsigned long long *>(nn2));
	});
}

int launch_pair_hist(nbco_ctx *c, const void *p, int dim, long long n, const PairBins &pb, unsigned long long *counts, double *nn2)
{
	if (counts) NBCO_HIP(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * ((size_t)pb.bins + 1), c->stream));
	if (nn2) hipLaunchKernelGGL(pair_fill_kernel, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, reinterpret_cast<unsigned long long *>(nn2), n, kPairInfBits);
	const bool lds = pb.bins <= kPairLdsBins;
	if (dim == 3)
	{
		if (lds) pair_hist_run<float, 3, true>(c, (const float *)p, n, pb, counts, nn2);
		else pair_hist_run<float, 3, false>(c, (const float *)p, n, pb, counts, nn2);
	}
	else
	{
		if (lds) pair_hist_run<double, 2, true>(c, (const double *)p, n, pb, counts, nn2);
		else pair_hist_run<double, 2, false>(c, (const double *)p, n, pb, counts, nn2);
	}
	if (counts)
		hipLaunchKernelGGL(pair_outside_kernel, dim3(1), dim3(kBlock), 0, c->stream, counts, pb.bins, (unsigned long long)n * (unsigned long long)(n - 1) / 2ull);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// ---- bond-orientational order, exact forms (bond_order_kernels.hpp) ---------------------------------
// the summary of a call from the wave records in `rec`: one workgroup adds them into c->small (doubles from kBondOut on), the host
// derives the means and the global Q.  Synchronises.
constexpr int kBondOut = 256;
int bond_summary_finish(nbco_ctx *c, const double *rec, long long records, long long n, int dim, nbco_bond_summary *sum_host)
{
	double *out = c->small.as<double>() + kBondOut;
	hipLaunchKernelGGL((bond_reduce_kernel<kBondRec, kBondRecBonds, kBondRecMax>), dim3(1), dim3(kBondGroups * kBondSlots), 0, c->stream, rec, records, out);
	NBCO_HIP(hipGetLastError());
	double h[kBondRec];
	NBCO_HIP(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	double S[kBondSums3], qsum[2] = {h[kBondRecQ], h[kBondRecQ + 1]};
	long long ints[3];
	memcpy(S, h, sizeof S);
	memcpy(ints, h + kBondRecBonds, sizeof ints);
	nbco_bond_summary s;
	memset(&s, 0, sizeof s);
	bond_summary_fill(S, qsum, ints[0], ints[1], ints[2], n, dim, s);
	*sum_host = s;
	return NBCO_OK;
}

int launch_bond_order(nbco_ctx *c, const void *p, int dim, long long n, double R2, int *nb, double *q, nbco_bond_summary *sum_host)
{
	const long long nt = (n + kBlock - 1) / kBlock, records = (n + 63) / 64;
	double *rec = nullptr;
	if (sum_host)
	{
		NBCO_TRY(c->reserve(c->part, sizeof(double) * kBondRec * (size_t)records));
		rec = c->part.as<double>();
	}
	const dim3 grid((unsigned)nt), block(kBlock);
	with_flag(sum_host != nullptr, [&](auto ws) {
		constexpr bool SUM = decltype(ws)::value;
		if (dim == 3) hipLaunchKernelGGL((bond_exact_kernel<float, 3, SUM>), grid, block, 0, c->stream, (const float *)p, n, R2, nb, q, rec);
		else hipLaunchKernelGGL((bond_exact_kernel<double, 2, SUM>), grid, block, 0, c->stream, (const double *)p, n, R2, nb, q, rec);
	});
	NBCO_HIP(hipGetLastError());
	return sum_host ? bond_summary_finish(c, rec, records, n, dim, sum_host) : NBCO_OK;
}

// nbco_bond_vectors: pass 1 alone, the records where q would go
int launch_bond_vectors(nbco_ctx *c, const float *p, long long n, double R2, int *nb, double *vec)
{
	const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
	hipLaunchKernelGGL((bond_exact_kernel<float, 3, false, true>), grid, block, 0, c->stream, p, n, R2, nb, vec, (double *)nullptr);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// the solid summary of a call from the wave records in `rec`, in the shape of bond_summary_finish.  Synchronises.
int bond_solid_finish(nbco_ctx *c, const double *rec, long long records, long long n, double dmin, int xi_min, nbco_solid_summary *sum_host)
{
	double *out = c->small.as<double>() + kBondOut;
	hipLaunchKernelGGL((bond_reduce_kernel<kSolidRec, kSolidRecBonds, kSolidRecMax>), dim3(1), dim3(kBondGroups * kBondSlots), 0, c->stream, rec, records, out);
	NBCO_HIP(hipGetLastError());
	double h[kSolidRec];
	NBCO_HIP(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	const double qsum[2] = {h[0], h[1]};
	long long ints[kSolidRec - kSolidRecBonds];
	memcpy(ints, h + kSolidRecBonds, sizeof ints);
	nbco_solid_summary s;
	memset(&s, 0, sizeof s);
	bond_solid_summary_fill(qsum, ints[0], ints[1], ints[2], ints[3], ints[4], n, dmin, xi_min, s);
	*sum_host = s;
	return NBCO_OK;
}

// nbco_bond_solid: pass 2 over the caller's records, or over the records of a pass 1 of its own in c->bond_vec
int launch_bond_solid(nbco_ctx *c, const float *p, long long n, double R2, const double *vec, double dmin, int xi_min, int *nb, int *xi, double *qbar,
                      nbco_solid_summary *sum_host)
{
	const long long records = (n + 63) / 64;
	if (!vec)
	{
		NBCO_TRY(c->reserve(c->bond_vec, sizeof(double) * kBondVec * (size_t)n));
		NBCO_TRY(launch_bond_vectors(c, p, n, R2, nullptr, c->bond_vec.as<double>()));
		vec = c->bond_vec.as<double>();
	}
	double *rec = nullptr;
	if (sum_host)
	{
		NBCO_TRY(c->reserve(c->part, sizeof(double) * kSolidRec * (size_t)records));
		rec = c->part.as<double>();
	}
	const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
	with_flag(sum_host != nullptr, [&](auto ws) {
		hipLaunchKernelGGL((bond_solid_exact_kernel<decltype(ws)::value>), grid, block, 0, c->stream, p, n, R2, vec, dmin, xi_min, nb, xi, qbar, rec);
	});
	NBCO_HIP(hipGetLastError());
	return sum_host ? bond_solid_finish(c, rec, records, n, dmin, xi_min, sum_host) : NBCO_OK;
}

// ---- sums on the wave-vector grid: static structure factor, mode records (structure_factor_kernels.hpp) ----
// The shape of a call, from n and the grid alone (never from the device): runs of ix of at most the term's last step, the cut of the items into
// workgroups (the fewest workgroups that keep 85 % of the lanes busy with `copies` copies of `lanes` items each, else the best cut up to
// four times as many), the tile that fills the LDS budget, and the particle ranges -- at least 512 particles each, no more of them than bring the launch to about 2048 workgroups
// or the partial sums to 256 MiB.
template <class Term>
static SkShape sk_shape(int dim, long long n, const nbco_sk_grid &g)
{
	constexpr int max_acc = last_step(typename Term::Steps{});
	SkShape s;
	s.hx = g.h[0]; s.hy = g.h[1]; s.hz = dim == 3 ? g.h[2] : 0;
	s.nch = (s.hx + max_acc) / max_acc;
	s.L = (s.hx + s.nch) / s.nch;
	s.ny = 2 * s.hy + 1; s.nz = 2 * s.hz + 1;
	s.items = s.nch * s.ny * s.nz;
	s.K = sk_count(g.h, dim);
	s.per = 1 + Term::kExtra + (s.hy + 1) + (dim == 3 ? s.hz + 1 : 0) + (s.nch > 1 ? s.nch : 0);
	s.tile = std::min(kSkBlock, kSkLdsBytes / (16 * s.per));
	const int kt0 = (s.items + kSkBlock - 1) / kSkBlock;
	int kt = kt0;
	double best = 0.0;
	for (int t = kt0; t <= 4 * kt0; ++t)
	{
		const int lanes = (s.items + t - 1) / t, copies = kSkBlock / lanes;
		const double busy = (double)s.items * copies / ((double)t * kSkBlock);
		if (busy > best) { best = busy; kt = t; }
		if (busy >= 0.85) break;
	}
	s.lanes = (s.items + kt - 1) / kt;
	s.copies = s.lanes <= kSkBlock / 2 ? kSkBlock / s.lanes : 1;
	long long r0 = std::min((n + 511) / 512, std::max(1LL, (long long)(2048 / kt)));
	r0 = std::max(1LL, std::min(r0, (256LL << 20) / (16 * Term::kParts * s.K)));
	s.range = ((n + r0 - 1) / r0 + 63) / 64 * 64;
	s.wx = g.kstep[0] / kSkTwoPi; s.wy = g.kstep[1] / kSkTwoPi; s.wz = dim == 3 ? g.kstep[2] / kSkTwoPi : 0.0;
	return s;
}

// The sums of a term over the n rows at p: record k (2 * Term::kParts doubles) goes to rec + k * stride.  `part` keeps the partial
// sums of the ranges where there are several.
template <class Term, bool DIM3, typename T>
static int kgrid_run(nbco_ctx *c, DevBuf &part, const T *p, long long n, const nbco_sk_grid &g, double *rec, long long stride, long long *n_used_host)
{
	constexpr int R = 2 * Term::kParts;
	const SkShape s = sk_shape<Term>(DIM3 ? 3 : 2, n, g);
	const long long ranges = (n + s.range - 1) / s.range;
	double *out = rec;
	long long ostride = stride;
	if (ranges > 1)
	{
		NBCO_TRY(c->reserve(part, sizeof(double) * R * (size_t)s.K * (size_t)ranges));
		out = part.as<double>();
		ostride = R;
	}
	const size_t lds = std::max((size_t)16 * s.per * s.tile, (size_t)16 * kSkBlock);   // the tables of a tile; the copies' sums at the end
	const dim3 grid((unsigned)((s.items + s.lanes - 1) / s.lanes), (unsigned)ranges), block(kSkBlock);
	with_step(typename Term::Steps{}, s.L, [&](auto a) {
		hipLaunchKernelGGL((kgrid_accumulate_kernel<Term, decltype(a)::value, DIM3, T>), grid, block, lds, c->stream, p, n, s, out, ostride);
	});
	NBCO_HIP(hipGetLastError());
	if (ranges > 1)
	{
		hipLaunchKernelGGL(sk_reduce_kernel<R>, dim3((unsigned)((R * s.K + kSkReduceJ - 1) / kSkReduceJ)), dim3(kSkBlock), 0, c->stream, (const double *)out, ranges, R * s.K, rec, stride);
		NBCO_HIP(hipGetLastError());
	}
	if (n_used_host)
	{
		// rho at k = 0, the first number of that record, is the exact count of the particles that counted
		const size_t k0 = (size_t)s.hy * (size_t)s.nz + (size_t)s.hz;
		double cnt = 0;
		NBCO_HIP(hipMemcpyAsync(&cnt, rec + k0 * (size_t)stride, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
		NBCO_HIP(hipStreamSynchronize(c->stream));
		*n_used_host = (long long)cnt;
	}
	return NBCO_OK;
}

int launch_structure_factor(nbco_ctx *c, const void *p, int dim, long long n, const nbco_sk_grid &g, double *rho, long long *n_used_host)
{
	if (dim == 3) return kgrid_run<SkTerm, true>(c, c->sk_part, (const float *)p, n, g, rho, 2, n_used_host);
	return kgrid_run<SkTerm, false>(c, c->sk_part, (const double *)p, n, g, rho, 2, n_used_host);
}

// record k of frame `frame` lies at series + 8 * frame + k * 8 * frames_cap
int launch_modes_record(nbco_ctx *c, const float *buf, long long n, const nbco_sk_grid &g, double *series, int frames_cap, int frame, long long *n_used_host)
{
	return kgrid_run<MdTerm, true>(c, c->md_part, buf, n, g, series + 8 * (size_t)frame, 8 * (long long)frames_cap, n_used_host);
}

// ---- tracked trajectories and their time correlations (time_corr_kernels.hpp) -----------------------
int launch_traj_record(nbco_ctx *c, const float *buf, long long n, const int *ids, float *traj, long long rows, int frames_cap, int frame, int stride)
{
	hipLaunchKernelGGL(traj_fill_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, traj, rows, (long long)frames_cap, frame);
	NBCO_HIP(hipGetLastError());
	hipLaunchKernelGGL(traj_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, buf, n, ids, traj, rows, (long long)frames_cap, frame, stride);
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// The lags a lane keeps, from the lags alone: 1 up to 64 lags, else pairs (2 up to 512 lags, 4 up to 1024, 8 beyond, at most max_a),
// with the lanes W of a row or a k (a multiple of 64) and the lags taken from the bottom.  Sets frames, lags, cap, half and W of s.
static int tc_lag_shape(int frames_cap, int frames, int lags, int max_a, TcShape &s)
{
	s.frames = frames; s.lags = lags; s.cap = frames_cap;
	if (lags <= 64) { s.half = lags; s.W = 64; return 1; }
	s.half = (lags + 1) / 2;
	const int A = std::min(max_a, s.half <= 256 ? 2 : s.half <= 512 ? 4 : 8);
	s.W = A == 2 ? (s.half + 63) / 64 * 64 : kTcBlock;
	return A;
}

// The shape of a call, from (rows, frames, lags) alone (never from the device): the lags a lane keeps, the lanes of a row, the rows
// a workgroup has in flight (what 256 lanes and 64 KiB of LDS hold) and the row ranges: no more than kTcMaxRanges, all but the last
// of one length.
static int tc_shape(long long rows, int frames_cap, int frames, int lags, TcShape &s)
{
	const int A = tc_lag_shape(frames_cap, frames, lags, 8, s);
	s.S = std::max(1, std::min(kTcBlock / s.W, kTcLdsBytes / (32 * frames)));
	const long long groups = (rows + s.S - 1) / s.S;
	const long long want = std::min(groups, (long long)kTcMaxRanges);
	s.range = (groups + want - 1) / want * s.S;
	s.ranges = (rows + s.range - 1) / s.range;
	return A;
}

int launch_time_corr(nbco_ctx *c, const float *traj, long long rows, int frames_cap, int frames, int lags, nbco_corr_lag *out_dev)
{
	TcShape s;
	const int A = tc_shape(rows, frames_cap, frames, lags, s);
	nbco_corr_lag *out = out_dev;
	if (s.ranges > 1)
	{
		NBCO_TRY(c->reserve(c->tc_part, sizeof(nbco_corr_lag) * (size_t)lags * (size_t)s.ranges));
		out = c->tc_part.as<nbco_corr_lag>();
	}
	const size_t lds = std::max((size_t)32 * (size_t)frames * (size_t)s.S, (size_t)8 * kTcBlock);
	const dim3 grid((unsigned)s.ranges), block(kTcBlock);
	with_step(std::integer_sequence<int, 1, 2, 4, 8>{}, A, [&](auto a) {
		hipLaunchKernelGGL((tc_accumulate_kernel<decltype(a)::value>), grid, block, lds, c->stream, traj, rows, s, out);
	});
	NBCO_HIP(hipGetLastError());
	if (s.ranges > 1)
	{
		hipLaunchKernelGGL(tc_reduce_kernel, dim3((unsigned)((8 * lags + kTcBlock - 1) / kTcBlock)), dim3(kTcBlock), 0, c->stream, (const nbco_corr_lag *)out, s.ranges, lags, out_dev);
		NBCO_HIP(hipGetLastError());
	}
	return NBCO_OK;
}

// ---- the time correlations of the collective modes (modes_kernels.hpp) -------------------------------
// The shape of a correlation call, from (frames, lags) alone: the lags a lane keeps (tc_lag_shape, at most 4), the lanes of a k and
// the k a workgroup serves (what 256 lanes and 64 KiB of LDS hold).
int launch_mode_corr(nbco_ctx *c, const double *series, const nbco_sk_grid &g, int frames_cap, int frames, int lags, nbco_mode_lag *out_dev)
{
	TcShape s;
	const int A = tc_lag_shape(frames_cap, frames, lags, 4, s);
	s.S = std::max(1, std::min(kTcBlock / s.W, kTcLdsBytes / (64 * frames)));
	const long long K = sk_count(g.h, 3);
	s.range = s.S;
	s.ranges = (K + s.S - 1) / s.S;
	const size_t lds = (size_t)64 * (size_t)frames * (size_t)s.S;
	const dim3 grid((unsigned)s.ranges), block(kTcBlock);
	with_step(std::integer_sequence<int, 1, 2, 4>{}, A, [&](auto a) {
		hipLaunchKernelGGL((mode_corr_kernel<decltype(a)::value>), grid, block, lds, c->stream, series, K, g, s, out_dev);
	});
	NBCO_HIP(hipGetLastError());
	return NBCO_OK;
}

// ---- aperture (aperture_kernels.hpp) -------------------------------------------------------------
// c->ap_cnt: the total (8 bytes, 16 reserved), then the levels of counts: tiles, tiles / 64, ..
constexpr size_t kApHead = 16;
static long long ap_level_size(long long tiles, int level) { for (int k = 0; k < level; ++k) tiles = (tiles + 63) >> kApGroupBits; return tiles; }

int launch_aperture_classify(nbco_ctx *c, const void *p, int dim, long long n, const ApRule &ap, bool tiles, long long *lost_host)
{
	const long long nt = (n + kBlock - 1) / kBlock;
	size_t ints = 0;
	if (tiles) for (int k = 0; k <= kApLevels; ++k) ints += (size_t)ap_level_size(nt, k);
	NBCO_TRY(c->reserve(c->ap_cnt, kApHead + sizeof(int) * ints));
	unsigned long long *total = c->ap_cnt.as<unsigned long long>();
	int *counts = reinterpret_cast<int *>(c->ap_cnt.as<char>() + kApHead);
	NBCO_HIP(hipMemsetAsync(total, 0, sizeof *total, c->stream));
	const dim3 grid((unsigned)nt), block(kBlock);
	if (dim == 3)
	{
		if (tiles) hipLaunchKernelGGL((aperture_classify_kernel<float, 3, true>), grid, block, 0, c->stream, (const float *)p, n, ap, counts, total);
		else hipLaunchKernelGGL((aperture_classify_kernel<float, 3, false>), grid, block, 0, c->stream, (const float *)p, n, ap, counts, total);
	}
	else
	{
		if (tiles) hipLaunchKernelGGL((aperture_classify_kernel<double, 2, true>), grid, block, 0, c->stream, (const double *)p, n, ap, counts, total);
		else hipLaunchKernelGGL((aperture_classify_kernel<double, 2, false>), grid, block, 0, c->stream, (const double *)p, n, ap, counts, total);
	}
	NBCO_HIP(hipGetLastError());
	unsigned long long h = 0;
	NBCO_HIP(hipMemcpyAsync(&h, total, sizeof h, hipMemcpyDeviceToHost, c->stream));
	NBCO_HIP(hipStreamSynchronize(c->stream));
	*lost_host = (long long)h;
	return NBCO_OK;
}

template <class T, int D>
static void aperture_scatter(nbco_ctx *c, T *buf, long long n, long long nk, const ApRule &ap, const ApOffsets &off, void *lost_dev, int *lost_row_dev,
                             const int *order_in, int *order_out)
{
	hipLaunchKernelGGL((aperture_scatter_kernel<T, D>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, (const T *)buf, n, nk, ap, off,
	                   c->ap_state.as<T>(), (T *)lost_dev, lost_row_dev, order_in, order_out);
}

int launch_aperture_compact(nbco_ctx *c, void *buf, int dim, long long n, long long lost, const ApRule &ap, void *lost_dev, int *lost_row_dev,
                            const int *order_in, int *order_out)
{
	const long long nk = n - lost;
	const size_t row = dim == 3 ? 9 * sizeof(float) : 6 * sizeof(double);
	NBCO_TRY(c->reserve(c->ap_state, row * (size_t)nk));   // (before anything is changed)
	// the counts of the classification, level by level, until one group holds a level
	ApOffsets off{};
	int *level = reinterpret_cast<int *>(c->ap_cnt.as<char>() + kApHead);
	long long m = (n + kBlock - 1) / kBlock;
	for (int k = 0; k < kApLevels; ++k)
	{
		const long long groups = (m + 63) >> kApGroupBits;
		hipLaunchKernelGGL(aperture_scan_kernel, dim3((unsigned)((groups + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, c->stream, level, m, level + m);
		off.level[k] = level;
		if (groups == 1) break;
		level += m;
		m = groups;
	}
	if (dim == 3) aperture_scatter<float, 3>(c, (float *)buf, n, nk, ap, off, lost_dev, lost_row_dev, order_in, order_out);
	else aperture_scatter<double, 2>(c, (double *)buf, n, nk, ap, off, lost_dev, lost_row_dev, order_in, order_out);
	NBCO_HIP(hipGetLastError());
	if (nk) NBCO_HIP(hipMemcpyAsync(buf, c->ap_state.ptr, row * (size_t)nk, hipMemcpyDeviceToDevice, c->stream));
	return NBCO_OK;
}

NBCO_CHECKED_COLLECT(nbco_checked_collect_reduce)
