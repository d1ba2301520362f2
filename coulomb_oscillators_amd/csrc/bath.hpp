// bath.hpp -- the Langevin bath (include/nbco.h, nbco_bath_apply): the exact Ornstein-Uhlenbeck step of the velocities,
// v' = (c1 v) + (c2 xi) per particle row and axis, with the coefficients of nbco_bath_coeffs as kernel arguments and the noise xi from
// Philox4x32-10 over (seed, tick, half, row, axis).  Every kernel that contains the step calls bath_kick, so that a particle sees the
// same roundings whichever pass moves it.
#pragma once
#include <cstdint>

struct Bath3 { float c1[3], c2[3]; uint32_t key[2], tick[2]; int half; };    // coefficients narrowed to float once on the host
struct Bath2 { double c1[2], c2[2]; uint32_t key[2], tick[2]; int half; };   // the 2-D fp64 form

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
	for (int r = 0; r < 10; ++r)
	{
		const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
		const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
		c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the noise of (row, axis): the four words summed as an integer, centred, scaled by sqrt(3) 2^-32 in double (one rounding)
__device__ __forceinline__ double bath_xi(const uint32_t (&key)[2], const uint32_t (&tick)[2], int half, long long row, int axis)
{
	uint32_t w[4];
	philox4x32_10((uint32_t)row, (uint32_t)(axis + 4 * half), tick[0], tick[1], key[0], key[1], w);
	const long long S = (long long)w[0] + (long long)w[1] + (long long)w[2] + (long long)w[3];
	return __dmul_rn((double)(S - 0x1FFFFFFFELL), 0x1.bb67ae8584caap-32);
}

// an axis with c1 = 1 and c2 = 0 (gamma = 0) is not touched at all: its bytes stay, and its noise is not drawn
__device__ __forceinline__ void bath_kick(const Bath3 &b, long long row, float (&v)[3])
{
#pragma clang fp contract(off)
#pragma unroll
	for (int a = 0; a < 3; ++a)
	{
		if (b.c1[a] == 1.f && b.c2[a] == 0.f) continue;
		const float xi = (float)bath_xi(b.key, b.tick, b.half, row, a);
		v[a] = __fadd_rn(__fmul_rn(b.c1[a], v[a]), __fmul_rn(b.c2[a], xi));
	}
}

__device__ __forceinline__ void bath_kick(const Bath2 &b, long long row, double (&v)[2])
{
#pragma clang fp contract(off)
#pragma unroll
	for (int a = 0; a < 2; ++a)
	{
		if (b.c1[a] == 1.0 && b.c2[a] == 0.0) continue;
		const double xi = bath_xi(b.key, b.tick, b.half, row, a);
		v[a] = __dadd_rn(__dmul_rn(b.c1[a], v[a]), __dmul_rn(b.c2[a], xi));
	}
}

// the same bath one tick later, opening half: what follows the closing half of a step inside a fused run
__device__ __forceinline__ Bath3 bath_next_open(const Bath3 &b)
{
	Bath3 o = b;
	o.half = 0;
	o.tick[0] = b.tick[0] + 1u;
	o.tick[1] = b.tick[1] + (o.tick[0] == 0u ? 1u : 0u);
	return o;
}
