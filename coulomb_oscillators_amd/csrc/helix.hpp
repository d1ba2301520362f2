// helix.hpp -- the drift in a uniform magnetic field (include/nbco.h, nbco_drift_b): free motion along a helix, x += A v, v = R v with
// the two matrices of nbco_helix_matrices.  The matrices are the same for every particle; they travel as kernel arguments.  Every
// kernel that contains the drift calls helix_drift, so that a particle sees the same roundings whichever pass moves it.
#pragma once

struct Helix3 { float A[9], R[9]; };     // row-major, narrowed to float once on the host
struct Helix2 { double A[4], R[4]; };    // the 2-D fp64 form

// x'[c] = A[c][0] vx + A[c][1] vy + A[c][2] vz + x[c],  v'[c] = R[c][0] vx + R[c][1] vy + R[c][2] vz, both from the old v, one
// rounding per fmaf in exactly this order (include/nbco.h states it; nbco_cpu.hpp and the tests' float32 model repeat it)
__device__ __forceinline__ void helix_drift(const Helix3 &h, float (&x)[3], float (&v)[3])
{
	const float vx = v[0], vy = v[1], vz = v[2];
#pragma unroll
	for (int c = 0; c < 3; ++c)
	{
		x[c] = fmaf(h.A[3 * c + 2], vz, fmaf(h.A[3 * c + 1], vy, fmaf(h.A[3 * c], vx, x[c])));
		v[c] = fmaf(h.R[3 * c + 2], vz, fmaf(h.R[3 * c + 1], vy, h.R[3 * c] * vx));
	}
}
