// lattice_dev.h -- sigma at one point of the box lattice: the lines k_dense_sigma (isosurface.hip) and k_edit_list_dense_sigma (edit.hip)
// share, so that a lattice point no edit touches gets the same bits from both.
#pragma once
#include "clift_dev.h"

// Lattice point p_a = lo_a (1 - s) + hi_a s (s = the caller's linspace value of that axis) and its normalised coordinates (renderer.py:633).
__device__ __forceinline__ void lattice_point(float3 lo, float3 hi, float3 inv_ext2, float a, float b, float c, float p[3], float xn[3]) {
    p[0] = lo.x * (1.f - a) + hi.x * a;
    p[1] = lo.y * (1.f - b) + hi.y * b;
    p[2] = lo.z * (1.f - c) + hi.z * c;
    xn[0] = (p[0] - lo.x) * inv_ext2.x - 1.f;
    xn[1] = (p[1] - lo.y) * inv_ext2.y - 1.f;
    xn[2] = (p[2] - lo.z) * inv_ext2.z - 1.f;
}

// Lane q of the 4 lanes of a point: the plane x line products of channels [4q, 4q + 4) + 16 per pass, summed over the three planes.  The
// caller adds the four lanes up (two __shfl_xor) and applies vm_sigma.
__device__ __forceinline__ float vm_density_lane(const VmP& t, const float xn[3], int q) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const VmTaps tp = vm_taps(t, i, xn);
        for (int c4 = q * 4; c4 < t.comps; c4 += 16) acc += f4_hsum(f4_mul(vm_plane4(t, i, tp, c4), vm_line4(t, i, tp, c4)));
    }
    return acc;
}

// softplus(density + shift) (tensoRF.py:114-125)
__device__ __forceinline__ float vm_sigma(float acc, float shift) {
    const float x = acc + shift;
    return (x > 20.f) ? x : log1pf(expf(x));
}
