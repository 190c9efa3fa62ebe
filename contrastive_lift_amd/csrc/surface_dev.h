// surface_dev.h -- the gradient of the VM density at one normalised point, in the lane roles of k_density_points: the body that
// k_density_grad_points (surface.hip) and the edited-scene gradient kernels (edit.hip) share, so that both carry the same bits.
#pragma once
#include "clift_dev.h"

// ============================================================================ un-weighted taps
// make_tap (clift_dev.h) folds "this tap is outside the table" into a zero WEIGHT.  A derivative needs the tap VALUES with the padding as the
// value 0 and the interpolation fractions as they are: the flags below are make_tap's own tests on make_tap's own index (the same expressions,
// hence the same floor), the fractions are its weights before the masking.
struct TapU {
    bool in0, in1;   // is tap i0 / i0 + 1 a texel of the table?
    float f0, f1;    // (1 - frac), frac
};
__device__ __forceinline__ TapU tap_unweighted(float x, int size) {
    TapU u;
    const float f = ((x + 1.0f) / 2.0f) * (float)(size - 1);
    const float fl = floorf(f);
    const int i0 = (int)fl;
    const int i1 = i0 + 1;
    u.f0 = ((fl + 1.0f) - f);
    u.f1 = (f - fl);
    u.in0 = !(i0 < 0 || i0 >= size);
    u.in1 = !(i1 < 0 || i1 >= size);
    return u;
}
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_keep(bool on, float4 a) { return on ? a : make_float4(0.f, 0.f, 0.f, 0.f); }
// s0 * a + s1 * b
__device__ __forceinline__ float4 f4_mix(float s0, float4 a, float s1, float4 b) { return f4_fma(s1, b, f4_scale(s0, a)); }

// ============================================================================ field gradient at one point, by its quad
// 4 lanes per point, lane q owns channels [4q, 4q + 4) (+16 per extra pass), quad sum by two xor shuffles.  The value repeats
// k_density_points' arithmetic term by term (the blends of vm_plane4 / vm_line4 on the masked weights, the channel order, the quad sum), so
// acc + shift carries the bits of clift_density_points(activation = 0).  Per plane i with axes (a, b) and line axis v, and channel c:
//   d/dx_a = (R_a - 1)/2 [(1 - f_b)(p10 - p00) + f_b (p11 - p01)] L,   d/dx_b likewise,   d/dx_v = (R_v - 1)/2 P (l1 - l0)
// inside the cell make_tap selects (floor: the right-sided derivative on a texel line), a tap outside the table counting as the value 0.
// ``on``: this lane's point is looked up (a lane that is off reads no table and adds zeros); the four lanes of a quad must all reach the
// shuffles.  Returns the quad's sums in every lane of the quad: acc = sigma_raw - shift, g = d sigma_raw / d xn.
__device__ __forceinline__ void vm_density_grad_quad(const VmP& t, const float xn[3], int q, bool on, float& acc, float g[3]) {
    acc = 0.f;
    g[0] = g[1] = g[2] = 0.f;
    const int C = t.comps;
    if (on) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int a, b, v;
            vm_axes(i, a, b, v);
            const VmTaps k = vm_taps(t, i, xn);
            const TapU ux = tap_unweighted(xn[a], t.res[a]), uy = tap_unweighted(xn[b], t.res[b]), uz = tap_unweighted(xn[v], t.res[v]);
            const int W = t.res[a];
            const float* pp = t.plane[i];
            const float* lp = t.line[i];
            const float w00 = k.tx.w0 * k.ty.w0, w10 = k.tx.w1 * k.ty.w0, w01 = k.tx.w0 * k.ty.w1, w11 = k.tx.w1 * k.ty.w1;
            float da = 0.f, db = 0.f, dv = 0.f;
            for (int c4 = q * 4; c4 < C; c4 += 16) {
                const float4 p00 = ld4(pp + ((size_t)k.ty.i0 * W + k.tx.i0) * C + c4);
                const float4 p10 = ld4(pp + ((size_t)k.ty.i0 * W + k.tx.i1) * C + c4);
                const float4 p01 = ld4(pp + ((size_t)k.ty.i1 * W + k.tx.i0) * C + c4);
                const float4 p11 = ld4(pp + ((size_t)k.ty.i1 * W + k.tx.i1) * C + c4);
                const float4 l0 = ld4(lp + (size_t)k.tz.i0 * C + c4);
                const float4 l1 = ld4(lp + (size_t)k.tz.i1 * C + c4);
                // the value: vm_plane4 / vm_line4 on the same reads
                float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
                P = f4_fma(w00, p00, P);
                P = f4_fma(w10, p10, P);
                P = f4_fma(w01, p01, P);
                P = f4_fma(w11, p11, P);
                float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
                L = f4_fma(k.tz.w0, l0, L);
                L = f4_fma(k.tz.w1, l1, L);
                acc += f4_hsum(f4_mul(P, L));
                // the partials: corner values with the padding as 0
                const float4 m00 = f4_keep(ux.in0 && uy.in0, p00), m10 = f4_keep(ux.in1 && uy.in0, p10);
                const float4 m01 = f4_keep(ux.in0 && uy.in1, p01), m11 = f4_keep(ux.in1 && uy.in1, p11);
                const float4 dPa = f4_mix(uy.f0, f4_sub(m10, m00), uy.f1, f4_sub(m11, m01));
                const float4 dPb = f4_mix(ux.f0, f4_sub(m01, m00), ux.f1, f4_sub(m11, m10));
                const float4 dL = f4_sub(f4_keep(uz.in1, l1), f4_keep(uz.in0, l0));
                da += f4_hsum(f4_mul(dPa, L));
                db += f4_hsum(f4_mul(dPb, L));
                dv += f4_hsum(f4_mul(P, dL));
            }
            g[a] += (0.5f * (float)(t.res[a] - 1)) * da;
            g[b] += (0.5f * (float)(t.res[b] - 1)) * db;
            g[v] += (0.5f * (float)(t.res[v] - 1)) * dv;
        }
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        g[j] += __shfl_xor(g[j], 1);
        g[j] += __shfl_xor(g[j], 2);
    }
}
