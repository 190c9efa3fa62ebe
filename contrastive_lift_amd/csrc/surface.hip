// surface.hip -- surface outputs of the ray route: the gradient of the VM density with respect to position, and per ray the
// median-depth hit and the composited field normal, both from what a march already stored.
//   k_density_grad_points   [d sigma_raw / dx, sigma_raw] at explicit normalised points: the lookup of k_density_points (march.hip) with the four
//                           bilinear corners kept un-blended, so that the value and both partials come from the same 18 table reads
//   k_ray_surface           one wave per ray: the first sample at which the transmittance left behind it, T - w, has fallen to 1 - q, the depth
//                           interpolated inside that sample's interval, and sum_k w_k n_k over the ray's active samples
// No atomics: every output element is written by one lane, the sums run in a fixed order -- two runs give the same bits.
#include "clift_dev.h"
#include "surface_dev.h"

// ============================================================================ field gradient at arbitrary points
// The lane roles of k_density_points: 4 lanes per point, the quad's arithmetic in vm_density_grad_quad (surface_dev.h, shared with the
// edited-scene gradient of edit.hip).  Column 3 carries the bits of clift_density_points(activation = 0).
__global__ __launch_bounds__(256) void k_density_grad_points(VmP t, const float* __restrict__ xn3, int ldx, long total, float shift, float3 scale,
                                                              float* __restrict__ out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long s = gid >> 2;
    const int q = (int)(gid & 3);
    if (s >= total) return;
    const float xn[3] = {xn3[s * ldx + 0], xn3[s * ldx + 1], xn3[s * ldx + 2]};
    float acc, g[3];
    vm_density_grad_quad(t, xn, q, true, acc, g);
    if (q == 0) *reinterpret_cast<float4*>(out + (size_t)s * 4) = make_float4(g[0] * scale.x, g[1] * scale.y, g[2] * scale.z, acc + shift);
}

extern "C" int clift_density_grad_points(const clift_vm_t* h_dens, const float* xn, int ldx, long n, float shift, const float* h_inv2, float* out,
                                         clift_stream_t s) {
    CLIFT_REQUIRE(h_dens != nullptr, "clift_density_grad_points: NULL table record");
    CLIFT_REQUIRE(h_dens->comps > 0 && h_dens->comps % 4 == 0, "clift_density_grad_points: comps must be a positive multiple of 4 (got %d)", h_dens->comps);
    CLIFT_REQUIRE(h_dens->res[0] >= 1 && h_dens->res[1] >= 1 && h_dens->res[2] >= 1, "clift_density_grad_points: table sizes must be positive");
    CLIFT_REQUIRE(ldx >= 3, "clift_density_grad_points: ldx must be >= 3");
    if (n <= 0) return 0;
    CLIFT_REQUIRE(n < (1L << 36), "clift_density_grad_points: %ld points, the limit is 2^36", n);
    CLIFT_REQUIRE(xn != nullptr && out != nullptr, "clift_density_grad_points: NULL buffer");
    const float3 scale = h_inv2 ? make_float3(h_inv2[0], h_inv2[1], h_inv2[2]) : make_float3(1.f, 1.f, 1.f);
    k_density_grad_points<<<cdiv(n * 4, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), xn, ldx, n, shift, scale, out);
    return clift_check_launch("clift_density_grad_points");
}

// ============================================================================ median hit and normal map of a ray
// One wave per ray, as k_march_fwd.  All comparisons are on the march's stored fp32 arrays: rem_k = T[k] - w[k] (one fp32 subtraction) is the
// transmittance left behind sample k, thr = 1 - q (one fp32 subtraction).
//   sweep 1: the S samples in chunks of 64, ballot of rem_k <= thr, lowest set bit; stops at the first chunk that has one.  prev = rem of the
//            sample before it (the lane before, or the last lane of the chunk before; 1 for k = 0), den = prev - rem_k,
//            f = den > 0 ? clamp((prev - thr) / den, 0, 1) : 0, z_med = z_k + f delta_k with the march's own z_k and delta_k (0 at k = S - 1).
//   sweep 2: the ray's segment [ray_start[r], ray_start[r + 1]) of the active list, 64 entries per trip: n = -g / |g| (0 where |g|^2 < 1e-30)
//            from row j of G, w from the stored weights at act_idx[j]; per-lane sums in list order, then the xor butterfly.
// Out of range entries of ray_start / act_idx (a caller's mistake) are clamped resp. skipped, never followed.
__global__ __launch_bounds__(256) void k_ray_surface(MarchP m, const float* __restrict__ rays, const float* __restrict__ jitter, int N,
                                                      const float* __restrict__ T_i, const float* __restrict__ w_i, const int* __restrict__ ray_start,
                                                      const int* __restrict__ act, int M, const float* __restrict__ G, float thr,
                                                      float* __restrict__ depth_med, int* __restrict__ k_med, float* __restrict__ normal) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    const int l = lane_id();
    const int S = m.S;
    const RayG g = load_ray(rays, r, m);
    const float jit = jitter ? jitter[r] : 0.f;
    // ---------------- sweep 1
    int km = -1;
    float zmed = 0.f;
    float last = 1.f;                                    // rem of the sample before this chunk
    for (int base = 0; base < S; base += 64) {
        const int k = base + l;
        const bool valid = k < S;
        const size_t o = (size_t)r * S + (valid ? k : 0);
        const float rem = valid ? __fsub_rn(T_i[o], w_i[o]) : 2.f;
        const unsigned long long bal = __ballot(valid && rem <= thr);
        if (bal != 0ull) {                               // wave-uniform
            const int first = __ffsll((long long)bal) - 1;
            const float rk = __shfl(rem, first);
            const float before = __shfl(rem, max(first - 1, 0));
            const float prev = first > 0 ? before : last;
            const float den = __fsub_rn(prev, rk);
            const float f = den > 0.f ? fminf(fmaxf(__fdiv_rn(__fsub_rn(prev, thr), den), 0.f), 1.f) : 0.f;
            km = base + first;
            const float z0 = sample_z(g, m, km, jit), z1 = sample_z(g, m, km + 1, jit);
            const float delta = km < S - 1 ? __fsub_rn(z1, z0) : 0.f;
            zmed = __fadd_rn(z0, __fmul_rn(f, delta));
            break;
        }
        last = __shfl(rem, 63);
    }
    // ---------------- sweep 2
    float ax = 0.f, ay = 0.f, az = 0.f;
    const int j0 = min(max(ray_start[r], 0), M), j1 = min(max(ray_start[r + 1], 0), M);
    const long NS = (long)N * S;
    for (int j = j0 + l; j < j1; j += 64) {
        const int sid = act[j];
        if (sid < 0 || (long)sid >= NS) continue;
        const float wv = w_i[sid];
        const float4 gr = ld4(G + (size_t)j * 4);
        const float len2 = gr.x * gr.x + gr.y * gr.y + gr.z * gr.z;
        if (len2 >= 1e-30f) {
            const float sc = -wv / sqrtf(len2);
            ax += sc * gr.x; ay += sc * gr.y; az += sc * gr.z;
        }
    }
    ax = wave_sum(ax); ay = wave_sum(ay); az = wave_sum(az);
    if (l == 0) {
        depth_med[r] = zmed;
        k_med[r] = km;
        *reinterpret_cast<float4*>(normal + (size_t)r * 4) = make_float4(ax, ay, az, 0.f);
    }
}

extern "C" int clift_ray_surface(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* T, const float* w,
                                 const int* ray_start, const int* act_idx, int M, const float* G, float q, float* depth_med, int* k_med,
                                 float* normal, clift_stream_t s) {
    CLIFT_REQUIRE(h_m != nullptr, "clift_ray_surface: NULL march record");
    CLIFT_REQUIRE(q > 0.f && q < 1.f, "clift_ray_surface: q must lie in (0, 1) (got %g)", (double)q);
    CLIFT_REQUIRE(h_m->n_samples >= 1, "clift_ray_surface: the march has no samples");
    CLIFT_REQUIRE(M >= 0, "clift_ray_surface: negative M");
    if (N <= 0) return 0;
    CLIFT_REQUIRE((long)N * h_m->n_samples < 2147483647L, "clift_ray_surface: N*S overflows int32 sample ids");
    CLIFT_REQUIRE(rays && T && w && ray_start && depth_med && k_med && normal, "clift_ray_surface: NULL buffer");
    CLIFT_REQUIRE(M == 0 || (act_idx && G), "clift_ray_surface: NULL act_idx / G with M = %d", M);
    const float thr = 1.0f - q;
    k_ray_surface<<<cdiv(N, 4), 256, 0, as_stream(s)>>>(to_dev(h_m), rays, jitter, N, T, w, ray_start, act_idx, M, G, thr, depth_med, k_med, normal);
    return clift_check_launch("clift_ray_surface");
}
