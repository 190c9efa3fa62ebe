// layers.hip -- amodal instance layers of the ray route: what every instance covers along a ray, also behind what hides it,
// from what a march already stored and one slot per listed sample.
//   k_sample_slots   one thread per list row: the class of the row's semantic output (first maximum), then inside that class's slot range the
//                    nearest centroid (mode 0) or the first maximum of the row's slot scores (mode 1)
//   k_ray_layers     one wave per ray: the ray's range of an alpha-list walked in order; per column (K instance slots and the rest column) a
//                    transmittance of its own, the scene's weight, the expected distance and the distance of the first entry
//   k_ray_layer_colour  the same walk with a colour per list row: per column its premultiplied colour and opacity when alone
// Every operation is rounded on its own (no fmaf), so that an fp32 numpy loop restates both kernels to the bit.  No atomics, no LDS: every
// output element is written once by one lane, the walks run in list order -- two runs give the same bits.
#include "clift_dev.h"

// ============================================================================ one slot per list row
__global__ __launch_bounds__(256) void k_sample_slots(const float* __restrict__ sem, int lds, int C, const float* __restrict__ feat, int ldf, int E,
                                                       const float* __restrict__ add, int lda, const int* __restrict__ cls_slots,
                                                       const float* __restrict__ cent, int K, int mode, long n, int* __restrict__ slot) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const float* sr = sem + (size_t)row * lds;
    int cls = 0;
    float best_s = sr[0];
    for (int c = 1; c < C; ++c) {
        const float v = sr[c];
        if (v > best_s) { best_s = v; cls = c; }
    }
    const long off = cls_slots[2 * cls], cnt = cls_slots[2 * cls + 1];
    // the class's range, cut to [0, K): nothing outside centroids (K, E) is read, no slot outside [0, K) is given
    const int lo = (int)max(off, 0L), hi = (int)min(off + cnt, (long)K);
    if (cnt <= 0 || hi <= lo) { slot[row] = -1; return; }
    const float* fr = feat + (size_t)row * ldf;
    const float* ar = add ? add + (size_t)row * lda : nullptr;
    int win = -1;
    if (mode == 0) {
        float best = INFINITY;
        for (int c = lo; c < hi; ++c) {
            const float* cr = cent + (size_t)c * E;
            float d2 = 0.f;
            for (int e = 0; e < E; ++e) {
                const float f = ar ? __fadd_rn(fr[e], ar[e]) : fr[e];
                const float d = __fsub_rn(f, cr[e]);
                d2 = __fadd_rn(d2, __fmul_rn(d, d));
            }
            if (d2 < best) { best = d2; win = c; }        // strict: the lowest index wins a tie; NaN and +inf never win
        }
    } else {
        const int ne = min(hi - lo, E);
        float best = ar ? __fadd_rn(fr[0], ar[0]) : fr[0];
        win = lo;
        for (int e = 1; e < ne; ++e) {
            const float f = ar ? __fadd_rn(fr[e], ar[e]) : fr[e];
            if (f > best) { best = f; win = lo + e; }
        }
    }
    slot[row] = win;
}

extern "C" int clift_sample_slots(const float* sem, int lds, int C, const float* feat, int ldf, int E, const float* add, int lda,
                                  const int* cls_slots, const float* centroids, int K, int mode, long n, int* slot, clift_stream_t s) {
    CLIFT_REQUIRE(C >= 1, "clift_sample_slots: C must be >= 1 (got %d)", C);
    CLIFT_REQUIRE(E >= 1, "clift_sample_slots: E must be >= 1 (got %d)", E);
    CLIFT_REQUIRE(K >= 0 && K <= 255, "clift_sample_slots: K must lie in [0, 255] (got %d)", K);
    CLIFT_REQUIRE(lds >= C, "clift_sample_slots: lds must be >= C");
    CLIFT_REQUIRE(ldf >= E, "clift_sample_slots: ldf must be >= E");
    CLIFT_REQUIRE(add == nullptr || lda >= E, "clift_sample_slots: lda must be >= E");
    CLIFT_REQUIRE(mode == 0 || mode == 1, "clift_sample_slots: mode must be 0 (nearest centroid) or 1 (slot scores) (got %d)", mode);
    if (n <= 0) return 0;
    CLIFT_REQUIRE(n < (1L << 31) * 256, "clift_sample_slots: %ld rows, the limit is 2^39", n);
    CLIFT_REQUIRE(sem && feat && cls_slots && slot, "clift_sample_slots: NULL buffer");
    CLIFT_REQUIRE(mode != 0 || K == 0 || centroids != nullptr, "clift_sample_slots: NULL centroids with K = %d", K);
    k_sample_slots<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(sem, lds, C, feat, ldf, E, add, lda, cls_slots, centroids, K, mode, n, slot);
    return clift_check_launch("clift_sample_slots");
}

// ============================================================================ the layers of a ray
// One wave per ray, as k_ray_surface.  Lane l owns the columns l, l + 64, l + 128, l + 192 < K + 1 in Q = ceil((K + 1) / 64) register sets: the
// set index is a compile-time constant everywhere (loops over Q are unrolled), nothing is indexed at run time and nothing goes to scratch.
// The ray's range of the list is read 64 entries per trip -- act_idx and slot coalesced, alpha and w gathered, z formed by the lane -- and the
// entries of a trip are then walked in order: the wave index is made scalar (readfirstlane), so the range, the mask of the entries that
// belong to the ray and the walk over its set bits are scalar, and an entry's (column, alpha, w, z) is read out of its lane with v_readlane.
// Only the lane that owns the column updates its registers.
struct LayerAcc {
    float Tc, V, Z, zf;
    bool seen;
};

__device__ __forceinline__ float read_lane(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }

template <int Q>
__global__ __launch_bounds__(256) void k_ray_layers(MarchP m, const float* __restrict__ rays, const float* __restrict__ jitter, int N,
                                                     const float* __restrict__ alpha, const float* __restrict__ w_i,
                                                     const int* __restrict__ ray_start, const int* __restrict__ act, int M,
                                                     const int* __restrict__ slot, int K, float* __restrict__ out) {
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= N) return;
    const int l = lane_id();
    const int S = m.S;
    const RayG g = load_ray(rays, r, m);
    const float jit = jitter ? jitter[r] : 0.f;
    LayerAcc acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = LayerAcc{1.f, 0.f, 0.f, 0.f, false};
    const int j0 = min(max(ray_start[r], 0), M), j1 = min(max(ray_start[r + 1], 0), M);
    const long first = (long)r * S;
    for (int base = j0; base < j1; base += 64) {
        const int j = base + l;
        const bool in = j < j1;
        const long sid = in ? (long)act[j] : -1L;
        const long kl = sid - first;
        const bool ok = in && sid >= 0 && kl >= 0 && kl < S;          // an entry of another ray or out of range: skipped, never followed
        const int k = ok ? (int)kl : 0;
        const int sl = ok ? slot[j] : -1;
        const int col = (sl >= 0 && sl < K) ? sl : K;
        const float a = ok ? alpha[sid] : 0.f;
        const float wv = ok ? w_i[sid] : 0.f;
        const float z = sample_z(g, m, k, jit);
        unsigned long long todo = __ballot(ok);
        while (todo != 0ull) {                                       // scalar: the entries of this trip, in list order
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const int c = __builtin_amdgcn_readlane(col, i);
            const float ai = read_lane(a, i), wi = read_lane(wv, i), zi = read_lane(z, i);
            const int set = c >> 6;
            if (l == (c & 63)) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (set == q) {
                        LayerAcc& A = acc[q];
                        if (!A.seen) { A.zf = zi; A.seen = true; }
                        const float u = __fmul_rn(A.Tc, ai);
                        A.Z = __fadd_rn(A.Z, __fmul_rn(u, zi));
                        A.V = __fadd_rn(A.V, wi);
                        A.Tc = __fmul_rn(A.Tc, __fsub_rn(1.f, ai));
                    }
                }
            }
        }
    }
    float* row = out + (size_t)r * (size_t)(K + 1) * 4;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = l + 64 * q;
        if (c <= K) *reinterpret_cast<float4*>(row + (size_t)c * 4) = make_float4(__fsub_rn(1.f, acc[q].Tc), acc[q].V, acc[q].Z, acc[q].zf);
    }
}

extern "C" int clift_ray_layers(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* alpha, const float* w,
                                const int* ray_start, const int* act_idx, int M, const int* slot, int K, float* out, clift_stream_t s) {
    CLIFT_REQUIRE(h_m != nullptr, "clift_ray_layers: NULL march record");
    CLIFT_REQUIRE(K >= 0 && K <= 255, "clift_ray_layers: K must lie in [0, 255] (got %d)", K);
    CLIFT_REQUIRE(h_m->n_samples >= 1, "clift_ray_layers: the march has no samples");
    CLIFT_REQUIRE(M >= 0, "clift_ray_layers: negative M");
    if (N <= 0) return 0;
    CLIFT_REQUIRE((long)N * h_m->n_samples < 2147483647L, "clift_ray_layers: N*S overflows int32 sample ids");
    CLIFT_REQUIRE(rays && alpha && w && ray_start && out, "clift_ray_layers: NULL buffer");
    CLIFT_REQUIRE(M == 0 || (act_idx && slot), "clift_ray_layers: NULL act_idx / slot with M = %d", M);
    const MarchP m = to_dev(h_m);
    const dim3 grid(cdiv(N, 4)), block(256);
    hipStream_t st = as_stream(s);
    switch (K / 64) {          // sets of 64 columns that K + 1 columns need, less one
    case 0: k_ray_layers<1><<<grid, block, 0, st>>>(m, rays, jitter, N, alpha, w, ray_start, act_idx, M, slot, K, out); break;
    case 1: k_ray_layers<2><<<grid, block, 0, st>>>(m, rays, jitter, N, alpha, w, ray_start, act_idx, M, slot, K, out); break;
    case 2: k_ray_layers<3><<<grid, block, 0, st>>>(m, rays, jitter, N, alpha, w, ray_start, act_idx, M, slot, K, out); break;
    default: k_ray_layers<4><<<grid, block, 0, st>>>(m, rays, jitter, N, alpha, w, ray_start, act_idx, M, slot, K, out); break;
    }
    return clift_check_launch("clift_ray_layers");
}

// ============================================================================ the colour of every layer of a ray
// The walk of k_ray_layers -- the same columns, the same skipped entries, the same order -- with the colour of a list row in place of its
// distance and weight: per column R, G, B += (Tc a) c and Tc *= 1 - a, every operation rounded on its own.  An entry without a colour (its
// row of rgb_row outside [0, n_rgb)) still takes its share of the column's transmittance; its colour is never read.  The march record gives S
// alone: no ray is loaded and no distance is formed.
struct ColourAcc {
    float Tc, R, G, B;
};

template <int Q>
__global__ __launch_bounds__(256) void k_ray_layer_colour(int S, int N, const float* __restrict__ alpha, const int* __restrict__ ray_start,
                                                           const int* __restrict__ act, int M, const int* __restrict__ slot, int K,
                                                           const float* __restrict__ rgb, int ldc, long n_rgb,
                                                           const int* __restrict__ rgb_row, float* __restrict__ out) {
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= N) return;
    const int l = lane_id();
    ColourAcc acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = ColourAcc{1.f, 0.f, 0.f, 0.f};
    const int j0 = min(max(ray_start[r], 0), M), j1 = min(max(ray_start[r + 1], 0), M);
    const long first = (long)r * S;
    for (int base = j0; base < j1; base += 64) {
        const int j = base + l;
        const bool in = j < j1;
        const long sid = in ? (long)act[j] : -1L;
        const long kl = sid - first;
        const bool ok = in && sid >= 0 && kl >= 0 && kl < S;          // an entry of another ray or out of range: skipped, never followed
        const int sl = ok ? slot[j] : -1;
        const int col = (sl >= 0 && sl < K) ? sl : K;
        const float a = ok ? alpha[sid] : 0.f;
        const long row = ok ? (rgb_row ? (long)rgb_row[j] : (long)j) : -1L;
        const bool has = row >= 0 && row < n_rgb;                     // no colour: rgb is not read
        const float* cr = rgb + (size_t)(has ? row : 0) * (size_t)ldc;
        const float cR = has ? cr[0] : 0.f, cG = has ? cr[1] : 0.f, cB = has ? cr[2] : 0.f;
        unsigned long long todo = __ballot(ok);
        const unsigned long long coloured = __ballot(has);
        while (todo != 0ull) {                                       // scalar: the entries of this trip, in list order
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const int c = __builtin_amdgcn_readlane(col, i);
            const float ai = read_lane(a, i), ri = read_lane(cR, i), gi = read_lane(cG, i), bi = read_lane(cB, i);
            const bool ci = (coloured >> i) & 1ull;
            const int set = c >> 6;
            if (l == (c & 63)) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (set == q) {
                        ColourAcc& A = acc[q];
                        const float u = __fmul_rn(A.Tc, ai);
                        if (ci) {
                            A.R = __fadd_rn(A.R, __fmul_rn(u, ri));
                            A.G = __fadd_rn(A.G, __fmul_rn(u, gi));
                            A.B = __fadd_rn(A.B, __fmul_rn(u, bi));
                        }
                        A.Tc = __fmul_rn(A.Tc, __fsub_rn(1.f, ai));
                    }
                }
            }
        }
    }
    float* orow = out + (size_t)r * (size_t)(K + 1) * 4;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = l + 64 * q;
        if (c <= K) *reinterpret_cast<float4*>(orow + (size_t)c * 4) = make_float4(acc[q].R, acc[q].G, acc[q].B, __fsub_rn(1.f, acc[q].Tc));
    }
}

extern "C" int clift_ray_layer_colour(const clift_march_t* h_m, int N, const float* alpha, const int* ray_start, const int* act_idx, int M,
                                      const int* slot, int K, const float* rgb, int ldc, long n_rgb, const int* rgb_row, float* out,
                                      clift_stream_t s) {
    CLIFT_REQUIRE(h_m != nullptr, "clift_ray_layer_colour: NULL march record");
    CLIFT_REQUIRE(K >= 0 && K <= 255, "clift_ray_layer_colour: K must lie in [0, 255] (got %d)", K);
    CLIFT_REQUIRE(h_m->n_samples >= 1, "clift_ray_layer_colour: the march has no samples");
    CLIFT_REQUIRE(M >= 0, "clift_ray_layer_colour: negative M");
    CLIFT_REQUIRE(ldc >= 3, "clift_ray_layer_colour: ldc must be >= 3 (got %d)", ldc);
    CLIFT_REQUIRE(n_rgb >= 0, "clift_ray_layer_colour: negative n_rgb");
    if (N <= 0) return 0;
    CLIFT_REQUIRE((long)N * h_m->n_samples < 2147483647L, "clift_ray_layer_colour: N*S overflows int32 sample ids");
    CLIFT_REQUIRE(alpha && ray_start && out, "clift_ray_layer_colour: NULL buffer");
    CLIFT_REQUIRE(M == 0 || (act_idx && slot), "clift_ray_layer_colour: NULL act_idx / slot with M = %d", M);
    CLIFT_REQUIRE(n_rgb == 0 || rgb != nullptr, "clift_ray_layer_colour: NULL rgb with n_rgb = %ld", n_rgb);
    const int S = h_m->n_samples;
    const dim3 grid(cdiv(N, 4)), block(256);
    hipStream_t st = as_stream(s);
    switch (K / 64) {          // sets of 64 columns that K + 1 columns need, less one
    case 0: k_ray_layer_colour<1><<<grid, block, 0, st>>>(S, N, alpha, ray_start, act_idx, M, slot, K, rgb, ldc, n_rgb, rgb_row, out); break;
    case 1: k_ray_layer_colour<2><<<grid, block, 0, st>>>(S, N, alpha, ray_start, act_idx, M, slot, K, rgb, ldc, n_rgb, rgb_row, out); break;
    case 2: k_ray_layer_colour<3><<<grid, block, 0, st>>>(S, N, alpha, ray_start, act_idx, M, slot, K, rgb, ldc, n_rgb, rgb_row, out); break;
    default: k_ray_layer_colour<4><<<grid, block, 0, st>>>(S, N, alpha, ray_start, act_idx, M, slot, K, rgb, ldc, n_rgb, rgb_row, out); break;
    }
    return clift_check_launch("clift_ray_layer_colour");
}
