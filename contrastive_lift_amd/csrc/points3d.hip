// points3d.hip -- the per-instance geometry of the 3-D lift: what the reference's inference/visualize_bboxes.py does one instance at a time on
// the host (filter_pointcloud :52-74 -- KDTree.query(points, k = 10), a percentile, a 3-sigma cut -- and get_tight_bbox :78-131 -- mean, PCA,
// extent), here for ALL instances of a scene per launch.  Points arrive sorted by instance: instance g owns rows seg[g] .. seg[g+1].
//
// k_knn_kth: brute force inside an instance.  One query per lane with its KT >= k smallest squared distances sorted in registers (KT doubles:
// 32 VGPRs at KT = 16); candidates staged in LDS as fp64 in tiles of 1024 (32 KB: five blocks per CU) and read at a wave-uniform address
// (a broadcast).  Blocks are cut from the ROW axis, 256 consecutive rows each, not from the instances: a lane finds its instance by a
// binary search in seg, the block stages the union of its lanes' instances and every wave walks only the part of a tile that its own lanes'
// instances overlap.  So a 50 000-point instance is 196 blocks of equal work, and four hundred 300-point instances are ~470 blocks that
// each scan two or three neighbours' rows in vain at worst -- no work list, nothing to build on either side, and the machine is filled alike.
// The distance is pinned (see clift.h): fp64, every product and sum rounded separately; the k smallest of a multiset of exactly reproducible
// numbers do not depend on the tile order, so the result is a function of the instance alone.
//
// k_segment_moments / k_segment_extent: one 256-thread block per instance, row lo + t + 256 j on thread t in order of j, an xor butterfly
// inside the wave and the four wave partials added in wave order: a fixed split, the same bits on every run (no atomics).
#include "clift_dev.h"

#define P3_TILE 1024
#define P3_THREADS 256

__device__ __forceinline__ int p3_clamp_row(long v, int n) { return (int)(v < 0 ? 0 : (v > (long)n ? (long)n : v)); }

struct __align__(16) P3Cand {
    double x, y, z, pad;
};

template <int KT>
__global__ __launch_bounds__(P3_THREADS) void k_knn_kth(const float* __restrict__ pts, int n, const long* __restrict__ seg, int G, int k,
                                                        double* __restrict__ out) {
    __shared__ P3Cand cand[P3_TILE];
    __shared__ int brange[2];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * P3_THREADS + tid;
    const bool live = row < (long)n;
    const int i = live ? (int)row : n - 1;                       // (n >= 1: the host returns before the launch otherwise)
    // instance of row i: the last g with seg[g] <= i (empty instances in between are skipped by the upper bound); none outside [seg[0], seg[G])
    int a = 0, b = G + 1;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (seg[m] <= (long)i) a = m + 1; else b = m;
    }
    int lo = 0, hi = 0;
    if (a >= 1 && a <= G) {
        lo = p3_clamp_row(seg[a - 1], n);
        hi = p3_clamp_row(seg[a], n);
    }
    const bool has = hi > lo;
    if (tid == 0) { brange[0] = 0x7fffffff; brange[1] = 0; }
    __syncthreads();
    if (has) { atomicMin(&brange[0], lo); atomicMax(&brange[1], hi); }
    int wlo = has ? lo : 0x7fffffff, whi = has ? hi : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, off));
        whi = max(whi, __shfl_xor(whi, off));
    }
    wlo = __builtin_amdgcn_readfirstlane(wlo);
    whi = __builtin_amdgcn_readfirstlane(whi);
    __syncthreads();
    const int blo = brange[0], bhi = brange[1];

    const double qx = (double)pts[(long)i * 3 + 0], qy = (double)pts[(long)i * 3 + 1], qz = (double)pts[(long)i * 3 + 2];
    double best[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) best[j] = INFINITY;

    for (int t0 = blo; t0 < bhi; t0 += P3_TILE) {
        const int cnt = min(P3_TILE, bhi - t0);
        __syncthreads();                                         // the previous tile has been read by every wave
        for (int c = tid; c < cnt; c += P3_THREADS) {
            const float* p = pts + (long)(t0 + c) * 3;
            P3Cand v;
            v.x = (double)p[0]; v.y = (double)p[1]; v.z = (double)p[2]; v.pad = 0.0;
            cand[c] = v;
        }
        __syncthreads();
        const int c0 = max(wlo, t0) - t0, c1 = min(whi, t0 + cnt) - t0;       // wave-uniform; empty when this wave's instances miss the tile
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            const P3Cand v = cand[c];
            const double dx = __dsub_rn(qx, v.x), dy = __dsub_rn(qy, v.y), dz = __dsub_rn(qz, v.z);
            const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            const int cg = t0 + c;
            if (cg >= lo && cg < hi && d2 < best[KT - 1]) {
                // sorted insert, top down: slot j takes its left neighbour when the new value goes left of it
#pragma unroll
                for (int j = KT - 1; j >= 1; --j) best[j] = d2 < best[j - 1] ? best[j - 1] : (d2 < best[j] ? d2 : best[j]);
                best[0] = d2 < best[0] ? d2 : best[0];
            }
        }
    }
    double kth = INFINITY;
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j == k - 1) kth = best[j];
    if (live) out[row] = kth;
}

extern "C" int clift_knn_kth_dist(const float* pts, long n, const long* seg, int G, int k, double* d2_out, clift_stream_t s) {
    CLIFT_REQUIRE(n >= 0 && n <= 0x7fffffffL - P3_TILE, "clift_knn_kth_dist: need 0 <= n < 2^31 - %d (got %ld)", P3_TILE, n);
    CLIFT_REQUIRE(G >= 0, "clift_knn_kth_dist: need G >= 0 (got %d)", G);
    CLIFT_REQUIRE(k >= 1 && k <= 16, "clift_knn_kth_dist: need 1 <= k <= 16 (got %d)", k);
    if (n == 0) return 0;
    CLIFT_REQUIRE(pts != nullptr && seg != nullptr && d2_out != nullptr, "clift_knn_kth_dist: NULL buffer");
    const hipStream_t st = as_stream(s);
    const int ni = (int)n, blocks = cdiv(n, P3_THREADS);
    if (k <= 4)       k_knn_kth<4><<<blocks, P3_THREADS, 0, st>>>(pts, ni, seg, G, k, d2_out);
    else if (k <= 8)  k_knn_kth<8><<<blocks, P3_THREADS, 0, st>>>(pts, ni, seg, G, k, d2_out);
    else if (k <= 12) k_knn_kth<12><<<blocks, P3_THREADS, 0, st>>>(pts, ni, seg, G, k, d2_out);
    else              k_knn_kth<16><<<blocks, P3_THREADS, 0, st>>>(pts, ni, seg, G, k, d2_out);
    return clift_check_launch("clift_knn_kth_dist");
}

// ----------------------------------------------------------------------------- per-instance sums
template <int NV>
__device__ __forceinline__ void p3_block_sum(double (&acc)[NV], double* __restrict__ dst) {
    __shared__ double part[4][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = __dadd_rn(acc[j], __shfl_xor(acc[j], off));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) part[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int j = threadIdx.x;
        dst[j] = __dadd_rn(__dadd_rn(__dadd_rn(part[0][j], part[1][j]), part[2][j]), part[3][j]);
    }
}

__global__ __launch_bounds__(P3_THREADS) void k_segment_moments(const float* __restrict__ pts, int n, const long* __restrict__ seg,
                                                                const unsigned char* __restrict__ keep, const double* __restrict__ centre,
                                                                double* __restrict__ out) {
    const int g = blockIdx.x;
    const int lo = p3_clamp_row(seg[g], n), hi = p3_clamp_row(seg[g + 1], n);
    const double c0 = centre ? centre[(long)g * 3 + 0] : 0.0, c1 = centre ? centre[(long)g * 3 + 1] : 0.0,
                 c2 = centre ? centre[(long)g * 3 + 2] : 0.0;
    double acc[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) acc[j] = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += P3_THREADS) {
        if (keep != nullptr && keep[i] == 0) continue;
        const float* p = pts + (long)i * 3;
        const double x = __dsub_rn((double)p[0], c0), y = __dsub_rn((double)p[1], c1), z = __dsub_rn((double)p[2], c2);
        acc[0] = __dadd_rn(acc[0], 1.0);
        acc[1] = __dadd_rn(acc[1], x);
        acc[2] = __dadd_rn(acc[2], y);
        acc[3] = __dadd_rn(acc[3], z);
        acc[4] = __dadd_rn(acc[4], __dmul_rn(x, x));
        acc[5] = __dadd_rn(acc[5], __dmul_rn(x, y));
        acc[6] = __dadd_rn(acc[6], __dmul_rn(x, z));
        acc[7] = __dadd_rn(acc[7], __dmul_rn(y, y));
        acc[8] = __dadd_rn(acc[8], __dmul_rn(y, z));
        acc[9] = __dadd_rn(acc[9], __dmul_rn(z, z));
    }
    p3_block_sum<10>(acc, out + (long)g * 10);
}

extern "C" int clift_segment_moments(const float* pts, long n, const long* seg, int G, const unsigned char* keep, const double* centre,
                                     double* out, clift_stream_t s) {
    CLIFT_REQUIRE(n >= 0 && n <= 0x7fffffffL - P3_THREADS, "clift_segment_moments: need 0 <= n < 2^31 - %d (got %ld)", P3_THREADS, n);
    CLIFT_REQUIRE(G >= 0, "clift_segment_moments: need G >= 0 (got %d)", G);
    if (G == 0) return 0;
    CLIFT_REQUIRE(seg != nullptr && out != nullptr && (pts != nullptr || n == 0), "clift_segment_moments: NULL buffer");
    k_segment_moments<<<G, P3_THREADS, 0, as_stream(s)>>>(pts, (int)n, seg, keep, centre, out);
    return clift_check_launch("clift_segment_moments");
}

__global__ __launch_bounds__(P3_THREADS) void k_segment_extent(const float* __restrict__ pts, int n, const long* __restrict__ seg,
                                                               const unsigned char* __restrict__ keep, const double* __restrict__ frame,
                                                               double* __restrict__ out) {
    __shared__ double part[4][6];
    const int g = blockIdx.x;
    const int lo = p3_clamp_row(seg[g], n), hi = p3_clamp_row(seg[g + 1], n);
    double A[9], ctr[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) A[j] = frame[(long)g * 12 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) ctr[j] = frame[(long)g * 12 + 9 + j];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lo + (int)threadIdx.x; i < hi; i += P3_THREADS) {
        if (keep != nullptr && keep[i] == 0) continue;
        const float* p = pts + (long)i * 3;
        const double x = __dsub_rn((double)p[0], ctr[0]), y = __dsub_rn((double)p[1], ctr[1]), z = __dsub_rn((double)p[2], ctr[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double v = __dadd_rn(__dadd_rn(__dmul_rn(A[3 * r], x), __dmul_rn(A[3 * r + 1], y)), __dmul_rn(A[3 * r + 2], z));
            mn[r] = fmin(mn[r], v);
            mx[r] = fmax(mx[r], v);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            mn[r] = fmin(mn[r], __shfl_xor(mn[r], off));
            mx[r] = fmax(mx[r], __shfl_xor(mx[r], off));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { part[wave][r] = mn[r]; part[wave][3 + r] = mx[r]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int j = threadIdx.x;
        const double v = j < 3 ? fmin(fmin(part[0][j], part[1][j]), fmin(part[2][j], part[3][j]))
                               : fmax(fmax(part[0][j], part[1][j]), fmax(part[2][j], part[3][j]));
        out[(long)g * 6 + j] = v;
    }
}

extern "C" int clift_segment_extent(const float* pts, long n, const long* seg, int G, const unsigned char* keep, const double* frame,
                                    double* out, clift_stream_t s) {
    CLIFT_REQUIRE(n >= 0 && n <= 0x7fffffffL - P3_THREADS, "clift_segment_extent: need 0 <= n < 2^31 - %d (got %ld)", P3_THREADS, n);
    CLIFT_REQUIRE(G >= 0, "clift_segment_extent: need G >= 0 (got %d)", G);
    if (G == 0) return 0;
    CLIFT_REQUIRE(seg != nullptr && frame != nullptr && out != nullptr && (pts != nullptr || n == 0), "clift_segment_extent: NULL buffer");
    k_segment_extent<<<G, P3_THREADS, 0, as_stream(s)>>>(pts, (int)n, seg, keep, frame, out);
    return clift_check_launch("clift_segment_extent");
}
