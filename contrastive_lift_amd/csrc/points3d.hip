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
//
// k_segment_mvee: the minimum-volume enclosing ellipsoid of every instance's kept rows by Khachiyan's algorithm (getMinVolEllipse :135-189,
// the reference's DEFAULT get_tight_bbox method) with O(N) work and memory per iteration instead of the reference's N x N products.  One
// 256-thread block per instance runs the whole loop: per iteration one pass over the rows (M_i = |L^-1 q_i|^2 from the 4 x 4 Cholesky factor,
// the argmax as a wave butterfly + four partials, lowest row on equal values) and a few hundred scalar flops on thread 0 (step, err, the
// rank-1 update of V, its factor), two barriers.  Thread 0 alone decides whether the loop goes on and says so in ONE LDS word that every
// thread reads after the second barrier.  The sums (mean, first V, centre and second moment) go through p3_block_sum; no atomics anywhere.
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

// ----------------------------------------------------------------------------- minimum-volume enclosing ellipsoid (Khachiyan)
// Choices (clift.h, ABI 25): the rows are centred on the mean of the instance's kept rows before q = (p - o, 1) is formed (M is affine
// invariant; V stays well conditioned); V is updated by the rank-1 form (1 - step) V + step q_j q_j^T; err is the closed form
// |step| sqrt(|u|^2 - 2 u_j + 1) with |u|^2 carried along; M_i = |L^-1 q_i|^2 with V = L L^T.  The scaling u <- (1 - step) u of iteration k is
// applied to a row when iteration k + 1 visits it (or by the closing pass), so an iteration reads and writes every kept row once.
#define MVEE_PIVOT_REL 1e-12
#define MVEE_OUT 14

// V = L L^T (lower), Li = L^-1.  false when a pivot is not above MVEE_PIVOT_REL of its diagonal entry or not finite (NaN compares false).
__device__ __forceinline__ bool mvee_factor(const double (&V)[4][4], double (&Li)[4][4]) {
    double L[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = V[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > MVEE_PIVOT_REL * V[j][j] && d < INFINITY)) return false;
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double v = V[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        Li[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) v = v + L[i][k] * Li[k][j];
            Li[i][j] = -v / L[i][i];
        }
    }
    return true;
}

enum { MVEE_GO = 0, MVEE_CONVERGED = 1, MVEE_MAX_ITER = 2, MVEE_DEGENERATE = 3 };

__global__ __launch_bounds__(P3_THREADS) void k_segment_mvee(const float* __restrict__ pts, int n, const long* __restrict__ seg,
                                                             const unsigned char* __restrict__ keep, double tolerance, int max_iter,
                                                             double* u, double* __restrict__ out) {
    __shared__ double s_sum[10];         // results of p3_block_sum
    __shared__ double s_li[10];          // L^-1, lower triangle row by row
    __shared__ double s_step;            // the step whose scaling of u is still to be applied (0: none)
    __shared__ int s_j;                  // its row
    __shared__ int s_state;              // THE word that ends the loop: MVEE_GO or the reason it stopped, written by thread 0 only
    __shared__ double s_m[4];
    __shared__ int s_i[4];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = p3_clamp_row(seg[g], n), hi = p3_clamp_row(seg[g + 1], n);
    double* o_g = out + (long)g * MVEE_OUT;

    // kept rows and their mean
    double a4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = lo + tid; i < hi; i += P3_THREADS) {
        if (keep != nullptr && keep[i] == 0) continue;
        const float* p = pts + (long)i * 3;
        a4[0] = __dadd_rn(a4[0], 1.0);
        a4[1] = __dadd_rn(a4[1], (double)p[0]);
        a4[2] = __dadd_rn(a4[2], (double)p[1]);
        a4[3] = __dadd_rn(a4[3], (double)p[2]);
    }
    p3_block_sum<4>(a4, s_sum);
    __syncthreads();
    const double m = s_sum[0];
    const double inv_m = 1.0 / m;
    const double ox = s_sum[1] * inv_m, oy = s_sum[2] * inv_m, oz = s_sum[3] * inv_m;
    __syncthreads();                                             // s_sum is written again below

    // u = 1 / m on the kept rows, 0 elsewhere; V = sum u q q^T
    double a9[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a9[k] = 0.0;
    const bool small = !(m >= 4.0);
    for (int i = lo + tid; i < hi; i += P3_THREADS) {
        const bool kept = keep == nullptr || keep[i] != 0;
        u[i] = kept && !small ? inv_m : 0.0;
        if (!kept || small) continue;
        const float* p = pts + (long)i * 3;
        const double x = __dsub_rn((double)p[0], ox), y = __dsub_rn((double)p[1], oy), z = __dsub_rn((double)p[2], oz);
        a9[0] = __dadd_rn(a9[0], x);
        a9[1] = __dadd_rn(a9[1], y);
        a9[2] = __dadd_rn(a9[2], z);
        a9[3] = __dadd_rn(a9[3], __dmul_rn(x, x));
        a9[4] = __dadd_rn(a9[4], __dmul_rn(x, y));
        a9[5] = __dadd_rn(a9[5], __dmul_rn(x, z));
        a9[6] = __dadd_rn(a9[6], __dmul_rn(y, y));
        a9[7] = __dadd_rn(a9[7], __dmul_rn(y, z));
        a9[8] = __dadd_rn(a9[8], __dmul_rn(z, z));
    }
    if (small) {                                                 // fewer than d + 1 points (m is block-uniform: read from LDS)
        if (tid < MVEE_OUT) o_g[tid] = tid == 0 ? m : (tid == 3 ? 2.0 : 0.0);
        return;
    }
    p3_block_sum<9>(a9, s_sum);
    __syncthreads();

    // thread 0's state of the iteration
    double V[4][4], Li[4][4], nsq = inv_m, err = 0.0;            // |u|^2 = m (1 / m)^2
    int iters = 0;
    if (tid == 0) {
        V[0][0] = s_sum[3] * inv_m; V[1][0] = s_sum[4] * inv_m; V[2][0] = s_sum[5] * inv_m; V[3][0] = s_sum[0] * inv_m;
        V[1][1] = s_sum[6] * inv_m; V[2][1] = s_sum[7] * inv_m; V[3][1] = s_sum[1] * inv_m;
        V[2][2] = s_sum[8] * inv_m; V[3][2] = s_sum[2] * inv_m;
        V[3][3] = 1.0;
        const bool ok = mvee_factor(V, Li);
        s_state = ok ? MVEE_GO : MVEE_DEGENERATE;
        s_step = 0.0;
        s_j = -1;
        if (ok) {
            int k = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) s_li[k++] = Li[r][c];
        }
    }
    __syncthreads();

    int state = s_state;
    while (state == MVEE_GO) {                                   // (thread 0 leaves MVEE_GO at iters == max_iter at the latest)
        const double step = s_step, keep1 = 1.0 - step;
        const int jp = s_j;
        const double l00 = s_li[0], l10 = s_li[1], l11 = s_li[2], l20 = s_li[3], l21 = s_li[4], l22 = s_li[5], l30 = s_li[6], l31 = s_li[7],
                     l32 = s_li[8], l33 = s_li[9];
        double bm = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = lo + tid; i < hi; i += P3_THREADS) {
            if (keep != nullptr && keep[i] == 0) continue;
            if (step != 0.0) {                                   // the previous iteration's u <- (1 - step) u, u_j += step
                double ui = __dmul_rn(keep1, u[i]);
                if (i == jp) ui = __dadd_rn(ui, step);
                u[i] = ui;
            }
            const float* p = pts + (long)i * 3;
            const double x = __dsub_rn((double)p[0], ox), y = __dsub_rn((double)p[1], oy), z = __dsub_rn((double)p[2], oz);
            const double y0 = __dmul_rn(l00, x);
            const double y1 = __dadd_rn(__dmul_rn(l10, x), __dmul_rn(l11, y));
            const double y2 = __dadd_rn(__dadd_rn(__dmul_rn(l20, x), __dmul_rn(l21, y)), __dmul_rn(l22, z));
            const double y3 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(l30, x), __dmul_rn(l31, y)), __dmul_rn(l32, z)), l33);
            const double mi = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(y0, y0), __dmul_rn(y1, y1)), __dmul_rn(y2, y2)), __dmul_rn(y3, y3));
            if (mi > bm) { bm = mi; bi = i; }                    // rows ascend on a thread: the first of equal values stays
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double om = __shfl_xor(bm, off);
            const int oi = __shfl_xor(bi, off);
            if (om > bm || (om == bm && oi < bi)) { bm = om; bi = oi; }
        }
        if (lane == 0) { s_m[wave] = bm; s_i[wave] = bi; }
        __syncthreads();                                         // partials written; every u row of this pass written
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (s_m[w] > bm || (s_m[w] == bm && s_i[w] < bi)) { bm = s_m[w]; bi = s_i[w]; }
            int next = MVEE_GO;
            double st = 0.0;
            if (!(bm > -INFINITY && bm < INFINITY) || bi < lo || bi >= hi) {
                next = MVEE_DEGENERATE;
            } else {
                st = (bm - 4.0) / (4.0 * (bm - 1.0));
                const double uj = u[bi];
                err = fabs(st) * sqrt(nsq - 2.0 * uj + 1.0);
                ++iters;
                if (!(err < INFINITY && err > -INFINITY)) {
                    next = MVEE_DEGENERATE;
                    st = 0.0;
                } else {
                    const double k1 = 1.0 - st;
                    nsq = (k1 * k1) * nsq + 2.0 * (st * k1) * uj + st * st;
                    if (!(err > tolerance)) next = MVEE_CONVERGED;
                    else if (iters >= max_iter) next = MVEE_MAX_ITER;
                    else {
                        const float* p = pts + (long)bi * 3;
                        const double q[4] = {__dsub_rn((double)p[0], ox), __dsub_rn((double)p[1], oy), __dsub_rn((double)p[2], oz), 1.0};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int c = 0; c <= r; ++c) V[r][c] = k1 * V[r][c] + st * (q[r] * q[c]);
                        if (mvee_factor(V, Li)) {
                            int k = 0;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
#pragma unroll
                                for (int c = 0; c <= r; ++c) s_li[k++] = Li[r][c];
                        } else {
                            next = MVEE_DEGENERATE;
                        }
                    }
                }
            }
            s_step = st;
            s_j = bi;
            s_state = next;
        }
        __syncthreads();                                         // the decision, read by every thread from the same word
        state = s_state;
    }

    // closing pass: the last step's scaling, then c = sum u p and the central second moment; or zeros for a degenerate instance
    const bool bad = state == MVEE_DEGENERATE;
    const double step = s_step, keep1 = 1.0 - step;
    const int jp = s_j;
#pragma unroll
    for (int k = 0; k < 9; ++k) a9[k] = 0.0;
    for (int i = lo + tid; i < hi; i += P3_THREADS) {
        if (keep != nullptr && keep[i] == 0) continue;
        if (bad) { u[i] = 0.0; continue; }
        double ui = u[i];
        if (step != 0.0) {
            ui = __dmul_rn(keep1, ui);
            if (i == jp) ui = __dadd_rn(ui, step);
            u[i] = ui;
        }
        const float* p = pts + (long)i * 3;
        const double x = __dsub_rn((double)p[0], ox), y = __dsub_rn((double)p[1], oy), z = __dsub_rn((double)p[2], oz);
        const double ux = __dmul_rn(ui, x), uy = __dmul_rn(ui, y), uz = __dmul_rn(ui, z);
        a9[0] = __dadd_rn(a9[0], ux);
        a9[1] = __dadd_rn(a9[1], uy);
        a9[2] = __dadd_rn(a9[2], uz);
        a9[3] = __dadd_rn(a9[3], __dmul_rn(ux, x));
        a9[4] = __dadd_rn(a9[4], __dmul_rn(ux, y));
        a9[5] = __dadd_rn(a9[5], __dmul_rn(ux, z));
        a9[6] = __dadd_rn(a9[6], __dmul_rn(uy, y));
        a9[7] = __dadd_rn(a9[7], __dmul_rn(uy, z));
        a9[8] = __dadd_rn(a9[8], __dmul_rn(uz, z));
    }
    p3_block_sum<9>(a9, s_sum);
    __syncthreads();
    if (tid == 0) {
        o_g[0] = m;
        o_g[1] = (double)iters;
        o_g[2] = bad ? 0.0 : err;
        o_g[3] = bad ? 2.0 : (state == MVEE_MAX_ITER ? 1.0 : 0.0);
        const double cx = s_sum[0], cy = s_sum[1], cz = s_sum[2];        // centre relative to the offset o
        o_g[4] = bad ? 0.0 : ox + cx;
        o_g[5] = bad ? 0.0 : oy + cy;
        o_g[6] = bad ? 0.0 : oz + cz;
        o_g[7] = bad ? 0.0 : s_sum[3] - cx * cx;
        o_g[8] = bad ? 0.0 : s_sum[4] - cx * cy;
        o_g[9] = bad ? 0.0 : s_sum[5] - cx * cz;
        o_g[10] = bad ? 0.0 : s_sum[6] - cy * cy;
        o_g[11] = bad ? 0.0 : s_sum[7] - cy * cz;
        o_g[12] = bad ? 0.0 : s_sum[8] - cz * cz;
        o_g[13] = 0.0;
    }
}

extern "C" int clift_segment_mvee(const float* pts, long n, const long* seg, int G, const unsigned char* keep, double tolerance, int max_iter,
                                  double* u, double* out, clift_stream_t s) {
    CLIFT_REQUIRE(n >= 0 && n <= 0x7fffffffL - P3_THREADS, "clift_segment_mvee: need 0 <= n < 2^31 - %d (got %ld)", P3_THREADS, n);
    CLIFT_REQUIRE(G >= 0, "clift_segment_mvee: need G >= 0 (got %d)", G);
    CLIFT_REQUIRE(max_iter >= 1 && max_iter <= 1000000, "clift_segment_mvee: need 1 <= max_iter <= 1000000 (got %d)", max_iter);
    CLIFT_REQUIRE(tolerance > 0.0, "clift_segment_mvee: need tolerance > 0 (got %g)", tolerance);
    if (G == 0) return 0;
    CLIFT_REQUIRE(seg != nullptr && out != nullptr && ((pts != nullptr && u != nullptr) || n == 0), "clift_segment_mvee: NULL buffer");
    k_segment_mvee<<<G, P3_THREADS, 0, as_stream(s)>>>(pts, (int)n, seg, keep, tolerance, max_iter, u, out);
    return clift_check_launch("clift_segment_mvee");
}
