// cluster.hip -- mean-shift of many seeds over one point set: the per-seed loop of sklearn's MeanShift.fit
// (sklearn/cluster/_mean_shift.py, _mean_shift_single_seed), which the reference runs on the CPU for every clustering of the
// rendered instance features (inference/render_panopli.py:196-368, extract_train_centroids.py, find_bandwidth.py).
//
// One 256-thread block per seed, the whole climb in one launch: seeds are independent, so a block that has converged simply exits
// (no grid-wide sync, no host round trip per step).  A block, not a wave, per seed because the seed counts are small (33 - 1400 on
// the MOS sweep of a 50 000-point subsample): four waves per seed keep four times as many loads in flight.  Every step the block
// streams the n points from global memory (50 000 x 3 fp32 = 600 KB: L2-resident after the first pass on an XCD).  Point i always
// goes to thread i % 256 and is added in index order; each wave folds its 64 partials with an xor butterfly (the same bits on every
// lane), and every thread adds the four wave partials from LDS in wave order.  The sum -- and so the mean -- depends only on the
// neighbour set: two seeds that reach the same set get bit-identical centres, which the exact-equality merge on the host relies on.
#include "clift_dev.h"

#define MS_MAX_D 32

template <int DM, bool EXACT>
__global__ __launch_bounds__(256) void k_meanshift(const float* __restrict__ X, int n, int ldx, int d_rt, const float* __restrict__ seeds,
                                                   int S, double bw2, double stop, int max_iter, float* __restrict__ centers,
                                                   int* __restrict__ counts, int* __restrict__ iters) {
    const int d = EXACT ? DM : d_rt;
    __shared__ double part[2][4][DM + 1];                    // per-wave partials (sums, count), double-buffered by step parity
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seed = blockIdx.x;
    float m[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) m[k] = k < d ? seeds[(long)seed * d + k] : 0.f;
    int it = 0, cnt = 0;
    while (true) {
        // neighbours: squared distance summed in fp64 in dimension order (sklearn's BallTree), <= bandwidth^2
        double acc[DM];
#pragma unroll
        for (int k = 0; k < DM; ++k) acc[k] = 0.0;
        int c = 0;
        for (int i = tid; i < n; i += 256) {
            const float* p = X + (long)i * ldx;
            float x[DM];
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < DM; ++k) {
                if (k < d) {
                    x[k] = p[k];
                    const double t = (double)x[k] - (double)m[k];
                    d2 += t * t;
                }
            }
            if (d2 <= bw2) {
                ++c;
#pragma unroll
                for (int k = 0; k < DM; ++k)
                    if (k < d) acc[k] += (double)x[k];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            c += __shfl_xor(c, off);
#pragma unroll
            for (int k = 0; k < DM; ++k)
                if (k < d) acc[k] += __shfl_xor(acc[k], off);
        }
        double (*pp)[DM + 1] = part[it & 1];
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < DM; ++k)
                if (k < d) pp[wave][k] = acc[k];
            pp[wave][DM] = (double)c;
        }
        __syncthreads();                                     // (the other buffer is rewritten only after the next step's barrier)
        c = (int)pp[0][DM] + (int)pp[1][DM] + (int)pp[2][DM] + (int)pp[3][DM];
#pragma unroll
        for (int k = 0; k < DM; ++k)
            if (k < d) acc[k] = ((pp[0][k] + pp[1][k]) + pp[2][k]) + pp[3][k];
        cnt = c;
        if (c == 0) break;                                   // empty neighbourhood: count 0, the seed is dropped on the host
        // new mean = neighbour mean rounded to fp32; stop on the fp32 norm of the step or at max_iter
        float s2 = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            if (k < d) {
                const float nm = (float)(acc[k] / (double)c);
                const float t = nm - m[k];
                s2 += t * t;
                m[k] = nm;
            }
        }
        if ((double)sqrtf(s2) <= stop || it == max_iter) break;
        ++it;
    }
#pragma unroll
    for (int k = 0; k < DM; ++k)
        if (k < d && tid == k) centers[(long)seed * d + k] = m[k];
    if (tid == 0) {
        counts[seed] = cnt;
        iters[seed] = it;
    }
}

template <int DM, bool EXACT>
static void launch_meanshift(const float* X, int n, int ldx, int d, const float* seeds, int S, double bw2, double stop, int max_iter,
                             float* centers, int* counts, int* iters, hipStream_t s) {
    k_meanshift<DM, EXACT><<<S, 256, 0, s>>>(X, n, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters);
}

extern "C" int clift_meanshift(const float* X, long n, int ldx, int d, const float* seeds, int S, double bandwidth, int max_iter,
                               float* centers, int* counts, int* iters, clift_stream_t s) {
    CLIFT_REQUIRE(d >= 1, "clift_meanshift: need d >= 1 (got %d)", d);
    CLIFT_REQUIRE(d <= MS_MAX_D, "clift_meanshift: d = %d exceeds the supported feature width %d", d, MS_MAX_D);
    CLIFT_REQUIRE(ldx >= d, "clift_meanshift: row stride ldx = %d < d = %d", ldx, d);
    CLIFT_REQUIRE(n >= 1 && n <= 0x7fffffffL, "clift_meanshift: need 1 <= n < 2^31 (got %ld)", n);
    CLIFT_REQUIRE(S >= 0, "clift_meanshift: need S >= 0 (got %d)", S);
    CLIFT_REQUIRE(bandwidth > 0.0 && bandwidth < INFINITY, "clift_meanshift: bandwidth must be positive and finite (got %g)", bandwidth);
    CLIFT_REQUIRE(max_iter >= 0, "clift_meanshift: need max_iter >= 0 (got %d)", max_iter);
    CLIFT_REQUIRE(X != nullptr && seeds != nullptr && centers != nullptr && counts != nullptr && iters != nullptr,
                  "clift_meanshift: NULL buffer");
    if (S == 0) return 0;
    const double bw2 = bandwidth * bandwidth, stop = 1e-3 * bandwidth;
    const hipStream_t st = as_stream(s);
    const int ni = (int)n;
    if (d == 3)       launch_meanshift<3, true>(X, ni, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters, st);
    else if (d <= 4)  launch_meanshift<4, false>(X, ni, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters, st);
    else if (d <= 8)  launch_meanshift<8, false>(X, ni, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters, st);
    else if (d <= 16) launch_meanshift<16, false>(X, ni, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters, st);
    else              launch_meanshift<32, false>(X, ni, ldx, d, seeds, S, bw2, stop, max_iter, centers, counts, iters, st);
    return clift_check_launch("clift_meanshift");
}
