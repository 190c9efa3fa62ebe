// emst.hip -- Euclidean minimum spanning tree of one point set by brute-force Boruvka: the tree under HDBSCAN(min_samples = 1), which the
// reference runs on the CPU for every --use_dbscan clustering of the rendered instance features (inference/render_panopli.py:236-241,
// extract_train_centroids.py, find_bandwidth.py).  With min_samples = 1 every core distance is 0, so the mutual-reachability graph is the
// plain Euclidean graph; the condensed-tree pass over the n - 1 edges stays on the host (contrastive_lift_amd/hdbscan.py).
//
// Edges are ordered STRICTLY by key = (d2, min(i, j), max(i, j)), d2 the fp64 squared distance.  The key belongs to the edge, not to the
// component that looks at it, so the only cycle a round of "every component takes its smallest outgoing edge" can close is two components
// taking the same edge -- duplicate points and lattices included.  A round is five launches on the stream, no grid-wide barrier:
//   k_emst_nearest  for every point the smallest-key edge to a point of another component, inside one slice of the other points.  A workgroup
//                   owns a tile of points (R per thread, in registers as fp64) and streams its slice through LDS, 256 points at a time; every
//                   lane reads the same LDS word (a broadcast), so with R = 4 the fp64 pipe, not the LDS, bounds the loop.  For a fixed i the
//                   key order over j is the order of j, so "first strictly smaller d2 while j ascends" is the smallest key.  The (point, slice)
//                   result is stored and its d2 goes into the component's minimum by an integer atomicMin on the bit pattern (a non-negative
//                   finite double orders like its bits).
//   k_emst_pair     among the stored results that reached the component's minimum d2: integer atomicMin on min * n + max.
//   k_emst_link     every root hooks to the root its edge leads to; of a mutual pair the smaller root stays.  A root that hooks writes the edge
//                   into the slot of its own (dying) index -- an index stops being a root once, so slots never collide.
//   k_emst_relabel  every point chases the root pointers to its new root (at most n steps, else the fault flag) and clears the minima.
// The fixed maximum of ceil(log2 n) rounds is launched without a host sync; cnt[k] holds the component count at the start of round k and every
// kernel of round k returns at once when it is 1.  k_emst_compact then packs the n - 1 used slots in ascending slot order, so two runs give
// the same bits, edge order included.  All atomics are integer min / add: order-independent.
#include "clift_dev.h"

#define EMST_MAX_D 32
#define EMST_TJ 256                                              // points of the slice held in LDS at a time
#define EMST_SPLITS CLIFT_EMST_SPLITS                            // upper bound of slices per point tile (sizes the stored results)
#define EMST_NONE 0xffffffffffffffffull
#define EMST_FAULT_CHASE 1                                       // info[2] bits
#define EMST_FAULT_NONFINITE 2
#define EMST_FAULT_DECODE 4

struct EmstWork {
    int* cnt;                     // [32] component count at the start of round k
    int* fault;
    unsigned long long* best_d2;  // [n] per root: bits of the smallest outgoing d2
    unsigned long long* best_pair;// [n] per root: min * n + max of the smallest-key outgoing edge
    double* slot_w;               // [n] edge written by the root that died at this index
    double* part_d2;              // [SPLITS][n] per (slice, point): d2 of the nearest outside point of the slice
    int* comp;                    // [n] root of the point's component
    int* parent;                  // [n] root pointers (meaningful at indices that are or were roots this round)
    int* slot_a;
    int* slot_b;
    int* used;                    // [n] 1 = the slot holds an edge
    int* part_j;                  // [SPLITS][n] the nearest outside point of the slice, -1 = none
};

static EmstWork emst_carve(void* work, long n) {
    EmstWork w;
    char* p = (char*)work;
    w.cnt = (int*)p;
    w.fault = (int*)(p + 128);
    p += 256;
    w.best_d2 = (unsigned long long*)p;   p += 8 * n;
    w.best_pair = (unsigned long long*)p; p += 8 * n;
    w.slot_w = (double*)p;                p += 8 * n;
    w.part_d2 = (double*)p;               p += 8 * n * EMST_SPLITS;
    w.comp = (int*)p;                     p += 4 * n;
    w.parent = (int*)p;                   p += 4 * n;
    w.slot_a = (int*)p;                   p += 4 * n;
    w.slot_b = (int*)p;                   p += 4 * n;
    w.used = (int*)p;                     p += 4 * n;
    w.part_j = (int*)p;
    return w;
}

__global__ __launch_bounds__(256) void k_emst_init(EmstWork w, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 32) w.cnt[i] = (i == 0) ? n : 0;
    if (i == 0) *w.fault = 0;
    if (i >= n) return;
    w.comp[i] = i;
    w.parent[i] = i;
    w.used[i] = 0;
    w.best_d2[i] = EMST_NONE;
    w.best_pair[i] = EMST_NONE;
}

// grid (point tiles, slices).  Slice s covers points [s * slice, min(n, (s + 1) * slice)), slice a multiple of EMST_TJ.
template <int DM, bool EXACT, int R>
__global__ __launch_bounds__(256) void k_emst_nearest(const float* __restrict__ X, int n, int ldx, int d_rt, EmstWork w, int round, int slice) {
    const int d = EXACT ? DM : d_rt;
    const int c0 = w.cnt[round];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) w.cnt[round + 1] = c0;      // k_emst_link of this round counts it down
    if (c0 <= 1) return;
    __shared__ float xs[EMST_TJ][DM];
    __shared__ int cs[EMST_TJ];
    const int tid = threadIdx.x;
    double xi[R][DM], best[R];
    int ci[R], bj[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = (blockIdx.x * R + r) * 256 + tid;
        best[r] = INFINITY;
        bj[r] = -1;
        ci[r] = i < n ? w.comp[i] : -1;
#pragma unroll
        for (int k = 0; k < DM; ++k) xi[r][k] = (i < n && k < d) ? (double)X[(long)i * ldx + k] : 0.0;
    }
    const int j0 = blockIdx.y * slice, j1 = min(n, j0 + slice);
    for (int jb = j0; jb < j1; jb += EMST_TJ) {                   // (j0, j1, slice are block-uniform: every thread reaches both barriers)
        __syncthreads();
        {
            const int j = jb + tid;
            const bool in = j < j1;
#pragma unroll
            for (int k = 0; k < DM; ++k) xs[tid][k] = (in && k < d) ? X[(long)j * ldx + k] : (in ? 0.f : NAN);      // a row past the slice never wins
            cs[tid] = in ? w.comp[j] : -1;
        }
        __syncthreads();
        const int cnt = min(EMST_TJ, j1 - jb);
        for (int t = 0; t < cnt; ++t) {
            double xj[DM];
#pragma unroll
            for (int k = 0; k < DM; ++k) xj[k] = (double)xs[t][k];
            const int cj = cs[t];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double d2 = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k) {
                    if (k < d) {
                        const double df = xi[r][k] - xj[k];
                        d2 += df * df;
                    }
                }
                if (cj != ci[r] && d2 < best[r]) {                // strict: the first (lowest) j keeps a tie; NaN and inf never pass
                    best[r] = d2;
                    bj[r] = jb + t;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = (blockIdx.x * R + r) * 256 + tid;
        if (i >= n) continue;
        const long o = (long)blockIdx.y * n + i;
        w.part_j[o] = bj[r];
        w.part_d2[o] = best[r];
        if (bj[r] >= 0) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(best[r]);
            unsigned long long* p = w.best_d2 + ci[r];
            if (b < *(volatile unsigned long long*)p) atomicMin(p, b);      // (the value only falls: a stale read costs one atomic, never a miss)
        }
    }
}

__global__ __launch_bounds__(256) void k_emst_pair(EmstWork w, int n, int round, int splits) {
    if (w.cnt[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int root = w.comp[i];
    const unsigned long long m = w.best_d2[root];
    unsigned long long key = EMST_NONE;
    bool any = false;
    for (int s = 0; s < splits; ++s) {
        const long o = (long)s * n + i;
        const int j = w.part_j[o];
        if (j < 0) continue;
        any = true;
        if ((unsigned long long)__double_as_longlong(w.part_d2[o]) != m) continue;
        const unsigned long long lo = (unsigned long long)min(i, j), hi = (unsigned long long)max(i, j);
        key = min(key, lo * (unsigned long long)n + hi);
    }
    if (!any) atomicOr(w.fault, EMST_FAULT_NONFINITE);            // other components exist, yet no finite distance to any of their points
    if (key != EMST_NONE) {
        unsigned long long* p = w.best_pair + root;
        if (key < *(volatile unsigned long long*)p) atomicMin(p, key);
    }
}

__global__ __launch_bounds__(256) void k_emst_link(EmstWork w, int n, int round) {
    if (w.cnt[round] <= 1) return;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n || w.comp[r] != r) return;
    const unsigned long long pair = w.best_pair[r];
    int to = r;
    if (pair != EMST_NONE) {
        const unsigned long long lo = pair / (unsigned long long)n, hi = pair % (unsigned long long)n;
        if (lo >= (unsigned long long)n) {
            atomicOr(w.fault, EMST_FAULT_DECODE);
        } else {
            const int other = w.comp[(int)lo] == r ? (int)hi : (int)lo;
            const int t = w.comp[other];
            const bool mutual = w.best_pair[t] == pair;
            if (t != r && !(mutual && r < t)) {
                to = t;
                w.slot_a[r] = (int)lo;
                w.slot_b[r] = (int)hi;
                w.slot_w[r] = sqrt(__longlong_as_double((long long)w.best_d2[r]));
                w.used[r] = 1;
                atomicSub(w.cnt + round + 1, 1);
            }
        }
    }
    w.parent[r] = to;
}

__global__ __launch_bounds__(256) void k_emst_relabel(EmstWork w, int n, int round) {
    if (w.cnt[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int c = w.comp[i], steps = 0;
    while (steps < n) {
        const int p = w.parent[c];
        if (p == c) break;
        c = p;
        ++steps;
    }
    if (w.parent[c] != c) atomicOr(w.fault, EMST_FAULT_CHASE);
    w.comp[i] = c;                                                // (read by no other thread of this launch)
    w.best_d2[i] = EMST_NONE;
    w.best_pair[i] = EMST_NONE;
}

// one workgroup: thread t owns slots [t * per, (t + 1) * per); exclusive scan of the per-thread counts in LDS
__global__ __launch_bounds__(1024) void k_emst_compact(EmstWork w, int n, int max_rounds, int* __restrict__ edge_a, int* __restrict__ edge_b,
                                                       double* __restrict__ edge_w, int* __restrict__ info) {
    __shared__ int scan[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += w.used[i] != 0;
    scan[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int total = scan[1023];
    int pos = scan[tid] - c;
    for (int i = lo; i < hi; ++i) {
        if (w.used[i] != 0 && pos < n - 1) {
            edge_a[pos] = w.slot_a[i];
            edge_b[pos] = w.slot_b[i];
            edge_w[pos] = w.slot_w[i];
            ++pos;
        }
    }
    for (int e = total + tid; e < n - 1; e += 1024) {             // only when the tree is incomplete (info[1] != 1)
        edge_a[e] = -1;
        edge_b[e] = -1;
        edge_w[e] = 0.0;
    }
    if (tid == 0) {
        int rounds = 0;
        for (int k = 0; k < max_rounds; ++k) rounds += w.cnt[k] > 1;
        info[0] = rounds;
        info[1] = w.cnt[max_rounds];
        info[2] = *w.fault;
        info[3] = 0;
    }
}

template <int DM, bool EXACT, int R>
static void launch_nearest(const float* X, int n, int ldx, int d, const EmstWork& w, int round, int* splits_out, hipStream_t s) {
    const int tiles = cdiv(n, 256 * R);
    int splits = cdiv(1024, tiles);
    splits = splits < 1 ? 1 : (splits > EMST_SPLITS ? EMST_SPLITS : splits);
    const int slice = cdiv(cdiv(n, splits), EMST_TJ) * EMST_TJ;
    splits = cdiv(n, slice);
    *splits_out = splits;
    k_emst_nearest<DM, EXACT, R><<<dim3(tiles, splits), 256, 0, s>>>(X, n, ldx, d, w, round, slice);
}

extern "C" long clift_emst_work_bytes(long n) { return n < 0 ? 0 : CLIFT_EMST_WORK_BYTES(n); }

extern "C" int clift_emst(const float* X, long n, int ldx, int d, int* edge_a, int* edge_b, double* edge_w, int* info, void* work,
                          long work_bytes, clift_stream_t s) {
    CLIFT_REQUIRE(d >= 1, "clift_emst: need d >= 1 (got %d)", d);
    CLIFT_REQUIRE(d <= EMST_MAX_D, "clift_emst: d = %d exceeds the supported feature width %d", d, EMST_MAX_D);
    CLIFT_REQUIRE(ldx >= d, "clift_emst: row stride ldx = %d < d = %d", ldx, d);
    CLIFT_REQUIRE(n >= 2, "clift_emst: need n >= 2 (got %ld)", n);
    CLIFT_REQUIRE(n <= CLIFT_EMST_MAX_N,
                  "clift_emst: n = %ld exceeds CLIFT_EMST_MAX_N = %d (the work is O(n^2 log n) distance evaluations: subsample first)", n,
                  CLIFT_EMST_MAX_N);
    CLIFT_REQUIRE(X != nullptr && edge_a != nullptr && edge_b != nullptr && edge_w != nullptr && info != nullptr && work != nullptr,
                  "clift_emst: NULL buffer");
    CLIFT_REQUIRE(((uintptr_t)work & 7) == 0, "clift_emst: work must be 8-byte aligned");
    CLIFT_REQUIRE(work_bytes >= CLIFT_EMST_WORK_BYTES(n), "clift_emst: work_bytes = %ld < CLIFT_EMST_WORK_BYTES(%ld) = %ld", work_bytes, n,
                  (long)CLIFT_EMST_WORK_BYTES(n));
    const hipStream_t st = as_stream(s);
    const int ni = (int)n, blocks = cdiv(n, 256);
    const EmstWork w = emst_carve(work, n);
    int max_rounds = 0;
    while ((1L << max_rounds) < n) ++max_rounds;                  // ceil(log2 n) <= 17: every round at least halves the component count
    k_emst_init<<<cdiv(n < 32 ? 32 : n, 256), 256, 0, st>>>(w, ni);
    for (int round = 0; round < max_rounds; ++round) {
        int splits = 1;
        if (d == 3)       launch_nearest<3, true, 4>(X, ni, ldx, d, w, round, &splits, st);
        else if (d <= 4)  launch_nearest<4, false, 2>(X, ni, ldx, d, w, round, &splits, st);
        else if (d <= 8)  launch_nearest<8, false, 2>(X, ni, ldx, d, w, round, &splits, st);
        else if (d <= 16) launch_nearest<16, false, 1>(X, ni, ldx, d, w, round, &splits, st);
        else              launch_nearest<32, false, 1>(X, ni, ldx, d, w, round, &splits, st);
        k_emst_pair<<<blocks, 256, 0, st>>>(w, ni, round, splits);
        k_emst_link<<<blocks, 256, 0, st>>>(w, ni, round);
        k_emst_relabel<<<blocks, 256, 0, st>>>(w, ni, round);
    }
    k_emst_compact<<<1, 1024, 0, st>>>(w, ni, max_rounds, edge_a, edge_b, edge_w, info);
    return clift_check_launch("clift_emst");
}
