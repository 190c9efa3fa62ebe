// assign.hip -- rectangular linear assignment on the device (clift_lsap) and the "linear_assignment" instance loss of one image
// (clift_assign_loss; reference trainer/train_panopli_tensorf.py:237-242, 332-342) without a host round trip.  ABI 27.
//
// The assignment problem is tiny (L <= E <= 512) and latency-bound: what counts is the dependent chain of one augmenting step (scan E
// columns, take the arg-min), not throughput.  ONE WAVE owns one matrix: lane l owns the columns l, l + 64, ... (8 per lane at E = 512), the
// per-column state of the shortest-path search -- dual v, path length, predecessor, row of the column, visited bit -- sits in registers, the
// arg-min is a 64-lane butterfly and a step needs no barrier.  LDS holds what is indexed by a run-time row or column (row duals, the two
// matchings, the predecessors for the walk back) and, when it fits, the matrix itself; barriers stand only around the walk back, once per row.
#include "clift_dev.h"
#include <float.h>
#include <limits.h>

#define LSAP_MAX_E CLIFT_LSAP_MAX_E
#define LSAP_CPL (LSAP_MAX_E / 64)                       // columns per lane
#define LSAP_STATE_BYTES (LSAP_MAX_E * (8 + 4 + 4 + 4))  // u (fp64), col4row, row4col, pred
#define LSAP_MAT_BYTES (144 * 1024)                      // matrix budget in LDS: state + matrix stay under the CU's 160 KiB
#define LSAP_ASSIGNED LSAP_MAX_E                         // key bit above the column index: the column has a row (loses ties)

// what np.nan_to_num makes of an entry before scipy sees it
__device__ __forceinline__ float lsap_clean(float c) {
    if (c != c) return 0.f;
    return fminf(fmaxf(c, -FLT_MAX), FLT_MAX);
}

// Shortest augmenting paths (Jonker-Volgenant in Crouse's rectangular form, the method of scipy.optimize.linear_sum_assignment), rows added
// one at a time.  Duals, path lengths and the running minimum in fp64, the reduced cost evaluated left to right as scipy does:
// minv + c - u[i] - v[j].  Ties between columns: the column without a row first, then the lowest index.  Called by all 64 lanes of a
// one-wave block; `mat_floats` = floats of dynamic LDS behind the state block.  Every loop is bounded by L or E.
__device__ void lsap_wave(const float* __restrict__ cost, long ld, int L, int E, int* __restrict__ col_of_row, double* __restrict__ total,
                          int mat_floats) {
    extern __shared__ double lsap_lds[];
    double* u = lsap_lds;
    int* col4row = reinterpret_cast<int*>(u + LSAP_MAX_E);
    int* row4col = col4row + LSAP_MAX_E;
    int* pred_s = row4col + LSAP_MAX_E;
    float* mat = reinterpret_cast<float*>(pred_s + LSAP_MAX_E);
    const int lane = threadIdx.x & 63;
    const bool staged = (long)L * E <= (long)mat_floats;
    if (staged)
        for (int r = 0; r < L; ++r)
            for (int c = lane; c < E; c += 64) mat[r * E + c] = lsap_clean(cost[(long)r * ld + c]);
    for (int i = lane; i < LSAP_MAX_E; i += 64) {
        u[i] = 0.0;
        col4row[i] = -1;
        row4col[i] = -1;
        pred_s[i] = -1;
    }
    double v[LSAP_CPL];
#pragma unroll
    for (int k = 0; k < LSAP_CPL; ++k) v[k] = 0.0;
    __syncthreads();
    for (int cur = 0; cur < L; ++cur) {
        double sh[LSAP_CPL];
        int pr[LSAP_CPL], r4c[LSAP_CPL];
        unsigned visited = 0;
#pragma unroll
        for (int k = 0; k < LSAP_CPL; ++k) {
            const int j = lane + 64 * k;
            sh[k] = INFINITY;
            pr[k] = -1;
            r4c[k] = j < E ? row4col[j] : -1;
        }
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < E && sink < 0; ++step) {
            const double ui = u[i];
            float c[LSAP_CPL];
#pragma unroll
            for (int k = 0; k < LSAP_CPL; ++k) {          // one coalesced row, all loads in flight before the first use
                const int j = lane + 64 * k;
                c[k] = 0.f;
                if (j < E) c[k] = staged ? mat[i * E + j] : lsap_clean(cost[(long)i * ld + j]);
            }
            double bv = INFINITY;
            int bk = INT_MAX;
#pragma unroll
            for (int k = 0; k < LSAP_CPL; ++k) {
                const int j = lane + 64 * k;
                if (j < E && !((visited >> k) & 1u)) {
                    const double r = minv + (double)c[k] - ui - v[k];
                    if (r < sh[k]) {
                        sh[k] = r;
                        pr[k] = i;
                    }
                    const int key = (r4c[k] >= 0 ? LSAP_ASSIGNED : 0) | j;
                    if (sh[k] < bv || (sh[k] == bv && key < bk)) {
                        bv = sh[k];
                        bk = key;
                    }
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double ov = __shfl_xor(bv, d);
                const int ok = __shfl_xor(bk, d);
                if (ov < bv || (ov == bv && ok < bk)) {
                    bv = ov;
                    bk = ok;
                }
            }
            if (bk == INT_MAX) break;                     // no column left to take: cannot happen with L <= E and finite entries
            minv = bv;
            const int j = bk & (LSAP_MAX_E - 1);
            if (lane == (j & 63)) visited |= 1u << (j >> 6);
            if (bk & LSAP_ASSIGNED) i = row4col[j];
            else sink = j;
        }
        if (sink >= 0) {
#pragma unroll
            for (int k = 0; k < LSAP_CPL; ++k) {
                const int j = lane + 64 * k;
                if ((visited >> k) & 1u) {
                    const double d = minv - sh[k];
                    v[k] -= d;
                    if (r4c[k] >= 0) u[r4c[k]] += d;      // the rows of the search tree other than `cur`: one per visited column
                }
                if (j < E) pred_s[j] = pr[k];
            }
            if (lane == 0) u[cur] += minv;
        }
        __syncthreads();
        if (sink >= 0 && lane == 0) {                     // walk back along the predecessors, flipping the matching
            int j = sink;
            for (int hop = 0; hop <= L; ++hop) {
                const int r = pred_s[j];
                if (r < 0) break;
                row4col[j] = r;
                const int t = col4row[r];
                col4row[r] = j;
                j = t;
                if (r == cur || j < 0) break;
            }
        }
        __syncthreads();
    }
    for (int r = lane; r < L; r += 64) {
        const int j = col4row[r];
        col_of_row[r] = j;
        u[r] = j >= 0 ? (double)lsap_clean(cost[(long)r * ld + j]) : 0.0;      // (the duals are no longer needed)
    }
    __syncthreads();
    if (total != nullptr && lane == 0) {
        double t = 0.0;
        for (int r = 0; r < L; ++r) t += u[r];            // row order, fp64
        *total = t;
    }
}

__global__ __launch_bounds__(64) void k_lsap(const float* __restrict__ cost, int ld, long batch_stride, int L, int E, int* __restrict__ col_of_row,
                                             double* __restrict__ total, int mat_floats) {
    const long b = blockIdx.x;
    lsap_wave(cost + b * batch_stride, ld, L, E, col_of_row + b * L, total ? total + b : nullptr, mat_floats);
}

static int lsap_dyn_bytes(long rows, int E, int* mat_floats) {
    long m = rows * E * 4L;
    if (m > LSAP_MAT_BYTES) m = 0;                        // the matrix stays in global memory (L2)
    *mat_floats = (int)(m / 4);
    return LSAP_STATE_BYTES + (int)m;
}

extern "C" int clift_lsap(const float* cost, int ld, long batch_stride, int nb, int L, int E, int* col_of_row, double* total, clift_stream_t s) {
    CLIFT_REQUIRE(nb >= 0 && L >= 0 && E >= 0, "clift_lsap: negative size (nb %d, L %d, E %d)", nb, L, E);
    CLIFT_REQUIRE(L <= E, "clift_lsap: L = %d rows > E = %d columns (transpose the problem)", L, E);
    CLIFT_REQUIRE(E <= LSAP_MAX_E, "clift_lsap: E = %d exceeds CLIFT_LSAP_MAX_E = %d", E, LSAP_MAX_E);
    if (nb == 0 || L == 0) return 0;
    CLIFT_REQUIRE(ld >= E, "clift_lsap: leading dimension ld = %d < E = %d", ld, E);
    CLIFT_REQUIRE(batch_stride >= 0, "clift_lsap: negative batch_stride");
    CLIFT_REQUIRE(cost != nullptr && col_of_row != nullptr, "clift_lsap: NULL buffer");
    int mat_floats = 0;
    const int dyn = lsap_dyn_bytes(L, E, &mat_floats);
    if (dyn > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsap), hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    k_lsap<<<nb, 64, dyn, as_stream(s)>>>(cost, ld, batch_stride, L, E, col_of_row, total, mat_floats);
    return clift_check_launch("clift_lsap");
}

// ============================================================================ the fused loss of one image
struct AssignWork {
    float2* stat;      // n: row maximum, sum of exp(x - max)
    int* amax;         // n: argmax (lowest index among maxima)
    float* rowloss;    // n: conf_i * CE_i
    float* cost;       // E * E when the caller passes no cost buffer
};
static inline long assign_align(long b) { return (b + 15) & ~15L; }
static AssignWork assign_carve(void* work, long n, int E) {
    char* p = static_cast<char*>(work);
    AssignWork w;
    w.stat = reinterpret_cast<float2*>(p);    p += assign_align(8 * n);
    w.amax = reinterpret_cast<int*>(p);       p += assign_align(4 * n);
    w.rowloss = reinterpret_cast<float*>(p);  p += assign_align(4 * n);
    w.cost = reinterpret_cast<float*>(p);
    return w;
}

// one wave per ray: the softmax statistics of the cost matrix and the argmax of the "already correct" rule
__global__ __launch_bounds__(256) void k_assign_rowstat(const float* __restrict__ x, int ld, int n, int E, float2* __restrict__ stat,
                                                         int* __restrict__ amax) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;
    const float* row = x + (size_t)r * ld;
    float mx = -INFINITY;
    int am = INT_MAX;                                     // (a lane without a column, E < 64, keeps INT_MAX and loses every tie)
    for (int c = lane; c < E; c += 64) {
        const float a = row[c];
        if (am == INT_MAX || a > mx) {                    // strict: the lowest index of a lane's columns wins
            mx = a;
            am = c;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float om = __shfl_xor(mx, d);
        const int oa = __shfl_xor(am, d);
        if (om > mx || (om == mx && oa < am)) {
            mx = om;
            am = oa;
        }
    }
    float se = 0.f;
    for (int c = lane; c < E; c += 64) se += expf(row[c] - mx);      // (a NaN score makes the sum, and with it the whole row, NaN: torch.softmax)
    se = wave_sum(se);
    if (lane == 0) {
        stat[r] = make_float2(mx, se);
        amax[r] = am == INT_MAX ? 0 : am;
    }
}

// One workgroup: the distinct labels, ascending, the first E of them.  n <= 8192: bitonic sort of the (sign-flipped) labels in LDS, adjacent
// differences, a scan.  Larger n: one block-wide "smallest label above the last one" reduction per id -- slow (E passes over the labels) but
// exact at any n.  Also clears the active flag for the launches behind it.
#define ASSIGN_SORT_MAX 8192
__global__ __launch_bounds__(1024) void k_assign_ids(const int* __restrict__ labels, int n, int E, int* __restrict__ ids, int* __restrict__ n_ids,
                                                      int* __restrict__ active) {
    __shared__ unsigned key[ASSIGN_SORT_MAX];
    __shared__ int scan[1024];
    __shared__ long long red[1024];
    const int tid = threadIdx.x;
    if (tid == 0) *active = 0;
    if (n <= ASSIGN_SORT_MAX) {
        int N2 = 2;
        while (N2 < n) N2 <<= 1;
        for (int i = tid; i < N2; i += 1024) key[i] = i < n ? ((unsigned)labels[i] ^ 0x80000000u) : 0xFFFFFFFFu;
        __syncthreads();
        for (int k = 2; k <= N2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < N2 / 2; t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const unsigned a = key[i], b = key[p];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b;
                        key[p] = a;
                    }
                }
                __syncthreads();
            }
        // (the padding sorts last and equals no smaller key; a real INT_MAX label has the padding's key and the first n entries hold it)
        const int per = N2 >= 1024 ? N2 / 1024 : 1;
        const int lo = min(n, tid * per), hi = min(n, lo + per);
        int cnt = 0;
        for (int i = lo; i < hi; ++i) cnt += (i == 0 || key[i] != key[i - 1]);
        scan[tid] = cnt;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int a = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += a;
            __syncthreads();
        }
        const int all = scan[1023];
        int pos = scan[tid] - cnt;
        for (int i = lo; i < hi; ++i)
            if (i == 0 || key[i] != key[i - 1]) {
                if (pos < E) ids[pos] = (int)(key[i] ^ 0x80000000u);
                ++pos;
            }
        const int L = min(all, E);
        for (int e = L + tid; e < E; e += 1024) ids[e] = 0;
        if (tid == 0) *n_ids = L;
        return;
    }
    long long last = (long long)INT_MIN - 1;
    int L = 0;
    for (int it = 0; it < E; ++it) {
        long long best = LLONG_MAX;
        for (int i = tid; i < n; i += 1024) {
            const long long a = labels[i];
            if (a > last && a < best) best = a;
        }
        red[tid] = best;
        __syncthreads();
        for (int off = 512; off > 0; off >>= 1) {
            if (tid < off && red[tid + off] < red[tid]) red[tid] = red[tid + off];
            __syncthreads();
        }
        best = red[0];
        __syncthreads();
        if (best == LLONG_MAX) break;                     // (uniform: every thread read the same red[0])
        if (tid == 0) ids[it] = (int)best;
        last = best;
        L = it + 1;
    }
    for (int e = L + tid; e < E; e += 1024) ids[e] = 0;
    if (tid == 0) *n_ids = L;
}

// Workgroup l: S[l][e] = sum of softmax(scores_i)[e] over the rays of ids[l], fp64, in ray order, and the cost row.  The rays are taken 256
// at a time: an ordered compaction (ballot + wave offsets) lists the chunk's rays of this id, then every thread adds its columns over the list.
// A masked sum: rays of other ids are never read.  No atomics.
__global__ __launch_bounds__(256) void k_assign_sums(const float* __restrict__ x, int ld, const int* __restrict__ labels, int n, int E,
                                                      const int* __restrict__ ids, const int* __restrict__ n_ids, const float2* __restrict__ stat,
                                                      float* __restrict__ cost) {
    __shared__ int list[256];
    __shared__ int wcnt[4];
    const int l = blockIdx.x, tid = threadIdx.x, w = tid >> 6, ln = tid & 63;
    if (l >= min(*n_ids, E)) return;
    const int id = ids[l];
    double acc0 = 0.0, acc1 = 0.0;
    const int e0 = tid, e1 = tid + 256;
    int count = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const bool m = i < n && labels[i] == id;
        const unsigned long long b = __ballot(m);
        if (ln == 0) wcnt[w] = __popcll(b);
        __syncthreads();
        int off = 0, all = 0;
        for (int q = 0; q < 4; ++q) {
            if (q < w) off += wcnt[q];
            all += wcnt[q];
        }
        if (m) list[off + __popcll(b & ((1ull << ln) - 1ull))] = i;
        __syncthreads();
        for (int q = 0; q < all; ++q) {
            const int r = list[q];
            const float2 st = stat[r];
            const float* row = x + (size_t)r * ld;
            if (e0 < E) acc0 += (double)(expf(row[e0] - st.x) / st.y);
            if (e1 < E) acc1 += (double)(expf(row[e1] - st.x) / st.y);
        }
        count += all;
        __syncthreads();
    }
    const float den = (float)count + 1e-4f;
    if (e0 < E) cost[(size_t)l * E + e0] = -((float)acc0 / den);
    if (e1 < E) cost[(size_t)l * E + e1] = -((float)acc1 / den);
}

// one wave: the matching of the L = n_ids rows that k_assign_sums wrote -- the solver of clift_lsap, not a second one
__global__ __launch_bounds__(64) void k_assign_solve(const float* __restrict__ cost, int E, const int* __restrict__ n_ids, int* __restrict__ slot_of_id,
                                                     int mat_floats) {
    const int L = min(max(*n_ids, 0), E);
    lsap_wave(cost, E, L, E, slot_of_id, nullptr, mat_floats);
    for (int e = L + (int)threadIdx.x; e < E; e += 64) slot_of_id[e] = 0;
}

__global__ __launch_bounds__(256) void k_assign_target(const int* __restrict__ labels, int n, int E, const int* __restrict__ ids,
                                                        const int* __restrict__ n_ids, const int* __restrict__ slot_of_id, const int* __restrict__ amax,
                                                        int* __restrict__ target, int* __restrict__ active) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool off = false;
    if (i < n) {
        const int L = min(max(*n_ids, 0), E), y = labels[i];
        int lo = 0, hi = L;                               // first index with ids[index] >= y
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ids[mid] < y) lo = mid + 1;
            else hi = mid;
        }
        int t = (lo < L && ids[lo] == y) ? slot_of_id[lo] : 0;
        t = min(max(t, 0), E - 1);
        target[i] = t;
        off = t != amax[i];
    }
    if (__any(off) && (threadIdx.x & 63) == 0) atomicOr(active, 1);      // an integer OR: the result does not depend on the order
}

// Per-ray cross entropy in the arithmetic of semantic_row_loss (losses.hip) on a one-hot target with unit class weights: the same sequential
// maximum, sum and log, the same gradient expression.  Inactive image: zeros are WRITTEN.
__global__ __launch_bounds__(64) void k_assign_ce(const float* __restrict__ x, int ld, const int* __restrict__ target, const float* __restrict__ conf,
                                                  int n, int E, const int* __restrict__ active, float* __restrict__ rowloss, float* __restrict__ grad,
                                                  int ldg) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float* g = grad ? grad + (size_t)i * ldg : nullptr;
    if (*active == 0) {
        rowloss[i] = 0.f;
        if (g)
            for (int c = 0; c < E; ++c) g[c] = 0.f;
        return;
    }
    const float* row = x + (size_t)i * ld;
    const int t = target[i];
    const float cf = conf ? conf[i] : 1.f;
    float mx = -INFINITY;
    for (int c = 0; c < E; ++c) mx = fmaxf(mx, row[c]);
    float se = 0.f;
    for (int c = 0; c < E; ++c) se += expf(row[c] - mx);
    const float lse = mx + logf(se);
    const float ce = 0.f - (row[t] - lse);
    rowloss[i] = ce * cf;
    if (g) {
        const float k = cf / (float)n;
        for (int c = 0; c < E; ++c) g[c] = k * (expf(row[c] - lse) - (c == t ? 1.f : 0.f));
    }
}

// one workgroup, fixed order: thread t adds rows t, t + 1024, ...; then a tree over the 1024 partial sums
__global__ __launch_bounds__(1024) void k_assign_reduce(const float* __restrict__ rowloss, int n, const int* __restrict__ active, float* __restrict__ loss) {
    __shared__ float part[1024];
    const int tid = threadIdx.x;
    float a = 0.f;
    for (int i = tid; i < n; i += 1024) a += rowloss[i];
    part[tid] = a;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) *loss = *active ? part[0] / (float)n : 0.f;
}

extern "C" long clift_assign_work_bytes(long n, int E) {
    if (n < 0 || E < 0) return 0;
    return CLIFT_ASSIGN_WORK_BYTES(n, E);
}

extern "C" int clift_assign_loss(const float* scores, int ld, const int* labels, const float* conf, int n, int E, int* ids, int* n_ids, float* cost,
                                 int* slot_of_id, int* target, float* loss, float* grad, int ldg, int* active, void* work, long work_bytes,
                                 clift_stream_t s) {
    CLIFT_REQUIRE(E >= 2 && E <= LSAP_MAX_E, "clift_assign_loss: E = %d outside the supported range [2, %d]", E, LSAP_MAX_E);
    CLIFT_REQUIRE(n >= 1 && n <= CLIFT_ASSIGN_MAX_N, "clift_assign_loss: n = %d outside [1, %d]", n, CLIFT_ASSIGN_MAX_N);
    CLIFT_REQUIRE(ld >= E, "clift_assign_loss: leading dimension ld = %d < E = %d", ld, E);
    CLIFT_REQUIRE(grad == nullptr || ldg >= E, "clift_assign_loss: gradient leading dimension ldg = %d < E = %d", ldg, E);
    CLIFT_REQUIRE(scores != nullptr && labels != nullptr && ids != nullptr && n_ids != nullptr && slot_of_id != nullptr && target != nullptr &&
                      loss != nullptr && active != nullptr && work != nullptr,
                  "clift_assign_loss: NULL buffer");
    CLIFT_REQUIRE(((uintptr_t)work & 15) == 0, "clift_assign_loss: work must be 16-byte aligned");
    CLIFT_REQUIRE(work_bytes >= CLIFT_ASSIGN_WORK_BYTES(n, E), "clift_assign_loss: work_bytes = %ld < CLIFT_ASSIGN_WORK_BYTES(%d, %d) = %ld", work_bytes,
                  n, E, (long)CLIFT_ASSIGN_WORK_BYTES(n, E));
    const hipStream_t st = as_stream(s);
    const AssignWork w = assign_carve(work, n, E);
    float* cm = cost ? cost : w.cost;
    int mat_floats = 0;
    int dyn = lsap_dyn_bytes(E, E, &mat_floats);          // L is known on the device only: room for E rows, or the whole budget --
    if (mat_floats == 0) {                                // the wave stages the matrix when the L rows it finds fit
        mat_floats = LSAP_MAT_BYTES / 4;
        dyn = LSAP_STATE_BYTES + LSAP_MAT_BYTES;
    }
    k_assign_rowstat<<<cdiv(n, 4), 256, 0, st>>>(scores, ld, n, E, w.stat, w.amax);
    k_assign_ids<<<1, 1024, 0, st>>>(labels, n, E, ids, n_ids, active);
    k_assign_sums<<<E, 256, 0, st>>>(scores, ld, labels, n, E, ids, n_ids, w.stat, cm);
    if (dyn > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_assign_solve), hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    k_assign_solve<<<1, 64, dyn, st>>>(cm, E, n_ids, slot_of_id, mat_floats);
    k_assign_target<<<cdiv(n, 256), 256, 0, st>>>(labels, n, E, ids, n_ids, slot_of_id, w.amax, target, active);
    k_assign_ce<<<cdiv(n, 64), 64, 0, st>>>(scores, ld, target, conf, n, E, active, w.rowloss, grad, ldg);
    k_assign_reduce<<<1, 1024, 0, st>>>(w.rowloss, n, active, loss);
    return clift_check_launch("clift_assign_loss");
}
