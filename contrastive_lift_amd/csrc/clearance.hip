// clearance.hip -- how far every instance of a keyed 3-D lattice can travel along the lattice axes before it meets another one:
// per ordered pair of keys and direction the smallest empty run between them (`pair`), per key and direction the free travel to first contact
// (`travel`) and the faces in contact once it has travelled (`landing`).  A sweep of unbounded length: a column is walked whole, with the last
// non-zero key and its index carried across any distance -- no tile, no halo, no bound on the run.  Integer counting only: the result is the
// same bits on every run, in any order of the atomics (the rules: clift.h).
//
// Layout: the work is a list of wave items on a fixed grid, taken with a stride of the grid's wave count, and every item reads coalesced.
//   axes 0, 1  an item is 64 neighbouring columns: a lane owns a column, neighbouring lanes own neighbouring i2, and each lane walks its column
//              with (last non-zero key, its index) in two registers; CLR_UNROLL loads are issued before the first is looked at.
//   axis 2     an item is a row, taken 64 points at a time (CLR_UNROLL chunks loaded ahead): the ballot of the non-zero points gives every
//              non-zero lane its predecessor -- the bits at and above the lane cleared, a count of leading zeros, one shuffle for that lane's
//              key --, and the last non-zero key and index of a chunk are carried wave-uniform into the next: a run may span many chunks.
// An event (u at i, v at j > i, background between) stands for two codes, (u, v, +a) and (v, u, -a), with the run g = j - i - 1.
//
// Two launches of ONE body: pass 1 takes the minima (pair, travel), pass 2 walks the same events again and counts those with
// g <= travel[u][d] + slack (landing).  Events are rare but skewed (one floor owns most): equal codes are folded inside the wave before any
// atomic -- pass 1 with a wave minimum, pass 2 with a popcount (wave_fold_equal of clift_dev.h) -- and with
// n_keys <= CLIFT_REL_LDS_KEYS the block works into a private table in LDS and sends its touched entries to memory once, when it ends; above
// it the folded atomics go straight to memory.  Only integer vector atomics: ds_min_i32, global_atomic_smin / _add, and flat_atomic_add /
// _smin where one atomic serves a destination picked at run time (the block's table or memory; pair or travel).
#include "keyed_lattice.h"

#define CLR_THREADS 256
#define CLR_WAVES (CLR_THREADS / 64)
#define CLR_UNROLL 8

static_assert(6L * CLIFT_REL_MAX_KEYS * CLIFT_REL_MAX_KEYS <= 0x7fffffffL, "a pair code fits an int");

struct ClrArgs {
    const int* key;
    int* pair; int* travel; int* landing; int* rejected;
    int n0, n1, n2, n_keys, slack, lds;
    long w0, w1, items;                                                               // column groups along axis 0, along axis 1; all items
};

// One event per lane at most (`event`: keys u at the lower and v at the upper end of an empty run of `run` points along axis a).  Wave
// collective: every lane of the wave calls it.  tab: the block's table in LDS, or nullptr.
template <bool SECOND>
__device__ __forceinline__ void clr_emit(const ClrArgs& g, int* tab, bool event, int u, int v, int a, int run, int lane) {
    if (__ballot(event) == 0ull) return;                                              // wave-uniform: the common case
    const int nk = g.n_keys, np = 6 * nk * nk;
    const int fwd = event ? (u * nk + v) * 6 + 2 * a : -1, bwd = event ? (v * nk + u) * 6 + 2 * a + 1 : -1;
    if (!SECOND) {
        // fwd names the unordered event: the lanes of one fwd code are the lanes of its bwd code
        wave_fold_equal(fwd, [&](int c, unsigned long long, int leader) {
            const int m = wave_min_i(fwd == c ? run : CLIFT_CLR_NONE);
            if (lane != leader) return;                                               // (after the wave minimum)
            if (tab) {
                atomicMin(&tab[fwd], m); atomicMin(&tab[bwd], m);
                atomicMin(&tab[np + u * 6 + 2 * a], m); atomicMin(&tab[np + v * 6 + 2 * a + 1], m);
            } else {
                atomicMin(g.pair + fwd, m); atomicMin(g.pair + bwd, m);
                atomicMin(g.travel + u * 6 + 2 * a, m); atomicMin(g.travel + v * 6 + 2 * a + 1, m);
            }
        });
    } else {
        // travel is final (pass 1 has ended); an event of (u, d) exists, so travel[u][d] <= run < 2^31 - 4
        int code[2];
        code[0] = event && run <= g.travel[u * 6 + 2 * a] + g.slack ? fwd : -1;
        code[1] = event && run <= g.travel[v * 6 + 2 * a + 1] + g.slack ? bwd : -1;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            wave_fold_equal(code[s], [&](int c, unsigned long long same, int leader) {
                if (lane == leader) atomicAdd(tab ? &tab[c] : g.landing + c, __popcll(same));
            });
    }
}

__global__ __launch_bounds__(256) void k_clr_init(int* __restrict__ pair, int* __restrict__ travel, long n_pair, long n_travel) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_pair; e += stride) pair[e] = CLIFT_CLR_NONE;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_travel; e += stride) travel[e] = CLIFT_CLR_NONE;
}

template <bool SECOND>
__global__ __launch_bounds__(CLR_THREADS) void k_lattice_clearance(const ClrArgs g) {
    extern __shared__ int clr_tab[];                                                  // pass 1: pair then travel (NONE); pass 2: landing (0)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = g.n_keys, np = 6 * nk * nk, nt = SECOND ? np : np + 6 * nk;
    int* tab = g.lds ? clr_tab : nullptr;
    if (tab) {
        for (int e = tid; e < nt; e += CLR_THREADS) tab[e] = SECOND ? 0 : CLIFT_CLR_NONE;
        __syncthreads();
    }
    const long n_waves = (long)gridDim.x * CLR_WAVES;
    const long plane = (long)g.n1 * g.n2;
    int rej = 0;
    for (long t = (long)blockIdx.x * CLR_WAVES + wave; t < g.items; t += n_waves) {  // wave-uniform
        if (t < g.w0 + g.w1) {
            // ---- 64 columns along axis 0 (the lane's column is (i1, i2) = c) or along axis 1 ((i0, i2) = c)
            const int a = t < g.w0 ? 0 : 1;
            const long c = (a == 0 ? t : t - g.w0) * 64 + lane;
            const int len = a == 0 ? g.n0 : g.n1;
            const long cols = a == 0 ? plane : (long)g.n0 * g.n2;
            const bool mine = c < cols;
            const long stride = a == 0 ? plane : (long)g.n2;
            const long base = a == 0 ? c : (c / g.n2) * plane + c % g.n2;            // (< 2^31 points: no overflow; unused where !mine)
            int last_k = -1, last_i = 0;
            for (int j0 = 0; j0 < len; j0 += CLR_UNROLL) {
                int kq[CLR_UNROLL];
#pragma unroll
                for (int q = 0; q < CLR_UNROLL; ++q) kq[q] = (mine && j0 + q < len) ? g.key[base + (long)(j0 + q) * stride] : 0;
#pragma unroll
                for (int q = 0; q < CLR_UNROLL; ++q) {
                    if (j0 + q >= len) break;                                         // wave-uniform
                    const int k = kq[q], j = j0 + q;
                    const bool ok = (unsigned)k < (unsigned)nk;
                    clr_emit<SECOND>(g, tab, ok && k > 0 && last_k > 0 && last_k != k, last_k, k, a, j - last_i - 1, lane);
                    if (k != 0) { last_k = ok ? k : -1; last_i = j; }                  // a rejected key ends the look from both sides
                }
            }
        } else {
            // ---- one row along axis 2, 64 points at a time
            const long row = t - g.w0 - g.w1;
            const int* line = g.key + row * g.n2;
            int carry_k = -1, carry_i = 0;                                            // wave-uniform
            for (int b0 = 0; b0 < g.n2; b0 += 64 * CLR_UNROLL) {
                int kq[CLR_UNROLL];
#pragma unroll
                for (int q = 0; q < CLR_UNROLL; ++q) {
                    const int i2 = b0 + 64 * q + lane;
                    kq[q] = i2 < g.n2 ? line[i2] : 0;
                }
#pragma unroll
                for (int q = 0; q < CLR_UNROLL; ++q) {
                    const int b = b0 + 64 * q;
                    if (b >= g.n2) break;                                             // wave-uniform
                    const int k = kq[q];
                    const bool ok = (unsigned)k < (unsigned)nk;
                    const int kk = ok ? k : -1;
                    if (!SECOND) rej += ok ? 0 : 1;                                   // every point is met once along axis 2 (beyond the row: k = 0)
                    const unsigned long long nz = __ballot(k != 0);
                    if (nz == 0ull) continue;                                         // wave-uniform
                    const unsigned long long below = nz & ((1ull << lane) - 1ull);
                    const int p = below != 0ull ? 63 - __clzll(below) : 0;
                    const int pk_lane = __shfl(kk, p);
                    const int pk = below != 0ull ? pk_lane : carry_k;
                    const int pi = below != 0ull ? b + p : carry_i;
                    clr_emit<SECOND>(g, tab, kk > 0 && pk > 0 && pk != kk, pk, kk, 2, b + lane - pi - 1, lane);
                    const int top = 63 - __clzll(nz);
                    carry_k = __builtin_amdgcn_readlane(kk, top);
                    carry_i = b + top;
                }
            }
        }
    }
    if (!SECOND) {
        rej = wave_sum_i(rej);
        if (lane == 0 && rej != 0) atomicAdd(g.rejected, rej);
    }
    if (tab) {
        __syncthreads();
        for (int e = tid; e < nt; e += CLR_THREADS) {                                 // the touched entries, once per block
            const int v = tab[e];
            if (SECOND) {
                if (v != 0) atomicAdd(g.landing + e, v);
            } else if (v != CLIFT_CLR_NONE) {
                atomicMin(e < np ? g.pair + e : g.travel + (e - np), v);
            }
        }
    }
}

extern "C" int clift_lattice_clearance(const int* key, int n0, int n1, int n2, int n_keys, int slack, int* pair, int* travel, int* landing,
                                       int* rejected, clift_stream_t s) {
    if (keyed_lattice_check("clift_lattice_clearance", n0, n1, n2, 0, n_keys, CLIFT_REL_MAX_KEYS)) return 1;
    CLIFT_REQUIRE(slack >= 0 && slack <= CLIFT_CLR_MAX_SLACK, "clift_lattice_clearance: slack must be 0 .. %d (got %d)", CLIFT_CLR_MAX_SLACK, slack);
    CLIFT_REQUIRE(key && pair && travel && landing && rejected, "clift_lattice_clearance: NULL device buffer");
    const hipStream_t st = as_stream(s);
    const long n_pair = 6L * n_keys * n_keys, n_travel = 6L * n_keys;
    hipError_t e = hipMemsetAsync(landing, 0, (size_t)n_pair * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(rejected, 0, sizeof(int), st);
    if (e != hipSuccess) {
        clift_set_error("clift_lattice_clearance: clearing the tables failed: %s", hipGetErrorString(e));
        return 2;
    }
    const long fill = (n_pair + 255) / 256;
    k_clr_init<<<(int)(fill < 1024 ? fill : 1024), 256, 0, st>>>(pair, travel, n_pair, n_travel);
    ClrArgs g;
    g.key = key; g.pair = pair; g.travel = travel; g.landing = landing; g.rejected = rejected;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.n_keys = n_keys; g.slack = slack;
    g.lds = n_keys <= CLIFT_REL_LDS_KEYS ? 1 : 0;
    g.w0 = n0 > 1 ? ((long)n1 * n2 + 63) / 64 : 0;                                    // a column of one point holds no event
    g.w1 = n1 > 1 ? ((long)n0 * n2 + 63) / 64 : 0;
    g.items = g.w0 + g.w1 + (long)n0 * n1;                                            // the rows are always walked: they count the rejected keys
    const int blocks = wave_item_blocks(g.items, CLR_WAVES, 4);
    const size_t lds1 = g.lds ? (size_t)(n_pair + n_travel) * sizeof(int) : 0, lds2 = g.lds ? (size_t)n_pair * sizeof(int) : 0;
    k_lattice_clearance<false><<<blocks, CLR_THREADS, lds1, st>>>(g);
    k_lattice_clearance<true><<<blocks, CLR_THREADS, lds2, st>>>(g);
    return clift_check_launch("clift_lattice_clearance");
}
