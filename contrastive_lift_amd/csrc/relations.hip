// relations.hip -- how the instances of a keyed 3-D lattice stand to one another: per key the point count, index sums and index
// box, per ordered pair of keys and axis the number of lattice faces between them (`faces`) and the number of contacts across a thin empty gap
// (`near`: a bounded look along +a through background, which no joint histogram of two arrays can express).  Integer counting only: the result
// is the same bits on every run, in any order of the adds (the rules: clift.h).
//
// Layout: the lattice is cut into 8 x 8 x 32 tiles and every block of a fixed grid takes one contiguous run of tiles.  A tile is read ONCE, as
// 16-bit words in LDS (keys are < 1024; 0xffff = no lattice point, 0xfffe = a key outside [0, n_keys)): the core, then for each axis the
// gap + 1 slabs beyond its positive face -- a pair or a look runs along one axis, so the edges and corners of the halo are never read and never
// loaded.  A wave is 2 rows of 32 points (lane = 32 * row + i2) and walks the 8 layers of the tile, so i0 is wave-uniform and the offsets along
// axes 1 and 2 are bit fields of the lane number.
//
// Skewed keys: label lattices are piecewise constant and one floor can own most points and most faces.
//   moments  equal keys are folded inside the wave (the loop of wave_fold_equal, clift_dev.h, written out in this file: through the helper
//            the kernel came out a VGPR smaller and 0.6 % slower in one of its timings).  Because the lanes' offsets are bit
//            fields of the lane number, the count, the three index sums and the index box of the lanes of one key all follow from the ballot
//            mask alone -- popcounts against five lane patterns, a count of leading and of trailing zeros -- without a shuffle.  The folded
//            record stays in the wave's registers while the next fold has the same key and goes to memory (ten atomics of one lane,
//            none waited for) when the key changes or the block ends: a wave inside one object costs ten atomics per BLOCK, not per row.
//   pairs    per axis one face code and one near code per lane, -1 where there is none; equal codes are folded by the same loop and the leader
//            adds the popcount.  A wave with no boundary in it pays six ballots.  With n_keys <= CLIFT_REL_LDS_KEYS the block counts into a
//            private table in LDS and adds its non-zero entries to memory once, when it ends; above it the folded adds go straight to memory.
// Only integer vector atomics (ds_add_u32, global_atomic_add / _add_x2 / _smin / _smax).
#include "keyed_lattice.h"

#define REL_THREADS 256
#define REL_T0 8
#define REL_T1 8
#define REL_T2 32
#define REL_HMAX (CLIFT_REL_MAX_GAP + 1)
#define REL_S1 (REL_T1 + REL_HMAX)
#define REL_S2 (REL_T2 + REL_HMAX)
#define REL_BOX ((REL_T0 + REL_HMAX) * REL_S1 * REL_S2)
#define REL_TAB (2 * 3 * CLIFT_REL_LDS_KEYS * CLIFT_REL_LDS_KEYS)
#define REL_OUT 0xffffu
#define REL_REJ 0xfffeu

static_assert(REL_THREADS == REL_T1 * REL_T2, "one thread per point of a tile layer");
static_assert(CLIFT_REL_MAX_KEYS <= REL_REJ, "keys are held as 16-bit words beside two sentinels");
static_assert(2L * 3 * CLIFT_REL_MAX_KEYS * CLIFT_REL_MAX_KEYS <= 0x7fffffffL, "a pair code fits an int");

typedef unsigned long long rel_u64;

struct RelArgs {
    const int* key;
    rel_u64* count; rel_u64* isum;
    int* ibox; int* faces; int* near; int* rejected;
    int n0, n1, n2, n_keys, gap, g1, g2;
    long tiles;
};

// the folded moments of one key, wave-uniform
struct RelAcc {
    int k, cnt;
    long s0, s1, s2;
    int lo0, lo1, lo2, hi0, hi1, hi2;
};

__device__ __forceinline__ unsigned rel_load(const RelArgs& g, int i0, int i1, int i2) {
    if ((unsigned)i0 >= (unsigned)g.n0 || (unsigned)i1 >= (unsigned)g.n1 || (unsigned)i2 >= (unsigned)g.n2) return REL_OUT;      // (a halo index past INT_MAX wraps: outside too)
    const int k = g.key[((long)i0 * g.n1 + i1) * g.n2 + i2];
    return (k < 0 || k >= g.n_keys) ? REL_REJ : (unsigned)k;
}

__device__ __forceinline__ void rel_flush(const RelArgs& g, const RelAcc& a, int lane) {
    if (a.k < 0 || lane != 0) return;                                                 // (no return value is used: the ten adds are issued back to back)
    atomicAdd(g.count + a.k, (rel_u64)a.cnt);
    atomicAdd(g.isum + 3 * a.k + 0, (rel_u64)a.s0);
    atomicAdd(g.isum + 3 * a.k + 1, (rel_u64)a.s1);
    atomicAdd(g.isum + 3 * a.k + 2, (rel_u64)a.s2);
    int* box = g.ibox + 6 * a.k;
    atomicMin(box + 0, a.lo0); atomicMin(box + 1, a.lo1); atomicMin(box + 2, a.lo2);
    atomicMax(box + 3, a.hi0); atomicMax(box + 4, a.hi1); atomicMax(box + 5, a.hi2);
}

// fold equal codes of the wave (code < 0: none) and add each popcount once: to the block's table, or to faces / near in memory
template <bool LDS>
__device__ __forceinline__ void rel_fold(const RelArgs& g, int* tab, int nf, int code, int lane) {
    unsigned long long todo = __ballot(code >= 0);                                   // wave-uniform: every lane of the wave walks the loop
    while (todo != 0ull) {
        const int leader = __ffsll(todo) - 1;
        const int c = __builtin_amdgcn_readlane(code, leader);
        const unsigned long long same = __ballot(code == c);
        if (lane == leader) {
            if (LDS) atomicAdd(&tab[c], __popcll(same));
            else atomicAdd(c < nf ? g.faces + c : g.near + (c - nf), __popcll(same));
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(64) void k_rel_init(int* __restrict__ ibox, int n_keys, int n0, int n1, int n2) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_keys * 6) return;
    const int j = e % 6;
    ibox[e] = j == 0 ? n0 : j == 1 ? n1 : j == 2 ? n2 : -1;
}

template <bool LDS>
__global__ __launch_bounds__(REL_THREADS) void k_lattice_relations(const RelArgs g) {
    __shared__ unsigned short s_key[REL_BOX];
    __shared__ int tab[LDS ? REL_TAB : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int z1 = tid >> 5, z2 = tid & 31;                                           // this thread's point of every layer
    const int H = g.gap + 1, nk = g.n_keys, nf = 3 * nk * nk;
    const long per = (g.tiles + gridDim.x - 1) / gridDim.x;
    const long t_lo = (long)blockIdx.x * per;
    const long t_hi = t_lo + per < g.tiles ? t_lo + per : g.tiles;
    if (t_lo >= t_hi) return;                                                         // block-uniform
    if (LDS) {
        for (int e = tid; e < 2 * nf; e += REL_THREADS) tab[e] = 0;                  // (the first barrier of the tile loop publishes it)
    }
    RelAcc acc;
    acc.k = -1; acc.cnt = 0; acc.s0 = acc.s1 = acc.s2 = 0; acc.lo0 = acc.lo1 = acc.lo2 = 0; acc.hi0 = acc.hi1 = acc.hi2 = 0;
    int rej = 0;
    for (long t = t_lo; t < t_hi; ++t) {
        const int b2 = (int)(t % g.g2) * REL_T2, b1 = (int)((t / g.g2) % g.g1) * REL_T1, b0 = (int)(t / ((long)g.g2 * g.g1)) * REL_T0;
#pragma unroll
        for (int z0 = 0; z0 < REL_T0; ++z0) s_key[(z0 * REL_S1 + z1) * REL_S2 + z2] = (unsigned short)rel_load(g, b0 + z0, b1 + z1, b2 + z2);
        for (int h = 0; h < H; ++h) {
            s_key[((REL_T0 + h) * REL_S1 + z1) * REL_S2 + z2] = (unsigned short)rel_load(g, b0 + REL_T0 + h, b1 + z1, b2 + z2);
            s_key[(z1 * REL_S1 + REL_T1 + h) * REL_S2 + z2] = (unsigned short)rel_load(g, b0 + z1, b1 + REL_T1 + h, b2 + z2);      // (z1 runs 0..7 = a layer)
        }
        for (int e = tid; e < REL_T0 * REL_T1 * H; e += REL_THREADS) {
            const int h = e >> 6, r = e & 63;
            s_key[((r >> 3) * REL_S1 + (r & 7)) * REL_S2 + REL_T2 + h] = (unsigned short)rel_load(g, b0 + (r >> 3), b1 + (r & 7), b2 + REL_T2 + h);
        }
        __syncthreads();
        const int i1w = b1 + (z1 & ~1);                                               // the wave's first row
        for (int z0 = 0; z0 < REL_T0; ++z0) {
            const int at = (z0 * REL_S1 + z1) * REL_S2 + z2;
            const unsigned u = s_key[at];
            const bool counted = u < REL_REJ;                                         // a lattice point with a key of the table
            rej += u == REL_REJ ? 1 : 0;
            // ---- moments: count, index sums and index box of the lanes of one key, from the ballot mask alone
            unsigned long long todo = __ballot(counted);
            while (todo != 0ull) {
                const int leader = __ffsll(todo) - 1;
                const int k = __builtin_amdgcn_readlane((int)u, leader);
                const unsigned long long same = __ballot(u == (unsigned)k);
                const unsigned lo32 = (unsigned)same, hi32 = (unsigned)(same >> 32), any = lo32 | hi32;
                const int cnt = __popcll(same), up = __popc(hi32);
                const int off2 = __popcll(same & 0xaaaaaaaaaaaaaaaaull) + 2 * __popcll(same & 0xccccccccccccccccull) +
                                 4 * __popcll(same & 0xf0f0f0f0f0f0f0f0ull) + 8 * __popcll(same & 0xff00ff00ff00ff00ull) +
                                 16 * __popcll(same & 0xffff0000ffff0000ull);
                const long s0 = (long)cnt * (b0 + z0), s1 = (long)cnt * i1w + up, s2 = (long)cnt * b2 + off2;
                const int lo1 = i1w + (lo32 != 0u ? 0 : 1), hi1 = i1w + (hi32 != 0u ? 1 : 0);
                const int lo2 = b2 + (__ffs(any) - 1), hi2 = b2 + 31 - __clz(any);
                if (k != acc.k) {
                    rel_flush(g, acc, lane);
                    acc.k = k; acc.cnt = cnt; acc.s0 = s0; acc.s1 = s1; acc.s2 = s2;
                    acc.lo0 = acc.hi0 = b0 + z0; acc.lo1 = lo1; acc.hi1 = hi1; acc.lo2 = lo2; acc.hi2 = hi2;
                } else {
                    acc.cnt += cnt; acc.s0 += s0; acc.s1 += s1; acc.s2 += s2;
                    acc.lo0 = min(acc.lo0, b0 + z0); acc.hi0 = max(acc.hi0, b0 + z0);
                    acc.lo1 = min(acc.lo1, lo1); acc.hi1 = max(acc.hi1, hi1);
                    acc.lo2 = min(acc.lo2, lo2); acc.hi2 = max(acc.hi2, hi2);
                }
                todo &= ~same;
            }
            // ---- pairs along each axis: the neighbour, and through background the first key within gap + 1 steps
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int st = a == 0 ? REL_S1 * REL_S2 : a == 1 ? REL_S2 : 1;
                int fcode = -1, ncode = -1;
                if (counted) {
                    const unsigned v = s_key[at + st];
                    if (v < REL_REJ && v != u) fcode = ((int)u * nk + (int)v) * 3 + a;
                    if (u != 0u && v == 0u) {
                        for (int d = 2; d <= H; ++d) {                                // H = gap + 1 <= REL_HMAX: inside the loaded slabs
                            const unsigned w = s_key[at + d * st];
                            if (w >= REL_REJ) break;                                  // the lattice ends, or a rejected key
                            if (w != 0u) {
                                if (w != u) ncode = nf + ((int)u * nk + (int)w) * 3 + a;
                                break;
                            }
                        }
                    }
                }
                rel_fold<LDS>(g, tab, nf, fcode, lane);
                if (H > 1) rel_fold<LDS>(g, tab, nf, ncode, lane);
            }
        }
        __syncthreads();                                                              // the next tile overwrites s_key
    }
    rel_flush(g, acc, lane);
    rej = wave_sum_i(rej);
    if (lane == 0 && rej != 0) atomicAdd(g.rejected, rej);
    if (LDS) {
        for (int e = tid; e < nf; e += REL_THREADS) {                                 // (after the tile loop's last barrier)
            const int v = tab[e];
            if (v != 0) atomicAdd(g.faces + e, v);
        }
        if (H > 1) {
            for (int e = tid; e < nf; e += REL_THREADS) {
                const int v = tab[nf + e];
                if (v != 0) atomicAdd(g.near + e, v);
            }
        }
    }
}

extern "C" int clift_lattice_relations(const int* key, int n0, int n1, int n2, int n_keys, int gap, long* count, long* isum, int* ibox, int* faces,
                                       int* near, int* rejected, clift_stream_t s) {
    if (keyed_lattice_check("clift_lattice_relations", n0, n1, n2, 0, n_keys, CLIFT_REL_MAX_KEYS)) return 1;
    CLIFT_REQUIRE(gap >= 0 && gap <= CLIFT_REL_MAX_GAP, "clift_lattice_relations: gap must be 0 .. %d (got %d)", CLIFT_REL_MAX_GAP, gap);
    CLIFT_REQUIRE((gap == 0) == (near == nullptr), "clift_lattice_relations: near must be NULL exactly when gap == 0 (gap %d, near %s)", gap,
                  near ? "given" : "NULL");
    CLIFT_REQUIRE(key && count && isum && ibox && faces && rejected, "clift_lattice_relations: NULL device buffer");
    const hipStream_t st = as_stream(s);
    const size_t nf = (size_t)3 * n_keys * n_keys;
    hipError_t e = hipMemsetAsync(count, 0, (size_t)n_keys * sizeof(long), st);
    if (e == hipSuccess) e = hipMemsetAsync(isum, 0, (size_t)3 * n_keys * sizeof(long), st);
    if (e == hipSuccess) e = hipMemsetAsync(faces, 0, nf * sizeof(int), st);
    if (e == hipSuccess && near) e = hipMemsetAsync(near, 0, nf * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(rejected, 0, sizeof(int), st);
    if (e != hipSuccess) {
        clift_set_error("clift_lattice_relations: clearing the tables failed: %s", hipGetErrorString(e));
        return 2;
    }
    k_rel_init<<<cdiv(6 * n_keys, 64), 64, 0, st>>>(ibox, n_keys, n0, n1, n2);
    RelArgs g;
    g.key = key; g.count = reinterpret_cast<rel_u64*>(count); g.isum = reinterpret_cast<rel_u64*>(isum);
    g.ibox = ibox; g.faces = faces; g.near = near; g.rejected = rejected;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.n_keys = n_keys; g.gap = gap;
    g.g1 = cdiv(n1, REL_T1); g.g2 = cdiv(n2, REL_T2);
    g.tiles = (long)cdiv(n0, REL_T0) * g.g1 * g.g2;                                   // <= total
    const int blocks = wave_item_blocks(g.tiles, 1, 4);                               // a block takes a run of tiles
    if (n_keys <= CLIFT_REL_LDS_KEYS) k_lattice_relations<true><<<blocks, REL_THREADS, 0, st>>>(g);
    else                              k_lattice_relations<false><<<blocks, REL_THREADS, 0, st>>>(g);
    return clift_check_launch("clift_lattice_relations");
}
