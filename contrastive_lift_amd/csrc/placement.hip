// placement.hip -- the placement map of a keyed 3-D lattice: for every translation t of an object's voxel shape over the
// lattice the number of its cells that collide (`overlap`), the number of its faces that look along a direction d onto something solid
// (`support`), the counts of the free and of the free and supported translations, and of each kind the one nearest to a target as the
// packed word (dist2 << 31) | lin_T of distance.hip.  A correlation of two bit sets; integer arithmetic only, so the result is the same
// bits on every run, in any order of the atomics (the rules: clift.h).
//
// Three launches in stream order over packed 64-bit words, bit b of word w of a row = the point z' = 64 w + b:
//   shape      the object's box grown by one cell on every side, c' = c + 1, as two masks of (m0 + 2)(m1 + 2) rows of MW words: its cells,
//              and its d-shadow {c + e_d : c in shape, c + e_d not in shape}.  A wave owns a word: the ballots of the two predicates.  The
//              first two threads also reset count, best and rejected.
//   pack       the lattice with one zero point around it on every side, p' = p + 1, as (n0 + 2)(n1 + 2) rows of WP words.  A wave reads 64
//              consecutive keys of a row, the ballot of "solid" is the word and one lane stores it; border rows and the words behind a
//              row are zero, so a window that starts at t2 or runs past n2 reads zeros and never leaves the row.  Every lattice point is
//              read by exactly one lane: the rejected keys are counted here.
//   correlate  overlap[t] = sum over s' of cells(s') P(t + s'), support[t] the same with the shadow: the grown box and the padded lattice
//              share the offset.  Lanes run along t2, a wave owns 64 consecutive t2 of one (t0, t1).  For a mask row (i, j) the words of
//              lattice row (t0 + i, t1 + j) and the mask words are wave-uniform; a lane forms its window (lo >> l) | (hi << (64 - l)), ANDs it
//              with each mask word and counts the bits.  Mask words without a bit and windows without a solid point are skipped, both
//              uniform branches.  Lanes with t2 >= T2 idle (accepted: DESIGN.md).  The counts and the two minima are carried over the items
//              of a wave and folded inside it, then one vector atomic each per wave (atomicAdd on int, atomicMin on unsigned long long).
#include "keyed_lattice.h"

#define PM_THREADS 256
#define PM_WAVES (PM_THREADS / 64)

typedef unsigned long long pm_word;

struct PmArgs {
    const int* key; const unsigned char* solid; const unsigned char* shape;
    pm_word* lat; pm_word* cells; pm_word* shadow;                                         // the three parts of `work`
    int* overlap; int* support; int* count; pm_word* best; int* rejected;
    int n0, n1, n2, n_keys, m0, m1, m2, dir, min_support, g0, g1, g2;
    int T0, T1, T2, Q, wp, mw;                                                             // Q = ceil(T2 / 64) chunks of t2
    long items;
};

// a word that every lane holds alike, as a scalar: the branches on it are uniform
__device__ __forceinline__ pm_word pm_uniform(pm_word v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((pm_word)hi << 32) | lo;
}

__device__ __forceinline__ bool pm_cell(const PmArgs& g, int c0, int c1, int c2) {
    if (c0 < 0 || c1 < 0 || c2 < 0 || c0 >= g.m0 || c1 >= g.m1 || c2 >= g.m2) return false;
    return g.shape[((long)c0 * g.m1 + c1) * g.m2 + c2] != 0;
}

__global__ __launch_bounds__(PM_THREADS) void k_pm_shape(const PmArgs g) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        g.count[threadIdx.x] = 0;
        g.best[threadIdx.x] = (pm_word)CLIFT_PM_NONE;
        if (threadIdx.x == 0) g.rejected[0] = 0;
    }
    const long n_waves = (long)gridDim.x * PM_WAVES;
    const int a = g.dir >> 1, sgn = (g.dir & 1) ? -1 : 1;
    for (long item = (long)blockIdx.x * PM_WAVES + wave; item < g.items; item += n_waves) {       // wave-uniform
        const int k = (int)(item % g.mw);
        const long row = item / g.mw;
        const int c0 = (int)(row / (g.m1 + 2)) - 1, c1 = (int)(row % (g.m1 + 2)) - 1, c2 = 64 * k + lane - 1;
        const bool cell = pm_cell(g, c0, c1, c2);
        const bool from = pm_cell(g, c0 - (a == 0 ? sgn : 0), c1 - (a == 1 ? sgn : 0), c2 - (a == 2 ? sgn : 0));
        const pm_word cb = __ballot(cell), sb = __ballot(from && !cell);
        if (lane == 0) {
            g.cells[item] = cb;
            g.shadow[item] = sb;
        }
    }
}

__global__ __launch_bounds__(PM_THREADS) void k_pm_pack(const PmArgs g) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n_waves = (long)gridDim.x * PM_WAVES;
    int rej = 0;
    for (long item = (long)blockIdx.x * PM_WAVES + wave; item < g.items; item += n_waves) {       // wave-uniform
        const int w = (int)(item % g.wp);
        const long row = item / g.wp;
        const int x = (int)(row / (g.n1 + 2)) - 1, y = (int)(row % (g.n1 + 2)) - 1, z = 64 * w + lane - 1;
        const bool inside = x >= 0 && y >= 0 && z >= 0 && x < g.n0 && y < g.n1 && z < g.n2;
        const int k = inside ? g.key[((long)x * g.n1 + y) * g.n2 + z] : 0;
        const bool ok = (unsigned)k < (unsigned)g.n_keys;
        rej += ok ? 0 : 1;                                                                 // (outside: k = 0)
        const pm_word word = __ballot(inside && ok && g.solid[ok ? k : 0] != 0);
        if (lane == 0) g.lat[item] = word;
    }
    rej = wave_sum_i(rej);
    if (lane == 0 && rej != 0) atomicAdd(g.rejected, rej);
}

__global__ __launch_bounds__(PM_THREADS) void k_pm_correlate(const PmArgs g) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n_waves = (long)gridDim.x * PM_WAVES;
    const int rows1 = g.m1 + 2, mw = g.mw, wp = g.wp;
    const long lat_pitch = (long)(g.n1 + 2) * wp;
    int n_free = 0, n_sup = 0;                                                             // wave-uniform
    pm_word best_free = (pm_word)CLIFT_PM_NONE, best_sup = (pm_word)CLIFT_PM_NONE;
    for (long item = (long)blockIdx.x * PM_WAVES + wave; item < g.items; item += n_waves) {       // wave-uniform
        const int q = (int)(item % g.Q);
        const long r = item / g.Q;
        const int t0 = (int)(r / g.T1), t1 = (int)(r % g.T1), t2 = 64 * q + lane;
        int ov = 0, su = 0;
        for (int i = 0; i < g.m0 + 2; ++i) {
            const pm_word* lrow = g.lat + (long)(t0 + i) * lat_pitch + (long)t1 * wp + q;
            const pm_word* crow = g.cells + (long)i * rows1 * mw;
            const pm_word* srow = g.shadow + (long)i * rows1 * mw;
            for (int j = 0; j < rows1; ++j, lrow += wp, crow += mw, srow += mw) {
                for (int k = 0; k < mw; ++k) {
                    const pm_word c = pm_uniform(crow[k]), s = pm_uniform(srow[k]);
                    if ((c | s) == 0ull) continue;
                    const pm_word lo = pm_uniform(lrow[k]), hi = pm_uniform(lrow[k + 1]);
                    if ((lo | hi) == 0ull) continue;
                    const pm_word win = (lo >> lane) | ((hi << 1) << (63 - lane));         // (lane 0: hi falls out whole)
                    ov += __popcll(win & c);
                    su += __popcll(win & s);
                }
            }
        }
        const bool mine = t2 < g.T2;
        const long lin = ((long)t0 * g.T1 + t1) * g.T2 + t2;
        if (mine) {
            g.overlap[lin] = ov;
            g.support[lin] = su;
        }
        const bool fr = mine && ov == 0, sp = fr && su >= g.min_support;
        n_free += __popcll(__ballot(fr));
        n_sup += __popcll(__ballot(sp));
        const long d0 = t0 - g.g0, d1 = t1 - g.g1, d2 = t2 - g.g2;
        const pm_word word = (pm_word)(((d0 * d0 + d1 * d1 + d2 * d2) << 31) | lin);
        if (fr && word < best_free) best_free = word;
        if (sp && word < best_sup) best_sup = word;
    }
    best_free = wave_min_u64(best_free);
    best_sup = wave_min_u64(best_sup);
    if (lane == 0) {
        if (n_free != 0) {
            atomicAdd(g.count, n_free);
            atomicMin(g.best, best_free);
        }
        if (n_sup != 0) {
            atomicAdd(g.count + 1, n_sup);
            atomicMin(g.best + 1, best_sup);
        }
    }
}

extern "C" int clift_lattice_placement(const int* key, int n0, int n1, int n2, int n_keys, const unsigned char* solid, const unsigned char* shape,
                                       int m0, int m1, int m2, int direction, int min_support, int t0, int t1, int t2, int* overlap, int* support,
                                       int* count, long* best, int* rejected, long* work, clift_stream_t s) {
    if (keyed_lattice_check("clift_lattice_placement", n0, n1, n2, CLIFT_DT_MAX_DIM, n_keys, CLIFT_REL_MAX_KEYS)) return 1;
    CLIFT_REQUIRE(m0 >= 1 && m1 >= 1 && m2 >= 1 && m0 <= n0 && m1 <= n1 && m2 <= n2,
                  "clift_lattice_placement: shape dimensions must be 1 .. the lattice's (got %d x %d x %d in %d x %d x %d)", m0, m1, m2, n0, n1, n2);
    CLIFT_REQUIRE(direction >= 0 && direction <= 5, "clift_lattice_placement: direction must be 0 .. 5 (got %d)", direction);
    CLIFT_REQUIRE(min_support >= 1, "clift_lattice_placement: min_support must be >= 1 (got %d)", min_support);
    PmArgs g;
    g.T0 = n0 - m0 + 1; g.T1 = n1 - m1 + 1; g.T2 = n2 - m2 + 1;
    CLIFT_REQUIRE(t0 >= 0 && t1 >= 0 && t2 >= 0 && t0 < g.T0 && t1 < g.T1 && t2 < g.T2,
                  "clift_lattice_placement: target must lie inside the %d x %d x %d translations (got %d, %d, %d)", g.T0, g.T1, g.T2, t0, t1, t2);
    CLIFT_REQUIRE(key && solid && shape && overlap && support && count && best && rejected && work, "clift_lattice_placement: NULL device buffer");
    g.key = key; g.solid = solid; g.shape = shape;
    g.overlap = overlap; g.support = support; g.count = count; g.best = reinterpret_cast<pm_word*>(best); g.rejected = rejected;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.n_keys = n_keys; g.m0 = m0; g.m1 = m1; g.m2 = m2;
    g.dir = direction; g.min_support = min_support; g.g0 = t0; g.g1 = t1; g.g2 = t2;
    g.mw = (int)CLIFT_PM_MASK_WORDS(m2); g.wp = (int)CLIFT_PM_ROW_WORDS(n2, m2); g.Q = (g.T2 + 63) / 64;
    const long lat_words = ((long)n0 + 2) * (n1 + 2) * g.wp, mask_words = ((long)m0 + 2) * (m1 + 2) * g.mw;
    g.lat = reinterpret_cast<pm_word*>(work); g.cells = g.lat + lat_words; g.shadow = g.cells + mask_words;
    const hipStream_t st = as_stream(s);
    const long sizes[3] = {mask_words, lat_words, (long)g.T0 * g.T1 * g.Q};
    for (int pass = 0; pass < 3; ++pass) {
        g.items = sizes[pass];
        const int blocks = wave_item_blocks(g.items, PM_WAVES, 8);
        if (pass == 0) k_pm_shape<<<blocks, PM_THREADS, 0, st>>>(g);
        else if (pass == 1) k_pm_pack<<<blocks, PM_THREADS, 0, st>>>(g);
        else k_pm_correlate<<<blocks, PM_THREADS, 0, st>>>(g);
    }
    return clift_check_launch("clift_lattice_placement");
}
