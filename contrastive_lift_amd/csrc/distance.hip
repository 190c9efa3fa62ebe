// distance.hip -- the exact Euclidean distance transform of a keyed 3-D lattice with the nearest site carried along: per point
// the packed word (dist2 << 31) | nearest, the minimum over all sites of (squared index distance, linear index of the site), and per key the
// smallest such word of its points (`key_min`).  Where clearance.hip looks along the six lattice directions, this looks everywhere.  Integer
// arithmetic only: the result is the same bits on every run, in any order of the atomics (the rules: clift.h).
//
// Three separable passes over packed words, z then y then x.  Adding (i - j)^2 << 31 to a word keeps the order of two words of one source
// point, so the minimum over j of in[j] + ((i - j)^2 << 31) along one axis after the other is the minimum of the packed word over all sites:
// distance first, the smaller linear index on a tie.
//   pass z     a wave owns a row, 64 points at a time.  The ballot of the site lanes gives every lane its nearest site at or below it (the
//              bits above the lane cleared, a count of leading zeros); the last site index of a chunk is carried wave-uniform into the next.
//              A backward sweep over the same row does the same with the bits above the lane and a count of trailing zeros (a site is a word
//              of the forward sweep with dist2 == 0) and keeps the smaller word.  The rejected keys are counted in the forward sweep.
//   pass y, x  a lane owns a column, neighbouring lanes own neighbouring i2, so a wave's load is one contiguous run of 8-byte words.  The lane
//              first walks its column once for the first and the last index that hold a word at all (lo, hi), then takes for each point i an
//              expanding search j = i -/+ r from its own word: r starts where the search first meets [lo, hi], and ends when r^2 exceeds the
//              best dist2 (strictly: a candidate with r^2 == dist2 ties on distance and may win on the index) or both ends have left
//              [lo, hi].  No per-lane storage.  CLIFT_DT_NONE is tested, never added to.  A column is cut into segments of `seg` points
//              where the lattice has too few columns to fill the device; every segment repeats the walk for lo and hi.
//   pass x     also folds key_min: equal keys inside the wave first (wave_fold_equal of clift_dev.h with a 64-bit wave minimum), then one
//              64-bit unsigned atomic minimum per distinct key and wave (global_atomic_umin_x2).
// Only vector loads, stores and atomics.  z writes `out`, y reads it into `work`, x reads `work` into `out`.
#include "keyed_lattice.h"

#define DT_THREADS 256
#define DT_WAVES (DT_THREADS / 64)
#define DT_UNROLL 8
#define DT_MIN_SEG 32

static_assert(3L * (CLIFT_DT_MAX_DIM - 1) * (CLIFT_DT_MAX_DIM - 1) <= 0x7fffffffL, "dist2 fits 31 bits");

struct DtArgs {
    const int* key; const unsigned char* site;
    const long* in; long* dst;
    unsigned long long* key_min; int* rejected;
    int n0, n1, n2, n_keys, axis, seg;
    long items;
};

__device__ __forceinline__ long dt_word(int d, long lin) { return (((long)d * d) << 31) | lin; }

__global__ __launch_bounds__(256) void k_dt_init(long* __restrict__ key_min, int n_keys) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_keys) key_min[e] = CLIFT_DT_NONE;
}

// pass z: dst[p] = the word of the nearest site of p's own row, CLIFT_DT_NONE for a row without one
__global__ __launch_bounds__(DT_THREADS) void k_dt_rows(const DtArgs g) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n_waves = (long)gridDim.x * DT_WAVES;
    const int n2 = g.n2;
    int rej = 0;
    for (long row = (long)blockIdx.x * DT_WAVES + wave; row < g.items; row += n_waves) {          // wave-uniform
        const long base = row * n2;
        int carry = -1;                                                                   // the last site index so far, wave-uniform
        for (int b = 0; b < n2; b += 64) {
            const int i = b + lane;
            const bool in_row = i < n2;
            const int k = in_row ? g.key[base + i] : 0;
            const bool ok = (unsigned)k < (unsigned)g.n_keys;
            rej += ok ? 0 : 1;                                                            // (beyond the row: k = 0)
            const bool is_site = in_row && ok && g.site[ok ? k : 0] != 0;
            const unsigned long long sb = __ballot(is_site);
            const unsigned long long below = sb & ((2ull << lane) - 1ull);                // at or below the lane (lane 63: all bits)
            const int p = below != 0ull ? b + 63 - __clzll(below) : carry;
            if (in_row) g.dst[base + i] = p >= 0 ? dt_word(i - p, base + p) : CLIFT_DT_NONE;
            if (sb != 0ull) carry = b + 63 - __clzll(sb);
        }
        if (carry < 0) continue;                                                          // no site in the row: all words stay NONE
        carry = -1;                                                                       // the first site index above, wave-uniform
        for (int b = ((n2 - 1) / 64) * 64; b >= 0; b -= 64) {
            const int i = b + lane;
            const bool in_row = i < n2;
            long w = in_row ? g.dst[base + i] : CLIFT_DT_NONE;                            // this lane's own store of the forward sweep
            const unsigned long long sb = __ballot(in_row && (w >> 31) == 0);
            const unsigned long long above = sb & ~((2ull << lane) - 1ull);               // strictly above the lane
            const int q = above != 0ull ? b + __ffsll(above) - 1 : carry;
            if (in_row && q >= 0) {
                const long c = dt_word(q - i, base + q);
                if (c < w) g.dst[base + i] = c;
            }
            if (sb != 0ull) carry = b + __ffsll(sb) - 1;
        }
    }
    rej = wave_sum_i(rej);
    if (lane == 0 && rej != 0) atomicAdd(g.rejected, rej);
}

// pass y (axis 1) and x (axis 0): dst[i] = min over j of in[j] + ((i - j)^2 << 31) over the words of the column that are not NONE
template <bool LAST>
__global__ __launch_bounds__(DT_THREADS) void k_dt_cols(const DtArgs g) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n_waves = (long)gridDim.x * DT_WAVES;
    const long plane = (long)g.n1 * g.n2;
    const int a = g.axis;
    const int len = a == 0 ? g.n0 : g.n1;
    const long cols = a == 0 ? plane : (long)g.n0 * g.n2;
    const long stride = a == 0 ? plane : (long)g.n2;
    const int segs = (len + g.seg - 1) / g.seg;
    for (long t = (long)blockIdx.x * DT_WAVES + wave; t < g.items; t += n_waves) {       // wave-uniform
        const long c = (t / segs) * 64 + lane;
        const int i_lo = (int)(t % segs) * g.seg, i_hi = min(i_lo + g.seg, len);
        const bool mine = c < cols;
        const long base = a == 0 ? c : (c / g.n2) * plane + c % g.n2;                    // (< 2^31 points: no overflow; unused where !mine)
        int lo = len, hi = -1;                                                            // the first and the last index that hold a word
        for (int j0 = 0; j0 < len; j0 += DT_UNROLL) {
            long wq[DT_UNROLL];
#pragma unroll
            for (int q = 0; q < DT_UNROLL; ++q) wq[q] = (mine && j0 + q < len) ? g.in[base + (long)(j0 + q) * stride] : CLIFT_DT_NONE;
#pragma unroll
            for (int q = 0; q < DT_UNROLL; ++q)
                if (wq[q] != CLIFT_DT_NONE) { lo = min(lo, j0 + q); hi = j0 + q; }
        }
        for (int i = i_lo; i < i_hi; ++i) {                                               // wave-uniform bounds
            const long at = base + (long)i * stride;
            long best = CLIFT_DT_NONE;
            if (mine) {
                best = g.in[at];
                // (NONE >> 31 = 2^32 - 1 is above every r^2: an empty best never ends the search)
                for (int r = max(1, max(lo - i, i - hi)); i - r >= lo || i + r <= hi; ++r) {
                    const long r2 = (long)r * r;
                    if ((best >> 31) < r2) break;
                    if (i - r >= lo) {
                        const long w = g.in[at - (long)r * stride];
                        if (w != CLIFT_DT_NONE) best = min(best, w + (r2 << 31));
                    }
                    if (i + r <= hi) {
                        const long w = g.in[at + (long)r * stride];
                        if (w != CLIFT_DT_NONE) best = min(best, w + (r2 << 31));
                    }
                }
                g.dst[at] = best;
            }
            if (LAST && g.key_min) {
                const int k = mine ? g.key[at] : 0;
                const int u = (best != CLIFT_DT_NONE && k > 0 && k < g.n_keys) ? k : -1;
                const unsigned long long word = (unsigned long long)(((best >> 31) << 31) | at);
                wave_fold_equal(u, [&](int ku, unsigned long long, int leader) {
                    const unsigned long long m = wave_min_u64(u == ku ? word : (unsigned long long)CLIFT_DT_NONE);
                    if (lane == leader) atomicMin(g.key_min + ku, m);
                });
            }
        }
    }
}

extern "C" int clift_lattice_distance(const int* key, int n0, int n1, int n2, int n_keys, const unsigned char* site, long* out, long* work,
                                      long* key_min, int* rejected, clift_stream_t s) {
    if (keyed_lattice_check("clift_lattice_distance", n0, n1, n2, CLIFT_DT_MAX_DIM, n_keys, CLIFT_REL_MAX_KEYS)) return 1;
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(key && site && out && work && rejected, "clift_lattice_distance: NULL device buffer");
    const char *ob = reinterpret_cast<const char*>(out), *wb = reinterpret_cast<const char*>(work);
    CLIFT_REQUIRE(ob + total * sizeof(long) <= wb || wb + total * sizeof(long) <= ob, "clift_lattice_distance: out and work overlap");
    const hipStream_t st = as_stream(s);
    const hipError_t e = hipMemsetAsync(rejected, 0, sizeof(int), st);
    if (e != hipSuccess) {
        clift_set_error("clift_lattice_distance: clearing the count failed: %s", hipGetErrorString(e));
        return 2;
    }
    if (key_min) k_dt_init<<<(n_keys + 255) / 256, 256, 0, st>>>(key_min, n_keys);
    const long want = (long)clift_persistent_cus() * 4;                                   // blocks of the fixed grid
    DtArgs g;
    g.key = key; g.site = site; g.key_min = reinterpret_cast<unsigned long long*>(key_min); g.rejected = rejected;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.n_keys = n_keys;
    g.axis = 2; g.seg = 0; g.in = nullptr; g.dst = out; g.items = (long)n0 * n1;
    k_dt_rows<<<wave_item_blocks(g.items, DT_WAVES, 4), DT_THREADS, 0, st>>>(g);
    for (int a = 1; a >= 0; --a) {
        const int len = a == 0 ? n0 : n1;
        const long groups = ((a == 0 ? (long)n1 * n2 : (long)n0 * n2) + 63) / 64;
        int seg = len;                                                                    // shorter segments until the grid has its waves
        while (seg > DT_MIN_SEG && groups * ((len + seg - 1) / seg) < want * DT_WAVES) seg = (seg + 1) / 2;
        g.axis = a; g.seg = seg; g.items = groups * ((len + seg - 1) / seg);
        g.in = a == 1 ? out : work; g.dst = a == 1 ? work : out;
        const int blocks = wave_item_blocks(g.items, DT_WAVES, 4);
        if (a == 1) k_dt_cols<false><<<blocks, DT_THREADS, 0, st>>>(g);
        else k_dt_cols<true><<<blocks, DT_THREADS, 0, st>>>(g);
    }
    return clift_check_launch("clift_lattice_distance");
}
