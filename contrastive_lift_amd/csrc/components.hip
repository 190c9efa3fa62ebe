// components.hip -- connected components of a keyed 3-D lattice: the step between the density lattice and its mesh.
// Two lattice points belong together iff they are neighbours under the connectivity and carry the same non-zero key; root[p] = the smallest
// linear index of p's component, -1 for background.  Union-find with link-to-smaller-root: parent[x] <= x always, so the root of a tree is
// its smallest member and the result does not depend on the order in which the unions happen -- two runs give the same bits.
//   pass 1  k_cc_local    one block per 4 x 8 x 16 tile: union-find in LDS over the tile's own neighbour pairs, tile-local roots written as
//                         global indices (within a tile the local and the global index order agree, both are lexicographic in (i, j, k))
//   pass 2  k_cc_merge    the neighbour pairs that cross a tile face, edge or corner: unions on the root words, atomic-min at device scope
//   pass 3  k_cc_flatten  every point chases to its final root
// No block waits for another (the passes are separate launches), and every loop is a root chase or a union retry whose index strictly
// descends.  Only half of each neighbourhood is visited -- the offsets whose first non-zero component is -1 -- since the pair relation
// is symmetric.
#include "keyed_lattice.h"

#define CC_T0 4
#define CC_T1 8
#define CC_T2 16
#define CC_TILE (CC_T0 * CC_T1 * CC_T2)

// the lexicographically negative half of the 26-neighbourhood: rows [0, 3) = minus the faces (connectivity 6), [0, 7) = minus the seven Kuhn
// edge classes of isosurface.hip, in their order (connectivity 14), [0, 13) = all (connectivity 26)
__device__ const signed char CC_OFF[13][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {-1, -1, 0}, {-1, 0, -1}, {0, -1, -1}, {-1, -1, -1},
                                              {-1, 1, 0}, {-1, 0, 1}, {0, -1, 1}, {-1, 1, 1}, {-1, -1, 1}, {-1, 1, -1}};

// parent words are read and written by many threads at once: relaxed atomics (SCOPE = workgroup for the LDS table, agent for the root words,
// whose readers sit on other XCDs).  A stale read returns an earlier parent, which is still an ancestor: the atomic-min below sorts it out.
template <int SCOPE>
__device__ __forceinline__ int cc_find(const int* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;                                                  // p < x: the chase descends
    }
}

// join the sets of a and b.  The larger root a gets the smaller root b as parent by atomic-min; if the word no longer held a, somebody else
// had given a the parent `old` < a in the meantime (the word now holds min(old, b)) and the sets of old and b are joined next: a + b strictly
// descends from retry to retry.
template <int SCOPE>
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find<SCOPE>(parent, a);
        b = cc_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

struct CcTile {
    int l0, l1, l2;          // position in the tile
    int i0, i1, i2;          // position in the lattice
    int b0, b1, b2;          // the tile's first lattice point
    bool in;                 // a lattice point (tiles overhang the lattice)
    long p;                  // its linear index
};
__device__ __forceinline__ CcTile cc_tile(int n0, int n1, int n2, int g1, int g2) {
    CcTile t;
    const int tid = threadIdx.x, blk = blockIdx.x;
    t.l2 = tid % CC_T2; t.l1 = (tid / CC_T2) % CC_T1; t.l0 = tid / (CC_T2 * CC_T1);
    t.b2 = (blk % g2) * CC_T2; t.b1 = ((blk / g2) % g1) * CC_T1; t.b0 = (blk / (g2 * g1)) * CC_T0;
    t.i0 = t.b0 + t.l0; t.i1 = t.b1 + t.l1; t.i2 = t.b2 + t.l2;
    t.in = t.i0 < n0 && t.i1 < n1 && t.i2 < n2;
    t.p = ((long)t.i0 * n1 + t.i1) * n2 + t.i2;
    return t;
}

__global__ __launch_bounds__(CC_TILE) void k_cc_local(const int* __restrict__ key, int n0, int n1, int n2, int nb, int g1, int g2, int* __restrict__ root) {
    __shared__ int s_key[CC_TILE];
    __shared__ int s_parent[CC_TILE];
    const CcTile t = cc_tile(n0, n1, n2, g1, g2);
    const int tid = threadIdx.x;
    const int k = t.in ? key[t.p] : 0;
    s_key[tid] = k;
    s_parent[tid] = tid;
    __syncthreads();
    if (k != 0) {
        for (int j = 0; j < nb; ++j) {
            const int m0 = t.l0 + CC_OFF[j][0], m1 = t.l1 + CC_OFF[j][1], m2 = t.l2 + CC_OFF[j][2];
            if (m0 < 0 || m1 < 0 || m2 < 0 || m0 >= CC_T0 || m1 >= CC_T1 || m2 >= CC_T2) continue;
            const int q = (m0 * CC_T1 + m1) * CC_T2 + m2;
            if (s_key[q] == k) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, tid, q);        // (overhang holds key 0: never joined)
        }
    }
    __syncthreads();
    if (!t.in) return;
    int out = -1;
    if (k != 0) {
        const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, tid);
        const int r2 = r % CC_T2, r1 = (r / CC_T2) % CC_T1, r0 = r / (CC_T2 * CC_T1);
        out = (int)(((long)(t.b0 + r0) * n1 + (t.b1 + r1)) * n2 + (t.b2 + r2));
    }
    root[t.p] = out;
}

__global__ __launch_bounds__(CC_TILE) void k_cc_merge(const int* __restrict__ key, int n0, int n1, int n2, int nb, int g1, int g2, int* root) {
    const CcTile t = cc_tile(n0, n1, n2, g1, g2);
    if (!t.in) return;
    const int k = key[t.p];
    if (k == 0) return;
    for (int j = 0; j < nb; ++j) {
        const int d0 = CC_OFF[j][0], d1 = CC_OFF[j][1], d2 = CC_OFF[j][2];
        const int m0 = t.l0 + d0, m1 = t.l1 + d1, m2 = t.l2 + d2;
        if (m0 >= 0 && m1 >= 0 && m2 >= 0 && m0 < CC_T0 && m1 < CC_T1 && m2 < CC_T2) continue;       // the tile's own pair: pass 1
        const int j0 = t.i0 + d0, j1 = t.i1 + d1, j2 = t.i2 + d2;
        if (j0 < 0 || j1 < 0 || j2 < 0 || j0 >= n0 || j1 >= n1 || j2 >= n2) continue;
        const long q = ((long)j0 * n1 + j1) * n2 + j2;
        if (key[q] == k) cc_union<__HIP_MEMORY_SCOPE_AGENT>(root, (int)t.p, (int)q);
    }
}

// In place: a word is overwritten with its final root while others still chase through it -- they read the old parent or the final root,
// both ancestors.  Workgroup scope suffices for these loads and stores: what pass 2 wrote is visible to every XCD after the kernel boundary,
// roots are never written here, and a word that another block has or has not yet rewritten holds an ancestor either way, so no block needs
// to see another block's stores of this launch (relaxed atomics only keep the accesses whole and un-hoisted).
__global__ __launch_bounds__(256) void k_cc_flatten(int* root, long total) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int r = __hip_atomic_load(root + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (r < 0 || r == (int)p) return;
    const int f = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(root, r);
    if (f != r) __hip_atomic_store(root + p, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

extern "C" int clift_cc_label(const int* key, int n0, int n1, int n2, int connectivity, int* root, clift_stream_t s) {
    if (keyed_lattice_check("clift_cc_label", n0, n1, n2, 0, 0, 0)) return 1;                   // (no key table: any non-zero key)
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(connectivity == 6 || connectivity == 14 || connectivity == 26, "clift_cc_label: connectivity must be 6, 14 (Kuhn) or 26 (got %d)",
                  connectivity);
    CLIFT_REQUIRE(key && root, "clift_cc_label: NULL device buffer");
    const int nb = connectivity == 6 ? 3 : connectivity == 14 ? 7 : 13;
    const int g0 = cdiv(n0, CC_T0), g1 = cdiv(n1, CC_T1), g2 = cdiv(n2, CC_T2);
    const long tiles = (long)g0 * g1 * g2;                     // <= total
    k_cc_local<<<(int)tiles, CC_TILE, 0, as_stream(s)>>>(key, n0, n1, n2, nb, g1, g2, root);
    k_cc_merge<<<(int)tiles, CC_TILE, 0, as_stream(s)>>>(key, n0, n1, n2, nb, g1, g2, root);
    k_cc_flatten<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(root, total);
    return clift_check_launch("clift_cc_label");
}
