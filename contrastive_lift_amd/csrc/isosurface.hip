// isosurface.hip -- the scene as a surface: sigma on a (possibly upsampled) lattice of the box, and a deterministic, scan-ordered
// iso-surface of a scalar lattice by marching tetrahedra on the Kuhn split.
// Reference rows: model/renderer/panopli_tensoRF_renderer.py:731-748 (get_dense_sigma; the reference keeps no extractor of its own).
#include "clift_dev.h"
#include "lattice_dev.h"

// ============================================================================ sigma on the lattice
// k_alpha_lattice (march.hip) without the alpha step: lattice point p_a = lo_a (1 - s) + hi_a s with s = the caller's linspace value of
// that axis, normalised like renderer.py:633, density + softplus like tensoRF.py:114-125.  4 lanes per lattice point (lane q owns channels
// [4q, 4q + 4) + 16 per pass), long indices, fully coalesced store.  The point and the per-lane sum live in lattice_dev.h: the edited lattice
// (k_edit_list_dense_sigma, edit.hip) shares them.
__global__ __launch_bounds__(256) void k_dense_sigma(VmP t, float3 lo, float3 hi, float3 inv_ext2, const float* __restrict__ s0,
                                                      const float* __restrict__ s1, const float* __restrict__ s2, int n0, int n1, int n2,
                                                      float shift, float* __restrict__ out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long v = gid >> 2, total = (long)n0 * n1 * n2;
    const int q = (int)(gid & 3);
    if (v >= total) return;
    const int i2 = (int)(v % n2), i1 = (int)((v / n2) % n1), i0 = (int)(v / ((long)n1 * n2));
    float p[3], xn[3];
    lattice_point(lo, hi, inv_ext2, s0[i0], s1[i1], s2[i2], p, xn);
    float acc = vm_density_lane(t, xn, q);
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (q == 0) out[v] = vm_sigma(acc, shift);
}

extern "C" int clift_dense_sigma(const clift_vm_t* h_dens, const float* h_lo3, const float* h_hi3, const float* h_inv_ext2, const float* s0,
                                 const float* s1, const float* s2, int n0, int n1, int n2, float shift, float* out, clift_stream_t s) {
    CLIFT_REQUIRE(h_dens && h_lo3 && h_hi3 && h_inv_ext2, "clift_dense_sigma: NULL host record");
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "clift_dense_sigma: comps must be a multiple of 4 (got %d)", h_dens->comps);
    CLIFT_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "clift_dense_sigma: lattice dimensions must be positive (got %d x %d x %d)", n0, n1, n2);
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(total < (1L << 36), "clift_dense_sigma: %ld lattice points, must be < 2^36", total);
    CLIFT_REQUIRE(s0 && s1 && s2 && out, "clift_dense_sigma: NULL device buffer");
    k_dense_sigma<<<cdiv(total * 4, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), make_float3(h_lo3[0], h_lo3[1], h_lo3[2]),
                                                                   make_float3(h_hi3[0], h_hi3[1], h_hi3[2]),
                                                                   make_float3(h_inv_ext2[0], h_inv_ext2[1], h_inv_ext2[2]), s0, s1, s2, n0, n1, n2, shift,
                                                                   out);
    return clift_check_launch("clift_dense_sigma");
}

// ============================================================================ marching tetrahedra on the Kuhn split
// Lattice (n0, n1, n2), x-major: lin(i, j, k) = (i n1 + j) n2 + k.  A corner of a cell is named by its offset bits dx + 2 dy + 4 dz.
// Cell (i, j, k) = 6 tetrahedra, one per permutation (a, b, c) of the axes in lexicographic order:
//     v0 = c000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = c111.
// Every tetrahedron edge runs from a lower to a higher corner with one of 7 offsets -- the edge CLASSES (1,0,0) (0,1,0) (0,0,1) (1,1,0)
// (1,0,1) (0,1,1) (1,1,1), in this order -- and is owned by its lower endpoint; neighbouring cells cut their shared face along the same
// diagonal, so the surface is face-consistent.  An edge whose endpoints classify differently (inside: vol >= level, NaN outside) carries
// one vertex, whose index is the rank of 7 lin(owner) + class among such edges: offset[owner] (an exclusive scan of the per-point
// counts, done by the caller) + the number of active classes of the owner below this one.  No atomics anywhere.
__device__ __forceinline__ int iso_class_bits(int cls) { return (0x7653421 >> (4 * cls)) & 7; }         // class -> offset bits
__device__ __forceinline__ int iso_bits_class(int bits) { return (0x65423100 >> (4 * bits)) & 7; }      // offset bits (1..7) -> class
__device__ __forceinline__ bool iso_inside(float v, float level) { return v >= level; }
__device__ __forceinline__ long iso_corner_off(int bits, int n1, int n2) {
    return (long)(bits & 1) * n1 * n2 + (long)((bits >> 1) & 1) * n2 + (long)((bits >> 2) & 1);
}
// corner bits of the 4 vertices of tetrahedron t (permutations in lexicographic order: a = t / 2, b = the t-th of 1 2 0 2 0 1)
__device__ __forceinline__ void iso_tet_corners(int t, int c[4]) {
    const int a = t >> 1, b = (0x102021 >> (4 * t)) & 3;
    c[0] = 0; c[1] = 1 << a; c[2] = c[1] | (1 << b); c[3] = 7;
}
__device__ __forceinline__ bool iso_tet_odd(int t) { return (0x26 >> t) & 1; }                          // (021) (102) (210)
__device__ __forceinline__ int iso_tet_case(int corner_mask, const int c[4]) {
    return ((corner_mask >> c[0]) & 1) | (((corner_mask >> c[1]) & 1) << 1) | (((corner_mask >> c[2]) & 1) << 2) | (((corner_mask >> c[3]) & 1) << 3);
}
// The crossed edges of a tetrahedron of an EVEN permutation as a cycle whose normal points from the inside corners to the outside ones,
// by case (bit v = corner v inside); local edges 0..5 = (v0v1, v0v2, v0v3, v1v2, v1v3, v2v3).  An odd permutation mirrors the
// tetrahedron: its cycle is this one reversed.  The winding is never taken from computed vertex positions (vertices that fall on a
// lattice point make zero-area triangles, whose geometric normal is noise).
__device__ const unsigned char ISO_POLY[16][4] = {{0, 0, 0, 0}, {0, 1, 2, 0}, {4, 3, 0, 0}, {1, 2, 4, 3}, {1, 3, 5, 0}, {3, 5, 2, 0}, {0, 4, 5, 1}, {2, 4, 5, 0},
                                                   {5, 4, 2, 0}, {0, 1, 5, 4}, {2, 5, 3, 0}, {5, 3, 1, 0}, {1, 3, 4, 2}, {0, 3, 4, 0}, {2, 1, 0, 0}, {0, 0, 0, 0}};
__device__ const unsigned char ISO_NPOLY[16] = {0, 3, 3, 4, 3, 4, 4, 3, 3, 4, 4, 3, 4, 3, 3, 0};
__device__ const unsigned char ISO_EDGE_LO[6] = {0, 0, 0, 1, 1, 2};
__device__ const unsigned char ISO_EDGE_HI[6] = {1, 2, 3, 2, 3, 3};

__device__ __forceinline__ void iso_coords(long p, int n1, int n2, int& i0, int& i1, int& i2) {
    i2 = (int)(p % n2);
    i1 = (int)((p / n2) % n1);
    i0 = (int)(p / ((long)n1 * n2));
}

// per lattice point: the 7-bit mask of its owned active edges, their number, and the triangle count of the cell it is the c000 corner of
__global__ __launch_bounds__(256) void k_iso_classify(const float* __restrict__ vol, int n0, int n1, int n2, float level, unsigned char* __restrict__ edge_mask,
                                                       int* __restrict__ n_vert, int* __restrict__ n_tri) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x, total = (long)n0 * n1 * n2;
    if (p >= total) return;
    int i0, i1, i2;
    iso_coords(p, n1, n2, i0, i1, i2);
    const bool in0 = iso_inside(vol[p], level);
    const bool has[3] = {i0 + 1 < n0, i1 + 1 < n1, i2 + 1 < n2};
    int mask = 0, corners = in0 ? 1 : 0;
#pragma unroll
    for (int cls = 0; cls < 7; ++cls) {
        const int bits = iso_class_bits(cls);
        const bool exists = (!(bits & 1) || has[0]) && (!(bits & 2) || has[1]) && (!(bits & 4) || has[2]);
        if (exists) {
            const bool in = iso_inside(vol[p + iso_corner_off(bits, n1, n2)], level);
            if (in != in0) mask |= 1 << cls;
            if (in) corners |= 1 << bits;
        }
    }
    int tris = 0;
    if (has[0] && has[1] && has[2] && corners != 0 && corners != 255) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            int c[4];
            iso_tet_corners(t, c);
            const int k = __popc(iso_tet_case(corners, c));
            tris += (k == 2) ? 2 : (k & 1);
        }
    }
    edge_mask[p] = (unsigned char)mask;
    n_vert[p] = __popc(mask);
    n_tri[p] = tris;
}

// gradient of vol at a lattice point by central differences in world units, one-sided at the border (every n_a >= 2)
__device__ __forceinline__ void iso_gradient(const float* __restrict__ vol, const float* const x[3], const int n[3], const int i[3], float g[3]) {
    const long stride[3] = {(long)n[1] * n[2], (long)n[2], 1};
    const long p = ((long)i[0] * n[1] + i[1]) * n[2] + i[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = max(i[a] - 1, 0), hi = min(i[a] + 1, n[a] - 1);
        g[a] = __fdiv_rn(__fsub_rn(vol[p + (hi - i[a]) * stride[a]], vol[p + (lo - i[a]) * stride[a]]), __fsub_rn(x[a][hi], x[a][lo]));
    }
}

// per lattice point: the vertices of its owned active edges.  p = pa + t (pb - pa), t = (level - va) / (vb - va) clamped to [0, 1], a = the
// owner; fp32, one rounding per operation (and -ffp-contract=off).  fmaxf / fminf drop a NaN: t = 0 then.
__global__ __launch_bounds__(256) void k_iso_vertices(const float* __restrict__ vol, int n0, int n1, int n2, float level, const float* __restrict__ x0,
                                                       const float* __restrict__ x1, const float* __restrict__ x2, const unsigned char* __restrict__ edge_mask,
                                                       const long* __restrict__ vert_off, long V, float* __restrict__ verts, float* __restrict__ normals) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x, total = (long)n0 * n1 * n2;
    if (p >= total) return;
    const int mask = edge_mask[p];
    if (mask == 0) return;
    const int n[3] = {n0, n1, n2};
    const float* const x[3] = {x0, x1, x2};
    int i[3];
    iso_coords(p, n1, n2, i[0], i[1], i[2]);
    const float va = vol[p];
    const float pa[3] = {x0[i[0]], x1[i[1]], x2[i[2]]};
    float ga[3] = {0.f, 0.f, 0.f};
    if (normals) iso_gradient(vol, x, n, i, ga);
    long out = vert_off[p];
    for (int cls = 0; cls < 7; ++cls) {
        if (!((mask >> cls) & 1)) continue;
        const long row = out++;
        if (row < 0 || row >= V) continue;                    // offsets that do not belong to this mask: write nothing
        const int bits = iso_class_bits(cls);
        const int d[3] = {bits & 1, (bits >> 1) & 1, (bits >> 2) & 1};
        if (i[0] + d[0] >= n0 || i[1] + d[1] >= n1 || i[2] + d[2] >= n2) continue;      // (a mask the classify pass never writes)
        const float vb = vol[p + iso_corner_off(bits, n1, n2)];
        float t = __fdiv_rn(__fsub_rn(level, va), __fsub_rn(vb, va));
        t = fminf(fmaxf(t, 0.f), 1.f);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float pb = x[a][i[a] + d[a]];
            verts[row * 3 + a] = __fadd_rn(pa[a], __fmul_rn(t, __fsub_rn(pb, pa[a])));
        }
        if (normals) {
            const int j[3] = {i[0] + d[0], i[1] + d[1], i[2] + d[2]};
            float gb[3], g[3];
            iso_gradient(vol, x, n, j, gb);
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = __fadd_rn(ga[a], __fmul_rn(t, __fsub_rn(gb[a], ga[a])));
            const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2])));
            const bool ok = isfinite(len) && len > 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) normals[row * 3 + a] = ok ? __fdiv_rn(-g[a], len) : 0.f;
        }
    }
}

// per cell, in scan order (cell, tetrahedron, triangle): 1 or 3 inside corners give one triangle, 2 give a quad, which is split along the
// diagonal through its smallest vertex index -- with the cycle rotated to start there, (q0 q1 q2) then (q0 q2 q3).
__global__ __launch_bounds__(256) void k_iso_faces(const float* __restrict__ vol, int n0, int n1, int n2, float level, const unsigned char* __restrict__ edge_mask,
                                                    const long* __restrict__ vert_off, const long* __restrict__ tri_off, long V, long F, int* __restrict__ faces) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x, total = (long)n0 * n1 * n2;
    if (p >= total) return;
    int i0, i1, i2;
    iso_coords(p, n1, n2, i0, i1, i2);
    if (i0 + 1 >= n0 || i1 + 1 >= n1 || i2 + 1 >= n2) return;
    int corners = 0;
#pragma unroll
    for (int bits = 0; bits < 8; ++bits)
        if (iso_inside(vol[p + iso_corner_off(bits, n1, n2)], level)) corners |= 1 << bits;
    if (corners == 0 || corners == 255) return;
    long out = tri_off[p];
    for (int t = 0; t < 6; ++t) {
        int c[4];
        iso_tet_corners(t, c);
        const int cs = iso_tet_case(corners, c);
        const int np = ISO_NPOLY[cs];
        if (np == 0) continue;
        const bool odd = iso_tet_odd(t);
        int q[4];
        for (int k = 0; k < np; ++k) {
            const int e = ISO_POLY[cs][odd ? np - 1 - k : k];
            const int cu = c[ISO_EDGE_LO[e]], cv = c[ISO_EDGE_HI[e]];
            const long owner = p + iso_corner_off(cu, n1, n2);
            const long id = vert_off[owner] + __popc((int)edge_mask[owner] & ((1 << iso_bits_class(cv ^ cu)) - 1));
            q[k] = (id >= 0 && id < V) ? (int)id : 0;
        }
        if (np == 3) {
            if (out >= 0 && out < F) { faces[out * 3] = q[0]; faces[out * 3 + 1] = q[1]; faces[out * 3 + 2] = q[2]; }
            ++out;
        } else {
            int m = 0;
            for (int k = 1; k < 4; ++k)
                if (q[k] < q[m]) m = k;
            const int r0 = q[m], r1 = q[(m + 1) & 3], r2 = q[(m + 2) & 3], r3 = q[(m + 3) & 3];
            if (out >= 0 && out < F) { faces[out * 3] = r0; faces[out * 3 + 1] = r1; faces[out * 3 + 2] = r2; }
            ++out;
            if (out >= 0 && out < F) { faces[out * 3] = r0; faces[out * 3 + 1] = r2; faces[out * 3 + 2] = r3; }
            ++out;
        }
    }
}

// the lattice size every iso-surface call checks before it touches the device; *total = 0 for a lattice with a dimension <= 0
static int iso_check_lattice(const char* who, int n0, int n1, int n2, long* total) {
    *total = (n0 > 0 && n1 > 0 && n2 > 0) ? (long)n0 * n1 * n2 : 0;
    CLIFT_REQUIRE(*total < CLIFT_ISO_LIMIT, "%s: %ld lattice points (%d x %d x %d), must be < 2^31", who, *total, n0, n1, n2);
    return 0;
}

extern "C" int clift_iso_classify(const float* vol, int n0, int n1, int n2, float level, unsigned char* edge_mask, int* n_vert, int* n_tri,
                                  clift_stream_t s) {
    long total;
    if (iso_check_lattice("clift_iso_classify", n0, n1, n2, &total)) return 1;
    CLIFT_REQUIRE(level == level, "clift_iso_classify: the level is NaN");
    if (n0 < 2 || n1 < 2 || n2 < 2) return 0;                // no cell: no surface, nothing written
    CLIFT_REQUIRE(vol && edge_mask && n_vert && n_tri, "clift_iso_classify: NULL device buffer");
    k_iso_classify<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(vol, n0, n1, n2, level, edge_mask, n_vert, n_tri);
    return clift_check_launch("clift_iso_classify");
}

extern "C" int clift_iso_vertices(const float* vol, int n0, int n1, int n2, float level, const float* x0, const float* x1, const float* x2,
                                  const unsigned char* edge_mask, const long* vert_off, long V, float* verts, float* normals, clift_stream_t s) {
    long total;
    if (iso_check_lattice("clift_iso_vertices", n0, n1, n2, &total)) return 1;
    CLIFT_REQUIRE(V >= 0 && V < CLIFT_ISO_LIMIT, "clift_iso_vertices: %ld vertices, must be >= 0 and < 2^31", V);
    if (n0 < 2 || n1 < 2 || n2 < 2 || V == 0) return 0;
    CLIFT_REQUIRE(vol && x0 && x1 && x2 && edge_mask && vert_off && verts, "clift_iso_vertices: NULL device buffer");
    k_iso_vertices<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(vol, n0, n1, n2, level, x0, x1, x2, edge_mask, vert_off, V, verts, normals);
    return clift_check_launch("clift_iso_vertices");
}

extern "C" int clift_iso_faces(const float* vol, int n0, int n1, int n2, float level, const unsigned char* edge_mask, const long* vert_off,
                               const long* tri_off, long V, long F, int* faces, clift_stream_t s) {
    long total;
    if (iso_check_lattice("clift_iso_faces", n0, n1, n2, &total)) return 1;
    CLIFT_REQUIRE(V >= 0 && V < CLIFT_ISO_LIMIT, "clift_iso_faces: %ld vertices, must be >= 0 and < 2^31", V);
    CLIFT_REQUIRE(F >= 0 && F < CLIFT_ISO_LIMIT, "clift_iso_faces: %ld faces, must be >= 0 and < 2^31", F);
    if (n0 < 2 || n1 < 2 || n2 < 2 || F == 0) return 0;
    CLIFT_REQUIRE(vol && edge_mask && vert_off && tri_off && faces, "clift_iso_faces: NULL device buffer");
    k_iso_faces<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(vol, n0, n1, n2, level, edge_mask, vert_off, tri_off, V, F, faces);
    return clift_check_launch("clift_iso_faces");
}
