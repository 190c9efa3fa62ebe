// edit_kernels_dev.h -- the four walk kernels of edit.hip, written ONCE and compiled twice: edit.hip includes this file with
//   EDIT_PROG = EditL,  EDIT_K(x) = k_edit_list_##x      the plain program (box edits)
//   EDIT_PROG = EditLS, EDIT_K(x) = k_edit_shaped_##x    the program with shape records
// No include guard, on purpose.  The kernels are spelled out against the program type rather than being wrappers around a templated body: a
// wrapper changed register allocation and block order of the plain kernels, and those must stay the instruction stream they were (the walk
// itself is a template on the program type, edit_walk_core; with EditL the shaped branch is not compiled).

// ============================================================================ density forward under an edit
// The march's own wave-per-sweep body (density_sweep, density_sweep_dev.h) with another look-up rule: no jitter, and lane = sample walks the
// program before the tap records are built from the EDITED position.  Same taps, same FMA order, same quad sum as clift_density_fwd, so a
// sample the edit neither remaps nor kills gets the very bits of the unedited pass.  A remapped point may leave the aabb: make_tap clamps
// every index and zeroes the weight of a tap outside the table (grid_sample's zero padding), as k_density_points relies on.  A killed sample
// reads no table at all.  With a remap the samples that are looked up are no prefix of the ray any more: the only early exit left is a
// sweep none of whose samples is looked up.
__global__ __launch_bounds__(64 * SWEEP_WAVES) void EDIT_K(density_fwd)(MarchP m, EDIT_PROG L, VmP t, const float* __restrict__ rays, int N,
                                                                        float* __restrict__ sigma) {
    density_sweep(m, t, rays, nullptr, N, sigma, [&](const RayG& g, float z, float xn[3]) {
        float d[3];
        const EditW s = edit_walk(g, m, L, z, xn, d);
        return s.in && !s.kill;
    });
}

// ============================================================================ positions and view directions of the active samples
// The same classification, recomputed (not stored: (N, S) flags would cost more traffic than the few dozen ops).  xa feeds the xyz heads and
// clift_vm_products_points, dirs feeds clift_app_encode_points.
// The walk recomputed, the view direction turned by every edit that remapped the sample
__global__ __launch_bounds__(256) void EDIT_K(active)(MarchP m, EDIT_PROG L, const float* __restrict__ rays, const int* __restrict__ act, int M,
                                                       float* __restrict__ xa, float* __restrict__ dirs) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= limit_rows(M)) return;
    float p[3], xn[3];
    const RayG g = edit_active_point(m, rays, act, s, p);
    float d[3] = {g.d[0], g.d[1], g.d[2]};
    edit_walk_point(L, p, d);
    edit_normalise(p, m.lo, m.inv2, xn);
    *reinterpret_cast<float4*>(xa + (size_t)s * 4) = make_float4(xn[0], xn[1], xn[2], 0.f);
    *reinterpret_cast<float4*>(dirs + (size_t)s * 4) = make_float4(d[0], d[1], d[2], 0.f);
}

// ============================================================================ the walk over arbitrary points
// One thread per row: world point (and view direction) in, the point (and direction) at which the field is to be looked up out, plus the
// state byte.  No aabb test and no table: what "inside the scene" means is the caller's business (mesh.label_vertices, the lattice below).
// A row no edit remaps is copied through untouched, so it keeps its input bits.  in == out is allowed (a thread reads its row, then writes it).
__global__ __launch_bounds__(256) void EDIT_K(points)(EDIT_PROG L, const float* pts, int ldp, const float* dirs, int ldd, long n, float* out_pts,
                                                       float* out_dirs, unsigned char* state) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float* pi = pts + (size_t)r * ldp;
    float p[3] = {pi[0], pi[1], pi[2]}, d[3] = {0.f, 0.f, 0.f};
    if (dirs != nullptr) {
        const float* di = dirs + (size_t)r * ldd;
        d[0] = di[0]; d[1] = di[1]; d[2] = di[2];
    }
    const EditH h = edit_walk_point(L, p, d);
    float* po = out_pts + (size_t)r * ldp;
    po[0] = p[0]; po[1] = p[1]; po[2] = p[2];
    if (dirs != nullptr) {
        float* dout = out_dirs + (size_t)r * ldd;
        dout[0] = d[0]; dout[1] = d[1]; dout[2] = d[2];
    }
    if (state != nullptr) state[r] = edit_state(h);
}

// ============================================================================ sigma on the lattice of the edited scene
// clift_dense_sigma (isosurface.hip) with the program in it, one launch.  k_dense_sigma gives 4 lanes to a lattice point for the 18 table
// reads; the walk is a few hundred VALU ops per point at 8 edits and would be done four times over if every lane of the quad walked.  So
// the two phases use two mappings of one wave's 64 points: for the walk lane = point (lattice_point, then edit_walk_point, each done ONCE
// per point), and for the taps four passes of 16 points x 4 lanes, as in density_sweep, the quad fetching its point's normalised
// position from the lane that walked it by __shfl -- registers only, no LDS.  The records arrive by scalar loads (L is a kernel
// argument, the trip count is wave-uniform).  A killed point reads no table and gets exactly 0; a pass none of whose 16 points is alive
// is skipped, and a wave all of whose points are killed leaves after the walk.  A point no edit remaps keeps the xn of lattice_point
// and goes through vm_density_lane / vm_sigma in k_dense_sigma's lane roles: the bits of clift_dense_sigma.  A remapped point is
// normalised with edit_walk's separately rounded ops; outside the box it reads zero padding (make_tap).  No atomics.
__global__ __launch_bounds__(256) void EDIT_K(dense_sigma)(VmP t, EDIT_PROG L, float3 lo, float3 hi, float3 inv_ext2, const float* __restrict__ s0,
                                                            const float* __restrict__ s1, const float* __restrict__ s2, int n0, int n1, int n2,
                                                            float shift, float* __restrict__ out, unsigned char* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const long total = (long)n0 * n1 * n2;
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long base = v - lane;                                      // the wave's first point (< total: the grid is cdiv(total, 256) and 256 = 4 waves)
    if (base >= total) return;                                       // wave-uniform
    const bool valid = v < total;
    const long vc = valid ? v : total - 1;                           // (the tail lanes walk the last point again: no divergence around the loop)
    const int i2 = (int)(vc % n2), i1 = (int)((vc / n2) % n1), i0 = (int)(vc / ((long)n1 * n2));
    float p[3], xn[3], d[3] = {0.f, 0.f, 0.f};
    lattice_point(lo, hi, inv_ext2, s0[i0], s1[i1], s2[i2], p, xn);
    const EditH h = edit_walk_point(L, p, d);
    if (h.hops > 0) {
        const float l3[3] = {lo.x, lo.y, lo.z}, inv3[3] = {inv_ext2.x, inv_ext2.y, inv_ext2.z};
        edit_normalise(p, l3, inv3, xn);
    }
    if (valid && state != nullptr) state[v] = edit_state(h);
    const unsigned long long on = __ballot(valid && !h.kill);
    if (on == 0) {                                                   // wave-uniform: nothing of this wave is looked up
        if (valid) out[v] = 0.f;
        return;
    }
    const int q = lane & 3;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int sl = pass * 16 + (lane >> 2);
        float sig = 0.f;
        if ((on >> (pass * 16)) & 0xffffull) {                       // wave-uniform: some point of this pass is looked up
            const float xq[3] = {__shfl(xn[0], sl), __shfl(xn[1], sl), __shfl(xn[2], sl)};
            const bool mine = (on >> sl) & 1ull;
            float acc = mine ? vm_density_lane(t, xq, q) : 0.f;
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (mine) sig = vm_sigma(acc, shift);
        }
        if (q == 0 && base + sl < total) out[base + sl] = sig;
    }
}
