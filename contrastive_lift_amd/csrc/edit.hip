// edit.hip -- scene-editing renders: the sampling front end with one box edit in it (delete / extract / duplicate / manipulate an instance).
// Reference: model/renderer/panopli_tensoRF_renderer.py:303-623 (forward_delete / _extract / _duplicate / _manipulate) on
// split_points_minimal (:785-797).  The render kernels recompute a sample's position from (ray, jitter, k), so a per-sample mask or a
// coordinate remap cannot be injected between them from outside: an edit render has these two kernels in their place and then runs on
// the point-wise kernels (clift_vm_products_points, clift_app_encode_points), the MLP chains and the march / compaction / compositing
// kernels unchanged.  Edits render without jitter (perturb = 0, is_train = False in the reference's four methods).  The density kernel is
// the march's own sweep body (density_sweep_dev.h) with another look-up rule, so an untouched sample has the bits of the plain pass.
// An edit PROGRAM (clift_edit_list_*) is an ordered list e_1 .. e_n of up to CLIFT_EDIT_MAX such edits in one render: scene_i is e_i applied
// to scene_{i-1}, and a sample is evaluated in scene_n by walking the list backwards (edit_walk).  The program is a by-value kernel
// argument: the records are the same for every lane, the trip count is wave-uniform and the records arrive through scalar loads.
// There is ONE kernel family, the program's: a single edit (clift_edit_density_fwd, clift_edit_active) is a program of one inside the library.
// The same walk also runs off the rays (clift_edit_list_points, clift_edit_list_dense_sigma) and, with the chain of the remaps carried beside
// the point, gives the gradient of the EDITED density for the surface outputs of an edited scene (clift_edit_list_density_grad_*, at the end).
#include "clift_dev.h"
#include "density_sweep_dev.h"
#include "lattice_dev.h"
#include "surface_dev.h"
#include <math.h>
#include <stddef.h>
CLIFT_ROWS_LIMIT_BINDER(edit)

struct BoxP {
    float A[9], c[3], lo[3], hi[3];
};
struct EditP {
    int mode;
    BoxP src, dst;
    float M[9], t[3], Dinv[9];
};

static inline BoxP to_dev(const clift_edit_box_t& b) {
    BoxP p;
    for (int i = 0; i < 9; ++i) p.A[i] = b.axes[i];
    for (int i = 0; i < 3; ++i) { p.c[i] = b.centre[i]; p.lo[i] = b.lo[i]; p.hi[i] = b.hi[i]; }
    return p;
}
static inline EditP to_dev(const clift_edit_t* e) {
    EditP p;
    p.mode = e->mode;
    p.src = to_dev(e->src);
    p.dst = to_dev(e->dst);
    for (int i = 0; i < 9; ++i) { p.M[i] = e->map_m[i]; p.Dinv[i] = e->dir_inv[i]; }
    for (int i = 0; i < 3; ++i) p.t[i] = e->map_t[i];
    return p;
}
// edit_finite walks the record as one int followed by floats only: no padding, nothing but floats after the mode
static_assert(sizeof(clift_edit_t) == sizeof(int) + 57 * sizeof(float) && offsetof(clift_edit_t, src) == sizeof(int), "clift_edit_t: int mode + 57 floats");
static bool edit_finite(const clift_edit_t* e) {
    const float* f = e->src.axes;                                       // the record is one int followed by floats only (clift.h)
    const int n = (int)((sizeof(clift_edit_t) - sizeof(int)) / sizeof(float));
    for (int i = 0; i < n; ++i)
        if (!isfinite(f[i])) return false;
    return true;
}
static int edit_check(const clift_edit_t* e, const char* who) {
    CLIFT_REQUIRE(e != nullptr, "%s: no edit record", who);
    CLIFT_REQUIRE(e->mode >= CLIFT_EDIT_DELETE && e->mode <= CLIFT_EDIT_MANIPULATE, "%s: unknown edit mode %d", who, e->mode);
    CLIFT_REQUIRE(edit_finite(e), "%s: the edit record holds a value that is not finite", who);
    return 0;
}
struct EditL {
    int n;
    EditP e[CLIFT_EDIT_MAX];
};
static_assert(sizeof(EditL) + sizeof(MarchP) + sizeof(VmP) + 64 < 4096, "the edit program travels as one kernel argument");
static int edit_list_check(const clift_edit_t* e, int n, const char* who, EditL* out) {
    CLIFT_REQUIRE(n >= 1 && n <= CLIFT_EDIT_MAX, "%s: a program holds 1 to %d edits (got n_edits = %d)", who, CLIFT_EDIT_MAX, n);
    CLIFT_REQUIRE(e != nullptr, "%s: no edit records", who);
    for (int i = 0; i < n; ++i) {
        CLIFT_REQUIRE(e[i].mode >= CLIFT_EDIT_DELETE && e[i].mode <= CLIFT_EDIT_MANIPULATE, "%s: edit %d: unknown edit mode %d", who, i, e[i].mode);
        CLIFT_REQUIRE(edit_finite(e + i), "%s: edit %d: the edit record holds a value that is not finite", who, i);
    }
    out->n = n;
    for (int i = 0; i < CLIFT_EDIT_MAX; ++i) out->e[i] = to_dev(e + (i < n ? i : 0));      // (the slots past n are never read)
    return 0;
}
// A single edit (clift_edit_density_fwd, clift_edit_active) is a program of one: the entry points keep their own checks and messages
// (edit_check) and run the list kernels.
static EditL edit_list_of_one(const clift_edit_t* e) {
    EditL L;
    L.n = 1;
    for (int i = 0; i < CLIFT_EDIT_MAX; ++i) L.e[i] = to_dev(e);
    return L;
}

// row-vector product of a row-major 3x3 with v, every multiply / add rounded separately, left to right
__device__ __forceinline__ float row3(const float* a, const float v[3]) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a[0], v[0]), __fmul_rn(a[1], v[1])), __fmul_rn(a[2], v[2]));
}
// lo <= A (p - c) <= hi, faces inclusive (a NaN coordinate is outside)
__device__ __forceinline__ bool in_box(const BoxP& b, const float p[3]) {
    const float d[3] = {__fsub_rn(p[0], b.c[0]), __fsub_rn(p[1], b.c[1]), __fsub_rn(p[2], b.c[2])};
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float q = row3(b.A + 3 * i, d);
        in = in && (b.lo[i] <= q) && (q <= b.hi[i]);
    }
    return in;
}

// One sample under an edit program, walked BACKWARDS from e_n to e_1: box classification in fp32 and the affine remap on the CURRENT point,
// every multiply and add rounded separately; a killed sample stops (sigma = 0, nothing is looked up); a sample inside edit i's destination
// box continues at M_i p + t_i with the view direction Dinv_i d.  World point and in-aabb flag come once, from the UNEDITED sample, with
// sample_xn's separately rounded ops (the reference takes mask_xyz before it remaps, :304,457,540); a sample no edit remaps keeps the bits
// of sample_xn.  L lives in the kernel-argument segment and i is wave-uniform: scalar loads, no scratch copy.
// The POINT form of the walk, shared by the ray kernels (edit_walk) and the point / lattice kernels below: p and d are walked in place.
struct EditH {
    bool kill;    // sigma = 0: some edit's kill rule named the point (p, d: where the walk stopped)
    int hops;     // how many edits remapped it (0 .. CLIFT_EDIT_MAX)
};
__device__ __forceinline__ unsigned char edit_state(const EditH& h) { return (unsigned char)(h.hops | (h.kill ? CLIFT_EDIT_STATE_KILLED : 0)); }
// ``hop(e, i)`` is called for every edit that remaps the point (i its 0-based position in the program), before p is replaced: what else
// travels with the point (the view direction, the Jacobian of the chain, the origin of a copy) is turned there.
template <class Hop>
__device__ __forceinline__ EditH edit_walk_core(const EditL& L, float p[3], Hop hop) {
    EditH h;
    h.kill = false;
    h.hops = 0;
    for (int i = L.n - 1; i >= 0; --i) {
        const EditP& e = L.e[i];
        const bool src = e.mode != CLIFT_EDIT_DUPLICATE && in_box(e.src, p);
        const bool mov = e.mode >= CLIFT_EDIT_DUPLICATE && in_box(e.dst, p);
        const bool kill = e.mode == CLIFT_EDIT_DELETE ? src : e.mode == CLIFT_EDIT_EXTRACT ? !src : e.mode == CLIFT_EDIT_MANIPULATE ? (src && !mov) : false;
        if (!h.kill && mov) {                               // (a killed sample has stopped: later tests see its last point, and change nothing)
            const float q[3] = {__fadd_rn(row3(e.M, p), e.t[0]), __fadd_rn(row3(e.M + 3, p), e.t[1]), __fadd_rn(row3(e.M + 6, p), e.t[2])};
            hop(e, i);
#pragma unroll
            for (int j = 0; j < 3; ++j) p[j] = q[j];
            ++h.hops;
        }
        h.kill = h.kill || kill;
    }
    return h;
}
__device__ __forceinline__ EditH edit_walk_point(const EditL& L, float p[3], float d[3]) {
    return edit_walk_core(L, p, [&](const EditP& e, int) {
        const float v[3] = {row3(e.Dinv, d), row3(e.Dinv + 3, d), row3(e.Dinv + 6, d)};
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = v[j];
    });
}
// The walk with the Jacobian of the chain beside the point: J (row-major 3x3) starts at the identity and becomes M_i J at
// every hop, every multiply and add rounded separately, so after the walk p' = J p + b with J = M_{i_h} ... M_{i_1}.
__device__ __forceinline__ EditH edit_walk_point_jac(const EditL& L, float p[3], float J[9]) {
#pragma unroll
    for (int j = 0; j < 9; ++j) J[j] = (j % 4 == 0) ? 1.f : 0.f;
    return edit_walk_core(L, p, [&](const EditP& e, int) {
        float N[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float col[3] = {J[c], J[3 + c], J[6 + c]};
#pragma unroll
            for (int r = 0; r < 3; ++r) N[3 * r + c] = row3(e.M + 3 * r, col);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) J[j] = N[j];
    });
}
// normalised coordinates of a walked point, every op rounded separately (sample_xn's ops)
__device__ __forceinline__ void edit_normalise(const float p[3], const float lo[3], const float inv2[3], float xn[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) xn[i] = __fsub_rn(__fmul_rn(__fsub_rn(p[i], lo[i]), inv2[i]), 1.0f);
}

struct EditW {
    bool in;      // inside the aabb (before any remap)
    bool kill;    // sigma = 0: some edit's kill rule named the sample
};
__device__ __forceinline__ EditW edit_walk(const RayG& g, const MarchP& m, const EditL& L, float z, float xn[3], float d[3]) {
    EditW s;
    float p[3];
    s.in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p[i] = __fadd_rn(g.o[i], __fmul_rn(g.d[i], z));
        s.in = s.in && !(m.lo[i] > p[i]) && !(p[i] > m.hi[i]);
        d[i] = g.d[i];
    }
    s.kill = edit_walk_point(L, p, d).kill;
    edit_normalise(p, m.lo, m.inv2, xn);
    return s;
}

// ============================================================================ density forward under an edit
// The march's own wave-per-sweep body (density_sweep, density_sweep_dev.h) with another look-up rule: no jitter, and lane = sample walks the
// program before the tap records are built from the EDITED position.  Same taps, same FMA order, same quad sum as clift_density_fwd, so a
// sample the edit neither remaps nor kills gets the very bits of the unedited pass.  A remapped point may leave the aabb: make_tap clamps
// every index and zeroes the weight of a tap outside the table (grid_sample's zero padding), as k_density_points relies on.  A killed sample
// reads no table at all.  With a remap the samples that are looked up are no prefix of the ray any more: the only early exit left is a
// sweep none of whose samples is looked up.
__global__ __launch_bounds__(64 * SWEEP_WAVES) void k_edit_list_density_fwd(MarchP m, EditL L, VmP t, const float* __restrict__ rays, int N,
                                                                            float* __restrict__ sigma) {
    density_sweep(m, t, rays, nullptr, N, sigma, [&](const RayG& g, float z, float xn[3]) {
        float d[3];
        const EditW s = edit_walk(g, m, L, z, xn, d);
        return s.in && !s.kill;
    });
}

extern "C" int clift_edit_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edit, const clift_vm_t* h_dens, const float* rays, int N,
                                      float* sigma, clift_stream_t s) {
    if (edit_check(h_edit, "clift_edit_density_fwd")) return 1;
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "clift_edit_density_fwd: comps must be a multiple of 4 (got %d)", h_dens->comps);
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_density_fwd: n_samples must be positive (got %d)", h_m->n_samples);
    if (N <= 0) return 0;
    k_edit_list_density_fwd<<<cdiv((long)N * cdiv(h_m->n_samples, 64), SWEEP_WAVES), 64 * SWEEP_WAVES, 0, as_stream(s)>>>(to_dev(h_m), edit_list_of_one(h_edit),
                                                                                                                          to_dev(h_dens), rays, N, sigma);
    return clift_check_launch("clift_edit_density_fwd");
}

extern "C" int clift_edit_list_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens,
                                           const float* rays, int N, float* sigma, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_density_fwd", &L)) return 1;
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "clift_edit_list_density_fwd: comps must be a multiple of 4 (got %d)", h_dens->comps);
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_list_density_fwd: n_samples must be positive (got %d)", h_m->n_samples);
    if (N <= 0) return 0;
    k_edit_list_density_fwd<<<cdiv((long)N * cdiv(h_m->n_samples, 64), SWEEP_WAVES), 64 * SWEEP_WAVES, 0, as_stream(s)>>>(to_dev(h_m), L, to_dev(h_dens),
                                                                                                                          rays, N, sigma);
    return clift_check_launch("clift_edit_list_density_fwd");
}

// ============================================================================ positions and view directions of the active samples
// The same classification, recomputed (not stored: (N, S) flags would cost more traffic than the few dozen ops).  xa feeds the xyz heads and
// clift_vm_products_points, dirs feeds clift_app_encode_points.
// Row s of the active list: its ray, and the UNEDITED world point of its sample (no jitter) with sample_xn's separately rounded ops.
__device__ __forceinline__ RayG edit_active_point(const MarchP& m, const float* __restrict__ rays, const int* __restrict__ act, long s, float p[3]) {
    const int sid = act[s];
    const int r = sid / m.S, k = sid - r * m.S;
    const RayG g = load_ray(rays, r, m);
    const float z = sample_z(g, m, k, 0.f);
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = __fadd_rn(g.o[i], __fmul_rn(g.d[i], z));
    return g;
}

// The walk recomputed, the view direction turned by every edit that remapped the sample
__global__ __launch_bounds__(256) void k_edit_list_active(MarchP m, EditL L, const float* __restrict__ rays, const int* __restrict__ act, int M,
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

extern "C" int clift_edit_active(const clift_march_t* h_m, const clift_edit_t* h_edit, const float* rays, const int* act_idx, int M, float* xa,
                                 float* dirs, clift_stream_t s) {
    if (edit_check(h_edit, "clift_edit_active")) return 1;
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_active: n_samples must be positive (got %d)", h_m->n_samples);
    CLIFT_REQUIRE(xa != nullptr && dirs != nullptr, "clift_edit_active: xa and dirs are both written");
    if (M <= 0) return 0;
    k_edit_list_active<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), edit_list_of_one(h_edit), rays, act_idx, M, xa, dirs);
    return clift_check_launch("clift_edit_active");
}

extern "C" int clift_edit_list_active(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const float* rays, const int* act_idx, int M,
                                      float* xa, float* dirs, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_active", &L)) return 1;
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_list_active: n_samples must be positive (got %d)", h_m->n_samples);
    CLIFT_REQUIRE(xa != nullptr && dirs != nullptr, "clift_edit_list_active: xa and dirs are both written");
    if (M <= 0) return 0;
    k_edit_list_active<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), L, rays, act_idx, M, xa, dirs);
    return clift_check_launch("clift_edit_list_active");
}

// k_edit_list_active with the ORIGIN of the content beside the position: the 1-based position of the first edit the backward
// walk meets that remaps the sample and is a DUPLICATE -- the last-applied copy in whose destination the sample sits -- or 0.  A later move
// of the copy remaps the sample first and the walk goes on to the copy: the origin stays.  A killed sample has stopped and keeps what it
// had.  No view direction is turned (no appearance chain follows); the point is walked with the ops of edit_walk, so xa has its bits.
__global__ __launch_bounds__(256) void k_edit_list_active_origin(MarchP m, EditL L, const float* __restrict__ rays, const int* __restrict__ act,
                                                                  int M, float* __restrict__ xa, unsigned char* __restrict__ origin,
                                                                  unsigned char* __restrict__ state) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= limit_rows(M)) return;
    float p[3], xn[3];
    edit_active_point(m, rays, act, s, p);
    int org = 0;
    const EditH h = edit_walk_core(L, p, [&](const EditP& e, int i) {
        if (org == 0 && e.mode == CLIFT_EDIT_DUPLICATE) org = i + 1;
    });
    edit_normalise(p, m.lo, m.inv2, xn);
    *reinterpret_cast<float4*>(xa + (size_t)s * 4) = make_float4(xn[0], xn[1], xn[2], 0.f);
    origin[s] = (unsigned char)org;
    if (state != nullptr) state[s] = edit_state(h);
}

extern "C" int clift_edit_list_active_origin(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const float* rays,
                                             const int* act_idx, int M, float* xa, unsigned char* origin, unsigned char* state, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_active_origin", &L)) return 1;
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_list_active_origin: n_samples must be positive (got %d)", h_m->n_samples);
    CLIFT_REQUIRE(xa != nullptr && origin != nullptr, "clift_edit_list_active_origin: xa and origin are both written (NULL given)");
    if (M <= 0) return 0;
    k_edit_list_active_origin<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), L, rays, act_idx, M, xa, origin, state);
    return clift_check_launch("clift_edit_list_active_origin");
}

// ============================================================================ the walk over arbitrary points
// One thread per row: world point (and view direction) in, the point (and direction) at which the field is to be looked up out, plus the
// state byte.  No aabb test and no table: what "inside the scene" means is the caller's business (mesh.label_vertices, the lattice below).
// A row no edit remaps is copied through untouched, so it keeps its input bits.  in == out is allowed (a thread reads its row, then writes it).
__global__ __launch_bounds__(256) void k_edit_list_points(EditL L, const float* pts, int ldp, const float* dirs, int ldd, long n, float* out_pts,
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

extern "C" int clift_edit_list_points(const clift_edit_t* h_edits, int n_edits, const float* pts, int ldp, const float* dirs, int ldd, long n,
                                      float* out_pts, float* out_dirs, unsigned char* state, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_points", &L)) return 1;
    CLIFT_REQUIRE(ldp >= 3 && (dirs == nullptr || ldd >= 3), "clift_edit_list_points: ldp and ldd must be >= 3 (got %d, %d)", ldp, ldd);
    CLIFT_REQUIRE(n >= 0 && n < (1L << 36), "clift_edit_list_points: %ld rows, must be in [0, 2^36)", n);
    if (n == 0) return 0;
    CLIFT_REQUIRE(pts != nullptr && out_pts != nullptr, "clift_edit_list_points: NULL pts or out_pts");
    CLIFT_REQUIRE((dirs == nullptr) == (out_dirs == nullptr), "clift_edit_list_points: dirs and out_dirs come together (both or neither NULL)");
    k_edit_list_points<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(L, pts, ldp, dirs, ldd, n, out_pts, out_dirs, state);
    return clift_check_launch("clift_edit_list_points");
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
__global__ __launch_bounds__(256) void k_edit_list_dense_sigma(VmP t, EditL L, float3 lo, float3 hi, float3 inv_ext2, const float* __restrict__ s0,
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

extern "C" int clift_edit_list_dense_sigma(const clift_vm_t* h_dens, const clift_edit_t* h_edits, int n_edits, const float* h_lo3, const float* h_hi3,
                                           const float* h_inv_ext2, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2,
                                           float shift, float* out, unsigned char* state, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_dense_sigma", &L)) return 1;
    CLIFT_REQUIRE(h_dens && h_lo3 && h_hi3 && h_inv_ext2, "clift_edit_list_dense_sigma: NULL host record");
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "clift_edit_list_dense_sigma: comps must be a multiple of 4 (got %d)", h_dens->comps);
    CLIFT_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "clift_edit_list_dense_sigma: lattice dimensions must be positive (got %d x %d x %d)", n0, n1, n2);
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(total < (1L << 36), "clift_edit_list_dense_sigma: %ld lattice points, must be < 2^36", total);
    CLIFT_REQUIRE(s0 && s1 && s2 && out, "clift_edit_list_dense_sigma: NULL device buffer");
    k_edit_list_dense_sigma<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), L, make_float3(h_lo3[0], h_lo3[1], h_lo3[2]),
                                                                        make_float3(h_hi3[0], h_hi3[1], h_hi3[2]),
                                                                        make_float3(h_inv_ext2[0], h_inv_ext2[1], h_inv_ext2[2]), s0, s1, s2, n0, n1,
                                                                        n2, shift, out, state);
    return clift_check_launch("clift_edit_list_dense_sigma");
}

// ============================================================================ gradient of the edited density
// sigma_e(p) = sigma_raw(p') with p' = J p + b the point the walk ends at, so grad sigma_e(p) = J^T g', g' the world gradient of the unedited
// field at p' (k_density_grad_points with its inv2 scaling).  The two mappings of k_edit_list_dense_sigma: for the walk lane = point (each of
// the wave's 64 points walked ONCE, J carried beside p), for the taps four passes of 16 points x 4 lanes in the lane roles of
// k_density_grad_points (vm_density_grad_quad, the shared body), the quad fetching xn, J and the hop count of its point by __shfl at the top
// of its pass -- registers only, no LDS.  The quad leader forms J^T g' row by row of J^T, every op rounded separately, left to right; a row
// no edit remapped stores g' itself, so it carries all four columns of clift_density_grad_points bit for bit.  A killed point reads no table
// and gets a row of zeros; a pass none of whose 16 points is alive is skipped.  One writer per element, no atomics.
__device__ __forceinline__ void edit_density_grad_wave(const VmP& t, const EditL& L, float p[3], bool valid, const float lo[3], const float inv2[3],
                                                       float shift, long base, long total, float* __restrict__ out,
                                                       unsigned char* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    float J[9], xn[3];
    const EditH h = edit_walk_point_jac(L, p, J);
    edit_normalise(p, lo, inv2, xn);
    if (valid && state != nullptr) state[base + lane] = edit_state(h);
    const unsigned long long on = __ballot(valid && !h.kill);
    if (on == 0) {                                                   // wave-uniform: nothing of this wave is looked up
        if (valid) *reinterpret_cast<float4*>(out + (size_t)(base + lane) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int q = lane & 3;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int sl = pass * 16 + (lane >> 2);
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((on >> (pass * 16)) & 0xffffull) {                       // wave-uniform: some point of this pass is looked up
            const float xq[3] = {__shfl(xn[0], sl), __shfl(xn[1], sl), __shfl(xn[2], sl)};
            float Jq[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) Jq[j] = __shfl(J[j], sl);
            const int hq = __shfl(h.hops, sl);
            const bool mine = (on >> sl) & 1ull;
            float acc, g[3];
            vm_density_grad_quad(t, xq, q, mine, acc, g);
            if (mine) {
                const float gw[3] = {g[0] * inv2[0], g[1] * inv2[1], g[2] * inv2[2]};
                row = make_float4(gw[0], gw[1], gw[2], acc + shift);
                if (hq > 0) {                                        // J^T g': column c of J against g'
                    row.x = __fadd_rn(__fadd_rn(__fmul_rn(Jq[0], gw[0]), __fmul_rn(Jq[3], gw[1])), __fmul_rn(Jq[6], gw[2]));
                    row.y = __fadd_rn(__fadd_rn(__fmul_rn(Jq[1], gw[0]), __fmul_rn(Jq[4], gw[1])), __fmul_rn(Jq[7], gw[2]));
                    row.z = __fadd_rn(__fadd_rn(__fmul_rn(Jq[2], gw[0]), __fmul_rn(Jq[5], gw[1])), __fmul_rn(Jq[8], gw[2]));
                }
            }
        }
        if (q == 0 && base + sl < total) *reinterpret_cast<float4*>(out + (size_t)(base + sl) * 4) = row;
    }
}

__global__ __launch_bounds__(256) void k_edit_list_density_grad_points(VmP t, EditL L, const float* __restrict__ pts, int ldp, long n, float3 lo,
                                                                        float3 inv2, float shift, float* __restrict__ out,
                                                                        unsigned char* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long base = v - lane;                                      // the wave's first row
    if (base >= n) return;                                           // wave-uniform
    const bool valid = v < n;
    const long vc = valid ? v : n - 1;                               // (the tail lanes walk the last point again: no divergence around the loop)
    const float* pi = pts + (size_t)vc * ldp;
    float p[3] = {pi[0], pi[1], pi[2]};
    const float l3[3] = {lo.x, lo.y, lo.z}, inv3[3] = {inv2.x, inv2.y, inv2.z};
    edit_density_grad_wave(t, L, p, valid, l3, inv3, shift, base, n, out, state);
}

// ... at the active samples of a march: the point of row s from (rays, act_idx[s]) with the very operations of k_edit_list_active
__global__ __launch_bounds__(256) void k_edit_list_density_grad_active(MarchP m, EditL L, VmP t, const float* __restrict__ rays,
                                                                        const int* __restrict__ act, int M, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long total = limit_rows(M);
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long base = v - lane;
    if (base >= total) return;                                       // wave-uniform
    const bool valid = v < total;
    float p[3];
    edit_active_point(m, rays, act, valid ? v : total - 1, p);
    edit_density_grad_wave(t, L, p, valid, m.lo, m.inv2, m.shift, base, total, out, nullptr);
}

static int edit_grad_table_check(const clift_vm_t* h_dens, const char* who) {
    CLIFT_REQUIRE(h_dens != nullptr, "%s: NULL table record", who);
    CLIFT_REQUIRE(h_dens->comps > 0 && h_dens->comps % 4 == 0, "%s: comps must be a positive multiple of 4 (got %d)", who, h_dens->comps);
    CLIFT_REQUIRE(h_dens->res[0] >= 1 && h_dens->res[1] >= 1 && h_dens->res[2] >= 1, "%s: table sizes must be positive", who);
    return 0;
}

extern "C" int clift_edit_list_density_grad_points(const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens, const float* pts, int ldp,
                                                   long n, const float* h_lo3, const float* h_inv2, float shift, float* out,
                                                   unsigned char* state, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_density_grad_points", &L)) return 1;
    if (edit_grad_table_check(h_dens, "clift_edit_list_density_grad_points")) return 1;
    CLIFT_REQUIRE(h_lo3 != nullptr && h_inv2 != nullptr, "clift_edit_list_density_grad_points: NULL lo / inv2");
    CLIFT_REQUIRE(ldp >= 3, "clift_edit_list_density_grad_points: ldp must be >= 3 (got %d)", ldp);
    CLIFT_REQUIRE(n >= 0 && n < (1L << 36), "clift_edit_list_density_grad_points: %ld rows, must be in [0, 2^36)", n);
    if (n == 0) return 0;
    CLIFT_REQUIRE(pts != nullptr && out != nullptr, "clift_edit_list_density_grad_points: NULL pts or out");
    k_edit_list_density_grad_points<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), L, pts, ldp, n, make_float3(h_lo3[0], h_lo3[1], h_lo3[2]),
                                                                            make_float3(h_inv2[0], h_inv2[1], h_inv2[2]), shift, out, state);
    return clift_check_launch("clift_edit_list_density_grad_points");
}

extern "C" int clift_edit_list_density_grad_active(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens,
                                                   const float* rays, const int* act_idx, int M, float* out, clift_stream_t s) {
    EditL L;
    if (edit_list_check(h_edits, n_edits, "clift_edit_list_density_grad_active", &L)) return 1;
    if (edit_grad_table_check(h_dens, "clift_edit_list_density_grad_active")) return 1;
    CLIFT_REQUIRE(h_m != nullptr, "clift_edit_list_density_grad_active: NULL march record");
    CLIFT_REQUIRE(h_m->n_samples > 0, "clift_edit_list_density_grad_active: n_samples must be positive (got %d)", h_m->n_samples);
    if (M <= 0) return 0;
    CLIFT_REQUIRE(rays != nullptr && act_idx != nullptr && out != nullptr, "clift_edit_list_density_grad_active: NULL rays, act_idx or out");
    k_edit_list_density_grad_active<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), L, to_dev(h_dens), rays, act_idx, M, out);
    return clift_check_launch("clift_edit_list_density_grad_active");
}
