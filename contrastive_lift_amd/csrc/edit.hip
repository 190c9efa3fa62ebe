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
// An edit may also carry a SHAPE, a bit lattice over its source box (clift_edit_shaped_*, clift_shape_pack): the four walk
// kernels live in edit_kernels_dev.h and are compiled twice, for the plain program (k_edit_list_*) and for the shaped one (k_edit_shaped_*).
// Layout of the host side: the program's own checks (edit_check, edit_list_check, edit_shapes_check), then per walk kernel ONE checked
// body that every tier of entry points calls -- the single edit, the list and the shaped program are thin wrappers that differ in how the
// program is resolved ("the entry points over the walk kernels"); the untwinned entry points (active_origin, shape_pack, density_grad_*)
// follow with their kernels.
#include "clift_dev.h"
#include "density_sweep_dev.h"
#include "lattice_dev.h"
#include "surface_dev.h"
#include <math.h>
#include <stddef.h>
#include <type_traits>
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

// ---- shaped edits: an edit may carry a bit lattice over its SOURCE box (clift_edit_shape_t); a point is part of the edit only
// where its cell's bit is set.  The shaped program is the plain one plus CLIFT_EDIT_MAX shape records, the same by-value kernel argument:
// pointer, dims and cell scale are wave-uniform and arrive by scalar loads; only the word read is a per-lane load.  The kernels of the plain
// program take EditL and never see this: their code is what it was.
struct ShapeP {
    const unsigned int* w;     // NULL: this edit has no shape (the box rule)
    int G[3];
    float inv[3];
};
struct EditLS {
    EditL L;
    ShapeP sh[CLIFT_EDIT_MAX];
};
static_assert(sizeof(EditLS) + sizeof(MarchP) + sizeof(VmP) + 64 < 4096, "the shaped edit program travels as one kernel argument");
// h_shapes == NULL is the plain program (*shaped = false, out->sh untouched); else n records, each checked before anything is launched
static int edit_shapes_check(const clift_edit_t* e, const clift_edit_shape_t* h, int n, const char* who, EditLS* out, bool* shaped) {
    if (edit_list_check(e, n, who, &out->L)) return 1;
    *shaped = h != nullptr;
    if (h == nullptr) return 0;
    for (int i = 0; i < n; ++i) {
        if (h[i].words == nullptr) continue;
        for (int a = 0; a < 3; ++a)
            CLIFT_REQUIRE(h[i].dims[a] >= 1 && h[i].dims[a] <= CLIFT_SHAPE_DIM_MAX, "%s: edit %d: shape dimension %d is %d, must be in 1 .. %d", who, i, a,
                          h[i].dims[a], CLIFT_SHAPE_DIM_MAX);
        CLIFT_REQUIRE((long)h[i].dims[0] * h[i].dims[1] * h[i].dims[2] < (1L << 31), "%s: edit %d: the shape has %ld cells, must be < 2^31", who, i,
                      (long)h[i].dims[0] * h[i].dims[1] * h[i].dims[2]);
        for (int a = 0; a < 3; ++a)
            CLIFT_REQUIRE(isfinite(h[i].inv_cell[a]) && h[i].inv_cell[a] > 0.f, "%s: edit %d: shape inv_cell[%d] must be finite and positive", who, i, a);
    }
    for (int i = 0; i < CLIFT_EDIT_MAX; ++i) {
        const clift_edit_shape_t& r = h[i < n ? i : 0];                         // (the slots past n are never read)
        ShapeP& d = out->sh[i];
        d.w = r.words;
        for (int a = 0; a < 3; ++a) { d.G[a] = r.words ? r.dims[a] : 1; d.inv[a] = r.words ? r.inv_cell[a] : 1.f; }
    }
    return 0;
}
__device__ __forceinline__ const EditL& edits_of(const EditL& L) { return L; }
__device__ __forceinline__ const EditL& edits_of(const EditLS& L) { return L.L; }

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

// The bit of world point x in the lattice over box b (the edit's SOURCE box): cell index per axis from (A (x - c) - lo) * inv, every op rounded
// on its own, floored and CLAMPED to 0 .. G - 1 (in float first: a NaN or an overflow ends at a border cell, never outside the words), then
// bit lin & 31 of word lin >> 5, lin = (i0 G1 + i1) G2 + i2 < 2^31.  An ordinary per-lane global load.
__device__ __forceinline__ bool shape_bit(const ShapeP& s, const BoxP& b, const float x[3]) {
    const float d[3] = {__fsub_rn(x[0], b.c[0]), __fsub_rn(x[1], b.c[1]), __fsub_rn(x[2], b.c[2])};
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = __fmul_rn(__fsub_rn(row3(b.A + 3 * a, d), b.lo[a]), s.inv[a]);
        idx[a] = (int)fminf(fmaxf(floorf(u), 0.f), (float)(s.G[a] - 1));
    }
    const unsigned int lin = ((unsigned int)idx[0] * (unsigned int)s.G[1] + (unsigned int)idx[1]) * (unsigned int)s.G[2] + (unsigned int)idx[2];
    return (s.w[lin >> 5] >> (lin & 31u)) & 1u;
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
// SHAPED (the program is an EditLS): an edit whose shape has words narrows both tests by its lattice -- src also needs the bit of p, mov
// the bit of the remapped point M p + t, both read in the SOURCE frame, and only by lanes already inside the box.  Whether edit i has words
// is wave-uniform.  The remapped point is formed with the ops of the hop below, so the hop's q is the one that was tested.
template <class Prog, class Hop>
__device__ __forceinline__ EditH edit_walk_core(const Prog& P, float p[3], Hop hop) {
    constexpr bool SHAPED = std::is_same<Prog, EditLS>::value;
    const EditL& L = edits_of(P);
    EditH h;
    h.kill = false;
    h.hops = 0;
    for (int i = L.n - 1; i >= 0; --i) {
        const EditP& e = L.e[i];
        bool src = e.mode != CLIFT_EDIT_DUPLICATE && in_box(e.src, p);
        bool mov = e.mode >= CLIFT_EDIT_DUPLICATE && in_box(e.dst, p);
        if constexpr (SHAPED) {
            const ShapeP& sh = P.sh[i];
            if (sh.w != nullptr) {                          // wave-uniform
                if (src) src = shape_bit(sh, e.src, p);
                if (mov) {
                    const float q[3] = {__fadd_rn(row3(e.M, p), e.t[0]), __fadd_rn(row3(e.M + 3, p), e.t[1]), __fadd_rn(row3(e.M + 6, p), e.t[2])};
                    mov = shape_bit(sh, e.src, q);
                }
            }
        }
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
template <class Prog>
__device__ __forceinline__ EditH edit_walk_point(const Prog& L, float p[3], float d[3]) {
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
template <class Prog>
__device__ __forceinline__ EditW edit_walk(const RayG& g, const MarchP& m, const Prog& L, float z, float xn[3], float d[3]) {
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

// ============================================================================ the walk kernels, per program type
// edit_kernels_dev.h holds k_edit_*_density_fwd, _active, _points and _dense_sigma, written once: compiled here for the plain program
// (k_edit_list_*: the instruction stream these kernels had before shapes existed) and for the shaped one (k_edit_shaped_*).
#define EDIT_PROG EditL
#define EDIT_K(x) k_edit_list_##x
#include "edit_kernels_dev.h"
#undef EDIT_PROG
#undef EDIT_K
#define EDIT_PROG EditLS
#define EDIT_K(x) k_edit_shaped_##x
#include "edit_kernels_dev.h"
#undef EDIT_PROG
#undef EDIT_K

// ============================================================================ the entry points over the walk kernels
// One checked host body per walk kernel (edit_density_fwd, edit_active, edit_points, edit_dense_sigma): it takes the public name (``who``:
// every message starts with it, and clift_check_launch reports under it), the program as its own check resolved it -- an EditLS and whether
// it is shaped -- and the rest of the arguments; it holds every check that follows the program's own, the early return and the launch:
// k_edit_shaped_* with the whole program when it is shaped, k_edit_list_* with its edits alone (an EditL) when it is not.  The public
// functions differ only in how they resolve the program: clift_edit_shaped_* by edit_shapes_check(h_edits, h_shapes), clift_edit_list_* by
// the same with no shapes (clift.h: "h_shapes == NULL gives the list entry point's behaviour"), the two single-edit names by edit_check
// and edit_list_of_one, with their own wording.  A check added to a body holds for every tier.
static inline float3 f3_of(const float* h) { return make_float3(h[0], h[1], h[2]); }

// ---- density forward under a program (the kernel: edit_kernels_dev.h)
static int edit_density_fwd(const char* who, const EditLS& P, bool shaped, const clift_march_t* h_m, const clift_vm_t* h_dens, const float* rays,
                            int N, float* sigma, clift_stream_t s) {
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "%s: comps must be a multiple of 4 (got %d)", who, h_dens->comps);
    CLIFT_REQUIRE(h_m->n_samples > 0, "%s: n_samples must be positive (got %d)", who, h_m->n_samples);
    if (N <= 0) return 0;
    const dim3 grid(cdiv((long)N * cdiv(h_m->n_samples, 64), SWEEP_WAVES)), block(64 * SWEEP_WAVES);
    if (shaped)
        k_edit_shaped_density_fwd<<<grid, block, 0, as_stream(s)>>>(to_dev(h_m), P, to_dev(h_dens), rays, N, sigma);
    else
        k_edit_list_density_fwd<<<grid, block, 0, as_stream(s)>>>(to_dev(h_m), P.L, to_dev(h_dens), rays, N, sigma);
    return clift_check_launch(who);
}

extern "C" int clift_edit_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edit, const clift_vm_t* h_dens, const float* rays, int N,
                                      float* sigma, clift_stream_t s) {
    if (edit_check(h_edit, "clift_edit_density_fwd")) return 1;
    EditLS P;
    P.L = edit_list_of_one(h_edit);
    return edit_density_fwd("clift_edit_density_fwd", P, false, h_m, h_dens, rays, N, sigma, s);
}

extern "C" int clift_edit_list_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens,
                                           const float* rays, int N, float* sigma, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, nullptr, n_edits, "clift_edit_list_density_fwd", &P, &shaped)) return 1;
    return edit_density_fwd("clift_edit_list_density_fwd", P, shaped, h_m, h_dens, rays, N, sigma, s);
}

extern "C" int clift_edit_shaped_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                                             const clift_vm_t* h_dens, const float* rays, int N, float* sigma, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, h_shapes, n_edits, "clift_edit_shaped_density_fwd", &P, &shaped)) return 1;
    return edit_density_fwd("clift_edit_shaped_density_fwd", P, shaped, h_m, h_dens, rays, N, sigma, s);
}

// ---- positions and view directions of the active samples
static int edit_active(const char* who, const EditLS& P, bool shaped, const clift_march_t* h_m, const float* rays, const int* act_idx, int M,
                       float* xa, float* dirs, clift_stream_t s) {
    CLIFT_REQUIRE(h_m->n_samples > 0, "%s: n_samples must be positive (got %d)", who, h_m->n_samples);
    CLIFT_REQUIRE(xa != nullptr && dirs != nullptr, "%s: xa and dirs are both written", who);
    if (M <= 0) return 0;
    if (shaped)
        k_edit_shaped_active<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), P, rays, act_idx, M, xa, dirs);
    else
        k_edit_list_active<<<cdiv(M, 256), 256, 0, as_stream(s)>>>(to_dev(h_m), P.L, rays, act_idx, M, xa, dirs);
    return clift_check_launch(who);
}

extern "C" int clift_edit_active(const clift_march_t* h_m, const clift_edit_t* h_edit, const float* rays, const int* act_idx, int M, float* xa,
                                 float* dirs, clift_stream_t s) {
    if (edit_check(h_edit, "clift_edit_active")) return 1;
    EditLS P;
    P.L = edit_list_of_one(h_edit);
    return edit_active("clift_edit_active", P, false, h_m, rays, act_idx, M, xa, dirs, s);
}

extern "C" int clift_edit_list_active(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const float* rays, const int* act_idx, int M,
                                      float* xa, float* dirs, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, nullptr, n_edits, "clift_edit_list_active", &P, &shaped)) return 1;
    return edit_active("clift_edit_list_active", P, shaped, h_m, rays, act_idx, M, xa, dirs, s);
}

extern "C" int clift_edit_shaped_active(const clift_march_t* h_m, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                                        const float* rays, const int* act_idx, int M, float* xa, float* dirs, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, h_shapes, n_edits, "clift_edit_shaped_active", &P, &shaped)) return 1;
    return edit_active("clift_edit_shaped_active", P, shaped, h_m, rays, act_idx, M, xa, dirs, s);
}

// ---- the walk over arbitrary points
static int edit_points(const char* who, const EditLS& P, bool shaped, const float* pts, int ldp, const float* dirs, int ldd, long n, float* out_pts,
                       float* out_dirs, unsigned char* state, clift_stream_t s) {
    CLIFT_REQUIRE(ldp >= 3 && (dirs == nullptr || ldd >= 3), "%s: ldp and ldd must be >= 3 (got %d, %d)", who, ldp, ldd);
    CLIFT_REQUIRE(n >= 0 && n < (1L << 36), "%s: %ld rows, must be in [0, 2^36)", who, n);
    if (n == 0) return 0;
    CLIFT_REQUIRE(pts != nullptr && out_pts != nullptr, "%s: NULL pts or out_pts", who);
    CLIFT_REQUIRE((dirs == nullptr) == (out_dirs == nullptr), "%s: dirs and out_dirs come together (both or neither NULL)", who);
    if (shaped)
        k_edit_shaped_points<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(P, pts, ldp, dirs, ldd, n, out_pts, out_dirs, state);
    else
        k_edit_list_points<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(P.L, pts, ldp, dirs, ldd, n, out_pts, out_dirs, state);
    return clift_check_launch(who);
}

extern "C" int clift_edit_list_points(const clift_edit_t* h_edits, int n_edits, const float* pts, int ldp, const float* dirs, int ldd, long n,
                                      float* out_pts, float* out_dirs, unsigned char* state, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, nullptr, n_edits, "clift_edit_list_points", &P, &shaped)) return 1;
    return edit_points("clift_edit_list_points", P, shaped, pts, ldp, dirs, ldd, n, out_pts, out_dirs, state, s);
}

extern "C" int clift_edit_shaped_points(const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits, const float* pts, int ldp,
                                        const float* dirs, int ldd, long n, float* out_pts, float* out_dirs, unsigned char* state, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, h_shapes, n_edits, "clift_edit_shaped_points", &P, &shaped)) return 1;
    return edit_points("clift_edit_shaped_points", P, shaped, pts, ldp, dirs, ldd, n, out_pts, out_dirs, state, s);
}

// ---- sigma on the lattice of the edited scene
static int edit_dense_sigma(const char* who, const EditLS& P, bool shaped, const clift_vm_t* h_dens, const float* h_lo3, const float* h_hi3,
                            const float* h_inv_ext2, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2, float shift, float* out,
                            unsigned char* state, clift_stream_t s) {
    CLIFT_REQUIRE(h_dens && h_lo3 && h_hi3 && h_inv_ext2, "%s: NULL host record", who);
    CLIFT_REQUIRE(h_dens->comps % 4 == 0, "%s: comps must be a multiple of 4 (got %d)", who, h_dens->comps);
    CLIFT_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "%s: lattice dimensions must be positive (got %d x %d x %d)", who, n0, n1, n2);
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(total < (1L << 36), "%s: %ld lattice points, must be < 2^36", who, total);
    CLIFT_REQUIRE(s0 && s1 && s2 && out, "%s: NULL device buffer", who);
    const float3 lo = f3_of(h_lo3), hi = f3_of(h_hi3), inv = f3_of(h_inv_ext2);
    if (shaped)
        k_edit_shaped_dense_sigma<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), P, lo, hi, inv, s0, s1, s2, n0, n1, n2, shift, out, state);
    else
        k_edit_list_dense_sigma<<<cdiv(total, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), P.L, lo, hi, inv, s0, s1, s2, n0, n1, n2, shift, out, state);
    return clift_check_launch(who);
}

extern "C" int clift_edit_list_dense_sigma(const clift_vm_t* h_dens, const clift_edit_t* h_edits, int n_edits, const float* h_lo3, const float* h_hi3,
                                           const float* h_inv_ext2, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2,
                                           float shift, float* out, unsigned char* state, clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, nullptr, n_edits, "clift_edit_list_dense_sigma", &P, &shaped)) return 1;
    return edit_dense_sigma("clift_edit_list_dense_sigma", P, shaped, h_dens, h_lo3, h_hi3, h_inv_ext2, s0, s1, s2, n0, n1, n2, shift, out, state, s);
}

extern "C" int clift_edit_shaped_dense_sigma(const clift_vm_t* h_dens, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                                             const float* h_lo3, const float* h_hi3, const float* h_inv_ext2, const float* s0, const float* s1,
                                             const float* s2, int n0, int n1, int n2, float shift, float* out, unsigned char* state,
                                             clift_stream_t s) {
    EditLS P;
    bool shaped;
    if (edit_shapes_check(h_edits, h_shapes, n_edits, "clift_edit_shaped_dense_sigma", &P, &shaped)) return 1;
    return edit_dense_sigma("clift_edit_shaped_dense_sigma", P, shaped, h_dens, h_lo3, h_hi3, h_inv_ext2, s0, s1, s2, n0, n1, n2, shift, out, state, s);
}

// ============================================================================ the origin of the content at the active samples
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

// ============================================================================ packing a shape
// flags (g0, g1, g2) bytes, x-major -> the bit lattice: bit lin of the words is 1 iff some flag within Chebyshev distance ``grow`` of cell
// lin is non-zero, the neighbourhood clipped at the border.  One thread per OUTPUT WORD builds its 32 bits in a register and stores the word
// once (bits past the last cell stay 0): no atomics, the same bits every run.
__global__ __launch_bounds__(256) void k_shape_pack(const unsigned char* __restrict__ flags, int g0, int g1, int g2, int grow, long n_words,
                                                    unsigned int* __restrict__ words) {
    const long wi = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    const long total = (long)g0 * g1 * g2;
    unsigned int word = 0;
    for (int b = 0; b < 32; ++b) {
        const long lin = wi * 32 + b;
        if (lin >= total) break;
        const int i2 = (int)(lin % g2), i1 = (int)((lin / g2) % g1), i0 = (int)(lin / ((long)g1 * g2));
        const int a0 = max(i0 - grow, 0), b0 = min(i0 + grow, g0 - 1), a1 = max(i1 - grow, 0), b1 = min(i1 + grow, g1 - 1);
        const int a2 = max(i2 - grow, 0), b2 = min(i2 + grow, g2 - 1);
        bool any = false;
        for (int j0 = a0; j0 <= b0 && !any; ++j0)
            for (int j1 = a1; j1 <= b1 && !any; ++j1) {
                const unsigned char* row = flags + ((long)j0 * g1 + j1) * g2;
                for (int j2 = a2; j2 <= b2; ++j2) any = any || row[j2] != 0;
            }
        word |= (any ? 1u : 0u) << b;
    }
    words[wi] = word;
}

extern "C" int clift_shape_pack(const unsigned char* flags, int g0, int g1, int g2, int grow, unsigned int* words, clift_stream_t s) {
    CLIFT_REQUIRE(g0 >= 1 && g0 <= CLIFT_SHAPE_DIM_MAX && g1 >= 1 && g1 <= CLIFT_SHAPE_DIM_MAX && g2 >= 1 && g2 <= CLIFT_SHAPE_DIM_MAX,
                  "clift_shape_pack: dimensions must be in 1 .. %d (got %d x %d x %d)", CLIFT_SHAPE_DIM_MAX, g0, g1, g2);
    CLIFT_REQUIRE(grow >= 0 && grow <= CLIFT_SHAPE_GROW_MAX, "clift_shape_pack: grow must be in 0 .. %d (got %d)", CLIFT_SHAPE_GROW_MAX, grow);
    CLIFT_REQUIRE(flags != nullptr && words != nullptr, "clift_shape_pack: NULL flags or words");
    const long n_words = ((long)g0 * g1 * g2 + 31) / 32;
    k_shape_pack<<<cdiv(n_words, 256), 256, 0, as_stream(s)>>>(flags, g0, g1, g2, grow, n_words, words);
    return clift_check_launch("clift_shape_pack");
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
    k_edit_list_density_grad_points<<<cdiv(n, 256), 256, 0, as_stream(s)>>>(to_dev(h_dens), L, pts, ldp, n, f3_of(h_lo3), f3_of(h_inv2), shift, out, state);
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
