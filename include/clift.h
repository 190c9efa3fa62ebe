/* clift.h -- C ABI of libclift.so: the MI355X (gfx950) kernels of the Contrastive-Lift render hot path.
 *
 * The reference (yashbhalgat/Contrastive-Lift) is pure Python/PyTorch: it has no FFI layer.  The
 * boundary a maintainer would bind is therefore the set of ATen-op groups its renderer/field/loss
 * objects bottom out in.  Every entry point below cites the reference
 * file:line whose arithmetic it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 / int32 data unless its name starts with h_ (host);
 *   - matrices are row-major with an explicit leading dimension where one is given;
 *   - VM tables are channels-last: plane i is [res[b_i]][res[a_i]][comps], line i is [res[v_i]][comps]
 *     with (a_i,b_i) = (0,1),(0,2),(1,2) and v_i = 2,1,0 (reference tensoRF.py:61-62,104-105; the PyTorch
 *     tensors keep the reference shape (1,C,H,W) and use channels_last strides);
 *   - the library never allocates or frees device memory, never synchronises the device and launches
 *     only on the caller's stream; the caller owns all buffers (torch tensors);
 *   - every function returns 0 on success, non-zero on error (message via clift_last_error());
 *     no C++ exception crosses this boundary;
 *   - one host thread per process drives the library (same threading model as the reference: one
 *     Python thread per DDP rank).
 */
#ifndef CLIFT_H
#define CLIFT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* clift_stream_t; /* hipStream_t */

/* ABI version (bumped on any signature change) and last error string of the calling process. */
int clift_version(void);
/* Data-parallel runs (reference: DDP buckets overlapped with backward, trainer/__init__.py:93-108): leave k of the 256 CUs to
 * the collective's kernels while an asynchronous all-reduce is in flight -- the persistent launches (one block per CU, held for the
 * whole launch) then use 256 - k blocks.  k = 0 restores the default.  Host state; takes effect at the next launch. */
int clift_set_cu_reserve(int k);
/* Kernel switches (ABI 21): one process-wide word of host state that the launch routing reads.  The cross-checks of the test-suite and the A/B
 * tools set it; production runs leave it 0.  The word is seeded ONCE, at its first use, from the environment -- CLIFT_NO_PERSISTENT (set to
 * anything), CLIFT_X6_TILED (set to anything), CLIFT_DENS_FWD=thread, CLIFT_DENS_SCATTER=walk -- so a process started with one of them behaves as
 * before; at run time it changes through clift_set_switches only (returns the previous word; takes effect at the next launch). */
enum {
    CLIFT_SWITCH_TILED_ONLY = 1,         /* every layer on the independent tiled / VALU kernels instead of the persistent and streaming ones */
    CLIFT_SWITCH_X6_TILED = 2,           /* fp32x6 on the tiled split kernel (csrc/gemm_split.hip) instead of the persistent split kernels */
    CLIFT_SWITCH_DENS_FWD_THREAD = 4,    /* clift_density_fwd: the per-thread lookup (the form the wave-per-sweep kernel replaced; bit-identical) */
    CLIFT_SWITCH_DENS_SCATTER_WALK = 8,  /* clift_density_bwd: the group-per-segment walk (the form for comps > 16) at any component count */
    CLIFT_SWITCH_ALL = 15
};
unsigned clift_set_switches(unsigned word);
unsigned clift_get_switches(void);
const char* clift_last_error(void);

/* One VM-decomposed table set (3 planes + 3 lines, equal component count). */
typedef struct {
    const float* plane[3];
    const float* line[3];
    int res[3]; /* Rx, Ry, Rz */
    int comps;  /* components per plane (16 density / 48 appearance in the reference configs) */
} clift_vm_t;

/* Gradient accumulators for a table set (same layout; accumulated into with atomics).
 * xcd_stride == 0: the pointers are the final gradient tables, accumulated with device-scope atomics.
 * xcd_stride  > 0: the pointers address copy 0 of EIGHT zero-initialised accumulation copies, xcd_stride floats
 *   apart; every XCD of the MI355X accumulates into its own copy with atomics that execute in its private L2
 *   (selected by the hardware XCC id, placement-independent); the caller then folds the copies into the real
 *   gradient with clift_xcd_reduce (which also re-zeroes them). */
typedef struct {
    float* plane[3];
    float* line[3];
    long xcd_stride;
} clift_vm_grad_t;

/* dst[i] += sum_{x<8} work[x*xcd_stride + i] for i < n; work is re-zeroed. */
int clift_xcd_reduce(float* work, long xcd_stride, long n, float* dst, clift_stream_t s);

/* Renderer state: reference model/renderer/panopli_tensoRF_renderer.py:42-71 (buffers bbox_aabb,
 * inv_box_extent; python attrs step_size, n_samples, distance_scale, raymarch_weight_thres) and
 * tensoRF.py:35 (splus_density_shift). */
typedef struct {
    float lo[3];
    float hi[3];
    float inv_ext2[3]; /* 2 / (hi - lo) */
    float step_size;
    int n_samples;
    float distance_scale;
    float density_shift;
    float weight_thres;
} clift_march_t;

/* ---- a1-a3: util/ray.py:8-12,25-31,46-54,81-99.  rays (H*W, 8) = [o, d, near, far].
 * *bad_count is incremented for every ray whose sphere discriminant is negative (reference asserts). */
int clift_gen_rays(int H, int W, const float* h_K9, const float* h_c2w16, float near_plane, float* rays,
                   int* bad_count, clift_stream_t s);

/* ---- a4-a6: renderer.py:800-817 (sampling; jitter = perturb*rand per ray, NULL for none), :633-634
 * (normalise), tensoRF.py:108-125 (density VM lookup + shift + softplus).  sigma (N, S), 0 outside the box. */
int clift_density_fwd(const clift_march_t* h_m, const clift_vm_t* h_dens, const float* rays, const float* jitter,
                      int N, float* sigma, clift_stream_t s);

/* Point-wise field API (reference TensorVMSplit.compute_density / compute_density_without_activation,
 * tensoRF.py:114-125; used by the dense alpha grid of the bbox shrink, renderer.py:717-754).  xn (n, ldx) normalised
 * coordinates; out (n). */
int clift_density_points(const clift_vm_t* h_dens, const float* xn, int ldx, long n, float shift, int activation,
                         float* out, clift_stream_t s);
/* Alpha-mask bounding box of the epoch-boundary shrink (renderer.py:669-680,717-729,752-754): alpha = 1 - exp(-softplus(density +
 * shift) * step) on the (g0,g1,g2) lattice of the box [h_lo3, h_hi3] (lattice coordinate of axis a at index i =
 * lo_a (1 - s_a[i]) + hi_a s_a[i]; s0/s1/s2 are DEVICE arrays holding the caller's linspace(0,1,g_a)), clamp to [0,1], 3^3 max-pool
 * (stride 1, padding 1), >= threshold.  alpha_work: g0*g1*g2 floats of scratch (left holding the un-pooled alpha, x-major);
 * box7 (device, 7 ints) = [min index per axis (3), max index per axis (3), number of voxels above the threshold]; min = INT_MAX
 * and max = -1 when none is. */
int clift_alpha_bbox(const clift_vm_t* h_dens, const float* h_lo3, const float* h_hi3, const float* h_inv_ext2, const float* s0,
                     const float* s1, const float* s2, int g0, int g1, int g2, float shift, float step, float threshold,
                     float* alpha_work, int* box7, clift_stream_t s);
/* Plane x line products at arbitrary points, F (n, 3*comps) (compute_appearance_feature before the basis, :127-134). */
int clift_vm_products_points(const clift_vm_t* h_vm, const float* xn, int ldx, long n, float* F, clift_stream_t s);
/* Appearance-MLP input assembly from explicit view directions (render_appearance_mlp(viewdirs, features), :400-408). */
int clift_app_encode_points(const float* feat, int ldf, int nf, int pe_feat, int pe_view, const float* dirs, int ldd,
                            long n, float* X, int ldx, clift_stream_t s);

/* ---- scene-editing renders (ABI 23): renderer.py:303-623 (forward_delete / forward_extract / forward_duplicate / forward_manipulate) on
 * split_points_minimal (:785-797).  One edit, resolved on the host to a plain record (contrastive_lift_amd/edit.py).
 * A box: world point p is inside iff lo <= axes (p - centre) <= hi component-wise, faces inclusive; axes is row-major and its ROWS are
 * the box axes.  Samples inside the destination box are looked up at p' = map_m p + map_t (row-major 3x3, then the offset) and their view
 * direction becomes dir_inv d; samples the kill rule names get sigma = 0 after the density lookup (:346,423,594).  Classification uses
 * the UNEDITED sample position in fp32, every multiply / add rounded separately.  All values of the record must be finite; the fields a
 * mode does not use (dst, map_*, dir_inv for delete / extract; src for duplicate) are ignored but still checked. */
enum {
    CLIFT_EDIT_DELETE = 0,      /* kill samples in src */
    CLIFT_EDIT_EXTRACT = 1,     /* kill samples not in src */
    CLIFT_EDIT_DUPLICATE = 2,   /* kill nothing; remap samples in dst */
    CLIFT_EDIT_MANIPULATE = 3   /* kill samples in src and not in dst; remap samples in dst */
};
typedef struct {
    float axes[9];
    float centre[3];
    float lo[3];
    float hi[3];
} clift_edit_box_t;
typedef struct {
    int mode; /* CLIFT_EDIT_* */
    clift_edit_box_t src;
    clift_edit_box_t dst;
    float map_m[9];
    float map_t[3];
    float dir_inv[9];
} clift_edit_t;
/* The edit form of clift_density_fwd, without jitter (edits render with perturb = 0, is_train = False): sigma (N, S), 0 outside the box
 * (the in-box test is taken BEFORE the remap, as the reference's mask_xyz is) and where the sample is killed; a remapped point that
 * leaves the box reads zero padding, like clift_density_points.  A sample that is neither remapped nor killed gets the bits of
 * clift_density_fwd. */
int clift_edit_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edit, const clift_vm_t* h_dens, const float* rays, int N,
                           float* sigma, clift_stream_t s);
/* For the compacted samples of such a pass: xa (M, 4) = the remapped normalised position [xn.x, xn.y, xn.z, 0] (input of the xyz heads and
 * of clift_vm_products_points with ldx = 4) and dirs (M, 4) = the ray direction, times dir_inv where the sample is in dst (input of
 * clift_app_encode_points with ldd = 4). */
int clift_edit_active(const clift_march_t* h_m, const clift_edit_t* h_edit, const float* rays, const int* act_idx, int M, float* xa,
                      float* dirs, clift_stream_t s);
/* Edit programs (ABI 24): an ordered list e_1 .. e_n of such records, 1 <= n <= CLIFT_EDIT_MAX, applied in ONE render: scene_0 is the trained
 * field, scene_i is e_i applied to scene_{i-1}.  A sample with world position p and view direction d is evaluated in scene_n by walking the
 * list BACKWARDS:
 *     in = aabb test of the UNEDITED p (taken once, before any remap)
 *     for i = n .. 1:  src = mode_i != DUPLICATE && p in src_i;  mov = mode_i >= DUPLICATE && p in dst_i
 *                      if the kill rule of mode_i names (src, mov): sigma = 0, stop
 *                      if mov: p = map_m_i p + map_t_i;  d = dir_inv_i d
 *     look the field up at (p, d)
 * Every box test and every remap acts on the CURRENT p in fp32 with separately rounded ops.  For n = 1 this is the single edit above, bit
 * for bit; a sample that no edit remaps or kills gets the bits of clift_density_fwd.  h_edits is a HOST array of n_edits records (it is
 * copied into the launch: no device buffer, nothing to keep alive).  n_edits outside 1 .. CLIFT_EDIT_MAX, an unknown mode or a non-finite
 * value in any record is an error whose message names the record's index; nothing is launched then. */
#define CLIFT_EDIT_MAX 8
int clift_edit_list_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens,
                                const float* rays, int N, float* sigma, clift_stream_t s);
int clift_edit_list_active(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const float* rays, const int* act_idx, int M,
                           float* xa, float* dirs, clift_stream_t s);
/* The same walk off the rays (an ABI 27 addition): over arbitrary points, and over the lattice of clift_dense_sigma.  Both take the program as
 * clift_edit_list_density_fwd does (a HOST array copied into the launch; the same errors, raised before anything is launched) and walk it with the
 * very operations above.  The STATE byte of a point: the number of edits that remapped it (0 .. CLIFT_EDIT_MAX) in CLIFT_EDIT_STATE_REMAPS,
 * CLIFT_EDIT_STATE_KILLED set if some kill rule named it.
 *
 * clift_edit_list_points: pts (n, ldp >= 3) world points, dirs (n, ldd >= 3) view directions or NULL.  out_pts / out_dirs (the same pitches; only
 * the first three columns of a row are written; out_dirs is NULL exactly when dirs is) = the world point and the direction at which the field is
 * to be looked up -- for a killed row the position at which its walk stopped.  state (n) uint8 or NULL.  There is NO aabb test: what "inside the
 * scene" means is the caller's decision.  A row that no edit remaps gets its input bits back, point and direction.  out_pts may be pts and
 * out_dirs may be dirs.  n == 0 returns 0 without a launch.  Errors: the program's, a pitch < 3, n < 0 or >= 2^36, a NULL pts or out_pts, dirs
 * without out_dirs or the reverse.
 *
 * clift_edit_list_dense_sigma: clift_dense_sigma (below; the same arguments with the same meaning) on the EDITED scene, one launch.  The lattice
 * point is formed as there, then walked.  A killed point gets exactly 0.0f and reads no table.  A remapped point is normalised with separately
 * rounded ops, (p - lo) * inv_ext2 - 1, and looked up; a source point outside the box reads zero padding, as in clift_edit_list_density_fwd and
 * clift_density_points.  A point that no edit remaps or kills gets the bits of clift_dense_sigma.  state (n0 n1 n2) uint8 or NULL.  No atomics:
 * two runs give the same bits.  Errors: clift_dense_sigma's and the program's, all raised before the device is touched. */
#define CLIFT_EDIT_STATE_KILLED 0x80
#define CLIFT_EDIT_STATE_REMAPS 0x0f
int clift_edit_list_points(const clift_edit_t* h_edits, int n_edits, const float* pts, int ldp, const float* dirs, int ldd, long n, float* out_pts,
                           float* out_dirs, unsigned char* state, clift_stream_t s);
int clift_edit_list_dense_sigma(const clift_vm_t* h_dens, const clift_edit_t* h_edits, int n_edits, const float* h_lo3, const float* h_hi3,
                                const float* h_inv_ext2, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2, float shift,
                                float* out, unsigned char* state, clift_stream_t s);
/* The walk of an alpha-list with the ORIGIN of its content (a further ABI 27 addition): clift_edit_list_active without the view
 * directions, for the layers of an edited scene.  One thread per list row; rows past the dynamic row limit are not written.  xa (M, 4): the bits
 * of clift_edit_list_active's xa for the same arguments, [xn, 0].  origin (M) uint8: walking the program backwards, i = n .. 1, the 1-based position
 * of the FIRST edit met that remaps the sample and has mode CLIFT_EDIT_DUPLICATE, 0 if the walk meets none -- the last-applied copy in whose
 * destination the sample sits.  A copy that a later edit moves keeps its origin (the move remaps the sample, then the walk meets the copy); for
 * a copy of a copy the outer one wins; a killed sample keeps what it had when its walk stopped.  state (M) uint8 or NULL: the byte of
 * clift_edit_list_points for the same world point.  M <= 0 returns 0 without a launch.  Errors, raised before anything is launched: the
 * program's, n_samples < 1, a NULL xa or origin. */
int clift_edit_list_active_origin(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const float* rays, const int* act_idx, int M,
                                  float* xa, unsigned char* origin, unsigned char* state, clift_stream_t s);
/* Shaped edits (further ABI 27 additions): an edit that follows an instance's shape, not its box.  A SHAPE is a bit lattice over
 * the SOURCE box of an edit, in that box's local frame: dims = (G0, G1, G2), each in 1 .. CLIFT_SHAPE_DIM_MAX; cell i_a of axis a covers
 * lo_a + i_a h_a .. lo_a + (i_a + 1) h_a with h_a = (hi_a - lo_a) / G_a; bits are x-major, lin = (i0 G1 + i1) G2 + i2 < 2^31, bit lin & 31 of
 * word lin >> 5; the words are uint32 in DEVICE memory (they must stay alive until the launch has run) and the unused high bits of the last
 * word are 0.  inv_cell[a] = fp32(G_a / (hi_a - lo_a)), formed in fp64 from the fp32 lo / hi of the record's src box.
 *
 * Membership of a world point x, in fp32 with every operation rounded on its own: q_a = row a of src.axes times (x - src.centre), as the box
 * test forms it; u_a = (q_a - src.lo_a) * inv_cell_a; i_a = floor(u_a) clamped to 0 .. G_a - 1; bit(x) = the bit of cell (i0, i1, i2).
 *
 * The walk of a program (above) with shapes: for an edit whose words are not NULL
 *     src = mode != DUPLICATE && p in src_i && bit(p)
 *     mov = mode >= DUPLICATE && p in dst_i && bit(map_m_i p + map_t_i)
 * -- the remapped point, which the walk forms anyway, is tested in the SOURCE frame; the index is clamped, so a remapped point that rounding
 * puts just outside the source box reads its border cell -- and the kill rules read these (DELETE src; EXTRACT !src; MANIPULATE src && !mov).  A
 * point in the destination box that is not part of the moved shape is not remapped: it keeps its own content and walks on.  An edit whose
 * words are NULL keeps the box rule; the two kinds mix freely.  An all-ones shape gives the bits of the plain box edit; a rigid move keeps
 * lo, hi and the local frame, so the moved object is addressed at its destination with the same words.
 *
 * clift_edit_shaped_*: the clift_edit_list_* entry point of the same name with h_shapes right behind h_edits: a HOST array of n_edits records
 * (copied into the launch like the edits), or NULL for the list entry point's behaviour, bit for bit.  Errors, raised before anything is
 * launched, the message naming the edit's index: the program's own; for a record with words, a dimension outside 1 .. CLIFT_SHAPE_DIM_MAX,
 * a product of the dimensions >= 2^31, an inv_cell that is not finite and positive.
 *
 * clift_shape_pack: flags (g0 g1 g2) bytes on the device, x-major -> words (ceil(g0 g1 g2 / 32)) uint32 on the device: bit = 1 iff some flag
 * within Chebyshev distance grow (0 .. CLIFT_SHAPE_GROW_MAX) of the cell is non-zero, the neighbourhood clipped at the lattice border (no
 * wrap).  One thread per output word, no atomics, every word written once: two runs give the same bits.  Errors: a dimension < 1 or
 * > CLIFT_SHAPE_DIM_MAX, grow out of range, a NULL buffer. */
#define CLIFT_SHAPE_DIM_MAX 1024
#define CLIFT_SHAPE_GROW_MAX 4
typedef struct {
    const unsigned int* words;   /* DEVICE memory; NULL: this edit has no shape (plain box edit) */
    int dims[3];
    float inv_cell[3];           /* fp32(G_a / (hi_a - lo_a)), formed in fp64 from the fp32 values of the record's src box */
} clift_edit_shape_t;
int clift_edit_shaped_density_fwd(const clift_march_t* h_m, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                                  const clift_vm_t* h_dens, const float* rays, int N, float* sigma, clift_stream_t s);
int clift_edit_shaped_active(const clift_march_t* h_m, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                             const float* rays, const int* act_idx, int M, float* xa, float* dirs, clift_stream_t s);
int clift_edit_shaped_points(const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits, const float* pts, int ldp,
                             const float* dirs, int ldd, long n, float* out_pts, float* out_dirs, unsigned char* state, clift_stream_t s);
int clift_edit_shaped_dense_sigma(const clift_vm_t* h_dens, const clift_edit_t* h_edits, const clift_edit_shape_t* h_shapes, int n_edits,
                                  const float* h_lo3, const float* h_hi3, const float* h_inv_ext2, const float* s0, const float* s1,
                                  const float* s2, int n0, int n1, int n2, float shift, float* out, unsigned char* state, clift_stream_t s);
int clift_shape_pack(const unsigned char* flags, int g0, int g1, int g2, int grow, unsigned int* words, clift_stream_t s);

/* ---- a7-a8: renderer.py:83-84,100-103,137,173-174,626-631 + eff_distloss (renderer.py:101).
 * Per sample alpha, T (transmittance before the sample), w = alpha*T, all (N, S).
 * ray_out (N, 8) = [opacity, depth, bg, w_total, wm_total, dist_loss, t_min, 0]; n_active (N) = #(w > thres). */
int clift_march_fwd(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* sigma,
                    float* alpha, float* T, float* w, float* ray_out, int* n_active, clift_stream_t s);

/* Backward of a7-a8: g_w (N,S) = dL/dw contributions from compositing (zero where inactive),
 * g_opacity (N) = dL/d(sum w), g_dist = device scalar dL/d(dist_reg) (nullable) -> dsigma (N,S) = dL/dsigma. */
int clift_march_bwd(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* alpha,
                    const float* T, const float* w, const float* ray_out, const float* g_w,
                    const float* g_opacity, const float* g_dist, float* dsigma, clift_stream_t s);

/* Backward of a6: scatter dsigma through softplus and the VM products into the table gradients.  sigma (nullable) = the (N,S) output of
 * clift_density_fwd for the same rays: with it the softplus derivative is 1 - exp(-sigma) per sample; without it the sample's feature is
 * summed again over planes and channels (same value to fp32 round-off). */
int clift_density_bwd(const clift_march_t* h_m, const clift_vm_t* h_dens, const clift_vm_grad_t* h_grad,
                      const float* rays, const float* jitter, int N, const float* dsigma, const float* sigma, clift_stream_t s);

/* ---- compaction of active samples (replaces the boolean-mask gathers renderer.py:103-108):
 * ray_start (N+1) = exclusive scan of n_active; act_idx[ray_start[r] .. ray_start[r+1]) = r*S + k in
 * increasing k for every k with w > thres. */
int clift_scan_counts(const int* n_active, int N, int* ray_start, clift_stream_t s);
int clift_compact_fill(const float* w, const int* ray_start, int N, int S, float thres, int* act_idx,
                       clift_stream_t s);

/* ---- sync-free steps (no read-back of the active-sample count; the reference syncs at every boolean-mask gather,
 * renderer.py:97,105).  The caller sizes the compacted buffers by a capacity `cap` and binds ONE device int as the
 * library's dynamic row limit: every per-sample kernel then clamps its row count to min(its argument, *limit) and the
 * persistent kernels re-balance their row ranges over the true count.  The caller keeps INT_MAX in *limit outside a
 * pass; clift_scan_counts_capped writes min(total, cap) into it (limit_out = the bound address), clamps the offsets to
 * cap and records total in *overflow when total > cap (samples past the capacity are dropped -- memory-safe, and the
 * caller is expected to raise the capacity); clift_compact_fill_capped writes only rows < cap.
 * Of the MLP-head entry points below, the bf16-mode kernels of csrc/layer_bf16.hip, layer_nb16.hip and head_bf16.hip do NOT clamp:
 * clift_xyz_head_bf16_fwd, clift_app_head_last2_bf16_fwd (forwards: the rows past the true count are computed and never read),
 * clift_xyz_head_first2_bf16_bwd and clift_out_layer_bwd_n128_bf16 (reductions: they need the true row count as their argument), like the
 * precision-1 routes of clift_gemm; bf16 mode does not run sync-free steps.  Every other one clamps (tests/test_gpu_head_cases.py holds each to
 * the reference of L rows, or to the bits of its rows < L), clift_colsum included. */
int clift_bind_rows_limit(const int* dev_limit);

/* XCD-private gradient shards (ABI 12).  The kernels that end by adding a per-block partial of a small gradient tensor to memory (the weight
 * gradients of the MLP layers, the K = 3 / output layers' gradients) are slowed by contention: all eight XCDs read-modify-write the same few
 * cache lines at the same moment (8 - 20 us per launch).  With shards a block adds into the copy of the gradient range that belongs to its
 * XCD, and the eight copies are folded into the gradients once per pass.  Record (40 bytes of device memory, little endian):
 *   int64 lo      address of the first float of the sharded gradient range      int64 bytes   its length
 *   int64 shard0  address of shard 0 (shard x at shard0 + x * stride; 8 shards, zero-initialised by the caller ONCE)
 *   int64 stride  bytes between shards                                           int32 enabled, int32 pad
 * clift_bind_grad_shards(record) publishes the record's address once per process (NULL unbinds).  A pass is bracketed, stream-ordered, by
 * clift_grad_shards_begin(record, src, zero, zero_n): record := *src with enabled = 1, and zero_n floats at `zero` are cleared (the launch
 * takes the place of the caller's gradient fill), and clift_grad_shards_fold(record, first, n, disable): gradients[first .. first + n) +=
 * the eight shards, which are cleared again; disable != 0 ends the bracket.  Outside a bracket every kernel adds straight into the
 * gradients (the autograd path, direct C callers: nothing changes for them). */
int clift_bind_grad_shards(const void* dev_record);
int clift_grad_shards_begin(void* dev_record, const void* dev_src, float* zero, long zero_n, clift_stream_t s);
int clift_grad_shards_fold(void* dev_record, long first, long n, int disable, clift_stream_t s);   /* NULL unbinds; one-time, synchronous */
int clift_scan_counts_capped(const int* n_active, int N, int* ray_start, int cap, int* limit_out, int* overflow,
                             clift_stream_t s);
int clift_compact_fill_capped(const float* w, const int* ray_start, int N, int S, float thres, int* act_idx, int cap,
                              clift_stream_t s);

/* ---- a9: tensoRF.py:127-134 (plane x line products, plane-major concat) on the compacted samples.
 * F (M, 3*comps); xa (M, 4) = [xn.x, xn.y, xn.z, 0] (input of the xyz MLP heads, tensoRF.py:142-156). */
int clift_app_gather_fwd(const clift_march_t* h_m, const clift_vm_t* h_app, const float* rays, const float* jitter,
                         const int* act_idx, int M, float* F, float* xa, clift_stream_t s);
/* xa only (instance / segment passes: renderer.py:204,285 evaluate the xyz heads without appearance). */
int clift_active_xyz(const clift_march_t* h_m, const float* rays, const float* jitter, const int* act_idx, int M,
                     float* xa, clift_stream_t s);
/* xa (nullable): the (M, 4) normalised positions clift_app_gather_fwd / clift_active_xyz produced for the same act_idx -- when
 * given (and comps <= 64), the backward runs in its wave-per-(segment, plane) form: the index work of a 32-sample segment is done once, in
 * parallel, and the serial walk keeps only the per-channel arithmetic (same per-sample terms, merged over 32 instead of 16 samples, i.e. a
 * different fp32 summation order). */
int clift_app_gather_bwd(const clift_march_t* h_m, const clift_vm_t* h_app, const clift_vm_grad_t* h_grad,
                         const float* rays, const float* jitter, const int* act_idx, int M, const float* dF,
                         const float* xa, clift_stream_t s);

/* ---- a10 input assembly: tensoRF.py:400-408,413-418.  X (M, ldx) = [feat(nf), dir(3), sin/cos PE(feat),
 * sin/cos PE(dir), zero pad]; ldx >= nf + 3 + 2*pe_feat*nf + 2*pe_view*3. */
int clift_app_encode_fwd(const float* feat, int ldf, int nf, int pe_feat, int pe_view, const float* rays,
                         const int* act_idx, int S, int M, float* X, int ldx, int x_bf16 /* X is bf16-stored */, clift_stream_t s);
int clift_app_encode_bwd(const float* feat, int ldf, int nf, int pe_feat, const float* dX, int ldx, int M,
                         float* dfeat, int lddf, clift_stream_t s);
/* The appearance head's front end in ONE launch (ABI 16): clift_app_gather_fwd, the basis Linear (tensoRF.py:65,127-134: feat = F Wb^T,
 * Wb (nf, 3*comps) with row pitch ldb, no bias) and clift_app_encode_fwd for tiles of 64 active samples, the products and the features
 * staying on the CU.  Writes xa (M, 4; nullable), feat (M, ldf; pad columns zero -- the encode backward reads it), X (M, ldx) fp32 and --
 * only when F is not NULL (a backward pass will want the products) -- F (M, 3*comps).  feat = F Wb^T runs on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32, two k halves added: fp32 round-off apart from the GEMM of the unfused path).  nf <= 28, nf <= ldf <= 28, ldx % 4 == 0, ldb % 4 == 0. */
int clift_app_front_fwd(const clift_march_t* h_m, const clift_vm_t* h_app, const float* rays, const float* jitter, const int* act_idx,
                        int M, const float* Wb, int ldb, int nf, int pe_feat, int pe_view, float* xa, float* feat, int ldf, float* X,
                        int ldx, float* F, clift_stream_t s);
/* ... with the choice of X's storage (ABI 17): x_bf16 = 1 writes X as (M, ldx) bf16, ldx even (bf16 mode: the appearance MLP's input is bf16-stored
 * like every other streamed activation of that mode); x_bf16 = 0 is clift_app_front_fwd. */
int clift_app_front_fwd_x(const clift_march_t* h_m, const clift_vm_t* h_app, const float* rays, const float* jitter, const int* act_idx,
                          int M, const float* Wb, int ldb, int nf, int pe_feat, int pe_view, float* xa, float* feat, int ldf, void* X,
                          int ldx, float* F, int x_bf16, clift_stream_t s);

/* ---- nn.Linear building block on the matrix cores (tensoRF.py:65,393-397,475-491,576-582 and their
 * backward).  C[m][n] (+)= act( sum_k A(m,k) * B(n,k) + bias[n] ) * (mask[m][n] > 0)
 *   A(m,k) = a_trans ? A[k*lda+m] : A[m*lda+k];   B(n,k) = b_trans ? B[k*ldb+n] : B[n*ldb+k].
 * precision 0: fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32, exact fp32 products).
 * precision 1: "bf16 mode" -- A and B are rounded to bf16 (RNE) on their way into LDS, products on
 *   v_mfma_f32_32x32x16_bf16 with fp32 accumulation; all tensors stay fp32 in memory (BASELINE config 3).
 * precision 2: "fp32x6" -- fp32-faithful products on the bf16 matrix cores: every operand value is split exactly into three
 *   bf16 terms and the six leading cross products are accumulated in fp32 (error below fp32 product rounding).  Applies to
 *   the forward / dgrad forms (a_trans = 0, no accumulate); other forms run as precision 0.  Needs `workspace` -- except for the forms that
 *   have persistent split kernels, which need none: N = K = 256 forward / masked dgrad and the 256 x 256 weight gradient (csrc/layer_x6*.hip)
 *   and, ABI 18, the 128-wide appearance layers (csrc/layer_n6.hip: forward K in {128, 160} -> N = 128, masked dgrad 128 -> 128, unmasked dgrad
 *   128 -> 160, weight gradients 128 x {128, 160} with a_trans = b_trans = accumulate = 1).
 * K % 4 == 0, lda/ldb % 4 == 0, 16-byte aligned bases.
 * split_k > 1 partitions K over blockIdx.z and requires accumulate = 1 (atomic add into C).
 * Dispatch (no change of contract): the N = K = 256 hidden-layer forms with M >= 4096 -- forward (plain A, [n][k] weights, no
 *   mask) and masked dgrad (b_trans, fp32 mask, no bias/act) -- run as persistent kernels (csrc/layer_f32.hip: weights in registers,
 *   rows streamed by LDS-DMA); in precision 1 with bf16-stored A / C (/ mask) the same forms and the 256 x 256 wgrad run as
 *   streaming kernels (csrc/layer_bf16.hip).  Everything else takes the tiled kernels (csrc/gemm*.hip).  clift_gemm_route (below) names the
 *   kernel a descriptor goes to.  CLIFT_SWITCH_TILED_ONLY forces the tiled kernels (A/B comparisons in tests/test_gpu_parity.py): the
 *   environment variable CLIFT_NO_PERSISTENT=1, read once at start, or clift_set_switches at run time.
 * Pad columns of the operands, i.e. [K, lda) of a row of A and [K, ldb) of a row of B (a_trans / b_trans: [M, lda), [N, ldb)): no kernel
 *   lets them into a result, and all but one never read them -- they may hold anything, NaN included.  The exception is the narrow-K input
 *   gradient (a_trans = 0, b_trans = 1, K <= lda <= 32, M >= 4096, no bias / act: CLIFT_GEMM_ROUTE_DGRAD_NARROW and _DGRAD_NARROW_BF16,
 *   csrc/narrow_stream.hip): it copies whole rows of A into LDS and multiplies the columns [K, lda) by zero weights, so there the pad columns
 *   of A must be FINITE (the engine's producers write zeros: clift_rows_act_bwd, clift_composite_bwd_act, clift_app_encode_bwd); a NaN or Inf
 *   in them becomes a NaN in that row of C, where the tiled kernel would have returned a number.  Rows of A / B / mask past the row count
 *   are never read, and nothing is written to the pad columns [N, ldc) of C (c_trans: [M, ldc)).
 * mask: an entry is ON if and only if its value is > 0 -- +0.0, -0.0, negative values and negative denormals are off; positive denormals
 *   and +inf are on.  A mask must be NaN-FREE: the fp32 comparison treats a NaN as off, the sign test of a bf16-stored mask (mask_bf16)
 *   treats a NaN with a clear sign bit as on. */
typedef struct {
    int M, N, K;
    const float* A; int lda; int a_trans;
    const float* B; int ldb; int b_trans;
    float* C; int ldc;
    const float* bias;              /* nullable */
    int act;                        /* 0 none, 1 relu */
    const float* mask; int ldmask;  /* nullable */
    int accumulate;
    int split_k;
    int c_trans;                    /* write C[n*ldc + m] (lets a narrow-M wgrad run as a narrow-N problem) */
    float* colsum;                  /* nullable; a_trans only: colsum[m] += sum_k A(m,k)  (bias gradient) */
    int precision;                  /* 0 fp32 operands, 1 bf16 operands (fp32 accumulate), 2 fp32x6 split (see above) */
    void* workspace;                /* precision 2 only: device scratch for the split weight planes, 16-byte aligned */
    long workspace_bytes;           /* >= clift_gemm_workspace_bytes(N, K) */
    int a_bf16, b_bf16, c_bf16, mask_bf16;  /* precision 1 only: the tensor is STORED as bf16 (2-byte elements, pitches in elements);
                                     * the pointers are passed through the float* fields */
    void* sign_bits;                /* nullable; precision 2, N = K = 256 persistent forms only (ABI 15): clift_sign_bits_bytes(M) bytes.  A forward
                                     * (act = 1) also WRITES the signs of its output there (one byte per lane of the kernel and 32-row tile: 32 B per
                                     * row); the masked dgrad of the NEXT layer (b_trans, mask = NULL) READS them instead of the 1 KB-per-row fp32 mask --
                                     * same results bit for bit.  The layout is private to csrc/layer_x6.hip: only pass what such a forward wrote for
                                     * the same M. */
} clift_gemm_t;
long clift_gemm_workspace_bytes(int N, int K);
/* The kernel clift_gemm runs a descriptor on (ABI 21).  clift_gemm_route checks the descriptor like clift_gemm does and returns the route, or
 * CLIFT_GEMM_ROUTE_INVALID with the message in clift_last_error(); it reads the descriptor and the switch word only -- no data pointer is
 * dereferenced (addresses count for their alignment), the device is not touched, `workspace` is not looked at (clift_gemm demands it for
 * CLIFT_GEMM_ROUTE_SPLIT_TILED).  The four routes CLIFT_GEMM_ROUTE_LAYER_X6 .. WGRAD_N6 are the persistent split kernels of precision 2. */
typedef enum {
    CLIFT_GEMM_ROUTE_INVALID = -1,
    CLIFT_GEMM_ROUTE_NONE = 0,          /* M == 0 or N == 0: nothing to launch */
    /* precision 2 (fp32x6) */
    CLIFT_GEMM_ROUTE_LAYER_X6,          /* csrc/layer_x6.hip: 256 x 256 forward / dgrad */
    CLIFT_GEMM_ROUTE_WGRAD_X6,          /* csrc/layer_x6w.hip: 256 x 256 weight gradient */
    CLIFT_GEMM_ROUTE_LAYER_N6,          /* csrc/layer_n6.hip: the 128-wide appearance layers, forward / dgrad */
    CLIFT_GEMM_ROUTE_WGRAD_N6,          /* ... their weight gradients */
    CLIFT_GEMM_ROUTE_SPLIT_TILED,       /* csrc/gemm_split.hip: any other forward / dgrad shape (needs the workspace) */
    /* precision 0 (exact fp32), and every precision 2 form without a split kernel */
    CLIFT_GEMM_ROUTE_LAYER_F32_FWD,     /* csrc/layer_f32.hip */
    CLIFT_GEMM_ROUTE_LAYER_F32_DGRAD,
    CLIFT_GEMM_ROUTE_DGRAD_NARROW,      /* csrc/narrow_stream.hip */
    CLIFT_GEMM_ROUTE_WGRAD_F32_QUADS,   /* csrc/layer_n128.hip */
    CLIFT_GEMM_ROUTE_WGRAD_N128,
    CLIFT_GEMM_ROUTE_LAYER_N128,
    CLIFT_GEMM_ROUTE_DGRAD_N160_PAIR,   /* LAYER_N128 on columns 0..127 + TILED_256X32 on columns 128..159 */
    CLIFT_GEMM_ROUTE_TILED_128X256,     /* csrc/gemm.hip, by block tile */
    CLIFT_GEMM_ROUTE_TILED_128X128,
    CLIFT_GEMM_ROUTE_TILED_256X32,
    /* precision 1 (bf16 operands) */
    CLIFT_GEMM_ROUTE_LAYER_BF16,        /* csrc/layer_bf16.hip */
    CLIFT_GEMM_ROUTE_WGRAD_BF16,
    CLIFT_GEMM_ROUTE_DGRAD_NARROW_BF16, /* csrc/narrow_stream.hip, bf16-stored mask / result */
    CLIFT_GEMM_ROUTE_LAYER_NB16,        /* csrc/layer_nb16.hip */
    CLIFT_GEMM_ROUTE_WGRAD_NB16,
    CLIFT_GEMM_ROUTE_TILED_BF16_128X256, /* csrc/gemm_bf16.hip, by block tile */
    CLIFT_GEMM_ROUTE_TILED_BF16_128X128,
    CLIFT_GEMM_ROUTE_TILED_BF16_256X32,
    CLIFT_GEMM_ROUTE_COUNT
} clift_gemm_route_t;
int clift_gemm_route(const clift_gemm_t* h);
const char* clift_gemm_route_name(int route);   /* "LAYER_X6", ...; "INVALID" for anything that is not a route */
long clift_sign_bits_bytes(int M);

/* Backward of a narrow output layer (no <= 32 outputs: 22 classes / 3 instance dims) over a 256-wide ReLU hidden layer in ONE pass over
 * the hidden activation H (tensoRF.py:480-481, 593-594 backward): dX = (H > 0) . (dOut W), gW += dOut^T H, gb += column sums of dOut.
 * dOut (M, ldd) fp32 with zero pad columns (no <= ldd <= 32, ldd % 4 == 0), W (no, 256) pitch ldw, H (M, 256) pitch ldh, dX (M, 256)
 * pitch ldx, gW (no, 256) pitch ldgw (accumulated), gb (no) nullable (accumulated); 16-byte aligned rows.  Replaces one clift_wgrad_narrow +
 * one masked clift_gemm(b_trans) call, which each stream H from memory.
 * The pad columns [no, ldd) of dOut must be FINITE (the kernel is the narrow dgrad stream of clift_gemm_t: whole rows go to LDS and meet zero
 * weights); pad columns of H / W, the rows of dOut / H past M and the rows of W past `no` are never read and may hold anything.  H is both the
 * mask (on iff > 0: +-0 and negative denormals are off, positive denormals on; NaN-free) and an operand of gW; gb sums the UNMASKED dOut.
 * Nothing is written outside dX[0..M)[0..nh), gW[0..no)[0..nh) and gb[0..no). */
int clift_out_layer_bwd(const float* dOut, int ldd, int no, const float* W, int ldw, const float* H, int ldh, int M,
                        float* dX, int ldx, float* gW, int ldgw, float* gb, clift_stream_t s);
/* ... over a hidden layer of nh units, nh % 32 == 0, nh <= 256 (ABI 16: the 128-wide appearance head, tensoRF.py:393-397 backward; its
 * dOut is the gradient of the pre-sigmoid colours, (M, 4) with a zero pad column).  Pitches >= nh. */
int clift_out_layer_bwd_nh(const float* dOut, int ldd, int no, const float* W, int ldw, const float* H, int ldh, int nh, int M,
                           float* dX, int ldx, float* gW, int ldgw, float* gb,
                           int h_bf16 /* H and dX are bf16-stored (bf16 mode, nh = 256): the products stay fp32 */, clift_stream_t s);
/* Forward of a narrow output layer over a 256-wide hidden activation, with the row activation that follows it, in ONE pass over H (ABI 15;
 * tensoRF.py:591-594 with :37 for the semantic head):  out[m][0..no) = act( H[m][0..256) W^T + b ),  no <= 32, act 0 = none, 2 = softmax over
 * the row.  H (M, ldh) fp32, W (no, 256) pitch ldw, b (no), out (M, ldo) -- columns [no, ldo) untouched.  Replaces clift_gemm (which streams H at
 * less than half the rate for so narrow an output) + clift_rows_act_fwd; results differ from that pair by fp32 summation order only.
 * Pad columns of H and W and rows of H past M are never read; a row's bits do not depend on the launch it is part of. */
int clift_out_layer_fwd(const float* H, int ldh, const float* W, int ldw, const float* b, int no, int M, float* out, int ldo, int act,
                        clift_stream_t s);
int clift_gemm(const clift_gemm_t* h_g, clift_stream_t s);

/* First layer of the xyz heads (in_features == 3): out (M, Nout) = act(x[:, :3] W^T + b); x is (M, 4), W (Nout, 3)
 * with row pitch ldw.  Each output is fmaf(w2, z, fmaf(w1, y, fmaf(w0, x, b))) -- the operation order every fused kernel that re-derives the
 * first layer's sign repeats.  x[:, 3] and the pad columns of W never enter a result (here and in every entry point below that takes x4:
 * they may hold anything); Nout % 4 == 0, ldo % 4 == 0; columns [Nout, ldo) of out are not written. */
int clift_linear_k3_fwd(const float* x4, const float* W, int ldw, const float* b, int M, int Nout, int relu,
                        float* out, int ldo, int out_bf16 /* out is bf16-stored (bf16 mode) */, clift_stream_t s);
/* First TWO layers of an xyz head in one launch (tensoRF.py:475-478, 576-579; 256-wide hidden layers, fp32):
 * h2 (M, ldh2) = relu(W1 relu(W0 x + b0) + b1).  The K = 3 layer is generated inside the second layer's persistent kernel
 * instead of being written (255 MB at the bench shape) and re-read.  h1 (nullable; (M, ldh1)) receives the first layer's
 * activation when a backward pass will need it.  Results are bit-identical to clift_linear_k3_fwd followed by clift_gemm. */
int clift_xyz_head_first2_fwd(const float* x4, const float* W0, int ldw0, const float* b0, const float* W1, int ldw1,
                              const float* b1, int M, float* h1, int ldh1, float* h2, int ldh2, clift_stream_t s);
/* clift_xyz_head_first2_fwd in fp32x6 arithmetic (ABI 13): the 256 x 256 layer as six bf16 products per fp32 product on the bf16 matrix
 * cores (csrc/layer_x6.hip), the K = 3 layer exact; the first layer's activation is never written (the backward does not need it:
 * clift_xyz_head_first2_bwd / clift_xyz_head_first2_wgrad).  Results within 1e-6 (row-max relative) of clift_xyz_head_first2_fwd. */
int clift_xyz_head_first2_x6_fwd(const float* x4, const float* W0, int ldw0, const float* b0, const float* W1, int ldw1,
                                 const float* b1, int M, float* h2, int ldh2, void* sign_bits /* nullable, see clift_gemm_t (ABI 15) */,
                                 clift_stream_t s);
/* Backward of the first TWO layers of an xyz head in bf16 mode, the part behind the second layer's weight gradient (ABI 16; the bf16 counterpart
 * of clift_xyz_head_first2_bwd, tensoRF.py:475-478, 576-579): dH2 (M, ldd) and the first activation h1 (M, ldm; the ReLU mask) bf16-STORED, W1
 * (256, 256) and the positions x4 (M, 4) fp32.  gW0 (256, ldg) += ((h1 > 0) . bf16(dH2 W1))^T x4[:, :3], gb0 += its column sums: the second
 * layer's input gradient is formed, rounded to bf16 and masked exactly as clift_gemm would store it, and consumed in the kernel -- never written. */
int clift_xyz_head_first2_bf16_bwd(const void* dH2, int ldd, const float* W1, int ldw1, const void* h1, int ldm, const float* x4, int M,
                                   float* gW0, int ldg, float* gb0, clift_stream_t s);
/* The fp32x6 counterparts of the three fused ends of an xyz head's backward / forward (ABI 14; csrc/layer_x6.hip, csrc/layer_x6w.hip): the
 * 256 x 256 products as six bf16 products per fp32 product of exactly three-way-split operands (fp32 accumulate; within 1e-6 row-max relative
 * of the exact-fp32 entry points they mirror), everything narrow -- the K = 3 layer, the ReLU masks, the E <= 4 output layer -- in exact fp32.
 *   clift_xyz_head_first2_x6_bwd    = clift_xyz_head_first2_bwd   (tensoRF.py:475-476, 576-577): dH1 never written, mask never read;
 *   clift_xyz_head_first2_x6_wgrad  = clift_xyz_head_first2_wgrad (tensoRF.py:477-478, 578-579): the first activation regenerated in the split;
 *   clift_xyz_head_last2_x6_fwd     = clift_xyz_head_last2_fwd    (tensoRF.py:478-481): the output layer applied to the tile in registers; the
 *     16 column-group partial sums of a row go through `workspace` (clift_xyz_head_last2_x6_workspace_bytes(M) bytes, 16-byte aligned,
 *     the caller's scratch until the call has run on the stream) and are added in a fixed order by a second small launch: deterministic,
 *     and a row's bits do not depend on how many rows share the launch. */
int clift_xyz_head_first2_x6_bwd(const float* dH2, int ldd, const float* W1, int ldw1, const float* W0, int ldw0, const float* b0,
                                 const float* x4, int M, float* gW0, int ldgw0, float* gb0, clift_stream_t s);
int clift_xyz_head_first2_x6_wgrad(const float* dH2, int ldd, const float* W0, int ldw0, const float* b0, const float* x4, int M,
                                   float* gW1, int ldgw1, float* gb1, clift_stream_t s);
long clift_xyz_head_last2_x6_workspace_bytes(int M);
int clift_xyz_head_last2_x6_fwd(const float* A, int lda, const float* W, int ldw, const float* b, const float* Wout, int ldwo,
                                const float* bout, int E, int M, float* hidden, int ldh, float* out, int ldo, void* workspace,
                                long workspace_bytes, clift_stream_t s);
/* Backward of the first TWO layers of an xyz head in one launch (tensoRF.py:475-478, 576-579; fp32, ABI 11).  dH2 (M, ldd) is the
 * gradient at the second layer's output, already masked by that layer's ReLU; W0 (256, 3) / b0 the first layer; x4 (M, 4) the sample
 * positions.  The second layer's input gradient dH1 = (W0 x + b0 > 0) . (dH2 W1) is formed tile by tile and consumed in place:
 *   gW0[n][0..2] += sum_m dH1[m][n] x4[m][0..2],   gb0[n] += sum_m dH1[m][n]
 * -- dH1 (1 KB per row) is never written, and the first layer's activation is not read: its sign is re-derived from the positions in the
 * forward's operation order (the same bits clift_linear_k3_fwd / clift_xyz_head_first2_fwd produced).  Replaces clift_gemm(b_trans, mask)
 * + clift_linear_k3_bwd; results differ from that pair by summation order only (both accumulate per-block partial sums with fp32
 * atomics).  The second layer's own weight gradient stays a clift_gemm call. */
int clift_xyz_head_first2_bwd(const float* dH2, int ldd, const float* W1, int ldw1, const float* W0, int ldw0, const float* b0,
                              const float* x4, int M, float* gW0, int ldgw0, float* gb0, clift_stream_t s);
/* Weight / bias gradient of the SECOND layer of an xyz head with its input -- the first layer's activation -- generated in-kernel from
 * the positions (ABI 11):  gW1[n][k] += sum_m dH2[m][n] relu(W0[k] . x4[m] + b0[k]),  gb1[n] += sum_m dH2[m][n]  (gb1 nullable).
 * With clift_xyz_head_first2_bwd this makes the first layer's activation (1 KB per sample) unnecessary for the backward: the forward
 * (clift_xyz_head_first2_fwd with h1 = NULL) never writes it.  Same bits as clift_gemm's weight gradient over the stored activation up
 * to the summation order of the per-block partial sums. */
int clift_xyz_head_first2_wgrad(const float* dH2, int ldd, const float* W0, int ldw0, const float* b0, const float* x4, int M,
                                float* gW1, int ldgw1, float* gb1, clift_stream_t s);
/* LAST hidden layer of an xyz head together with its narrow output layer (E <= 4 outputs: the instance heads,
 * tensoRF.py:478-481): h = relu(A W^T + b), out[:, 0:E] = h Wout^T + bout, in one launch -- the output layer is applied to the
 * tile while it is in registers instead of re-reading the 1 KB-per-row activation.  `hidden` (nullable, (M, ldh)) receives h when
 * a backward pass will need it.  The E sums are formed in a fixed order (deterministic); they differ from clift_gemm's by
 * summation order only. */
int clift_xyz_head_last2_fwd(const float* A, int lda, const float* W, int ldw, const float* b, const float* Wout, int ldwo,
                             const float* bout, int E, int M, float* hidden, int ldh, float* out, int ldo, clift_stream_t s);

/* Last hidden layer of the appearance MLP + its output layer + sigmoid in one launch (tensoRF.py:395-397,410; 128-wide, fp32):
 * h = relu(A W^T + b) (written to `hidden` if non-null), pre = h Wout^T + bout (written if `pre` non-null), out = sigmoid ?
 * 1/(1+exp(-pre)) : pre.  E <= 4.  Deterministic; differs from clift_gemm + clift_rows_act_fwd by summation order only. */
int clift_app_head_last2_fwd(const float* A, int lda, const float* W, int ldw, const float* b, const float* Wout, int ldwo,
                             const float* bout, int E, int M, float* hidden, int ldh, float* pre, int ldp, float* out, int ldo,
                             int sigmoid, clift_stream_t s);
/* fp32x6 (ABI 18; csrc/layer_n6.hip): the same pair of layers with the 128 x 128 product as six bf16 products of exactly three-way-split
 * operands (fp32-faithful, see clift_gemm precision 2), the output layer in exact fp32 FMAs on the finished tile, its four column-group shares
 * summed in a fixed order; `hidden` (M, ldh) fp32 or NULL (not written).  E <= 4. */
int clift_app_head_last2_x6_fwd(const float* A, int lda, const float* W, int ldw, const float* b, const float* Wout, int ldwo,
                                const float* bout, int E, int M, float* hidden, int ldh, float* out, int ldo, int sigmoid,
                                clift_stream_t s);
/* bf16 mode (ABI 17; csrc/layer_nb16.hip): the same pair of layers over a bf16-STORED input activation A (M, lda), W (128, 128) fp32 rounded to
 * bf16 in the kernel, fp32 accumulate; `hidden` (M, ldh) bf16-stored or NULL; the output layer takes the bf16-rounded hidden activation (what
 * the unfused pair would read back) against fp32 output weights, its four column-group shares summed in a fixed order.  E <= 4. */
int clift_app_head_last2_bf16_fwd(const void* A, int lda, const float* W, int ldw, const float* b, const float* Wout, int ldwo,
                                  const float* bout, int E, int M, void* hidden, int ldh, float* out, int ldo, int sigmoid,
                                  clift_stream_t s);
/* bf16 mode (ABI 17): backward of the no <= 4 wide output layer over the bf16-stored 128-wide hidden activation H (tensoRF.py:397 backward), one
 * pass over H:  dX (M, ldx) bf16-stored = (H > 0) . (dOut W),  gW (no, 128) += dOut^T H,  gb (no) += column sums of dOut (nullable).
 * dOut (M, ldd) fp32 with ldd >= 4 (pad columns ignored: [no, ldd) may hold anything, NaN included), products fp32.  Does not clamp to the device
 * row limit (see clift_bind_rows_limit). */
int clift_out_layer_bwd_n128_bf16(const float* dOut, int ldd, int no, const float* W, int ldw, const void* H, int ldh, int M,
                                  void* dX, int ldx, float* gW, int ldgw, float* gb, clift_stream_t s);
/* bf16 mode: the first three layers of an xyz head (K = 3 layer + two 256 x 256 hidden layers, tensoRF.py:475-479, 576-579) and,
 * for E in [1,4], its E-wide output layer, in ONE launch with the activations resident in LDS (bf16 operands, fp32 accumulate --
 * the arithmetic of clift_linear_k3_fwd + clift_gemm(precision 1) with bf16-stored activations).  h1 / h2 / h3: nullable bf16-stored
 * (M, 256) destinations of the hidden activations, passed only when a backward pass will need them; E = 0: no output layer, h3
 * (required) is the result; E > 0: out (M, ldo) fp32. */
int clift_xyz_head_bf16_fwd(const float* x4, const float* W0, int ldw0, const float* b0, const float* W1, int ldw1,
                            const float* b1, const float* W2, int ldw2, const float* b2, const float* Wout, int ldwo,
                            const float* bout, int E, int M, void* h1, void* h2, void* h3, float* out, int ldo,
                            clift_stream_t s);
/* dW (Nout,3; pitch ldw) += dH^T x ; db (Nout) += colsum(dH).  db nullable.  Pad columns of dH, x4[:, 3] and rows past M are never read;
 * columns [3, ldw) of dW are not written. */
int clift_linear_k3_bwd(const float* x4, const float* dH, int ldh, int M, int Nout, float* dW, int ldw, float* db,
                        int dh_bf16 /* dH is bf16-stored */, clift_stream_t s);
/* Narrow weight gradient (out_features no <= 32: the last layer of every head, tensoRF.py:395,480,581, and the basis
 * Linear :65 seen from its narrow side): gW (no, ni; pitch ldw) += dY^T X over M samples, gb (no; nullable) += colsum(dY).
 * A streaming VALU reduction at HBM rate instead of a mostly-padding matrix-core tile (from 4096 rows on, for ni = 256 -- fp32 X: any multiple
 * of 4 in [32, 256] -- and ldd <= 32: a matrix-core stream, csrc/narrow_stream.hip).  Pad columns [no, ldd) of dY and [ni, ldx) of X never enter
 * a result, in either kernel, and may hold anything; rows past M are never read. */
int clift_wgrad_narrow(const float* dY, int ldd, int no, const float* X, int ldx, int ni, int M, float* gW, int ldw,
                       float* gb, int x_bf16 /* X is bf16-stored */, clift_stream_t s);
/* db (N) += colsum(dY (M,N)); dY has row pitch ld >= N, its pad columns are never read.  Clamps M to the device row limit like every
 * per-sample kernel (a capacity-sized launch sums the true rows only). */
int clift_colsum(const float* dY, int ld, int M, int N, float* db, clift_stream_t s);

/* Row activations of the head outputs: kind 1 = sigmoid (tensoRF.py:385,410), 2 = softmax (tensoRF.py:37,593);
 * the backward also accepts kind 0 = identity (re-pitches dout (M,C) into the 4-float-aligned dpre (M,ldd)).  C <= 64, ldd <= 64.  The forward
 * writes columns [0, C) of out only; the backward WRITES ZEROS into the pad columns [C, ldd) of dpre, for every kind (dpre is the finite-pad A
 * operand of the narrow dgrad stream).  Pad columns of pre / out / dout are never read.  The softmax subtracts the row maximum. */
int clift_rows_act_fwd(const float* pre, int ldp, int M, int C, int kind, float* out, int ldo, clift_stream_t s);
int clift_rows_act_bwd(const float* out, int ldo, const float* dout, int lddo, int M, int C, int kind, float* dpre,
                       int ldd, clift_stream_t s);

/* ---- a13 compositing: renderer.py:137-167.  rgb_s (M,3) sem_s (M,C) inst_s (M,D) are per-active-sample
 * head outputs (NULL to skip a head).  Outputs rgb_raw (N,3) (pre-clamp), rgb_map (N,3), sem_raw (N,C)
 * (weighted sums), sem_map (N,C) (log-normalised when softmax_mode), inst_map (N,D). */
int clift_composite_fwd(const float* w, const int* ray_start, const int* act_idx, int N, int C, int D,
                        const float* rgb_s, const float* sem_s, const float* inst_s, const float* ray_out,
                        int softmax_mode, int white_bg, float* rgb_raw, float* rgb_map, float* sem_raw,
                        float* sem_map, float* inst_map, clift_stream_t s);
/* Backward.  stop_grad = renderer.stop_semantic_grad (w detached for semantics/instances, renderer.py:144-147).
 * Writes d_rgb_s/d_sem_s/d_inst_s (per active sample, M rows), g_w at the active positions of a ZEROED (N,S)
 * buffer, g_opacity (N).  Any of g_rgb/g_sem/g_inst (and the matching head buffers) may be NULL (treated as
 * zero / skipped).  ge_work: scratch of N*(3+C+D) floats. */
int clift_composite_bwd(const float* w, const int* ray_start, const int* act_idx, int N, int S, int M, int C, int D,
                        const float* rgb_s, const float* sem_s, const float* inst_s, const float* rgb_raw,
                        const float* sem_raw, int softmax_mode, int white_bg, int stop_grad, const float* g_rgb,
                        const float* g_sem, const float* g_inst, float* ge_work, float* d_rgb_s, float* d_sem_s,
                        float* d_inst_s, float* g_w, float* g_opacity, clift_stream_t s);
/* The same with the heads' output activations folded in (ABI 16): instead of d_rgb_s / d_sem_s / d_inst_s it writes the gradients w.r.t. the
 * PRE-activation outputs of the heads' last layers, in the zero-padded rows their backward kernels take -- dpre_rgb (M, ld_rgb): sigmoid backward
 * (tensoRF.py:398); dpre_sem (M, ld_sem): sem_kind 2 = softmax backward over the row (tensoRF.py:37,593), 0 = identity; dpre_i0 / dpre_i1
 * (M, ld_inst): instance columns [0, E) / [E, 2E) (fast / slow half, tensoRF.py:505-511; each nullable) -- so no clift_rows_act_bwd launch
 * follows.  The head buffers rgb_s / sem_s / inst_s must be given for the heads whose gradient is wanted.
 * Every column of [0, ld) of a row below M is written when its head is given.  E >= 1 and D <= 2 E (anything else is refused); D need be
 * neither E nor 2 E: a half that D does not fill is zero in the columns D does not reach, like the pads -- D < E leaves dpre_i0 [D, ld_inst)
 * and all of dpre_i1 zero, E < D < 2 E leaves dpre_i1 [D - E, ld_inst) zero -- so the next launch can take the rows as a gradient operand
 * as they are. */
int clift_composite_bwd_act(const float* w, const int* act_idx, int N, int S, int M, int C, int D, const float* rgb_s, const float* sem_s,
                            const float* inst_s, const float* rgb_raw, const float* sem_raw, int softmax_mode, int white_bg, int stop_grad,
                            const float* g_rgb, const float* g_sem, const float* g_inst, float* ge_work, int sem_kind, float* dpre_rgb,
                            int ld_rgb, float* dpre_sem, int ld_sem, float* dpre_i0, float* dpre_i1, int ld_inst, int E, float* g_w,
                            float* g_opacity, clift_stream_t s);

/* ---- a18: model/loss/loss.py:14-22 on one channels-last plane (H,W,C); loss_accum[0] += weight*TV(x);
 * grad (nullable) += weight * dTV/dx. */
int clift_tv_fwd_bwd(const float* plane, int H, int W, int C, float weight, float* grad, float* loss_accum,
                     clift_stream_t s);
/* The same for up to CLIFT_TV_MAX planes in ONE launch (total_tv_loss, tensoRF.py:248-290: three density + three appearance
 * planes every step; each of those passes is a few MB, i.e. launch-latency-sized on this chip). */
#define CLIFT_TV_MAX 8
typedef struct {
    int n;
    const float* plane[CLIFT_TV_MAX];
    float* grad[CLIFT_TV_MAX];      /* nullable per plane */
    int H[CLIFT_TV_MAX], W[CLIFT_TV_MAX], C[CLIFT_TV_MAX];
    float weight[CLIFT_TV_MAX];
} clift_tv_set_t;
int clift_tv_fwd_bwd_multi(const clift_tv_set_t* set, float* loss_accum, clift_stream_t s);

/* ---- a19 pixel losses of training_step (trainer/train_panopli_tensorf.py:155-160,177-178):
 * out2[0] += mean((mask*(rgb-gt))^2); out2[1] += mean_i( mask_i conf_i * -sum_c cw_c p_ic log_softmax(sem_i)_c ).
 * g_rgb = w_rgb * d out2[0]/d rgb ; g_sem = w_sem * d out2[1]/d sem (either nullable); maskf (N) 0/1, nullable. */
int clift_pixel_losses(const float* rgb, const float* rgb_gt, const float* sem, const float* probs,
                       const float* conf, const float* class_w, const float* maskf, int N, int C, float w_rgb,
                       float w_sem, float* out2, float* g_rgb, float* g_sem, clift_stream_t s);

/* The same with SCELoss in place of the cross entropy (config use_symmetric_ce, trainer T:74-77; model/loss/loss.py:36-59):
 * per pixel alpha * CE + beta * RCE, RCE = -sum_c clamp(softmax(sem . cw), 1e-8, 1)_c log(clamp(p_c, 1e-8, 1)) cw_c. */
int clift_pixel_losses_sce(const float* rgb, const float* rgb_gt, const float* sem, const float* probs,
                           const float* conf, const float* class_w, const float* maskf, int N, int C, float w_rgb,
                           float w_sem, float alpha, float beta, float* out2, float* g_rgb, float* g_sem,
                           clift_stream_t s);
/* Per-pixel (reduction='none') form of the two semantic losses, as the reference's loss callables return them
 * (CrossEntropyLoss(weight, reduction='none') with soft targets: sce = 0; SCELoss: sce = 1): loss_rows (N),
 * grad_rows (N, C; nullable) = d loss_rows[i] / d pred[i, :]. */
int clift_semantic_loss_rows(const float* pred, const float* probs, const float* class_w, int N, int C, int sce,
                             float alpha, float beta, float* loss_rows, float* grad_rows, clift_stream_t s);

/* ---- segment-consistency term of training_step (trainer/train_panopli_tensorf.py:185-197): feats (B, ld) rendered semantic
 * features of the rays of G 2D segments, group (B) segment index of each ray.  target class of a segment = argmax of the mean
 * feature row (torch_scatter.scatter_mean); loss[0] += mean_i( class_w[t_i] conf_i CE(feats_i, t_i) ); grad (B, ldg), nullable,
 * = scale * d loss / d feats.  work >= G*C + G floats (zeroed by the call). */
int clift_segment_loss(const float* feats, int ld, const int* group, const float* conf, const float* class_w, int B,
                       int C, int G, float scale, float* work, float* loss, float* grad, int ldg, clift_stream_t s);

/* ---- a16: model/loss/loss.py:62-82.  loss[0] = value; g_feat (B,E) = d loss / d features (nullable).  1 <= E <= 32.  The value is the
 * sum of the per-row terms in a fixed order (kept in work): the same inputs give the same bits. */
int clift_contrastive(const float* feat, const int* labels, int B, int E, float temperature, float* loss,
                      float* g_feat, float* work /* >= 4*B floats */, clift_stream_t s);

/* ---- a17: trainer/train_panopli_tensorf.py:261-309 (use_proj = False).  inst (B, 2E) = [fast | slow];
 * loss[0] = value; g_inst (B,2E) = gradient (zero for the slow half and the slow ray set).
 * work >= 8*B + 2*B*E floats. */
int clift_slow_fast(const float* inst, const int* labels, const float* conf, int B, int E, float* loss,
                    float* g_inst, float* work, clift_stream_t s);

/* ---- inference post-processing: inference/render_panopli.py:371-419 (assign_clusters: per-class cdist + argmin against
 * cached centroids).  labels[i] = argmin_c |feat_i - centroid_c| where valid[i] != 0 (NULL = all), else -1.  feat (n, ldf), ldf >= E;
 * the lowest index wins a tie.  A row whose squared distance to every centroid is NaN (a NaN feature, or NaN centroids) or
 * overflows to +inf gets -1, like an invalid row: no distance compares below the running minimum, which starts at +inf. */
int clift_nearest_centroid(const float* feat, int ldf, int E, const float* centroids, int K, const unsigned char* valid,
                           long n, int* labels, clift_stream_t s);

/* ---- mean-shift (ABI 19): the per-seed climb of sklearn MeanShift.fit (sklearn/cluster/_mean_shift.py, _mean_shift_single_seed), which the
 * reference runs for every clustering of rendered instance features (inference/render_panopli.py:196-368).  X (n, ldx) fp32 points,
 * seeds (S, d) fp32.  For every seed, until the fp32 norm of the step is <= 1e-3 * bandwidth or max_iter steps were completed:
 * neighbours = the points with sum_k (double(x_k) - double(m_k))^2 <= bandwidth^2 (fp64, dimension order), m = fp32(fp64 neighbour
 * sum / count).  Writes centers (S, d) (the last mean), counts (S) (neighbours of the last step; 0 = empty neighbourhood, the centre is
 * then the last mean reached) and iters (S) (completed iterations).  The sum runs over a fixed split of the points, so the centre depends
 * only on the neighbour set (bit-identical for two seeds that end on the same set).  1 <= d <= 32 (larger d is an error), ldx >= d,
 * n < 2^31, bandwidth > 0, max_iter >= 0. */
int clift_meanshift(const float* X, long n, int ldx, int d, const float* seeds, int S, double bandwidth, int max_iter,
                    float* centers, int* counts, int* iters, clift_stream_t s);

/* ---- Euclidean minimum spanning tree (ABI 26; csrc/emst.hip): the tree under HDBSCAN(min_samples = 1), which the reference fits on the CPU for
 * every --use_dbscan clustering (inference/render_panopli.py:236-241, 321-326).  With min_samples = 1 all core distances are 0 and the
 * mutual-reachability graph is the plain Euclidean graph.  X (n, ldx) fp32 device rows, the first d columns used.  Writes the n - 1 edges of a
 * minimum spanning tree of the complete graph: edge_a[e] < edge_b[e] point indices, edge_w[e] = sqrt(d2) in fp64, correctly rounded, with
 * d2 = sum_k (double(x_ak) - double(x_bk))^2 added in dimension order, every product and sum rounded separately (no contraction) -- the
 * arithmetic of clift_knn_kth_dist, and the number sklearn's fp64 tree computes.  Brute-force Boruvka under the STRICT edge order
 * (d2, min(i, j), max(i, j)): per round every point finds its smallest-key edge to another component (all comparisons on the fp64 d2), every
 * component takes the smallest of them (integer atomicMin on the bits of d2, then on min * n + max), hooks to the component the edge leads to
 * (of a mutual pair the smaller root stays) and writes the edge into the slot of its dying root; the used slots are packed in ascending slot
 * order.  Two runs give the same bits, edge order included; the weight multiset is that of every minimum spanning tree.  The fixed maximum of
 * ceil(log2 n) rounds is launched without a host sync (separate launches on the stream, no grid-wide barrier); the kernels of a round return at
 * once when one component is left.
 * info (4 ints, device): rounds executed; components left (1 on success); fault flags (0 on success); 0.  Fault flags: 1 = a root chain longer
 * than n (internal); 2 = NON-FINITE INPUT: some point had no finite d2 to any point of another component (a NaN or infinite coordinate, or a d2
 * that overflows) -- such candidates are never taken, the components they would join stay apart, components left is then > 1 and the edges past
 * the n - components written ones are (-1, -1, 0); 4 = an edge key that does not decode (internal).  The call never loops on such input: every
 * device loop is bounded by n or by its slice.  The caller reads info and treats fault != 0 or components != 1 as an error.
 * work: a device buffer of at least CLIFT_EMST_WORK_BYTES(n) bytes, 8-byte aligned, contents irrelevant before and undefined after.
 * Errors (non-zero return, nothing launched): n outside [2, CLIFT_EMST_MAX_N] (the work is O(n^2 log n); the callers subsample to 50 000), d outside
 * [1, 32], ldx < d, a NULL buffer, a misaligned work, work_bytes too small.  d == 3 is the specialised instantiation. */
#define CLIFT_EMST_MAX_N 131072
#define CLIFT_EMST_SPLITS 16
#define CLIFT_EMST_WORK_BYTES(n) (256L + (long)(n) * (3L * 8 + CLIFT_EMST_SPLITS * 8L + 5L * 4 + CLIFT_EMST_SPLITS * 4L))
long clift_emst_work_bytes(long n);      /* CLIFT_EMST_WORK_BYTES(n) for callers that cannot see the macro */
int clift_emst(const float* X, long n, int ldx, int d, int* edge_a, int* edge_b, double* edge_w, int* info, void* work, long work_bytes,
               clift_stream_t s);

/* ---- linear assignment (ABI 27; csrc/assign.hip): the Hungarian step of the reference's "linear_assignment" instance loss
 * (trainer/train_panopli_tensorf.py:237-242, 332-342; scipy.optimize.linear_sum_assignment on the host there) and that loss for one image.
 *
 * clift_lsap solves nb independent rectangular problems: minimise sum_r cost[r][col_of_row[r]] over assignments with distinct columns.  cost: fp32,
 * row-major L x E with leading dimension ld >= E, problem b at cost + b * batch_stride (floats; any value >= 0, 0 = the same matrix nb times).
 * 0 <= L <= E <= CLIFT_LSAP_MAX_E.  col_of_row (nb, L) int32; total (nb) fp64, nullable: the optimum, summed in row order in fp64.  An entry
 * counts as np.nan_to_num makes it: NaN = 0, +-inf = +-FLT_MAX.  Shortest augmenting paths (Jonker-Volgenant, scipy's method), duals, path lengths
 * and the running minimum in fp64: scipy's assignment whenever the optimum is unique.  Ties between columns: a column without a row first, then
 * the lowest index.  One wave per problem, one workgroup each; the matrix is staged in LDS when L * E * 4 <= 144 KiB, else read through L2.
 * Errors: a negative size, L > E, E > CLIFT_LSAP_MAX_E, ld < E, batch_stride < 0, a NULL cost / col_of_row.  nb == 0 or L == 0 returns 0 at once.
 *
 * clift_assign_loss: one image of the loss.  scores (n, ld) fp32, labels (n) int32 (any values; id 0 is an id like every other), conf (n) fp32
 * (NULL = all 1).  In this order:
 *   1. ids (E) = the distinct labels, ascending, the first E of them; n_ids (1) = L <= E; ids[L..E) = 0;
 *   2. p_i = softmax(scores_i) in fp32; S[l][e] = sum of p_i[e] over the rays with labels_i == ids[l] (a masked sum: other rays are not read),
 *      fp64, in ray order; cost[l][e] = -(float(S[l][e]) / (float(count_l) + 1e-4f)).  cost (E, E) fp32, rows [0, L) written, nullable;
 *   3. slot_of_id (E) = the clift_lsap solution of that L x E matrix (the same device code); slot_of_id[L..E) = 0;
 *   4. target_i (n) = slot_of_id[l] where labels_i == ids[l], l < L, else 0;
 *   5. active (1) = 1 if any target_i != argmax_e scores_i[e] (lowest index among maxima), else 0;
 *   6. active: loss (1) = (1/n) sum_i conf_i CE(scores_i, target_i), the rows added in a fixed order; grad (n, ldg; nullable) =
 *      (conf_i / n)(softmax(scores_i) - onehot(target_i)); the per-ray arithmetic is clift_semantic_loss_rows';
 *   7. not active: loss = 0 and grad is WRITTEN as zeros ("should never reinforce correct labels": the term is a constant).
 * No floating-point atomic anywhere: two calls on one input give the same bits in every output.  n <= 8192 sorts the labels in LDS; a larger n
 * extracts one id per pass over the labels (slow, exact).  2 <= E <= CLIFT_LSAP_MAX_E, 1 <= n <= CLIFT_ASSIGN_MAX_N.  work: a device buffer of at
 * least CLIFT_ASSIGN_WORK_BYTES(n, E) bytes, 16-byte aligned, contents irrelevant before and undefined after.  Seven launches on the stream, no
 * synchronisation, no allocation.  Errors: sizes out of range, ld < E, ldg < E with a grad, a NULL required buffer, work misaligned or too small. */
#define CLIFT_LSAP_MAX_E 512
#define CLIFT_ASSIGN_MAX_N 1048576
#define CLIFT_ASSIGN_WORK_BYTES(n, E) (256L + 16L * ((long)(n) + 4) + 4L * (long)(E) * (long)(E))
int clift_lsap(const float* cost, int ld, long batch_stride, int nb, int L, int E, int* col_of_row, double* total, clift_stream_t s);
long clift_assign_work_bytes(long n, int E);      /* CLIFT_ASSIGN_WORK_BYTES(n, E) for callers that cannot see the macro */
int clift_assign_loss(const float* scores, int ld, const int* labels, const float* conf, int n, int E, int* ids, int* n_ids, float* cost,
                      int* slot_of_id, int* target, float* loss, float* grad, int ldg, int* active, void* work, long work_bytes, clift_stream_t s);

/* ---- instances in 3-D (ABI 20; csrc/points3d.hip): the per-instance steps of the reference's inference/visualize_bboxes.py (filter_pointcloud
 * :52-74, get_tight_bbox :78-131) for ALL instances of a scene per launch.  pts (n, 3) fp32, rows SORTED BY INSTANCE; seg (G + 1) int64 device
 * offsets, non-decreasing, 0 <= seg[g] <= n: instance g owns rows seg[g] .. seg[g+1] (may be empty).  n < 2^31 - 1024.  Entries of seg outside
 * [0, n] are clamped, never followed.
 *
 * clift_knn_kth_dist: d2_out[i] (n) fp64 = the SQUARED distance from row i to its k-th nearest row of the same instance, itself included
 * (sklearn.neighbors.KDTree(P).query(P, k)[0][:, -1], squared).  The distance of rows a, b is ((dx*dx + dy*dy) + dz*dz) with
 * dx = double(a.x) - double(b.x) (likewise dy, dz), every product and sum rounded separately to fp64 (no contraction) -- the number sklearn's
 * fp64 KD-tree computes; the k smallest of these do not depend on the order the candidates are visited in.  1 <= k <= 16.  Every row of an
 * instance with fewer than k rows gets +inf (the KD-tree raises there), and so does a row outside [seg[0], seg[G]). */
int clift_knn_kth_dist(const float* pts, long n, const long* seg, int G, int k, double* d2_out, clift_stream_t s);
/* clift_segment_moments: out (G, 10) fp64, per instance over its rows i with keep[i] != 0 (keep (n) uint8; NULL = all rows), with
 * q = double(p) - centre[g] (centre (G, 3) fp64; NULL = zero):  count, sum qx, qy, qz, sum qx*qx, qx*qy, qx*qz, qy*qy, qy*qz, qz*qz.
 * fp64, every product and sum rounded separately, over a FIXED split of the instance's rows (row seg[g] + t + 256 j on thread t in order of j,
 * 64 threads folded by an xor butterfly, the four partials added in order): no atomics, two runs give the same bits.  An instance without
 * kept rows gets zeros.  (Two calls -- centre = NULL for the mean, then centre = mean -- give centred second moments without cancellation.) */
int clift_segment_moments(const float* pts, long n, const long* seg, int G, const unsigned char* keep, const double* centre, double* out,
                          clift_stream_t s);
/* clift_segment_extent: frame (G, 12) fp64 = the 3 x 3 axes A row-major, then the centre c.  out (G, 6) fp64 = per instance the minimum
 * (3) and the maximum (3), over its kept rows, of  v_r = ((A[r][0]*qx + A[r][1]*qy) + A[r][2]*qz),  q = double(p) - c, rounded as above.
 * An instance without kept rows gets +inf / -inf. */
int clift_segment_extent(const float* pts, long n, const long* seg, int G, const unsigned char* keep, const double* frame, double* out,
                         clift_stream_t s);
/* clift_segment_mvee (ABI 25): the minimum-volume enclosing ellipsoid of every instance's kept rows by Khachiyan's algorithm (the reference's
 * getMinVolEllipse, visualize_bboxes.py:135-189, its default get_tight_bbox method) in O(rows) work and memory per iteration, all instances in
 * ONE launch, one workgroup per instance, the loop inside the kernel.  With m = the number of kept rows of instance g, d = 3, q_i = (p_i, 1),
 * u_i = 1 / m:  repeat  V = sum u_i q_i q_i^T,  M_i = q_i^T V^-1 q_i,  j = argmax M (the LOWEST row on equal values),
 * step = (M_j - d - 1) / ((d + 1) (M_j - 1)),  u <- (1 - step) u,  u_j += step,  err = |u_new - u_old|_2  while err > tolerance (at least once)
 * and fewer than max_iter iterations were made.  Then c = sum u_i p_i and C = sum u_i p_i p_i^T - c c^T.
 * u (n) fp64: the weights; 0 on rows that are not kept and on every row of a status-2 instance.  Rows outside [seg[0], seg[G]) are not written.
 * out (G, 14) fp64 = m, iters, err, status, c (3), Cxx Cxy Cxz Cyy Cyz Czz, 0.
 * status 0: converged.  1: stopped at max_iter (c and C of the last iterate).  2: degenerate -- m < 4 (an empty instance included), or V not
 * positive definite at some iteration (a Cholesky pivot not above 1e-12 of its diagonal entry: coplanar or collinear points), or a non-finite
 * pivot, M_j or err; c, C and err are then 0.  One instance's failure touches no other instance's output.
 * Choices taken: the rows are centred on the fp64 mean of the instance's kept rows before q is formed (M is affine invariant; V stays well
 * conditioned); V follows the rank-1 form (1 - step) V + step q_j q_j^T after the first sum; M_i = |L^-1 q_i|^2 with V = L L^T (Cholesky);
 * err is the closed form |step| sqrt(|u|^2 - 2 u_j + 1) with |u|^2 carried by its own recurrence.  All arithmetic fp64, products and sums
 * rounded separately; the sums run over the fixed split of clift_segment_moments and the argmax is exact, so two runs give the same bits, u
 * included (no atomics).  Whether the loop goes on is decided by one thread per iteration and read by all from one LDS word; max_iter bounds
 * the loop unconditionally.  Errors: n or G out of range as above, max_iter outside [1, 1000000], tolerance <= 0 (or NaN), a NULL required
 * buffer.  G == 0 returns 0 before any launch. */
int clift_segment_mvee(const float* pts, long n, const long* seg, int G, const unsigned char* keep, double tolerance, int max_iter, double* u,
                       double* out, clift_stream_t s);

/* ---- scoring (ABI 22; csrc/overlap.hip): the joint histogram of two label maps, per frame, after a per-frame class remapping -- the table under
 * panoptic quality, the confusion matrix and the robust-class shares (contrastive_lift_amd/overlap.py).  Everything is DEVICE memory.  a_cls,
 * a_inst, b_cls, b_inst: (P) int32 rows, P = frame_off[F]; frame_off (F + 1) int64, non-decreasing from 0: frame f owns rows frame_off[f] ..
 * frame_off[f+1] (may be empty).  a_base, a_stride (F, Ca) and b_base, b_stride (F, Cb) int32: the slot of row i of frame f on side a is
 *     sa = a_base[f][a_cls[i]] + a_stride[f][a_cls[i]] * a_inst[i]        (sb likewise),
 * and the row adds 1 to counts[f][sa][sb], counts (F, NA, NB) int32.  In this order: a row whose class is outside [0, Ca) resp. [0, Cb) on either
 * side is REJECTED; else a row with a negative base on either side is DROPPED (counted nowhere: classes the caller leaves out, invalid pixels);
 * else a row with a non-zero stride and a NULL instance array or a negative instance id, or with a slot outside [0, NA) resp. [0, NB), on either
 * side is REJECTED.  A rejected row adds 1 to rejected[f] (F) and nothing else; the caller reads rejected and raises.  No address outside counts
 * and rejected is ever written.  a_inst / b_inst may be NULL when every stride of that side is 0.  The call clears counts and rejected on the
 * stream itself, neither allocates nor synchronises (P is read on the device: the caller vouches that the row arrays hold frame_off[F] rows and
 * that the offsets are monotone -- a piece of a non-monotone list is skipped or counted twice, never followed out of the row range).  Integer
 * adds only: two runs give the same bits.  Errors (clift_last_error): F < 0, NA or NB or Ca or Cb < 1, NA * NB >= 2^31, a NULL required
 * buffer.  F == 0 returns 0 at once; frame_off[F] == 0 leaves the cleared tables.  NA * NB <= 8192 counts in a block-private LDS table. */
int clift_label_overlap(const int* a_cls, const int* a_inst, const int* b_cls, const int* b_inst, const long* frame_off, int F,
                        const int* a_base, const int* a_stride, int Ca, const int* b_base, const int* b_stride, int Cb, int NA, int NB,
                        int* counts, int* rejected, clift_stream_t s);

/* ---- the scene as a surface (an ABI 27 addition; csrc/isosurface.hip).
 *
 * clift_dense_sigma: out (n0, n1, n2) fp32, x-major = softplus(density + shift) on a lattice of the box: lattice point p_a = lo_a (1 - s) + hi_a s
 * with s = s_a[i_a] (three device arrays, the caller's torch.linspace(0, 1, n_a)), normalised with inv_ext2 -- the coordinate arithmetic of
 * clift_alpha_bbox.  With n_a = grid_dim_a * upsample this is the reference's TensoRFRenderer.get_dense_sigma (renderer.py:731-748) in one launch.
 * Errors: comps not a multiple of 4, a dimension < 1, >= 2^36 lattice points, a NULL buffer.
 *
 * Iso-surface of a scalar lattice by MARCHING TETRAHEDRA ON THE KUHN SPLIT.  vol (n0, n1, n2) fp32, x-major: lin(i, j, k) = (i n1 + j) n2 + k.
 * "Inside" is vol >= level; NaN is outside.  Cell (i, j, k) splits into 6 tetrahedra, one per permutation (a, b, c) of the axes in lexicographic
 * order: v0 = c000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = c111.  The complex has 7 edge classes per lattice point -- offsets (1,0,0) (0,1,0) (0,0,1)
 * (1,1,0) (1,0,1) (0,1,1) (1,1,1), in this order; an edge is owned by its lower endpoint and exists when both endpoints are lattice points.  An edge
 * whose endpoints classify differently carries exactly one vertex, at p = pa + t (pb - pa), t = (level - va) / (vb - va) clamped to [0, 1] (a NaN t
 * becomes 0), a = the owner, fp32 with one rounding per operation; its INDEX is the rank of the key 7 lin(owner) + class among such edges.  A
 * tetrahedron with 1 or 3 inside corners gives one triangle; with 2 a quad, split along the diagonal through its smallest vertex index: the cycle
 * rotated to start there, (q0 q1 q2) then (q0 q2 q3).  The winding comes from a case table and the parity of the permutation, never from computed
 * positions: the normal points from inside to outside.  Faces are ordered by scan: (cell by lin, tetrahedron, triangle).  The mesh is a closed,
 * consistently oriented 2-manifold wherever the surface does not meet the lattice boundary.  No atomics: two runs give the same bits.
 *
 * Three calls; the caller scans between the first and the others (exclusive prefix sums of n_vert and n_tri over lin, int64, and ONE read of
 * the two totals V and F, which size verts and faces):
 *   clift_iso_classify: edge_mask (N) uint8 = the owned active classes of every lattice point (bit = class), n_vert (N) int32 = their number,
 *     n_tri (N) int32 = the triangles of the cell whose c000 corner the point is (0 where there is no such cell).  N = n0 n1 n2.
 *   clift_iso_vertices: verts (V, 3) fp32 world positions from the per-axis coordinate arrays x0 (n0), x1 (n1), x2 (n2); normals (V, 3) fp32,
 *     NULL skips them: minus the central-difference gradient of vol (world units, one-sided at the border) at the two endpoints, interpolated with
 *     the same t, normalised (0 0 0 where the length is zero or not finite).
 *   clift_iso_faces: faces (F, 3) int32.
 * A row outside [0, V) resp. [0, F) -- offsets that do not belong to the mask -- is never written.
 * Errors, all checked before the device is touched: N, V or F >= CLIFT_ISO_LIMIT = 2^31 (the message names the limit), a negative V or F, a NaN
 * level, a NULL buffer.  A lattice with a dimension < 2 (n <= 0 included) has no cell: every call returns 0 without a launch; so do
 * clift_iso_vertices with V == 0 and clift_iso_faces with F == 0 (an all-inside or all-outside lattice). */
#define CLIFT_ISO_LIMIT 2147483648L
int clift_dense_sigma(const clift_vm_t* h_dens, const float* h_lo3, const float* h_hi3, const float* h_inv_ext2, const float* s0,
                      const float* s1, const float* s2, int n0, int n1, int n2, float shift, float* out, clift_stream_t s);
int clift_iso_classify(const float* vol, int n0, int n1, int n2, float level, unsigned char* edge_mask, int* n_vert, int* n_tri,
                       clift_stream_t s);
int clift_iso_vertices(const float* vol, int n0, int n1, int n2, float level, const float* x0, const float* x1, const float* x2,
                       const unsigned char* edge_mask, const long* vert_off, long V, float* verts, float* normals, clift_stream_t s);
int clift_iso_faces(const float* vol, int n0, int n1, int n2, float level, const unsigned char* edge_mask, const long* vert_off,
                    const long* tri_off, long V, long F, int* faces, clift_stream_t s);

/* ---- connected components of a keyed lattice (a further ABI 27 addition; csrc/components.hip).
 *
 * key (n0, n1, n2) int32, x-major like vol: lin(i, j, k) = (i n1 + j) n2 + k; 0 is background.  Two lattice points belong together iff they are
 * neighbours under `connectivity` and carry the same non-zero key; a component is a class of the transitive closure.  connectivity: 6 = faces,
 * 26 = full, 14 = the KUHN neighbourhood +-d for the seven non-zero d in {0,1}^3 -- exactly the seven edge classes of the iso-surface entries
 * above, so that with key = (vol >= level) every face of that mesh belongs to one component of the inside set and to no second one (all vertex
 * pairs of a Kuhn tetrahedron are Kuhn edges).
 * root (N) int32, N = n0 n1 n2: root[p] = the smallest linear index of any point of p's component, -1 where key[p] == 0.  The result is defined
 * without reference to execution order: two runs give the same bits.  Union-find with link-to-smaller-root in three launches (a 4 x 8 x 16 tile
 * in LDS; the pairs across tile borders by device-scope atomic-min on the root words; a flattening pass).  No workgroup waits for another, and
 * every loop is a root chase or a union retry whose index strictly descends.  Memory: nothing beside key and root.
 * Errors, all checked before the device is touched: a dimension < 1, N >= CLIFT_ISO_LIMIT = 2^31 (the message names the limit), a connectivity
 * other than 6 / 14 / 26, a NULL buffer. */
int clift_cc_label(const int* key, int n0, int n1, int n2, int connectivity, int* root, clift_stream_t s);

/* ---- relations of a keyed lattice (a further ABI 27 addition; csrc/relations.hip): per key its extent, per ordered pair of keys
 * the faces between them and their contacts across a thin empty gap -- the counts under a scene graph (contrastive_lift_amd/relations.py).
 *
 * key (n0, n1, n2) int32, x-major as above; key 0 is background, valid keys are 0 .. n_keys - 1.  All results are integers and each is defined
 * without reference to execution order: two runs give the same bits.
 *   count (n_keys) int64: the points with key k, background included.  isum (n_keys, 3) int64: the sum of the index i_a over them.
 *   ibox (n_keys, 6) int32: min_0 min_1 min_2 max_0 max_1 max_2 of the indices; min_a = n_a and max_a = -1 for a key that no point carries.
 *   faces (n_keys, n_keys, 3) int32: every pair of lattice points (p, p + e_a) that both exist, with u = key[p], v = key[p + e_a], u != v, adds 1
 *     to faces[u][v][a] -- u is the lower point along axis a.  Background counts: faces[u][0][a] are u's free faces towards +a, faces[0][v][a]
 *     are v's free faces towards -a.  The diagonal stays 0.
 *   near, same shape, NULL exactly when gap == 0 (gap 0 .. CLIFT_REL_MAX_GAP): for every p with u = key[p] != 0 and key[p + e_a] == 0, look on
 *     along +a at d = 2 .. gap + 1 while p + d e_a is a lattice point and stop at the first non-background key v; if v != u, add 1 to
 *     near[u][v][a] (a hole in one object, u 0 u, adds nothing).  A near contact is counted from its lower side only, once.
 *   rejected (1) int32: a point whose key is outside [0, n_keys) adds 1 here and nothing else: no pair contains it, a look-through stops at it.
 * The call clears its tables on the stream itself; it neither allocates nor synchronises.  One pass over 8 x 8 x 32 tiles held in LDS with the
 * gap + 1 slabs beyond each positive face; equal keys and equal (u, v, a) are folded inside the wave before any atomic, and with
 * n_keys <= CLIFT_REL_LDS_KEYS the pair counts go to a block-private LDS table first (2 x 3 x 32 x 32 ints = 24 KiB beside the 12.2 KiB tile:
 * four 256-thread blocks per CU out of the CU's 160 KiB, which is what the fixed grid asks for); above it the folded adds go straight to memory.
 * Errors, all checked before the device is touched: a dimension < 1, N >= CLIFT_ISO_LIMIT = 2^31 (the message names the limit), n_keys outside
 * 1 .. CLIFT_REL_MAX_KEYS, gap outside 0 .. CLIFT_REL_MAX_GAP, near without gap or gap without near, a NULL required buffer. */
#define CLIFT_REL_LDS_KEYS 32
#define CLIFT_REL_MAX_KEYS 1024
#define CLIFT_REL_MAX_GAP 4
int clift_lattice_relations(const int* key, int n0, int n1, int n2, int n_keys, int gap, long* count, long* isum, int* ibox, int* faces,
                            int* near, int* rejected, clift_stream_t s);

/* ---- clearance of a keyed lattice (a further ABI 27 addition; csrc/clearance.hip): how far every key can travel along the six
 * lattice directions before it meets another key, and on how many faces it then rests -- a look of UNBOUNDED length, where `near` above stops
 * after CLIFT_REL_MAX_GAP points (contrastive_lift_amd/clearance.py; inference/edit_scene.py --settle).
 *
 * key (n0, n1, n2) int32 as above: key 0 is background, valid keys are 0 .. n_keys - 1 (1 <= n_keys <= CLIFT_REL_MAX_KEYS), N = n0 n1 n2 < 2^31.
 * Directions: d = 2a for +a, d = 2a + 1 for -a, a = 0, 1, 2.
 * Events.  In one column of the lattice along axis a take two points at indices i < j with keys u (at i) and v (at j), both valid and non-zero,
 *   u != v, and every point strictly between them of key 0: then g = j - i - 1 >= 0 is an event (u, v, 2a, g) and an event (v, u, 2a + 1, g).
 *   Two such points with u == v are no event (a rigid object does not stop on its own handle).  A point whose key lies outside [0, n_keys) is
 *   counted in `rejected` and ends the look from both sides: no event crosses it.  The lattice border is no obstacle and gives no event (the
 *   distance to it follows from ibox above).
 * Outputs, all int32, all filled by the call itself, each defined without reference to execution order (two runs give the same bits):
 *   pair (n_keys, n_keys, 6): the minimum g over the events (u, v, d, .), CLIFT_CLR_NONE where there is none; rows and columns of key 0 and the
 *     diagonal stay NONE.
 *   travel (n_keys, 6): min_v pair[u][v][d] -- the lattice steps key u can be shifted along d before its first point meets another key.
 *   landing (n_keys, n_keys, 6): the number of events (u, v, d, g) with g <= travel[u][d] + slack, slack 0 .. CLIFT_CLR_MAX_SLACK: the faces on
 *     which u rests on v once it has travelled; 0 where travel is NONE.
 *   rejected (1): as above.
 * With `faces` and `near` of clift_lattice_relations, for u, v >= 1: pair[u][v][2a] == 0 exactly where faces[u][v][a] > 0, and for gap = G >= 1
 * pair[u][v][2a] <= G exactly where faces[u][v][a] + near[u][v][a] > 0.
 * Two launches of one kernel body in stream order -- the minima by atomic-min, then the same events again for the counts --; every axis is read
 * coalesced (axes 0, 1: a lane per column; axis 2: a wave per row, the predecessor of a point from the ballot of the non-zero lanes) and a
 * column is walked whole, whatever its length.  Equal codes are folded inside the wave before any atomic; with n_keys <= CLIFT_REL_LDS_KEYS the
 * block works into a private LDS table (at most 6 x 32 x 33 ints = 24.75 KiB) first.  The call neither allocates nor synchronises.
 * Errors, all checked before the device is touched: a dimension < 1, N >= CLIFT_ISO_LIMIT = 2^31 (the message names the limit), n_keys outside
 * 1 .. CLIFT_REL_MAX_KEYS, slack outside 0 .. CLIFT_CLR_MAX_SLACK, a NULL buffer. */
#define CLIFT_CLR_MAX_SLACK 4
#define CLIFT_CLR_NONE 0x7fffffff
int clift_lattice_clearance(const int* key, int n0, int n1, int n2, int n_keys, int slack, int* pair, int* travel, int* landing, int* rejected,
                            clift_stream_t s);

/* ---- distance transform of a keyed lattice (a further ABI 27 addition; csrc/distance.hip): the exact Euclidean distance of
 * every lattice point to the nearest site, with that site carried along (a feature transform) -- where the clearance above looks along the six
 * lattice directions only (contrastive_lift_amd/distance.py; inference/extract_mesh.py --separation, inference/edit_scene.py --check_placement).
 *
 * Lattice and keys.  key (n0, n1, n2) int32, x-major: lin = (i0 n1 + i1) n2 + i2; N = n0 n1 n2 < 2^31 and every dimension is
 *   1 .. CLIFT_DT_MAX_DIM = 16384, so that dist2 <= 3 * 16383^2 < 2^31.  Valid keys are 0 .. n_keys - 1, 1 <= n_keys <= CLIFT_REL_MAX_KEYS.  A
 *   point whose key lies outside that range is counted in `rejected` (1) int32; it is no site and contributes to nothing.
 * Sites.  site: n_keys bytes on the device.  A point is a site when its key is valid and site[key] != 0.  Key 0 (background) may be a site:
 *   that gives the transform of the complement, the distance to the nearest empty point.
 * Result.  out (N) int64: out[p] = (dist2 << 31) | nearest with dist2 = min over the sites s of |p - s|^2 in index units (an integer) and
 *   nearest = the lin of a site at that distance; of several sites at that distance the one with the smallest lin.  That is: out[p] is the
 *   minimum of the packed word over all sites.  out[p] = CLIFT_DT_NONE where there is no site at all.  A site has dist2 = 0 and itself as
 *   nearest.  The rule is separable: in a pass along one axis take the packed word with its dist2 field increased by (i - j)^2 and the minimum
 *   over j; the passes z, y, x compose to the minimum over all sites.
 * Per-key minimum.  key_min (n_keys) int64, may be NULL: key_min[u] = min over the points p with key u of (dist2(p) << 31) | lin(p) for the
 *   valid keys u >= 1 -- the point of u nearest to a site, the smaller lin on a tie.  key_min[0] and the keys that no point carries stay
 *   CLIFT_DT_NONE, and so does everything when there is no site.  One 64-bit unsigned minimum per entry: the order of the atomics cannot
 *   change the result.
 * Metric.  Distances are in index units: the nearest site in index space, not in world space, is taken (the voxels of the density lattice are
 *   nearly but not exactly cubic).  World distances are formed afterwards in fp64 from the lattice ticks of p and of nearest and are exact for
 *   the pair that was chosen.  There are no per-axis weights.
 * work (N) int64 is scratch for the passes; its contents after the call are unspecified.  out and work must not overlap.  The call fills out,
 * key_min and rejected itself, on its stream; it neither allocates nor synchronises.  Two runs give the same bits.
 * Errors, all checked before the device is touched: a dimension outside 1 .. CLIFT_DT_MAX_DIM, N >= CLIFT_ISO_LIMIT = 2^31 (the message names
 * the limit), n_keys outside 1 .. CLIFT_REL_MAX_KEYS, a NULL buffer (key_min excepted), out and work overlapping. */
#define CLIFT_DT_MAX_DIM 16384
#define CLIFT_DT_NONE 0x7fffffffffffffffL
int clift_lattice_distance(const int* key, int n0, int n1, int n2, int n_keys, const unsigned char* site, long* out, long* work, long* key_min,
                           int* rejected, clift_stream_t s);

/* ---- placement map of a keyed lattice (a further ABI 27 addition; csrc/placement.hip): for EVERY translation of an object's
 * voxel shape over the lattice the number of cells that collide and the number of faces it would rest on, and the free (and supported)
 * translation nearest to a target -- where the transform above answers for one position and the clearance for one axis
 * (contrastive_lift_amd/placement.py; inference/edit_scene.py --snap_placement).
 *
 * Lattice and keys.  key (n0, n1, n2) int32, x-major, every dimension 1 .. CLIFT_DT_MAX_DIM, N = n0 n1 n2 < 2^31; valid keys are
 *   0 .. n_keys - 1, 1 <= n_keys <= CLIFT_REL_MAX_KEYS.  solid: n_keys bytes on the device.  A point is solid when its key is valid and
 *   solid[key] != 0.  A point whose key lies outside [0, n_keys) is counted in `rejected` (1) int32 and is not solid.
 * Object.  shape (m0, m1, m2) uint8 on the device, x-major, 1 <= m_a <= n_a: the object's cells in its own box, a non-zero byte is a cell.
 *   A shape without any cell gives overlap = support = 0 everywhere (every translation then counts as free, none as supported); the Python
 *   layer refuses it.
 * Direction.  d = 0 .. 5 as for the clearance: d = 2a is +a, d = 2a + 1 is -a; e_d is the unit index step along d.
 * Translations.  T = (n0 - m0 + 1, n1 - m1 + 1, n2 - m2 + 1): the object lies wholly inside the lattice with the corner of its box at t,
 *   lin_T(t) = (t0 T1 + t1) T2 + t2.  target (t0, t1, t2) by value, 0 <= target_a < T_a.
 * Outputs, all filled by the call itself, each defined without reference to execution order (two runs give the same bits):
 *   overlap (T) int32: overlap[t] = #{c in shape : solid(t + c)}, the cells that collide at t.
 *   support (T) int32: support[t] = #{c in shape : c + e_d not in shape, t + c + e_d a lattice point and solid} -- the faces of the object
 *     that look along d onto something solid.  A neighbour outside the shape's box is "not in the shape".  A neighbour outside the lattice
 *     is NOT support: the lattice border is not a floor.
 *   count (2) int32: count[0] = the number of free translations (overlap == 0), count[1] = the number of free translations that also have
 *     support >= min_support (min_support >= 1).
 *   best (2) int64: best[0] = the minimum over the free t of (|t - target|^2 << 31) | lin_T(t), best[1] the same minimum over the free and
 *     supported t; CLIFT_PM_NONE where there is none.  The squared index distance comes first, the smaller lin_T wins a tie: the packing
 *     and the argument of key_min above -- one 64-bit unsigned minimum per entry, the order of the atomics cannot change it.
 *   rejected (1): as above.
 * work: scratch of CLIFT_PM_WORK_WORDS(n0, n1, n2, m0, m1, m2) int64 words = (n0 + 2) (n1 + 2) WP + 2 (m0 + 2) (m1 + 2) MW with
 *   MW = ceil((m2 + 2) / 64) and WP = ceil((n2 - m2 + 1) / 64) + MW; its contents after the call are unspecified.
 * Three launches in stream order, integer arithmetic, vector stores and atomics only.  The lattice is bit-packed along z (the ballot of
 *   "solid" over 64 keys is one word) with one zero point around it on every side and zero words behind every row, the shape into two masks
 *   over its box grown by one: its cells, and its d-shadow {c + e_d : c in shape, c + e_d not in shape}.  overlap and support are the same
 *   correlation with the two masks: lanes run along t2, a lane's 64-bit window of a packed row is (lo >> l) | (hi << (64 - l)), ANDed with
 *   the mask word and counted.  Metric: index units, as for the distance transform.  The call neither allocates nor synchronises.
 * Errors, all checked before the device is touched: a lattice or shape dimension outside 1 .. CLIFT_DT_MAX_DIM, m_a > n_a,
 * N >= CLIFT_ISO_LIMIT = 2^31 (the message names the limit), n_keys outside 1 .. CLIFT_REL_MAX_KEYS, direction outside 0 .. 5,
 * min_support < 1, a target outside T, a NULL buffer. */
#define CLIFT_PM_NONE CLIFT_DT_NONE
#define CLIFT_PM_MASK_WORDS(m2) (((long)(m2) + 2 + 63) / 64)
#define CLIFT_PM_ROW_WORDS(n2, m2) (((long)(n2) - (m2) + 1 + 63) / 64 + CLIFT_PM_MASK_WORDS(m2))
#define CLIFT_PM_WORK_WORDS(n0, n1, n2, m0, m1, m2) \
    (((long)(n0) + 2) * ((n1) + 2) * CLIFT_PM_ROW_WORDS(n2, m2) + 2 * ((long)(m0) + 2) * ((m1) + 2) * CLIFT_PM_MASK_WORDS(m2))
int clift_lattice_placement(const int* key, int n0, int n1, int n2, int n_keys, const unsigned char* solid, const unsigned char* shape, int m0,
                            int m1, int m2, int direction, int min_support, int t0, int t1, int t2, int* overlap, int* support, int* count,
                            long* best, int* rejected, long* work, clift_stream_t s);

/* ---- surface outputs of the ray route (a further ABI 27 addition; csrc/surface.hip).
 *
 * clift_density_grad_points: out (n, 4) fp32, row = [gx, gy, gz, sigma_raw] at the normalised points xn (n, ldx >= 3), where
 *   sigma_raw(xn) = sum_i sum_c P_ic(xn[a_i], xn[b_i]) L_ic(xn[v_i]) + shift  is what clift_density_points(activation = 0) evaluates (column 3
 *   carries its bits) and g = d sigma_raw / d xn is its analytic derivative inside the cell the lookup selects by floor: on a texel line the
 *   right-sided derivative.  A tap outside the table counts as the value 0, so at the table's edge the derivative sees the step to the padding;
 *   farther than one texel outside everything is 0.  h_inv2 (host, 3 floats; the inv_ext2 of clift_march_t) scales the gradient to world units,
 *   g_a * inv2_a; NULL leaves it with respect to xn.
 *   Errors: comps not a positive multiple of 4, a table size < 1, ldx < 3, n >= 2^36, a NULL buffer.  n <= 0 returns 0 without a launch.
 *
 * clift_ray_surface: per ray of a march (the record, rays and jitter of clift_march_fwd; T, w (N, S) as it wrote them; ray_start (N + 1) and
 *   act_idx (M) of clift_scan_counts / clift_compact_fill; G (M, 4) = clift_density_grad_points at the active samples, world units), with
 *   rem_k = T[k] - w[k] and thr = 1 - q, each one fp32 subtraction, q in (0, 1):
 *     k_med[r] = min{k : rem_k <= thr}, or -1 (then depth_med[r] = 0);
 *     depth_med[r] = z_k + f delta_k,  f = den > 0 ? clamp((prev - thr) / den, 0, 1) : 0,  den = prev - rem_k,  prev = rem_{k-1} (1 for k = 0),
 *       z_k and delta_k = z_{k+1} - z_k (0 at k = S - 1) the march's own fp32 expressions;
 *     normal[r] = [sum over the ray's active samples, in list order, of w_k n_k, 0],  n = -g / |g| where |g|^2 >= 1e-30, else 0: un-normalised,
 *       its length is at most the opacity.
 *   One wave per ray, no atomics: two runs give the same bits.  M = 0 (G and act_idx may be NULL) and rays without active samples are fine.
 *   Errors: q outside (0, 1), S < 1, M < 0, N S >= 2^31 - 1, a NULL buffer.  N <= 0 returns 0 without a launch. */
int clift_density_grad_points(const clift_vm_t* h_dens, const float* xn, int ldx, long n, float shift, const float* h_inv2, float* out,
                              clift_stream_t s);
int clift_ray_surface(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* T, const float* w,
                      const int* ray_start, const int* act_idx, int M, const float* G, float q, float* depth_med, int* k_med, float* normal,
                      clift_stream_t s);

/* ---- amodal instance layers of the ray route (a further ABI 27 addition; csrc/layers.hip): per ray and per instance slot the
 * opacity, weight and distance of that instance ALONE, also where other things hide it.  Both work on a list of samples in the layout of
 * clift_scan_counts / clift_compact_fill (ray_start (N + 1), act_idx (M), ordered by ray, then by sample); the engine lists by alpha > threshold
 * rather than by w, so that samples behind an occluder are in it.
 *
 * clift_sample_slots: slot[row] for the n rows of a list, one thread per row, one launch.
 *   class    cls = the index of the first maximum of sem[row, 0 .. C): c* = 0, then for c = 1 .. C - 1: if sem[c] > sem[c*] then c* = c
 *            (a NaN never compares greater).
 *   range    (off, cnt) = cls_slots[cls], cls_slots (C, 2) int32 in DEVICE memory.  cnt <= 0 gives -1.  The range is cut to [0, K):
 *            lo = max(off, 0), hi = min(off + cnt, K), an empty cut gives -1; nothing outside centroids (K, E) is ever read and no slot
 *            outside [0, K) is ever given.
 *   feature  f_e = feat[row, e], or feat[row, e] + add[row, e] (one fp32 addition) when add (n, lda >= E) is not NULL.
 *   mode 0   nearest centroid of centroids[lo .. hi): d = f_e - c_e, d2 = d2 + d * d over e = 0 .. E - 1, EVERY operation rounded to fp32 on its
 *            own; the running minimum starts at +inf and is replaced on strict <, so the lowest index wins a tie and a row whose distances
 *            are all NaN or +inf has no winner and gets -1.  The slot is the winner's index in centroids.
 *   mode 1   for models whose instance outputs are slot scores (linear assignment): lo + the index of the first maximum (the rule of the
 *            class) of f_0 .. f_{min(hi - lo, E) - 1}.  centroids is not read and may be NULL.
 *   Separate rounding is deliberate: clift_nearest_centroid forms its distances with fmaf, which a numpy loop cannot restate; here an fp32
 *   numpy loop, one operation per statement, reproduces every label exactly.  The two may therefore disagree on a near tie.
 *   Errors: C < 1, E < 1, K < 0, K > 255, lds < C, ldf < E, lda < E with add, a mode other than 0 / 1, a NULL buffer (sem, feat, cls_slots,
 *   slot), mode 0 with K > 0 and NULL centroids.  n <= 0 returns 0 without a launch.
 *
 * clift_ray_layers: out (N, K + 1, 4) fp32 for the rays of a march (the record, rays and jitter of clift_march_fwd; alpha, w (N, S) as it wrote
 *   them).  Every list entry j carries slot[j]; a value in [0, K) is that column, anything else the rest column K.  For ray r and column c, over
 *   the entries j = ray_start[r] .. ray_start[r + 1] - 1 in list order whose column is c, with sid = act_idx[j], k = sid - r S (an entry with k
 *   outside [0, S) -- another ray's, or out of range -- is skipped, never followed), a = alpha[sid], z = z_k the march's own fp32 expression,
 *   starting from Tc = 1, V = 0, Z = 0, zf = 0, seen = false, each line ONE separately rounded fp32 operation:
 *       if !seen: zf = z, seen = true
 *       u  = Tc * a
 *       Z  = Z + (u * z)
 *       V  = V + w[sid]
 *       Tc = Tc * (1 - a)
 *   and out[r, c] = [A = 1 - Tc, V, Z, zf]: the opacity of column c rendered alone, the weight the whole scene gives it (what is visible),
 *   its un-normalised expected distance when alone, the distance of its first listed sample.  A column without entries is [0, 0, 0, 0].
 *   One wave per ray, every (ray, column) written once as one float4, no atomics and no LDS: two runs give the same bits.  ray_start is
 *   clamped to [0, M].  M = 0 (act_idx and slot may be NULL) is fine: every row is zeros.
 *   Errors: K < 0, K > 255, S < 1, M < 0, N S >= 2^31 - 1, a NULL buffer, NULL act_idx / slot with M > 0.  N <= 0 returns 0 without a launch. */
int clift_sample_slots(const float* sem, int lds, int C, const float* feat, int ldf, int E, const float* add, int lda, const int* cls_slots,
                       const float* centroids, int K, int mode, long n, int* slot, clift_stream_t s);
int clift_ray_layers(const clift_march_t* h_m, const float* rays, const float* jitter, int N, const float* alpha, const float* w,
                     const int* ray_start, const int* act_idx, int M, const int* slot, int K, float* out /* (N, K+1, 4) */, clift_stream_t s);

/* ---- amodal colour layers (a further ABI 27 addition; csrc/layers.hip): the colour of every column of clift_ray_layers when
 * rendered alone, from one colour per list row.
 *
 * clift_ray_layer_colour: out (N, K + 1, 4) fp32 rows [R, G, B, A], column K the rest.  alpha (N, S) as the march wrote it (S = h_m->n_samples,
 *   the only field of the record that is read); ray_start, act_idx, M, slot, K exactly what clift_ray_layers takes, with its column rule (a
 *   slot in [0, K) is that column, anything else column K) and its skip rule (an entry with k = act_idx[j] - r S outside [0, S) is skipped,
 *   never followed; ray_start is clamped to [0, M]).  rgb (n_rgb, ldc >= 3) fp32 holds one row of colours per coloured list row; rgb_row (M)
 *   int32 names the row of rgb that belongs to list row j, NULL means j itself.  An entry whose rgb_row lies outside [0, n_rgb) takes part in
 *   the transmittance of its column but adds no colour, and rgb is not read for it.  Per entry of column c in list order, from Tc = 1,
 *   R = G = B = 0, each operation ONE separately rounded fp32 operation (no fma):
 *       u  = Tc * a
 *       R  = R + (u * r);  G = G + (u * g);  B = B + (u * b)        (a coloured entry only)
 *       Tc = Tc * (1 - a)
 *   and A = 1 - Tc: the colour is premultiplied and knows no background; A has the bits of column 0 of clift_ray_layers on the same inputs.
 *   One wave per ray, every (ray, column) written once as one float4, no atomics, no LDS: two runs give the same bits.  M = 0 (act_idx, slot,
 *   rgb_row and rgb may be NULL) writes zeros.
 *   Errors: a NULL record, K < 0, K > 255, S < 1, M < 0, ldc < 3, n_rgb < 0, N S >= 2^31 - 1, NULL alpha / ray_start / out, NULL act_idx / slot
 *   with M > 0, NULL rgb with n_rgb > 0.  N <= 0 returns 0 without a launch. */
int clift_ray_layer_colour(const clift_march_t* h_m, int N, const float* alpha, const int* ray_start, const int* act_idx, int M,
                           const int* slot, int K, const float* rgb, int ldc, long n_rgb, const int* rgb_row, float* out /* (N, K+1, 4) */,
                           clift_stream_t s);

/* ---- surface outputs of an EDITED scene (a further ABI 27 addition; csrc/edit.hip): the gradient of the raw density of the
 * scene an edit program describes.  The walk of clift_edit_list_points remaps a world point p h times, by the edits i_1 .. i_h in walk order,
 * and ends at p' = J p + b with J = M_{i_h} ... M_{i_1} (the identity for h = 0; formed in fp32, every multiply and add rounded separately).
 * The edited raw density is sigma_e(p) = sigma_raw(p'), and away from box faces its world gradient is J^T g', g' the world gradient of the
 * unedited field at p' (clift_density_grad_points with h_inv2).  J^T, not an inverse: this holds for every affine map, rigid or not.  The
 * step of sigma_e across a box face is not part of the gradient.
 *
 * clift_edit_list_density_grad_points: pts (n, ldp >= 3) world points; h_lo3, h_inv2 (host, 3 floats each: lo and inv_ext2 of
 *   clift_march_t) normalise the walked point, xn = (p' - lo) * inv2 - 1 with separately rounded ops; out (n, 4) fp32 rows
 *   [gx, gy, gz, sigma_raw(p')], a killed row all zeros (no table is read for it); state (n) uint8 or NULL, the byte of clift_edit_list_points.
 *   Column 3 of a row that is not killed carries the bits of clift_density_points(activation = 0) at xn; a row that is neither remapped nor
 *   killed carries all four columns of clift_density_grad_points at xn.  No aabb test: a point outside the box reads zero padding.
 *   Errors: the program's, comps not a positive multiple of 4, a table size < 1, ldp < 3, n < 0 or >= 2^36, a NULL buffer.  n == 0 returns 0
 *   without a launch.
 * clift_edit_list_density_grad_active: the same for the active samples of a march under the program (the record and rays of
 *   clift_edit_list_active, act_idx (M) of clift_compact_fill): the point of row s is formed from its ray and sample index with the very
 *   operations of clift_edit_list_active, lo / inv_ext2 / density_shift come from the march record; out (M, 4).  The same world point gives
 *   the same bits in both entry points.  Rows past the dynamic row limit are not written.  M <= 0 returns 0 without a launch.
 * Both: one writer per element, no atomics -- two runs give the same bits. */
int clift_edit_list_density_grad_points(const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens, const float* pts, int ldp, long n,
                                        const float* h_lo3, const float* h_inv2, float shift, float* out, unsigned char* state,
                                        clift_stream_t s);
int clift_edit_list_density_grad_active(const clift_march_t* h_m, const clift_edit_t* h_edits, int n_edits, const clift_vm_t* h_dens,
                                        const float* rays, const int* act_idx, int M, float* out, clift_stream_t s);

/* ---- optimiser plumbing on flat fp32 ranges: torch.optim.Adam semantics (L2 weight decay folded into the
 * gradient; bias correction with step >= 1) and the slow-net EMA (trainer T:325-329). */
int clift_adam(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
               float weight_decay, int step, clift_stream_t s);
int clift_ema(float* slow, const float* fast, long n, float momentum, clift_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* CLIFT_H */
