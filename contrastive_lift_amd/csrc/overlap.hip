// overlap.hip -- the joint histogram of two label maps, per frame, after a per-frame class remapping: the one primitive under panoptic quality
// (segment intersections, areas, void overlaps), the confusion matrix and the per-frame class shares of the robust-class filter
// (contrastive_lift_amd/overlap.py, metrics.py).  Integer counting only: the result is the same bits on every run, in any order of the adds.
//
// Row i of frame f (rows frame_off[f] .. frame_off[f+1]) goes to slot  sa = a_base[f][a_cls[i]] + a_stride[f][a_cls[i]] * a_inst[i]  on side a,
// sb likewise on side b, and adds 1 to counts[f][sa][sb] (the rules for dropped and rejected rows: clift.h).
//
// Layout: the row axis is cut into OV_BLOCK_ROWS-row pieces and every block of a fixed grid takes one contiguous run of pieces; a block finds
// the frame of its first row by a binary search in frame_off (as points3d.hip does for instances) and walks on from there, so one 100 000-pixel
// frame and two hundred 37-pixel frames fill the machine alike and nothing is built on the host.  The row count is frame_off[F], read on the
// device: the host never sees it and the call does not synchronise.
//
// Skewed keys: label images are piecewise constant, so most of a wave's 64 lanes hold the same (sa, sb) and one stuff segment can own half a
// frame -- one atomic per pixel would serialise on a handful of addresses.  Equal keys are folded inside the wave first (wave_fold_equal of
// clift_dev.h) and the leader alone adds their popcount: a wave of one key costs one atomic, 64 distinct keys the same atomics as before.
//
// LDS tables: when NA * NB <= OV_LDS_INTS = 8192 ints (32 KiB: five 256-thread blocks per CU out of the CU's 160 KiB, the same budget as the
// candidate tile of points3d.hip, and above the 4 blocks per CU the fixed grid asks for) the block counts into a private table in LDS and adds
// only its non-zero entries to memory when it leaves a frame -- with several pieces of one frame per block, one flush per ~P / grid rows.  Larger
// tables (scene-level scoring: thousands x a thousand slots) take the wave-folded atomics straight to memory.
//
// The piece size is reasoned, not tuned: clearing and scanning a full 8192-entry table is 64 LDS steps per thread, so a block should own at least
// as many row steps (16 per piece) for the table not to dominate; smaller pieces were not measured.  Its price is at the small end: a 100 000-pixel
// view is 25 pieces, so 25 of the grid's blocks work and the others leave after one load of frame_off[F] -- such a call is bound by its launch.
#include "clift_dev.h"

#define OV_THREADS 256
#define OV_BLOCK_ROWS 4096
#define OV_LDS_INTS 8192

struct OvArgs {
    const int* a_cls; const int* a_inst; const int* b_cls; const int* b_inst;
    const long* frame_off;
    const int* a_base; const int* a_stride; const int* b_base; const int* b_stride;
    int* counts; int* rejected;
    int F, Ca, Cb, NA, NB;
};

// slot of one side: 0 = counted (slot set), 1 = dropped, 2 = rejected.  The class is known to be inside [0, C) here.
__device__ __forceinline__ int ov_slot(const int* __restrict__ base, const int* __restrict__ stride, const int* __restrict__ inst, int cls, long i,
                                       int N, int& slot) {
    const int b = base[cls];
    if (b < 0) return 1;
    const int st = stride[cls];
    long s = (long)b;
    if (st != 0) {
        if (inst == nullptr) return 2;
        const int v = inst[i];
        if (v < 0) return 2;
        s += (long)st * (long)v;
    }
    if (s < 0 || s >= (long)N) return 2;
    slot = (int)s;
    return 0;
}

template <bool LDS>
__global__ __launch_bounds__(OV_THREADS) void k_label_overlap(const OvArgs g) {
    __shared__ int tab[LDS ? OV_LDS_INTS : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int F = g.F, NAB = g.NA * g.NB;
    const long P = g.frame_off[F];
    if (P <= 0) return;
    const long pieces = (P + OV_BLOCK_ROWS - 1) / OV_BLOCK_ROWS;
    const long per = (pieces + gridDim.x - 1) / gridDim.x * OV_BLOCK_ROWS;          // rows per block: whole pieces
    const long R0 = (long)blockIdx.x * per;
    const long R1 = R0 + per < P ? R0 + per : P;
    if (R0 >= R1) return;
    // frame of row R0: the last f with frame_off[f] <= R0 (empty frames in between are skipped by the upper bound); 0 when there is none
    int lo_f = 0, hi_f = F + 1;
    while (lo_f < hi_f) {
        const int m = (lo_f + hi_f) >> 1;
        if (g.frame_off[m] <= R0) lo_f = m + 1; else hi_f = m;
    }
    for (int f = lo_f > 0 ? lo_f - 1 : 0; f < F; ++f) {                              // everything in this loop header is block-uniform
        const long o0 = g.frame_off[f], o1 = g.frame_off[f + 1];
        if (o0 >= R1) break;
        const long lo = o0 > R0 ? o0 : R0, hi = o1 < R1 ? o1 : R1;                 // inside [R0, R1), itself inside [0, frame_off[F])
        if (lo >= hi) continue;
        const int* __restrict__ ab = g.a_base + (long)f * g.Ca;
        const int* __restrict__ as = g.a_stride + (long)f * g.Ca;
        const int* __restrict__ bb = g.b_base + (long)f * g.Cb;
        const int* __restrict__ bs = g.b_stride + (long)f * g.Cb;
        int* __restrict__ dst = g.counts + (long)f * NAB;
        if (LDS) {
            for (int e = tid; e < NAB; e += OV_THREADS) tab[e] = 0;
            __syncthreads();
        }
        int rej = 0;
        for (long i0 = lo; i0 < hi; i0 += OV_THREADS) {
            const long i = i0 + tid;
            int key = -1;
            if (i < hi) {
                const int ca = g.a_cls[i], cb = g.b_cls[i];
                if (ca < 0 || ca >= g.Ca || cb < 0 || cb >= g.Cb) {
                    rej += 1;
                } else {
                    int sa = 0, sb = 0;
                    const int ra = ov_slot(ab, as, g.a_inst, ca, i, g.NA, sa);
                    const int rb = ov_slot(bb, bs, g.b_inst, cb, i, g.NB, sb);
                    if (ra == 1 || rb == 1) {
                        // dropped: a negative base on either side wins over everything but a class outside its table
                    } else if (ra == 2 || rb == 2) {
                        rej += 1;
                    } else {
                        key = sa * g.NB + sb;                                        // < NA * NB <= INT_MAX (checked on the host)
                    }
                }
            }
            wave_fold_equal(key, [&](int k, unsigned long long same, int leader) {
                if (lane == leader) atomicAdd(LDS ? &tab[k] : &dst[k], __popcll(same));
            });
        }
        rej = wave_sum_i(rej);
        if (lane == 0 && rej != 0) atomicAdd(&g.rejected[f], rej);
        if (LDS) {
            __syncthreads();
            for (int e = tid; e < NAB; e += OV_THREADS) {
                const int v = tab[e];
                if (v != 0) atomicAdd(&dst[e], v);
            }
            __syncthreads();                                                         // the next frame clears the table
        }
    }
}

extern "C" int clift_label_overlap(const int* a_cls, const int* a_inst, const int* b_cls, const int* b_inst, const long* frame_off, int F,
                                   const int* a_base, const int* a_stride, int Ca, const int* b_base, const int* b_stride, int Cb, int NA,
                                   int NB, int* counts, int* rejected, clift_stream_t s) {
    CLIFT_REQUIRE(F >= 0, "clift_label_overlap: need F >= 0 (got %d)", F);
    CLIFT_REQUIRE(NA >= 1 && NB >= 1, "clift_label_overlap: need NA >= 1 and NB >= 1 (got %d, %d)", NA, NB);
    CLIFT_REQUIRE(Ca >= 1 && Cb >= 1, "clift_label_overlap: need Ca >= 1 and Cb >= 1 (got %d, %d)", Ca, Cb);
    CLIFT_REQUIRE((long)NA * (long)NB <= 0x7fffffffL, "clift_label_overlap: NA * NB = %ld does not fit an int", (long)NA * (long)NB);
    if (F == 0) return 0;
    CLIFT_REQUIRE(a_cls != nullptr && b_cls != nullptr && frame_off != nullptr && a_base != nullptr && a_stride != nullptr &&
                  b_base != nullptr && b_stride != nullptr && counts != nullptr && rejected != nullptr, "clift_label_overlap: NULL buffer");
    const hipStream_t st = as_stream(s);
    const long nab = (long)NA * (long)NB;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)F * (size_t)nab * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(rejected, 0, (size_t)F * sizeof(int), st);
    if (e != hipSuccess) {
        clift_set_error("clift_label_overlap: clearing the tables failed: %s", hipGetErrorString(e));
        return 2;
    }
    OvArgs g;
    g.a_cls = a_cls; g.a_inst = a_inst; g.b_cls = b_cls; g.b_inst = b_inst; g.frame_off = frame_off;
    g.a_base = a_base; g.a_stride = a_stride; g.b_base = b_base; g.b_stride = b_stride;
    g.counts = counts; g.rejected = rejected;
    g.F = F; g.Ca = Ca; g.Cb = Cb; g.NA = NA; g.NB = NB;
    const int blocks = clift_persistent_cus() * 4;
    if (nab <= OV_LDS_INTS) k_label_overlap<true><<<blocks, OV_THREADS, 0, st>>>(g);
    else                    k_label_overlap<false><<<blocks, OV_THREADS, 0, st>>>(g);
    return clift_check_launch("clift_label_overlap");
}
