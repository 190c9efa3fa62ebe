#!/usr/bin/env python3
"""Run the iso-surface kernels' own code on the CPU, under the address and undefined-behaviour sanitizers, against the numpy restatement.

    python tools/iso_host_check.py [--cxx g++] [--keep DIR]

The device functions and the three kernels of csrc/isosurface.hip (everything between ``iso_class_bits`` and the host entry points) are
copied verbatim into a stand-alone C++ program behind a small shim (``__global__`` and friends defined away, ``blockIdx`` / ``threadIdx``
as globals, the ``__f*_rn`` intrinsics as single fp32 operations), with a loop over blocks and threads around each kernel body and a
serial exclusive scan between the passes.  The program is built with ``-fsanitize=address,undefined -ffp-contract=off`` and run on every
case of tests/mesh_cases.py (closed cases, the open surface, a field with NaN and infinity, all 256 single cells); keys, positions,
faces with their order, and normals are compared with the restatement bit for bit.  An out-of-bounds index or a wrong table entry shows
here, without a GPU.  No GPU code is run and nothing is preloaded: the sanitizers are linked into the program itself.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import mesh_cases as mc                                         # noqa: E402

SHIM = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct D3 { long x; };
static D3 blockIdx, threadIdx; static D3 blockDim = {256};
static inline int __popc(int x) { return __builtin_popcount((unsigned)x); }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fsqrt_rn(float a) { return sqrtf(a); }
using std::max; using std::min; using std::isfinite;
'''
MAIN = r'''
#define EACH_THREAD(call) for (long b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) { blockIdx.x = b; threadIdx.x = t; call; }
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); int n[3]; float level;
    if (!f || fread(n, 4, 3, f) != 3 || fread(&level, 4, 1, f) != 1) return 2;
    long N = (long)n[0] * n[1] * n[2];
    float* vol = (float*)malloc(N * 4); if (fread(vol, 4, N, f) != (size_t)N) return 2;
    float* x[3]; for (int a = 0; a < 3; a++) { x[a] = (float*)malloc(n[a] * 4); if (fread(x[a], 4, n[a], f) != (size_t)n[a]) return 2; }
    fclose(f);
    unsigned char* mask = (unsigned char*)malloc(N); int* nv = (int*)malloc(N * 4); int* nt = (int*)malloc(N * 4);
    long blocks = (N + 255) / 256;
    EACH_THREAD(k_iso_classify(vol, n[0], n[1], n[2], level, mask, nv, nt))
    long* vo = (long*)malloc(N * 8); long* to = (long*)malloc(N * 8); long V = 0, F = 0;
    for (long p = 0; p < N; p++) { vo[p] = V; V += nv[p]; to[p] = F; F += nt[p]; }
    float* verts = (float*)malloc(V * 12); float* nrm = (float*)malloc(V * 12); int* faces = (int*)malloc(F * 12);   /* exact sizes: ASan sees one row too far */
    memset(verts, 0xff, V * 12); memset(nrm, 0xff, V * 12); memset(faces, 0xff, F * 12);
    EACH_THREAD(k_iso_vertices(vol, n[0], n[1], n[2], level, x[0], x[1], x[2], mask, vo, V, verts, nrm))
    EACH_THREAD(k_iso_faces(vol, n[0], n[1], n[2], level, mask, vo, to, V, F, faces))
    FILE* o = fopen(argv[2], "wb"); fwrite(&V, 8, 1, o); fwrite(&F, 8, 1, o); fwrite(verts, 4, V * 3, o); fwrite(nrm, 4, V * 3, o); fwrite(faces, 4, F * 3, o);
    for (long p = 0; p < N; p++) for (int c = 0; c < 7; c++) if ((mask[p] >> c) & 1) { long k = 7 * p + c; fwrite(&k, 8, 1, o); }
    fclose(o);
    free(vol); free(mask); free(nv); free(nt); free(vo); free(to); free(verts); free(nrm); free(faces); for (int a = 0; a < 3; a++) free(x[a]);
    return 0;
}
'''


def build(cxx, work):
    src = open(os.path.join(REPO, "contrastive_lift_amd", "csrc", "isosurface.hip")).read()
    body = src[src.index("__device__ __forceinline__ int iso_class_bits"):src.index("// the lattice size every iso-surface call checks")]
    cpp, exe = os.path.join(work, "iso_host.cpp"), os.path.join(work, "iso_host")
    with open(cpp, "w") as f:
        f.write(SHIM + body + MAIN)
    subprocess.run([cxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe, cpp], check=True)
    return exe


def run(exe, work, case):
    inp, out = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array(case["vol"].shape, np.int32).tobytes() + np.float32(case["level"]).tobytes() + np.ascontiguousarray(case["vol"], np.float32).tobytes())
        for t in case["ticks"]:
            f.write(np.asarray(t, np.float32).tobytes())
    subprocess.run([exe, inp, out], check=True)
    b = open(out, "rb").read()
    V, F = (int(v) for v in np.frombuffer(b[:16], np.int64))
    o = 16
    verts = np.frombuffer(b, np.float32, V * 3, o).reshape(-1, 3)
    normals = np.frombuffer(b, np.float32, V * 3, o + V * 12).reshape(-1, 3)
    faces = np.frombuffer(b, np.int32, F * 3, o + V * 24).reshape(-1, 3)
    keys = np.frombuffer(b, np.int64, -1, o + V * 24 + F * 12)
    return keys, verts, normals, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", default=None, help="directory to build in and keep (default: a temporary one)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        os.makedirs(work, exist_ok=True)
        exe = build(a.cxx, work)
        odd = mc.random_case(5)
        odd["vol"][3, 4, 5], odd["vol"][2, 2, 2], odd["name"] = np.nan, np.inf, "nonfinite"
        cases = mc.closed_cases() + [mc.open_case(), odd] + [mc.single_cell_case(p) for p in range(256)]
        for c in cases:
            keys, verts, normals, faces = run(exe, work, c)
            rk, rv, rf = mc.marching_tetrahedra(c["vol"], c["level"], c["ticks"])
            assert np.array_equal(keys, rk), (c["name"], "keys")
            assert verts.tobytes() == rv.tobytes(), (c["name"], "positions", mc.ulp_distance(verts, rv))
            assert np.array_equal(faces, rf), (c["name"], "faces or their order")
            if len(rk):
                assert normals.tobytes() == mc.vertex_normals(c["vol"], c["level"], c["ticks"], rk).tobytes(), (c["name"], "normals")
            if not c["name"].startswith("cell"):
                print(f"{c['name']}: {len(keys)} vertices, {len(faces)} faces: keys, positions, faces (order included) and normals bit-equal")
        print(f"all {len(cases)} cases equal the restatement; no sanitizer report")


if __name__ == "__main__":
    main()
