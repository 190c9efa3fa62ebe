#!/usr/bin/env python3
"""Generate golden G25 (scene-editing renders) by running the REFERENCE's own four edit methods on the CPU (build container only).

    python tests/golden/make_edit_golden.py            # needs the reference checkout of make_golden.py (read-only, never copied)

``TensoRFRenderer.forward_delete / forward_extract / forward_duplicate / forward_manipulate`` (model/renderer/panopli_tensoRF_renderer.py:
303-623) on G6's scene (seed 61, grid 9 x 13 x 17, C = 4, E = 3, 96 rays, S = 38), semantic_weight_mode "softmax" and "none", black and
white background.  One box (extent (0.9, 0.8, 0.7), position (0.05, -0.02, 0.03), yawed 0.6 rad about z) and one motion (translation
(0.3, 0.15, -0.1), rotation = the same yaw).  ``forward_duplicate`` holds a ``torch.eye(3).cuda()`` (:462): ``torch.Tensor.cuda`` is swapped
for the identity around that one call -- it contributes no arithmetic.  Inputs and the four outputs per case are stored; parameters are
not (rebuilt from the seed, like every other fixture).

The generator fails unless
  * the edit shows: each method's depth differs from the unedited ``forward`` (perturb 0, is_train False) by at least 0.05 on some ray, in
    every mode / background case;
  * few samples sit on a box face: a ray is "on a face" when any of its samples has a box-frame coordinate, computed in fp64 from the
    reference's fp32 sample points, within 1e-5 of a face plane of the source box or of either destination box (a port that classifies
    with other fp32 roundings than the reference's 4 x 4 inverse may put such a sample on the other side).  The ray mask is stored
    (``on_face``); at most 4 of the 96 rays may be in it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (helpers only: stand-ins, scene, reference model / renderer builders)

EXTENT, POSITION, YAW = (0.9, 0.8, 0.7), (0.05, -0.02, 0.03), 0.6
TRANSLATION = (0.3, 0.15, -0.1)
MIN_DEPTH_CHANGE, FACE_EPS, FACE_CAP = 0.05, 1e-5, 4


def yaw_matrix(a):
    c, s = np.cos(a), np.sin(a)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def near_face(pts64, axes_cols, centre, extent):
    """(N, S) bool: some box-frame coordinate (axes = COLUMNS of ``axes_cols``) within FACE_EPS of +-extent / 2."""
    q = (pts64 - centre) @ axes_cols
    return (np.abs(np.abs(q) - extent / 2) < FACE_EPS).any(-1)


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f"reference not found at {mg.REF}: golden vectors can only be regenerated in the build container")
    torch.set_num_threads(4)
    mg.install_stand_ins()
    import model.renderer.panopli_tensoRF_renderer as RR
    res, C, E = (9, 13, 17), 4, 3
    aabb = torch.tensor([[-0.9, -0.7, -0.5], [0.8, 0.7, 0.6]])
    P, rays, _ = mg._scene(61, res, C, E, aabb, 96)
    bbox = {"extent": torch.tensor(EXTENT), "position": torch.tensor(POSITION), "orientation": yaw_matrix(YAW)}
    t, R = torch.tensor(TRANSLATION), yaw_matrix(YAW)
    out = dict(res=np.array(res), C=C, E=E, seed=61, shift=-3.0, aabb=aabb, rays=rays, extent=bbox["extent"], position=bbox["position"],
               orientation=bbox["orientation"], translation=t, rotation=R)
    for mode in ("softmax", "none"):
        for white in (False, True):
            tag = f"{mode}_{'w' if white else 'b'}"
            m = mg.build_reference_model(P, res, C, E, shift=-3.0, softmax=(mode == "softmax"))
            rr = mg.build_reference_renderer(aabb, res, mode)
            with torch.no_grad():
                base_depth = rr.forward(m, rays, 0, white, False)[3]
            results = {"delete": rr.forward_delete(m, rays, white, bbox), "extract": rr.forward_extract(m, rays, white, bbox),
                       "manipulate": rr.forward_manipulate(m, rays, white, bbox, t, R)}
            real_cuda = torch.Tensor.cuda
            torch.Tensor.cuda = lambda self, *a, **k: self              # renderer.py:462 torch.eye(3).cuda(): no arithmetic
            try:
                results["duplicate"] = rr.forward_duplicate(m, rays, white, bbox, t, R)
            finally:
                torch.Tensor.cuda = real_cuda
            for op, (rgb, sem, inst, depth) in results.items():
                change = float((depth - base_depth).abs().max())
                print(f"{tag} {op}: max depth change against forward {change:.4f}")
                assert change >= MIN_DEPTH_CHANGE, (tag, op, change)
                assert all(bool(torch.isfinite(x).all()) for x in (rgb, sem, inst, depth)), (tag, op)
                out.update({f"{tag}.{op}.rgb": rgb, f"{tag}.{op}.sem": sem, f"{tag}.{op}.inst": inst, f"{tag}.{op}.depth": depth})
    rr = mg.build_reference_renderer(aabb, res, "softmax")
    out["n_samples"] = rr.n_samples
    pts = RR.sample_points_in_box(rays, rr.bbox_aabb, rr.n_samples, rr.step_size, 0, False)[0].double().numpy()
    O, pos, ext = bbox["orientation"].double().numpy(), bbox["position"].double().numpy(), bbox["extent"].double().numpy()
    R64, t64 = R.double().numpy(), t.double().numpy()
    faces = {"src": near_face(pts, O, pos, ext), "dst_duplicate": near_face(pts, R64 @ O, R64 @ pos + t64, ext),
             "dst_manipulate": near_face(pts, R64 @ O, pos + t64, ext)}
    for k, f in faces.items():
        print(f"rays with a sample within {FACE_EPS} of a face of {k}: {int(f.any(-1).sum())} of {rays.shape[0]}")
    on_face = np.any([f.any(-1) for f in faces.values()], axis=0)
    assert int(on_face.sum()) <= FACE_CAP, int(on_face.sum())
    out["on_face"] = on_face
    mg.npz("g25_scene_edit", **out)


if __name__ == "__main__":
    main()
