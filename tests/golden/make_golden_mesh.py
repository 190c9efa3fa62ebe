#!/usr/bin/env python3
"""Generate golden G27 (the scene as a volume) by running the REFERENCE's own methods on the CPU (build container only).

    python tests/golden/make_golden_mesh.py            # needs the reference checkout of make_golden.py (read-only, never copied)

``TensoRFRenderer.get_dense_sigma(m, upsample)`` for upsample 1 and 2 and ``get_instance_clusters(m, mode)`` for 'alpha' and 'full'
(model/renderer/panopli_tensoRF_renderer.py:731-748, 636-666) on the set-up of G10: grid (9, 13, 17), seed 101, G10's box, blob amplitude
2.5 / sigma_g 0.3, density shift -3, C = 2, E = 3 (slow-fast: the instance head returns 6 columns).  ``random.seed(0)`` is called before
EACH ``get_instance_clusters`` call.  Parameters are not stored (rebuilt from the seed, like every other fixture).

Also stored, for the tests' near-tie rule: per voxel (x-major) the gap between the two largest instance outputs (``inst_gap``), the number
of voxels whose gap is below 1e-4 (``n_near_tie``), and the smallest relative distance of any voxel's alpha from ``alpha_mask_threshold``
(``alpha_margin``: a port whose alpha differs in the last bits keeps the same voxels while this stays far above fp32 round-off).

The generator fails unless the near-tie share is at most 1 % and the alpha margin at least 1e-4; the seed would change, not the caps.
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (helpers only: stand-ins, reference model / renderer builders, npz)

SEED, RES, C, E, SHIFT = 101, (9, 13, 17), 2, 3, -3.0
TIE_GAP, TIE_SHARE, ALPHA_MARGIN = 1e-4, 0.01, 1e-4


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f"reference not found at {mg.REF}: golden vectors can only be regenerated in the build container")
    torch.set_num_threads(4)
    mg.install_stand_ins()
    aabb = torch.tensor([[-0.9, -0.7, -0.5], [0.8, 0.7, 0.6]])
    P = mg.op.add_blob(mg.op.make_params(SEED, RES, C, E), RES, amplitude=2.5, sigma_g=0.3)
    m = mg.build_reference_model(P, RES, C, E, shift=SHIFT)
    rr = mg.build_reference_renderer(aabb, RES, "softmax")
    out = dict(res=np.array(RES), seed=SEED, aabb=aabb, shift=SHIFT, C=C, E=E, alpha_mask_threshold=rr.alpha_mask_threshold)
    with torch.no_grad():
        for u in (1, 2):
            out[f"sigma_u{u}"] = rr.get_dense_sigma(m, u)
        for mode in ("alpha", "full"):
            random.seed(0)
            xyz, labels = rr.get_instance_clusters(m, mode)
            out[f"{mode}.xyz"], out[f"{mode}.labels"] = xyz, labels
            print(f"get_instance_clusters({mode!r}): {xyz.shape[0]} voxels, labels {sorted(set(labels.tolist()))}")
        alpha, dense_xyz = rr.get_dense_alpha(m)
        xn = rr.normalize_coordinates(dense_xyz).view(-1, 3)
        scores = m.render_instance_mlp(None, m.compute_instance_feature(xn))
        top = torch.topk(scores, 2, dim=1).values
        gap = (top[:, 0] - top[:, 1]).view(RES)
    n_tie = int((gap < TIE_GAP).sum())
    margin = float(((alpha.clamp(0, 1) - rr.alpha_mask_threshold).abs() / rr.alpha_mask_threshold).min())
    print(f"{n_tie} of {gap.numel()} voxels with a top-two gap below {TIE_GAP}; smallest relative alpha margin {margin:.3e}")
    assert n_tie <= TIE_SHARE * gap.numel(), "too many near ties: change the seed"
    assert margin >= ALPHA_MARGIN, "a voxel's alpha sits on the threshold: change the seed"
    out.update(inst_gap=gap, n_near_tie=n_tie, alpha_margin=margin)
    mg.npz("g27_dense_volume", **out)


if __name__ == "__main__":
    main()
