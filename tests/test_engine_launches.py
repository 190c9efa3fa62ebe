"""What the engine launches, pinned without a GPU: render / feature passes and the point-wise utilities run on CPU stand-in tensors with
``engine.call`` replaced by a recorder (engine_recorder.py), and every launch -- entry point, scalars, NULL-ness, which buffer each pointer is
in and where, struct fields, clift_gemm routes -- is compared with tests/golden/engine_launches.json, recorded from the engine as it stood
before its head / compositing sequences were gathered into shared helpers.

``cases()`` enumerates 860 cases on a 16^3 field, 64 rays, 22 classes, 6 instance features, the active-row count dictated by the stand-in:
  * one baseline per (mode, field, M, pass): modes fp32 / bf16 / fp32x6; fields = xyz heads with and without slow-fast, the semantic head on
    its own grid, the instance head on its own grid with slow-fast, both on grids; M in {0, 63, 300, 4096} (the code's thresholds are
    M >= 64 and M >= 4096, M == 0 skips the heads); passes = render forward + backward with grad_heads all four / the trainer's main-pass
    set / () (forward only), the instance feature pass with slow_grad off / on, the semantic feature pass                          (360)
  * the sync-free (cap=) render passes, fp32 and fp32x6                                                                            (80)
  * semantic_weight_mode argmax / none, white background, argmax on white, on the slow-fast xyz field and the all-grid field; the
    semantic feature pass without softmax weights                                                                                  (120)
  * slow-fast xyz field, M = 4096, one at a time: each fusion flag cleared, KEEP_FIRST_ACT set, kernel_switches(tiled_only=True),
    kernel_switches(x6_tiled=True)                                                                                                 (234)
  * COMPOSITE_ACT_FUSED cleared on the grid fields and together with argmax weights (the remaining compositing call sites)          (63)
  * the point-wise utilities, once per mode                                                                                         (3)
The golden file holds, per case, the sequence of entry points (indices into ``names``) and the sha256 of the full record, plus the sha256 of
the enumeration.

``edit_cases()`` enumerates 108 scene-edit renders (``engine.edit_forward``) the same way, against tests/golden/engine_edit_launches.json,
recorded from the engine as it stood while ``edit_forward`` still carried its own copies of the march prologue, the appearance layers and the
compositing tail (recorder and test extended, engine.py untouched).  Slow-fast xyz field (heads on grids are refused), 64 rays:
  * per mode: M in {0, 300, 4096} x (softmax weights, softmax on white, argmax) x (one delete, one move with a rotation, a list of a copy
    and a delete), ``weight_thres`` 0                                                                                              (81)
  * per mode: one delete at weight_thres 1e-4                                                                                       (3)
  * per mode, M = 4096, the move and the list: kernel_switches(tiled_only=True), kernel_switches(x6_tiled=True), APP_X6 cleared,
    APP_BF16 cleared                                                                                                               (24)

``head_cases()`` enumerates 309 cases against tests/golden/engine_head_launches.json, recorded from the engine as it stood while
``xyz_mlp_fwd`` chose its kernels as it launched and ``xyz_mlp_bwd`` inferred that choice from the activation list:
  * direct head calls, ``engine.xyz_mlp_fwd`` then ``engine.xyz_mlp_bwd`` on zero-filled tensors (weight rows pitched to a multiple of 4): per
    mode, the shapes of ``HEADS`` x M in {63, 4096} x keep_first True / False.  The record is the launches, then the outcome ("ok" or the
    exception's type and message: with keep_first False the backward's refusal), then -- a backward that ran -- the sorted buffer numbers
    of what the caller's ``keep`` list holds (the tensor lifetimes the side-stream mode relies on)                                   (72)
  * the two standard shapes at M = 4096, one at a time: KEEP_FIRST_ACT set, the three head fusion flags cleared, the two kernel switches
    set -- and KEEP_FIRST_ACT and the two switches applied to the forward only ("fwd:") or to the backward only ("bwd:")           (144)
  * the instance shape with the row softmax (the softmax behind a fused output layer)                                                (6)
  * ``feat_mlp_fwd`` / ``feat_mlp_bwd`` on the two grid-head shapes of the ``both_grid`` field, same M and keep                      (24)
  * the passes added since the first golden file was recorded, slow-fast xyz field, M in {0, 300}: surface_forward, render_forward +
    surface_from_ctx, edit_surface_forward and edit_forward + edit_surface_from_ctx (a move; a copy and a delete), layers_forward (a
    centroid table and a score table, with and without use_delta; the two scans report M // 2 and M rows)                           (60)
  * per mode: density_grad_points with world True and False, edit_density_grad_points(want_state=True)                              (3)

``python tests/test_engine_launches.py --dump DIR`` writes the full records of all three enumerations, one JSON file per case, for diffing two
trees; ``--golden`` / ``--golden-edit`` / ``--golden-heads`` rewrites one golden file from the tree it runs in."""
import contextlib
import hashlib
import json
import os
import sys

import pytest
import torch

from conftest import REPO
from engine_recorder import Recorder

GOLDEN = os.path.join(REPO, "tests", "golden", "engine_launches.json")
GOLDEN_EDIT = os.path.join(REPO, "tests", "golden", "engine_edit_launches.json")
GOLDEN_HEADS = os.path.join(REPO, "tests", "golden", "engine_head_launches.json")
GRID, RAYS, CLASSES, DIM_INST = 16, 64, 22, 6
MODES = ("fp32", "bf16", "fp32x6")
ROWS = (0, 63, 300, 4096)
FIELDS = {   # TensorVMSplit arguments
    "xyz_sf": dict(use_semantic_mlp=True, use_instance_mlp=True, slow_fast_mode=True),
    "xyz": dict(use_semantic_mlp=True, use_instance_mlp=True, slow_fast_mode=False),
    "sem_grid": dict(use_semantic_mlp=False, num_semantics_comps=(32, 32, 32), use_instance_mlp=True, slow_fast_mode=True),
    "inst_grid_sf": dict(use_semantic_mlp=True, use_instance_mlp=False, num_instance_comps=(32, 32, 32), slow_fast_mode=True),
    "both_grid": dict(use_semantic_mlp=False, num_semantics_comps=(32, 32, 32), use_instance_mlp=False, num_instance_comps=(32, 32, 32),
                      slow_fast_mode=False),
}
PASSES = ("render_all", "render_main", "render_fwd", "feat_inst", "feat_inst_slow", "feat_sem")
CLEARED = ("APP_FRONT_FUSED", "COMPOSITE_ACT_FUSED", "APP_OUT_BWD_FUSED", "FUSE_HEAD_BF16", "FIRST2_BF16_BWD_FUSED", "OUT_BWD_BF16_FUSED",
           "APP_SCATTER_XA", "DENS_BWD_SIGMA", "APP_BF16", "APP_X6")
VARIATIONS = tuple("-" + f for f in CLEARED) + ("+KEEP_FIRST_ACT", "tiled_only", "x6_tiled")
KEYS = ("mode", "field", "M", "pass", "weights", "white", "cap", "vary")
EDIT_KEYS = ("mode", "edit", "M", "weights", "white", "thres", "vary")
EDITS = ("delete", "move", "copy+delete")
HEAD_KEYS = ("mode", "what", "M", "keep", "vary")
HEADS = {   # (out, in) per layer
    "instance": [(256, 3), (256, 256), (256, 256), (3, 256)],
    "semantic": [(256, 3), (256, 256), (256, 256), (256, 256), (22, 256)],
    "h128": [(128, 3), (128, 128), (5, 128)],
    "three": [(256, 3), (256, 256), (3, 256)],
    "two": [(256, 3), (3, 256)],
    "wideE": [(256, 3), (256, 256), (256, 256), (8, 256)],
}
GRID_HEADS = {"grid_sem": "render_semantic_mlp", "grid_inst": "render_instance_mlp"}      # (feat_mlp_*: shapes of the both_grid field)
HEAD_VARIATIONS = ("+KEEP_FIRST_ACT", "-FUSE_HEAD_BF16", "-FIRST2_BF16_BWD_FUSED", "-OUT_BWD_BF16_FUSED", "tiled_only", "x6_tiled")
MIXED = tuple(f"{side}:{v}" for v in ("+KEEP_FIRST_ACT", "tiled_only", "x6_tiled") for side in ("fwd", "bwd"))
NEW_PASSES = ("surface", "render_fwd+surface", "edit_surface:move", "edit_surface:copy+delete", "edit+surface:move", "edit+surface:copy+delete",
              "layers:centroids", "layers:centroids+delta", "layers:scores", "layers:scores+delta")


def cases():
    out = []

    def add(mode, field, M, pas, weights="softmax", white=0, cap=0, vary=""):
        out.append(dict(zip(KEYS, (mode, field, M, pas, weights, white, cap, vary))))

    for mode in MODES:
        for field in FIELDS:
            for M in ROWS:
                for pas in PASSES:
                    add(mode, field, M, pas)
                if mode != "bf16":
                    add(mode, field, M, "render_all", cap=1)
                    add(mode, field, M, "render_main", cap=1)
        for field in ("xyz_sf", "both_grid"):
            for M in ROWS:
                for weights, white in (("argmax", 0), ("none", 0), ("softmax", 1), ("argmax", 1)):
                    add(mode, field, M, "render_all", weights=weights, white=white)
                add(mode, field, M, "feat_sem", weights="none")
        for vary in VARIATIONS:
            for pas in PASSES:
                add(mode, "xyz_sf", 4096, pas, vary=vary)
        for field in ("sem_grid", "both_grid"):
            for pas in ("render_all", "feat_inst_slow", "feat_sem"):
                add(mode, field, 4096, pas, vary="-COMPOSITE_ACT_FUSED")
            add(mode, field, 300, "render_all", vary="-COMPOSITE_ACT_FUSED")
        # (not with slow_grad: at the recorded commit the slow net of a grid instance head could not be differentiated with this flag cleared --
        # the unfused branch never defined the fused slow row that the chain named, a NameError)
        for pas in ("render_main", "feat_inst", "feat_sem"):
            add(mode, "inst_grid_sf", 4096, pas, vary="-COMPOSITE_ACT_FUSED")
        for field in ("xyz_sf", "both_grid"):
            for M in (300, 4096):
                for white in (0, 1):
                    add(mode, field, M, "render_all", weights="argmax", white=white, vary="-COMPOSITE_ACT_FUSED")
        add(mode, "xyz_sf", 4096, "render_main", weights="argmax", vary="-COMPOSITE_ACT_FUSED")
        add(mode, "xyz_sf", 4096, "render_main", weights="argmax")
        add(mode, "-", 301, "points")
    return out


def edit_cases():
    out = []

    def add(mode, edit, M, weights="softmax", white=0, thres=0.0, vary=""):
        out.append(dict(zip(EDIT_KEYS, (mode, edit, M, weights, white, thres, vary))))

    for mode in MODES:
        for M in (0, 300, 4096):
            for weights, white in (("softmax", 0), ("softmax", 1), ("argmax", 0)):
                for edit in EDITS:
                    add(mode, edit, M, weights, white)
        add(mode, "delete", 300, thres=1e-4)
        for vary in ("tiled_only", "x6_tiled", "-APP_X6", "-APP_BF16"):     # (the appearance tail and the xyz heads branch on them)
            for edit in ("move", "copy+delete"):
                add(mode, edit, 4096, vary=vary)
    return out


def head_cases():
    out = []

    def add(mode, what, M, keep="", vary=""):
        out.append(dict(zip(HEAD_KEYS, (mode, what, M, keep, vary))))

    for mode in MODES:
        for what in tuple(HEADS) + tuple(GRID_HEADS):
            for M in (63, 4096):
                for keep in (True, False):
                    add(mode, what, M, keep)
        for what in ("instance", "semantic"):
            for vary in HEAD_VARIATIONS + MIXED:
                for keep in (True, False):
                    add(mode, what, 4096, keep, vary)
        for keep in (True, False):
            add(mode, "instance", 4096, keep, "softmax")
        for M in (0, 300):
            for pas in NEW_PASSES:
                add(mode, pas, M)
        add(mode, "grad_points", 301)
    return out


def case_name(c):       # (the keys of a case are in KEYS / EDIT_KEYS / HEAD_KEYS order)
    return "/".join(str(v) for v in c.values())


def cases_sha256(cs):
    return hashlib.sha256(json.dumps([list(c.values()) for c in cs]).encode()).hexdigest()


# ----------------------------------------------------------------------------- running one case
_models = {}


def field_on_cpu(kind, grid=GRID, classes=CLASSES, dim_inst=DIM_INST):
    import contrastive_lift_amd as cl
    key = (kind, grid, classes, dim_inst)
    if key not in _models:
        torch.manual_seed(0)
        _models[key] = cl.TensorVMSplit([grid] * 3, num_semantic_classes=classes, dim_feature_instance=dim_inst, splus_density_shift=-3.0, device="cpu",
                                        **FIELDS[kind])
    return _models[key]


def renderer_on_cpu(weights, grid=GRID):
    import contrastive_lift_amd as cl
    return cl.TensoRFRenderer(torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), [grid] * 3, semantic_weight_mode=weights, step_ratio=0.5)


@contextlib.contextmanager
def variation(vary):
    from contrastive_lift_amd import engine
    if vary in ("tiled_only", "x6_tiled"):
        with engine.kernel_switches(**{vary: True}):
            yield
    elif vary:
        name, prev = vary[1:], getattr(engine, vary[1:])
        setattr(engine, name, vary[0] == "+")
        try:
            yield
        finally:
            setattr(engine, name, prev)
    else:
        yield


def run_pass(engine, model, renderer, pas, rays, jitter, white, cap, n_classes, dim_inst):
    """One forward (+ backward) of the engine; returns the context."""
    N, gv = rays.shape[0], model.named_grad_views()
    g = lambda *shape: torch.ones(shape, dtype=torch.float32, device=rays.device)
    if pas == "render_all":
        _, ctx = engine.render_forward(model, renderer, rays, jitter, white, cap=cap)
        engine.render_backward(model, ctx, gv, g(N, 3), g(N, n_classes), g(N, dim_inst), g(1), density_grad=True, slow_grad=True)
    elif pas == "render_main":       # (the trainer's main pass)
        _, ctx = engine.render_forward(model, renderer, rays, jitter, white, grad_heads=("app", "sem"), want_dist=False, cap=cap)
        engine.render_backward(model, ctx, gv, g(N, 3), g(N, n_classes), None, None, density_grad=True)
    elif pas == "render_fwd":
        _, ctx = engine.render_forward(model, renderer, rays, jitter, white, grad_heads=(), cap=cap)
    elif pas in ("feat_inst", "feat_inst_slow"):
        _, ctx = engine.feature_forward(model, renderer, rays, jitter, "instance", cap=cap)
        engine.feature_backward(model, ctx, gv, g(N, dim_inst), slow_grad=pas == "feat_inst_slow")
    else:
        _, ctx = engine.feature_forward(model, renderer, rays, jitter, "semantic", cap=cap)
        engine.feature_backward(model, ctx, gv, g(N, n_classes))
    return ctx


def run_points(engine, n):
    xyz = torch.zeros((n, 3), dtype=torch.float32)
    m = field_on_cpu("xyz_sf")
    engine.density_points(m, xyz)
    engine.density_points(m, xyz, activation=False)
    feats = engine.appearance_feature_points(m, xyz)
    engine.appearance_mlp_points(m.render_appearance_mlp, xyz, feats)
    engine.xyz_mlp_points(m.render_semantic_mlp.mlp, xyz)
    engine.xyz_mlp_points(m.render_instance_mlp.slow_mlp, xyz)
    m = field_on_cpu("both_grid")
    engine.feat_mlp_points(m.render_semantic_mlp.mlp, engine.grid_feature_points(m, "semantic", xyz))
    engine.feat_mlp_points(m.render_instance_mlp.mlp, engine.grid_feature_points(m, "instance", xyz))


def edit_program(kind):
    """The edits of an edit case (an ``Edit`` or a list of them) on one fixed box; every number is a binary fraction and the rotation a
    quarter turn about z, so that the records hold the same bits wherever they are resolved."""
    from contrastive_lift_amd import edit
    box = edit.EditBox([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [0.125, -0.25, 0.0625], [-0.375, -0.25, -0.1875], [0.375, 0.25, 0.1875])
    t, R = [0.25, 0.0, -0.125], [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    return {"delete": lambda: edit.delete(box), "move": lambda: edit.move(box, t, R), "copy+delete": lambda: [edit.copy(box, t), edit.delete(box)],
            "copy+copy": lambda: [edit.copy(box, t), edit.copy(box, [-0.25, 0.0, 0.125], R)]}[kind]()


def slot_table(kind):
    """The ``layers.SlotTable`` of a layer case: three centroids over two thing classes, or slot scores over three columns (the fast
    instance net of the slow-fast field gives three)."""
    import numpy as np
    from contrastive_lift_amd.layers import SlotTable
    if kind == "scores":
        return SlotTable.from_scores((1, 3, 5), CLASSES, DIM_INST // 2)
    return SlotTable.from_centroids({1: np.zeros((2, DIM_INST // 2), np.float32), 3: np.full((1, DIM_INST // 2), 0.5, np.float32)}, (1, 3, 5), CLASSES)


def run_new_pass(engine, model, renderer, pas, rays, jitter):
    """One of NEW_PASSES; returns the context."""
    kind, _, arg = pas.partition(":")
    if kind == "surface":
        return engine.surface_forward(model, renderer, rays, jitter)[1]
    if kind == "render_fwd+surface":
        _, ctx = engine.render_forward(model, renderer, rays, jitter, False, grad_heads=())
        engine.surface_from_ctx(model, renderer, ctx)
    elif kind == "edit_surface":
        _, ctx = engine.edit_surface_forward(model, renderer, rays, edit_program(arg))
    elif kind == "edit+surface":
        _, ctx = engine.edit_forward(model, renderer, rays, edit_program(arg), False)
        engine.edit_surface_from_ctx(model, renderer, ctx)
    else:
        table, _, delta = arg.partition("+")
        _, ctx = engine.layers_forward(model, renderer, rays, slot_table(table), jitter, use_delta=bool(delta))
    return ctx


def run_grad_points(engine, model, renderer, n):
    xyz = torch.zeros((n, 3), dtype=torch.float32)
    engine.density_grad_points(model, xyz, world=True, renderer=renderer)
    engine.density_grad_points(model, xyz, world=False)
    engine.edit_density_grad_points(model, renderer, xyz, edit_program("copy+delete"), want_state=True)


def head_tensors(c):
    """(layers, gradient layers) of a direct head case: zero-filled, the weights' row pitch a multiple of 4."""
    if c["what"] in HEADS:
        shapes = HEADS[c["what"]]
    else:
        seq = getattr(field_on_cpu("both_grid"), GRID_HEADS[c["what"]]).mlp
        shapes = [tuple(m.weight.shape) for m in seq if isinstance(m, torch.nn.Linear)]
    lin = lambda o, i: (torch.zeros((o, (i + 3) // 4 * 4))[:, :i], torch.zeros(o))
    return [lin(o, i) for o, i in shapes], [lin(o, i) for o, i in shapes]


def record_head(engine, c, pointers):
    """A direct head case: forward, then backward, each under its side of the case's variation; the launches, the outcome and -- a backward
    that ran -- what ``keep`` holds."""
    side, _, vary = c["vary"].rpartition(":")
    softmax, vary = vary == "softmax", "" if vary == "softmax" else vary
    layers, glayers = head_tensors(c)
    M, n_out = c["M"], layers[-1][0].shape[0]
    xa = torch.zeros((M, layers[0][0].stride(0)))           # (the positions of an xyz head, the feature rows of a grid head)
    out, dpre = torch.zeros((M, n_out)), torch.zeros((M, (n_out + 3) // 4 * 4))
    out_act = 2 if (softmax or c["what"] in ("semantic", "grid_sem")) else 0
    roots = [xa, out, dpre] + [t for pairs in (layers, glayers) for pair in pairs for t in pair]
    keep, ran = [], False
    with Recorder(roots=lambda: roots, pointers=pointers) as rec:
        try:
            if c["what"] in HEADS:
                with variation(vary if side != "bwd" else ""):
                    acts = engine.xyz_mlp_fwd(layers, xa, M, out, n_out, keep_first=c["keep"], out_act=out_act)
                with variation(vary if side != "fwd" else ""):
                    engine.xyz_mlp_bwd(layers, glayers, xa, acts, dpre, M, keep)
            else:
                with engine._grid_precision():
                    acts = engine.feat_mlp_fwd(layers, xa, M, out, n_out, keep=c["keep"], out_act=out_act)
                    engine.feat_mlp_bwd(layers, glayers, xa, acts, dpre, M, keep)
            ran, outcome = True, "ok"
        except AssertionError:
            raise
        except Exception as e:
            outcome = f"{type(e).__name__}: {e}"
        rec.launches.append(["outcome", [outcome]])
        if ran:
            rec.launches.append(["keep", [sorted(rec.buffer_number(t) for t in keep)]])
    return rec.launches


def record(c, pointers=True):
    """The launches of one case: [[entry point, arguments(, route)], ...]."""
    from contrastive_lift_amd import engine
    prev = engine.set_mlp_precision(c["mode"])
    try:
        if "what" in c and (c["what"] in HEADS or c["what"] in GRID_HEADS):
            return record_head(engine, c, pointers)
        if "what" in c:
            model, renderer = field_on_cpu("xyz_sf"), renderer_on_cpu("softmax")
            rays, jitter = torch.zeros((RAYS, 8), dtype=torch.float32), torch.zeros((RAYS,), dtype=torch.float32)
            with Recorder(active=(c["M"] // 2, c["M"]) if c["what"].startswith("layers") else c["M"], roots=lambda: [model.param_flat, rays, jitter],
                          pointers=pointers) as rec:
                if c["what"] == "grad_points":
                    run_grad_points(engine, model, renderer, c["M"])
                else:
                    run_new_pass(engine, model, renderer, c["what"], rays, jitter)
            return rec.launches
        with variation(c["vary"]):
            if "edit" in c:
                model, renderer, rays = field_on_cpu("xyz_sf"), renderer_on_cpu(c["weights"]), torch.zeros((RAYS, 8), dtype=torch.float32)
                with Recorder(active=c["M"], roots=lambda: [model.param_flat, rays], pointers=pointers) as rec:
                    engine.edit_forward(model, renderer, rays, edit_program(c["edit"]), bool(c["white"]), weight_thres=c["thres"])
                return rec.launches
            if c["pass"] == "points":
                models = [field_on_cpu("xyz_sf"), field_on_cpu("both_grid")]
                with Recorder(roots=lambda: [m.param_flat for m in models], pointers=pointers) as rec:
                    run_points(engine, c["M"])
                return rec.launches
            model, renderer = field_on_cpu(c["field"]), renderer_on_cpu(c["weights"])
            rays, jitter = torch.zeros((RAYS, 8), dtype=torch.float32), torch.zeros((RAYS,), dtype=torch.float32)
            roots = lambda: [model.param_flat, model.grad_flat, rays, jitter] + list(model.__dict__.get("_xcd_ws", {}).values())
            with Recorder(active=c["M"], roots=roots, pointers=pointers) as rec:
                run_pass(engine, model, renderer, c["pass"], rays, jitter, bool(c["white"]), c["M"] if c["cap"] else None, CLASSES, DIM_INST)
            return rec.launches
    finally:
        engine.set_mlp_precision(prev)


def digest(launches):
    return hashlib.sha256(json.dumps(launches).encode()).hexdigest()


def golden_document(cs):
    names, rows = [], {}
    for c in cs:
        launches = record(c)
        for n, *_ in launches:
            if n not in names:
                names.append(n)
        rows[case_name(c)] = [[names.index(n) for n, *_ in launches], digest(launches)]
    return dict(cases_sha256=cases_sha256(cs), names=names, cases=rows)


# ----------------------------------------------------------------------------- tests
def compare_with_golden(golden, cs):
    doc = json.load(open(golden))
    assert len(cs) == len(doc["cases"]) and cases_sha256(cs) == doc["cases_sha256"], "cases() no longer enumerates what the golden file was recorded for"
    bad = []
    for c in cs:
        first, second = record(c), record(c)
        assert json.dumps(first) == json.dumps(second), f"{case_name(c)}: two recordings of the same tree differ"
        seq, sha = doc["cases"][case_name(c)]
        got = [n for n, *_ in first]
        want = [doc["names"][i] for i in seq]
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append(f"{case_name(c)}: launch {k} is {got[k] if k < len(got) else 'missing'}, recorded {want[k] if k < len(want) else 'nothing'}")
        elif digest(first) != sha:
            bad.append(f"{case_name(c)}: same entry points, other arguments (compare --dump of the two trees)")
    assert not bad, f"{len(bad)} of {len(cs)} cases differ:\n" + "\n".join(bad[:20])


def test_engine_launches_match_the_recorded_ones():
    compare_with_golden(GOLDEN, cases())


def test_edit_launches_match_the_recorded_ones():
    compare_with_golden(GOLDEN_EDIT, edit_cases())


def test_head_launches_match_the_recorded_ones():
    compare_with_golden(GOLDEN_HEADS, head_cases())


BRACKETED = {   # the module attributes of engine that bench.py's roofline replays replace, and the entry point each of them launches
    "gemm": "clift_gemm", "first2": "clift_xyz_head_first2_fwd", "last2": "clift_xyz_head_last2_fwd", "app_last2": "clift_app_head_last2_fwd",
    "first2_bwd": "clift_xyz_head_first2_bwd", "first2_wgrad": "clift_xyz_head_first2_wgrad", "first2_x6": "clift_xyz_head_first2_x6_fwd",
    "last2_x6": "clift_xyz_head_last2_x6_fwd", "first2_x6_bwd": "clift_xyz_head_first2_x6_bwd", "first2_x6_wgrad": "clift_xyz_head_first2_x6_wgrad",
    "out_layer_fwd": "clift_out_layer_fwd", "head_bf16": "clift_xyz_head_bf16_fwd"}


@pytest.mark.parametrize("mode", MODES)
def test_bench_brackets_see_every_launch(mode):
    """bench.py's roofline replays replace the module attributes of BRACKETED by wrappers and call the originals positionally.  With
    counting wrappers of bench.py's positional shapes in their place, one recorded render forward + backward at M = 4096 enters each wrapper
    exactly as often as its entry point occurs in the record (``gemm``: every clift_gemm launch): the engine reaches each of them through the
    module global at call time, with arguments the wrappers' signatures take."""
    from contrastive_lift_amd import engine
    real, entered = {n: getattr(engine, n) for n in BRACKETED}, dict.fromkeys(BRACKETED, 0)

    def count(name):
        entered[name] += 1
        return real[name]

    wrappers = {
        "gemm": lambda M, N, K, A, lda, B, ldb, Cm, ldc, **kw: count("gemm")(M, N, K, A, lda, B, ldb, Cm, ldc, **kw),
        "first2": lambda M, *args: count("first2")(M, *args),
        "last2": lambda M, h, W, b, Wo, bo, hidden, *args: count("last2")(M, h, W, b, Wo, bo, hidden, *args),
        "app_last2": lambda M, H1, W2, b2, W3, *args: count("app_last2")(M, H1, W2, b2, W3, *args),
        "first2_bwd": lambda M, *args: count("first2_bwd")(M, *args),
        "first2_wgrad": lambda M, *args: count("first2_wgrad")(M, *args),
        "first2_x6": lambda M, *args: count("first2_x6")(M, *args),
        "last2_x6": lambda M, h, W, b, Wo, bo, hidden, *args: count("last2_x6")(M, h, W, b, Wo, bo, hidden, *args),
        "first2_x6_bwd": lambda M, *args: count("first2_x6_bwd")(M, *args),
        "first2_x6_wgrad": lambda M, *args: count("first2_x6_wgrad")(M, *args),
        "out_layer_fwd": lambda M, h, W, *args: count("out_layer_fwd")(M, h, W, *args),
        "head_bf16": lambda M, xa, l0, l1, l2, lout, h1, h2, h3, out, ldo, col_off: count("head_bf16")(M, xa, l0, l1, l2, lout, h1, h2, h3, out, ldo, col_off),
    }
    for name, w in wrappers.items():
        setattr(engine, name, w)
    try:
        launches = record(dict(zip(KEYS, (mode, "xyz_sf", 4096, "render_all", "softmax", 0, 0, ""))))
    finally:
        for name, fn in real.items():
            setattr(engine, name, fn)
    launched = {name: sum(l[0] == entry for l in launches) for name, entry in BRACKETED.items()}
    assert launched["gemm"] > 0 and entered == launched


def run_edit(engine, model, renderer, pas, rays, jitter, white, cap, n_classes, dim_inst):
    """run_pass for the scene-edit render ``pas`` = "edit:<kind of edit_program>" (no jitter, no backward)."""
    return engine.edit_forward(model, renderer, rays, edit_program(pas[5:]), white)[1]


def run_layers(engine, model, renderer, pas, rays, jitter, white, cap, n_classes, dim_inst):
    """run_pass for the amodal layer pass (no backward)."""
    return engine.layers_forward(model, renderer, rays, slot_table("centroids"), jitter)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("mode, pas", [("fp32x6", "render_all"), ("bf16", "render_all"), ("fp32x6", "edit:copy+copy"), ("fp32x6", "layers")],
                         ids=["fp32x6", "bf16", "fp32x6-edit", "fp32x6-layers"])
def test_stand_in_launches_what_the_gpu_run_launches(mode, pas):
    """The recorder's stand-in cannot drift from reality: a render forward + backward of 512 rays on the 32^3 synthetic scene, really launched,
    and the same pass on the CPU stand-in with the row count the device found, give the same entry points with the same scalars.  Likewise an
    edit render of the same rays under a program of two copies (which kill nothing: M > 0), and the layer pass, whose two scans the stand-in
    answers with the lengths of the march's list and of its alpha-list."""
    run = run_edit if pas.startswith("edit:") else run_layers if pas == "layers" else run_pass
    from contrastive_lift_amd import engine
    from contrastive_lift_amd.synthetic import make_scene
    n, grid = 512, 32
    model, renderer, pool = make_scene(grid=grid, num_classes=CLASSES, max_instances=DIM_INST // 2, device="cuda", image=64, n_cams=1)
    rays = pool[torch.randperm(pool.shape[0], generator=torch.Generator().manual_seed(3))[:n].to(pool.device)].contiguous()
    jitter = torch.rand((n,), generator=torch.Generator().manual_seed(4)).to(pool.device)
    prev = engine.set_mlp_precision(mode)
    try:
        with Recorder(launch=engine.call, pointers=False) as real:
            ctx = run(engine, model, renderer, pas, rays, jitter, False, None, CLASSES, DIM_INST)
        torch.cuda.synchronize()
        assert ctx.M > 0
        cpu_model = field_on_cpu("xyz_sf", grid=grid)
        with Recorder(active=(ctx.M_render, ctx.M) if pas == "layers" else ctx.M, pointers=False) as stand_in:
            run(engine, cpu_model, renderer_on_cpu("softmax", grid), pas, torch.zeros((n, 8)), torch.zeros((n,)), False, None, CLASSES, DIM_INST)
    finally:
        engine.set_mlp_precision(prev)
    assert [l[0] for l in stand_in.launches] == [l[0] for l in real.launches]
    assert stand_in.launches == real.launches


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        os.makedirs(sys.argv[2], exist_ok=True)
        for c in cases() + edit_cases() + head_cases():
            with open(os.path.join(sys.argv[2], case_name(c).replace("/", "__") + ".json"), "w") as f:
                f.write("\n".join(json.dumps(l) for l in record(c)) + "\n")
    elif sys.argv[1:2] == ["--golden"]:
        with open(GOLDEN, "w") as f:
            json.dump(golden_document(cases()), f, separators=(",", ":"))
            f.write("\n")
    elif sys.argv[1:2] == ["--golden-edit"]:
        with open(GOLDEN_EDIT, "w") as f:
            json.dump(golden_document(edit_cases()), f, separators=(",", ":"))
            f.write("\n")
    elif sys.argv[1:2] == ["--golden-heads"]:
        with open(GOLDEN_HEADS, "w") as f:
            json.dump(golden_document(head_cases()), f, separators=(",", ":"))
            f.write("\n")
    else:
        sys.exit("usage: test_engine_launches.py --dump DIR | --golden | --golden-edit | --golden-heads")
