#!/usr/bin/env python3
"""Render a trained scene with one boxed instance deleted, extracted, copied or moved -- or with an ordered list of such edits.

    python inference/edit_scene.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt --bboxes bboxes.pkl --instance ID
                                   --op delete|extract|copy|move [--translate x y z] [--rotate_deg rx ry rz] [--pad 0.0]
                                   [--render_trajectory] [--image_dim H W] [--weight_thres 0] [--save_surface [--surface_quantile 0.5]]
                                   [--save_layers --cached_centroids_path C [--layers_level 0.5] [--layers_colour [--layers_colour_rest]]]
                                   [--follow_shape --cached_centroids_path C [--shape_grid 32] [--shape_grow 1] [--shape_alpha 0.5]]
                                   [--settle [AXIS] [--settle_upsample 1] [--settle_slack 0]]
                                   [--check_placement [--placement_upsample 1]]
                                   [--snap_placement [AXIS] [--snap_upsample 1] [--snap_min_support 1]]
    python inference/edit_scene.py --ckpt_path ... --bboxes bboxes.pkl --script edits.json [--render_trajectory] ...

``bboxes.pkl`` comes from ``inference/fit_bboxes.py`` (one oriented box per instance id).  ``copy`` and ``move`` are rigid: the box content
undergoes x -> R (x - pos) + pos + t with R = Rz Ry Rx of ``--rotate_deg`` and t = ``--translate`` (contrastive_lift_amd/edit.py; the
reference's forward_duplicate / forward_manipulate arithmetic, which is not rigid for R != I, stays available as
``TensoRFRenderer.forward_duplicate`` / ``forward_manipulate``).  Fitted boxes hug the filtered points: ``--pad`` grows the box on every
side.  Checkpoint loading and the frame loop are those of ``inference/render_panopli.py``; under torch.distributed.run every frame is
rendered as row-tiles over the ranks.  Writes ``rgb/*.png``, ``pred_semantics/*.png`` (uint8) and ``depth/*.npy`` under
``runs/<scene>_<test|trajectory>_<experiment>_edit_<op>_<id>/``.  ``--save_surface`` adds the surface outputs of the EDITED scene
(DESIGN.md 6h), in the files of ``inference/render_panopli.py --save_surface``: ``surface/<frame>.npz`` (depth_median, hit, normals) and
``vis_normals/<frame>.png``; ``--surface_quantile Q`` moves the hit from the median (0.5) to another quantile of the ray's weight.
``--save_layers`` adds the amodal instance layers of the EDITED scene, in the files of ``inference/render_panopli.py
--save_layers``: ``layers/<frame>.npz``, ``layers/<frame>.json`` and ``vis_amodal/<frame>.png``, in the scene's fixed slot numbering with
one more slot per copy of the program (slot_class -1, slot_index = the copy's 0-based position in the program), and
``layers/<frame>_change.json``: per slot what the edit hid, revealed or removed (``layers.compare`` of the unedited and the edited frame,
one more plain layer pass per frame).  The slots come from ``--cached_centroids_path`` (a linear-assignment model needs none).
``--layers_colour [--layers_colour_rest]`` adds the colour layers of the edited scene as ``render_panopli.py`` does for a
plain one: ``colour`` in the npz and ``vis_amodal_rgb/<frame>/slot_<k>.png``, the copy's slot included.

``--script FILE.json`` applies up to 8 edits in ONE render (``edit.EditProgram``), in file order.  The file holds a list of
``{"instance": id, "op": "delete|extract|copy|move", "translate": [x, y, z], "rotate_deg": [rx, ry, rz], "pad": p, "at": "moved"}``;
only ``instance`` and ``op`` are required.  Each entry's box is ``boxes[instance]`` AS FITTED IN THE UNEDITED SCENE, whatever earlier
entries did: an entry that acts on an object after an earlier entry has moved it still names the same instance, and says
``"at": "moved"`` -- its box is then the destination box of the most recent earlier ``move`` of that instance, so its motion composes
with that move ("move it, then turn it where it now stands").  Without the flag a later entry addresses the place where the object
stood at first.  Output goes to ``..._edit_script_<file stem>/``.

``--follow_shape`` makes every edit follow the instance's SHAPE, not its box: the cells of a ``--shape_grid``^3 lattice over
the box whose centre holds density (``--shape_alpha``, as ``--alpha_level`` of inference/extract_mesh.py) of the box's most frequent
instance slot, grown by ``--shape_grow`` cells (``edit.EditShape.from_field``; the slot table is ``render_panopli.layers_table``'s, so
``--cached_centroids_path`` is required unless the model is a linear-assignment one).  Deleting a cup then leaves the table under it,
and a moved chair takes no floor along and covers nothing but itself at the destination.  One line per edit reports the chosen slot and
the cells set, occupied and in all.  A script entry may say ``"shape": true|false`` (default: the flag); an ``"at": "moved"`` entry
reuses the shape of the move it refers to and must not pad the box again.  Output names get ``_shape`` behind them.
``--follow_shape`` cannot be combined with ``--save_surface`` or ``--save_layers``: those passes walk the boxes alone.

``--settle [AXIS]`` (with ``--op move|copy``, or a ``--script`` whose last entry is a move or a copy) drops the object that the last edit
places along AXIS (one of +x -x +y -y +z -z, default -z) until it touches the rest of the edited scene (DESIGN.md 6n;
``clearance.settle_offset``): the density lattice of the edited scene at ``--settle_upsample`` times the grid is keyed -- the moved content,
everything else, empty --, one kernel finds the free travel of the moved content along AXIS in lattice steps
(clift_lattice_clearance), and the last edit is rebuilt with that translation added (a shape is reused as it is).  One line reports
``settled by N steps = D along AXIS onto F faces`` (``--settle_slack S`` counts the faces up to S steps further away); the output folder
gets ``_settled`` behind its name.  When nothing stands in the way the tool says so and renders the edit as given.  A BOX move carries a
slab of its surroundings along -- the floor under a chair --, which is in contact already, so its travel is usually 0: ``--follow_shape``
is the intended companion.

``--check_placement`` (with ``--op move|copy``, or a ``--script`` whose last entry is one) says whether the object that the last edit places
collides with what stood at its destination (``distance.placement``, clift_lattice_distance): on the lattice at
``--placement_upsample`` times the grid, the moved content against the density of the scene before the paste.  One line reports
``placement: collides on N cells, depth D`` (D: how many lattice steps the deepest overlapping point lies inside what was there) or
``placement: touches|clear, gap G cells = W`` (the true distance to the rest of the scene, in lattice steps and in world units), and
``placement.json`` in the output folder holds the numbers and the two world points.  With ``--settle`` the settled edit is checked.  The
render itself does not change.

``--snap_placement [AXIS]`` (with ``--op move|copy``, or a ``--script`` whose last entry is one; not together with ``--settle``) moves the
object that the last edit places to the NEAREST translation at which it collides with nothing and stands (DESIGN.md 6p;
``placement.snap_offset``, clift_lattice_placement): on the lattice at ``--snap_upsample`` times the grid one kernel counts, for every
translation of the moved content, the cells that collide with what stood there before the paste and the faces that look along AXIS (default
-z) onto it; the nearest translation without a collision and with at least ``--snap_min_support`` such faces is added to the last edit as
``--settle`` adds its drop.  One line reports ``snapped by (dx, dy, dz) steps = W onto F faces (was: collides on N cells)`` (W: the length
of the world translation) or ``not snapped: no free supported position`` (the edit is then rendered as given); the output folder gets
``_snapped`` behind its name and ``snap.json`` holds the numbers.  With ``--check_placement`` the snapped edit is checked.
"""
import argparse
import functools
import json
import math
import os
import pickle
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import render_panopli as rp                                           # noqa: E402
from contrastive_lift_amd import edit as ed                           # noqa: E402
from contrastive_lift_amd import inference as inf                     # noqa: E402
from contrastive_lift_amd.config import load_run_config               # noqa: E402
from contrastive_lift_amd.lattice import DIRECTIONS as UP_AXES        # noqa: E402

OPS = ("delete", "extract", "copy", "move")


def resolve_edit(boxes, instance, op, translate=(0.0, 0.0, 0.0), rotate_deg=(0.0, 0.0, 0.0), pad=0.0, box=None, shape=None):
    """One edit of the fitted box of ``instance`` -- or of ``box`` (an ``EditBox``) in its place, where the object no longer stands there.
    ``shape``: the ``edit.EditShape`` the edit follows (over that box), or a callable ``shape(box)`` that makes it (``field_shapes``)."""
    if instance not in boxes:
        raise SystemExit(f"instance {instance} has no box (boxes: {sorted(boxes)})")
    box = ed.EditBox.from_fitted(boxes[instance], pad=pad) if box is None else box.padded(pad)
    if callable(shape):
        shape = shape(box)
    if op == "delete":
        return ed.delete(box, shape=shape)
    if op == "extract":
        return ed.extract(box, shape=shape)
    R = ed.rotation_from_euler_deg(*rotate_deg)
    return (ed.copy if op == "copy" else ed.move)(box, np.asarray(translate, dtype=np.float64), R, shape=shape)


def field_shapes(model, renderer, table, grid=32, grow=1, alpha=0.5, use_delta=False):
    """What ``--follow_shape`` hands to ``resolve_edit`` / ``resolve_program``: ``shape_of(box)`` reads the shape of the instance in ``box``
    from the trained field (``EditShape.from_field``: the most frequent slot of ``table`` among the occupied cells) and prints one line per
    edit.  ``alpha`` turns into the density threshold by ``extract_mesh.default_level``, so it means what ``--alpha_level`` means."""
    import extract_mesh as xm
    sigma_min, dims = xm.default_level(renderer, float(alpha)), (int(grid),) * 3

    def shape_of(box):
        try:
            sh = ed.EditShape.from_field(model, renderer, box, table, dims=dims, grow=int(grow), sigma_min=sigma_min, use_delta=use_delta)
        except ValueError as err:
            raise SystemExit(f"--follow_shape: {err}")
        print(f"shape: slot {sh.slot}, {sh.n_set} cells set, {sh.n_occupied} occupied, {sh.n_cells} in all (sigma >= {sigma_min:.6g}, grow {int(grow)})")
        return sh
    return shape_of


def add_shape_arguments(ap):
    """The flags of ``--follow_shape``, shared with inference/extract_mesh.py."""
    ap.add_argument("--follow_shape", action="store_true",
                    help="the edit follows the instance's shape, not its box: only the cells of the box that hold density of the box's main "
                         "instance leave, arrive or stay (DESIGN.md 6k); needs the slot table of --cached_centroids_path (a linear_assignment "
                         "model needs none)")
    ap.add_argument("--shape_grid", type=int, default=32, metavar="G", help="--follow_shape: cells per axis of the shape lattice over the box")
    ap.add_argument("--shape_grow", type=int, default=1, metavar="R", help="--follow_shape: grow the shape by this many cells (0 .. 4)")
    ap.add_argument("--shape_alpha", type=float, default=0.5, metavar="A",
                    help="--follow_shape: a cell is occupied where one training-step sample would have this opacity (what --alpha_level of "
                         "inference/extract_mesh.py means)")


def script_asks_for_shapes(path):
    """Whether an entry of the ``--script`` file says ``"shape": true`` (None: no script)."""
    if path is None:
        return False
    with open(path) as f:
        entries = json.load(f)
    return isinstance(entries, list) and any(isinstance(e, dict) and e.get("shape") is True for e in entries)


def shape_table(config, scene, cached_centroids_path):
    """The slot table ``--follow_shape`` reads (``render_panopli.layers_table``); without centroids and without a linear-assignment model a
    ``SystemExit``."""
    try:
        return rp.layers_table(config, scene, cached_centroids_path)
    except ValueError:
        raise SystemExit("--follow_shape needs --cached_centroids_path (or a linear_assignment model): the shape follows one slot of the scene's table")


_ENTRY_KEYS = {"instance", "op", "translate", "rotate_deg", "pad", "at", "shape"}


def resolve_program(boxes, entries, follow_shape=False, shape_of=None):
    """The ``EditProgram`` of a ``--script`` list, in list order.  Every entry acts on ``boxes[instance]`` as fitted in the unedited scene;
    with ``"at": "moved"`` on the destination box of the most recent earlier ``move`` of the same instance.  An entry follows a shape where
    its ``"shape"`` says so (default: ``follow_shape``): ``shape_of(box)`` makes it (``field_shapes``); an ``"at": "moved"`` entry reuses
    the shape object of the move it refers to -- a rigid move keeps the local frame --, so it must not pad the box again."""
    if not isinstance(entries, list) or not 1 <= len(entries) <= ed.MAX_EDITS:
        raise SystemExit(f"an edit script is a list of 1 to {ed.MAX_EDITS} entries")
    edits, moved_to, moved_shape = [], {}, {}
    for i, entry in enumerate(entries):
        if not isinstance(entry, dict) or not {"instance", "op"} <= set(entry) <= _ENTRY_KEYS:
            raise SystemExit(f"entry {i}: needs \"instance\" and \"op\", and may hold {sorted(_ENTRY_KEYS)} only (got {entry!r})")
        instance, op = entry["instance"], entry["op"]
        if op not in OPS:
            raise SystemExit(f"entry {i}: unknown op {op!r} (one of {', '.join(OPS)})")
        at = entry.get("at", "fitted")
        if at not in ("fitted", "moved"):
            raise SystemExit(f"entry {i}: \"at\" is \"fitted\" or \"moved\" (got {at!r})")
        if at == "moved" and instance not in moved_to:
            raise SystemExit(f"entry {i}: \"at\": \"moved\" needs an earlier move of instance {instance}")
        shaped, pad, shape = entry.get("shape", bool(follow_shape)), float(entry.get("pad", 0.0)), None
        if not isinstance(shaped, bool):
            raise SystemExit(f"entry {i}: \"shape\" is true or false (got {shaped!r})")
        if shaped and at == "moved":
            if moved_shape.get(instance) is None:
                raise SystemExit(f"entry {i}: \"shape\" with \"at\": \"moved\" reuses the shape of the move it refers to, and that move of instance "
                                 f"{instance} follows none")
            if pad != 0.0:
                raise SystemExit(f"entry {i}: \"pad\": {pad} on a shaped \"at\": \"moved\" entry: the shape it reuses was made over the moved box as "
                                 "it is; pad the move instead")
            shape = moved_shape[instance]
        elif shaped:
            if shape_of is None:
                raise SystemExit(f"entry {i}: a shaped entry needs the trained field to read the shape from (--follow_shape / \"shape\": true)")
            shape = shape_of
        e = resolve_edit(boxes, instance, op, entry.get("translate", (0.0, 0.0, 0.0)), entry.get("rotate_deg", (0.0, 0.0, 0.0)),
                         pad, box=moved_to[instance] if at == "moved" else None, shape=shape)
        if op == "move":
            moved_to[instance], moved_shape[instance] = e.dst, e.shape
        edits.append(e)
    return ed.EditProgram(edits)


SHAPE_WITH_SURFACE_OR_LAYERS = ("--follow_shape (or a script entry with \"shape\": true) cannot be combined with --save_surface or --save_layers: "
                                "those passes walk the boxes alone and would drop the shapes (shaped surfaces and layers are not built yet)")


SETTLE_WANTS_A_MOTION = "--settle drops the object that a move or a copy places: give it with --op move|copy, or with a --script whose last entry is one"


def check_settle(edit):
    """``SystemExit`` unless the last edit of ``edit`` is a copy or a move."""
    if ed.as_program(edit)[-1].mode not in (ed.DUPLICATE, ed.MANIPULATE):
        raise SystemExit(SETTLE_WANTS_A_MOTION)


def settled_edit(edit, offset):
    """``edit`` (an ``Edit`` or an ``EditProgram``) with the world translation ``offset`` added to its LAST edit, a copy or a move: that
    edit goes through the same constructor again with translate + offset.  Its rotation is read back from the map (M = R^-1), its
    translation from the two box centres; a shape is reused as it is -- a rigid move keeps lo, hi and the frame."""
    program = ed.as_program(edit)
    last = program[-1]
    make = ed.copy if last.mode == ed.DUPLICATE else ed.move
    moved = make(last.src, (last.dst.centre - last.src.centre) + np.asarray(offset, np.float64), np.linalg.inv(last.M), shape=last.shape)
    return moved if isinstance(edit, ed.Edit) else ed.EditProgram(list(program.edits[:-1]) + [moved])


def settle(model, renderer, edit, direction="-z", upsample=1, slack=0):
    """``--settle``: (the edit to render, the dict of ``clearance.settle_offset``); prints the one line."""
    from contrastive_lift_amd import clearance as clr
    check_settle(edit)
    found = clr.settle_offset(model, renderer, edit, direction=direction, upsample=int(upsample), slack=int(slack))
    if not found["found"]:
        print(f"not settled: nothing stands in the way along {direction} ({found['n_moved']} lattice points moved); the edit is rendered as given")
        return edit, found
    print(f"settled by {found['steps']} steps = {found['steps'] * found['spacing']:.4f} along {direction} onto {found['faces']} faces")
    return settled_edit(edit, found["offset"]), found


SNAP_WANTS_A_MOTION = ("--snap_placement moves the object that a move or a copy places: give it with --op move|copy, or with a --script whose last "
                       "entry is one")
SNAP_WITH_SETTLE = "--snap_placement cannot be combined with --settle: the snap chooses the whole translation, the drop along an axis included"


def check_snap(edit):
    """``SystemExit`` unless the last edit of ``edit`` is a copy or a move."""
    if ed.as_program(edit)[-1].mode not in (ed.DUPLICATE, ed.MANIPULATE):
        raise SystemExit(SNAP_WANTS_A_MOTION)


def snap_line(found):
    """The one line of ``--snap_placement`` for the dict of ``placement.snap_offset``."""
    if not found["found"]:
        return "not snapped: no free supported position"
    was = f"collides on {found['overlap_before']} cells" if found["overlap_before"] > 0 else f"free on {found['support_before']} faces"
    dx, dy, dz = (int(x) for x in found["steps"])
    return f"snapped by ({dx}, {dy}, {dz}) steps = {math.sqrt(sum(float(x) ** 2 for x in found['offset'])):.4f} onto {found['support']} faces (was: {was})"


def snap(model, renderer, edit, out, direction="-z", upsample=1, min_support=1, write=True):
    """``--snap_placement``: (the edit to render, the dict of ``placement.snap_offset``); prints the one line and writes ``out``/snap.json."""
    from contrastive_lift_amd import placement as pm
    check_snap(edit)
    found = pm.snap_offset(model, renderer, edit, direction=direction, upsample=int(upsample), min_support=int(min_support))
    print(snap_line(found))
    if write:
        Path(out).mkdir(exist_ok=True, parents=True)
        with open(Path(out) / "snap.json", "w") as f:
            json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in found.items()}, f, indent=1)
    return (settled_edit(edit, found["offset"]) if found["found"] else edit), found


PLACEMENT_WANTS_A_MOTION = ("--check_placement checks the object that a move or a copy places: give it with --op move|copy, or with a --script "
                            "whose last entry is one")


def check_placement_edit(edit):
    """``SystemExit`` unless the last edit of ``edit`` is a copy or a move."""
    if ed.as_program(edit)[-1].mode not in (ed.DUPLICATE, ed.MANIPULATE):
        raise SystemExit(PLACEMENT_WANTS_A_MOTION)


def placement_line(found):
    """The one line of ``--check_placement`` for the dict of ``distance.placement``."""
    if found["verdict"] == "collides":
        return f"placement: collides on {found['overlap']} cells, depth {math.sqrt(found['depth2']):.2f}"
    if found["gap2"] is None:
        return f"placement: {found['verdict']}, nothing else in the scene"
    world = math.sqrt(sum((a - b) ** 2 for a, b in zip(found["moved_point"], found["rest_point"])))
    return f"placement: {found['verdict']}, gap {math.sqrt(found['gap2']):.2f} cells = {world:.4f}"


def check_placement(model, renderer, edit, out, upsample=1, write=True):
    """``--check_placement``: the dict of ``distance.placement`` for ``edit``; prints the one line and writes ``out``/placement.json."""
    from contrastive_lift_amd import distance as dt
    check_placement_edit(edit)
    found = dt.placement(model, renderer, edit, upsample=int(upsample))
    print(placement_line(found))
    if write:
        Path(out).mkdir(exist_ok=True, parents=True)
        with open(Path(out) / "placement.json", "w") as f:
            json.dump(found, f, indent=1)
    return found


def edit_scene_checkpoint(config, edit, tag, trajectory_name="trajectory_blender", test_only=True, device="cuda:0", weight_thres=0.0,
                          save_surface=False, surface_quantile=0.5, save_layers=False, cached_centroids_path=None, layers_level=0.5,
                          layers_colour=False, layers_colour_rest=False, settle_options=None, placement_options=None, snap_options=None):
    """``settle_options``: dict(direction, upsample, slack) of ``--settle``; the folder gets ``_settled`` behind its name.
    ``placement_options``: dict(upsample) of ``--check_placement``; the edit that is rendered (the settled one under ``--settle``) is
    checked and ``placement.json`` written beside the frames; the render itself does not change.
    ``snap_options``: dict(direction, upsample, min_support) of ``--snap_placement``; the folder gets ``_snapped`` behind its name."""
    if (layers_colour or layers_colour_rest) and not save_layers:
        raise ValueError("layers_colour needs save_layers")
    out = Path(f"{rp.output_dirname(config, trajectory_name, test_only, False, False)}_edit_{tag}{'_settled' if settle_options else ''}{'_snapped' if snap_options else ''}")
    device, rank = rp.distributed_device(device)
    scene, model, renderer = rp.load_for_inference(config, device)
    H, W = scene.image_dim
    if callable(edit):              # --follow_shape: the shapes are read from the field, so the edit is resolved once the field is loaded
        edit = edit(scene, model, renderer)
    if ed.as_program(edit).is_shaped and (save_surface or save_layers):
        raise SystemExit(SHAPE_WITH_SURFACE_OR_LAYERS)
    if settle_options:              # (every rank computes the same offset: integer tables of the same lattice)
        edit = settle(model, renderer, edit, **settle_options)[0]
    if snap_options:                # (every rank computes the same integers; rank 0 writes)
        edit = snap(model, renderer, edit, out, write=rank == 0, **snap_options)[0]
    if placement_options:           # (every rank computes the same integers; rank 0 writes)
        check_placement(model, renderer, edit, out, write=rank == 0, **placement_options)
    if save_layers:
        table = rp.layers_table(config, scene, cached_centroids_path)
        table_edit = table.for_program(edit)
        layers_fn = functools.partial(inf.render_rays_layers, table=table, use_delta=bool(config.use_delta))
        edit_layers_fn = functools.partial(inf.render_rays_edit_layers, table=table, edit=edit, use_delta=bool(config.use_delta),
                                           colour=bool(layers_colour), colour_rest=bool(layers_colour_rest))
    if save_surface:
        render_fn = functools.partial(inf.render_rays_edit_surface, edit=edit, weight_thres=float(weight_thres), q=float(surface_quantile))
    else:
        render_fn = functools.partial(inf.render_rays_edit, edit=edit, weight_thres=float(weight_thres))
    if rank == 0:
        for d in ("rgb", "pred_semantics", "depth"):
            (out / d).mkdir(exist_ok=True, parents=True)
    with torch.no_grad():
        for name, rays, K_frame in rp.scene_frames(scene, trajectory_name, test_only):
            p_rgb, p_sem, _, p_dist, *p_surface = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg,
                                                                          render_fn=render_fn)
            if save_layers:         # every rank renders its tiles of the two layer passes (each ends in a collective); rank 0 writes
                lay_after, _, _, *lay_colour = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg, render_fn=edit_layers_fn)
                lay_before = inf.render_rays_sharded(model, renderer, rays, int(config.chunk), scene.white_bg, render_fn=layers_fn)[0]
            if rank != 0:
                continue
            rgb = (p_rgb.reshape(H, W, 3).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
            Image.fromarray(rgb).save(out / "rgb" / f"{name}.png")
            Image.fromarray(p_sem.argmax(dim=1).reshape(H, W).cpu().numpy().astype(np.uint8)).save(out / "pred_semantics" / f"{name}.png")
            np.save(out / "depth" / f"{name}.npy", inf.distance_to_depth(K_frame, p_dist.view(H, W)).reshape(H, W).cpu().numpy())
            if save_surface:
                p_dmed, p_hit, p_nrm = p_surface
                rp.write_surface_frame(out, name, inf.distance_to_depth(K_frame, p_dmed.view(H, W)).reshape(H, W), (p_hit > 0.5).reshape(H, W),
                                       p_nrm.reshape(H, W, 3))
            if save_layers:
                write_layers(out, name, lay_before, lay_after, table, table_edit, H, W, p_rgb, layers_level, colour=lay_colour[0] if lay_colour else None)
                del lay_before, lay_after, lay_colour
    return out


def change_summary(frame_name, before, after, table, table_edit, level):
    """The dict of ``layers/<frame>_change.json``: ``layers.compare`` of the unedited and the edited frame, one entry per slot that has an
    amodal pixel on either side."""
    from contrastive_lift_amd import layers as ly
    col = {k: v.cpu().numpy() for k, v in ly.compare(before, after, table, table_edit, level).items()}
    keys = ("amodal_pixels_before", "amodal_pixels_after", "visible_pixels_before", "visible_pixels_after", "newly_hidden", "revealed", "gone")
    present = np.nonzero((col["amodal_pixels_before"] > 0) | (col["amodal_pixels_after"] > 0))[0]
    return dict(frame=str(frame_name), level=float(level), n_slots=int(table_edit.K), n_base_slots=int(table.K),
                copy_edit=[int(i) for i in table_edit.copy_edit],
                slots=[dict(slot=int(i), slot_class=int(col["slot_class"][i]), slot_index=int(col["slot_index"][i]),
                            **{k: int(col[k][i]) for k in keys}) for i in present])


def write_layers(out, name, before, after, table, table_edit, H, W, p_rgb, level, colour=None):
    """The files of ``--save_layers`` for one frame, from the layers of the unedited (``before``) and the edited (``after``) frame: the
    edited scene's written like ``render_panopli.py --save_layers`` writes a plain one (with ``colour``, the edited scene's colour layers,
    like ``--layers_colour``: a copy has a slot and so an image of its own), and ``layers/<frame>_change.json``."""
    rp.write_layers_frame(out, name, after, table_edit, H, W, p_rgb, level, **({} if colour is None else {"colour": colour}))
    with open(out / "layers" / f"{name}_change.json", "w") as f:
        json.dump(change_summary(name, before, after, table, table_edit, level), f, indent=1)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--bboxes", type=str, required=True, help="bboxes.pkl of inference/fit_bboxes.py")
    ap.add_argument("--instance", type=int, help="instance id (a key of bboxes.pkl); required without --script")
    ap.add_argument("--op", choices=OPS, help="required without --script")
    ap.add_argument("--script", type=str, metavar="FILE.json",
                    help="an ordered list of edits applied in one render (see the doc string); instead of --instance / --op")
    ap.add_argument("--translate", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="copy / move: translation t")
    ap.add_argument("--rotate_deg", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("RX", "RY", "RZ"),
                    help="copy / move: rotation about the box centre, R = Rz Ry Rx (degrees)")
    ap.add_argument("--pad", type=float, default=0.0, help="grow the fitted box by this much on every side")
    ap.add_argument("--render_trajectory", action="store_true")
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384])
    ap.add_argument("--weight_thres", type=float, default=0.0,
                    help="evaluate the heads where w > this (0: every sample with weight, like the reference's edit renders; 1e-4: the plain render's threshold)")
    ap.add_argument("--save_surface", action="store_true",
                    help="also write surface/<frame>.npz (depth_median, hit, normals) and vis_normals/<frame>.png of the EDITED scene, as "
                         "inference/render_panopli.py --save_surface does for the unedited one")
    ap.add_argument("--surface_quantile", type=float, default=0.5, metavar="Q",
                    help="--save_surface: the hit is where the ray has lost this share of its transmittance (0.5: the median depth)")
    ap.add_argument("--save_layers", action="store_true",
                    help="also write layers/<frame>.npz, layers/<frame>.json, vis_amodal/<frame>.png of the EDITED scene (one more slot per copy) "
                         "and layers/<frame>_change.json, what the edit hid, revealed or removed per slot")
    ap.add_argument("--cached_centroids_path", type=str, default=None,
                    help="--save_layers: all_centroids.pkl of inference/extract_train_centroids.py (not needed for a linear_assignment model)")
    ap.add_argument("--layers_level", type=float, default=0.5, help="the opacity above which --save_layers counts a pixel into a mask")
    rp.add_layers_colour_arguments(ap)
    add_shape_arguments(ap)
    ap.add_argument("--settle", type=str, nargs="?", const="-z", default=None, metavar="AXIS",
                    help="with --op move|copy, or a --script that ends in one: drop the object that the last edit places along AXIS (one of "
                         "+x -x +y -y +z -z, default -z) until it touches the rest of the edited scene, report the lattice steps and the faces "
                         "in contact, and render into ..._settled.  A BOX move carries a slab of its surroundings along, so its travel is "
                         "usually 0: --follow_shape is the intended companion")
    ap.add_argument("--settle_upsample", type=int, default=None, metavar="U", help="--settle: the lattice is the grid times this factor per axis (default 1)")
    ap.add_argument("--settle_slack", type=int, default=None, metavar="S",
                    help="--settle: count the faces up to S lattice steps further away than the first contact (0 .. 4, default 0)")
    ap.add_argument("--check_placement", action="store_true",
                    help="with --op move|copy, or a --script that ends in one: say whether the object that the last edit places collides with "
                         "what stood there -- on how many lattice cells and how deep -- or how far it is from the rest of the scene (the true "
                         "distance, not along an axis), and write placement.json beside the frames.  With --settle the settled edit is checked")
    ap.add_argument("--placement_upsample", type=int, default=None, metavar="U",
                    help="--check_placement: the lattice is the grid times this factor per axis (default 1)")
    ap.add_argument("--snap_placement", type=str, nargs="?", const="-z", default=None, metavar="AXIS",
                    help="with --op move|copy, or a --script that ends in one: move the object that the last edit places to the nearest "
                         "translation at which it collides with nothing and rests on faces that look along AXIS (one of +x -x +y -y +z -z, "
                         "default -z), report the steps and the faces, write snap.json and render into ..._snapped.  Not together with --settle")
    ap.add_argument("--snap_upsample", type=int, default=None, metavar="U", help="--snap_placement: the lattice is the grid times this factor per axis (default 1)")
    ap.add_argument("--snap_min_support", type=int, default=None, metavar="F",
                    help="--snap_placement: the faces along AXIS that a position needs to count as supported (>= 1, default 1)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):                                    # "--settle -z": argparse would read the value as an option
        if argv[i] in ("--settle", "--snap_placement") and argv[i + 1] in UP_AXES:
            argv[i:i + 2] = [f"{argv[i]}={argv[i + 1]}", None]
    args = ap.parse_args([x for x in argv if x is not None])
    rp.check_layers_colour_arguments(ap, args)
    if args.settle is None:
        for flag in ("settle_upsample", "settle_slack"):
            if getattr(args, flag) is not None:
                ap.error(f"--{flag} needs --settle")
    else:
        if args.settle not in UP_AXES:
            ap.error(f"--settle: AXIS is one of {' '.join(UP_AXES)} (got {args.settle!r})")
        if args.script is None and args.op not in ("move", "copy"):
            ap.error(SETTLE_WANTS_A_MOTION)
        args.settle_upsample = 1 if args.settle_upsample is None else args.settle_upsample
        args.settle_slack = 0 if args.settle_slack is None else args.settle_slack
        if args.settle_upsample < 1:
            ap.error(f"--settle_upsample must be >= 1 (got {args.settle_upsample})")
        if not 0 <= args.settle_slack <= 4:
            ap.error(f"--settle_slack must be 0 .. 4 (got {args.settle_slack})")
    if args.snap_placement is None:
        for flag in ("snap_upsample", "snap_min_support"):
            if getattr(args, flag) is not None:
                ap.error(f"--{flag} needs --snap_placement")
    else:
        if args.snap_placement not in UP_AXES:
            ap.error(f"--snap_placement: AXIS is one of {' '.join(UP_AXES)} (got {args.snap_placement!r})")
        if args.settle is not None:
            ap.error(SNAP_WITH_SETTLE)
        if args.script is None and args.op not in ("move", "copy"):
            ap.error(SNAP_WANTS_A_MOTION)
        args.snap_upsample = 1 if args.snap_upsample is None else args.snap_upsample
        args.snap_min_support = 1 if args.snap_min_support is None else args.snap_min_support
        if args.snap_upsample < 1:
            ap.error(f"--snap_upsample must be >= 1 (got {args.snap_upsample})")
        if args.snap_min_support < 1:
            ap.error(f"--snap_min_support must be >= 1 (got {args.snap_min_support})")
    if not args.check_placement:
        if args.placement_upsample is not None:
            ap.error("--placement_upsample needs --check_placement")
    else:
        if args.script is None and args.op not in ("move", "copy"):
            ap.error(PLACEMENT_WANTS_A_MOTION)
        args.placement_upsample = 1 if args.placement_upsample is None else args.placement_upsample
        if args.placement_upsample < 1:
            ap.error(f"--placement_upsample must be >= 1 (got {args.placement_upsample})")
    if args.follow_shape and (args.save_surface or args.save_layers):
        raise SystemExit(SHAPE_WITH_SURFACE_OR_LAYERS)
    if args.script is not None and (args.instance is not None or args.op is not None):
        ap.error("--script holds the edits: give it without --instance / --op")
    if args.script is None and (args.instance is None or args.op is None):
        ap.error("--instance and --op are required without --script")
    return args


def main(argv=None):
    args = parse_args(argv)
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.subsample_frames = 1
    cfg.image_dim = list(args.image_dim)
    with open(args.bboxes, "rb") as f:
        boxes = pickle.load(f)
    entries = None
    if args.script is not None:
        with open(args.script) as f:
            entries, tag = json.load(f), f"script_{Path(args.script).stem}"
    else:
        tag = f"{args.op}_{args.instance}"
    shaped = args.follow_shape or script_asks_for_shapes(args.script)
    if shaped and (args.save_surface or args.save_layers):
        raise SystemExit(SHAPE_WITH_SURFACE_OR_LAYERS)

    def the_edit(scene, model, renderer):
        shape_of = None
        if shaped:
            table = shape_table(cfg, scene, args.cached_centroids_path)
            shape_of = field_shapes(model, renderer, table, args.shape_grid, args.shape_grow, args.shape_alpha, bool(cfg.use_delta))
        if entries is not None:
            return resolve_program(boxes, entries, follow_shape=args.follow_shape, shape_of=shape_of)
        return resolve_edit(boxes, args.instance, args.op, args.translate, args.rotate_deg, args.pad, shape=shape_of)
    if args.follow_shape:
        tag += "_shape"
    if not shaped:                  # (no field is needed: resolve now, so that a bad script stops before the checkpoint is loaded)
        the_edit = the_edit(None, None, None)
        if args.settle is not None:
            check_settle(the_edit)
        if args.check_placement:
            check_placement_edit(the_edit)
        if args.snap_placement is not None:
            check_snap(the_edit)
    settle_options = None if args.settle is None else dict(direction=args.settle, upsample=args.settle_upsample, slack=args.settle_slack)
    print(edit_scene_checkpoint(cfg, the_edit, tag, test_only=not args.render_trajectory, weight_thres=args.weight_thres,
                                save_surface=args.save_surface, surface_quantile=args.surface_quantile, save_layers=args.save_layers,
                                cached_centroids_path=args.cached_centroids_path, layers_level=args.layers_level,
                                layers_colour=args.layers_colour, layers_colour_rest=args.layers_colour_rest,
                                **({} if settle_options is None else {"settle_options": settle_options}),
                                **({"placement_options": dict(upsample=args.placement_upsample)} if args.check_placement else {}),
                                **({} if args.snap_placement is None else
                                   {"snap_options": dict(direction=args.snap_placement, upsample=args.snap_upsample, min_support=args.snap_min_support)})))


if __name__ == "__main__":
    main()
