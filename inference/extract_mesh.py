#!/usr/bin/env python3
"""Export a trained scene as a labelled surface mesh: every vertex carries colour, semantic class and instance id.

    python inference/extract_mesh.py --ckpt_path runs/<experiment>/checkpoints/<x>.ckpt [--upsample 2] [--alpha_level 0.5 | --level SIGMA]
                                     [--cached_centroids_path all_centroids.pkl] [--split_instances] [--save_voxel_cloud]
                                     [--min_component VOXELS] [--keep_largest K] [--connectivity {6,kuhn,26}] [--split_disconnected [MIN_VOXELS]]
                                     [--relations [--relations_gap 1] [--up_axis +z] [--relations_min_faces 4]]
                                     [--clearance [--clearance_slack 0]] [--separation [--separation_max_cells N]]
                                     [--bboxes bboxes.pkl (--instance ID --op delete|extract|copy|move [--translate x y z] [--rotate_deg rx ry rz]
                                                           [--pad 0.0] | --script edits.json)]

The checkpoint is loaded exactly as by ``inference/render_panopli.py`` (its ``load_for_inference``).  sigma is evaluated on the
``upsample``-times refined lattice of the scene box (``TensoRFRenderer.get_dense_sigma``, the reference's renderer.py:731-748, one launch),
its iso-surface is extracted on the device by marching tetrahedra (``mesh.extract_isosurface``: deterministic, scan ordered, closed and
consistently oriented wherever the surface stays off the box), and every vertex is labelled by the field's own heads
(``mesh.label_vertices``): class = argmax of the semantic head, colour = the appearance head seen along minus the normal, instance id =
the nearest cached centroid of the vertex's class, numbered like ``pred_surrogateid`` (0 = stuff) -- or, without
``--cached_centroids_path``, 1 + the argmax of the instance head for vertices of thing classes (the reference's per-voxel rule of
``get_instance_clusters``; meaningful for ``linear_assignment`` models) and 0 for stuff.

Writes ``mesh.ply`` (binary little-endian; x y z nx ny nz red green blue semantic instance, int face lists) into the folder
``render_panopli.py`` renders to; ``--split_instances`` adds ``mesh_instance_<id>.ply`` per instance id (the faces whose three vertices
carry that id); ``--save_voxel_cloud`` adds ``voxelcloud.pkl``: the voxels of ``get_instance_clusters(mode='alpha')`` (drawn with seed 0)
with class and instance id by the same rule as the vertices and a colour from the appearance head at a ZERO view direction (a voxel
has no normal), in the layout of ``pointcloud.pkl``, so ``inference/fit_bboxes.py --pointcloud`` reads it unchanged -- unlike ``pointcloud.pkl`` it
holds the whole occupied volume, not only what some test camera saw.  Prints the time of every stage (device events).

The raw iso-surface of a learnt density is full of floaters.  ``--min_component VOXELS`` / ``--keep_largest K`` label the connected components
of the inside lattice points on the device (``components.filter_components``, clift_cc_label) and push the small ones below the level before
the surface is extracted: with the default ``--connectivity kuhn`` (the mesher's own seven edge classes) a mesh face belongs to exactly one
component, so what is left is the unfiltered mesh minus whole closed pieces.  ``--split_disconnected [MIN_VOXELS]`` cures ids that two
objects share across the room (the nearest centroid knows nothing of space): every inside lattice point gets its id by the vertices' rule
(zero normals, as for the voxel cloud), the lattice of thing ids is split into components (``components.split_disconnected``: the largest
piece of an id keeps it, every other piece of at least MIN_VOXELS points gets a fresh id), and a vertex takes the new id of the inside
endpoint of its edge wherever its own id is that point's original id.  Without these flags the files are byte-identical to what the tool
wrote before it had them.  (The voxel cloud lives on another lattice, the model grid: it is neither filtered nor split.)

``--bboxes`` with ``--instance`` / ``--op`` or with ``--script`` meshes the EDITED scene: the edit (``inference/edit_scene.py``'s
``resolve_edit`` / ``resolve_program``: the same boxes, the same rigid copy / move, the same script format) is walked at every lattice point
inside the density launch (``get_dense_sigma(edit=)``, clift_edit_list_dense_sigma) and at every vertex before it is labelled
(``label_vertices(edit=)``), so a moved object keeps its class, id and colour and a copy carries the original's id (``--split_disconnected``
gives the copy a fresh one).  The file is ``mesh_edit_<op>_<id>.ply`` or ``mesh_edit_script_<stem>.ply`` beside ``mesh.ply``, the
``--split_instances`` files are ``mesh_edit_..._instance_<id>.ply``; the component flags act on the edited lattice.  At a cut face -- where
a box face passes through matter: an extracted or moved object's sides, the hole a delete leaves -- the mesh is closed by a cap whose colour
and labels are the field's values just inside the object.  ``--save_voxel_cloud`` is refused together with an edit: that cloud lives on the
model grid through ``get_instance_clusters``, which knows nothing of edits.  ``--follow_shape`` (with ``--shape_grid``, ``--shape_grow``,
``--shape_alpha``, as in inference/edit_scene.py) makes the edits follow the instance's shape, not its box: the shapes are
read from the field once it is loaded, the slot table comes from ``--cached_centroids_path`` (a linear-assignment model needs none), and
the file is ``mesh_edit_<tag>_shape.ply``.

``--relations`` says how the instances stand to one another on the lattice that is meshed (after ``--min_component`` / ``--keep_largest``):
every inside lattice point gets its class and id in one call (``lattice_nodes``, by the vertices' rule with zero normals; with
``--split_disconnected`` the split ids, so a copy and its original are two nodes), every (class, id) pair becomes a node
(``relations.node_keys``), and one kernel counts per node its extent and free faces and per pair of nodes the lattice faces between them
and the contacts across at most ``--relations_gap`` empty lattice points (``relations.lattice_relations``, clift_lattice_relations).
``relations.npz`` (``relations_edit_<tag>.npz`` under an edit) holds the raw tables and the node list, ``relations.json`` (``relations_edit_
<tag>.json``) the scene graph (``relations.SceneGraph``): per node voxels, volume, centroid, box and free area, and "on" (along ``--up_axis``,
with its support ratio) and "beside" between nodes with at least ``--relations_min_faces`` contacts.  Under an edit the lattice and the
labels are the edited scene's, labelled where the content came from: the graph of a move shows what the moved object touches at its
destination.  Without the flag nothing changes.

``--clearance`` says how far every node of that labelled lattice -- the nodes of ``--relations``; with both flags the labelling is done once --
can travel along the six lattice directions before it meets another node (``clearance.lattice_clearance``, clift_lattice_clearance: a look
of unbounded length, where ``--relations_gap`` stops after 4 points).  ``clearance.npz`` (``clearance_edit_<tag>.npz`` under an edit) holds
the raw tables pair, travel and landing and the node list, ``clearance.json`` (``clearance_edit_<tag>.json``) per node and direction the
steps, the distance, the nodes it would then rest on with their face counts (``--clearance_slack S``: up to S steps further away) and the
steps to the lattice border (``clearance.Clearance``).  ``relations.json`` and ``relations.npz`` do not change.

``--separation`` gives the true distance between every two nodes of that labelled lattice (the labelling is shared with ``--relations`` and
``--clearance``), diagonal neighbours included, which the axis looks of the two other stages cannot see (``distance.separation``,
clift_lattice_distance: one exact Euclidean distance transform per node, at most 255 nodes).  ``separation.npz``
(``separation_edit_<tag>.npz`` under an edit) holds the raw tables gap2, at and to and the node list, ``separation.json``
(``separation_edit_<tag>.json``) per node its nearest other node and per pair of nodes the distance in lattice steps and in world units
with the two points (``distance.Separation``; ``--separation_max_cells N``: only the pairs at most N steps apart).  The other files do not
change.
"""
import argparse
import os
import pickle
import random
import sys
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import render_panopli as rp                                           # noqa: E402
from contrastive_lift_amd import clearance as clr                     # noqa: E402
from contrastive_lift_amd import distance as dt                       # noqa: E402
from contrastive_lift_amd import components as cc                     # noqa: E402
from contrastive_lift_amd import lattice                              # noqa: E402
from contrastive_lift_amd import mesh as cm                           # noqa: E402
from contrastive_lift_amd import relations as rel                     # noqa: E402
from contrastive_lift_amd.config import load_run_config               # noqa: E402


def default_level(renderer, alpha_level):
    """The sigma at which ONE sample of a training step would have opacity ``alpha_level``: alpha = 1 - exp(-sigma step distance_scale).
    ``renderer`` comes from ``load_for_inference``, which halves the step ratio (RP:104): the training step is twice its step.
    (``lattice.default_level``, which ``clearance.settle_offset`` shares; a bad ``alpha_level`` ends the tool.)"""
    try:
        return lattice.default_level(renderer, alpha_level)
    except ValueError as err:
        raise SystemExit(str(err))


class StageTimer:
    """Device time of consecutive stages (events on the current stream), printed at the end."""

    def __init__(self):
        self.marks = [("", self._event())]

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def done(self, name):
        self.marks.append((name, self._event()))

    def report(self):
        torch.cuda.synchronize()
        times = {name: self.marks[i][1].elapsed_time(e) for i, (name, e) in enumerate(self.marks[1:])}
        print("stage times (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in times.items()))
        return times


def surrogate_ids(model, renderer, points, normals, thing_classes, centroids, use_delta, chunk=2 ** 20, edit=None):
    """(semantics, instances, rgb) of world points: ``mesh.label_vertices``; without centroids its 0-based head argmax becomes 1 + argmax
    on thing classes and 0 on stuff, so that 0 means stuff in every file this tool writes.  ``edit``: the points are points of the edited
    scene (``label_vertices(edit=)``)."""
    kw = {} if edit is None else {"edit": edit}
    sem, inst, rgb = cm.label_vertices(model, renderer, points, normals, thing_classes, centroids=centroids, chunk=chunk, use_delta=use_delta, **kw)
    if centroids is None:
        thing = torch.isin(sem, torch.tensor(sorted(int(c) for c in thing_classes), dtype=torch.int64, device=sem.device))
        inst = torch.where(thing, inst + 1, torch.zeros_like(inst))
    return sem, inst, rgb


def lattice_ids(model, renderer, sigma, level, things, centroids, use_delta, chunk=2 ** 20, edit=None):
    """The id lattice ``--split_disconnected`` works on: (n0, n1, n2) int32, the instance id (``surrogate_ids`` with zero normals) of every
    inside lattice point of a thing class, 0 elsewhere.  ONE call for all inside points: with centroids the numbering offsets every class
    by the labels seen before it in that call, so ids of separate calls do not compare; ``chunk`` only bounds the field evaluation inside
    ``mesh.label_vertices``.  ``edit``: sigma is the edited lattice, and every point is labelled where its content came from."""
    inside = (sigma >= torch.tensor(float(level), dtype=torch.float32, device=sigma.device)).reshape(-1).nonzero().reshape(-1)
    ids = torch.zeros(sigma.numel(), dtype=torch.int32, device=sigma.device)
    ticks = renderer.lattice_ticks(sigma.shape)
    n1, n2 = int(sigma.shape[1]), int(sigma.shape[2])
    xyz = torch.stack([ticks[0][inside // (n1 * n2)], ticks[1][(inside // n2) % n1], ticks[2][inside % n2]], 1).contiguous()
    ids[inside] = surrogate_ids(model, renderer, xyz, torch.zeros_like(xyz), things, centroids, use_delta, chunk=chunk, edit=edit)[1].int()
    return ids.view(sigma.shape)


def lattice_nodes(model, renderer, sigma, level, things, centroids, use_delta, chunk=2 ** 20, edit=None):
    """The sibling of ``lattice_ids`` that keeps the class -> (sem, ids), both (n0, n1, n2) int32: class and instance id of every inside
    lattice point by the same ONE call of ``surrogate_ids`` with zero normals (``ids`` is what ``lattice_ids`` returns: 0 on stuff), and
    sem = -1, ids = 0 outside."""
    inside = (sigma >= torch.tensor(float(level), dtype=torch.float32, device=sigma.device)).reshape(-1).nonzero().reshape(-1)
    sem = torch.full((sigma.numel(),), -1, dtype=torch.int32, device=sigma.device)
    ids = torch.zeros(sigma.numel(), dtype=torch.int32, device=sigma.device)
    ticks = renderer.lattice_ticks(sigma.shape)
    n1, n2 = int(sigma.shape[1]), int(sigma.shape[2])
    xyz = torch.stack([ticks[0][inside // (n1 * n2)], ticks[1][(inside // n2) % n1], ticks[2][inside % n2]], 1).contiguous()
    if inside.numel():
        p_sem, p_ids, _ = surrogate_ids(model, renderer, xyz, torch.zeros_like(xyz), things, centroids, use_delta, chunk=chunk, edit=edit)
        sem[inside], ids[inside] = p_sem.int(), p_ids.int()
    return sem.view(sigma.shape), ids.view(sigma.shape)


def scene_relations(renderer, sem, ids, gap=1, up="+z", min_faces=4):
    """The relations of a labelled lattice (``lattice_nodes``; ``ids`` may be the split ids) -> dict(tables, nodes, key, graph)."""
    key, nodes = rel.node_keys(sem, ids)
    if len(nodes) + 1 > rel.MAX_KEYS:
        raise SystemExit(f"--relations: {len(nodes)} (class, instance) nodes, at most {rel.MAX_KEYS - 1} can be related -- raise --min_component "
                         f"or the MIN_VOXELS of --split_disconnected on a frothy scene")
    tables = rel.lattice_relations(key, n_keys=len(nodes) + 1, gap=int(gap))
    graph = rel.SceneGraph.from_counts(tables, nodes, renderer.lattice_ticks(key.shape), up=up, min_faces=min_faces)
    return dict(tables=tables, nodes=nodes, key=key, graph=graph)


def relations_stem(edit_tag=None):
    """File stem of the relations: ``relations``, or ``relations_edit_<tag>`` for an edited scene; ``<stem>.npz`` and ``<stem>.json``."""
    return "relations" if edit_tag is None else f"relations_edit_{edit_tag}"


def write_relations(out, stem, r, gap):
    """``<stem>.npz``: the raw tables (near absent at gap 0), the node list (K, 2) = (class, instance) of keys 1..K, and the gap;
    ``<stem>.json``: the graph."""
    arrays = {k: v.cpu().numpy() for k, v in r["tables"].items() if v is not None}
    np.savez(Path(out) / f"{stem}.npz", nodes=np.asarray(r["nodes"], np.int64).reshape(-1, 2), gap=np.asarray(int(gap)), **arrays)
    with open(Path(out) / f"{stem}.json", "w") as f:
        f.write(r["graph"].to_json(indent=1))


def scene_clearance(renderer, sem, ids, slack=0, related=None):
    """The clearance of a labelled lattice (``lattice_nodes``; ``ids`` may be the split ids) -> dict(tables, nodes, key, summary, slack).
    ``related``: the result of ``scene_relations`` on the same labels -- its keys, nodes and index boxes are used as they are."""
    key, nodes = (related["key"], related["nodes"]) if related is not None else rel.node_keys(sem, ids)
    if len(nodes) + 1 > rel.MAX_KEYS:
        raise SystemExit(f"--clearance: {len(nodes)} (class, instance) nodes, at most {rel.MAX_KEYS - 1} can be swept -- raise --min_component "
                         f"or the MIN_VOXELS of --split_disconnected on a frothy scene")
    tables = clr.lattice_clearance(key, n_keys=len(nodes) + 1, slack=int(slack))
    box = dict(relations=related["tables"]) if related is not None else dict(key=key)
    summary = clr.Clearance.from_tables(tables, nodes, renderer.lattice_ticks(key.shape), slack=int(slack), **box)
    return dict(tables=tables, nodes=nodes, key=key, summary=summary, slack=int(slack))


def clearance_stem(edit_tag=None):
    """File stem of the clearance: ``clearance``, or ``clearance_edit_<tag>`` for an edited scene; ``<stem>.npz`` and ``<stem>.json``."""
    return "clearance" if edit_tag is None else f"clearance_edit_{edit_tag}"


def write_clearance(out, stem, c):
    """``<stem>.npz``: the raw tables, the node list (K, 2) = (class, instance) of keys 1..K, and the slack; ``<stem>.json``: the summary."""
    arrays = {k: v.cpu().numpy() for k, v in c["tables"].items()}
    np.savez(Path(out) / f"{stem}.npz", nodes=np.asarray(c["nodes"], np.int64).reshape(-1, 2), slack=np.asarray(int(c["slack"])), **arrays)
    with open(Path(out) / f"{stem}.json", "w") as f:
        f.write(c["summary"].to_json(indent=1))


def scene_separation(renderer, sem, ids, max_cells=None, related=None):
    """The true gaps between the nodes of a labelled lattice (``lattice_nodes``; ``ids`` may be the split ids) -> dict(tables, nodes, key,
    summary).  ``related``: a result of ``scene_relations`` or ``scene_clearance`` on the same labels -- its keys and nodes are used."""
    key, nodes = (related["key"], related["nodes"]) if related is not None else rel.node_keys(sem, ids)
    if len(nodes) + 1 > dt.MAX_SEPARATION_KEYS:
        raise SystemExit(f"--separation: {len(nodes)} (class, instance) nodes, at most {dt.MAX_SEPARATION_KEYS - 1} get a transform each -- raise "
                         f"--min_component or the MIN_VOXELS of --split_disconnected on a frothy scene")
    tables = dt.separation(key, n_keys=len(nodes) + 1)
    summary = dt.Separation.from_tables(tables, nodes, renderer.lattice_ticks(key.shape), max_cells=max_cells)
    return dict(tables=tables, nodes=nodes, key=key, summary=summary)


def separation_stem(edit_tag=None):
    """File stem of the separation: ``separation``, or ``separation_edit_<tag>`` for an edited scene; ``<stem>.npz`` and ``<stem>.json``."""
    return "separation" if edit_tag is None else f"separation_edit_{edit_tag}"


def write_separation(out, stem, s):
    """``<stem>.npz``: the raw tables gap2, at, to and the node list (K, 2) = (class, instance) of keys 1..K; ``<stem>.json``: the summary."""
    arrays = {k: s["tables"][k].cpu().numpy() for k in ("gap2", "at", "to")}
    np.savez(Path(out) / f"{stem}.npz", nodes=np.asarray(s["nodes"], np.int64).reshape(-1, 2), **arrays)
    with open(Path(out) / f"{stem}.json", "w") as f:
        f.write(s["summary"].to_json(indent=1))


def split_vertex_ids(inst, keys, sigma, level, ids, min_voxels, connectivity, return_lattice=False):
    """-> (vertex ids after the split, table {fresh id: parent}).  A vertex takes the new id of the inside endpoint of its edge when its own
    id equals that point's original id; otherwise it keeps its id.  Fresh ids start above every id in use, the vertices' included (a vertex
    on a class boundary can carry an id that no lattice point has).  ``return_lattice``: the id lattice after the split as a third result."""
    above = int(inst.max()) + 1 if inst.numel() else 1
    new_ids, table = cc.split_disconnected(ids, connectivity=connectivity, min_voxels=min_voxels, first_fresh=above)
    at = cc.vertex_owner_inside(keys, sigma, level)
    old, new = ids.reshape(-1)[at].long(), new_ids.reshape(-1)[at].long()
    out = torch.where(inst == old, new, inst)
    return (out, table, new_ids) if return_lattice else (out, table)


def surface_stages(model, renderer, sigma, level, things, centroids, use_delta, timer, min_component=0, keep_largest=None, connectivity="kuhn",
                   split_disconnected=None, edit=None, relations=None, clearance=None, separation=None):
    """Everything between the density lattice and the files: (components) - isosurface - label_vertices - (split), each closed by a mark
    of ``timer``.  ``edit``: sigma is the lattice of the edited scene (``get_dense_sigma(edit=)``); vertices and lattice points are then
    labelled where their content came from.  -> dict(verts, faces, normals, sem, inst, rgb, sigma (as meshed), info (of filter_components, or None), table (of
    split_disconnected, or None)).  ``relations``: dict(gap, up, min_faces) adds the stage "relations" and the key ``relations``
    (``scene_relations`` of the lattice as meshed; with ``split_disconnected`` on the split ids).  ``clearance``: dict(slack) adds the stage
    "clearance" and the key ``clearance`` (``scene_clearance`` of the same labels; with ``relations`` the labelling is shared).
    ``separation``: dict(max_cells) adds the stage "separation" and the key ``separation`` (``scene_separation``, the labelling shared)."""
    info = table = None
    labelled = relations is not None or clearance is not None or separation is not None
    if int(min_component or 0) > 0 or keep_largest is not None:
        sigma, info = cc.filter_components(sigma, level, min_voxels=min_component, keep_largest=keep_largest, connectivity=connectivity)
        timer.done("components")
    verts, faces, normals, *keys = cm.extract_isosurface(sigma, level, renderer.lattice_ticks(sigma.shape), return_keys=split_disconnected is not None)
    timer.done("isosurface")
    sem, inst, rgb = surrogate_ids(model, renderer, verts, normals, things, centroids, use_delta, edit=edit)
    timer.done("label_vertices")
    if labelled:                                                      # class and id of the inside points, once: the split below works on these ids
        p_sem, p_ids = lattice_nodes(model, renderer, sigma, level, things, centroids, use_delta, edit=edit)
        if split_disconnected is None:
            timer.done("lattice_nodes")
    if split_disconnected is not None:
        ids = lattice_ids(model, renderer, sigma, level, things, centroids, use_delta, edit=edit) if not labelled else p_ids
        inst, table, *split = split_vertex_ids(inst, keys[0], sigma, level, ids, int(split_disconnected), connectivity, return_lattice=labelled)
        timer.done("split")
    out = dict(verts=verts, faces=faces, normals=normals, sem=sem, inst=inst, rgb=rgb, sigma=sigma, info=info, table=table)
    if relations is not None:
        out["relations"] = scene_relations(renderer, p_sem, split[0] if split_disconnected is not None else p_ids, **relations)
        timer.done("relations")
    if clearance is not None:
        out["clearance"] = scene_clearance(renderer, p_sem, split[0] if split_disconnected is not None else p_ids, related=out.get("relations"), **clearance)
        timer.done("clearance")
    if separation is not None:
        out["separation"] = scene_separation(renderer, p_sem, split[0] if split_disconnected is not None else p_ids,
                                             related=out.get("relations") or out.get("clearance"), **separation)
        timer.done("separation")
    return out


def extract_mesh(config, upsample=2, alpha_level=0.5, level=None, cached_centroids_path=None, split_instances=False, save_voxel_cloud=False,
                 device="cuda:0", min_component=0, keep_largest=None, connectivity="kuhn", split_disconnected=None, edit=None, edit_tag=None, relations=None,
                 clearance=None, separation=None):
    """``relations``: dict(gap, up, min_faces) of ``--relations``; ``clearance``: dict(slack) of ``--clearance``; ``separation``: dict(max_cells) of ``--separation``.``edit`` (an ``edit.Edit`` / ``EditProgram``) with its ``edit_tag`` (``edit_tag_of``): mesh the edited scene into ``mesh_edit_<tag>.ply``.
    ``edit`` may be a callable ``edit(config, scene, model, renderer)`` that resolves it once the field is loaded (``--follow_shape``)."""
    if edit is not None and save_voxel_cloud:
        raise SystemExit(VOXEL_CLOUD_WITH_EDIT)
    if edit is not None and not edit_tag:
        raise ValueError("extract_mesh: an edit needs its edit_tag (the file is mesh_edit_<tag>.ply)")
    stem = mesh_stem(edit_tag if edit is not None else None)
    out = rp.output_dirname(config, "trajectory_blender", True, False, False)
    out.mkdir(exist_ok=True, parents=True)
    device = torch.device(device)
    scene, model, renderer = rp.load_for_inference(config, device)
    things = list(scene.segmentation_data.fg_classes)
    centroids = None
    if cached_centroids_path is not None:
        with open(cached_centroids_path, "rb") as f:
            centroids = pickle.load(f)
    level = default_level(renderer, alpha_level) if level is None else float(level)
    use_delta = bool(getattr(config, "use_delta", False))
    if callable(edit):
        edit = edit(config, scene, model, renderer)
    timer = StageTimer()
    sigma = renderer.get_dense_sigma(model, upsample) if edit is None else renderer.get_dense_sigma(model, upsample, edit=edit)
    timer.done("dense_sigma")
    m = surface_stages(model, renderer, sigma, level, things, centroids, use_delta, timer, min_component=min_component, keep_largest=keep_largest,
                       connectivity=connectivity, split_disconnected=split_disconnected, edit=edit, **({} if relations is None else {"relations": relations}),
                       **({} if clearance is None else {"clearance": clearance}), **({} if separation is None else {"separation": separation}))
    verts, faces, normals, sem, inst, rgb = (m[k] for k in ("verts", "faces", "normals", "sem", "inst", "rgb"))
    times = timer.report()
    print(f"sigma lattice {tuple(sigma.shape)}, level {level:.6g}: {verts.shape[0]} vertices, {faces.shape[0]} faces, "
          f"instance ids {sorted(torch.unique(inst).tolist())}")
    if m["info"] is not None:
        print(f"components ({connectivity}): {m['info']['K']} of the inside set, {len(m['info']['kept'])} kept, "
              f"{m['info']['dropped']} lattice points dropped")
    if m["table"] is not None:
        print(f"split_disconnected ({connectivity}, pieces of at least {int(split_disconnected)} points): {len(m['table'])} fresh ids")
    cm.write_ply(out / f"{stem}.ply", verts, faces, normals, rgb, sem, inst)
    if relations is not None:
        write_relations(out, relations_stem(edit_tag if edit is not None else None), m["relations"], relations["gap"])
        g = m["relations"]["graph"]
        print(f"relations (gap {relations['gap']}, up {relations['up']}): {len(g.nodes)} nodes, {len(g.pairs)} pairs in contact, "
              f"{sum(r['relation'] == 'on' for r in g.relations)} on, {sum(r['relation'] == 'beside' for r in g.relations)} beside")
    if clearance is not None:
        write_clearance(out, clearance_stem(edit_tag if edit is not None else None), m["clearance"])
        c = m["clearance"]["summary"]
        print(f"clearance (slack {clearance['slack']}): {len(c.nodes)} nodes, "
              f"{sum(d['steps'] is not None for n in c.nodes for d in n['directions'].values())} of {6 * len(c.nodes)} looks end at another node")
    if separation is not None:
        write_separation(out, separation_stem(edit_tag if edit is not None else None), m["separation"])
        s = m["separation"]["summary"]
        closest = min(s.pairs, key=lambda p: p["gap2"], default=None)
        print(f"separation: {len(s.nodes)} nodes, {len(s.pairs)} pairs" + (f" within {s.max_cells:g} cells" if s.max_cells is not None else "")
              + (f", the closest {closest['a']} - {closest['b']} at {closest['cells']:.2f} cells = {closest['distance']:.4f}" if closest else ""))
    if split_instances:
        f_inst = inst[faces.long()]                                   # (F, 3)
        for i in torch.unique(inst).tolist():
            sel = faces[(f_inst == i).all(1)].long()
            if sel.shape[0] == 0:
                continue
            used, renum = torch.unique(sel, return_inverse=True)
            cm.write_ply(out / f"{stem}_instance_{int(i)}.ply", verts[used], renum.int(), normals[used], rgb[used], sem[used], inst[used])
    if save_voxel_cloud:
        state = random.getstate()                                     # the draw is seeded for a reproducible file; the caller's generator is put back
        random.seed(0)
        try:
            xyz, _ = renderer.get_instance_clusters(model, "alpha")
        finally:
            random.setstate(state)
        v_sem, v_inst, v_rgb = surrogate_ids(model, renderer, xyz, torch.zeros_like(xyz), things, centroids, use_delta)
        cloud = {"points": xyz.cpu().numpy().astype(np.float32), "instances": v_inst.cpu().numpy().astype(np.uint16),
                 "semantics": v_sem.cpu().numpy().astype(np.uint8), "rgb": (v_rgb.cpu().numpy().clip(0, 1) * 255).astype(np.uint8)}
        with open(out / "voxelcloud.pkl", "wb") as f:
            pickle.dump(cloud, f)
    return out, times


VOXEL_CLOUD_WITH_EDIT = ("--save_voxel_cloud cannot be combined with an edit: the voxel cloud lives on the model grid through "
                         "get_instance_clusters, which knows nothing of edits -- export it without --bboxes")
EDIT_OPS = ("delete", "extract", "copy", "move")                      # edit_scene.OPS (checked in resolve_cli_edit)


def mesh_stem(edit_tag=None):
    """File stem of the mesh: ``mesh``, or ``mesh_edit_<tag>`` for an edited scene; ``<stem>.ply`` and ``<stem>_instance_<id>.ply``."""
    return "mesh" if edit_tag is None else f"mesh_edit_{edit_tag}"


def edit_tag_of(args):
    """``<op>_<id>`` or ``script_<file stem>`` (the tags of inference/edit_scene.py's output folders), with ``_shape`` behind it under
    ``--follow_shape``; None without an edit."""
    suffix = "_shape" if getattr(args, "follow_shape", False) else ""
    if args.script is not None:
        return f"script_{Path(args.script).stem}{suffix}"
    return None if args.op is None else f"{args.op}_{args.instance}{suffix}"


def resolve_cli_edit(args, shape_of=None):
    """(edit, tag) of the parsed command line, (None, None) without an edit: the boxes of ``--bboxes`` through inference/edit_scene.py's
    ``resolve_edit`` / ``resolve_program``.  ``shape_of`` (``edit_scene.field_shapes`` of the loaded field) makes the shapes of
    ``--follow_shape`` and of script entries with ``"shape": true``."""
    tag = edit_tag_of(args)
    if tag is None:
        return None, None
    import json
    import edit_scene as es
    assert tuple(es.OPS) == EDIT_OPS
    with open(args.bboxes, "rb") as f:
        boxes = pickle.load(f)
    follow = bool(getattr(args, "follow_shape", False))
    if follow and shape_of is None:
        raise SystemExit("--follow_shape reads the shapes from the trained field: resolve the edit once the field is loaded (cli_edit_of)")
    if args.script is not None:
        with open(args.script) as f:
            return es.resolve_program(boxes, json.load(f), follow_shape=follow, shape_of=shape_of), tag
    return es.resolve_edit(boxes, args.instance, args.op, args.translate, args.rotate_deg, args.pad, shape=shape_of if follow else None), tag


def cli_edit_of(args):
    """What ``extract_mesh(edit=)`` takes for the parsed command line: the resolved edit, or under ``--follow_shape`` a callable that
    resolves it with the shapes of the loaded field (the slot table from ``render_panopli.layers_table``)."""
    import edit_scene as es
    if not (getattr(args, "follow_shape", False) or es.script_asks_for_shapes(args.script)):
        return resolve_cli_edit(args)[0]

    def late(config, scene, model, renderer):
        table = es.shape_table(config, scene, args.cached_centroids_path)
        return resolve_cli_edit(args, es.field_shapes(model, renderer, table, args.shape_grid, args.shape_grow, args.shape_alpha,
                                                      bool(getattr(config, "use_delta", False))))[0]
    return late


def relations_options(args):
    """What ``extract_mesh(relations=)`` takes for the parsed command line; None without ``--relations``."""
    if not args.relations:
        return None
    return dict(gap=args.relations_gap, up=args.up_axis, min_faces=args.relations_min_faces)


def clearance_options(args):
    """What ``extract_mesh(clearance=)`` takes for the parsed command line; None without ``--clearance``."""
    if not args.clearance:
        return None
    return dict(slack=0 if args.clearance_slack is None else args.clearance_slack)


def separation_options(args):
    """What ``extract_mesh(separation=)`` takes for the parsed command line; None without ``--separation``."""
    if not args.separation:
        return None
    return dict(max_cells=args.separation_max_cells)


class _Parser(argparse.ArgumentParser):
    """The cross-argument rules of the edit flags, checked where the arguments are parsed."""

    def parse_args(self, args=None, namespace=None):
        args = list(sys.argv[1:] if args is None else args)
        for i in range(len(args) - 1):                                # "--up_axis -z": argparse would read the value as an option
            if args[i] == "--up_axis" and args[i + 1] in rel.UP_AXES:
                args[i:i + 2] = [f"--up_axis={args[i + 1]}", None]
        a = super().parse_args([x for x in args if x is not None], namespace)
        if a.clearance_slack is not None and not a.clearance:
            self.error("--clearance_slack needs --clearance")
        if a.clearance:
            a.clearance_slack = 0 if a.clearance_slack is None else a.clearance_slack
        if a.separation_max_cells is not None and not a.separation:
            self.error("--separation_max_cells needs --separation")
        if a.separation_max_cells is not None and not a.separation_max_cells >= 0.0:
            self.error(f"--separation_max_cells must be >= 0 (got {a.separation_max_cells:g})")
        if a.script is None and (a.instance is None) != (a.op is None):
            self.error("--instance and --op come together")
        if edit_tag_of(a) is None:
            if a.follow_shape:
                raise SystemExit("--follow_shape shapes an edit: give --bboxes with --instance ID --op OP, or with --script FILE.json")
            if a.bboxes is not None:
                self.error("--bboxes needs an edit: --instance ID --op OP, or --script FILE.json")
            return a
        if a.script is not None and a.instance is not None:
            self.error("--script holds the edits: give it without --instance / --op")
        if a.bboxes is None:
            self.error("an edit needs --bboxes (bboxes.pkl of inference/fit_bboxes.py)")
        if a.save_voxel_cloud:
            raise SystemExit(VOXEL_CLOUD_WITH_EDIT)
        return a


def build_parser():
    ap = _Parser(description="Extract a labelled surface mesh (mesh.ply) from a trained checkpoint.")
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--upsample", type=int, default=2, help="sigma lattice = grid x this factor per axis")
    lv = ap.add_mutually_exclusive_group()
    lv.add_argument("--alpha_level", type=float, default=0.5,
                    help="iso level as an opacity: the surface is sigma* = -ln(1 - alpha_level) / (training step size x distance_scale), the sigma "
                         "at which one training-step sample would have this alpha.  This default is a judgement: nobody has measured it against "
                         "a real scene -- look at the mesh and set --level if it is too fat or too thin")
    lv.add_argument("--level", type=float, default=None, help="iso level as a sigma value (overrides --alpha_level)")
    ap.add_argument("--cached_centroids_path", type=str, required=False,
                    help="all_centroids.pkl of extract_train_centroids.py: instance id = nearest centroid of the vertex's class, numbered like "
                         "pred_surrogateid.  Without it: 1 + argmax of the instance head on thing classes, 0 on stuff")
    ap.add_argument("--split_instances", action="store_true", help="also write mesh_instance_<id>.ply per instance id")
    ap.add_argument("--save_voxel_cloud", action="store_true",
                    help="also write voxelcloud.pkl (the occupied voxels, class and id as for the vertices, rgb at a zero view direction, in "
                         "pointcloud.pkl's layout) for inference/fit_bboxes.py")
    ap.add_argument("--min_component", type=int, default=0, metavar="VOXELS",
                    help="drop every connected component of the inside lattice points with fewer than this many points before meshing (0 = off)")
    ap.add_argument("--keep_largest", type=int, default=None, metavar="K", help="keep only the K largest components (ties: the smaller first point)")
    ap.add_argument("--connectivity", type=str, default="kuhn", choices=["6", "kuhn", "26"],
                    help="what makes two lattice points neighbours: kuhn = the mesher's seven edge classes (14 neighbours), under which every mesh "
                         "face belongs to exactly one component")
    ap.add_argument("--split_disconnected", type=int, nargs="?", const=1, default=None, metavar="MIN_VOXELS",
                    help="give the separated pieces of one instance id ids of their own: the largest keeps the id, every other piece of at least "
                         "MIN_VOXELS lattice points (default 1) gets a fresh one; mesh_instance_<id>.ply follows the new ids (the PLY holds ids up "
                         "to 65535: raise MIN_VOXELS or --min_component on a frothy scene)")
    ap.add_argument("--relations", action="store_true",
                    help="also write relations.npz (raw tables) and relations.json (the scene graph) next to the mesh: per (class, instance) node "
                         "its extent and free area, per pair of nodes their contacts, and what stands on or beside what")
    ap.add_argument("--relations_gap", type=int, default=1, choices=list(range(rel.MAX_GAP + 1)), metavar="G",
                    help="--relations: a contact may look through up to G empty lattice points (0 .. %d; objects of a density field are "
                         "usually separated by a thin gap at the level set)" % rel.MAX_GAP)
    ap.add_argument("--up_axis", type=str, default="+z", choices=list(rel.UP_AXES), help="--relations: the scene's up direction")
    ap.add_argument("--relations_min_faces", type=int, default=4, metavar="N", help="--relations: contacts below this count name no relation")
    ap.add_argument("--clearance", action="store_true",
                    help="also write clearance.npz (raw tables) and clearance.json next to the mesh: per (class, instance) node and lattice "
                         "direction the free travel to the next node in lattice steps and as a distance, the nodes it would rest on with their "
                         "face counts, and the steps to the lattice border (DESIGN.md 6n); the nodes are those of --relations")
    ap.add_argument("--clearance_slack", type=int, default=None, choices=list(range(clr.MAX_SLACK + 1)), metavar="S",
                    help="--clearance: count the faces up to S lattice steps further away than the first contact (0 .. %d, default 0)" % clr.MAX_SLACK)
    ap.add_argument("--separation", action="store_true",
                    help="also write separation.npz (raw tables) and separation.json next to the mesh: the true distance between every two "
                         "(class, instance) nodes -- diagonal neighbours included, which the axis looks of --relations and --clearance do not "
                         "see --, in lattice steps and as a world distance with the two points (DESIGN.md 6o); the nodes are those of --relations")
    ap.add_argument("--separation_max_cells", type=float, default=None, metavar="N",
                    help="--separation: list only the pairs at most N lattice steps apart in separation.json (default: every pair)")
    ap.add_argument("--image_dim", type=int, nargs=2, default=[256, 384], help="as render_panopli.py (the scene loader wants it)")
    ap.add_argument("--bboxes", type=str, default=None, help="bboxes.pkl of inference/fit_bboxes.py: mesh the scene under an edit (with --instance / --op or --script)")
    ap.add_argument("--instance", type=int, default=None, help="instance id (a key of bboxes.pkl) the edit acts on")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--op", choices=EDIT_OPS, default=None, help="the edit; the file is mesh_edit_<op>_<id>.ply")
    which.add_argument("--script", type=str, default=None, metavar="FILE.json",
                       help="an ordered list of up to 8 edits (the format of inference/edit_scene.py --script); the file is mesh_edit_script_<stem>.ply")
    ap.add_argument("--translate", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="copy / move: translation t")
    ap.add_argument("--rotate_deg", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("RX", "RY", "RZ"),
                    help="copy / move: rotation about the box centre, R = Rz Ry Rx (degrees)")
    ap.add_argument("--pad", type=float, default=0.0, help="grow the fitted box by this much on every side")
    import edit_scene as es
    es.add_shape_arguments(ap)
    return ap


if __name__ == "__main__":
    args = build_parser().parse_args()
    cfg = load_run_config(Path(args.ckpt_path).parents[1] / "config.yaml")
    cfg.resume = args.ckpt_path
    cfg.image_dim = list(args.image_dim)
    the_edit, the_tag = cli_edit_of(args), edit_tag_of(args)
    print(extract_mesh(cfg, upsample=args.upsample, alpha_level=args.alpha_level, level=args.level,
                       cached_centroids_path=args.cached_centroids_path, split_instances=args.split_instances,
                       save_voxel_cloud=args.save_voxel_cloud, min_component=args.min_component, keep_largest=args.keep_largest,
                       connectivity=args.connectivity, split_disconnected=args.split_disconnected, edit=the_edit, edit_tag=the_tag,
                       relations=relations_options(args), **({} if clearance_options(args) is None else {"clearance": clearance_options(args)}),
                       **({} if separation_options(args) is None else {"separation": separation_options(args)}))[0])
