"""Amodal instance layers: the slot table that numbers the instances of a scene once, and what a frame's layers say about
every instance -- its amodal and visible pixels, how much of it is hidden, which one lies in front along a ray.

A layer array is ``(N, K + 1, 4)`` fp32 from ``engine.layers_forward`` / ``inference.render_rays_layers``: per ray and per column the row
``[A, V, Z, zf]`` -- the opacity of that column rendered alone, the weight the whole scene gives it, its un-normalised expected distance
when alone, the distance of its first listed sample.  Columns ``0 .. K - 1`` are the table's instance slots, column ``K`` is the rest
(stuff, unassigned, out of range).

Layers of an EDITED scene (``engine.edit_layers_forward``) have ``c`` more instance columns, one per copy of the edit program:
``SlotTable.for_program`` numbers them ``K .. K + c - 1`` behind the table's own slots, ``retarget`` sends a listed sample that a copy
brought to that copy's column, and ``compare`` says per slot what an edit hid, revealed or removed.

COLOUR layers (``colour=True`` on either pass) are ``(N, K + 1, 4)`` fp32 rows ``[R, G, B, A]`` over the same columns: the
premultiplied colour of every column rendered alone, without a background; ``unpremultiply`` and ``over`` turn them into what an image wants.
"""
import numpy as np
import torch

from . import edit as _edit

MAX_SLOTS = 255          # clift_ray_layers keeps K + 1 <= 256 columns in the registers of one wave


class SlotTable:
    """The instance slots of a scene: a FIXED numbering of (thing class, centroid index) pairs.

    ``inference.assign_cluster_labels`` numbers the instances of a set of frames by the classes that happen to be present in it (every class
    is offset by the labels seen before it), so an id means something only together with that set.  A slot table numbers every centroid of
    every thing class once, in ascending class order, whatever a frame contains: slot ``s`` is centroid ``slot_index[s]`` of class
    ``slot_class[s]`` in every frame and every chunk, which is what lets layers of different frames be compared.  The two numberings differ
    as soon as a class with centroids is absent from the frames.

    Attributes: ``K`` slots; ``num_classes``; ``cls_slots`` (num_classes, 2) int32, the (first slot, count) of every class, count 0 for a
    stuff class or a class without centroids; ``slot_class`` (K) and ``slot_index`` (K) int64; ``centroids`` (K, E) fp32 or None;
    ``mode`` 0 (nearest centroid) or 1 (the instance outputs are slot scores); ``E`` the feature width the table expects.

    A table made by ``for_program`` has ``c`` copy slots behind those: ``K`` counts them, ``K_base`` does not, ``copy_edit`` (c,) int64 holds the
    0-based program position of the edit every copy slot belongs to and ``base`` is the table it was made from.  ``cls_slots`` and
    ``centroids`` stay the base table's: no sample is ASSIGNED to a copy slot, it is sent there (``retarget``)."""

    def __init__(self, num_classes, cls_slots, slot_class, slot_index, centroids, mode, E, copy_edit=(), base=None):
        self.num_classes = int(num_classes)
        self.cls_slots = np.ascontiguousarray(cls_slots, dtype=np.int32).reshape(self.num_classes, 2)
        self.slot_class = np.asarray(slot_class, dtype=np.int64).reshape(-1)
        self.slot_index = np.asarray(slot_index, dtype=np.int64).reshape(-1)
        self.K = int(self.slot_class.shape[0])
        self.copy_edit = np.asarray(copy_edit, dtype=np.int64).reshape(-1)
        self.K_base, self.base = self.K - int(self.copy_edit.shape[0]), base
        self.mode, self.E = int(mode), int(E)
        if self.K > MAX_SLOTS:
            raise ValueError(f"SlotTable: {self.K} slots, the layer kernel holds at most {MAX_SLOTS}")
        self.centroids = None if centroids is None else np.ascontiguousarray(centroids, dtype=np.float32).reshape(self.K_base, self.E)
        self._dev = {}

    @classmethod
    def from_centroids(cls, centroids, thing_classes, num_classes):
        """From the dict of an ``all_centroids.pkl`` (class -> (k, E) array): the thing classes below ``num_classes`` that have at least one
        centroid get consecutive slot ranges in ascending class order."""
        num_classes = int(num_classes)
        cls_slots = np.zeros((num_classes, 2), np.int32)
        slot_class, slot_index, rows, E = [], [], [], None
        for c in sorted(set(int(c) for c in thing_classes)):
            if not 0 <= c < num_classes or c not in centroids:
                continue
            cent = np.asarray(centroids[c], dtype=np.float32)
            if cent.size == 0:
                continue
            cent = cent.reshape(cent.shape[0], -1)
            if E is None:
                E = cent.shape[1]
            elif cent.shape[1] != E:
                raise ValueError(f"SlotTable: class {c} has centroids of width {cent.shape[1]}, earlier classes {E}")
            cls_slots[c] = (len(slot_class), cent.shape[0])
            slot_class += [c] * cent.shape[0]
            slot_index += list(range(cent.shape[0]))
            rows.append(cent)
        E = 1 if E is None else E
        return cls(num_classes, cls_slots, slot_class, slot_index, np.concatenate(rows, 0) if rows else np.zeros((0, E), np.float32), 0, E)

    @classmethod
    def from_scores(cls, thing_classes, num_classes, E):
        """For models whose instance outputs are slot scores (linear assignment): every thing class gets the range [0, E), a sample's slot is the
        first maximum of its scores.  The slots are shared by the classes: ``slot_class`` is -1."""
        num_classes, E = int(num_classes), int(E)
        cls_slots = np.zeros((num_classes, 2), np.int32)
        for c in set(int(c) for c in thing_classes):
            if 0 <= c < num_classes:
                cls_slots[c] = (0, E)
        return cls(num_classes, cls_slots, [-1] * E, list(range(E)), None, 1, E)

    def for_program(self, program):
        """The table of the layers of the scene ``program`` describes (an ``edit.EditProgram``, or what ``edit.as_program`` takes): this
        table's K slots, then one slot per DUPLICATE edit in program order -- slot ``K + j`` belongs to the j-th copy, its ``slot_class`` is -1,
        its ``slot_index`` and ``copy_edit[j]`` that edit's 0-based position in the program.  A program without a copy gives a table of
        the same K slots.  ``K + c > 255`` is refused."""
        if self.copy_edit.shape[0]:
            raise ValueError("SlotTable.for_program: this table already holds copy slots (take the table it was made from, .base)")
        copies = _edit.as_program(program).copies()
        K, c = self.K, len(copies)
        if K + c > MAX_SLOTS:
            raise ValueError(f"SlotTable.for_program: {K} slots and {c} copies, the layer kernel holds at most {MAX_SLOTS} columns beside the rest")
        return SlotTable(self.num_classes, self.cls_slots, np.concatenate([self.slot_class, np.full(c, -1, np.int64)]),
                         np.concatenate([self.slot_index, np.asarray(copies, np.int64)]), self.centroids, self.mode, self.E, copy_edit=copies,
                         base=self)

    def origin_columns(self):
        """int32 lookup from a sample's origin (the 1-based program position of the copy its content came through) to that copy's column;
        entry 0 and the entries of edits that are no copies are -1 -- an origin names a copy, so a sample with a slot never reads them."""
        lut = np.full(int(self.copy_edit.max()) + 2 if self.copy_edit.shape[0] else 1, -1, np.int32)
        for j, i in enumerate(self.copy_edit):
            lut[int(i) + 1] = self.K_base + j
        return lut

    def on(self, device):
        """(cls_slots, centroids or None) as tensors on ``device``, made once per device."""
        key = str(device)
        if key not in self._dev:
            cent = None if self.centroids is None or self.K_base == 0 else torch.from_numpy(self.centroids).to(device)
            self._dev[key] = (torch.from_numpy(self.cls_slots).to(device), cent)
        return self._dev[key]


def _check_layers(layers, table=None):
    if layers.dim() != 3 or layers.shape[2] != 4:
        raise ValueError(f"layers must be (N, K + 1, 4), got {tuple(layers.shape)}")
    if table is not None and layers.shape[1] != table.K + 1:
        raise ValueError(f"layers has {layers.shape[1]} columns, the table {table.K} slots (+ the rest column)")


@torch.no_grad()
def summarise(layers, table, level=0.5):
    """Per slot of ``table`` over the rays of ``layers`` (N, K + 1, 4) (the rest column is left out), tensors of length K on the layers'
    device: ``amodal_pixels`` = #(A > level), ``visible_pixels`` = #(V > level), ``occlusion`` = 1 - sum V / sum A (0 where sum A = 0),
    ``mean_distance`` = the mean of Z / A over the amodal pixels (0 where there is none); with ``slot_class`` and ``slot_index``."""
    _check_layers(layers, table)
    K = table.K
    A, V, Z = (layers[:, :K, i].double() for i in range(3))
    amodal = A > level
    sum_a, sum_v = A.sum(0), V.sum(0)
    occ = torch.where(sum_a > 0, 1.0 - sum_v / torch.where(sum_a > 0, sum_a, torch.ones_like(sum_a)), torch.zeros_like(sum_a))
    dist = torch.where(amodal, Z / torch.where(amodal, A, torch.ones_like(A)), torch.zeros_like(A)).sum(0)
    n_am = amodal.sum(0)
    return dict(amodal_pixels=n_am, visible_pixels=(V > level).sum(0), occlusion=occ,
                mean_distance=torch.where(n_am > 0, dist / n_am.clamp(min=1), torch.zeros_like(dist)),
                slot_class=torch.from_numpy(table.slot_class).to(layers.device), slot_index=torch.from_numpy(table.slot_index).to(layers.device))


@torch.no_grad()
def front_order(layers, level=0.5):
    """Per ray the slots (instance columns; the rest column is left out) with A > level, nearest first by ``zf``, a tie by the lower slot:
    (order (N, K) int64, padded with -1 behind the ray's last slot; count (N) int64)."""
    _check_layers(layers)
    K = layers.shape[1] - 1
    A, zf = layers[:, :K, 0], layers[:, :K, 3]
    on = A > level
    key = torch.where(on, zf, torch.full_like(zf, float("inf")))
    idx = torch.sort(key, dim=1, stable=True)[1]
    order = torch.where(torch.gather(on, 1, idx), idx, torch.full_like(idx, -1))
    return order, on.sum(1)


def _check_colour(colour):
    if colour.shape[-1] != 4:
        raise ValueError(f"a colour layer array ends in [R, G, B, A], got {tuple(colour.shape)}")


@torch.no_grad()
def unpremultiply(colour, eps=1e-6):
    """Colour layers (..., 4) rows [R, G, B, A] with premultiplied colours (``engine.layers_forward(colour=True)``) -> the same
    shape with RGB / A where A > ``eps`` and 0 elsewhere; A is kept.  What an RGBA image file wants."""
    colour = torch.as_tensor(colour)
    _check_colour(colour)
    A = colour[..., 3:4]
    on = A > eps
    rgb = torch.where(on, colour[..., :3] / torch.where(on, A, torch.ones_like(A)), torch.zeros_like(colour[..., :3]))
    return torch.cat([rgb, A], -1)


@torch.no_grad()
def over(colour, background):
    """Premultiplied colour layers (..., 4) over ``background`` (a scalar, (3,) or anything that broadcasts against (..., 3)) -> (..., 3):
    RGB + (1 - A) background."""
    colour = torch.as_tensor(colour)
    _check_colour(colour)
    background = torch.as_tensor(background, dtype=colour.dtype, device=colour.device)
    return colour[..., :3] + (1.0 - colour[..., 3:4]) * background


@torch.no_grad()
def retarget(base_slots, origin, table):
    """The column of every listed sample of an edited scene: ``base_slots`` (M,) int32 of clift_sample_slots under the BASE table, ``origin``
    (M,) uint8 of clift_edit_list_active_origin, ``table`` the table of ``for_program``.  A sample with origin i > 0 and a base slot in [0, K)
    goes to the column of edit i; a sample whose base slot is -1 (stuff, unassigned) stays in the rest column whatever its origin; a sample
    with origin 0 -- a moved object too -- keeps its slot.  One elementwise step; -> (M,) int32."""
    base_slots = torch.as_tensor(base_slots)
    origin = torch.as_tensor(origin).to(base_slots.device)
    lut = torch.from_numpy(table.origin_columns()).to(base_slots.device)
    copied = (origin > 0) & (base_slots >= 0) & (base_slots < table.K_base)
    return torch.where(copied, lut[origin.long().clamp(max=lut.shape[0] - 1)], base_slots.to(torch.int32)).to(torch.int32)


@torch.no_grad()
def compare(before, after, table_before, table_after, level=0.5):
    """What an edit did to every instance, from the layers of the SAME rays before (N, K + 1, 4) and after (N, K' + 1, 4) it, K' = K + c with
    the copy columns of ``table_after`` behind the K slots both tables share.  Tensors of length K' on the layers' device:
    ``amodal_pixels_before`` / ``_after`` = #(A > level), ``visible_pixels_before`` / ``_after`` = #(V > level),
    ``newly_hidden`` = #(V_before > level and V_after <= level and A_after > level) -- still there, no longer seen --, ``revealed`` =
    #(V_after > level and V_before <= level and A_before > level), ``gone`` = #(A_before > level and A_after <= level); with ``slot_class``
    and ``slot_index`` of ``table_after``.  A copy column has zeros on the before side."""
    _check_layers(before, table_before)
    _check_layers(after, table_after)
    K, K2 = table_before.K, table_after.K
    if before.shape[0] != after.shape[0]:
        raise ValueError(f"compare: {before.shape[0]} rays before, {after.shape[0]} after (the rays must be the same)")
    if K2 < K or not (np.array_equal(table_after.slot_class[:K], table_before.slot_class)
                      and np.array_equal(table_after.slot_index[:K], table_before.slot_index)):
        raise ValueError("compare: the table after the edit must begin with the slots of the table before it")
    Ab = torch.zeros((after.shape[0], K2), dtype=after.dtype, device=after.device)
    Vb = torch.zeros_like(Ab)
    Ab[:, :K], Vb[:, :K] = before[:, :K, 0], before[:, :K, 1]
    Aa, Va = after[:, :K2, 0], after[:, :K2, 1]
    return dict(amodal_pixels_before=(Ab > level).sum(0), amodal_pixels_after=(Aa > level).sum(0),
                visible_pixels_before=(Vb > level).sum(0), visible_pixels_after=(Va > level).sum(0),
                newly_hidden=((Vb > level) & (Va <= level) & (Aa > level)).sum(0),
                revealed=((Va > level) & (Vb <= level) & (Ab > level)).sum(0),
                gone=((Ab > level) & (Aa <= level)).sum(0),
                slot_class=torch.from_numpy(table_after.slot_class).to(after.device),
                slot_index=torch.from_numpy(table_after.slot_index).to(after.device))
