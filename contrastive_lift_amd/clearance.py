"""Clearance of a keyed 3-D lattice (csrc/clearance.hip: clift_lattice_clearance): how far every instance can travel along
the lattice axes before it meets another one, on how many faces it then rests, and the translation that settles a moved or copied object.

    tables = lattice_clearance(key, n_keys=len(nodes) + 1, slack=0)      # pair, travel, landing, rejected: integer tables
    summary = Clearance.from_tables(tables, nodes, ticks, key=key)       # fp64 on the host; summary.to_json()
    drop = settle_offset(model, renderer, edit.move(box, t, shape=sh))   # steps, offset (3,), faces, found, ...

The tables (the rules in full: include/clift.h).  Key 0 is background, valid keys are 0 .. n_keys - 1.  Directions are numbered d = 2a for +a
and d = 2a + 1 for -a (``DIRECTIONS``).  In a column along axis a, two points at i < j with valid non-zero keys u != v and nothing but
background between them are an event of run g = j - i - 1 for (u, v, 2a) and for (v, u, 2a + 1); equal keys are no event, a key outside
[0, n_keys) is counted in ``rejected`` and ends the look from both sides, the lattice border gives no event.  ``pair[u][v][d]`` is the
smallest run (``NONE`` where there is no event), ``travel[u][d]`` = min_v pair[u][v][d] the steps u can be shifted along d before its first
point meets another key, ``landing[u][v][d]`` the number of events with g <= travel[u][d] + ``slack``: the faces on which u then rests on v.

``backend="device"`` is one call (two launches of one kernel body); ``backend="host"`` gives the same integers in vectorised numpy (a
forward fill of the last non-zero index per axis, np.minimum.at and np.add.at) for machines and tests without a GPU.  What the lattice
modules share is in ``lattice``.
"""
import numpy as np
import torch

from . import _lib, lattice
from .lattice import DIRECTIONS, direction_index
from .lattice import lattice_points, settle_key   # noqa: F401  (still read as clearance.settle_key, ...)

MAX_SLACK = 4                    # CLIFT_CLR_MAX_SLACK
NONE = 0x7fffffff                # CLIFT_CLR_NONE: no event
TABLES = ("pair", "travel", "landing", "rejected")


def _check_slack(slack):
    slack = int(slack)
    if not 0 <= slack <= MAX_SLACK:
        raise ValueError(f"slack must be 0 .. {MAX_SLACK} (got {slack})")
    return slack


def _tables_host(key, n_keys, slack):
    k = key.cpu().numpy().astype(np.int64)
    valid = (k >= 0) & (k < n_keys)
    kv = np.where(valid, k, -1)                                            # -1: rejected
    pair = np.full((n_keys, n_keys, 6), NONE, np.int64)
    events = []
    for a in range(3):
        m = np.moveaxis(kv, a, 2)                                          # the axis of the look last
        n = m.shape[2]
        idx = np.where(m != 0, np.arange(n), -1)                           # a rejected point is an end of a look too
        pred = np.full(m.shape, -1, np.int64)
        pred[:, :, 1:] = np.maximum.accumulate(idx, axis=2)[:, :, :-1]     # the last non-zero point strictly below
        pk = np.take_along_axis(m, np.maximum(pred, 0), 2)
        hit = (m > 0) & (pred >= 0) & (pk > 0) & (pk != m)
        u, v, g = pk[hit], m[hit], (np.arange(n) - pred - 1)[hit]
        np.minimum.at(pair[:, :, 2 * a], (u, v), g)
        np.minimum.at(pair[:, :, 2 * a + 1], (v, u), g)
        events.append((u, v, g))
    travel = pair.min(axis=1)
    landing = np.zeros((n_keys, n_keys, 6), np.int64)
    for a, (u, v, g) in enumerate(events):
        up, down = g <= travel[u, 2 * a] + slack, g <= travel[v, 2 * a + 1] + slack
        np.add.at(landing[:, :, 2 * a], (u[up], v[up]), 1)
        np.add.at(landing[:, :, 2 * a + 1], (v[down], u[down]), 1)
    out = dict(pair=pair.astype(np.int32), travel=travel.astype(np.int32), landing=landing.astype(np.int32),
               rejected=np.asarray([int((~valid).sum())], np.int32))
    return {name: torch.from_numpy(v).to(key.device) for name, v in out.items()}


@torch.no_grad()
def clearance_tables(key, n_keys=None, slack=0, backend="device"):
    """The tables of clift_lattice_clearance as a dict of int32 tensors on key's device -- pair and landing (n_keys, n_keys, 6), travel
    (n_keys, 6), rejected (1) -- whatever ``rejected`` says (``lattice_clearance`` raises on it).  ``n_keys=None``: max(key) + 1, one read
    of the lattice's maximum."""
    key, n_keys = lattice.prepare(key, n_keys, "lattice_clearance")
    slack = _check_slack(slack)
    if lattice.check_backend(backend) == "host":
        return _tables_host(key, n_keys, slack)
    lattice.require_device(key, "lattice_clearance")
    dev, (n0, n1, n2) = key.device, key.shape
    out = dict(pair=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), travel=torch.empty((n_keys, 6), dtype=torch.int32, device=dev),
               landing=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), rejected=torch.empty(1, dtype=torch.int32, device=dev))
    _lib.call("clift_lattice_clearance", _lib.ptr(key), n0, n1, n2, n_keys, slack, _lib.ptr(out["pair"]), _lib.ptr(out["travel"]),
              _lib.ptr(out["landing"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


@torch.no_grad()
def lattice_clearance(key, n_keys=None, slack=0, backend="device"):
    """``clearance_tables`` of a key lattice (n0, n1, n2) bool or integer; raises CliftError when a point's key lies outside [0, n_keys)."""
    out = clearance_tables(key, n_keys, slack, backend)
    lattice.raise_on_rejected(out, out["travel"].shape[0], "lattice_clearance")
    return out


def offset_of(steps, ticks, direction):
    """The world translation (3,) fp64 of ``steps`` lattice steps along ``direction`` ("+x" .. "-z") on a lattice with the three uniform
    coordinate arrays ``ticks``: steps times the tick spacing of that axis, signed."""
    d = direction_index(direction)
    _, step = lattice.host_ticks(ticks)
    out = np.zeros(3, np.float64)
    out[d // 2] = (1.0 if d % 2 == 0 else -1.0) * int(steps) * step[d // 2]
    return out


class Clearance(lattice.Summary):
    """The summary of ``Clearance.from_tables``: ``nodes``, one dict per key 1..K with, per direction, ``steps`` (None: nothing stands in the
    way), ``distance``, ``onto`` and ``border_steps``."""

    def __init__(self, slack, nodes):
        self.slack, self.nodes = slack, nodes

    @classmethod
    def from_tables(cls, tables, nodes, ticks, key=None, relations=None, slack=0):
        """``tables``: the tables of ``lattice_clearance`` with n_keys = len(nodes) + 1 (``slack``: what they were made with, recorded);
        ``nodes``: the (class, instance) pairs of ``relations.node_keys``; ``ticks``: the three uniform coordinate arrays of the lattice
        (``renderer.lattice_ticks``).  Everything in fp64 on the host.

        Per node and direction: ``steps`` = travel, ``distance`` = steps x the tick spacing of that axis, ``onto`` = the nodes v with
        landing[u][v][d] > 0 and their face counts, ``border_steps`` = the lattice steps from the node's index box to the lattice border
        along d.  The index box is ``relations["ibox"]`` when a dict of ``lattice_relations`` is passed, else it is computed from the
        ``key`` lattice; without either border_steps is None."""
        host = lattice.to_host(tables, ("travel", "landing"), np.int64)
        travel, landing = host["travel"], host["landing"]
        K = lattice.node_count(travel, nodes)
        ticks, step = lattice.host_ticks(ticks)
        shape = [t.shape[0] for t in ticks]
        box = None
        if relations is not None:
            box = lattice.to_host(relations, ("ibox",), np.int64)["ibox"]
        elif key is not None:
            box = lattice.index_box(key, K + 1)
        out = []
        for k in range(1, K + 1):
            node = dict(key=k, semantic=int(nodes[k - 1][0]), instance=int(nodes[k - 1][1]), directions={})
            for d, name in enumerate(DIRECTIONS):
                a, found = d // 2, travel[k, d] != NONE
                border = None
                if box is not None and box[k, 3 + a] >= 0:
                    border = int(shape[a] - 1 - box[k, 3 + a] if d % 2 == 0 else box[k, a])
                node["directions"][name] = dict(steps=int(travel[k, d]) if found else None,
                                                distance=float(travel[k, d] * abs(step[a])) if found else None,
                                                onto=[dict(key=int(v), faces=int(landing[k, v, d])) for v in np.nonzero(landing[k, :, d])[0]],
                                                border_steps=border)
            out.append(node)
        return cls(int(slack), out)

    def to_dict(self):
        return dict(slack=self.slack, directions=list(DIRECTIONS), nodes=self.nodes)


@torch.no_grad()
def settle_offset(model, renderer, edit, direction="-z", upsample=1, level=None, slack=0):
    """How far to drop the object that the LAST edit of ``edit`` (an ``Edit`` or an ``EditProgram``; a copy or a move, else ValueError)
    places, along ``direction``, until it touches the rest of the edited scene: the density lattice of the edited scene
    (``get_dense_sigma(edit=)`` at ``upsample``), its points that the last edit remapped (``apply_to_points`` of that edit alone, with its
    shape) as key 2, all other density as key 1 (``lattice.settle_key``), and ``lattice_clearance`` of the three keys.  ``level=None``:
    ``lattice.default_level`` of alpha 0.5.  -> dict(steps = travel[2][d], offset (3,) fp64 world translation, faces = landing[2][1][d], found, n_moved, direction, spacing);
    ``found`` is False, steps None and the offset zero when nothing stands in the way.  No density of the moved object on the lattice
    is a CliftError."""
    d = direction_index(direction)
    slack = _check_slack(slack)
    key, ticks, n_moved = lattice.settle_key(model, renderer, edit, upsample, level)
    if n_moved == 0:
        lattice.refuse_empty_moved("settle_offset")
    tables = lattice_clearance(key, 3, slack)
    steps, faces = int(tables["travel"][2, d]), int(tables["landing"][2, 1, d])
    found = steps != NONE
    _, step = lattice.host_ticks(ticks)
    return dict(steps=steps if found else None, offset=offset_of(steps, ticks, direction) if found else np.zeros(3, np.float64),
                faces=faces, found=found, n_moved=n_moved, direction=direction, spacing=float(abs(step[d // 2])))
