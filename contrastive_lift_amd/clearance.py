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
forward fill of the last non-zero index per axis, np.minimum.at and np.add.at) for machines and tests without a GPU.
"""
import json
import math

import numpy as np
import torch

from . import _lib
from .components import CC_LIMIT, _as_key, _check_backend
from .relations import MAX_KEYS, UP_AXES

MAX_SLACK = 4                    # CLIFT_CLR_MAX_SLACK
NONE = 0x7fffffff                # CLIFT_CLR_NONE: no event
DIRECTIONS = UP_AXES             # "+x", "-x", "+y", "-y", "+z", "-z": direction d = 2 a + (0 for +, 1 for -)
TABLES = ("pair", "travel", "landing", "rejected")


def _check_sizes(n_keys, slack):
    n_keys, slack = int(n_keys), int(slack)
    if not 1 <= n_keys <= MAX_KEYS:
        raise ValueError(f"n_keys must be 1 .. {MAX_KEYS} (got {n_keys})")
    if not 0 <= slack <= MAX_SLACK:
        raise ValueError(f"slack must be 0 .. {MAX_SLACK} (got {slack})")
    return n_keys, slack


def direction_index(direction):
    """"+x" .. "-z" -> d = 2 a + (0 for +, 1 for -)."""
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be one of {', '.join(DIRECTIONS)} (got {direction!r})")
    return DIRECTIONS.index(direction)


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
    key = _as_key(key)
    n0, n1, n2 = (int(x) for x in key.shape)
    if n0 * n1 * n2 >= CC_LIMIT:
        raise _lib.CliftError(f"lattice_clearance: {n0 * n1 * n2} lattice points, must be < 2^31")
    if key.numel() == 0:
        raise ValueError(f"key must have at least one point along every axis, got {tuple(key.shape)}")
    if n_keys is None:
        n_keys = max(int(key.max()), 0) + 1
    n_keys, slack = _check_sizes(n_keys, slack)
    if _check_backend(backend) == "host":
        return _tables_host(key, n_keys, slack)
    if not key.is_cuda:
        raise _lib.CliftError(f"lattice_clearance: backend='device' wants the key on the GPU, got {key.device}")
    dev = key.device
    out = dict(pair=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), travel=torch.empty((n_keys, 6), dtype=torch.int32, device=dev),
               landing=torch.empty((n_keys, n_keys, 6), dtype=torch.int32, device=dev), rejected=torch.empty(1, dtype=torch.int32, device=dev))
    _lib.call("clift_lattice_clearance", _lib.ptr(key), n0, n1, n2, n_keys, slack, _lib.ptr(out["pair"]), _lib.ptr(out["travel"]),
              _lib.ptr(out["landing"]), _lib.ptr(out["rejected"]), _lib.stream())
    return out


@torch.no_grad()
def lattice_clearance(key, n_keys=None, slack=0, backend="device"):
    """``clearance_tables`` of a key lattice (n0, n1, n2) bool or integer; raises CliftError when a point's key lies outside [0, n_keys)."""
    out = clearance_tables(key, n_keys, slack, backend)
    rejected = int(out["rejected"][0])
    if rejected > 0:
        raise _lib.CliftError(f"lattice_clearance: {rejected} lattice points carry a key outside [0, {out['travel'].shape[0]})")
    return out


def _host_ticks(ticks):
    ticks = [np.asarray(t.cpu() if torch.is_tensor(t) else t, np.float64) for t in ticks]
    step = np.asarray([(t[-1] - t[0]) / (t.shape[0] - 1) if t.shape[0] > 1 else 0.0 for t in ticks])
    return ticks, step


def offset_of(steps, ticks, direction):
    """The world translation (3,) fp64 of ``steps`` lattice steps along ``direction`` ("+x" .. "-z") on a lattice with the three uniform
    coordinate arrays ``ticks``: steps times the tick spacing of that axis, signed."""
    d = direction_index(direction)
    _, step = _host_ticks(ticks)
    out = np.zeros(3, np.float64)
    out[d // 2] = (1.0 if d % 2 == 0 else -1.0) * int(steps) * step[d // 2]
    return out


def index_box(key, n_keys):
    """(n_keys, 6) int64 = min_0 min_1 min_2 max_0 max_1 max_2 of the indices of every key's points (``ibox`` of ``lattice_relations``:
    min_a = n_a, max_a = -1 for a key nobody carries), in numpy on the host."""
    k = (key.cpu().numpy() if torch.is_tensor(key) else np.asarray(key)).astype(np.int64)
    box = np.empty((n_keys, 6), np.int64)
    box[:, :3], box[:, 3:] = np.asarray(k.shape), -1
    valid = (k >= 0) & (k < n_keys)
    at = np.nonzero(valid)
    for a in range(3):
        np.minimum.at(box[:, a], k[valid], at[a])
        np.maximum.at(box[:, 3 + a], k[valid], at[a])
    return box


class Clearance:
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
        host = {k: (tables[k].cpu().numpy() if torch.is_tensor(tables[k]) else np.asarray(tables[k])).astype(np.int64) for k in ("travel", "landing")}
        travel, landing = host["travel"], host["landing"]
        K = len(nodes)
        if travel.shape[0] != K + 1:
            raise ValueError(f"the tables hold {travel.shape[0]} keys, the node list wants {K + 1}")
        ticks, step = _host_ticks(ticks)
        shape = [t.shape[0] for t in ticks]
        box = None
        if relations is not None:
            box = (relations["ibox"].cpu().numpy() if torch.is_tensor(relations["ibox"]) else np.asarray(relations["ibox"])).astype(np.int64)
        elif key is not None:
            box = index_box(key, K + 1)
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

    def to_json(self, **kw):
        return json.dumps(self.to_dict(), **kw)

    def __eq__(self, other):
        return isinstance(other, Clearance) and self.to_dict() == other.to_dict()


def default_level(renderer, alpha_level):
    """The sigma at which ONE sample of a training step would have opacity ``alpha_level``: alpha = 1 - exp(-sigma step distance_scale).
    ``renderer`` comes from ``load_for_inference``, which halves the step ratio: the training step is twice its step."""
    if not 0.0 < alpha_level < 1.0:
        raise ValueError(f"--alpha_level must lie in (0, 1) (got {alpha_level})")
    train_step = 2.0 * renderer.step_size_host
    return -math.log(1.0 - alpha_level) / (train_step * float(renderer.distance_scale))


def lattice_points(ticks):
    """(n0 n1 n2, 3) fp32 world points of the lattice with the coordinate arrays ``ticks``, x-major."""
    return torch.stack(torch.meshgrid(*[t.float() for t in ticks], indexing="ij"), -1).reshape(-1, 3).contiguous()


@torch.no_grad()
def settle_key(model, renderer, edit, upsample=1, level=None):
    """The key lattice ``settle_offset`` works on -> (key (n0, n1, n2) int32, ticks, n_moved): 2 where the edited scene holds density that
    the LAST edit of ``edit`` placed, 1 on all other density, 0 below the level."""
    from . import edit as ed
    program = ed.as_program(edit)
    last = program[len(program) - 1]
    if last.mode not in (ed.DUPLICATE, ed.MANIPULATE):
        raise ValueError(f"settle_offset: the last edit must be a copy or a move (it is a {last.name})")
    level = default_level(renderer, 0.5) if level is None else float(level)
    sigma = renderer.get_dense_sigma(model, int(upsample), edit=program)
    ticks = renderer.lattice_ticks(sigma.shape)
    state = ed.EditProgram([last]).apply_to_points(lattice_points(ticks), backend="device")[2]
    moved = ((state & ed.STATE_REMAPS) >= 1).view(sigma.shape)
    inside = sigma >= torch.tensor(level, dtype=torch.float32, device=sigma.device)
    key = torch.where(inside, torch.where(moved, 2, 1), 0).int()
    return key, ticks, int((key == 2).sum())


@torch.no_grad()
def settle_offset(model, renderer, edit, direction="-z", upsample=1, level=None, slack=0):
    """How far to drop the object that the LAST edit of ``edit`` (an ``Edit`` or an ``EditProgram``; a copy or a move, else ValueError)
    places, along ``direction``, until it touches the rest of the edited scene: the density lattice of the edited scene
    (``get_dense_sigma(edit=)`` at ``upsample``), its points that the last edit remapped (``apply_to_points`` of that edit alone, with its
    shape) as key 2, all other density as key 1, and ``lattice_clearance`` of the three keys.  ``level=None``: ``default_level`` of alpha
    0.5.  -> dict(steps = travel[2][d], offset (3,) fp64 world translation, faces = landing[2][1][d], found, n_moved, direction, spacing);
    ``found`` is False, steps None and the offset zero when nothing stands in the way.  No density of the moved object on the lattice
    is a CliftError."""
    d = direction_index(direction)
    n_keys, slack = _check_sizes(3, slack)
    key, ticks, n_moved = settle_key(model, renderer, edit, upsample, level)
    if n_moved == 0:
        raise _lib.CliftError("settle_offset: no lattice point at or above the level holds content that the last edit placed (the moved set is "
                              "empty): is the destination outside the scene box, the level too high, or the lattice too coarse?")
    tables = lattice_clearance(key, n_keys, slack)
    steps, faces = int(tables["travel"][2, d]), int(tables["landing"][2, 1, d])
    found = steps != NONE
    _, step = _host_ticks(ticks)
    return dict(steps=steps if found else None, offset=offset_of(steps, ticks, direction) if found else np.zeros(3, np.float64),
                faces=faces, found=found, n_moved=n_moved, direction=direction, spacing=float(abs(step[d // 2])))
