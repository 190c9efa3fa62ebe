"""What the modules on a keyed 3-D lattice share: ``relations``, ``clearance``, ``distance``, ``placement`` and ``components``
all take a lattice (n0, n1, n2) of int32 keys -- key 0 is background, valid keys are 0 .. n_keys - 1, a ``rejected`` table counts the others --
with ``backend="device"`` (the kernel) or ``"host"`` (numpy), and build their summaries in fp64 from the lattice ticks.  Here are the limits,
the prologue of their entry points, the small host helpers of their summaries and the key lattices of an edited scene.  This module imports
none of the five.
"""
import json
import math

import numpy as np
import torch

from . import _lib

CC_LIMIT = 2 ** 31               # CLIFT_ISO_LIMIT: a lattice holds fewer points
MAX_KEYS = 1024                  # CLIFT_REL_MAX_KEYS
MAX_DIM = 16384                  # CLIFT_DT_MAX_DIM: distance and placement
NONE_WORD = 0x7fffffffffffffff   # CLIFT_DT_NONE, CLIFT_PM_NONE: a packed word (dist2 << 31) | lin where there is none
INDEX_MASK = 0x7fffffff          # the lin field of a packed word
BACKENDS = ("device", "host")
DIRECTIONS = ("+x", "-x", "+y", "-y", "+z", "-z")                          # direction d = 2 a + (0 for +, 1 for -)


def check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend must be 'device' or 'host' (got {backend!r})")
    return backend


def direction_index(direction):
    """"+x" .. "-z" -> d = 2 a + (0 for +, 1 for -)."""
    if direction not in DIRECTIONS:
        raise ValueError(f"direction must be one of {', '.join(DIRECTIONS)} (got {direction!r})")
    return DIRECTIONS.index(direction)


def as_key(key):
    """-> (int32 contiguous tensor (n0, n1, n2), on the caller's device)."""
    if not torch.is_tensor(key):
        key = torch.from_numpy(np.ascontiguousarray(key))
    if key.dim() != 3:
        raise ValueError(f"key must be (n0, n1, n2), got {tuple(key.shape)}")
    if key.dtype.is_floating_point or key.dtype.is_complex:
        raise ValueError(f"key must be bool or integer, got {key.dtype}")
    return key.to(torch.int32).contiguous()


def as_lattice(key, what):
    """``as_key`` of a lattice with fewer than 2^31 points; ``what`` names the caller in the message."""
    key = as_key(key)
    n0, n1, n2 = (int(x) for x in key.shape)
    if n0 * n1 * n2 >= CC_LIMIT:
        raise _lib.CliftError(f"{what}: {n0 * n1 * n2} lattice points, must be < 2^31")
    return key


def prepare(key, n_keys, what, max_dim=None):
    """The prologue of an entry point -> (key as ``as_lattice`` gives it, n_keys as an int).  A lattice without a point and, with
    ``max_dim``, a dimension above it are ValueErrors; ``n_keys=None`` is max(key) + 1, one read of the lattice's maximum."""
    key = as_lattice(key, what)
    if key.numel() == 0:
        raise ValueError(f"key must have at least one point along every axis, got {tuple(key.shape)}")
    if max_dim is not None and max(key.shape) > max_dim:
        raise ValueError(f"every lattice dimension must be 1 .. {max_dim} (got {' x '.join(map(str, key.shape))})")
    if n_keys is None:
        n_keys = max(int(key.max()), 0) + 1
    n_keys = int(n_keys)
    if not 1 <= n_keys <= MAX_KEYS:
        raise ValueError(f"n_keys must be 1 .. {MAX_KEYS} (got {n_keys})")
    return key, n_keys


def require_device(key, what):
    if not key.is_cuda:
        raise _lib.CliftError(f"{what}: backend='device' wants the key on the GPU, got {key.device}")


def raise_on_rejected(out, n_keys, what):
    rejected = int(out["rejected"][0])
    if rejected > 0:
        raise _lib.CliftError(f"{what}: {rejected} lattice points carry a key outside [0, {n_keys})")


def key_table(sites, n_keys):
    """A choice of keys (the sites of ``distance``, the solid keys of ``placement``) -> (n_keys,) numpy bool.  None: every key >= 1; an int:
    that key; an iterable of keys; a bool array of length n_keys."""
    n_keys = int(n_keys)
    table = np.zeros(n_keys, bool)
    if sites is None:
        table[1:] = True
        return table
    if torch.is_tensor(sites):
        sites = sites.cpu().numpy()
    if isinstance(sites, np.ndarray) and sites.dtype == np.bool_:
        if sites.shape != (n_keys,):
            raise ValueError(f"a bool site table holds n_keys = {n_keys} entries, got shape {tuple(sites.shape)}")
        return sites.copy()
    keys = [sites] if isinstance(sites, (int, np.integer)) else list(sites)
    for k in keys:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"sites is None, a key, an iterable of keys or a bool array of length n_keys (got an entry {k!r})")
        if not 0 <= int(k) < n_keys:
            raise ValueError(f"site key {int(k)} lies outside [0, {n_keys})")
        table[int(k)] = True
    return table


# ----------------------------------------------------------------------------- the host side of the summaries
def host_ticks(ticks):
    """The three uniform coordinate arrays of a lattice -> (the arrays in fp64 on the host, the signed tick spacing per axis (3,))."""
    ticks = [np.asarray(t.cpu() if torch.is_tensor(t) else t, np.float64) for t in ticks]
    step = np.asarray([(t[-1] - t[0]) / (t.shape[0] - 1) if t.shape[0] > 1 else 0.0 for t in ticks])
    return ticks, step


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


def to_host(tables, names, dtype=None):
    """{name: tables[name] as a numpy array on the host, cast to ``dtype`` if given; None where the tables hold none}."""
    out = {}
    for name in names:
        v = tables.get(name)
        if v is not None:
            v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            v = v if dtype is None else v.astype(dtype)
        out[name] = v
    return out


def node_count(table, nodes):
    """K = len(nodes), after checking that ``table`` has a row per key 0 .. K."""
    if table.shape[0] != len(nodes) + 1:
        raise ValueError(f"the tables hold {table.shape[0]} keys, the node list wants {len(nodes) + 1}")
    return len(nodes)


class Summary:
    """``to_json`` and ``==`` of a summary, from its ``to_dict``."""

    def to_json(self, **kw):
        return json.dumps(self.to_dict(), **kw)

    def __eq__(self, other):
        return isinstance(other, type(self)) and self.to_dict() == other.to_dict()


# ----------------------------------------------------------------------------- the key lattices of an edited scene
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


def refuse_empty_moved(what):
    raise _lib.CliftError(f"{what}: no lattice point at or above the level holds content that the last edit placed (the moved set is "
                          "empty): is the destination outside the scene box, the level too high, or the lattice too coarse?")


@torch.no_grad()
def settle_key(model, renderer, edit, upsample=1, level=None):
    """The key lattice ``clearance.settle_offset`` works on -> (key (n0, n1, n2) int32, ticks, n_moved): 2 where the edited scene holds
    density that the LAST edit of ``edit`` placed, 1 on all other density, 0 below the level."""
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


def scene_before(edit):
    """What stands where the LAST edit of ``edit`` places its object, as an edit program (None: the unedited scene): for a move the program
    with its last edit replaced by a delete of the same source box and shape, for a copy the program without its last edit."""
    from . import edit as ed
    program = ed.as_program(edit)
    last = program[len(program) - 1]
    if last.mode not in (ed.DUPLICATE, ed.MANIPULATE):
        raise ValueError(f"placement: the last edit must be a copy or a move (it is a {last.name})")
    head = list(program)[:-1]
    if last.mode == ed.MANIPULATE:
        head.append(ed.Edit(ed.DELETE, last.src, shape=last.shape))
    return ed.EditProgram(head) if head else None


@torch.no_grad()
def placement_key(model, renderer, edit, upsample=1, level=None):
    """The key lattice of ``distance.placement`` and ``placement.snap_offset`` -> (key (n0, n1, n2) int32 = R + 2 M, ticks): M the content
    that the LAST edit of ``edit`` placed, on the lattice of the edited scene (key 2 of ``settle_key``), R the density >= level of the scene
    before the paste (``scene_before``) on the same lattice."""
    before = scene_before(edit)
    level = default_level(renderer, 0.5) if level is None else float(level)
    moved_key, ticks, _ = settle_key(model, renderer, edit, upsample, level)
    sigma = renderer.get_dense_sigma(model, int(upsample), edit=before) if before is not None else renderer.get_dense_sigma(model, int(upsample))
    rest = sigma >= torch.tensor(level, dtype=torch.float32, device=sigma.device)
    return (rest.int() + 2 * (moved_key == 2).int()).int(), ticks
