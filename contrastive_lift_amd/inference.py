"""Inference render loop and post-processing -- mirror of reference inference/render_panopli.py:108-140 (per-frame
chunked rendering with is_train=False and the halved step ratio), util/camera.py:86-104 (distance_to_depth),
RP:422-427 (create_instances_from_semantics), RP:371-419 (assign_clusters) and RP:196-368 (MeanShift clustering: sklearn on the CPU exactly like
the reference, or DeviceMeanShift with the per-seed climb on the GPU).
"""
import numpy as np
import torch

from . import _lib, engine
from .hdbscan import DeviceHDBSCAN


def _render_chunks(rays, chunk, per_chunk):
    """The chunk loop of every ``render_rays*``: ``per_chunk(rays[i:i + chunk])`` -> a tuple of tensors, one row per ray, that the chunk's
    pass no longer owns (a view of its ``ray_out`` is cloned by the caller); the tuples are concatenated output by output.  ``chunk`` of 0
    or None renders all rays at once.  Whatever the pass kept beside its outputs (the context) is dropped before the next chunk starts."""
    chunk = int(chunk) if chunk and int(chunk) > 0 else rays.shape[0]
    outs = [per_chunk(rays[i:i + chunk]) for i in range(0, rays.shape[0], chunk)]
    return tuple(torch.cat(x, 0) for x in zip(*outs))


def _render_outputs(o):
    return o["rgb"], o["semantics"], o["instances"], o["depth"].clone()


def _surface_outputs(s):
    return s["depth_median"], s["hit"].to(torch.float32), s["normals"].contiguous()


def _layer_outputs(o):
    """layers, opacity, depth -- and the colour layers behind them where the pass formed them."""
    return (o["layers"], o["opacity"].clone(), o["depth"].clone()) + ((o["colour"],) if "colour" in o else ())


@torch.no_grad()
def render_rays(model, renderer, rays, chunk, white_bg=False):
    """Chunked renderer(model, rays[i:i+chunk], perturb, white_bg, is_train=False) (RP:114-120): returns
    rgb (P,3), semantics (P,C), instances (P,D), distance (P,)."""
    return _render_chunks(rays, chunk, lambda r: _render_outputs(engine.render_forward(model, renderer, r, None, bool(white_bg), grad_heads=())[0]))


@torch.no_grad()
def render_rays_edit(model, renderer, rays, chunk, white_bg=False, edit=None, weight_thres=0.0):
    """``render_rays`` under one scene edit or an ordered program of them (``edit.Edit`` / ``edit.EditProgram``, handed to
    engine.edit_forward as given): the same chunking and the same outputs.  With ``edit``
    and ``weight_thres`` bound (functools.partial) it has the ``render_fn`` signature of ``render_rays_sharded``, which then cuts an edited
    frame into row-tiles over the ranks like a plain one."""
    if edit is None:
        raise ValueError("render_rays_edit: an edit is required")
    return _render_chunks(rays, chunk, lambda r: _render_outputs(engine.edit_forward(model, renderer, r, edit, bool(white_bg), weight_thres=weight_thres)[0]))


@torch.no_grad()
def render_rays_surface(model, renderer, rays, chunk, white_bg=False, q=0.5):
    """``render_rays`` plus the surface outputs of every chunk's march (engine.surface_from_ctx, two more launches per chunk): returns
    rgb (P,3), semantics (P,C), instances (P,D), distance (P,), distance_median (P,), hit (P,) as float 0 / 1, normals (P,3) --
    the un-normalised sums of w n.  The first four are ``render_rays``' own.  It has the ``render_fn`` signature of ``render_rays_sharded``
    (bind ``q`` with functools.partial), which carries all seven over the ranks."""
    def per_chunk(r):
        o, ctx = engine.render_forward(model, renderer, r, None, bool(white_bg), grad_heads=())
        return _render_outputs(o) + _surface_outputs(engine.surface_from_ctx(model, renderer, ctx, q))

    return _render_chunks(rays, chunk, per_chunk)


@torch.no_grad()
def render_rays_edit_surface(model, renderer, rays, chunk, white_bg=False, edit=None, weight_thres=0.0, q=0.5):
    """``render_rays_edit`` plus the surface outputs of the edited scene from every chunk's march (engine.edit_surface_from_ctx, two more
    launches per chunk): the seven outputs of ``render_rays_surface`` -- rgb, semantics, instances, distance, distance_median, hit as float
    0 / 1, normals -- of which the first four are ``render_rays_edit``'s own.  With ``edit``, ``weight_thres`` and ``q`` bound
    (functools.partial) it has the ``render_fn`` signature of ``render_rays_sharded``."""
    if edit is None:
        raise ValueError("render_rays_edit_surface: an edit is required")

    def per_chunk(r):
        o, ctx = engine.edit_forward(model, renderer, r, edit, bool(white_bg), weight_thres=weight_thres)
        return _render_outputs(o) + _surface_outputs(engine.edit_surface_from_ctx(model, renderer, ctx, q))

    return _render_chunks(rays, chunk, per_chunk)


@torch.no_grad()
def render_rays_layers(model, renderer, rays, chunk, white_bg=False, table=None, alpha_thres=None, use_delta=False, colour=False, colour_rest=False):
    """Chunked ``engine.layers_forward``: the amodal instance layers of the rays under the slot table ``table``
    (``layers.SlotTable``).  Returns layers (P, K + 1, 4) rows [A, V, Z, zf], opacity (P,), distance (P,) -- the last two of the whole scene, as
    ``render_rays`` gives them.  A ray's layers depend on that ray alone, so the chunking changes no bit.  ``white_bg`` is accepted and unused
    (no colour is formed): with ``table``, ``alpha_thres`` and ``use_delta`` bound (functools.partial) it has the ``render_fn`` signature of
    ``render_rays_sharded``.  With ``colour`` a fourth output follows: colour (P, K + 1, 4) rows [R, G, B, A], premultiplied, without a
    background (``colour_rest``: the rest column is coloured too)."""
    if table is None:
        raise ValueError("render_rays_layers: a slot table is required (layers.SlotTable)")
    return _render_chunks(rays, chunk, lambda r: _layer_outputs(engine.layers_forward(model, renderer, r, table, alpha_thres=alpha_thres, use_delta=use_delta,
                                                                                      colour=colour, colour_rest=colour_rest)[0]))


@torch.no_grad()
def render_rays_edit_layers(model, renderer, rays, chunk, white_bg=False, table=None, edit=None, alpha_thres=None, use_delta=False, colour=False,
                            colour_rest=False):
    """Chunked ``engine.edit_layers_forward``: the amodal instance layers of the scene ``edit`` describes, under the slot table
    ``table`` extended by one column per copy (``table.for_program(edit)`` names them).  Returns layers (P, K + c + 1, 4), opacity (P,),
    distance (P,) like ``render_rays_layers``; a ray's layers depend on that ray alone, so the chunking changes no bit.  With ``table``,
    ``edit``, ``alpha_thres`` and ``use_delta`` bound (functools.partial) it has the ``render_fn`` signature of ``render_rays_sharded``.
    With ``colour`` a fourth output follows, colour (P, K + c + 1, 4), as in ``render_rays_layers``."""
    if table is None:
        raise ValueError("render_rays_edit_layers: a slot table is required (layers.SlotTable)")
    if edit is None:
        raise ValueError("render_rays_edit_layers: an edit is required")
    return _render_chunks(rays, chunk,
                          lambda r: _layer_outputs(engine.edit_layers_forward(model, renderer, r, edit, table, alpha_thres=alpha_thres, use_delta=use_delta,
                                                                              colour=colour, colour_rest=colour_rest)[0]))


def tile_bounds(n, world):
    """Contiguous row-tile boundaries of n rays over `world` ranks (sizes differ by at most one)."""
    return [(n * r) // world for r in range(world + 1)]


@torch.no_grad()
def render_rays_sharded(model, renderer, rays, chunk, white_bg=False, render_fn=None):
    """Multi-GPU frame render (BASELINE configs[4]): the rays of a frame are cut into contiguous row-tiles, one
    per rank; every rank renders its tile with no communication, then ONE all-gather (RCCL over xGMI; 4*(4+C+D) bytes per
    ray) assembles the per-ray outputs on every rank.  With no process group it is ``render_rays``.
    ``render_fn(model, renderer, rays, chunk, white_bg)`` defaults to ``render_rays`` (injectable for CPU tests)."""
    import torch.distributed as dist
    fn = render_fn or render_rays
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return fn(model, renderer, rays, chunk, white_bg)
    world, rank = dist.get_world_size(), dist.get_rank()
    P = rays.shape[0]
    b = tile_bounds(P, world)
    n_mine = b[rank + 1] - b[rank]
    # a rank whose tile is empty (fewer rays than ranks) renders one ray so that it knows the output widths, and keeps none
    mine = fn(model, renderer, rays[b[rank]:b[rank + 1]] if n_mine else rays[:1], chunk, white_bg)
    mine = tuple(x[:n_mine] for x in mine)
    widths = [int(np.prod(x.shape[1:])) for x in mine]                    # (1 for a per-ray scalar; the layers' (K + 1, 4) rows travel flat)
    packed = torch.cat([x.reshape(n_mine, w) for x, w in zip(mine, widths)], 1)
    cap = max(b[r + 1] - b[r] for r in range(world))                      # equal-size slots: tiles differ by <= 1 ray
    slot = torch.zeros((cap, packed.shape[1]), dtype=packed.dtype, device=packed.device)
    slot[:packed.shape[0]] = packed
    if dist.get_backend() != "nccl":           # CPU-side backends (gloo in the tests) gather host copies
        host = slot.cpu()
        slots = [torch.empty_like(host) for _ in range(world)]
        dist.all_gather(slots, host)
        slots = [s_.to(slot.device) for s_ in slots]
    else:
        slots = [torch.empty_like(slot) for _ in range(world)]
        dist.all_gather(slots, slot)
    full = torch.cat([slots[r][:b[r + 1] - b[r]] for r in range(world)], 0)
    outs, c = [], 0
    for x, w in zip(mine, widths):
        o = full[:, c:c + w]
        outs.append(o.reshape((-1,) + tuple(x.shape[1:])).contiguous())
        c += w
    return tuple(outs)


def distance_to_depth(K, dist):
    """util/camera.py:86-104 for a (H,W) distance image on the device: z = dist / |K^-1 [u, v, 1]|."""
    H, W = dist.shape
    dev = dist.device
    u, v = torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy")
    uvh = torch.stack([u.reshape(-1), v.reshape(-1), torch.ones(H * W, device=dev, dtype=torch.long)], -1).to(dist.dtype)
    tmp = uvh @ torch.inverse(torch.as_tensor(K, dtype=dist.dtype, device=dev)).T
    return dist.reshape(-1) / torch.linalg.norm(tmp, dim=1)


def create_instances_from_semantics(instances, semantics, thing_classes):
    """RP:422-427: prepend a column that is +inf for stuff pixels and -inf for thing pixels."""
    stuff = ~torch.isin(semantics.argmax(dim=1), torch.tensor(list(thing_classes), device=semantics.device))
    padded = torch.full((instances.shape[0], instances.shape[1] + 1), -float("inf"), device=instances.device)
    padded[:, 1:] = instances
    padded[stuff, 0] = float("inf")
    return padded


def _one_hot(all_labels, num_images, device):
    all_labels = all_labels + 1                                  # -1,0,..,K-1 -> 0,1,..,K
    n_lab = int(all_labels.max()) + 1
    onehot = torch.zeros((all_labels.shape[0], n_lab), dtype=torch.float64, device=device)
    onehot[torch.arange(all_labels.shape[0], device=device), all_labels] = 1
    return onehot.view(num_images, -1, n_lab)


@torch.no_grad()
def assign_cluster_labels(features, sem, thing, all_centroids):
    """The labelling of RP:371-419 on device rows: features (P, E) fp32, sem (P) class ids, thing (P) bool.  Per thing class present, in
    ascending order, the nearest cached centroid (clift_nearest_centroid); labels of successive classes are offset so they stay
    disjoint; rows that are not things get -1.  -> (P) int64.  ``label + 1`` is the id written to pred_surrogateid (0 = stuff)."""
    device = features.device
    f = features.contiguous()
    labels = torch.full((f.shape[0],), -1, dtype=torch.int64, device=device)
    max_label = 0
    for cls in torch.unique(sem[thing]).tolist():
        cent = torch.as_tensor(np.asarray(all_centroids[cls]), dtype=torch.float32, device=device).contiguous()
        valid = (thing & (sem == cls)).to(torch.uint8).contiguous()
        lab = torch.empty((f.shape[0],), dtype=torch.int32, device=device)
        _lib.call("clift_nearest_centroid", _lib.ptr(f), f.shape[1], f.shape[1], _lib.ptr(cent), cent.shape[0], _lib.ptr(valid),
                  f.shape[0], _lib.ptr(lab), _lib.stream())
        sel = valid.bool()
        labels[sel] = lab[sel].long() + max_label
        if bool(sel.any()):
            max_label = int(labels[sel].max()) + 1
    return labels


@torch.no_grad()
def assign_clusters(all_thing_features, all_points_semantics, all_centroids, device, num_images):
    """RP:371-419: per thing class, nearest cached centroid (clift_nearest_centroid on the device); stuff pixels get
    label -1; labels of successive classes are offset so they stay disjoint; returns one-hot (num_images, P, K+1)."""
    feats = torch.as_tensor(all_thing_features, dtype=torch.float32, device=device)
    sem = torch.cat([s.to(device) for s in all_points_semantics], 0).argmax(-1)
    labels = assign_cluster_labels(feats[:, 1:], sem, feats[:, 0] == -float("inf"), all_centroids)
    return _one_hot(labels, num_images, device)


def _check_hdbscan(hdbscan):
    if hdbscan not in ("sklearn", "device"):
        raise ValueError(f"hdbscan must be 'sklearn' or 'device' (got {hdbscan!r})")
    return hdbscan


def _hdbscan_fit(pts, cluster_size, hdbscan="sklearn", device=None):
    """RP:236-241 / 321-326: HDBSCAN(min_cluster_size, min_samples=1, allow_single_cluster=True) on the rescaled subsample; returns
    (labels, centroids (K, d) or None when every point is noise).  centroid k = the membership-probability-weighted mean of cluster k's
    points -- the ``weighted_cluster_centroid`` of the hdbscan package the reference imports.  That package is not in this image: the fit
    comes from the package when it is importable and otherwise from ``sklearn.cluster.HDBSCAN`` (scikit-learn >= 1.3: the same algorithm,
    adopted from that package -- mutual-reachability MST, condensed tree, excess-of-mass selection; PARITY UNPINNED against the package
    itself).  ``hdbscan="device"`` runs the same fit as DeviceHDBSCAN (hdbscan.py: the minimum spanning tree by
    clift_emst on ``device``, the tree pass on the host), pinned to sklearn's estimator: equal labels, probabilities to rounding."""
    if _check_hdbscan(hdbscan) == "device":
        cl = DeviceHDBSCAN(cluster_size, min_samples=1, allow_single_cluster=True, device="cuda" if device is None else device).fit(pts)
        labels, prob = cl.labels_, cl.probabilities_
    else:
        try:
            import hdbscan as _pkg                                 # the reference's dependency (requirements.txt)
            cl = _pkg.HDBSCAN(min_cluster_size=cluster_size, min_samples=1, prediction_data=True, allow_single_cluster=True).fit(pts)
            labels, prob = cl.labels_, cl.probabilities_
        except ImportError:
            from sklearn.cluster import HDBSCAN
            cl = HDBSCAN(min_cluster_size=cluster_size, min_samples=1, allow_single_cluster=True, copy=True).fit(pts)
            labels, prob = cl.labels_, cl.probabilities_
    ids = [k for k in np.unique(labels) if k != -1]
    if not ids:
        return labels, None
    return labels, np.stack([np.average(pts[labels == k], weights=prob[labels == k], axis=0) for k in ids])


def _nearest_centroid(points, centroids, device):
    """RP:244-254: every point to its nearest centroid (squared distances through clift_nearest_centroid on the device; ties -> lowest index,
    as torch.argmin over cdist)."""
    f = torch.as_tensor(np.ascontiguousarray(points), dtype=torch.float32, device=device).contiguous()
    c = torch.as_tensor(np.ascontiguousarray(centroids), dtype=torch.float32, device=device).contiguous()
    if f.device.type != "cuda":
        return torch.argmin(torch.cdist(f, c), dim=-1).cpu().numpy()
    valid = torch.ones((f.shape[0],), dtype=torch.uint8, device=device)
    lab = torch.empty((f.shape[0],), dtype=torch.int32, device=device)
    _lib.call("clift_nearest_centroid", _lib.ptr(f), f.shape[1], f.shape[1], _lib.ptr(c), c.shape[0], _lib.ptr(valid), f.shape[0], _lib.ptr(lab),
              _lib.stream())
    return lab.cpu().numpy().astype(np.int64)


def bin_seeds(X, bin_size, min_bin_freq=1):
    """sklearn.cluster.get_bin_seeds, vectorised: bins np.round(X / bin_size) (in X's dtype), the bins holding at least ``min_bin_freq``
    points in order of first occurrence, as fp32 and scaled back by ``bin_size``; X itself when bin_size is 0 or every point is its own bin."""
    if bin_size == 0:
        return X
    binned = np.round(X / bin_size) + 0.0                         # (+ 0.0: -0.0 and 0.0 are one bin, as they are one dict key)
    uniq, first, freq = np.unique(binned, axis=0, return_index=True, return_counts=True)
    keep = freq >= min_bin_freq
    seeds = uniq[keep][np.argsort(first[keep], kind="stable")].astype(np.float32)
    if len(seeds) == len(X):
        return X
    return seeds * bin_size


def device_shift(X, seeds, bandwidth, max_iter, device):
    """clift_meanshift on ``device``: returns (centers (S, d) fp32, counts (S,) int, iters (S,) int) as numpy arrays."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CliftError(f"DeviceMeanShift: clift_meanshift runs on a GPU device, got {dev}")
    x = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float32), device=dev)
    sd = torch.as_tensor(np.ascontiguousarray(seeds, dtype=np.float32), device=dev)
    S, d = sd.shape
    centers = torch.empty((S, d), dtype=torch.float32, device=dev)
    counts = torch.empty((S,), dtype=torch.int32, device=dev)
    iters = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.call("clift_meanshift", _lib.ptr(x), x.shape[0], x.shape[1], d, _lib.ptr(sd), S, float(bandwidth), int(max_iter), _lib.ptr(centers),
              _lib.ptr(counts), _lib.ptr(iters), _lib.stream())
    return centers.cpu().numpy(), counts.cpu().numpy().astype(np.int64), iters.cpu().numpy().astype(np.int64)


class DeviceMeanShift:
    """sklearn ``MeanShift(bandwidth, bin_seeding=True, min_bin_freq, cluster_all=False, max_iter)`` with the per-seed climb on the GPU
    (clift_meanshift: one launch for all seeds).  The host part is sklearn's ``fit``: bin seeding (``bin_seeds``), results with exactly
    equal centre tuples merged, seeds with an empty neighbourhood dropped (ValueError when none is left), sorted by (count, centre)
    descending, then near-duplicates within ``bandwidth`` removed with sklearn's NearestNeighbors (the centre with more points stays).
    ``fit`` sets ``cluster_centers_`` (K, d) fp32 and ``n_iter_``; ``predict`` is the nearest centre (clift_nearest_centroid).
    X is taken as fp32 (the reference clusters fp32 features).  ``shift_fn(X, seeds, bandwidth, max_iter) -> (centers, counts, iters)``
    replaces the device climb (CPU tests of the host logic)."""

    def __init__(self, bandwidth, min_bin_freq=10, max_iter=300, device="cuda", shift_fn=None):
        self.bandwidth, self.min_bin_freq, self.max_iter = float(bandwidth), int(min_bin_freq), int(max_iter)
        self.device = device
        self.shift_fn = shift_fn or (lambda X, seeds, bw, it: device_shift(X, seeds, bw, it, self.device))

    def fit(self, X):
        from sklearn.neighbors import NearestNeighbors
        X = np.ascontiguousarray(X, dtype=np.float32)
        bw = self.bandwidth
        seeds = bin_seeds(X, bw, self.min_bin_freq)
        centers, counts, iters = self.shift_fn(X, seeds, bw, self.max_iter)
        centers = np.asarray(centers, dtype=np.float32)
        intensity = {}
        for c, n in zip(centers, np.asarray(counts).tolist()):
            if n:
                intensity[tuple(c)] = n
        self.n_iter_ = int(np.max(iters)) if len(iters) else 0
        if not intensity:
            raise ValueError(f"No point was within bandwidth={bw:f} of any seed. Try a different seeding strategy or increase the bandwidth.")
        ranked = sorted(intensity.items(), key=lambda tup: (tup[1], tup[0]), reverse=True)
        sorted_centers = np.array([tup[0] for tup in ranked])
        unique = np.ones(len(sorted_centers), dtype=bool)
        nbrs = NearestNeighbors(radius=bw).fit(sorted_centers)
        for i, center in enumerate(sorted_centers):
            if unique[i]:
                unique[nbrs.radius_neighbors([center], return_distance=False)[0]] = 0
                unique[i] = 1
        self.cluster_centers_ = sorted_centers[unique]
        return self

    def predict(self, X):
        return _nearest_centroid(np.asarray(X, dtype=np.float32), self.cluster_centers_, self.device)


def _meanshift(pts, bandwidth, meanshift, device):
    """The reference's MeanShift(bandwidth, cluster_all=False, bin_seeding=True, min_bin_freq=10) fit: sklearn on the CPU ("sklearn") or
    DeviceMeanShift ("device")."""
    if meanshift == "sklearn":
        from sklearn.cluster import MeanShift
        return MeanShift(bandwidth=bandwidth, cluster_all=False, bin_seeding=True, min_bin_freq=10).fit(pts)
    if meanshift == "device":
        return DeviceMeanShift(bandwidth, min_bin_freq=10, device=device).fit(pts)
    raise ValueError(f"meanshift must be 'sklearn' or 'device' (got {meanshift!r})")


def cluster(all_thing_features, bandwidth, device, num_images, num_points=50000, use_silverman=False, use_dbscan=False, cluster_size=500,
            meanshift="sklearn", hdbscan="sklearn"):
    """RP:196-263: 3-sigma outlier filter, per-axis rescale to the
    unit box, a 50000-point subsample drawn with ``np.random.choice`` from numpy's GLOBAL generator exactly as the reference
    does (seed it with ``np.random.seed`` for reproducible runs), sklearn MeanShift (optionally with Silverman's bandwidth) or, with
    ``use_dbscan``, HDBSCAN (``_hdbscan_fit``), then every pixel is assigned to its nearest cluster.  Returns (one-hot (num_images, P, K+1) float64, centroids in feature
    units).  Scenes with fewer thing pixels than ``num_points`` use all of them (the reference raises there).  ``meanshift="device"`` runs
    the MeanShift fit as DeviceMeanShift (GPU) instead of sklearn, ``hdbscan="device"`` the HDBSCAN fit as DeviceHDBSCAN."""
    _check_hdbscan(hdbscan)
    feats = np.asarray(all_thing_features)
    thing = feats[..., 0] == -float("inf")
    f_th = feats[thing][:, 1:]
    f_all = feats[:, 1:]
    mu, sd = f_th.mean(axis=0), f_th.std(axis=0)
    keep = np.all(np.abs(f_th - mu) < 3 * sd, axis=1)
    cf = f_th[keep]
    bias = cf.min(axis=0)
    factor = 1 / (cf.max(axis=0) - cf.min(axis=0))
    cr = (cf - bias) * factor
    idx = np.random.choice(cr.shape[0], num_points, replace=False) if cr.shape[0] >= num_points else np.arange(cr.shape[0])
    pts = cr[idx]
    if use_silverman:
        from scipy.stats import gaussian_kde
        bandwidth = gaussian_kde(pts.T, bw_method="silverman").covariance_factor()
    if use_dbscan:                                                # RP:236-255: HDBSCAN on the subsample, then EVERY point to its nearest centroid
        _, centers = _hdbscan_fit(pts, cluster_size, hdbscan, device)
        if centers is None:
            raise _lib.CliftError("HDBSCAN found no cluster (every sampled point is noise); the reference fails here too (np.stack of an empty list)")
        all_labels = _nearest_centroid((f_all.reshape(-1, f_all.shape[-1]) - bias) * factor, centers, device)
    else:
        ms = _meanshift(pts, bandwidth, meanshift, device)
        all_labels = ms.predict((f_all.reshape(-1, f_all.shape[-1]) - bias) * factor)
        centers = ms.cluster_centers_
    all_labels[~thing] = -1
    all_labels = all_labels + 1                                   # -1,0,..,K-1 -> 0,1,..,K
    K1 = centers.shape[0] + 1                                      # width = number of centroids + 1 (not max label + 1)
    onehot = torch.zeros((all_labels.shape[0], K1), dtype=torch.float64, device=device)
    onehot[torch.arange(all_labels.shape[0], device=device), torch.as_tensor(all_labels, dtype=torch.int64, device=device)] = 1
    return onehot.view(num_images, -1, K1), centers / factor + bias


def cluster_segmentwise(all_thing_features, all_points_semantics, bandwidth, device, num_images, num_points=50000, use_silverman=False,
                        use_dbscan=False, cluster_size=500, meanshift="sklearn", return_dict=False, hdbscan="sklearn"):
    """RP:265-368: the clustering of ``cluster`` (MeanShift, or HDBSCAN with ``use_dbscan``) run separately inside every predicted thing class, labels of
    successive classes offset so they stay disjoint; classes with fewer than 100 (filtered) points get no instances (-1).
    Returns (one-hot (num_images, P, max label + 2) float64, concatenated centroids in feature units).  Like the reference,
    a class that is skipped for having too few points still appends the previous class's centroids (rescaled with its own
    statistics) to the returned list -- only the one-hot output is consumed by the render script.  ``meanshift="device"`` runs the fits
    as DeviceMeanShift, ``hdbscan="device"`` the HDBSCAN fits as DeviceHDBSCAN.  With ``return_dict`` the centroids come back as the reference's per-class cache (extract_train_centroids.py:211-313):
    ``{thing class (np.int64): centroids in feature units}``, incl. that stale entry for a skipped class; this is the mapping that
    ``assign_clusters`` (--cached_centroids_path) reads."""
    _check_hdbscan(hdbscan)
    sem = torch.cat([s_.cpu() for s_ in all_points_semantics], 0).argmax(-1).numpy()
    feats = np.asarray(all_thing_features)
    thing = feats[..., 0] == -float("inf")
    f_th = feats[thing][:, 1:]
    n_all = feats.shape[0]
    th_sem = sem[thing]
    all_labels = np.zeros(n_all, dtype=np.int32)
    th_labels = np.zeros(f_th.shape[0], dtype=np.int32)
    max_label = 0
    cents_all, cents_by_cls, centroids = [], {}, None
    for cls in np.unique(th_sem):
        m = th_sem == cls
        fc = f_th[m]
        mu, sd = fc.mean(axis=0), fc.std(axis=0)
        cf = fc[np.all(np.abs(fc - mu) < 3 * sd, axis=1)]
        if cf.shape[0] == 0:
            th_labels[m] = -1
            continue
        bias = cf.min(axis=0)
        factor = 1 / (cf.max(axis=0) - cf.min(axis=0))
        cr = (cf - bias) * factor
        idx = np.arange(cr.shape[0]) if cr.shape[0] < num_points else np.random.choice(cr.shape[0], num_points, replace=False)
        pts = cr[idx]
        if use_dbscan:                                              # RP:320-342
            _, cents = _hdbscan_fit(pts, cluster_size, hdbscan, device)
            if cents is not None:
                centroids = cents
                lab = _nearest_centroid((fc.reshape(-1, fc.shape[-1]) - bias) * factor, cents, device).astype(np.int32)
            else:
                lab = -1 * np.ones(fc.shape[0], dtype=np.int32)
        elif pts.shape[0] < 100:                                    # too few points for MeanShift
            lab = -1 * np.ones(fc.shape[0], dtype=np.int32)
        else:
            bw = bandwidth
            if use_silverman:
                from scipy.stats import gaussian_kde
                bw = gaussian_kde(pts.T, bw_method="silverman").covariance_factor()
            ms = _meanshift(pts, bw, meanshift, device)
            centroids = ms.cluster_centers_
            lab = ms.predict((fc.reshape(-1, fc.shape[-1]) - bias) * factor)
        if centroids is not None:
            cents_all.append(centroids / factor + bias)
            cents_by_cls[cls] = cents_all[-1]
        lab[lab != -1] += max_label
        if np.any(lab != -1):
            max_label = lab.max() + 1
        th_labels[m] = lab
    all_labels[thing] = th_labels
    all_labels[~thing] = -1
    onehot = _one_hot(torch.as_tensor(all_labels, dtype=torch.int64, device=device), num_images, device)
    if return_dict:
        return onehot, cents_by_cls
    return onehot, (np.concatenate(cents_all, axis=0) if cents_all else np.zeros((0, f_th.shape[1])))


def psnr(image_pred, image_gt):
    """util/metrics.py:25-26."""
    return -10 * torch.log10(torch.mean((image_pred.detach() - image_gt) ** 2))


class ConfusionMatrix:
    """util/metrics.py:29-75: confusion counts + robust mIoU (classes that are rare in both marginals are ignored).
    ``backend="device"`` / ``"counts"``: the counts come from one label-overlap count per batch (overlap.py: classes against classes, one
    frame; ground truth outside [0, n) is dropped like the host mask does) -- "device" takes CUDA tensors as they are.  ``add_batch`` may
    name another backend for one batch."""

    def __init__(self, num_classes, ignore_class=None, robust=0.005, backend="host"):
        from . import overlap
        self.n, self.ignore, self.robust, self.backend = num_classes, list(ignore_class or []), robust, overlap.check_backend(backend)
        self.cm = np.zeros((num_classes, num_classes))

    def _matrix(self, gt, pred):
        m = (gt >= 0) & (gt < self.n)
        return np.bincount(self.n * gt[m].astype(int) + pred[m], minlength=self.n ** 2).reshape(self.n, self.n)

    def _matrix_counted(self, gt, pred, backend):
        from . import overlap
        counter = overlap.Counter(backend, gt.device if torch.is_tensor(gt) and gt.is_cuda else None)
        gt, pred = counter.labels(gt), counter.labels(pred)
        if gt.shape[0] != pred.shape[0]:
            raise ValueError("ground truth and prediction differ in size")
        n = self.n
        a_base = np.concatenate([np.arange(n), [-1]]).astype(np.int32)[None]                  # class n = "outside [0, n)": dropped
        pred = counter.int32(pred, *counter.extremes([pred])[0])
        counts = counter.count(counter.remap_outside(gt, n), None, pred, None, [0, int(gt.shape[0])], a_base, np.zeros((1, n + 1), np.int32),
                               np.arange(n, dtype=np.int32)[None], np.zeros((1, n), np.int32), n, n)
        return counter.host(counts)[0]

    def _miou(self, cm):
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm))
        a0, a1, tot = cm.sum(0), cm.sum(1), cm.sum()
        nonrobust = np.where((a0 / tot < self.robust) & (a1 / tot < self.robust))[0].tolist()
        for i in self.ignore + nonrobust:
            iou[i] = np.nan
        return np.nanmean(iou)

    def add_batch(self, gt_image, pre_image, return_miou=False, backend=None):
        from . import overlap
        backend = self.backend if backend is None else overlap.check_backend(backend)
        if backend == "host":
            cm = self._matrix(np.asarray(gt_image), np.asarray(pre_image))
        else:
            cm = self._matrix_counted(gt_image, pre_image, backend)
        self.cm += cm
        if return_miou:
            return self._miou(cm)

    def get_miou(self):
        return self._miou(self.cm)
