"""Embeddings at the reference's 3LC hook points.

The reference hands one activation of each network to 3LC's ``EmbeddingsMetricsCollector`` and reduces the collected table with PaCMAP
so that uploads can be browsed by similarity:

    scripts/process_new_raw/process_pipeline.py:328-351   EmbeddingsMetricsCollector([52]), ``--embedding_layer`` on the command line
    scripts/train/train_unet.py:219                        UNet ``named_modules()[52]`` = down4.maxpool_conv.1.double_conv.5
    scripts/train/train_classifier.py:32,212               ResNet ``named_modules()[90]`` = global_pool

The reading this rests on (3LC is not part of the reference tree): the collector reduces a hooked (B, C, H, W) output with its default
reshape strategy "mean" -- the mean over the non-batch, non-channel dimensions, (B, C).  The HIP engines compute exactly that on the
device, inside the forward (``HipEngine.unet_forward(..., want_embedding=True)`` and its siblings, ``ChessVision.process_images(...,
embeddings=True)``), and for any other stored layer on request (``HipEngine.activation_channel_means``).  With the alternative strategy
"flatten" index 90 gives the same vector (global_pool's output is (B, 512)); at index 52 it needs the whole tensor, for which
``HipEngine.activation`` remains the way.

This module holds what needs no device: the reference's integer layer indices as tap names, the host form of the reduction for
model objects that are not HIP models, and the host form of the neighbour search.  The HIP model objects are not ``nn.Module``s that
take forward hooks.

What the table is collected for: the reference reduces it with ``run.reduce_embeddings_by_foreign_table_url(..., method="pacmap")``
(``process_pipeline.py:351``, ``train_classifier.py:312``).  The exact k-nearest-neighbour graph it (and UMAP) starts from is served:
``neighbours`` here is the definition and the checker in numpy, ``HipEngine.embedding_neighbours`` / ``ChessVision.embedding_neighbours``
the device form, equal to it bit for bit.  ``stack`` turns ``process_images(..., embeddings=True)`` results into the table,
``duplicate_groups`` answers "which uploads are near-duplicates".  The reduction itself is the last part of this file: ``pacmap`` is the
definition in numpy (a reading of the paper and of the package's defaults, see there), ``HipEngine.pacmap_pairs`` /
``HipEngine.pacmap_optimise`` / ``ChessVision.reduce_embeddings`` the device form, equal to it bit for bit.  After it, the other half of
that call: ``pacmap_fit`` keeps what placing further tables into the same map needs (``EmbeddingMap``), ``pacmap_transform`` places
them (a reading of the package's ``transform``); ``HipEngine.pacmap_place_pairs`` / ``HipEngine.pacmap_place`` /
``ChessVision.fit_embedding_map`` / ``ChessVision.place_embeddings`` are the device form, again bit for bit.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

UNET_HOOK_INDEX = 52                 # train_unet.py:219, process_pipeline.py:328
CLASSIFIER_HOOK_INDEX = 90           # train_classifier.py:32 (resnet18)
_RESNET_DEPTHS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _double_conv(prefix: str) -> list[str]:
    return [prefix, prefix + ".double_conv"] + [f"{prefix}.double_conv.{i}" for i in range(6)]


def module_names(model: str, bilinear: bool = False) -> list[str]:
    """``[name for name, _ in net.named_modules()]`` of the reference's ``UNet(3, 1, bilinear)`` (model "unet"; the order is the same
    for both variants, only the type of ``upN.up`` differs) or of timm's ``resnet18`` / ``resnet34`` (in_chans=1, 13 classes), as a
    plain list: index i of it is the reference's integer layer index i."""
    if model == "unet":
        names = [""] + _double_conv("inc")
        for i in range(1, 5):
            p = f"down{i}"
            names += [p, p + ".maxpool_conv", p + ".maxpool_conv.0"] + _double_conv(p + ".maxpool_conv.1")
        for i in range(1, 5):
            p = f"up{i}"
            names += [p, p + ".up"] + _double_conv(p + ".conv")
        return names + ["outc", "outc.conv"]
    if model.startswith("yolov8"):
        raise ValueError(f"{model}: the reference's integer layer indices are positions in named_modules() of its UNet and its timm ResNets; "
                         "a YOLOv8-cls classifier has no such table here -- name the tap by its state-dict prefix instead ('model.4.m.1', "
                         "'model.9.conv'; 'global_pool' is the pooled model.9.conv output, the embedding)")
    if model not in _RESNET_DEPTHS:
        raise ValueError(f"model must be 'unet', 'resnet18' or 'resnet34', got {model!r}")
    names = ["", "conv1", "bn1", "act1", "maxpool"]
    for layer, depth in enumerate(_RESNET_DEPTHS[model], start=1):
        names.append(f"layer{layer}")
        for b in range(depth):
            p = f"layer{layer}.{b}"
            names += [p] + [f"{p}.{leaf}" for leaf in ("conv1", "bn1", "drop_block", "act1", "aa", "conv2", "bn2", "act2")]
            if b == 0 and layer > 1:
                names += [p + ".downsample", p + ".downsample.0", p + ".downsample.1"]
    return names + ["global_pool", "global_pool.pool", "global_pool.flatten", "fc"]


def _unet_tap(name: str) -> str | None:
    """The engine tap that holds the output of UNet module ``name``, or None: the engines store the output of every ReLU, max-pool and
    up-sampling (BatchNorm is folded into the convolution's epilogue, so a bare Conv2d / BatchNorm2d output never exists)."""
    if name.startswith("outc"):
        return None                                  # the single-channel logits are the forward's result, not a stored tensor
    if name.endswith((".double_conv.2", ".double_conv.5", ".maxpool_conv.0", ".up")):
        return name
    for tail in (".maxpool_conv.1.double_conv", ".maxpool_conv.1", ".maxpool_conv", ".conv.double_conv", ".conv", ".double_conv"):
        if name.endswith(tail):                      # a container: its output is its last ReLU's, which the block's own tap aliases
            return name[:-len(tail)]
    if name == "inc" or (name[:-1] in ("down", "up") and name[-1:] in "1234"):
        return name
    return None


def _resnet_tap(name: str) -> str | None:
    if name in ("act1", "maxpool") or name in ("layer1", "layer2", "layer3", "layer4"):
        return name
    if name.startswith("global_pool"):
        return "global_pool"                         # the pooled layer4 output (HipEngine.activation_channel_means takes the name)
    parts = name.split(".")
    if len(parts) == 2 and parts[0].startswith("layer"):
        return name                                  # a block's output
    if len(parts) == 3 and parts[2] in ("act1", "aa"):
        return ".".join(parts[:2]) + ".act1"         # aa is an Identity behind act1 (drop_block, the one before it, passes bn1's output on)
    if len(parts) == 3 and parts[2] == "act2":
        return ".".join(parts[:2])
    if len(parts) >= 3 and parts[2] == "downsample" and (len(parts) == 3 or parts[3] == "1"):
        return ".".join(parts[:3])                   # the shortcut after its BatchNorm
    return None


def _absent(model: str, precision: str | None) -> set[str]:
    """Taps an engine of ``precision`` fuses away with the default switches (None: not known, nothing is excluded here and the engine
    answers CV_ERR_INVALID naming the tap)."""
    if precision is None:
        return set()
    if model == "unet":
        out = {"up4", "up4.conv.double_conv.5"}      # the last convolution carries OutConv in its epilogue
        if precision == "f16x3":
            out.add("inc.double_conv.2")             # the fused inc pair
        return out
    out = set()
    if precision != "f32":
        out.add("act1")                              # stem + max-pool in one kernel
    if precision == "f16r":                          # layer1 (up to three blocks) as one chained launch
        out |= {f"layer1.{b}.act1" for b in range(min(_RESNET_DEPTHS[model][0], 3))}
    return out


def tap_for_index(model: str, index: int, bilinear: bool = False, precision: str | None = None) -> str:
    """The reference's integer layer index (``--embedding_layer``, an index into ``named_modules()``) as the name of the engine tap that
    holds that module's output: ``tap_for_index("unet", 52) == "down4.maxpool_conv.1.double_conv.5"``, ``tap_for_index("resnet18", 90)
    == "global_pool"``.  ``ValueError`` naming the index, the module and the nearest materialised taps when the engines never store that
    output (a bare Conv2d or BatchNorm2d, the root module, OutConv's single channel, the classifier's ``fc``), or -- with ``precision``
    given -- when an engine of that precision fuses it away."""
    names = module_names(model, bilinear)
    if not 0 <= int(index) < len(names):
        raise ValueError(f"{model} has {len(names)} modules: layer index {index} is out of range")
    index = int(index)
    tap_of = _unet_tap if model == "unet" else _resnet_tap
    absent = _absent(model, precision)

    def tap(i):
        t = tap_of(names[i]) if names[i] else None
        return None if t in absent else t

    found = tap(index)
    if found is not None:
        return found
    before = next((f"{i} ({tap(i)})" for i in range(index - 1, -1, -1) if tap(i)), None)
    after = next((f"{i} ({tap(i)})" for i in range(index + 1, len(names)) if tap(i)), None)
    near = " and ".join(n for n in (before, after) if n)
    why = f"fused away by the {precision} engine" if names[index] and tap_of(names[index]) else "never stored by the HIP engines"
    raise ValueError(f"layer index {index} of {model} is module '{names[index] or '<root>'}', whose output is {why}; "
                     f"nearest materialised: {near}")


def channel_mean(nchw) -> np.ndarray:
    """(B, C, H, W) -> (B, C) float32: the mean over the spatial dimensions, computed in float64.  The host form of the reduction, for
    hooked outputs of model objects that are not HIP models; a (B, C) input (global_pool) is returned as float32 unchanged."""
    a = np.asarray(nchw.detach().cpu() if hasattr(nchw, "detach") else nchw)
    if a.ndim < 2:
        raise ValueError(f"channel_mean expects (B, C, ...), got shape {a.shape}")
    if a.ndim == 2:
        return a.astype(np.float32)
    return a.astype(np.float64).mean(axis=tuple(range(2, a.ndim))).astype(np.float32)


# ---- exact nearest neighbours: the definition (include/chessvision_hip.h: cv_embedding_neighbours) -----------------------------------
MAX_NEIGHBOURS = 64


@dataclasses.dataclass
class Neighbours:
    """``indices`` (Q, k) int32, -1 where fewer than k corpus rows were eligible or the query row is not finite; ``sq_distances``
    (Q, k) float64 squared Euclidean distances (+inf / NaN in those slots); ``stats``: the record of ``cv_neighbour_stats_t`` as a
    dict (the numpy form certifies nothing: every finite row counts as an exact-path row)."""
    indices: np.ndarray
    sq_distances: np.ndarray
    stats: dict


def _table(a, name: str) -> np.ndarray:
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name} must be a (rows, channels) table with at least one row and one channel, got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def check_neighbour_arguments(q: int, n: int, c_q: int, c_n: int, k: int, corpus_given: bool, exclude_self) -> bool:
    """The argument rules both forms share; returns the effective ``exclude_self``."""
    if c_q != c_n:
        raise ValueError(f"queries have {c_q} channels, the corpus {c_n}")
    if not 1 <= int(k) <= MAX_NEIGHBOURS:
        raise ValueError(f"k must be in [1, {MAX_NEIGHBOURS}], got {k}")
    if exclude_self is None:
        exclude_self = not corpus_given
    if exclude_self and q != n:
        raise ValueError(f"exclude_self drops corpus row i for query row i and needs as many queries as corpus rows, got {q} and {n}")
    return bool(exclude_self)


def neighbours(queries, corpus=None, k: int = 10, exclude_self=None) -> Neighbours:
    """The k nearest corpus rows of every query row, exactly, in numpy -- the definition the device form is held to bit for bit.

    ``D(a, b)``: ``s = 0.0``; for ascending channel c: ``t = float64(a[c]) - float64(b[c])``; ``s = s + t * t`` (product rounded,
    then sum rounded: an explicit loop, because numpy's pairwise ``sum`` adds in another order).  Row i of the result holds the k
    eligible corpus rows with the smallest ``(D, j)``, ascending: distance first, corpus index second.  ``corpus=None``: the graph of
    the table against itself, ``exclude_self`` then defaults to True.  ``exclude_self`` drops corpus row ``j == i`` by index (an
    exact duplicate elsewhere stays, at distance 0.0).  A corpus row with a NaN or an infinity is never returned; a query row with
    one gets indices -1 and distances NaN; slots beyond the eligible rows are index -1, distance +inf."""
    a = _table(queries, "queries")
    b = a if corpus is None else _table(corpus, "corpus")
    exclude_self = check_neighbour_arguments(a.shape[0], b.shape[0], a.shape[1], b.shape[1], k, corpus is not None, exclude_self)
    q, n, c = a.shape[0], b.shape[0], a.shape[1]
    k = int(k)
    q_bad = ~np.isfinite(a).all(axis=1)
    b_bad = ~np.isfinite(b).all(axis=1)
    indices = np.full((q, k), -1, np.int32)
    dist = np.full((q, k), np.inf, np.float64)
    b64 = np.where(b_bad[:, None], 0.0, b.astype(np.float64))
    a64 = np.where(q_bad[:, None], 0.0, a.astype(np.float64))
    step = max(1, (1 << 24) // n)                            # query rows per piece: 128 MB of float64 distances
    for lo in range(0, q, step):
        hi = min(q, lo + step)
        d = np.zeros((hi - lo, n), np.float64)
        for ch in range(c):                                   # strictly ascending c, one rounding per product and per sum
            t = a64[lo:hi, ch, None] - b64[None, :, ch]
            d += t * t
        d[:, b_bad] = np.inf
        if exclude_self:
            d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        eligible = np.isfinite(d)                             # D of two finite float32 rows never overflows float64
        order = np.argsort(d, axis=1, kind="stable")[:, :k]   # stable: equal distances stay in index order
        picked = np.take_along_axis(d, order, axis=1)
        ok = np.take_along_axis(eligible, order, axis=1)
        kk = order.shape[1]
        indices[lo:hi, :kk] = np.where(ok, order, -1)
        dist[lo:hi, :kk] = np.where(ok, picked, np.inf)
    indices[q_bad] = -1
    dist[q_bad] = np.nan
    finite_rows = int(q - q_bad.sum())
    stats = {"query_rows": q, "certified_rows": 0, "exact_rows": finite_rows, "nonfinite_query_rows": int(q_bad.sum()),
             "nonfinite_corpus_rows": int(b_bad.sum())}
    return Neighbours(indices, dist, stats)


def duplicate_groups(neigh: Neighbours, radius: float) -> list[list[int]]:
    """Rows of a table's own neighbour graph (``neighbours(table)``) joined wherever ``sq_distance <= radius ** 2``: the connected
    groups with more than one member, each ascending, ordered by their first row -- "which uploads are near-duplicates".  Host
    union-find.  Only pairs inside the graph's k are seen: a group of more than k + 1 mutual duplicates may come back in pieces."""
    idx, dist = np.asarray(neigh.indices), np.asarray(neigh.sq_distances)
    parent = list(range(idx.shape[0]))

    def find(i: int) -> int:
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    limit = float(radius) ** 2
    for i, j in zip(*np.nonzero((idx >= 0) & (dist <= limit))):
        other = int(idx[i, j])
        if other >= len(parent):
            raise ValueError("duplicate_groups needs the graph of a table against itself")
        ra, rb = find(int(i)), find(other)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups: dict[int, list[int]] = {}
    for i in range(len(parent)):
        groups.setdefault(find(i), []).append(i)
    return [g for _, g in sorted(groups.items()) if len(g) > 1]


def stack(results, which: str = "board_extractor"):
    """``process_images(..., embeddings=True)`` results -> ``(table, keys)``: the (N, C) float32 table of ``which`` ("board_extractor":
    one row per image, "classifier": 64 rows per image with a board) and the (N, 2) int32 ``(image, square)`` key of each row (square
    -1 for the extractor's rows).  Images without embeddings -- for "classifier": without a board -- are skipped."""
    if which not in ("board_extractor", "classifier"):
        raise ValueError(f"which must be 'board_extractor' or 'classifier', got {which!r}")
    rows, keys = [], []
    for i, res in enumerate(results):
        emb = getattr(res, "embeddings", None)
        part = getattr(emb, which, None) if emb is not None else None
        if part is None:
            continue
        part = np.asarray(part, dtype=np.float32)
        if which == "board_extractor":
            rows.append(part.reshape(1, -1))
            keys.append([(i, -1)])
        else:
            rows.append(part.reshape(part.shape[0], -1))
            keys.append([(i, s) for s in range(part.shape[0])])
    if not rows:
        return np.zeros((0, 0), np.float32), np.zeros((0, 2), np.int32)
    return np.concatenate(rows, axis=0), np.asarray([k for ks in keys for k in ks], dtype=np.int32).reshape(-1, 2)


# ---- PaCMAP: the definition (include/chessvision_hip.h: cv_pacmap_pairs, cv_pacmap_optimise) -----------------------------------------
# A READING of Wang, Huang, Rudin, Shaposhnik, "Understanding How Dimension Reduction Tools Work" (JMLR 2021) and of the defaults of
# the authors' ``pacmap`` package; no copy of the package is part of this project.  Where the reading departs from the package it says
# so: the neighbour candidates are exact (no annoy) and at most MAX_NEIGHBOURS of them, the random draws come from a counter-based
# generator (other numbers, the same distribution), the gradient is a gather in a fixed order (equal to the package's scatter up to the
# order of float32 sums), and the Adam bias powers are running products.  DESIGN.md section 4 "Embedding reduction".
PACMAP_MAX_NEIGHBOURS, PACMAP_MAX_MID_NEAR, PACMAP_MAX_FURTHER = 32, 16, 64      # csrc/pacmap.h
PACMAP_PCA_DIMS = 100
PACMAP_MID_NEAR_DRAWS = 6
PACMAP_MAX_DRAWS = 1 << 16               # draws of one point in one stream; never reached with the argument rules below
PACMAP_MAX_ROWS = 1 << 22                # kNeighbourMaxRows
PACMAP_ITERATIONS = 450
PACMAP_KIND_SHIFT = 28                   # an incidence entry: other point | kind << 28 (0 neighbour, 1 mid-near, 2 further)
_U64 = np.uint64


@dataclasses.dataclass
class PacmapPairs:
    """``neighbours`` (N, n_neighbors), ``mid_near`` (N, n_MN), ``further`` (N, n_FP): int32 partners of every point; ``stats``: the
    neighbour search's record plus ``mid_near_draws`` and ``further_draws`` (rejected draws included) and ``candidates`` (kc)."""
    neighbours: np.ndarray
    mid_near: np.ndarray
    further: np.ndarray
    stats: dict


@dataclasses.dataclass
class Reduction:
    """``coordinates`` (N, 2) float32; ``pairs``: the ``PacmapPairs`` they were optimised over; ``n_neighbors``; ``stats`` = pairs.stats."""
    coordinates: np.ndarray
    pairs: PacmapPairs
    n_neighbors: int
    stats: dict


def pacmap_mix(x) -> np.ndarray:
    """The splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    with np.errstate(over="ignore"):
        x = x + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
        return x ^ (x >> _U64(31))


def pacmap_key(seed: int, stream: int, i) -> np.ndarray:
    """``mix(seed ^ mix((stream << 40) | i))`` for an array of points i."""
    i = np.atleast_1d(np.asarray(i)).astype(np.uint64)
    return pacmap_mix(_U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ pacmap_mix(_U64(int(stream) << 40) | i))


def pacmap_draw(key, t, n: int) -> np.ndarray:
    """Draw number t of the points whose keys are given: ``((mix(key + t) >> 32) * n) >> 32``, an index in [0, n)."""
    with np.errstate(over="ignore"):
        x = pacmap_mix(np.asarray(key, np.uint64) + np.asarray(t, np.uint64))
        return (((x >> _U64(32)) * _U64(int(n))) >> _U64(32)).astype(np.int64)


def pacmap_default_neighbours(n: int) -> int:
    return 10 if n < 10000 else int(round(10 + 15 * (math.log10(n) - 4)))


def check_pacmap_arguments(n: int, n_neighbors=None, n_MN=None, n_FP=None) -> tuple[int, int, int, int]:
    """The argument rules both forms share -> ``(n_neighbors, n_MN, n_FP, kc)`` with the defaults filled in; kc is the number of
    exact candidates the scaled-distance choice looks at."""
    n = int(n)
    nn = pacmap_default_neighbours(n) if n_neighbors is None else int(n_neighbors)
    if not 1 <= nn <= PACMAP_MAX_NEIGHBOURS:
        raise ValueError(f"n_neighbors must be in [1, {PACMAP_MAX_NEIGHBOURS}], got {nn}" +
                         (f" (the default for {n} rows)" if n_neighbors is None else ""))
    nmn = int(round(0.5 * nn)) if n_MN is None else int(n_MN)
    nfp = int(round(2 * nn)) if n_FP is None else int(n_FP)
    if not 0 <= nmn <= PACMAP_MAX_MID_NEAR:
        raise ValueError(f"n_MN must be in [0, {PACMAP_MAX_MID_NEAR}], got {nmn}")
    if not 0 <= nfp <= PACMAP_MAX_FURTHER:
        raise ValueError(f"n_FP must be in [0, {PACMAP_MAX_FURTHER}], got {nfp}")
    least = max(7, PACMAP_MID_NEAR_DRAWS + nmn, nn + nfp + 1)
    if n < least:
        raise ValueError(f"n_neighbors={nn}, n_MN={nmn}, n_FP={nfp} need at least {least} rows, the table has {n}")
    if n > PACMAP_MAX_ROWS:
        raise ValueError(f"the table has {n} rows, the neighbour search takes at most {PACMAP_MAX_ROWS}")
    if 2 * n * (nn + nmn + nfp) >= 1 << 31:
        raise ValueError(f"{n} rows with {nn + nmn + nfp} pairs each: the incidence lists' int32 offsets overflow")
    return nn, nmn, nfp, min(nn + 50, MAX_NEIGHBOURS, n - 1)


def _finite_table(a, name: str) -> np.ndarray:
    a = _table(a, name)
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds a NaN or an infinity")
    return a


def _principal_axes(centred: np.ndarray, dims: int) -> np.ndarray:
    """(C, dims) float64: eigenvectors of the covariance by descending eigenvalue, each flipped so that its largest-magnitude
    component is positive."""
    cov = centred.T @ centred / max(1, centred.shape[0] - 1)
    w, v = np.linalg.eigh(cov)
    axes = v[:, np.argsort(-w, kind="stable")[:dims]]
    top = np.abs(axes).argmax(axis=0)
    return axes * np.where(axes[top, np.arange(axes.shape[1])] < 0, -1.0, 1.0)


def _pacmap_preprocess_fit(table) -> tuple[np.ndarray, dict]:
    """``pacmap_preprocess`` and the float64 parameters it used (``EmbeddingMap``'s ``projected``, ``channel_mean``, ``axes``,
    ``minimum``, ``maximum``), so that ``pacmap_preprocess_new`` can apply the same operations to other rows."""
    x = _finite_table(table, "table").astype(np.float64)
    par = {"projected": x.shape[1] > PACMAP_PCA_DIMS, "channels": x.shape[1], "axes": np.zeros((x.shape[1], 0), np.float64),
           "minimum": 0.0, "maximum": 0.0}
    if par["projected"]:
        par["channel_mean"] = x.mean(axis=0)
        x = x - par["channel_mean"]
        par["axes"] = _principal_axes(x, PACMAP_PCA_DIMS)
        x = x @ par["axes"]
    else:
        par["minimum"] = float(x.min())
        x = x - x.min()
        top = x.max()
        par["maximum"] = float(top)
        if top > 0:
            x = x / top
        par["channel_mean"] = x.mean(axis=0)
        x = x - par["channel_mean"]
    return np.ascontiguousarray(x, dtype=np.float32), par


def pacmap_preprocess(table) -> np.ndarray:
    """(N, C) -> float32 (N, C'): more than 100 channels are centred and projected onto the 100 leading principal axes; otherwise
    the table is shifted by its global minimum, divided by its global maximum (where that is not zero) and centred.  float64 on the
    host; the result is an INPUT of both forms, so nothing downstream depends on LAPACK's rounding."""
    return _pacmap_preprocess_fit(table)[0]


def _pacmap_init_fit(pre, projected: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``pacmap_init`` and what it used when not projected: the (C',) float64 mean of ``pre`` and the (C', 2) (one column for a
    one-channel table) float64 axes; both empty when projected."""
    x = _finite_table(pre, "pre").astype(np.float64)
    mean, axes = np.zeros(0, np.float64), np.zeros((x.shape[1], 0), np.float64)
    if not projected:
        mean = x.mean(axis=0)
        x = x - mean
        axes = _principal_axes(x, 2)
        x = x @ axes
    y = np.zeros((x.shape[0], 2), np.float64)
    y[:, :min(2, x.shape[1])] = 0.01 * x[:, :2]
    return y.astype(np.float32), mean, axes


def pacmap_init(pre, projected: bool = False) -> np.ndarray:
    """float32 (N, 2): 0.01 x the first two columns of ``pre`` when ``pacmap_preprocess`` projected (``projected=True``: the table had
    more than 100 channels), otherwise 0.01 x the two leading principal axes of ``pre`` by the same rule.  A one-channel table gets
    a zero second coordinate."""
    return _pacmap_init_fit(pre, projected)[0]


def _pacmap_sigma(d: np.ndarray) -> np.ndarray:
    """(rows,) float64 scale of every row of ascending candidate distances ``d`` (rows, kc): max(mean of sqrt(D) at candidate ranks
    3, 4, 5, 1e-10), summed in rank order; with three candidates or fewer the last one's sqrt(D)."""
    kc = d.shape[1]
    root = np.sqrt(d)
    if kc > 3:
        hi = min(kc, 6)
        s = root[:, 3].copy()
        for r in range(4, hi):
            s = s + root[:, r]
        sigma = s / float(hi - 3)
    else:
        sigma = root[:, kc - 1].copy()
    return np.maximum(sigma, 1e-10)


def _pacmap_scaled_choice(idx: np.ndarray, d: np.ndarray, nn: int, sigma: np.ndarray | None = None) -> np.ndarray:
    """Row i keeps the nn candidates with the smallest ``(D_ij / (sigma_i * sigma_j), j)``; sigma_i = ``_pacmap_sigma`` of the row's
    own candidates, sigma_j the same (a table against itself) or, where ``sigma`` is given, that array's entry j (new rows against
    a fitted basis)."""
    own = _pacmap_sigma(d)
    scaled = d / (own[:, None] * (own if sigma is None else sigma)[idx])
    order = np.lexsort((idx, scaled), axis=1)[:, :nn]
    return np.take_along_axis(idx, order, axis=1).astype(np.int32)


def _pacmap_draw_until(key, t, n: int, want: int, forbidden: np.ndarray, what: str) -> np.ndarray:
    """Every point draws until it holds ``want`` distinct indices that are not itself and not in its row of ``forbidden`` (N, F);
    ``t`` (N,) uint64, the points' draw counters, moves on.  -> held (N, want) int64, in the order drawn."""
    rows = key.shape[0]
    held = np.full((rows, want), -1, np.int64)
    count = np.zeros(rows, np.int64)
    while True:
        a = np.flatnonzero(count < want)
        if a.size == 0:
            return held
        if (t[a] >= _U64(PACMAP_MAX_DRAWS)).any():
            raise RuntimeError(f"pacmap: a point drew {PACMAP_MAX_DRAWS} {what} candidates without filling its list")
        j = pacmap_draw(key[a], t[a], n)
        t[a] += _U64(1)
        ok = (j != a) & ~(held[a] == j[:, None]).any(axis=1) & ~(forbidden[a] == j[:, None]).any(axis=1)
        sel = a[ok]
        held[sel, count[sel]] = j[ok]
        count[sel] += 1


def pacmap_pairs(pre, n_neighbors=None, n_MN=None, n_FP=None, seed: int = 0) -> PacmapPairs:
    """The three pair sets of a preprocessed table, in numpy -- the definition the device form is held to exactly.

    Neighbours: the exact graph of ``pre`` (``neighbours``, kc = min(n_neighbors + 50, 64, N - 1) candidates) re-ranked by the
    scaled distance.  Mid-near (stream 1), slot by slot: draw until six distinct indices are held that are neither i nor an earlier
    mid-near partner of i; the partner is the SECOND smallest by ``(D(i, .), j)``.  Further (stream 2): draw until n_FP distinct
    indices are held that are neither i nor in i's neighbour row.  Draw t of point i in a stream is ``pacmap_draw(pacmap_key(seed,
    stream, i), t, N)``; t counts every draw, rejected ones included."""
    return _pacmap_pairs_sigma(pre, n_neighbors, n_MN, n_FP, seed)[0]


def _pacmap_pairs_sigma(pre, n_neighbors=None, n_MN=None, n_FP=None, seed: int = 0) -> tuple[PacmapPairs, np.ndarray]:
    """``pacmap_pairs`` and the (N,) float64 scale of every row that its neighbour choice used (``EmbeddingMap.sigma``)."""
    x = _finite_table(pre, "pre")
    n = x.shape[0]
    nn, nmn, nfp, kc = check_pacmap_arguments(n, n_neighbors, n_MN, n_FP)
    graph = neighbours(x, k=kc)
    nbr = _pacmap_scaled_choice(graph.indices.astype(np.int64), graph.sq_distances, nn)

    x64 = x.astype(np.float64)
    rows = np.arange(n)
    key = pacmap_key(seed, 1, rows)
    t = np.zeros(n, np.uint64)
    mid = np.full((n, nmn), -1, np.int64)
    for slot in range(nmn):
        held = _pacmap_draw_until(key, t, n, PACMAP_MID_NEAR_DRAWS, mid[:, :slot], "mid-near")
        d = np.zeros(held.shape, np.float64)
        for ch in range(x.shape[1]):                          # D of neighbours(): ascending channel, product and sum each rounded
            diff = x64[:, ch, None] - x64[held, ch]
            d += diff * diff
        mid[:, slot] = held[rows, np.lexsort((held, d), axis=1)[:, 1]]
    mid_draws = int(t.sum())

    t = np.zeros(n, np.uint64)
    far = _pacmap_draw_until(pacmap_key(seed, 2, rows), t, n, nfp, nbr, "further")
    stats = dict(graph.stats, candidates=kc, mid_near_draws=mid_draws, further_draws=int(t.sum()))
    return PacmapPairs(nbr, mid.astype(np.int32), far.astype(np.int32), stats), _pacmap_sigma(graph.sq_distances)


def pacmap_incidence(pairs: PacmapPairs, mid_near: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """The incident entries of every point as a CSR structure -> ``(offsets (N + 1,) int32, entries int32)``, an entry being
    ``other | kind << 28``.  Point p's list: its own neighbour pairs by slot, its own mid-near pairs, its own further pairs, then the
    entries where p is another point's partner, ordered by (kind, source point, slot).  ``mid_near=False`` leaves the mid-near
    entries out and keeps the order of the rest (the lists of iterations 200 and later)."""
    kinds = [np.asarray(pairs.neighbours), np.asarray(pairs.mid_near), np.asarray(pairs.further)]
    if not mid_near:
        kinds[1] = kinds[1][:, :0]
    n = kinds[0].shape[0]
    own = np.concatenate([a.astype(np.int64) | (k << PACMAP_KIND_SHIFT) for k, a in enumerate(kinds)], axis=1)
    per = own.shape[1]
    dst = np.concatenate([a.astype(np.int64).ravel() for a in kinds])                  # (kind, source, slot) order already
    src = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), a.shape[1]) | (k << PACMAP_KIND_SHIFT) for k, a in enumerate(kinds)])
    if dst.size and (dst.min() < 0 or dst.max() >= n):
        raise ValueError("pacmap_incidence: a partner index lies outside the table")
    order = np.argsort(dst, kind="stable")
    incoming = np.bincount(dst, minlength=n)
    offsets = np.concatenate([[0], np.cumsum(per + incoming)])
    if offsets[-1] >= 1 << 31:
        raise ValueError("pacmap_incidence: the int32 offsets overflow")
    entries = np.empty(int(offsets[-1]), np.int32)
    entries[(offsets[:-1, None] + np.arange(per)).ravel()] = own.ravel()
    first = np.cumsum(incoming) - incoming
    at = dst[order]
    entries[offsets[:-1][at] + per + np.arange(dst.size) - first[at]] = src[order]
    return offsets.astype(np.int32), entries


def pacmap_schedule(iterations: int = PACMAP_ITERATIONS) -> np.ndarray:
    """(iterations, 4) float32 rows ``(lr_t, w_n, w_MN, w_FP)``: float64 on the host, rounded once.  ``lr_t = sqrt(1 - b2) / (1 - b1)``
    with b1 = 0.9^(it+1) and b2 = 0.999^(it+1) as running products (``b *= beta`` per iteration: the same bits in every language)."""
    out = np.empty((int(iterations), 4), np.float64)
    b1 = b2 = 1.0
    for it in range(int(iterations)):
        b1 *= 0.9
        b2 *= 0.999
        if it < 100:
            w = (2.0, (1.0 - it / 100.0) * 1000.0 + (it / 100.0) * 3.0, 1.0)
        elif it < 200:
            w = (3.0, 3.0, 1.0)
        else:
            w = (1.0, 0.0, 1.0)
        out[it] = (math.sqrt(1.0 - b2) / (1.0 - b1),) + w
    return out.astype(np.float32)


class _PacmapWalk:
    """The incidence lists laid out for numpy: points sorted by descending list length, so that the points that still have an entry
    at position ``pos`` are a prefix, and per position the other point, the kind and the kind's constants of every such point."""

    def __init__(self, offsets: np.ndarray, entries: np.ndarray):
        f32 = np.float32
        lens = np.diff(offsets.astype(np.int64))
        self.perm = np.argsort(-lens, kind="stable")
        sorted_lens = lens[self.perm]
        start = offsets.astype(np.int64)[self.perm]
        add = np.array([10.0, 10000.0, 1.0], f32)
        num = np.array([20.0, 20000.0, 2.0], f32)
        sign = np.array([1.0, 1.0, -1.0], f32)
        self.steps = []
        for pos in range(int(sorted_lens.max()) if lens.size else 0):
            r = int(np.searchsorted(-sorted_lens, -pos, side="left"))     # points with more than pos entries
            e = entries[start[:r] + pos]
            kind = e >> PACMAP_KIND_SHIFT
            self.steps.append((r, e & ((1 << PACMAP_KIND_SHIFT) - 1), kind, add[kind], num[kind], sign[kind]))

    def gradient(self, y: np.ndarray, weights) -> np.ndarray:
        """(N, 2) float32 gradient of every point at coordinates y, every operation rounded once to float32, entries in list order."""
        f32 = np.float32
        wk = np.asarray(weights, f32)
        ys = y[self.perm]
        y0, y1, s0, s1 = y[:, 0], y[:, 1], ys[:, 0].copy(), ys[:, 1].copy()
        g0, g1 = np.zeros(y.shape[0], f32), np.zeros(y.shape[0], f32)
        for r, other, kind, add, num, sign in self.steps:
            e0 = s0[:r] - y0[other]
            e1 = s1[:r] - y1[other]
            d = f32(1.0) + e0 * e0
            d = d + e1 * e1
            t = add + d
            w = wk[kind] * (num / (t * t))
            g0[:r] = g0[:r] + sign * (w * e0)                 # g - x and g + (-x) are the same float32
            g1[:r] = g1[:r] + sign * (w * e1)
        g = np.empty_like(y)
        g[self.perm, 0], g[self.perm, 1] = g0, g1
        return g


def pacmap_trajectory(init, pairs: PacmapPairs, keep=(PACMAP_ITERATIONS,)) -> dict:
    """``{iterations: coordinates}`` for every count in ``keep``, from ONE run of max(keep) iterations: the state after k iterations
    does not depend on how many follow.  ``pacmap_optimise`` is the last of them."""
    y = np.ascontiguousarray(np.asarray(init, np.float32)).copy()
    n = np.asarray(pairs.neighbours).shape[0]
    if y.shape != (n, 2) or not np.isfinite(y).all():
        raise ValueError(f"init must be a finite ({n}, 2) array, got shape {y.shape}")
    keep = sorted(int(k) for k in keep)
    if not keep or keep[0] < 0:
        raise ValueError("iteration counts must be non-negative")
    f32 = np.float32
    schedule = pacmap_schedule(keep[-1])
    c1, c2, eps = f32(1.0 - 0.9), f32(1.0 - 0.999), f32(1e-7)
    m, v = np.zeros_like(y), np.zeros_like(y)
    walks = {}
    out = {0: y.copy()} if keep[0] == 0 else {}
    with np.errstate(all="ignore"):
        for it in range(keep[-1]):
            lr, w_n, w_mn, w_fp = schedule[it]
            with_mid = it < 200
            if with_mid not in walks:
                walks[with_mid] = _PacmapWalk(*pacmap_incidence(pairs, with_mid))
            g = walks[with_mid].gradient(y, (w_n, w_mn, w_fp))
            m = m + c1 * (g - m)
            v = v + c2 * (g * g - v)
            y = y - (lr * m) / (np.sqrt(v) + eps)
            if it + 1 in keep:
                out[it + 1] = y.copy()
    return out


def pacmap_optimise(init, pairs: PacmapPairs, iterations: int = PACMAP_ITERATIONS) -> np.ndarray:
    """(N, 2) float32 coordinates after ``iterations`` Adam steps from ``init`` -- the definition the device form is held to bit for
    bit.  Per iteration every point gathers over its incidence list (``pacmap_incidence``) at the PREVIOUS iteration's coordinates:

        e = Y[p] - Y[q];  d = 1;  d = d + e0*e0;  d = d + e1*e1
        neighbour:  t = 10 + d;     w = w_n  * (20    / (t*t));  g = g + w*e
        mid-near:   t = 10000 + d;  w = w_MN * (20000 / (t*t));  g = g + w*e        (left out from iteration 200 on, w_MN = 0)
        further:    t = 1 + d;      w = w_FP * (2     / (t*t));  g = g - w*e
        m = m + c1*(g - m);  v = v + c2*(g*g - v);  Y = Y - (lr_t*m) / (sqrt(v) + 1e-7)

    in float32, one rounding per operation; ``pacmap_schedule`` holds lr_t and the weights."""
    return pacmap_trajectory(init, pairs, (int(iterations),))[int(iterations)]


def pacmap(table, n_neighbors=None, n_MN=None, n_FP=None, seed: int = 0, init="pca", iterations: int = PACMAP_ITERATIONS) -> Reduction:
    """The whole reduction in numpy: preprocess, pairs, initialise (``init="pca"`` or an (N, 2) array), optimise."""
    return pacmap_fit(table, n_neighbors, n_MN, n_FP, seed, init, iterations).reduction


def pacmap_fit_inputs(table, init="pca") -> tuple[np.ndarray, np.ndarray, dict]:
    """``(pre, start, parameters)``: the two host arrays both forms start from, and the float64 parameters of the preprocessing and
    of the "pca" start that ``map_from_fit`` stores."""
    x = _finite_table(table, "table")
    pre, par = _pacmap_preprocess_fit(x)
    pca, par["start_mean"], par["start_axes"] = _pacmap_init_fit(pre, projected=par["projected"])
    if isinstance(init, str):
        if init != "pca":
            raise ValueError(f"init must be 'pca' or an (N, 2) array, got {init!r}")
        return pre, pca, par
    start = np.ascontiguousarray(np.asarray(init.detach().cpu() if hasattr(init, "detach") else init), dtype=np.float32)
    if start.shape != (x.shape[0], 2) or not np.isfinite(start).all():
        raise ValueError(f"init must be 'pca' or a finite ({x.shape[0]}, 2) array, got shape {start.shape}")
    return pre, start, par


def pacmap_inputs(table, init="pca") -> tuple[np.ndarray, np.ndarray]:
    """``(pre, start)``: the two host arrays both forms start from."""
    return pacmap_fit_inputs(table, init)[:2]


# ---- placing new rows into a fitted map (include/chessvision_hip.h: cv_pacmap_basis_scale, cv_pacmap_place_pairs, cv_pacmap_place) ----
# Again a READING, of the ``pacmap`` package's ``transform``: pairs from every new point to its nearest basis points by the scaled
# distance, the attraction term alone, the basis held still, the same 450-step schedule.  Where it departs from the package: the
# neighbour candidates are exact and at most MAX_NEIGHBOURS of them, and the Adam bias powers are running products.  DESIGN.md section 4
# "Placing new points".
@dataclasses.dataclass
class EmbeddingMap:
    """A fitted map, everything ``pacmap_transform`` needs to place other rows into it.  ``reduction``: the ``Reduction`` of the
    basis; ``pre`` (N, C') float32: the preprocessed basis, exactly the array the fit used; ``sigma`` (N,) float64: the basis rows'
    scale in the neighbour choice.  The preprocessing, float64: ``projected``, ``channels`` (C of the fitted table),
    ``channel_mean`` (C,) -- of the table when projected, of the shifted and scaled table otherwise --, ``axes`` (C, 100) when
    projected ((C, 0) otherwise), ``minimum`` and ``maximum``: the table's global minimum and its global maximum after the shift
    (0.0 when projected).  The "pca" start when not projected: ``start_mean`` (C',), the mean of ``pre``, and ``start_axes`` (C', 2)
    ((C', 1) for a one-channel table); both empty when projected."""
    reduction: Reduction
    pre: np.ndarray
    sigma: np.ndarray
    projected: bool
    channels: int
    channel_mean: np.ndarray
    axes: np.ndarray
    minimum: float
    maximum: float
    start_mean: np.ndarray
    start_axes: np.ndarray


@dataclasses.dataclass
class Placement:
    """``coordinates`` (Q, 2) float32 of the new rows in the map; ``neighbours`` (Q, n_neighbors) int32: the basis rows each was
    pulled towards; ``stats``: the neighbour search's record plus ``candidates`` (kc)."""
    coordinates: np.ndarray
    neighbours: np.ndarray
    stats: dict


def map_from_fit(reduction: Reduction, pre: np.ndarray, sigma: np.ndarray, parameters: dict) -> EmbeddingMap:
    """The ``EmbeddingMap`` of a fit from its parts (``parameters``: the dict of ``pacmap_fit_inputs``)."""
    return EmbeddingMap(reduction, pre, np.ascontiguousarray(sigma, dtype=np.float64), **parameters)


def pacmap_fit(table, n_neighbors=None, n_MN=None, n_FP=None, seed: int = 0, init="pca",
               iterations: int = PACMAP_ITERATIONS) -> EmbeddingMap:
    """``pacmap`` that keeps what placing needs: ``pacmap_fit(t).reduction`` IS ``pacmap(t)``."""
    pre, start, par = pacmap_fit_inputs(table, init)
    pairs, sigma = _pacmap_pairs_sigma(pre, n_neighbors, n_MN, n_FP, seed)
    coords = pacmap_optimise(start, pairs, iterations)
    return map_from_fit(Reduction(coords, pairs, int(pairs.neighbours.shape[1]), pairs.stats), pre, sigma, par)


def pacmap_preprocess_new(map: EmbeddingMap, table) -> np.ndarray:
    """(Q, C) rows of the kind the map was fitted on -> float32 (Q, C'): the float64 operations of ``pacmap_preprocess`` with the
    map's stored parameters (a global maximum of zero is not divided by, as in the fit).  Like ``map.pre`` an INPUT of both forms."""
    x = _finite_table(table, "table").astype(np.float64)
    if x.shape[1] != map.channels:
        raise ValueError(f"table has {x.shape[1]} channels, the map was fitted on {map.channels}")
    if map.projected:
        x = x - map.channel_mean
        x = x @ map.axes
    else:
        x = x - map.minimum
        if map.maximum > 0:
            x = x / map.maximum
        x = x - map.channel_mean
    return np.ascontiguousarray(x, dtype=np.float32)


def check_pacmap_place_arguments(q: int, n: int, c_new: int, c: int, n_neighbors: int) -> int:
    """The argument rules both forms of the placement share -> kc, the number of exact candidates of a new row."""
    if c_new != c:
        raise ValueError(f"the new rows have {c_new} channels, the map's basis {c}")
    if not 1 <= q <= PACMAP_MAX_ROWS:
        raise ValueError(f"between 1 and {PACMAP_MAX_ROWS} new rows can be placed at once, got {q}")
    if not 1 <= n_neighbors <= PACMAP_MAX_NEIGHBOURS or n < max(7, n_neighbors + 1) or n > PACMAP_MAX_ROWS:
        raise ValueError(f"a map of {n} rows with n_neighbors={n_neighbors} is outside what pacmap fits")
    return min(n_neighbors + 50, MAX_NEIGHBOURS, n)


def _place_tables(map: EmbeddingMap, pre_new) -> tuple[np.ndarray, int, int]:
    x = _finite_table(pre_new, "pre_new")
    nn = int(map.reduction.n_neighbors)
    return x, nn, check_pacmap_place_arguments(x.shape[0], map.pre.shape[0], x.shape[1], map.pre.shape[1], nn)


def _pacmap_place_pairs(map: EmbeddingMap, pre_new) -> tuple[np.ndarray, dict]:
    x, nn, kc = _place_tables(map, pre_new)
    graph = neighbours(x, corpus=map.pre, k=kc, exclude_self=False)
    nbr = _pacmap_scaled_choice(graph.indices.astype(np.int64), graph.sq_distances, nn, sigma=np.asarray(map.sigma, np.float64))
    return nbr, dict(graph.stats, candidates=kc)


def pacmap_place_pairs(map: EmbeddingMap, pre_new) -> np.ndarray:
    """(Q, n_neighbors) int32, the basis rows every new row is pulled towards -- the definition the device form is held to index for
    index.  Candidates: the kc = min(n_neighbors + 50, 64, N) exact nearest basis rows (``neighbours(pre_new, corpus=map.pre)``, no
    row excluded).  sigma_q of a new row: the fit's rule on its own candidates (max(mean of sqrt(D) at ranks 3, 4, 5, 1e-10)); the
    row keeps the n_neighbors candidates with the smallest ``(D_qj / (sigma_q * map.sigma[j]), j)``, ascending."""
    return _pacmap_place_pairs(map, pre_new)[0]


def pacmap_place_init(map: EmbeddingMap, pre_new) -> np.ndarray:
    """float32 (Q, 2): the fit's "pca" start evaluated at the new rows -- 0.01 x the first two columns when the map projected,
    otherwise 0.01 x ``(pre_new - map.start_mean) @ map.start_axes``."""
    x = _place_tables(map, pre_new)[0].astype(np.float64)
    if not map.projected:
        x = x - map.start_mean
        x = x @ map.start_axes
    y = np.zeros((x.shape[0], 2), np.float64)
    y[:, :min(2, x.shape[1])] = 0.01 * x[:, :2]
    return y.astype(np.float32)


def check_pacmap_place_inputs(init, basis_coordinates, pairs) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(init (Q, 2) float32, basis (N, 2) float32, pairs (Q, nn) int32)`` of a placement as dense host arrays, shapes checked."""
    host = lambda a: np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    y = np.ascontiguousarray(host(init), dtype=np.float32)
    yb = np.ascontiguousarray(host(basis_coordinates), dtype=np.float32)
    p = np.ascontiguousarray(host(pairs), dtype=np.int32)
    if p.ndim != 2 or not 1 <= p.shape[1] <= PACMAP_MAX_NEIGHBOURS or not 1 <= p.shape[0] <= PACMAP_MAX_ROWS:
        raise ValueError(f"pairs must be a (Q, n_neighbors) table with Q >= 1 and 1 <= n_neighbors <= {PACMAP_MAX_NEIGHBOURS}, "
                         f"got shape {p.shape}")
    if y.shape != (p.shape[0], 2) or not np.isfinite(y).all():
        raise ValueError(f"init must be a finite ({p.shape[0]}, 2) array, got shape {y.shape}")
    if yb.ndim != 2 or yb.shape[1] != 2 or not 1 <= yb.shape[0] <= PACMAP_MAX_ROWS or not np.isfinite(yb).all():
        raise ValueError(f"basis_coordinates must be a finite (N, 2) array, got shape {yb.shape}")
    return y, yb, p


def pacmap_place_trajectory(init, basis_coordinates, pairs, keep=(PACMAP_ITERATIONS,)) -> dict:
    """``{iterations: coordinates}`` for every count in ``keep``, from ONE run of max(keep) iterations of ``pacmap_place``."""
    y, yb, p = check_pacmap_place_inputs(init, basis_coordinates, pairs)
    y = y.copy()
    keep = sorted(int(k) for k in keep)
    if not keep or keep[0] < 0:
        raise ValueError("iteration counts must be non-negative")
    f32 = np.float32
    live = (p >= 0) & (p < yb.shape[0])
    at = np.where(live, p, 0)
    b0, b1 = yb[at, 0], yb[at, 1]                             # (Q, nn): the partners' coordinates never move
    schedule = pacmap_schedule(keep[-1])
    c1, c2, eps, one, ten, twenty = f32(1.0 - 0.9), f32(1.0 - 0.999), f32(1e-7), f32(1.0), f32(10.0), f32(20.0)
    m, v = np.zeros_like(y), np.zeros_like(y)
    out = {0: y.copy()} if keep[0] == 0 else {}
    with np.errstate(all="ignore"):
        for it in range(keep[-1]):
            lr, w_n = schedule[it, 0], schedule[it, 1]
            g = np.zeros_like(y)
            for u in range(p.shape[1]):                       # slots in order, every operation rounded once to float32
                e0 = y[:, 0] - b0[:, u]
                e1 = y[:, 1] - b1[:, u]
                d = one + e0 * e0
                d = d + e1 * e1
                t = ten + d
                w = w_n * (twenty / (t * t))
                g[:, 0] = np.where(live[:, u], g[:, 0] + w * e0, g[:, 0])
                g[:, 1] = np.where(live[:, u], g[:, 1] + w * e1, g[:, 1])
            m = m + c1 * (g - m)
            v = v + c2 * (g * g - v)
            y = y - (lr * m) / (np.sqrt(v) + eps)
            if it + 1 in keep:
                out[it + 1] = y.copy()
    return out


def pacmap_place(init, basis_coordinates, pairs, iterations: int = PACMAP_ITERATIONS) -> np.ndarray:
    """(Q, 2) float32 coordinates of the new points after ``iterations`` Adam steps from ``init`` -- the definition the device form
    is held to bit for bit.  ``basis_coordinates`` (N, 2): the fitted map, held still; ``pairs`` (Q, nn) int32: every new point's
    partners in it (``pacmap_place_pairs``).  Per iteration and new point p, with Yb the basis coordinates:

        g = 0;  for slot u in order (a partner outside [0, N) is skipped):
            e = Y[p] - Yb[b_u];  d = 1;  d = d + e0*e0;  d = d + e1*e1;  t = 10 + d;  w = w_n * (20 / (t*t));  g = g + w*e
        m = m + c1*(g - m);  v = v + c2*(g*g - v);  Y[p] = Y[p] - (lr_t*m) / (sqrt(v) + 1e-7)

    in float32, one rounding per operation; lr_t and w_n are columns 0 and 1 of ``pacmap_schedule`` (2, then 3, then 1).  No
    mid-near and no further term: a new point is only pulled.  No new point reads another, so a batch equals its rows placed one
    at a time, bit for bit."""
    return pacmap_place_trajectory(init, basis_coordinates, pairs, (int(iterations),))[int(iterations)]


def pacmap_transform_inputs(map: EmbeddingMap, table, init="pca") -> tuple[np.ndarray, np.ndarray]:
    """``(pre_new, start)``: the two host arrays both forms of the placement start from."""
    pre_new = pacmap_preprocess_new(map, table)
    _place_tables(map, pre_new)
    if isinstance(init, str):
        if init != "pca":
            raise ValueError(f"init must be 'pca' or a (Q, 2) array, got {init!r}")
        return pre_new, pacmap_place_init(map, pre_new)
    start = np.ascontiguousarray(np.asarray(init.detach().cpu() if hasattr(init, "detach") else init), dtype=np.float32)
    if start.shape != (pre_new.shape[0], 2) or not np.isfinite(start).all():
        raise ValueError(f"init must be 'pca' or a finite ({pre_new.shape[0]}, 2) array, got shape {start.shape}")
    return pre_new, start


def pacmap_transform(map: EmbeddingMap, table, init="pca", iterations: int = PACMAP_ITERATIONS) -> Placement:
    """The whole placement in numpy: preprocess with the map's parameters, pairs into the basis, initialise, place."""
    pre_new, start = pacmap_transform_inputs(map, table, init)
    nbr, stats = _pacmap_place_pairs(map, pre_new)
    return Placement(pacmap_place(start, map.reduction.coordinates, nbr, iterations), nbr, stats)


_MAP_ARRAYS = ("pre", "sigma", "channel_mean", "axes", "start_mean", "start_axes")
_PAIR_ARRAYS = ("neighbours", "mid_near", "further")


def save_map(path, map: EmbeddingMap) -> None:
    """One ``.npz`` of arrays and scalars (no pickle), written to exactly ``path``; ``load_map`` reproduces every array bit for bit."""
    keys = sorted(map.reduction.stats)
    content = {name: np.asarray(getattr(map, name)) for name in _MAP_ARRAYS}
    content.update({name: np.asarray(getattr(map.reduction.pairs, name)) for name in _PAIR_ARRAYS})
    content.update(coordinates=np.asarray(map.reduction.coordinates), n_neighbors=np.int64(map.reduction.n_neighbors),
                   projected=np.bool_(map.projected), channels=np.int64(map.channels), minimum=np.float64(map.minimum),
                   maximum=np.float64(map.maximum), stats_keys=np.asarray(keys, dtype=np.str_),
                   stats_values=np.asarray([int(map.reduction.stats[k]) for k in keys], dtype=np.int64), format=np.int64(1))
    with open(path, "wb") as f:
        np.savez(f, **content)


def load_map(path) -> EmbeddingMap:
    """The ``EmbeddingMap`` that ``save_map`` wrote."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != 1:
            raise ValueError(f"{path} is not an embedding map of this version")
        stats = {str(k): int(v) for k, v in zip(z["stats_keys"], z["stats_values"])}
        pairs = PacmapPairs(*(z[name] for name in _PAIR_ARRAYS), stats)
        reduction = Reduction(z["coordinates"], pairs, int(z["n_neighbors"]), stats)
        return EmbeddingMap(reduction, z["pre"], z["sigma"], bool(z["projected"]), int(z["channels"]), z["channel_mean"], z["axes"],
                            float(z["minimum"]), float(z["maximum"]), z["start_mean"], z["start_axes"])


