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
(``process_pipeline.py:351``, ``train_classifier.py:312``).  The PaCMAP reduction itself stays out of scope; the exact k-nearest-
neighbour graph it (and UMAP) starts from is served: ``neighbours`` here is the definition and the checker in numpy,
``HipEngine.embedding_neighbours`` / ``ChessVision.embedding_neighbours`` the device form, equal to it bit for bit.  ``stack`` turns
``process_images(..., embeddings=True)`` results into the table, ``duplicate_groups`` answers "which uploads are near-duplicates".
"""
from __future__ import annotations

import dataclasses

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
