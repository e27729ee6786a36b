"""Tables, shapes and reference results that tests/test_pacmap_cpu.py, tests/test_gpu_pacmap.py and tests/test_gpu_pacmap_stream.py
share.  Every table comes from a seed; the numpy form of a case (``reference``) is computed once per process and handed out read-only.

The shapes are the smallest at which each path can go wrong: the least table the argument rules admit (7 x 1, kc = N - 1 = 6), a table
of more than one wave of points (65 x 3), 100 channels (the widest table that is NOT projected) and 513 (projected), one point that is
the neighbour of hundreds (the shell; with n_neighbors = 16 the centre is kept by 243 of the 256: an incoming list much longer than
any own list), rows all equal (sigma at its clamp, every distance a tie, all coordinates zero), exact duplicates among distinct rows,
the largest admitted n_neighbors and n_FP at their least N (kc = 64), and both sides of the N = 10000 step of the default n_neighbors
(pairs only)."""
from __future__ import annotations

import dataclasses

import numpy as np

from chessvision import embeddings

SNAPSHOTS = (1, 100, 200, 450)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    kind: str
    n: int
    c: int
    n_neighbors: int | None = None
    n_MN: int | None = None
    n_FP: int | None = None
    seed: int = 0
    optimise: bool = True


def clusters(n: int, c: int, seed: int, count: int = 13) -> tuple[np.ndarray, np.ndarray]:
    """``count`` Gaussian clusters: unit-normal centres, unit-normal noise around them (the noise as wide as the centres are apart per
    channel) -> (table float32, labels)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((count, c))
    labels = rng.integers(0, count, n)
    return (centres[labels] + rng.standard_normal((n, c))).astype(np.float32), labels


def purity(coords: np.ndarray, labels: np.ndarray) -> float:
    """Leave-one-out 1-NN label purity: the share of points whose nearest other point in the map carries their label."""
    y = coords.astype(np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(1)] == labels).mean())


def table(case: Case) -> np.ndarray:
    rng = np.random.default_rng(case.seed + 77)
    n, c = case.n, case.c
    if case.kind == "iid":
        return rng.standard_normal((n, c)).astype(np.float32)
    if case.kind == "clusters":
        return clusters(n, c, case.seed)[0]
    if case.kind == "shell":                                  # row 0 the centre, the rest on the unit sphere around it
        x = rng.standard_normal((n, c))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x[0] = 0.0
        return (x + 3.0).astype(np.float32)
    if case.kind == "equal":
        return np.full((n, c), 0.625, np.float32)
    if case.kind == "duplicates":                             # 40 rows are exact copies of row 0
        x = np.maximum(rng.standard_normal((n, c)), 0.0).astype(np.float32)
        x[rng.permutation(n)[:40]] = x[0]
        return x
    raise ValueError(case.kind)


CASES = [
    Case("least-7x1", "iid", 7, 1, n_neighbors=2),                                        # n_MN 1, n_FP 4, kc = N - 1 = 6
    Case("iid-65x3", "iid", 65, 3),                                                       # kc = 60
    Case("clusters-300x100", "clusters", 300, 100),
    Case("projected-300x513", "clusters", 300, 513),
    Case("shell-257x8", "shell", 257, 8, n_neighbors=16),                                 # the centre: 243 incoming neighbour entries
    Case("equal-64x4", "equal", 64, 4),
    Case("duplicates-2048x32", "duplicates", 2048, 32),
    Case("widest-97x5", "iid", 97, 5, n_neighbors=32, n_MN=16, n_FP=64, seed=3),          # the least N for 32 / 16 / 64; kc = 64
    Case("below-step-9999x16", "iid", 9999, 16, optimise=False),
    Case("at-step-10000x16", "iid", 10000, 16, optimise=False),
]
BY_ID = {c.id: c for c in CASES}

_REFERENCE: dict = {}


def reference(case: Case) -> dict:
    """``pre``, ``init``, ``pairs`` and (where the case optimises) ``coords`` = {iterations: (N, 2)} of the numpy form, read-only."""
    if case.id not in _REFERENCE:
        pre, init = embeddings.pacmap_inputs(table(case))
        pairs = embeddings.pacmap_pairs(pre, case.n_neighbors, case.n_MN, case.n_FP, case.seed)
        coords = embeddings.pacmap_trajectory(init, pairs, SNAPSHOTS) if case.optimise else {}
        for a in (pre, init, pairs.neighbours, pairs.mid_near, pairs.further, *coords.values()):
            a.setflags(write=False)
        _REFERENCE[case.id] = {"pre": pre, "init": init, "pairs": pairs, "coords": coords}
    return _REFERENCE[case.id]
