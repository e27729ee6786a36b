"""Fitted maps, new rows and reference placements that tests/test_pacmap_place_cpu.py, tests/test_gpu_pacmap_place.py and
tests/test_gpu_pacmap_place_stream.py share.  Every table comes from a seed; the numpy form of a case (``reference``) is computed once
per process and handed out read-only.

The shapes are the smallest at which each path can go wrong: one new row over the least basis the fit admits (kc = N = 7: every basis
row is a candidate, one lane); a full wave of new rows, and one more (one lane in a second workgroup); n_neighbors = 32 (the on-chip
partner store at its limit, kc = 64); held-out rows of the two cluster tables (unprojected preprocessing with the stored minimum,
maximum and mean; projected with the stored mean and axes); rows all equal (sigma at its clamp, every scaled distance a tie, a zero
maximum that is not divided by); and exact copies of basis rows and of each other (D = 0 candidates)."""
from __future__ import annotations

import dataclasses

import numpy as np

import pacmap_cases as pc
from chessvision import embeddings

SNAPSHOTS = pc.SNAPSHOTS
HELD_OUT = 64                                   # of the 364 rows of a cluster table; the first 300 are the basis


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    basis: str                                  # a case of pacmap_cases, or "clusters" / "projected": the 364-row tables below
    q: int
    kind: str = "iid"


CASES = [
    Case("least-7x1-q1", "least-7x1", 1),
    Case("wave-edge-65x3-q64", "iid-65x3", 64),
    Case("wave-edge-65x3-q65", "iid-65x3", 65),
    Case("widest-97x5-q3", "widest-97x5", 3),
    Case("clusters-300x100-q64", "clusters", HELD_OUT, "held-out"),
    Case("projected-300x513-q64", "projected", HELD_OUT, "held-out"),
    Case("equal-64x4-q6", "equal-64x4", 6, "equal"),
    Case("copies-2048x32-q56", "duplicates-2048x32", 56, "copies"),
]
BY_ID = {c.id: c for c in CASES}
CLUSTER_CHANNELS = {"clusters": 100, "projected": 513}

_MAPS: dict = {}
_REFERENCE: dict = {}


def cluster_table(basis: str) -> tuple[np.ndarray, np.ndarray]:
    """The 364-row table and its labels; rows [:300] are the basis, rows [300:] the held-out rows."""
    return pc.clusters(300 + HELD_OUT, CLUSTER_CHANNELS[basis], 0)


def basis_table(basis: str) -> np.ndarray:
    return cluster_table(basis)[0][:300] if basis in CLUSTER_CHANNELS else pc.table(pc.BY_ID[basis])


def fitted(basis: str) -> embeddings.EmbeddingMap:
    """The numpy fit over a basis, once per process, its arrays read-only."""
    if basis not in _MAPS:
        fit = pc.BY_ID.get(basis, pc.Case(basis, "clusters", 300, CLUSTER_CHANNELS.get(basis, 0)))
        m = embeddings.pacmap_fit(basis_table(basis), fit.n_neighbors, fit.n_MN, fit.n_FP, fit.seed)
        for a in (m.pre, m.sigma, m.reduction.coordinates, m.reduction.pairs.neighbours):
            a.setflags(write=False)
        _MAPS[basis] = m
    return _MAPS[basis]


def new_rows(case: Case) -> np.ndarray:
    basis = basis_table(case.basis)
    rng = np.random.default_rng(1000 + case.q)
    if case.kind == "held-out":
        return cluster_table(case.basis)[0][300:]
    if case.kind == "equal":                                  # five rows equal to every basis row, one far from all of them
        x = np.full((case.q, basis.shape[1]), 0.625, np.float32)
        x[-1] = 3.0
        return x
    if case.kind == "copies":                                 # 40 exact copies of basis rows, 8 of them copies of each other, 16 fresh
        picks = rng.permutation(basis.shape[0])[:40]
        picks[33:] = picks[32]
        fresh = np.maximum(rng.standard_normal((16, basis.shape[1])), 0.0).astype(np.float32)
        return np.concatenate([basis[picks], fresh])[rng.permutation(56)]
    return rng.standard_normal((case.q, basis.shape[1])).astype(np.float32)


def reference(case: Case) -> dict:
    """``map``, ``table`` (the new rows), ``pre_new``, ``init``, ``pairs`` (Q, nn), ``stats`` and ``coords`` = {iterations: (Q, 2)}
    of the numpy form, read-only."""
    if case.id not in _REFERENCE:
        m = fitted(case.basis)
        table = new_rows(case)
        pre_new, init = embeddings.pacmap_transform_inputs(m, table)
        pairs, stats = embeddings._pacmap_place_pairs(m, pre_new)
        coords = embeddings.pacmap_place_trajectory(init, m.reduction.coordinates, pairs, SNAPSHOTS)
        for a in (table, pre_new, init, pairs, *coords.values()):
            a.setflags(write=False)
        _REFERENCE[case.id] = {"map": m, "table": table, "pre_new": pre_new, "init": init, "pairs": pairs, "stats": stats, "coords": coords}
    return _REFERENCE[case.id]
