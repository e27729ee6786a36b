"""CPU, only where the authors' ``pacmap`` package is installed (it is not on a stock ROCm box, so this is skipped there): the quality
figure of tests/test_pacmap_place_cpu.py -- how many of the 64 held-out rows of the 13-cluster table land next to a basis point of their
own label -- of this project's numpy form beside the package's ``transform`` of the same rows into its own fit of the same basis.  The
two maps differ (other random pairs, approximate neighbours in the package), so coordinates are not compared; what the reading has to
match is that a placed row ends up in its own cluster.  The tolerance is one row of 64, the granularity of the figure; both figures
are printed either way."""
from __future__ import annotations

import numpy as np
import pytest

import pacmap_place_cases as ppc

pacmap = pytest.importorskip("pacmap")


def _agreement(placed: np.ndarray, basis: np.ndarray, labels: np.ndarray) -> int:
    y, yb = placed.astype(np.float64), basis.astype(np.float64)
    nearest = ((y[:, None, :] - yb[None, :, :]) ** 2).sum(-1).argmin(1)
    return int((labels[:300][nearest] == labels[300:]).sum())


def test_held_out_label_agreement_is_within_one_row_of_the_package():
    case = ppc.BY_ID["clusters-300x100-q64"]
    ref = ppc.reference(case)
    table, labels = ppc.cluster_table(case.basis)
    ours = _agreement(ref["coords"][450], ref["map"].reduction.coordinates, labels)
    reducer = pacmap.PaCMAP(n_components=2, random_state=0, save_tree=True)
    basis = np.asarray(reducer.fit_transform(table[:300], init="pca"), np.float32)
    theirs = _agreement(np.asarray(reducer.transform(table[300:], basis=table[:300]), np.float32), basis, labels)
    print(f"held-out rows next to a basis point of their own label: this project {ours} of 64, the pacmap package {theirs} of 64")
    assert ours >= theirs - 1, (ours, theirs)
