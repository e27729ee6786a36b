"""CPU, only where the authors' ``pacmap`` package is installed (it is not on a stock ROCm box, so this is skipped there): the quality
figure of tests/test_pacmap_cpu.py -- leave-one-out 1-NN label purity of the 2-D map of the 13-cluster table -- of this project's
numpy form beside the package's on the same table.  The two draw different random pairs and the package's neighbours are approximate,
so the maps differ; what the reading has to match is how well the map keeps the clusters apart.  The tolerance is three points' worth
of purity on 300 (0.01), the granularity at which two runs of the package itself with different seeds were expected to differ; the
figures are printed either way."""
from __future__ import annotations

import numpy as np
import pytest

import pacmap_cases as pc

pacmap = pytest.importorskip("pacmap")


def test_purity_is_within_three_points_of_the_package():
    case = pc.BY_ID["clusters-300x100"]
    table, labels = pc.clusters(case.n, case.c, case.seed)
    ours = pc.purity(pc.reference(case)["coords"][450], labels)
    theirs = pc.purity(np.asarray(pacmap.PaCMAP(n_components=2, random_state=0).fit_transform(table, init="pca"), np.float32), labels)
    print(f"leave-one-out 1-NN purity: this project {ours:.4f}, the pacmap package {theirs:.4f}")
    assert ours >= theirs - 3 / case.n, (ours, theirs)
