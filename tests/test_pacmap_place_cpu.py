"""CPU: the numpy definition of placing new rows into a fitted PaCMAP map (``chessvision.embeddings``: ``pacmap_fit``,
``pacmap_preprocess_new``, ``pacmap_place_pairs``, ``pacmap_place_init``, ``pacmap_place``, ``pacmap_transform``, ``save_map`` /
``load_map``) and ``ChessVision.fit_embedding_map`` / ``place_embeddings`` without a HIP model.  Cases and their results (computed once
per process): tests/pacmap_place_cases.py."""
from __future__ import annotations

import numpy as np
import pytest

import pacmap_cases as pc
import pacmap_place_cases as ppc
from chessvision import ChessVision, embeddings as emb

CLUSTER_CASES = [ppc.BY_ID["clusters-300x100-q64"], ppc.BY_ID["projected-300x513-q64"]]


def _bits(a: np.ndarray) -> bytes:
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=[c.id for c in CLUSTER_CASES])
def test_fit_is_the_reduction_plus_what_placing_needs(case):
    m = ppc.fitted(case.basis)
    table = ppc.basis_table(case.basis)
    want = emb.pacmap(table)
    assert _bits(m.reduction.coordinates) == _bits(want.coordinates) and m.reduction.n_neighbors == want.n_neighbors == 10
    for name in ("neighbours", "mid_near", "further"):
        assert np.array_equal(getattr(m.reduction.pairs, name), getattr(want.pairs, name)), name
    assert m.reduction.stats == want.stats
    assert _bits(m.pre) == _bits(emb.pacmap_preprocess(table)) and m.pre.dtype == np.float32
    assert m.projected == (table.shape[1] > 100) and m.channels == table.shape[1]
    assert m.sigma.dtype == np.float64 and m.sigma.shape == (300,) and (m.sigma >= 1e-10).all()
    # sigma is the scale the neighbour choice used: mean sqrt(D) of the exact graph's ranks 3, 4, 5
    graph = emb.neighbours(m.pre, k=60)
    assert np.array_equal(m.sigma, (np.sqrt(graph.sq_distances[:, 3]) + np.sqrt(graph.sq_distances[:, 4]) +
                                    np.sqrt(graph.sq_distances[:, 5])) / 3.0)
    if m.projected:
        assert m.axes.shape == (513, 100) and m.start_axes.size == 0 and m.minimum == m.maximum == 0.0
    else:
        assert m.axes.size == 0 and m.start_axes.shape == (100, 2) and m.start_mean.shape == (100,)
        assert m.minimum == float(table.astype(np.float64).min()) and m.maximum == float((table.astype(np.float64) - m.minimum).max())


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=[c.id for c in CLUSTER_CASES])
def test_basis_rows_preprocess_to_within_one_ulp_of_the_fit(case):
    """Not bitwise: the float64 product of fewer or other rows may be blocked differently by the BLAS."""
    m = ppc.fitted(case.basis)
    again = emb.pacmap_preprocess_new(m, ppc.basis_table(case.basis))
    assert again.dtype == np.float32 and again.shape == m.pre.shape
    ulp = np.spacing(np.abs(m.pre))
    assert (np.abs(again.astype(np.float64) - m.pre.astype(np.float64)) <= ulp).all()
    start = emb.pacmap_place_init(m, m.pre)                   # the fit's start, evaluated at the basis rows themselves
    want = emb.pacmap_init(m.pre, projected=m.projected)
    assert np.abs(start.astype(np.float64) - want).max() <= 4 * np.spacing(np.abs(want).max())


def test_equal_rows_tie_by_index_and_a_zero_maximum_is_not_divided_by():
    ref = ppc.reference(ppc.BY_ID["equal-64x4-q6"])
    m = ref["map"]
    assert m.maximum == 0.0 and (m.sigma == 1e-10).all() and not m.pre.any()
    assert not ref["pre_new"][:5].any() and np.array_equal(ref["pre_new"][5], np.full(4, 2.375, np.float32))
    assert np.array_equal(ref["pairs"], np.tile(np.arange(10, dtype=np.int32), (6, 1)))
    for coords in ref["coords"].values():
        assert np.isfinite(coords).all()


def test_copies_sit_on_zero_distances_and_equal_rows_get_equal_results():
    ref = ppc.reference(ppc.BY_ID["copies-2048x32-q56"])
    m, table = ref["map"], ref["table"]
    graph = emb.neighbours(ref["pre_new"], corpus=m.pre, k=1, exclude_self=False)
    assert int((graph.sq_distances[:, 0] == 0.0).sum()) == 40
    _, inverse, counts = np.unique(table, axis=0, return_inverse=True, return_counts=True)
    assert counts.max() == 8
    same = np.flatnonzero(inverse.ravel() == counts.argmax())
    for name in ("pairs", "init"):
        assert (ref[name][same] == ref[name][same[0]]).all(), name
    assert (ref["coords"][450][same].view(np.uint32) == ref["coords"][450][same[0]].view(np.uint32)).all()


@pytest.mark.parametrize("case", ppc.CASES, ids=[c.id for c in ppc.CASES])
def test_pairs_have_the_structure_the_definition_gives_them(case):
    ref = ppc.reference(case)
    m, pairs = ref["map"], ref["pairs"]
    n, nn = m.pre.shape[0], m.reduction.n_neighbors
    kc = min(nn + 50, 64, n)
    assert pairs.dtype == np.int32 and pairs.shape == (case.q, nn) and ref["stats"]["candidates"] == kc
    assert pairs.min() >= 0 and pairs.max() < n
    graph = emb.neighbours(ref["pre_new"], corpus=m.pre, k=kc, exclude_self=False)
    for i in range(case.q):
        assert len(set(pairs[i])) == nn and set(pairs[i]) <= set(graph.indices[i])
    if kc == n:
        assert (np.sort(graph.indices, axis=1) == np.arange(n)).all()
    assert ref["coords"][450].dtype == np.float32 and np.isfinite(ref["coords"][450]).all()


def test_placement_is_independent_of_the_batch_and_of_its_order():
    ref = ppc.reference(ppc.BY_ID["clusters-300x100-q64"])
    m, table = ref["map"], ref["table"]
    whole = emb.pacmap_transform(m, table)
    assert _bits(whole.coordinates) == _bits(ref["coords"][450]) and np.array_equal(whole.neighbours, ref["pairs"])
    back = emb.pacmap_transform(m, table[::-1])
    assert _bits(back.coordinates[::-1]) == _bits(whole.coordinates) and np.array_equal(back.neighbours[::-1], whole.neighbours)
    for i in (0, 31, 63):
        alone = emb.pacmap_transform(m, table[i:i + 1])
        assert _bits(alone.coordinates[0]) == _bits(whole.coordinates[i]) and np.array_equal(alone.neighbours[0], whole.neighbours[i])


def test_trajectory_snapshots_do_not_depend_on_what_follows():
    ref = ppc.reference(ppc.BY_ID["wave-edge-65x3-q65"])
    yb = ref["map"].reduction.coordinates
    assert _bits(ref["coords"][100]) == _bits(emb.pacmap_place(ref["init"], yb, ref["pairs"], 100))
    assert _bits(emb.pacmap_place(ref["init"], yb, ref["pairs"], 0)) == _bits(ref["init"])
    skipped = ref["pairs"].copy()
    skipped[:, 3] = -1                                        # a partner outside [0, N) is skipped: the same as a row without that slot
    assert _bits(emb.pacmap_place(ref["init"], yb, skipped, 7)) == _bits(emb.pacmap_place(ref["init"], yb, np.delete(ref["pairs"], 3, axis=1), 7))


def test_first_step_pulls_towards_the_partners():
    """Iteration 0 by hand in float64: the gradient of the attraction term alone, then Adam's first step (m = c1 g, v = c2 g^2)."""
    ref = ppc.reference(ppc.BY_ID["wave-edge-65x3-q64"])
    yb, y0 = ref["map"].reduction.coordinates.astype(np.float64), ref["init"].astype(np.float64)
    e = y0[:, None, :] - yb[ref["pairs"]]
    d = 1.0 + (e ** 2).sum(-1)
    g = (2.0 * (20.0 / (10.0 + d) ** 2))[..., None] * e
    g = g.sum(1)
    lr = float(emb.pacmap_schedule(1)[0, 0])
    want = y0 - lr * (0.1 * g) / (np.sqrt(0.001 * g * g) + 1e-7)
    got = emb.pacmap_place(ref["init"], ref["map"].reduction.coordinates, ref["pairs"], 1)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def test_save_and_load_round_trip(tmp_path):
    m = ppc.fitted("clusters")
    path = tmp_path / "map.npz"
    emb.save_map(path, m)
    back = emb.load_map(path)
    for name in ("pre", "sigma", "channel_mean", "axes", "start_mean", "start_axes"):
        a, b = getattr(m, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and _bits(a) == _bits(b), name
    assert (back.projected, back.channels, back.minimum, back.maximum) == (m.projected, m.channels, m.minimum, m.maximum)
    assert _bits(back.reduction.coordinates) == _bits(m.reduction.coordinates) and back.reduction.n_neighbors == m.reduction.n_neighbors
    for name in ("neighbours", "mid_near", "further"):
        a, b = getattr(m.reduction.pairs, name), getattr(back.reduction.pairs, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert back.reduction.stats == m.reduction.stats == back.reduction.pairs.stats
    table = ppc.reference(ppc.BY_ID["clusters-300x100-q64"])["table"]
    assert _bits(emb.pacmap_transform(back, table).coordinates) == _bits(ppc.reference(ppc.BY_ID["clusters-300x100-q64"])["coords"][450])
    projected = ppc.fitted("projected")
    emb.save_map(path, projected)
    assert _bits(emb.load_map(path).axes) == _bits(projected.axes) and emb.load_map(path).projected
    np.savez(tmp_path / "other.npz", pre=m.pre)
    with pytest.raises(ValueError):
        emb.load_map(tmp_path / "other.npz")


def test_argument_errors():
    m = ppc.fitted("clusters")
    good = ppc.reference(ppc.BY_ID["clusters-300x100-q64"])["table"]
    with pytest.raises(ValueError, match="channels"):
        emb.pacmap_transform(m, good[:, :99])
    bad = good.copy()
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="NaN or an infinity"):
        emb.pacmap_transform(m, bad)
    bad[3, 7] = np.inf
    with pytest.raises(ValueError, match="NaN or an infinity"):
        emb.pacmap_preprocess_new(m, bad)
    with pytest.raises(ValueError, match="at least one row"):
        emb.pacmap_transform(m, good[:0])
    with pytest.raises(ValueError, match="init must"):
        emb.pacmap_transform(m, good, init=np.zeros((63, 2), np.float32))
    with pytest.raises(ValueError, match="init must"):
        emb.pacmap_transform(m, good, init=np.full((64, 2), np.nan, np.float32))
    with pytest.raises(ValueError, match="init must"):
        emb.pacmap_transform(m, good, init="random")
    with pytest.raises(ValueError, match="channels"):
        emb.pacmap_place_pairs(m, np.zeros((4, 99), np.float32))
    with pytest.raises(ValueError, match="init must"):
        emb.pacmap_place(np.zeros((3, 2), np.float32), m.reduction.coordinates, np.zeros((4, 10), np.int32))
    with pytest.raises(ValueError, match="basis_coordinates must"):
        emb.pacmap_place(np.zeros((4, 2), np.float32), np.zeros((300, 3), np.float32), np.zeros((4, 10), np.int32))
    with pytest.raises(ValueError, match="pairs must"):
        emb.pacmap_place(np.zeros((4, 2), np.float32), m.reduction.coordinates, np.zeros((4, 33), np.int32))
    with pytest.raises(ValueError, match="method must"):
        ChessVision(lazy_load=True).fit_embedding_map(ppc.basis_table("clusters"), method="umap")


def test_chessvision_without_a_hip_model_runs_the_numpy_form():
    case = ppc.BY_ID["wave-edge-65x3-q65"]
    ref = ppc.reference(case)
    cv = ChessVision(lazy_load=True)
    m = cv.fit_embedding_map(ppc.basis_table(case.basis))
    assert _bits(m.reduction.coordinates) == _bits(pc.reference(pc.BY_ID[case.basis])["coords"][450])
    assert _bits(m.sigma) == _bits(ref["map"].sigma) and _bits(m.pre) == _bits(ref["map"].pre)
    got = cv.place_embeddings(m, ref["table"])
    assert isinstance(got, emb.Placement) and _bits(got.coordinates) == _bits(ref["coords"][450])
    assert np.array_equal(got.neighbours, ref["pairs"]) and got.stats == ref["stats"]
    start = np.random.default_rng(0).standard_normal((65, 2)).astype(np.float32)
    seeded = cv.place_embeddings(m, ref["table"], init=start)
    assert _bits(seeded.coordinates) == _bits(emb.pacmap_place(start, m.reduction.coordinates, ref["pairs"]))


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=[c.id for c in CLUSTER_CASES])
def test_held_out_rows_land_in_their_own_cluster(case):
    """Every one of the 64 held-out rows lands next to a basis point of its own label, and ends within 0.01 of the mean coordinate
    of its partners (a point that is only pulled comes to rest among what pulls it).  Measured when the case was written: 64 of 64
    in both cases; the largest distance to the partners' mean 0.0054 (clusters) and 0.0053 (projected) on maps about 40 wide."""
    ref = ppc.reference(case)
    labels = ppc.cluster_table(case.basis)[1]
    yb = ref["map"].reduction.coordinates.astype(np.float64)
    y = ref["coords"][450].astype(np.float64)
    nearest = ((y[:, None, :] - yb[None, :, :]) ** 2).sum(-1).argmin(1)
    agree = int((labels[:300][nearest] == labels[300:]).sum())
    off = np.sqrt(((y - yb[ref["pairs"]].mean(1)) ** 2).sum(-1))
    print(f"{case.id}: {agree} of 64 next to their own label, largest distance to the partners' mean {off.max():.4f}, "
          f"map extent {np.ptp(yb, axis=0)}")
    assert agree == 64
    assert (off <= 0.01).all()
