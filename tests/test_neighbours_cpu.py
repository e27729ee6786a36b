"""CPU: the numpy form of the exact neighbour search (chessvision/embeddings.py: neighbours, duplicate_groups, stack), the ctypes
surface of the C entry, and the host emulation of the device filter (tests/neighbour_cases.py) against the documented error bound."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import neighbour_cases as nc
from chessvision import ChessVision, embeddings


def _same(got, idx, dist) -> bool:
    return np.array_equal(got.indices, idx) and np.array_equal(got.sq_distances.view(np.int64), dist.view(np.int64))


@pytest.mark.parametrize("case", [c for c in nc.CASES if c.n <= 300 and (c.q or c.n) <= 300], ids=lambda c: c.id)
def test_numpy_form_equals_an_independent_float64_brute_force(case):
    a, b, self_graph = case.tables()
    got = embeddings.neighbours(a, None if self_graph else b, case.k)
    assert got.indices.dtype == np.int32 and got.sq_distances.dtype == np.float64 and got.indices.shape == (a.shape[0], case.k)
    assert _same(got, *nc.brute_neighbours(a, b, case.k, self_graph))


def test_numpy_form_against_scikit_learn_brute_force():
    sk = pytest.importorskip("sklearn.neighbors")
    for kind, c in (("a", 33), ("c", 512)):
        x = nc.make(kind, 200, c, 3)
        k = 10
        got = embeddings.neighbours(x, k=k)
        dist, idx = sk.NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x.astype(np.float64)).kneighbors(x.astype(np.float64))
        full = np.sort(nc.brute_sq_distances(x, x) + np.diag(np.full(200, np.inf)), axis=1)
        clear = full[:, k] - full[:, k - 1] > 1e-9 * full[:, k]                          # the k-th gap is not a tie
        assert clear.sum() > 150
        for i in np.flatnonzero(clear):
            theirs = [j for j in idx[i] if j != i][:k]
            assert set(theirs) == set(got.indices[i].tolist())
            np.testing.assert_allclose(np.sort(dist[i][idx[i] != i][:k] ** 2), got.sq_distances[i], rtol=1e-12, atol=0)


def test_ties_are_ordered_by_distance_then_corpus_index():
    x = nc.make("d", 120, 4, 5)                                                         # integers 0..2: at most 17 distinct distances
    got = embeddings.neighbours(x, k=64)
    d = nc.brute_sq_distances(x, x)
    for i in range(120):
        pairs = list(zip(got.sq_distances[i].tolist(), got.indices[i].tolist()))
        assert pairs == sorted(pairs) and all(dv == d[i, j] and j != i for dv, j in pairs)
        assert len(set(got.sq_distances[i].tolist())) < 20                              # ties really are everywhere
        worst = pairs[-1]
        assert all((d[i, j], j) > worst for j in range(120) if j != i and j not in got.indices[i])


def test_k_beyond_the_corpus_fills_with_minus_one_and_infinity():
    a, b = nc.make("a", 5, 7, 1), nc.make("a", 3, 7, 2)
    got = embeddings.neighbours(a, b, k=10)
    assert (got.indices[:, :3] >= 0).all() and (got.indices[:, 3:] == -1).all() and np.isinf(got.sq_distances[:, 3:]).all()
    own = embeddings.neighbours(b, k=3)                                                  # 2 eligible rows each
    assert (own.indices[:, 2] == -1).all() and (own.indices[:, :2] >= 0).all()
    assert embeddings.neighbours(b[:1], k=1).indices.tolist() == [[-1]]


def test_exclude_self_drops_the_row_by_index_and_keeps_a_duplicate():
    x = nc.make("a", 20, 9, 4)
    x[13] = x[2]
    got = embeddings.neighbours(x, k=3)
    assert got.indices[2, 0] == 13 and got.sq_distances[2, 0] == 0.0 and got.indices[13, 0] == 2
    assert all(i not in got.indices[i] for i in range(20))
    kept = embeddings.neighbours(x, x, k=3)                                              # a corpus given: exclude_self defaults to False
    assert kept.indices[2, :2].tolist() == [2, 13] and kept.indices[13, :2].tolist() == [2, 13]
    with pytest.raises(ValueError, match="exclude_self"):
        embeddings.neighbours(x[:5], x, k=3, exclude_self=True)
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match="k must"):
            embeddings.neighbours(x, k=bad_k)
    with pytest.raises(ValueError, match="channels"):
        embeddings.neighbours(x, x[:, :5])


def test_non_finite_rows_on_both_sides():
    x = nc.make("h", 30, 6, 7)                                                          # rows 0, 15 and 29 hold NaN, +inf, -inf
    got = embeddings.neighbours(x, k=5)
    for bad in (0, 15, 29):
        assert (got.indices[bad] == -1).all() and np.isnan(got.sq_distances[bad]).all()
        assert bad not in got.indices
    good = [i for i in range(30) if i not in (0, 15, 29)]
    assert (got.indices[good] >= 0).all() and np.isfinite(got.sq_distances[good]).all()
    assert got.stats == {"query_rows": 30, "certified_rows": 0, "exact_rows": 27, "nonfinite_query_rows": 3, "nonfinite_corpus_rows": 3}
    few = embeddings.neighbours(x[:3], x[13:17], k=4)                                    # 3 eligible corpus rows
    assert (few.indices[1:, 3] == -1).all() and np.isinf(few.sq_distances[1:, 3]).all() and np.isnan(few.sq_distances[0]).all()


def test_duplicate_groups():
    x = nc.make("a", 40, 16, 9)
    x[7] = x[3]
    x[21] = x[3] + np.float32(1e-4)
    x[30] = x[11]
    graph = embeddings.neighbours(x, k=4)
    assert embeddings.duplicate_groups(graph, 0.0) == [[3, 7], [11, 30]]
    assert embeddings.duplicate_groups(graph, 1e-2) == [[3, 7, 21], [11, 30]]
    assert embeddings.duplicate_groups(embeddings.neighbours(nc.make("a", 10, 16, 1), k=2), 1e-3) == []


def test_stack_on_hand_made_result_records():
    def result(seed, board=True):
        rng = np.random.default_rng(seed)
        emb = SimpleNamespace(board_extractor=rng.random(8).astype(np.float32), classifier=rng.random((64, 5)).astype(np.float32) if board else None)
        return SimpleNamespace(embeddings=emb)

    results = [result(0), result(1, board=False), SimpleNamespace(embeddings=None), result(2)]
    table, keys = embeddings.stack(results, "board_extractor")
    assert table.shape == (3, 8) and keys.tolist() == [[0, -1], [1, -1], [3, -1]]
    assert np.array_equal(table[2], results[3].embeddings.board_extractor)
    table, keys = embeddings.stack(results, "classifier")
    assert table.shape == (128, 5) and keys[0].tolist() == [0, 0] and keys[63].tolist() == [0, 63] and keys[64].tolist() == [3, 0]
    assert np.array_equal(table[64:], results[3].embeddings.classifier)
    empty, none = embeddings.stack([], "classifier")
    assert empty.shape[0] == 0 and none.shape == (0, 2)
    with pytest.raises(ValueError):
        embeddings.stack(results, "unet")


def test_chessvision_without_a_hip_model_runs_the_numpy_form():
    x = nc.make("c", 50, 12, 2)
    got = ChessVision(lazy_load=True).embedding_neighbours(x, k=4)
    assert _same(got, *nc.brute_neighbours(x, x, 4, True)) and got.stats["certified_rows"] == 0


def test_ctypes_prototypes_and_the_scratch_size_entry():
    import __graft_entry__ as ge

    ge.build()
    from chessvision import hip_backend as hb

    lib = hb.load_library()
    protos = {name: (res, args) for name, res, args in hb.SYMBOLS}
    assert protos["cv_embedding_neighbours_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    res, args = protos["cv_embedding_neighbours"]
    assert res is ctypes.c_int and len(args) == 14 and args[12] is ctypes.c_size_t
    assert lib.cv_abi_version() == 6
    small, large = lib.cv_embedding_neighbours_scratch_bytes(4, 65536, 512, 10), lib.cv_embedding_neighbours_scratch_bytes(16384, 16384, 512, 10)
    assert 65536 * 512 * 4 < small < 2 * 65536 * 512 * 4                                 # the centred corpus copy dominates
    assert 2 * 16384 * 512 * 4 < large < 4 * 16384 * 512 * 4
    assert small % 256 == 0 and large % 256 == 0
    for q, n, c, k in ((0, 5, 5, 5), (5, 0, 5, 5), (5, 5, 0, 5), (5, 5, 4097, 5), (5, 5, 5, 0), (5, 5, 5, 65), ((1 << 22) + 1, 5, 5, 5)):
        assert lib.cv_embedding_neighbours_scratch_bytes(q, n, c, k) == 0
    assert lib.cv_embedding_neighbours_scratch_bytes(1, 1, 1, 1) > 0 and lib.cv_embedding_neighbours_scratch_bytes(5, 5, 4096, 64) > 0
    # a null engine is refused before anything else is looked at
    assert lib.cv_embedding_neighbours(None, None, 1, None, 1, 1, 1, 0, None, None, None, None, 0, None) == 1
    assert b"null engine" in lib.cv_last_error()


# ---- the filter, emulated: the bound holds, and centring is why -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b", "c", "f"])
@pytest.mark.parametrize("c", [4, 33, 512, 1024])
def test_documented_bound_covers_the_float32_filter_error(kind, c):
    x = nc.make(kind, 150, c, 11)
    r = nc.emulate(x, x, 10, True)
    assert 0.0 < r["ratio"] < 1.0, r["ratio"]
    assert r["lost"] == 0


@pytest.mark.parametrize("case", nc.CERTIFIED_CASES, ids=lambda c: c.id)
def test_emulation_certifies_every_row_of_the_cases_the_gpu_test_caps(case):
    a, b, self_graph = case.tables()
    r = nc.emulate(a, b, case.k, self_graph)
    assert r["certified"].all() and r["lost"] == 0
    assert r["margin"].min() > 8.0, r["margin"].min()                                    # D_k sits many E below T - E: no summation order undoes it


@pytest.mark.parametrize("case", nc.EXACT_PATH_CASES, ids=lambda c: c.id)
def test_emulation_leaves_rows_uncertified_where_the_gpu_test_demands_the_exact_path(case):
    a, b, self_graph = case.tables()
    r = nc.emulate(a, b, case.k, self_graph)
    assert (~r["certified"][r["finite_queries"]]).any()


def test_uncentred_filter_loses_the_neighbours_of_offset_data():
    x = nc.make("b", 257, 512, 0)
    centred, raw = nc.emulate(x, x, 10, True), nc.emulate(x, x, 10, True, centre=False)
    assert centred["lost"] == 0 and centred["certified"].all()
    assert raw["lost"] > 0.5 * 257 * 10 and not raw["certified"].any()                   # most true neighbours are not even candidates
