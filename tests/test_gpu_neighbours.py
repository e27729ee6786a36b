"""GPU: ``HipEngine.embedding_neighbours`` (cv_embedding_neighbours) against the numpy form ``chessvision.embeddings.neighbours``, bit
for bit -- indices and the float64 bits of the squared distances -- once through the filter (auto) and once with every row on the exact
path.  Shapes, data kinds and the host emulation that picked the certified cases: tests/neighbour_cases.py.

Two conditions keep the exact path from hiding a broken filter, and the filter from hiding a broken exact path: on the iid, offset
and clustered tables EVERY finite row must be certified in auto mode (the emulation certifies all of them with D_k more than 16 E below
T - E, far outside what another float32 summation order can move); on the duplicate, tight-cluster and overflow tables some rows must
take the exact path.  Every input tensor starts 4 bytes into its allocation."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import neighbour_cases as nc
from chessvision import ChessVision, embeddings, hip_backend as hb, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = hb.HipEngine(precision="f32")
    yield eng
    eng.close()


def _odd(a: np.ndarray) -> torch.Tensor:
    """The table on the device, 4 bytes into its allocation."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(a.shape)
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    return view


_REFERENCE: dict = {}


def _reference(case: nc.Case):
    """The numpy form of a case, computed once and shared by both modes (arrays marked read-only)."""
    if case.id not in _REFERENCE:
        a, b, self_graph = case.tables()
        ref = embeddings.neighbours(a, None if self_graph else b, case.k)
        for arr in (a, b, ref.indices, ref.sq_distances):
            arr.setflags(write=False)
        _REFERENCE[case.id] = (a, b, self_graph, ref)
    return _REFERENCE[case.id]


def _run(engine, case: nc.Case, exact_only: bool):
    a, b, self_graph, ref = _reference(case)
    qa = _odd(a)
    got = engine.embedding_neighbours(qa, None if self_graph else _odd(b), case.k, exact_only=exact_only)
    assert np.array_equal(got.indices, ref.indices), _first(got, ref)
    assert np.array_equal(got.sq_distances.view(np.int64), ref.sq_distances.view(np.int64)), _first(got, ref)
    s, q = got.stats, a.shape[0]
    assert s["query_rows"] == q
    assert s["nonfinite_query_rows"] == ref.stats["nonfinite_query_rows"] and s["nonfinite_corpus_rows"] == ref.stats["nonfinite_corpus_rows"]
    assert s["certified_rows"] + s["exact_rows"] + s["nonfinite_query_rows"] == q, s
    if exact_only:
        assert s["certified_rows"] == 0, s
    return got


def _first(got, ref) -> str:
    bad = np.argwhere((got.indices != ref.indices) | (got.sq_distances.view(np.int64) != ref.sq_distances.view(np.int64)))
    i, t = (int(v) for v in bad[0])
    return (f"{len(bad)} slots differ, first at row {i} slot {t}: index {got.indices[i, t]} for {ref.indices[i, t]}, "
            f"D {got.sq_distances[i, t]!r} for {ref.sq_distances[i, t]!r}; stats {got.stats}")


@pytest.mark.parametrize("exact_only", [False, True], ids=["auto", "exact_only"])
@pytest.mark.parametrize("case", nc.CASES, ids=[c.id for c in nc.CASES])
def test_equals_the_numpy_form_bit_for_bit(engine, case, exact_only):
    _run(engine, case, exact_only)


@pytest.mark.parametrize("exact_only", [False, True], ids=["auto", "exact_only"])
@pytest.mark.parametrize("case", nc.CERTIFIED_CASES, ids=[c.id for c in nc.CERTIFIED_CASES])
def test_iid_offset_and_clustered_tables_are_certified_row_for_row(engine, case, exact_only):
    got = _run(engine, case, exact_only)
    if not exact_only:
        finite = got.stats["query_rows"] - got.stats["nonfinite_query_rows"]
        assert got.stats["certified_rows"] == finite and got.stats["exact_rows"] == 0, got.stats


@pytest.mark.parametrize("exact_only", [False, True], ids=["auto", "exact_only"])
@pytest.mark.parametrize("case", nc.EXACT_PATH_CASES, ids=[c.id for c in nc.EXACT_PATH_CASES])
def test_duplicates_tight_clusters_and_overflow_take_the_exact_path(engine, case, exact_only):
    got = _run(engine, case, exact_only)
    assert got.stats["exact_rows"] > 0, got.stats


def test_two_runs_are_bit_identical_on_the_default_and_on_a_side_stream(engine):
    case = nc.Case("c", 0, 257, 512, 10)
    a = _odd(case.tables()[0])

    def once():
        i, d, s = engine.embedding_neighbours_dev(a, a, case.k, exclude_self=True)
        return i.cpu().numpy().tobytes(), d.cpu().numpy().tobytes(), s.cpu().numpy().tobytes()

    first = once()
    assert once() == first
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert once() == first and once() == first
    side.synchronize()


def test_argument_errors_of_the_c_entry(engine):
    lib = engine._lib
    a = _odd(nc.make("a", 8, 5, 0))
    b = _odd(nc.make("a", 9, 5, 1))
    idx = torch.empty((8, 64), dtype=torch.int32, device="cuda")
    dist = torch.empty((8, 64), dtype=torch.float64, device="cuda")
    need = int(lib.cv_embedding_neighbours_scratch_bytes(8, 9, 5, 10))
    assert need > 0 and lib.cv_embedding_neighbours_scratch_bytes(8, 9, 5, 0) == 0 and lib.cv_embedding_neighbours_scratch_bytes(8, 9, 0, 10) == 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(q=8, n=9, c=5, k=10, flags=0, scratch_bytes=need, corpus=b):
        status = lib.cv_embedding_neighbours(engine._h, a.data_ptr(), q, corpus.data_ptr(), n, c, k, flags, idx.data_ptr(), dist.data_ptr(), None,
                                             scratch.data_ptr(), scratch_bytes, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(k=0), "k must"), (dict(k=65), "k must"), (dict(c=0), "c must"), (dict(scratch_bytes=need - 1), "scratch_bytes"),
                         (dict(flags=1), "exclude-self needs q == n"), (dict(q=0), "q must"), (dict(n=0), "n must"), (dict(flags=4), "flags")):
        status, message = call(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)              # CV_ERR_INVALID, naming the argument
    assert lib.cv_embedding_neighbours(None, a.data_ptr(), 8, b.data_ptr(), 9, 5, 10, 0, idx.data_ptr(), dist.data_ptr(), None,
                                       scratch.data_ptr(), need, 0) == 1
    assert call()[0] == 0                                                              # and the call as it should be goes through
    torch.cuda.synchronize()
    with pytest.raises(hb.HipBackendError, match="k must"):
        engine.embedding_neighbours_dev(a, b, 65)
    with pytest.raises(ValueError):
        engine.embedding_neighbours(a, b, 10, exclude_self=True)


def test_end_to_end_both_tables_of_a_process_images_job(tmp_path):
    """8 synthetic boards, two of them the same photo: process_images(embeddings=True) -> stack -> ChessVision.embedding_neighbours
    equals the numpy form on the same arrays for both tables, and the twins are each other's first neighbour among the uploads."""
    pe, pc = synthetic.save_checkpoints(tmp_path, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3")
    try:
        photos = [synthetic.board_photo(700 + s) for s in range(7)]
        photos.insert(5, photos[1].copy())
        results = cv.process_images(photos, embeddings=True)
        for which, k in (("board_extractor", 3), ("classifier", 10)):
            table, keys = embeddings.stack(results, which)
            assert table.shape[0] == keys.shape[0] > 0 and table.dtype == np.float32
            got = cv.embedding_neighbours(table, k=k)
            ref = embeddings.neighbours(table, k=k)
            assert np.array_equal(got.indices, ref.indices) and np.array_equal(got.sq_distances.view(np.int64), ref.sq_distances.view(np.int64))
            assert got.stats["query_rows"] == table.shape[0]
            looked_up = cv.embedding_neighbours(torch.from_numpy(table[:3]).cuda(), table, k=k)     # the lookup shape, device tensor in
            ref = embeddings.neighbours(table[:3], table, k=k)
            assert np.array_equal(looked_up.indices, ref.indices) and np.array_equal(looked_up.sq_distances.view(np.int64), ref.sq_distances.view(np.int64))
            if which == "board_extractor":
                rows = {int(img): r for r, (img, _) in enumerate(keys)}
                assert got.indices[rows[1], 0] == rows[5] and got.indices[rows[5], 0] == rows[1]
                assert got.sq_distances[rows[1], 0] == 0.0
                assert [rows[1], rows[5]] in embeddings.duplicate_groups(got, 1e-6)
    finally:
        cv.close()
