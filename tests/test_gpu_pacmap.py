"""GPU: ``HipEngine.pacmap_pairs`` (cv_pacmap_pairs) and ``HipEngine.pacmap_optimise`` (cv_pacmap_optimise) against the numpy form of
``chessvision.embeddings``, exactly: the three pair sets index for index with the same draw counts, the coordinates after 1, 100, 200
and 450 iterations as uint32 views.  Cases and their numpy results (computed once per process): tests/pacmap_cases.py.  The device
optimiser starts from the NUMPY pairs, so a pairs bug cannot hide an optimiser bug or the other way round; ``reduce_embeddings`` chains
the two on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import pacmap_cases as pc
from chessvision import ChessVision, embeddings as emb, hip_backend as hb, synthetic

pytestmark = pytest.mark.gpu

OPTIMISED = [c for c in pc.CASES if c.optimise]


@pytest.fixture(scope="module")
def engine():
    eng = hb.HipEngine(precision="f32")
    yield eng
    eng.close()


def _first(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    i, t = (int(v) for v in bad[0])
    return f"{len(bad)} of {want.size} differ, first at row {i} slot {t}: {got[i, t]!r} for {want[i, t]!r}"


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_pairs_equal_the_numpy_form(engine, case):
    ref = pc.reference(case)
    got = engine.pacmap_pairs(ref["pre"], case.n_neighbors, case.n_MN, case.n_FP, case.seed)
    want = ref["pairs"]
    for name in ("neighbours", "mid_near", "further"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), f"{name}: {_first(g, w)}"
    for key in ("candidates", "mid_near_draws", "further_draws", "query_rows", "nonfinite_query_rows", "nonfinite_corpus_rows"):
        assert got.stats[key] == want.stats[key], (key, got.stats, want.stats)
    assert got.stats["certified_rows"] + got.stats["exact_rows"] == case.n


@pytest.mark.parametrize("case", OPTIMISED, ids=[c.id for c in OPTIMISED])
def test_coordinates_equal_the_numpy_form_bit_for_bit(engine, case):
    ref = pc.reference(case)
    for iterations in pc.SNAPSHOTS:
        got = engine.pacmap_optimise(ref["init"], ref["pairs"], iterations)
        want = ref["coords"][iterations]
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"after {iterations} iterations: {_first(got, want)}"
    assert np.array_equal(engine.pacmap_optimise(ref["init"], ref["pairs"], 0), ref["init"])


def test_two_calls_give_the_same_bytes_on_the_default_and_on_a_side_stream(engine):
    case = pc.BY_ID["shell-257x8"]
    ref = pc.reference(case)
    pre = torch.tensor(ref["pre"]).cuda()
    offsets, entries = (torch.tensor(a).cuda() for a in emb.pacmap_incidence(ref["pairs"]))
    init = torch.tensor(ref["init"]).cuda()

    def once():
        outs = engine.pacmap_pairs_dev(pre, 16, 8, 32, case.seed) + (engine.pacmap_optimise_dev(init, offsets, entries, 450),)
        return tuple(o.cpu().numpy().tobytes() for o in outs)

    first = once()
    assert once() == first
    assert first[4] == ref["coords"][450].tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert once() == first and once() == first
    side.synchronize()


def test_argument_errors_of_the_c_entries(engine):
    lib = engine._lib
    plan = hb.PacmapPlan()
    assert lib.cv_pacmap_plan(300, 100, 10, 5, 20, ctypes.byref(plan)) == 0
    assert (plan.n, plan.c, plan.n_neighbors, plan.n_mn, plan.n_fp, plan.candidates) == (300, 100, 10, 5, 20, 60)
    assert plan.pairs_scratch_bytes >= lib.cv_embedding_neighbours_scratch_bytes(300, 300, 100, 60) and plan.optimise_scratch_bytes >= 4 * 300 * 8
    for args, word in (((30, 100, 10, 5, 20), "n must"), ((300, 0, 10, 5, 20), "c must"), ((300, 100, 33, 5, 20), "n_neighbors must"),
                       ((300, 100, 10, 17, 20), "n_mn must"), ((300, 100, 10, 5, 65), "n_fp must"), (((1 << 22) + 1, 4, 10, 5, 20), "n must")):
        assert lib.cv_pacmap_plan(*args, ctypes.byref(plan)) == 1 and word in lib.cv_last_error().decode(), args
    assert lib.cv_pacmap_plan(300, 100, 10, 5, 20, None) == 1

    ref = pc.reference(pc.BY_ID["iid-65x3"])
    pre, init = torch.tensor(ref["pre"]).cuda(), torch.tensor(ref["init"]).cuda()
    offsets, entries = (torch.tensor(a).cuda() for a in emb.pacmap_incidence(ref["pairs"]))
    assert lib.cv_pacmap_plan(65, 3, 10, 5, 20, ctypes.byref(plan)) == 0
    need_p, need_o = int(plan.pairs_scratch_bytes), int(plan.optimise_scratch_bytes)
    scratch = torch.empty(max(need_p, need_o), dtype=torch.uint8, device="cuda")
    nbr, mid, far = (torch.empty((65, k), dtype=torch.int32, device="cuda") for k in (10, 5, 20))
    out = torch.empty((65, 2), dtype=torch.float32, device="cuda")

    def pairs(n=65, c=3, nn=10, nmn=5, nfp=20, scratch_bytes=need_p, eng=engine._h, mid_ptr=mid.data_ptr()):
        status = lib.cv_pacmap_pairs(eng, pre.data_ptr(), n, c, nn, nmn, nfp, 0, nbr.data_ptr(), mid_ptr, far.data_ptr(), None,
                                     scratch.data_ptr(), scratch_bytes, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(n=30), "n must"), (dict(nn=0), "n_neighbors must"), (dict(nmn=-1), "n_mn must"), (dict(nfp=65), "n_fp must"),
                         (dict(c=4097), "c must"), (dict(scratch_bytes=need_p - 1), "scratch_bytes"), (dict(mid_ptr=None), "mid_near must")):
        status, message = pairs(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)
    assert pairs(eng=None)[0] == 1
    assert pairs()[0] == 0

    def optimise(n=65, n_entries=int(entries.numel()), iterations=3, scratch_bytes=need_o, out_ptr=out.data_ptr()):
        status = lib.cv_pacmap_optimise(engine._h, init.data_ptr(), n, offsets.data_ptr(), entries.data_ptr(), n_entries, iterations, out_ptr,
                                        scratch.data_ptr(), scratch_bytes, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(n=6), "n must"), (dict(n_entries=0), "n_entries must"), (dict(iterations=-1), "iterations must"),
                         (dict(scratch_bytes=need_o - 1), "scratch_bytes"), (dict(out_ptr=init.data_ptr()), "out must"),
                         (dict(out_ptr=out.data_ptr() + 4), "out must")):
        status, message = optimise(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)
    assert optimise()[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), emb.pacmap_optimise(ref["init"], ref["pairs"], 3))
    with pytest.raises(ValueError):
        engine.pacmap_pairs(ref["pre"][:30])
    with pytest.raises(ValueError):
        engine.pacmap_pairs(torch.full((65, 3), float("nan")))


def test_reduce_embeddings_end_to_end_equals_the_numpy_form(tmp_path):
    """A ChessVision with a HIP model plugged in: pairs and optimiser on its engine, chained, equal ``embeddings.pacmap`` on the same
    table -- the default path, a seeded one with fewer neighbours and a caller's starting coordinates, and a device tensor in."""
    pe, pc_path = synthetic.save_checkpoints(tmp_path, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc_path), precision="f16x3")
    try:
        _ = cv.classifier                                     # plug the HIP model in; no image is processed
        case = pc.BY_ID["projected-300x513"]
        table = pc.table(case)
        got = cv.reduce_embeddings(table)
        ref = pc.reference(case)
        assert got.coordinates.tobytes() == ref["coords"][450].tobytes() and got.n_neighbors == 10
        for name in ("neighbours", "mid_near", "further"):
            assert np.array_equal(getattr(got.pairs, name), getattr(ref["pairs"], name)), name
        assert got.stats["query_rows"] == 300 and got.stats["certified_rows"] + got.stats["exact_rows"] == 300
        small = pc.table(pc.BY_ID["iid-65x3"])
        start = np.random.default_rng(1).standard_normal((65, 2)).astype(np.float32)
        got = cv.reduce_embeddings(torch.from_numpy(small).cuda(), n_neighbors=5, seed=9, init=start)
        want = emb.pacmap(small, n_neighbors=5, seed=9, init=start)
        assert got.coordinates.tobytes() == want.coordinates.tobytes() and np.array_equal(got.pairs.further, want.pairs.further)
        with pytest.raises(ValueError):
            cv.reduce_embeddings(table, method="umap")
    finally:
        cv.close()
