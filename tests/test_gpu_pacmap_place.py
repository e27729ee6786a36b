"""GPU: ``HipEngine.pacmap_basis_scale_dev`` (cv_pacmap_basis_scale), ``pacmap_place_pairs`` (cv_pacmap_place_pairs) and
``pacmap_place`` (cv_pacmap_place) against the numpy form of ``chessvision.embeddings``, exactly: the basis rows' scale bit for bit,
the pairs index for index, the coordinates after 1, 100, 200 and 450 iterations as uint32 views.  Cases and their numpy results
(computed once per process): tests/pacmap_place_cases.py.  The device placement starts from the NUMPY pairs, so a pairs bug cannot
hide a placement bug or the other way round; ``place_embeddings`` chains the two on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import pacmap_place_cases as ppc
from chessvision import ChessVision, embeddings as emb, hip_backend as hb, synthetic

pytestmark = pytest.mark.gpu

BASES = sorted({c.basis for c in ppc.CASES})


@pytest.fixture(scope="module")
def engine():
    eng = hb.HipEngine(precision="f32")
    yield eng
    eng.close()


def _first(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    i, t = (int(v) for v in bad[0])
    return f"{len(bad)} of {want.size} differ, first at row {i} slot {t}: {got[i, t]!r} for {want[i, t]!r}"


@pytest.mark.parametrize("basis", BASES)
def test_basis_scale_equals_the_numpy_form_bit_for_bit(engine, basis):
    m = ppc.fitted(basis)
    got = engine.pacmap_basis_scale_dev(torch.tensor(m.pre).cuda(), m.reduction.n_neighbors).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == m.sigma.shape
    assert np.array_equal(got.view(np.uint64), m.sigma.view(np.uint64)), _first(got[:, None], m.sigma[:, None])


@pytest.mark.parametrize("case", ppc.CASES, ids=[c.id for c in ppc.CASES])
def test_pairs_equal_the_numpy_form(engine, case):
    ref = ppc.reference(case)
    got, stats = engine.pacmap_place_pairs(ref["map"], ref["pre_new"])
    want = ref["pairs"]
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), _first(got, want)
    for key in ("candidates", "query_rows", "nonfinite_query_rows", "nonfinite_corpus_rows"):
        assert stats[key] == ref["stats"][key], (key, stats, ref["stats"])
    assert stats["certified_rows"] + stats["exact_rows"] == case.q


@pytest.mark.parametrize("case", ppc.CASES, ids=[c.id for c in ppc.CASES])
def test_coordinates_equal_the_numpy_form_bit_for_bit(engine, case):
    ref = ppc.reference(case)
    basis = ref["map"].reduction.coordinates
    for iterations in ppc.SNAPSHOTS:
        got = engine.pacmap_place(ref["init"], basis, ref["pairs"], iterations)
        want = ref["coords"][iterations]
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"after {iterations} iterations: {_first(got, want)}"
    assert np.array_equal(engine.pacmap_place(ref["init"], basis, ref["pairs"], 0).view(np.uint32), ref["init"].view(np.uint32))


def test_a_batch_equals_its_rows_reversed_and_placed_alone(engine):
    """130 new rows over the clusters basis: three workgroups, the last with two lanes.  No new point reads another, so the same rows
    in reversed order (other lanes, other workgroups) and rows 0, 63, 64 and 129 alone give the same bits."""
    m = ppc.fitted("clusters")
    held_out = ppc.cluster_table("clusters")[0][300:]
    table = np.concatenate([held_out, held_out[::-1] + np.float32(0.25), held_out[:2] - np.float32(0.5)])
    assert table.shape == (130, 100)
    pre_new, init = emb.pacmap_transform_inputs(m, table)
    basis = m.reduction.coordinates

    def place(rows):
        pairs, _ = engine.pacmap_place_pairs(m, pre_new[rows])
        return pairs, engine.pacmap_place(init[rows], basis, pairs)

    pairs, coords = place(np.arange(130))
    want = emb.pacmap_transform(m, table)
    assert np.array_equal(pairs, want.neighbours) and np.array_equal(coords.view(np.uint32), want.coordinates.view(np.uint32))
    back_pairs, back = place(np.arange(130)[::-1])
    assert np.array_equal(back_pairs[::-1], pairs) and np.array_equal(back[::-1].view(np.uint32), coords.view(np.uint32))
    for i in (0, 63, 64, 129):
        alone_pairs, alone = place(np.array([i]))
        assert np.array_equal(alone_pairs[0], pairs[i]) and np.array_equal(alone[0].view(np.uint32), coords[i].view(np.uint32)), i


def test_a_partner_outside_the_basis_is_skipped(engine):
    ref = ppc.reference(ppc.BY_ID["widest-97x5-q3"])
    basis = ref["map"].reduction.coordinates
    pairs = ref["pairs"].copy()
    pairs[0, 31], pairs[1, 0], pairs[2, 7] = -1, 97, 1 << 30
    got = engine.pacmap_place(ref["init"], basis, pairs, 20)
    assert np.array_equal(got.view(np.uint32), emb.pacmap_place(ref["init"], basis, pairs, 20).view(np.uint32))


def test_two_calls_give_the_same_bytes_on_the_default_and_on_a_side_stream(engine):
    ref = ppc.reference(ppc.BY_ID["clusters-300x100-q64"])
    m = ref["map"]
    pre_new, pre, sigma = torch.tensor(ref["pre_new"]).cuda(), torch.tensor(m.pre).cuda(), torch.tensor(m.sigma).cuda()
    init, basis = torch.tensor(ref["init"]).cuda(), torch.tensor(m.reduction.coordinates).cuda()

    def once():
        pairs, _ = engine.pacmap_place_pairs_dev(pre_new, pre, sigma, 10)
        outs = (engine.pacmap_basis_scale_dev(pre, 10), pairs, engine.pacmap_place_dev(init, basis, pairs, 450))
        return tuple(o.cpu().numpy().tobytes() for o in outs)

    first = once()
    assert once() == first
    assert first == (m.sigma.tobytes(), ref["pairs"].tobytes(), ref["coords"][450].tobytes())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert once() == first and once() == first
    side.synchronize()


def test_argument_errors_of_the_c_entries(engine):
    lib = engine._lib
    plan = hb.PacmapPlacePlan()
    assert lib.cv_pacmap_place_plan(64, 300, 100, 10, ctypes.byref(plan)) == 0
    assert (plan.q, plan.n, plan.c, plan.n_neighbors, plan.candidates, plan.reserved) == (64, 300, 100, 10, 60, 0)
    assert plan.pairs_scratch_bytes >= lib.cv_embedding_neighbours_scratch_bytes(64, 300, 100, 60)
    assert plan.scale_scratch_bytes >= lib.cv_embedding_neighbours_scratch_bytes(300, 300, 100, 60)
    assert lib.cv_pacmap_place_plan(1, 7, 1, 2, ctypes.byref(plan)) == 0 and plan.candidates == 7
    for args, word in (((0, 300, 100, 10), "q must"), (((1 << 22) + 1, 300, 100, 10), "q must"), ((64, 6, 100, 2), "n must"),
                       ((64, 10, 100, 10), "n must"), ((64, 300, 0, 10), "c must"), ((64, 300, 100, 33), "n_neighbors must")):
        assert lib.cv_pacmap_place_plan(*args, ctypes.byref(plan)) == 1 and word in lib.cv_last_error().decode(), args
    assert lib.cv_pacmap_place_plan(64, 300, 100, 10, None) == 1

    ref = ppc.reference(ppc.BY_ID["wave-edge-65x3-q64"])
    m = ref["map"]
    pre_new, pre, sigma = torch.tensor(ref["pre_new"]).cuda(), torch.tensor(m.pre).cuda(), torch.tensor(m.sigma).cuda()
    init, basis = torch.tensor(ref["init"]).cuda(), torch.tensor(m.reduction.coordinates).cuda()
    assert lib.cv_pacmap_place_plan(64, 65, 3, 10, ctypes.byref(plan)) == 0
    need_p, need_s = int(plan.pairs_scratch_bytes), int(plan.scale_scratch_bytes)
    scratch = torch.empty(max(need_p, need_s), dtype=torch.uint8, device="cuda")
    nbr = torch.empty((64, 10), dtype=torch.int32, device="cuda")
    out = torch.empty((64, 2), dtype=torch.float32, device="cuda")
    scale = torch.empty(65, dtype=torch.float64, device="cuda")

    def pairs(q=64, n=65, c=3, nn=10, scratch_bytes=need_p, eng=engine._h, sigma_ptr=sigma.data_ptr(), nbr_ptr=nbr.data_ptr()):
        status = lib.cv_pacmap_place_pairs(eng, pre_new.data_ptr(), q, pre.data_ptr(), n, c, nn, sigma_ptr, nbr_ptr, None,
                                           scratch.data_ptr(), scratch_bytes, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(q=0), "q must"), (dict(n=6), "n must"), (dict(nn=0), "n_neighbors must"), (dict(c=4097), "c must"),
                         (dict(scratch_bytes=need_p - 1), "scratch_bytes"), (dict(sigma_ptr=None), "sigma must"),
                         (dict(sigma_ptr=sigma.data_ptr() + 4), "sigma must"), (dict(nbr_ptr=None), "neighbours must")):
        status, message = pairs(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)
    assert pairs(eng=None)[0] == 1
    assert pairs()[0] == 0

    def basis_scale(n=65, c=3, nn=10, scratch_bytes=need_s, out_ptr=scale.data_ptr()):
        status = lib.cv_pacmap_basis_scale(engine._h, pre.data_ptr(), n, c, nn, out_ptr, scratch.data_ptr(), scratch_bytes, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(n=6), "n must"), (dict(nn=33), "n_neighbors must"), (dict(c=0), "c must"),
                         (dict(scratch_bytes=need_s - 1), "scratch_bytes"), (dict(out_ptr=None), "sigma must")):
        status, message = basis_scale(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)
    assert basis_scale()[0] == 0

    def place(q=64, n=65, nn=10, iterations=3, out_ptr=out.data_ptr(), basis_ptr=basis.data_ptr()):
        status = lib.cv_pacmap_place(engine._h, init.data_ptr(), q, basis_ptr, n, nbr.data_ptr(), nn, iterations, out_ptr, 0)
        return status, lib.cv_last_error().decode()

    for kwargs, word in ((dict(q=0), "q must"), (dict(n=0), "n must"), (dict(nn=33), "n_neighbors must"), (dict(iterations=-1), "iterations must"),
                         (dict(out_ptr=init.data_ptr()), "out must"), (dict(out_ptr=out.data_ptr() + 4), "out must"),
                         (dict(basis_ptr=None), "basis must")):
        status, message = place(**kwargs)
        assert status == 1 and word in message, (kwargs, status, message)
    assert place()[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(nbr.cpu().numpy(), ref["pairs"]) and np.array_equal(scale.cpu().numpy(), m.sigma)
    assert np.array_equal(out.cpu().numpy(), emb.pacmap_place(ref["init"], m.reduction.coordinates, ref["pairs"], 3))
    with pytest.raises(ValueError):
        engine.pacmap_place_pairs(m, ref["pre_new"][:, :2])
    with pytest.raises(ValueError):
        engine.pacmap_place(ref["init"][:5], m.reduction.coordinates, ref["pairs"])
    with pytest.raises(hb.HipBackendError):
        engine.pacmap_place_dev(init, basis, nbr.to(torch.int64))


def test_fit_and_place_end_to_end_equal_the_numpy_form(tmp_path):
    """A ChessVision with a HIP model plugged in: the fit's pairs, optimiser and basis scale on its engine equal
    ``embeddings.pacmap_fit``; the placement's pairs and single launch, chained, equal ``embeddings.pacmap_transform`` -- the default
    path, a caller's starting coordinates, and a map that went through ``save_map`` / ``load_map``."""
    pe, pc_path = synthetic.save_checkpoints(tmp_path, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc_path), precision="f16x3")
    try:
        _ = cv.classifier                                     # plug the HIP model in; no image is processed
        for case in (ppc.BY_ID["clusters-300x100-q64"], ppc.BY_ID["projected-300x513-q64"]):
            ref = ppc.reference(case)
            want = ref["map"]
            got = cv.fit_embedding_map(ppc.basis_table(case.basis))
            assert got.reduction.coordinates.tobytes() == want.reduction.coordinates.tobytes() and got.reduction.n_neighbors == 10
            for name in ("neighbours", "mid_near", "further"):
                assert np.array_equal(getattr(got.reduction.pairs, name), getattr(want.reduction.pairs, name)), name
            assert got.pre.tobytes() == want.pre.tobytes() and got.sigma.dtype == np.float64 and got.sigma.tobytes() == want.sigma.tobytes()
            assert got.reduction.coordinates.tobytes() == cv.reduce_embeddings(ppc.basis_table(case.basis)).coordinates.tobytes()
            placed = cv.place_embeddings(got, ref["table"])
            assert placed.coordinates.tobytes() == ref["coords"][450].tobytes() and np.array_equal(placed.neighbours, ref["pairs"])
            assert placed.stats["query_rows"] == 64 and placed.stats["candidates"] == 60
        emb.save_map(tmp_path / "map.npz", got)
        start = np.random.default_rng(1).standard_normal((64, 2)).astype(np.float32)
        placed = cv.place_embeddings(emb.load_map(tmp_path / "map.npz"), torch.from_numpy(ref["table"].copy()).cuda(), init=start)
        assert placed.coordinates.tobytes() == emb.pacmap_transform(want, ref["table"], init=start).coordinates.tobytes()
        with pytest.raises(ValueError):
            cv.place_embeddings(got, ref["table"][:, :99])
    finally:
        cv.close()
