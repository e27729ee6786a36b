"""CPU: the numpy form of the PaCMAP reduction (``chessvision.embeddings``: pacmap_preprocess, pacmap_init, pacmap_pairs,
pacmap_incidence, pacmap_schedule, pacmap_optimise) -- the definition that tests/test_gpu_pacmap.py holds the device form to.  The
generator against values worked out with Python integers, the argument rules, the structure of the three pair sets recomputed without
a look at the module's own code paths, the gather gradient against a float64 symmetric scatter, determinism, and the one quality
figure: leave-one-out 1-NN label purity of the map of the 13-cluster table against that of its PCA-2 map (profiles/pacmap.md)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import neighbour_cases as nc
import pacmap_cases as pc
from chessvision import ChessVision, embeddings as emb

M64 = (1 << 64) - 1
STRUCTURE_CASES = [c for c in pc.CASES if c.n <= 2048]


def _mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _draw(seed: int, stream: int, i: int, t: int, n: int) -> int:
    key = _mix(seed ^ _mix((stream << 40) | i))
    return ((_mix((key + t) & M64) >> 32) * n) >> 32


def test_generator_against_hand_computed_values():
    assert _mix(0) == 0xE220A8397B1DCDAF                      # the first output of splitmix64 from state 0
    assert [int(v) for v in emb.pacmap_mix([0, 1])] == [0xE220A8397B1DCDAF, 0x910A2DEC89025CC1]
    assert int(emb.pacmap_key(0, 1, [0])[0]) == 0x3329F979F9A0BAA4
    assert int(emb.pacmap_key(7, 2, [12345])[0]) == 0x41058438DAB2E9D7
    assert list(emb.pacmap_draw(emb.pacmap_key(0, 1, [5] * 6), np.arange(6), 1000)) == [647, 110, 633, 631, 21, 57]
    assert list(emb.pacmap_draw(emb.pacmap_key(7, 2, [12345] * 4), np.arange(4), 16384)) == [5116, 15590, 11567, 7055]
    rng = np.random.default_rng(0)
    for _ in range(50):                                       # and the wrapping arithmetic against Python integers
        seed, stream, i, t = int(rng.integers(0, 1 << 62)), int(rng.integers(1, 3)), int(rng.integers(0, 1 << 22)), int(rng.integers(0, 5000))
        n = int(rng.integers(7, 1 << 22))
        assert int(emb.pacmap_draw(emb.pacmap_key(seed, stream, [i]), [t], n)[0]) == _draw(seed, stream, i, t, n)
    assert int(emb.pacmap_key(-1, 1, [3])[0]) == _mix(M64 ^ _mix((1 << 40) | 3))      # a negative seed is its 64-bit two's complement


def test_argument_rules():
    assert emb.check_pacmap_arguments(300) == (10, 5, 20, 60)
    assert emb.check_pacmap_arguments(9999)[0] == 10 and emb.check_pacmap_arguments(10000)[0] == 10
    assert emb.check_pacmap_arguments(100000) == (25, 12, 50, 64)                  # round(10 + 15 * (5 - 4)), round(12.5) = 12
    assert emb.check_pacmap_arguments(7, 2) == (2, 1, 4, 6)                        # kc = N - 1
    assert emb.check_pacmap_arguments(97, 32) == (32, 16, 64, 64)
    assert emb.check_pacmap_arguments(40, 1) == (1, 0, 2, 39)                      # round(0.5) = 0: no mid-near pairs
    for kwargs in (dict(n=96, n_neighbors=32), dict(n=6, n_neighbors=1), dict(n=7, n_neighbors=2, n_MN=2), dict(n=300, n_neighbors=33),
                   dict(n=300, n_neighbors=0), dict(n=300, n_MN=17), dict(n=300, n_FP=65), dict(n=30), dict(n=(1 << 22) + 1, n_neighbors=10),
                   dict(n=1 << 22)):
        with pytest.raises(ValueError):
            emb.check_pacmap_arguments(**kwargs)
    good = nc.make("a", 40, 5, 0)
    for bad in (np.nan, np.inf):
        x = good.copy()
        x[3, 2] = bad
        for fn in (emb.pacmap_preprocess, emb.pacmap_init, emb.pacmap_pairs, emb.pacmap):
            with pytest.raises(ValueError):
                fn(x)
    with pytest.raises(ValueError):
        emb.pacmap(good, init="random")
    with pytest.raises(ValueError):
        emb.pacmap(good, init=np.zeros((39, 2), np.float32))
    with pytest.raises(ValueError):
        ChessVision(lazy_load=True).reduce_embeddings(good, method="umap")


def test_preprocess_and_init():
    x = pc.table(pc.BY_ID["projected-300x513"])
    pre = emb.pacmap_preprocess(x)
    assert pre.shape == (300, 100) and pre.dtype == np.float32
    x64 = x.astype(np.float64)
    centred = x64 - x64.mean(0)
    w, v = np.linalg.eigh(np.cov(centred.T))
    var = (pre.astype(np.float64) ** 2).sum(0) / 299
    assert np.allclose(var, w[::-1][:100], rtol=1e-4) and (np.diff(var) <= 1e-4 * var[:-1]).all()          # descending eigenvalues
    for col in range(100):                                     # each column is the projection on one axis, largest component positive
        axis = v[:, ::-1][:, col]
        axis = axis * np.sign(axis[np.abs(axis).argmax()])
        assert np.allclose(pre[:, col], centred @ axis, atol=1e-4)
    assert np.array_equal(emb.pacmap_init(pre, projected=True), (0.01 * pre[:, :2].astype(np.float64)).astype(np.float32))
    low = pc.table(pc.BY_ID["iid-65x3"])
    pre = emb.pacmap_preprocess(low)
    scaled = (low.astype(np.float64) - low.min()) / (float(low.max()) - float(low.min()))
    assert np.allclose(pre, scaled - scaled.mean(0), atol=1e-6) and pre.shape == low.shape
    init = emb.pacmap_init(pre)
    assert init.shape == (65, 2) and init.dtype == np.float32
    assert np.var(init[:, 0]) >= np.var(init[:, 1]) > 0
    assert np.array_equal(emb.pacmap_preprocess(pc.table(pc.BY_ID["equal-64x4"])), np.zeros((64, 4), np.float32))
    assert (emb.pacmap_init(emb.pacmap_preprocess(pc.table(pc.BY_ID["least-7x1"])))[:, 1] == 0).all()


@pytest.mark.parametrize("case", STRUCTURE_CASES, ids=[c.id for c in STRUCTURE_CASES])
def test_pair_sets_have_the_structure_the_definition_gives_them(case):
    ref = pc.reference(case)
    pre, pairs = ref["pre"], ref["pairs"]
    n = case.n
    nn, nmn, nfp, kc = emb.check_pacmap_arguments(n, case.n_neighbors, case.n_MN, case.n_FP)
    assert pairs.neighbours.shape == (n, nn) and pairs.mid_near.shape == (n, nmn) and pairs.further.shape == (n, nfp)
    assert all(a.dtype == np.int32 for a in (pairs.neighbours, pairs.mid_near, pairs.further)) and pairs.stats["candidates"] == kc
    rows = np.arange(n)[:, None]
    for a in (pairs.neighbours, pairs.mid_near, pairs.further):
        assert ((a >= 0) & (a < n)).all() and (a != rows).all()
        s = np.sort(a, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()                  # none repeats inside a row
    assert not (pairs.further[:, :, None] == pairs.neighbours[:, None, :]).any()

    # neighbours: python tuples sorted, on distances recomputed by the brute force of tests/neighbour_cases.py
    d = nc.brute_sq_distances(pre, pre)
    others = d.copy()
    np.fill_diagonal(others, np.inf)
    hi = min(kc, 6)
    nearest = np.sort(others, axis=1)[:, :hi]
    sigma = [max(sum(math.sqrt(nearest[i, r]) for r in range(3, hi)) / (hi - 3), 1e-10) for i in range(n)]
    for i in range(0, n, max(1, n // 64)):
        cand = sorted((d[i, j], j) for j in range(n) if j != i)[:kc]
        want = sorted((dj / (sigma[i] * sigma[j]), j) for dj, j in cand)[:nn]
        assert [j for _, j in want] == list(pairs.neighbours[i]), i

    # mid-near and further: the draws replayed one by one with Python integers
    total_mid = total_far = 0
    for i in range(n):
        t, partners = 0, []
        for _ in range(nmn):
            held = []
            while len(held) < 6:
                j = _draw(case.seed, 1, i, t, n)
                t += 1
                if j != i and j not in held and j not in partners:
                    held.append(j)
            partners.append(sorted((d[i, j], j) for j in held)[1][1])
        total_mid += t
        assert partners == list(pairs.mid_near[i]), i
        t, held, near = 0, [], set(pairs.neighbours[i].tolist())
        while len(held) < nfp:
            j = _draw(case.seed, 2, i, t, n)
            t += 1
            if j != i and j not in near and j not in held:
                held.append(j)
        total_far += t
        assert held == list(pairs.further[i]), i
    assert pairs.stats["mid_near_draws"] == total_mid and pairs.stats["further_draws"] == total_far


def test_equal_rows_break_every_tie_by_index():
    pairs = pc.reference(pc.BY_ID["equal-64x4"])["pairs"]
    for i in (0, 5, 63):
        assert list(pairs.neighbours[i]) == [j for j in range(64) if j != i][:10]


def test_incidence_lists_are_in_the_defined_order():
    pairs = pc.reference(pc.BY_ID["shell-257x8"])["pairs"]
    offsets, entries = emb.pacmap_incidence(pairs)
    n = 257
    kinds = (pairs.neighbours, pairs.mid_near, pairs.further)
    want = [[(k, int(q)) for k, a in enumerate(kinds) for q in a[p]] for p in range(n)]
    for k, a in enumerate(kinds):                             # incoming: kind, then source ascending, then slot
        for src in range(n):
            for q in a[src]:
                want[int(q)].append((k + 10, src))
    per = sum(a.shape[1] for a in kinds)
    for p in range(n):                                        # a stable sort by kind keeps (source, slot) order
        want[p] = want[p][:per] + [(k - 10, q) for k, q in sorted(want[p][per:], key=lambda kq: kq[0])]
    assert offsets.dtype == np.int32 and entries.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == entries.size == 2 * n * per
    assert offsets[1] - offsets[0] - per > 200                # the centre is the neighbour of most of the shell
    for p in range(n):
        got = [(int(e) >> 28, int(e) & ((1 << 28) - 1)) for e in entries[offsets[p]:offsets[p + 1]]]
        assert got == want[p], p
    off2, ent2 = emb.pacmap_incidence(pairs, mid_near=False)
    for p in (0, 1, 200):
        assert list(ent2[off2[p]:off2[p + 1]]) == [e for e in entries[offsets[p]:offsets[p + 1]] if (int(e) >> 28) != 1]


def test_schedule():
    s = emb.pacmap_schedule(450)
    assert s.shape == (450, 4) and s.dtype == np.float32
    assert tuple(s[0, 1:]) == (2.0, 1000.0, 1.0) and tuple(s[99, 1:]) == (2.0, np.float32(0.01 * 1000 + 0.99 * 3), 1.0)
    assert tuple(s[100, 1:]) == tuple(s[199, 1:]) == (3.0, 3.0, 1.0) and tuple(s[200, 1:]) == tuple(s[449, 1:]) == (1.0, 0.0, 1.0)
    lr = [math.sqrt(1 - 0.999 ** (it + 1)) / (1 - 0.9 ** (it + 1)) for it in range(450)]
    assert np.allclose(s[:, 0], lr, rtol=1e-6, atol=0)        # the running products are within float32 rounding of the powers
    assert np.array_equal(emb.pacmap_schedule(7), s[:7])


@pytest.mark.parametrize("case_id", ["clusters-300x100", "shell-257x8"])
def test_gather_gradient_equals_a_float64_symmetric_scatter(case_id):
    """One iteration: the package's form -- every pair (i, j) adds w * (y_i - y_j) to i and subtracts it from j -- in float64 against
    the float32 gather over the incidence lists, to 1e-5 of the largest gradient component."""
    ref = pc.reference(pc.BY_ID[case_id])
    pairs = ref["pairs"]
    y = (ref["init"].astype(np.float64) * 100).astype(np.float32)              # spread out, so that the three kinds all matter
    w_n, w_mn, w_fp = 2.0, 1000.0, 1.0
    g = np.zeros(y.shape, np.float64)
    y64 = y.astype(np.float64)
    for a, (add, num, w, sign) in ((pairs.neighbours, (10.0, 20.0, w_n, 1.0)), (pairs.mid_near, (10000.0, 20000.0, w_mn, 1.0)),
                                   (pairs.further, (1.0, 2.0, w_fp, -1.0))):
        for i in range(a.shape[0]):
            for j in a[i]:
                e = y64[i] - y64[j]
                t = add + 1.0 + e @ e
                step = sign * w * (num / (t * t)) * e
                g[i] += step
                g[j] -= step
    got = emb._PacmapWalk(*emb.pacmap_incidence(pairs)).gradient(y, (w_n, w_mn, w_fp))
    assert got.dtype == np.float32
    assert np.abs(got - g).max() <= 1e-5 * np.abs(g).max(), (np.abs(got - g).max(), np.abs(g).max())


def test_first_step_is_adam_on_that_gradient():
    ref = pc.reference(pc.BY_ID["iid-65x3"])
    init, pairs = ref["init"], ref["pairs"]
    s = emb.pacmap_schedule(1)[0]
    g = emb._PacmapWalk(*emb.pacmap_incidence(pairs)).gradient(init, s[1:])
    f32 = np.float32
    m = f32(1.0 - 0.9) * g
    v = f32(1.0 - 0.999) * (g * g)
    want = init - (s[0] * m) / (np.sqrt(v) + f32(1e-7))
    assert np.array_equal(ref["coords"][1].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(emb.pacmap_optimise(init, pairs, 1), ref["coords"][1])
    assert np.array_equal(emb.pacmap_optimise(init, pairs, 0), init)


def test_seeds():
    case = pc.BY_ID["iid-65x3"]
    ref = pc.reference(case)
    other = emb.pacmap_pairs(ref["pre"], seed=1)
    assert np.array_equal(other.neighbours, ref["pairs"].neighbours)               # no draw goes into the neighbours
    assert not np.array_equal(other.mid_near, ref["pairs"].mid_near) and not np.array_equal(other.further, ref["pairs"].further)
    again = emb.pacmap(pc.table(case), seed=case.seed)
    assert again.coordinates.tobytes() == ref["coords"][450].tobytes()
    for name in ("neighbours", "mid_near", "further"):
        assert getattr(again.pairs, name).tobytes() == getattr(ref["pairs"], name).tobytes()
    assert again.n_neighbors == 10 and again.stats == ref["pairs"].stats


def test_chessvision_without_a_hip_model_runs_the_numpy_form():
    case = pc.BY_ID["iid-65x3"]
    got = ChessVision(lazy_load=True).reduce_embeddings(pc.table(case))
    assert got.coordinates.tobytes() == pc.reference(case)["coords"][450].tobytes()
    start = np.random.default_rng(0).standard_normal((65, 2)).astype(np.float32)
    seeded = ChessVision(lazy_load=True).reduce_embeddings(pc.table(case), n_neighbors=5, seed=3, init=start)
    assert seeded.n_neighbors == 5 and seeded.pairs.mid_near.shape == (65, 2) and seeded.pairs.further.shape == (65, 10)
    assert np.array_equal(seeded.coordinates, emb.pacmap(pc.table(case), n_neighbors=5, seed=3, init=start).coordinates)


def test_the_map_of_the_13_cluster_table_is_at_least_as_pure_as_its_pca_map():
    """Measured when the case was written (profiles/pacmap.md): the reduction 1.000, PCA-2 0.617."""
    case = pc.BY_ID["clusters-300x100"]
    labels = pc.clusters(case.n, case.c, case.seed)[1]
    ref = pc.reference(case)
    reduced, pca = pc.purity(ref["coords"][450], labels), pc.purity(ref["init"], labels)
    print(f"leave-one-out 1-NN purity: reduction {reduced:.4f}, PCA-2 {pca:.4f}")
    assert np.isfinite(ref["coords"][450]).all()
    assert reduced >= pca, (reduced, pca)
