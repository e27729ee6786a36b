"""Measurements behind profiles/pacmap_place.md: placing 64, 1024 and 16384 new rows into a map fitted on a 1024 x 512 and on a
16384 x 512 table (the tables of tests/dev/pacmap_bench.py) -- device time of one ``cv_pacmap_place_pairs`` call and of one
450-iteration ``cv_pacmap_place`` call, the host preprocessing of the new rows, the numpy form's time beside them (and whether the
two agree: pairs index for index, coordinates bit for bit), and what the parent offers for the same rows: ``reduce_embeddings`` of
basis plus new rows, host steps included, run in alternation with the whole placement (host steps included as well).

    python tests/dev/pacmap_place_bench.py --out pacmap_place_bench.json [--numpy-all]

Device times are device events around single calls after two warm-up calls, profiler off; whole-call times are the host clock around
a call that ends with the result on the host.  Needs an MI355X; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests"), str(ROOT / "tests" / "dev")]

from chessvision import embeddings as emb, hip_backend as hb  # noqa: E402
from pacmap_bench import ITERATIONS, SHAPES, note, table, timed  # noqa: E402

NEW_ROWS = (64, 1024, 16384)
NUMPY_LIMIT = 1 << 24                          # new rows x basis rows of the float64 brute-force search timed by default


def device_fit(eng, x: np.ndarray) -> emb.EmbeddingMap:
    """``ChessVision.fit_embedding_map`` on a bare engine."""
    pre, start, parameters = emb.pacmap_fit_inputs(x)
    pairs = eng.pacmap_pairs(pre, seed=0)
    nn = int(pairs.neighbours.shape[1])
    sigma = eng.pacmap_basis_scale_dev(torch.from_numpy(pre).cuda(), nn).cpu().numpy()
    return emb.map_from_fit(emb.Reduction(eng.pacmap_optimise(start, pairs), pairs, nn, pairs.stats), pre, sigma, parameters)


def device_place(eng, m: emb.EmbeddingMap, rows: np.ndarray) -> emb.Placement:
    """``ChessVision.place_embeddings`` on a bare engine: host preprocessing, uploads, both device calls, the result on the host."""
    pre_new, start = emb.pacmap_transform_inputs(m, rows)
    nbr, stats = eng.pacmap_place_pairs(m, pre_new)
    return emb.Placement(eng.pacmap_place(start, m.reduction.coordinates, nbr), nbr, stats)


def device_refit(eng, x: np.ndarray) -> np.ndarray:
    """``ChessVision.reduce_embeddings`` on a bare engine: what the parent offers for the same rows."""
    pre, start = emb.pacmap_inputs(x)
    return eng.pacmap_optimise(start, eng.pacmap_pairs(pre, seed=0))


def clock(call, reps: int = 3) -> dict:
    call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(times)), "ms_min": min(times), "ms_max": max(times), "calls": reps}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="pacmap_place_bench.json")
    ap.add_argument("--numpy-all", action="store_true", help="time the numpy form at 16384 new rows over 16384 basis rows too")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    out = Path(args.out)
    eng = hb.HipEngine(precision="f32")
    report: dict = {"iterations": ITERATIONS, "shapes": {}}

    for n, c in SHAPES:
        x = table(n, c, 1)
        t0 = time.perf_counter()
        m = device_fit(eng, x)
        shape = {"fit_s": time.perf_counter() - t0, "n_neighbors": m.reduction.n_neighbors, "new_rows": {}}
        pre_dev, sigma_dev = torch.from_numpy(m.pre).cuda(), torch.from_numpy(m.sigma).cuda()
        basis_dev = torch.from_numpy(m.reduction.coordinates).cuda()
        shape["basis_scale"] = timed(lambda: eng.pacmap_basis_scale_dev(pre_dev, m.reduction.n_neighbors))
        report["shapes"][f"{n}x{c}"] = shape
        for q in NEW_ROWS:
            rows = table(q, c, 1)[::-1].copy() + np.float32(0.01)          # the basis' clusters (same seed, so same centres), other rows
            t0 = time.perf_counter()
            pre_new, start = emb.pacmap_transform_inputs(m, rows)
            entry = {"host_preprocess_ms": (time.perf_counter() - t0) * 1e3}
            new_dev, start_dev = torch.from_numpy(pre_new).cuda(), torch.from_numpy(start).cuda()
            entry["pairs"] = timed(lambda: eng.pacmap_place_pairs_dev(new_dev, pre_dev, sigma_dev, m.reduction.n_neighbors))
            nbr_dev, stats = eng.pacmap_place_pairs_dev(new_dev, pre_dev, sigma_dev, m.reduction.n_neighbors)
            entry["pairs"]["stats"] = [int(v) for v in stats.cpu().numpy()]
            entry["place"] = timed(lambda: eng.pacmap_place_dev(start_dev, basis_dev, nbr_dev, ITERATIONS))
            got_pairs, got = nbr_dev.cpu().numpy(), eng.pacmap_place_dev(start_dev, basis_dev, nbr_dev, ITERATIONS).cpu().numpy()
            whole = np.concatenate([x, rows])
            for k in range(2):                                             # in alternation: placement, then the parent's refit
                entry.setdefault("whole_placement", []).append(clock(lambda: device_place(eng, m, rows)))
                entry.setdefault("parent_refit_of_basis_plus_new", []).append(clock(lambda: device_refit(eng, whole)))
            shape["new_rows"][str(q)] = entry
            note(out, report, json.dumps({f"{q} into {n}x{c}": entry}))
            if q * n > NUMPY_LIMIT and not args.numpy_all:
                continue
            t0 = time.perf_counter()
            want_pairs = emb.pacmap_place_pairs(m, pre_new)
            entry["numpy_pairs_s"] = time.perf_counter() - t0
            entry["pairs_equal"] = bool(np.array_equal(got_pairs, want_pairs))
            t0 = time.perf_counter()
            want = emb.pacmap_place(start, m.reduction.coordinates, want_pairs, ITERATIONS)
            entry["numpy_place_s"] = time.perf_counter() - t0
            entry["coordinates_bit_identical"] = bool(np.array_equal(want.view(np.uint32), got.view(np.uint32)))
            note(out, report, json.dumps({f"{q} into {n}x{c} numpy": [entry["numpy_pairs_s"], entry["numpy_place_s"]],
                                          "equal": [entry["pairs_equal"], entry["coordinates_bit_identical"]]}))
    eng.close()


if __name__ == "__main__":
    main()
