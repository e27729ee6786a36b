"""Measurements behind profiles/embedding_neighbours.md: time of one ``cv_embedding_neighbours`` call at the three shapes of interest,
the certified share, the price of ``exact_only``, the same graph by CPU brute force, and the certified share on embeddings the
pipeline itself produced (a 256-board ``process_images`` job with the synthetic weights; the eight committed real photos).

    python tests/dev/neighbours_bench.py --out neighbours.json                 # everything, device events around whole calls
    rocprofv3 --kernel-trace -d DIR -o nb -- python tests/dev/neighbours_bench.py --trace-only
                                                                               # per-kernel split: CALLS_PER_SHAPE calls per shape, in SHAPES order

Needs an MI355X; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")]

from chessvision import ChessVision, embeddings, hip_backend as hb, synthetic  # noqa: E402

SHAPES = [(16384, 16384, 512), (4096, 4096, 1024), (4, 65536, 512)]           # (q, n, c); q == n: the table against itself
K = 10
CALLS_PER_SHAPE = 3                                                           # --trace-only: one warm-up + two traced calls
MFMA_F32_TFLOPS = 155.0                                                       # measured exact-f32 MFMA rate of the MI355X


def table(n: int, c: int, seed: int) -> torch.Tensor:
    """13 clusters of spread 0.15 around post-ReLU centres, generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.relu(torch.randn((13, c), generator=g, device="cuda"))
    which = torch.randint(0, 13, (n,), generator=g, device="cuda")
    return (centres[which] + 0.15 * torch.randn((n, c), generator=g, device="cuda")).contiguous()


def tables(q: int, n: int, c: int):
    corpus = table(n, c, 1)
    return (corpus, corpus, True) if q == n else (table(q, c, 2), corpus, False)


def timed(eng, a, b, self_graph, exact_only=False, reps=5, min_ms=300.0):
    """Median, min and max of single calls between device events, after two warm-up calls; reps grows until the window holds min_ms."""
    for _ in range(2):
        out = eng.embedding_neighbours_dev(a, b, K, exclude_self=self_graph, exact_only=exact_only)
    torch.cuda.synchronize()
    times = []
    while len(times) < reps or (sum(times) < min_ms and len(times) < 200):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = eng.embedding_neighbours_dev(a, b, K, exclude_self=self_graph, exact_only=exact_only)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    stats = out[2].cpu().numpy()
    return {"ms_median": float(np.median(times)), "ms_min": min(times), "ms_max": max(times), "calls": len(times),
            "stats": {name: int(stats[i]) for i, name in enumerate(hb.NEIGHBOUR_STATS)}}, out


def cpu_brute(a: np.ndarray, b: np.ndarray, self_graph: bool) -> dict:
    """The same graph on the host in float32, 16 threads: scikit-learn's brute force where installed, else the numpy GEMM form."""
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    try:
        from sklearn.neighbors import NearestNeighbors

        nn = NearestNeighbors(n_neighbors=K + (1 if self_graph else 0), algorithm="brute", n_jobs=16).fit(b)
        nn.kneighbors(a)
        how = "sklearn NearestNeighbors(algorithm='brute', n_jobs=16)"
    except ImportError:
        nb = (b * b).sum(1)
        for lo in range(0, a.shape[0], 2048):
            d = (a[lo:lo + 2048] ** 2).sum(1)[:, None] + nb[None, :] - 2.0 * (a[lo:lo + 2048] @ b.T)
            np.argpartition(d, K, axis=1)
        how = "numpy float32 GEMM form + argpartition"
    return {"seconds": time.perf_counter() - t0, "how": how}


def certified_share(eng, tab: np.ndarray, k: int = K) -> dict:
    got = eng.embedding_neighbours(tab, k=k)
    finite = got.stats["query_rows"] - got.stats["nonfinite_query_rows"]
    return {"rows": int(tab.shape[0]), "channels": int(tab.shape[1]), "certified": got.stats["certified_rows"], "exact": got.stats["exact_rows"],
            "share": got.stats["certified_rows"] / max(1, finite)}


def pipeline_tables(out: dict, tmp: Path) -> None:
    pe, pc = synthetic.save_checkpoints(tmp, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3")
    eng = cv.classifier.engine
    jobs = {"synthetic256": [synthetic.board_photo(2000 + s) for s in range(256)],
            "real8": [np.ascontiguousarray(np.load(ROOT / "tests" / "golden" / f"photos8_{i}.npz")["bgr"][0]) for i in range(8)]}
    for name, photos in jobs.items():
        results = cv.process_images(photos, embeddings=True, fallback_quad=True, return_crops=False)
        for which in ("board_extractor", "classifier"):
            tab, _ = embeddings.stack(results, which)
            if tab.shape[0] > 1:
                out[f"{name}/{which}"] = certified_share(eng, tab, min(K, tab.shape[0] - 1))
    cv.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="neighbours_bench.json")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--tmp", default="/tmp/neighbours_bench_weights")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    eng = hb.HipEngine(precision="f32")
    if args.trace_only:
        for q, n, c in SHAPES:
            a, b, self_graph = tables(q, n, c)
            for _ in range(CALLS_PER_SHAPE):
                eng.embedding_neighbours_dev(a, b, K, exclude_self=self_graph)
            torch.cuda.synchronize()
        a, b, self_graph = tables(*SHAPES[0])
        eng.embedding_neighbours_dev(a, b, K, exclude_self=self_graph, exact_only=True)
        torch.cuda.synchronize()
        return
    report: dict = {"k": K, "shapes": {}}
    for q, n, c in SHAPES:
        a, b, self_graph = tables(q, n, c)
        entry, _ = timed(eng, a, b, self_graph)
        entry["filter_flop"] = 2.0 * q * n * c
        entry["whole_call_tflops"] = entry["filter_flop"] / (entry["ms_median"] * 1e-3) / 1e12
        entry["whole_call_share_of_f32_mfma"] = entry["whole_call_tflops"] / MFMA_F32_TFLOPS
        entry["scratch_bytes"] = int(eng._lib.cv_embedding_neighbours_scratch_bytes(q, n, c, K))
        entry["cpu"] = cpu_brute(a.cpu().numpy(), b.cpu().numpy(), self_graph)
        report["shapes"][f"{q}x{n}x{c}"] = entry
        print(json.dumps({f"{q}x{n}x{c}": entry}), flush=True)
        if (q, n, c) == SHAPES[0]:
            exact, _ = timed(eng, a, b, self_graph, exact_only=True, reps=2, min_ms=0.0)
            report["exact_only_16384x16384x512"] = exact
            print(json.dumps({"exact_only": exact}), flush=True)
    report["pipeline"] = {}
    os.makedirs(args.tmp, exist_ok=True)
    pipeline_tables(report["pipeline"], Path(args.tmp))
    print(json.dumps(report["pipeline"]), flush=True)
    Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
