"""GPU: YOLOv8-cls, all five scales, at the batch sizes of a full chunk, the chunk loop with a one-square tail and the small launches,
engines at the DEFAULT chunk size, every output row checked.  A sibling of tests/test_gpu_batch_sweep.py on its scaffolding
(``batch_sweep.pool_rows``, ``Sweep``, the rule that nothing more is started on the device after a forward that failed outright).

  * engines: all five scales at f16x3, n also at f32 (f16 has no whole-model bar in this project; its layers are held one by one by
    tests/test_gpu_yolov8_layer_local.py).  ``yolo_cls_load`` halves the chunk of l and x to 8192 (no workspace tensor may reach 4 GiB):
    ``CHUNK`` states it and the sweep asserts it, so 16385 / 16384 / 8193 / 8192 cover a full chunk and a one-square tail of both;
  * oracle: the float64 helper (``yolov8_cls_ref.make(...).double()``) on the 257 squares of ``batch_sweep.resnet_pool_u8``, once per scale;
  * at each size three forwards on the same device buffers, the output poisoned with NaN before each: first and third bit-identical,
    clean guard, every row of the third within 1e-3 max(1, max|ref row|) of its oracle row (the rule of test_layer_taps_match_the_helper;
    the float32 helper alone sits at 0.002 of it or less);
  * duplicate rows: rows i and i + 257 hold the same pool input; inside one chunk of one forward they are bit-equal -- a square's
    arithmetic does not depend on its place in the batch.  No tolerance;
  * the u8 entry once per size: its soft-max within 1e-6 of the soft-max of the float path's logits;
  * at 1025 and at the largest size the (row, 1280) embedding within 1e-3 max(1, max|ref row|) of the helper's pooled features, and the
    logits of that call bit-equal to the call without it.

One line per (scale, precision, n) goes to yolov8_batch_sweep.jsonl beside the parity report; profiles/yolov8_cls_parity.md is made from it.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import batch_sweep as bs  # noqa: E402
import layer_local as ll  # noqa: E402
import yolov8_cls_ref  # noqa: E402
from chessvision import synthetic  # noqa: E402
from test_gpu_batch_sweep import NAN, Sweep, _default_chunk_engine, _forward, _stop_after_a_fault  # noqa: E402
from test_gpu_models import OUT  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = [("n", "f32")] + [(s, "f16x3") for s in ("n", "s", "m", "l", "x")]
SIZES = (16385, 16384, 8193, 8192, 4097, 1025, 1024, 1000, 256, 100, 65, 64, 63, 7, 1)       # largest first: the workspace grows once
EMBEDDING_AT = (1025, max(SIZES))
CHUNK = {"n": 16384, "s": 16384, "m": 16384, "l": 8192, "x": 8192}      # yolo_cls_load: worst tensor x 4 bytes x chunk < 2^32
ROW_BAR = 1e-3                                                          # x max(1, max|ref row|)


def _record(payload):
    try:
        OUT.mkdir(exist_ok=True)
        with open(OUT / "yolov8_batch_sweep.jsonl", "a") as f:
            f.write(json.dumps(payload) + "\n")
    except OSError:
        pass


_ORACLES = {}


def _oracle(scale):
    """(state dict, pool as bytes, pool as float32, float64 logits (257, 13), float64 pooled features (257, 1280)) -- once per scale"""
    if scale not in _ORACLES:
        _ORACLES.clear()                                                  # one scale at a time: x's weights are large
        sd = synthetic.yolov8_cls_state_dict(2, scale)
        net = yolov8_cls_ref.make(scale, sd).double()
        u8 = bs.resnet_pool_u8()
        x = ll.squares_f32(u8)
        with torch.no_grad():
            pooled = torch.cat([net.pooled(x[lo:lo + 64].double()) for lo in range(0, bs.RESNET_POOL, 64)])
            logits = net.model[9].linear(pooled)
        _ORACLES[scale] = (sd, torch.from_numpy(u8), x, logits, pooled)
    return _ORACLES[scale]


def rel_row_figures(got: torch.Tensor, ref: torch.Tensor, metric: str) -> dict:
    """Every row of ``got`` within ROW_BAR x max(1, max|ref row|) of its float64 oracle row; a NaN is a failure."""
    d = (got.to(torch.float64) - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))).amax(1)
    bar = ROW_BAR * ref.abs().amax(1).clamp_min(1.0)
    ratio = d / bar
    row = int(ratio.argmax())
    return {"ok": bool((d <= bar).all()), "ratio": float(ratio[row]), "metric": metric, "row": row, "err": float(d[row]), "bar": float(bar[row]),
            "figures": {metric: (float(d[row]), float(bar[row]))}}


def _rows_in_the_workspace(eng, model) -> int:
    """Rows of the chunk the last forward left behind: the size query of ``cv_activation_channel_means`` (nothing is launched)."""
    import ctypes

    dims = (ctypes.c_int64 * 2)()
    assert eng._lib.cv_activation_channel_means(eng._h, model.encode(), b"model.9.conv", None, 0, dims, None) == 0, eng._lib.cv_last_error()
    return int(dims[0])


class YoloSweep(Sweep):
    """``Sweep`` with this file's checks per size; ``check(stage)`` and its failure text are the parent's."""

    def __init__(self, scale, prec, eng, x_pool, ref_logits, ref_pooled, u8_pool):
        super().__init__(f"yolov8{scale}-cls", prec, "", eng, x_pool, ref_logits, SIZES, u8_pool=u8_pool)
        self.scale, self.ref_pooled = scale, ref_pooled.cuda()
        self.unequal_duplicates, self.pairs_checked, self.chunk_rows, self.emb_logits_differ = [], {}, {}, []
        self.seconds = {"three forwards": 0.0, "u8 entry": 0.0, "embedding": 0.0}

    def run(self):
        cap, eng, chunk = max(self.batches), self.eng, CHUNK[self.scale]
        x = torch.empty((cap, 1, 64, 64), device="cuda")
        out = torch.empty((cap, 13), device="cuda")
        x_u8 = torch.empty((cap, 64, 64), dtype=torch.uint8, device="cuda")
        probs = torch.empty((cap, 13), device="cuda")
        for n in self.batches:
            rows = bs.pool_rows(n, self.pool)
            idx = torch.from_numpy(rows).cuda()
            torch.index_select(self.x_pool, 0, idx, out=x[:n])
            ref = self.ref_pool[idx]
            t0 = time.perf_counter()
            first = None
            for rep in range(3):                                     # the same pointers every time: eager, capture, replay
                out[:n].fill_(NAN)
                _forward(eng, "cv_resnet18_forward", x, n, out)
                if rep == 0:
                    first = out[:n].clone()
            eng.check_numerics()
            if not torch.equal(first, out[:n]):
                self.not_identical.append(n)
            self._figures(n, "three forwards", rel_row_figures(out[:n], ref, "logit"), rows)
            logits = out[:n].clone()
            # the rows the last chunk left in the workspace: n = chunk + 1 leaves one, a full chunk all of them
            self.chunk_rows[n] = _rows_in_the_workspace(eng, self.model)
            pairs = 0
            for lo in range(0, n, chunk):                            # rows i and i + 257 of one chunk hold the same pool input
                hi = min(n, lo + chunk)
                if hi - lo > self.pool:
                    pairs += hi - lo - self.pool
                    same = (logits[lo:hi - self.pool] == logits[lo + self.pool:hi]).all(1)
                    if not bool(same.all()):
                        i = lo + int((~same).to(torch.int8).argmax())
                        self.unequal_duplicates.append((n, i, i + self.pool, int((~same).sum())))
            self.pairs_checked[n] = pairs
            t1 = time.perf_counter()
            torch.index_select(self.u8_pool, 0, idx, out=x_u8[:n])
            probs[:n].fill_(NAN)
            _forward(eng, "cv_resnet18_forward_u8", x_u8, n, probs)
            eng.check_numerics()
            self._figures(n, "u8 entry", bs.u8_figures(probs[:n], logits), rows)
            t2 = time.perf_counter()
            if n in EMBEDDING_AT:
                got, emb = eng.resnet18_forward(x[:n], want_embedding=True)
                if not torch.equal(got, logits):
                    self.emb_logits_differ.append(n)
                self._figures(n, "embedding", rel_row_figures(emb, self.ref_pooled[idx], "embedding"), rows)
            t3 = time.perf_counter()
            for key, dt in (("three forwards", t1 - t0), ("u8 entry", t2 - t1), ("embedding", t3 - t2)):
                self.seconds[key] += dt
            w = next(r for r in self.results if r["n"] == n and r["stage"] == "three forwards")
            _record({"model": self.model, "prec": self.prec, "n": n, "chunk": chunk, "rows_of_last_chunk": self.chunk_rows[n],
                     "identical": n not in self.not_identical, "duplicate_pairs": pairs,
                     "duplicates_equal": not any(u[0] == n for u in self.unequal_duplicates),
                     "results": [r for r in self.results if r["n"] == n], "worst_row_ratio": w["ratio"], "ok": w["ok"]})
        self.classes = []                                            # no census here: the forms are tests/test_gpu_yolov8_layer_local.py's
        for key, s in self.seconds.items():
            print(f"batch sweep {self.model} {self.prec}: {key} {s:.1f} s over {len(self.batches)} sizes")
        return self

    def check(self, stage, sizes=None):
        """The parent's check over the sizes of ``stage``, without the census text (this sweep has none)."""
        sizes = list(self.batches if sizes is None else sizes)
        rs = [r for r in self.results if r["stage"] == stage]
        assert [r["n"] for r in rs] == sizes, ([r["n"] for r in rs], sizes)
        for r in rs:
            print(f"{self.model} {self.prec} n={r['n']:5d} {stage}: {r['metric']} {r['err']:.3e} / {r['bar']:.3e} = {r['ratio']:.4f} "
                  f"row {r['row']} pool {r['pool']}")
        bad = [r for r in rs if not r["ok"]]
        assert not bad, f"{len(bad)} of {len(rs)} sizes outside the bar:\n" + "\n".join(
            f"{self.model} {self.prec} n = {r['n']} [{stage}]: worst row {r['row']}{' (the last row)' if r['last_row'] else ''} = pool input "
            f"{r['pool']}, {r['metric']} {r['err']:.3e} over bar {r['bar']:.3e}" for r in bad)


@pytest.fixture(scope="module", params=PARAMS, ids=[f"{s}-{p}" for s, p in PARAMS])
def sweep(request):
    scale, prec = request.param
    with _stop_after_a_fault():
        sd, u8_pool, x_pool, ref_logits, ref_pooled = _oracle(scale)
        eng = _default_chunk_engine(prec)
        try:
            eng.load_yolo_cls(sd, f"yolov8{scale}-cls")
            yield YoloSweep(scale, prec, eng, x_pool, ref_logits, ref_pooled, u8_pool).run()
        finally:
            eng.close()


def test_three_forwards_on_fixed_buffers_every_row(sweep):
    assert sweep.not_identical == [], f"first and third forward differ in their bits at n = {sweep.not_identical}"
    sweep.check("three forwards")


def test_full_chunks_and_one_square_tails_are_what_the_sizes_say(sweep):
    """The 4 GiB rule of yolo_cls_load: 16384 squares per chunk, 8192 for l and x; ``chunk + 1`` runs the chunk loop with a tail of one."""
    chunk = CHUNK[sweep.scale]
    want = {n: (n - 1) % chunk + 1 for n in SIZES}
    assert sweep.chunk_rows == want, (sweep.chunk_rows, want)
    assert want[chunk] == chunk and want[chunk + 1] == 1 and want[16385] == 1


def test_rows_holding_the_same_square_in_one_chunk_are_bit_equal(sweep):
    for n, pairs in sweep.pairs_checked.items():
        print(f"{sweep.model} {sweep.prec} n={n:5d}: {pairs} duplicate pairs compared")
    assert all(sweep.pairs_checked[n] > 0 for n in SIZES if n > bs.RESNET_POOL) and sweep.pairs_checked[256] == 0
    assert sweep.unequal_duplicates == [], "rows of one chunk that hold the same pool input differ in their bits: " + "; ".join(
        f"n = {n}: rows {i} and {j} ({k} pairs of that chunk differ)" for n, i, j, k in sweep.unequal_duplicates[:12])


def test_u8_entry_is_the_softmax_of_the_float_path_every_row(sweep):
    sweep.check("u8 entry")


def test_embeddings_match_the_pooled_features_and_change_no_logit(sweep):
    assert sweep.emb_logits_differ == [], f"asking for the embedding changed a logit at n = {sweep.emb_logits_differ}"
    sweep.check("embedding", sizes=[n for n in SIZES if n in EMBEDDING_AT])
