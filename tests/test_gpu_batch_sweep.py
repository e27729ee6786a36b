"""GPU: both networks at every batch size the launch planner tells apart, engines at the DEFAULT chunk sizes, every output row checked.

``Engine::run_conv`` picks a launch form per layer from step functions of the images in the launch and of the chunk size the weights were
packed for (halo / generic kernel, the 256 -> 128-row fallback, split-K and its ragged last split, the 8 x 16 patch, position-major rows,
paired launches, the LDS-resident transposed conv from 8 boards, the split shortcut kernel from 1024 squares, the packed 8 x 8 image mode,
hipGraph replay).  The other GPU tests visit these forms at hand-picked sizes and mostly with small chunks; here the production engines
(64 images / 16384 squares per chunk) walk the sizes ``process_images`` really hands them:

  * UNet: N = 65 down to 1 (65 = the chunk loop with a one-image tail); ResNet: 64 k for k = 1..64 (every fourth k for ResNet-34), the
    ragged sizes of ``batch_sweep.RESNET_RAGGED``, 8192, 16384 and 16385;
  * at each size three forwards on the same device buffers (eager, capture, hipGraph replay where the engine replays at all), output
    poisoned with NaN before each: the first and third results are bit-identical, the numeric guard stays clean, and EVERY row of the third is
    inside the whole-model bars of tests/test_gpu_models.py against the torch CPU oracle of its pool input (``batch_sweep.row_figures``);
  * the ResNet u8 entry once per size: its soft-max within 1e-6 of the soft-max of the float path's logits;
  * one profiled forward per size -- the eager, unpaired, never-replayed form of the same layers -- checked the same way; the profile's
    (layer, kernel) pairs are the census;
  * the tripwire: every census class that begins at a size small enough to tap (UNet N <= 4, ResNet n <= 256) has its smallest member in
    ``test_gpu_layer_local.LAYER_LOCAL_AT_DEFAULT_CHUNK``, i.e. a layer-by-layer float64 check of that very form.

The f16 / f16r bars have about 2x of room, so their pools are first screened input by input in the forms the layer-local suite verifies
(``unet_chunk=2`` N = 1, ``resnet_chunk=128`` n = 64); an input over the bar there is replaced by the next seed, at most 2 of 11 images and
8 of 257 squares.  Each parameter appends one record to batch_sweep.jsonl beside the parity report of test_gpu_models.py; profiles/batch_sweep.md is ``batch_sweep.render`` of it.
"""
from __future__ import annotations

import json
import time

import pytest
import torch

import batch_sweep as bs
import layer_local as ll
import resnet34_ref
from chessvision import synthetic
from oracle import synth
from test_gpu_layer_local import LAYER_LOCAL_AT_DEFAULT_CHUNK
from test_gpu_models import OUT

pytestmark = pytest.mark.gpu

UNET_PARAMS = [("f32", False), ("f32", True), ("f16x3", False), ("f16x3", True), ("f16", False)]
RESNET_PARAMS = [("resnet18", p) for p in ("f32", "f16x3", "f16r", "f16")] + [("resnet34", p) for p in ("f16x3", "f16r")]
TAPPABLE = {"unet": 4, "resnet18": 256, "resnet34": 256}
NAN = float("nan")


_FAULT = []                                   # a forward that failed outright: nothing more is started on the device by this module


class _stop_after_a_fault:
    def __enter__(self):
        if _FAULT:
            pytest.fail(f"not run: an earlier sweep of this module ended in {_FAULT[0]}")

    def __exit__(self, kind, exc, tb):
        if exc is not None and not isinstance(exc, (AssertionError, GeneratorExit)) and not _FAULT:
            _FAULT.append(f"{kind.__name__}: {str(exc)[:200]}")
        return False


def _record(payload):
    try:
        OUT.mkdir(exist_ok=True)
        with open(OUT / "batch_sweep.jsonl", "a") as f:
            f.write(json.dumps(payload) + "\n")
    except OSError:
        pass


def _default_chunk_engine(prec):
    """HipEngine at the library's own chunk sizes, whatever the environment of the run says."""
    from chessvision.hip_backend import HipEngine

    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("CHESSVISION_HIP_UNET_CHUNK", raising=False)
        mp.delenv("CHESSVISION_HIP_RESNET_CHUNK", raising=False)
        return HipEngine(precision=prec)
    finally:
        mp.undo()


def _forward(eng, entry, x, n, out):
    status = getattr(eng._lib, entry)(eng._h, x.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if status != 0:
        raise RuntimeError(f"{entry} at n = {n}: status {status}, {eng._lib.cv_last_error()}")


class Sweep:
    """One parameter's walk: buffers, oracle rows, results per (n, stage), census."""

    def __init__(self, model, prec, variant, eng, x_pool, ref_pool, batches, u8_pool=None, replaced=None):
        self.model, self.prec, self.variant, self.eng = model, prec, variant, eng
        self.kind = "unet" if model == "unet" else "resnet"
        self.pool = x_pool.shape[0]
        self.batches = list(batches)
        self.x_pool, self.ref_pool = x_pool.cuda(), ref_pool.cuda()
        self.u8_pool = None if u8_pool is None else u8_pool.cuda()
        self.replaced = replaced or {}
        self.results, self.census, self.seconds = [], {}, {"three forwards": 0.0, "u8 entry": 0.0, "profiled forward": 0.0}
        self.not_identical = []

    def _figures(self, n, stage, fig, rows):
        fig.update(n=n, stage=stage, pool=int(rows[fig["row"]]), last_row=fig["row"] == n - 1)
        self.results.append(fig)

    def run(self):
        cap = max(self.batches)
        entry = "cv_unet_forward" if self.kind == "unet" else "cv_resnet18_forward"
        x = torch.empty((cap,) + tuple(self.x_pool.shape[1:]), device="cuda")
        out = torch.empty((cap,) + tuple(self.ref_pool.shape[1:]), device="cuda")
        x_u8 = None if self.u8_pool is None else torch.empty((cap, 64, 64), dtype=torch.uint8, device="cuda")
        probs = None if self.u8_pool is None else torch.empty((cap, 13), device="cuda")
        eng = self.eng
        for n in self.batches:                                       # largest first: the elastic workspace grows once
            rows = bs.pool_rows(n, self.pool)
            idx = torch.from_numpy(rows).cuda()
            torch.index_select(self.x_pool, 0, idx, out=x[:n])
            ref = self.ref_pool[idx]
            t0 = time.perf_counter()
            first = None
            for rep in range(3):                                     # the same pointers every time: eager, capture, replay
                out[:n].fill_(NAN)                                   # a call that wrote nothing must not pass on the previous call's rows
                _forward(eng, entry, x, n, out)
                if rep == 0:
                    first = out[:n].clone()
            eng.check_numerics()
            if not torch.equal(first, out[:n]):
                self.not_identical.append(n)
            self._figures(n, "three forwards", bs.row_figures(self.kind, self.prec, out[:n], ref), rows)
            logits = out[:n].clone()
            t1 = time.perf_counter()
            if x_u8 is not None:
                torch.index_select(self.u8_pool, 0, idx, out=x_u8[:n])
                probs[:n].fill_(NAN)
                _forward(eng, "cv_resnet18_forward_u8", x_u8, n, probs)
                eng.check_numerics()
                self._figures(n, "u8 entry", bs.u8_figures(probs[:n], logits), rows)
            t2 = time.perf_counter()
            out[:n].fill_(NAN)
            self.census[n] = bs.profile_into(eng, self.model, x, n, out)
            eng.check_numerics()
            self._figures(n, "profiled forward", bs.row_figures(self.kind, self.prec, out[:n], ref), rows)
            t3 = time.perf_counter()
            for key, dt in (("three forwards", t1 - t0), ("u8 entry", t2 - t1), ("profiled forward", t3 - t2)):
                self.seconds[key] += dt
        if x_u8 is None:
            self.seconds.pop("u8 entry")
        self.classes = bs.classes(self.census)
        _record({"model": self.model, "prec": self.prec, "variant": self.variant, "census": {str(n): s for n, s in self.census.items()},
                 "results": self.results, "replaced": {str(j): r for j, r in self.replaced.items()}, "seconds": self.seconds,
                 "thinned": False, "not_identical": self.not_identical})
        for key, s in self.seconds.items():
            print(f"batch sweep {self.model} {self.prec} {self.variant}: {key} {s:.1f} s over {len(self.batches)} sizes")
        for c in self.classes:
            print(f"batch sweep {self.model} {self.prec} {self.variant}: class n in {{{bs.ranges(c['members'], self.batches)}}}")
        return self

    def check(self, stage):
        """One AssertionError naming every failing size of ``stage``; each figure is printed before anything is asserted."""
        rs = [r for r in self.results if r["stage"] == stage]
        assert len(rs) == len(self.batches)
        for r in rs:
            print(f"{self.model} {self.prec} {self.variant} n={r['n']:5d} {stage}: {r['metric']} {r['err']:.3e} / {r['bar']:.3e} = {r['ratio']:.3f} "
                  f"row {r['row']} pool {r['pool']}")
        passing = [n for n in self.batches if all(r["ok"] for r in self.results if r["n"] == n)]
        bad = [r for r in rs if not r["ok"]]
        lines = []
        for r in bad[:12]:
            figures = ", ".join(f"{k} {v:.4g} (bar {b:.4g})" for k, (v, b) in r["figures"].items())
            lines.append(f"{self.model} {self.prec} {self.variant or '-'} n = {r['n']} [{stage}]: worst row {r['row']}"
                         f"{' (the last row)' if r['last_row'] else ''} = pool input {r['pool']}, {r['metric']} {r['err']:.3e} over bar {r['bar']:.3e}; "
                         f"{figures}\n  " + bs.describe_class(self.classes, r["n"], passing))
        assert not bad, f"{len(bad)} of {len(rs)} sizes outside the bar: n = {sorted(r['n'] for r in bad)}\n" + "\n".join(lines)


def _screened(cap, over_bar):
    return bs.screen_pool(over_bar, cap)


# ---- UNet -------------------------------------------------------------------------------------------------------------------------------
def _unet_pool(net, replaced):
    x = ll.unet_f32(bs.unet_pool_u8(replaced))
    with torch.no_grad():
        return x, net(x)


@pytest.fixture(scope="module", params=UNET_PARAMS, ids=[f"{p}-{'bilinear' if b else 'convT'}" for p, b in UNET_PARAMS])
def unet_sweep(request):
    from chessvision.hip_backend import HipEngine

    prec, bilinear = request.param
    with _stop_after_a_fault():
        yield from _unet_sweep(HipEngine, prec, bilinear)


def _unet_sweep(HipEngine, prec, bilinear):
    net = synth.make_unet(seed=1, bilinear=bilinear)
    replaced = {}
    if prec not in bs.F32_GRADE:                           # the pool input by input in the form the layer-local suite verifies
        small = HipEngine(precision=prec, unet_chunk=2)
        small.load_unet(net.state_dict())

        def over_bar(rep):
            x, ref = _unet_pool(net, rep)
            return [j for j in range(bs.UNET_POOL)
                    if not bs.row_figures("unet", prec, small.unet_forward(x[j:j + 1]), ref[j:j + 1].cuda())["ok"]]
        try:
            replaced = _screened(bs.UNET_MAX_REPLACED, over_bar)
        finally:
            small.close()
    x_pool, ref_pool = _unet_pool(net, replaced)
    eng = _default_chunk_engine(prec)
    eng.load_unet(net.state_dict())
    try:
        yield Sweep("unet", prec, "bilinear" if bilinear else "convT", eng, x_pool, ref_pool, bs.UNET_BATCHES, replaced=replaced).run()
    finally:
        eng.close()


def test_unet_three_forwards_on_fixed_buffers_every_row(unet_sweep):
    assert unet_sweep.not_identical == [], f"first and third forward differ in their bits at N = {unet_sweep.not_identical}"
    unet_sweep.check("three forwards")


def test_unet_profiled_eager_forward_every_row(unet_sweep):
    unet_sweep.check("profiled forward")


# ---- ResNet -----------------------------------------------------------------------------------------------------------------------------
def _resnet(arch):
    return synth.make_resnet(seed=2) if arch == "resnet18" else resnet34_ref.make_resnet34(synthetic.resnet34_state_dict(2))


def _resnet_pool(net, replaced):
    u8 = bs.resnet_pool_u8(replaced)
    x = ll.squares_f32(u8)
    with torch.no_grad():
        return torch.from_numpy(u8), x, net(x)


@pytest.fixture(scope="module", params=RESNET_PARAMS, ids=[f"{a}-{p}" for a, p in RESNET_PARAMS])
def resnet_sweep(request):
    from chessvision.hip_backend import HipEngine

    arch, prec = request.param
    with _stop_after_a_fault():
        yield from _resnet_sweep(HipEngine, arch, prec)


def _resnet_sweep(HipEngine, arch, prec):
    net = _resnet(arch)
    sd = {k: v for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    replaced = {}
    if prec not in bs.F32_GRADE:
        small = HipEngine(precision=prec, resnet_chunk=128)
        small.load_resnet(sd, arch)

        def over_bar(rep):
            _, x, ref = _resnet_pool(net, rep)
            bad = set()
            for lo in (0, 64, 128, 192, bs.RESNET_POOL - 64):          # n = 64 each; the last slice overlaps the one before
                got = small.resnet18_forward(x[lo:lo + 64])
                for j in range(64):                                   # row by row: arg-max agreement of ONE square is 0 or 1
                    if not bs.row_figures("resnet", prec, got[j:j + 1], ref[lo + j:lo + j + 1].cuda())["ok"]:
                        bad.add(lo + j)
            return bad
        try:
            replaced = _screened(bs.RESNET_MAX_REPLACED, over_bar)
        finally:
            small.close()
    u8_pool, x_pool, ref_pool = _resnet_pool(net, replaced)
    eng = _default_chunk_engine(prec)
    eng.load_resnet(sd, arch)
    try:
        yield Sweep(arch, prec, "", eng, x_pool, ref_pool, bs.resnet_batches(4 if arch == "resnet34" else 1), u8_pool=u8_pool,
                    replaced=replaced).run()
    finally:
        eng.close()


def test_resnet_three_forwards_on_fixed_buffers_every_row(resnet_sweep):
    assert resnet_sweep.not_identical == [], f"first and third forward differ in their bits at n = {resnet_sweep.not_identical}"
    resnet_sweep.check("three forwards")


def test_resnet_u8_entry_is_the_softmax_of_the_float_path_every_row(resnet_sweep):
    resnet_sweep.check("u8 entry")


def test_resnet_profiled_eager_forward_every_row(resnet_sweep):
    resnet_sweep.check("profiled forward")


# ---- the tripwire -----------------------------------------------------------------------------------------------------------------------
def _tripwire(sweep):
    listed = [n for (model, prec, variant, n) in LAYER_LOCAL_AT_DEFAULT_CHUNK if (model, prec, variant) == (sweep.model, sweep.prec, sweep.variant)]
    missing = bs.tripwire(sweep.classes, listed, TAPPABLE[sweep.model])
    text = []
    for n in missing:
        k = next(i for i, c in enumerate(sweep.classes) if c["smallest"] == n)
        diff = bs.signature_diff(sweep.classes[k]["signature"], sweep.classes[k - 1]["signature"]) if k else []
        text.append(f"({sweep.model!r}, {sweep.prec!r}, {sweep.variant!r}, {n}): a launch form of its own for n in "
                    f"{{{bs.ranges(sweep.classes[k]['members'], sweep.batches)}}}" + "".join(f"\n    {layer}: {ka}   (class before: {kb})" for layer, ka, kb in diff))
    assert not missing, ("census classes without a layer-local case at the default chunk -- add them to "
                         "test_gpu_layer_local.LAYER_LOCAL_AT_DEFAULT_CHUNK:\n  " + "\n  ".join(text))


def test_unet_every_small_batch_form_has_its_layer_local_case(unet_sweep):
    _tripwire(unet_sweep)


def test_resnet_every_small_batch_form_has_its_layer_local_case(resnet_sweep):
    _tripwire(resnet_sweep)
