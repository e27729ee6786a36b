"""Batch-size sweep: both networks at every batch size the launch planner tells apart, every output row against the torch CPU oracle.

TEST INFRASTRUCTURE -- a plain module (no conftest) beside tests/layer_local.py; imports nothing from ``chessvision.hip_backend`` (the
engine is handed in), so tests/test_batch_sweep_cpu.py drives everything but ``census`` without a GPU.

``Engine::run_conv`` picks a launch form per layer from step functions of the images in the launch and of the chunk size the weights were
packed for.  The sweep runs engines at the DEFAULT chunk sizes over the whole range of batch sizes production hands them, and

  * ``pool_index`` decides which input sits in which row: the pools (11 images, 257 squares) are coprime to every tile, image-group and
    chunk size of the engine, so no two rows a tiling bug could swap hold the same input, and the index also moves with ``n``, so a given
    input meets every row position over the sweep;
  * ``census`` asks the engine's own profile which kernel ran each layer at each n; ``classes`` groups the n with identical answers:
    a class is one launch form of the whole network, its smallest member is the first n at which that form appears;
  * ``row_figures`` holds every row to the whole-model bars of tests/test_gpu_models.py (``BARS``; none is new);
  * ``screen_pool`` applies the replacement rule of the f16 / f16r pools; ``render`` writes profiles/batch_sweep.md.
"""
from __future__ import annotations

import json
import sys
from collections import OrderedDict

import numpy as np
import torch

import layer_local as ll

UNET_POOL, RESNET_POOL = 11, 257
UNET_KINDS = ("random", "photo", "border", "random", "photo", "random", "photo", "random", "photo", "random", "photo")
UNET_SEED, RESNET_SEED, RESNET_SPECIALS_AT = 101, 103, 120
UNET_MAX_REPLACED, RESNET_MAX_REPLACED = 2, 8

UNET_BATCHES = tuple(range(65, 0, -1))                                   # 65 = the default chunk + 1: the chunk loop with a one-image tail
RESNET_RAGGED = (1, 7, 63, 65, 100, 1000, 1023, 1024, 1025, 4095, 4097)
RESNET_LARGE = (8192, 16384, 16385)                                       # 16385 = the default chunk + 1


def resnet_batches(every_kth: int = 1) -> tuple:
    """64 k for k = 1..64 (``every_kth``: every fourth k for ResNet-34) + the ragged sizes + 8192, 16384, 16385; largest first."""
    ks = [64 * k for k in range(1, 65) if k % every_kth == 0]
    return tuple(sorted(set(ks) | set(RESNET_RAGGED) | set(RESNET_LARGE), reverse=True))


# ---- which input sits in which row ----------------------------------------------------------------------------------------------
def pool_index(i, n: int, pool: int):
    """Pool input in row ``i`` of a batch of ``n`` (``i`` an int or an integer array)."""
    return (i + 3 * n) % pool


def pool_rows(n: int, pool: int) -> np.ndarray:
    return pool_index(np.arange(n, dtype=np.int64), n, pool)


# ---- the pools --------------------------------------------------------------------------------------------------------------------
def unet_slot(j: int, replaced: int = 0):
    """(kind, seed) of UNet pool slot ``j`` after ``replaced`` replacements: the next seed; the border image has no seed and gives way to
    random bytes."""
    kind = UNET_KINDS[j]
    if replaced and kind == "border":
        kind = "random"
    return kind, UNET_SEED + 7 * j + 1000 * replaced


def unet_pool_u8(replaced: dict | None = None) -> np.ndarray:
    """(11, 256, 256, 3) uint8; ``replaced`` = {slot: how many times it was replaced}."""
    replaced = replaced or {}
    out = np.zeros((UNET_POOL, 256, 256, 3), dtype=np.uint8)
    for j in range(UNET_POOL):
        kind, seed = unet_slot(j, replaced.get(j, 0))
        out[j] = ll.unet_images_u8(seed, [kind])[0]
    return out


def resnet_pool_u8(replaced: dict | None = None) -> np.ndarray:
    """(257, 64, 64) uint8: random squares with the nine special ones in a row; a replaced slot takes the random square of the next seed."""
    replaced = replaced or {}
    sq = ll.squares_u8(RESNET_SEED, RESNET_POOL, ll.specials_from(RESNET_SPECIALS_AT))
    for j, r in replaced.items():
        if r:
            sq[j] = ll.squares_u8(RESNET_SEED + r, RESNET_POOL, {})[j]
    return sq


# ---- the bars of tests/test_gpu_models.py ---------------------------------------------------------------------------------------------
F32_GRADE = ("f32", "f16x3")
BARS = {
    "unet": {"f32": {"logit_abs": 1e-3, "iou": 0.9999}, "f16": {"logit_rel": 5e-3, "iou": 0.995, "prob": 2e-2}},
    "resnet": {"f32": {"logit_abs": 1e-3, "agree": 1.0}, "f16": {"logit_rel": 5e-3, "prob": 1e-3, "agree": 0.99}},
}
U8_SOFTMAX_BAR = 1e-6


def bars_for(model: str, prec: str) -> dict:
    return BARS["unet" if model == "unet" else "resnet"]["f32" if prec in F32_GRADE else "f16"]


def _finite_or_inf(d: torch.Tensor) -> torch.Tensor:
    return torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))     # a NaN on either side is a failure, not a pass


def row_figures(model: str, prec: str, got: torch.Tensor, ref: torch.Tensor) -> dict:
    """Every row of ``got`` (n, ...) against its oracle row ``ref`` (same shape, same device).  Returns {"ok", "ratio" (worst figure over
    its bar; for the floors, the shortfall over the allowed shortfall), "metric", "row" (worst row of the per-row metric that is closest to
    its bar), "err", "bar", "figures": {metric: (value, bar)}}.  ``ok`` is the conjunction of every bar, as the whole-model tests assert
    them: f32-grade logits <= 1e-3 per row; f16-grade logits <= 5e-3 max(1, max|ref row|) per row and probabilities per row; mask IoU
    (UNet) and arg-max agreement (ResNet) over the batch."""
    bars = bars_for(model, prec)
    n = got.shape[0]
    g, r = got.reshape(n, -1).to(torch.float64), ref.reshape(n, -1).to(torch.float64)
    figures, per_row = {}, {}
    d = _finite_or_inf((g - r).abs()).amax(1)
    if "logit_abs" in bars:
        per_row["logit"] = (d, torch.full_like(d, bars["logit_abs"]))
    else:
        per_row["logit"] = (d, bars["logit_rel"] * r.abs().amax(1).clamp_min(1.0))
    if "prob" in bars:
        if model == "unet":
            pg, pr = torch.sigmoid(g), torch.sigmoid(r)
        else:
            pg, pr = torch.softmax(g, 1), torch.softmax(r, 1)
        dp = _finite_or_inf((pg - pr).abs()).amax(1)
        per_row["prob"] = (dp, torch.full_like(dp, bars["prob"]))
    worst = {"ratio": -1.0}
    ok = True
    for metric, (err, bar) in per_row.items():
        ratio = err / bar
        row = int(ratio.argmax())
        figures[metric] = (float(err[row]), float(bar[row]))
        ok = ok and bool((err <= bar).all())
        if float(ratio[row]) > worst["ratio"]:
            worst = {"ratio": float(ratio[row]), "metric": metric, "row": row, "err": float(err[row]), "bar": float(bar[row])}
    if model == "unet":                                                      # mask = sigmoid(logit) > 0.5 = logit > 0, over the batch
        mg, mr = g > 0, r > 0
        union = float((mg | mr).sum())
        value = float((mg & mr).sum()) / union if union else 1.0             # two empty masks are identical
        floor, key = bars["iou"], "iou"
    else:
        value = int((g.argmax(1) == r.argmax(1)).sum()) / n                # a count over n: all rows equal is exactly 1.0
        floor, key = bars["agree"], "agree"
    figures[key] = (value, floor)
    ok = ok and value >= floor
    short = (1.0 - value) / (1.0 - floor) if floor < 1.0 else (0.0 if value >= floor else float("inf"))
    if short > worst["ratio"]:
        if model == "unet":
            rows_bad = (mg != mr).reshape(n, -1).sum(1)
        else:
            rows_bad = (g.argmax(1) != r.argmax(1)).to(torch.int64)
        worst = {"ratio": short, "metric": key, "row": int(rows_bad.argmax()), "err": 1.0 - value, "bar": 1.0 - floor}
    return {"ok": bool(ok), **worst, "figures": figures}


def u8_figures(probs: torch.Tensor, float_logits: torch.Tensor) -> dict:
    """The u8 classifier entry: its soft-max within 1e-6 of the soft-max of the float path's logits, every row."""
    d = _finite_or_inf((probs.to(torch.float64) - torch.softmax(float_logits.to(torch.float64), 1)).abs()).amax(1)
    row = int(d.argmax())
    return {"ok": bool((d <= U8_SOFTMAX_BAR).all()), "ratio": float(d[row]) / U8_SOFTMAX_BAR, "metric": "u8_softmax", "row": row,
            "err": float(d[row]), "bar": U8_SOFTMAX_BAR, "figures": {"u8_softmax": (float(d[row]), U8_SOFTMAX_BAR)}}


# ---- the f16 / f16r pools: an input over the bar in the verified forms is replaced by the next seed ---------------------------------------
def screen_pool(over_bar, cap: int, max_rounds: int = 4) -> dict:
    """``over_bar(replaced) -> iterable of pool slots over the bar`` with the pool built from ``replaced`` = {slot: times replaced}.
    Replaces until no slot is over the bar; AssertionError when more than ``cap`` distinct slots had to be replaced, or when a slot is
    still over the bar after ``max_rounds`` seeds.  Returns ``replaced`` ({} when the pool stands as it is)."""
    replaced: dict = {}
    for _ in range(max_rounds):
        bad = sorted(set(int(j) for j in over_bar(dict(replaced))))
        if not bad:
            return replaced
        for j in bad:
            replaced[j] = replaced.get(j, 0) + 1
        assert len(replaced) <= cap, (f"{len(replaced)} pool inputs are over the bar in the launch forms the layer-local suite verifies "
                                      f"(slots {sorted(replaced)}); at most {cap} may be replaced")
    raise AssertionError(f"pool slots {bad} are still over the bar after {max_rounds} seeds")


# ---- the census: which kernel ran each layer at each n ---------------------------------------------------------------------------------
def signature(entries) -> tuple:
    return tuple((e["name"], e["kernel"]) for e in entries)


def census(engine, model: str, batches, x: torch.Tensor) -> dict:
    """{n: ((entry name, kernel string), ...)} from ``HipEngine.profile(model, x[:n])``, in launch order."""
    return {int(n): signature(engine.profile(model, x[:n])[3]) for n in batches}


def profile_into(engine, model: str, x: torch.Tensor, n: int, out: torch.Tensor) -> tuple:
    """One profiled forward of rows [0, n) of ``x`` INTO ``out`` (what ``HipEngine.profile`` does with a result tensor of its own): the
    eager, unpaired form of the layers.  Returns the signature."""
    import ctypes

    lib, h = engine._lib, engine._h
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    conv_ms, all_ms, launches = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    status = lib.cv_profile_convs(h, model.encode(), x.data_ptr(), n, out.data_ptr(), 1, stream, ctypes.byref(conv_ms),
                                  ctypes.byref(launches), ctypes.byref(all_ms))
    assert status == 0, (model, n, lib.cv_last_error())
    entries, idx = [], 0
    name, kern = ctypes.create_string_buffer(128), ctypes.create_string_buffer(160)
    ms, macs, is_conv = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
    while lib.cv_profile_entry(h, idx, name, 128, ctypes.byref(ms), ctypes.byref(macs), ctypes.byref(is_conv)) == 0:
        assert lib.cv_profile_entry_kernel(h, idx, kern, 160) == 0
        entries.append({"name": name.value.decode(), "kernel": kern.value.decode()})
        idx += 1
    return signature(entries)


def classes(cen: dict) -> list:
    """Group the n with identical signatures: [{"smallest", "largest", "members" (ascending), "signature"}], by smallest member."""
    groups: OrderedDict = OrderedDict()
    for n in sorted(cen):
        groups.setdefault(cen[n], []).append(n)
    return [{"smallest": m[0], "largest": m[-1], "members": m, "signature": sig} for sig, m in groups.items()]


def class_of(cls: list, n: int) -> dict:
    return next(c for c in cls if n in c["members"])


def ranges(members, swept=None) -> str:
    """[1, 2, 3, 7, 9, 10] -> "1-3, 7, 9-10".  With ``swept`` (every size that was run) a run of consecutive SWEPT sizes that skips
    integers is written "a..b": [64, 128, 192, 1000] of a sweep over 64, 128, 192, 256, 1000 -> "64..192, 1000"."""
    members = sorted(members)
    order = {n: k for k, n in enumerate(sorted(swept if swept is not None else members))}
    runs = []
    for n in members:
        if runs and (n == runs[-1][-1] + 1 or (swept is not None and order[n] == order[runs[-1][-1]] + 1)):
            runs[-1].append(n)
        else:
            runs.append([n])
    def text(r):
        if len(r) == 1:
            return str(r[0])
        return f"{r[0]}-{r[-1]}" if r[-1] - r[0] == len(r) - 1 else (f"{r[0]}..{r[-1]}" if len(r) > 2 else f"{r[0]}, {r[1]}")
    return ", ".join(text(r) for r in runs)


def signature_diff(a: tuple, b: tuple) -> list:
    """[(layer, kernel in a, kernel in b)] where the two differ; a layer launched in only one of them shows "-" on the other side.  The
    k-th launch of a name is matched with the k-th (a batch past the chunk size runs every layer once per chunk)."""
    def keyed(sig):
        seen, out = {}, OrderedDict()
        for name, kern in sig:
            k = seen.get(name, 0)
            seen[name] = k + 1
            out[(name, k)] = kern
        return out
    ka, kb = keyed(a), keyed(b)
    rows = []
    for key in list(ka) + [k for k in kb if k not in ka]:
        va, vb = ka.get(key, "-"), kb.get(key, "-")
        if va != vb:
            rows.append((key[0] if key[1] == 0 else f"{key[0]} #{key[1] + 1}", va or "(no kernel string)", vb or "(no kernel string)"))
    return rows


def describe_class(cls: list, n: int, passing) -> str:
    """For a failure message: the class of ``n`` and the (layer, kernel) pairs in which it differs from the class of the nearest n in
    ``passing``."""
    c = class_of(cls, n)
    swept = [m for k in cls for m in k["members"]]
    text = f"census class of n = {n}: n in {{{ranges(c['members'], swept)}}}"
    others = [m for m in passing if m not in c["members"]]
    if not others:
        return text + "; no n outside this class passed"
    near = min(others, key=lambda m: (abs(m - n), m))
    diff = signature_diff(c["signature"], class_of(cls, near)["signature"])
    return text + f"; against the nearest passing n = {near} of another class it differs in:\n    " + "\n    ".join(
        f"{layer}: {ka}   (n = {near}: {kb})" for layer, ka, kb in diff)


def tripwire(cls: list, listed, small: int) -> list:
    """The smallest members of the classes that begin at or under ``small`` and are NOT in ``listed``."""
    return [c["smallest"] for c in cls if c["smallest"] <= small and c["smallest"] not in set(listed)]


def thin(cls: list, batches) -> list:
    """The sizes to keep when a sweep has to be thinned: the smallest and largest member of every class and their two neighbours among
    ``batches``; interior members of a class go."""
    order = sorted(batches)
    keep = set()
    for c in cls:
        for edge in (c["smallest"], c["largest"]):
            at = order.index(edge)
            keep.update(order[max(0, at - 1):at + 2])
    return sorted(keep, reverse=True)


# ---- the report -------------------------------------------------------------------------------------------------------------------------
FORM_MARKS = (("splitK", "split-K"), ("8x16", "the 8 x 16 halo patch"), ("IMG8", "the packed 8 x 8 image mode"), (",POS", "position-major rows"),
              ("convt2x2_lds_kernel", "the LDS-resident transposed conv"), ("shortcut1x1s2_kernel", "the LDS-resident shortcut kernel"),
              ("CHAIN", "the chained layer1"), ("x256,", "256-pixel tiles of the generic kernel"), ("<float,256x", "256-row tiles"),
              ("<half_t,256x", "256-row tiles"), ("<split_t,256x", "256-row tiles"))


def render(records: list) -> str:
    """Markdown of profiles/batch_sweep.md from the records the GPU tests write (one dict per sweep parameter: {"model", "prec",
    "variant", "census": {n: signature}, "results": [{"n", "stage", "ok", "ratio", "metric", "row", "pool", "last_row", ...}],
    "replaced": {slot: times}, "seconds": {stage: s}, "thinned": bool})."""
    out = ["# Batch sweep: both networks at every batch size the launch planner tells apart", "",
           "What `tests/test_gpu_batch_sweep.py` measured on an MI355X (gfx950) with engines at the default chunk sizes (64 images / 16384",
           "squares).  A census class is a set of batch sizes at which every layer ran the same kernel (`HipEngine.profile`); `a-b` is every",
           "size from a to b, `a..b` every SWEPT size from a to b.  `err / bar` is the worst figure of a class over its bar in any stage (three forwards on fixed buffers, the u8",
           "entry, the profiled eager forward), every row compared; the bars are those of `tests/test_gpu_models.py`.", ""]
    for rec in records:
        cen = {int(n): tuple(tuple(p) for p in sig) for n, sig in rec["census"].items()}
        cls = classes(cen)
        title = f"{rec['model']} {rec['prec']}" + (f" {rec['variant']}" if rec.get("variant") else "")
        out += [f"## {title}", ""]
        secs = ", ".join(f"{k} {v:.1f} s" for k, v in rec.get("seconds", {}).items())
        out += [f"{len(cen)} batch sizes, {len(cls)} classes; wall time: {secs or 'not recorded'}."
                + ("  Thinned: interior members of a class were dropped." if rec.get("thinned") else ""), ""]
        rep = rec.get("replaced") or {}
        out += ["Replaced pool inputs: " + (", ".join(f"slot {j} ({r}x)" for j, r in sorted((int(j), r) for j, r in rep.items())) if rep else "none")
                + ".", ""]
        out += ["| class | n | worst err / bar | metric | at n | stage | worst row is the last row | passed |", "|---|---|---|---|---|---|---|---|"]
        for k, c in enumerate(cls):
            rs = [r for r in rec["results"] if r["n"] in c["members"]]
            if rs:
                w = max(rs, key=lambda r: r["ratio"])
                out.append(f"| {k} | {ranges(c['members'], cen)} | {w['ratio']:.3f} | {w['metric']} | {w['n']} | {w['stage']} | "
                           f"{'yes' if w['last_row'] else 'no'} | {'yes' if all(r['ok'] for r in rs) else 'NO'} |")
            else:
                out.append(f"| {k} | {ranges(c['members'], cen)} | - | - | - | - | - | not run |")
        out += ["", "Sizes at which some layer runs a form (by its mark in the kernel string):", ""]
        for mark, what in FORM_MARKS:
            ns = [n for n in sorted(cen) if any(mark in kern for _, kern in cen[n])]
            if ns:
                out.append(f"* {what} (`{mark}`): n in {{{ranges(ns, cen)}}}")
        out += ["", "Layers whose kernel changes from one class to the next:", ""]
        for k in range(1, len(cls)):
            out.append(f"* class {k - 1} (from n = {cls[k - 1]['smallest']}) -> class {k} (from n = {cls[k]['smallest']}):")
            for layer, ka, kb in signature_diff(cls[k - 1]["signature"], cls[k]["signature"]):
                out.append(f"    * `{layer}`: `{ka}` -> `{kb}`")
        if len(cls) == 1:
            out.append("* one class only")
        out.append("")
    return "\n".join(out) + "\n"


def load_records(path) -> list:
    """The LAST record of every (model, prec, variant) in a jsonl file the GPU tests appended to."""
    last: OrderedDict = OrderedDict()
    with open(path) as f:
        for line in f:
            if line.strip():
                rec = json.loads(line)
                last[(rec["model"], rec["prec"], rec.get("variant", ""))] = rec
    return list(last.values())


if __name__ == "__main__":                               # python tests/batch_sweep.py <batch_sweep.jsonl of the GPU tests> > profiles/batch_sweep.md
    sys.stdout.write(render(load_records(sys.argv[1])))
