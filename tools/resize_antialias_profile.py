"""Measurements of profiles/resize_antialias.md: 256 boards of 512 x 512 through ``process_images`` in every resize mode the package has
(2 warm-up calls, then 5 timed calls per mode, modes alternating), and the resize kernels alone, event-timed on resident images.

usage: python tools/resize_antialias_profile.py [PKG_ROOT [TAG]]
PKG_ROOT: a ``chessvision-3lc_amd`` directory with its built library (default: this tree's); pointing it at a checkout of another commit
and alternating the two in one session is how the default path is compared across commits.  One JSON line per figure."""
import json, sys, tempfile, time
from pathlib import Path
pkg = sys.argv[1] if len(sys.argv) > 1 else str(Path(__file__).resolve().parent.parent / "chessvision-3lc_amd")
tag = sys.argv[2] if len(sys.argv) > 2 else "this tree"
sys.path.insert(0, pkg)
import inspect
import numpy as np, torch
from chessvision import ChessVision, synthetic
assert torch.cuda.is_available()
import chessvision
assert chessvision.__file__.startswith(pkg), chessvision.__file__
d = tempfile.mkdtemp()
pe, pc = synthetic.save_checkpoints(d, segmenting=True)
cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3")
images = [synthetic.board_photo(200 + s) for s in range(256)]
modes = ["area", "antialias"] if "resize" in inspect.signature(ChessVision.process_images).parameters else ["area"]
def call(mode, timings):
    kw = {} if mode == "area" and len(modes) == 1 else {"resize": mode}
    t0 = time.perf_counter()
    res = cv.process_images(images, fallback_quad=True, return_crops=False, timings=timings, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res
for mode in modes:
    for _ in range(2):
        call(mode, {})
for rnd in range(5):                      # modes alternate inside the process
    for mode in modes:
        tm = {}
        s, res = call(mode, tm)
        print(json.dumps({"tag": tag, "mode": mode, "round": rnd, "boards_per_s": round(256 / s, 1), "resize_ms": round(tm["resize_ms"], 4),
                          "unet_ms": round(tm["unet_ms"], 3), "jobs": tm["jobs"]}), flush=True)
if len(modes) == 2:
    eng = cv._get_engine("unet")
    dev = torch.from_numpy(np.stack(images)).cuda()
    for name, fn, nbytes in (("resize_antialias_f32", lambda: eng.resize_antialias_f32(dev), 256 * (512 * 512 * 3 + 4 * 3 * 256 * 256)),
                             ("resize_area_u8", lambda: eng.resize_area_u8(dev), 256 * (512 * 512 * 3 + 3 * 256 * 256))):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(50):
                fn()
            b.record(); torch.cuda.synchronize()
            reps.append(a.elapsed_time(b) / 50)
        print(json.dumps({"tag": tag, "kernel": name, "ms_per_call": [round(r, 4) for r in reps], "compulsory_MB": round(nbytes / 1e6, 1),
                          "GBps_best": round(nbytes / min(reps) / 1e6, 1), "GBps_median": round(nbytes / sorted(reps)[2] / 1e6, 1)}), flush=True)
    # other geometries, 8 images each: too few tiles to fill the chip
    for h, w in ((1536, 2048), (1024, 768), (300, 400)):
        x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (8, h, w, 3), dtype=np.uint8)).cuda()
        for _ in range(5):
            eng.resize_antialias_f32(x)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            eng.resize_antialias_f32(x)
        b.record(); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / 50
        nbytes = 8 * (h * w * 3 + 4 * 3 * 65536)
        print(json.dumps({"tag": tag, "kernel": f"resize_antialias_f32 8x{h}x{w}", "ms_per_call": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1)}), flush=True)
cv._get_engine("unet").check_numerics()
