"""Measurements of profiles/threshold_sweep.md: 256 boards of 512 x 512, default precision.  For T in {1, 3, 9}: T consecutive
``evaluate_images`` calls (the way of the commit before ``evaluate_thresholds``) against ONE ``evaluate_thresholds`` call, 2 warm-up
rounds, then 5 timed rounds with the two alternating inside the process; every timed window ends in a device synchronise.  Then the
levels kernel alone on 64 resident images, event-timed, with its algorithmic bytes.  One JSON line per figure.

usage: python tools/threshold_sweep_profile.py [N_IMAGES]"""
import json, statistics, sys, tempfile, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "chessvision-3lc_amd"))
import numpy as np, torch
from chessvision import ChessVision, synthetic
assert torch.cuda.is_available(), "the profile needs an MI355X"
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
GRIDS = {1: [0.5], 3: [0.3, 0.5, 0.7], 9: [round(0.1 * k, 1) for k in range(1, 10)]}
HBM_TBPS = 6.29                                  # measured float4 copy rate of the part (8.0 spec)
d = tempfile.mkdtemp()
pe, pc = synthetic.save_checkpoints(d, segmenting=True)
cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
images = [synthetic.board_photo(200 + s) for s in range(N)]
fens = ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"] * N
yy, xx = np.mgrid[:256, :256]
masks = [np.where((yy > 40) & (yy < 215) & (xx > 45) & (xx < 210), 255, 0).astype(np.uint8) for _ in range(N)]


def baseline(grid):
    tm = {}
    t0 = time.perf_counter()
    reports = [cv.evaluate_images(images, true_fens=fens, label_masks=masks, threshold=t, timings=tm) for t in grid]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, tm, sum(r.position is not None for rep in reports for r in rep.results)


def sweep(grid):
    tm = {}
    t0 = time.perf_counter()
    rep = cv.evaluate_thresholds(images, grid, true_fens=fens, label_masks=masks, timings=tm)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, tm, rep


def spread(values):
    return {"median_s": round(statistics.median(values), 4), "min_s": round(min(values), 4), "max_s": round(max(values), 4)}


HOST = ("stage_s", "wait_masks_s", "contours_s", "homography_s", "wait_probs_s", "decode_s", "assemble_s", "evaluation", "drain_s")
GPU = ("resize_ms", "unet_ms", "levels_ms", "seg_ms", "warp_ms", "resnet_ms")
for T, grid in GRIDS.items():
    for _ in range(2):
        baseline(grid), sweep(grid)
    base_s, sweep_s, last = [], [], None
    for rnd in range(5):                          # the two alternate inside the process
        bs, btm, found = baseline(grid)
        ss, stm, rep = sweep(grid)
        base_s.append(bs), sweep_s.append(ss)
        last = (btm, stm, rep, found)
    btm, stm, rep, found = last
    assert rep.boards_found == found
    print(json.dumps({"T": T, "images": N, "baseline": spread(base_s), "sweep": spread(sweep_s),
                      "sweep_over_baseline": round(statistics.median(sweep_s) / statistics.median(base_s), 4),
                      "sweep_over_one_call": round(statistics.median(sweep_s) / (statistics.median(base_s) / T), 4),
                      "boards_found": rep.boards_found, "boards_classified": rep.boards_classified,
                      "classified_ratio": round(rep.boards_classified / max(1, rep.boards_found), 4)}), flush=True)
    print(json.dumps({"T": T, "last_round": "baseline (T calls, summed)", "host_s": {k: round(btm.get(k, 0.0), 4) for k in HOST},
                      "gpu_ms": {k: round(btm.get(k, 0.0), 3) for k in GPU}}), flush=True)
    print(json.dumps({"T": T, "last_round": "sweep", "host_s": {k: round(stm.get(k, 0.0), 4) for k in HOST},
                      "gpu_ms": {k: round(stm.get(k, 0.0), 3) for k in GPU}}), flush=True)

# the levels kernel alone: 64 resident images, with labels; 4 B logit + 1 B label read, 1 B level written per pixel
eng = cv._get_engine("unet")
rng = np.random.default_rng(0)
logits = torch.from_numpy(rng.normal(0, 4, (64, 1, 256, 256)).astype(np.float32)).cuda()
labels = torch.from_numpy(np.stack(masks[:1] * 64)).cuda()
nbytes = 64 * 65536 * 6
for T, grid in GRIDS.items():
    for _ in range(5):
        eng.threshold_levels_dev(logits, grid, labels)
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            eng.threshold_levels_dev(logits, grid, labels)
        b.record(); torch.cuda.synchronize()
        reps.append(a.elapsed_time(b) / 50)
    med = statistics.median(reps)
    print(json.dumps({"kernel": "threshold_levels_kernel", "T": T, "images": 64, "ms_per_call": [round(r, 4) for r in reps],
                      "algorithmic_MB": round(nbytes / 1e6, 2), "GBps_median": round(nbytes / med / 1e6, 1),
                      "hbm_fraction_of_6.29TBps": round(nbytes / med / 1e6 / (HBM_TBPS * 1e3), 4),
                      "note": "includes the launch and two output allocations per call; one workgroup per image = 64 of 256 CUs"}), flush=True)
eng.check_numerics()
