#!/usr/bin/env python3
"""bench.py -- boards/sec of the ChessVision CNN hot path on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path over one batch of synthetic boards, resident in HBM:
    UNet(3->1) forward on B 256x256 images  +  ResNet-18 forward on 64*B 64x64 squares
(BASELINE.json configs[3]/[4]: the end-to-end batch of 256 boards per GPU; the classical-CV stages between the two models
are SURVEY.md section 8(f) rows, reported in the `pipeline_e2e` block, never inside `value`).

    python bench.py --gpus N --steps K --warmup W [--dtype f16x3|f32|f16] [--unet-variant convT|bilinear] [--boards B]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last step's outputs when --dump-outputs is given, and prints the
headline line.  Everything else -- the rooflines (event-timed passes of their own), the CPU baseline and the oracle parity, the
other precisions and the bilinear variant, the host-images-to-FEN pipeline legs and the multi-rank checks -- runs with --full
(--no-cpu-baseline / --no-extras then trim it as before).

N > 1 from a bare shell: the process re-launches itself under torch.distributed.run (one rank per GPU, RCCL) BEFORE anything
touches the GPU, relays rank 0's JSON line and exits with the children's return code.  Under a launcher (WORLD_SIZE set) it
runs as one rank.  Weights are generated on rank 0 and replicated with ONE RCCL broadcast; boards are sharded (each rank owns
B boards, no data-path collective) => "scaling": "weak".  Rank 0 prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "chessvision-3lc_amd"))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (importing torch does not initialise the GPU)

# MI355X dense MFMA peaks (MI355X_MICROARCH.md, chip table): f32-input MFMA 157.3 TF, f16 MFMA ~2500 TF; HBM3E 8 TB/s.
# f16x3 computes every algorithmic MAC with THREE f16 MFMA products (hi*hi + hi*lo + lo*hi), so the dense peak of
# that arithmetic type is 2500 / 3 algorithmic TFLOP/s; the line also carries the fraction of the raw f16 peak.
PEAK_TFLOPS = {"f32": 157.3, "f16": 2500.0, "f16x3": 2500.0 / 3.0, "f16r": 2500.0}
MFMA_PER_MAC = {"f32": 1, "f16": 1, "f16x3": 3, "f16r": 1}
HBM_PEAK_GBS = 8000.0
PMC_FILE = "profiles/r06_pmc_traffic.json"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def visible_gpus() -> int:
    """GPUs this process tree may use, WITHOUT bringing the HIP runtime up in the parent (it only launches children): the visibility
    variables when set, else the KFD topology (nodes with SIMDs are GPUs); torch's count only when neither can be read."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip() != ""])
    try:
        n = 0
        for node in Path("/sys/class/kfd/kfd/topology/nodes").iterdir():
            props = dict(line.split()[:2] for line in (node / "properties").read_text().splitlines() if len(line.split()) >= 2)
            n += int(props.get("simd_count", "0")) > 0
        if n:
            return n
    except (OSError, ValueError):
        pass
    return torch.cuda.device_count()


def relaunch_under_torchrun(args, argv) -> int:
    """--gpus N > 1 without a launcher: start N ranks as a CHILD process tree (never exec: a process that has touched the GPU
    must not be replaced, and this parent has not touched it yet) and hand back its return code."""
    n_dev = visible_gpus()
    share = os.environ.get("CV_DIST_BACKEND") == "gloo"      # gloo ranks may share a GPU (the N > 1 path on a one-GPU box)
    if n_dev < args.gpus and not (share and n_dev >= 1):
        log(f"bench.py: --gpus {args.gpus} but only {n_dev} device(s) visible")
        return 2
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + argv
    log("bench.py: launching", " ".join(cmd))
    return subprocess.run(cmd, env=env).returncode          # children inherit stdout: rank 0's JSON line is relayed as is


def kernel_source_hash():
    """sha256 over chessvision-3lc_amd/csrc (*.hip, *.h, *.cpp, Makefile; names included, sorted) -- the same digest
    tools/pmc_traffic.py stores next to the counters it reduces."""
    import hashlib

    root = ROOT / "chessvision-3lc_amd" / "csrc"
    h = hashlib.sha256()
    for f in sorted(p for p in root.iterdir() if p.suffix in (".hip", ".h", ".cpp") or p.name == "Makefile"):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()


def pmc_traffic(dtype, unet_chunk, resnet_chunk, unet_launches, resnet_launches):
    """Per-launch HBM bytes of the conv family from the committed rocprofv3 PMC passes (separate --pmc FETCH_SIZE / WRITE_SIZE
    runs of the same chunk sizes, gfx950-corrected, tools/pmc_collect.sh).  Not measured by this run: the field carries its
    source, and it is only reported while the kernels are the ones the counters were collected on -- the profile stores the
    sha256 of csrc/ at collection time and a different digest today gives (None, reason).  Returns (bytes per launch | None,
    reason | None)."""
    path = ROOT / PMC_FILE
    if not path.exists():
        return None, f"{PMC_FILE} is not committed"
    if (unet_chunk, resnet_chunk) != (64, 16384):
        return None, "the committed counters are for chunks of 64 boards / 16384 squares"
    t = json.load(open(path))
    u, r = t.get(f"{dtype}_unet"), t.get(f"{dtype}_resnet18")
    if not u or not r:
        return None, f"no {dtype} counters in {PMC_FILE}"
    now = kernel_source_hash()
    for blk in (u, r):
        if blk.get("kernel_source_sha256") != now:
            return None, (f"stale: {PMC_FILE} was collected on kernel sources {str(blk.get('kernel_source_sha256'))[:12]}, this tree is "
                          f"{now[:12]} -- re-run tools/pmc_collect.sh")
    total = u["hbm_bytes_per_launch"] * unet_launches + r["hbm_bytes_per_launch"] * resnet_launches
    return total / max(1, unet_launches + resnet_launches), None


# ---- CPU baseline leg: the ONLY place bench.py touches oracle/ (as the checker and the timed CPU port) -------------------
def cpu_baseline(x_cpu, sq_cpu, gpu_logits, gpu_cls, e2e_images=None, budget_s: float = 12.0, e2e_results=None, fp16_search_s: float = 0.0,
                 device=None):
    """Time the oracle (torch-CPU restatement = the arithmetic the reference runs) on a bounded sample:
      (i)  the reference-style loop -- UNet batch 1 + classifier batch 64 per board (core.py:215-220,236-241) -- at the thread
           count that is fastest on this box (swept: the default of one thread per logical core oversubscribes this loop);
      (ii) batched (UNet b=8, ResNet-18 b=512), what a batched CPU implementation would reach.
    The same outputs check the GPU results; with `e2e_images` the oracle pipeline also produces reference FENs."""
    from oracle import pipeline_ref, synth

    unet, resnet = synth.make_unet(1), synth.make_resnet(2)
    unet = unet.to(memory_format=torch.channels_last)            # core.py:89
    ncpu = os.cpu_count() or 1
    default_threads = torch.get_num_threads()
    sweep = {}
    with torch.no_grad():
        unet(x_cpu[:1]); resnet(sq_cpu[:64])                      # warm-up
        for t in sorted({t for t in (8, 16, 32, 64, 128, default_threads) if t <= max(ncpu, 1)}):
            torch.set_num_threads(t)
            unet(x_cpu[:1]); resnet(sq_cpu[:64])
            t0 = time.perf_counter()
            for b in range(2):
                unet(x_cpu[b:b + 1]); resnet(sq_cpu[b * 64:(b + 1) * 64])
            sweep[t] = 2 / (time.perf_counter() - t0)
        best = max(sweep, key=sweep.get)
        torch.set_num_threads(best)
        errs_u, errs_r, ref_u, ref_r = [], [], [], []
        t0 = time.perf_counter()
        done = 0
        while done < min(64, x_cpu.shape[0]):
            lo = unet(x_cpu[done:done + 1])
            cl = resnet(sq_cpu[done * 64:(done + 1) * 64])
            errs_u.append(float((lo - gpu_logits[done:done + 1]).abs().max()))
            errs_r.append(float((cl - gpu_cls[done * 64:(done + 1) * 64]).abs().max()))
            ref_u.append(lo); ref_r.append(cl)
            done += 1
            if time.perf_counter() - t0 >= budget_s:
                break
        dt = time.perf_counter() - t0
        nb = min(8, x_cpu.shape[0])
        unet(x_cpu[:nb]); resnet(sq_cpu[:nb * 64])
        t1 = time.perf_counter()
        unet(x_cpu[:nb]); resnet(sq_cpu[:nb * 64])
        batched = nb / (time.perf_counter() - t1)
        fens = None
        if e2e_images is not None:
            from chessvision import synthetic
            from oracle.unet_ref import UNet
            seg = UNet(3, 1, False)
            seg.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.unet_state_dict(1, segmenting=True).items()}, strict=False)
            ref = pipeline_ref.process_images(seg.eval(), resnet, e2e_images, fallback_quad=True)
            fens = []
            for k, r in enumerate(ref):
                # byte work is bit-exact (round 4: OpenCV's order of operations on host, device and in the oracle): a device board
                # that differs from the oracle's is REPORTED as a mismatch, never re-classified
                dev = e2e_results[k].board_extraction.board_image if e2e_results is not None else None
                same = dev is not None and dev.shape == r.board_extraction.board_image.shape and bool((dev == r.board_extraction.board_image).all())
                fens.append((r.position.fen, r.position.original_fen, r.position.model_probabilities, not same))
        # the fp16 classifier's parity margin on MORE than one network (VERDICT r05 'weak' 1): 4096 squares (BASELINE configs[2]) on weight
        # seeds x {He-normal, stressed}, worst soft-max error against this oracle; bounded by `fp16_search_s` seconds, seed 5 (the worst
        # of tests/dev/f16r_seed_search.py) first.  tests/test_gpu_models.py asserts the whole 8 x 2 grid.
        search = None
        if fp16_search_s > 0:
            from chessvision.hip_backend import HipEngine
            rows, t_s = [], time.perf_counter()
            for seed in (5, 4, 2, 0, 1, 3, 6, 7):
                sq_s = synth.squares_input(seed=1000 + seed, n=4096)
                for wname in ("he_normal", "stress"):
                    if rows and time.perf_counter() - t_s > fp16_search_s:
                        break
                    net = synth.make_resnet(seed=seed)
                    if wname == "stress":
                        synth.load(net, synth.stress_resnet_state_dict(seed))
                    p_ref = torch.softmax(net(sq_s), 1)
                    e16 = HipEngine(device, precision="f16r", resnet_chunk=4096)
                    e16.load_resnet18(net.state_dict())
                    p = torch.softmax(e16.resnet18_forward(sq_s).cpu(), 1)
                    e16.close()
                    rows.append({"seed": seed, "weights": wname, "prob_err": float((p - p_ref).abs().max())})
            worst = max(rows, key=lambda r: r["prob_err"])
            search = {"networks": len(rows), "squares": 4096, "worst_prob_err": worst["prob_err"], "worst_case": f"seed {worst['seed']} {worst['weights']}",
                      "rows": rows, "seconds": round(time.perf_counter() - t_s, 1),
                      "bar": "soft-max within 1e-3 of the fp32 oracle on EVERY network (tests/test_gpu_models.py walks 8 seeds x 2 weight kinds)"}
        torch.set_num_threads(default_threads)
    base = {"value": round(done / dt, 3), "unit": "boards/sec", "cores": best, "kind": "port",
            "sample": f"{done} boards, reference-style loop (UNet b=1 + ResNet-18 b=64 per board), torch {torch.__version__} CPU fp32 "
                      f"channels_last, {best} threads (fastest of the sweep), {ncpu} logical CPUs",
            "thread_sweep_boards_per_sec": {str(k): round(v, 3) for k, v in sweep.items()},
            "batched": {"value": round(batched, 3), "unit": "boards/sec", "cores": best,
                        "sample": f"one pass of UNet b={nb} + ResNet-18 b={nb * 64} after one warm-up pass"}}
    return (base, {"unet_logit_max_abs_err": max(errs_u), "resnet_logit_max_abs_err": max(errs_r), "boards_checked": done}, fens,
            (torch.cat(ref_u), torch.cat(ref_r)), search)


def pipeline_e2e(dtype: str, n_boards: int = 256, n_checked: int = 8):
    """BASELINE configs[3] end to end through the public API: 512x512 BGR photos on the HOST -> ChessVision.process_images
    (staging, H2D, resize, UNet, mask D2H, C++ contour, warp+split, ResNet-18, softmax, D2H, C++ FEN).  The UNet weights are
    random except for one rewired channel that makes it segment the synthetic photos (synthetic.make_segmenting), so the
    contour stage sees realistic masks; boards without a quadrangle go through fallback_quad.  Reported beside the headline,
    never as `value`.  Returns (block, images of the checked subset, results of the checked subset)."""
    import tempfile

    from chessvision import ChessVision, synthetic

    with tempfile.TemporaryDirectory() as d:
        pe, pc = synthetic.save_checkpoints(d, segmenting=True)
        cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision=dtype)
        images = [synthetic.board_photo(s) for s in range(n_boards)]
        cv.process_images(images[:96], fallback_quad=True, return_crops=False)   # warm-up (lazy model init, pinned buffers, workspace)
        try:
            latency = process_image_latency(cv)
        except Exception as exc:                                                   # extra figure only
            latency = {"error": repr(exc)}
        best, tm_best, res, calls = None, None, None, []
        for _ in range(5):                                   # five calls: the call contains host staging copies, and the host is shared
            tm = {}
            t0 = time.perf_counter()
            res = cv.process_images(images, fallback_quad=True, timings=tm, return_crops=False)
            dt = time.perf_counter() - t0
            calls.append(dt)
            if best is None or dt < best:
                best, tm_best = dt, tm
        # the same job with the classifier in its fp16 mode (BASELINE configs[4] says fp16): UNet on the headline engine, ResNet-18 on "f16r"
        mixed = None
        if "+" not in dtype and dtype != "f16r":
            try:
                cv2_ = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision=f"{dtype}+f16r")
                cv2_.process_images(images[:96], fallback_quad=True, return_crops=False)
                tbest, r2 = None, None
                for _ in range(3):
                    t0 = time.perf_counter()
                    r2 = cv2_.process_images(images, fallback_quad=True, return_crops=False)
                    dt = time.perf_counter() - t0
                    tbest = dt if tbest is None or dt < tbest else tbest
                np_ = __import__("numpy")
                perr = max(float(np_.abs(a.position.model_probabilities - b.position.model_probabilities).max()) for a, b in zip(res, r2))
                same = sum(a.position.fen == b.position.fen and a.position.original_fen == b.position.original_fen for a, b in zip(res, r2))
                mixed = {"precision": f"{dtype}+f16r", "boards_per_sec": round(n_boards / tbest, 1),
                         "prob_max_abs_diff_vs_headline_precision": perr, "fen_identical_to_headline_precision": f"{same}/{n_boards}"}
            except Exception as exc:
                mixed = {"error": repr(exc)}
    classified = sum(r.position is not None for r in res)
    whole = cv._scale_quadrangle(__import__("numpy").array([[[255, 0]], [[0, 0]], [[0, 255]], [[255, 255]]], "int32"), (512, 512))
    found = sum(r.board_extraction.quadrangle is not None and not (r.board_extraction.quadrangle == whole).all() for r in res)
    calls.sort()
    block = {"boards_per_sec": round(n_boards / best, 1), "boards_per_sec_median": round(n_boards / calls[len(calls) // 2], 1),
             "boards_per_sec_min": round(n_boards / calls[-1], 1), "calls": len(calls),
             "boards": n_boards, "classified": classified, "quadrangles_found": found,
             "stages": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in tm_best.items()},
             "note": "host images in, FEN out (boards_per_sec = best of 5 calls, median and slowest beside it; the headline value is a 20-step MEAN of the resident CNN passes); one host thread software-pipelined against the GPU in jobs of 64 boards, "
                     "copies on side streams; stages: host seconds (*_s) and event-timed GPU milliseconds (*_ms) summed over the jobs"}
    if mixed is not None:
        block["classifier_fp16"] = mixed
    block["latency"] = latency
    return block, images[:n_checked], res[:n_checked]


class _DeviceMemory:
    """Device-wide memory in use (total - free of hipMemGetInfo: every process on the GPU counts, the engines' hipMalloc'd workspaces
    included), sampled at the points where the footprint peaks; ``peak_gb`` is the largest sample this rank saw."""

    def __init__(self, device):
        self.device, self.peak, self.total = device, 0, 0

    def sample(self):
        free, total = torch.cuda.mem_get_info(self.device)
        self.total = total
        self.peak = max(self.peak, total - free)
        return total - free

    @property
    def peak_gb(self):
        return self.peak / 1e9


class _LazyPhotos:
    """The global list of synthetic board photos; a photo is only rendered when its index is touched (a rank touches its shard)."""

    def __init__(self, n):
        self.n = n
        self.cache = {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from chessvision import synthetic
        if i not in self.cache:
            self.cache[i] = synthetic.board_photo(i)
        return self.cache[i]


def pipeline_e2e_sharded(dtype, boards_per_rank, rank, world, device, cvd, mem=None):
    """BASELINE configs[4] literally: ONE list of world * B photos, ``distributed.process_images_sharded`` (rank r processes
    photos r::world through host staging, resize, UNet, contours, warp, ResNet-18, FEN; probabilities / quadrangles / masks are
    all-gathered and re-interleaved).  Every rank times its own shard; the block carries min / mean / max over the ranks and
    the whole-job rate (all boards / slowest rank, gather included).  Collective: every rank must call this."""
    import tempfile

    from chessvision import ChessVision, synthetic

    n_global = world * boards_per_rank
    photos = _LazyPhotos(n_global)
    with tempfile.TemporaryDirectory() as d:
        pe, pc = synthetic.save_checkpoints(d, segmenting=True)      # same seeds on every rank: identical weights
        cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision=dtype)
        _ = cv.board_extractor, cv.classifier                         # load + calibrate, then take rank 0's tensor exponents
        cal = {"identical_across_ranks": True}
        for model, engine in (("unet", cv._get_engine("unet")), ("resnet18", cv._get_engine("resnet18"))):
            rep = cvd.sync_calibration(engine, device, models=(model,))      # the two engines of a mixed precision, one model each
            cal["identical_across_ranks"] = cal["identical_across_ranks"] and rep["identical_across_ranks"]
        for i in cvd.shard_indices(n_global, rank, world):
            photos[i]                                                 # render this rank's shard before any clock starts
        warm = _LazyPhotos(min(96, boards_per_rank) * world)
        warm.cache = photos.cache
        cvd.process_images_sharded(cv, warm, fallback_quad=True, gather=False, return_crops=False)
        if mem is not None:
            mem.sample()                                              # every rank's engines are loaded and their workspaces grown
        best = None
        for _ in range(3):
            tm = {}
            cvd.barrier(device)
            t0 = time.perf_counter()
            res = cvd.process_images_sharded(cv, photos, fallback_quad=True, return_crops=False, timings=tm)
            total = time.perf_counter() - t0
            if best is None or total < best[0]:
                best = (total, tm["shard_s"], tm["gather_s"], res)
        total, shard_s, gather_s, res = best
        # The gathered list must be in the caller's order: rank 0 recomputes the first photo of every OTHER rank's shard itself
        # (and one from the middle of each) and compares FEN and probabilities with what the gather delivered for that index.
        order_checked = order_bad = 0
        if rank == 0 and world > 1:
            import numpy as np
            picks = sorted({r for r in range(1, world)} | {r + world * (boards_per_rank // 2) for r in range(1, world)})
            picks = [i for i in picks if i < n_global]
            own = cv.process_images([photos[i] for i in picks], fallback_quad=True, return_crops=False)
            for i, mine in zip(picks, own):
                got = res[i]
                same = (got is not None and got.position is not None and mine.position is not None and got.position.fen == mine.position.fen and
                        float(np.abs(got.position.model_probabilities - mine.position.model_probabilities).max()) <= 1e-6)
                order_checked += 1
                order_bad += not same
    rate = cvd.stats_over_ranks(boards_per_rank / shard_s, device)
    whole = n_global / cvd.max_over_ranks(total, device)
    gather = cvd.stats_over_ranks(gather_s, device)
    fens = sum(r is not None and r.position is not None for r in res)
    return {"boards_per_sec_per_rank": {k: round(v, 1) for k, v in rate.items()}, "boards_per_sec_whole_job": round(whole, 1),
            "gather_s": {k: round(v, 4) for k, v in gather.items()}, "gather_s_per_rank": [round(v, 4) for v in cvd.list_over_ranks(gather_s, device)],
            "shard_s_per_rank": [round(v, 4) for v in cvd.list_over_ranks(shard_s, device)],
            "global_boards": n_global, "fens_on_rank0": fens, "order_checked_on_rank0": order_checked, "order_mismatches": order_bad,
            "calibration_identical_across_ranks": cal["identical_across_ranks"],
            "note": "host photos in, FEN out on every rank (best of 3 calls); per-rank rate = shard boards / that rank's process_images time; "
                    "whole job = all boards / slowest rank's call including the all_gather of probabilities, quadrangles and masks"}


def classifier_fp16(eng_main, x, sq, B, rsd, args, device, cvd, oracle_out):
    """BASELINE configs[2]'s arithmetic for the classifier: precision "f16r" (one f16 MFMA product per MAC, f32 accumulate, f32
    residual trunk, f32 shortcut convolutions) -- throughput of the ResNet-18 pass alone, of the step with the UNet left on the
    headline engine, its own MFMA roofline (dense f16 peak, 1 product per MAC) and its parity against the same oracle outputs
    as `parity_vs_oracle` (4096 squares = configs[2]'s batch when 64 boards were checked)."""
    from chessvision.hip_backend import HipEngine

    XS, XW = args.extra_steps, args.extra_warmup
    e = HipEngine(device, precision="f16r", unet_chunk=args.unet_chunk, resnet_chunk=args.resnet_chunk)
    e.load_resnet18(rsd)

    def timed(fn):
        for _ in range(XW):
            fn()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(XS):
            o = fn()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / XS, o

    t_cls, cls = timed(lambda: e.resnet18_forward(sq, check=False))
    t_ref, _ = timed(lambda: eng_main.resnet18_forward(sq, check=False))
    t_step, _ = timed(lambda: (eng_main.unet_forward(x, check=False), e.resnet18_forward(sq, check=False)))
    e.check_numerics()
    e.resnet18_forward(sq, check=False)                   # the event-timed passes at the clocks of a busy chip (as rooflines() does)
    c_ms, c_n, a_ms, entries = e.profile("resnet18", sq, iters=3)
    flop = sum(2.0 * en["macs"] for en in entries if en["conv"])
    ach = flop / (c_ms * 1e-3) / 1e12
    block = {"precision": "f16r", "squares": int(sq.shape[0]), "ms_per_pass": round(t_cls * 1e3, 3), "squares_per_sec": round(sq.shape[0] / t_cls, 1),
             "headline_engine_ms_per_pass": round(t_ref * 1e3, 3), "steps": XS, "warmup": XW,
             "step_with_headline_unet": {"ms_per_step": round(t_step * 1e3, 3), "boards_per_sec": round(B / t_step, 2)},
             "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_TFLOPS["f16r"], "unit": "TFLOP/s",
                          "frac": round(ach / PEAK_TFLOPS["f16r"], 4), "launches": c_n // 3, "profiled_passes": 3, "avg_launch_ms": round(c_ms / max(c_n, 1), 4)}}
    if oracle_out is not None:
        ref = oracle_out[1]
        got = cls[:ref.shape[0]].cpu()
        p, p_ref = torch.softmax(got, 1), torch.softmax(ref, 1)
        block["parity_vs_oracle"] = {"squares_checked": int(ref.shape[0]), "prob_max_abs_err": float((p - p_ref).abs().max()),
                                     "logit_max_abs_err": float((got - ref).abs().max()),
                                     "argmax_agreement": float((p.argmax(1) == p_ref.argmax(1)).float().mean()),
                                     "bar": "soft-max probabilities within 1e-3 of the fp32 oracle (SURVEY.md section 8d config 3)"}
    e.close()
    return block


def byte_kernel_rooflines(eng, device, n_boards=256):
    """HBM roofline of the SURVEY section 8f byte kernels on the pipeline's job shape (n_boards 512x512 BGR photos resident in HBM):
    algorithmic bytes (input once + outputs once) / event-timed launch / 8 TB/s.  Events are recorded on torch's current stream,
    which is the stream the C ABI launches these kernels on."""
    import numpy as np

    from chessvision import synthetic
    from chessvision.hip_backend import board_homographies

    rng = np.random.default_rng(0)
    base = np.stack([synthetic.board_photo(s) for s in range(8)])
    imgs = torch.from_numpy(np.concatenate([base] * (n_boards // 8))).to(device)
    quads = np.stack([np.array([[430, 40], [60, 55], [45, 440], [470, 450]], np.float32) + rng.uniform(-25, 25, (4, 2)).astype(np.float32)
                      for _ in range(n_boards)])
    inv = torch.from_numpy(board_homographies(quads).reshape(n_boards, 9)).pin_memory()

    def timed(fn, iters=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize(device)
        return a.elapsed_time(b) / iters

    out = {}
    for name, fn, nbytes in (
            ("resize_area_u8", lambda: eng.resize_area_u8(imgs, (256, 256)), n_boards * (512 * 512 * 3 + 256 * 256 * 3)),
            ("extract_squares_u8", lambda: eng.extract_squares_u8(imgs, inv, want_boards=True), n_boards * (512 * 512 * 3 + 2 * 512 * 512))):
        ms = timed(fn)
        out[name] = {"bound": "hbm", "achieved": round(nbytes / ms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4), "launches": 1, "ms_per_step": round(ms, 4),
                     "algorithmic_mb_per_launch": round(nbytes / 1e6, 2), "boards_per_launch": n_boards}
    out["extract_squares_u8"]["note"] = ("warp + gray + flip + split incl. the rectified boards; ~75 integer + fp64 vector instructions per pixel "
                                         "(OpenCV-exact double-precision coordinates): VALU-bound, not HBM-bound (DESIGN.md section 4)")
    return out


def concurrent_requests(cv, images, threads=4, per_thread=200):
    """`process_image` from `threads` request threads of one instance; every result (FEN + probabilities) is kept and compared with
    the serial call's AFTER the timed loop.  Returns requests/s, the number of slots and the number of differing results."""
    import threading

    import numpy as np

    slots = cv.warm_request_slots(threads)
    want = [cv.process_image(im) for im in images]
    n_img = len(images)
    got = [[None] * per_thread for _ in range(threads)]

    def worker(t):
        mine = got[t]
        for k in range(per_thread):
            r = cv.process_image(images[(t + k) % n_img])
            mine[k] = None if r.position is None else (r.position.fen, r.position.model_probabilities)   # (the 0.8 MB of images go)

    def run_threads(fn):
        ths = [threading.Thread(target=fn, args=(t,)) for t in range(threads)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        return time.perf_counter() - t0

    # the replicas have never run: their first call grows the workspace, their second records the hipGraphs -- outside the timed loop
    run_threads(lambda t: [cv.process_image(images[(t + k) % n_img]) for k in range(20)])
    dt = run_threads(worker)
    bad = 0
    for t in range(threads):
        for k, r in enumerate(got[t]):
            w = want[(t + k) % n_img]
            if (r is None) != (w.position is None) or (r is not None and (
                    r[0] != w.position.fen or not np.array_equal(r[1], w.position.model_probabilities))):
                bad += 1
    return {"per_sec": round(threads * per_thread / dt, 1), "slots": slots, "calls": threads * per_thread, "differing": bad}


def process_image_latency(cv, iters=100):
    """Median wall milliseconds of `ChessVision.process_image` -- the entry point the reference's Flask endpoint and eval script
    call (cv_endpoint.py:159, evaluate.py:270) -- on 512x512 photos, warm, one call at a time (host image in, FEN out)."""
    import numpy as np

    from chessvision import synthetic

    images = [synthetic.board_photo(1000 + s) for s in range(8)]
    for im in images:
        cv.process_image(im)
    times, found = [], 0
    for k in range(iters):
        t0 = time.perf_counter()
        r = cv.process_image(images[k % 8])
        times.append((time.perf_counter() - t0) * 1e3)
        found += int(r.position is not None)
    a = np.array(times)
    # the same entry point from four request threads of ONE instance (the reference's Flask app: a global instance, threaded server,
    # cv_endpoint.py:131-133): every thread gets a request slot of its own (engines, staging block, stream), results are the serial ones.
    # (Until late in round 6 this read 1480-2120 requests/s against 2310-2375 in tests/dev/concurrent_probe.py: the four slots were
    # first used all at once here, and the HIP runtime binds streams to hardware queues at first use -- ChessVision._warm_slot.)
    conc = {}
    try:
        inside = concurrent_requests(cv, images)
        conc = {"concurrent4_per_sec": inside["per_sec"], "concurrent4_slots": inside["slots"], "concurrent4_calls": inside["calls"],
                "concurrent4_results_differing_from_serial": inside["differing"], "serial_per_sec": round(1e3 / float(np.median(a)), 1)}
    except Exception as exc:                                                  # extra figure only
        conc["concurrent4_error"] = repr(exc)
    return {"process_image_ms_median": round(float(np.median(a)), 3), "process_image_ms_p10": round(float(np.percentile(a, 10)), 3),
            "process_image_ms_p90": round(float(np.percentile(a, 90)), 3), "iters": iters, "boards_found": found, **conc,
            "image": "512x512x3 uint8 on the host", "note": "UNet B=1 + ResNet-18 B=64 (split-K launches, hipGraph replay), C++ contours, "
                                                              "device resize / warp; the host waits twice per call (an event behind the UNet, one stream synchronisation at the end)"}


def measure(eng, x, sq, steps, warmup, device, cvd, streams=None):
    """W warm-up steps, then exactly K timed steps bracketed by barrier + synchronize; returns (seconds, outputs of the last step)."""
    def step():
        if streams is None:
            return eng.unet_forward(x, check=False), eng.resnet18_forward(sq, check=False)
        cur = torch.cuda.current_stream(device)
        for st in streams:
            st.wait_stream(cur)
        with torch.cuda.stream(streams[0]):
            a = eng.unet_forward(x, check=False)
        with torch.cuda.stream(streams[1]):
            b = eng.resnet18_forward(sq, check=False)
        for st in streams:
            cur.wait_stream(st)
        return a, b

    for _ in range(warmup):
        out = step()
    cvd.barrier(device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize(device)
    cvd.barrier(device)
    elapsed = cvd.max_over_ranks(time.perf_counter() - t0, device)
    eng.check_numerics()                                           # the numeric guard, once for the whole run
    return elapsed, out


DUMP_LIMIT_BYTES = 60_000_000                                      # under the 64 MB a dump may hold, .npy headers included


def dump_outputs(dst, out):
    """What a caller of the timed path receives from its last step, as float32 .npy files in `dst`:
      resnet18_logits.npy  (squares, 13), every square (up to half the limit, else a seeded sample of squares)
      unet_logits.npy      (boards, 1, 256, 256), every board when it fits the rest of the limit, else the boards of a fixed
                           seeded sample (numpy default_rng(0), sorted indices; 225 of the default 256 boards)
    The sample depends on the shapes only, so two builds run with the same arguments write the same rows."""
    import numpy as np

    dst = Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    room = DUMP_LIMIT_BYTES
    for name, t, share in (("resnet18_logits", out[1], 0.5), ("unet_logits", out[0], 1.0)):
        n, row = t.shape[0], t[0].numel() * 4
        k = min(n, int(room * share) // row)
        if k < n:
            keep = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
            t = t[torch.from_numpy(keep).to(t.device)]
        a = t.float().cpu().numpy()
        np.save(dst / f"{name}.npy", a)
        room -= a.nbytes


def rooflines(eng, x, sq, dtype, B, quiet=False):
    """HIP-event timing of every launch of one step on the launch stream (cv_profile_convs): the MFMA roofline of the conv
    family and the HBM roofline of each memory-bound kernel (algorithmic bytes / event time / 8 TB/s)."""
    conv_ms = conv_n = 0
    conv_flop = conv_bytes = all_ms = 0.0
    table, launches, per_model, hbm, chunks, by_kernel = {}, {}, {}, {}, {}, {}
    for model, inp in (("unet", x), ("resnet18", sq)):
        # one un-timed pass right in front of the event-timed one: the launches are timed at the clocks of a busy chip, not at
        # what the DVFS governor ramps through after the host-side pause since the timed region
        (eng.unet_forward if model == "unet" else eng.resnet18_forward)(inp, check=False)
        c_ms, c_n, a_ms, entries = eng.profile(model, inp, iters=1)
        conv_ms += c_ms; conv_n += c_n; all_ms += a_ms
        launches[model] = c_n
        per_model[model] = [c_ms, 0.0]
        probe = "down1.maxpool_conv.1.double_conv.0" if model == "unet" else "layer1.0.conv1"      # one launch per chunk
        chunks[model] = max(1, sum(e["name"] == probe for e in entries))
        for e in entries:
            if e["conv"]:
                conv_flop += 2.0 * e["macs"]
                conv_bytes += e["bytes"]
                per_model[model][1] += 2.0 * e["macs"]
                k = by_kernel.setdefault(e["kernel"], [0.0, 0.0, 0])
                k[0] += e["ms"]; k[1] += 2.0 * e["macs"]; k[2] += 1
            else:
                h = hbm.setdefault(e["name"], [0.0, 0.0, 0, 0.0])
                h[0] += e["ms"]; h[1] += e["bytes"]; h[2] += 1; h[3] += 2.0 * e["macs"]
            t = table.setdefault(f"{model}:{e['name']}", [0.0, 0.0, 0.0])
            t[0] += e["ms"]; t[1] += 2.0 * e["macs"]; t[2] += e["bytes"]
    if not quiet:
        for k, (ms, fl, by) in table.items():
            log(f"  {k:52s} {ms:9.3f} ms {fl / (ms * 1e-3) / 1e12 if ms > 0 else 0:8.1f} TFLOP/s {by / (ms * 1e-3) / 1e9 if ms > 0 else 0:9.1f} GB/s")
    achieved = conv_flop / (conv_ms * 1e-3) / 1e12
    peak = PEAK_TFLOPS[dtype]
    roof = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4),
            "algorithmic_bytes": conv_bytes / max(conv_n, 1),
            "kernel": "conv family: conv3x3_halo_kernel + conv_igemm_kernel + inc0_mfma_kernel, all instantiations", "launches_per_step": conv_n,
            "avg_launch_ms": round(conv_ms / max(conv_n, 1), 4), "algorithmic_gflop_per_step": round(conv_flop / 1e9, 2),
            "by_model": {m: {"achieved": round(fl / (ms * 1e-3) / 1e12, 2), "frac": round(fl / (ms * 1e-3) / 1e12 / peak, 4)}
                         for m, (ms, fl) in per_model.items()},       # north_star: >= 50 % on the UNet conv stages
            "mfma_products_per_mac": MFMA_PER_MAC[dtype],
            "mfma_issued_tflops": round(achieved * MFMA_PER_MAC[dtype], 2),
            "frac_of_raw_mfma_peak": round(achieved * MFMA_PER_MAC[dtype] / (157.3 if dtype == "f32" else 2500.0), 4),
            "conv_family_hbm_gbs": round(conv_bytes / (conv_ms * 1e-3) / 1e9, 1)}
    # the instantiation that holds most of the step's time, reproducible from a rocprofv3 kernel trace by template name
    dom = max(by_kernel, key=lambda k: by_kernel[k][0])
    roof["dominant"] = {"kernel": dom, "launches_per_step": by_kernel[dom][2], "avg_launch_ms": round(by_kernel[dom][0] / by_kernel[dom][2], 4),
                        "ms_per_step": round(by_kernel[dom][0], 3), "share_of_conv_time": round(by_kernel[dom][0] / conv_ms, 4),
                        "algorithmic_gflop": round(by_kernel[dom][1] / 1e9, 2),
                        "achieved": round(by_kernel[dom][1] / (by_kernel[dom][0] * 1e-3) / 1e12, 2),
                        "frac": round(by_kernel[dom][1] / (by_kernel[dom][0] * 1e-3) / 1e12 / peak, 4)}
    roof["by_kernel"] = {k: {"launches": v[2], "ms_per_step": round(v[0], 3), "achieved": round(v[1] / (v[0] * 1e-3) / 1e12, 2)}
                         for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][0])}
    roof_hbm = {}
    for name, (ms, by, cnt, fl) in hbm.items():
        if ms <= 0:
            continue
        blk = {"bound": "hbm", "achieved": round(by / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "launches": cnt, "ms_per_step": round(ms, 4),
               "algorithmic_mb_per_launch": round(by / cnt / 1e6, 2)}
        if fl > 1e9:      # the fused stem is a conv on the matrix cores (K padded 49 -> 64): carry its MFMA figure as well
            blk["mfma_tflops_algorithmic"] = round(fl / (ms * 1e-3) / 1e12, 1)
            blk["mfma_frac_of_dtype_peak"] = round(fl / (ms * 1e-3) / 1e12 / peak, 4)
        roof_hbm[name] = blk
    roof["launches_by_model"] = {m: launches[m] for m in ("unet", "resnet18")}
    launches["chunks"] = chunks
    return roof, roof_hbm, launches, conv_ms, conv_n, all_ms


def flatten_evidence(result):
    """The driver's record of this line keeps `config`, `roofline` and `cpu_baseline` -- about 23 scalar entries each, names cut at 40
    characters, strings at 128 -- and only the NAMES of the other top-level blocks.  The figures a reader needs to judge the run are
    therefore mirrored into `config` and `roofline` as flat scalars under SHORT names and placed FIRST; the longer
    names of earlier rounds follow for the tests and tools that read them."""
    cfg, roof = result["config"], result["roofline"]

    def pick(d, *path):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d

    def put(dst, key, val):
        if val is not None and not isinstance(val, (dict, list)):
            dst[key] = val

    lat = pick(result, "pipeline_e2e", "latency")
    head = {}
    for key in ("workload", "boards_per_gpu", "global_boards_per_step", "gflop_per_board"):
        put(head, key, cfg.get(key))
    put(head, "par_unet_err", pick(result, "parity_vs_oracle", "unet_logit_max_abs_err"))       # headline engine vs the fp32 CPU oracle, same run
    put(head, "par_resnet_err", pick(result, "parity_vs_oracle", "resnet_logit_max_abs_err"))
    put(head, "par_boards", pick(result, "parity_vs_oracle", "boards_checked"))
    put(head, "cls16_frac", pick(result, "classifier_fp16", "roofline", "frac"))                # fp16 classifier (configs[2]): of the 2.5 PF f16 peak
    put(head, "cls16_ms", pick(result, "classifier_fp16", "ms_per_pass"))
    put(head, "cls16_prob_err", pick(result, "classifier_fp16", "parity_vs_oracle", "prob_max_abs_err"))
    put(head, "cls16_worst_err", pick(result, "classifier_fp16_seed_search", "worst_prob_err"))  # worst network of the seed search
    put(head, "cls16_worst_nets", pick(result, "classifier_fp16_seed_search", "networks"))
    put(head, "cls16_step_bps", pick(result, "classifier_fp16", "step_with_headline_unet", "boards_per_sec"))
    put(head, "f32_bps", pick(result, "by_dtype", "f32", "value"))
    put(head, "f32_frac", pick(result, "by_dtype", "f32", "roofline", "frac"))
    put(head, "bil_bps", pick(result, "by_variant", "bilinear", "value"))
    put(head, "e2e_bps", pick(result, "pipeline_e2e", "boards_per_sec"))                         # host photos -> FEN: best of 5 calls ...
    put(head, "e2e_bps_median", pick(result, "pipeline_e2e", "boards_per_sec_median"))          # ... their median ...
    put(head, "e2e_bps_min", pick(result, "pipeline_e2e", "boards_per_sec_min"))                # ... and the slowest
    put(head, "e2e_fen_bad", pick(result, "pipeline_e2e", "fen_mismatches"))
    if isinstance(lat, dict):
        put(head, "lat_ms_median", lat.get("process_image_ms_median"))
        put(head, "conc4_per_sec", lat.get("concurrent4_per_sec"))
    put(head, "rccl_ranks_seen", result.get("rccl_ranks_seen"))
    put(head, "e2e_ranks_bps", pick(result, "pipeline_e2e_ranks", "boards_per_sec_whole_job"))

    put(cfg, "dist_backend", result.get("dist_backend"))
    put(cfg, "init_s_max_over_ranks", pick(result, "init_s", "max"))
    put(cfg, "device_memory_peak_used_gb", pick(result, "device_memory", "peak_used_gb_max_over_ranks"))
    put(cfg, "pipeline_e2e_ranks_order_mismatches", pick(result, "pipeline_e2e_ranks", "order_mismatches"))
    put(cfg, "pipeline_e2e_ranks_gather_s_max", pick(result, "pipeline_e2e_ranks", "gather_s", "max"))
    put(cfg, "calibration_identical_across_ranks", pick(result, "calibration_sync", "identical_across_ranks"))
    put(cfg, "sharding_gathered_in_order", pick(result, "sharding", "gathered_in_order"))
    put(cfg, "parity_unet_logit_max_abs_err", pick(result, "parity_vs_oracle", "unet_logit_max_abs_err"))
    put(cfg, "parity_resnet_logit_max_abs_err", pick(result, "parity_vs_oracle", "resnet_logit_max_abs_err"))
    put(cfg, "parity_boards_checked", pick(result, "parity_vs_oracle", "boards_checked"))
    put(cfg, "pipeline_e2e_boards_per_sec", pick(result, "pipeline_e2e", "boards_per_sec"))
    if pick(result, "pipeline_e2e", "boards_per_sec") and result.get("value"):
        cfg["pipeline_e2e_frac_of_resident_rate"] = round(result["pipeline_e2e"]["boards_per_sec"] / result["value"], 4)
    put(cfg, "pipeline_e2e_fen_checked", pick(result, "pipeline_e2e", "fen_checked"))
    put(cfg, "pipeline_e2e_fen_mismatches", pick(result, "pipeline_e2e", "fen_mismatches"))
    put(cfg, "pipeline_e2e_board_byte_mismatches_vs_oracle", pick(result, "pipeline_e2e", "board_byte_mismatches_vs_oracle"))
    put(cfg, "pipeline_e2e_prob_max_abs_err_vs_oracle", pick(result, "pipeline_e2e", "prob_max_abs_err_vs_oracle"))
    put(cfg, "pipeline_e2e_fp16_classifier_boards_per_sec", pick(result, "pipeline_e2e", "classifier_fp16", "boards_per_sec"))
    if isinstance(lat, dict):
        for k in ("process_image_ms_median", "process_image_ms_p10", "process_image_ms_p90"):
            put(cfg, "latency_" + k, lat.get(k))
    for dt in ("f32", "f16"):
        put(cfg, f"{dt}_boards_per_sec", pick(result, "by_dtype", dt, "value"))
        put(cfg, f"{dt}_roofline_frac", pick(result, "by_dtype", dt, "roofline", "frac"))
        put(cfg, f"{dt}_parity_unet_logit_max_abs_err", pick(result, "by_dtype", dt, "parity_vs_oracle", "unet_logit_max_abs_err"))
    put(cfg, "classifier_fp16_step_boards_per_sec", pick(result, "classifier_fp16", "step_with_headline_unet", "boards_per_sec"))
    put(cfg, "classifier_fp16_prob_max_abs_err", pick(result, "classifier_fp16", "parity_vs_oracle", "prob_max_abs_err"))
    put(cfg, "bilinear_variant_boards_per_sec", pick(result, "by_variant", "bilinear", "value"))
    put(cfg, "pipeline_e2e_ranks_whole_job_boards_per_sec", pick(result, "pipeline_e2e_ranks", "boards_per_sec_whole_job"))
    put(cfg, "pipeline_e2e_ranks_precision", pick(result, "pipeline_e2e_ranks", "precision"))
    for k in ("min", "mean", "max"):
        put(cfg, f"pipeline_e2e_ranks_boards_per_sec_{k}", pick(result, "pipeline_e2e_ranks", "boards_per_sec_per_rank", k))
    ordered = dict(head)
    for k, v in cfg.items():
        ordered.setdefault(k, v)
    if isinstance(lat, dict):
        ordered["latency"] = lat                                 # the block itself, last
    result["config"] = ordered

    rhead = {}
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "kernel", "launches_per_step", "avg_launch_ms"):
        if key in roof:
            rhead[key] = roof[key]                               # `traffic` stays even when null (the contract names it)
    put(rhead, "dominant_kernel", pick(roof, "dominant", "kernel"))
    put(rhead, "dominant_frac", pick(roof, "dominant", "frac"))
    put(rhead, "dominant_avg_launch_ms", pick(roof, "dominant", "avg_launch_ms"))
    put(rhead, "unet_conv_frac", pick(roof, "by_model", "unet", "frac"))
    put(rhead, "resnet18_conv_frac", pick(roof, "by_model", "resnet18", "frac"))
    hbm_all = dict(result.get("roofline_hbm") or {})
    for name, blk in (pick(result, "by_variant", "bilinear", "roofline_hbm") or {}).items():
        hbm_all.setdefault(name, blk)                            # the bilinear variant's up-sampling kernel
    short = {"upsample": "hbm_upsample_frac", "stem": "hbm_stem_frac", "head": "hbm_head_frac", "resize": "hbm_resize_frac",
             "extract_squares": "hbm_warp_frac"}
    for name, blk in hbm_all.items():
        if isinstance(blk, dict) and "frac" in blk:
            for word, key in short.items():
                if word in name:
                    rhead.setdefault(key, blk["frac"])
    put(rhead, "dominant_launches_per_step", pick(roof, "dominant", "launches_per_step"))
    put(rhead, "dominant_share_of_conv_time", pick(roof, "dominant", "share_of_conv_time"))
    for name, blk in hbm_all.items():
        if isinstance(blk, dict) and "frac" in blk:
            key = "hbm_" + "".join(c if c.isalnum() else "_" for c in name).strip("_")
            rhead[key + "_frac"] = blk["frac"]
            rhead[key + "_gbs"] = blk["achieved"]
    for k, v in roof.items():
        rhead.setdefault(k, v)
    result["roofline"] = rhead


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default=os.environ.get("CV_BENCH_DTYPE", "f16x3"), choices=["f32", "f16", "f16x3"])
    ap.add_argument("--unet-variant", default="convT", choices=["convT", "bilinear"],
                    help="UNet up-sampling: transposed conv (default checkpoint layout) or bilinear (train_unet.py:440,461-465)")
    ap.add_argument("--boards", type=int, default=256, help="boards per GPU per step")
    ap.add_argument("--unet-chunk", type=int, default=64)
    ap.add_argument("--resnet-chunk", type=int, default=16384)
    ap.add_argument("--overlap", type=int, default=int(os.environ.get("CV_BENCH_OVERLAP", "0")),
                    help="1: enqueue the UNet pass and the ResNet pass of a step on two HIP streams (they are independent)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the by_dtype / by_variant / pipeline_e2e blocks")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--fp16-search-budget", type=float, default=45.0,
                    help="seconds for the fp16 classifier's worst-case search over weight seeds (oracle leg; 0 = skip)")
    ap.add_argument("--extra-steps", type=int, default=10, help="timed steps of each by_dtype / by_variant / classifier_fp16 leg")
    ap.add_argument("--extra-warmup", type=int, default=3)
    ap.add_argument("--e2e-precision", default=None,
                    help="precision of the sharded host-images-to-FEN leg at N > 1 (BASELINE configs[4] says fp16: default "
                         "'<dtype>+f16r' = the headline UNet with the classifier in its fp16 mode)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: rooflines, CPU baseline + oracle parity, other precisions / variant, pipeline legs, multi-rank checks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0's boards) as float32 .npy files into DIR")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args, sys.argv[1:]))

    # Only the JSON line may reach stdout: native libraries (RCCL prints "Librccl path : ..." through C stdio, flushed at exit)
    # write to file descriptor 1 behind Python's back, so fd 1 is pointed at stderr for the whole run and the line goes to a
    # private duplicate of the real stdout.
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    from chessvision import distributed as cvd
    from chessvision import synthetic
    from chessvision.hip_backend import HipEngine

    rank, world, device = cvd.init_process_group()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if device.type != "cuda":
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")

    # ---- weights: rank 0 generates, one RCCL broadcast replicates ----
    t_init = time.perf_counter()
    bilinear = args.unet_variant == "bilinear"
    uspec, rspec = synthetic.unet_spec(bilinear), synthetic.resnet18_spec()
    usd = cvd.broadcast_state_dict(synthetic.unet_state_dict(1, bilinear) if rank == 0 else None, uspec, device)
    rsd = cvd.broadcast_state_dict(synthetic.resnet18_state_dict(2) if rank == 0 else None, rspec, device)
    if args.full:
        rccl_ranks = cvd.count_ranks(device)                     # an all-reduce of ones over RCCL: every rank really took part

    def make_engine(dtype, unet_sd=usd):
        e = HipEngine(device, precision=dtype, unet_chunk=args.unet_chunk, resnet_chunk=args.resnet_chunk)
        e.load_unet(unet_sd)
        e.load_resnet18(rsd)
        return e

    eng = make_engine(args.dtype)
    calibration = cvd.sync_calibration(eng, device)              # every rank computes with rank 0's tensor exponents
    torch.cuda.synchronize(device)
    init_mine = time.perf_counter() - t_init
    if args.full:
        init_s = cvd.stats_over_ranks(init_mine, device)   # weights: generate (rank 0) + broadcast + pack + calibrate
        init_per_rank = cvd.list_over_ranks(init_mine, device)
        mem = _DeviceMemory(device)

    # ---- synthetic inputs, resident in HBM before the timed region ----
    # ONE global batch of world * B boards, board i drawn from its own seed; rank r holds boards r::world of it (SURVEY.md
    # section 8e, BASELINE configs[4]) -- no rank ever materialises another rank's boards.
    B = args.boards
    mine = list(cvd.shard_indices(world * B, rank, world))
    x = torch.empty((B, 3, 256, 256), dtype=torch.float32, device=device)
    sq = torch.empty((B * 64, 1, 64, 64), dtype=torch.float32, device=device)
    gen = torch.Generator(device=device)
    for k, i in enumerate(mine):
        gen.manual_seed(1234 + i)
        x[k] = torch.randint(0, 256, (3, 256, 256), dtype=torch.uint8, device=device, generator=gen)
        sq[k * 64:(k + 1) * 64] = torch.randint(0, 256, (64, 1, 64, 64), dtype=torch.uint8, device=device, generator=gen)
    x /= 255.0
    sq /= 255.0
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)] if args.overlap else None

    elapsed, out = measure(eng, x, sq, args.steps, args.warmup, device, cvd, streams)
    if args.full:
        mem.sample()                                      # every rank's workspace has grown to its chunk
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)

    headline = {
        "metric": "boards/sec (UNet 256x256 seg + 64-sq classify)",
        "value": round(value, 2), "unit": "boards/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
    }
    workload = (f"e2e-cnn b={B}/GPU: UNet(3->1,{'bilinear' if bilinear else 'convT'}) 256x256 x{B} boards + ResNet-18(1ch,13cls) x{B * 64} "
                "squares/step; in HBM (configs[3])")
    parallelism = f"replicas x{world}, boards sharded, weights RCCL-broadcast once"
    if not args.full:
        if rank == 0:
            macs_board = eng.model_macs("unet") + 64 * eng.model_macs("resnet18")
            result = {**headline,
                      "config": {"workload": workload, "boards_per_gpu": B, "global_boards_per_step": world * B, "parallelism": parallelism,
                                 "gflop_per_board": round(2 * macs_board / 1e9, 3)},
                      "calibration_sync": calibration, "host_threads_per_rank": cvd.host_threads(),
                      "e2e_tflops": round(2 * macs_board * value / 1e12, 2)}
            log(f"  step: {ms_per_step:.2f} ms over {args.steps} timed steps")
            print(json.dumps(result), file=json_out, flush=True)
        cvd.barrier(device)
        cvd.shutdown()
        return

    # outputs stay rank-local in a throughput run; one small gather proves the shard map: per board its global index and a
    # checksum of its 64 x 13 logits travel rank-major and must re-interleave to 0 .. world*B-1
    tag = torch.stack([torch.tensor(mine, dtype=torch.float64, device=device),
                       out[1].double().reshape(B, -1).sum(1)], dim=1)
    gathered = cvd.interleave_shards(cvd.all_gather_rows(tag), world).cpu()
    shard_ok = bool((gathered[:, 0] == torch.arange(world * B, dtype=torch.float64)).all()) and bool(torch.isfinite(gathered[:, 1]).all())

    # N > 1: every rank also runs the full host-images-to-FEN pipeline on its shard of one global list of photos
    e2e_ranks = None
    if world > 1 and not args.no_extras:
        e2e_prec = args.e2e_precision or (args.dtype if "+" in args.dtype or args.dtype == "f16r" else f"{args.dtype}+f16r")
        # the sharded pipeline loads its own engines: the throughput engine's workspace (27 GB at the default chunks) is released first so
        # that eight ranks sharing ONE device (the gloo test of configs[4]'s global shape) stay inside its 288 GB; rank 0 reloads it for
        # the roofline pass below
        eng.close()
        eng = None
        e2e_ranks = pipeline_e2e_sharded(e2e_prec, B, rank, world, device, cvd, mem)
        e2e_ranks["precision"] = e2e_prec
    peak_mem = cvd.max_over_ranks(mem.peak_gb, device)

    if rank != 0:
        cvd.barrier(device)                              # leave together with rank 0 (it still profiles and reports)
        cvd.shutdown()
        return

    if eng is None:
        eng = make_engine(args.dtype)
    roof, roof_hbm, launches, conv_ms, conv_n, all_ms = rooflines(eng, x, sq, args.dtype, B)
    if not args.no_extras:
        try:
            roof_hbm.update(byte_kernel_rooflines(eng, device))
        except Exception as exc:
            roof_hbm["byte_kernels_error"] = repr(exc)
    macs_board = eng.model_macs("unet") + 64 * eng.model_macs("resnet18")
    log(f"  step: {ms_per_step:.2f} ms; event-timed kernels {all_ms:.2f} ms; conv family {conv_ms:.2f} ms over {conv_n} launches")

    # effective chunk sizes from the number of passes (the f32 engine halves the classifier chunk to stay under 4 GiB per tensor)
    eff_unet = B // launches["chunks"]["unet"]
    eff_resnet = B * 64 // launches["chunks"]["resnet18"]
    traffic, traffic_why = (None, "bilinear variant: no counters committed") if bilinear else \
        pmc_traffic(args.dtype, args.unet_chunk, args.resnet_chunk, launches["unet"], launches["resnet18"])
    roof["traffic"] = traffic
    if traffic is None:
        roof["traffic_null_reason"] = traffic_why
    roof["traffic_source"] = (f"{PMC_FILE} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950-corrected; a committed profile "
                              "of this workload, NOT collected by this run)") if traffic is not None else None
    roof["traffic_unit"] = "HBM bytes per conv launch; algorithmic_bytes = compulsory bytes per launch (cv_profile_entry_bytes)"

    variant_name = "bilinear up-sampling" if bilinear else "transposed-conv"
    result = {
        **headline,
        "config": {"workload": workload,
                   "boards_per_gpu": B, "global_boards_per_step": world * B, "unet_chunk": eff_unet,
                   "resnet_chunk": eff_resnet, "parallelism": parallelism,
                   "gflop_per_board": round(2 * macs_board / 1e9, 3)},
        "rccl_ranks_seen": rccl_ranks, "dist_backend": cvd.backend_name(),
        "init_s": {k: round(v, 3) for k, v in init_s.items()}, "init_s_per_rank": [round(v, 3) for v in init_per_rank],
        "calibration_sync": calibration,
        "device_memory": {"peak_used_gb_max_over_ranks": round(peak_mem, 2), "device_total_gb": round(mem.total / 1e9, 2),
                          "note": "hipMemGetInfo total - free, device-wide (ranks sharing one GPU under CV_DIST_BACKEND=gloo all count), sampled after "
                                  "the timed steps and after the sharded pipeline's warm-up"},
        "sharding": {"global_boards": world * B, "rule": "rank r owns boards r::world", "gathered_in_order": shard_ok},
        "host_threads_per_rank": cvd.host_threads(),
        "e2e_tflops": round(2 * macs_board * value / 1e12, 2),
        "roofline": roof,
        "roofline_hbm": roof_hbm,
    }
    if e2e_ranks is not None:
        result["pipeline_e2e_ranks"] = e2e_ranks
    oracle_out = None
    if world == 1 and not args.no_cpu_baseline:
        e2e_block = e2e_imgs = e2e_res = None
        if not args.no_extras:
            try:
                e2e_block, e2e_imgs, e2e_res = pipeline_e2e(args.dtype)
            except Exception as exc:                                      # extra figure only; never hides the headline
                e2e_block = {"error": repr(exc)}
        nchk = min(B, 64)
        base, parity, ref_fens, oracle_out, fp16_search = cpu_baseline(x[:nchk].cpu(), sq[:nchk * 64].cpu(), out[0][:nchk].cpu(), out[1][:nchk * 64].cpu(),
                                              e2e_images=e2e_imgs, budget_s=args.cpu_budget, e2e_results=e2e_res,
                                              fp16_search_s=0.0 if args.no_extras else args.fp16_search_budget, device=device)
        result["cpu_baseline"] = base
        result["parity_vs_oracle"] = parity
        if fp16_search is not None:
            result["classifier_fp16_seed_search"] = fp16_search
        if e2e_block is not None:
            if ref_fens is not None and e2e_res is not None:
                import numpy as np
                mism = sum((r.position.fen, r.position.original_fen) != (f[0], f[1]) for r, f in zip(e2e_res, ref_fens))
                perr = max(float(np.abs(r.position.model_probabilities - f[2]).max()) for r, f in zip(e2e_res, ref_fens))
                e2e_block.update({"fen_checked": len(ref_fens), "fen_mismatches": mism, "prob_max_abs_err_vs_oracle": perr,
                                  "board_byte_mismatches_vs_oracle": sum(bool(f[3]) for f in ref_fens)})
            result["pipeline_e2e"] = e2e_block
    if world == 1 and not args.no_extras:
        # the other arithmetic types and the other checkpoint variant, XS steps after XW warm-ups each, with their own roofline and parity
        XS, XW = args.extra_steps, args.extra_warmup
        by_dtype = {}
        for dt in ("f32", "f16"):
            if dt == args.dtype:
                continue
            try:
                e2 = make_engine(dt)
                el, o2 = measure(e2, x, sq, XS, XW, device, cvd)
                r2, _, _, _, _, _ = rooflines(e2, x, sq, dt, B, quiet=True)
                entry = {"value": round(B * XS / el, 2), "unit": "boards/sec", "ms_per_step": round(el / XS * 1e3, 3), "steps": XS, "warmup": XW,
                         "roofline": {k: r2[k] for k in ("bound", "achieved", "peak", "unit", "frac", "by_model")}}
                if oracle_out is not None:                                # same oracle outputs as parity_vs_oracle above
                    nb_ = oracle_out[0].shape[0]
                    entry["parity_vs_oracle"] = {"unet_logit_max_abs_err": float((o2[0][:nb_].cpu() - oracle_out[0]).abs().max()),
                                                 "resnet_logit_max_abs_err": float((o2[1][:nb_ * 64].cpu() - oracle_out[1]).abs().max()),
                                                 "boards_checked": nb_}
                by_dtype[dt] = entry
                e2.close()
            except Exception as exc:
                by_dtype[dt] = {"error": repr(exc)}
        result["by_dtype"] = by_dtype
        try:
            result["classifier_fp16"] = classifier_fp16(eng, x, sq, B, rsd, args, device, cvd, oracle_out)
        except Exception as exc:
            result["classifier_fp16"] = {"error": repr(exc)}
        if not bilinear:
            try:
                usd_b = synthetic.unet_state_dict(1, True)
                e3 = make_engine(args.dtype, usd_b)
                el, _ = measure(e3, x, sq, XS, XW, device, cvd)
                r3, h3, _, _, _, _ = rooflines(e3, x, sq, args.dtype, B, quiet=True)
                mb = e3.model_macs("unet") + 64 * e3.model_macs("resnet18")
                result["by_variant"] = {"bilinear": {"value": round(B * XS / el, 2), "unit": "boards/sec", "ms_per_step": round(el / XS * 1e3, 3), "steps": XS, "warmup": XW,
                                                     "gflop_per_board": round(2 * mb / 1e9, 3),
                                                     "roofline": {k: r3[k] for k in ("bound", "achieved", "peak", "unit", "frac", "by_model")},
                                                     "roofline_hbm": {k: v for k, v in h3.items() if "upsample" in k}}}
                e3.close()
            except Exception as exc:
                result["by_variant"] = {"bilinear": {"error": repr(exc)}}
    flatten_evidence(result)
    print(json.dumps(result), file=json_out, flush=True)
    cvd.barrier(device)
    cvd.shutdown()


if __name__ == "__main__":
    main()
