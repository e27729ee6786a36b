"""Measurements behind profiles/jpeg_orientation.md.

    python tests/dev/jpeg_orientation_bench.py recon                      # 256 photos of 512 x 512: plain, tags 3 / 6 / 8, a device copy
    python tests/dev/jpeg_orientation_bench.py pipeline                   # process_encoded on 256 streams, with and without "exif"
    python tests/dev/jpeg_orientation_bench.py pipeline --package DIR     # the same streams through another build of the package
                                                                          # (DIR holds chessvision/ and lib/; an older one has no keyword)

``recon``: the coefficients of the eight committed photos, repeated 32 times, on the device; 30 rounds in which the variants alternate,
each between two device events.  Every turned result is first compared with the plain one turned on the host.  ``pipeline``: the same
256 streams as they are, with tag 6 on all, and with tags [0, 6, 8, 3, 5, 1, 6, 6] in runs of eight (an EXIF block is spliced in behind
SOI, the scan is untouched); one warm-up and five timed calls per variant, alternating, host clock around the whole call.  One
``RESULT {json}`` line per figure.  Needs an MI355X; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
GOLDEN = ROOT / "tests" / "golden"
MIXED_TAGS = [0, 6, 8, 3, 5, 1, 6, 6]


def photo_blobs() -> list:
    import numpy as np

    blobs = []
    for tag in "ab":
        z = np.load(GOLDEN / f"photos8_jpeg_{tag}.npz")
        blobs += [z[f"blob_{k}"].tobytes() for k in range(len(z["names"]))]
    return blobs


def with_tag(blob: bytes, tag: int) -> bytes:
    """The same stream with a little-endian EXIF block carrying ``tag`` behind SOI (tag 0: the stream as it is)."""
    if not tag:
        return blob
    tiff = b"II" + (42).to_bytes(2, "little") + (8).to_bytes(4, "little")
    ifd = (1).to_bytes(2, "little") + (0x0112).to_bytes(2, "little") + (3).to_bytes(2, "little") + (1).to_bytes(4, "little") \
        + int(tag).to_bytes(2, "little") + b"\x00\x00" + (0).to_bytes(4, "little")
    payload = b"Exif\x00\x00" + tiff + ifd
    return blob[:2] + b"\xff\xe1" + (len(payload) + 2).to_bytes(2, "big") + payload + blob[2:]


def report(label: str, **record) -> None:
    print("RESULT " + json.dumps({"label": label, **record}), flush=True)


def recon(label: str) -> None:
    import numpy as np
    import torch

    from chessvision import jpeg
    from chessvision.hip_backend import HipEngine

    eng = HipEngine(precision="f32")
    blobs = photo_blobs() * 32
    n = len(blobs)
    infos = [jpeg.jpeg_info(b) for b in blobs]
    info = infos[0]
    assert n == 256 and info.geometry == (512, 512, 3, 2, 2)
    co, qt = np.empty((n, 64 * info.blocks), np.int16), np.empty((n, 3, 64), np.uint16)
    jpeg.entropy_decode_many(blobs, infos, co, qt)
    co_d, qt_d = torch.from_numpy(co).cuda(), torch.from_numpy(qt.view(np.int16)).cuda()
    dst = torch.empty((n, 512, 512, 3), dtype=torch.uint8, device="cuda")
    dst2 = torch.empty_like(dst)
    variants = {"plain": lambda: eng.jpeg_reconstruct_dev(co_d, qt_d, info, "bgr", out=dst)}
    for tag in (3, 6, 8):
        variants[f"tag{tag}"] = (lambda t: lambda: eng.jpeg_reconstruct_dev(co_d, qt_d, info, "bgr", out=dst, orientation=t))(tag)
    variants["d2d_copy"] = lambda: dst2.copy_(dst)
    variants["plain"]()
    plain = dst.cpu().numpy()
    for tag in (3, 6, 8):                                # right before fast: every 17th image against the plain one turned on the host
        variants[f"tag{tag}"]()
        got = dst.cpu().numpy()
        ok = all(np.array_equal(got[k], jpeg.apply_orientation(plain[k], tag)) for k in range(0, n, 17))
        report(label, check=f"tag{tag} equals the plain decode turned", ok=bool(ok))
        assert ok
    for fn in variants.values():                         # warm up every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times: dict = {k: [] for k in variants}
    for _ in range(30):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1000.0)
    for k, v in times.items():
        v.sort()
        report(label, what=k, us_median=round(statistics.median(v), 1), us_min=round(v[0], 1), us_p90=round(v[int(0.9 * len(v))], 1), reps=len(v))
    eng.close()


def pipeline(label: str) -> None:
    from chessvision import ChessVision, jpeg, synthetic

    has_keyword = hasattr(jpeg, "apply_orientation")
    pe, pc = synthetic.save_checkpoints(Path(tempfile.mkdtemp()), segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    base = photo_blobs()
    sets = {"plain_streams": [base[k % 8] for k in range(256)],
            "all_tag6": [with_tag(base[k % 8], 6) for k in range(256)],
            "mixed_tags": [with_tag(base[k % 8], MIXED_TAGS[(k // 8) % 8]) for k in range(256)]}
    runs = [(name, "ignore") for name in sets] + ([("all_tag6", "exif"), ("mixed_tags", "exif")] if has_keyword else [])
    rates: dict = {r: [] for r in runs}
    for rep in range(6):                                 # the first round warms up
        for name, mode in runs:
            kw = {"orientation": "exif"} if mode == "exif" else {}
            tm: dict = {}
            t0 = time.perf_counter()
            res = cv.process_encoded(sets[name], fallback_quad=True, timings=tm, **kw)
            dt = time.perf_counter() - t0
            assert len(res) == 256 and all(x.position is not None for x in res)
            if rep:
                rates[(name, mode)].append((256 / dt, tm.get("jobs"), tm.get("jpeg_ms")))
    for (name, mode), v in rates.items():
        bps = sorted(x[0] for x in v)
        report(label, streams=name, orientation=mode, boards_per_s_median=round(statistics.median(bps), 1), min=round(bps[0], 1),
               max=round(bps[-1], 1), calls=len(bps), jobs=v[0][1], jpeg_ms_last=None if v[-1][2] is None else round(float(v[-1][2]), 3))
    cv.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("recon", "pipeline"))
    ap.add_argument("--package", default=str(ROOT / "chessvision-3lc_amd"), help="directory holding chessvision/ and lib/")
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    {"recon": recon, "pipeline": pipeline}[args.mode](args.label)


if __name__ == "__main__":
    main()
