#!/usr/bin/env python3
"""Write the JPEG decoder's fixtures.  Run in the build container only (the one place Pillow and the reference's data exist):

    python tests/golden/make_jpeg_cases.py

jpeg_cases.npz -- synthetic streams WRITTEN by Pillow (libjpeg-turbo) with Pillow's own decode of each as the expected pixels:

    names            (N,) str     every case, in order
    kind             (N,) str     "group" (decoded, three per geometry), "feature" and "extra" (decoded), "refusal" (must be refused)
    group            (N,) str     "<sampling>_<w>x<h>" for the cases one launch decodes together, "" otherwise
    reason           (N,) str     for refusals: a word the reported reason must contain
    blob/<name>      uint8        the stream
    pixels/<name>    uint8        Pillow's decode: (h, w, 3) RGB, or (h, w) for 1-component streams (absent for refusals)
    orientation      (N,) int     the EXIF orientation tag the stream carries (0: none)
    pillow_version, libjpeg_turbo_version   str

  geometries: 4:2:0 on the full grid w, h in {1, 2, 3, 15, 16, 17, 33} (chroma planes 1, 2 and odd samples wide and high, exactly
  one MCU, one pixel past an MCU); 4:2:2, 4:4:4 and gray on the diagonal plus (33, 15) and (15, 33).  Each geometry three times, so
  that one launch sees three quantisation tables: noise at quality 100 (every coefficient live, the clamps hit), a gradient at 75,
  a flat image at 30 (DC-only blocks).

photos8_jpeg_{a,b}.npz -- the original bytes of the eight reference photos named in photos8_{i}.npz["names"] (data the reference's
programs read); their expected pixels are the existing photos8_{i}.npz["bgr"].

    names (4,) str | blob_0 .. blob_3 uint8
"""
from __future__ import annotations

import io
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, features

HERE = Path(__file__).resolve().parent
REFERENCE_TEST_DATA = "/root/reference/data/test"        # where make_photos.py found the eight photos
GRID = (1, 2, 3, 15, 16, 17, 33)


def content(rng, kind, w, h):
    if kind == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 1:
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(xx * 7 + 3) % 256, (yy * 5 + 40) % 256, ((xx + yy) * 3 + 90) % 256], axis=2).astype(np.uint8)
    return np.broadcast_to(np.array([200, 60, 110], np.uint8), (h, w, 3)).copy()


def encode(arr, sampling, **kw):
    im = Image.fromarray(arr, "RGB")
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}[sampling]
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return np.frombuffer(buf.getvalue(), np.uint8)


def pillow_pixels(blob):
    return np.asarray(Image.open(io.BytesIO(blob.tobytes())))


def segments(blob):
    """(marker, offset of its FF, end of its segment) up to and including SOS."""
    b, pos, out = blob.tobytes(), 2, []
    while True:
        marker, length = b[pos + 1], int.from_bytes(b[pos + 2:pos + 4], "big")
        out.append((marker, pos, pos + 2 + length))
        pos += 2 + length
        if marker == 0xDA:
            return out


def main():
    rng = np.random.default_rng(20260)
    names, kinds, groups, reasons, orient, arrays = [], [], [], [], [], {}

    def add(name, kind, blob, group="", reason="", orientation=0):
        names.append(name); kinds.append(kind); groups.append(group); reasons.append(reason); orient.append(orientation)
        arrays[f"blob/{name}"] = blob
        if kind != "refusal":
            arrays[f"pixels/{name}"] = pillow_pixels(blob)

    diagonal = [(s, s) for s in GRID] + [(33, 15), (15, 33)]
    for sampling, geoms in (("420", [(w, h) for w in GRID for h in GRID]), ("422", diagonal), ("444", diagonal), ("gray", diagonal)):
        for w, h in geoms:
            for kind, quality in ((0, 100), (1, 75), (2, 30)):
                add(f"{sampling}_{w}x{h}_{kind}", "group", encode(content(rng, kind, w, h), sampling, quality=quality), group=f"{sampling}_{w}x{h}")

    base = content(rng, 0, 48, 40) // 2 + content(rng, 1, 48, 40) // 2
    add("optimize", "feature", encode(base, "420", quality=85, optimize=True))
    add("restart_blocks", "feature", encode(base, "420", quality=85, restart_marker_blocks=1))
    add("restart_rows", "feature", encode(base, "420", quality=85, restart_marker_rows=1))
    add("quality1", "feature", encode(base, "420", quality=1))
    exif = Image.Exif()
    exif[0x0112] = 6
    add("exif_orientation", "feature", encode(base, "420", quality=85, exif=exif), orientation=6)
    add("comment", "feature", encode(base, "420", quality=85, comment=b"a COM segment the parser skips"))

    add("progressive", "refusal", encode(base, "420", quality=85, progressive=True), reason="progressive")
    small = encode(content(rng, 1, 16, 16), "420", quality=75)
    s411 = small.copy()                                        # luma sampling 2x2 -> 4x1 in the frame header: 4:1:1
    sof = next(s for s in segments(small) if s[0] == 0xC0)
    assert s411[sof[1] + 11] == 0x22
    s411[sof[1] + 11] = 0x41
    add("sampling_411", "refusal", s411, reason="sampling")
    segs = segments(small)
    dqt = next(s for s in segs if s[0] == 0xDB)
    dht = next(s for s in segs if s[0] == 0xC4)
    sos = segs[-1]
    cuts = {"truncated_in_marker_code": dqt[1] + 1, "truncated_in_marker_length": dqt[1] + 3, "truncated_in_quant_table": dqt[1] + 30,
            "truncated_in_huffman_table": dht[1] + 12, "truncated_in_frame_header": sof[1] + 8, "truncated_in_scan_header": sos[1] + 6,
            "truncated_at_scan_start": sos[2], "truncated_in_scan": (sos[2] + len(small)) // 2, "truncated_before_eoi": len(small) - 2,
            "truncated_in_eoi": len(small) - 1, "truncated_after_soi": 2, "truncated_in_soi": 1}
    for name, cut in cuts.items():
        add(name, "refusal", small[:cut].copy(), reason="truncated")

    # two small colour pictures of a geometry of their own, for calls that mix geometries (kind "extra": decoded like a feature)
    for k in range(2):
        add(f"mixed_64x48_{k}", "extra", encode(content(rng, 0, 64, 48) // 4 + content(rng, 1, 64, 48) // 2, "420", quality=90))

    np.savez_compressed(HERE / "jpeg_cases.npz", names=np.array(names), kind=np.array(kinds), group=np.array(groups), reason=np.array(reasons),
                        orientation=np.array(orient, np.int32), pillow_version=np.array(PIL.__version__),
                        libjpeg_turbo_version=np.array(str(features.version("libjpeg_turbo"))), **arrays)
    print("jpeg_cases.npz:", len(names), "cases,", (HERE / "jpeg_cases.npz").stat().st_size, "bytes")

    photo_names = [str(np.load(HERE / f"photos8_{i}.npz")["names"][0]) for i in range(8)]
    for tag, part in (("a", photo_names[:4]), ("b", photo_names[4:])):
        blobs = {}
        for k, name in enumerate(part):
            folder, file = name.split("/")
            blobs[f"blob_{k}"] = np.frombuffer((Path(REFERENCE_TEST_DATA) / folder / "raw" / file).read_bytes(), np.uint8)
        np.savez(HERE / f"photos8_jpeg_{tag}.npz", names=np.array(part), **blobs)
        print(f"photos8_jpeg_{tag}.npz:", (HERE / f"photos8_jpeg_{tag}.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
