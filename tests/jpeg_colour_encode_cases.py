"""The cases of the colour JPEG encoder's tests (tests/golden/jpeg_colour_encode_cases.npz, written by
tests/golden/make_jpeg_colour_encode_cases.py): how the inputs are made, how the file is read, the one real photo (a committed picture,
cropped here, never stored) and the six streams that are transcoded.  Images are BGR unless a group says otherwise."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
# (h, w): heights 2, 8 and 24 for the vertical chroma padding (rows fill no row group / no block), widths across 8, 16 and 32 for the
# horizontal one, (8, 17), (17, 33) and (33, 31) for dummy luma blocks on the right and at the bottom
GEOMETRIES = [(1, 1), (2, 9), (8, 8), (8, 17), (9, 16), (16, 16), (17, 33), (24, 40), (33, 31), (64, 64)]
SUBSAMPLINGS = ["4:2:0", "4:2:2", "4:4:4"]
QUALITIES = [1, 50, 95, 100]
THIRD = ["primaries", "binary", "const"]                # the third image of a group rotates through these
KINDS = ["noise", "smooth"] + THIRD
RGB_GROUPS = [((17, 33), "4:2:0", 95), ((9, 16), "4:2:2", 50), ((8, 17), "4:4:4", 100)]      # the same arrays read as RGB
PHOTO_CROP = (slice(200, 296), slice(180, 308))         # 96 x 128 of photos8_0
PHOTO_QUALITY, PHOTO_SUBSAMPLING = 95, "4:2:0"
# (file, name of the stream, quality, subsampling): what transcode_jpegs(orientation="exif") is held to; tags 0, 1, 6 and 8, one gray
TRANSCODES = [("jpeg_cases", "420_33x33_0", 95, "4:2:0"), ("jpeg_cases", "422_15x33_1", 50, "4:2:2"), ("jpeg_cases", "gray_17x17_0", 95, "4:2:0"),
              ("jpeg_orientation_cases", "420_15x33_t6", 95, "4:2:0"), ("jpeg_orientation_cases", "444_33x15_t8", 100, "4:4:4"),
              ("jpeg_orientation_cases", "422_15x33_t1", 1, "4:2:0")]


def make_image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "smooth":                                # one field, another phase in every channel
        return np.stack([np.clip(128 + 90 * np.sin(yy / 9.0 + 0.3 + 2.1 * c) * np.cos(xx / 13.0 + 1.3 * c) + 20 * (xx / max(1, w - 1)), 0, 255)
                         for c in range(3)], axis=-1).astype(np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "primaries":                             # 3 x 5 patches of saturated colours: chroma steps inside blocks
        table = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
        return table[((yy // 3) * 3 + xx // 5 + seed) % 8]
    if kind == "const":
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    raise ValueError(kind)


def image_seed(gi: int, kind: str) -> int:
    return 1000 * gi + sum(map(ord, kind))


def group_kinds(gi: int, si: int, qi: int) -> list[str]:
    """The three images that go into ONE launch for geometry gi, subsampling si, quality qi: different content in one batch."""
    return ["noise", "smooth", THIRD[(gi + si + qi) % 3]]


def group_list() -> list[tuple]:
    """(name, (h, w), subsampling, quality, channel_order, kinds) of every launch group, in the order of the file.  If the file has to
    shrink, qualities go at 64 x 64, never a geometry."""
    out = []
    for gi, (h, w) in enumerate(GEOMETRIES):
        for si, sub in enumerate(SUBSAMPLINGS):
            for qi, q in enumerate(QUALITIES):
                out.append((f"{h}x{w}-{sub}-q{q}", (h, w), sub, q, "bgr", group_kinds(gi, si, qi)))
    for (h, w), sub, q in RGB_GROUPS:
        out.append((f"{h}x{w}-{sub}-q{q}-rgb", (h, w), sub, q, "rgb", ["noise", "smooth", "primaries"]))
    return out


def photo() -> np.ndarray:
    """The first committed photo, 512 x 512 BGR."""
    return np.ascontiguousarray(np.load(GOLDEN / "photos8_0.npz")["bgr"][0])


def photo_crop() -> np.ndarray:
    return np.ascontiguousarray(photo()[PHOTO_CROP])


def transcode_blobs() -> list[bytes]:
    """The six input streams, read from the decoder's committed cases."""
    out = []
    for file, name, _, _ in TRANSCODES:
        if file == "jpeg_cases":
            out.append(np.load(GOLDEN / "jpeg_cases.npz")[f"blob/{name}"].tobytes())
        else:
            z = np.load(GOLDEN / "jpeg_orientation_cases.npz")
            k = list(z["names"]).index(name)
            out.append(z["blobs"][z["blob_at"][k]:z["blob_at"][k + 1]].tobytes())
    return out


@functools.lru_cache(maxsize=None)
def load():
    return np.load(GOLDEN / "jpeg_colour_encode_cases.npz")


def _file(z, k: int) -> bytes:
    return z["files"][int(z["file_at"][k]):int(z["file_at"][k + 1])].tobytes()


def groups(z):
    """(name, quality, subsampling, channel_order, images (3, h, w, 3), [file bytes] * 3) per launch group."""
    k = 0
    for name, (h, w), sub, q, order, kinds in group_list():
        yield name, q, sub, order, np.stack([z[f"image/{h}x{w}/{kind}"] for kind in kinds]), [_file(z, k + i) for i in range(3)]
        k += 3


def extra_files(z) -> tuple[bytes, list[bytes]]:
    """(the cropped photo's file, the six transcoded files): they follow the groups' files."""
    k = 3 * len(group_list())
    return _file(z, k), [_file(z, k + 1 + i) for i in range(len(TRANSCODES))]
