"""CPU: the colour JPEG encoder without a device.  ``jpeg.encode_colour`` (the numpy form, the checker of the kernels) against the
committed files Pillow wrote (tests/golden/jpeg_colour_encode_cases.npz) and against live Pillow, the two halves of the codec against
each other, the host C++ (second table set, 623-byte header, size bounds) under sanitizers in a stand-alone program, the C ABI's new
symbols, and the argument checks that must trip before an engine exists."""
from __future__ import annotations

import hashlib
import inspect
import io
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_colour_encode_cases as cases
from chessvision import ChessVision, hip_backend, jpeg

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "chessvision-3lc_amd" / "csrc"
N_GROUPS = 10 * 3 * 4 + 3


@pytest.fixture(scope="module")
def golden():
    return cases.load()


def test_numpy_form_equals_every_golden_file(golden):
    n, names = 0, []
    for name, q, sub, order, images, files in cases.groups(golden):
        names.append(name)
        for k, (a, want) in enumerate(zip(images, files)):
            assert jpeg.encode_colour(a, q, sub, order) == want, (name, k)
            n += 1
    assert n == 3 * N_GROUPS and len(set(names)) == N_GROUPS
    for h, w in cases.GEOMETRIES:                                 # no geometry, subsampling or quality went missing
        assert all(f"{h}x{w}-{sub}-q{q}" in names for sub in cases.SUBSAMPLINGS for q in cases.QUALITIES)
    assert sum(name.endswith("-rgb") for name in names) == 3
    crop_file, _ = cases.extra_files(golden)
    assert cases.photo_crop().shape == (96, 128, 3)
    assert jpeg.encode_colour(cases.photo_crop(), cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING) == crop_file


def test_numpy_form_equals_the_real_photo(golden):
    photo = cases.photo()
    assert photo.shape == (512, 512, 3) and photo.std() > 20                         # a picture, not a blank
    blob = jpeg.encode_colour(photo, cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING)
    assert len(blob) == int(golden["photo_length"])
    assert hashlib.sha256(blob).digest() == golden["photo_sha256"].tobytes()


def test_the_cases_hold_stuffing_chroma_zero_runs_and_dummies(golden):
    files = [f for *_, fs in cases.groups(golden) for f in fs]
    assert sum(f[623:-2].count(b"\xff\x00") for f in files) >= 100
    assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" and f[621:623] == b"\x3f\x00" for f in files)
    zrl = dummy = 0
    for name, q, sub, order, images, _ in cases.groups(golden):
        if name.split("-")[0] not in ("8x17", "17x33", "33x31"):
            continue
        for a in images:
            zz, comp, real = jpeg.encode_colour_coefficients(a, q, sub, order)
            pos = np.where(zz != 0, np.arange(64), -1)
            pos[:, 0] = 0
            prev = np.maximum.accumulate(pos, axis=1)
            b, k = np.nonzero(zz[:, 1:])
            zrl += int(np.any((k - prev[b, k] >= 16) & (comp[b] > 0)))
            d = np.nonzero(~real)[0]
            assert np.all(comp[d] == 0) and np.all(zz[d, 1:] == 0) and np.array_equal(zz[d, 0], zz[d - 1, 0])
            dummy += int(np.any(zz[d - 1, 0] != 0))
    assert zrl >= 1 and dummy >= 1


def test_numpy_form_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    sizes = [(1, 1), (2, 2), (2, 9), (5, 23), (8, 8), (8, 40), (16, 24), (24, 8), (31, 17), (40, 33)]
    n = 0
    for sub in cases.SUBSAMPLINGS:
        for k, (h, w) in enumerate(sizes):
            for q in ((-3, 1, 50, 100), (0, 10, 95, 400), (49, 51, 75, 101))[k % 3]:
                a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if q % 2 else cases.make_image("smooth", h, w, 0)
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, "JPEG", quality=min(100, max(1, q)), subsampling=sub)    # Pillow refuses what libjpeg clamps
                assert jpeg.encode_colour(a, q, sub, "rgb") == buf.getvalue(), (sub, h, w, q)
                assert jpeg.encode_colour(a[..., ::-1], q, sub, "bgr") == buf.getvalue(), (sub, h, w, q)
                n += 1
    assert n == 120


def test_decoder_reads_what_the_encoder_writes(golden):
    """The project's decoder reads every file the numpy form writes, and the coefficients it finds are the encoder's own real
    blocks (the decoder's planes are padded to whole MCUs: it sees the dummy blocks too, as the DC they carry and no AC)."""
    n = 0
    for name, q, sub, order, images, _ in cases.groups(golden):
        hs, vs = jpeg.SUBSAMPLINGS[sub]
        for a in images:
            blob = jpeg.encode_colour(a, q, sub, order)
            info = jpeg.jpeg_info(blob)
            assert info.supported and (info.height, info.width, info.components, info.luma_h, info.luma_v) == (*a.shape[:2], 3, hs, vs)
            coeffs, qtables, _ = jpeg.entropy_decode(blob, info)
            zz, comp, real = jpeg.encode_colour_coefficients(a, q, sub, order)
            (yr, yc), (cr, cc), _ = info.plane_blocks
            planes = np.split(coeffs.reshape(-1, 64), [yr * yc, yr * yc + cr * cc])
            per = hs * vs + 2
            mine = zz.reshape(cr, cc, per, 64)
            nat = np.zeros_like(mine)
            nat[..., jpeg.ZIGZAG] = mine                                       # the decoder hands out natural order
            luma = planes[0].reshape(cr, vs, cc, hs, 64).transpose(0, 2, 1, 3, 4).reshape(cr, cc, hs * vs, 64)
            mask = real.reshape(cr, cc, per)
            assert np.array_equal(luma[mask[..., :hs * vs]], nat[..., :hs * vs, :][mask[..., :hs * vs]]), name
            assert np.array_equal(luma, nat[..., :hs * vs, :]), name           # ... and the dummies as written
            assert np.array_equal(planes[1].reshape(cr, cc, 64), nat[..., per - 2, :]) and np.array_equal(planes[2].reshape(cr, cc, 64), nat[..., per - 1, :])
            assert np.array_equal(qtables[0], jpeg.encode_quant_table(q)) and np.array_equal(qtables[1], jpeg.encode_chroma_quant_table(q))
            n += 1
    assert n == 3 * N_GROUPS


def test_host_header_and_tables_equal_the_numpy_form():
    for h, w, q, sub in [(1, 1, 0, "4:2:0"), (7, 9, 1, "4:2:2"), (512, 512, 95, "4:2:0"), (4096, 4096, 100, "4:4:4"), (64, 64, 101, "4:2:2"),
                         (8, 16, 50, "4:4:4")]:
        header, qt = hip_backend.jpeg_colour_header(h, w, q, sub)
        assert header == jpeg.colour_header(w, h, q, sub) and len(header) == jpeg.COLOUR_HEADER_BYTES == 623
        assert np.array_equal(qt[0], jpeg.encode_quant_table(q)) and np.array_equal(qt[1], jpeg.encode_chroma_quant_table(q))
    luma, chroma = 20 + 63 * 26, 22 + 63 * 26
    assert hip_backend.jpeg_colour_max_bytes(8, 8, "4:4:4") == (623 + 2 * ((luma + 2 * chroma + 7) // 8) + 2 + 15) // 16 * 16
    assert hip_backend.jpeg_colour_max_bytes(8, 8, "4:2:0") == (623 + 2 * ((4 * luma + 2 * chroma + 7) // 8) + 2 + 15) // 16 * 16      # 3 dummies
    assert hip_backend.jpeg_colour_max_bytes(9, 17, "4:2:2") == (623 + 2 * ((2 * 2 * (2 * luma + 2 * chroma) + 7) // 8) + 2 + 15) // 16 * 16
    for bad in ((4097, 8, "4:2:0"), (8, 0, "4:2:0")):
        with pytest.raises(hip_backend.HipBackendError):
            hip_backend.jpeg_colour_max_bytes(*bad)
    with pytest.raises(ValueError):
        hip_backend.jpeg_colour_max_bytes(8, 8, "4:1:1")


def test_max_bytes_holds_every_golden_file_and_an_adversarial_one(golden):
    for name, q, sub, order, images, files in cases.groups(golden):
        cap = hip_backend.jpeg_colour_max_bytes(*images.shape[1:3], sub)
        assert all(len(f) <= cap for f in files), name
    rng = np.random.default_rng(11)
    for sub in cases.SUBSAMPLINGS:
        worst = 0
        for _ in range(4):
            a = (rng.integers(0, 2, (16, 16, 3)) * 255).astype(np.uint8)              # 0/255 noise at quality 100
            worst = max(worst, len(jpeg.encode_colour(a, 100, sub)))
        assert 623 < worst <= hip_backend.jpeg_colour_max_bytes(16, 16, sub), sub


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "chessvision_hip.h").read_text()
    lib = hip_backend.load_library()
    declared = {name for name, _, _ in hip_backend.SYMBOLS}
    for name in ("cv_jpeg_encode_colour_u8", "cv_jpeg_colour_header", "cv_jpeg_colour_max_bytes"):
        assert re.search(rf"\bint {name}\(", header) and name in declared and getattr(lib, name)
    assert "#define CV_JPEG_COLOUR_HEADER_BYTES 623" in header
    assert lib.cv_abi_version() == hip_backend.ABI_VERSION == 6
    for fn, names in ((ChessVision.encode_colour, ["self", "images", "quality", "subsampling", "channel_order"]),
                      (ChessVision.transcode_jpegs, ["self", "blobs", "quality", "subsampling", "orientation"]),
                      (jpeg.encode_colour, ["image", "quality", "subsampling", "channel_order"])):
        p = inspect.signature(fn).parameters
        assert list(p) == names and p["quality"].default == 95 and p["subsampling"].default == "4:2:0"
    assert inspect.signature(ChessVision.encode_colour).parameters["channel_order"].default == "bgr"
    assert inspect.signature(ChessVision.transcode_jpegs).parameters["orientation"].default == "ignore"


def test_bad_arguments_raise_before_any_engine_exists():
    cv = ChessVision()
    good = np.zeros((8, 8, 3), np.uint8)
    for bad in (np.zeros((0, 8, 3), np.uint8), np.zeros((8, 0, 3), np.uint8), np.zeros((4097, 1, 3), np.uint8), np.zeros((1, 4097, 3), np.uint8),
                np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.int8), np.zeros((8, 8, 2), np.uint8), np.zeros((8, 8), np.uint8)):
        with pytest.raises(ValueError):
            cv.encode_colour([good, bad])
        with pytest.raises(ValueError):
            jpeg.encode_colour(bad)
    for kw in ({"subsampling": "4:1:1"}, {"subsampling": 2}, {"channel_order": "gray"}, {"channel_order": "rbg"}):
        with pytest.raises(ValueError):
            cv.encode_colour([good], **kw)
        with pytest.raises(ValueError):
            jpeg.encode_colour(good, **kw)
    blob = jpeg.encode_colour(good)
    with pytest.raises(ValueError):
        cv.transcode_jpegs([blob], subsampling="4:1:1")
    with pytest.raises(ValueError):
        cv.transcode_jpegs([blob], orientation="auto")
    with pytest.raises(jpeg.UnsupportedJpeg):
        cv.transcode_jpegs([blob, blob[:300]])
    tall = bytearray(jpeg.encode_colour(good))
    at = tall.index(b"\xff\xc0") + 5
    tall[at:at + 2] = (4097).to_bytes(2, "big")                    # a header that promises 4097 rows: refused by size before any decode
    with pytest.raises(ValueError, match="4096"):
        cv.transcode_jpegs([blob, bytes(tall)])
    assert cv.encode_colour([]) == [] and cv.transcode_jpegs([]) == []
    assert cv._engines == {}


def test_host_tables_under_sanitizers_equal_the_numpy_form(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    exe = tmp_path / "jpeg_enc_colour_host"
    out = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                          "-static-libasan", "-static-libubsan", "-pthread", f"-I{CSRC}", str(ROOT / "tests" / "jpeg_enc_colour_host" / "main.cpp"),
                          str(CSRC / "jpeg.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0 and ("libasan" in out.stderr or "libubsan" in out.stderr):
        pytest.skip("g++ has no sanitizer runtime on this machine")
    assert out.returncode == 0, out.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "records.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "jpeg enc colour host: ok records: 1224" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    raw = (tmp_path / "records.bin").read_bytes()
    size = 20 + 623 + 256 + 96 + 2048
    assert len(raw) == 1224 * size
    codes = [(jpeg._huffman_codes(jpeg.DC_BITS, jpeg.DC_VALS), jpeg._huffman_codes(jpeg.AC_BITS, jpeg.AC_VALS)),
             (jpeg._huffman_codes(jpeg.DC1_BITS, jpeg.DC1_VALS), jpeg._huffman_codes(jpeg.AC1_BITS, jpeg.AC1_VALS))]
    names = {(2, 2): "4:2:0", (2, 1): "4:2:2", (1, 1): "4:4:4"}
    seen = set()
    for k in range(1224):
        rec = raw[k * size:(k + 1) * size]
        w, h, q, hs, vs = struct.unpack("<5i", rec[:20])
        seen.add((w, q, hs, vs))
        assert rec[20:643] == jpeg.colour_header(w, h, q, names[(hs, vs)]), (w, h, q, hs, vs)
        div = np.frombuffer(rec[643:899], "<u2").reshape(2, 64)
        assert np.array_equal(div[0], (jpeg.encode_quant_table(q) << 3)[jpeg.ZIGZAG])
        assert np.array_equal(div[1], (jpeg.encode_chroma_quant_table(q) << 3)[jpeg.ZIGZAG])
        dcs, acs = np.frombuffer(rec[899:995], "<u4").reshape(2, 12), np.frombuffer(rec[995:], "<u4").reshape(2, 256)
        for s, (dc, ac) in enumerate(codes):
            assert [(int(v) >> 8, int(v) & 255) for v in dcs[s]] == [dc[c] for c in range(12)]
            assert all(((int(acs[s][c]) >> 8, int(acs[s][c]) & 255) == ac[c]) if c in ac else acs[s][c] == 0 for c in range(256))
    assert seen == {(w, q, hs, vs) for w in (1, 7, 8, 4096) for q in range(102) for hs, vs in names}
