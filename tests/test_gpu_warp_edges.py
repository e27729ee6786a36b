"""GPU: the board warp (``extract_squares_u8_kernel``, and ``extract_squares_u8_float_kernel`` under CV_WARP=float) at its edges -- the
cases of tests/byte_edge_cases.py: concave, self-crossing, collinear, degenerate and sub-pixel quadrangles, quadrangles on and beyond
the frame, photos one and two pixels wide or tall, photos beyond the int16 range of OpenCV's map.  Byte equality with the host
restatement AND the independent oracle on every case, through every route into the kernel; no tolerance.

All cases of one photo shape travel in ONE call (N photos, N matrices), so the per-image matrix and image offsets are part of it."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import byte_edge_cases as bec
from chessvision import ChessVision, hip_backend, synthetic, utils

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _run_groups(eng, want_boards=True):
    """{case id: (squares (64,64,64), board (512,512) | None)} through ``HipEngine.extract_squares_u8`` (the ``_dev`` entry), one call
    per photo shape."""
    out = {}
    for ids in bec.warp_groups().values():
        photos = np.stack([bec.warp_case(k)[0] for k in ids])
        inv = hip_backend.board_homographies(np.stack([bec.warp_case(k)[1] for k in ids]), bec.BOARD)
        squares, boards = eng.extract_squares_u8(torch.from_numpy(photos), inv, want_boards=want_boards)
        squares = squares.cpu().numpy().reshape(len(ids), 64, 64, 64)
        boards = boards.cpu().numpy() if want_boards else [None] * len(ids)
        for i, k in enumerate(ids):
            out[k] = (squares[i], boards[i])
    return out


@pytest.fixture(scope="module")
def device(engines):
    return _run_groups(engines["f32"])


@pytest.mark.parametrize("case_id", bec.WARP_IDS)
def test_board_and_squares_equal_host_chain_and_oracle(device, case_id):
    squares, board = device[case_id]
    host = bec.gray_flip_host(bec.host_board_bgr(case_id))
    assert np.array_equal(board, host), (int(np.abs(board.astype(int) - host.astype(int)).max()), float((board != host).mean()))
    assert np.array_equal(board, bec.gray_flip_oracle(bec.oracle_board_bgr(case_id)))
    assert np.array_equal(squares, ChessVision.extract_squares(board)[..., 0])


def test_squares_without_boards_equal_those_with_boards(engines, device):
    alone = _run_groups(engines["f32"], want_boards=False)
    for case_id in bec.WARP_IDS:
        assert alone[case_id][1] is None
        assert np.array_equal(alone[case_id][0], device[case_id][0]), case_id


@pytest.mark.parametrize("case_id", bec.ROUTE_IDS)
def test_host_matrix_entry_gives_the_same_bytes(engines, device, case_id):
    """``cv_extract_squares_u8``: the matrices in HOST memory, staged by the library."""
    eng, lib = engines["f32"], hip_backend.load_library()
    photo, quad = bec.warp_case(case_id)
    h, w, _ = photo.shape
    inv = np.ascontiguousarray(hip_backend.board_homographies(quad[None], bec.BOARD), dtype=np.float64).reshape(9)
    image = torch.from_numpy(photo[None]).to(eng.device)
    squares = torch.empty((64, 64, 64), dtype=torch.uint8, device=eng.device)
    boards = torch.empty((1, 512, 512), dtype=torch.uint8, device=eng.device)
    stream = int(torch.cuda.current_stream(eng.device).cuda_stream)
    status = lib.cv_extract_squares_u8(eng._h, image.data_ptr(), 1, h, w, inv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       squares.data_ptr(), boards.data_ptr(), stream)
    assert status == 0, lib.cv_last_error()
    assert np.array_equal(boards[0].cpu().numpy(), device[case_id][1])
    assert np.array_equal(squares.cpu().numpy(), device[case_id][0])


@pytest.fixture(scope="module")
def cv_f32(tmp_path_factory):
    pe, pc = synthetic.save_checkpoints(tmp_path_factory.mktemp("weights_warp_edges"))
    return ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f32")


@pytest.mark.parametrize("case_id", ["convex", "9x2"])
def test_matrix_as_kernel_argument_through_process_image(cv_f32, case_id):
    """``cv_process_image``: one board whose matrix rides in the kernel arguments.  A 37 x 53 and a 9 x 2 photo (the resize in front
    enlarges them); the quadrangle is whatever the call reports -- with ``fallback_quad`` the whole mask scaled by h / 256 on both
    axes, as in the reference -- and board and squares equal the host chain on that quadrangle."""
    photo = bec.warp_case(case_id)[0]
    res = hip_backend.process_image_native(cv_f32.board_extractor.engine, cv_f32.classifier.engine, photo, fallback_quad=True)
    assert res["found"]
    quad = res["quadrangle"]
    assert quad.shape == (4, 1, 2) and quad.dtype == np.float32
    board = bec.gray_flip_host(utils.extract_perspective(photo, quad.reshape(4, 2), bec.BOARD))
    assert np.array_equal(res["board"], board)
    assert np.array_equal(res["board"], bec.gray_flip_oracle(bec.cref.extract_board(photo, quad.reshape(4, 2), bec.BOARD)))
    assert np.array_equal(res["squares"], ChessVision.extract_squares(board))


FLOAT_SCRIPT = r"""
import sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/chessvision-3lc_amd"); sys.path.insert(0, "ROOT/tests")
import numpy as np, torch
import byte_edge_cases as bec
from chessvision import classical
from chessvision.hip_backend import HipEngine, board_homographies

assert classical.warp_mode() == "float"
eng = HipEngine(precision="f32", unet_chunk=2, resnet_chunk=128)
for ids in bec.warp_groups().values():
    photos = np.stack([bec.warp_case(k)[0] for k in ids])
    inv = board_homographies(np.stack([bec.warp_case(k)[1] for k in ids]), bec.BOARD)
    squares, boards = eng.extract_squares_u8(torch.from_numpy(photos), inv)
    boards = boards.cpu().numpy()
    for i, k in enumerate(ids):
        assert np.array_equal(boards[i], bec.gray_flip_host(bec.host_board_float_bgr(k))), k          # device == host, whole board
        for rows, band in bec.oracle_bands_float_bgr(k):
            assert np.array_equal(boards[i][rows.start:rows.stop], bec.gray_flip_oracle(band)), (k, rows)   # == scalar oracle
eng.close()
print("WARP_EDGES_FLOAT_OK")
"""


def test_float_reading_device_equals_host_and_oracle_on_every_case():
    """CV_WARP=float in a child process (the library reads it once per process): every case of the table."""
    env = dict(os.environ)
    env["CV_WARP"] = "float"
    out = subprocess.run([sys.executable, "-c", FLOAT_SCRIPT.replace("ROOT", str(ROOT))], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "WARP_EDGES_FLOAT_OK" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
