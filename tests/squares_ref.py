"""Shared by tests/test_evaluate_squares_cpu.py and tests/test_gpu_evaluate_squares.py: the derived bound, the crafted rows, torch in
float64 as the reference of the per-square records, the reference's ``validate()`` restated, the fixture and the oracle's view of it.
Shares no code with ``chessvision/evaluation.py``."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

FIXTURE = Path(__file__).resolve().parent / "golden" / "squares_val.npz"


def bound(x) -> float:
    """loss / confidence / max_logit / logsumexp against float64: one ulp each for expf, logf, two subtractions and 13 additions, at
    magnitudes bounded by max|x| + log 13 -- 2^-21 (1 + max|x|)."""
    return 2.0 ** -21 * (1.0 + float(np.nanmax(np.abs(x))))


def crafted_rows():
    """(logits (R,13) float32, labels (R,) int) -- the rows the issue names."""
    rows, labels = [], []
    rows.append(np.full(13, 0.75, np.float32)); labels.append(4)                       # all 13 equal: rank = 12 - t, predicted 0
    r = np.linspace(-1, 1, 13).astype(np.float32); r[3] = r[9] = 2.5; rows.append(r); labels.append(3)       # tie at the top, true class first
    rows.append(r.copy()); labels.append(9)                                            # ... true class last of the tie
    rows.append(r.copy()); labels.append(0)                                            # ... tie not involving the true class
    r = np.linspace(1, -1, 13).astype(np.float32); r[5] = r[6] = -0.25; rows.append(r); labels.append(6)     # tie below the top
    r = np.linspace(-2, 2, 13).astype(np.float32); r[7] = np.nan; rows.append(r); labels.append(2)           # a NaN row
    r = np.linspace(-2, 2, 13).astype(np.float32); r[0] = np.nan; rows.append(r); labels.append(-1)          # NaN first, unlabelled
    rows.append(np.linspace(-3, 3, 13).astype(np.float32)); labels.append(-1)          # label -1
    r = np.zeros(13, np.float32); r[11] = 80.0; rows.append(r); labels.append(0)       # spread 80: exp underflows to 0, loss 80
    rows.append(r.copy()); labels.append(11)
    return np.stack(rows), np.asarray(labels, np.int64)


def torch_reference(x, t):
    """float64 torch: log_softmax, stable argsort.  NaN rows and unlabelled rows are returned as NaN / the documented codes."""
    xt = torch.from_numpy(np.asarray(x, np.float32)).double()
    n = xt.shape[0]
    ls = torch.log_softmax(xt, dim=1)
    order = torch.argsort(xt, dim=1, stable=True)              # ascending; among equals the higher index is nearer the top
    nan = torch.isnan(xt).any(dim=1).numpy()
    loss, rank = np.full(n, np.nan), np.full(n, -1, np.int64)
    for i in range(n):
        if t[i] < 0:
            continue
        rank[i] = 13 if nan[i] else 12 - int((order[i] == int(t[i])).nonzero()[0, 0])
        if not nan[i]:
            loss[i] = -float(ls[i, int(t[i])])
    conf = torch.softmax(xt, dim=1).max(dim=1).values.numpy()
    return {"loss": loss, "rank": rank, "confidence": np.where(nan, np.nan, conf), "nan": nan,
            "max_logit": np.where(nan, np.nan, xt.max(dim=1).values.numpy()),
            "logsumexp": np.where(nan, np.nan, torch.logsumexp(xt, dim=1).numpy()),
            "predicted": torch.argmax(xt, dim=1).numpy()}


def check_against_torch(scores, x, t, what):
    ref = torch_reference(x, t)
    clean = ~ref["nan"]
    assert np.array_equal(scores.rank, ref["rank"]), what
    assert np.array_equal(scores.label, t), what
    assert np.array_equal(scores.flags & 1, ref["nan"].astype(np.int32)), what
    assert np.array_equal(scores.predicted[clean], ref["predicted"][clean]), what       # torch.argmax: the first maximum
    b = bound(x[clean])
    worst = {}
    for k in ("loss", "confidence", "max_logit", "logsumexp"):
        got = np.asarray(getattr(scores, k), np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(ref[k])), (what, k)
        ok = ~np.isnan(ref[k])
        worst[k] = float(np.abs(got[ok] - ref[k][ok]).max()) if ok.any() else 0.0
    print(f"square_records {what}: worst {worst} bound {b:.3e}")
    assert all(v <= b for v in worst.values()), (what, worst, b)
    return worst


def validate_restated(loss, predicted, label, nan_row, batch_size):
    """validate() of train_classifier.py:90-111 over rows already scored: running_loss += mean loss of the batch's labelled rows,
    val_loss = running_loss / batches, accuracy = 100 * correct / total.  Unlabelled rows are not part of the table."""
    n = len(loss)
    bs = batch_size if batch_size > 0 else n
    running, batches, correct, total = 0.0, 0, 0, 0
    for lo in range(0, n, bs):
        keep = label[lo:lo + bs] >= 0
        if not keep.any():
            continue
        running += float(np.mean(loss[lo:lo + bs][keep].astype(np.float64)))
        batches += 1
        total += int(keep.sum())
        correct += int((keep & (predicted[lo:lo + bs] == label[lo:lo + bs]) & ~nan_row[lo:lo + bs]).sum())
    return running / batches, 100.0 * correct / total, total, correct, batches



def fixture():
    """(squares (130,64,64) uint8, labels (130,) int8) of tests/golden/squares_val.npz."""
    with np.load(FIXTURE) as z:
        return z["squares"].copy(), z["labels"].copy()


def to_tensor_normalize(u8, mean, std):
    """torchvision's ToTensor + Normalize([mean], [std]) on (N,64,64) uint8, on the CPU: (N,1,64,64) float32."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).float().div(255)
    if mean is not None:
        x = x.sub(mean).div(std)
    return x[:, None].contiguous()
