"""Oracle of the ground-truth scores: float64 numpy restatements of the segmentation scores from a logits array and a label mask, and
plain-Python loops for FEN labels, ranks, top-k and position accuracy.  Shares no code with ``chessvision/evaluation.py``."""
from __future__ import annotations

import math

import numpy as np

SYMBOLS = "BKNPQRbknpqrf"
EPS = 1e-6


# ---- segmentation ------------------------------------------------------------------------------------------------------------------
def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def seg_sums(logits, mask, threshold=0.5):
    """The record's fields in float64: counts and the three sums.  NaN logits: counted, excluded from the prediction, and every sum
    becomes NaN."""
    x = np.asarray(logits, dtype=np.float64).reshape(-1)
    t = np.asarray(mask).reshape(-1) != 0
    v = sigmoid64(x)
    with np.errstate(invalid="ignore"):
        pred = v > threshold
    terms = np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))
    has_nan = bool(np.isnan(x).any())
    return {
        "n_label": int(t.sum()), "n_pred": int(pred.sum()), "n_both": int((pred & t).sum()), "n_nan": int(np.isnan(x).sum()),
        "bce_sum": math.nan if has_nan else float(np.sum(terms)),
        "sig_sum": math.nan if has_nan else float(np.sum(v)),
        "sig_label_sum": math.nan if has_nan else float(np.sum(v[t])),
        "count": int(x.size),
    }


def dice(inter, sets_sum):
    if sets_sum == 0:
        sets_sum = 2 * inter
    return (2 * inter + EPS) / (sets_sum + EPS)


def seg_finish(r):
    """Record fields -> the six scores (upstream Pytorch-UNet's dice_coeff per image: epsilon 1e-6, sets_sum == 0 -> 2 * inter)."""
    count, n_label, n_pred, n_both = r["count"], r["n_label"], r["n_pred"], r["n_both"]
    bce = r["bce_sum"] / count
    dice_loss = 1.0 - dice(r["sig_label_sum"], r["sig_sum"] + n_label)
    union = n_pred + n_label - n_both
    return {"bce": bce, "dice_loss": dice_loss, "loss": dice_loss + bce, "dice": dice(n_both, n_pred + n_label),
            "iou": 1.0 if union == 0 else n_both / union, "pixel_accuracy": (count - n_pred - n_label + 2 * n_both) / count}


def seg_scores(logits, mask, threshold=0.5):
    return seg_finish(seg_sums(logits, mask, threshold))


# ---- positions ---------------------------------------------------------------------------------------------------------------------
def fen_symbols(fen):
    """64 symbols, a8..h1, "f" for empty; ValueError for a malformed placement."""
    out = []
    ranks = fen.split(" ")[0].split("/")
    if len(ranks) != 8:
        raise ValueError("ranks")
    for rank in ranks:
        n = 0
        for ch in rank:
            if ch.isdigit() and 1 <= int(ch) <= 8:
                out += ["f"] * int(ch)
                n += int(ch)
            elif ch in SYMBOLS[:12]:
                out.append(ch)
                n += 1
            else:
                raise ValueError("symbol")
        if n != 8:
            raise ValueError("rank sum")
    return out


def fen_indices(fen):
    return [SYMBOLS.index(s) for s in fen_symbols(fen)]


def rank_of_true(row, t):
    """#{j: p_j > p_t} + #{j > t: p_j == p_t}; 13 when the row holds a NaN."""
    if any(math.isnan(float(v)) for v in row):
        return 13
    r = 0
    for j in range(13):
        if row[j] > row[t] or (j > t and row[j] == row[t]):
            r += 1
    return r


def rank_by_stable_argsort(row, t):
    """The place of t from the top of np.argsort(kind="stable") (rows without NaN)."""
    order = list(np.argsort(np.asarray(row), kind="stable"))
    return 12 - order.index(t)


def argmax_first(row):
    best = 0
    for k in range(1, 13):
        if row[k] > row[best]:
            best = k
    return best


def board_scores(probs, labels):
    """(64,13) probabilities, 64 true class indices per row -> dict of per-square lists and the board's hits[13], mean loss, n_nan."""
    ranks, preds, conf, loss = [], [], [], []
    n_nan = 0
    for i in range(64):
        row = [np.float32(v) for v in probs[i]]
        t = int(labels[i])
        nan = any(math.isnan(float(v)) for v in row)
        n_nan += nan
        ranks.append(rank_of_true(row, t))
        preds.append(argmax_first(row))
        conf.append(math.nan if nan else float(max(row)))
        p = float(row[t])
        loss.append(math.nan if math.isnan(p) else (math.inf if p == 0.0 else -math.log(p)))
    hits = [sum(1 for r in ranks if r < k) for k in range(1, 14)]
    return {"rank": ranks, "predicted": preds, "confidence": conf, "loss": loss, "hits": hits, "mean_loss": sum(loss) / 64.0,
            "n_nan": n_nan}


def position_accuracy(predicted_fen, true_fen):
    a, b = fen_symbols(predicted_fen), fen_symbols(true_fen)
    return sum(1 for x, y in zip(a, b) if x == y) / 64
