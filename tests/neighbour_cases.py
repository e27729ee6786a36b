"""Data kinds, shapes and the host emulation of the filter that tests/test_neighbours_cpu.py and tests/test_gpu_neighbours.py share.

The emulation restates the device filter in numpy: channel means of the finite corpus rows (float64 sum, rounded to float32), float32
centred rows, float32 squared norms, the float32 GEMM form ``(|a|^2 + |b|^2) - 2 a.b``, the ``k + SLACK`` smallest ``(approximate, j)``
per row, ``T`` = the smallest approximate distance not kept, and the certificate ``D_k < T - E`` with
``E = 2^-24 (2 C + 12) (|a~|^2 + max_j |b~_j|^2) + (4 C + 8) 2^-149`` (DESIGN.md section 4 "Embedding neighbours").  numpy's float32
matmul adds in another order than the MFMA chain does; the bound holds for every order, so the emulation may certify a row the
device does not only where ``D_k`` sits within rounding of ``T - E``: ``emulate`` reports the smallest margin so that the GPU cases
can be chosen away from it."""
from __future__ import annotations

import dataclasses

import numpy as np

SLACK = 16                    # csrc/neighbours.h: kNeighbourSlack
TILE = 64                     # kNeighbourTile: query rows and corpus rows of one MFMA tile
K_STEP = 32                   # kNeighbourKStep
EXACT_BATCH = 256             # corpus rows the exact kernel scores per pass


def brute_sq_distances(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """D for every pair, channel by channel in ascending order, float64 -- written without a look at chessvision.embeddings."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    d = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for ch in range(a.shape[1]):
        t = a64[:, ch][:, None] - b64[:, ch][None, :]
        d = d + t * t
    return d


def brute_neighbours(a, b, k, exclude_self):
    """(indices, sq_distances) by a python sort of (D, j) tuples per row: the order the issue defines, spelled out."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = brute_sq_distances(a, b)
    q_bad, b_bad = ~np.isfinite(a).all(1), ~np.isfinite(b).all(1)
    idx = np.full((a.shape[0], k), -1, np.int32)
    dist = np.full((a.shape[0], k), np.inf, np.float64)
    for i in range(a.shape[0]):
        if q_bad[i]:
            dist[i] = np.nan
            continue
        pairs = sorted((float(d[i, j]), j) for j in range(b.shape[0]) if not b_bad[j] and not (exclude_self and j == i))[:k]
        for t, (dv, j) in enumerate(pairs):
            idx[i, t], dist[i, t] = j, dv
    return idx, dist


# ---- data kinds ------------------------------------------------------------------------------------------------------------------------
def relu_normal(rng, n, c):
    return np.maximum(rng.standard_normal((n, c)), 0.0).astype(np.float32)


def clustered(rng, n, c, clusters, spread):
    centres = np.maximum(rng.standard_normal((clusters, c)), 0.0)
    return (centres[rng.integers(0, clusters, n)] + spread * rng.standard_normal((n, c))).astype(np.float32)


def make(kind: str, n: int, c: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "a":                                          # iid post-ReLU normal
        return relu_normal(rng, n, c)
    if kind == "b":                                          # far from the origin: the reason the filter centres
        return (10.0 + 1e-3 * rng.standard_normal((n, c))).astype(np.float32)
    if kind == "c":                                          # 13 clusters of spread 0.15 around post-ReLU centres
        return clustered(rng, n, c, 13, 0.15)
    if kind == "d":                                          # integers: ties everywhere, float32 arithmetic exact
        return rng.integers(0, 3, (n, c)).astype(np.float32)
    if kind == "e":                                          # 100 exact copies of one row: more ties than SLACK
        x = relu_normal(rng, n, c)
        x[rng.permutation(n)[:100]] = x[0]
        return x
    if kind == "f":                                          # two tight clusters: neighbours closer together than the bound can tell apart
        return clustered(rng, n, c, 2, 0.02)
    if kind == "g":                                          # two rows whose squares overflow float32
        x = relu_normal(rng, n, c)
        x[[1, n - 2]] *= np.float32(1e25)
        return x
    if kind == "h":                                          # NaN / +inf / -inf rows
        x = relu_normal(rng, n, c)
        x[0, 0] = np.nan
        x[n // 2, c // 2] = np.inf
        x[n - 1, c - 1] = -np.inf
        return x
    raise ValueError(kind)


@dataclasses.dataclass(frozen=True)
class Case:
    kind: str
    q: int                    # 0: the table against itself (exclude_self)
    n: int
    c: int
    k: int
    seed: int = 0

    @property
    def id(self) -> str:
        return f"{self.kind}-q{self.q or 'self'}-n{self.n}-c{self.c}-k{self.k}"

    def tables(self):
        corpus = make(self.kind, self.n, self.c, self.seed)
        if not self.q:
            return corpus, corpus, True
        kind = "a" if self.kind in ("e", "g") else self.kind
        return make(kind, self.q, self.c, self.seed + 1000), corpus, False


_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
_CHANNELS = (1, 3, 4, 5, 31, 32, 33, 512, 1024)
_KS = (1, 2, 10, 64)
# every size as a self graph and as the corpus of a 3-row query table, channels and k cycling so that each appears with small and large n
CASES = [Case("a", 0, n, _CHANNELS[i % 9], _KS[i % 4]) for i, n in enumerate(_SIZES)]
CASES += [Case("a", 3, n, _CHANNELS[(i + 4) % 9], _KS[(i + 2) % 4]) for i, n in enumerate(_SIZES)]
CASES += [Case("a", q, 3, _CHANNELS[(i + 7) % 9], _KS[(i + 1) % 4]) for i, q in enumerate(_SIZES)]
CASES += [
    Case("a", 3, 257, 512, 10), Case("a", 257, 3, 33, 10),                      # q != n both ways
    Case("a", 0, 257, 1024, 64), Case("a", 0, 257, 31, 48), Case("a", 0, 257, 33, 49),   # k + SLACK at the 64-lane edge of a list
    Case("a", 0, EXACT_BATCH - 1, 5, 10), Case("a", 0, EXACT_BATCH, 5, 10), Case("a", 65, EXACT_BATCH + 1, 4, 2),
    Case("a", 1025, 7745, 5, 10),                                              # 17 query tiles, 122 corpus tiles: 31 splits of 4, the last one of 2
    Case("a", 32705, 129, 3, 2),                                               # 512 query tiles: no split at all, one workgroup walks all 3 corpus tiles
    Case("d", 0, 257, 4, 10), Case("d", 0, 64, 4, 64), Case("d", 65, 129, 4, 2),
    Case("h", 0, 129, 33, 10), Case("h", 65, 257, 5, 2), Case("h", 0, 5, 3, 10),
]
CERTIFIED_CASES = [Case(kind, 0, 257, c, 10) for kind in "abc" for c in (512, 1024)] + \
                  [Case(kind, 129, 257, 512, 10) for kind in "abc"]
EXACT_PATH_CASES = [Case("e", 0, 257, 512, 10), Case("f", 0, 257, 1024, 10), Case("g", 0, 257, 512, 10), Case("g", 17, 129, 33, 2)]


# ---- the filter, emulated --------------------------------------------------------------------------------------------------------------
def error_bound(c: int, na: np.ndarray, nb_max: float) -> np.ndarray:
    return np.ldexp((2.0 * c + 12.0) * (na.astype(np.float64) + float(nb_max)), -24) + np.ldexp(4.0 * c + 8.0, -149)


def emulate(queries: np.ndarray, corpus: np.ndarray, k: int, exclude_self: bool, centre: bool = True) -> dict:
    """-> certified (Q,) bool, margin (Q,) = (T - E - D_k) / E where T is finite (+inf elsewhere), ratio = max |approximate - D| / E,
    lost = true top-k neighbours missing from the candidates."""
    q, n, c = queries.shape[0], corpus.shape[0], corpus.shape[1]
    b_ok = np.isfinite(corpus).all(1)
    q_ok = np.isfinite(queries).all(1)
    mean = np.zeros(c, np.float32)
    if centre and b_ok.any():
        mean = (corpus[b_ok].astype(np.float64).sum(0) / b_ok.sum()).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.where(q_ok[:, None], queries - mean, np.float32(0)).astype(np.float32)
        b = np.where(b_ok[:, None], corpus - mean, np.float32(0)).astype(np.float32)
        na, nb = (a * a).sum(1, dtype=np.float32), (b * b).sum(1, dtype=np.float32)
        approx = ((na[:, None] + nb[None, :]) - np.float32(2) * (a @ b.T)).astype(np.float32)
        exact = brute_sq_distances(np.where(q_ok[:, None], queries, 0), np.where(b_ok[:, None], corpus, 0))
    eligible = np.broadcast_to(b_ok[None, :], (q, n)).copy()
    if exclude_self:
        eligible[np.arange(q), np.arange(q)] = False
    nb_max = nb[b_ok].max() if b_ok.any() else np.float32(0)
    e = error_bound(c, na, nb_max)
    with np.errstate(invalid="ignore"):
        bad = (~np.isfinite(approx) & eligible).any(1) | ~np.isfinite(na) | ~np.isfinite(nb_max)
    key = np.where(eligible & np.isfinite(approx), approx, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    kp = k + SLACK
    certified, margin, lost = np.zeros(q, bool), np.full(q, np.inf), 0
    for i in range(q):
        if not q_ok[i]:
            continue
        count = int(np.isfinite(key[i]).sum())
        cand = order[i, :min(kp, count)]
        t = key[i, order[i, kp]] if count > kp else np.inf
        truth = sorted((exact[i, j], j) for j in range(n) if eligible[i, j])[:k]
        lost += sum(1 for _, j in truth if j not in set(cand.tolist()))
        if bad[i]:
            continue
        if not np.isfinite(t):
            certified[i] = True
            continue
        dk = np.sort(exact[i, cand])[k - 1]
        certified[i] = dk < float(t) - e[i]
        margin[i] = (float(t) - e[i] - dk) / e[i] if e[i] > 0 else np.inf
    with np.errstate(invalid="ignore"):
        err = np.where(eligible & np.isfinite(approx) & q_ok[:, None], np.abs(approx.astype(np.float64) - exact), 0.0)
        ratio = float((err.max(1) / np.maximum(e, 1e-300))[~bad & q_ok].max()) if (~bad & q_ok).any() else 0.0
    return {"certified": certified, "margin": margin, "ratio": ratio, "lost": lost, "finite_queries": q_ok}
