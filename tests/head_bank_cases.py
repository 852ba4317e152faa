"""Case table of the head-bank tests (tests/test_head_bank_host.py, tests/test_head_bank_gpu.py): the kernel's rows-per-tile, the
tolerances with their derivations, and seeded banks and embeddings whose logits stay within +-16.  numpy only."""
import numpy as np

import head_bank_ref as ref

T = 16                              # KWS_HEADS_TILE_ROWS, include/kws.h: consecutive rows one block handles (the host test holds it to the header)
ROW_COUNTS = (1, T - 1, T, T + 1, 4 * T + 1)
EMBED_SIZES = (4, 48, 128)          # the smallest, the recurrent models', the CNNs'
MAX_CLASSES = {4: 256, 48: 128, 128: 64}          # kws_head_fit_max_classes(E); the host test holds the table to the library
LOGIT_LIMIT = 16.0

# Probabilities against the float64 softmax of the RETURNED float32 logits, |logit| <= 16.  l - m rounds once (u) on a value of
# at most 32, which the exponential turns into a relative error of at most 32 u; expf is within 1 ulp (2 u); the sum over C terms
# rounds C - 1 times; one division (u).  Up to C = 100 the worst case of all of them is below 140 u < 256 u, and p <= 1, so the
# absolute error is below 256 u = 2^-16.  At C = 256 the additions alone could reach 255 u if every rounding fell the same way,
# which no data does (they grow like sqrt(C) u); the bound is kept at 2^-16 for every class count.
PROB_ATOL = 2.0 ** -16
# score_heads' mean loss against the float64 reference: -log of a float32 probability carries the relative error of p (< 256 u = 1.6e-5
# in the worst case above, in practice a few u) as an ABSOLUTE error of the log, against losses of order 1: relative 1e-5.
LOSS_RTOL = 1e-5


def logit_cases():
    """(E, class counts of the bank's heads): every E with C_h in {2, 3, 64, the maximum} as two-head banks of one class count (rows
    that alternate between the two never form a run, rows in blocks of T do), and banks mixing class counts"""
    out = []
    for E in EMBED_SIZES:
        for C in sorted({2, 3, min(64, MAX_CLASSES[E]), MAX_CLASSES[E]}):
            out.append((E, (C, C)))
    out += [(4, (2, 3, 64, 256)), (48, (2, 3, 64, 128)), (128, (2, 3, 12, 64)), (128, (3, 5, 12)), (48, (7, 31, 32, 33))]
    return out


def case_id(case):
    return "E%d-%s" % (case[0], "_".join(str(c) for c in case[1]))


def make_case(E, classes, N, seed):
    """-> (emb (N, E) float32, [(kernel, bias)] float32) with every reference logit within +-LOGIT_LIMIT (checked here)"""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((N, E)).astype(np.float32)
    heads = []
    for C in classes:
        k = rng.uniform(-1.0, 1.0, (E, C)).astype(np.float32)
        b = rng.uniform(-1.0, 1.0, (C,)).astype(np.float32)
        top = float(np.abs(ref.logits(emb, (k, b))).max())
        if top > 12.0:                                            # a power of two: the scaled weights are still the float32 drawn
            s = 2.0 ** np.floor(np.log2(12.0 / top))
            k, b = (k * s).astype(np.float32), (b * s).astype(np.float32)
        assert float(np.abs(ref.logits(emb, (k, b))).max()) <= LOGIT_LIMIT
        heads.append((k, b))
    return emb, heads


def cyclic_ids(R, H):
    """neighbouring rows never share a head (H >= 2): no tile is a run"""
    return (np.arange(R) % H).astype(np.int32)


def block_ids(R, H):
    """tiles of T rows of one head: every full tile is a run"""
    return ((np.arange(R) // T) % H).astype(np.int32)


# ---- the independence test's pairs ---------------------------------------------------------------------------------------------
def independence_pairs(H):
    """(embedding row, head) pairs sorted by head: runs of T - 1, T + 1 and 2 T rows of heads 0, 1, 2 -- the first two straddle a tile
    border, the third fills two tiles -- then one row of every other head.  Pair i reads embedding row i."""
    assert H > 3
    heads = [0] * (T - 1) + [1] * (T + 1) + [2] * (2 * T) + list(range(3, H))
    return np.arange(len(heads), dtype=np.int32), np.array(heads, np.int32)


def distinct_batches(heads):
    """the pairs dealt to batches in which every row has a different head -> list of index arrays"""
    left = {}
    for i, h in enumerate(heads):
        left.setdefault(int(h), []).append(i)
    out = []
    while any(left.values()):
        out.append(np.array([v.pop(0) for v in left.values() if v], np.int64))
    return out
