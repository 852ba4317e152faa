"""The exact cases of the nearest-neighbour tests (tests/test_knn_gpu.py, tests/test_knn_host.py) with the reason for each, and
their data.

The kernel (csrc/kws_knn.hip) gives a block a tile of 128 queries, 32 per wave, and walks the reference rows in tiles of 32, one
32 x 32 MFMA tile per wave; the columns are taken in groups of 8 (a width of E % 8 == 4 leaves half a group of zeros); a query's
list holds at most KWS_KNN_MAX_K = 64 entries.  The shapes sit one below, at and one above those edges (and those of 64 rows, two
tiles).

Embeddings are integers from -4..4: a dot product is at most 128 * 16 = 2048 and a squared distance at most 128 * 64 = 8192 in
magnitude, every partial sum is an integer below 2^24, so float32 computes them exactly in any order and idx / score must EQUAL the
float64 reference.  So few values make equal scores abundant, and reference rows 1 and N - 2 are copies of rows N - 1 and 0 (where N
allows), so that the rule "equal score: the lower index first" decides in every case."""
import collections

import numpy as np

import knn_ref as kr

Shape = collections.namedtuple("Shape", "Q N why")

# (Q, N) of the issue
SHAPES = [
    Shape(1, 1, "one query, one row: every k > 1 is a tail of -1; with an exclusion nothing is left at all"),
    Shape(1, 5, "k = 5 is all rows, k = 5 with an exclusion is one short, k = 32 / 64 are mostly tail"),
    Shape(33, 31, "one query past a wave's 32; one row short of a reference tile"),
    Shape(129, 257, "one query past the block's 128 (a second block of one query); one row past eight reference tiles"),
    Shape(130, 1025, "two queries in the second block; 33 tiles, the last with one row: the shape of the slices test"),
]
# the edges of the tiles that were built, where the issue's shapes do not sit on them already
EDGE_SHAPES = [
    Shape(32, 63, "a full wave of queries; one row short of two reference tiles"),
    Shape(127, 64, "one query short of the block's tile; exactly two reference tiles"),
    Shape(128, 65, "exactly the block's tile; one row into the third reference tile"),
    Shape(31, 33, "one query short of a wave; one row into the second reference tile"),
    Shape(5, 32, "exactly one reference tile"),
]
WIDTHS = (4, 48, 128)           # half a column group (padded with zeros) / the recurrent models / the CNNs and the most the kernel takes
EDGE_WIDTHS = (8, 12, 124)      # exactly one group / one and a half / the widest with half a group of padding
KS = (1, 5, 32, 64)             # the threshold is the only entry / a usual k / half / KWS_KNN_MAX_K
SLICES = (1, 2, 7, 64, 0)       # one / two / an odd split of 33 tiles (5 each, the last slice has 3) / more slices than tiles / the default

_data = {}
_ref = {}


def data(Q, N, E):
    """-> (queries (Q, E), refs (N, E), exclude (Q)) float32 / int32, the same for every test that names the shape"""
    key = (Q, N, E)
    if key not in _data:
        rng = np.random.default_rng(Q * 100003 + N * 101 + E)
        refs = rng.integers(-4, 5, (N, E)).astype(np.float32)
        if N >= 4:
            refs[1] = refs[N - 1]
            refs[N - 2] = refs[0]
        queries = rng.integers(-4, 5, (Q, E)).astype(np.float32)
        queries[0] = refs[0]                                        # distance 0, and the copy of row 0 ties with it
        exclude = (np.arange(Q) % N).astype(np.int32)
        if Q >= 3:
            exclude[Q // 2] = -1                                    # "none" in the middle of the others
        for a in (queries, refs, exclude):
            a.setflags(write=False)
        _data[key] = (queries, refs, exclude)
    return _data[key]


def expected(Q, N, E, metric, with_exclude):
    """the reference at k = 64, computed once per (shape, metric, exclusion): a smaller k is its first k columns"""
    key = (Q, N, E, metric, with_exclude)
    if key not in _ref:
        q, r, ex = data(Q, N, E)
        idx, score = kr.knn(q, r, 64, metric, ex if with_exclude else None)
        idx.setflags(write=False)
        score.setflags(write=False)
        _ref[key] = (idx, score)
    return _ref[key]
