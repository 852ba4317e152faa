"""numpy reference of the query-by-example search (include/kws.h: kws_dtw, kws_dtw_peaks): the slope-constrained subsequence DTW in
float32 (the kernel's arithmetic) and in float64, a tiled variant, a brute-force enumerator of the paths for tiny cases, and the
greedy peak picker."""
import numpy as np

DOT, L2 = 0, 1


def local_cost(q, x, metric, dtype=np.float32):
    """(L, n) costs of template rows against frames: one chain over the columns in ascending order, as the kernel's FMAs (exact on
    the integer test data whatever the rounding of the intermediate product)"""
    q, x = np.asarray(q, dtype), np.asarray(x, dtype)
    acc = np.zeros((q.shape[0], x.shape[0]), dtype)
    for k in range(q.shape[1]):
        if metric == L2:
            e = q[:, k, None] - x[None, :, k]
            acc = acc + e * e
        else:
            acc = acc + q[:, k, None] * x[None, :, k]
    return acc if metric == L2 else (dtype(1) - acc).astype(dtype)


def dtw_from_cost(d, first=0, dtype=np.float32):
    """The recurrence over a cost matrix d (L, n) -> (C of the last row (n), S of the last row (n)), NOT yet divided by L.  Column
    indices reported in S are offset by `first` (a tile that starts at frame `first`)."""
    d = np.asarray(d, dtype)
    L, n = d.shape
    inf = dtype(np.inf)
    two = dtype(2)
    outC = np.full((n,), inf, dtype)
    outS = np.full((n,), -1, np.int64)
    # the columns j - 1 and j - 2 of C and S; a candidate that does not exist is +inf / -1, which never wins
    C1, C2 = np.full((L,), inf, dtype), np.full((L,), inf, dtype)
    S1, S2 = np.full((L,), -1, np.int64), np.full((L,), -1, np.int64)

    def down(v, k, fill):                            # row i takes row i - k
        out = np.full_like(v, fill)
        out[k:] = v[:len(v) - k]
        return out

    with np.errstate(invalid="ignore"):
        for j in range(n):
            col = d[:, j]
            c1, s1 = down(C1, 1, inf) + col, down(S1, 1, -1)
            c2, s2 = down(C2, 1, inf) + col, down(S2, 1, -1)
            c3, s3 = down(C1, 2, inf) + two * col, down(S1, 2, -1)
            best, s = c1.copy(), s1.copy()
            for cv, sv in ((c2, s2), (c3, s3)):      # in candidate order: a tie keeps the lower number
                win = cv < best
                best[win], s[win] = cv[win], sv[win]
            best[0], s[0] = col[0], first + j
            dead = ~(best < inf)
            best[dead], s[dead] = inf, -1
            C2, S2, C1, S1 = C1, S1, best, s
            outC[j], outS[j] = best[L - 1], s[L - 1]
    return outC, outS


def dtw(q, x, metric, max_frames=None, dtype=np.float32):
    """One template (L, D) against one recording (n, D) -> (cost (max_frames) dtype, start (max_frames) int32); frames past n are
    +inf / -1"""
    q, x = np.asarray(q), np.asarray(x)
    L, n = q.shape[0], x.shape[0]
    F = n if max_frames is None else max_frames
    cost = np.full((F,), np.inf, dtype)
    start = np.full((F,), -1, np.int32)
    if n and L:
        c, s = dtw_from_cost(local_cost(q, x, metric, dtype), 0, dtype)
        cost[:n] = c / dtype(L)
        start[:n] = s
    return cost, start


def dtw_tiled(q, x, metric, tile, dtype=np.float32):
    """The same through tiles of `tile` frames that each start 2 (L - 1) frames early"""
    q, x = np.asarray(q), np.asarray(x)
    L, n = q.shape[0], x.shape[0]
    cost = np.full((n,), np.inf, dtype)
    start = np.full((n,), -1, np.int32)
    for t0 in range(0, n, tile):
        t1 = min(n, t0 + tile)
        c0 = max(0, t0 - 2 * (L - 1))
        c, s = dtw_from_cost(local_cost(q, x[c0:t1], metric, dtype), c0, dtype)
        cost[t0:t1] = (c / dtype(L))[t0 - c0:]
        start[t0:t1] = s[t0 - c0:]
    return cost, start


def dtw_many(templates, lengths, rows, n_frames, metric, dtype=np.float32):
    """templates (Q, Lmax, D) / lengths (Q), rows (R, max_frames, D) / n_frames (R) -> cost, start (R, Q, max_frames)"""
    R, F = rows.shape[0], rows.shape[1]
    Q = templates.shape[0]
    cost = np.full((R, Q, F), np.inf, dtype)
    start = np.full((R, Q, F), -1, np.int32)
    for r in range(R):
        for k in range(Q):
            cost[r, k], start[r, k] = dtw(templates[k, :lengths[k]], rows[r, :n_frames[r]], metric, F, dtype)
    return cost, start


def brute_force(d):
    """Every path by enumeration, in float64 on a cost matrix d (L, n) -> (best weighted sum per end frame (n), the set of starts that
    reach it per end frame).  A path moves (1,1) or (1,2) at weight 1, or (2,1) at weight 2; it starts in row 0 at any frame."""
    d = np.asarray(d, np.float64)
    L, n = d.shape
    best = np.full((n,), np.inf)
    starts = [set() for _ in range(n)]

    def walk(i, j, total, s):
        if i == L - 1:
            if total < best[j]:
                best[j] = total
                starts[j] = {s}
            elif total == best[j]:
                starts[j].add(s)
            return
        for di, dj, w in ((1, 1, 1.0), (1, 2, 1.0), (2, 1, 2.0)):
            if i + di < L and j + dj < n:
                walk(i + di, j + dj, total + w * d[i + di, j + dj], s)

    for j0 in range(n):
        walk(0, j0, d[0, j0], j0)
    return best, starts


def peaks(cost, start, group, G, threshold, min_gap, K):
    """cost, start (R, Q, F), group (Q) -> count (R, G), end, hit_start, hit_template (R, G, K) int32, hit_cost (R, G, K) float32"""
    cost, start, group = np.asarray(cost, np.float32), np.asarray(start), np.asarray(group)
    R, Q, F = cost.shape
    count = np.zeros((R, G), np.int32)
    end = np.full((R, G, K), -1, np.int32)
    hs = np.full((R, G, K), -1, np.int32)
    ht = np.full((R, G, K), -1, np.int32)
    hc = np.full((R, G, K), np.inf, np.float32)
    for r in range(R):
        for g in range(G):
            mem = np.nonzero(group == g)[0]
            if mem.size == 0:
                continue
            sub = cost[r, mem]
            arg = np.argmin(sub, axis=0)                     # the first minimum: the lower template
            curve = sub[arg, np.arange(F)]
            live = np.isfinite(curve) & (curve <= np.float32(threshold))
            for k in range(K):
                if not live.any():
                    break
                f = int(np.argmin(np.where(live, curve, np.inf)))         # the first minimum: the lower frame
                tq = int(mem[arg[f]])
                end[r, g, k], hs[r, g, k], hc[r, g, k], ht[r, g, k] = f, start[r, tq, f], curve[f], tq
                live[max(0, f - min_gap + 1):f + min_gap] = False
                count[r, g] += 1
    return count, end, hs, hc, ht
