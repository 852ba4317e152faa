"""Query by example: where does something that sounds like these few recordings occur?  (include/kws.h: kws_dtw, kws_dtw_peaks;
csrc/kws_dtw.hip)  No model, no labels, no one-second framing: subsequence dynamic time warping of the examples'
MFCC rows against the rows of whole recordings.

    t = Templates.enroll(pr, ["yes_1.wav", "yes_2.wav", "no_1.wav"], ["yes", "yes", "no"])      # trimmed to their speech by Vad
    cost, start = match(t, recordings)                    # (R, Q, max_frames) on the GPU: the cost of the best match ENDING at each frame
    hits = search(t, recordings, threshold=0.25)          # Hits: recording, keyword, template, start_s, end_s, cost
    word, cost = classify(t, clips)                       # per clip the keyword with the lowest cost anywhere inside it

`recordings` is what kws_amd.stream.scan takes: a list of 1-D int16 arrays, or a padded (R, n) int16 array / CUDA tensor with
`lengths`.  The arithmetic is the kernels': float32, the same bits for every `tile_frames`.  Everything is validated on the host
before any device work (ValueError)."""
import numpy as np

from . import lib as _l

METRICS = ("cosine", "l2")


def _torch():
    import torch
    return torch


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Hits(object):
    """numpy arrays of equal length, ordered by (recording, keyword, end): recording, keyword (an index into Templates.keywords),
    template, start_s, end_s, cost; start_frame and end_frame are the row indices behind the times."""

    def __init__(self, recording, keyword, template, start_s, end_s, cost, start_frame, end_frame, keywords):
        self.recording, self.keyword, self.template = recording, keyword, template
        self.start_s, self.end_s, self.cost = start_s, end_s, cost
        self.start_frame, self.end_frame, self.keywords = start_frame, end_frame, keywords

    def __len__(self):
        return int(self.recording.shape[0])

    def rows(self):
        """[(recording, keyword name, template, start_s, end_s, cost)]"""
        return [(int(r), self.keywords[int(k)], int(t), float(a), float(b), float(c))
                for r, k, t, a, b, c in zip(self.recording, self.keyword, self.template, self.start_s, self.end_s, self.cost)]


# ---- host-side validation -------------------------------------------------------------------------------------------------------
def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(METRICS), metric))


def _check_tile(tile_frames):
    tile_frames = int(tile_frames)
    if tile_frames != 0 and not 32 <= tile_frames <= 2 ** 20:
        raise ValueError("tile_frames = %d: 0 (the library chooses) or 32..2^20" % tile_frames)
    return tile_frames


def _check_rows(rows, n_frames, name="rows"):
    torch = _torch()
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or rows.dtype != torch.float32 or not rows.is_contiguous() or rows.shape[1] < 1:
        raise ValueError("%s must be a contiguous float32 tensor of shape (R, max_frames, D), max_frames >= 1" % name)
    R, F, D = (int(v) for v in rows.shape)
    if D < 1 or D > 64:
        raise ValueError("D = %d: rows are 1..64 wide" % D)
    if F > 2 ** 30:
        raise ValueError("max_frames = %d, at most 2^30" % F)
    n = n_frames.detach().cpu().numpy() if isinstance(n_frames, torch.Tensor) else np.asarray(n_frames)
    n = n.reshape(-1)
    if n.shape[0] != R or n.dtype.kind not in "iu" or (n.size and (n.min() < 0 or n.max() > F)):
        raise ValueError("n_frames must give one row count in 0..%d per entry of %s" % (F, name))
    return R, F, D, n.astype(np.int32)


def _check_templates(t):
    if not isinstance(t, Templates):
        raise ValueError("templates must be a Templates object (Templates.enroll, Templates.from_rows)")


def _pad4(rows):
    D = int(rows.shape[-1])
    if D % 4 == 0:
        return rows
    return _torch().nn.functional.pad(rows, (0, 4 - D % 4)).contiguous()         # zero columns change neither metric


def _unit(rows):
    """kws_rows_normalize over the rows of an (A, F, D) tensor"""
    torch = _torch()
    out = torch.empty_like(rows)
    N, D = int(rows.shape[0] * rows.shape[1]), int(rows.shape[2])
    if N:
        with torch.cuda.device(rows.device):
            _l.check(_l.get_lib().kws_rows_normalize(rows.data_ptr(), N, D, out.data_ptr(), None, _stream()))
    return out


def _subtract_mean(rows, n):
    """rows (A, F, D) minus the mean of each entry's first n[a] rows; the rows past them stay zero"""
    torch = _torch()
    F = rows.shape[1]
    live = (torch.arange(F, device=rows.device)[None, :] < n[:, None]).to(rows.dtype)[:, :, None]
    mean = (rows * live).sum(dim=1, keepdim=True) / n.clamp(min=1).to(rows.dtype)[:, None, None]
    return ((rows - mean) * live).contiguous()


class Templates(object):
    """The enrolled examples: rows (Q, Lmax, D) float32 on the GPU (zero past each length), lengths (Q) host int32, keywords (the G
    names), group (Q) host int32 -- the keyword of each template, non-decreasing --, source (Q): what each template was made from."""

    def __init__(self, rows, lengths, keywords, group, source=None, cmn=False, pr=None, featurizer=None):
        self.rows, self.lengths, self.keywords, self.group = rows, lengths, list(keywords), group
        self.source, self.cmn, self.pr, self.featurizer = source, bool(cmn), pr, featurizer
        self._dev = None

    def __len__(self):
        return int(self.lengths.shape[0])

    def device_tables(self):
        """(lengths, group) as int32 device tensors"""
        if self._dev is None:
            torch = _torch()
            self._dev = (torch.from_numpy(self.lengths).to(self.rows.device), torch.from_numpy(self.group).to(self.rows.device))
        return self._dev

    @staticmethod
    def _order(keywords, Q):
        """-> (names in order of first appearance, group per example, the stable order that sorts the examples by group)"""
        keywords = list(keywords)
        if len(keywords) != Q or Q < 1:
            raise ValueError("%d keywords for %d examples (at least one example, one keyword each)" % (len(keywords), Q))
        if Q > _l.DTW_MAX_Q:
            raise ValueError("%d examples, at most %d" % (Q, _l.DTW_MAX_Q))
        names = []
        for k in keywords:
            if not isinstance(k, str) or not k:
                raise ValueError("a keyword must be a non-empty string, not %r" % (k,))
            if k not in names:
                names.append(k)
        group = np.array([names.index(k) for k in keywords], np.int32)
        return names, group, np.argsort(group, kind="stable")

    @classmethod
    def from_rows(cls, rows, lengths, keywords, cmn=False, pr=None, featurizer=None):
        """Templates from feature rows that already exist: rows (Q, Lmax, D) float32 CUDA tensor, lengths (Q) in 1..Lmax <= 64"""
        torch = _torch()
        Q, Lmax, D, n = _check_rows(rows, lengths, "template rows")
        if Lmax > _l.DTW_MAX_ROWS:
            raise ValueError("templates of %d rows: at most %d" % (Lmax, _l.DTW_MAX_ROWS))
        if n.size and n.min() < 1:
            raise ValueError("a template has no rows")
        names, group, order = cls._order(keywords, Q)
        if not rows.is_cuda:
            raise ValueError("template rows must live on the GPU")
        idx = torch.from_numpy(order).to(rows.device)
        rows, n = rows[idx].contiguous(), n[order]
        if cmn:
            rows = _subtract_mean(rows, torch.from_numpy(n).to(rows.device))
        return cls(rows, n, names, group[order], source=[int(i) for i in order], cmn=cmn, pr=pr, featurizer=featurizer)

    @classmethod
    def enroll(cls, pr, clips_or_paths, keywords, trim=True, featurizer=None, cmn=False):
        """One template per example.  clips_or_paths: wav paths (16-bit PCM at pr.sample_rate) and / or 1-D int16 arrays; keywords: the
        word each one says.  trim: cut every example to the span Vad finds speech in (an example without speech is refused).  An
        example of more than 64 rows is refused.  cmn: subtract each example's mean row (match then does the same to every recording)."""
        from .vad import Vad, read_wav
        clips_or_paths = list(clips_or_paths)
        names, group, order = cls._order(keywords, len(clips_or_paths))
        if pr.use_delta:
            raise ValueError("query by example works on the plain MFCC rows (use_delta = False)")
        W, H, rate = int(pr.window_samples), int(pr.hop_samples), int(pr.sample_rate)
        clips = []
        for i, c in enumerate(clips_or_paths):
            if isinstance(c, (str, bytes)) or hasattr(c, "__fspath__"):
                data, r = read_wav(c)
                if r != rate:
                    raise ValueError("%s is at %d Hz, the featurizer at %d Hz" % (c, r, rate))
            else:
                data = np.asarray(c)
                if data.ndim != 1 or data.dtype != np.int16:
                    raise ValueError("example %d must be a wav path or a 1-D int16 array" % i)
            clips.append(np.ascontiguousarray(data))
        def row_counts():
            frames = [0 if c.size < W else (c.size - W) // H + 1 for c in clips]
            for i, (c, f) in enumerate(zip(clips, frames)):
                if f < 1:
                    raise ValueError("example %d (%s) is %.3f s long, shorter than one window of %.3f s" % (i, keywords[i], c.size / rate, W / rate))
                if f > _l.DTW_MAX_ROWS:
                    raise ValueError("example %d (%s) is %.3f s long (%d rows); a template holds at most %d rows, %.3f s"
                                     % (i, keywords[i], c.size / rate, f, _l.DTW_MAX_ROWS, ((_l.DTW_MAX_ROWS - 1) * H + W) / rate))
            return frames

        if not trim:
            row_counts()                      # known from the sample counts alone
        torch = _torch()
        if not torch.cuda.is_available():
            raise ValueError("enrolment runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        if trim:
            spans = Vad(rate).detect(clips).span.cpu().numpy()
            for i, (b, e) in enumerate(spans):
                if e <= b:
                    raise ValueError("example %d (%s) has no speech; enrol it with trim=False if it is meant as it is" % (i, keywords[i]))
                clips[i] = clips[i][int(b):int(e)]
        frames = row_counts()
        clips, frames = [clips[i] for i in order], np.array([frames[i] for i in order], np.int32)
        if featurizer is None:
            from .featurizer import Featurizer
            featurizer = Featurizer(pr)
        rows, _ = _featurize(pr, featurizer, clips, None, max_frames=int(frames.max()))
        rows = _pad4(rows)
        if cmn:
            rows = _subtract_mean(rows, torch.from_numpy(frames).to(rows.device))
        return cls(rows, frames, names, group[order], source=[int(i) for i in order], cmn=cmn, pr=pr, featurizer=featurizer)


def _featurize(pr, featurizer, recordings, lengths, max_frames=None):
    """kws_featurize_long -> (rows (R, max_frames, n_mfcc) CUDA float32, host int32 row counts)"""
    from .stream import _pack_recordings
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    wav, lens = _pack_recordings(torch, recordings, lengths, dev)
    W, H = int(pr.window_samples), int(pr.hop_samples)
    n = np.array([0 if v < W else (v - W) // H + 1 for v in lens], np.int32)
    F = max(1, int(n.max()) if n.size else 1) if max_frames is None else int(max_frames)
    R = len(lens)
    rows = torch.empty((R, F, int(pr.n_mfcc)), dtype=torch.float32, device=dev)
    if R:
        d_len = torch.tensor(lens, dtype=torch.int32).to(dev)
        _l.check(_l.get_lib().kws_featurize_long(featurizer._h, wav.data_ptr(), _l.WAV_I16, R, int(wav.shape[1]), d_len.data_ptr(), F,
                                                 rows.data_ptr(), _stream()))
    return rows, np.minimum(n, F).astype(np.int32)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def match_rows(templates, rows, n_frames, metric="cosine", tile_frames=0):
    """kws_dtw on feature rows that already exist: rows (R, max_frames, D) float32 CUDA tensor, n_frames (R) -> (cost (R, Q, max_frames)
    float32, start (R, Q, max_frames) int32) on the GPU.  cost[r, q, j] is the cost per template row of the best match of template q
    that ENDS at frame j of recording r, start[r, q, j] the frame it begins at; +inf / -1 where no match ends."""
    torch = _torch()
    _check_templates(templates)
    _check_metric(metric)
    tile_frames = _check_tile(tile_frames)
    R, F, D, n = _check_rows(rows, n_frames)
    if (D + 3) // 4 * 4 != int(templates.rows.shape[2]):
        raise ValueError("rows are %d wide, the templates %d" % (D, int(templates.rows.shape[2])))
    if not rows.is_cuda or rows.device != templates.rows.device:
        raise ValueError("rows must live on the GPU the templates live on")
    dev = rows.device
    Q, Lmax = len(templates), int(templates.rows.shape[1])
    cost = torch.empty((R, Q, F), dtype=torch.float32, device=dev)
    start = torch.empty((R, Q, F), dtype=torch.int32, device=dev)
    if R == 0:
        return cost, start
    n_d = torch.from_numpy(n).to(dev)
    rows, tr = _pad4(rows), templates.rows
    if templates.cmn:
        rows = _subtract_mean(rows, n_d)
    if metric == "cosine":
        rows, tr = _unit(rows), _unit(tr)
    L = _l.get_lib()
    Dp = int(rows.shape[2])
    need = int(L.kws_dtw_workspace_bytes(R, Q, F, Dp, tile_frames))
    if need < 0:
        _l.check(need)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        _l.check(L.kws_dtw(tr.data_ptr(), templates.device_tables()[0].data_ptr(), Q, Lmax, rows.data_ptr(), n_d.data_ptr(), R, F, Dp,
                           _l.DTW_METRICS["l2" if metric == "l2" else "dot"], tile_frames, cost.data_ptr(), start.data_ptr(),
                           ws.data_ptr() if ws is not None else None, need, _stream()))
    return cost, start


def _recording_rows(templates, recordings, lengths):
    if templates.pr is None or templates.featurizer is None:
        raise ValueError("these templates were made from rows (Templates.from_rows): match them with match_rows")
    return _featurize(templates.pr, templates.featurizer, recordings, lengths)


def match(templates, recordings, lengths=None, metric="cosine", tile_frames=0):
    """Every template against every recording -> (cost, start) as match_rows returns them, over the rows kws_featurize_long gives the
    recordings.  metric 'cosine': both sides go through kws_rows_normalize, the local cost is 1 - cos; 'l2': the squared distance."""
    _check_templates(templates)
    _check_metric(metric)
    _check_tile(tile_frames)
    if not _torch().cuda.is_available():
        raise ValueError("matching runs on the GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    rows, n = _recording_rows(templates, recordings, lengths)
    return match_rows(templates, rows, n, metric, tile_frames)


def peaks(templates, cost, start, threshold, min_gap, max_hits):
    """kws_dtw_peaks -> (count (R, G), end, start, cost, template (R, G, max_hits)) on the GPU, in the order of selection"""
    torch = _torch()
    _check_templates(templates)
    threshold, min_gap, K = float(threshold), int(min_gap), int(max_hits)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    if min_gap < 1:
        raise ValueError("min_gap = %d frames: at least 1" % min_gap)
    if K < 1 or K > _l.DTW_MAX_HITS:
        raise ValueError("max_hits = %d: 1..%d" % (K, _l.DTW_MAX_HITS))
    Q, G = len(templates), len(templates.keywords)
    for name, t, dt in (("cost", cost, torch.float32), ("start", start, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != dt or not t.is_contiguous() or t.shape[1] != Q or t.shape[2] < 1:
            raise ValueError("%s must be a contiguous %s tensor of shape (R, %d, max_frames)" % (name, dt, Q))
    if tuple(cost.shape) != tuple(start.shape):
        raise ValueError("cost is %s, start %s" % (tuple(cost.shape), tuple(start.shape)))
    if not cost.is_cuda or not start.is_cuda:
        raise ValueError("cost and start must live on the GPU (match returns them there)")
    dev = cost.device
    R, F = int(cost.shape[0]), int(cost.shape[2])
    count = torch.zeros((R, G), dtype=torch.int32, device=dev)
    end, hs, ht = (torch.empty((R, G, K), dtype=torch.int32, device=dev) for _ in range(3))
    hc = torch.empty((R, G, K), dtype=torch.float32, device=dev)
    if R:
        with torch.cuda.device(dev):
            _l.check(_l.get_lib().kws_dtw_peaks(cost.data_ptr(), start.data_ptr(), R, Q, F, templates.device_tables()[1].data_ptr(),
                                                templates.group.ctypes.data, G, threshold, min_gap, K, count.data_ptr(), end.data_ptr(),
                                                hs.data_ptr(), hc.data_ptr(), ht.data_ptr(), _stream()))
    return count, end, hs, hc, ht


def search(templates, recordings, lengths=None, metric="cosine", tile_frames=0, threshold=0.3, min_gap_s=0.5, max_hits=16):
    """Where the keywords occur -> Hits.  Per (recording, keyword) up to max_hits detections whose cost is <= threshold, no two ends
    closer than min_gap_s.  A detection spans the samples [start_frame hop, end_frame hop + window)."""
    _check_templates(templates)
    _check_metric(metric)
    _check_tile(tile_frames)
    threshold, min_gap_s, K = float(threshold), float(min_gap_s), int(max_hits)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    if not min_gap_s >= 0.0:
        raise ValueError("min_gap_s = %g seconds" % min_gap_s)
    if K < 1 or K > _l.DTW_MAX_HITS:
        raise ValueError("max_hits = %d: 1..%d" % (K, _l.DTW_MAX_HITS))
    if templates.pr is None:
        raise ValueError("these templates were made from rows (Templates.from_rows): use match_rows and peaks")
    pr = templates.pr
    H, W, rate = int(pr.hop_samples), int(pr.window_samples), float(pr.sample_rate)
    min_gap = max(1, int(round(min_gap_s * rate / H)))
    cost, start = match(templates, recordings, lengths, metric, tile_frames)
    count, end, hs, hc, ht = (t.cpu().numpy() for t in peaks(templates, cost, start, threshold, min_gap, K))
    keep = np.arange(K)[None, None, :] < count[:, :, None]
    rec, kw, _ = np.nonzero(keep)
    e, s, c, t = end[keep], hs[keep], hc[keep], ht[keep]
    order = np.lexsort((e, kw, rec))
    rec, kw, e, s, c, t = rec[order], kw[order], e[order], s[order], c[order], t[order]
    return Hits(rec.astype(np.int64), kw.astype(np.int64), t.astype(np.int64), s * H / rate, (e * H + W) / rate, c, s.astype(np.int64),
                e.astype(np.int64), list(templates.keywords))


def classify(templates, clips, lengths=None, metric="cosine"):
    """Per clip the keyword whose templates match best ANYWHERE inside it (the subsequence minimum: silence around the word does not
    count against it) -> (keyword index (B) int64, cost (B) float32) as numpy arrays; a clip nothing matches gets -1 / +inf."""
    _check_templates(templates)
    _check_metric(metric)
    torch = _torch()
    cost, _ = match(templates, clips, lengths, metric)
    best = cost.amin(dim=2)                                               # (B, Q)
    group = templates.device_tables()[1].long()
    G = len(templates.keywords)
    per = torch.full((best.shape[0], G), float("inf"), dtype=torch.float32, device=best.device)
    per = per.scatter_reduce(1, group[None, :].expand(best.shape[0], -1), best, reduce="amin")
    val, idx = per.min(dim=1)
    idx = torch.where(torch.isfinite(val), idx, torch.full_like(idx, -1))
    return idx.cpu().numpy(), val.cpu().numpy()
