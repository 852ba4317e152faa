"""Clip-level score statistics: per-keyword ROC / DET curves, AUC, equal-error rate, the miss rate at a false-accept rate, top-k
accuracy and calibration.

ScoreStats accumulates three integer arrays on the device with one kernel per batch (kws_score_hist, include/kws.h) and derives every
figure on the host from those counts, in float64 over integer prefix sums:

    hist (C, 2, bins)      hist[c, 1] the scores for class c of the clips labelled c (targets), hist[c, 0] of the clips labelled with
                           another class (non-targets: for a keyword they include the background clips)
    rank_counts (C,)       clips by the rank of their true class (0 = the arg-max; ties go to the lower index, as in the heads)
    calib (2, bins)        clips by the bin of their largest score, and the correctly classified ones among them

A score p falls into bin min(bins - 1, floor(p * bins)) (p <= 0 and NaN: bin 0), thresholds are t_j = j / bins, and a detection at t_j
means "score bin >= j"; the curves are therefore exact for thresholds on that grid and know nothing finer."""
import numpy as np

from . import lib as _l


def uses_lds(num_classes, bins):
    """whether kws_score_hist counts a (num_classes, bins) shape in LDS or straight into global memory (host only)"""
    return bool(_l.get_lib().kws_score_hist_uses_lds(int(num_classes), int(bins)))


class ScoreStats(object):
    """ScoreStats(num_classes, bins=1024, device=None): zeroed counts on `device` (a CUDA device; None = the current one).
    ScoreStats.from_counts(hist, rank_counts, calib) wraps host arrays instead: the curve arithmetic needs no device."""

    def __init__(self, num_classes, bins=1024, device=None):
        import torch
        self.num_classes, self.bins = int(num_classes), int(bins)
        if self.num_classes < 1 or self.bins < 2:
            raise ValueError("num_classes must be >= 1 and bins >= 2")
        if not torch.cuda.is_available():
            raise _l.KwsError(-3, "no HIP device: score statistics are counted on the GPU (no CPU fallback); "
                                  "ScoreStats.from_counts takes host arrays")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.hist = torch.zeros((self.num_classes, 2, self.bins), dtype=torch.int64, device=dev)
        self.rank_counts = torch.zeros((self.num_classes,), dtype=torch.int64, device=dev)
        self.calib = torch.zeros((2, self.bins), dtype=torch.int64, device=dev)

    @classmethod
    def from_counts(cls, hist, rank_counts, calib):
        self = cls.__new__(cls)
        self.hist = np.array(hist, dtype=np.int64, order="C")
        self.rank_counts = np.array(rank_counts, dtype=np.int64, order="C")
        self.calib = np.array(calib, dtype=np.int64, order="C")
        self.num_classes, two, self.bins = self.hist.shape
        if two != 2 or self.rank_counts.shape != (self.num_classes,) or self.calib.shape != (2, self.bins):
            raise ValueError("expected hist (C, 2, bins), rank_counts (C,), calib (2, bins)")
        return self

    def _on_host(self):
        return isinstance(self.hist, np.ndarray)

    # ---- accumulation ---------------------------------------------------------------------------------------------------------
    def update(self, probs, labels):
        """probs (B, C) float32 and labels (B,) int32 CUDA tensors on the accumulator's device: one kernel on the current stream, no
        synchronisation.  Labels outside [0, C) are skipped."""
        import torch
        if self._on_host():
            raise TypeError("a ScoreStats built from host counts does not accumulate")
        if probs.dim() != 2 or probs.shape[1] != self.num_classes or labels.numel() != probs.shape[0]:
            raise ValueError("expected probs (B, %d) and B labels, got %s and %s" % (self.num_classes, tuple(probs.shape), tuple(labels.shape)))
        if probs.device != self.hist.device or labels.device != self.hist.device:
            raise ValueError("probs and labels must be on %s" % (self.hist.device,))
        if probs.shape[0] == 0:
            return self
        p = probs.to(torch.float32).contiguous()
        y = labels.reshape(-1).to(torch.int32).contiguous()
        with torch.cuda.device(self.hist.device):
            _l.check(_l.get_lib().kws_score_hist(p.data_ptr(), y.data_ptr(), p.shape[0], self.num_classes, self.bins, self.hist.data_ptr(),
                                                 self.rank_counts.data_ptr(), self.calib.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
        return self

    def merge(self, other):
        """adds the counts of another accumulator of the same shape (on any device, or on the host)"""
        if (other.num_classes, other.bins) != (self.num_classes, self.bins):
            raise ValueError("cannot merge (%d classes, %d bins) into (%d, %d)" % (other.num_classes, other.bins, self.num_classes, self.bins))
        for name in ("hist", "rank_counts", "calib"):
            mine, theirs = getattr(self, name), getattr(other, name)
            if self._on_host():
                mine += theirs if other._on_host() else theirs.cpu().numpy()
            else:
                import torch
                mine += (torch.from_numpy(theirs) if other._on_host() else theirs).to(mine.device)
        return self

    def counts(self):
        """-> (hist, rank_counts, calib) as host int64 arrays (synchronises)"""
        if self._on_host():
            return self.hist.copy(), self.rank_counts.copy(), self.calib.copy()
        return self.hist.cpu().numpy(), self.rank_counts.cpu().numpy(), self.calib.cpu().numpy()

    # ---- figures --------------------------------------------------------------------------------------------------------------
    def totals(self):
        """-> (targets, non_targets) per class, int64"""
        hist = self.counts()[0]
        return hist[:, 1].sum(1), hist[:, 0].sum(1)

    def curves(self):
        """-> dict of thresholds (bins + 1,) = j / bins, and tpr, fpr, frr = 1 - tpr of shape (C, bins + 1): the rates of "score bin
        >= j" among a class's targets and non-targets (1 at j = 0, 0 at j = bins).  NaN rows for a class without targets (tpr, frr)
        or without non-targets (fpr)."""
        hist = self.counts()[0]
        C, bins = self.num_classes, self.bins
        above = np.zeros((C, 2, bins + 1), np.int64)                     # above[..., j] = count of bins >= j
        above[:, :, :bins] = np.cumsum(hist[:, :, ::-1], axis=2)[:, :, ::-1]
        tot = above[:, :, 0].astype(np.float64)
        tot[tot == 0] = np.nan
        rates = above.astype(np.float64) / tot[:, :, None]
        return {"thresholds": np.arange(bins + 1, dtype=np.float64) / bins, "tpr": rates[:, 1], "fpr": rates[:, 0], "frr": 1.0 - rates[:, 1]}

    def auc(self):
        """-> (C,) area under the ROC curve as the Mann-Whitney statistic of the binned scores: the fraction of (target, non-target)
        pairs in which the target's bin is the higher one, equal bins counting a half.  The numerator is an exact integer."""
        hist = self.counts()[0]
        out = np.full((self.num_classes,), np.nan)
        for c in range(self.num_classes):
            t, n = [int(v) for v in hist[c, 1]], [int(v) for v in hist[c, 0]]
            T, N = sum(t), sum(n)
            if T == 0 or N == 0:
                continue
            twice, below = 0, 0                                          # Python integers: no 2^63 limit on the pair count
            for tj, nj in zip(t, n):
                twice += tj * (2 * below + nj)
                below += nj
            out[c] = twice / (2 * T * N)
        return out

    def eer(self):
        """-> (eer (C,), threshold (C,)): where frr (rising with the threshold) crosses fpr (falling), linearly interpolated between
        the two neighbouring thresholds j / bins."""
        cv = self.curves()
        th, C = cv["thresholds"], self.num_classes
        rate, where = np.full((C,), np.nan), np.full((C,), np.nan)
        for c in range(C):
            d = cv["frr"][c] - cv["fpr"][c]                               # -1 at j = 0 ... +1 at j = bins, non-decreasing
            if np.isnan(d[0]):
                continue
            j = int(np.argmax(d >= 0))                                   # first threshold at which frr >= fpr; j >= 1
            a = -d[j - 1] / (d[j] - d[j - 1])
            rate[c] = cv["frr"][c, j - 1] + a * (cv["frr"][c, j] - cv["frr"][c, j - 1])
            where[c] = th[j - 1] + a * (th[j] - th[j - 1])
        return rate, where

    def at_far(self, max_far=0.01):
        """-> (threshold (C,), frr (C,)): the lowest threshold j / bins whose false-accept rate is <= max_far, and the miss rate there.
        j = bins (nothing is detected, fpr 0) always qualifies."""
        cv = self.curves()
        C = self.num_classes
        where, miss = np.full((C,), np.nan), np.full((C,), np.nan)
        for c in range(C):
            if np.isnan(cv["fpr"][c, 0]) or np.isnan(cv["frr"][c, 0]):
                continue
            j = int(np.argmax(cv["fpr"][c] <= max_far))
            where[c], miss[c] = cv["thresholds"][j], cv["frr"][c, j]
        return where, miss

    def top_k(self, k):
        """-> fraction of the counted clips whose true class is among the k best scores (NaN without clips)"""
        rank = self.counts()[1]
        total = int(rank.sum())
        if total == 0:
            return float("nan")
        return float(int(rank[:max(0, min(int(k), self.num_classes))].sum()) / total)

    def ece(self):
        """-> (ece, table): the expected calibration error sum_b n_b / n |accuracy_b - confidence_b| over the bins of the largest score,
        with the bin's mid-point (b + 0.5) / bins as its confidence, so the figure is resolved to 1 / (2 * bins) and no finer; table is
        a dict of confidence (bins,), count (bins,), accuracy (bins,; NaN where a bin is empty): the reliability diagram."""
        calib = self.counts()[2]
        n = calib[0].astype(np.float64)
        conf = (np.arange(self.bins, dtype=np.float64) + 0.5) / self.bins
        acc = np.full((self.bins,), np.nan)
        filled = calib[0] > 0
        acc[filled] = calib[1][filled] / n[filled]
        total = float(n.sum())
        ece = float(np.sum(n[filled] * np.abs(acc[filled] - conf[filled])) / total) if total else float("nan")
        return ece, {"confidence": conf, "count": calib[0].copy(), "accuracy": acc}
