"""float64 numpy oracle of the weight averaging kws_optimizer_step folds into its update (include/kws.h KWS_AVG_*): the schedules of
MovingAverage, SWA and Lookahead (common/model_utils.py: average_args) and the two formulas, on flat buffers with a segment list.
Nothing is kept between calls but the slot the caller owns."""
import numpy as np

NONE, BLEND, SYNC = 0, 1, 2


def f32(x):
    return float(np.float32(x))


def ema_args(k, average_decay=0.99, start_step=0):
    """always BLEND; the slot follows the weights until start_step"""
    return BLEND, (1.0 if k < start_step else f32(1.0 - average_decay))


def swa_args(k, start_averaging=0, average_period=10):
    """a snapshot every average_period updates from start_averaging on; snapshot number n (0-based) enters the mean with 1/(n+1)"""
    d = k - start_averaging
    if d < 0 or d % average_period != 0:
        return NONE, 0.0
    return BLEND, f32(1.0 / (d // average_period + 1))


def lookahead_args(k, sync_period=6, slow_step_size=0.5):
    """the update that completes a group of sync_period pulls the slow weights and restarts the fast ones there"""
    if (k + 1) % sync_period != 0:
        return NONE, 0.0
    return SYNC, f32(slow_step_size)


SCHEDULES = {"ema": ema_args, "swa": swa_args, "lookahead": lookahead_args}


def apply(mode, alpha, p, avg, segments, dtype=np.float64):
    """p: the parameters after this step's update; p and avg are changed in place inside the segments [(offset, size), ...] only.
    dtype=np.float32 restates the kernel's own arithmetic (one rounding per operation, nothing contracted)."""
    if mode == NONE:
        return
    al = dtype(alpha)
    for o, n in segments:
        a, q = avg[o:o + n].astype(dtype), p[o:o + n].astype(dtype)
        if mode == BLEND:
            avg[o:o + n] = a - (a - q) * al
        elif mode == SYNC:
            s = a + al * (q - a)
            avg[o:o + n] = s
            p[o:o + n] = s
        else:
            raise ValueError("unknown averaging mode %r" % (mode,))
