"""numpy restatement of the counter-based draws of the raw-audio augmentation stages (csrc/kws_wave_stage.h: aug_hash, aug_unit,
aug_uniform), shared by tests/test_augment_gpu.py, tests/test_reverb_gpu.py, tests/filter_ref.py and tests/speed_ref.py."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def np_hash(seed, step, index):
    """aug_hash(seed, step, index) for an array of indices (taken modulo 2^32)"""
    index = np.asarray(index, np.uint64) & M32
    key_lo = np.uint64((seed & 0xFFFFFFFF) ^ ((step * 0x27D4EB2F) & 0xFFFFFFFF))
    key_hi = np.uint64(((seed >> 32) + step) & 0xFFFFFFFF)
    h = index ^ key_lo
    h = (h + key_hi * np.uint64(0x9E3779B9)) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def np_unit(h):
    """aug_unit: float32 in [0, 1) from the hash's upper 24 bits"""
    return (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def np_uniform(h, n):
    """aug_uniform: integer in [0, n)"""
    return ((h * np.asarray(n, np.uint64)) >> np.uint64(32)).astype(np.int64)


def np_pick(seed, step, pos, rate, K):
    """aug_pick with two fields per clip (reverb, filter): one of K with probability `rate`, else -1"""
    pos = np.asarray(pos, np.uint64)
    return np.where(np_unit(np_hash(seed, step, 2 * pos)) < np.float32(rate), np_uniform(np_hash(seed, step, 2 * pos + 1), K), -1)
