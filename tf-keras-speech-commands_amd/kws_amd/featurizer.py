"""Device featurizer: a thin owner of a `kws_featurizer` handle (include/kws.h)."""
import ctypes

import numpy as np

from . import lib as _l
from .augment import _clip_batch


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _l.KwsError(-3, "no HIP device visible to torch: the featurizer has no CPU fallback")
    return torch


def params_struct(pr):
    return _l.KwsParams(float(pr.buffer_t), float(pr.window_t), float(pr.hop_t), int(pr.sample_rate),
                        int(pr.sample_depth), int(pr.n_fft), int(pr.n_filt), int(pr.n_mfcc), int(bool(pr.use_delta)))


def params_key(pr):
    return (float(pr.buffer_t), float(pr.window_t), float(pr.hop_t), int(pr.sample_rate), int(pr.sample_depth),
            int(pr.n_fft), int(pr.n_filt), int(pr.n_mfcc), bool(pr.use_delta))


def derive_geometry(pr):
    """classifier/params.py derived properties computed by the C ABI (host only, no GPU needed)."""
    g = _l.KwsGeometry()
    p = params_struct(pr)
    _l.check(_l.get_lib().kws_params_derive(ctypes.byref(p), ctypes.byref(g)))
    return g.as_dict()


class Featurizer(object):
    """Batched waveform -> (B, n_features, feature_size) features on the current HIP device."""

    def __init__(self, pr, bank="mel"):
        self._L = _l.get_lib()
        self._h = ctypes.c_void_p()
        self.bank_kind = {"mel": _l.BANK_MEL, "bark": _l.BANK_BARK}[bank]
        p = params_struct(pr)
        _l.check(self._L.kws_featurizer_create(ctypes.byref(p), self.bank_kind, ctypes.byref(self._h)))
        g = _l.KwsGeometry()
        _l.check(self._L.kws_featurizer_geometry(self._h, ctypes.byref(g)))
        self.geometry = g.as_dict()
        self.n_filt, self.n_fft, self.n_mfcc = int(pr.n_filt), int(pr.n_fft), int(pr.n_mfcc)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.kws_featurizer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_cu_share(self, blocks_per_cu):
        """2 (default): a launch may fill every CU's LDS (fastest alone); 1: half of it, leaving room for kernels of other
        streams (featurizing beside a train step: kws_amd.pipeline.FeaturePipeline sets this)."""
        _l.check(self._L.kws_featurizer_set_cu_share(self._h, int(blocks_per_cu)))

    def occupancy(self):
        """(resident clips per compute unit, LDS bytes per clip) the HIP runtime reports for this featurizer's kernel."""
        nb, lds = ctypes.c_int(0), ctypes.c_size_t(0)
        _l.check(self._L.kws_featurizer_occupancy(self._h, ctypes.byref(nb), ctypes.byref(lds)))
        return nb.value, lds.value

    def bank(self):
        out = np.zeros((self.n_filt, self.n_fft // 2 + 1), np.float32)
        _l.check(self._L.kws_featurizer_bank(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size))
        return out

    @staticmethod
    def _dtype_code(t):
        torch = _torch()
        if t.dtype == torch.float32:
            return _l.WAV_F32
        if t.dtype == torch.int16:
            return _l.WAV_I16
        raise TypeError("waveforms must be float32 or int16, got %s" % t.dtype)

    def __call__(self, wav, valid_len=None, out=None, index=None, augment=None, step=0, position_base=0):
        """wav: CUDA tensor (rows, stride) float32|int16; valid_len: optional CUDA int32 (rows,).  index: optional CUDA int32 (B,): featurize
        the B rows wav[index[b]] in place of all rows (kws_featurize_gather: a shuffled minibatch of a device-resident dataset, no copy).
        augment: optional kws_amd.augment.WaveAugment: featurize the clips with background noise mixed in, drawn for (its seed, `step`)
        at global batch positions position_base + b (kws_augment_plan + kws_featurize_gather_augmented).  With a RIR bank the clips are
        reverberated first (kws_reverb_apply into a scratch buffer of this featurizer); with a filter bank they are filtered next
        (kws_filter_apply, in place in that scratch); then noised (if it has a noise bank) and featurized from there.  With a speed or
        loudness range the clips are perturbed before all of that (kws_speed_apply into the scratch; into a second buffer when a
        reverberation follows, which does not run in place).  With a tempo or pitch range the clips go through the phase vocoder first
        of all (kws_pitch_apply into a scratch buffer of its own when another of these stages follows; its workspace is this
        featurizer's too, one per stream)."""
        torch = _torch()
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index, "(B, stride)")
        g = self.geometry
        if out is None:
            out = torch.empty((B, g["n_features"], g["feature_size"]), dtype=torch.float32, device=wav.device)
        elif out.numel() < B * g["n_features"] * g["feature_size"] or not out.is_contiguous():
            raise ValueError("out is too small for %d clips" % B)
        if augment is not None and (augment.vocodes or augment.perturbs or augment.rirs is not None or augment.filters is not None):
            # tempo / pitch, speed / loudness, reverberation, then the filter (in place), into this featurizer's scratch on the call's
            # stream; then noise (or nothing)
            ms = g["max_samples"]
            wet, lens = self._reverb_scratch(B, ms, wav.device), self._reverb_lengths(B, wav.device)
            if augment.vocodes:
                last = not (augment.perturbs or augment.rirs is not None or augment.filters is not None)
                pv, pv_lens = (wet, lens) if last else self._scratch(B, ms, wav.device, "_pv_bufs")
                augment.pitch_perturb(wav, valid_len=valid_len, index=index, step=step, position_base=position_base, max_samples=ms, out=pv,
                                      lengths=pv_lens, tempo_used=False, pitch_used=False,
                                      workspace=self._pitch_workspace(B, ms, augment.pitch_n_fft, wav.device))
                wav, index, valid_len = pv, None, pv_lens
            if augment.perturbs:
                pre, pre_lens = (wet, lens) if augment.rirs is None else self._scratch(B, ms, wav.device, "_sp_bufs")
                augment.perturb(wav, valid_len=valid_len, index=index, step=step, position_base=position_base, max_samples=ms, out=pre,
                                lengths=pre_lens, speed_used=False, gain_used=False)
                wav, index, valid_len = pre, None, pre_lens
            if augment.rirs is not None:
                augment.reverberate(wav, valid_len=valid_len, index=index, step=step, position_base=position_base, max_samples=ms, out=wet,
                                    lengths=lens, rir_used=False)
                wav, index, valid_len = wet, None, lens
            if augment.filters is not None:
                augment.filter(wav, valid_len=valid_len, index=index, step=step, position_base=position_base, max_samples=ms, out=wet,
                               lengths=lens, filter_used=False)
            wav, index, valid_len, stride, ix, vl = wet, None, lens, ms, 0, lens.data_ptr()
            if augment.noise is None:
                augment = None
        if augment is not None:
            plan = augment.plan(wav, valid_len=valid_len, index=index, step=step, position_base=position_base, max_samples=g["max_samples"])
            _l.check(self._L.kws_featurize_gather_augmented(self._h, wav.data_ptr(), self._dtype_code(wav), ix, B, stride,
                                                            augment.noise.handle(), plan.data_ptr(), out.data_ptr(),
                                                            torch.cuda.current_stream().cuda_stream))
            return out
        _l.check(self._L.kws_featurize_gather(self._h, wav.data_ptr(), self._dtype_code(wav), ix, B, stride, vl, out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
        return out

    def _scratch(self, B, ms, device, name):
        """((B, ms) float32 rows, (B,) int32 lengths) of the scratch `name`, one buffer per stream (grown on demand)"""
        torch = _torch()
        key = torch.cuda.current_stream().cuda_stream
        bufs = self.__dict__.setdefault(name, {})
        buf = bufs.get(key)
        if buf is None or buf[0].shape[0] < B or buf[0].shape[1] != ms or buf[0].device != device:
            buf = bufs[key] = (torch.empty((B, ms), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.int32, device=device))
        return buf[0][:B], buf[1][:B]

    def _pitch_workspace(self, B, ms, n_fft, device):
        """the vocoder's workspace for min(B, PITCH_TILE_CLIPS) clips at a time, one per stream (grown on demand)"""
        from .augment import PITCH_TILE_CLIPS, pitch_workspace_bytes
        torch = _torch()
        key = torch.cuda.current_stream().cuda_stream
        need = pitch_workspace_bytes(n_fft, ms, max(1, min(B, PITCH_TILE_CLIPS)))
        bufs = self.__dict__.setdefault("_pv_ws", {})
        ws = bufs.get(key)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = bufs[key] = torch.empty((need,), dtype=torch.uint8, device=device)
        return ws

    def _reverb_scratch(self, B, ms, device):
        """(B, ms) float32 rows the reverberated clips go to"""
        return self._scratch(B, ms, device, "_rv_bufs")[0]

    def _reverb_lengths(self, B, device):
        return self._rv_bufs[_torch().cuda.current_stream().cuda_stream][1][:B]

    def raw(self, wav, n_samples=None):
        """vectorize_raw semantics: (B, n) -> (B, n_frames, n_mfcc), no padding / clipping / deltas."""
        torch = _torch()
        if not wav.is_cuda or wav.dim() != 2 or not wav.is_contiguous():
            raise ValueError("wav must be a contiguous CUDA tensor of shape (B, n)")
        B, stride = wav.shape
        n = stride if n_samples is None else int(n_samples)
        nf = self._L.kws_featurize_raw_frames(self._h, n)
        out = torch.empty((B, nf, self.n_mfcc), dtype=torch.float32, device=wav.device)
        if nf:
            _l.check(self._L.kws_featurize_raw(self._h, wav.data_ptr(), self._dtype_code(wav), B, stride, n,
                                               out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return out
