"""ctypes bindings of include/kws.h."""
import ctypes
import os

from .build import LIB_PATH


ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM, ERR_WORKSPACE, ERR_COMM = -1, -2, -3, -4, -5, -6   # include/kws.h


class KwsError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("kws error %d: %s" % (code, message))
        self.code = code


class KwsParams(ctypes.Structure):
    _fields_ = [("buffer_t", ctypes.c_double), ("window_t", ctypes.c_double), ("hop_t", ctypes.c_double),
                ("sample_rate", ctypes.c_int32), ("sample_depth", ctypes.c_int32), ("n_fft", ctypes.c_int32),
                ("n_filt", ctypes.c_int32), ("n_mfcc", ctypes.c_int32), ("use_delta", ctypes.c_int32)]


class KwsGeometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("window_samples", "hop_samples", "max_samples", "buffer_samples", "n_features", "feature_size")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KwsTensorInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("ndim", ctypes.c_int32), ("shape", ctypes.c_int32 * 4),
                ("trainable", ctypes.c_int32), ("offset", ctypes.c_int64), ("size", ctypes.c_int64)]


OVERLAP_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p)     # kws_train_args.overlap_callback


class KwsTrainArgs(ctypes.Structure):
    _fields_ = [("feat", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("class_weights", ctypes.c_void_p),
                ("B", ctypes.c_int32), ("ignore_index", ctypes.c_int32), ("params", ctypes.c_void_p),
                ("state", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("ws", ctypes.c_void_p),
                ("ws_bytes", ctypes.c_size_t), ("dropout_seed", ctypes.c_uint64), ("grad_scale", ctypes.c_float),
                ("probs", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("bucket_event", ctypes.c_void_p),
                ("forward_event", ctypes.c_void_p), ("overlap_event", ctypes.c_void_p),
                ("overlap_callback", OVERLAP_CB), ("overlap_user", ctypes.c_void_p), ("comm", ctypes.c_void_p),
                ("comm_state_weight", ctypes.c_float), ("feat_moments", ctypes.c_void_p)]


OPT_KINDS = {"sgd": 0, "rmsprop": 1, "adam": 2}                                          # include/kws.h KWS_OPT_*
OPT_NESTEROV, OPT_CENTERED, OPT_AMSGRAD = 1, 2, 4
AVG_NONE, AVG_BLEND, AVG_SYNC = 0, 1, 2                                                  # include/kws.h KWS_AVG_*


class KwsOptimizerArgs(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("flags", ctypes.c_int32), ("params", ctypes.c_void_p), ("grads", ctypes.c_void_p),
                ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("vhat", ctypes.c_void_p), ("mg", ctypes.c_void_p),
                ("mom", ctypes.c_void_p), ("ws", ctypes.c_void_p), ("ws_bytes", ctypes.c_int64), ("n_blocks", ctypes.c_int32),
                ("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("momentum", ctypes.c_float), ("t", ctypes.c_int64), ("grad_scale", ctypes.c_float), ("clipvalue", ctypes.c_float),
                ("clipnorm", ctypes.c_float), ("global_clipnorm", ctypes.c_float), ("avg", ctypes.c_void_p),
                ("avg_mode", ctypes.c_int32), ("avg_alpha", ctypes.c_float)]


class KwsHeadJob(ctypes.Structure):
    """kws_head_job: one head of a kws_head_fit launch (include/kws.h); 80 bytes"""
    _fields_ = [("order_offset", ctypes.c_int64), ("weight_offset", ctypes.c_int64), ("class_weight_offset", ctypes.c_int64),
                ("t0", ctypes.c_int64), ("n_order", ctypes.c_int32), ("batch", ctypes.c_int32), ("num_classes", ctypes.c_int32),
                ("ignore_index", ctypes.c_int32), ("optimizer", ctypes.c_int32), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("momentum", ctypes.c_float), ("reserved", ctypes.c_int32 * 2)]


AUG_MAX_SNR = 16
AUG_MAX_SNR_DB = 200.0    # kws_augment_plan refuses SNRs outside [-200, 200] dB (include/kws.h)


class KwsAugmentParams(ctypes.Structure):
    _fields_ = [("noised_rate", ctypes.c_float), ("n_snr", ctypes.c_int32), ("snr_db", ctypes.c_float * AUG_MAX_SNR),
                ("max_shift", ctypes.c_int32), ("max_samples", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class KwsAugClip(ctypes.Structure):
    _fields_ = [("apply", ctypes.c_int32), ("segment", ctypes.c_int32), ("offset", ctypes.c_int32), ("shift", ctypes.c_int32),
                ("length", ctypes.c_int32), ("snr_db", ctypes.c_float), ("gain", ctypes.c_float), ("voice_length", ctypes.c_int32)]


class KwsSynthParams(ctypes.Structure):
    _fields_ = [("gap_lo", ctypes.c_int32), ("gap_hi", ctypes.c_int32), ("lead_in", ctypes.c_int32), ("clip_cap", ctypes.c_int32),
                ("n_snr", ctypes.c_int32), ("snr_db", ctypes.c_float * AUG_MAX_SNR), ("bed_gain_lo", ctypes.c_float),
                ("bed_gain_hi", ctypes.c_float), ("max_gain", ctypes.c_float), ("fade", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("seed", ctypes.c_uint64)]


class KwsReverbParams(ctypes.Structure):
    _fields_ = [("reverb_rate", ctypes.c_float), ("rescale", ctypes.c_int32), ("max_samples", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64)]


REVERB_MAX_SAMPLES = 16384


class KwsFilterParams(ctypes.Structure):
    _fields_ = [("filter_rate", ctypes.c_float), ("rescale", ctypes.c_int32), ("max_samples", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64)]


FILTER_MAX_SECTIONS = 4
FILTER_MAX_PADLEN = 32
FILTER_MAX_SAMPLES = 16320


class KwsSpeedParams(ctypes.Structure):
    _fields_ = [("speed_rate", ctypes.c_float), ("speed_lo", ctypes.c_float), ("speed_hi", ctypes.c_float),
                ("loud_rate", ctypes.c_float), ("loud_lo_db", ctypes.c_float), ("loud_hi_db", ctypes.c_float),
                ("max_samples", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class KwsPitchParams(ctypes.Structure):
    _fields_ = [("tempo_rate", ctypes.c_float), ("tempo_lo", ctypes.c_float), ("tempo_hi", ctypes.c_float),
                ("pitch_rate", ctypes.c_float), ("pitch_lo", ctypes.c_float), ("pitch_hi", ctypes.c_float),
                ("n_fft", ctypes.c_int32), ("max_samples", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64)]


PITCH_N_FFT = (256, 512, 1024)
PITCH_MAX_SAMPLES = 1 << 20


FMASK_MAX = 4
FMASK_FILL = {"zero": 0, "mean": 1}                                                      # include/kws.h KWS_FMASK_*


class KwsFeatureMaskParams(ctypes.Structure):
    _fields_ = [("rate", ctypes.c_float), ("n_time", ctypes.c_int32), ("max_time_width", ctypes.c_int32), ("n_freq", ctypes.c_int32),
                ("max_freq_width", ctypes.c_int32), ("max_warp", ctypes.c_int32), ("fill", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("seed", ctypes.c_uint64)]


class KwsFmaskClip(ctypes.Structure):
    _fields_ = [("apply", ctypes.c_int32), ("warp_center", ctypes.c_int32), ("warp_shift", ctypes.c_int32), ("n_time", ctypes.c_int32),
                ("n_freq", ctypes.c_int32), ("t0", ctypes.c_int32 * FMASK_MAX), ("tw", ctypes.c_int32 * FMASK_MAX),
                ("f0", ctypes.c_int32 * FMASK_MAX), ("fw", ctypes.c_int32 * FMASK_MAX)]


QUANT_TENSORS = 6
QUANT_MAX_CLASSES = 48
QUANT_MAX, QUANT_RELU6, QUANT_KL = 0, 1, 2
# the methods that turn bare calibrated maxima into ranges; "kl" needs histograms (kws_amd.quant.calibrate_kl / from_histograms)
QUANT_METHODS = {"max": QUANT_MAX, "relu6": QUANT_RELU6}
# every method a quantized snapshot may record (its `method` field, the .npz __meta__)
QUANT_SNAPSHOT_METHODS = {"max": QUANT_MAX, "relu6": QUANT_RELU6, "kl": QUANT_KL}
QUANT_HIST_BINS = 2048


class KwsQSimpleCnn(ctypes.Structure):
    """kws_qsimple_cnn: the int8 simple_cnn on the host (include/kws.h)"""
    _fields_ = [("num_classes", ctypes.c_int32), ("method", ctypes.c_int32), ("inv_s0", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("amax", ctypes.c_double * QUANT_TENSORS), ("scale", ctypes.c_double * QUANT_TENSORS),
                ("conv_w1", ctypes.c_int8 * (9 * 16)), ("conv_w2", ctypes.c_int8 * (9 * 16 * 32)),
                ("conv_w3", ctypes.c_int8 * (9 * 32 * 64)), ("conv_w4", ctypes.c_int8 * (9 * 64 * 128)),
                ("dense_w", ctypes.c_int8 * (256 * 128)), ("head_w", ctypes.c_int8 * (128 * QUANT_MAX_CLASSES)),
                ("M1", ctypes.c_float * 16), ("B1", ctypes.c_float * 16), ("M2", ctypes.c_float * 32), ("B2", ctypes.c_float * 32),
                ("M3", ctypes.c_float * 64), ("B3", ctypes.c_float * 64), ("M4", ctypes.c_float * 128), ("B4", ctypes.c_float * 128),
                ("Md", ctypes.c_float * 128), ("Bd", ctypes.c_float * 128),
                ("Mh", ctypes.c_float * QUANT_MAX_CLASSES), ("head_bias", ctypes.c_float * QUANT_MAX_CLASSES)]


QLITE_TENSORS = 10


class KwsQSimpleCnnLite(ctypes.Structure):
    """kws_qsimple_cnn_lite: the int8 simple_cnn_lite on the host (include/kws.h)"""
    _fields_ = [("num_classes", ctypes.c_int32), ("method", ctypes.c_int32), ("inv_s0", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("amax", ctypes.c_double * QLITE_TENSORS), ("scale", ctypes.c_double * QLITE_TENSORS),
                ("dw_w1", ctypes.c_int8 * 9), ("dw_w2", ctypes.c_int8 * (9 * 16)), ("dw_w3", ctypes.c_int8 * (9 * 32)),
                ("dw_w4", ctypes.c_int8 * (9 * 64)),
                ("pw_w1", ctypes.c_int8 * 16), ("pw_w2", ctypes.c_int8 * (16 * 32)), ("pw_w3", ctypes.c_int8 * (32 * 64)),
                ("pw_w4", ctypes.c_int8 * (64 * 128)),
                ("dense_w", ctypes.c_int8 * (256 * 128)), ("head_w", ctypes.c_int8 * (128 * QUANT_MAX_CLASSES)),
                ("bq1", ctypes.c_int32 * 16), ("bq2", ctypes.c_int32 * 32), ("bq3", ctypes.c_int32 * 64), ("bq4", ctypes.c_int32 * 128),
                ("Mu1", ctypes.c_float * 1), ("Mu2", ctypes.c_float * 16), ("Mu3", ctypes.c_float * 32), ("Mu4", ctypes.c_float * 64),
                ("M1", ctypes.c_float * 16), ("B1", ctypes.c_float * 16), ("M2", ctypes.c_float * 32), ("B2", ctypes.c_float * 32),
                ("M3", ctypes.c_float * 64), ("B3", ctypes.c_float * 64), ("M4", ctypes.c_float * 128), ("B4", ctypes.c_float * 128),
                ("Md", ctypes.c_float * 128), ("Bd", ctypes.c_float * 128),
                ("Mh", ctypes.c_float * QUANT_MAX_CLASSES), ("head_bias", ctypes.c_float * QUANT_MAX_CLASSES)]


QUANT_DYNAMIC = 3               # the dynamic-range int8 of simple_gru / simple_lstm (no calibration)
QRNN_MAX_STEPS, QRNN_MAX_FEATURES, QRNN_UNITS = 128, 64, 48


class KwsQSimpleRnn(ctypes.Structure):
    """kws_qsimple_rnn: the dynamic-range int8 simple_gru / simple_lstm on the host (include/kws.h)"""
    _fields_ = [("kind", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("feature_size", ctypes.c_int32),
                ("method", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("kernel", ctypes.c_int8 * (QRNN_MAX_FEATURES * 4 * QRNN_UNITS)),
                ("recurrent_kernel", ctypes.c_int8 * (QRNN_UNITS * 4 * QRNN_UNITS)),
                ("head_w", ctypes.c_int8 * (QRNN_UNITS * QUANT_MAX_CLASSES)),
                ("kernel_scale", ctypes.c_float * (4 * QRNN_UNITS)), ("recurrent_scale", ctypes.c_float * (4 * QRNN_UNITS)),
                ("bias", ctypes.c_float * (8 * QRNN_UNITS)),
                ("head_scale", ctypes.c_float * QUANT_MAX_CLASSES), ("head_bias", ctypes.c_float * QUANT_MAX_CLASSES)]


MODEL_KINDS = {"simple_cnn": 0, "simple_cnn_lite": 1, "simple_gru": 2, "simple_lstm": 3}
BANK_MEL, BANK_BARK = 0, 1
WAV_F32, WAV_I16 = 0, 1
RAW_F64, RAW_F32 = 0, 1
VAD_ALIGN = {"left": 0, "center": 1}                                                    # include/kws.h KWS_VAD_ALIGN_*
DET_UNLABELLED, DET_HIT, DET_DUPLICATE, DET_FALSE_ALARM = 0, 1, 2, 3                     # include/kws.h KWS_DET_*
RAGGED_SLOT, RAGGED_CARRY, RAGGED_LEN, RAGGED_NEW, RAGGED_RESET, RAGGED_FIELDS = 0, 1, 2, 3, 4, 8   # include/kws.h KWS_RAGGED_*
# include/kws.h KWS_RATE_*
(RATE_BANK, RATE_IN_ROW, RATE_IN_LEN, RATE_N_LO, RATE_N_HI, RATE_OUT_ROW, RATE_FIRST_LO, RATE_FIRST_HI, RATE_COUNT, RATE_HIST_IN,
 RATE_HIST_OUT, RATE_FLAGS, RATE_FIELDS) = range(13)
RATE_RESTART, RATE_FINAL = 1, 2
RATE_MAX_BANKS = 16
HEADS_MAX_CLASSES, HEADS_TILE_ROWS = 256, 16                                            # include/kws.h KWS_HEADS_*
KNN_MAX_K = 64
KNN_METRICS = {"dot": 0, "l2": 1}                                                       # include/kws.h KWS_KNN_*
DTW_MAX_ROWS, DTW_MAX_HITS, DTW_MAX_Q = 64, 64, 1024
DTW_METRICS = {"dot": 0, "l2": 1}                                                       # include/kws.h KWS_DTW_*

_lib = None


def get_lib():
    """Load libkws_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libkws_hip.so is missing at %s: build it with `python -m kws_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch ships its own libamdhip64 and the host side of this package uses torch for device memory and
    # streams, so torch is loaded FIRST and libkws_hip.so binds to the runtime it brought.  Loaded the other way round (this library, then
    # torch) the process holds two runtimes and the second one sees no device (__graft_entry__: build() followed by smoke() in one process).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass                    # a torch-free host (tests of the C ABI alone): the system runtime the library links against
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    L.kws_version.restype = ctypes.c_char_p
    L.kws_last_error.restype = ctypes.c_char_p
    L.kws_build_id.restype = ctypes.c_char_p
    L.kws_device_count.restype = i32
    L.kws_params_default.argtypes = [ctypes.POINTER(KwsParams)]
    L.kws_params_default.restype = None
    L.kws_params_derive.argtypes = [ctypes.POINTER(KwsParams), ctypes.POINTER(KwsGeometry)]
    L.kws_featurizer_create.argtypes = [ctypes.POINTER(KwsParams), i32, ctypes.POINTER(vp)]
    L.kws_featurizer_destroy.argtypes = [vp]
    L.kws_featurizer_destroy.restype = None
    L.kws_featurizer_geometry.argtypes = [vp, ctypes.POINTER(KwsGeometry)]
    L.kws_featurizer_bank.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t]
    L.kws_featurize.argtypes = [vp, vp, i32, i32, i64, vp, fp, vp]
    L.kws_featurize_gather.argtypes = [vp, vp, i32, vp, i32, i64, vp, fp, vp]
    L.kws_featurizer_set_cu_share.argtypes = [vp, i32]
    L.kws_featurize_raw.argtypes = [vp, vp, i32, i32, i64, i32, fp, vp]
    L.kws_featurize_long.argtypes = [vp, vp, i32, i32, i64, vp, i32, fp, vp]
    u64, f32 = ctypes.c_uint64, ctypes.c_float
    L.kws_model_create.argtypes = [i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.kws_model_create_stacked.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.kws_model_num_layers.argtypes = [vp]
    L.kws_model_destroy.argtypes = [vp]
    L.kws_model_destroy.restype = None
    for n in ("kws_model_param_count", "kws_model_state_count"):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = i64
    L.kws_model_num_tensors.argtypes = [vp]
    L.kws_model_tensor_info.argtypes = [vp, i32, ctypes.POINTER(KwsTensorInfo)]
    L.kws_model_workspace_bytes.argtypes = [vp, i32, i32]
    L.kws_model_workspace_bytes.restype = i64
    L.kws_model_forward.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.c_size_t, vp, vp, vp]
    L.kws_model_train_fwd_bwd.argtypes = [vp, ctypes.POINTER(KwsTrainArgs), vp]
    L.kws_model_bind_device.argtypes = [vp]
    L.kws_model_prepare_inference.argtypes = [vp, i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.kws_model_invalidate_prepared.argtypes = [vp]
    L.kws_feature_moments_workspace_bytes.argtypes = [i32]
    L.kws_feature_moments_workspace_bytes.restype = i64
    L.kws_feature_moments.argtypes = [vp, i32, i32, i32, vp, vp, ctypes.c_size_t, vp]
    L.kws_model_grad_split.argtypes = [vp]
    L.kws_model_grad_split.restype = i64
    L.kws_loss_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.kws_confusion_counts.argtypes = [vp, vp, i32, i32, vp, vp]
    L.kws_score_hist_uses_lds.argtypes = [i32, i32]
    L.kws_score_hist.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.kws_sgd_step.argtypes = [vp, vp, i64, f32, f32, vp]
    L.kws_rmsprop_step.argtypes = [vp, vp, vp, i64, f32, f32, f32, f32, vp]
    L.kws_adam_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, f32, vp]
    L.kws_optimizer_workspace_bytes.argtypes = [ctypes.POINTER(i64), ctypes.POINTER(i64), i32]
    L.kws_optimizer_workspace_bytes.restype = i64
    L.kws_optimizer_plan.argtypes = [ctypes.POINTER(i64), ctypes.POINTER(i64), i32, vp, i64, ctypes.POINTER(ctypes.c_int32)]
    L.kws_optimizer_step.argtypes = [ctypes.POINTER(KwsOptimizerArgs), vp]
    L.kws_optimizer_swap.argtypes = [vp, vp, vp, i64, i32, vp]
    f64 = ctypes.c_double
    L.kws_featurizer_occupancy.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_size_t)]
    L.kws_decoder_create.argtypes = [ctypes.POINTER(f64), i32, f64, i32, f64, f64, ctypes.POINTER(vp)]
    L.kws_decoder_destroy.argtypes = [vp]
    L.kws_decoder_destroy.restype = None
    L.kws_decoder_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]
    L.kws_decoder_table.argtypes = [vp, ctypes.POINTER(f64), ctypes.c_size_t]
    L.kws_decoder_decode.argtypes = [vp, vp, i32, vp, i64, vp]
    L.kws_decoder_encode.argtypes = [vp, f64, ctypes.POINTER(f64)]
    L.kws_stream_push_rows.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.kws_trigger_update.argtypes = [vp, vp, i32, i32, f64, i32, i32, vp, vp, vp]
    L.kws_stream_postprocess.argtypes = [vp, vp, i32, i32, i32, f64, i32, i32, vp, vp, vp, vp, vp]
    L.kws_stream_ragged_append.argtypes = [vp, i64, i32, i32, vp, i64, vp, i32, i32, i32, i32, vp, i64, vp, vp]
    L.kws_stream_ragged_push_rows.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, fp, vp]
    L.kws_stream_ragged_postprocess.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kws_rate_bank_create.argtypes = [i32, i32, i32, ctypes.c_double, ctypes.c_double, ctypes.POINTER(vp)]
    L.kws_rate_bank_destroy.argtypes = [vp]
    L.kws_rate_bank_destroy.restype = None
    L.kws_rate_bank_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.kws_rate_bank_weights.argtypes = [vp, vp, ctypes.c_size_t]
    L.kws_rate_counts.argtypes = [vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kws_rate_convert.argtypes = [ctypes.POINTER(vp), i32, vp, i64, i32, vp, i32, vp, i64, i32, vp, fp, i64, i32, i32, vp]
    L.kws_stream_gather_windows.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, i32, i64, i32, fp, vp]
    L.kws_stream_scan_postprocess.argtypes = [vp, vp, i32, i32, i32, vp, i64, i32, f64, i32, i32, vp, vp, vp, vp, i64, vp]
    L.kws_stream_sweep.argtypes = [vp, vp, i32, i64, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.kws_stream_collect.argtypes = [vp, vp, i32, i64, vp, i32, i32, f64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.kws_stream_peaks.argtypes = [vp, vp, i32, i64, vp, i32, f64, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.kws_set_matrix_precision.argtypes = [i32]
    L.kws_get_matrix_precision.restype = i32
    L.kws_set_inference_precision.argtypes = [i32]
    L.kws_get_inference_precision.restype = i32
    L.kws_model_set_precision.argtypes = [vp, i32, i32]
    L.kws_model_get_precision.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.kws_model_set_deterministic.argtypes = [vp, i32]
    L.kws_model_set_overlap_point.argtypes = [vp, i32]
    L.kws_comm_unique_id.argtypes = [vp]
    L.kws_comm_init.argtypes = [i32, i32, vp, ctypes.POINTER(vp)]
    L.kws_comm_destroy.argtypes = [vp]
    L.kws_comm_destroy.restype = None
    L.kws_comm_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.kws_allreduce_grads.argtypes = [vp, vp, i64, i64, vp, i64, f32, vp]
    L.kws_comm_allreduce.argtypes = [vp, vp, i64, i32, i32, vp]
    L.kws_comm_broadcast.argtypes = [vp, vp, i64, i32, vp]
    L.kws_comm_timing.argtypes = [vp, i32]
    L.kws_comm_last_us.argtypes = [vp, ctypes.POINTER(f32), ctypes.POINTER(f32)]
    L.kws_prof_enable.argtypes = [i32]
    L.kws_prof_report.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.kws_prof_report.restype = i64
    L.kws_noise_bank_create.argtypes = [vp, i32, vp, i32, ctypes.POINTER(vp)]
    L.kws_noise_bank_destroy.argtypes = [vp]
    L.kws_noise_bank_destroy.restype = None
    L.kws_noise_bank_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), vp]
    L.kws_augment_plan.argtypes = [vp, ctypes.POINTER(KwsAugmentParams), vp, i32, vp, i32, i64, vp, i64, i64, vp, vp, vp]
    L.kws_augment_apply.argtypes = [vp, vp, vp, i32, vp, i32, i64, i32, vp, i64, vp, vp]
    L.kws_featurize_gather_augmented.argtypes = [vp, vp, i32, vp, i32, i64, vp, vp, fp, vp]
    L.kws_rir_bank_create.argtypes = [vp, vp, i32, i32, ctypes.POINTER(vp)]
    L.kws_rir_bank_destroy.argtypes = [vp]
    L.kws_rir_bank_destroy.restype = None
    L.kws_rir_bank_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.kws_reverb_apply.argtypes = [vp, ctypes.POINTER(KwsReverbParams), vp, i32, vp, i32, i64, vp, i64, i64, vp, vp, i64, vp, vp, vp]
    L.kws_filter_bank_create.argtypes = [vp, i32, vp, i32, ctypes.POINTER(vp)]
    L.kws_filter_bank_destroy.argtypes = [vp]
    L.kws_filter_bank_destroy.restype = None
    L.kws_filter_bank_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.kws_filter_apply.argtypes = [vp, ctypes.POINTER(KwsFilterParams), vp, i32, vp, i32, i64, vp, i64, i64, vp, vp, i64, vp, vp, vp]
    L.kws_resampler_create.argtypes = [i32, i32, f64, f64, ctypes.POINTER(vp)]
    L.kws_resampler_destroy.argtypes = [vp]
    L.kws_resampler_destroy.restype = None
    L.kws_resampler_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(f64), ctypes.POINTER(f64)]
    L.kws_resampler_table.argtypes = [vp, vp, ctypes.c_size_t]
    L.kws_speed_apply.argtypes = [vp, ctypes.POINTER(KwsSpeedParams), vp, i32, vp, i32, i64, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp]
    L.kws_pitch_workspace_bytes.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    L.kws_pitch_stft.argtypes = [vp, i32, vp, i32, i64, vp, i32, vp, i32, vp]
    L.kws_pitch_apply.argtypes = [vp, ctypes.POINTER(KwsPitchParams), vp, i32, vp, i32, i64, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp,
                                  ctypes.c_size_t, vp]
    L.kws_feature_mask_draw.argtypes = [ctypes.POINTER(KwsFeatureMaskParams), i32, i32, i64, i64, ctypes.POINTER(KwsFmaskClip)]
    L.kws_feature_mask.argtypes = [ctypes.POINTER(KwsFeatureMaskParams), vp, vp, i32, i32, i32, i64, i64, vp, vp, vp]
    L.kws_feature_mask_max_clip.restype = i64
    L.kws_model_calibrate.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.c_size_t, vp, vp]
    L.kws_quantize_simple_cnn.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(KwsQSimpleCnn)]
    L.kws_qmodel_create.argtypes = [vp, ctypes.POINTER(KwsQSimpleCnn), ctypes.POINTER(vp)]
    L.kws_qmodel_destroy.argtypes = [vp]
    L.kws_qmodel_destroy.restype = None
    L.kws_qmodel_workspace_bytes.argtypes = [vp, i32]
    L.kws_qmodel_workspace_bytes.restype = i64
    L.kws_qmodel_forward.argtypes = [vp, vp, i32, vp, ctypes.c_size_t, vp, vp, vp, vp]
    L.kws_model_calibrate_lite.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.c_size_t, vp, vp]
    L.kws_quantize_simple_cnn_lite.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(KwsQSimpleCnnLite)]
    L.kws_qmodel_create_lite.argtypes = [vp, ctypes.POINTER(KwsQSimpleCnnLite), ctypes.POINTER(vp)]
    L.kws_model_calibrate_hist.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.c_size_t, vp, vp, vp]
    L.kws_quant_kl_ranges.argtypes = [vp, vp, i32, vp, vp]
    L.kws_quantize_simple_rnn.argtypes = [vp, vp, ctypes.POINTER(KwsQSimpleRnn)]
    L.kws_qmodel_create_rnn.argtypes = [vp, ctypes.POINTER(KwsQSimpleRnn), ctypes.POINTER(vp)]
    f64 = ctypes.c_double
    L.kws_vad_create.argtypes = [i32, f64, f64, f64, f64, f64, f64, ctypes.POINTER(vp)]
    L.kws_vad_destroy.argtypes = [vp]
    L.kws_vad_destroy.restype = None
    L.kws_vad_info.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int32)] * 5
    L.kws_vad_windows.argtypes = [vp, i64]
    L.kws_vad_windows.restype = i64
    L.kws_vad_workspace_bytes.argtypes = [vp, i32, i32]
    L.kws_vad_workspace_bytes.restype = i64
    L.kws_vad_detect.argtypes = [vp, vp, i32, i32, i64, vp, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.kws_vad_gather_clips.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    L.kws_synth_plan.argtypes = [vp, ctypes.POINTER(KwsSynthParams), vp, i32, i32, i64, vp, vp, i32, vp, i32, i32, i64, vp, vp, vp]
    L.kws_synth_render.argtypes = [vp, vp, i32, i32, i64, vp, vp, i32, vp, i32, i64, i32, vp, i32, i64, vp]
    L.kws_model_embed_size.argtypes = [vp]
    L.kws_model_embed.argtypes = [vp, vp, i32, vp, vp, vp, ctypes.c_size_t, vp, vp]
    L.kws_head_fit_max_classes.argtypes = [i32]
    L.kws_head_fit.argtypes = [vp, vp, i64, i32, vp, vp, ctypes.POINTER(KwsHeadJob), vp, i32, vp, vp, vp, vp, vp]
    L.kws_heads_apply.argtypes = [vp, i64, i32, vp, vp, i64, vp, i64, i64, vp, i64, vp, vp, i32, i32, vp, vp, vp, vp]
    L.kws_rows_normalize.argtypes = [vp, i64, i32, vp, vp, vp]
    L.kws_knn_workspace_bytes.argtypes = [i64, i64, i32, i32, i32]
    L.kws_knn_workspace_bytes.restype = i64
    L.kws_knn.argtypes = [vp, i64, vp, i64, i32, i32, i32, vp, i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.kws_knn_vote.argtypes = [vp, vp, i64, i32, vp, i64, i32, i32, vp, vp, vp, vp, vp]
    L.kws_dtw_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    L.kws_dtw_workspace_bytes.restype = i64
    L.kws_dtw.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.kws_dtw_peaks.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, f32, i32, i32, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise KwsError(rc, get_lib().kws_last_error().decode("utf-8", "replace"))


def version():
    return get_lib().kws_version().decode()


def build_id():
    """{source file: sha1 prefix} the loaded library was built from"""
    out = {}
    for item in get_lib().kws_build_id().decode().split(";"):
        if item:
            k, v = item.split(":")
            out[k] = v
    return out


def device_count():
    return get_lib().kws_device_count()


MATRIX_FP32, MATRIX_BF16X6 = 0, 1
INFER_FP32, INFER_FP16 = 0, 1
FEATURE_MOMENTS = 100
COMM_ID_BYTES = 128
DT_F32, DT_F64, DT_I32, DT_I64 = 0, 1, 2, 3
OP_SUM, OP_MAX, OP_AVG = 0, 1, 2


def set_matrix_precision(mode):
    """Library-wide DEFAULT (a model follows it until DeviceModel.set_precision gives it its own): MATRIX_BF16X6
    (three-way bf16 split on the matrix cores, fp32-level error) or MATRIX_FP32 (exact fp32 MFMA)."""
    check(get_lib().kws_set_matrix_precision(int(mode)))


def get_matrix_precision():
    return get_lib().kws_get_matrix_precision()


def set_inference_precision(mode):
    """INFER_FP32 (default) or INFER_FP16: simple_cnn_lite inference with fp16 activations and matrix operands, fp32
    accumulation (BASELINE configs[4]); other model kinds ignore the switch."""
    check(get_lib().kws_set_inference_precision(int(mode)))


def get_inference_precision():
    return get_lib().kws_get_inference_precision()


def prof_enable(on=True):
    check(get_lib().kws_prof_enable(1 if on else 0))


def prof_report():
    """{kernel name: {"count": n, "total_ms": t}} for the launches since prof_enable(True)"""
    import json
    L = get_lib()
    n = L.kws_prof_report(None, 0)
    buf = ctypes.create_string_buffer(int(n) + 16)
    L.kws_prof_report(buf, len(buf))
    return json.loads(buf.value.decode())
