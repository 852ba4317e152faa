#!/usr/bin/env python3
"""Train a keyword-spotting model on your own dataset (mirror of the reference's train.py:22-137 for the native runtime).

Same flags, callbacks and flow as the reference: features from get_dataset, Adam / RMSprop / SGD with the optional decay schedule,
(weighted) sparse cross entropy, checkpoints on the best val_accuracy.  Checkpoints are .npz files (KWSModel.save: Keras-ordered arrays;
HDF5 needs h5py) and the TensorBoard scalars become one JSON line per epoch (logs/000/train_log.jsonl).

Beyond the reference: --raw_audio trains on the waveforms (get_audio_dataset; every batch is featurized on the GPU inside the step
pipeline), and --noise_path mixes background noise into every training clip afresh in every epoch, with the knobs of the reference's
offline tool tools/audio_process/add_noise.py (--snr, --noised_rate) and an optional random time shift (--time_shift_ms).  --rir_path
(a folder of room impulse responses) or --simulate_rirs N (N simulated rooms) reverberates a --reverb_rate share of the training clips
before the noise, as tools/audio_process/audio_reverberation.py does offline; either works without --noise_path.  --filter_rate filters
that share of the training clips at zero phase with a Butterworth design drawn from a bank of --num_filters random ones
(--filter_types, --filter_order), after the room and before the noise, as tools/audio_process/wav_filter.py does offline.
--speed_range LO,HI plays a --speed_rate share of the training clips at a ratio drawn from the range (tempo and pitch together) and
--loudness_range LO_DB,HI_DB sets a --loudness_rate share to a level drawn from the range (dBFS), before every other stage, as
tools/audio_process/audio_convert.py resamples and levels files offline.
--tempo_range LO,HI stretches a --tempo_rate share of the training clips in time without changing their pitch and --pitch_range LO,HI
shifts a --pitch_rate share by that many semitones without changing their duration (a phase vocoder, before the speed change).
--time_mask N,W / --freq_mask N,W / --time_warp W are SpecAugment of the features (--mask_rate, --mask_fill), drawn per clip and per
step behind the featurizer or the cached features: they work with and without --raw_audio.
The optimizer takes the Keras options the reference's command line leaves at their defaults: --clipnorm, --global_clipnorm and
--clipvalue (any optimizer), --momentum (sgd, rmsprop), --nesterov (sgd), --centered (rmsprop) and --amsgrad (adam).
--average_type wraps the optimizer as the reference's get_averaged_optimizer does: ema and swa keep an average of the weights on the
GPU, which is what gets validated, checkpointed and written as trained_final; lookahead changes the trained weights themselves.
--freeze_backbone (with --weights_path, also a checkpoint of another class count) keeps every layer but the softmax layer fixed and
trains that layer alone on embeddings computed once, one kernel launch per epoch (kws_amd.transfer; adam or sgd only)."""
import argparse
import os
import sys

import numpy as np

sys.path.append(os.path.dirname(os.path.realpath(__file__)))


def main(argv=None):
    args = parse_args(argv)
    from classifier.data import get_audio_dataset, get_dataset
    from classifier.loss import SparseCategoricalCrossEntropy, WeightedSparseCategoricalCrossEntropy
    from classifier.model import get_model
    from classifier.params import inject_params
    from common.callbacks import (AverageModelCheckpoint, CheckpointCleanCallBack, EarlyStopping, JsonlLogger, ModelCheckpoint,
                                  ReduceLROnPlateau, TerminateOnNaN)
    from common.model_utils import get_averaged_optimizer, get_optimizer
    from common.utils import get_classes

    log_dir = args.log_dir
    os.makedirs(log_dir, exist_ok=True)
    class_names = get_classes(args.classes_path)
    assert class_names[0] == 'background', '1st class should be background.'
    num_classes = len(class_names)
    if args.noise_path and not args.raw_audio:
        raise SystemExit('--noise_path needs --raw_audio (the noise is mixed into the waveforms before featurization)')
    has_rirs = bool(args.rir_path) or bool(args.simulate_rirs)
    if args.rir_path and args.simulate_rirs:
        raise SystemExit('give one RIR source: --rir_path or --simulate_rirs')
    if args.reverb_rate is not None and not has_rirs:
        raise SystemExit('--reverb_rate needs a RIR source: --rir_path or --simulate_rirs')
    if has_rirs and not args.raw_audio:
        raise SystemExit('--rir_path / --simulate_rirs need --raw_audio (the waveforms are reverberated before featurization)')
    if args.simulate_rirs is not None and args.simulate_rirs < 1:
        raise SystemExit('--simulate_rirs needs a positive number of rooms')
    if args.filter_rate is not None and not args.raw_audio:
        raise SystemExit('--filter_rate needs --raw_audio (the waveforms are filtered before featurization)')
    if args.num_filters < 1:
        raise SystemExit('--num_filters needs a positive bank size')
    for flag in ('speed_range', 'speed_rate', 'loudness_range', 'loudness_rate', 'tempo_range', 'tempo_rate', 'pitch_range', 'pitch_rate'):
        if getattr(args, flag) is not None and not args.raw_audio:
            raise SystemExit('--%s needs --raw_audio (the waveforms are perturbed before featurization)' % flag)
    if args.speed_rate is not None and args.speed_range is None:
        raise SystemExit('--speed_rate needs --speed_range')
    if args.loudness_rate is not None and args.loudness_range is None:
        raise SystemExit('--loudness_rate needs --loudness_range')
    if args.tempo_rate is not None and args.tempo_range is None:
        raise SystemExit('--tempo_rate needs --tempo_range')
    if args.pitch_rate is not None and args.pitch_range is None:
        raise SystemExit('--pitch_rate needs --pitch_range')
    perturb = perturb_options(args)
    mask = mask_options(args)
    opt_options = optimizer_options(args)
    freeze_check(args)

    # callbacks for training process
    logging = JsonlLogger(os.path.join(log_dir, 'train_log.jsonl'))
    averaged = args.average_type in ('ema', 'swa')       # the optimizer keeps an average to validate and save; lookahead does not
    checkpoint_path = os.path.join(log_dir, 'ep{epoch:03d}-loss{loss:.3f}-accuracy{accuracy:.3f}-val_loss{val_loss:.3f}-val_accuracy{val_accuracy:.3f}.npz')
    checkpoint_kw = dict(monitor='val_accuracy', mode='max', verbose=1, save_weights_only=False, save_best_only=True, period=1)
    checkpoint = AverageModelCheckpoint(False, checkpoint_path, **checkpoint_kw) if averaged else \
        ModelCheckpoint(checkpoint_path, **checkpoint_kw)
    reduce_lr = ReduceLROnPlateau(monitor='val_accuracy', factor=0.5, mode='max', patience=10, verbose=1, cooldown=0, min_lr=1e-10)
    early_stopping = EarlyStopping(monitor='val_accuracy', min_delta=0, patience=50, verbose=1, mode='max')
    checkpoint_clean = CheckpointCleanCallBack(log_dir, max_keep=5)
    terminate_on_nan = TerminateOnNaN()
    callbacks = [logging, checkpoint, reduce_lr, early_stopping, terminate_on_nan, checkpoint_clean]

    # load & update audio params
    if args.params_path:
        inject_params(args.params_path)

    # get train & val dataset
    len_train = len_val = None
    if args.raw_audio:
        if args.val_data_path:
            x_train, len_train, y_train, _, _, _ = get_audio_dataset(args.train_data_path, class_names)
            x_val, len_val, y_val, _, _, _ = get_audio_dataset(args.val_data_path, class_names)
        else:
            assert args.val_split > 0, 'no val data split.'
            x_train, len_train, y_train, x_val, len_val, y_val = get_audio_dataset(args.train_data_path, class_names, args.val_split)
    elif args.val_data_path:
        x_train, y_train, _, _ = get_dataset(args.train_data_path, class_names)
        x_val, y_val, _, _ = get_dataset(args.val_data_path, class_names)
    else:
        assert args.val_split > 0, 'no val data split.'
        x_train, y_train, x_val, y_val = get_dataset(args.train_data_path, class_names, args.val_split)

    augment = None
    rirs = None
    if has_rirs:
        from kws_amd.augment import RirBank, simulate_rirs
        rirs = RirBank(args.rir_path if args.rir_path else simulate_rirs(args.simulate_rirs))
    reverb_rate = 1.0 if args.reverb_rate is None else args.reverb_rate
    filters = None
    filter_rate = 1.0 if args.filter_rate is None else args.filter_rate
    if args.filter_rate is not None:
        from kws_amd.augment import FilterBank, random_filters
        try:
            filters = FilterBank(random_filters(args.num_filters, types=args.filter_types, order=args.filter_order))
        except ValueError as e:
            raise SystemExit('--filter_types / --filter_order: %s' % e)
    if args.noise_path:
        from kws_amd.augment import NoiseBank, WaveAugment
        augment = WaveAugment(NoiseBank(args.noise_path), snr=args.snr, noised_rate=args.noised_rate, time_shift_ms=args.time_shift_ms,
                              rirs=rirs, reverb_rate=reverb_rate, filters=filters, filter_rate=filter_rate, **perturb)
    elif args.time_shift_ms:
        raise SystemExit('--time_shift_ms is part of the noise augmentation: give --noise_path too')
    elif rirs is not None or filters is not None or perturb:
        from kws_amd.augment import WaveAugment
        augment = WaveAugment(None, rirs=rirs, reverb_rate=reverb_rate, filters=filters, filter_rate=filter_rate, **perturb)

    # SpecAugment of the features: with cached features as well as with --raw_audio
    feature_mask = None
    if mask:
        from kws_amd.augment import FeatureMask
        feature_mask = FeatureMask(**mask)

    # prepare optimizer
    if args.decay_type:
        callbacks.remove(reduce_lr)
    steps_per_epoch = max(1, len(x_train) // args.batch_size)
    decay_steps = steps_per_epoch * args.epochs
    optimizer = get_optimizer(args.optimizer, args.learning_rate, average_type=None, decay_type=args.decay_type, decay_steps=decay_steps,
                              **opt_options)
    optimizer = get_averaged_optimizer(args.average_type, optimizer)

    # prepare loss according to loss type
    if args.background_bias:
        assert args.background_bias > 0 and args.background_bias < 1, 'background bias should between 0 and 1'
        weights = [args.background_bias] + [(1.0 - args.background_bias) / (num_classes - 1)] * (num_classes - 1)
        losses = WeightedSparseCategoricalCrossEntropy(np.array(weights))
    else:
        losses = SparseCategoricalCrossEntropy()

    # get train model
    if args.freeze_backbone:
        # the checkpoint may hold another class count: every tensor of matching name and shape is loaded, the head keeps its initial value
        model = get_model(args.model_type, num_classes, num_layers=args.rnn_layers)
        model.load_weights(args.weights_path, by_name=True, skip_mismatch=True)
        # a checkpoint of the same class count also brought its head: training continues from it; otherwise the head starts afresh
        path = args.weights_path if os.path.exists(args.weights_path) else args.weights_path + '.npz'
        with np.load(path, allow_pickle=False) as z:
            head_loaded = 'score_predict/kernel' in z.files and z['score_predict/kernel'].shape == model.get_weights()[-2].shape
        print('Load backbone weights {} ({}).'.format(args.weights_path, 'with its head' if head_loaded else 'new head'))
    else:
        model = get_model(args.model_type, num_classes, weights_path=args.weights_path, num_layers=args.rnn_layers)
    model.compile(optimizer=optimizer, loss=losses, metrics=['accuracy'])
    model.summary()

    if args.raw_audio:
        # the validation clips are featurized once (never augmented), with their lengths
        from common.data_utils import get_featurizer
        import torch
        x_val = get_featurizer()(torch.from_numpy(x_val).cuda(), torch.from_numpy(len_val).cuda()).cpu().numpy()
    print('Train on {} samples, val on {} samples, with batch size {}.'.format(len(x_train), len(x_val), args.batch_size))
    fit_kw = dict(sample_lengths=len_train, augment=augment) if args.raw_audio else {}
    if averaged:
        fit_kw['validate_averaged'] = True
    if feature_mask is not None:
        fit_kw['feature_mask'] = feature_mask
    if args.freeze_backbone:
        # only score_predict trains: embeddings once (or once per epoch under augmentation), one head-fit launch per epoch
        from kws_amd.transfer import fit_frozen
        history = fit_frozen(model, x_train, y_train, batch_size=args.batch_size, epochs=args.epochs, validation_data=(x_val, y_val),
                             callbacks=callbacks, verbose=1, init='model' if head_loaded else None, **fit_kw)
    else:
        history = model.fit(x_train, y_train, batch_size=args.batch_size, epochs=args.epochs, validation_data=(x_val, y_val),
                            validation_freq=1, callbacks=callbacks, shuffle=True, verbose=1, **fit_kw)

    # Finally store model
    if averaged:
        optimizer.assign_average_vars(model)
    model.save(os.path.join(log_dir, 'trained_final.npz'))
    return history


# the optimizer options beyond the reference's command line, and the optimizers they belong to
OPTIMIZER_FLAGS = {'clipnorm': ('adam', 'rmsprop', 'sgd'), 'global_clipnorm': ('adam', 'rmsprop', 'sgd'),
                   'clipvalue': ('adam', 'rmsprop', 'sgd'), 'momentum': ('rmsprop', 'sgd'), 'nesterov': ('sgd',),
                   'centered': ('rmsprop',), 'amsgrad': ('adam',)}


def optimizer_options(args):
    """keyword arguments of get_optimizer for the optimizer flags given on the command line (none: the reference's optimizer)"""
    kw = {}
    for name, kinds in OPTIMIZER_FLAGS.items():
        value = getattr(args, name)
        if value is None or value is False:
            continue
        if args.optimizer not in kinds:
            raise SystemExit('--%s is an option of %s, not of --optimizer %s' % (name, ' / '.join(kinds), args.optimizer))
        kw[name] = value
    return kw


def freeze_check(args):
    """--freeze_backbone trains score_predict alone (kws_amd.transfer): what its head trainer does not cover is refused here"""
    if not args.freeze_backbone:
        return
    if not args.weights_path:
        raise SystemExit('--freeze_backbone needs --weights_path: the backbone to freeze')
    if args.optimizer == 'rmsprop':
        raise SystemExit('--freeze_backbone trains the head with adam or sgd, not --optimizer rmsprop')
    for flag in ('clipnorm', 'global_clipnorm', 'clipvalue'):
        if getattr(args, flag) is not None:
            raise SystemExit('--freeze_backbone does not clip gradients: drop --%s' % flag)
    if args.nesterov or args.amsgrad:
        raise SystemExit('--freeze_backbone trains the head with plain adam or sgd momentum: drop --nesterov / --amsgrad')
    if args.average_type is not None:
        raise SystemExit('--freeze_backbone does not average weights: drop --average_type')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('--freeze_backbone runs on one GPU: it is not data parallel (WORLD_SIZE > 1)')


def parse_range(flag, text, lo, hi):
    """'LO,HI' -> (LO, HI) with lo <= LO <= HI <= hi"""
    try:
        a, b = (float(x) for x in text.split(','))
    except ValueError:
        raise SystemExit('--%s needs two numbers LO,HI, got %r' % (flag, text))
    if not lo <= a <= b <= hi:
        raise SystemExit('--%s needs %g <= LO <= HI <= %g, got %r' % (flag, lo, hi, text))
    return a, b


def perturb_options(args):
    """keyword arguments of WaveAugment for the speed / loudness / tempo / pitch flags given on the command line (none: no such stage)"""
    kw = {}
    if args.speed_range is not None:
        kw['speed'] = parse_range('speed_range', args.speed_range, 0.5, 2.0)
        kw['speed_rate'] = 1.0 if args.speed_rate is None else args.speed_rate
    if args.loudness_range is not None:
        kw['loudness'] = parse_range('loudness_range', args.loudness_range, -80.0, 0.0)
        kw['loudness_rate'] = 1.0 if args.loudness_rate is None else args.loudness_rate
    if args.tempo_range is not None:
        kw['tempo'] = parse_range('tempo_range', args.tempo_range, 0.5, 2.0)
        kw['tempo_rate'] = 1.0 if args.tempo_rate is None else args.tempo_rate
    if args.pitch_range is not None:
        kw['pitch'] = parse_range('pitch_range', args.pitch_range, -12.0, 12.0)
        kw['pitch_rate'] = 1.0 if args.pitch_rate is None else args.pitch_rate
    for flag in ('speed_rate', 'loudness_rate', 'tempo_rate', 'pitch_rate'):
        if flag in kw and not 0.0 <= kw[flag] <= 1.0:
            raise SystemExit('--%s must be in 0.0~1.0, got %r' % (flag, kw[flag]))
    return kw


def parse_mask(flag, text):
    """'N,W' -> (N, W): N masks of up to W frames or coefficients"""
    try:
        n, w = (int(x) for x in text.split(','))
    except ValueError:
        raise SystemExit('--%s needs two integers N,W, got %r' % (flag, text))
    if not 0 <= n <= 4 or w < 0:
        raise SystemExit('--%s needs 0 <= N <= 4 masks of width W >= 0, got %r' % (flag, text))
    return n, w


def mask_options(args):
    """keyword arguments of FeatureMask for the SpecAugment flags given on the command line (none: no such stage, and no object); a
    kind of mask that is not asked for is off"""
    if args.time_mask is None and args.freq_mask is None and args.time_warp is None:
        for flag in ('mask_rate', 'mask_fill'):
            if getattr(args, flag) is not None:
                raise SystemExit('--%s needs --time_mask, --freq_mask or --time_warp' % flag)
        return {}
    kw = dict(time_masks=0, time_width=0, freq_masks=0, freq_width=0, warp=0, rate=1.0, fill='mean')
    if args.time_mask is not None:
        kw['time_masks'], kw['time_width'] = parse_mask('time_mask', args.time_mask)
    if args.freq_mask is not None:
        kw['freq_masks'], kw['freq_width'] = parse_mask('freq_mask', args.freq_mask)
    if args.time_warp is not None:
        if args.time_warp < 0:
            raise SystemExit('--time_warp needs W >= 0 frames, got %r' % args.time_warp)
        kw['warp'] = args.time_warp
    if args.mask_rate is not None:
        if not 0.0 <= args.mask_rate <= 1.0:
            raise SystemExit('--mask_rate must be in 0.0~1.0, got %r' % args.mask_rate)
        kw['rate'] = args.mask_rate
    if args.mask_fill is not None:
        kw['fill'] = args.mask_fill
    return kw


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='train a keyword-spotting model on the GPU')
    # Model definition options
    parser.add_argument('--model_type', type=str, required=False, default='simple_cnn',
                        help='classifier model type: simple_cnn/simple_cnn_lite/simple_gru/simple_lstm, default=%(default)s')
    parser.add_argument('--rnn_layers', type=int, required=False, default=1,
                        help="recurrent layers of simple_gru / simple_lstm, 1..4 (the reference's num_layers); the CNN types take 1 only, default=%(default)s")
    parser.add_argument('--weights_path', type=str, required=False, default=None,
                        help="Pretrained model/weights file for fine tune (the file holds no optimizer state: with --average_type the "
                             "average starts from the loaded weights)")

    parser.add_argument('--freeze_backbone', action='store_true',
                        help="transfer to the classes of --classes_path: load every matching tensor of --weights_path (a checkpoint of another "
                             "class count works), keep all of it fixed and train only the softmax layer, on embeddings computed once "
                             "(once per epoch under augmentation). adam or sgd (--momentum) only; no clipping, averaging or data parallelism")

    # Data options
    parser.add_argument('--train_data_path', type=str, required=True,
                        help='path to train dataset')
    parser.add_argument('--val_data_path', type=str, required=False, default=None,
                        help='path to val dataset')
    parser.add_argument('--val_split', type=float, required=False, default=0.15,
                        help="validation data persentage in dataset if no val dataset provide, default=%(default)s")
    parser.add_argument('--classes_path', type=str, required=True,
                        help='path to class definitions')
    parser.add_argument('--params_path', type=str, required=False, default=None,
                        help='path to params json file')

    # Training options
    parser.add_argument('--background_bias', type=float, required=False, default=None,
                        help="background loss bias (0~1) when training. lower values may cause more false positives if set, default=%(default)s")
    parser.add_argument('--batch_size', type=int, required=False, default=512,
                        help="Batch size for train, default=%(default)s")
    parser.add_argument('--optimizer', type=str, required=False, default='adam', choices=['adam', 'rmsprop', 'sgd'],
                        help="optimizer for training (adam/rmsprop/sgd), default=%(default)s")
    parser.add_argument('--learning_rate', type=float, required=False, default=1e-3,
                        help="Initial learning rate, default=%(default)s")
    parser.add_argument('--clipnorm', type=float, required=False, default=None,
                        help="clip each variable's gradient to this L2 norm (tf.clip_by_norm), default off")
    parser.add_argument('--global_clipnorm', type=float, required=False, default=None,
                        help="clip the gradient of all variables together to this L2 norm (tf.clip_by_global_norm), default off")
    parser.add_argument('--clipvalue', type=float, required=False, default=None,
                        help="clip every gradient entry to [-clipvalue, clipvalue], default off")
    parser.add_argument('--momentum', type=float, required=False, default=None,
                        help="momentum of sgd / rmsprop, in [0, 1], default 0")
    parser.add_argument('--nesterov', action='store_true', help="Nesterov momentum (sgd)")
    parser.add_argument('--centered', action='store_true', help="centered RMSprop (rmsprop)")
    parser.add_argument('--amsgrad', action='store_true', help="the AMSGrad variant of Adam (adam)")
    parser.add_argument('--average_type', type=str, required=False, default=None, choices=[None, 'ema', 'swa', 'lookahead'],
                        help="weights average type: ema keeps an exponential moving average (decay 0.99) and swa the mean of every 10th "
                             "step's weights, which are then what is validated, checkpointed and saved; lookahead pulls the trained weights "
                             "to slow ones every 6 steps. Checkpoints hold no optimizer state, so a run resumed with --weights_path starts "
                             "its average from the loaded weights. default=%(default)s")
    parser.add_argument('--decay_type', type=str, required=False, default=None, choices=[None, 'cosine', 'exponential', 'polynomial', 'piecewise_constant'],
                        help="Learning rate decay type, default=%(default)s")
    parser.add_argument('--epochs', type=int, required=False, default=100,
                        help="Total training epochs, default=%(default)s")
    parser.add_argument('--log_dir', type=str, required=False, default=os.path.join('logs', '000'),
                        help="directory of the checkpoints, the epoch log and the final weights, default=%(default)s")

    # Raw-audio training and background-noise augmentation (tools/audio_process/add_noise.py, drawn per clip and per step)
    parser.add_argument('--raw_audio', action='store_true',
                        help="train on the waveforms of <train_data_path>/sounds (featurized on the GPU every step) instead of cached features")
    parser.add_argument('--noise_path', type=str, required=False, default=None,
                        help="background noise .wav file or directory: mix it into every training clip (needs --raw_audio)")
    parser.add_argument('--snr', type=str, required=False, default='50',
                        help="Sound Noise Ratio (SNR) choice in dB, separate with comma if more than one. default=%(default)s")
    parser.add_argument('--noised_rate', type=float, required=False, default=1.0,
                        help="random percentage rate of adding noise to voice audio (0.0~1.0). default=%(default)s")
    parser.add_argument('--time_shift_ms', type=float, required=False, default=0.0,
                        help="random time shift of every training clip by up to +-this many ms (0: off). default=%(default)s")
    # Room reverberation (tools/audio_process/audio_reverberation.py, drawn per clip and per step)
    parser.add_argument('--rir_path', type=str, required=False, default=None,
                        help="room impulse response .wav file or directory: reverberate the training clips (needs --raw_audio)")
    parser.add_argument('--simulate_rirs', type=int, required=False, default=None,
                        help="simulate this many random rooms (the reference's gpuRIR draws) as the RIR bank (needs --raw_audio)")
    parser.add_argument('--reverb_rate', type=float, required=False, default=None,
                        help="random percentage rate of reverberating the training clips (0.0~1.0). default=1.0")
    # Butterworth filtering (tools/audio_process/wav_filter.py, drawn per clip and per step)
    parser.add_argument('--filter_rate', type=float, required=False, default=None,
                        help="random percentage rate of filtering the training clips (0.0~1.0; needs --raw_audio). default: off")
    parser.add_argument('--filter_types', type=str, required=False, default='lowpass,highpass,bandpass',
                        help="comma list of the filter types drawn for the bank (lowpass, highpass, bandpass, bandstop). default=%(default)s")
    parser.add_argument('--filter_order', type=int, required=False, default=4,
                        help="order of the Butterworth filters. default=%(default)s")
    parser.add_argument('--num_filters', type=int, required=False, default=64,
                        help="number of random filters in the bank. default=%(default)s")
    # Speed and loudness perturbation (tools/audio_process/audio_convert.py, drawn per clip and per step)
    parser.add_argument('--speed_range', type=str, required=False, default=None,
                        help="LO,HI: play the training clips at a random ratio in this range, 0.5~2.0 (needs --raw_audio). default: off")
    parser.add_argument('--speed_rate', type=float, required=False, default=None,
                        help="random percentage rate of changing the speed of the training clips (0.0~1.0). default=1.0")
    parser.add_argument('--loudness_range', type=str, required=False, default=None,
                        help="LO_DB,HI_DB: set the training clips to a random loudness in this range in dBFS, -80~0, written --loudness_range -30,-15 or --loudness_range=-30,-15 (needs --raw_audio). default: off")
    parser.add_argument('--loudness_rate', type=float, required=False, default=None,
                        help="random percentage rate of setting the loudness of the training clips (0.0~1.0). default=1.0")
    # Tempo and pitch perturbation (a phase vocoder, drawn per clip and per step, before the speed change)
    parser.add_argument('--tempo_range', type=str, required=False, default=None,
                        help="LO,HI: stretch the training clips in time at a random tempo in this range, 0.5~2.0, pitch unchanged (needs --raw_audio). default: off")
    parser.add_argument('--tempo_rate', type=float, required=False, default=None,
                        help="random percentage rate of changing the tempo of the training clips (0.0~1.0). default=1.0")
    parser.add_argument('--pitch_range', type=str, required=False, default=None,
                        help="LO,HI: shift the pitch of the training clips by a random number of semitones in this range, -12~12, duration unchanged, written --pitch_range -2,2 or --pitch_range=-2,2 (needs --raw_audio). default: off")
    parser.add_argument('--pitch_rate', type=float, required=False, default=None,
                        help="random percentage rate of shifting the pitch of the training clips (0.0~1.0). default=1.0")
    # SpecAugment of the features (time warp, time masks, frequency masks; drawn per clip and per step, with or without --raw_audio)
    parser.add_argument('--time_mask', type=str, required=False, default=None,
                        help="N,W: overwrite N blocks of up to W frames of every training clip's features (N <= 4). default: off")
    parser.add_argument('--freq_mask', type=str, required=False, default=None,
                        help="N,W: overwrite N blocks of up to W coefficients of every training clip's features (N <= 4). default: off")
    parser.add_argument('--time_warp', type=int, required=False, default=None,
                        help="W: move one random frame of every training clip by up to W frames and interpolate the rest. default: off")
    parser.add_argument('--mask_rate', type=float, required=False, default=None,
                        help="random percentage rate of masking / warping the training clips (0.0~1.0). default=1.0")
    parser.add_argument('--mask_fill', type=str, required=False, default=None, choices=['zero', 'mean'],
                        help="what a masked entry becomes: zero, or the clip's own mean of that coefficient. default=mean")
    # "--loudness_range -30,-15": argparse takes a value that starts with '-' and is no plain number for an option, so bind it with '='
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 2, -1, -1):
        if argv[i] in ('--loudness_range', '--pitch_range'):
            argv[i:i + 2] = [argv[i] + '=' + argv[i + 1]]
    args = parser.parse_args(argv)
    if args.rnn_layers != 1 and args.model_type not in ('simple_gru', 'simple_lstm'):
        parser.error('--rnn_layers %d does not apply to %s: only simple_gru / simple_lstm stack layers' % (args.rnn_layers, args.model_type))
    return args


if __name__ == '__main__':
    main()
