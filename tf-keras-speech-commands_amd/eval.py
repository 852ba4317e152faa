#!/usr/bin/env python3
"""Evaluate a trained keyword-spotting model on a dataset (mirror of the reference's eval.py for the native runtime).

The reference predicts one sample at a time through five foreign runtimes and builds the confusion matrix with sklearn
(eval.py:201-256).  Here the whole set is scored in GPU batches and the confusion counts are accumulated on the device
(kws_confusion_counts); the printed summary is the reference's: accuracy, then the matrix.  --curves adds what the reference has no
counterpart for: per-class AUC, equal-error rate and miss rate at a false-accept rate, top-k accuracy and the calibration error, from score
statistics counted on the device (kws_score_hist, kws_amd.metrics)."""
import argparse
import os
import sys

import numpy as np

sys.path.append(os.path.dirname(os.path.realpath(__file__)))
from classifier.data import get_dataset
from classifier.model import get_model
from classifier.params import inject_params
from common.utils import get_classes
from kws_amd import lib as _l


def evaluate_accuracy(model, x, y, class_names, batch_size=4096):
    """-> (top-1 accuracy, confusion matrix [label, prediction] as int64 numpy)"""
    import torch
    dm = model._device()
    xd, is_audio = model._to_device_inputs(x)
    yd = model._labels(y, xd.shape[0])
    C = len(class_names)
    counts = torch.zeros((C, C), dtype=torch.int32, device=xd.device)
    L = _l.get_lib()
    for i in range(0, xd.shape[0], batch_size):
        _, am = dm.forward(model._features_of(xd[i:i + batch_size], is_audio).contiguous(), False, True)
        yb = yd[i:i + batch_size].contiguous()
        _l.check(L.kws_confusion_counts(yb.data_ptr(), am.data_ptr(), yb.numel(), C, counts.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    cm = counts.cpu().numpy().astype(np.int64)
    total = int(cm.sum())
    return (float(np.trace(cm)) / total if total else 0.0), cm


RNN_TYPES = ('simple_gru', 'simple_lstm')


def evaluate_int8(model, x, y, class_names, x_calib, calib_samples=1000, method='max', batch_size=4096, seed=0):
    """int8 post-training quantization (KWSModel.quantize) calibrated on `calib_samples` clips of x_calib drawn without replacement
    (seeded), then scored on (x, y) -> (quantized model, int8 accuracy, fp32 / int8 arg-max agreement, int8 confusion matrix).
    x_calib None: the dynamic-range int8 of simple_gru / simple_lstm, which takes no calibration."""
    import torch
    if x_calib is None:
        qmodel = model.quantize(None, method=method, batch_size=batch_size)
    else:
        n_cal = min(int(calib_samples), len(x_calib))
        idx = np.sort(np.random.default_rng(seed).choice(len(x_calib), n_cal, replace=False))
        qmodel = model.quantize(np.asarray(x_calib)[idx], method=method, batch_size=batch_size)
    dm = model._device()
    xd, is_audio = model._to_device_inputs(x)
    yd = model._labels(y, xd.shape[0])
    C = len(class_names)
    counts = torch.zeros((C, C), dtype=torch.int32, device=xd.device)
    agree = torch.zeros((), dtype=torch.int64, device=xd.device)
    L = _l.get_lib()
    for i in range(0, xd.shape[0], batch_size):
        f = model._features_of(xd[i:i + batch_size], is_audio).contiguous()
        _, am32 = dm.forward(f, False, True)
        _, am8 = qmodel.quantized.forward(f)
        agree += (am32 == am8).sum()
        yb = yd[i:i + batch_size].contiguous()
        _l.check(L.kws_confusion_counts(yb.data_ptr(), am8.data_ptr(), yb.numel(), C, counts.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    cm = counts.cpu().numpy().astype(np.int64)
    total = int(cm.sum())
    return qmodel, (float(np.trace(cm)) / total if total else 0.0), (float(agree.item()) / total if total else 0.0), cm


def print_score_table(stats, class_names, max_far=0.01, top_k=3, title=None, baseline=None):
    """The per-keyword operating points of a kws_amd.metrics.ScoreStats: one row per class, then top-1..k accuracy and the ECE.
    baseline: the ScoreStats of another model on the same clips (the float model, for an int8 table): two more columns hold this model's
    EER and miss rate minus the baseline's."""
    targets, non_targets = stats.totals()
    auc = stats.auc()
    eer, eer_t = stats.eer()
    far_t, far_miss = stats.at_far(max_far)
    w = max(8, max(len(c) for c in class_names) + 1)
    if title:
        print(title)
    extra = ['', ''] + [''] * len(class_names)
    if baseline is not None:
        d_eer, d_miss = eer - baseline.eer()[0], far_miss - baseline.at_far(max_far)[1]
        extra = ['%10s%12s' % ('EER-fp32', 'miss-fp32')] + ['%+10.4f%+12.4f' % (d_eer[i], d_miss[i]) for i in range(len(class_names))]
    print('%*s%9s%12s%9s%9s%9s%12s%12s' % (w, 'class', 'targets', 'non-targets', 'AUC', 'EER', 'EER thr', 'miss@%g' % max_far,
                                            'thr@%g' % max_far) + extra[0])
    for i, c in enumerate(class_names):
        print('%*s%9d%12d%9.4f%9.4f%9.4f%12.4f%12.4f' % (w, c[:w - 1], targets[i], non_targets[i], auc[i], eer[i], eer_t[i], far_miss[i],
                                                          far_t[i]) + extra[1 + i])
    print('  '.join('top-%d accuracy %.4f' % (k, stats.top_k(k)) for k in range(1, max(1, min(top_k, len(class_names))) + 1)))
    print('ECE %.4f (%d confidence bins)' % (stats.ece()[0], stats.bins))


def write_curves_csv(path, stats, class_names, tag=None):
    """class,threshold,tpr,fpr for every class and threshold j / bins (tag: a prefix of the class column, for a second model)"""
    cv = stats.curves()
    with open(path, 'w' if tag is None else 'a') as f:
        if tag is None:
            f.write('class,threshold,tpr,fpr\n')
        for i, c in enumerate(class_names):
            name = c if tag is None else '%s:%s' % (tag, c)
            for t, tp, fp in zip(cv['thresholds'], cv['tpr'][i], cv['fpr'][i]):
                f.write('%s,%.10g,%.10g,%.10g\n' % (name, t, tp, fp))


def print_confusion_matrix(cm, class_names):
    w = max(8, max(len(c) for c in class_names) + 1)
    print(' ' * w + ''.join('%*s' % (w, c[:w - 1]) for c in class_names))
    for i, c in enumerate(class_names):
        print('%*s' % (w, c[:w - 1]) + ''.join('%*d' % (w, v) for v in cm[i]))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='evaluate a trained model (.npz weights) on a dataset')
    parser.add_argument('--model_type', type=str, default='simple_cnn')
    parser.add_argument('--rnn_layers', type=int, default=1, help="recurrent layers of simple_gru / simple_lstm, 1..4 (the reference's num_layers); the CNN types take 1 only, default=%(default)s")
    parser.add_argument('--weights_path', type=str, required=True)
    parser.add_argument('--dataset_path', type=str, required=True)
    parser.add_argument('--classes_path', type=str, required=True)
    parser.add_argument('--params_path', type=str, default=None)
    parser.add_argument('--batch_size', type=int, default=4096)
    parser.add_argument('--int8', default=False, action='store_true',
                        help='also quantize the model to int8 (post-training; dynamic-range for simple_gru / simple_lstm) and report its '
                             'accuracy and agreement')
    parser.add_argument('--calib_path', type=str, default=None, help='dataset to calibrate the int8 ranges on (default: the evaluated set)')
    parser.add_argument('--calib_samples', type=int, default=1000, help='calibration clips, drawn with a fixed seed')
    parser.add_argument('--quant_method', type=str, default=None, choices=['max', 'relu6', 'kl', 'dynamic'],
                        help="simple_cnn / simple_cnn_lite activation ranges: calibrated maxima ('max', the default), 6 for every ReLU6 "
                             "tensor ('relu6'), or the ranges of least KL divergence of a second, histogram pass ('kl', the reference's MNN "
                             "recipe); simple_gru / simple_lstm: 'dynamic' (dynamic-range int8, no calibration: their only method)")
    parser.add_argument('--save_quantized', type=str, default=None, help='write the int8 model to this .npz')
    parser.add_argument('--curves', default=False, action='store_true',
                        help='also print per-class AUC, equal-error rate and the miss rate at --max_far, top-k accuracy and the expected '
                             'calibration error (with --int8: for the quantized model as well)')
    parser.add_argument('--bins', type=int, default=1024, help='score bins of --curves (thresholds j / bins), default=%(default)s')
    parser.add_argument('--max_far', type=float, default=0.01, help='false-accept rate of the operating point --curves reports, default=%(default)s')
    parser.add_argument('--top_k', type=int, default=3, help='--curves prints top-1 .. top-k accuracy, default=%(default)s')
    parser.add_argument('--curves_csv', type=str, default=None, help='with --curves: write class,threshold,tpr,fpr to this file')
    args = parser.parse_args(argv)
    rnn = args.model_type in RNN_TYPES
    if args.rnn_layers != 1 and not rnn:
        parser.error('--rnn_layers %d does not apply to %s: only simple_gru / simple_lstm stack layers' % (args.rnn_layers, args.model_type))
    if args.bins < 2 or args.top_k < 1 or not 0.0 <= args.max_far <= 1.0:
        parser.error('--bins must be >= 2, --top_k >= 1 and --max_far within [0, 1]')
    if args.curves_csv and not args.curves:
        parser.error('--curves_csv needs --curves')
    if args.int8 and args.quant_method is not None and (args.quant_method == 'dynamic') != rnn:
        parser.error("--quant_method %s does not apply to %s: simple_gru / simple_lstm take 'dynamic' only, the CNNs max, relu6 or kl"
                     % (args.quant_method, args.model_type))
    return args


def main(argv=None):
    args = parse_args(argv)
    rnn = args.model_type in RNN_TYPES
    class_names = get_classes(args.classes_path)
    assert class_names[0] == 'background', '1st class should be background.'
    if args.params_path:
        inject_params(args.params_path)
    x, y, _, _ = get_dataset(args.dataset_path, class_names)
    model = get_model(args.model_type, len(class_names), weights_path=args.weights_path, num_layers=args.rnn_layers)
    acc, cm = evaluate_accuracy(model, x, y, class_names, args.batch_size)
    print('%d correct out of %d samples, accuracy %.4f' % (int(np.trace(cm)), int(cm.sum()), acc))
    print_confusion_matrix(cm, class_names)
    if args.curves:
        stats = model.evaluate_scores(x, y, args.batch_size, args.bins)
        print_score_table(stats, class_names, args.max_far, args.top_k)
        if args.curves_csv:
            write_curves_csv(args.curves_csv, stats, class_names)
    if args.int8 and rnn:
        # dynamic-range int8: no calibration, so --calib_path / --calib_samples are not read
        qmodel, acc8, agree, cm8 = evaluate_int8(model, x, y, class_names, None, method='dynamic', batch_size=args.batch_size)
        print('int8 (dynamic range): %d correct out of %d samples, accuracy %.4f' % (int(np.trace(cm8)), int(cm8.sum()), acc8))
    elif args.int8:
        method = args.quant_method or 'max'
        x_calib = x if not args.calib_path else get_dataset(args.calib_path, class_names)[0]
        qmodel, acc8, agree, cm8 = evaluate_int8(model, x, y, class_names, x_calib, args.calib_samples, method, args.batch_size)
        print('int8 (%s calibration, %d clips): %d correct out of %d samples, accuracy %.4f'
              % (method, min(args.calib_samples, len(x_calib)), int(np.trace(cm8)), int(cm8.sum()), acc8))
    if args.int8:
        print('fp32 / int8 argmax agreement %.4f' % agree)
        print_confusion_matrix(cm8, class_names)
        if args.curves:
            stats8 = model.evaluate_scores(x, y, args.batch_size, args.bins, quantized=qmodel)
            print_score_table(stats8, class_names, args.max_far, args.top_k, title='int8:', baseline=stats)
            if args.curves_csv:
                write_curves_csv(args.curves_csv, stats8, class_names, tag='int8')
        if args.save_quantized:
            qmodel.save(args.save_quantized)
            print('Saved int8 model {}.'.format(args.save_quantized))


if __name__ == '__main__':
    main()
