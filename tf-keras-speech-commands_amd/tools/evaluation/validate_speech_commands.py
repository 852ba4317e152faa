#!/usr/bin/env python3
"""Top-k classes of one audio file, or of every file of a directory, with the forward time (mirror of the reference's
tools/evaluation/validate_speech_commands.py for the native runtime).

The reference loads one file at a time into one of five foreign runtimes, predicts once to warm up, times `loop_count` predictions and
prints the k best classes.  Here every file is decoded, featurized and scored in ONE batch on the GPU; the printed time is the average
of `loop_count` forward passes over that batch (after one warm-up pass), and the per-file lines and the optional result files
(<output_path>/<file name>.txt, one "class: score" line per rank) are the reference's.

    python tools/evaluation/validate_speech_commands.py --model_type simple_cnn --weights_path weights.npz \\
        --audio_path FILE_OR_DIR --classes_path classes.txt [--params_path params.json] [--top_k 1] [--loop_count 1] [--output_path DIR]
"""
import argparse
import glob
import os
import sys
import time

import numpy as np

sys.path.append(os.path.join(os.path.dirname(os.path.realpath(__file__)), '..', '..'))
from classifier.model import get_model
from classifier.params import inject_params, pr
from common.data_utils import get_featurizer, load_wav
from common.utils import get_classes


def load_batch(audio_files):
    """-> (wav (N, max_samples) float32 head-aligned, lengths (N,) int32): the layout of classifier.data.extract_features"""
    wav = np.zeros((len(audio_files), pr.max_samples), np.float32)
    lens = np.zeros((len(audio_files),), np.int32)
    for j, path in enumerate(audio_files):
        a = load_wav(path)[:pr.max_samples]
        wav[j, :len(a)] = a
        lens[j] = len(a)
    return wav, lens


def validate_speech_commands(model, audio_files, class_names, top_k, loop_count, output_path):
    """-> (top-k scores (N, k), top-k class indices (N, k)) as numpy; prints and writes what the reference does"""
    import torch
    wav, lens = load_batch(audio_files)
    feat = get_featurizer()(torch.from_numpy(wav).cuda(), torch.from_numpy(lens).cuda()).contiguous()
    dm = model._device()
    dm.forward(feat, True, False)                            # once first, as the reference: nothing is loaded inside the timed loop
    torch.cuda.synchronize()
    start = time.time()
    for _ in range(loop_count):
        probs, _ = dm.forward(feat, True, False)
    torch.cuda.synchronize()
    end = time.time()
    print("Average Inference time: {:.8f}ms".format((end - start) * 1000 / loop_count))
    scores, index = torch.topk(probs, top_k, dim=1)
    scores, index = scores.cpu().numpy(), index.cpu().numpy()
    if output_path:
        os.makedirs(output_path, exist_ok=True)
    for j, audio_file in enumerate(audio_files):
        lines = ['%s: %.3f' % (class_names[index[j, i]], scores[j, i]) for i in range(top_k)]
        if len(audio_files) > 1:
            print(audio_file)
        for s in lines:
            print(s)
        if output_path:
            name = os.path.splitext(os.path.basename(audio_file))[0] + '.txt'
            with open(os.path.join(output_path, name), 'w') as f:
                f.write(''.join(s + '\n' for s in lines))
    return scores, index


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='print the top-k classes of audio files under a trained model (.npz weights)')
    parser.add_argument('--model_type', help='simple_cnn / simple_cnn_lite / simple_gru / simple_lstm, default=%(default)s', type=str,
                        default='simple_cnn')
    parser.add_argument('--rnn_layers', help='recurrent layers of simple_gru / simple_lstm, default=%(default)s', type=int, default=1)
    parser.add_argument('--weights_path', help='trained weights (.npz)', type=str, required=True)
    parser.add_argument('--audio_path', help='a wav file, or a directory whose files are all scored in one batch', type=str, required=True)
    parser.add_argument('--classes_path', help='text file of class names, background first', type=str, required=True)
    parser.add_argument('--params_path', help='json file of audio parameters to inject', type=str, required=False, default=None)
    parser.add_argument('--top_k', help='classes printed per file, best first, default=%(default)s', type=int, required=False, default=1)
    parser.add_argument('--loop_count', help='timed forward passes over the batch, default=%(default)s', type=int, default=1)
    parser.add_argument('--output_path', help='directory for one <file name>.txt of the printed lines per audio file, default=%(default)s',
                        type=str, required=False, default=None)
    args = parser.parse_args(argv)
    if args.top_k < 1 or args.loop_count < 1:
        parser.error('--top_k and --loop_count must be at least 1')
    return args


def main(argv=None):
    args = parse_args(argv)
    class_names = get_classes(args.classes_path)
    assert class_names[0] == 'background', '1st class should be background.'
    if args.top_k > len(class_names):
        raise SystemExit('--top_k %d exceeds the %d classes' % (args.top_k, len(class_names)))
    if args.params_path:
        inject_params(args.params_path)
    model = get_model(args.model_type, len(class_names), weights_path=args.weights_path, num_layers=args.rnn_layers)
    if os.path.isdir(args.audio_path):
        audio_files = sorted(glob.glob(os.path.join(args.audio_path, '*')))
    else:
        audio_files = [args.audio_path]
    if not audio_files:
        raise SystemExit('no audio file at ' + args.audio_path)
    return validate_speech_commands(model, audio_files, class_names, args.top_k, args.loop_count, args.output_path)


if __name__ == '__main__':
    main()
