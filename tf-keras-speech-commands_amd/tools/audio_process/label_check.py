#!/usr/bin/env python3
"""Look at a labelled dataset in pairs before training on it (kws_amd.neighbors): clips whose nearest neighbours in a model's
embedding space carry another label, and clips that exist twice -- inside the dataset, or in it and in a second one (the leakage
check between a training and a validation set).  The other checks of this folder look at one file at a time.

    python label_check.py --dataset_path D --classes_path classes.txt --weights_path W.npz [--model_type simple_cnn] [--rnn_layers 1]
                          [--params_path params.json] [--other_path D2] [--k 10] [--dup_threshold 0.9995] [--output_csv PATH]

D holds one folder of wav files per class (D/<class>/*.wav, or D/sounds/<class>/*.wav as the training layout has it).  The clips are
loaded with classifier.data.load_audio_samples, featurized and embedded in batches on the GPU (kws_amd.transfer.embed), and two tables
are printed: the suspected labels (file, label, suggested label, the share of the neighbours with the file's own label, the share
with the suggested one), the most suspicious first, and the duplicate pairs (file, file, cosine).  --output_csv writes both tables
into one csv file with a leading `table` column.  The exit status is 0 whether or not anything is found."""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="suspected labels and duplicate clips of a dataset, by nearest neighbours of its embeddings")
    ap.add_argument("--dataset_path", type=str, required=True, help="folder with one sub-folder of wav files per class")
    ap.add_argument("--classes_path", type=str, required=True, help="text file of class names")
    ap.add_argument("--weights_path", type=str, required=True, help="trained weights (.npz) of the model that embeds the clips")
    ap.add_argument("--model_type", type=str, default="simple_cnn", help="simple_cnn / simple_cnn_lite / simple_gru / simple_lstm. default=%(default)s")
    ap.add_argument("--rnn_layers", type=int, default=1, help="recurrent layers of simple_gru / simple_lstm. default=%(default)s")
    ap.add_argument("--params_path", type=str, default=None, help="json file of audio parameters to inject")
    ap.add_argument("--other_path", type=str, default=None, help="a second dataset (e.g. the validation set): clips of both are reported")
    ap.add_argument("--k", type=int, default=10, help="neighbours that vote on a label. default=%(default)s")
    ap.add_argument("--dup_threshold", type=float, default=0.9995, help="cosine from which two clips count as duplicates. default=%(default)s")
    ap.add_argument("--output_csv", type=str, default=None, help="write both tables to this csv file")
    return ap


def sounds_dir(path, class_names):
    sub = os.path.join(path, "sounds")
    return sub if os.path.isdir(sub) and not os.path.isdir(os.path.join(path, class_names[0])) else path


def embed_dataset(model, path, class_names):
    """-> (files, labels (N) int, emb (N, E) on the GPU)"""
    from classifier.data import get_sample_list, load_audio_samples
    from kws_amd.transfer import embed
    root = sounds_dir(path, class_names)
    x, lengths, words = load_audio_samples(root, class_names)
    files = [s["file"] for s in get_sample_list(root, class_names)]
    y = np.array([class_names.index(w) for w in words], dtype=np.int64)
    return files, y, embed(model, x, sample_lengths=lengths)            # featurized and embedded 4096 clips at a time


def main(argv=None):
    args = build_parser().parse_args(argv)
    from classifier.model import get_model
    from classifier.params import inject_params
    from common.utils import get_classes
    from kws_amd import neighbors
    class_names = get_classes(args.classes_path)
    if args.params_path:
        inject_params(args.params_path)
    model = get_model(args.model_type, len(class_names), weights_path=args.weights_path, num_layers=args.rnn_layers)
    files, y, emb = embed_dataset(model, args.dataset_path, class_names)
    rows = []
    print("%d clips, %d classes, embeddings %d wide" % (len(files), len(class_names), emb.shape[1] if len(files) else 0))
    if len(files) > 1:
        issues = neighbors.label_issues(emb, y, max(2, len(class_names)), k=min(args.k, len(files) - 1))
        print("Suspected labels: %d" % len(issues))
        for r, lab, sug, own, sup in zip(issues.rows, issues.label, issues.suggested, issues.own_share, issues.support):
            print("  %s: %s -> %s (own share %.2f, support %.2f)" % (files[r], class_names[lab], class_names[sug], own, sup))
            rows.append(["label", files[r], class_names[lab], class_names[sug], "%.4f" % own, "%.4f" % sup])
        a, b, c = neighbors.duplicates(emb, threshold=args.dup_threshold)
        print("Duplicate pairs inside %s: %d" % (args.dataset_path, len(a)))
        for i, j, cos in zip(a, b, c):
            print("  %s == %s (cosine %.6f)" % (files[i], files[j], cos))
            rows.append(["duplicate", files[i], files[j], "", "%.6f" % cos, ""])
    if args.other_path and len(files):
        files2, _, emb2 = embed_dataset(model, args.other_path, class_names)
        if len(files2):
            a, b, c = neighbors.duplicates(emb, emb2, threshold=args.dup_threshold)
            print("Duplicate pairs between %s and %s: %d" % (args.dataset_path, args.other_path, len(a)))
            for i, j, cos in zip(a, b, c):
                print("  %s == %s (cosine %.6f)" % (files[i], files2[j], cos))
                rows.append(["leak", files[i], files2[j], "", "%.6f" % cos, ""])
    if args.output_csv:
        with open(args.output_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["table", "file", "label_or_other_file", "suggested", "own_share_or_cosine", "support"])
            w.writerows(rows)
        print("Wrote %d rows to %s" % (len(rows), args.output_csv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
