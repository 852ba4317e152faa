#!/usr/bin/env python3
"""Find a keyword in recordings from a few example recordings of it, without a trained model (kws_amd.qbe: subsequence dynamic time
warping of the examples' MFCC rows against the recordings' on the GPU).

    python keyword_search.py --enroll_path DIR --input_wav FILE_OR_DIR --threshold 0.25 [--metric cosine|l2] [--min_gap_s 0.5]
                             [--max_hits 16] [--no_trim] [--output_csv PATH] [--save_dir DIR]

DIR holds one folder per keyword with its example wav files: <keyword>/*.wav.  One line per hit is printed; --save_dir cuts every hit
out as <keyword>/<file>_<n>.wav.
"""
import argparse
import csv
import glob
import os
import sys
import wave

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from kws_amd.vad import read_wav  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description="query-by-example keyword search in wav files, on the GPU")
    ap.add_argument("--enroll_path", type=str, required=True, help="directory of examples, laid out as <keyword>/*.wav")
    ap.add_argument("--input_wav", type=str, required=True, help="wav file or directory to search")
    ap.add_argument("--threshold", type=float, required=True, help="largest cost per template row that counts as a hit")
    ap.add_argument("--metric", type=str, default="cosine", choices=["cosine", "l2"], help="local distance. default=%(default)s")
    ap.add_argument("--min_gap_s", type=float, default=0.5, help="seconds between the ends of two hits of a keyword. default=%(default)s")
    ap.add_argument("--max_hits", type=int, default=16, help="hits per keyword and file. default=%(default)s")
    ap.add_argument("--no_trim", action="store_true", help="take the examples as they are instead of trimming them to their speech")
    ap.add_argument("--output_csv", type=str, default=None, help="write the hits here: file, keyword, template, start_s, end_s, cost")
    ap.add_argument("--save_dir", type=str, default=None, help="cut every hit out as <keyword>/<file>_<n>.wav under this directory")
    return ap


def wav_files(path):
    return [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "*.wav")))


def examples(enroll_path):
    """-> ([wav path], [keyword]) from <keyword>/*.wav, keywords in sorted order"""
    paths, words = [], []
    for kw in sorted(os.listdir(enroll_path)):
        for p in sorted(glob.glob(os.path.join(enroll_path, kw, "*.wav"))):
            paths.append(p)
            words.append(kw)
    if not paths:
        raise SystemExit("no examples under %s (expected <keyword>/*.wav)" % enroll_path)
    return paths, words


def main(argv=None):
    args = build_parser().parse_args(argv)
    from classifier.params import pr
    from kws_amd import qbe
    paths, words = examples(args.enroll_path)
    templates = qbe.Templates.enroll(pr, paths, words, trim=not args.no_trim)
    files = wav_files(args.input_wav)
    recs = []
    for p in files:
        data, rate = read_wav(p)
        if rate != pr.sample_rate:
            raise SystemExit("%s is at %d Hz, the featurizer at %d Hz" % (p, rate, pr.sample_rate))
        recs.append(data)
    hits = qbe.search(templates, recs, metric=args.metric, threshold=args.threshold, min_gap_s=args.min_gap_s, max_hits=args.max_hits)
    H, W = int(pr.hop_samples), int(pr.window_samples)
    rows, counts = [], {}
    for i, (r, kw, t, a, b, c) in enumerate(hits.rows()):
        name = os.path.basename(files[r])
        rows.append((name, kw, os.path.basename(paths[templates.source[t]]), "%.3f" % a, "%.3f" % b, "%.6f" % c))
        print("%s %s %.3f-%.3f s cost %.4f (%s)" % (name, kw, a, b, c, rows[-1][2]))
        if args.save_dir:
            n = counts.get((r, kw), 0)
            counts[(r, kw)] = n + 1
            os.makedirs(os.path.join(args.save_dir, kw), exist_ok=True)
            cut = recs[r][int(hits.start_frame[i]) * H:int(hits.end_frame[i]) * H + W]
            with wave.open(os.path.join(args.save_dir, kw, "%s_%d.wav" % (os.path.splitext(name)[0], n)), "wb") as wf:
                wf.setnchannels(1)
                wf.setsampwidth(2)
                wf.setframerate(int(pr.sample_rate))
                wf.writeframes(cut.astype("<i2").tobytes())
    if args.output_csv:
        with open(args.output_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("file", "keyword", "template", "start_s", "end_s", "cost"))
            w.writerows(rows)
    print("%d hits in %d files" % (len(rows), len(files)))


if __name__ == "__main__":
    main()
