#!/usr/bin/env python3
"""Find silent wav files by their energy per second and move them away (kws_amd.vad: one device call per directory).

    python silent_check.py --wav_path DIR_OR_FILE --threshold 0.2 --target_path DIR
"""
import argparse
import os
import shutil

from _common import detect_all, wav_files


def build_parser():
    ap = argparse.ArgumentParser(description="check & move silent wav files by energy per second, on the GPU")
    ap.add_argument("--wav_path", type=str, required=True, help="wav file or directory to check")
    ap.add_argument("--threshold", type=float, default=0.2, help="energy per second below which a file is silent. default=%(default)s")
    ap.add_argument("--target_path", type=str, required=True, help="where the silent files of a directory are moved")
    return ap


def silent_flags(wav_path, threshold):
    """-> {file: bool}"""
    out = {}
    for _, names, _, res, _ in detect_all(wav_files(wav_path)):
        for name, flag in zip(names, res.is_silent(threshold)):
            out[name] = bool(flag)
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.target_path, exist_ok=True)
    flags = silent_flags(args.wav_path, args.threshold)
    if os.path.isfile(args.wav_path):
        print('silent flag for {}: {}'.format(args.wav_path, flags[args.wav_path]))
    else:
        silent = [n for n, f in flags.items() if f]
        for n in silent:
            shutil.move(n, args.target_path)
        print('Found {} silent audio files'.format(len(silent)))


if __name__ == "__main__":
    main()
