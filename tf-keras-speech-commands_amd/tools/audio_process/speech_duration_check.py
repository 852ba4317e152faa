#!/usr/bin/env python3
"""Where the speech starts and ends in a wav file or in every wav file of a directory, by the band-energy detector
(kws_amd.vad.Vad): the whole directory is packed once and analysed in one device call.

    python speech_duration_check.py --wav_path DIR_OR_FILE --vad_type simple [--json OUT]
"""
import argparse
import json

from _common import detect_all, wav_files

VAD_TYPES = ("simple",)


def build_parser():
    ap = argparse.ArgumentParser(description="speech begin / end time of wav files by voice-activity detection on the GPU")
    ap.add_argument("--wav_path", type=str, required=True, help="wav file or directory to check")
    ap.add_argument("--vad_type", type=str, default="simple", help="detector type; only 'simple' is offered. default=%(default)s")
    ap.add_argument("--json", type=str, default=None, help="write {file: [begin_s, end_s]} here")
    return ap


def speech_durations(wav_path, vad_type="simple"):
    """-> {file: (speech_begin, speech_end)} in seconds; (0.0, 0.0) where no speech interval was found"""
    if vad_type not in VAD_TYPES:
        raise ValueError('Unsupported VAD type')
    out = {}
    for _, names, _, res, _ in detect_all(wav_files(wav_path)):
        for name, (b, e) in zip(names, res.span_seconds):
            out[name] = (float(b), float(e))
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    spans = speech_durations(args.wav_path, args.vad_type)
    for name, (b, e) in spans.items():
        print('{}: speech start at {}s, end at {}s'.format(name, b, e))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({k: list(v) for k, v in spans.items()}, f, indent=1)


if __name__ == "__main__":
    main()
