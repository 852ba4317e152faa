#!/usr/bin/env python3
"""Cut every detected speech interval of a wav file or a directory out into a wav file of its own (kws_amd.vad: one
detection call and one clip gather per directory).

    python vad_split.py --wav_path DIR_OR_FILE --output_path DIR [--clip_length 1.0] [--pad_before 0.1] [--pad_after 0.1]
"""
import argparse
import os
import wave

import numpy as np

from _common import detect_all, wav_files


def build_parser():
    ap = argparse.ArgumentParser(description="split wav files into one clip per detected speech interval, on the GPU")
    ap.add_argument("--wav_path", type=str, required=True, help="wav file or directory to split")
    ap.add_argument("--output_path", type=str, required=True, help="directory for the clips")
    ap.add_argument("--clip_length", type=float, default=1.0, help="clip length in seconds. default=%(default)s")
    ap.add_argument("--pad_before", type=float, default=0.0, help="seconds kept in front of an interval. default=%(default)s")
    ap.add_argument("--pad_after", type=float, default=0.0, help="seconds kept after an interval. default=%(default)s")
    ap.add_argument("--align", type=str, default="left", choices=["left", "center"],
                    help="where a short cut sits in its clip: zeros in front (left) or on both sides. default=%(default)s")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.output_path, exist_ok=True)
    total = 0
    for rate, names, _, res, vad in detect_all(wav_files(args.wav_path)):
        clips, triples = vad.clips(None, res, int(args.clip_length * rate), int(args.pad_before * rate), int(args.pad_after * rate),
                                   args.align)
        pcm = np.clip(np.round(clips.cpu().numpy() * 32768.0), -32768, 32767).astype("<i2")
        counts = {}
        for row, (rec, _, _) in zip(pcm, triples.cpu().tolist()):
            i = counts.get(rec, 0)
            counts[rec] = i + 1
            stem = os.path.splitext(os.path.basename(names[rec]))[0]
            with wave.open(os.path.join(args.output_path, "%s_%03d.wav" % (stem, i)), "wb") as wf:
                wf.setnchannels(1)
                wf.setsampwidth(2)
                wf.setframerate(rate)
                wf.writeframes(row.tobytes())
            total += 1
    print('Wrote {} clips'.format(total))


if __name__ == "__main__":
    main()
