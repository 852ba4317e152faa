"""Voice-activity detection of about one hour of 16 kHz int16 audio, cut three ways: 3600 recordings of 1 s, 60 of 60 s and one
of 3600 s.  Per case: the device time of the two kernels of kws_vad_detect (the library's per-launch timing, medians over the
rounds), audio seconds per second of device time, and next to them the time HBM needs just to read the samples at 8 TB/s.

    python tools/vadbench.py [--rounds 5] [--out profiles/vadbench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-keras-speech-commands_amd"))
import torch

from kws_amd import lib as _l
from kws_amd.vad import Vad

RATE = 16000
CASES = {"3600x1s": (3600, 1), "60x60s": (60, 60), "1x3600s": (1, 3600)}      # recordings, seconds each
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "vadbench.json"))
    args = ap.parse_args()
    vad = Vad(RATE)
    gen = torch.Generator(device="cuda").manual_seed(5)
    record = {"device": torch.cuda.get_device_name(0), "sample_rate": RATE, "rounds": args.rounds,
              "build_id": {"kws_vad.hip": _l.build_id().get("kws_vad.hip")}, "cases": {}}
    for name, (R, secs) in CASES.items():
        n = secs * RATE - 37                                       # not a multiple of the hop
        wav = torch.randint(-3000, 3000, (R, n), generator=gen, device="cuda", dtype=torch.int16)
        lens = [n - 11 * (r % 7) for r in range(R)]
        vad.detect(wav, lens)                                      # warm-up: the matrix upload, the allocator
        torch.cuda.synchronize()
        times = {"vad_ratio_i16": [], "vad_smooth": []}
        for _ in range(args.rounds):
            _l.prof_enable(True)
            vad.detect(wav, lens)
            torch.cuda.synchronize()
            rep = _l.prof_report()
            _l.prof_enable(False)
            for k in times:
                times[k].append(rep[k]["total_ms"])
        med = {k: statistics.median(v) for k, v in times.items()}
        total_ms = sum(med.values())
        audio_s = sum(lens) / RATE
        hbm_ms = 2.0 * sum(lens) / HBM_BYTES_PER_S * 1e3
        record["cases"][name] = {"recordings": R, "seconds_each": secs, "audio_seconds": audio_s, "kernel_ms": med,
                                 "kernel_ms_all_rounds": times, "detect_ms": total_ms,
                                 "audio_seconds_per_second": audio_s / (total_ms * 1e-3),
                                 "hbm_read_ms_at_8TBps": hbm_ms, "times_hbm_read": total_ms / hbm_ms}
        print(name, json.dumps(record["cases"][name]["kernel_ms"]), "detect %.3f ms, %.3g audio-s/s, HBM read %.4f ms"
              % (total_ms, audio_s / (total_ms * 1e-3), hbm_ms))
        del wav
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
