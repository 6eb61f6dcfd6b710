"""Writes profiles/plc_examples.json: the waveform error of the packet loss concealment (the host twin gtcrn_plc_rows_pcm16_host)
on the first 12 s of the golden speech examples at 16 kHz / 160 against zero fill, by the function tests/test_plc_host.py
asserts on (tests/plc_cases.py, speech_figures).  No GPU is needed.

    python tools/plc_examples.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as graft  # noqa: E402
import plc_cases as PC  # noqa: E402


def main():
    graft.build()
    from gtcrn_micro_amd import plc_rows_host
    host = lambda x, lost, hist, rec, prm, slots, count, law: plc_rows_host(x, lost, hist, rec, prm, slots, count, law)
    out = {"what": "summed error energy of the concealed packets / summed energy of the true packets (zero fill = 1), over the lost "
                   "packets above -40 dBov; median of the per-packet ratios; 16 kHz / 160, losses at [25::20], [46::60], [47::120]"}
    for which in ("noisy", "enh"):
        out[which] = PC.speech_figures(host, which)
        print(which, out[which])
    with open(os.path.join(ROOT, "profiles", "plc_examples.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
