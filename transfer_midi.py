#!/usr/bin/env python3
"""``python transfer_midi.py --config gmm_model_config.json [--params model.pt] in.mid out.mid [--lmbda 1.0]`` - a whole MIDI file through the arousal
faders of a trained GM-VAE on the MI355X HIP path: every 4-beat window is transferred and the windows are stitched back into one file (see
music-fader-nets_amd/transfer.py; the package directory is not a Python identifier, so it is loaded through mfn_import)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mfn_import import load_package  # noqa: E402

load_package()
from music_fader_nets_amd.transfer import main  # noqa: E402

if __name__ == "__main__":
    main()
