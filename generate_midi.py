#!/usr/bin/env python3
"""``python generate_midi.py --config gmm_model_config.json [--params model.pt] OUT_DIR [--rows 8 --rhythm 1 --note 0 --key 0]`` - pieces drawn from the
mixture prior of a trained GM-VAE on the MI355X HIP path: z_r / z_n from the chosen (or a drawn) rhythm- and note-density component, decoded and written
as MIDI files (see music-fader-nets_amd/latent.py; the package directory is not a Python identifier, so it is loaded through mfn_import)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mfn_import import load_package  # noqa: E402

load_package()
from music_fader_nets_amd.latent import main  # noqa: E402

if __name__ == "__main__":
    main()
