"""music-fader-nets_amd: MI355X-native GM-VAE (MusicAttrRegGMVAE) training / inference path of Music FaderNets.

The directory name contains '-' (it follows the upstream repo name), so import it through
``mfn_import.load_package()`` at the repo root, which registers it as ``music_fader_nets_amd``.
"""
from . import arith  # noqa: F401
from .gmm_model import MusicAttrRegGMVAE  # noqa: F401
from .trainer import GMVAETrainer, VAETrainer, beta_schedule, convert_to_one_hot  # noqa: F401
from .vae_model import MusicAttrRegVAE  # noqa: F401
from .model_v2 import MusicAttrCVAE, MusicAttrFaderNets, MusicAttrSingleVAE  # noqa: F401
from .trainer_v2 import CVAETrainer, FaderTrainer, GLSRTrainer, SingleVAETrainer  # noqa: F401
from .constrain import Constraints, EventVocab  # noqa: F401
from .decode import beam_decode, clean_output, continue_from, fader_sweep, fed_tokens, greedy_decode, sample_decode  # noqa: F401
from .epochs import cpu_state_dict, evaluation_phase, training_phase, training_phase_v2  # noqa: F401
from .attributes import EventGrid, controllability, event_attributes, sweep_scores  # noqa: F401
from .notes import NoteVocab, Notes, Piece, estimate_chroma, notes_to_tokens, stitch_notes, tokens_to_notes  # noqa: F401
from .midi import MidiNotes, midi_segments, read_midi, write_midi, write_midis  # noqa: F401
from .transfer import Transferred, transfer_midi, transfer_piece  # noqa: F401
from .latent import generate, latent_classes, mix_latents, morph, prior_latents  # noqa: F401
from .likelihood import Likelihood, likelihood_report, marginal_likelihood  # noqa: F401
from .disentangle import Disentanglement, disentanglement, disentanglement_report  # noqa: F401
from .report import RowMatches, ScoredTokens, TokenScores, match_rows, reconstruction_report, score_tokens, token_scores  # noqa: F401
from .evaluators import GMMNoteEvaluator, GMMRhythmEvaluator, arousal_transfer, run_through_gmm  # noqa: F401

__all__ = ["MusicAttrRegGMVAE", "MusicAttrRegVAE", "MusicAttrSingleVAE", "MusicAttrCVAE", "MusicAttrFaderNets", "SingleVAETrainer", "CVAETrainer",
           "FaderTrainer", "GLSRTrainer", "GMVAETrainer", "VAETrainer", "beta_schedule", "convert_to_one_hot", "clean_output", "fader_sweep",
           "greedy_decode", "sample_decode", "beam_decode", "Constraints", "EventVocab", "EventGrid", "event_attributes", "sweep_scores", "controllability", "NoteVocab", "Notes", "tokens_to_notes", "notes_to_tokens", "estimate_chroma", "MidiNotes", "read_midi", "write_midi", "write_midis", "midi_segments", "continue_from", "fed_tokens", "training_phase", "training_phase_v2", "cpu_state_dict", "GMMRhythmEvaluator", "GMMNoteEvaluator", "arousal_transfer", "run_through_gmm", "evaluation_phase", "token_scores", "match_rows", "score_tokens",
           "reconstruction_report", "TokenScores", "RowMatches", "ScoredTokens", "Piece", "stitch_notes", "Transferred", "transfer_piece", "transfer_midi",
           "prior_latents", "generate", "mix_latents", "morph", "latent_classes",
           "Likelihood", "marginal_likelihood", "likelihood_report",
           "Disentanglement", "disentanglement", "disentanglement_report"]
