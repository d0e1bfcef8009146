"""syncfusion_amd -- MI355X (gfx950) implementation of SyncFusion's generation hot path.

Public surface = the reference's own: ``DiffusionModel`` / ``UNetV0`` / ``VDiffusion`` /
``VSampler`` (audio_diffusion_pytorch), ``Encoder1d`` (audio_encoders_pytorch), ``VideoOnsetNet``
(main.onset_net), ``Model`` (main.module_diffusion) and ``generate_dataset`` (main.generation).  All arithmetic
runs in ``lib/libsyncfusion_amd.so`` (hand-written HIP, C ABI in include/syncfusion_amd.h).
"""
from . import _lib  # noqa: F401
from . import audio_features, autograd, clap, clap_text, denoise, evaluation, fad, frame_transforms, jpeg, onset_test, onset_training, shards, training, video_chunks  # noqa: F401
from .config import instantiate, instantiate_class, instantiate_frames_transforms, instantiate_model_yaml
from .diffusion import DiffusionModel, LinearSchedule, PowerSchedule, UNetV0, VDiffusion, VInpainter, VSampler
from .solvers import solver_table
from .guidance import evaluation_rows, plan_segments, scale_table
from .audio_features import MelSpectrogram, mel_filterbank, onset_detect, onset_strength
from .denoise import SpectralGateConfig, chunk_rows, istft, merge_rows, reduce_noise, stft
from .encoder1d import Encoder1d
from .evaluation import evaluate_onsets
from .clap import ClapAudioConfig, ClapAudioEmbedder
from .clap_text import ClapEmbedder, ClapTextConfig, ClapTokenizer
from .fad import VGGish, VGGishConfig, embedding_statistics, evaluate_fad, frechet_distance
from .jpeg import JpegInfo, decode_jpeg_batch, parse_jpeg
from .generation import (generate_batch, generate_dataset, generate_long, inpaint_batch, long_windows, prepare_gt_for_fad,
                         regions_to_keep_mask, vary_batch)
from .module import Model, RandomEmbedder
from .module_onset import Model as OnsetModel
from .onset_net import VideoOnsetNet
from .onset_test import OnsetTestStage, annotation_rows, pack_onset_preds, test_onset_model
from .video_chunks import run_onset_test
from .onset_training import GraphedOnsetTrainStep
from .onset_glue import cut_prefix_crop, onsets_to_track
from .resample import resample
from .training import allreduce_gradients

__all__ = ["DiffusionModel", "UNetV0", "VDiffusion", "VSampler", "LinearSchedule", "Encoder1d", "VideoOnsetNet", "Model", "OnsetModel",
           "GraphedOnsetTrainStep",           "RandomEmbedder", "generate_batch", "generate_dataset", "instantiate", "instantiate_model_yaml", "onsets_to_track", "cut_prefix_crop", "resample",
           "allreduce_gradients", "frame_transforms", "instantiate_class", "instantiate_frames_transforms",
           "audio_features", "evaluation", "MelSpectrogram", "mel_filterbank", "onset_detect", "onset_strength", "evaluate_onsets",
           "fad", "VGGish", "VGGishConfig", "embedding_statistics", "frechet_distance", "evaluate_fad",
           "VInpainter", "inpaint_batch", "generate_long", "long_windows", "regions_to_keep_mask",
           "onset_test", "OnsetTestStage", "annotation_rows", "pack_onset_preds", "test_onset_model", "prepare_gt_for_fad",
           "jpeg", "JpegInfo", "decode_jpeg_batch", "parse_jpeg", "run_onset_test",
           "clap", "ClapAudioConfig", "ClapAudioEmbedder", "clap_text", "ClapEmbedder", "ClapTextConfig", "ClapTokenizer",
           "denoise", "SpectralGateConfig", "reduce_noise", "stft", "istft", "chunk_rows", "merge_rows",
           "solver_table", "PowerSchedule", "vary_batch", "scale_table", "plan_segments", "evaluation_rows"]
__version__ = "0.1.0"
