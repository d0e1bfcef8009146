"""The --audio_denoise step of the reference's preprocessing (script/gh_preprocess_videos.py:91-100) on the device: every
`*.resampled.wav` under --input_dir becomes `*.resampled_denoised.wav` beside it, through syncfusion_amd.reduce_noise
(n_fft 1024, hop 256, the non-stationary mask unless --stationary).

    python tools/preprocess_audio.py --input_dir DIR [--audio_bitdepth 32|16] [--stationary] [--device cuda|cpu]

--audio_bitdepth 32 writes IEEE-float wav (save_wav), 16 writes 16-bit PCM (save_wav_pcm16); 24 is refused.  --device cpu runs the fp64
restatement of tests/denoise_ref.py on the host instead of the library: a slow cross-check, not a product path.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SUFFIX_IN, SUFFIX_OUT = ".resampled.wav", ".resampled_denoised.wav"


def denoise_file(src: Path, dst: Path, bitdepth: int, stationary: bool, device: str) -> None:
    from syncfusion_amd.generation import load_wav, save_wav, save_wav_pcm16

    wav, sr = load_wav(src)
    if device == "cpu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import denoise_ref

        out = torch.from_numpy(denoise_ref.reduce_noise_ref(wav.numpy(), sr, n_fft=1024, hop=256, stationary=stationary)).to(torch.float32)
    else:
        from syncfusion_amd.denoise import reduce_noise

        out = reduce_noise(wav, sr, stationary=stationary, n_fft=1024, hop_length=256, device=device).cpu()
    (save_wav if bitdepth == 32 else save_wav_pcm16)(dst, out, sr)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input_dir", required=True)
    ap.add_argument("--audio_bitdepth", type=int, default=32)
    ap.add_argument("--stationary", action="store_true")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.audio_bitdepth == 24:
        raise SystemExit("preprocess_audio: 24-bit output is not supported (no 24-bit writer or reader here); use --audio_bitdepth 32 or 16")
    if a.audio_bitdepth not in (16, 32):
        raise SystemExit(f"preprocess_audio: --audio_bitdepth must be 32 or 16, got {a.audio_bitdepth}")
    files = sorted(p for p in Path(a.input_dir).rglob("*" + SUFFIX_IN))
    if not files:
        raise SystemExit(f"preprocess_audio: no *{SUFFIX_IN} under {a.input_dir}")
    for src in files:
        dst = src.with_name(src.name[:-len(SUFFIX_IN)] + SUFFIX_OUT)
        denoise_file(src, dst, a.audio_bitdepth, a.stationary, a.device)
        print(f"{src} -> {dst}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
