"""The reference's ``script/test_onset_model.sh`` (``trainer.test`` of ``main.module_onset.Model`` with its ``log_annotations`` /
``concat_annotations``) on the device: the onset net over the test split of a frame directory, the four epoch figures, and per video the
annotated and the predicted onset times under ``OUT/media/annotations/{target,pred}/<video>.times.csv``:

    python tools/test_onset_model.py --root_dir DIR --split_file test.txt --checkpoint onset.ckpt --out_dir OUT
                                     [--data_yaml cfg/data/data-onset-greatesthit-augment.yaml] [--batch_size 16] [--num_workers 8]

``--checkpoint``: a Lightning checkpoint (``state_dict`` with ``model.net.model.*`` / ``model.fc.*`` keys) or a bare state dict of the net.
``--data_yaml``: the data config whose ``test_frames_transforms`` block is the test chain (``null`` there, or no file: the dataset's default
chain).  The pred directory feeds ``tools/pack_onset_preds.py``.  syncfusion_amd/onset_test.py says what is restated."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root_dir", type=str, required=True)
    ap.add_argument("--split_file", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--data_yaml", type=str, default=None)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--num_workers", type=int, default=8)
    ap.add_argument("--frame_file_suffix", type=str, default=".jpg")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("test_onset_model: no GPU visible (the net has no CPU path)")
    from syncfusion_amd import OnsetModel, VideoOnsetNet, config, test_onset_model

    model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False))       # the optimizer arguments play no part in a test run
    ckpt = torch.load(a.checkpoint, map_location="cpu")
    sd = ckpt.get("state_dict", ckpt)
    if any(k.startswith("model.") for k in sd):
        model.load_state_dict(sd)
    else:
        model.model.load_state_dict(sd)
    chain = None
    if a.data_yaml:
        node = config.load_yaml(a.data_yaml)["data"]["init_args"].get("test_frames_transforms")
        chain = config.instantiate_frames_transforms(node) if node is not None else None
    res = test_onset_model(model, a.root_dir, a.split_file, a.out_dir, batch_size=a.batch_size, frames_transforms=chain,
                           frame_file_suffix=a.frame_file_suffix, num_workers=a.num_workers)
    for key in ("loss/test", "metrics/test/AP", "metrics/test/Acc", "metrics/test/OnsNumAcc"):
        print(f"{key}: {res[key]:.6f}")
    n_pred = sum(len(v["pred"]) for v in res["videos"].values())
    print(f"{len(res['videos'])} videos, {n_pred} predicted onsets -> {os.path.join(a.out_dir, 'media', 'annotations')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
