"""Pack the predicted onsets of ``tools/test_onset_model.py`` into shards: every sample of the input shards gets a ``<key>.times.pred.csv``
member from ``PRED_DIR/<basename(key)>.times.csv`` -- the ``test_onset_preds.tar`` the reference's predicted-onset generation run reads
(``times.pred.csv`` in main/dataset_diffusion.py:28-34):

    python tools/pack_onset_preds.py --pred_dir OUT/media/annotations/pred --out_dir SHARDS_PRED [--skip_empty] SHARD [SHARD ...]

Each ``SHARD`` (a path, a glob pattern or a ``{000..012}`` range) is written under its own base name into ``--out_dir``.  Keys without a
prediction file and keys whose file is empty are listed; ``--skip_empty`` leaves those samples out (the slicer asserts on a sample without
predicted onsets, as the reference does)."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("shards", nargs="+")
    ap.add_argument("--pred_dir", type=str, required=True)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--skip_empty", action="store_true")
    a = ap.parse_args(argv)
    from syncfusion_amd import pack_onset_preds
    from syncfusion_amd.shards import expand_shards

    os.makedirs(a.out_dir, exist_ok=True)
    for shard in expand_shards(a.shards):
        out = os.path.join(a.out_dir, os.path.basename(shard))
        if os.path.abspath(out) == os.path.abspath(shard):
            raise SystemExit(f"pack_onset_preds: {out} is the input shard")
        missing, empty = pack_onset_preds(shard, a.pred_dir, out, skip_empty=a.skip_empty)
        print(f"{shard} -> {out}: {len(missing)} keys without a prediction file, {len(empty)} with an empty one")
        for key in missing:
            print(f"  missing: {key}")
        for key in empty:
            print(f"  empty:   {key}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
