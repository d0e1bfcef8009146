"""The reference's ``run_prepare_gh_gt_pred.sh`` step (``main.dataset_diffusion.prepare_gt_for_fad``): the ground-truth chunks of a shard set as
wav files, under the names ``generate_dataset`` gives the generated ones -- the ``--gt_path`` of ``tools/evaluate_fad.py``:

    python tools/prepare_gt.py --shards 'DIR/test-{000..003}.tar' --out_dir GT [--sample_rate 48000] [--chunk_size 262144]
                               [--downsample_rate 16000] [--one_chunk_per_track] [--batch_size 16]

The chunks are cut as for generation (``shards.sfx_chunks``, ``cut_prefix`` off); with ``--downsample_rate`` they are resampled on the
device."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shards", type=str, nargs="+", required=True)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--sample_rate", type=int, default=48000)
    ap.add_argument("--chunk_size", type=int, default=2 ** 18)
    ap.add_argument("--downsample_rate", type=int, default=None)
    ap.add_argument("--one_chunk_per_track", action="store_true")
    ap.add_argument("--batch_size", type=int, default=16)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("prepare_gt: no GPU visible (the resampler has no CPU path)")
    from syncfusion_amd import prepare_gt_for_fad
    from syncfusion_amd.shards import sfx_chunks

    data = sfx_chunks(a.shards, sample_rate=a.sample_rate, chunk_size=a.chunk_size, cut_prefix=False,
                      one_chunk_per_track=a.one_chunk_per_track, device=torch.device("cuda"))
    written = prepare_gt_for_fad(a.out_dir, data, batch_size=a.batch_size, num_workers=0, sample_rate=a.sample_rate,
                                 one_chunk_per_track=a.one_chunk_per_track, downsample_rate=a.downsample_rate)
    print(f"{len(written)} files -> {a.out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
