"""The reference's FAD evaluation (``main.evaluation.evaluate_fad``, run by script/evaluate_diffusion.py:31-36) on the device: VGGish embeddings
of every wav of ``--gt_path`` (the background set) and ``--experiment_path`` (the generated set), their Gaussian statistics and the Fréchet
distance, printed in the reference's format:

    FAD = 1.2345

    python tools/evaluate_fad.py --experiment_path DIR --gt_path DIR --weights vggish.pth [--out metrics.csv] [--batch_size 64]

``--weights``: a torchvggish ``.pth`` state dict (``pproc.*`` keys are ignored); without it the environment variable
SYNCFUSION_VGGISH_WEIGHTS names the file.  Nothing is downloaded.  ``--out`` writes the one-line csv the reference's DataFrame gives
(header ``,FAD``, row ``0,<value>``).  syncfusion_amd/fad.py says what is restated from the published algorithm and is still unpinned."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--experiment_path", type=str, required=True)
    ap.add_argument("--gt_path", type=str, required=True)
    ap.add_argument("--weights", type=str, default=None)
    ap.add_argument("--out", type=str, default=None, help="csv file to write")
    ap.add_argument("--batch_size", type=int, default=64)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("evaluate_fad: no GPU visible (the network has no CPU path)")
    from syncfusion_amd.fad import evaluate_fad, write_metrics_csv

    res = evaluate_fad(a.experiment_path, a.gt_path, weights=a.weights, batch_size=a.batch_size)
    print(f"FAD = {res['FAD']}")
    if a.out:
        write_metrics_csv(a.out, res["FAD"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
