"""The reference's ``script/evaluate_onset.py`` (run by ``script/evaluate_onset.sh``) on the device front end: onset detection on every wav of
``--tar_dir`` and ``--gen_dir``, then onset-count accuracy, detection accuracy and detection AP of each generated file against the target of
the same name, and the reference's closing line in its format:

    #onset acc: 0.8333, detection acc: 0.7500, detection ap: 0.8125

    python tools/evaluate_onset.py --gen_dir DIR [--tar_dir data/AMT_test/target_sound] [--delta 0.1] [--remove_head S] [--multi_delta]
                                   [--batch_size 64] [--per_file]

``--plt`` and ``--longer_det`` of the reference are not offered (syncfusion_amd/evaluation.py says what is restated and what is defined
where the reference is not)."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gen_dir", type=str, required=True)
    ap.add_argument("--tar_dir", type=str, default="data/AMT_test/target_sound")
    ap.add_argument("--delta", type=float, default=0.1)
    ap.add_argument("--remove_head", type=float, default=None)
    ap.add_argument("--multi_delta", action="store_true")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--per_file", action="store_true", help="one line per generated file before the summary")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("evaluate_onset: no GPU visible (the detector has no CPU path)")
    from syncfusion_amd.evaluation import evaluate_onsets, summary_line

    res = evaluate_onsets(a.gen_dir, a.tar_dir, delta=a.delta, remove_head=a.remove_head, multi_delta=a.multi_delta, batch_size=a.batch_size)
    if a.per_file:
        for name, r in res["per_file"].items():
            note = f"  (resampled from {r['resampled_from']} Hz)" if r["resampled_from"] else ""
            print(f"{name}: target {r['n_tar']} generated {r['n_gen']} count match {r['count_match']} acc {r['acc']:.4f} ap {r['ap']:.4f}{note}")
    print(summary_line(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
