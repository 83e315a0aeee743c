#!/usr/bin/env python3
"""Gather the test results of every category: what MinkowskiNet/lib/collect_partnet_results.py does.

    python -m csn_amd.collect_partnet_results <base_dir> [K]

Walks ``<base_dir>/<experiment>/*evaluation/results/results_log.txt`` — the file test mode writes (``csn_amd.test_split``) — over the
experiments in sorted order; with ``K`` only the experiments whose directory name contains ``-k<K>-``.  Prints the Part IoUs and the
Shape IoUs as lists and as ``=SPLIT("...", ",")`` lines for a spreadsheet.
"""
import os
import sys
from typing import List, Optional, Tuple

RESULTS = os.path.join("results", "results_log.txt")


def collect_results(base_dir: str, K: Optional[str] = None) -> Tuple[List[float], List[float]]:
    """(part_ious, shape_ious), one entry per ``*evaluation`` directory.  A missing ``results_log.txt`` is a ``FileNotFoundError``
    naming the file."""
    if not os.path.isdir(base_dir):
        raise NotADirectoryError(f"'{base_dir}' is not a directory")
    tag = None if K is None else f"-k{K}-"
    experiments = sorted(os.path.join(base_dir, f) for f in os.listdir(base_dir) if tag is None or tag in f)
    part_iou, shape_iou = [], []
    for experiment in experiments:
        if not os.path.isdir(experiment):
            continue
        for f in sorted(os.listdir(experiment)):
            if not f.endswith("evaluation"):
                continue
            results_log = os.path.join(experiment, f, RESULTS)
            if not os.path.isfile(results_log):
                raise FileNotFoundError(f"no results log at '{results_log}'")
            with open(results_log) as fin:
                for line in fin:
                    words = line.strip().split()
                    if not words:
                        continue
                    if words[0].lower() == "part":
                        part_iou.append(float(words[-1]))
                    if words[0].lower() == "shape":
                        shape_iou.append(float(words[-1]))
    return part_iou, shape_iou


def _split_line(values: List[float]) -> str:
    return '=SPLIT("' + ",".join(str(v) for v in values) + '", ",")'


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) not in (1, 2):
        print(__doc__, file=sys.stderr)
        return 2
    part_iou, shape_iou = collect_results(argv[0], argv[1] if len(argv) == 2 else None)
    print("PART IOU:")
    print("---------")
    print(part_iou)
    print(_split_line(part_iou))
    print("SHAPE IOU:")
    print("----------")
    print(shape_iou)
    print(_split_line(shape_iou))
    return 0


if __name__ == "__main__":
    sys.exit(main())
