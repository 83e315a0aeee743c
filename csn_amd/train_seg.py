#!/usr/bin/env python3
"""Train an ``HRNetSeg``, the baseline cross-shape attention is measured against (or a ``Res16UNet``: ``--model Res16UNet34C``), or test one: what MinkowskiNet/tasks/main_seg.py
does, on ``csn_amd.minkowski_trainer.SegTrainer`` and ``test_split``.

    python -m csn_amd.train_seg --log_dir <out> --model HRNetSeg3S --lr 0.05 --optimizer SGD --batch_size 8
                                --scheduler ReduceLROnPlateau --max_epoch 200
                                --data_root <sem_seg_h5/Category-3> --train_files train-00.h5 ... --val_files val-00.h5 ...
    python -m csn_amd.train_seg --is_train False --weights <out>/weights.pth --log_dir <out>/evaluation --model HRNetSeg3S
                                --data_root <...> --test_files test-00.h5 ...

The arguments are those of ``python -m csn_amd.train_csn`` (see there) without ``--k_neighbors``, ``--d_model`` and ``--n_head``:
scripts/train_hrnet.sh is the first line, scripts/test_hrnet.sh the second.  ``--iter_size`` other than 1 is refused by the trainer.
Test mode needs ``--weights`` and ``--test_files`` (or ``--synthetic N``) and no other split.
"""
import sys

from . import train_csn

# (the parser's default is the last name)
MODELS = ("Res16UNet14", "Res16UNet14A", "Res16UNet14A2", "Res16UNet14B", "Res16UNet14B2", "Res16UNet14B3", "Res16UNet14C", "Res16UNet18",
          "Res16UNet18A", "Res16UNet18B", "Res16UNet34", "Res16UNet34A", "Res16UNet34B", "Res16UNet34C", "HRNetSeg2S", "HRNetSeg3S")


def build_parser():
    return train_csn.build_parser("python -m csn_amd.train_seg", MODELS, __doc__, csn=False)


def parse_args(argv=None):
    """(TrainConfig with ``k_neighbors = 0``, the remaining arguments).  Exits with status 2 on an unknown argument or an unusable
    combination."""
    return train_csn.parse_args(argv, build_parser())


def main(argv=None) -> int:
    cfg, args = parse_args(argv)
    return train_csn.run(cfg, args, csn=False)


if __name__ == "__main__":
    sys.exit(main())
