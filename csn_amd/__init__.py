"""csn_amd — MI355X-native cross-shape attention (the hot path of marios2019/CSN's MID-FC/csa_models.py).

    from csn_amd.csa_models import get_model, CrossShapeAt, MultiHeadAttention, ScaledDotProductAttention

The attention arithmetic lives in csn_amd/libcsn_hip.so (C ABI: include/csn_hip.h, sources: csn_amd/csrc).
"""
from ._lib import CsnError, build, lib, LIB_PATH  # noqa: F401


def set_math_mode(mode) -> None:
    """Process-wide default arithmetic of the contractions: 'fp32' (exact fp32 matrix cores), 'bf16x3' (the library's
    default: three bf16 products per fp32 product, inside the 1e-4 contract), 'bf16' / 'fp16' (one product; outside it).
    Per model: ``get_model(..., math=...)``; per block of calls: ``csn_amd.functional.math_mode``."""
    from . import functional as CF
    from . import _lib
    _lib.check(lib().csn_set_math_mode(CF.mode_id(mode)), "csn_set_math_mode")

__version__ = "0.1.0"

# the MinkowskiNet head's loss, metrics and train / test steps (MinkowskiNet/lib/trainer_csn.py:188-224, 400-500)
from .minkowski_training import (SegBatch, SegMeter, evaluate, load_me_head_state, neighbor_batches, seg_loss,  # noqa: E402,F401
                                 train_iter)

# sparse 3D convolution on voxel rows: the primitive of the HRNet backbone (MinkowskiNet/models/hrnet.py:39-53, 89-111, 233-239)
from .minkowski_conv import (KernelMap, SparseBasicBlock, SparseConv3d, SparseConvTranspose3d, build_kernel_map,  # noqa: E402,F401
                             sparse_conv3d)
# the kernel-2 stride-2 convolution and its transposed form over an octant map (MinkowskiNet/models/res16unet.py: conv*s2, convtr*s2)
from .minkowski_conv import (OctantMap, SparseConvDown2, SparseConvUp2, build_octant_map, cat_conv3d,  # noqa: E402,F401
                             octant_conv_down, octant_conv_up)

# the HRNet backbone and HRNetSimCSN on voxel rows, on the fused convolution + BatchNorm kernels (MinkowskiNet/models/hrnet.py:31-163,
# 296-454)
from .minkowski_hrnet import (HRBasicBlock, HRNetBackbone, HRNetSimCSN2S, HRNetSimCSN3S, HRNetSimCSN4S, VoxelPyramid,  # noqa: E402,F401
                              bn_act, build_pyramid, conv_stats, load_me_hrnet_state)
from .minkowski_hrnet import GroupedPyramid, bn_act_groups, conv_stats_groups, group_pyramid, merge_batches  # noqa: E402,F401
# the plain segmentation networks (hrnet.py:214-293) and the backbone's one-launch-per-convolution inference primitive, on fp32
# or (maps16_dtype: math mode "bf16" / "fp16" with rows_single_product) 16-bit maps
from .minkowski_hrnet import (HRNetSeg, HRNetSeg2S, HRNetSeg3S, HRNetSeg4S, load_me_seg_state,  # noqa: E402,F401
                              maps16_dtype, sparse_conv_bn_act)
# bf16 activation maps of the backbone's training graph (tuning.train_maps16): the map type conv_stats / bn_act take and give, and
# whether the math mode and rows_single_product admit it right now
from .minkowski_hrnet import Map16, train_maps16_open  # noqa: E402,F401

# the Res16UNet family (MinkowskiNet/models/res16unet.py) on the octant convolutions and the fused blocks; octant_conv_bn_act is the
# inference primitive of its resolution changes, on fp32 maps or (single_product / 16-bit tensors, where maps16_dtype() names a
# type) as one 16-bit product on fp32 or 16-bit maps; octant_conv_stats / cat_conv_stats are the training nodes of
# tuning.unet_fused_tail (the BatchNorm statistics from the product's epilogue; they feed bn_act)
from .minkowski_unet import (Res16UNet14, Res16UNet14A, Res16UNet14A2, Res16UNet14B, Res16UNet14B2, Res16UNet14B3,  # noqa: E402,F401
                             Res16UNet14C, Res16UNet14D, Res16UNet18, Res16UNet18A, Res16UNet18B, Res16UNet18D, Res16UNet34,
                             Res16UNet34A, Res16UNet34B, Res16UNet34C, Res16UNet50, Res16UNet101, Res16UNetBase, UNetBasicBlock,
                             UNetPyramid, build_unet_pyramid, cat_conv_stats, load_me_unet_state, octant_conv_bn_act,
                             octant_conv_stats)

# point fields: the points of a batch quantised to voxel rows, and voxel logits interpolated back onto the points
# (MinkowskiNet/lib/trainer_csn.py:236-260 TensorField(...).sparse(), :200-205 and :463-471 soutput.interpolate(field))
from .minkowski_field import PointField, batch_points  # noqa: E402,F401

# resident point collections: a category's points on the device, normalised once, augmented and collated per batch
# (MinkowskiNet/lib/dataset.py:104-126, 221-252, lib/transforms.py:12-89, 195-225, lib/voxelizer.py:34-45)
from .minkowski_points import AugmentParams, AugmentSpec, PointBatch, PointCollection  # noqa: E402,F401

# the training procedure around them: optimizer, schedules, the patience-driven graph rebuilds, checkpoints and resume
# (MinkowskiNet/lib/solvers.py, lib/trainer_csn.py:20-186, 262-395, lib/dataloader.py; the CLI is ``python -m csn_amd.train_csn``)
from .minkowski_solvers import TrainConfig, initialize_optimizer, initialize_scheduler  # noqa: E402,F401
from .minkowski_trainer import CSNTrainer, InfSampler, PatienceState  # noqa: E402,F401
# the HRNetSeg baseline's procedure and test mode for both model families (lib/trainer_seg.py, tasks/main_csn.py:121-141,
# tasks/main_seg.py:124-130; the CLIs are ``python -m csn_amd.train_seg`` and ``--is_train False`` of either, and
# ``python -m csn_amd.collect_partnet_results`` gathers the result files)
from .minkowski_trainer import BestValues, SegTrainer, checkpoint_num_labels, load_model_state, test_split  # noqa: E402,F401
