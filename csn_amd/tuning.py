"""Data-flow switches of the step and the bench's event hook — kept out of the product modules.

Every switch selects between two forms of the SAME arithmetic (a fused pass and the plain pass it replaced, or two data
flows of the attention backward); the defaults are the measured-faster forms.  With ONE exception nothing here
changes results beyond fp32 rounding: ``rows_single_product`` selects arithmetic — with it the bf16 / fp16 math modes round the
operands of the MinkowskiNet row products to 16 bits instead of running them as bf16x3 (off by default).
`tests/test_gpu_module.py::test_fused_data_flow_equals_the_unfused_one` and `tests/test_gpu_flash.py` flip the others through ``override`` to check one form against the other (`bench.py` times the launches
through csn_amd._lib.set_call_hook, not through anything here).  The state is process-wide on purpose: autograd runs the backward on its own threads, and a step must see the
same switches in both passes.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field, fields, replace
from typing import Dict, Optional

# attention backward data flows (resolved once per step by csn_amd.functional.step_form, run by _MHAEvals):
KEEP_SCORES = 0      # the forward writes the raw scores S, the dQ kernel reads them back and leaves P / dS for the dK / dV products
RECOMPUTE_DQ = 1     # the forward keeps only lse; the dQ kernel rebuilds S = Qs K^T (one more product), P / dS still travel
FLASH = 2            # ... and a key-stationary kernel rebuilds P / dS for dK / dV: no score-sized tensor exists at all


@dataclass
class Tuning:
    kv_tiles: bool = True            # 16-bit modes: K / V leave the projection as tile planes (csn_project_f32, out_split = 2)
    fused_point_sums: bool = True    # False: pooled sums by a streaming pass over the maps
    link_mix: bool = True            # False: the mix backward writes per-evaluation gradient maps
    # linked mix, bf16x3 at d = 256, plans whose mixed evaluations are not pooled: the mix's reductions (d comp, d gamma, d beta)
    # come out of the LayerNorm backward of the mixed evaluations, which the mix's backward launches itself.  False: a pass of
    # their own over the maps (csn_mix_bwd_f32) and one LayerNorm backward launch over all evaluations
    fused_mix_bwd: bool = True
    grouped_dkv: bool = True         # False: dK / dV by one read-modify-write launch per colour
    grouped_dq: bool = True          # False: dQ likewise
    grouped_fwd: bool = True         # 16-bit modes: the forward's evaluations grouped by query slot (the query operand staged once per group)
    fused_compat_head: bool = True   # False: the compatibility head as torch ops (two nn.Linear, normalize, einsum, softmax)
    act16: bool = True               # bf16 / fp16 modes, linked mix: Qs, Ctx, xhat, dZ, dCtx between the launches as 16-bit maps
    # bf16x3, kept scores: S and the P / dS planes stored [key tile][query][32 keys], so that every wave instruction that touches
    # them moves 1 KB in one piece.  Measured +-0 over the config-3 step (27.69 vs 27.68 ms, profiles/r4k_ab_score_layout.txt):
    # the 16-byte pieces 2 KB apart were not what the dQ kernel or the dV / dK products wait for.  Off; kept as the measured
    # form (tests/test_gpu_score_layout.py holds it to the row-major step bit for bit)
    tile_major_scores: bool = False
    # Q, K and V of all slots from ONE pass over x (csn_project_qkv_f32: three row sets of the streaming kernel walking the same
    # chunks) where every slot needs all three.  The same bits, 1.15 GB less HBM traffic per step (FETCH / WRITE passes), and not
    # faster: the launch alone 1.96 ms against 0.54 + 1.06 + launch gap = 1.78 for the two calls, the config-3 step 26.95 against
    # 26.99 ms (profiles/r4t_qkv_one_pass.txt).  Off; kept as the measured form (tests/test_gpu_wx.py holds it bit for bit)
    qkv_one_pass: bool = False
    # bf16x3 at d = 256, kept scores, grouped dQ and dK / dV: the dQ kernel leaves the scores untouched (no P planes written over
    # them), a key-stationary kernel forms dV from the scores (csn_block_attn_bwd_dv_scores_f32) and the plane product runs for dK
    # alone — the dQ launch writes 5.2 GB less per config-3 step (the dV kernel reads S where the product read P).  dQ and dK keep their bits; dV is the same three products summed in another
    # order.  Taken in either score layout where csn_attn_bwd_dv_scores_available says so; the default is what profiles/dv_scores_ab_step.txt measured
    dv_from_scores: bool = True
    # One head of the model's width (H = 1, C = d = 256, the configuration the metric is quoted on), bf16x3, kept scores,
    # no input gradients: W_k is folded into W_q and W_v into W_fc (M = W_k^T W_q / t, W_fv = W_fc W_v, exact fp32
    # products of csn_fold_weights_f32), the attention kernels run on the tile planes of x itself as both "K" and "V"
    # (csn_tile_planes_f32), and the backward is ONE dQ call that writes nothing score-sized (probs_tiles = 3) plus two 256-row
    # weight gradients, unfolded to dW_q, dW_k, dW_v, dW_fc by csn_unfold_wgrads_f32.  K, V, dK, dV, dscores and their launches do not
    # exist.  Unlike its neighbours this re-associates products: results move by fp32 / bf16x3 rounding (both forms measured against
    # a float64 restatement: DESIGN.md §2 "Folded projections"; tests/test_gpu_folded.py for the kernels and the default step,
    # tests/test_gpu_folded_plans.py for every plan, live switch and block edge).  The dropout masks are the same bits.  Where
    # any condition fails the unfolded calls run and give their bits.  The decision never looks at the grad mode.
    # One more condition lives here: an ``override`` block that NAMES a switch which exists only in the unfolded step
    # (UNFOLDED_ONLY: dv_from_scores, grouped_dkv, qkv_one_pass — the folded step has no dV / dK product and no K | V projection,
    # so it would ignore them silently) asks for the unfolded step — whatever value it gives the switch: an A/B of such a switch
    # (scripts/ab_step.py, tests/test_gpu_dv_scores.py::test_module_step_with_dv_from_scores) keeps measuring the launches it names
    folded_projections: bool = True
    # the folded step's dQ kernel (k = v = the planes of x) requests every 32-key tile ONCE and commits the same registers into
    # both LDS images, instead of once per image (attn_bf16x3.hip KV_SAME; the library's key CSN_DEV_KV_SAME, set before the
    # launch).  The same LDS contents, the same bits (tests/test_gpu_kv_same.py); timing: profiles/folded_tiles_ab_step.txt
    kv_same: bool = True
    # the folded step's dQ kernel runs as four waves and 64 queries per work-group on ONE LDS tile image that serves both of a
    # tile's reads, two independent work-groups per CU, instead of eight waves on two images (attn_bf16x3.hip WG64; the library's
    # key CSN_DEV_ATTN_WG64, set before the launch; off: the instance ``kv_same`` selects).  The same arithmetic per query row, the
    # same bits (tests/test_gpu_attn_wg64.py); timing: profiles/wg64_ab_step.txt
    wg64: bool = True
    named: frozenset = frozenset()   # the switches the enclosing override blocks name (kept by ``override``; not a switch itself)
    # attention backward data flow by (math mode of the backward: 1 bf16x3, 2 bf16 — fp16 forwards run their backward in 2;
    # head width), or by mode alone; taken where the kernels have an instance for it (csn_attn_bwd_grouping bits 2 / 3),
    # KEEP_SCORES otherwise.  Measured per mode and width, DESIGN.md §4 "data flow A/B": at d = 256 the extra matrix products
    # cost what the score traffic saves, at d <= 128 a score costs the same bytes for a fraction of the FLOPs
    score_flow: Dict[object, int] = field(default_factory=lambda: {
        1: KEEP_SCORES,                                   # bf16x3 at d = 256: three LDS images of two planes do not fit one CU
        2: RECOMPUTE_DQ,                                  # one plane, d = 256: -4.7 % of the config-3 step (profiles/r3l_flow_ab_step.txt)
        **{(2, d): FLASH for d in (32, 64, 96, 128)},     # config 5: 18.5 -> 17.1 (recompute) -> 15.4 ms (flash)
        **{(1, d): FLASH for d in (32, 64, 96)}, (1, 128): RECOMPUTE_DQ})

    # cross-length / ragged attention (csn_amd.minkowski_attention._CrossMHA, hence MultiHeadAttention.forward, forward_varlen and
    # SimCSNHead): the score-free backward (csn_cross_attn_bwd_flash_f32 / csn_varlen_attn_bwd_flash_f32) — the forward keeps only
    # lse, nothing score-sized is saved or allocated.  False: never.  True: wherever csn_cross_attn_flash_available says so
    # (CsnError where it does not).  None: only when the three score-sized tensors of the kept flow exceed cross_score_budget
    # (cross_takes_score_free) — a call that fits keeps its flow, its bits and its memory
    cross_score_free: Optional[bool] = None
    # bytes for that automatic decision; None: what the device can still give at forward time (free device memory + what the
    # caching allocator holds but has not handed out)
    cross_score_budget: Optional[int] = None
    # kernel maps and voxel pyramids of DEVICE tensors (csn_amd.minkowski_conv.build_kernel_map, csn_amd.minkowski_hrnet.build_pyramid
    # with backend=None, hence PointField.pyramid and HRNetSimCSN.forward on bare coordinates) through the kernels of include/csn_hip.h
    # section 17 instead of one searchsorted per offset in torch ops; likewise the octant maps and the U-Net's pyramid
    # (build_octant_map, csn_amd.minkowski_unet.build_unet_pyramid, hence PointField.unet_pyramid and Res16UNet*.forward on bare
    # coordinates) through sections 17 and 22.  The same integers (tests/test_gpu_kernel_map.py, tests/test_gpu_octant_map.py), so every
    # launch downstream is the same launch.  CPU tensors keep the torch backend whatever this says.  Off: opt-in until the default is
    # flipped on its own (timing: DESIGN.md "Kernel maps" and "Native octant maps", scripts/bench_kernel_map.py, bench_unet_pyramid.py)
    native_kernel_maps: bool = False
    # math modes "bf16" / "fp16" on the MinkowskiNet side: fc_layer, the sparse convolutions and their statistics form (_RowsFC,
    # _SparseConv, _ConvStats) run ONE 16-bit product per operand pair (csn_set_thread_rows16; an fp16 forward runs its backward in
    # bf16) instead of bf16x3.  Unlike every other switch here this one selects ARITHMETIC: operands are rounded to 16 bits, the
    # results leave the 1e-4 contract of bf16x3 as those modes do on the attention side.  Modes fp32 / bf16x3 never see it.  Off:
    # opt-in until the default is flipped in a change of its own (errors and timing: DESIGN.md "Single-product row products")
    rows_single_product: bool = False
    # HRNetBackbone in eval mode with autograd disabled (validation, construct_shape_graph, test-time prediction; fused=True only):
    # every convolution + BatchNorm (+ residual, + ReLU) is ONE launch of include/csn_hip.h section 19 instead of sparse_conv3d +
    # bn_act, a branch sum accumulates in one buffer, and the concatenated result is written in place (no torch.cat).  A branch sum
    # is added in an order of its own, so results differ from the two-launch path by fp32 rounding.  Training, grad-enabled and
    # fused=False calls never see it.  Off: opt-in (bytes and timing: DESIGN.md "Inference backbone", scripts/bench_hrnet.py).
    # The Res16UNets under the same conditions (Res16UNetBase._forward_infer): section 19 for the stem and the blocks, section 23
    # for the eight resolution changes, a decoder level's [up | skip] input written in place, a convolution over more than 256
    # columns as a chain of two launches — again a summation order of its own (DESIGN.md "Inference U-Net", scripts/bench_unet.py)
    eval_epilogue: bool = False
    # HRNetBackbone's inference graph (where eval_epilogue already applies, and ONLY there) in math mode "bf16" / "fp16" with
    # rows_single_product: the maps between the launches are stored as bf16 / fp16 rows (include/csn_hip.h section 24) instead of
    # fp32 rows that their consumer's first instruction rounds to 16 bits anyway — gather bytes, map writes and residual reads halve.
    # The stem's input, the (N, out_channels) result and the launches that write its column blocks stay fp32.  Every product is the
    # same; a stored map (and a branch sum, per launch) is rounded once more, so results stay in the class those modes already have
    # (tests/test_gpu_maps16.py holds the graph bit for bit to the fp32-map graph with every stored map rounded once).  In every
    # other combination — modes fp32 / bf16x3, rows_single_product off, eval_epilogue off, training, grad enabled, fused=False — it
    # changes nothing: the same launches, the same bits.  The Res16UNets ignore it: their inference graph has switches of its own
    # (octant_single_product and unet_maps16, below).  Off: opt-in (bytes and timing: DESIGN.md
    # "16-bit inference maps", scripts/bench_hrnet_maps16.py)
    infer_maps16: bool = False
    # The Res16UNets' inference graph (where eval_epilogue already applies to them, and ONLY there) in math mode "bf16" / "fp16" with
    # rows_single_product.  octant_single_product: the eight resolution changes run as ONE 16-bit product per operand pair
    # (include/csn_hip.h section 25) instead of bf16x3 (section 23) — arithmetic, like rows_single_product, which by itself never
    # reaches the octant products; the maps stay fp32 and the kernel-3 / kernel-1 launches stay section 19.  unet_maps16: every
    # stored map between the launches is a bf16 / fp16 tensor (sections 24 and 25), the four [up | skip] buffers included; it implies
    # the single-product octant products.  The stem's input, a chain's running sum over more than 256 columns (an fp32 scratch map,
    # so that the sum is rounded once) and the last block's output, which ``final`` reads, stay fp32
    # (tests/test_gpu_unet16.py holds the graph bit for bit to the fp32-map graph with every stored map rounded once).  In every
    # other combination — modes fp32 / bf16x3, rows_single_product off, eval_epilogue off, training, grad enabled, fused=False —
    # both change nothing: the same launches, the same bits.  infer_maps16 stays ignored by these networks, and the HRNet classes
    # ignore these two.  Off: opt-in (bytes and timing: DESIGN.md "16-bit inference U-Net", scripts/bench_unet.py --infer)
    octant_single_product: bool = False
    unet_maps16: bool = False
    # A Res16UNet built with fused=True in TRAINING mode: the two layer kinds that still ran an ATen BatchNorm take the fused nodes
    # of the rest of the network.  Each of the eight resolution changes is octant_conv_stats (include/csn_hip.h section 26: the
    # octant product forms the BatchNorm statistics in its epilogue) + bn_act(relu=True); in a decoder block that reads more than
    # 256 columns conv1 and downsample.0 are cat_conv_stats (section 27: a chain over the parts, the last launch with the
    # statistics) and join the block's bn_act sums.  No ATen normalisation is left in the step; num_batches_tracked and the running
    # statistics advance as ATen's do.  Results differ from the ATen path by fp32 rounding (the statistics are merged from 32-row
    # partials in fp64, the normalisation is one fused multiply-add).  Eval mode, fused=False, the inference graph and the HRNet
    # classes never see it: the same calls, the same bits.  Off: opt-in (timing: DESIGN.md "Fused U-Net tail", scripts/bench_unet.py)
    unet_fused_tail: bool = False
    # kNN shape graphs (construct_shape_graph with screen=None, CrossShapeAt.get_knn_graph / get_knn_graph_big): an fp16 pass over all
    # pairs (csn_ragged_retrieval_screen_f16) names the candidates that provably cannot be among a row's top K — more than
    # 2 * screen_eps below its K-th best screen score — and only the rest are scored by the exact fp32 kernels.  The SAME integers
    # come out (tests/test_gpu_retrieval_screen.py); the fp32 measure alone ranks.  Off: opt-in — the share of pairs that survives the
    # screen on real PartNet features is not measured (DESIGN.md "fp16 screen of the shape graph", scripts/bench_retrieval_screen.py)
    retrieval_screen: bool = False

    # HRNetSimCSN.forward(queries, keys) with key batches: the K + 1 batches are merged into one coordinate set
    # (csn_amd.minkowski_hrnet.merge_batches), the backbone runs ONCE, and every BatchNorm takes its statistics per row group
    # (include/csn_hip.h section 20) — each batch stays its own BatchNorm batch, the running statistics see the batches in the same
    # order.  The weight gradients become one sum over all rows instead of K + 1 sums added by autograd: results differ from the
    # separate passes by rounding.  Batches given as prebuilt VoxelPyramids, an unfused backbone in training and merged maps past
    # the kernels' 2 GiB window keep the separate passes.  Off: opt-in (DESIGN.md "Grouped passes", scripts/bench_hrnet_groups.py)
    grouped_passes: bool = False
    # HRNetBackbone.forward on a fused=True backbone in TRAINING mode, math mode "bf16" with rows_single_product, on a plain
    # VoxelPyramid: every ReLU output that only the project's own nodes read — the inner and outer outputs of the blocks, the branch
    # sums, the inner steps of the exchange paths and final transitions, bn1s1 — is stored as bf16 rows (include/csn_hip.h section
    # 28) instead of fp32 rows that the next convolution and its weight gradient round to bf16 anyway: the map's write and its
    # three reads (the gather, the weight gradient's gather, the ReLU mask of the backward) halve, and autograd keeps 2 bytes an
    # element alive instead of 4.  z, the statistics, every gradient map, the stem's input and the three kinds of map torch.cat joins
    # (bn0s1, branch 0's last block output, the last step of each final transition) stay fp32.  No product changes; a stored map is
    # rounded once (tests/test_gpu_train_maps16_net.py holds the step bit for bit to the fp32-map graph with every stored map rounded
    # once).  Ignored — the same calls, the same bits — everywhere else: math mode "fp16" (its backward runs in bf16: an fp16 map
    # would be rounded a second time by the weight gradient), fp32 and bf16x3, rows_single_product off, fused=False, a GroupedPyramid
    # (and with it grouped_passes), eval mode (of the backbone or of any submodule: a frozen block or BatchNorm), and the
    # Res16UNets.  Off: opt-in (bytes and timing: DESIGN.md "16-bit training maps", scripts/bench_hrnet_train_maps16.py)
    train_maps16: bool = False

    def flow_for(self, mode: int, d_head: int) -> int:
        return self.score_flow.get((mode, d_head), self.score_flow.get(mode, KEEP_SCORES))

    def takes_fold(self) -> bool:
        """folded_projections, unless an enclosing override block names a switch of the unfolded step alone"""
        return self.folded_projections and not (self.named & UNFOLDED_ONLY)


UNFOLDED_ONLY = frozenset({"dv_from_scores", "grouped_dkv", "qkv_one_pass"})


def cross_takes_score_free(score_bytes: int, budget: int, available: bool) -> bool:
    """The automatic rule of ``cross_score_free=None``: score-free when the flow has kernels for the call's mode and head width
    AND the kept flow's score-sized tensors (``score_bytes`` = 3 * b * H * lq4 * Tp * 4: the scores, the backward's working copy
    and dscores) exceed ``budget``.  Deliberately conservative: it counts the score tensors alone."""
    return bool(available) and score_bytes > budget


_current = Tuning()


def current() -> Tuning:
    return _current


@contextlib.contextmanager
def override(**changes):
    """``with tuning.override(grouped_dq=False): ...`` — the switches inside the block, the previous ones after it.
    NOT thread-safe: the object is process-wide and swapped without a lock.  A step is safe against it all the same — every
    forward snapshots the switches into its autograd context and its backward reads only that snapshot."""
    global _current
    names = {f.name for f in fields(Tuning)} - {"named"}
    unknown = set(changes) - names
    if unknown:
        raise TypeError(f"unknown tuning switch(es): {sorted(unknown)}")
    saved = _current
    _current = replace(saved, **changes, named=saved.named | frozenset(changes))
    try:
        yield _current
    finally:
        _current = saved
