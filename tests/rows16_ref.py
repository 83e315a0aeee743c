"""Reference side of the single-product row products (math modes "bf16" / "fp16" with ``csn_set_thread_rows16(1)``; include/csn_hip.h
sections 13, 14, 15a): the kernels round every matrix operand once to 16 bits (nearest even) and multiply exactly (the product of
two bf16 or two fp16 values is exact in fp32), so their yardstick is the float64 reference of tests/sparse_conv_ref.py /
tests/rows_fc_ref.py fed operands rounded on the CPU.

  ``round16``   a tensor's values rounded to fp32 and then to bf16 / fp16 by torch's CPU casts (nearest even), returned as float32 —
                the maps the kernels read are fp32, so that is the rounding they see
  ``conv``      an autograd convolution for ``hrnet_ref.backbone(conv_fn=...)``: the forward is the float64 product of rounded x and
                w, the backward the float64 products of bf16-rounded dy with bf16-rounded w and x (an fp16 forward runs its backward
                in bf16)
tests/test_cpu_rows16.py pins both."""
import torch

from tests import sparse_conv_ref as R

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MODES = {"bf16": 2, "fp16": 3}                # CSN_MATH_BF16 / CSN_MATH_FP16
FP16_MIN_NORMAL = 2.0 ** -14


def round16(t, kind):
    return t.detach().to(torch.float32).to(DTYPES[kind]).to(torch.float32)


def no_subnormals(t):
    """``t`` with every entry below 2^-14 in magnitude set to zero: nothing an fp16 kernel reads is subnormal, before or after
    rounding (a magnitude >= 2^-14 rounds to a normal fp16 value)."""
    return torch.where(t.abs() < FP16_MIN_NORMAL, torch.zeros_like(t), t)


class _Conv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, g, kind):
        ctx.g = g
        ctx.save_for_backward(x, w)
        return R.fwd(g, round16(x, kind), round16(w, kind))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        b = R.bwd(ctx.g, round16(dy, "bf16"), round16(x, "bf16"), round16(w, "bf16"))
        return b["dx"], b["dw"], None, None


def conv(kind):
    """``conv_fn(geometry, x, w)`` of ``hrnet_ref.backbone`` in the arithmetic of math mode ``kind``."""
    return lambda g, x, w: _Conv16.apply(x, w, g, kind)
