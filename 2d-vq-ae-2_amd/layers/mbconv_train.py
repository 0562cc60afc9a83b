"""The trainable form of the MBConv mirror: same constructor, same parameters, buffers and state dict, but in train mode, or with
an input that requires grad, `forward` builds a graph (vqae_amd.train_mbconv.block_forward: fused HIP forward / backward for the
BatchNorms, the depthwise conv and the SE product, torch's conv2d for the dense convs), with batch-statistic BatchNorm and the
running-statistics update in train mode.  Select through Hydra in the reference's stock Encoder / Decoder with
    _target_: vqae_amd.layers.mbconv_train.MBConv
In `.eval()` with nothing that requires grad it is the inference mirror of conv_block.py, which is unchanged.
"""
import torch

from .. import train_mbconv
from .conv_block import MBConv as _InferenceBlock


class MBConv(_InferenceBlock):
    def forward_nhwc(self, x):
        if self.training or (torch.is_grad_enabled() and x.requires_grad):
            return train_mbconv.block_forward_nhwc(self, x)
        return super().forward_nhwc(x)

    def forward(self, inp: torch.Tensor):
        if self.training or (torch.is_grad_enabled() and inp.requires_grad):
            return train_mbconv.block_forward(self, inp)
        return super().forward(inp)
