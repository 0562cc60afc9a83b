"""The trainable form of the PreActFixupResBlock mirror: same constructor, same parameters and state dict, but `forward`
builds a graph (vqae_amd.train.block_forward: fused HIP forward / backward for everything that is not a convolution,
torch's conv2d for the convolutions).  Select through Hydra in the reference's stock Encoder / Decoder with
    _target_: vqae_amd.layers.fixup_train.PreActFixupResBlock
The inference mirror of conv_block.py is unchanged and still runs under no_grad.
"""
import torch

from .. import train
from .conv_block import PreActFixupResBlock as _InferenceBlock


class PreActFixupResBlock(_InferenceBlock):
    def forward(self, inp: torch.Tensor):
        return train.block_forward(self, inp)
