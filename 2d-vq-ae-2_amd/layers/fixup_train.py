"""The trainable form of the PreActFixupResBlock mirror: same constructor, same parameters and state dict, but `forward`
builds a graph (vqae_amd.train.block_forward: fused HIP forward / backward for everything that is not a convolution,
torch's conv2d for the convolutions).  Select through Hydra in the reference's stock Encoder / Decoder with
    _target_: vqae_amd.layers.fixup_train.PreActFixupResBlock
The keyword `conv1x1` ("torch", the default, or "hip") is train.block_forward's: "hip" runs the 1x1, stride-1 convs and the op
in front of each as one fused HIP node (csrc/conv_train.hip).  The independent keyword `conv_down` ("torch" | "hip") does the
same for the two 2x2, stride-2 convs of a 'down' block, the independent keyword `conv3x3` ("torch" | "hip") for the circular
3x3 conv of a 'same' or 'out' block (csrc/conv_train.hip), the independent keyword `conv3x3z` ("torch" | "hip") for the
zero-padded 3x3 skip_conv of an 'out' block (csrc/conv_train_thin.hip).  The independent keyword `conv_up` ("torch" | "hip")
selects the order of an 'up' block: "hip" runs conv2 and the skip_conv at low resolution and the bicubic x2 inside the two
fused ops behind them (csrc/up_train.hip).
The inference mirror of conv_block.py is unchanged and still runs under no_grad.
"""
import torch

from .. import train
from .conv_block import PreActFixupResBlock as _InferenceBlock


class PreActFixupResBlock(_InferenceBlock):
    def __init__(self, *args, conv1x1: str = "torch", conv_down: str = "torch", conv3x3: str = "torch",
                 conv3x3z: str = "torch", conv_up: str = "torch", **kwargs):
        super().__init__(*args, **kwargs)
        train.conv_routes(conv1x1=conv1x1, conv_down=conv_down, conv3x3=conv3x3, conv3x3z=conv3x3z, conv_up=conv_up)
        self.conv1x1, self.conv_down, self.conv3x3, self.conv3x3z = conv1x1, conv_down, conv3x3, conv3x3z
        self.conv_up = conv_up

    def forward(self, inp: torch.Tensor):
        return train.block_forward(self, inp, conv1x1=self.conv1x1, conv_down=self.conv_down, conv3x3=self.conv3x3,
                                   conv3x3z=self.conv3x3z, conv_up=self.conv_up)
