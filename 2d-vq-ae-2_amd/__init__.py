"""vqae_amd -- MI355X-native (gfx950) VQ-AE inference hot path, a drop-in for the conv-encoder ->
vector-quantise -> conv-decoder forward pass of sara-nl/2D-VQ-AE-2.

The directory is named `2d-vq-ae-2_amd` (not an importable identifier); import it as `vqae_amd`
through the loader module of the same name at the repository root.

Layout: csrc/ (HIP kernels + C ABI, built into libvqae_hip.so), _lib.py / ops.py (ctypes binding),
native.py (whole-model handle), layers/ + model.py (mirrors of the reference's module API),
extract_embeddings.py (whole-slide driver), metrics.py (reconstruction metrics) + validate.py (dataset
validation driver), reconstruct.py (stored code grids -> uint8 slide pixels), ingest.py (uint8 slide arrays -> code and
label grids, no DataLoader), classifier.py (the downstream slide
classifier on stored code grids: heatmaps and scores), classifier_train.py + optim.py (its training: the fused backward, the
LAMB / SAM mirrors and the device-resident optimiser step; FusedAdam / FusedAdamW / FusedLamb: the fused multi-tensor step for
any parameter list), train.py + layers/fixup_train.py (training through the Fixup mirrors: fused HIP forward / backward of
every non-conv op of a block around torch's conv2d; block_forward, forward_train, step), train_mbconv.py +
layers/mbconv_train.py (the same for the MBConv mirrors: fused batch-statistic BatchNorm, depthwise conv and SE product),
code_stats.py (exact code / label histograms of stored code grids and
the loss weights read off them), dist.py (one-process-per-GPU sharding over RCCL).
"""
from . import (_lib, classifier, classifier_train, code_stats, ingest, ops, optim, reconstruct, spec, train,  # noqa: F401
               train_mbconv)
from .classifier import CNNClassifier, classify_hdf5, classify_slide  # noqa: F401
from .classifier_train import (ce_loss_and_grads, collate_random_crop, embeddings_split, loss_and_grads,  # noqa: F401
                               smooth_targets, train_hdf5)
from .code_stats import (class_weights, code_histogram, histogram_hdf5, label_histogram_hdf5, perplexity,  # noqa: F401
                         pos_weight_hdf5)
from .ingest import encode_arrays_hdf5, encode_region, encode_slide  # noqa: F401
from .native import NativeVQAE  # noqa: F401
from .optim import SAM, ClassifierTrainer, FusedAdam, FusedAdamW, FusedLamb, Lamb  # noqa: F401
from .reconstruct import reconstruct_hdf5, reconstruct_overview, reconstruct_region, reconstruct_slide  # noqa: F401
from .spec import SPECS, VQAESpec  # noqa: F401
from .train import block_forward, forward_train, step  # noqa: F401
